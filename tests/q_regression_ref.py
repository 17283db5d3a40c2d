"""The float64 restatement of one QRegression step (tonic/torch/updaters/critics.py:31-53) from a critic's
state_dict: values = critic(observations, actions) with the ObservationActionEncoder's MeanStd (and its clip), the
torso, the value head — squashed as low + sigmoid(z) (high - low) under a Return normaliser — the loss through
torch.nn.functional with reduction 'mean', and the per-tensor gradients of that mean loss.

tests/test_q_regression_host.py holds it to the unmodified reference's own QRegression on the CPU;
tests/test_gpu_q_regression.py holds tonic_q_regression_grad and the updater to it."""
import re

import torch

F = torch.nn.functional
ACTIVATIONS = {'ReLU': torch.relu, 'Tanh': torch.tanh, 'ELU': F.elu}
LOSSES = ('mse', 'l1', 'smooth_l1', 'huber')


def loss_terms(values, returns, kind='mse', param=None):
    """The loss of every row (reduction 'none'); their mean is the reference's loss."""
    if kind == 'mse':
        return F.mse_loss(values, returns, reduction='none')
    if kind == 'l1':
        return F.l1_loss(values, returns, reduction='none')
    if kind == 'smooth_l1':
        return F.smooth_l1_loss(values, returns, reduction='none', beta=param)
    assert kind == 'huber'
    return F.huber_loss(values, returns, reduction='none', delta=param)


def kink(kind, param=None):
    """|q - y| at which the rule's gradient changes form: None for MSE, 0 for L1 (and smooth-L1 with beta = 0)."""
    if kind == 'mse':
        return None
    return 0.0 if kind == 'l1' else float(param)


def torch_loss(kind, param=None):
    """The torch.nn loss object of a rule (what the updater's `loss=` takes); None for MSE, the default."""
    return {'mse': lambda: None, 'l1': torch.nn.L1Loss, 'smooth_l1': lambda: torch.nn.SmoothL1Loss(beta=param),
            'huber': lambda: torch.nn.HuberLoss(delta=param)}[kind]()


def leaves(state, dtype=torch.float64):
    """A critic's weights and biases out of its state_dict (`torso.model.<2 l>.{weight,bias}`, then
    `head.v_layer.{weight,bias}`: parameters() order) as leaves that require gradients."""
    layers = sorted({int(m.group(1)) for m in (re.match(r'torso\.model\.(\d+)\.weight$', k) for k in state) if m})
    keys = [f'torso.model.{i}.{name}' for i in layers for name in ('weight', 'bias')]
    keys += ['head.v_layer.weight', 'head.v_layer.bias']
    return [state[k].detach().cpu().to(dtype).clone().requires_grad_() for k in keys]


def values_of(params, observations, actions, activation, mean=None, std=None, clip=None, low=None, high=None):
    """critic(observations, actions) (encoders.py:28-31, mean_stds.py:34-39, utils.py:4-23, critics.py:15-20)."""
    x = observations
    if mean is not None:
        x = (x - mean) / std
        if clip is not None:
            x = torch.clamp(x, -clip, clip)
    x = torch.cat([x, actions], dim=-1)
    act = ACTIVATIONS[activation]
    for layer in range(len(params) // 2 - 1):
        x = act(F.linear(x, params[2 * layer], params[2 * layer + 1]))
    z = F.linear(x, params[-2], params[-1]).squeeze(-1)
    if low is None:
        return z
    return low + torch.sigmoid(z) * (high - low)


def step(state, observations, actions, returns, activation, loss=('mse', None), mean=None, std=None, clip=None,
         low=None, high=None, dtype=torch.float64):
    """One step's values, loss terms, mean loss and the gradients of the mean loss per tensor (parameters() order)."""
    to = lambda v: None if v is None else torch.as_tensor(v).detach().cpu().to(dtype)     # noqa: E731
    params = leaves(state, dtype)
    values = values_of(params, to(observations), to(actions), activation, to(mean), to(std), clip, to(low), to(high))
    terms = loss_terms(values, to(returns), *loss)
    total = terms.mean()
    total.backward()
    return dict(params=params, values=values.detach(), terms=terms.detach(), loss=total.detach(),
                grads=[p.grad for p in params])
