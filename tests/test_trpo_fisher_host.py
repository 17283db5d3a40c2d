"""The float64 NumPy statement of TRPO's actor mathematics (tests/trpo_fisher_ref.py) against torch float64
autograd on a float64 copy of `models.Actor`: the loss, its gradient, the KL — and the claim the HIP path rests
on, that with the behaviour policy the network's own output the Hessian the reference takes by double
backward (optimizers.py:36-48 over the `_kl` of updaters.py) IS the Gauss-Newton product J^T M J v.  No kernel
is involved; runs on the CPU."""
import numpy as np
import pytest
import torch

import trpo_fisher_ref as ref
from tonic_amd.environments import Box
from tonic_amd.torch import models
from tonic_amd.torch.updaters import TrustRegionPolicyGradient

TORSOS = {'default': ((64, 64), 'tanh'), 'relu32': ((32,), 'relu'), 'tanh3': ((64, 64, 64), 'tanh'),
          'relu4': ((48, 32, 24, 16), 'relu')}
ACTIVATIONS = {'tanh': torch.nn.Tanh, 'relu': torch.nn.ReLU}
RTOL = 1e-10


def make_actor(O, A, sizes, activation, seed, log_scale=None, saturate=0.0):
    """A float64 `models.Actor` with random parameters (`saturate` > 0: a head bias that drives mu to +-1) and
    its flat parameter vector in parameters() order."""
    torch.manual_seed(seed)
    actor = models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, ACTIVATIONS[activation]),
                         head=models.DetachedScaleGaussianPolicyHead())
    actor.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    actor.double()
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(torch.as_tensor(rng.standard_normal(tuple(p.shape)) * 0.1))
        if log_scale is not None:
            actor.head.log_scale.copy_(torch.as_tensor(np.asarray(log_scale, np.float64)).reshape(1, A))
        if saturate:
            actor.head.loc_layer[0].bias.copy_(
                torch.as_tensor(saturate * np.where(np.arange(A) % 2 == 0, 1.0, -1.0)))
    variables = models.network_variables(actor)
    theta = np.concatenate([p.detach().numpy().reshape(-1) for p in variables])
    return actor, variables, theta


def flat(tensors):
    return torch.cat([t.reshape(-1) for t in tensors]).detach().numpy()


def hessian_vector(updater, variables, observations, locs, scales, v):
    """optimizers.py:36-48 on the updater's own `_kl`."""
    first = torch.cat([t.reshape(-1) for t in torch.autograd.grad(
        updater._kl(observations, locs, scales), variables, create_graph=True)])
    return flat(torch.autograd.grad((first * torch.as_tensor(v)).sum(), variables, allow_unused=True))


def assert_close(got, want, what):
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= RTOL * scale + 1e-300, (what, np.abs(got - want).max(), scale)


CASES = [(name, 6, None, 0.0) for name in TORSOS] + [
    ('default', 1, None, 0.0), ('default', 32, None, 0.0),
    # log_scale inside the clamp, pushed below scale_min and above scale_max (softplus(s) + 1e-8 vs [1e-4, 1])
    ('default', 6, [-1.0, -12.0, 0.2, 2.0, -0.3, 0.54], 0.0),
    ('relu32', 3, [-20.0, 5.0, -2.0], 0.0),
    ('default', 6, None, 25.0), ('relu4', 4, None, 25.0)]       # mu saturated at +-1


@pytest.mark.parametrize('torso,A,log_scale,saturate', CASES)
def test_reference_matches_float64_autograd(torso, A, log_scale, saturate):
    sizes, activation = TORSOS[torso]
    O, n = 17, 96
    actor, variables, theta = make_actor(O, A, sizes, activation, 7 + A, log_scale, saturate)
    rng = np.random.RandomState(A)
    x = rng.standard_normal((n, O)) * 1.5
    observations = torch.as_tensor(x)
    updater = TrustRegionPolicyGradient(entropy_coeff=0.01)
    updater.model = type('Model', (), {'actor': actor})()
    with torch.no_grad():
        behaviour = actor(observations)
        locs, scales = behaviour.loc.clone(), behaviour.stddev.clone()
        actions = locs + scales * torch.as_tensor(rng.standard_normal((n, A)))
        old = behaviour.log_prob(actions).sum(-1) + torch.as_tensor(rng.standard_normal(n) * 0.3)
    adv = torch.as_tensor(rng.standard_normal(n))
    args = (O, A, sizes, activation)

    hs, mu, sigma, dsigma = ref.forward(theta, x, *args)
    assert_close(mu, locs.numpy(), 'mu')
    assert_close(sigma, scales.numpy()[0], 'sigma')
    if saturate:
        assert np.abs(mu).min() > 1 - 1e-12                      # (really saturated)

    loss = updater._loss(observations, actions, old, adv)
    want = flat(torch.autograd.grad(loss, variables)) * n
    assert_close(ref.loss_sum(theta, x, actions.numpy(), adv.numpy(), old.numpy(), 0.01, *args),
                 float(loss.detach()) * n, 'loss')
    assert_close(ref.loss_grad_sums(theta, x, actions.numpy(), adv.numpy(), old.numpy(), 0.01, *args), want,
                 'loss gradient')

    # KL at displaced parameters against the behaviour policy
    moved = theta * (1 + 1e-2 * rng.standard_normal(theta.size))
    with torch.no_grad():
        offset = 0
        for p in variables:
            saved = p.clone()
            p.copy_(torch.as_tensor(moved[offset:offset + p.numel()]).reshape(p.shape))
            offset += p.numel()
            p.saved = saved
        kl = float(updater._kl(observations, locs, scales)) * n * A
        for p in variables:
            p.copy_(p.saved)
    assert_close(ref.kl_sum(moved, x, mu, sigma, *args), kl, 'kl')
    assert ref.kl_sum(theta, x, mu, sigma, *args) == 0.0

    slots, P = ref.layout(*args[:3])
    ls = dict((name, at) for name, _, at in slots)['log_scale']
    vectors = {'random': rng.standard_normal(P)}
    vectors['log_scale only'] = np.zeros(P)
    vectors['log_scale only'][ls:ls + A] = rng.standard_normal(A)
    vectors['first layer only'] = np.zeros(P)
    vectors['first layer only'][:sizes[0] * (O + 1)] = rng.standard_normal(sizes[0] * (O + 1))
    for name, v in vectors.items():
        want = hessian_vector(updater, variables, observations, locs, scales, v) * n * A
        got = ref.fisher_vector_sums(theta, x, v, *args)
        assert_close(got, want, 'F v, ' + name)
        # outside the clamp the scale does not move: that row of F is exactly zero
        outside = dsigma == 0.0
        assert np.all(got[ls:ls + A][outside] == 0.0) and np.all(want[ls:ls + A][outside] == 0.0)
    if log_scale is not None:
        assert (dsigma == 0.0).sum() >= 2 and (dsigma != 0.0).any()
