"""The float64 restatement of one SAC iteration with a learned entropy coefficient, on torch CPU: the critic step's
TD target (tonic/torch/updaters/critics.py:202-235) and the actor step's objective (actors.py:238-267) with
alpha = exp(log_alpha) in the place of the reference's fixed 0.2, then the coefficient's own loss

    J(log_alpha) = -mean(log_alpha * (log_probs + target_entropy))

on the log-probabilities of the actor step's sample (SAC's automatic temperature adjustment; the reference has no line
for it) and its step by a torch.optim rule on a float64 leaf.

Networks enter as callables — ``policy(observations) -> (loc, scale)``, ``critic(observations, actions) -> q`` — so the
same statements serve plain float64 modules (tests/test_entropy_coeff_host.py) and the float64 images of a packed
model (tests/test_gpu_entropy_coeff.py)."""
import math

import torch

OPTIMIZERS = {
    'adam': lambda params: torch.optim.Adam(params, lr=3e-4),
    'adam_fast': lambda params: torch.optim.Adam(params, lr=0.05),
    'sgd': lambda params: torch.optim.SGD(params, lr=0.02, momentum=0.9),
    'rmsprop': lambda params: torch.optim.RMSprop(params, lr=0.01),
}


def squashed_sample(loc, scale, eps):
    """SquashedMultivariateNormalDiag.rsample_with_log_prob with the draws given (models/actors.py:11-16)."""
    raw = loc + scale * eps
    actions = torch.tanh(raw)
    log_probs = torch.distributions.Normal(loc, scale).log_prob(raw) - torch.log(1 - actions ** 2 + 1e-6)
    return actions, log_probs.sum(-1)


def td_targets(policy, target_critics, batch, eps, log_alpha):
    """y = r + discount (min q'(s', a') - alpha log pi(a' | s')), a' the online policy's sample on s' (no gradients)."""
    with torch.no_grad():
        actions, log_probs = squashed_sample(*policy(batch['next_observations']), eps)
        values = torch.min(*[critic(batch['next_observations'], actions) for critic in target_critics])
        values = values - math.exp(float(log_alpha)) * log_probs
        return batch['rewards'] + batch['discounts'] * values


def critic_loss(critics, batch, returns):
    """(sum over the critics of mean (q - y)^2, the q of every critic)."""
    values = [critic(batch['observations'], batch['actions']) for critic in critics]
    return sum(((q - returns) ** 2).mean() for q in values), values


def actor_terms(policy, critics, observations, eps, log_alpha):
    """(alpha log pi(a | s) - min q(s, a) per row, log pi(a | s) per row), a the policy's sample on s."""
    actions, log_probs = squashed_sample(*policy(observations), eps)
    values = torch.min(*[critic(observations, actions) for critic in critics])
    return math.exp(float(log_alpha)) * log_probs - values, log_probs


def coeff_loss(log_alpha, log_probs, target_entropy):
    """J: `log_alpha` a float64 leaf, `log_probs` detached."""
    return -(log_alpha * (log_probs.detach() + target_entropy)).mean()


def coeff_sums(log_alpha, log_probs, target_entropy):
    """What the actor entry leaves for the coefficient's step: the gradient SUM dJ / d log_alpha times the row
    count, and the statistics' sums."""
    excess = (log_probs.detach().double() + target_entropy)
    return dict(grad=-excess.sum(), loss=-float(log_alpha) * excess.sum(), log_prob=log_probs.detach().double().sum(),
                rows=float(log_probs.shape[0]), terms=excess)


class Coefficient:
    """log_alpha as a float64 leaf with its torch.optim rule; `step(log_probs)` is the coefficient's update."""

    def __init__(self, log_alpha, target_entropy, optimizer):
        self.log_alpha = torch.tensor(float(log_alpha), dtype=torch.float64, requires_grad=True)
        self.target_entropy = float(target_entropy)
        self.optimizer = optimizer([self.log_alpha])

    @property
    def value(self):
        return float(self.log_alpha.detach())

    def step(self, log_probs):
        self.optimizer.zero_grad()
        loss = coeff_loss(self.log_alpha, log_probs, self.target_entropy)
        loss.backward()
        self.optimizer.step()
        return float(loss.detach())


def iteration(policy, critics, target_critics, batch, eps_critic, eps_actor, coefficient, critic_step=None,
              actor_step=None):
    """One iteration in the agent's order: the critic step with alpha_t, the actor step with alpha_t (through the
    critics the critic step has moved when `critic_step` moves them), the coefficient's step to alpha_{t+1}.
    critic_step(loss) / actor_step(loss): the caller's optimizer steps of the networks (None: the gradients stay on
    the leaves).  Returns the quantities of the iteration."""
    log_alpha = coefficient.value
    returns = td_targets(policy, target_critics, batch, eps_critic, log_alpha)
    c_loss, values = critic_loss(critics, batch, returns)
    if critic_step is not None:
        critic_step(c_loss)
    terms, log_probs = actor_terms(policy, critics, batch['observations'], eps_actor, log_alpha)
    a_loss = terms.mean()
    if actor_step is not None:
        actor_step(a_loss)
    sums = coeff_sums(log_alpha, log_probs, coefficient.target_entropy)
    j = coefficient.step(log_probs)
    return dict(log_alpha=log_alpha, returns=returns, critic_loss=c_loss, values=values, actor_terms=terms,
                actor_loss=a_loss, log_probs=log_probs.detach(), coeff_loss=j, coeff_sums=sums,
                next_log_alpha=coefficient.value)
