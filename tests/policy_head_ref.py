"""Restatement of the Gaussian policy heads with scale bounds (tonic/torch/models/actors.py:69-98 with
``scale_min`` / ``scale_max``), shared by tests/test_policy_head_host.py (which holds it to the unmodified reference)
and tests/test_gpu_policy_head.py (whose yardstick it is).

- float64, torch (autograd): ``gaussian_head``, ``squashed``, ``Networks`` (the forward passes of a model's float64
  leaves) and the SAC actor objective ``sac_actor_terms``;
- float32, NumPy: ``head32`` / ``act32``, what the acting kernels compute after the heads' linear layers.

softplus is torch's (threshold 20); clamp passes the gradient where the value lies within [scale_min, scale_max],
bounds included, and nowhere else (torch.clamp's backward)."""
import numpy as np
import torch

SAC_LOG_EPSILON = 1e-6              # models/actors.py:15


def gaussian_head(loc_pre, scale_pre, scale_min, scale_max, tanh_loc):
    """GaussianPolicyHead.forward on the outputs of its two linear layers: (loc, scale).  tanh_loc: loc_activation
    = Tanh (MPO); False: Identity (SAC).  scale_activation = Softplus."""
    scale = torch.clamp(torch.nn.functional.softplus(scale_pre), scale_min, scale_max)
    return (torch.tanh(loc_pre) if tanh_loc else loc_pre), scale


def squashed(loc, scale, noise):
    """SquashedMultivariateNormalDiag.rsample_with_log_prob with the draws given (models/actors.py:11-16)."""
    raw = loc + scale * noise
    action = torch.tanh(raw)
    log_prob = torch.distributions.Normal(loc, scale).log_prob(raw) - torch.log(1 - action ** 2 + SAC_LOG_EPSILON)
    return action, log_prob.sum(-1)


def regimes(scale_pre, scale_min, scale_max):
    """Shares of the elements whose softplus lies below, inside and above the bounds, and the smallest distance of a
    softplus to a bound (float64)."""
    raw = torch.nn.functional.softplus(scale_pre.detach().double())
    below, above = float((raw < scale_min).double().mean()), float((raw > scale_max).double().mean())
    distance = float(torch.minimum((raw - scale_min).abs(), (raw - scale_max).abs()).min())
    return below, 1.0 - below - above, above, distance


class Networks:
    """The float64 forward passes of an actor (torso + loc and scale heads) and a critic on lists of leaves in
    parameters() order, the observation normaliser on the critic's input only (the reference's Actor hands its
    normaliser to the encoder's `action_space` slot, actors.py:128-129 vs encoders.py:5-8)."""

    def __init__(self, layers, mean, std, scale_min, scale_max, tanh_loc, activation=torch.relu):
        self.L, self.mean, self.std = layers, mean, std
        self.scale_min, self.scale_max, self.tanh_loc, self.act = scale_min, scale_max, tanh_loc, activation

    def _torso(self, params, x):
        for layer in range(self.L):
            x = self.act(torch.nn.functional.linear(x, params[2 * layer], params[2 * layer + 1]))
        return x

    def heads(self, params, obs):
        h, L = self._torso(params, obs), self.L
        return (torch.nn.functional.linear(h, params[2 * L], params[2 * L + 1]),
                torch.nn.functional.linear(h, params[2 * L + 2], params[2 * L + 3]))

    def policy(self, params, obs):
        return gaussian_head(*self.heads(params, obs), self.scale_min, self.scale_max, self.tanh_loc)

    def critic(self, params, obs, act):
        h = self._torso(params, torch.cat([(obs - self.mean) / self.std, act], -1))
        return torch.nn.functional.linear(h, params[2 * self.L], params[2 * self.L + 1]).squeeze(-1)


def sac_actor_terms(networks, actor, critics, obs, noise, entropy_coeff):
    """TwinCriticSoftDeterministicPolicyGradient (updaters/actors.py:238-267), per sample: its loss is the mean."""
    action, log_prob = squashed(*networks.policy(actor, obs), noise)
    values = torch.min(*[networks.critic(c, obs, action) for c in critics])
    return entropy_coeff * log_prob - values


# ---------------------------------------------------------------- float32, NumPy: acting

def softplus32(x):
    """torch.nn.functional.softplus in float32: log1p(exp(x)), x itself above the threshold 20."""
    x = np.asarray(x, np.float32)
    with np.errstate(over='ignore'):
        return np.where(x > np.float32(20), x, np.log1p(np.exp(x, dtype=np.float32), dtype=np.float32))


def head32(scale_pre, scale_min, scale_max):
    """sigma = clamp(softplus(pre), scale_min, scale_max) with the bounds as float32."""
    return np.minimum(np.maximum(softplus32(scale_pre), np.float32(scale_min)), np.float32(scale_max))


def act32(loc_out, scale_pre, eps, scale_min, scale_max, squash):
    """The action of one acting step from the head layers' outputs, float32 operation by operation: squash (SAC)
    tanh(loc + eps * sigma) with loc the linear output, else (MPO) loc + sigma * eps with loc = tanh(linear output)
    given as `loc_out`; eps None: the greedy action."""
    loc_out = np.asarray(loc_out, np.float32)
    if eps is None:
        return np.tanh(loc_out) if squash else loc_out
    sigma = head32(scale_pre, scale_min, scale_max)
    eps = np.asarray(eps, np.float32)
    if squash:
        return np.tanh(loc_out + eps * sigma, dtype=np.float32)
    return loc_out + sigma * eps
