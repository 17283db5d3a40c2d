"""DMPO restated in stock torch on the CPU, for the tests: MPO's Gaussian actor and dual step on a categorical critic
over one support, the critic trained by a distributional Expected-SARSA step.

Written from the semantics in include/tonic_hip.h (tonic_distributional_expected_sarsa_grad,
tonic_distributional_mpo_actor_grad).  The networks are td4_ref.Networks — leaf tensors of ONE dtype, float64 for the
gradient tests, float32 for `Learner` — with the single critic under both of its twin names; the projection is the
package's own models.CategoricalWithSupport through td4_ref.categorical; the actor step is
tests/mpo_surface_reference.py's with `target_critic(...)` replaced by the mean of the critic's distribution.  Reads
nothing outside the repository."""
import types

import numpy as np
import torch

import td4_ref
from mpo_surface_reference import mpo_reference

SINGLE = {'actor': 'actor', 'critic_1': 'critic', 'critic_2': 'critic', 'target_actor': 'target_actor',
          'target_critic_1': 'target_critic', 'target_critic_2': 'target_critic'}


class Networks(td4_ref.Networks):
    """td4_ref.Networks of a single-critic model ('critic_1' / 'target_critic_1' are the critic and its target; the
    second names hold copies nobody reads) with a GaussianPolicyHead on the actors: params['actor'] =
    [torso ..., W_loc, b_loc, W_scale, b_scale], loc = tanh(.), sigma = clamp(softplus(.), scale_min, scale_max)."""

    @classmethod
    def of_model(cls, model, layers, activation='ReLU', dtype=torch.float64):
        nets = cls({name: getattr(model, attribute) for name, attribute in SINGLE.items()},
                   model.observation_normalizer, model.target_critic.head.values, layers, activation, dtype)
        # (the bounds as the float32 the kernels clamp to: updaters.policy_head_rule)
        nets.scale_bounds = (float(np.float32(model.actor.head.scale_min)),
                             float(np.float32(model.actor.head.scale_max)))
        return nets

    def gaussian(self, name, observations):
        params, x = self.params[name], observations
        for layer in range(self.L):
            x = self.act(torch.nn.functional.linear(x, params[2 * layer], params[2 * layer + 1]))
        loc = torch.tanh(torch.nn.functional.linear(x, params[2 * self.L], params[2 * self.L + 1]))
        scale = torch.nn.functional.softplus(torch.nn.functional.linear(x, params[2 * self.L + 2],
                                                                        params[2 * self.L + 3]))
        return loc, torch.clamp(scale, *self.scale_bounds)

    def value(self, name, observations, actions):
        """The mean of the critic's distribution: sum_i softmax(logits)_i z_i."""
        return (torch.softmax(self.logits(name, observations, actions), -1) * self.values).sum(-1)


def sampled_actions(nets, observations, eps, S):
    """a_s = loc_t + sigma_t eps_s of the target actor, [S, B, A] (eps: [S * B, A], row s * B + m)."""
    loc, scale = nets.gaussian('target_actor', observations)
    return loc[None] + scale[None] * eps.to(nets.dtype).view(S, observations.shape[0], -1)


def project(values, probabilities, returns):
    """CategoricalWithSupport.project of the distribution `probabilities` [B, NA] (not of logits)."""
    distribution = td4_ref.categorical(values, torch.zeros_like(probabilities))
    distribution.probabilities = probabilities
    return distribution.project(returns)


def critic_targets(nets, batch, eps, S):
    """dict(targets [B, NA] — the projection of the mixture of the S target distributions —, mixture, samples
    [S, B, NA], returns)."""
    with torch.no_grad():
        B = batch['observations'].shape[0]
        actions = sampled_actions(nets, batch['next_observations'], eps, S)
        logits = nets.logits('target_critic_1', batch['next_observations'].repeat(S, 1), actions.reshape(S * B, -1))
        samples = torch.softmax(logits, -1).view(S, B, -1)
        mixture = samples.mean(0)
        returns = batch['rewards'][:, None] + batch['discounts'][:, None] * nets.values[None]
        targets = project(nets.values, mixture, returns)
    return dict(targets=targets, mixture=mixture, samples=samples, returns=returns)


def critic_step(nets, batch, eps, S):
    """loss = mean_m -sum_i T_i log_softmax(critic(s, a))_i, backward into 'critic_1'; the targets' dict with the
    per-row terms, the loss and q (the online critic's means) added."""
    out = critic_targets(nets, batch, eps, S)
    logits = nets.logits('critic_1', batch['observations'], batch['actions'])
    terms = -(out['targets'] * torch.log_softmax(logits, -1)).sum(-1)
    loss = terms.mean()
    loss.backward()
    out.update(loss=loss.detach(), terms=terms.detach(),
               q=(torch.softmax(logits, -1) * nets.values).sum(-1).detach())
    return out


def actor_step(nets, observations, eps, duals, floor, u, S, penalization, per_dim):
    """mpo_surface_reference.mpo_reference on these networks, the E-step's q the target critic's means; backward
    into 'actor' and the dual leaves.  `u`: anything with epsilon, epsilon_penalty, epsilon_mean, epsilon_std.
    Returns mpo_reference's tuple."""
    ref = types.SimpleNamespace(
        policy=lambda name, obs: nets.gaussian(name, obs),
        critic=lambda name, obs, actions: nets.value(name, obs, actions))
    return mpo_reference(ref, 'actor', 'target_actor', 'target_critic_1', observations, eps.to(nets.dtype), duals,
                         floor, u, S, penalization, per_dim)


DUAL_NAMES = ('log_temperature', 'log_alpha_mean', 'log_alpha_std', 'log_penalty_temperature')


def actor_outputs(nets, observations, eps, duals, u, S, joint):
    """actor_step's results under the names `actor_errors` compares: actor (the leaves' gradients), the dual
    gradients by name, stats, actor_loss — and what the comparison scales by: temperature_scale, tempering,
    sigmoid(log T) of both temperatures."""
    penal = bool(u.action_penalization)
    leaves, stats, actor_loss, floored, actions, temperature_scale, tempering = actor_step(
        nets, observations.to(nets.dtype), eps, duals, u.min_log_dual, u, S, penal, not joint)
    out = dict(actor=[as_numpy(p.grad) for p in nets.params['actor']], stats=np.asarray(stats, np.float64),
               actor_loss=actor_loss, floored=floored, actions=actions, temperature_scale=temperature_scale,
               tempering=tempering)
    for name, leaf in zip(DUAL_NAMES, leaves):
        out[name] = as_numpy(leaf.grad) if leaf.grad is not None else np.zeros(len(leaf))
        out['sigmoid/' + name] = float(torch.sigmoid(leaf.detach()[0]))
    return out


def actor_errors(got, want, u, S, joint):
    """Every output's error in the units tests/test_gpu_mpo_surface.py::_compare holds it in: a tensor's largest
    |got - want| over its largest |want| (actor: the largest over the tensors; the alphas), a temperature's gradient
    over max(|want|, sigmoid(log T) (|epsilon| + log S)), a statistic over |want| — the temperature loss over
    max(|want|, T (|epsilon| + mean |LSE| + log S)) —, keyed actor / <dual name> / actor_loss / stat <i>."""
    def tensor(g, w):
        return float(np.abs(np.asarray(g, np.float64) - w).max() / max(np.abs(w).max(), 1e-30))
    penal, K = bool(u.action_penalization), len(want['log_alpha_mean'])
    errors = dict(actor=max(tensor(g, w) for g, w in zip(got['actor'], want['actor'])))
    for name in DUAL_NAMES:
        if name == 'log_penalty_temperature' and not penal:
            continue
        g, w = np.asarray(got[name], np.float64), want[name]
        if name in ('log_temperature', 'log_penalty_temperature'):
            epsilon = u.epsilon if name == 'log_temperature' else u.epsilon_penalty
            scale = max(abs(float(w[0])), want['sigmoid/' + name] * (abs(epsilon) + np.log(S)))
            errors[name] = abs(float(g[0]) - float(w[0])) / scale
        else:
            errors[name] = tensor(g, w)
    errors['actor_loss'] = abs(got['actor_loss'] - want['actor_loss']) / max(abs(want['actor_loss']), 1e-30)
    for i in range(8 + 2 * K + (1 if penal else 0)):
        scale = max(abs(want['stats'][i]), want['temperature_scale'] if i == 6 else 0.0, 1e-30)
        errors[f'stat {min(i, 8)}'] = max(errors.get(f'stat {min(i, 8)}', 0.0),
                                          abs(float(got['stats'][i]) - want['stats'][i]) / scale)
    return errors


class Learner:
    """Whole iterations in float32: the critic step, the actor and dual step (torch.optim.Adam: critic and actor
    lr 3e-4, duals lr 1e-2, the updaters' defaults) and the polyak update of both targets."""

    def __init__(self, model, layers, activation, updater, critic_samples, target_coeff=0.005):
        self.nets = Networks.of_model(model, layers, activation, torch.float32)
        p = self.nets.params
        self.critic_optimizer = torch.optim.Adam(p['critic_1'], lr=3e-4)
        self.actor_optimizer = torch.optim.Adam(p['actor'], lr=3e-4)
        self.u, self.S_c, self.target_coeff = updater, critic_samples, target_coeff
        self.duals = updater.duals.detach().cpu().clone()
        self.dual_state = torch.optim.Adam([torch.nn.Parameter(self.duals)], lr=1e-2)

    def iteration(self, batch, eps_critic, eps_actor):
        """Returns (the critic step's dict, the actor step's statistics row)."""
        nets, p, u = self.nets, self.nets.params, self.u
        self.critic_optimizer.zero_grad()
        out = critic_step(nets, batch, eps_critic, self.S_c)
        self.critic_optimizer.step()
        self.actor_optimizer.zero_grad()
        # (mpo_reference holds the duals in float64; the networks and what flows into them stay float32)
        duals = self.dual_state.param_groups[0]['params'][0]
        leaves, stats, _, floored, *_ = actor_step(
            nets, batch['observations'], eps_actor, duals.detach().numpy(), u.min_log_dual, u, u.num_samples,
            bool(u.action_penalization), bool(u.per_dim_constraining))
        self.actor_optimizer.step()
        grads = [leaf.grad if leaf.grad is not None else torch.zeros_like(leaf) for leaf in leaves]
        with torch.no_grad():                   # the floored duals are what the step starts from (actors.py:347-356)
            kept = duals[-1].clone()
            duals.copy_(torch.as_tensor(floored, dtype=torch.float32))
            if not u.action_penalization:       # (the penalty temperature is neither floored nor moved)
                duals[-1] = kept
        duals.grad = torch.cat(grads).to(torch.float32)
        self.dual_state.step()
        with torch.no_grad():
            for online, target in (('actor', 'target_actor'), ('critic_1', 'target_critic_1')):
                for o, t in zip(p[online], p[target]):
                    t.mul_(1 - self.target_coeff)
                    t.add_(self.target_coeff * o)
        return out, stats

    def snapshot(self):
        out = {name: [t.detach().numpy().copy() for t in self.nets.params[name]]
               for name in ('actor', 'critic_1', 'target_actor', 'target_critic_1')}
        out['duals'] = [self.dual_state.param_groups[0]['params'][0].detach().numpy().copy()]
        return out


def as_numpy(tensor):
    return np.asarray(tensor.detach().cpu().numpy(), np.float64)
