"""Float64 restatement of MaximumAPosterioriPolicyOptimization.__call__ (updaters/actors.py:318-464) for either KL
constraint, shared by tests/test_mpo_surface_host.py (which holds it to the unmodified reference updater) and
tests/test_gpu_mpo_surface.py (whose yardstick it is).  Modelled on `_mpo_reference` of
tests/test_gpu_offpolicy_grads.py, which states the per-dimension constraint only and stays as it is."""
import numpy as np
import torch

FLOAT_EPSILON = 1e-8                # updaters/actors.py:6


def mpo_reference(ref, actor, target_actor, frozen, obs, eps, duals, floor, u, S, penalization, per_dim):
    """ref: the networks' float64 forward passes (`Ref` of test_gpu_offpolicy_grads); actor / target_actor / frozen:
    float64 leaves; obs [B, O], eps [S * B, A] float64; duals [2 K + 2] = {log_temperature, log_alpha_mean[K],
    log_alpha_std[K], log_penalty_temperature} with K = A (per_dim) or 1 (the KLs of the Independent normals,
    actors.py:422-426); floor: min_log_dual as the float32 the reference holds it in (actors.py:285); u: epsilon,
    epsilon_penalty, epsilon_mean, epsilon_std.  loss.backward() has run on return.
    Returns (dual leaves, stats [9 + 2 K], actor loss, floored duals, actions, the temperature losses' term size,
    max |Q| / T) — the tuple of `_mpo_reference`."""
    B, A = obs.shape[0], eps.shape[-1]
    K = A if per_dim else 1
    assert len(duals) == 2 * K + 2
    with torch.no_grad():
        loc_t, scale_t = ref.policy(target_actor, obs)
        actions = loc_t[None] + scale_t[None] * eps.view(S, B, A)
        values = ref.critic(frozen, obs.repeat(S, 1), actions.reshape(S * B, A)).view(S, B)
    floored = torch.maximum(torch.as_tensor(np.asarray(duals), dtype=torch.float64),
                            torch.tensor(float(np.float32(floor)), dtype=torch.float64))
    log_t = floored[:1].clone().requires_grad_()
    log_am = floored[1:1 + K].clone().requires_grad_()
    log_as = floored[1 + K:1 + 2 * K].clone().requires_grad_()
    log_p = floored[1 + 2 * K:].clone().requires_grad_()
    softplus = torch.nn.functional.softplus

    scales = []          # the size of the temperature losses' terms: T (|epsilon| + mean |LSE| + log S)

    def weights_and_loss(q, epsilon, temperature):
        tempered = q.detach() / temperature
        weights = torch.softmax(tempered, 0).detach()
        lse = torch.logsumexp(tempered, 0)
        scales.append(float(temperature.detach()) * (abs(epsilon) + float(lse.detach().abs().mean()) + np.log(q.shape[0])))
        return weights, temperature * (epsilon + lse.mean() - np.log(q.shape[0]))

    loc, scale = ref.policy(actor, obs)
    temperature = softplus(log_t) + FLOAT_EPSILON
    alpha_mean, alpha_std = softplus(log_am) + FLOAT_EPSILON, softplus(log_as) + FLOAT_EPSILON
    weights, temperature_loss = weights_and_loss(values, u.epsilon, temperature)
    penalty_temperature = softplus(log_p) + FLOAT_EPSILON
    if penalization:
        costs = -torch.norm(actions - torch.clamp(actions, -1, 1), dim=-1)
        pw, pl = weights_and_loss(costs, u.epsilon_penalty, penalty_temperature)
        weights = weights + pw
        temperature_loss = temperature_loss + pl
    normal = torch.distributions.Normal
    fixed_std, fixed_mean = normal(loc, scale_t), normal(loc_t, scale)
    policy_mean_loss = -((fixed_std.log_prob(actions).sum(-1) * weights).sum(0)).mean()
    policy_std_loss = -((fixed_mean.log_prob(actions).sum(-1) * weights).sum(0)).mean()
    target = normal(loc_t, scale_t)
    kl_mean = torch.distributions.kl.kl_divergence(target, fixed_std)            # [B, A]
    kl_std = torch.distributions.kl.kl_divergence(target, fixed_mean)
    if not per_dim:          # kl_divergence of Independent(., 1): the sum over the event dimension -> [B]
        kl_mean, kl_std = kl_mean.sum(-1, keepdim=True), kl_std.sum(-1, keepdim=True)
    kl_mean, kl_std = kl_mean.mean(0), kl_std.mean(0)                            # [K]
    kl_mean_loss, alpha_mean_loss = (alpha_mean.detach() * kl_mean).sum(), \
        (alpha_mean * (u.epsilon_mean - kl_mean.detach())).sum()
    kl_std_loss, alpha_std_loss = (alpha_std.detach() * kl_std).sum(), \
        (alpha_std * (u.epsilon_std - kl_std.detach())).sum()
    loss = policy_mean_loss + policy_std_loss + kl_mean_loss + kl_std_loss + alpha_mean_loss + alpha_std_loss + \
        temperature_loss
    loss.backward()
    stats = [policy_mean_loss, policy_std_loss, kl_mean_loss, kl_std_loss, alpha_mean_loss, alpha_std_loss,
             temperature_loss, temperature[0]]
    stats = np.concatenate([np.array([float(s.detach()) for s in stats]), alpha_mean.detach().numpy(),
                            alpha_std.detach().numpy(), penalty_temperature.detach().numpy()])
    actor_loss = float((policy_mean_loss + policy_std_loss + kl_mean_loss + kl_std_loss).detach())
    tempering = float(values.abs().max() / temperature.detach())         # max |Q| / T
    return (log_t, log_am, log_as, log_p), stats, actor_loss, floored.numpy(), actions, sum(scales), tempering
