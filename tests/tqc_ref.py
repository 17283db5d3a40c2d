"""TQC (Kuznetsov et al. 2020, truncated quantile critics) restated in float64 torch, with `torch.sort` and autograd:
what tests/test_gpu_tqc.py holds the HIP entries to.

Per batch row: M quantiles per critic, two critics, d = top_quantiles_to_drop_per_net, K = 2 (M - d).
  Z = sort(pool of the two TARGET critics' M values), y_j = r + disc (Z_j - alpha logp'), j < K
  tau_i = (2 i + 1) / (2 M), u_ij = y_j - theta_zi, rho_ij = |tau_i - 1{u_ij < 0}| huber_1(u_ij)
  loss_m = sum_z (1 / (M K)) sum_i sum_j rho_ij        (the twin convention, loss_1 + loss_2)
"""
import torch


def truncated_targets(target_1, target_2, rewards, discounts, logp, alpha, drop):
    """y [B, K] and, for the tests' own assertions, `source` [B, 2 M]: the critic (0 / 1) each sorted value came
    from."""
    M = target_1.shape[1]
    K = 2 * (M - drop)
    pooled, order = torch.sort(torch.cat([target_1, target_2], dim=1), dim=1)
    y = rewards[:, None] + discounts[:, None] * (pooled[:, :K] - alpha * logp[:, None])
    return y, (order >= M).long()


def errors(theta, y):
    """u [B, M, K] = y_j - theta_i."""
    return y[:, None, :] - theta[:, :, None]


def quantile_huber_rows(theta, y):
    """(1 / (M K)) sum_i sum_j rho_ij per row: theta [B, M] against the kept targets y [B, K]."""
    M = theta.shape[1]
    tau = (2 * torch.arange(M, dtype=theta.dtype) + 1) / (2 * M)
    u = errors(theta, y)
    a = u.abs()
    huber = torch.where(a <= 1, 0.5 * u * u, a - 0.5)
    weight = (tau[None, :, None] - (u < 0).to(theta.dtype)).abs()
    return (weight * huber).mean(dim=(1, 2))


def critic_rows(target_1, target_2, theta_1, theta_2, rewards, discounts, logp, alpha, drop):
    """loss_m [B] = loss_1 + loss_2 of the two online critics against the one truncated target set."""
    y, _ = truncated_targets(target_1, target_2, rewards, discounts, logp, alpha, drop)
    y = y.detach()
    return quantile_huber_rows(theta_1, y) + quantile_huber_rows(theta_2, y)


def critic_rows_with_gradients(target_1, target_2, theta_1, theta_2, rewards, discounts, logp, alpha, drop):
    """(loss_m [B], d loss_m / d theta_1 [B, M], d loss_m / d theta_2 [B, M], q1 [B], q2 [B]) by autograd; all inputs
    float64."""
    theta_1 = theta_1.detach().clone().requires_grad_()
    theta_2 = theta_2.detach().clone().requires_grad_()
    rows = critic_rows(target_1, target_2, theta_1, theta_2, rewards, discounts, logp, alpha, drop)
    rows.sum().backward()                     # (the rows are independent: the sum's gradient is each row's own)
    return rows.detach(), theta_1.grad, theta_2.grad, theta_1.detach().mean(dim=1), theta_2.detach().mean(dim=1)


def actor_rows(theta_1, theta_2, logp, alpha):
    """alpha logp - Q, Q the mean of the two online critics' 2 M quantiles."""
    return alpha * logp - 0.5 * (theta_1.mean(dim=1) + theta_2.mean(dim=1))
