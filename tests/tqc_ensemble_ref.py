"""TQC on an ensemble of N critics restated in float64 torch: tests/tqc_ref.py over a list of N critics, with
`torch.sort` and autograd — what tests/test_gpu_tqc_ensemble.py holds the HIP entries to.

Per batch row: M quantiles per critic, N critics, d = top_quantiles_to_drop_per_net, K = N (M - d).
  Z = sort(pool of the N TARGET critics' M values), y_j = r + disc (Z_j - alpha logp'), j < K
  tau_i = (2 i + 1) / (2 M), u_ij = y_j - theta_zi, rho_ij = |tau_i - 1{u_ij < 0}| huber_1(u_ij)
  loss_m = sum_z (1 / (M K)) sum_i sum_j rho_ij        (the twin convention, extended over z)

At N = 2 every function returns exactly what tqc_ref's returns (asserted below, on CPU data, when imported).
"""
import torch

import tqc_ref


def truncated_targets(targets, rewards, discounts, logp, alpha, drop):
    """y [B, K] and `source` [B, N M]: the critic (0 .. N - 1) each sorted value came from."""
    N, M = len(targets), targets[0].shape[1]
    K = N * (M - drop)
    pooled, order = torch.sort(torch.cat(list(targets), dim=1), dim=1)
    y = rewards[:, None] + discounts[:, None] * (pooled[:, :K] - alpha * logp[:, None])
    return y, torch.div(order, M, rounding_mode='floor')


def critic_rows(targets, thetas, rewards, discounts, logp, alpha, drop):
    """loss_m [B] = the sum over the N online critics of their loss against the one truncated target set."""
    y, _ = truncated_targets(targets, rewards, discounts, logp, alpha, drop)
    y = y.detach()
    rows = tqc_ref.quantile_huber_rows(thetas[0], y)
    for theta in thetas[1:]:
        rows = rows + tqc_ref.quantile_huber_rows(theta, y)
    return rows


def critic_rows_with_gradients(targets, thetas, rewards, discounts, logp, alpha, drop):
    """(loss_m [B], [d loss_m / d theta_z [B, M]] * N, q [B] = (1 / N) sum_z mean_i theta_zi) by autograd; all inputs
    float64."""
    thetas = [theta.detach().clone().requires_grad_() for theta in thetas]
    rows = critic_rows(targets, thetas, rewards, discounts, logp, alpha, drop)
    rows.sum().backward()                     # (the rows are independent: the sum's gradient is each row's own)
    q = torch.stack([theta.detach().mean(dim=1) for theta in thetas]).mean(dim=0)
    return rows.detach(), [theta.grad for theta in thetas], q


def actor_rows(thetas, logp, alpha):
    """alpha logp - Q, Q the mean of the N online critics' N M quantiles."""
    return alpha * logp - torch.stack([theta.mean(dim=1) for theta in thetas]).mean(dim=0)


def _equals_the_twin_reference_at_two():
    g = torch.Generator().manual_seed(0)
    B, M, drop, alpha = 7, 5, 2, 0.3
    t1, t2, th1, th2 = (torch.randn(B, M, generator=g, dtype=torch.float64) * 3 for _ in range(4))
    r, logp = (torch.randn(B, generator=g, dtype=torch.float64) for _ in range(2))
    disc = torch.where(torch.arange(B) % 3 == 0, 0.0, 0.99).double()
    y, source = truncated_targets([t1, t2], r, disc, logp, alpha, drop)
    twin_y, twin_source = tqc_ref.truncated_targets(t1, t2, r, disc, logp, alpha, drop)
    assert torch.equal(y, twin_y) and torch.equal(source, twin_source)
    rows, grads, q = critic_rows_with_gradients([t1, t2], [th1, th2], r, disc, logp, alpha, drop)
    twin = tqc_ref.critic_rows_with_gradients(t1, t2, th1, th2, r, disc, logp, alpha, drop)
    assert torch.equal(rows, twin[0]) and torch.equal(grads[0], twin[1]) and torch.equal(grads[1], twin[2])
    assert torch.equal(q, torch.stack([twin[3], twin[4]]).mean(dim=0))
    assert torch.equal(actor_rows([th1, th2], logp, alpha), tqc_ref.actor_rows(th1, th2, logp, alpha))


_equals_the_twin_reference_at_two()
