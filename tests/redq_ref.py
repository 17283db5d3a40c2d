"""REDQ (Chen et al. 2021, randomized ensembled double Q-learning) restated in float64 torch for the tests: the
subset a device word names, the minimum over it with torch's NaN propagation, the critic rows of ALL N online critics
under a critic-loss rule with their gradients, and the actor's terms."""
import torch

MSE, L1, SMOOTH_L1, HUBER = 0, 1, 2, 3                 # tonic_critic_loss_t kinds (include/tonic_hip.h)


def subset_of(mask, N):
    """The critics (0-based, ascending) a word names among N: the low N bits; none of them set means all N."""
    members = [z for z in range(N) if (int(mask) >> z) & 1]
    return members or list(range(N))


def mask_of(members):
    mask = 0
    for z in members:
        mask |= 1 << int(z)
    return mask


def subset_min(targets, members):
    """min over the subset of the target critics' values [B] — torch.minimum, which keeps a NaN — and which member
    holds it (the first on a tie; -1 where the minimum is a NaN)."""
    low = targets[members[0]]
    for z in members[1:]:
        low = torch.minimum(low, targets[z])
    who = torch.full(low.shape, -1, dtype=torch.int64)
    for z in reversed(members):
        who = torch.where(targets[z] == low, torch.full_like(who, z), who)
    return low, who


def td_target(targets, rewards, discounts, logp_next, alpha, members):
    low, _ = subset_min(targets, members)
    return rewards + discounts * (low - alpha * logp_next)


def loss_terms(e, kind, param):
    """The rule's per-sample term l(e), as torch.nn.functional's mse / l1 / smooth_l1 / huber losses define it."""
    z = e.abs()
    if kind == MSE:
        return e * e
    if kind == HUBER:
        return torch.where(z < param, 0.5 * e * e, param * (z - 0.5 * param))
    if kind == SMOOTH_L1 and param > 0:
        return torch.where(z < param, 0.5 * e * e / param, z - 0.5 * param)
    return z


def loss_slopes(e, kind, param):
    """d l / d e in closed form (a NaN error: NaN, except where the rule is the sign alone, which gives 0)."""
    if kind == MSE:
        return 2 * e
    if kind == HUBER:
        return torch.where(e <= -param, torch.full_like(e, -param), torch.where(e >= param, torch.full_like(e, param), e))
    if kind == SMOOTH_L1 and param > 0:
        return torch.where(e <= -param, -torch.ones_like(e), torch.where(e >= param, torch.ones_like(e), e / param))
    return (e > 0).to(e.dtype) - (e < 0).to(e.dtype)


def critic_rows(targets, qs, rewards, discounts, logp_next, alpha, members, kind=MSE, param=0.0):
    """loss_m [B] = sum_z l(Q_z - y) over all N online critics (differentiable in `qs`)."""
    y = td_target(targets, rewards, discounts, logp_next, alpha, members).detach()
    return sum(loss_terms(q - y, kind, param) for q in qs)


def critic_rows_with_gradients(targets, qs, rewards, discounts, logp_next, alpha, members, kind=MSE, param=0.0):
    """(loss_m [B], [d loss_m / d Q_z [B]], q [B] = the mean over the critics), the gradients in closed form."""
    y = td_target(targets, rewards, discounts, logp_next, alpha, members)
    errors = [q - y for q in qs]
    loss = sum(loss_terms(e, kind, param) for e in errors)
    return loss, [loss_slopes(e, kind, param) for e in errors], sum(qs) / len(qs)


def actor_rows(qs, logp, alpha):
    """alpha logp - (1 / N) sum_z Q_z(s, a) [B]."""
    return alpha * logp - sum(qs) / len(qs)
