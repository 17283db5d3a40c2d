"""GPU tests of TQC on an ensemble of 2 .. 8 critics against the float64 restatement tests/tqc_ensemble_ref.py.

1. the ensemble critic loss kernel alone (tonic_debug_ensemble_quantile_loss) on crafted rows: unsorted targets whose
   pooled order interleaves all N critics, identical target critics, rows with discount 0, errors on both sides of
   |u| = 1, sentinels behind the M columns; a lone wave, a ragged workgroup and a general batch; pools of one, two and
   four values per lane.  Bit-identical launches; the twin kernel at N = 2; the critics permuted; the coefficient read
   on the device; non-finite targets.
2. tonic_ensemble_quantile_q_grad / _actor_grad: gradient sums per tensor and the logged statistics against float64
   autograd (the conventions and bounds of tests/test_gpu_offpolicy_grads.py), with the float coefficient and with
   the coefficient read on the device, whose own block is checked as well; the workspace query to the byte.
3. the agent: a whole update as a captured graph against the host loop of the same entries, bit for bit, without and
   with a tuner; save / load; the log keys; gradient clipping.

Every check prints the largest error it saw before it asserts."""
import math

import numpy as np
import pytest

import tqc_ensemble_ref as ref_n
import test_gpu_tqc as twin
from test_gpu_offpolicy_grads import _batch, _check, _check_stat, _f64, _set_normalizer, _squashed, _stats
from test_gpu_offpolicy_torsos import ACTIVATIONS, _grad_sums
from test_gpu_tqc import QuantileRef, bits, pad16

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# profiles/tqc_ensemble_accuracy.md: the largest errors of the loss kernel over the cases below, measured on one
# MI355X, times four (the margin of tests/test_gpu_tqc.py, for other inputs' rounding); the cap of 1e-5 does not bind
DLOGITS_BOUND = 4 * 5.041e-08       # max |dlogits - float64| over a row / the row's largest |d loss / d theta|
VALUE_BOUND = 4 * 5.904e-08         # loss_m, q relative to float64
assert DLOGITS_BOUND <= 1e-5 and VALUE_BOUND <= 1e-5
ALPHA = 0.2


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


# ---------------------------------------------------------------- 1. the loss kernel alone

LOSS_CASES = [(2, 25, 2),       # today's case
              (3, 22, 5),       # a pool of 66: the first with two values per lane
              (5, 25, 2),       # the paper's
              (5, 7, 3),        # a pool of 35, padded
              (3, 1, 0),        # M = 1
              (8, 32, 0),       # a pool of 256, nothing dropped
              (8, 32, 31)]      # K = 8
LOSS_BATCHES = (1, 5, 37)
INTERLEAVED, TWINS, RANDOM = 0, 1, 2                                    # row m's kind: m % 3


def crafted_rows(B, N, M, seed=0):
    """float32 `targets` / `thetas` [N, B, M], the rows' vectors and kinds: tests/test_gpu_tqc.py's rows over N
    critics.  Values sit around +5 so that q stays away from 0 (its error is relative); an interleaved row's sorted
    pool reads critic 0 1 .. N - 1 0 1 .. and spans 1.4 M above the base whatever N is, the online quantiles lie +-3
    around it: errors of every size and both signs."""
    rng = np.random.RandomState(100000 * N + 1000 * M + 10 * B + seed)
    base = 5.0 + rng.uniform(-1, 1, size=(B, 1))
    k = np.arange(M)[None]
    targets = np.stack([base + (N * k + z) * (1.4 / N) for z in range(N)])
    kinds = np.arange(B) % 3
    for m in range(B):
        for z in range(N):
            targets[z, m] = targets[z, m, rng.permutation(M)]                        # unsorted
        if kinds[m] == TWINS:
            targets[:, m] = targets[0, m]
        elif kinds[m] == RANDOM:
            targets[:, m] = 5.0 + rng.normal(size=(N, M)) * 3
    rows = dict(targets=targets, thetas=base[None] + rng.uniform(-3, 3, size=(N, B, M)),
                rewards=rng.uniform(-1, 1, size=B), discounts=np.where(np.arange(B) % 4 == 3, 0.0, 0.99),
                logp=rng.normal(size=B) * 2 - 1)
    return {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in rows.items()}, kinds


def reference(rows, d, alpha=ALPHA):
    """(loss_m, [d loss_m / d theta_z], q), the kept values' sources and the errors u [B, N M, K] in float64."""
    r = {k: v.double() for k, v in rows.items()}
    targets, thetas = list(r['targets']), list(r['thetas'])
    out = ref_n.critic_rows_with_gradients(targets, thetas, r['rewards'], r['discounts'], r['logp'], alpha, d)
    y, source = ref_n.truncated_targets(targets, r['rewards'], r['discounts'], r['logp'], alpha, d)
    u = torch.cat([y[:, None, :] - theta[:, :, None] for theta in thetas], dim=1)
    return out, source, u


_loss_reference = {}


def loss_reference(B, N, M, d, alpha=ALPHA):
    """The float64 outputs of a case, computed once."""
    key = (B, N, M, d, alpha)
    if key not in _loss_reference:
        rows, kinds = crafted_rows(B, N, M)
        _loss_reference[key] = (rows, kinds) + reference(rows, d, alpha)
    return _loss_reference[key]


SENTINELS = (777.0, -777.0, float('nan'), 555.0, float('inf'), -1e30, 0.0, 3.0)


def launch_loss(lib, rows, d, alpha=ALPHA, log_alpha=None, ld=None):
    """(dlogits [N, B, ld], sample_m [2, B]) of the kernel on `rows`; what lies behind the M columns of the inputs is
    a sentinel of the critic's own, never read."""
    from tonic_amd import _lib
    N, B, M = rows['targets'].shape
    ld, Bp, p = ld or pad16(M), pad16(B), _lib.ptr

    def padded(x, shift):
        out = torch.empty((N, B, ld), dtype=torch.float32)
        for z in range(N):
            out[z] = SENTINELS[(z + shift) % len(SENTINELS)]
        out[:, :, :M] = x
        return out.cuda()
    targets, thetas = padded(rows['targets'], 0), padded(rows['thetas'], 2)
    r, disc, logp = rows['rewards'].cuda(), rows['discounts'].cuda(), rows['logp'].cuda()
    dlogits = torch.full((N, B, ld), float('nan'), device='cuda')
    sample_m = torch.full((3, Bp), float('nan'), device='cuda')
    _lib.check(lib.tonic_debug_ensemble_quantile_loss(
        p(targets), p(thetas), ld, p(r), p(disc), p(logp), M, N, d, float(alpha), p(log_alpha), p(dlogits), p(sample_m),
        B, Bp, 0, _lib.current_stream()), 'tonic_debug_ensemble_quantile_loss')
    torch.cuda.synchronize()
    assert np.array_equal(bits(sample_m[2, :B]), np.zeros(B, np.int32)), 'the third row of the {loss, q} form is not 0'
    return dlogits.cpu(), sample_m[:2, :B].cpu()


def loss_errors(got, want, M):
    """(the dlogits' error in units of the row's largest |d loss / d theta|, the values' relative error); the padded
    columns are exactly 0."""
    dlogits, sample_m = got
    loss, grads, q = want
    grads = torch.stack(grads)                                    # [N, B, M]
    assert torch.equal(dlogits[:, :, M:], torch.zeros_like(dlogits[:, :, M:])), 'a padded column is not 0'
    scale = grads.abs().amax(dim=(0, 2))                          # [B]
    flat = scale == 0
    assert not dlogits[:, flat, :M].any() and not flat.all()
    scale = torch.where(flat, torch.ones_like(scale), scale)
    gradient = float(((dlogits[:, :, :M].double() - grads).abs().amax(dim=(0, 2)) / scale).max())
    value = max(float(((sample_m[i].double() - w).abs() / w.abs()).max()) for i, w in enumerate((loss, q)))
    return gradient, value


@pytest.mark.parametrize('B', LOSS_BATCHES)
@pytest.mark.parametrize('N,M,d', LOSS_CASES)
def test_loss_kernel_vs_float64_on_crafted_rows(lib, N, M, d, B):
    rows, kinds, want, source, u = loss_reference(B, N, M, d)
    K, everyone = N * (M - d), set(range(N))
    # what the rows were crafted for, asserted on the reference
    for m in np.flatnonzero(kinds == INTERLEAVED):
        kept, dropped = set(source[m, :K].tolist()), set(source[m, K:].tolist())
        assert kept == everyone and (d == 0 or dropped == everyone), (m, kept, dropped)
        assert source[m, :N].tolist() == list(range(N))                      # 0 1 .. N - 1 0 1 ..: interleaved
    for m in np.flatnonzero(kinds == TWINS):
        assert all(torch.equal(rows['targets'][z, m], rows['targets'][0, m]) for z in range(N))
    if B >= 5:
        assert (kinds == TWINS).any() and (kinds == RANDOM).any() and (rows['discounts'] == 0).any()
        assert (u.abs() < 1).any() and (u > 1).any() and (u < -1).any()
        if M > 1:
            live = u[rows['discounts'] != 0]
            assert ((live > 0) & (live < 1)).any() and ((live < 0) & (live > -1)).any()
    got = launch_loss(lib, rows, d)
    gradient, value = loss_errors(got, want, M)
    print(f'N={N} M={M} d={d} B={B}: dlogits {gradient:.3e} of the row\'s largest gradient, values {value:.3e} relative')
    again = launch_loss(lib, rows, d)
    for a, b in zip(got, again):
        assert np.array_equal(bits(a), bits(b)), 'two launches on the same inputs differ'
    assert gradient <= DLOGITS_BOUND and value <= VALUE_BOUND, (gradient, value)


def test_loss_kernel_on_rows_wider_than_their_quantiles(lib):
    """ld = 32 over M = 7: 25 padded columns per critic, all 0, and the outputs of ld = 16."""
    rows, _, want, _, _ = loss_reference(5, 5, 7, 3)
    narrow, wide = launch_loss(lib, rows, 3), launch_loss(lib, rows, 3, ld=32)
    assert wide[0].shape == (5, 5, 32)
    loss_errors(wide, want, 7)
    assert np.array_equal(bits(wide[0][:, :, :7]), bits(narrow[0][:, :, :7]))
    assert np.array_equal(bits(wide[1]), bits(narrow[1]))


@pytest.mark.parametrize('N,M,d', [(3, 22, 5), (5, 25, 2), (8, 32, 2)])
def test_loss_kernel_permutes_with_its_critics(lib, N, M, d):
    """Identical target critics and the online critics handed over in another order: the gradients in that order, bit
    for bit (a quantile's sum does not depend on the lane and register that hold it); the row's values to rounding."""
    rows, _ = crafted_rows(37, N, M)
    rows['targets'] = rows['targets'][:1].expand(N, -1, -1).clone()
    order = np.random.RandomState(N).permutation(N)
    assert (order != np.arange(N)).any()
    dlogits, sample_m = launch_loss(lib, rows, d)
    permuted, permuted_m = launch_loss(lib, dict(rows, thetas=rows['thetas'][order].clone()), d)
    assert np.array_equal(bits(permuted), bits(dlogits[order]))
    np.testing.assert_allclose(permuted_m.numpy(), sample_m.numpy(), rtol=4e-7)       # (the sums' order: float64)


def test_loss_kernel_reads_the_coefficient_on_the_device(lib):
    B, N, M, d = 5, 5, 25, 2
    log_alpha = torch.tensor([math.log(0.35)], dtype=torch.float32)
    rows, _, want, _, _ = loss_reference(B, N, M, d, alpha=math.exp(float(log_alpha.double())))
    got = launch_loss(lib, rows, d, alpha=123.0, log_alpha=log_alpha.cuda())      # (the float is then unused)
    gradient, value = loss_errors(got, want, M)
    print(f'device coefficient: dlogits {gradient:.3e}, values {value:.3e}')
    assert gradient <= DLOGITS_BOUND and value <= VALUE_BOUND, (gradient, value)


def test_loss_kernel_terminates_on_non_finite_targets(lib):
    """A pool of 256 with NaN, +-inf and a whole NaN row: the launch returns, and the untouched row is unchanged."""
    rows, _ = crafted_rows(5, 8, 32)
    clean = launch_loss(lib, rows, 2)
    rows['targets'] = rows['targets'].clone()
    rows['targets'][0, 0, 3], rows['targets'][5, 1, :] = float('nan'), float('inf')
    rows['targets'][7, 2, 7], rows['targets'][1, 3, 0] = float('-inf'), float('nan')
    rows['targets'][:, 3, :] = float('nan')
    dlogits, sample_m = launch_loss(lib, rows, 2)                 # (returns: that is the test)
    assert torch.isfinite(dlogits[:, 4]).all() and torch.isfinite(sample_m[:, 4]).all()
    assert np.array_equal(bits(dlogits[:, 4]), bits(clean[0][:, 4]))
    assert np.array_equal(bits(sample_m[:, 4]), bits(clean[1][:, 4]))


# ---------------------------------------------------------------- 2. the entries against float64 autograd

def _model(tt, sizes, activation, M, N):
    act = ACTIVATIONS[activation]
    head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                        distribution=tt.models.SquashedMultivariateNormalDiag)
    return tt.models.ActorCriticEnsembleWithTargets(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=tt.models.QuantileValueHead(M)),
        num_critics=N, observation_normalizer=tt.normalizers.MeanStd())


def _agent(O, A, B, sizes, activation, M, N, drop, tuner=None, iterations=1, seed=9, replay_size=1000, **updater):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    agent = tt.agents.TQC(
        model=_model(tt, sizes, activation, M, N),
        replay=tonic_amd.replays.Buffer(size=replay_size, batch_iterations=iterations, batch_size=B, steps_before_batches=0,
                                        steps_between_batches=1),
        critic_updater=tt.updaters.TruncatedQuantileQLearning(top_quantiles_to_drop_per_net=drop, **updater),
        actor_updater=tt.updaters.TwinCriticQuantileSoftPolicyGradient(**updater), entropy_coeff_updater=tuner)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=seed)
    assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
    assert agent._u.route().fused_kind is None
    assert agent.model.flat_critics.count % N == 0 and agent.critic_updater.count == agent.model.flat_critics.count
    return agent


def _critics(model, target=False):
    prefix = 'target_critic_' if target else 'critic_'
    return [getattr(model, f'{prefix}{z}') for z in range(1, model.num_critics + 1)]


def _spread_targets(agent, gain=8.0, seed=0):
    """tests/test_gpu_tqc.py's `_spread_targets` over the N target critics: away from the online ones and from each
    other, so that the sort has something to truncate."""
    from tonic_amd.torch.models import network_variables
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for critic in _critics(agent.model, target=True):
            for p in network_variables(critic):
                p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.1, dtype=torch.float32, device=p.device)
            critic.head.quantile_layer.weight.mul_(gain)
            critic.head.quantile_layer.bias.add_(
                torch.as_tensor(rng.normal(size=critic.head.num_quantiles), dtype=torch.float32, device=p.device))


ENTRY_CASES = {
    # name: (sizes, activation, B, N, M, drop, O, A)
    'paper': ((32, 32), 'ReLU', 33, 5, 25, 2, 17, 6),
    'tanh_layers': ((48, 32), 'Tanh', 5, 3, 7, 1, 17, 6),
}
LOG_ALPHA = math.log(0.35)
TARGET_ENTROPY = -2.5


@pytest.mark.parametrize('coefficient', ['float', 'device'])
@pytest.mark.parametrize('case', ENTRY_CASES)
def test_entries_vs_float64_autograd(lib, case, coefficient):
    import tonic_amd.torch as tt
    sizes, activation, B, N, M, drop, O, A = ENTRY_CASES[case]
    tuner = None
    if coefficient == 'device':
        tuner = tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=math.exp(LOG_ALPHA), target_entropy=TARGET_ENTROPY)
    agent = _agent(O, A, B, sizes, activation, M, N, drop, tuner=tuner)
    rng = np.random.RandomState(B + M)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, 0.5 + rng.uniform(size=O))
    _spread_targets(agent)
    m, critic_u, actor_u = agent.model, agent.critic_updater, agent.actor_updater
    alpha = ALPHA
    if tuner is not None:
        assert critic_u.entropy_coeff_updater is tuner and actor_u.entropy_coeff_updater is tuner
        alpha = math.exp(float(tuner.log_entropy_coeff.double()))
        critic_u.entropy_coeff = actor_u.entropy_coeff = 77.0            # (unused with a tuner)
    ref = QuantileRef(agent, len(sizes), activation)
    batch = _batch(rng, B, O, A)
    eps, eps_actor = (torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32) for _ in range(2))
    critics, targets = _critics(m), _critics(m, target=True)
    assert len(critics) == len(targets) == N
    actor = _f64(m.actor)
    online, frozen = [_f64(c) for c in critics], [_f64(c) for c in targets]
    d = {k: v.double() for k, v in batch.items()}
    gpu = {k: v.cuda() for k, v in batch.items()}
    # ---- the critic step
    with torch.no_grad():
        loc, scale = ref.policy(actor, d['next_observations'])
        a, logp = _squashed(loc, scale, eps.double())
        pool = [ref.critic(p, d['next_observations'], a) for p in frozen]
        _, source = ref_n.truncated_targets(pool, d['rewards'], d['discounts'], logp, alpha, drop)
    # the truncation is not trivial: every critic among the kept values, and rows that drop values of several critics
    K = N * (M - drop)
    assert all(set(source[r, :K].tolist()) == set(range(N)) for r in range(B))
    assert max(len(set(source[r, K:].tolist())) for r in range(B)) > 1
    thetas = [ref.critic(p, d['observations'], d['actions']) for p in online]
    rows = ref_n.critic_rows(pool, thetas, d['rewards'], d['discounts'], logp, alpha, drop)
    rows.mean().backward()
    info = torch.zeros(8, device='cuda')
    critic_u.enqueue(gpu, eps.cuda(), info)
    stats = _stats(critic_u)
    assert stats[5] == B and (stats[[2, 3, 4, 6, 7]] == 0).all(), stats
    got = _grad_sums(critics, critic_u.grad_sums, B)
    leaves = [leaf for p in online for leaf in p]
    assert len(got) == len(leaves) == N * (2 * len(sizes) + 2)
    names = [f'critic {i // (2 * len(sizes) + 2) + 1} tensor {i % (2 * len(sizes) + 2)}' for i in range(len(got))]
    worst = _check(got, leaves, names, None)
    print(f'{case} {coefficient}: critic tensors {worst:.3e}')
    _check(got, leaves, names)
    _check_stat(stats[0] / B, rows.detach().mean(), rows.detach(), 'critic loss')
    q = torch.stack([theta.detach().mean(dim=1) for theta in thetas]).mean(dim=0)
    _check_stat(stats[1] / B, q.mean(), q, 'q')
    # ---- the actor step, through the critics the critic step has just moved
    online = [_f64(c) for c in critics]
    loc, scale = ref.policy(actor, d['observations'])
    a, logp = _squashed(loc, scale, eps_actor.double())
    terms = ref_n.actor_rows([ref.critic(p, d['observations'], a) for p in online], logp, alpha)
    terms.mean().backward()
    actor_u.enqueue(gpu['observations'], eps_actor.cuda(), info)
    stats = _stats(actor_u)
    assert stats[5] == B and (np.delete(stats, [0, 5]) == 0).all(), stats
    got = _grad_sums([m.actor], actor_u.grad_sums, B)
    worst = _check(got, actor, [f'actor {i}' for i in range(len(actor))], None)
    print(f'{case} {coefficient}: actor tensors {worst:.3e}')
    _check(got, actor, [f'actor {i}' for i in range(len(actor))])
    _check_stat(stats[0] / B, terms.detach().mean(), terms.detach(), 'actor loss')
    if tuner is not None:          # the coefficient's block, as tonic_tempered_actor_q_grad lays it out
        torch.cuda.synchronize()
        block = tuner.grad_sums.cpu().double().numpy()
        log_alpha, lp = float(tuner.log_entropy_coeff.double()), logp.detach()
        excess = lp + TARGET_ENTROPY
        _check_stat(block[0], -excess.sum(), excess * B, 'd J / d log_alpha')
        _check_stat(block[1], -log_alpha * excess.sum(), log_alpha * excess * B, 'coefficient loss')
        _check_stat(block[2], lp.sum(), lp * B, 'sum of log-probabilities')
        _check_stat(block[3], alpha * B, None, 'alpha B')
        assert block[6] == B and (block[[4, 5, 7, 8]] == 0).all(), block
    agent.close()


def test_workspace_query_is_exact(lib):
    """Both entries run in a workspace of exactly the query's bytes and write nothing behind it; with one byte less
    they return the workspace error and write nothing at all.  The twin query is the ensemble's at N = 2, no more than
    the twin layout of its own asked for."""
    from test_tqc_ensemble_host import TWIN_QUERY
    B, O, A, N, M = 33, 17, 6, 5, 25
    agent = _agent(O, A, B, (32, 32), 'ReLU', M, N, 2)
    _spread_targets(agent)
    critic_u, actor_u = agent.critic_updater, agent.actor_updater
    need = lib.tonic_ensemble_quantile_workspace_bytes(B, O, A, critic_u.hidden, M, N)
    assert need == critic_u._workspace_bytes(B) == actor_u._workspace_bytes(B) and need % 256 == 0
    assert need > lib.tonic_quantile_workspace_bytes(B, O, A, critic_u.hidden, M)
    rng = np.random.RandomState(1)
    batch = {k: v.cuda() for k, v in _batch(rng, B, O, A).items()}
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32).cuda()
    info = torch.zeros(8, device='cuda')
    guard = 4096
    steps = ((critic_u, lambda: critic_u.enqueue(batch, eps, info)),
             (actor_u, lambda: actor_u.enqueue(batch['observations'], eps, info)))
    for updater, step in steps:
        arena = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device='cuda')
        updater._offpolicy_workspace = lambda rows, arena=arena: arena[:need]
        updater.grad_sums.zero_()
        step()
        torch.cuda.synchronize()
        assert bool((arena[need:] == 0xA5).all()), 'a write behind the workspace'
        assert float(updater.grad_sums[updater.count + 5]) == B and not bool((arena[:need] == 0xA5).all())
        arena.fill_(0xA5)
        updater._offpolicy_workspace = lambda rows, arena=arena: arena[:need - 1]
        kept = updater.grad_sums.clone()
        with pytest.raises(Exception, match=f'workspace of {need - 1} bytes, {need} needed'):
            step()
        torch.cuda.synchronize()
        assert bool((arena == 0xA5).all()) and torch.equal(updater.grad_sums, kept), 'a refused call wrote'
    for key, before in TWIN_QUERY.items():
        answer = lib.tonic_quantile_workspace_bytes(*key)
        assert answer == lib.tonic_ensemble_quantile_workspace_bytes(*key, 2) and 0 < answer <= before, key
    agent.close()


# ---------------------------------------------------------------- 3. the agent

N_AGENT, M_AGENT = 3, 7


def _filled_agent(B, iterations, tuner_kwargs=None, sizes=(32, 32), O=17, A=6, rows=30, W=4, **updater):
    import tonic_amd.torch as tt
    tuner = tt.updaters.EntropyCoeffTuning(**tuner_kwargs) if tuner_kwargs is not None else None
    agent = _agent(O, A, B, sizes, 'ReLU', M_AGENT, N_AGENT, 2, tuner=tuner, iterations=iterations, seed=7,
                   replay_size=rows * W, **updater)
    rng = np.random.RandomState(321)
    for _ in range(rows - 3):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        row = {k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()}
        agent.replay.store(normalizer=agent.model.observation_normalizer, **row)
    return agent


@pytest.mark.parametrize('tuned', [False, True])
def test_captured_update_equals_the_host_loop(lib, monkeypatch, tuned):
    B, iterations, A = 33, 2, 6
    fast = dict(initial_entropy_coeff=0.5, optimizer=lambda params: torch.optim.Adam(params, lr=0.05)) if tuned else None
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH', raising=False)
    captured = _filled_agent(B, iterations, fast)
    before = {k: v.clone() for k, v in captured.model.state_dict().items()}
    got, graphs = twin._updates(captured, 3, iterations, B, A)             # the capture's own update, then two replays
    assert graphs[0] is not None and all(g is graphs[0] for g in graphs), 'the graph was captured again'
    monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    eager = _filled_agent(B, iterations, fast)
    want, none = twin._updates(eager, 3, iterations, B, A)
    assert all(g is None for g in none)
    for call, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(('infos', 'coefficient rows', 'log_entropy_coeff'), g, w):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (call, name)
    moved = 0
    for key, value in captured.model.state_dict().items():
        assert np.array_equal(bits(value), bits(eager.model.state_dict()[key])), key
        moved += int(not torch.equal(value, before[key]))
    assert moved >= 8 + 12 * N_AGENT                      # actor, every critic and all targets took their steps
    infos = got[-1][0]
    assert np.isfinite(infos).all() and (infos[:, :, 6] == 1.0).all() and (infos[0, :, 0] > 0).all()
    assert (infos[0, :, 2] == 0).all() and (infos[0, :, 1] != 0).all()       # the ensemble's row: loss, q, nothing
    if tuned:
        trajectory = np.concatenate([g[2] for g in got])
        assert len(set(trajectory.tolist())) == 3                     # alpha moved on every call
        assert abs(float(trajectory[-1]) - math.log(0.5)) > 1e-2
    captured.close()
    eager.close()


def test_save_load_and_log_keys(lib, tmp_path, monkeypatch):
    import tonic_amd.torch as tt
    B, iterations, A = 33, 1, 6
    fast = dict(initial_entropy_coeff=0.5, optimizer=lambda params: torch.optim.Adam(params, lr=0.05))
    agent = _filled_agent(B, iterations, fast)
    out, _ = twin._updates(agent, 2, iterations, B, A)
    stored = []
    monkeypatch.setattr(tt.agents.logger, 'store', lambda key, value, **kwargs: stored.append(key))
    agent._log_update(out[-1][0], out[-1][1])
    keys = set(stored)
    assert {'critic/loss', 'critic/q', 'actor/loss', 'entropy_coeff/value'} <= keys, keys
    assert not keys & {'critic/q1', 'critic/q2'}, keys
    # the updater's drop-in call names the same row
    batch = {k: v.cuda() for k, v in _batch(np.random.RandomState(0), B, 17, A).items()}
    row = agent.critic_updater(**batch)
    assert sorted(row) == ['loss', 'q'] and all(np.isfinite(float(v)) for v in row.values())
    path = str(tmp_path / 'agent')
    agent.save(path)
    saved = torch.load(path + '.pt', map_location='cpu')
    assert sorted(saved) == sorted(agent.model.state_dict())
    assert saved[f'critic_{N_AGENT}.head.quantile_layer.weight'].shape == (M_AGENT, 32)
    assert f'target_critic_{N_AGENT}.head.quantile_layer.bias' in saved and f'critic_{N_AGENT + 1}.head' not in str(sorted(saved))
    fresh = _filled_agent(B, iterations, dict(initial_entropy_coeff=2.0))
    assert any(not torch.equal(v, agent.model.state_dict()[k]) for k, v in fresh.model.state_dict().items())
    fresh.load(path)
    assert np.array_equal(bits(fresh.entropy_coeff_updater.log_entropy_coeff),
                          bits(agent.entropy_coeff_updater.log_entropy_coeff))
    for key, value in agent.model.state_dict().items():
        assert np.array_equal(bits(fresh.model.state_dict()[key]), bits(value)), key
    # the loaded agent goes on as the saved one does
    a, _ = twin._updates(agent, 1, iterations, B, A)
    b, _ = twin._updates(fresh, 1, iterations, B, A)
    assert np.array_equal(a[0][0].view(np.int32)[0], b[0][0].view(np.int32)[0])        # the critic step's row
    agent.close()
    fresh.close()


def test_gradient_clip_runs_and_clips(lib):
    B, O, A, clip = 33, 17, 6, 1e-3
    rng = np.random.RandomState(3)
    batch = {k: v.cuda() for k, v in _batch(rng, B, O, A).items()}
    eps = torch.as_tensor(rng.normal(size=(2, B, A)), dtype=torch.float32).cuda()
    sums = {}
    for name, value in (('free', 0), ('clipped', clip)):
        agent = _agent(O, A, B, (32, 32), 'ReLU', M_AGENT, N_AGENT, 2, gradient_clip=value)
        _spread_targets(agent)
        info = torch.zeros(8, device='cuda')
        agent.critic_updater.enqueue(batch, eps[0], info)
        agent.actor_updater.enqueue(batch['observations'], eps[1], info)
        torch.cuda.synchronize()
        assert float(info[6]) == 1.0
        assert agent.critic_updater.count == agent.model.flat_critics.count
        sums[name] = [u.grad_sums[:u.count].double().cpu() / B for u in (agent.critic_updater, agent.actor_updater)]
        agent.close()
    # the critic step: the same inputs, so the clipped sums are the free ones scaled down to the norm `clip` — the norm
    # of the whole N-critic block, every critic's part of it moved
    free, clipped = sums['free'][0], sums['clipped'][0]
    norm = float(free.norm())
    assert norm > 10 * clip
    blocks = free.view(N_AGENT, -1).norm(dim=1)
    assert (blocks > 0).all() and (blocks < norm).all()
    print(f'critic gradient norm {norm:.3e} -> {float(clipped.norm()):.3e}')
    np.testing.assert_allclose(float(clipped.norm()), clip, rtol=1e-4)
    np.testing.assert_allclose(clipped.numpy(), (free * (clip / norm)).numpy(), rtol=0, atol=1e-5 * clip)
    assert float(sums['free'][1].norm()) > 10 * clip
    np.testing.assert_allclose(float(sums['clipped'][1].norm()), clip, rtol=1e-4)
