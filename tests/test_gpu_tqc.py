"""GPU tests of TQC (truncated quantile critics) against the float64 restatement tests/tqc_ref.py.

1. the critic loss kernel alone in the twin form (tonic_debug_ensemble_quantile_loss at N = 2 with the twin row
   {loss, q1, q2}) on crafted rows: unsorted targets whose pooled order interleaves the two critics, identical target critics, rows with discount 0, errors on both
   sides of |u| = 1; a lone wave, a ragged workgroup and a general batch; K = 2 at both ends of M, no truncation,
   2 M = 64 and a row wider than 2 M.  Bit-identical launches; the bits of the twin kernel this one replaced
   (tests/golden/tqc_twin_loss_parent.npz, scripts/tqc_twin_rows_record.py).
2. tonic_truncated_quantile_q_grad / _actor_grad: gradient sums per tensor and the logged statistics against float64
   autograd (the conventions and bounds of tests/test_gpu_offpolicy_grads.py), with the float coefficient and with
   the coefficient read on the device, whose own block is checked as well.
3. the agent: a whole update as a captured graph against the host loop of the same entries, bit for bit, without and
   with a tuner; save / load; two ranks against one; gradient clipping.

Every check prints the largest error it saw before it asserts."""
import hashlib
import math
import os

import numpy as np
import pytest

import tqc_ref
from test_gpu_offpolicy_grads import Ref, _batch, _check, _check_stat, _f64, _set_normalizer, _squashed, _stats
from test_gpu_offpolicy_torsos import ACTIVATIONS, _grad_sums

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# profiles/tqc_accuracy.md: the largest errors of the loss kernel over the cases below, measured on one MI355X, times
# four; the cap of 1e-5 does not bind
DLOGITS_BOUND = 4 * 5.849e-07       # max |dlogits - float64| over a row / the row's largest |d loss / d theta|
VALUE_BOUND = 4 * 5.928e-08         # loss_m, q1, q2 relative to float64
assert DLOGITS_BOUND <= 1e-5 and VALUE_BOUND <= 1e-5
ALPHA = 0.2


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def bits(tensor):
    return tensor.detach().cpu().contiguous().view(torch.int32).numpy()


def pad16(n):
    return (n + 15) // 16 * 16


# ---------------------------------------------------------------- 1. the loss kernel alone

LOSS_CASES = [(1, 0), (2, 1), (25, 2), (25, 0), (32, 2), (32, 31)]       # (M, d)
LOSS_BATCHES = (1, 5, 37)
INTERLEAVED, TWINS, RANDOM = 0, 1, 2                                    # row m's kind: m % 3


def crafted_rows(B, M, seed=0):
    """float32 rows [B, M] and the rows' kinds.  Values sit around +5 so that q1 / q2 stay away from 0 (their error
    is relative); the targets span up to 2 M * 0.7 above that, the online quantiles +-3 around it: errors of every
    size and both signs."""
    rng = np.random.RandomState(1000 * M + 10 * B + seed)
    base = 5.0 + rng.uniform(-1, 1, size=(B, 1))
    k = np.arange(M)[None]
    t1, t2 = base + 2 * k * 0.7, base + (2 * k + 1) * 0.7                # sorted pool: 1 2 1 2 ...
    kinds = np.arange(B) % 3
    for m in range(B):
        t1[m], t2[m] = t1[m, rng.permutation(M)], t2[m, rng.permutation(M)]           # unsorted
        if kinds[m] == TWINS:
            t2[m] = t1[m]
        elif kinds[m] == RANDOM:
            t1[m], t2[m] = 5.0 + rng.normal(size=M) * 3, 5.0 + rng.normal(size=M) * 3
    rows = dict(target_1=t1, target_2=t2, theta_1=base + rng.uniform(-3, 3, size=(B, M)),
                theta_2=base + rng.uniform(-3, 3, size=(B, M)), rewards=rng.uniform(-1, 1, size=B),
                discounts=np.where(np.arange(B) % 4 == 3, 0.0, 0.99), logp=rng.normal(size=B) * 2 - 1)
    return {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in rows.items()}, kinds


_loss_reference = {}


def loss_reference(B, M, d, alpha=ALPHA):
    """The float64 outputs of a case, computed once."""
    key = (B, M, d, alpha)
    if key not in _loss_reference:
        rows, kinds = crafted_rows(B, M)
        r = {k: v.double() for k, v in rows.items()}
        out = tqc_ref.critic_rows_with_gradients(r['target_1'], r['target_2'], r['theta_1'], r['theta_2'],
                                                 r['rewards'], r['discounts'], r['logp'], alpha, d)
        y, source = tqc_ref.truncated_targets(r['target_1'], r['target_2'], r['rewards'], r['discounts'], r['logp'],
                                              alpha, d)
        u = torch.cat([tqc_ref.errors(r['theta_1'], y), tqc_ref.errors(r['theta_2'], y)], dim=1)
        _loss_reference[key] = (rows, kinds, out, source, u)
    return _loss_reference[key]


def launch_loss(lib, rows, M, d, alpha=ALPHA, log_alpha=None):
    from tonic_amd import _lib
    B, ld, Bp, p = rows['rewards'].shape[0], pad16(M), pad16(rows['rewards'].shape[0]), _lib.ptr

    def padded(x, fill):                          # [B, ld]: what lies behind the M columns is never read
        out = torch.full((B, ld), fill, dtype=torch.float32)
        out[:, :M] = x
        return out.cuda()
    targets = torch.stack([padded(rows['target_1'], 777.0), padded(rows['target_2'], -777.0)])       # [2][B, ld]
    thetas = torch.stack([padded(rows['theta_1'], float('nan')), padded(rows['theta_2'], 555.0)])
    r, disc, logp = rows['rewards'].cuda(), rows['discounts'].cuda(), rows['logp'].cuda()
    dlogits = torch.full((2, B, ld), float('nan'), device='cuda')
    sample_m = torch.full((3, Bp), float('nan'), device='cuda')
    _lib.check(lib.tonic_debug_ensemble_quantile_loss(
        p(targets), p(thetas), ld, p(r), p(disc), p(logp), M, 2, d, float(alpha), p(log_alpha), p(dlogits),
        p(sample_m), B, Bp, 1, _lib.current_stream()), 'tonic_debug_ensemble_quantile_loss')
    torch.cuda.synchronize()
    return dlogits[0].cpu(), dlogits[1].cpu(), sample_m[:, :B].cpu()


def loss_errors(got, want, M):
    """(the dlogits' error in units of the row's largest |d loss / d theta|, the values' relative error)."""
    g1, g2, sample_m = got
    loss, d1, d2, q1, q2 = want
    assert torch.equal(g1[:, M:], torch.zeros_like(g1[:, M:])) and torch.equal(g2[:, M:], torch.zeros_like(g2[:, M:]))
    scale = torch.maximum(d1.abs().max(dim=1)[0], d2.abs().max(dim=1)[0])
    flat = scale == 0           # (M = 1: tau = 1/2 between the two kept targets, +1/2 - 1/2 — exactly 0 in float32 too)
    assert not (g1[flat, :M].any() or g2[flat, :M].any()) and not flat.all()
    scale = torch.where(flat, torch.ones_like(scale), scale)
    gradient = max(float(((g1[:, :M].double() - d1).abs().max(dim=1)[0] / scale).max()),
                   float(((g2[:, :M].double() - d2).abs().max(dim=1)[0] / scale).max()))
    value = max(float(((sample_m[i].double() - w).abs() / w.abs()).max()) for i, w in enumerate((loss, q1, q2)))
    return gradient, value


@pytest.mark.parametrize('B', LOSS_BATCHES)
@pytest.mark.parametrize('M,d', LOSS_CASES)
def test_loss_kernel_vs_float64_on_crafted_rows(lib, M, d, B):
    rows, kinds, want, source, u = loss_reference(B, M, d)
    K = 2 * (M - d)
    # what the rows were crafted for, asserted on the reference
    for m in np.flatnonzero(kinds == INTERLEAVED):
        kept, dropped = set(source[m, :K].tolist()), set(source[m, K:].tolist())
        assert kept == {0, 1} and (d == 0 or dropped == {0, 1}), (m, kept, dropped)
    assert torch.equal(rows['target_1'][kinds == TWINS], rows['target_2'][kinds == TWINS])
    if B >= 5:
        assert (kinds == TWINS).any() and (kinds == RANDOM).any() and (rows['discounts'] == 0).any()
        assert (u.abs() < 1).any() and (u > 1).any() and (u < -1).any()
        if M > 1:
            live = u[rows['discounts'] != 0]
            assert ((live > 0) & (live < 1)).any() and ((live < 0) & (live > -1)).any()
    got = launch_loss(lib, rows, M, d)
    gradient, value = loss_errors(got, want, M)
    print(f'M={M} d={d} B={B}: dlogits {gradient:.3e} of the row\'s largest gradient, values {value:.3e} relative')
    again = launch_loss(lib, rows, M, d)
    for a, b in zip(got, again):
        assert np.array_equal(bits(a), bits(b)), 'two launches on the same inputs differ'
    assert gradient <= DLOGITS_BOUND and value <= VALUE_BOUND, (gradient, value)


def rows_digest(rows):
    """sha256 of a case's input rows, in the order crafted_rows names them."""
    digest = hashlib.sha256()
    for name in ('target_1', 'target_2', 'theta_1', 'theta_2', 'rewards', 'discounts', 'logp'):
        digest.update(rows[name].contiguous().numpy().tobytes())
    return digest.hexdigest()


def ulps_apart(a, b):
    """How many float32 values lie between a and b, elementwise (finite values)."""
    def ordered(x):
        i = x.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (ordered(a) - ordered(b)).abs()


def test_loss_kernel_equals_the_retired_twin_kernel(lib):
    """tests/golden/tqc_twin_loss_parent.npz holds what the twin kernel of the commit before the fold
    (truncated_quantile_critic_loss_kernel: critic z = lane / 32, one wave_sum over that placement) wrote on
    crafted_rows for LOSS_CASES x LOSS_BATCHES, recorded by scripts/tqc_twin_rows_record.py.  The kernel kept gives
    the same dlogits bit for bit, padding included; loss_m, q1 and q2 are float64 sums over another lane placement
    cast once: within 1 float32 ulp."""
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tqc_twin_loss_parent.npz'))
    worst = 0
    for M, d in LOSS_CASES:
        for B in LOSS_BATCHES:
            key = f'M{M}_d{d}_B{B}'
            rows, _ = crafted_rows(B, M)
            assert rows_digest(rows) == str(golden[key + '_inputs_sha256']), f'{key}: the crafted rows changed'
            g1, g2, sample_m = launch_loss(lib, rows, M, d)
            assert np.array_equal(bits(g1), golden[key + '_dlogits_1'].view(np.int32)), key
            assert np.array_equal(bits(g2), golden[key + '_dlogits_2'].view(np.int32)), key
            apart = ulps_apart(sample_m, torch.as_tensor(golden[key + '_sample_m']))
            print(f'{key}: sample_m differs from the recording in {int((apart > 0).sum())} of {apart.numel()} values, '
                  f'by at most {int(apart.max())} ulp')
            worst = max(worst, int(apart.max()))
    assert worst <= 1, worst


def test_loss_kernel_does_not_care_which_twin_is_dropped(lib):
    """Identical target critics handed over in either order, and the two online critics swapped: the same bits, the
    gradients swapped."""
    rows, _ = crafted_rows(37, 25)
    rows['target_2'] = rows['target_1'].clone()
    g1, g2, sample_m = launch_loss(lib, rows, 25, 2)
    swapped = dict(rows, theta_1=rows['theta_2'], theta_2=rows['theta_1'])
    s1, s2, swapped_m = launch_loss(lib, swapped, 25, 2)
    assert np.array_equal(bits(g1), bits(s2)) and np.array_equal(bits(g2), bits(s1))
    assert np.array_equal(bits(sample_m[1]), bits(swapped_m[2])) and np.array_equal(bits(sample_m[2]), bits(swapped_m[1]))
    np.testing.assert_allclose(swapped_m[0].numpy(), sample_m[0].numpy(), rtol=4e-7)       # (loss_1 + loss_2: one add)


def test_loss_kernel_reads_the_coefficient_on_the_device(lib):
    B, M, d = 5, 25, 2
    log_alpha = torch.tensor([math.log(0.35)], dtype=torch.float32)
    rows, _, want, _, _ = loss_reference(B, M, d, alpha=math.exp(float(log_alpha.double())))
    got = launch_loss(lib, rows, M, d, alpha=123.0, log_alpha=log_alpha.cuda())      # (the float is then unused)
    gradient, value = loss_errors(got, want, M)
    print(f'device coefficient: dlogits {gradient:.3e}, values {value:.3e}')
    assert gradient <= DLOGITS_BOUND and value <= VALUE_BOUND, (gradient, value)


def test_loss_kernel_terminates_on_non_finite_targets(lib):
    rows, _ = crafted_rows(5, 32)
    rows['target_1'][0, 3], rows['target_1'][1, :] = float('nan'), float('inf')
    rows['target_2'][2, 7], rows['target_2'][3, 0] = float('-inf'), float('nan')
    rows['target_1'][3, :] = float('nan')
    g1, g2, sample_m = launch_loss(lib, rows, 32, 2)             # (returns: that is the test)
    assert torch.isfinite(g1[4]).all() and torch.isfinite(sample_m[:, 4]).all()      # an untouched row is as ever


# ---------------------------------------------------------------- 2. the entries against float64 autograd

class QuantileRef(Ref):
    """tests/test_gpu_offpolicy_grads.py's float64 networks with SAC's policy under the head's own scale bounds and a
    critic of M outputs."""

    def __init__(self, agent, layers, activation):
        super().__init__(agent, 'sac', layers, activation)
        bounds = agent.critic_updater.scale_bounds
        self.bounds = (float(bounds[0]), float(bounds[1]))

    def policy(self, params, obs):
        h, L = self._torso(params, obs), self.L
        scale = torch.nn.functional.softplus(self._linear(params, h, 2 * L + 2))
        return self._linear(params, h, 2 * L), torch.clamp(scale, *self.bounds)

    def critic(self, params, obs, act):
        return self._linear(params, self._torso(params, torch.cat([self.norm(obs), act], -1)), 2 * self.L)


def _model(tt, sizes, activation, M, bounds=None, clip=None):
    act = ACTIVATIONS[activation]
    extra = dict(scale_min=bounds[0], scale_max=bounds[1]) if bounds else {}
    head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                        distribution=tt.models.SquashedMultivariateNormalDiag, **extra)
    return tt.models.ActorTwinCriticWithTargets(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=tt.models.QuantileValueHead(M)),
        observation_normalizer=tt.normalizers.MeanStd(clip=clip) if clip else tt.normalizers.MeanStd())


def _agent(O, A, B, sizes, activation, M, drop, tuner=None, bounds=None, clip=None, iterations=1, seed=9,
           replay_size=1000, **updater):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    agent = tt.agents.TQC(
        model=_model(tt, sizes, activation, M, bounds, clip),
        replay=tonic_amd.replays.Buffer(size=replay_size, batch_iterations=iterations, batch_size=B, steps_before_batches=0,
                                        steps_between_batches=1),
        critic_updater=tt.updaters.TruncatedQuantileQLearning(top_quantiles_to_drop_per_net=drop, **updater),
        actor_updater=tt.updaters.TwinCriticQuantileSoftPolicyGradient(**updater), entropy_coeff_updater=tuner)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=seed)
    assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
    assert agent._u.route().fused_kind is None
    return agent


def _spread_targets(agent, gain=8.0, seed=0):
    """The target critics away from the online ones and from each other, their head weights times `gain` (as
    tests/test_gpu_td4.py's `_spread_targets`): freshly initialised heads give quantiles that hardly differ, and a
    sort of those would truncate next to nothing."""
    from tonic_amd.torch.models import network_variables
    rng = np.random.RandomState(seed)
    model = agent.model
    with torch.no_grad():
        for critic in (model.target_critic_1, model.target_critic_2):
            for p in network_variables(critic):
                p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.1, dtype=torch.float32, device=p.device)
            critic.head.quantile_layer.weight.mul_(gain)
            critic.head.quantile_layer.bias.add_(
                torch.as_tensor(rng.normal(size=critic.head.num_quantiles), dtype=torch.float32, device=p.device))


ENTRY_CASES = {
    # name: (sizes, activation, B, M, drop, O, A, extras)
    'one_row': ((32, 32), 'ReLU', 1, 2, 1, 3, 1, {}),
    'ragged': ((32, 32), 'ReLU', 5, 25, 2, 17, 6, {}),
    'full_wave': ((32, 32), 'ReLU', 37, 32, 2, 17, 6, {}),
    'tanh_layers': ((48, 40, 32), 'Tanh', 37, 25, 2, 17, 6, {}),
    'wide': ((256, 256), 'ReLU', 37, 25, 2, 17, 6, {}),
    'clip': ((32, 32), 'ReLU', 37, 25, 2, 17, 6, dict(clip=0.8)),
    'bounds': ((32, 32), 'ReLU', 37, 25, 2, 17, 6, dict(bounds=(0.05, 0.4))),
}
LOG_ALPHA = math.log(0.35)
TARGET_ENTROPY = -2.5


@pytest.mark.parametrize('coefficient', ['float', 'device'])
@pytest.mark.parametrize('case', ENTRY_CASES)
def test_entries_vs_float64_autograd(lib, case, coefficient):
    import tonic_amd.torch as tt
    sizes, activation, B, M, drop, O, A, extras = ENTRY_CASES[case]
    tuner = None
    if coefficient == 'device':
        tuner = tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=math.exp(LOG_ALPHA), target_entropy=TARGET_ENTROPY)
    agent = _agent(O, A, B, sizes, activation, M, drop, tuner=tuner, **extras)
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
    if 'bounds' in extras:
        assert ref.bounds == (float(np.float32(0.05)), float(np.float32(0.4)))
    batch = _batch(rng, B, O, A)
    eps, eps_actor = (torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32) for _ in range(2))
    critics, targets = [m.critic_1, m.critic_2], [m.target_critic_1, m.target_critic_2]
    actor = _f64(m.actor)
    online, frozen = [_f64(c) for c in critics], [_f64(c) for c in targets]
    d = {k: v.double() for k, v in batch.items()}
    gpu = {k: v.cuda() for k, v in batch.items()}
    # ---- the critic step
    with torch.no_grad():
        loc, scale = ref.policy(actor, d['next_observations'])
        a, logp = _squashed(loc, scale, eps.double())
        t1, t2 = (ref.critic(p, d['next_observations'], a) for p in frozen)
        _, source = tqc_ref.truncated_targets(t1, t2, d['rewards'], d['discounts'], logp, alpha, drop)
    if 'clip' in extras:
        assert (ref.norm(d['observations']).abs() == 0.8).any()                       # the clip binds
    if 'bounds' in extras:
        raw = torch.nn.functional.softplus(ref._linear(actor, ref._torso(actor, d['observations']), 2 * len(sizes) + 2))
        assert (raw < ref.bounds[0]).any() or (raw > ref.bounds[1]).any()             # so does a bound of the scale
    if B > 1:      # the truncation is not trivial: both critics among the kept and, mostly, among the dropped values
        K = 2 * (M - drop)
        assert all(set(source[r, :K].tolist()) == {0, 1} for r in range(B))
        assert np.mean([len(set(source[r, K:].tolist())) for r in range(B)]) > 1.2
    thetas = [ref.critic(p, d['observations'], d['actions']) for p in online]
    rows = tqc_ref.critic_rows(t1, t2, *thetas, d['rewards'], d['discounts'], logp, alpha, drop)
    rows.mean().backward()
    info = torch.zeros(8, device='cuda')
    critic_u.enqueue(gpu, eps.cuda(), info)
    stats = _stats(critic_u)
    assert stats[5] == B and (stats[[3, 4, 6, 7]] == 0).all(), stats
    got = _grad_sums(critics, critic_u.grad_sums, B)
    leaves = [leaf for p in online for leaf in p]
    worst = _check(got, leaves, [f'critic {i}' for i in range(len(got))], None)
    print(f'{case} {coefficient}: critic tensors {worst:.3e}')
    _check(got, leaves, [f'critic {i}' for i in range(len(got))])
    _check_stat(stats[0] / B, rows.detach().mean(), rows.detach(), 'critic loss')
    for i, theta in enumerate(thetas):
        q = theta.detach().mean(dim=1)
        _check_stat(stats[1 + i] / B, q.mean(), q, f'q{i + 1}')
    # ---- the actor step, through the critics the critic step has just moved
    online = [_f64(c) for c in critics]
    loc, scale = ref.policy(actor, d['observations'])
    a, logp = _squashed(loc, scale, eps_actor.double())
    terms = tqc_ref.actor_rows(*[ref.critic(p, d['observations'], a) for p in online], logp, alpha)
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


# ---------------------------------------------------------------- 3. the agent

def _filled_agent(B, iterations, tuner_kwargs=None, sizes=(32, 32), M=25, O=17, A=6, rows=30, W=4, **updater):
    import tonic_amd.torch as tt
    tuner = tt.updaters.EntropyCoeffTuning(**tuner_kwargs) if tuner_kwargs is not None else None
    agent = _agent(O, A, B, sizes, 'ReLU', M, 2, tuner=tuner, iterations=iterations, seed=7, replay_size=rows * W,
                   **updater)
    rng = np.random.RandomState(321)
    for _ in range(rows - 3):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        row = {k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()}
        agent.replay.store(normalizer=agent.model.observation_normalizer, **row)
    return agent


def _updates(agent, calls, iterations, B, A):
    """`calls` update calls with indices and noise of their own; (what every call left, the graphs seen)."""
    rng = np.random.RandomState(5)
    out, graphs = [], []
    tuner = agent.entropy_coeff_updater
    for _ in range(calls):
        indices = rng.randint(0, agent.replay.size * agent.replay.global_workers, size=(iterations, B)).astype(np.int64)
        eps = rng.normal(size=(iterations, 2, B, A)).astype(np.float32)
        infos = agent.enqueue_update(indices, eps)
        torch.cuda.synchronize()
        out.append([infos.cpu().numpy().copy()] + ([] if tuner is None else [
            agent._u.slot.stats.cpu().numpy().copy(), tuner.log_entropy_coeff.cpu().numpy().copy()]))
        graphs.append(agent._u.slot.graph)
    return out, graphs


@pytest.mark.parametrize('tuned', [False, True])
def test_captured_update_equals_the_host_loop(lib, monkeypatch, tuned):
    B, iterations, A = 33, 2, 6
    fast = dict(initial_entropy_coeff=0.5, optimizer=lambda params: torch.optim.Adam(params, lr=0.05)) if tuned else None
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH', raising=False)
    captured = _filled_agent(B, iterations, fast)
    before = {k: v.clone() for k, v in captured.model.state_dict().items()}
    got, graphs = _updates(captured, 3, iterations, B, A)             # the capture's own update, then two replays
    assert graphs[0] is not None and all(g is graphs[0] for g in graphs), 'the graph was captured again'
    monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    eager = _filled_agent(B, iterations, fast)
    want, none = _updates(eager, 3, iterations, B, A)
    assert all(g is None for g in none)
    for call, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(('infos', 'coefficient rows', 'log_entropy_coeff'), g, w):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (call, name)
    moved = 0
    for key, value in captured.model.state_dict().items():
        assert np.array_equal(bits(value), bits(eager.model.state_dict()[key])), key
        moved += int(not torch.equal(value, before[key]))
    assert moved >= 20                                    # actor, critics and all targets took their steps
    infos = got[-1][0]
    assert np.isfinite(infos).all() and (infos[:, :, 6] == 1.0).all() and (infos[0, :, 0] > 0).all()
    if tuned:
        trajectory = np.concatenate([g[2] for g in got])
        assert len(set(trajectory.tolist())) == 3                     # alpha moved on every call
        assert abs(float(trajectory[-1]) - math.log(0.5)) > 1e-2
    captured.close()
    eager.close()


def test_save_and_load_round_trip(lib, tmp_path):
    B, iterations, A = 33, 1, 6
    fast = dict(initial_entropy_coeff=0.5, optimizer=lambda params: torch.optim.Adam(params, lr=0.05))
    agent = _filled_agent(B, iterations, fast)
    _updates(agent, 2, iterations, B, A)
    path = str(tmp_path / 'agent')
    agent.save(path)
    assert sorted(torch.load(path + '.entropy_coeff.pt')) == ['log_entropy_coeff']
    saved = torch.load(path + '.pt', map_location='cpu')
    assert sorted(saved) == sorted(agent.model.state_dict())
    assert saved['critic_2.head.quantile_layer.weight'].shape == (25, 32)
    fresh = _filled_agent(B, iterations, dict(initial_entropy_coeff=2.0))
    fresh.load(path)
    assert np.array_equal(bits(fresh.entropy_coeff_updater.log_entropy_coeff),
                          bits(agent.entropy_coeff_updater.log_entropy_coeff))
    assert abs(float(agent.entropy_coeff_updater.log_entropy_coeff) - math.log(0.5)) > 1e-2
    for key, value in agent.model.state_dict().items():
        assert np.array_equal(bits(fresh.model.state_dict()[key]), bits(value)), key
    plain = _filled_agent(B, iterations)
    plain.save(str(tmp_path / 'plain'))
    assert os.path.exists(str(tmp_path / 'plain') + '.pt')
    assert not os.path.exists(str(tmp_path / 'plain') + '.entropy_coeff.pt')
    for a in (agent, fresh, plain):
        a.close()


def test_gradient_clip_runs_and_clips(lib):
    B, O, A, M, clip = 33, 17, 6, 25, 1e-3
    rng = np.random.RandomState(3)
    batch = {k: v.cuda() for k, v in _batch(rng, B, O, A).items()}
    eps = torch.as_tensor(rng.normal(size=(2, B, A)), dtype=torch.float32).cuda()
    sums = {}
    for name, value in (('free', 0), ('clipped', clip)):
        agent = _agent(O, A, B, (32, 32), 'ReLU', M, 2, gradient_clip=value)
        _spread_targets(agent)
        info = torch.zeros(8, device='cuda')
        agent.critic_updater.enqueue(batch, eps[0], info)
        agent.actor_updater.enqueue(batch['observations'], eps[1], info)
        torch.cuda.synchronize()
        assert float(info[6]) == 1.0
        sums[name] = [u.grad_sums[:u.count].double().cpu() / B for u in (agent.critic_updater, agent.actor_updater)]
        agent.close()
    # the critic step: the same inputs, so the clipped sums are the free ones scaled down to the norm `clip`
    free, clipped = sums['free'][0], sums['clipped'][0]
    norm = float(free.norm())
    assert norm > 10 * clip
    print(f'critic gradient norm {norm:.3e} -> {float(clipped.norm()):.3e}')
    np.testing.assert_allclose(float(clipped.norm()), clip, rtol=1e-4)
    np.testing.assert_allclose(clipped.numpy(), (free * (clip / norm)).numpy(), rtol=0, atol=1e-5 * clip)
    # the actor step runs behind a differently stepped critic: its norm alone
    assert float(sums['free'][1].norm()) > 10 * clip
    np.testing.assert_allclose(float(sums['clipped'][1].norm()), clip, rtol=1e-4)


def test_two_ranks_equal_single_process(tmp_path):
    """Sharded Buffer + global index / noise streams: two ranks give the update one process holding the union batch
    gives — parameters and log_entropy_coeff (tests/test_gpu_entropy_coeff.py's tolerances)."""
    from test_gpu_multirank import launch
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mp_tqc_worker.py')
    outs = {}
    for world in (1, 2):
        outs[world] = str(tmp_path / f'tqc{world}.npz')
        launch(world, outs[world], 29931 + world, command=(worker,))
    a, b = np.load(outs[1]), np.load(outs[2])
    np.testing.assert_allclose(b['infos'], a['infos'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(b['coeff_infos'], a['coeff_infos'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(b['log_entropy_coeff'], a['log_entropy_coeff'], rtol=0, atol=2e-5)
    assert float(a['log_entropy_coeff'][0]) != float(np.float32(math.log(0.5)))
    for key in a.files:
        if key in ('infos', 'coeff_infos', 'log_entropy_coeff'):
            continue
        diff = np.abs(b[key] - a[key])          # (Adam and float32-noise gradient elements: test_gpu_multirank.py)
        assert diff.max() < 3e-3 and np.mean(diff > 2e-5) < 1e-3, (key, diff.max())
