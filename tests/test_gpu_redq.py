"""GPU tests of REDQ against the float64 restatement tests/redq_ref.py.

1. the subset critic loss kernel alone (tonic_debug_ensemble_subset_loss) on crafted rows: every rule with errors on
   both sides of its knee, rows with discount 0, identical target critics, sentinels behind column 0 and behind row B;
   a lone wave, a ragged workgroup and a general batch; subsets of one, some and all critics, the empty word and bits
   above N.  Bit-identical launches; the coefficient read on the device; non-finite targets inside and outside S.
2. tonic_ensemble_subset_q_grad and tonic_ensemble_quantile_actor_grad at M = 1: gradient sums per tensor and the logged
   statistics against float64 autograd (the conventions and bounds of tests/test_gpu_offpolicy_grads.py), with the float
   coefficient and with a tuner, whose block is checked as well; the workspace query to the byte.
3. the agent: a captured update whose subsets differ per iteration and per call against the host loop of the same
   entries, bit for bit; a replay with other subsets; TONIC_AMD_UPDATE_CHUNK on and off; save / load; the log keys;
   gradient clipping; two ranks against one process.

Every check prints the largest error it saw before it asserts."""
import math
import os

import numpy as np
import pytest

import redq_ref as ref
from test_gpu_offpolicy_grads import _batch, _check, _check_stat, _f64, _set_normalizer, _squashed, _stats
from test_gpu_offpolicy_torsos import ACTIVATIONS, _grad_sums
from test_gpu_tqc import QuantileRef, bits, pad16

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# profiles/redq_accuracy.md: the largest errors of the loss kernel over the cases below, measured on one MI355X, times
# four (the margin of tests/test_gpu_tqc.py, for other inputs' rounding); the cap of 1e-5 does not bind
DQ_BOUND = 4 * 5.775e-08            # max |dq - float64| over a row / the row's largest |d l / d Q|
VALUE_BOUND = 4 * 1.264e-07         # loss_m, q relative to float64
assert DQ_BOUND <= 1e-5 and VALUE_BOUND <= 1e-5
ALPHA = 0.2
LD = 16                             # the entries' pitch of a critic's one output


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


# ---------------------------------------------------------------- 1. the loss kernel alone

LOSS_CASES = [(2, 0b11),            # both of two
              (3, 0b100),           # bit 2 only
              (5, 0b01010),         # two of five
              (8, 0x80),            # bit 7 only
              (8, 0xFF),            # all
              (5, 0),               # no bit: all
              (3, -3)]              # 0xFFFFFFFD: bits 0 and 2, and every bit above N as well
LOSS_BATCHES = (1, 5, 37)
RULES = {'mse': (ref.MSE, 0.0), 'l1': (ref.L1, 0.0), 'smooth_l1': (ref.SMOOTH_L1, 0.5), 'huber': (ref.HUBER, 1.0)}
SPREAD, TIES, RANDOM = 0, 1, 2                                       # row m's kind: m % 3


def crafted_rows(B, N, seed=0):
    """float32 `targets` / `qs` [N, B] and the rows' vectors and kinds.  Values sit around +5 so that q stays away
    from 0 (its error is relative).  A spread row's target critics lie 0.7 apart in an order that turns by one critic
    from one spread row to the next (so every critic is the lowest of any subset somewhere), a tie row's are
    identical, a random row's are anything; the online values lie +-3 around the base: errors of every size and both
    signs, on both sides of the knees at 0.5 and 1."""
    rng = np.random.RandomState(100000 * N + 10 * B + seed)
    base = 5.0 + rng.uniform(-1, 1, size=B)
    kinds = np.arange(B) % 3
    targets = np.empty((N, B))
    for m in range(B):
        targets[:, m] = base[m] + 0.7 * ((np.arange(N) + m // 3) % N)
        if kinds[m] == TIES:
            targets[:, m] = targets[0, m]
        elif kinds[m] == RANDOM:
            targets[:, m] = 5.0 + rng.normal(size=N) * 3
    rows = dict(targets=targets, qs=base[None] + rng.uniform(-3, 3, size=(N, B)),
                rewards=rng.uniform(-1, 1, size=B), discounts=np.where(np.arange(B) % 4 == 3, 0.0, 0.99),
                logp=rng.normal(size=B) * 2 - 1)
    return {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in rows.items()}, kinds


def reference(rows, mask, rule, alpha=ALPHA):
    """((loss_m, [d loss_m / d Q_z], q), the errors e [N, B]) in float64."""
    r = {k: v.double() for k, v in rows.items()}
    N = r['targets'].shape[0]
    members = ref.subset_of(mask, N)
    kind, param = RULES[rule]
    out = ref.critic_rows_with_gradients(list(r['targets']), list(r['qs']), r['rewards'], r['discounts'], r['logp'],
                                         alpha, members, kind, param)
    y = ref.td_target(list(r['targets']), r['rewards'], r['discounts'], r['logp'], alpha, members)
    return out, r['qs'] - y[None]


_loss_reference = {}


def loss_reference(B, N, mask, rule, alpha=ALPHA):
    """The float64 outputs of a case, computed once."""
    key = (B, N, mask, rule, alpha)
    if key not in _loss_reference:
        rows, kinds = crafted_rows(B, N)
        _loss_reference[key] = (rows, kinds) + reference(rows, mask, rule, alpha)
    return _loss_reference[key]


SENTINELS = (777.0, -777.0, float('nan'), 555.0, float('inf'), -1e30, 0.0, 3.0)
UNTOUCHED = 123.0


def launch_loss(lib, rows, mask, rule, alpha=ALPHA, log_alpha=None, ld=LD):
    """(dq [N, B], sample_m [2, B]) of the kernel on `rows`.  What lies behind column 0 and behind row B of the inputs
    is a sentinel of the critic's own, never read; behind column 0 the outputs are exact zeros, and behind row B they
    are what they were."""
    from tonic_amd import _lib
    N, B = rows['targets'].shape
    Bp, p = pad16(B), _lib.ptr

    def padded(x, shift):
        out = torch.empty((N, Bp, ld), dtype=torch.float32)
        for z in range(N):
            out[z] = SENTINELS[(z + shift) % len(SENTINELS)]
        out[:, :B, 0] = x
        return out.cuda()
    targets, qs = padded(rows['targets'], 0), padded(rows['qs'], 2)
    r, disc, logp = rows['rewards'].cuda(), rows['discounts'].cuda(), rows['logp'].cuda()
    word = torch.tensor([mask], dtype=torch.int32).cuda()
    kind, param = RULES[rule]
    loss = _lib.CriticLoss(kind=kind, param=param)
    dq = torch.full((N, Bp, ld), UNTOUCHED, device='cuda')
    sample_m = torch.full((3, Bp), UNTOUCHED, device='cuda')
    import ctypes
    _lib.check(lib.tonic_debug_ensemble_subset_loss(
        p(targets), p(qs), ld, p(r), p(disc), p(logp), N, p(word), float(alpha), p(log_alpha), ctypes.addressof(loss),
        p(dq), p(sample_m), B, Bp, _lib.current_stream()), 'tonic_debug_ensemble_subset_loss')
    torch.cuda.synchronize()
    dq, sample_m = dq.cpu(), sample_m.cpu()
    assert np.array_equal(bits(dq[:, :B, 1:]), np.zeros((N, B, ld - 1), np.int32)), 'a column behind the first is not 0'
    assert (dq[:, B:] == UNTOUCHED).all() and (sample_m[:, B:] == UNTOUCHED).all(), 'a write behind row B'
    assert np.array_equal(bits(sample_m[2, :B]), np.zeros(B, np.int32)), 'the third row of the {loss, q} form is not 0'
    return dq[:, :B, 0].clone(), sample_m[:2, :B].clone()


def loss_errors(got, want):
    """(dq's error in units of the row's largest |d l / d Q|, the values' relative error)."""
    dq, sample_m = got
    loss, grads, q = want
    grads = torch.stack(grads)                                    # [N, B]
    scale = grads.abs().amax(dim=0)
    assert (scale > 0).all()
    gradient = float(((dq.double() - grads).abs().amax(dim=0) / scale).max())
    value = max(float(((sample_m[i].double() - w).abs() / w.abs()).max()) for i, w in enumerate((loss, q)))
    return gradient, value


@pytest.mark.parametrize('B', LOSS_BATCHES)
@pytest.mark.parametrize('N,mask', LOSS_CASES)
def test_loss_kernel_vs_float64_on_crafted_rows(lib, N, mask, B):
    members = ref.subset_of(mask, N)
    for rule, (kind, param) in RULES.items():
        rows, kinds, want, e = loss_reference(B, N, mask, rule)
        if B >= 5:                                                # what the rows were crafted for, on the reference
            assert (kinds == TIES).any() and (kinds == RANDOM).any() and (rows['discounts'] == 0).any()
            for m in np.flatnonzero(kinds == TIES):
                assert (rows['targets'][:, m] == rows['targets'][0, m]).all()
            knee = param if param else 1.0
            assert (e.abs() < knee).any() and (e > knee).any() and (e < -knee).any()
        if B == 37:
            spread = torch.as_tensor(kinds == SPREAD)
            _, who = ref.subset_min(list(rows['targets'].double()), members)
            assert set(who[spread].tolist()) == set(members)      # every member of S is the minimum somewhere
            if len(members) < N:                                  # ... and somewhere a critic outside S lies below it
                low = rows['targets'][members].amin(dim=0)
                assert (rows['targets'].amin(dim=0) < low).any()
        got = launch_loss(lib, rows, mask, rule)
        gradient, value = loss_errors(got, want)
        print(f'N={N} mask={mask} B={B} {rule}: dq {gradient:.3e} of the row\'s largest slope, values {value:.3e} '
              'relative')
        again = launch_loss(lib, rows, mask, rule)
        for a, b in zip(got, again):
            assert np.array_equal(bits(a), bits(b)), 'two launches on the same inputs differ'
        assert gradient <= DQ_BOUND and value <= VALUE_BOUND, (rule, gradient, value)


def test_loss_kernel_words_that_name_the_same_subset(lib):
    """Bits at and above N are ignored and the empty word is the full one: the same bits out."""
    rows, _ = crafted_rows(37, 5)
    for same in ((0b01010, 0b01010 | 0x20, 0b01010 | -32), (0, 0b11111, -1, 0x7FFFFFE0)):
        outs = [launch_loss(lib, rows, mask, 'huber') for mask in same]
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert np.array_equal(bits(a), bits(b)), same
    # ... and two different subsets give different targets
    a, b = launch_loss(lib, rows, 0b01010, 'mse'), launch_loss(lib, rows, 0b00101, 'mse')
    assert not np.array_equal(bits(a[0]), bits(b[0]))
    # the pitch does not matter
    narrow, wide = launch_loss(lib, rows, 0b01010, 'mse', ld=1), launch_loss(lib, rows, 0b01010, 'mse', ld=32)
    for x, y, z in zip(a, narrow, wide):
        assert np.array_equal(bits(x), bits(y)) and np.array_equal(bits(x), bits(z))


def test_loss_kernel_reads_the_coefficient_on_the_device(lib):
    B, N, mask = 5, 5, 0b01010
    log_alpha = torch.tensor([math.log(0.35)], dtype=torch.float32)
    rows, _, want, _ = loss_reference(B, N, mask, 'mse', alpha=math.exp(float(log_alpha.double())))
    got = launch_loss(lib, rows, mask, 'mse', alpha=123.0, log_alpha=log_alpha.cuda())    # (the float is then unused)
    gradient, value = loss_errors(got, want)
    print(f'device coefficient: dq {gradient:.3e}, values {value:.3e}')
    assert gradient <= DQ_BOUND and value <= VALUE_BOUND, (gradient, value)
    plain = launch_loss(lib, rows, mask, 'mse')
    assert not np.array_equal(bits(plain[0]), bits(got[0]))


@pytest.mark.parametrize('rule', RULES)
def test_loss_kernel_on_non_finite_targets(lib, rule):
    """Inside S a NaN makes the row's loss NaN whatever the other members hold (torch.min; fminf would drop it), +inf
    is the reference's value; outside S neither is read: the row is bit-equal to the clean one."""
    nan, inf = float('nan'), float('inf')
    N, mask, B = 5, 0b01010, 8                                   # S = {1, 3}
    rows, _ = crafted_rows(B, N)
    rows['discounts'] = torch.full((B,), 0.99)
    clean = launch_loss(lib, rows, mask, rule)
    dirty = dict(rows, targets=rows['targets'].clone())
    t = dirty['targets']
    t[1, 0] = nan                        # row 0: a NaN in the FIRST member, a finite second
    t[3, 1] = nan                        # row 1: a finite first, a NaN in the LAST
    t[1, 2], t[3, 2] = nan, inf          # row 2: NaN and +inf
    t[3, 3] = inf                        # row 3: one +inf, the other member finite: the finite one
    t[1, 4] = t[3, 4] = inf              # row 4: all of S +inf
    t[0, 5], t[2, 5], t[4, 5] = nan, inf, -inf                   # row 5: only outside S
    t[1, 6] = -inf                       # row 6: -inf inside S
    dq, sample_m = launch_loss(lib, dirty, mask, rule)
    (loss, grads, q), _ = reference(dirty, mask, rule)
    loss32, grads32 = loss.float(), torch.stack(grads).float()
    for m in (0, 1, 2):
        assert torch.isnan(sample_m[0, m]) and torch.isnan(loss[m]), (m, sample_m[0, m])
    for m in (4, 6):                     # the reference's value: +-inf, or a NaN where the reference has one
        assert np.array_equal(sample_m[0, m].numpy(), loss32[m].numpy(), equal_nan=True), (m, sample_m[0, m], loss32[m])
        assert np.array_equal(dq[:, m].numpy(), grads32[:, m].numpy(), equal_nan=True), (m, dq[:, m], grads32[:, m])
    assert torch.isfinite(loss[3]) and torch.isfinite(sample_m[0, 3])
    assert abs(float(sample_m[0, 3]) - float(loss[3])) <= VALUE_BOUND * float(loss[3])
    for m in (5, 7):                     # untouched
        assert np.array_equal(bits(dq[:, m]), bits(clean[0][:, m])), m
        assert np.array_equal(bits(sample_m[:, m]), bits(clean[1][:, m])), m
    assert np.array_equal(bits(sample_m[1]), bits(clean[1][1]))          # q reads no target


# ---------------------------------------------------------------- 2. the entries against float64 autograd

class EnsembleRef(QuantileRef):
    """tests/test_gpu_tqc.py's float64 networks with a critic of one output, squeezed."""

    def critic(self, params, obs, act):
        return super().critic(params, obs, act).squeeze(-1)


def _model(tt, sizes, activation, N):
    act = ACTIVATIONS[activation]
    head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                        distribution=tt.models.SquashedMultivariateNormalDiag)
    return tt.models.ActorCriticEnsembleWithTargets(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=tt.models.ValueHead()),
        num_critics=N, observation_normalizer=tt.normalizers.MeanStd())


def _agent(O, A, B, sizes, activation, N, subset_size, tuner=None, iterations=1, seed=9, replay_size=1000, loss=None,
           **updater):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    agent = tt.agents.REDQ(
        model=_model(tt, sizes, activation, N),
        replay=tonic_amd.replays.Buffer(size=replay_size, batch_iterations=iterations, batch_size=B, steps_before_batches=0,
                                        steps_between_batches=1),
        critic_updater=tt.updaters.EnsembleSoftQLearning(loss=loss, subset_size=subset_size, **updater),
        actor_updater=tt.updaters.EnsembleSoftPolicyGradient(**updater), entropy_coeff_updater=tuner)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=seed)
    assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
    assert agent._u.route().fused_kind is None
    assert agent.model.flat_critics.count % N == 0 and agent.critic_updater.count == agent.model.flat_critics.count
    return agent


def _spread_targets(agent, gain=8.0, seed=0):
    """The N target critics away from the online ones and from each other, so that which of them are in S matters."""
    from tonic_amd.torch.models import network_variables
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for critic in agent.model.critics(target=True):
            for p in network_variables(critic):
                p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.1, dtype=torch.float32, device=p.device)
            critic.head.v_layer.weight.mul_(gain)
            critic.head.v_layer.bias.add_(torch.as_tensor(rng.normal(size=1), dtype=torch.float32, device=p.device))


ENTRY_CASES = {
    # name: (sizes, activation, B, N, subset_size, loss, O, A)
    'five_two': ((32, 32), 'ReLU', 33, 5, 2, None, 17, 6),
    'tanh_layers_one': ((48, 32), 'Tanh', 5, 3, 1, None, 17, 6),
    'two_two_huber': ((32, 32), 'ReLU', 33, 2, 2, ('huber', 1.0), 17, 6),
}
LOG_ALPHA = math.log(0.35)
TARGET_ENTROPY = -2.5


def _telling_subset(pool, N, size):
    """The first subset of `size` critics, in itertools' order, each member of which holds the minimum over the
    subset in some row and whose minimum differs from the minimum over all N in some row (size < N) — a kernel that
    ignores the mask, or reads one member only, cannot pass on it."""
    import itertools
    lowest = torch.stack(pool).amin(dim=0)
    for members in itertools.combinations(range(N), size):
        low, who = ref.subset_min(pool, list(members))
        if set(who.tolist()) == set(members) and (size == N or bool((low != lowest).any())):
            return list(members)
    raise AssertionError('no subset tells: spread the target critics further')


@pytest.mark.parametrize('coefficient', ['float', 'device'])
@pytest.mark.parametrize('case', ENTRY_CASES)
def test_entries_vs_float64_autograd(lib, case, coefficient):
    import tonic_amd.torch as tt
    sizes, activation, B, N, size, loss, O, A = ENTRY_CASES[case]
    tuner = None
    if coefficient == 'device':
        tuner = tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=math.exp(LOG_ALPHA), target_entropy=TARGET_ENTROPY)
    module = torch.nn.HuberLoss(delta=loss[1]) if loss else None
    kind, param = RULES[loss[0]] if loss else (ref.MSE, 0.0)
    agent = _agent(O, A, B, sizes, activation, N, size, tuner=tuner, loss=module)
    rng = np.random.RandomState(B + N)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, 0.5 + rng.uniform(size=O))
    _spread_targets(agent, seed=3)            # (a seed under which the target critics cross in all three cases)
    m, critic_u, actor_u = agent.model, agent.critic_updater, agent.actor_updater
    alpha = ALPHA
    if tuner is not None:
        assert critic_u.entropy_coeff_updater is tuner and actor_u.entropy_coeff_updater is tuner
        alpha = math.exp(float(tuner.log_entropy_coeff.double()))
        critic_u.entropy_coeff = actor_u.entropy_coeff = 77.0            # (unused with a tuner)
    net = EnsembleRef(agent, len(sizes), activation)
    batch = _batch(rng, B, O, A)
    eps, eps_actor = (torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32) for _ in range(2))
    critics, targets = m.critics(), m.critics(target=True)
    assert len(critics) == len(targets) == N
    actor = _f64(m.actor)
    online, frozen = [_f64(c) for c in critics], [_f64(c) for c in targets]
    d = {k: v.double() for k, v in batch.items()}
    gpu = {k: v.cuda() for k, v in batch.items()}
    # ---- the critic step
    with torch.no_grad():
        loc, scale = net.policy(actor, d['next_observations'])
        a, logp = _squashed(loc, scale, eps.double())
        pool = [net.critic(p, d['next_observations'], a) for p in frozen]
    members = _telling_subset(pool, N, size)
    # asserted on the reference alone: each member of S is the arg-min in some row, and in some row the minimum over S
    # is not the minimum over all N
    low, who = ref.subset_min(pool, members)
    assert set(who.tolist()) == set(members)
    if size < N:
        assert bool((low != torch.stack(pool).amin(dim=0)).any())
    word = torch.tensor([ref.mask_of(members) | (0x40 << N)], dtype=torch.int32).cuda()     # (and a bit above N)
    qs = [net.critic(p, d['observations'], d['actions']) for p in online]
    rows = ref.critic_rows(pool, qs, d['rewards'], d['discounts'], logp, alpha, members, kind, param)
    rows.mean().backward()
    info = torch.zeros(8, device='cuda')
    critic_u.enqueue(gpu, eps.cuda(), info, subset=word)
    stats = _stats(critic_u)
    assert stats[5] == B and (stats[[2, 3, 4, 6, 7]] == 0).all(), stats
    got = _grad_sums(critics, critic_u.grad_sums, B)
    leaves = [leaf for p in online for leaf in p]
    per = 2 * len(sizes) + 2
    assert len(got) == len(leaves) == N * per
    names = [f'critic {i // per + 1} tensor {i % per}' for i in range(len(got))]
    worst = _check(got, leaves, names, None)
    print(f'{case} {coefficient}: S = {members}, critic tensors {worst:.3e}')
    _check(got, leaves, names)
    _check_stat(stats[0] / B, rows.detach().mean(), rows.detach(), 'critic loss')
    q = torch.stack([v.detach() for v in qs]).mean(dim=0)
    _check_stat(stats[1] / B, q.mean(), q, 'q')
    # ---- the actor step, through the critics the critic step has just moved
    online = [_f64(c) for c in critics]
    loc, scale = net.policy(actor, d['observations'])
    a, logp = _squashed(loc, scale, eps_actor.double())
    terms = ref.actor_rows([net.critic(p, d['observations'], a) for p in online], logp, alpha)
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
    """Both steps run in a workspace of exactly the query's bytes and write nothing behind it; with one byte less they
    return the workspace error and write nothing at all."""
    B, O, A, N = 33, 17, 6, 5
    agent = _agent(O, A, B, (32, 32), 'ReLU', N, 2)
    _spread_targets(agent)
    critic_u, actor_u = agent.critic_updater, agent.actor_updater
    need = lib.tonic_ensemble_q_workspace_bytes(B, O, A, critic_u.hidden, N)
    assert need == critic_u._workspace_bytes(B) == actor_u._workspace_bytes(B) and need % 256 == 0
    assert need == lib.tonic_ensemble_quantile_workspace_bytes(B, O, A, critic_u.hidden, 1, N)
    rng = np.random.RandomState(1)
    batch = {k: v.cuda() for k, v in _batch(rng, B, O, A).items()}
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32).cuda()
    word = torch.tensor([0b00110], dtype=torch.int32).cuda()
    info = torch.zeros(8, device='cuda')
    guard = 4096
    steps = ((critic_u, lambda: critic_u.enqueue(batch, eps, info, subset=word)),
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
    agent.close()


# ---------------------------------------------------------------- 3. the agent

N_AGENT, SIZE_AGENT = 3, 2
PAIRS = (0b011, 0b101, 0b110)


def _filled_agent(B, iterations, tuner_kwargs=None, sizes=(32, 32), O=17, A=6, rows=30, W=4, size=SIZE_AGENT, **updater):
    import tonic_amd.torch as tt
    tuner = tt.updaters.EntropyCoeffTuning(**tuner_kwargs) if tuner_kwargs is not None else None
    agent = _agent(O, A, B, sizes, 'ReLU', N_AGENT, size, tuner=tuner, iterations=iterations, seed=7,
                   replay_size=rows * W, **updater)
    _spread_targets(agent, gain=2.0)
    rng = np.random.RandomState(321)
    for _ in range(rows - 3):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        row = {k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()}
        agent.replay.store(normalizer=agent.model.observation_normalizer, **row)
    return agent


def _subsets(call, iterations, shift=0):
    """Explicit masks that differ per iteration and per call."""
    return np.array([PAIRS[(call + it + shift) % 3] for it in range(iterations)], np.int64)


def _updates(agent, calls, iterations, B, A, shift=lambda call: 0):
    """`calls` update calls with indices, noise and subsets of their own; (what every call left, the graphs seen)."""
    rng = np.random.RandomState(5)
    out, graphs = [], []
    tuner = agent.entropy_coeff_updater
    for call in range(calls):
        indices = rng.randint(0, agent.replay.size * agent.replay.global_workers, size=(iterations, B)).astype(np.int64)
        eps = rng.normal(size=(iterations, 2, B, A)).astype(np.float32)
        subsets = _subsets(call, iterations, shift(call))
        infos = agent.enqueue_update(indices, eps, subsets=subsets)
        torch.cuda.synchronize()
        assert np.array_equal(agent._u.slot.subsets.cpu().numpy(), subsets.astype(np.int32))
        out.append([infos.cpu().numpy().copy()] + ([] if tuner is None else [
            agent._u.slot.stats.cpu().numpy().copy(), tuner.log_entropy_coeff.cpu().numpy().copy()]))
        graphs.append(agent._u.slot.graph)
    return out, graphs


@pytest.mark.parametrize('tuned', [False, True])
def test_captured_update_equals_the_host_loop(lib, monkeypatch, tuned):
    B, iterations, A = 33, 3, 6
    fast = dict(initial_entropy_coeff=0.5, optimizer=lambda params: torch.optim.Adam(params, lr=0.05)) if tuned else None
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH', raising=False)
    captured = _filled_agent(B, iterations, fast)
    before = {k: v.clone() for k, v in captured.model.state_dict().items()}
    got, graphs = _updates(captured, 3, iterations, B, A)             # the capture's own update, then two replays
    assert graphs[0] is not None and all(g is graphs[0] for g in graphs), 'the graph was captured again'
    assert len(set(_subsets(0, iterations).tolist())) == 3 and not np.array_equal(_subsets(0, 3), _subsets(1, 3))
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
    assert moved >= 8 + 12 * N_AGENT                      # actor, every critic and all targets took their steps
    infos = got[-1][0]
    assert np.isfinite(infos).all() and (infos[:, :, 6] == 1.0).all() and (infos[0, :, 0] > 0).all()
    assert (infos[0, :, 2] == 0).all() and (infos[0, :, 1] != 0).all()       # the ensemble's row: loss, q, nothing
    if tuned:
        trajectory = np.concatenate([g[2] for g in got])
        assert len(set(trajectory.tolist())) == 3                     # alpha moved on every call
    # the same graph replayed with OTHER subsets on its second call: the same first call, another second
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH')
    other = _filled_agent(B, iterations, fast)
    others, graphs = _updates(other, 2, iterations, B, A, shift=lambda call: call)
    assert graphs[0] is not None and graphs[1] is graphs[0]
    assert np.array_equal(others[0][0].view(np.int32), got[0][0].view(np.int32))
    assert not np.array_equal(others[1][0][0, :, 0], got[1][0][0, :, 0]), 'the replay did not follow its subsets'
    for agent in (captured, eager, other):
        agent.close()


def test_chunk_setting_does_not_move_an_update(lib, monkeypatch):
    """agent._update with the subsets drawn: TONIC_AMD_UPDATE_CHUNK=10 and =0 leave the same bits (the split route
    keeps one graph per call either way), and the words in the Slot are the agent's own seeded stream."""
    import tonic_amd.torch as tt
    B, iterations = 16, 20
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH', raising=False)
    states, infos = [], []
    for chunk in ('10', '0'):
        monkeypatch.setenv('TONIC_AMD_UPDATE_CHUNK', chunk)
        agent = _filled_agent(B, iterations, sizes=(16, 16))
        torch.manual_seed(11)                                       # (the noise stream of this update)
        agent._update(steps=100)
        torch.cuda.synchronize()
        drawn = agent._u.slots[0].subsets.cpu().numpy()
        stream = np.random.RandomState((7 + tt.agents.REDQ.SUBSET_STREAM) % 2 ** 32)
        assert np.array_equal(drawn, tt.updaters.draw_subset_masks(stream, iterations, N_AGENT, SIZE_AGENT))
        assert len(set(drawn.tolist())) == 3 and set(drawn.tolist()) <= set(PAIRS)
        states.append({k: v.clone() for k, v in agent.model.state_dict().items()})
        infos.append(np.array(agent.last_infos))
        agent.close()
    assert np.array_equal(infos[0].view(np.int32), infos[1].view(np.int32))
    for key, value in states[0].items():
        assert np.array_equal(bits(value), bits(states[1][key])), key


def test_save_load_and_log_keys(lib, tmp_path, monkeypatch):
    import tonic_amd.torch as tt
    B, iterations, A = 33, 1, 6
    fast = dict(initial_entropy_coeff=0.5, optimizer=lambda params: torch.optim.Adam(params, lr=0.05))
    agent = _filled_agent(B, iterations, fast)
    out, _ = _updates(agent, 2, iterations, B, A)
    stored = []
    monkeypatch.setattr(tt.agents.logger, 'store', lambda key, value, **kwargs: stored.append(key))
    agent._log_update(out[-1][0], out[-1][1])
    keys = set(stored)
    assert {'critic/loss', 'critic/q', 'actor/loss', 'entropy_coeff/value', 'entropy_coeff/loss'} <= keys, keys
    assert not keys & {'critic/q1', 'critic/q2'}, keys
    # the updater's drop-in call names the same row
    batch = {k: v.cuda() for k, v in _batch(np.random.RandomState(0), B, 17, A).items()}
    row = agent.critic_updater(**batch)
    assert sorted(row) == ['loss', 'q'] and all(np.isfinite(float(v)) for v in row.values())
    assert bin(int(agent.critic_updater._subset[0])).count('1') == SIZE_AGENT
    path = str(tmp_path / 'agent')
    agent.save(path)
    assert sorted(torch.load(path + '.entropy_coeff.pt')) == ['log_entropy_coeff']
    saved = torch.load(path + '.pt', map_location='cpu')
    assert sorted(saved) == sorted(agent.model.state_dict())
    assert saved[f'critic_{N_AGENT}.head.v_layer.weight'].shape == (1, 32)
    assert f'target_critic_{N_AGENT}.head.v_layer.bias' in saved and f'critic_{N_AGENT + 1}.head' not in str(sorted(saved))
    fresh = _filled_agent(B, iterations, dict(initial_entropy_coeff=2.0))
    assert any(not torch.equal(v, agent.model.state_dict()[k]) for k, v in fresh.model.state_dict().items())
    fresh.load(path)
    assert np.array_equal(bits(fresh.entropy_coeff_updater.log_entropy_coeff),
                          bits(agent.entropy_coeff_updater.log_entropy_coeff))
    for key, value in agent.model.state_dict().items():
        assert np.array_equal(bits(fresh.model.state_dict()[key]), bits(value)), key
    # the loaded agent goes on as the saved one does
    a, _ = _updates(agent, 1, iterations, B, A)
    b, _ = _updates(fresh, 1, iterations, B, A)
    assert np.array_equal(a[0][0].view(np.int32)[0], b[0][0].view(np.int32)[0])        # the critic step's row
    plain = _filled_agent(B, iterations)
    plain.save(str(tmp_path / 'plain'))
    assert os.path.exists(str(tmp_path / 'plain') + '.pt')
    assert not os.path.exists(str(tmp_path / 'plain') + '.entropy_coeff.pt')
    for each in (agent, fresh, plain):
        each.close()


def test_gradient_clip_runs_and_clips(lib):
    B, O, A, clip = 33, 17, 6, 1e-3
    rng = np.random.RandomState(3)
    batch = {k: v.cuda() for k, v in _batch(rng, B, O, A).items()}
    eps = torch.as_tensor(rng.normal(size=(2, B, A)), dtype=torch.float32).cuda()
    word = torch.tensor([0b101], dtype=torch.int32).cuda()
    sums = {}
    for name, value in (('free', 0), ('clipped', clip)):
        agent = _agent(O, A, B, (32, 32), 'ReLU', N_AGENT, SIZE_AGENT, gradient_clip=value)
        _spread_targets(agent)
        info = torch.zeros(8, device='cuda')
        agent.critic_updater.enqueue(batch, eps[0], info, subset=word)
        agent.actor_updater.enqueue(batch['observations'], eps[1], info)
        torch.cuda.synchronize()
        assert float(info[6]) == 1.0
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


def test_two_ranks_equal_single_process(tmp_path):
    """Sharded Buffer + global index / noise / subset streams: two ranks of B / 2 give the update one process holding
    the union batch gives (the bounds of tests/test_gpu_tqc.py's two-rank test), and hold the same masks."""
    from test_gpu_multirank import launch
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mp_redq_worker.py')
    outs = {}
    for world in (1, 2):
        outs[world] = str(tmp_path / f'redq{world}.npz')
        launch(world, outs[world], 29941 + world, command=(worker,))
    a, b = np.load(outs[1]), np.load(outs[2])
    alone = np.load(outs[1] + '.masks0.npy')
    first, second = np.load(outs[2] + '.masks0.npy'), np.load(outs[2] + '.masks1.npy')
    assert alone.shape == (4,) and np.array_equal(first, second) and np.array_equal(first, alone)
    assert all(bin(int(mask)).count('1') == 2 and 0 < mask < 32 for mask in alone)
    np.testing.assert_allclose(b['infos'], a['infos'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(b['coeff_infos'], a['coeff_infos'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(b['log_entropy_coeff'], a['log_entropy_coeff'], rtol=0, atol=2e-5)
    assert float(a['log_entropy_coeff'][0]) != float(np.float32(math.log(0.5)))
    for key in a.files:
        if key in ('infos', 'coeff_infos', 'log_entropy_coeff', 'masks'):
            continue
        diff = np.abs(b[key] - a[key])          # (Adam and float32-noise gradient elements: test_gpu_multirank.py)
        assert diff.max() < 3e-3 and np.mean(diff > 2e-5) < 1e-3, (key, diff.max())
