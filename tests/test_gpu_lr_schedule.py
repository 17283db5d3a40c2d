"""tonic_scheduled_optimizer_step / tonic_scheduled_adam_step_pair (csrc/optim.hip: scheduled_optimizer_kernel) through
the C ABI: the rate a launch reads from the device's own step count, bit for bit against the `math` restatement
(tests/lr_schedule_ref.py), and every rule of the optimizer family at that rate against its float32 statement
(tests/optim_family_ref.py with `lr` replaced by lr_t), bit for bit.

| case                                         | decided by                                                             |
|----------------------------------------------|------------------------------------------------------------------------|
| plain SGD, p = 0, sums = 1, grad_scale = 1   | p = -F32(lr_t): the rate itself, read back                             |
| state[0] = 0, 1, period -1 / +0 / +1,        | the segments' `min`, `>=`, `//` and the milestone's `>=`; 10^6: the    |
| 2 period + 3, m - 1, m, m + 1, 10^6          | int64 step count far beyond every period                               |
| n = 1, 1031                                  | one thread of one workgroup; five workgroups, the last ragged          |
| every rule x {linear, cosine}, 7 steps from  | where lr stands in each rule: step_size, AdamW's decay, SGD / RMSprop  |
| state[0] = 0 and period - 3, n = 1031        | the rate's own kink (linear's cap, cosine's turn) inside the 7 steps   |
| polynomial past total_iters                  | lr_t = 0: parameters keep their bits, the moments move                 |
| schedule = NULL                              | the unscheduled entries' launches and bits                             |
| pair (1031, 70), one schedule NULL; skip     | each network on its own counter; a skipped launch does not advance it |
| flag, all-zero advantages, KL stop           |                                                                        |
| polyak: block of 1031 at 1031 in 2 * 1031 + 5| the targets outside and inside the block as in the unscheduled launch  |

Bit comparisons use safe steps only (lr_schedule_ref.safe_rate: by the reference alone, a base rate at which no step's
float32 constant depends on the last bits of lr_t; no step is dropped).  Every buffer lies between sentinel margins
(test_gpu_optim.Guarded)."""
import ctypes

import numpy as np
import pytest

import lr_schedule_ref as sref
import numpy_port as port
import optim_family_ref as ref
from test_gpu_optim import F32, NAN, STATE_MARK, STATS, Guarded, Net, bits, expected_row, same_bits
from test_gpu_optim_family import FamilyNet, check, rule_of, start_slots
from test_oracle_golden import ADAM_GRAD_SCALE as GRAD_SCALE
from test_oracle_golden import adam_case

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

N = 1031


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


def by_reference(packed):
    return ctypes.byref(packed) if packed is not None else None


def scheduled_step(lib, net, packed, grad_scale=GRAD_SCALE, kind=0, skip=None, adv_stats=None, kl_threshold=0.0,
                   polyak=(None, None, 0, 0, 0.0), params=None):
    from tonic_amd import _lib
    _lib.check(lib.tonic_scheduled_optimizer_step(
        params if params is not None else net.p.ptr(), net.sums.ptr(),
        net.slots.ptr() if net.slots is not None else None, net.state.ptr(), net.n, grad_scale,
        ctypes.byref(net.packed), kind, kl_threshold, 0.0, adv_stats,
        net.info.ptr() if net.info is not None else None, skip, *polyak, by_reference(packed), None),
        'tonic_scheduled_optimizer_step')


def derived(rule, step_of=None):
    """(lr_t, t) -> the float32 constants `rule` rounds from lr_t when t steps have been taken."""
    def constants(lr_t, t):
        if rule['kind'] in ('adam', 'adamw'):
            out = [F32(lr_t / (1.0 - rule['betas'][0] ** (t + 1)))]
            if rule['kind'] == 'adamw':
                out.append(F32(1.0 - lr_t * rule['weight_decay']))
            return out
        return [F32(lr_t)]
    return constants


# ------------------------------------------------------------------------------------------------ reading the rate

@pytest.mark.parametrize('n', [1, N])
@pytest.mark.parametrize('name', list(sref.SCHEDULES))
def test_the_rate_read_back(lib, name, n):
    """Plain SGD from p = 0 with gradient sums of 1 and grad_scale 1 leaves p = -F32(lr_t), at every edge step."""
    schedule, steps = sref.SCHEDULES[name][1], sref.edge_steps(name)
    rule = dict(kind='sgd', lr=0.0, weight_decay=0.0, maximize=False, momentum=0.0, dampening=0.0, nesterov=False)
    rule['lr'] = sref.safe_rate(schedule, steps, derived(rule))
    packed = sref.pack(schedule)
    for t in steps:
        net = FamilyNet(rule, np.zeros(n, F32), [], step=t, info=False)
        net.load(np.ones(n, F32))
        scheduled_step(lib, net, packed, grad_scale=1.0)
        got, _, state, _ = net.read()
        lr_t = sref.value(schedule, rule['lr'], t)
        want = np.full(n, -F32(lr_t), F32) + F32(0)            # (-0.0 + 0: p - lr_t * g with lr_t = 0 is +0)
        assert same_bits(got, want), (name, n, t, got[0], -F32(lr_t))
        assert state.tolist() == [t + 1, 0, STATE_MARK, 0], state
        host = lib.tonic_lr_schedule_value(ctypes.byref(packed), rule['lr'], t)
        assert F32(host) == F32(lr_t)


# ------------------------------------------------------------------------------------------------ every rule

@pytest.mark.parametrize('early', [True, False], ids=['from-zero', 'from-period-3'])
@pytest.mark.parametrize('schedule_name', ['linear', 'cosine'])
@pytest.mark.parametrize('name', list(ref.CONFIGURATIONS))
def test_every_rule_at_the_scheduled_rate(lib, name, schedule_name, early):
    """Seven consecutive steps: parameters and every state buffer equal `family_statement` with lr = lr_t bit for bit
    after each launch; the state words are those of the unscheduled step."""
    _, schedule, period = sref.SCHEDULES[schedule_name]
    start = 0 if early else period - 3
    steps = list(range(start, start + 7))
    rule = rule_of(name)
    rule['lr'] = sref.safe_rate(schedule, steps, derived(rule), rates=(rule['lr'],) + sref.BASE_RATES)
    p, _, _, sums = adam_case(N, 7, 41)
    slots = start_slots(rule, N, start, 41)
    net = FamilyNet(rule, p, slots, step=start, info=False)
    packed = sref.pack(schedule)
    want_p, want_slots = p, slots
    rates = []
    for k, t in enumerate(steps):
        net.load(sums[k])
        scheduled_step(lib, net, packed)
        lr_t = sref.value(schedule, rule['lr'], t)
        rates.append(lr_t)
        want_p, want_slots = ref.family_statement(dict(rule, lr=lr_t), want_p, sums[k], want_slots, t + 1, GRAD_SCALE)
        got_p, got_slots, state, _ = net.read()
        check(f'{name} under {schedule_name}, step {t + 1}', rule, got_p, got_slots, want_p, want_slots)
        assert state.tolist() == [t + 1, 0, STATE_MARK, 0], state
    assert len(set(rates)) >= 4 and not same_bits(want_p, p)


def test_polynomial_past_its_end_is_a_zero_rate(lib):
    """lr_t = 0: the parameters keep their bits while the moments move."""
    _, schedule, period = sref.SCHEDULES['polynomial']
    rule = dict(rule_of('adam-maximize'), maximize=False)
    p, m, v, sums = adam_case(N, 1, 42, warm=True)
    net = FamilyNet(rule, p, [m, v], step=period + 2, info=False)
    net.load(sums[0])
    scheduled_step(lib, net, sref.pack(schedule))
    got_p, (got_m, got_v), state, _ = net.read()
    assert sref.value(schedule, rule['lr'], period + 2) == 0.0
    assert same_bits(got_p, p) and state.tolist() == [period + 3, 0, STATE_MARK, 0]
    _, want_m, want_v = port.adam_statement(p, sums[0], m, v, period + 3, GRAD_SCALE, 0.0)
    assert same_bits(got_m, want_m) and same_bits(got_v, want_v) and not same_bits(got_m, m)


# ------------------------------------------------------------------------------------------------ NULL schedules

@pytest.mark.parametrize('name', ['adamw', 'sgd-nesterov', 'rmsprop-centered-momentum'])
def test_a_null_schedule_is_the_unscheduled_step(lib, name):
    rule = rule_of(name)
    p, _, _, sums = adam_case(N, 2, 43)
    nets = [FamilyNet(rule, p, start_slots(rule, N, 5, 43), step=5) for _ in range(2)]
    for k in range(2):
        for net in nets:
            net.load(sums[k])
        nets[0].step(lib, kind=2)
        scheduled_step(lib, nets[1], None, kind=2)
    (p0, s0, st0, i0), (p1, s1, st1, i1) = nets[0].read(), nets[1].read()
    assert same_bits(p0, p1) and all(same_bits(a, b) for a, b in zip(s0, s1))
    assert st0.tolist() == st1.tolist() == [7, 0, STATE_MARK, 0] and same_bits(i0, i1)


def pair_step(lib, actor, critic, schedules, entry='tonic_scheduled_adam_step_pair', kl_threshold=0.0, adv_stats=None,
              skip=None, lrs=(3e-4, 1e-3)):
    from tonic_amd import _lib
    tail = () if schedules is None else tuple(by_reference(s) for s in schedules)
    _lib.check(getattr(lib, entry)(
        actor.p.ptr(), actor.sums.ptr(), actor.m.ptr(), actor.v.ptr(), actor.state.ptr(), actor.n, lrs[0], 1,
        kl_threshold, 0.0, adv_stats, actor.info.ptr(), skip,
        critic.p.ptr(), critic.sums.ptr(), critic.m.ptr(), critic.v.ptr(), critic.state.ptr(), critic.n, lrs[1], 2,
        critic.info.ptr(), GRAD_SCALE, 0.9, 0.999, 1e-8, *tail, None), entry)


def pair_nets(steps=(0, 0), seed=44):
    nets = []
    for n, step, s in ((N, steps[0], seed), (70, steps[1], seed + 1)):
        p, m, v, sums = adam_case(n, 4, s, warm=True)
        nets.append((Net(p, m, v, step=step), (p, m, v), sums))
    return nets


def test_a_null_pair_is_the_unscheduled_pair(lib):
    results = []
    for schedules in (None, (None, None)):
        (actor, _, sums_a), (critic, _, sums_c) = pair_nets(steps=(3, 8))
        actor.load(sums_a[0]), critic.load(sums_c[0])
        pair_step(lib, actor, critic, schedules,
                  entry='tonic_adam_step_pair' if schedules is None else 'tonic_scheduled_adam_step_pair',
                  kl_threshold=1e9)
        results.append(actor.read() + critic.read())
    for a, b in zip(*results):
        assert same_bits(a, b)
    assert results[0][3].tolist() == [4, 0, STATE_MARK, 0] and results[0][8].tolist() == [9, 0, STATE_MARK, 0]


# ------------------------------------------------------------------------------------------------ skip and stop

def adam_at(rule_lr, schedule, before, sums, t):
    """The Adam statement of the step taken after t steps at the schedule's rate (None: the base rate)."""
    return port.adam_statement(before[0], sums, before[1], before[2], t + 1, GRAD_SCALE,
                               sref.value(schedule, rule_lr, t))


@pytest.mark.parametrize('scheduled', ['actor', 'critic'])
def test_the_pair_counts_each_network_on_its_own_and_skips_do_not_advance(lib, scheduled):
    """Four launches of the pair at n = (1031, 70), one schedule NULL: a plain step; a launch whose KL is above the
    threshold (the step is taken, the stop flag rises); a launch behind the raised flag (skip = &state[1]: the actor's
    count, hence its next rate, stays while the critic's advances); and, flag cleared, an all-zero-advantage launch
    (the actor's count stays again).  Every taken step equals the Adam statement at the rate of ITS network's count."""
    _, cosine, period = sref.SCHEDULES['cosine']
    starts = (2, period - 2)
    rule = dict(kind='adam', betas=(0.9, 0.999), weight_decay=0.0)
    lrs = [3e-4, 1e-3]
    which = 0 if scheduled == 'actor' else 1
    counts = list(range(starts[which], starts[which] + 4))
    lrs[which] = sref.safe_rate(cosine, counts, derived(rule), rates=(lrs[which],) + sref.BASE_RATES)
    schedules = [None, None]
    schedules[which] = cosine
    packed = [sref.pack(s) for s in schedules]
    (actor, want_a, sums_a), (critic, want_c, sums_c) = pair_nets(steps=starts)
    zero_adv = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32, device='cuda')
    skip = actor.state.ptr(1)
    kl = float(F32(STATS[1]) * F32(GRAD_SCALE))
    taken_a, taken_c = starts
    plan = [dict(kl_threshold=2 * kl), dict(kl_threshold=kl / 2), dict(kl_threshold=2 * kl),
            dict(kl_threshold=2 * kl, adv_stats=zero_adv.data_ptr())]
    for k, arguments in enumerate(plan):
        if k == 3:
            actor.state.tensor[64 + 1] = 0                       # (the flag is the agent's to clear: a new update)
        actor.load(sums_a[k]), critic.load(sums_c[k])
        pair_step(lib, actor, critic, packed, skip=skip, lrs=lrs, **arguments)
        if k in (0, 1):                                          # the actor's step is taken
            want_a = adam_at(lrs[0], schedules[0], want_a, sums_a[k], taken_a)
            taken_a += 1
        want_c = adam_at(lrs[1], schedules[1], want_c, sums_c[k], taken_c)
        taken_c += 1
        got_a, got_c = actor.read(), critic.read()
        for name, got, want in zip(('p', 'exp_avg', 'exp_avg_sq'), got_a[:3], want_a):
            assert same_bits(got, want), f'launch {k}: the actor\'s {name}'
        for name, got, want in zip(('p', 'exp_avg', 'exp_avg_sq'), got_c[:3], want_c):
            assert same_bits(got, want), f'launch {k}: the critic\'s {name}'
        assert got_a[3].tolist() == [taken_a, 1 if k in (1, 2) else 0, STATE_MARK, 0], (k, got_a[3])
        assert got_c[3].tolist() == [taken_c, 0, STATE_MARK, 0], (k, got_c[3])
    assert (taken_a, taken_c) == (starts[0] + 2, starts[1] + 4)
    row, stop = expected_row(1, kl_threshold=kl / 2)
    assert stop


def test_a_set_skip_flag_leaves_the_single_step_where_it_was(lib):
    rule = rule_of('sgd-momentum')
    p, _, _, sums = adam_case(N, 1, 45)
    slots = start_slots(rule, N, 3, 45)
    net = FamilyNet(rule, p, slots, step=3)
    net.load(sums[0])
    flag = torch.ones(1, dtype=torch.int32, device='cuda')
    scheduled_step(lib, net, sref.pack(sref.SCHEDULES['linear'][1]), skip=flag.data_ptr())
    got_p, got_slots, state, info = net.read()
    assert same_bits(got_p, p) and same_bits(got_slots[0], slots[0])
    assert state.tolist() == [3, 0, STATE_MARK, 0] and np.isnan(info).all()


# ------------------------------------------------------------------------------------------------ polyak

def test_polyak_rides_in_the_scheduled_launch(lib):
    """A block of 1031 at offset 1031 in buffers of 2 * 1031 + 5: the block's targets mix with the NEW parameters, the
    targets outside with their (unchanged) online values — the unscheduled launch's expectations at the rate lr_t."""
    total, offset, coeff, t = 2 * N + 5, N, 0.005, 5
    _, schedule, _ = sref.SCHEDULES['warmup-cosine']
    rule = dict(rule_of('adam-maximize'), maximize=False)
    rule['lr'] = sref.safe_rate(schedule, [t], derived(rule), rates=(rule['lr'],) + sref.BASE_RATES)
    rng = np.random.RandomState(46)
    online_host, target_host = rng.normal(size=total).astype(F32), rng.normal(size=total).astype(F32)
    _, m, v, sums = adam_case(N, 1, 46, warm=True)
    online, target = Guarded(online_host), Guarded(target_host)
    net = FamilyNet(rule, online_host[offset:offset + N].copy(), [m, v], step=t, info=False)
    net.load(sums[0])
    scheduled_step(lib, net, sref.pack(schedule), params=online.ptr(offset),
                   polyak=(target.ptr(), online.ptr(), total, offset, coeff))
    lr_t = sref.value(schedule, rule['lr'], t)
    want_p, want_m, want_v = port.adam_statement(online_host[offset:offset + N], sums[0], m, v, t + 1, GRAD_SCALE, lr_t)
    want_online = online_host.copy()
    want_online[offset:offset + N] = want_p
    want_target = port.polyak([target_host], [want_online], coeff)[0]
    got_online, got_target = online.read(), target.read()
    assert same_bits(got_online, want_online) and same_bits(got_target, want_target)
    _, (got_m, got_v), state, _ = net.read()
    assert same_bits(got_m, want_m) and same_bits(got_v, want_v) and state.tolist() == [t + 1, 0, STATE_MARK, 0]
    outside = np.r_[0:offset, offset + N:total]
    assert not same_bits(got_target[outside], target_host[outside])
