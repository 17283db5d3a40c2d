"""tonic_optimizer_step (csrc/optim.hip: optimizer_kernel) through the C ABI: every rule of the optimizer family against
its float32 statement (tests/optim_family_ref.py) BIT FOR BIT — parameters and every state buffer, after each launch.

The launch is the one behind tonic_adam_step, so the sizes are those of tests/test_gpu_optim.py, decided by the same constants:

| case                                    | decided by                                                                  |
|-----------------------------------------|-----------------------------------------------------------------------------|
| n = 1, 255, 256, 257                    | 256 threads: one ragged / full workgroup, two                               |
| n = 32 768, 32 769                      | adam_blocks_for caps the grid at 128 workgroups: the last size without and  |
|                                         | the first with a second pass of the grid-stride loop                        |
| n = 98 311                              | three passes, the last one ragged                                           |
| state[0] = 0 | 999                      | SGD's `buf = g` (only at 0; its buffer is pre-filled with 7 there: what it  |
|                                         | holds is not used), bias corrections far from / near 1, zero / warm state   |
| 3 steps, gradients x 1, 1e-2, 1e-4      | amsgrad: exp_avg_sq falls below max_exp_avg_sq, which must stay             |
| skip flag set                           | `if (a.skip != nullptr && *a.skip != 0) return` ahead of everything         |
| polyak: block first / last / whole,     | workgroups >= adam_blocks update the targets OUTSIDE the block, `extra` =   |
| total - n = 2048 x 256 + 777, (2, 1)    | ceil((total - n) / 256) capped at 2048                                      |
| stats_kind 1 .. 4, kl above threshold,  | adam_finalize, as behind tonic_adam_step: rows, stop flag and counter must    |
| adv_stats[2] = 1; n = 300, 40 000       | equal what tonic_adam_step writes for the same sums (2 / 128 workgroups)    |

Every buffer lies between sentinel margins (test_gpu_optim.Guarded) that must come back untouched; the state buffers
of a rule are ONE allocation of slots x n floats, so a slot written past its end lands in its neighbour and shows
there.  Measured on the MI355X: see DESIGN.md section 2."""
import ctypes

import numpy as np
import pytest

import numpy_port as port
import optim_family_ref as ref
from test_gpu_optim import (ADAM_SIZES, F32, GRAD_SCALE, NAN, STATE_MARK, STATS, Guarded, Net, adam_step, bits,
                            expected_row, same_bits)
from test_oracle_golden import adam_case

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

NAMES = list(ref.CONFIGURATIONS)
SHRINK = (1.0, 1e-2, 1e-4)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


def rule_of(name):
    from tonic_amd.torch import updaters
    return updaters.optimizer_hyperparameters(ref.factory(name), 1e-3)


class FamilyNet:
    """One network's buffers for tonic_optimizer_step.  `read()` -> p, [state buffers], state, info_row."""

    def __init__(self, rule, p, slots, step=0, info=True):
        from tonic_amd.torch import updaters
        self.rule, self.packed, self.n = rule, updaters.optimizer_rule(rule), p.size
        assert len(slots) == len(ref.slot_names(rule))
        self.p = Guarded(p)
        self.slots = Guarded(np.concatenate(slots)) if slots else None
        self.state = Guarded(np.array([step, 0, STATE_MARK, 0], np.int32))
        self.info = Guarded(np.full(8, NAN, F32)) if info else None

    def load(self, sums, stats=STATS):
        self.sums_host = np.concatenate([sums, stats]).astype(F32)
        self.sums = Guarded(self.sums_host)

    def step(self, lib, kind=0, kl_threshold=0.0, entropy_coeff=0.0, adv_stats=None, skip=None, params=None,
             polyak=(None, None, 0, 0, 0.0)):
        from tonic_amd import _lib
        _lib.check(lib.tonic_optimizer_step(
            params if params is not None else self.p.ptr(), self.sums.ptr(),
            self.slots.ptr() if self.slots is not None else None, self.state.ptr(), self.n, GRAD_SCALE,
            ctypes.byref(self.packed), kind, kl_threshold, entropy_coeff, adv_stats,
            self.info.ptr() if self.info is not None else None, skip, *polyak, None), 'tonic_optimizer_step')

    def read(self):
        assert same_bits(self.sums.read(), self.sums_host), 'the optimizer only READS the gradient sums'
        slots = list(self.slots.read().reshape(-1, self.n)) if self.slots is not None else []
        return self.p.read(), slots, self.state.read(), self.info.read() if self.info is not None else None


def start_slots(rule, n, start, seed):
    """Zero state at step 0 — but SGD's buffer holds 7: the first step taken must not use it — warm state later."""
    if start:
        return ref.warm_slots(rule, n, seed)
    fill = 7.0 if rule['kind'] == 'sgd' else 0.0
    return [np.full(n, fill, F32) for _ in ref.slot_names(rule)]


def check(what, rule, got_p, got_slots, want_p, want_slots):
    for name, got, want in [('parameters', got_p, want_p)] + list(zip(ref.slot_names(rule), got_slots, want_slots)):
        differ = np.flatnonzero(bits(got) != bits(want))
        assert differ.size == 0, (f'{what}: {name} differ from the statement in {differ.size} of {got.size} elements, '
                                  f'first [{differ[0]}]: {got[differ[0]]!r} != {want[differ[0]]!r}')


@pytest.mark.parametrize('start', [0, 999], ids=['from-zero', 'from-999'])
@pytest.mark.parametrize('n', ADAM_SIZES)
@pytest.mark.parametrize('name', NAMES)
def test_family_step_sizes(lib, name, n, start):
    """Three consecutive steps with shrinking gradients: parameters and every state buffer equal the statement bit for
    bit after EACH launch, the counter advances by one per launch, the arrivals word is back at 0 and state[1],
    state[2] are left alone."""
    rule = rule_of(name)
    p, _, _, sums = adam_case(n, 3, 31)
    slots = start_slots(rule, n, start, 31)
    net = FamilyNet(rule, p, slots, step=start, info=False)
    want_p, want_slots = p, slots
    for k in range(3):
        step_sums = (sums[k] * F32(SHRINK[k])).astype(F32)
        net.load(step_sums)
        net.step(lib)
        want_p, want_slots = ref.family_statement(rule, want_p, step_sums, want_slots, start + k + 1, GRAD_SCALE)
        got_p, got_slots, state, _ = net.read()
        check(f'{name}, n = {n}, step {start + k + 1}', rule, got_p, got_slots, want_p, want_slots)
        assert state.tolist() == [start + k + 1, 0, STATE_MARK, 0], state
    assert np.isfinite(want_p).all() and (n == 1 or not same_bits(want_p, p))
    if rule.get('amsgrad') and n > 1:
        assert (want_slots[2] > want_slots[1]).any(), 'the maximum was never above the running average'


def test_family_plain_adam_is_adam_statement(lib):
    """The Adam rule without its options through the new entry: `numpy_port.adam_statement`, as tonic_adam_step."""
    n = 4097
    p, m, v, sums = adam_case(n, 2, 32, warm=True)
    rule = dict(rule_of('adam-maximize'), maximize=False)
    net = FamilyNet(rule, p, [m, v], step=5)
    want = (p, m, v)
    for k in range(2):
        net.load(sums[k])
        net.step(lib)
        want = port.adam_statement(want[0], sums[k], want[1], want[2], 6 + k, GRAD_SCALE, rule['lr'])
        got_p, got_slots, _, _ = net.read()
        check(f'step {6 + k}', rule, got_p, got_slots, want[0], list(want[1:]))


@pytest.mark.parametrize('n', [300, 40_000])
@pytest.mark.parametrize('name', NAMES)
def test_family_skip_flag_changes_nothing(lib, name, n):
    """A set skip flag: parameters, EVERY state buffer, the counter and the info row are untouched."""
    rule = rule_of(name)
    p, _, _, sums = adam_case(n, 1, 33)
    slots = ref.warm_slots(rule, n, 33)
    flag = Guarded(np.array([7], np.int32))
    net = FamilyNet(rule, p, slots, step=3)
    net.load(sums[0])
    net.step(lib, kind=1, kl_threshold=-1.0, skip=flag.ptr())
    got_p, got_slots, state, info = net.read()
    assert same_bits(got_p, p) and all(same_bits(g, s) for g, s in zip(got_slots, slots))
    assert state.tolist() == [3, 0, STATE_MARK, 0] and flag.read().tolist() == [7]
    assert same_bits(info, np.full(8, NAN, F32)), info


@pytest.mark.parametrize('n', [300, 40_000])
@pytest.mark.parametrize('name', NAMES)
def test_family_rows_are_adam_steps_rows(lib, name, n):
    """stats_kind 1 .. 4 (kind 1 with a kl above the threshold and an entropy coefficient): the info row and the state
    block equal, bit for bit, what tonic_adam_step writes for the same sums — and the step itself is the statement.
    Then the all-zero-advantages case: no step, the counter does not move, loss = kl = clip_fraction = 0, no stop."""
    rule = rule_of(name)
    p, m, v, sums = adam_case(n, 1, 34)
    slots = ref.warm_slots(rule, n, 34)
    want_p, want_slots = ref.family_statement(rule, p, sums[0], slots, 6, GRAD_SCALE)
    for kind in (1, 2, 3, 4):
        adam, net = Net(p, m, v, step=5), FamilyNet(rule, p, slots, step=5)
        adam.load(sums[0])
        net.load(sums[0])
        adam_step(lib, adam, kind=kind, kl_threshold=1e-3, entropy_coeff=0.01)
        net.step(lib, kind=kind, kl_threshold=1e-3, entropy_coeff=0.01)
        *_, adam_state, adam_info = adam.read()
        got_p, got_slots, state, info = net.read()
        check(f'{name}, n = {n}, kind {kind}', rule, got_p, got_slots, want_p, want_slots)
        assert same_bits(info, adam_info) and same_bits(state, adam_state), (kind, info, adam_info, state, adam_state)
        assert same_bits(info, expected_row(kind, entropy_coeff=0.01, kl_threshold=1e-3)[0])
        assert state.tolist() == [6, int(kind == 1), STATE_MARK, 0], (kind, state)
    adv_stats = Guarded(np.array([0.25, 1.5, 1.0, 1.0], F32))
    adam, net = Net(p, m, v, step=5), FamilyNet(rule, p, slots, step=5)
    adam.load(sums[0])
    net.load(sums[0])
    adam_step(lib, adam, kind=1, kl_threshold=1e-3, entropy_coeff=0.01, adv_stats=adv_stats.ptr())
    net.step(lib, kind=1, kl_threshold=1e-3, entropy_coeff=0.01, adv_stats=adv_stats.ptr())
    *_, adam_state, adam_info = adam.read()
    got_p, got_slots, state, info = net.read()
    assert same_bits(got_p, p) and all(same_bits(g, s) for g, s in zip(got_slots, slots))
    assert same_bits(info, adam_info) and same_bits(state, adam_state)
    assert state.tolist() == [5, 0, STATE_MARK, 0] and info[:2].tolist() == [0.0, 0.0] and info[5] == 0.0


def polyak_case(lib, name, offset, n, total):
    coeff = 0.005
    rule = rule_of(name)
    p, _, _, sums = adam_case(n, 2, 35)
    slots = start_slots(rule, n, 0, 35)
    rng = np.random.RandomState([offset, n, total % 65521])
    online = rng.standard_normal(total).astype(F32)
    online[offset:offset + n] = p
    target = rng.standard_normal(total).astype(F32)
    d_online, d_target = Guarded(online), Guarded(target)
    net = FamilyNet(rule, p, slots)
    want_p, want_slots = p, slots
    for k in range(2):
        net.load(sums[k])
        net.step(lib, kind=4, params=d_online.ptr(offset),
                 polyak=(d_target.ptr(), d_online.ptr(), total, offset, coeff))
        want_p, want_slots = ref.family_statement(rule, want_p, sums[k], want_slots, k + 1, GRAD_SCALE)
        online = online.copy()
        online[offset:offset + n] = want_p
        target = port.polyak([target], [online], coeff)[0]
        _, got_slots, state, info = net.read()
        got_online, got_target = d_online.read(), d_target.read()
        what = f'{name}: block [{offset}, +{n}) of {total}, step {k + 1}'
        check(what, rule, got_online[offset:offset + n], got_slots, want_p, want_slots)
        assert same_bits(got_online, online), f'{what}: the online buffer outside the block moved'
        differ = np.flatnonzero(bits(got_target) != bits(target))
        assert differ.size == 0, f'{what}: {differ.size} target entries differ, first [{differ[0]}]'
        assert state.tolist() == [k + 1, 0, STATE_MARK, 0], state
        assert same_bits(info, expected_row(4)[0]), info
    assert same_bits(net.p.read(), p), 'the block is updated in the online buffer, nowhere else'


@pytest.mark.parametrize('name', NAMES)
def test_family_polyak_tail(lib, name):
    """Every rule with the polyak tail, the block in the middle of the buffer: targets inside the block follow the
    STEPPED value, targets outside follow their online value, once per step, bit for bit (`numpy_port.polyak`)."""
    polyak_case(lib, name, 333, 1000, 5000)


@pytest.mark.parametrize('offset,n,total', [(0, 1000, 5000), (4000, 1000, 5000), (0, 5000, 5000),
                                            (333, 1000, 1000 + 2048 * 256 + 777), (0, 1, 2), (1, 1, 2)],
                         ids=['block-first', 'block-last', 'block-whole', 'outside-strided', 'two-first',
                              'two-last'])
def test_family_polyak_edges(lib, offset, n, total):
    """The edges of test_gpu_optim.test_adam_polyak_step_edges for the rule with the most state."""
    polyak_case(lib, 'rmsprop-centered-momentum', offset, n, total)


def test_family_entry_validates(lib):
    """Refused before any GPU work: a block outside the online buffer, params that are not that block, missing state."""
    rule = rule_of('sgd-momentum')
    p, _, _, sums = adam_case(16, 1, 36)
    net = FamilyNet(rule, p, start_slots(rule, 16, 0, 36))
    net.load(sums[0])
    online, target = Guarded(np.zeros(32, F32)), Guarded(np.zeros(32, F32))
    for params, polyak in ((online.ptr(20), (target.ptr(), online.ptr(), 32, 20, 0.005)),
                           (online.ptr(4), (target.ptr(), online.ptr(), 32, 8, 0.005))):
        status = lib.tonic_optimizer_step(params, net.sums.ptr(), net.slots.ptr(), net.state.ptr(), 16, GRAD_SCALE,
                                          ctypes.byref(net.packed), 0, 0.0, 0.0, None, None, None, *polyak, None)
        assert status == -1 and b'block' in lib.tonic_last_error()
    status = lib.tonic_optimizer_step(net.p.ptr(), net.sums.ptr(), None, net.state.ptr(), 16, GRAD_SCALE,
                                      ctypes.byref(net.packed), 0, 0.0, 0.0, None, None, None, None, None, 0, 0, 0.0,
                                      None)
    assert status == -1
    assert same_bits(net.p.read(), p) and net.state.read().tolist() == [0, 0, STATE_MARK, 0]
