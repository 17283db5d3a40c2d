"""Every path of the optimizer kernels (csrc/optim.hip) through the C ABI, at the sizes where its routing changes.

Each case names the constant in optim.hip that makes it what it is: whoever moves a constant moves the case with it.

| entry / kernel                | case                                    | decided by                                           |
|-------------------------------|-----------------------------------------|------------------------------------------------------|
| tonic_adam_step / optimizer_  | n = 1, 255, 256, 257                    | 256 threads: one ragged / full workgroup, two        |
| kernel<AdamRule<false>>       | n = 32 768, 32 769                      | adam_blocks_for caps the grid at 128 workgroups:     |
|                               |                                         | the last size without and the first with a second    |
|                               |                                         | pass of the grid-stride loop                         |
|                               | n = 98 311                              | three passes, the last one ragged                    |
|                               | state[0] = 0 | 999                      | bias corrections far from / near 1                   |
| adam_finalize                 | n = 300 (2 workgroups), 40 000 (128)    | the LAST workgroup to arrive at state[3] finalises   |
|                               | stats_kind 1 .. 4, info_row NULL        | which info_row slots are written                     |
|                               | kl <, ==, > kl_threshold                | the strict `kl > kl_threshold`; state[1]             |
|                               | entropy_coeff 0 | 0.01                  | `loss -= entropy_coeff * entropy`                    |
|                               | adv_stats[2] = 1                        | all_zero: no step, counter kept, loss = kl = cf = 0  |
| skip flag                     | *d_skip_flag != 0; skip = &state[1]     | `if (a.skip != nullptr && *a.skip != 0) return`      |
| tonic_adam_step_pair          | (40 000, 300), (300, 40 000),           | both networks share gridDim.x = blocks of the LONGER |
|                               | (4097, 4097), (5000, 1)                 | one; the shorter one's spare workgroups still arrive |
|                               | first network skipped / all-zero        | blockIdx.y = 0 returns or idles, blockIdx.y = 1 steps |
| tonic_adam_polyak_step        | offset 0; block ending at total;        | workgroups >= adam_blocks update the targets OUTSIDE |
|                               | block = whole buffer (extra = 0);       | the block, `extra` = ceil((total - n) / 256) capped  |
|                               | total - n = 2048 x 256 + 777; (2, 1)    | at 2048: beyond it their loop strides                |
| the Adam entries ==           | n = 1, 257, 32 769, 40 000; step 0, 999 | optim_fill: the entries' four numbers as the plain-  |
| tonic_optimizer_step          | polyak: block last / whole              | Adam tonic_optimizer_t, their moments as slot 0, 1   |
| tonic_clip_grad_norm          | n = 1, 7, 1023, 1024, 1025              | 1024 elements per partial workgroup: one, then two   |
|                               | n = 65 536, 65 537                      | kClipBlocks = 64: slices of 1024, then of 1025 with  |
|                               |                                         | a short last one                                     |
|                               | n = 262 147                             | scale grid capped at 1024 x 256 = 262 144: 3 strided |

References.  `numpy_port.adam_statement` is the kernels' float32 expression, operation by operation: parameters and
both moments must equal it BIT FOR BIT (-ffp-contract=off, correctly rounded divide and sqrt; the step's constants are
formed in float64 on the device as in Python and rounded once).  Parameters are also held to `numpy_port.adam_f64`
within 2 x ADAM_F64_UNITS of `adam_f64_unit` (one ulp of the parameter + lr * 2**-23): ADAM_F64_UNITS is the
statement's own distance from float64 over 7 steps, measured on the CPU by
test_oracle_golden.py::test_adam_statement_against_torch_and_float64 on the inputs of `adam_case` used here.
Measured on the MI355X: bit-identical in every case, so the kernels' distance from float64 is the statement's — at
most 3.8 units after the three steps taken here (n = 32 769, from step 999), against the bound of 16.
Logged statistics: F32(sum) * F32(grad_scale), bit for bit.  Polyak: `numpy_port.polyak`, bit for bit.
Clipping: `numpy_port.clip_grad_norm_f64` (exactly rounded sum of squares): norm and coefficient within one float32
ulp (the kernel adds float64 partials in another order, so one rounding may flip), every element within 2 ulps of
F32(sum * coef); measured on the MI355X: norm at most 0.47 ulps off, coefficient 0.34, elements 0.92.  (With the
coefficient formed in float32 from the rounded norm, as before this module, it was 1.16 ulps off at n = 1024.)

Every buffer lies between two margins of MARGIN sentinel words (NaN for floats, STATE_FILL for `state`) that must come
back untouched, like the 8 statistic slots behind grad_sums[n] and grad_sums itself (the optimizer only reads them).
"""
import numpy as np
import pytest

import numpy_port as port
from test_oracle_golden import ADAM_GRAD_SCALE as GRAD_SCALE
from test_oracle_golden import ADAM_LR as LR
from test_oracle_golden import adam_case

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

F32 = np.float32
MARGIN = 64                       # words (256 bytes: the inner buffer keeps the allocation's alignment)
STATE_FILL = 0x5A5A5A5A
STATE_MARK = 0x01234567           # state[2]: no kernel reads or writes it
NAN = F32('nan')
STATS = np.array([12.5, 0.37, 3.0, -51.8, 7.4, 111.0, 222.0, 333.0], F32)      # the 8 slots behind grad_sums[n]
ADAM_SIZES = [1, 255, 256, 257, 32_768, 32_769, 98_311]
CLIP_SIZES = [1, 7, 1023, 1024, 1025, 65_536, 65_537, 262_147]


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


class Guarded:
    """A device buffer (float32 or int32) between two margins of sentinel words."""

    def __init__(self, inner):
        inner = np.ascontiguousarray(inner).reshape(-1)
        assert inner.dtype in (np.float32, np.int32)
        self.size = inner.size
        host = np.full(self.size + 2 * MARGIN, NAN if inner.dtype == np.float32 else STATE_FILL, inner.dtype)
        self.fill = int(bits(host)[0])
        host[MARGIN:MARGIN + self.size] = inner
        self.tensor = torch.from_numpy(host).cuda()

    def ptr(self, offset=0):
        assert 0 <= offset < self.size
        return self.tensor.data_ptr() + 4 * (MARGIN + offset)

    def read(self):
        host = self.tensor.cpu().numpy()
        margins = np.concatenate([bits(host)[:MARGIN], bits(host)[MARGIN + self.size:]])
        assert (margins == self.fill).all(), 'a kernel wrote outside its buffer'
        return host[MARGIN:MARGIN + self.size].copy()


class Net:
    """One network's optimizer buffers.  `read()` -> p, m, v, state, info_row (None without one)."""

    def __init__(self, p, m, v, step=0, info=True):
        self.n = p.size
        self.p, self.m, self.v = Guarded(p), Guarded(m), Guarded(v)
        self.state = Guarded(np.array([step, 0, STATE_MARK, 0], np.int32))
        self.info = Guarded(np.full(8, NAN, F32)) if info else None
        self.sums = None

    def load(self, sums, stats=STATS):
        self.sums_host = np.concatenate([sums, stats]).astype(F32)
        assert self.sums_host.size == self.n + 8
        self.sums = Guarded(self.sums_host)

    def read(self):
        assert same_bits(self.sums.read(), self.sums_host), 'the optimizer only READS the gradient sums'
        return (self.p.read(), self.m.read(), self.v.read(), self.state.read(),
                self.info.read() if self.info is not None else None)


def adam_step(lib, net, lr=LR, kind=0, kl_threshold=0.0, entropy_coeff=0.0, adv_stats=None, skip=None, row=0):
    from tonic_amd import _lib
    _lib.check(lib.tonic_adam_step(
        net.p.ptr(), net.sums.ptr(), net.m.ptr(), net.v.ptr(), net.state.ptr(), net.n, GRAD_SCALE, lr, 0.9, 0.999,
        1e-8, kind, kl_threshold, entropy_coeff, adv_stats, net.info.ptr(8 * row) if net.info is not None else None,
        skip, None), 'tonic_adam_step')


def scaled(stat):
    """A logged statistic: F32(sum) * F32(grad_scale), one float32 product."""
    return F32(stat) * F32(GRAD_SCALE)


def expected_row(kind, stats=STATS, entropy_coeff=0.0, kl_threshold=0.0, all_zero=False):
    """adam_finalize's info_row for `kind` (NaN = the slot keeps its sentinel) and whether it raises the stop."""
    row = np.full(8, NAN, F32)
    if kind == 1:
        loss, kl, clip_fraction = scaled(stats[0]), scaled(stats[1]), scaled(stats[2])
        entropy, std = scaled(stats[3]), scaled(stats[4])
        if entropy_coeff != 0.0:
            loss = F32(loss - F32(F32(entropy_coeff) * entropy))
        if all_zero:
            loss = kl = clip_fraction = F32(0)
        stop = bool(kl > F32(kl_threshold))
        row[:] = [loss, kl, entropy, clip_fraction, std, 1.0 if stop else 0.0, 1.0, 0.0]
        return row, stop
    count = {0: 0, 2: 2, 3: 3, 4: 1}[kind]
    row[:count] = [scaled(s) for s in stats[:count]]
    if kind:
        row[6] = 1.0
    return row, False


class Statement:
    """The float32 statement and the float64 reference side by side, step by step."""

    def __init__(self, p, m, v, step=0):
        self.p, self.m, self.v, self.step = p, m, v, step
        self.p64, self.m64, self.v64 = p, m, v

    def advance(self, sums, lr=LR):
        self.step += 1
        self.p, self.m, self.v = port.adam_statement(self.p, sums, self.m, self.v, self.step, GRAD_SCALE, lr)
        self.p64, self.m64, self.v64 = port.adam_f64(self.p64, sums, self.m64, self.v64, self.step, GRAD_SCALE, lr)

    def check(self, what, p, m, v, lr=LR):
        """Bit equality with the statement (all three), then the float64 bound (parameters) -> its units."""
        for name, got, want in (('parameters', p, self.p), ('exp_avg', m, self.m), ('exp_avg_sq', v, self.v)):
            differ = np.flatnonzero(bits(got) != bits(want))
            assert differ.size == 0, (f'{what}: {name} differ from adam_statement in {differ.size} of {got.size} '
                                      f'elements, first [{differ[0]}]: {got[differ[0]]!r} != {want[differ[0]]!r}')
        units = float((np.abs(p - self.p64) / port.adam_f64_unit(self.p64, lr)).max())
        assert units <= 2 * port.ADAM_F64_UNITS, f'{what}: {units:.2f} units from adam_f64'
        return units


# ------------------------------------------------------------------ tonic_adam_step: sizes, three steps

@pytest.mark.parametrize('start', [0, 999], ids=['from-zero', 'from-999'])
@pytest.mark.parametrize('n', ADAM_SIZES)
def test_adam_step_sizes(lib, n, start):
    """Three consecutive steps: every element equals the statement bit for bit after EACH launch (a skipped
    grid-stride pass, a stale step counter or a second finalisation shows at once), the counter advances by one per
    launch, the arrivals word is back at 0 and state[1], state[2] are left alone."""
    p, m, v, sums = adam_case(n, 3, 1, warm=start != 0)
    net, want = Net(p, m, v, step=start, info=False), Statement(p, m, v, step=start)
    zero = slice(n // 2, n // 2 + n // 5)
    worst = 0.0
    for k in range(3):
        net.load(sums[k])
        adam_step(lib, net)
        want.advance(sums[k])
        got_p, got_m, got_v, state, _ = net.read()
        worst = max(worst, want.check(f'n = {n}, step {start + k + 1}', got_p, got_m, got_v))
        assert state.tolist() == [start + k + 1, 0, STATE_MARK, 0], state
        if start == 0:           # m = v = 0, denom = eps: an exactly zero gradient moves nothing
            assert same_bits(got_p[zero], p[zero]) and not got_m[zero].any() and not got_v[zero].any()
    print(f'adam n = {n} from step {start}: {worst:.2f} units from float64 (bound {2 * port.ADAM_F64_UNITS:g})')


# ------------------------------------------------------------------ adam_finalize

def kl_thresholds():
    """kl_threshold just above, at and just below the kl the kernel forms: kl is below, equal, above."""
    kl = scaled(STATS[1])
    return [('kl-below', float(np.nextafter(kl, F32(np.inf))), False), ('kl-equal', float(kl), False),
            ('kl-above', float(np.nextafter(kl, F32(-np.inf))), True)]


@pytest.mark.parametrize('n', [300, 40_000])
def test_finalize_ppo_actor_row(lib, n):
    """stats_kind 1: the row {loss, kl, entropy, clip_fraction, std, stop, 1, 0}, the entropy term (a product and a
    subtraction, two roundings), the STRICT `kl > kl_threshold` and state[1]."""
    p, m, v, sums = adam_case(n, 1, 2)
    want = Statement(p, m, v)
    want.advance(sums[0])
    for entropy_coeff in (0.0, 0.01):
        for name, threshold, stops in kl_thresholds():
            net = Net(p, m, v)
            net.load(sums[0])
            adam_step(lib, net, kind=1, kl_threshold=threshold, entropy_coeff=entropy_coeff)
            got_p, got_m, got_v, state, info = net.read()
            what = f'n = {n}, entropy_coeff {entropy_coeff}, {name}'
            want.check(what, got_p, got_m, got_v)
            row, stop = expected_row(1, entropy_coeff=entropy_coeff, kl_threshold=threshold)
            assert stop == stops, what
            assert same_bits(info, row), (what, info, row)
            assert state.tolist() == [1, int(stops), STATE_MARK, 0], (what, state)
    assert expected_row(1, entropy_coeff=0.01)[0][0] != expected_row(1)[0][0]


@pytest.mark.parametrize('n', [300, 40_000])
@pytest.mark.parametrize('kind', [2, 3, 4])
def test_finalize_other_rows(lib, n, kind):
    """stats_kind 2, 3, 4 write {2, 3, 1} scaled sums and info_row[6] = 1; every other slot keeps its sentinel and
    state[1] stays 0 whatever the threshold."""
    p, m, v, sums = adam_case(n, 1, 2)
    want = Statement(p, m, v)
    want.advance(sums[0])
    net = Net(p, m, v)
    net.load(sums[0])
    adam_step(lib, net, kind=kind, kl_threshold=-1.0, entropy_coeff=0.01)
    got_p, got_m, got_v, state, info = net.read()
    want.check(f'n = {n}, kind {kind}', got_p, got_m, got_v)
    row, _ = expected_row(kind)
    assert np.isnan(row).sum() == {2: 5, 3: 4, 4: 6}[kind]
    assert same_bits(info, row), (info, row)
    assert state.tolist() == [1, 0, STATE_MARK, 0], state


@pytest.mark.parametrize('n', [300, 40_000])
def test_finalize_all_zero_advantages(lib, n):
    """adv_stats[2] != 0 (actors.py:71): no step — parameters, moments and counter unchanged — loss = kl =
    clip_fraction = 0, entropy and std kept, info_row[6] = 1, no stop even with a kl sum above the threshold; with
    adv_stats[2] == 0 the same call steps and stops."""
    p, m, v, sums = adam_case(n, 1, 3, warm=True)
    for flag in (1.0, 0.0):
        adv_stats = Guarded(np.array([0.25, 1.5, flag, 1.0], F32))
        net = Net(p, m, v, step=5)
        net.load(sums[0])
        adam_step(lib, net, kind=1, kl_threshold=1e-3, entropy_coeff=0.01, adv_stats=adv_stats.ptr())
        got_p, got_m, got_v, state, info = net.read()
        assert same_bits(adv_stats.read(), np.array([0.25, 1.5, flag, 1.0], F32))
        row, stop = expected_row(1, entropy_coeff=0.01, kl_threshold=1e-3, all_zero=bool(flag))
        assert same_bits(info, row), (flag, info, row)
        if flag:
            assert not stop and same_bits(got_p, p) and same_bits(got_m, m) and same_bits(got_v, v)
            assert info.tolist()[:2] == [0.0, 0.0] and info[3] == 0.0 and info[5] == 0.0 and info[6] == 1.0
            assert info[2] == scaled(STATS[3]) and info[4] == scaled(STATS[4])
            assert state.tolist() == [5, 0, STATE_MARK, 0], state
        else:
            want = Statement(p, m, v, step=5)
            want.advance(sums[0])
            want.check(f'n = {n}, advantages not all zero', got_p, got_m, got_v)
            assert stop and state.tolist() == [6, 1, STATE_MARK, 0], state


@pytest.mark.parametrize('n', [300, 40_000])
def test_finalize_without_info_row(lib, n):
    """info_row = NULL with every kind: the step is taken, the counter advances and nothing else is written (kind 1
    raises no stop without a row)."""
    p, m, v, sums = adam_case(n, 1, 4)
    want = Statement(p, m, v)
    want.advance(sums[0])
    for kind in (0, 1, 2, 3, 4):
        net = Net(p, m, v, info=False)
        net.load(sums[0])
        adam_step(lib, net, kind=kind, kl_threshold=-1.0, entropy_coeff=0.01)
        got_p, got_m, got_v, state, _ = net.read()
        want.check(f'n = {n}, kind {kind}, no row', got_p, got_m, got_v)
        assert state.tolist() == [1, 0, STATE_MARK, 0], (kind, state)


# ------------------------------------------------------------------ the skip flag

@pytest.mark.parametrize('n', [300, 40_000])
def test_skip_flag_changes_nothing(lib, n):
    p, m, v, sums = adam_case(n, 1, 5, warm=True)
    flag = Guarded(np.array([7], np.int32))
    net = Net(p, m, v, step=3)
    net.load(sums[0])
    adam_step(lib, net, kind=1, kl_threshold=-1.0, skip=flag.ptr())
    got_p, got_m, got_v, state, info = net.read()
    assert same_bits(got_p, p) and same_bits(got_m, m) and same_bits(got_v, v)
    assert state.tolist() == [3, 0, STATE_MARK, 0] and flag.read().tolist() == [7]
    assert same_bits(info, np.full(8, NAN, F32)), info


@pytest.mark.parametrize('n', [300, 40_000])
def test_skip_flag_is_the_ppo_stop(lib, n):
    """PPO's pattern: four launches with skip = &state[1], one info row each; the second launch's kl exceeds the
    threshold.  It still steps (ppo.py:43-46 stops AFTER the update), launches three and four do nothing: the counter
    ends at 2, their rows keep info[6] == 0 and the parameters are two statement steps."""
    p, m, v, sums = adam_case(n, 4, 6)
    net, want = Net(p, m, v), Statement(p, m, v)
    net.info = Guarded(np.zeros(32, F32))                       # (the agents' table starts as zeros)
    kl_sums = [0.1, 0.9, 0.1, 0.9]
    threshold = 0.5 * GRAD_SCALE
    rows = []
    for k in range(4):
        stats = STATS.copy()
        stats[1] = kl_sums[k]
        net.load(sums[k], stats)
        adam_step(lib, net, kind=1, kl_threshold=threshold, skip=net.state.ptr(1), row=k)
        if k < 2:
            want.advance(sums[k])
            rows.append(expected_row(1, stats, kl_threshold=threshold)[0])
        got_p, got_m, got_v, state, info = net.read()
        want.check(f'n = {n}, launch {k + 1}', got_p, got_m, got_v)
        assert state.tolist() == [min(k + 1, 2), int(k >= 1), STATE_MARK, 0], (k, state)
    assert rows[0][5] == 0.0 and rows[1][5] == 1.0
    assert same_bits(info, np.concatenate(rows + [np.zeros(16, F32)])), info
    assert info[2 * 8 + 6] == 0.0 and info[3 * 8 + 6] == 0.0


# ------------------------------------------------------------------ tonic_adam_step_pair

def pair_step(lib, a, b, lr_a, lr_b, kl_threshold, entropy_coeff, adv_stats, skip):
    from tonic_amd import _lib
    _lib.check(lib.tonic_adam_step_pair(
        a.p.ptr(), a.sums.ptr(), a.m.ptr(), a.v.ptr(), a.state.ptr(), a.n, lr_a, 1, kl_threshold, entropy_coeff,
        adv_stats, a.info.ptr(), skip,
        b.p.ptr(), b.sums.ptr(), b.m.ptr(), b.v.ptr(), b.state.ptr(), b.n, lr_b, 2, b.info.ptr(),
        GRAD_SCALE, 0.9, 0.999, 1e-8, None), 'tonic_adam_step_pair')


@pytest.mark.parametrize('mode', ['both-step', 'first-skipped', 'first-all-zero'])
@pytest.mark.parametrize('n_a,n_b', [(40_000, 300), (300, 40_000), (4097, 4097), (5000, 1)])
def test_adam_step_pair_equals_two_calls(lib, n_a, n_b, mode):
    """One launch for two networks (PPO: actor kind 1, critic kind 2, their own learning rates) against two
    tonic_adam_step calls, bit for bit: parameters, moments, info rows and both state blocks, after each of two
    steps.  gridDim.x is sized by the LONGER network, so the shorter one's workgroups beyond its own need do no
    element work and must still arrive at ITS counter — or its finalisation never runs (or runs at the next launch).
    With the first network skipped by its flag, or idle because its advantages are all zero, the second still steps."""
    lr_a, lr_b, threshold, entropy_coeff = 3e-4, 1e-3, 1e9, 0.01
    pa, ma, va, sums_a = adam_case(n_a, 2, 7)
    pb, mb, vb, sums_b = adam_case(n_b, 2, 8, warm=True)
    flag = Guarded(np.array([1 if mode == 'first-skipped' else 0], np.int32))
    adv = Guarded(np.array([0.0, 1.0, 1.0 if mode == 'first-all-zero' else 0.0, 1.0], F32))
    stats_b = STATS[::-1].copy()
    results = []
    for paired in (True, False):
        a, b = Net(pa, ma, va), Net(pb, mb, vb, step=40)
        per_step = []
        for k in range(2):
            a.load(sums_a[k])
            b.load(sums_b[k], stats_b)
            if paired:
                pair_step(lib, a, b, lr_a, lr_b, threshold, entropy_coeff, adv.ptr(), flag.ptr())
            else:
                adam_step(lib, a, lr=lr_a, kind=1, kl_threshold=threshold, entropy_coeff=entropy_coeff,
                          adv_stats=adv.ptr(), skip=flag.ptr())
                adam_step(lib, b, lr=lr_b, kind=2)
            per_step.append(a.read() + b.read())
        results.append(per_step)
    names = [f'{net}.{what}' for net in 'ab' for what in ('params', 'exp_avg', 'exp_avg_sq', 'state', 'info')]
    for k in range(2):
        for name, got, want in zip(names, results[0][k], results[1][k]):
            assert same_bits(got, want), f'step {k + 1}: {name} of the pair differs from the single call'
    # and what both did is the statement: the second network always steps, the first one unless skipped / idle
    got = results[0][1]
    want_b = Statement(pb, mb, vb, step=40)
    want_a = Statement(pa, ma, va)
    for k in range(2):
        want_b.advance(sums_b[k], lr_b)
        if mode == 'both-step':
            want_a.advance(sums_a[k], lr_a)
    want_a.check('first network', *got[:3], lr=lr_a)
    want_b.check('second network', *got[5:8], lr=lr_b)
    assert got[3].tolist() == [2 if mode == 'both-step' else 0, 0, STATE_MARK, 0], got[3]
    assert got[8].tolist() == [42, 0, STATE_MARK, 0], got[8]
    assert same_bits(got[9], expected_row(2, stats_b)[0]), got[9]
    row_a = {'both-step': expected_row(1, entropy_coeff=entropy_coeff, kl_threshold=threshold)[0],
             'first-skipped': np.full(8, NAN, F32),
             'first-all-zero': expected_row(1, entropy_coeff=entropy_coeff, kl_threshold=threshold,
                                            all_zero=True)[0]}[mode]
    assert same_bits(got[4], row_a), got[4]


# ------------------------------------------------------------------ tonic_adam_polyak_step

@pytest.mark.parametrize('offset,n,total', [(0, 1000, 5000), (4000, 1000, 5000), (0, 5000, 5000),
                                            (333, 1000, 1000 + 2048 * 256 + 777), (0, 1, 2), (1, 1, 2)],
                         ids=['block-first', 'block-last', 'block-whole', 'outside-strided', 'two-first',
                              'two-last'])
def test_adam_polyak_step_edges(lib, offset, n, total):
    """The optimizer block at offset 0, ending at `total`, equal to the whole buffer (`extra` = 0: no workgroup for
    the outside range) and with more outside entries than 2048 workgroups cover in one pass.  Two steps: the online
    block equals the statement and the rest of the online buffer is untouched; EVERY target entry, inside and outside
    the block, equals numpy_port.polyak of the NEW online values — once per step, bit for bit."""
    from tonic_amd import _lib
    coeff = 0.005
    p, m, v, sums = adam_case(n, 2, 9)
    rng = np.random.RandomState([offset, n, total % 65521])
    online = rng.standard_normal(total).astype(F32)
    online[offset:offset + n] = p
    target = rng.standard_normal(total).astype(F32)
    d_online, d_target = Guarded(online), Guarded(target)
    net, want = Net(p, m, v), Statement(p, m, v)
    for k in range(2):
        net.load(sums[k])
        _lib.check(lib.tonic_adam_polyak_step(
            d_online.ptr(), net.sums.ptr(), net.m.ptr(), net.v.ptr(), net.state.ptr(), offset, n, total, GRAD_SCALE,
            LR, 0.9, 0.999, 1e-8, 4, net.info.ptr(), d_target.ptr(), coeff, None), 'tonic_adam_polyak_step')
        want.advance(sums[k])
        online = online.copy()
        online[offset:offset + n] = want.p
        target = port.polyak([target], [online], coeff)[0]
        _, got_m, got_v, state, info = net.read()
        got_online, got_target = d_online.read(), d_target.read()
        what = f'block [{offset}, +{n}) of {total}, step {k + 1}'
        want.check(what, got_online[offset:offset + n], got_m, got_v)
        assert same_bits(got_online, online), f'{what}: the online buffer outside the block moved'
        differ = np.flatnonzero(bits(got_target) != bits(target))
        assert differ.size == 0, f'{what}: {differ.size} target entries differ, first [{differ[0]}]'
        assert state.tolist() == [k + 1, 0, STATE_MARK, 0], state
        assert same_bits(info, expected_row(4)[0]), info
    assert same_bits(net.p.read(), p), 'the block is updated in the online buffer, nowhere else'


# ------------------------------------------------------------------ the Adam entries are the optimizer entry

class SlotNet(Net):
    """The same buffers with both moments in ONE allocation, as tonic_optimizer_step takes its state slots."""

    def __init__(self, p, m, v, step=0):
        super().__init__(p, m, v, step)
        self.m = self.v = None
        self.slots = Guarded(np.concatenate([m, v]))

    def read(self):
        assert same_bits(self.sums.read(), self.sums_host), 'the optimizer only READS the gradient sums'
        slots = self.slots.read()
        return self.p.read(), slots[:self.n], slots[self.n:], self.state.read(), self.info.read()


def plain_adam_rule(lr=LR):
    from tonic_amd.torch import updaters
    rule = dict(kind='adam', lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False)
    assert updaters.plain_adam(rule)
    return updaters.optimizer_rule(rule)


def optimizer_step(lib, net, params, kind, kl_threshold=0.0, entropy_coeff=0.0, adv_stats=None, skip=None,
                   polyak=(None, None, 0, 0, 0.0)):
    import ctypes
    from tonic_amd import _lib
    rule = plain_adam_rule()
    _lib.check(lib.tonic_optimizer_step(
        params, net.sums.ptr(), net.slots.ptr(), net.state.ptr(), net.n, GRAD_SCALE, ctypes.byref(rule), kind,
        kl_threshold, entropy_coeff, adv_stats, net.info.ptr(), skip, *polyak, None), 'tonic_optimizer_step')


RESULT_NAMES = ('parameters', 'exp_avg', 'exp_avg_sq', 'state', 'info row')


@pytest.mark.parametrize('start', [0, 999], ids=['from-zero', 'from-999'])
@pytest.mark.parametrize('n', [1, 257, 32_769, 40_000])
def test_adam_step_is_optimizer_step(lib, n, start):
    """tonic_adam_step and tonic_optimizer_step with the plain-Adam rule from identical inputs — the PPO actor's
    statistics (kind 1) with an adv_stats row, an info row and a skip pointer holding 0: parameters, both moments,
    `state` and the info row equal bit for bit.  (Both are held to adam_statement elsewhere in this module and in
    test_gpu_optim_family.py; this pins the wrappers' translation of arguments.)  32 768 = 128 workgroups x 256
    threads: n = 32 769 is the first size at which one thread walks two elements."""
    p, m, v, sums = adam_case(n, 1, 21, warm=start != 0)
    adv = Guarded(np.array([0.0, 1.0, 0.0, 1.0], F32))
    flag = Guarded(np.array([0], np.int32))
    threshold, entropy_coeff = 0.0, 0.01                     # (kl = STATS[1] x scale > 0: the stop flag is raised)
    entry, family = Net(p, m, v, step=start), SlotNet(p, m, v, step=start)
    entry.load(sums[0])
    family.load(sums[0])
    adam_step(lib, entry, kind=1, kl_threshold=threshold, entropy_coeff=entropy_coeff, adv_stats=adv.ptr(),
              skip=flag.ptr())
    optimizer_step(lib, family, family.p.ptr(), 1, threshold, entropy_coeff, adv.ptr(), flag.ptr())
    got, want = family.read(), entry.read()
    for name, g, w in zip(RESULT_NAMES, got, want):
        assert same_bits(g, w), f'n = {n}: {name} of tonic_optimizer_step differ from tonic_adam_step'
    assert want[3].tolist() == [start + 1, 1, STATE_MARK, 0], want[3]
    assert same_bits(want[4], expected_row(1, entropy_coeff=entropy_coeff, kl_threshold=threshold)[0]), want[4]
    assert not same_bits(want[0], p) and not same_bits(want[1], m) and not same_bits(want[2], v)


@pytest.mark.parametrize('offset,n,total', [(4000, 1000, 5000), (0, 5000, 5000)], ids=['block-last', 'block-whole'])
def test_adam_polyak_step_is_optimizer_step(lib, offset, n, total):
    """tonic_adam_polyak_step and tonic_optimizer_step with the plain-Adam rule and a target, from identical inputs:
    the whole online buffer, both moments, `state`, the info row and EVERY target entry, inside and outside the
    block, equal bit for bit."""
    from tonic_amd import _lib
    coeff = 0.005
    p, m, v, sums = adam_case(n, 1, 22, warm=True)
    rng = np.random.RandomState([offset, n, total])
    online = rng.standard_normal(total).astype(F32)
    online[offset:offset + n] = p
    target = rng.standard_normal(total).astype(F32)
    entry, family = Net(p, m, v, step=3), SlotNet(p, m, v, step=3)
    buffers = []
    for net in (entry, family):
        net.load(sums[0])
        d_online, d_target = Guarded(online), Guarded(target)
        if net is entry:
            _lib.check(lib.tonic_adam_polyak_step(
                d_online.ptr(), net.sums.ptr(), net.m.ptr(), net.v.ptr(), net.state.ptr(), offset, n, total,
                GRAD_SCALE, LR, 0.9, 0.999, 1e-8, 4, net.info.ptr(), d_target.ptr(), coeff, None),
                'tonic_adam_polyak_step')
        else:
            optimizer_step(lib, net, d_online.ptr(offset), 4,
                           polyak=(d_target.ptr(), d_online.ptr(), total, offset, coeff))
        buffers.append((d_online.read(), d_target.read()) + net.read()[1:])
    names = ('online buffer', 'target buffer') + RESULT_NAMES[1:]
    for name, w, g in zip(names, *buffers):
        assert same_bits(g, w), f'{name} of tonic_optimizer_step differ from tonic_adam_polyak_step'
    got_online, got_target, _, _, state, info = buffers[0]
    outside = np.ones(total, bool)
    outside[offset:offset + n] = False
    assert same_bits(got_online[outside], online[outside]) and not same_bits(got_online[~outside], p)
    assert (bits(got_target) != bits(target)).mean() > 0.9, 'the targets moved, inside and outside the block'
    assert state.tolist() == [4, 0, STATE_MARK, 0] and same_bits(info, expected_row(4)[0])
    assert same_bits(entry.p.read(), p) and same_bits(family.p.read(), p)


# ------------------------------------------------------------------ one storage for the optimizer state

def assert_moment_views(optim, what):
    """`exp_avg` / `exp_avg_sq` are the first two state slots, and a step has been taken into them."""
    assert optim.slots.numel() == 2 * optim.count, what
    assert optim.exp_avg.data_ptr() == optim.slots.data_ptr(), what
    assert optim.exp_avg_sq.data_ptr() == optim.slots.data_ptr() + 4 * optim.count, what
    torch.cuda.synchronize()
    assert int(optim.state[0]) >= 1, f'{what}: no step was taken'
    slots = optim.slots.cpu().numpy()
    assert np.isfinite(slots).all() and slots[:optim.count].any() and slots[optim.count:].any(), what


@pytest.mark.parametrize('kind', ['ppo', 'ddpg', 'mpo'])
def test_default_agents_keep_their_moments_in_the_slots(lib, kind):
    """Default (plain Adam) PPO, DDPG and MPO agents after their first updates on `Synthetic` (O = 3, A = 2, two
    workers; PPO on 2 x 8 rows, the others at B = 17): what the pair launch and the fused off-policy iteration step
    through `exp_avg` / `exp_avg_sq` IS the updater's one `slots` tensor — for MPO's duals too."""
    import tonic_amd
    import tonic_amd.torch as tt
    O, A, W = 3, 2, 2
    env = tonic_amd.environments.distribute(lambda: tonic_amd.environments.Synthetic(O, A, max_episode_steps=5), 1, W)
    env.initialize(seed=5)
    if kind == 'ppo':
        agent = tt.agents.PPO(replay=tonic_amd.replays.Segment(size=8, batch_iterations=2))
    else:
        replay = tonic_amd.replays.Buffer(size=200, batch_iterations=1, batch_size=17, steps_before_batches=W * 4,
                                          steps_between_batches=W * 4)
        agent = (tt.agents.DDPG if kind == 'ddpg' else tt.agents.MPO)(replay=replay)
    agent.initialize(env.observation_space, env.action_space, seed=5)
    observations = env.start()
    for t in range(16 if kind == 'ppo' else 12):
        actions = agent.step(observations, t * W)
        observations, infos = env.step(actions)
        agent.update(**infos, steps=t * W)
    for name in ('actor_updater', 'critic_updater'):
        updater = getattr(agent, name)
        assert updater.plain and not updater.stock
        assert_moment_views(updater, f'{kind} {name}')
    if kind == 'mpo':
        assert_moment_views(agent.actor_updater.dual_optim, 'mpo duals')
    agent.close()


# ------------------------------------------------------------------ tonic_clip_grad_norm

def clip(lib, sums, workspace, scale, max_norm, skip=None):
    from tonic_amd import _lib
    _lib.check(lib.tonic_clip_grad_norm(sums.ptr(), sums.size - 8, scale, max_norm, skip, workspace.ptr(),
                                        4 * workspace.size, None), 'tonic_clip_grad_norm')


def ulps(got, want):
    """|got - want| in float32 ulps of `want` (a float64 value or array)."""
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want).astype(F32)).astype(np.float64)


@pytest.mark.parametrize('case', ['above', 'below', 'zero'])
@pytest.mark.parametrize('n', CLIP_SIZES)
def test_clip_grad_norm_sizes(lib, n, case):
    """Norm above max_norm (scaled), below it (coef = 1: the sums come back bit-identical) and an all-zero gradient
    (coef = max_norm / 1e-6 clamped to 1: unchanged, finite).  A partial workgroup that drops or doubles an element
    of its slice moves the norm by ~1 / n, far beyond the one ulp allowed."""
    scale = 1.0 / 1024
    rng = np.random.RandomState([n % 65521, 12])
    grads = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 1, size=n) / scale).astype(F32)
    if case == 'zero':
        grads[:] = 0.0
    norm = port.clip_grad_norm_f64(grads, scale, 1.0)[0]
    # (a third, not a quarter: a coefficient next to a power of two would be counted in the ulps of the binade below)
    max_norm = {'above': float(F32(norm / 3)), 'below': float(F32(norm * 4)), 'zero': 0.25}[case]
    norm, coef, want = port.clip_grad_norm_f64(grads, scale, max_norm)
    assert {'above': 0.33 < coef < 0.34, 'below': coef == 1.0, 'zero': coef == 1.0 and norm == 0.0}[case]
    host = np.concatenate([grads, STATS])
    words = lib.tonic_clip_workspace_bytes(n) // 4
    assert lib.tonic_clip_workspace_bytes(n) == 64 * 8 + 16           # kClipBlocks partials + {coef, norm}
    sums, workspace = Guarded(host), Guarded(np.full(words, NAN, F32))
    clip(lib, sums, workspace, scale, max_norm)
    got, report = sums.read(), workspace.read()[128:130]
    assert same_bits(got[n:], STATS), 'the statistic slots are not gradients'
    assert np.isfinite(got).all() and np.isfinite(report).all()
    norm_ulps = 0.0 if norm == 0.0 and report[1] == 0.0 else float(ulps(report[1], norm))
    coef_ulps = float(ulps(report[0], coef))
    nonzero = want != 0.0
    assert same_bits(got[:n][~nonzero], grads[~nonzero])
    element_ulps = float(ulps(got[:n][nonzero], want[nonzero]).max()) if nonzero.any() else 0.0
    print(f'clip n = {n} {case}: norm {norm_ulps:.2f} ulps, coef {coef_ulps:.2f} ulps, elements {element_ulps:.2f}')
    assert norm_ulps <= 1.0 and coef_ulps <= 1.0, (report, norm, coef)
    assert element_ulps <= 2.0
    if case != 'above':
        assert report[0] == 1.0 and same_bits(got[:n], grads)
    # a second launch on the same inputs: the same bits (fixed-order partial sums)
    again = Guarded(host)
    clip(lib, again, workspace, scale, max_norm)
    assert same_bits(again.read(), got) and same_bits(workspace.read()[128:130], report)
    # under the skip flag neither kernel reads or writes anything
    flag = Guarded(np.array([-1], np.int32))
    skipped, untouched = Guarded(host), Guarded(np.full(words, NAN, F32))
    clip(lib, skipped, untouched, scale, max_norm, skip=flag.ptr())
    assert same_bits(skipped.read(), host) and same_bits(untouched.read(), np.full(words, NAN, F32))
