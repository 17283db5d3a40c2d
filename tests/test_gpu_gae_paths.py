"""Every kernel behind `tonic_gae_lambda_returns`, at the shapes where its path begins, ends or wraps.

`gae_layout()` (csrc/gae.hip) picks one of five kernels by shape and by `chunks`.  Each case below names the kernel
it reaches and the constant that makes it so: whoever moves a constant moves the case with it.

| case | shapes (T x W), chunks                         | kernel                 | decided by                                   |
|------|------------------------------------------------|------------------------|----------------------------------------------|
| 1    | (1 | 7 | 8 | 21) x 16384 / 16389, chunks = 1   | gae_scan_kernel        | W >= 16384 (use_stream); kUnroll = 8: T = 1,  |
|      |                                                |                        | 7 remainder loop only, 8 unrolled only, 21 both |
| 1    | 21 x 65537, chunks = 0                         | gae_scan_kernel        | T <= 4 * 16 (no one-pass), then W >= 16384    |
| 1    | 65 x 65537, chunks = 0                         | gae_scan_kernel        | T > 64, so `W < 65536` in use_onepass decides: |
|      |                                                |                        | the 65536 threshold (bit-exact only above it)  |
| 1    | 100 x 70, 19 x 48, key gae_stream = 0          | gae_scan_kernel        | g_gae_stream == 0 (use_stream)               |
| 2    | T list x (16 | 48), chunks = 1                 | gae_stream16_kernel    | W % kStreamCols (16) == 0, W < 16384;        |
|      |                                                |                        | kStreamRows = 64: 1 .. 10 chunks, ragged first |
|      |                                                |                        | chunk (T % 64, T % 4); kStreamDepth = 4: ring  |
|      |                                                |                        | wraps from 5 chunks, pre-requests chunks 0..5  |
| 3    | 576 x 16                                       | gae_stream16_kernel    | plain flags, [kStreamDepth][kStreamRows / 4]  |
| 3    | 576 x 15; 576 x 16 with key gae_stream = 3     | gae_stream_kernel      | the same ring, dword helpers                 |
| 4    | T list x (1 | 15 | 17 | 33), chunks = 1        | gae_stream_kernel      | W % 16 != 0: ragged last workgroup           |
| 5    | 128 x W, chunks = 0                            | stream16 / stream      | T <= seg_waves(W) * kSegRowsPerWave = 8 * 16  |
| 5    | (129 .. 1029) x (1 | 64 | 65 | 70), chunks 0,3,8 | gae_onepass_kernel<8> | T > 128, W < kWideColumns = 8192; 64-column   |
|      |                                                |                        | tiles: W = 64 one, 65 / 70 two (ragged)       |
| 5    | 64 x (8192 | 8195), chunks = 0                 | stream16 / stream      | T <= 4 * 16 (seg_waves = 4 from W = 8192)    |
| 5    | (65 | 81 | 200) x (8192 | 8195), chunks 0,3,8  | gae_onepass_kernel<4>  | T > 64, 8192 <= W < 65536; 8195: ragged tile  |
| 6    | 10245 x 70 (81 segments of 128 rows)           | gae_onepass_kernel<8>  | kFarSegments = 64: segments 0 .. 15 have more |
| 6    | 4483 x 8195 (71 segments of 64 rows)           | gae_onepass_kernel<4>  | than 64 later ones and wait for a hand-over  |
| 7    | one-pass shapes of 5 and 6, lambda = 0         | gae_onepass_kernel     | step 4's replay: the chain's operation order |
| 8    | 400 x (5 | 70), chunks = 0 (4 segments)        | gae_onepass_kernel<8>  | maps with b = 0 / b = 1; write_adv_stats     |
| 9    | one shape per kernel                           | all five + gae_stats   | block_sums -> gae_stats_kernel -> moments    |
| 10   | 257 x 70 and 100 x 70 in shards of 32 + 38     | adv_stats_from_moments | {sum, sum_sq, -min, max, count} merged       |

T list = {1, 3, 4, 5, 63, 64, 65} + {64 k, 64 k + 1 : k = 2 .. 9}.

References.  The exact chains (`chunks = 1`, or T too short for the one-pass form) equal `numpy_port.lambda_returns`
bit for bit and their advantages equal `returns - values` bit for bit.  The one-pass form re-associates the chain, so
it is held to a float64 evaluation of the same recurrence with the kernel's float32 scalars
(`numpy_port.lambda_returns_f64`): per COLUMN, |error| <= 1e-5 x max |reference| of that column, no floor — column j
carries rewards, values and next-values scaled by 10 ** (j % 7 - 3), so a wrong carry in a small column cannot hide
behind a large neighbour.  1e-5 is the north star's figure (`assert_grads_close`); the float32 chain itself reaches
2.9e-6 on these inputs (gamma = lambda = 1), a float32 emulation of the one-pass composition 5.5e-7.

Statistics: float64 two-pass mean and population std of the float32 advantages the kernel RETURNED, to 1e-6 relative
(the kernel accumulates in float64; |mean| / std <= 1e3 here, so s1 / n - mean^2 loses ~1e-10); moments' sum and sum
of squares to 1e-12 relative against math.fsum, min / max / count exact.

No input here holds a NaN or an infinity: the one-pass carries use the all-ones word (a NaN) as "not yet written".

Every one-pass test prints the largest per-column |error| / max |reference| it met (`pytest -s`).  Measured on the
MI355X, largest per family: <8> boundaries 5.3e-7, <4> boundaries 6.5e-7, extremes 4.0e-7, <8> past the stash 7.2e-7,
<4> past the stash 7.7e-7 — the hardware agrees with the CPU emulation's order of magnitude, a factor 13 inside 1e-5.
"""
import contextlib
import functools
import math

import numpy as np
import pytest

import numpy_port as port
from test_gpu_parity import dev, run_gae

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

PAIRS = [(0.99, 0.97), (0.9, 0.5), (1.0, 1.0), (0.99, 0.0)]       # the goldens' four (gamma, lambda)
DENSITIES = [0.0, 1e-3, 0.15]
T_LIST = [1, 3, 4, 5, 63, 64, 65] + [64 * k + r for k in range(2, 10) for r in (0, 1)]
COLUMN_TOL = 1e-5


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


@contextlib.contextmanager
def gae_stream_key(lib, value):
    """Tuning key gae_stream for the duration of a block: 0 = lane = column scan, 3 = dword helpers.  (2 and 4 are
    developer probes that leave outputs unwritten: never set here.)"""
    from tonic_amd import _lib
    assert value in (0, 3)
    _lib.check(lib.tonic_set_tuning(b'gae_stream', value), 'tuning')
    try:
        yield
    finally:
        _lib.check(lib.tonic_set_tuning(b'gae_stream', 1), 'tuning')


# Reuse is by position: a test asks for one (T, W, density) at a time and the parametrised lists below keep equal
# triples NEXT to each other (the past-the-stash lists are ordered density first for that reason), so two entries
# are enough and a large set (4483 x 8195: 735 MB, ~2 s to draw) is drawn once per density, not once per test.
# Reordering those lists costs time only, never correctness: a miss draws the same numbers again.
@functools.lru_cache(maxsize=2)
def make_inputs(T, W, density, seed=0):
    """-> next_values, rewards, resets, terminations, values (read-only).  Column j is scaled by 10 ** (j % 7 - 3);
    a transition resets with probability `density`, half of the resets terminate."""
    rng = np.random.default_rng([T, W, int(round(density * 1e6)), seed])
    scale = (10.0 ** (np.arange(W) % 7 - 3)).astype(np.float32)
    nv, rew, val = (rng.standard_normal((T, W), dtype=np.float32) * scale for _ in range(3))
    if density > 0:
        hit = rng.random((T, W), dtype=np.float32) < density
        term = (hit & (rng.random((T, W), dtype=np.float32) < 0.5)).astype(np.float32)
        rst = hit.astype(np.float32)
    else:
        rst, term = np.zeros((T, W), np.float32), np.zeros((T, W), np.float32)
    out = (nv, rew, rst, term, val)
    for a in out:
        a.setflags(write=False)
    return out


def column_error(got, ref64):
    """Largest |got - ref| / max |ref| over the columns, each column against its own maximum (no floor)."""
    assert got.dtype == np.float32 and ref64.dtype == np.float64 and got.shape == ref64.shape
    assert np.isfinite(got).all(), 'an output element is NaN / inf (never written?)'
    err, scale = np.zeros(got.shape[1]), np.zeros(got.shape[1])
    for t0 in range(0, got.shape[0], 512):                        # (blocks: no [T, W] float64 temporaries)
        err = np.maximum(err, np.abs(got[t0:t0 + 512] - ref64[t0:t0 + 512]).max(axis=0))
        scale = np.maximum(scale, np.abs(ref64[t0:t0 + 512]).max(axis=0))
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def check_onepass(what, got_ret, got_adv, val, ref64):
    """Per-column bound on the returns; advantages are `returns - values` of the kernel's own returns."""
    worst = column_error(got_ret, ref64)
    print(f'one-pass per-column error: {what}: {worst:.3e}')
    assert worst <= COLUMN_TOL, f'{what}: per-column error {worst:.3e} > {COLUMN_TOL:g}'
    assert np.array_equal(got_adv, got_ret - val), f'{what}: advantages != returns - values'
    return worst


def check_exact(what, inputs, gamma, lam, got_ret, got_adv):
    nv, rew, rst, term, val = inputs
    want = port.lambda_returns(nv, rew, rst, term, gamma, lam)
    assert np.array_equal(got_ret, want), f'{what}: returns differ from the float32 chain'
    assert np.array_equal(got_adv, want - val), f'{what}: advantages != returns - values'


def check_stats(what, adv, stats, moments=None):
    """stats[0:2] against the float64 two-pass mean / population std of the RETURNED advantages; flags by
    segments.py:43-46; moments = {sum, sum_sq, -min, max, count}."""
    a = adv.astype(np.float64).reshape(-1)
    mean = a.sum() / a.size                                       # (pairwise float64 sums: ~1e-15)
    std = math.sqrt(((a - mean) ** 2).sum() / a.size)
    constant = adv.min() == adv.max()
    if constant:
        assert stats[1] == 0.0, f'{what}: std of a constant array must be exactly 0'
        np.testing.assert_allclose(stats[0], mean, rtol=1e-6, atol=0, err_msg=what)
    else:
        np.testing.assert_allclose(stats[:2], [mean, std], rtol=1e-6, atol=0, err_msg=what)
    assert stats[2] == (1.0 if not adv.any() else 0.0), f'{what}: all_zero flag'
    assert stats[3] == (0.0 if constant else 1.0), f'{what}: normalise flag'
    if moments is not None:
        np.testing.assert_allclose(moments[:2], [math.fsum(a), math.fsum(a * a)], rtol=1e-12, atol=0,
                                   err_msg=what)
        assert moments[2] == -float(adv.min()) and moments[3] == float(adv.max()), f'{what}: -min / max'
        assert moments[4] == adv.size, f'{what}: count'


# ------------------------------------------------------------------ 1. gae_scan_kernel, exact

@pytest.mark.parametrize('T,W,chunks', [(1, 16384, 1), (7, 16389, 1), (8, 16389, 1), (21, 16389, 1),
                                        (21, 65537, 0), (65, 65537, 0)])
def test_scan_kernel_exact(lib, T, W, chunks):
    """Lane = column scan by width: kUnroll = 8 rows per batch — T = 1 and 7 run the remainder loop alone, 8 the
    unrolled loop alone, 21 both (two batches + five rows); W = 16389 and 65537 leave a ragged last workgroup.
    65 x 65537 with chunks = 0 is long enough for the one-pass form (T > 64): only `W < 65536` in use_onepass keeps
    it on the exact chain, so this case fails bit-exactness if that threshold moves up."""
    for density in (0.0, 0.15):
        inputs = make_inputs(T, W, density)
        for gamma, lam in PAIRS:
            ret, adv, stats = run_gae(lib, *inputs, gamma, lam, chunks)
            check_exact(f'scan {T}x{W} d={density} ({gamma}, {lam})', inputs, gamma, lam, ret, adv)


@pytest.mark.parametrize('T,W', [(100, 70), (19, 48)])
def test_scan_kernel_exact_by_tuning_key(lib, T, W):
    """The same kernel at small W (tuning key gae_stream = 0), bit for bit what the streamed kernels give."""
    for density in DENSITIES:
        inputs = make_inputs(T, W, density)
        for gamma, lam in PAIRS:
            with gae_stream_key(lib, 0):
                ret, adv, stats = run_gae(lib, *inputs, gamma, lam, 1)
            what = f'scan (key) {T}x{W} d={density} ({gamma}, {lam})'
            check_exact(what, inputs, gamma, lam, ret, adv)
            ret_s, adv_s, stats_s = run_gae(lib, *inputs, gamma, lam, 1)
            assert np.array_equal(ret, ret_s) and np.array_equal(adv, adv_s), what
            np.testing.assert_allclose(stats, stats_s, rtol=1e-6, atol=0, err_msg=what)


# ------------------------------------------------- 2. / 4. the streamed kernels, exact, every chunk count

def stream_densities(T):
    return (0.0, 0.15, 1e-3) if T == 577 else (0.0, 0.15)


@pytest.mark.parametrize('W', [16, 48])
@pytest.mark.parametrize('T', T_LIST)
def test_stream16_kernel_exact(lib, T, W):
    """gae_stream16_kernel (W % 16 == 0): 1 .. 10 chunks of kStreamRows = 64 rows through a ring of kStreamDepth = 4
    slots, the first chunk ragged by T % 64 and T % 4; W = 48 is three workgroups."""
    for density in stream_densities(T):
        inputs = make_inputs(T, W, density)
        for gamma, lam in PAIRS:
            ret, adv, stats = run_gae(lib, *inputs, gamma, lam, 1)
            check_exact(f'stream16 {T}x{W} d={density} ({gamma}, {lam})', inputs, gamma, lam, ret, adv)


@pytest.mark.parametrize('W', [1, 15, 17, 33])
@pytest.mark.parametrize('T', T_LIST)
def test_stream_kernel_exact(lib, T, W):
    """gae_stream_kernel (dword helpers, W % 16 != 0): the same pipeline with a ragged last workgroup."""
    for density in stream_densities(T):
        inputs = make_inputs(T, W, density)
        for gamma, lam in PAIRS:
            ret, adv, stats = run_gae(lib, *inputs, gamma, lam, 1)
            check_exact(f'stream {T}x{W} d={density} ({gamma}, {lam})', inputs, gamma, lam, ret, adv)


# ------------------------------------------------------------------ 3. the plain-flag ring

@pytest.mark.parametrize('W,key', [(16, None), (15, None), (16, 3)], ids=['stream16', 'stream-w15', 'stream-key3'])
@pytest.mark.parametrize('c', range(9))
def test_stream_plain_flag_ring(lib, c, W, key):
    """Nine chunks with ONE reset cell, in chunk c (position j of chunk k is time row T - 1 - 64 k - j).  Every
    other row group is plain, and the plain flags of chunk c share their ring slot with chunks c - 4 and c + 4:
    a flag left over from four chunks earlier makes the chain skip the reset.  The cell's row group
    ((7 c + 3) % 64 // 4 = 0, 2, 4, 6, 7, 9, 11, 13, 14) and column ((5 c + 1) % W) move with c."""
    T = 9 * 64
    nv, rew, _, _, val = make_inputs(T, W, 0.0)
    row, col = T - 1 - 64 * c - (7 * c + 3) % 64, (5 * c + 1) % W
    for terminates in (False, True):
        rst, term = np.zeros((T, W), np.float32), np.zeros((T, W), np.float32)
        rst[row, col] = 1.0
        term[row, col] = 1.0 if terminates else 0.0
        inputs = (nv, rew, rst, term, val)
        with (gae_stream_key(lib, key) if key is not None else contextlib.nullcontext()):
            ret, adv, stats = run_gae(lib, *inputs, 0.99, 0.97, 1)
        # the cell matters: without it the column's earlier returns differ
        plain = port.lambda_returns(nv, rew, 0 * rst, 0 * term, 0.99, 0.97)
        assert not np.array_equal(plain[:row + 1, col], port.lambda_returns(*inputs[:4], 0.99, 0.97)[:row + 1, col])
        check_exact(f'flag ring W={W} key={key} chunk {c} terminates={terminates}', inputs, 0.99, 0.97, ret, adv)


# ------------------------------------------------------------------ 5. one-pass boundaries

def run_boundary(lib, T, W, seg_rows, family, densities=DENSITIES):
    worst = 0.0
    for density in densities:
        inputs = make_inputs(T, W, density)
        for gamma, lam in PAIRS:
            what = f'{family} {T}x{W} d={density} ({gamma}, {lam})'
            ret, adv, stats = run_gae(lib, *inputs, gamma, lam, 0)
            if T <= seg_rows or lam == 0.0:
                # still the exact chain / case 7: the carry is multiplied by 0, the chain's bits
                check_exact(what, inputs, gamma, lam, ret, adv)
            if T > seg_rows:
                ref64 = port.lambda_returns_f64(*inputs[:4], gamma, lam)
                worst = max(worst, check_onepass(what, ret, adv, inputs[4], ref64))
            check_stats(what, adv, stats)
            for chunks in (3, 8):                                           # the segment length is fixed
                ret_c, adv_c, stats_c = run_gae(lib, *inputs, gamma, lam, chunks)
                assert np.array_equal(ret_c, ret) and np.array_equal(adv_c, adv), (what, chunks)
                assert np.array_equal(stats_c, stats), (what, chunks)
    if T > seg_rows:
        print(f'one-pass per-column error, worst of {family} {T}x{W}: {worst:.3e}')


@pytest.mark.parametrize('W', [1, 64, 65, 70])
@pytest.mark.parametrize('T', [128, 129, 130, 144, 145, 255, 257, 1029])
def test_onepass8_boundaries(lib, T, W):
    """gae_onepass_kernel<8> from T = 129 (T = 128 is still the exact chain): a last segment of 1, 2, 16, 17 and
    127 rows, 2, 3 and 9 segments, one and two column tiles (ragged at W = 65, 70).
    Largest per-column error measured on the MI355X: 5.3e-7 (1029 x 70, no resets, (0.99, 0.97)); 5.1e-7 at
    gamma = lambda = 1, 1.2e-7 at (0.9, 0.5), 1.0e-7 at lambda = 0.  Each run prints its own (`pytest -s`)."""
    run_boundary(lib, T, W, 128, 'onepass<8>')


@pytest.mark.parametrize('density', DENSITIES)
@pytest.mark.parametrize('W', [8192, 8195])
@pytest.mark.parametrize('T', [64, 65, 81, 200])
def test_onepass4_boundaries(lib, T, W, density):
    """gae_onepass_kernel<4> from W = 8192 and T = 65 (T = 64 is still the exact chain): a last segment of 1, 17
    and 8 rows, a ragged last tile at W = 8195.
    Largest per-column error measured on the MI355X: 6.5e-7 (65 x 8192, density 1e-3, gamma = lambda = 1); 5.8e-7 at
    (0.99, 0.97), 1.5e-7 at (0.9, 0.5), 1.1e-7 at lambda = 0.  Each run prints its own (`pytest -s`)."""
    run_boundary(lib, T, W, 64, 'onepass<4>', [density])


# ------------------------------------------------------------------ 8. extremes across 4 segments

@pytest.mark.parametrize('W', [5, 70])
def test_onepass_extremes(lib, W):
    """T = 400 (four 128-row segments): maps that forget the carry (b = 0), a chain that never resets, and the
    constant / all-zero advantage flags folded from several workgroups' partial moments.
    Largest per-column error measured on the MI355X: 4.0e-7 (nothing ever resets, gamma = lambda = 1, W = 70);
    7.5e-8 with every transition a time-out, exactly 0 with every transition terminating.  Each run prints its own."""
    T = 400
    nv, rew, _, _, val = make_inputs(T, W, 0.0)
    zeros, ones = np.zeros((T, W), np.float32), np.ones((T, W), np.float32)
    for what, rst, term, gamma, lam in [('every transition a time-out', ones, zeros, 0.99, 0.97),
                                        ('every transition terminating', ones, ones, 0.99, 0.97),
                                        ('nothing ever resets', zeros, zeros, 1.0, 1.0)]:
        ret, adv, stats, mom = run_gae(lib, nv, rew, rst, term, val, gamma, lam, 0, moments=True)
        ref64 = port.lambda_returns_f64(nv, rew, rst, term, gamma, lam)
        check_onepass(f'{what} 400x{W}', ret, adv, val, ref64)
        check_stats(f'{what} 400x{W}', adv, stats, mom)
    # b = 0 everywhere: nothing is re-associated, the chain's bits
    for rst, term in ((ones, zeros), (ones, ones)):
        ret, adv, stats = run_gae(lib, nv, rew, rst, term, val, 0.99, 0.97, 0)
        check_exact(f'b = 0 400x{W}', (nv, rew, rst, term, val), 0.99, 0.97, ret, adv)
    # all-zero inputs: all_zero set, no normalisation
    ret, adv, stats, mom = run_gae(lib, zeros, zeros, zeros, zeros, zeros, 0.99, 0.97, 0, moments=True)
    assert not ret.any() and not adv.any()
    assert stats[0] == 0.0 and stats[1] == 0.0 and stats[2] == 1.0 and stats[3] == 0.0
    assert np.array_equal(mom, [0.0, 0.0, 0.0, 0.0, T * W])
    # constant non-zero advantage (returns == rewards == 1, values == 0): std exactly 0, normalisation skipped
    ret, adv, stats, mom = run_gae(lib, zeros, ones, ones, ones, zeros, 0.99, 0.97, 0, moments=True)
    assert np.array_equal(ret, ones) and np.array_equal(adv, ones)
    assert stats[0] == 1.0 and stats[1] == 0.0 and stats[2] == 0.0 and stats[3] == 0.0
    assert np.array_equal(mom, [T * W, T * W, -1.0, 1.0, T * W])


# ------------------------------------------------------------------ 9. statistics and moments on every path

@pytest.mark.parametrize('T,W,chunks,key', [(21, 16389, 1, None), (100, 70, 1, 0), (129, 48, 1, None),
                                            (129, 33, 1, None), (129, 48, 1, 3), (257, 70, 0, None),
                                            (81, 8195, 0, None)],
                         ids=['scan', 'scan-key0', 'stream16', 'stream', 'stream-key3', 'onepass8', 'onepass4'])
def test_statistics_and_moments(lib, T, W, chunks, key):
    """{mean, std, all_zero, normalise} and {sum, sum_sq, -min, max, count} of every kernel's partial moments
    (block_sums -> gae_stats_kernel), against float64 two-pass values of the advantages the kernel returned; the
    call without a moments pointer gives the same statistics."""
    for density in (0.0, 0.15):
        inputs = make_inputs(T, W, density)
        for gamma, lam in PAIRS[:2]:
            what = f'stats {T}x{W} chunks={chunks} key={key} d={density} ({gamma}, {lam})'
            with (gae_stream_key(lib, key) if key is not None else contextlib.nullcontext()):
                ret, adv, stats, mom = run_gae(lib, *inputs, gamma, lam, chunks, moments=True)
                ret_n, adv_n, stats_n = run_gae(lib, *inputs, gamma, lam, chunks)
            check_stats(what, adv, stats, mom)
            assert np.array_equal(stats_n, stats) and np.array_equal(adv_n, adv), what


# ------------------------------------------------------------------ 10. rank merge without ranks

def merged_stats(lib, moments):
    """What Segment.compute_returns does with the ranks' moment vectors (SUM of [0, 1, 4], MAX of [2, 3]) with plain
    torch ops, then tonic_advantage_stats_from_moments."""
    from tonic_amd import _lib
    parts = [torch.as_tensor(m, dtype=torch.float64).cuda() for m in moments]
    merged = torch.empty(5, dtype=torch.float64, device='cuda')
    merged[0:2] = sum(p[0:2] for p in parts)
    merged[4:5] = sum(p[4:5] for p in parts)
    merged[2:4] = torch.stack([p[2:4] for p in parts]).max(dim=0).values
    stats = torch.full((4,), float('nan'), device='cuda')
    _lib.check(lib.tonic_advantage_stats_from_moments(merged.data_ptr(), stats.data_ptr(), None), 'merge')
    torch.cuda.synchronize()
    return stats.cpu().numpy()


@pytest.mark.parametrize('T,chunks', [(257, 0), (100, 1)], ids=['onepass', 'chain'])
@pytest.mark.parametrize('zero_shard', [None, 0, 1, 'both'])
def test_rank_merge_of_moments(lib, T, chunks, zero_shard):
    """W = 70 as two worker shards of 32 and 38 columns, merged the way the ranks merge them: the whole batch's
    statistics to 1e-6 relative, the same flags — also when one shard's (or every shard's) advantages are all zero."""
    W, cut = 70, 32
    inputs = [a.copy() for a in make_inputs(T, W, 0.15)]
    zeroed = {None: slice(0, 0), 0: slice(0, cut), 1: slice(cut, W), 'both': slice(0, W)}[zero_shard]
    for a in inputs:
        a[:, zeroed] = 0.0
    ret, adv, stats, mom = run_gae(lib, *inputs, 0.99, 0.97, chunks, moments=True)
    check_stats(f'whole batch, zero shard {zero_shard}', adv, stats, mom)
    shards = []
    for k, cols in enumerate((slice(0, cut), slice(cut, W))):
        part = [np.ascontiguousarray(a[:, cols]) for a in inputs]
        ret_k, adv_k, stats_k, mom_k = run_gae(lib, *part, 0.99, 0.97, chunks, moments=True)
        check_stats(f'shard {k}, zero shard {zero_shard}', adv_k, stats_k, mom_k)
        assert stats_k[2] == (1.0 if zero_shard in (k, 'both') else 0.0)
        # a column's returns do not depend on its neighbours
        assert np.array_equal(ret_k, ret[:, cols]) and np.array_equal(adv_k, adv[:, cols])
        shards.append(mom_k)
        # one shard's vector alone gives that shard's own statistics
        assert np.array_equal(merged_stats(lib, [mom_k]), stats_k)
    got = merged_stats(lib, shards)
    np.testing.assert_allclose(got[:2], stats[:2], rtol=1e-6, atol=0)
    assert np.array_equal(got[2:], stats[2:]), (got, stats)
    assert got[2] == (1.0 if zero_shard == 'both' else 0.0) and got[3] == (0.0 if zero_shard == 'both' else 1.0)


# ------------------------------------------------------------------ 7. lambda = 0 on the one-pass path

@pytest.mark.parametrize('T,W', [(1029, 65), (200, 8195)])
def test_onepass_lambda_zero_is_the_chain(lib, T, W):
    """With lambda = 0 the carry is multiplied by zero, so the one-pass replay (step 4) must give the float32
    chain's returns BIT FOR BIT: this pins its operation order, which no tolerance can."""
    inputs = make_inputs(T, W, 1e-3)
    ret, adv, stats = run_gae(lib, *inputs, 0.99, 0.0, 0)
    check_exact(f'lambda = 0, {T}x{W}', inputs, 0.99, 0.0, ret, adv)


# ------------------------------------------------------------------ 6. past the LDS stash

def run_past_stash(lib, T, W, density, gamma, lam, family):
    inputs = make_inputs(T, W, density)
    what = f'{family} {T}x{W} d={density} ({gamma}, {lam})'
    d = [dev(a) for a in inputs]                 # one upload for the three launches
    first = run_gae(lib, *d, gamma, lam, 0, moments=True)
    ref64 = port.lambda_returns_f64(*inputs[:4], gamma, lam)
    check_onepass(what, first[0], first[1], inputs[4], ref64)
    check_stats(what, first[1], first[2])
    assert first[3][2] == -float(first[1].min()) and first[3][3] == float(first[1].max())
    assert first[3][4] == T * W
    # the walk may start from different segments run to run and must not show it
    for again in range(2):
        other = run_gae(lib, *d, gamma, lam, 0, moments=True)
        for a, b, name in zip(first, other, ('returns', 'advantages', 'stats', 'moments')):
            assert np.array_equal(a, b), f'{what}: {name} differ between launches'


@pytest.mark.parametrize('density,gamma,lam', [(0.0, 0.99, 0.97), (0.0, 1.0, 1.0), (1e-3, 0.99, 0.97),
                                               (1e-3, 1.0, 1.0)])
def test_onepass8_past_the_stash(lib, density, gamma, lam):
    """T = 80 x 128 + 5: 81 segments.  A workgroup stashes the maps of kFarSegments = 64 later segments; segments
    0 .. 15 have more, and wait for the `inclusive` hand-over of the segment 64 ahead (need == 2).
    Largest per-column error measured on the MI355X: 7.2e-7 (no resets, gamma = lambda = 1); 4.5e-7 at (0.99, 0.97).
    Each run prints its own (`pytest -s`)."""
    run_past_stash(lib, 80 * 128 + 5, 70, density, gamma, lam, 'onepass<8> past the stash')


@pytest.mark.parametrize('density,gamma,lam', [(0.0, 0.99, 0.97), (0.0, 1.0, 1.0), (1e-3, 0.99, 0.97),
                                               (1e-3, 1.0, 1.0)])
def test_onepass4_past_the_stash(lib, density, gamma, lam):
    """T = 70 x 64 + 3: 71 segments of the 4-wave form, 129 column tiles (the last one ragged); segments 0 .. 5
    wait for a hand-over.  The largest case of the module; its input draw and float64 reference dominate its time.
    Largest per-column error measured on the MI355X: 7.7e-7 (no resets, gamma = lambda = 1); 5.9e-7 at (0.99, 0.97).
    Measured time on the MI355X host: 1.5 s for the slowest of the four cases (the one that draws the inputs), 0.6 s
    for one that reuses them.  Each run prints its own error (`pytest -s`)."""
    run_past_stash(lib, 70 * 64 + 3, 8195, density, gamma, lam, 'onepass<4> past the stash')


@pytest.mark.parametrize('T,W', [(80 * 128 + 5, 70), (70 * 64 + 3, 8195)])
def test_onepass_lambda_zero_past_the_stash(lib, T, W):
    """The same past the LDS stash: the hand-over feeds a carry that lambda = 0 discards."""
    inputs = make_inputs(T, W, 1e-3)
    ret, adv, stats = run_gae(lib, *inputs, 0.99, 0.0, 0)
    check_exact(f'lambda = 0, {T}x{W}', inputs, 0.99, 0.0, ret, adv)
