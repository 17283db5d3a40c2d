"""The GEMM block's reference and case table on the host (tests/gemm_block_ref.py): the float64 reference against a
triple loop in Python integers, the exactness condition of every table entry, and the table's coverage of the
kernels' path selection as restated there — an unreached path is named."""
from fractions import Fraction

import numpy as np
import pytest

import gemm_block_ref as ref


def triple_loop(mode, p, z=0):
    """C and colsum of a problem in exact rational arithmetic (act none / ReLU), element by element."""
    f = p.form
    frac = lambda x: Fraction(float(x))
    a, b = p.a.logical(z), p.b.logical(z)
    c = [[None] * p.N for _ in range(p.M)]
    for m in range(p.M):
        for n in range(p.N):
            total = Fraction(0)
            for k in range(p.K):
                x = a[m][k] if mode[0] == 'N' else a[k][m]
                y = b[n][k] if mode[1] == 'T' else b[k][n]
                total += frac(x) * frac(y)
            v = frac(f['alpha']) * total
            if p.bias is not None:
                v += frac(p.bias.logical(z)[0][n])
            if f['act'] == ref.ACT_RELU:
                v = max(v, Fraction(0))
            if p.mask is not None:
                s = frac(p.mask.logical(z)[m][n])
                if f['mask_act'] == ref.ACT_TANH:
                    v = v * (1 - s * s)
                elif f['mask_act'] == ref.ACT_ELU:
                    v = v if s > 0 else v * (s + 1)
                else:
                    v = v if s > 0 else Fraction(0)
            if f['accumulate']:
                v += frac(p.c.logical(z)[m][n])
            c[m][n] = v
    colsum = None
    if mode == 'TN':
        colsum = [sum(frac(a[k][m]) for k in range(p.K)) for m in range(p.M)]
    return c, colsum


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('case', [ref.Case('tiny_full', 3, 5, 7, 'full', pa='odd', pb='product', batch=2),
                                  ref.Case('tiny_tanh_mask', 2, 1, 19, 'tanh_mask', pc='odd', pm='tight'),
                                  ref.Case('tiny_elu_mask', 5, 2, 1, 'elu_mask', pa='wide', share_bias=True, batch=2)],
                         ids=lambda c: c.name)
def test_reference_equals_a_triple_loop_in_integers(mode, case):
    p = ref.make_problem(mode, case, seed=3)
    for z in range(case.batch):
        c, colsum = triple_loop(mode, p, z)
        assert [[Fraction(float(x)) for x in row] for row in p.ref_c[z]] == c
        if mode == 'TN':
            assert [Fraction(float(x)) for x in p.ref_colsum[z]] == colsum


def test_pitches_and_images():
    from tonic_amd import _lib
    lib = _lib.load()
    for cols in range(1, 300):
        assert ref.weight_ld(cols) == lib.tonic_mlp_weight_stride(cols)
    for width in ref.MN_POOL + ref.K_POOL:
        assert ref.pitch_of('tight', width) == width
        assert ref.pitch_of('odd', width) % 2 == 1 and ref.pitch_of('odd', width) >= width + 3
        assert ref.pitch_of('wide', width) % 32 == 0 and 0 <= ref.pitch_of('wide', width) - width < 32
        assert ref.pitch_of('product', width) >= width and ref.pitch_of('product', width) % 32 != 0
    assert ref.pitch_of('wide', 37) == 64
    p = ref.make_problem('TN', ref.Case('image', 5, 3, 7, 'full', pa='odd', pb='product', pc='odd', batch=2,
                                        share_b=True))
    for op, rows, cols in ((p.a, 7, 5), (p.b, 7, 3), (p.c, 5, 3), (p.mask, 5, 3), (p.bias, 1, 3), (p.colsum, 1, 5)):
        assert op.image.shape[1:] == (rows + 1, op.pitch) and op.pitch >= cols
        assert np.isfinite(op.logical(0)).all() or op is p.colsum
        outside = np.ones(op.image.shape, bool)
        outside[:, :rows, :cols] = False
        assert np.isnan(op.image[outside]).all() and outside.sum() > 0
        assert op.stride == (0 if op is p.b else (rows + 1) * op.pitch) and (op.stride == 0 or op.stride >= rows * op.pitch)
    assert p.b.image.shape[0] == 1 and p.a.image.shape[0] == 2
    one = p.slice(1)
    assert one.batch == 1 and np.array_equal(one.a.logical(0), p.a.logical(1)) and one.ref_c[0] is p.ref_c[1]


def test_exactness_condition_holds_for_every_table_entry():
    """Inputs on the integer / eighths grids, K inside the range, the float64 reference a float32 (asserted in
    make_problem), and dimensions from the pools only (one tile-count case apart)."""
    every = [(mode, c) for mode in ref.MODES for c in ref.TABLE]
    every += [(mode, c) for _, mode, _, _, members in ref.GROUPS for c in members]
    for mode, c in every:
        assert (c.M, c.N, c.K) == ref.BIG or (c.M in ref.MN_POOL and c.N in ref.MN_POOL and c.K in ref.K_POOL), c
        assert c.K * 16 < 2 ** 24 and c.K <= ref.K_EXACT_MAX
        form = ref.FORMS[c.form]
        assert form['alpha'] in (1.0, 0.5) and form['act'] in (ref.ACT_NONE, ref.ACT_RELU)
        if (c.M, c.N, c.K) == ref.BIG and mode != 'NT':
            continue                                   # (same draws' ranges; the GPU test builds it anyway)
        p = ref.make_problem(mode, c)
        for op in (p.a, p.b, p.bias) + ((p.c,) if form['accumulate'] else ()):
            if op is not None:
                x = op.image[:, :op.rows, :op.cols]
                assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 4
        if p.mask is not None:
            x = p.mask.image[:, :p.M, :p.N] * 8
            assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8
            assert p.mask.pitch != p.c.pitch or c.pm == c.pc, 'ldmask must differ from ldc where the kinds differ'


def test_table_reaches_every_path():
    missing = sorted(ref.required_paths() - ref.reached_paths())
    assert not missing, 'paths of gemm16.hip no table case reaches:\n  ' + '\n  '.join(missing)
    # ... and the check can fail: without its K = 1029 cases the table loses the generic kernel's second round
    fewer = [c for c in ref.TABLE if c.K != 1029]
    assert 'NT: rounds=2' in ref.required_paths() - ref.reached_paths(fewer)
    assert 'TN group: wide form' in ref.required_paths() - ref.reached_paths(groups=[g for g in ref.GROUPS
                                                                                     if len(g[4]) <= 4])


def test_path_selection_restates_the_launch_code():
    """Spot values worked out by hand from gemm16.hip (waves_per_tile, per_block, first[], the TN tile's choices)."""
    assert [ref.waves_per_tile(K, 1) for K in (1, 16, 17, 32, 41, 49, 69, 256, 1029)] == [1, 1, 2, 2, 4, 4, 8, 16, 16]
    assert ref.waves_per_tile(256, 512) == 4 and ref.waves_per_tile(1024, 4096) == 16
    assert ref.generic_path([(33, 33)], 15, 1) == dict(S=1, per_block=4, rounds=1, part_empty=True, first=[0, 2])
    assert ref.generic_path([(17, 33), (33, 1), (2, 15), (31, 97)], 32, 1)['first'] == [0, 2, 4, 5, 9]
    assert ref.generic_path([(17, 33)], 1029, 1)['rounds'] == 2 and ref.generic_path([(17, 33)], 1024, 1)['rounds'] == 1
    p = ref.tn_path(37, 33, 19, 64, 33, True)
    assert p['forms'] == {(False, True), (True, False)} and p['vector_partial'] and p['owner'] == 1 and p['blocks'] == 4
    assert [ref.tn_path(1, 1, K, 1, 1, False)['owner'] for K in (15, 19, 41, 49, 69, 256)] == [0, 1, 2, 3, 0, None]
    assert [ref.tn_path(1, 1, K, 1, 1, False)['rounds'] for K in (256, 257, 271, 272, 528)] == [1, 1, 1, 2, 2]
    assert ref.kernel_of('TN', ref.FORMS['plain_acc']) == 'tn' and ref.kernel_of('TN', ref.FORMS['bias']) == 'generic'
    assert ref.kernel_of('NN', ref.FORMS['plain']) == 'generic'


def test_nonfinite_reference():
    case = ref.Case('nonfinite', 5, 4, 19, 'bias')
    p = ref.make_problem('TN', case)
    p.a.image[0, 18, 2] = np.inf
    p.b.image[0, 3, 1] = np.nan
    c, bad, colsum, bad_colsum = ref.nonfinite_reference(p)
    assert bad.sum() == 4 + 5 - 1 and bad[2].all() and bad[:, 1].all() and np.isfinite(c).all()
    assert bad_colsum.tolist() == [False, False, True, False, False]
    with np.errstate(invalid='ignore'):
        direct = p.compute_reference().ref_c[0]
    assert np.array_equal(~np.isfinite(direct), bad) and np.array_equal(direct[~bad], c[~bad])
