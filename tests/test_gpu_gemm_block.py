"""The small-batch GEMM block (tonic_amd/csrc/gemm16.hip) on every path, through tonic_gemm_group_f32: the generic
kernels and the interleaved weight-gradient kernels against EXACT float64 sums (tests/gemm_block_ref.py: integer
inputs, so any summation order gives the reference bit for bit), at padded pitches inside NaN images, with the
batch dimension and all six strides, in groups of 2 to 6 problems, with every epilogue form; tanh / ELU outputs
and random-normal data against float64 within the bounds the older tests use; non-finite inputs stay where
they are; bad arguments are refused before any launch."""
import numpy as np
import pytest

import gemm_block_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

INVALID = -1                                       # TONIC_ERR_INVALID_ARGUMENT
OPERANDS = ('a', 'b', 'c', 'bias', 'mask', 'colsum')


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


class Launch:
    """The device images of `problems` and their tonic_gemm_problem array; run() launches and reads everything back."""

    def __init__(self, problems):
        from tonic_amd import _lib
        self.problems = problems
        self.array = (_lib.GemmProblem * max(len(problems), 1))()
        self.device = []
        for q, p in zip(self.array, problems):
            # (as int32: the NaN payloads travel as they are)
            tensors = {name: None if getattr(p, name) is None else
                       torch.from_numpy(getattr(p, name).image.view(np.int32)).cuda() for name in OPERANDS}
            self.device.append(tensors)
            for name in OPERANDS:
                setattr(q, name, None if tensors[name] is None else tensors[name].data_ptr())
                setattr(q, 'stride_' + name, 0 if tensors[name] is None else getattr(p, name).stride)
            q.M, q.N, q.K = p.M, p.N, p.K
            q.lda, q.ldb, q.ldc = p.a.pitch, p.b.pitch, p.c.pitch
            q.ldmask = p.mask.pitch if p.mask is not None else p.c.pitch
            q.act, q.mask_act, q.accumulate = p.form['act'], p.form['mask_act'], p.form['accumulate']
            q.alpha = p.form['alpha']

    def run(self, lib, mode, count=None, batch=None):
        """-> (status, per problem {operand: image read back, float32})"""
        count = len(self.problems) if count is None else count
        batch = self.problems[0].batch if batch is None else batch
        status = lib.tonic_gemm_group_f32(mode.encode(), self.array, count, batch, None)
        return status, self.read()

    def read(self):
        torch.cuda.synchronize()
        return [{name: t.cpu().numpy().view(np.float32) for name, t in tensors.items() if t is not None}
                for tensors in self.device]


def run(lib, mode, problems):
    from tonic_amd import _lib
    status, out = Launch(problems).run(lib, mode)
    _lib.check(status, 'tonic_gemm_group_f32')
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def assert_outside_untouched(p, out, what=''):
    """Everything but the logical C and colsum is bit-identical to what was uploaded: the inputs whole, the padding
    and guard rows of the outputs."""
    for name in ('a', 'b', 'bias', 'mask'):
        if getattr(p, name) is not None:
            assert np.array_equal(bits(out[name]), bits(getattr(p, name).image)), f'{what}{name} image changed'
    for name in ('c', 'colsum'):
        op = getattr(p, name)
        if op is not None:
            after = bits(out[name]).copy()
            after[:, :op.rows, :op.cols] = 0
            assert np.array_equal(after, op.outside()), f'{what}{name}: written outside the logical matrix'


def assert_exact(p, out, what=''):
    for z in range(p.batch):
        got = out['c'][z, :p.M, :p.N].astype(np.float64)
        assert np.array_equal(got, p.ref_c[z]), \
            f'{what}C[z={z}]: {(got != p.ref_c[z]).sum()} of {got.size} elements differ from the exact sums'
        if p.colsum is not None:
            got = out['colsum'][z, 0, :p.M].astype(np.float64)
            assert np.array_equal(got, p.ref_colsum[z]), f'{what}colsum[z={z}]'
    assert_outside_untouched(p, out, what)


def case_id(c):
    return c.name


# ---------------------------------------------------------------------------------------- exact results
@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('case', ref.TABLE, ids=case_id)
def test_exact_sums(lib, mode, case):
    p = ref.make_problem(mode, case)
    assert_exact(p, run(lib, mode, [p])[0])


# ------------------------------------------------------------------------------- tanh and ELU outputs
worst_activation_error = {}


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('case', ref.ACT_CASES, ids=case_id)
def test_tanh_and_elu_outputs(lib, mode, case):
    """act 2 and 3 on exact pre-activations (eighths): float64 tanh / expm1 within rtol = atol = 1e-5 — the figures
    test_torso_grads_vs_float64_autograd holds this path's forward values to; positive ELU outputs exactly."""
    p = ref.make_problem(mode, case)
    out = run(lib, mode, [p])[0]
    worst = worst_abs = 0.0
    for z in range(p.batch):
        got = out['c'][z, :p.M, :p.N].astype(np.float64)
        want = p.ref_c[z]
        pre, _ = ref.reference(mode, p.a.logical(z), p.b.logical(z), p.bias.logical(z)[0], alpha=p.form['alpha'])
        assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)       # exact pre-activations
        if p.form['act'] == ref.ACT_ELU:
            assert (pre > 0).any() and (pre < 0).any()
            assert np.array_equal(got[pre > 0], pre[pre > 0]), 'positive ELU outputs are the pre-activations'
        error = np.abs(got - want)
        worst = max(worst, float((error / (ref.ACT_TOL + ref.ACT_TOL * np.abs(want))).max()))
        worst_abs = max(worst_abs, float(error.max()))
        if p.colsum is not None:
            assert np.array_equal(out['colsum'][z, 0, :p.M].astype(np.float64), p.ref_colsum[z])
    key = 'tanh' if p.form['act'] == ref.ACT_TANH else 'elu'
    worst_activation_error[key] = max(worst_activation_error.get(key, 0.0), worst)
    print(f'\n{key} {mode} {case.name}: largest error {worst_abs:.3e} = {worst:.3e} of the bound '
          f'(atol = rtol = {ref.ACT_TOL}); so far {worst_activation_error[key]:.3e} of it')
    assert worst <= 1.0
    assert_outside_untouched(p, out)


# ------------------------------------------------------------------------------------ batch and strides
@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('case', [c for c in ref.TABLE if c.batch > 1], ids=case_id)
def test_batch_members_equal_their_own_launches(lib, mode, case):
    """batch 2 and 3 with per-z operands that differ, stride 0 on B and on the bias: every z slice is bit-identical
    to the same problem launched alone, and both are the reference."""
    p = ref.make_problem(mode, case)
    assert not np.array_equal(p.a.logical(0), p.a.logical(1)) and not np.array_equal(p.ref_c[0], p.ref_c[1])
    assert (p.b.stride == 0) == case.share_b and (p.bias is None or (p.bias.stride == 0) == case.share_bias)
    together = run(lib, mode, [p])[0]
    assert_exact(p, together)
    for z in range(p.batch):
        one = p.slice(z)
        alone = run(lib, mode, [one])[0]
        assert_exact(one, alone, f'z={z} alone: ')
        assert np.array_equal(bits(alone['c'][0]), bits(together['c'][z])), f'z={z}'
        if p.colsum is not None:
            assert np.array_equal(bits(alone['colsum'][0]), bits(together['colsum'][z])), f'z={z}'


# ----------------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize('name,mode,K,batch,members', ref.GROUPS, ids=[f'{g[0]}-{g[1]}' for g in ref.GROUPS])
def test_group_members_equal_their_own_launches(lib, name, mode, K, batch, members):
    """Groups of 2 and 4 problems on the generic kernels, 2, 4, 5 and 6 on the weight-gradient kernels (differing
    M, N, epilogues and pitches; one-tile problems side by side): each problem is bit-identical to its own launch
    and to the reference."""
    problems = [ref.make_problem(mode, c, seed=i) for i, c in enumerate(members)]
    grouped = run(lib, mode, problems)
    for i, (p, out) in enumerate(zip(problems, grouped)):
        assert_exact(p, out, f'problem {i} ({members[i].name}) in the group: ')
        alone = run(lib, mode, [p])[0]
        assert_exact(p, alone, f'problem {i} alone: ')
        assert np.array_equal(bits(alone['c']), bits(out['c'])), i
        if p.colsum is not None:
            assert np.array_equal(bits(alone['colsum']), bits(out['colsum'])), i


# ----------------------------------------------------------------------------------- random-normal data
@pytest.mark.parametrize('K', [19, 257, 1029])
@pytest.mark.parametrize('path', ['NT', 'NN', 'TN-generic', 'TN'])
def test_random_normal_data(lib, path, K):
    """test_gemm16_vs_numpy's form and bound, 2e-6 sqrt(K) max(1, |ref|max), at the learner's padded pitches."""
    mode = path[:2]
    kinds = dict(pa='product', pb='product', pc='product', pm='tight')
    product = None
    for form in ('plain', 'full'):
        if (path == 'TN-generic' and form == 'plain') or (path == 'TN' and form == 'full'):
            continue
        p = ref.make_problem(mode, ref.Case('normal', 63, 33, K, form, **kinds), data='normal')
        assert ref.kernel_of(mode, p.form) == ('tn' if path == 'TN' else 'generic')
        al, bl = ref.logical_ops(mode, p.a.logical(0).astype(np.float64), p.b.logical(0).astype(np.float64))
        product = al @ bl
        tol = 2e-6 * np.sqrt(K) * max(1.0, np.abs(product).max())
        bound = tol if form == 'plain' else tol + 1e-6
        out = run(lib, mode, [p])[0]
        error = np.abs(out['c'][0, :p.M, :p.N] - p.ref_c[0]).max()
        print(f'\n{path} K={K} {form}: error / bound = {error / bound:.3f}')
        assert error <= bound
        if p.colsum is not None:
            np.testing.assert_allclose(out['colsum'][0, 0, :p.M], p.ref_colsum[0], rtol=1e-5, atol=1e-4)
        assert_outside_untouched(p, out)


# ---------------------------------------------------------------------------------- non-finite isolation
def poke(p, operand, index, k, value):
    """op(A)[index, k] or op(B)[k, index] of batch member 0, in the stored layout."""
    if operand == 'a':
        where = (index, k) if p.mode[0] == 'N' else (k, index)
    else:
        where = (index, k) if p.mode[1] == 'T' else (k, index)
    getattr(p, operand).image[(0,) + where] = value


@pytest.mark.parametrize('K', [19, 69])
@pytest.mark.parametrize('operand', ['a', 'b'])
@pytest.mark.parametrize('path', ['NT', 'NN', 'TN-generic', 'TN'])
def test_non_finite_inputs_stay_in_their_rows_and_columns(lib, path, operand, K):
    """One +inf at the last valid k of a ragged K (where the generic kernel zeroes the clamped re-read by a multiply)
    and one NaN, in A or in B: every output whose float64 reference is finite is exact, every other one is
    non-finite (inf against NaN is not told apart), nothing outside the logical C changes."""
    mode = path[:2]
    form = 'bias_acc' if path == 'TN-generic' else 'plain_acc'
    p = ref.make_problem(mode, ref.Case('nonfinite', 17, 33, K, form, pa='odd', pb='product', pc='odd'))
    assert ref.kernel_of(mode, p.form) == ('tn' if path == 'TN' else 'generic') and K % 16
    poke(p, operand, 3, K - 1, np.inf)
    poke(p, operand, 9, 5, np.nan)
    want, bad, want_sum, bad_sum = ref.nonfinite_reference(p)
    assert bad.sum() == 2 * (p.N if operand == 'a' else p.M)
    out = run(lib, mode, [p])[0]
    got = out['c'][0, :p.M, :p.N].astype(np.float64)
    assert np.array_equal(got[~bad], want[~bad]), f'{(got != want)[~bad].sum()} finite outputs are wrong'
    assert not np.isfinite(got[bad]).any()
    if p.colsum is not None:
        got = out['colsum'][0, 0, :p.M].astype(np.float64)
        assert np.array_equal(got[~bad_sum], want_sum[~bad_sum]) and not np.isfinite(got[bad_sum]).any()
        assert bad_sum.sum() == (2 if operand == 'a' else 0)
    assert_outside_untouched(p, out)


# --------------------------------------------------------------------------------------------- refusals
def refusals():
    plain = [ref.Case(f'm{i}', 17, 33, 19, 'plain', pa='product', pb='product', pc='product') for i in range(7)]
    biased = [plain[0]] * 4 + [ref.Case('biased', 17, 33, 19, 'bias')]
    other_k = [plain[0], ref.Case('k41', 17, 33, 41, 'plain')]
    return [
        ('mode_TT', 'TT', plain[:1], {}, None),
        ('mode_TT_group', 'TT', plain[:2], {}, None),
        ('mode_one_letter', 'T', plain[:1], {}, None),
        ('group_differs_in_K', 'TN', other_k, {}, None),
        ('group_differs_in_K_generic', 'NT', other_k, {}, None),
        ('five_with_a_bias', 'TN', biased, {}, None),
        ('five_not_TN', 'NT', plain[:5], {}, None),
        ('count_0', 'TN', plain[:2], dict(count=0), None),
        ('count_7', 'TN', plain[:7], {}, None),
        ('batch_0', 'NT', plain[:1], dict(batch=0), None),
        ('null_a', 'NT', plain[:1], {}, (0, 'a')),
        ('null_b_in_a_group', 'TN', plain[:3], {}, (2, 'b')),
        ('null_c_in_a_wide_group', 'TN', plain[:6], {}, (4, 'c')),
        ('no_problems', 'NT', plain[:1], dict(null_array=True), None),
    ]


@pytest.mark.parametrize('name,mode,cases,how,null', refusals(), ids=[r[0] for r in refusals()])
def test_bad_arguments_are_refused_before_any_launch(lib, name, mode, cases, how, null):
    """Each is TONIC_ERR_INVALID_ARGUMENT from the host's own checks (no kernel ever sees a bad pointer), leaves
    every image as it was, and leaves the device usable: the valid launch that follows passes."""
    data_mode = mode if mode in ref.MODES else 'TN'
    problems = [ref.make_problem(data_mode, c, seed=i) for i, c in enumerate(cases)]
    launch = Launch(problems)
    if null is not None:
        setattr(launch.array[null[0]], null[1], None)
    if how.get('null_array'):
        status, after = lib.tonic_gemm_group_f32(mode.encode(), None, 1, 1, None), launch.read()
    else:
        status, after = launch.run(lib, mode, **{k: v for k, v in how.items() if k in ('count', 'batch')})
    assert status == INVALID, lib.tonic_last_error()
    assert lib.tonic_last_error()
    for p, out in zip(problems, after):
        for operand in out:
            assert np.array_equal(bits(out[operand]), bits(getattr(p, operand).image)), (name, operand)
    good = ref.make_problem('TN', ref.Case('after', 33, 17, 19, 'plain', pa='odd', pb='odd', pc='odd'))
    assert_exact(good, run(lib, 'TN', [good])[0])
