"""Reference, inputs and case table of the small-batch GEMM block (tonic_amd/csrc/gemm16.hip), for
tests/test_gemm_block_host.py (no GPU) and tests/test_gpu_gemm_block.py.

One problem is   C = [c0 +] mask'(act(alpha * op(A) op(B) + bias)),   colsum[m] = sum_k A[k][m] (TN),
computed here in float64 from the LOGICAL matrices; the device gets every operand at its pitch inside an image
whose every other float is a NaN (the columns beyond the row length, one guard row after each matrix).

Exact inputs: A, B, bias and c0 are integers in [-4, 4], alpha is 1 or 0.5, mask values are multiples of 1/8 in
[-1, 1].  With K <= 5000 every product, every partial sum IN ANY ORDER and every step of the epilogue (act none or
ReLU, every mask_act: 1 - a * a and a + 1 are exact on eighths) is a float32 — |sums| <= 16 K < 2^24, and the widest
value, c0 + (alpha * sum + bias) * (1 - a * a), is a multiple of 1 / 128 below 2^17 — so the kernels must give the
reference BIT FOR BIT whatever their summation order: no tolerance can hide a dropped or doubled k-term, or a wrong
element that is small next to the matrix maximum.  `make_problem` asserts the range condition on its own inputs and
that the float64 reference is a float32.

The PATH SELECTION below (waves_per_tile, generic_path, tn_path) MIRRORS gemm16.hip's constants — kGemmGroup = 4
chunks in flight, kGemmMaxWaves = 16, 2048 waves to fill the chip, kTnWaves = kTnDepth = 4, kGemmGroupMax = 4,
kGemmGroupWide = 6, 16 x 32 and 32 x 32 tiles — and MUST FOLLOW THEM: it exists so that the table's coverage of the
kernels' paths can be checked on the CPU, and it proves nothing once it differs from the code."""
import dataclasses

import numpy as np

ACT_NONE, ACT_RELU, ACT_TANH, ACT_ELU = 0, 1, 2, 3

MN_POOL = (1, 2, 15, 16, 17, 31, 32, 33, 63, 65, 97)
K_POOL = (1, 15, 16, 17, 19, 32, 41, 49, 69, 256, 257, 528, 1029)
BIG = (1024, 256, 256)             # the one case with enough tiles that S stays below the chunk count
K_EXACT_MAX = 5000


# ------------------------------------------------------------------------------------------ reference
def activation(v, act):
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_ELU:
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
    assert act == ACT_NONE
    return v


def mask_derivative(v, a, mask_act):
    """gemm16.h: ACT_NONE / ACT_RELU: mask > 0;  ACT_TANH: 1 - mask^2;  ACT_ELU: mask > 0 ? 1 : mask + 1."""
    if mask_act == ACT_TANH:
        return v * (1.0 - a * a)
    if mask_act == ACT_ELU:
        return np.where(a > 0, v, v * (a + 1.0))
    return np.where(a > 0, v, 0.0)


def logical_ops(mode, a, b):
    """op(A) [M, K] and op(B) [K, N] of the stored matrices."""
    assert mode in ('NT', 'NN', 'TN')
    return (a if mode[0] == 'N' else a.T), (b.T if mode[1] == 'T' else b)


def reference(mode, a, b, bias=None, mask=None, c0=None, act=0, mask_act=0, accumulate=0, alpha=1.0):
    """-> (C [M, N], colsum [M] or None), float64, from the logical matrices as stored (A is [K, M] for TN ...)."""
    f = lambda x: None if x is None else np.asarray(x, np.float64)
    a, b, bias, mask, c0 = f(a), f(b), f(bias), f(mask), f(c0)
    al, bl = logical_ops(mode, a, b)
    v = np.float64(alpha) * (al @ bl)
    if bias is not None:
        v = v + bias[None, :]
    v = activation(v, act)
    if mask is not None:
        v = mask_derivative(v, mask, mask_act)
    if accumulate:
        v = c0 + v
    return v, (a.sum(0) if mode == 'TN' else None)


# ------------------------------------------------------------------------------------- path selection
def weight_ld(cols):
    """tonic_mlp_weight_stride (mlpfwd.h): a multiple of 4 floats that is no multiple of 32."""
    ld = (cols + 3) // 4 * 4
    return ld + 4 if ld % 32 == 0 else ld


def pitch_of(kind, width):
    if kind == 'tight':
        return width
    if kind == 'odd':                      # 8-byte loads and stores on 4-byte boundaries
        return width + 3 if (width + 3) % 2 else width + 4
    if kind == 'product':                  # the learner's own: weight_ld of the width padded to 16
        return weight_ld((width + 15) // 16 * 16)
    if kind == 'wide':                     # >= 32 x tiles: a partial tile whose rows outlast the tile
        return (width + 31) // 32 * 32
    raise ValueError(kind)


def waves_per_tile(K, tiles_total):
    chunks = (K + 15) // 16
    S = 1
    while S < 16 and S * 4 < chunks:
        S *= 2
    while S < 16 and S < chunks and tiles_total * S < 2048:
        S *= 2
    return S


def kernel_of(mode, form):
    """'tn': the interleaved weight-gradient kernel (plain TN), else 'generic'."""
    plain = not form['bias'] and not form['mask'] and form['act'] == ACT_NONE
    return 'tn' if mode == 'TN' and plain else 'generic'


def generic_path(shapes, K, batch):
    """gemm16_kernel / gemm16_group_kernel over problems `shapes` = [(M, N), ...] of one launch."""
    tiles = [((M + 15) // 16) * ((N + 31) // 32) for M, N in shapes]
    S = waves_per_tile(K, sum(tiles) * batch)
    per_block = 1 if S >= 4 else 4 // S
    chunks = (K + 15) // 16
    first = np.cumsum([0] + [(t + per_block - 1) // per_block for t in tiles])
    return dict(S=S, per_block=per_block, rounds=2 if chunks > 4 * S else 1,
                part_empty=any(t % per_block for t in tiles), first=[int(x) for x in first])


def tn_path(M, N, K, lda, ldb, colsum):
    """gemm_tn_group_kernel's choices for one problem: the set of (EDGE, COLSUM) over its 32 x 32 tiles, whether a
    partial tile takes the vector loads, the wave that owns the ragged chunk, the rounds of wave 0's pipeline
    (wave 0 walks ceil(full / 4) chunks, four per round: a second round from K = 272 on.  K = 257 is one FULL round of
    all four waves, every slot's clamped re-request issued, and then the ragged chunk; K = 528 is three rounds)."""
    forms, vector_partial = set(), False
    for tm in range((M + 31) // 32):
        for tn in range((N + 31) // 32):
            edge = 32 * tm + 32 > lda or 32 * tn + 32 > ldb
            forms.add((edge, bool(colsum) and tn == 0))
            if not edge and (32 * tm + 32 > M or 32 * tn + 32 > N):
                vector_partial = True
    full = K // 16
    return dict(forms=forms, vector_partial=vector_partial, small_k=full == 0,
                owner=full % 4 if K % 16 else None, rounds=2 if full > 16 else 1,
                blocks=((M + 31) // 32) * ((N + 31) // 32))


# --------------------------------------------------------------------------------------------- inputs
FORMS = {
    'plain': dict(bias=False, mask=False, act=0, mask_act=0, accumulate=0, alpha=1.0),
    'plain_acc': dict(bias=False, mask=False, act=0, mask_act=0, accumulate=1, alpha=0.5),
    'bias': dict(bias=True, mask=False, act=0, mask_act=0, accumulate=0, alpha=0.5),
    'bias_acc': dict(bias=True, mask=False, act=0, mask_act=0, accumulate=1, alpha=0.5),
    'bias_relu': dict(bias=True, mask=False, act=1, mask_act=0, accumulate=0, alpha=1.0),
    'relu_mask': dict(bias=False, mask=True, act=0, mask_act=1, accumulate=1, alpha=1.0),
    'none_mask': dict(bias=True, mask=True, act=0, mask_act=0, accumulate=0, alpha=1.0),
    'tanh_mask': dict(bias=False, mask=True, act=0, mask_act=2, accumulate=0, alpha=1.0),
    'elu_mask': dict(bias=True, mask=True, act=0, mask_act=3, accumulate=1, alpha=0.5),
    'full': dict(bias=True, mask=True, act=1, mask_act=1, accumulate=1, alpha=0.5),     # test_gemm16_vs_numpy's
    # tanh / ELU OUTPUTS: the exact pre-activations scaled by 1/8 (alpha and the bias in eighths); not bit-exact
    'tanh_out': dict(bias=True, mask=False, act=2, mask_act=0, accumulate=0, alpha=0.125, bias_scale=0.125),
    'elu_out': dict(bias=True, mask=False, act=3, mask_act=0, accumulate=0, alpha=0.125, bias_scale=0.125),
}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    form: str = 'plain'
    pa: str = 'tight'          # pitch kinds of A, B, C and the mask (the mask's differs from C's: ldmask != ldc)
    pb: str = 'tight'
    pc: str = 'tight'
    pm: str = 'odd'
    batch: int = 1
    colsum: bool = True        # TN: ask for the column sums
    share_b: bool = False      # stride 0 on B
    share_bias: bool = False   # stride 0 on the bias


def nan_image(shape, rng):
    """Quiet NaNs of either sign with random payloads: a NaN that moved is a different NaN."""
    bits = rng.integers(1, 1 << 22, size=shape, dtype=np.uint32) | np.uint32(0x7fc00000)
    bits |= rng.integers(0, 2, size=shape, dtype=np.uint32) << np.uint32(31)
    return bits.view(np.float32)


class Operand:
    """`values` [nz, rows, cols] inside a NaN image [nz, rows + 1, pitch]; nz = 1 and stride 0 when shared."""

    def __init__(self, values, pitch, rng, shared=False):
        values = np.asarray(values, np.float32)
        nz, self.rows, self.cols = values.shape
        assert pitch >= self.cols and (nz == 1 or not shared)
        self.pitch = pitch
        self.image = nan_image((nz, self.rows + 1, pitch), rng)
        self.image[:, :self.rows, :self.cols] = values
        self.stride = 0 if shared else (self.rows + 1) * pitch       # >= rows x pitch

    def logical(self, z=0):
        return self.image[0 if self.stride == 0 else z, :self.rows, :self.cols]

    def outside(self):
        """The image as uint32 with the logical part zeroed: what no kernel may change."""
        bits = self.image.view(np.uint32).copy()
        bits[:, :self.rows, :self.cols] = 0
        return bits

    def slice(self, z):
        one = Operand.__new__(Operand)
        one.rows, one.cols, one.pitch, one.stride = self.rows, self.cols, self.pitch, self.stride
        zz = 0 if self.stride == 0 else z
        one.image = self.image[zz:zz + 1].copy()
        return one


@dataclasses.dataclass
class Problem:
    mode: str
    M: int
    N: int
    K: int
    batch: int
    form: dict
    a: Operand
    b: Operand
    c: Operand
    bias: Operand = None
    mask: Operand = None
    colsum: Operand = None
    ref_c: list = None         # per z: float64 [M, N]
    ref_colsum: list = None    # per z: float64 [M] (TN with colsum)

    def compute_reference(self):
        f = self.form
        self.ref_c, self.ref_colsum = [], []
        for z in range(self.batch):
            c, s = reference(self.mode, self.a.logical(z), self.b.logical(z),
                             None if self.bias is None else self.bias.logical(z)[0],
                             None if self.mask is None else self.mask.logical(z), self.c.logical(z),
                             f['act'], f['mask_act'], f['accumulate'], f['alpha'])
            self.ref_c.append(c)
            self.ref_colsum.append(s)
        if self.colsum is None:
            self.ref_colsum = None
        return self

    def slice(self, z):
        """Batch member z as a problem of its own (batch = 1, its own copies of the images)."""
        part = lambda op: None if op is None else op.slice(z)
        one = Problem(self.mode, self.M, self.N, self.K, 1, self.form, part(self.a), part(self.b), part(self.c),
                      part(self.bias), part(self.mask), part(self.colsum))
        one.ref_c = [self.ref_c[z]]
        one.ref_colsum = None if self.ref_colsum is None else [self.ref_colsum[z]]
        return one


def stored_shapes(mode, M, N, K):
    return ((M, K) if mode[0] == 'N' else (K, M)), ((N, K) if mode[1] == 'T' else (K, N))


def make_problem(mode, case, seed=0, data='exact'):
    """The operands of `case` in `mode` (images, pitches, strides) and its float64 reference.  data = 'exact': the
    integer inputs of the module docstring, checked for exactness; 'normal': standard normal float32 draws."""
    form = FORMS[case.form]
    rng = np.random.default_rng([seed, case.M, case.N, case.K, sum(map(ord, mode + case.name))])
    M, N, K, nz = case.M, case.N, case.K, case.batch
    a_shape, b_shape = stored_shapes(mode, M, N, K)
    if data == 'exact':
        assert K <= K_EXACT_MAX and K * 16 < 2 ** 24
        draw = lambda *shape: rng.integers(-4, 5, size=shape).astype(np.float32)
        draw_mask = lambda *shape: (rng.integers(-8, 9, size=shape) / 8.0).astype(np.float32)
    else:
        draw = draw_mask = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    def ends_nonzero(x, k_axis):
        """No zero at k = 0 and k = K - 1: a first or last k-term that is dropped shows in EVERY output."""
        x = np.moveaxis(x, k_axis, 0)
        x[0][x[0] == 0] = 1
        x[-1][x[-1] == 0] = -1
        return np.moveaxis(x, 0, k_axis)
    a = Operand(ends_nonzero(draw(nz, *a_shape), 2 if mode[0] == 'N' else 1), pitch_of(case.pa, a_shape[1]), rng)
    b = Operand(ends_nonzero(draw(1 if case.share_b else nz, *b_shape), 2 if mode[1] == 'T' else 1),
                pitch_of(case.pb, b_shape[1]), rng, case.share_b)
    # not accumulating: C starts as NaN, so that an element the kernel does not write shows
    c0 = draw(nz, M, N) if form['accumulate'] else nan_image((nz, M, N), rng)
    c = Operand(c0, pitch_of(case.pc, N), rng)
    bias = mask = colsum = None
    if form['bias']:
        values = draw(1 if case.share_bias else nz, 1, N) * np.float32(form.get('bias_scale', 1.0))
        bias = Operand(values, N + 5, rng, case.share_bias)
    if form['mask']:
        mask = Operand(draw_mask(nz, M, N), pitch_of(case.pm, N), rng)
    if mode == 'TN' and case.colsum:
        colsum = Operand(nan_image((nz, 1, M), rng), M + 5, rng)
    problem = Problem(mode, M, N, K, nz, form, a, b, c, bias, mask, colsum).compute_reference()
    if data == 'exact' and form['act'] in (ACT_NONE, ACT_RELU):
        for z in range(nz):            # the float64 reference IS a float32: nothing was rounded on the way
            assert np.array_equal(problem.ref_c[z].astype(np.float32).astype(np.float64), problem.ref_c[z])
            assert np.abs(logical_ops(mode, a.logical(z), b.logical(z))[0]).sum(1).max() * 4 < 2 ** 24
    return problem


def nonfinite_reference(problem, z=0):
    """For a problem (act none, no mask) with ±inf / NaN placed in A or B: the float64 reference of the inputs with
    those elements zeroed, and the mask of outputs that are non-finite — every output of a row of op(A) / a column
    of op(B) that holds one (inf x 0 = NaN, inf x nonzero = inf: no finite result can come of it).
    -> (C, bad [M, N], colsum or None, bad_colsum [M] or None)"""
    f = problem.form
    assert f['act'] == ACT_NONE and not f['mask']
    a, b = problem.a.logical(z).astype(np.float64), problem.b.logical(z).astype(np.float64)
    al, bl = logical_ops(problem.mode, a, b)
    bad = ~np.isfinite(al).all(1)[:, None] | ~np.isfinite(bl).all(0)[None, :]
    clean = lambda x: np.where(np.isfinite(x), x, 0.0)
    c, s = reference(problem.mode, clean(a), clean(b), None if problem.bias is None else problem.bias.logical(z)[0],
                     None, problem.c.logical(z), 0, 0, f['accumulate'], f['alpha'])
    if problem.colsum is None:
        return c, bad, None, None
    return c, bad, s, ~np.isfinite(a).all(0)


# ---------------------------------------------------------------------------------------------- table
# Every case runs in NT, NN and TN.  In TN the plain forms ('plain', 'plain_acc') take the interleaved kernel, every
# other form the generic one with both operands k-strided — the only road to the generic kernel's own column sums.
def _table():
    C = Case
    t = [
        # ---- K <= 16: one chunk, S = 1, four tiles per workgroup; the TN kernel's ragged chunk is the whole product
        C('k1_value_head', 17, 1, 1, 'bias', pa='odd'),
        C('k1_plain', 2, 33, 1, 'plain', pb='odd', pc='odd'),
        C('k15_six_tiles', 33, 33, 15, 'full', pa='odd', pb='odd', pc='product'),         # 6 tiles: 4 + 2
        C('k15_plain_edge', 33, 17, 15, 'plain', pa='tight', pb='tight', pc='odd'),
        C('k16_full_block', 17, 33, 16, 'tanh_mask', pa='product', pb='product', pc='product', pm='tight'),  # 4
        C('k16_plain_vector', 65, 63, 16, 'plain_acc', pa='wide', pb='wide', pc='odd'),
        C('k16_one_tile', 16, 32, 16, 'relu_mask'),
        C('k15_batch3', 31, 2, 15, 'elu_mask', pa='odd', pb='product', pc='odd', pm='product', batch=3),
        # ---- K = 17 .. 32: two chunks, S = 2, two tiles per workgroup
        C('k17_three_tiles', 33, 17, 17, 'bias_relu', pa='odd', pb='odd', pc='odd'),       # 3 tiles: 2 + 1
        C('k17_plain', 65, 15, 17, 'plain', pa='product', pb='product', pc='product'),
        C('k19_owner1', 63, 65, 19, 'plain', pa='odd', pb='odd', pc='tight'),
        C('k19_elu_mask', 15, 97, 19, 'elu_mask', pa='product', pb='odd', pc='product', pm='tight'),
        C('k32_two_tiles', 32, 32, 32, 'none_mask', pa='product', pb='product', pc='odd', pm='product'),
        C('k32_plain_nosum', 97, 31, 32, 'plain', pa='wide', pb='wide', pc='product', colsum=False),
        C('k32_batch2_shared', 17, 33, 32, 'full', pa='odd', pb='tight', pc='odd', batch=2, share_b=True,
          share_bias=True),
        # ---- three to four chunks: S = 4, one tile per workgroup from here on
        C('k41_owner2', 33, 63, 41, 'plain_acc', pa='tight', pb='product', pc='odd'),
        C('k41_tanh_mask', 31, 33, 41, 'tanh_mask', pa='odd', pb='product', pc='tight', pm='product'),
        C('k49_owner3', 65, 2, 49, 'plain', pa='product', pb='tight', pc='tight', colsum=False),
        C('k49_bias', 1, 65, 49, 'bias', pa='odd', pb='odd', pc='odd'),
        C('k49_batch3_plain', 17, 33, 49, 'plain', pa='wide', pb='odd', pc='product', batch=3, share_b=True),
        # ---- five chunks: S = 8
        C('k69_owner0', 97, 97, 69, 'plain', pa='product', pb='product', pc='product'),
        C('k69_full', 63, 31, 69, 'full', pa='product', pb='odd', pc='odd', pm='tight'),
        C('k69_plain_nosum_vector', 33, 16, 69, 'plain_acc', pa='wide', pb='product', pc='tight', colsum=False),
        C('k69_batch2', 16, 17, 69, 'relu_mask', pa='tight', pb='odd', pc='product', batch=2),
        # ---- sixteen chunks and more: S = 16
        C('k256_plain', 33, 33, 256, 'plain', pa='odd', pb='odd', pc='odd'),
        C('k256_elu_mask', 17, 65, 256, 'elu_mask', pa='product', pb='product', pc='product', pm='odd'),
        C('k257_ragged_after_full_round', 65, 31, 257, 'plain', pa='product', pb='wide', pc='tight'),
        C('k257_bias_relu', 2, 15, 257, 'bias_relu', pa='odd', pb='odd', pc='tight'),
        C('k528_tn_rounds', 33, 65, 528, 'plain_acc', pa='tight', pb='product', pc='product'),
        C('k528_tn_rounds_vector', 63, 32, 528, 'plain', pa='wide', pb='tight', pc='odd', colsum=False, batch=2),
        C('k528_none_mask', 15, 1, 528, 'none_mask', pa='product', pb='tight', pc='odd', pm='product'),
        C('k1029_generic_rounds', 17, 33, 1029, 'full', pa='odd', pb='product', pc='product', pm='odd'),
        C('k1029_plain', 31, 17, 1029, 'plain', pa='product', pb='odd', pc='tight'),
        C('k1029_tanh_mask_batch2', 1, 2, 1029, 'tanh_mask', pa='tight', pb='odd', pc='odd', pm='tight', batch=2,
          share_b=True),
        # ---- tiles enough that S stays below the chunk count (test_gemm16_vs_numpy's first shape)
        C('big_full', *BIG, 'full', pa='product', pb='product', pc='product', pm='tight'),
        C('big_plain', *BIG, 'plain', pa='product', pb='product', pc='product'),
    ]
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return t


TABLE = _table()
MODES = ('NT', 'NN', 'TN')

# tanh / ELU outputs (act 2 and 3), every mode; rtol = atol = ACT_TOL except the positive ELU branch, which is exact
ACT_TOL = 1e-5
ACT_CASES = [Case(f'{form}_{M}x{N}x{K}', M, N, K, form, pa=pa, pb=pb, pc=pc, batch=batch, colsum=True)
             for form in ('tanh_out', 'elu_out')
             for M, N, K, pa, pb, pc, batch in ((17, 33, 1, 'odd', 'odd', 'odd', 1),
                                                (33, 15, 17, 'product', 'product', 'product', 2),
                                                (31, 65, 41, 'tight', 'odd', 'product', 1),
                                                (2, 97, 257, 'odd', 'tight', 'odd', 1))]

# Grouped launches: (name, modes, K, batch, members); a member's K is the group's.
def _groups():
    m = lambda M, N, form='plain', **kw: Case(f'{M}x{N}_{form}', M, N, 0, form, **kw)
    generic2 = [m(33, 17, 'full', pa='odd', pb='product', pc='odd'),
                m(16, 65, 'tanh_mask', pa='product', pb='odd', pc='product', pm='tight')]
    generic4 = [m(17, 33, 'bias_relu', pa='odd', pb='odd', pc='product'),          # 4, 3, 1 and 6 tiles:
                m(33, 1, 'elu_mask', pa='product', pb='tight', pc='odd'),          # part-empty workgroups
                m(2, 15, 'bias', pa='tight', pb='product', pc='tight'),            # between neighbours
                m(31, 97, 'relu_mask', pa='product', pb='product', pc='product', pm='tight')]
    tn = [m(32, 32, pa='product', pb='product', pc='product'),                     # one tile each:
          m(1, 2, pa='odd', pb='odd', pc='odd'),                                   # every first[] boundary
          m(33, 65, pa='tight', pb='wide', pc='product'),                          # falls between neighbours
          m(17, 31, 'plain_acc', pa='wide', pb='odd', pc='tight'),
          m(65, 16, pa='product', pb='tight', pc='odd'),
          m(15, 33, 'plain_acc', pa='odd', pb='product', pc='product')]
    nosum = lambda members: [dataclasses.replace(c, colsum=False) for c in members]
    mixed = lambda members: [dataclasses.replace(c, colsum=i % 2 == 0) for i, c in enumerate(members)]
    groups = [
        ('generic2_k15', ('NT', 'NN', 'TN'), 15, 1, generic2),        # S = 1: four tiles per workgroup
        ('generic2_k69', ('NT', 'NN'), 69, 2, generic2),
        ('generic4_k16', ('NT', 'NN', 'TN'), 16, 1, generic4),
        ('generic4_k32', ('NT', 'NN'), 32, 1, generic4),              # S = 2: two tiles per workgroup
        ('generic4_k1029', ('NT', 'NN', 'TN'), 1029, 1, generic4),
        ('tn2_k19', ('TN',), 19, 1, tn[:2]),
        ('tn2_k257_nosum', ('TN',), 257, 2, nosum(tn[2:4])),
        ('tn4_k41', ('TN',), 41, 1, tn[:4]),
        ('tn4_k15_nosum', ('TN',), 15, 1, nosum(tn[1:5])),
        ('tn5_k49', ('TN',), 49, 1, tn[:5]),
        ('tn5_k528_nosum', ('TN',), 528, 1, nosum(tn[1:6])),
        ('tn6_k69', ('TN',), 69, 2, tn),
        ('tn6_k16_mixed', ('TN',), 16, 1, mixed(tn)),
    ]
    return [(name, mode, K, batch, [dataclasses.replace(c, K=K, batch=batch) for c in members])
            for name, modes, K, batch, members in groups for mode in modes]


GROUPS = _groups()


# ------------------------------------------------------------------------------------------- coverage
def required_paths():
    need = set()
    for kernel in ('NT', 'NN', 'TN-generic'):
        need |= {f'{kernel}: S={S}' for S in (1, 2, 4, 8, 16)}
        need |= {f'{kernel}: per_block={p}' for p in (4, 2, 1)}
        need |= {f'{kernel}: per_block={p}, last workgroup part empty' for p in (4, 2)}
        need |= {f'{kernel}: rounds={r}' for r in (1, 2)}
        need |= {f'{kernel}: batch={z}' for z in (1, 2, 3)}
        need |= {f'{kernel}: S below the chunk count', f'{kernel}: B stride 0', f'{kernel}: bias stride 0'}
    need |= {'TN-generic: colsum with S=1', 'TN-generic: colsum with S>1'}
    need |= {f'TN: {e}, {c}' for e in ('EDGE', 'vector') for c in ('colsum', 'no colsum')}
    need |= {f'TN: ragged owner wave {w}' for w in range(4)}
    need |= {'TN: K < 16', 'TN: partial tile on the vector path', 'TN: rounds=1', 'TN: rounds=2', 'TN: B stride 0',
             'TN: accumulate'}
    need |= {f'TN: batch={z}' for z in (1, 2, 3)}
    for kernel in ('NT', 'NN'):
        need |= {f'{kernel} group: {n} problems' for n in (2, 4)}
        need |= {f'{kernel} group: per_block={p}, a workgroup part empty' for p in (4, 2)}
    need |= {f'TN group: {n} problems, {c}' for n in (2, 4, 5, 6) for c in ('colsum', 'no colsum')}
    need |= {'TN group: wide form', 'TN group: one-tile problems side by side', 'TN-generic group: colsum'}
    return need


def _pitches(mode, c):
    a_shape, b_shape = stored_shapes(mode, c.M, c.N, c.K)
    return pitch_of(c.pa, a_shape[1]), pitch_of(c.pb, b_shape[1])


def reached_paths(table=None, groups=None):
    table = TABLE if table is None else table
    groups = GROUPS if groups is None else groups
    got = set()
    for mode in MODES:
        for c in table:
            form = FORMS[c.form]
            lda, ldb = _pitches(mode, c)
            if kernel_of(mode, form) == 'tn':
                p = tn_path(c.M, c.N, c.K, lda, ldb, c.colsum)
                got |= {f"TN: {'EDGE' if e else 'vector'}, {'colsum' if s else 'no colsum'}" for e, s in p['forms']}
                got |= {f"TN: rounds={p['rounds']}", f'TN: batch={c.batch}'}
                if p['owner'] is not None:
                    got.add(f"TN: ragged owner wave {p['owner']}")
                for flag, text in ((p['small_k'], 'TN: K < 16'), (c.share_b, 'TN: B stride 0'),
                                   (p['vector_partial'], 'TN: partial tile on the vector path'),
                                   (form['accumulate'], 'TN: accumulate')):
                    if flag:
                        got.add(text)
                continue
            kernel = mode if mode != 'TN' else 'TN-generic'
            p = generic_path([(c.M, c.N)], c.K, c.batch)
            got |= {f"{kernel}: S={p['S']}", f"{kernel}: per_block={p['per_block']}", f"{kernel}: rounds={p['rounds']}",
                    f'{kernel}: batch={c.batch}'}
            if p['part_empty']:
                got.add(f"{kernel}: per_block={p['per_block']}, last workgroup part empty")
            if p['S'] < (c.K + 15) // 16:
                got.add(f'{kernel}: S below the chunk count')
            if c.share_b:
                got.add(f'{kernel}: B stride 0')
            if c.share_bias and form['bias'] and c.batch > 1:
                got.add(f'{kernel}: bias stride 0')
            if kernel == 'TN-generic' and c.colsum:
                got.add('TN-generic: colsum with S=1' if p['S'] == 1 else 'TN-generic: colsum with S>1')
    for name, mode, K, batch, members in groups:
        kernels = {kernel_of(mode, FORMS[c.form]) for c in members}
        n = len(members)
        if kernels == {'tn'}:
            sums = {c.colsum for c in members}
            got |= {f"TN group: {n} problems, {'colsum' if s else 'no colsum'}" for s in sums}
            if n > 4:
                got.add('TN group: wide form')
            ones = [tn_path(c.M, c.N, K, *_pitches(mode, c), c.colsum)['blocks'] == 1 for c in members]
            if any(x and y for x, y in zip(ones, ones[1:])):
                got.add('TN group: one-tile problems side by side')
            continue
        assert n <= 4, name
        p = generic_path([(c.M, c.N) for c in members], K, batch)
        if mode == 'TN':
            if any(c.colsum for c in members):
                got.add('TN-generic group: colsum')
            continue
        got.add(f'{mode} group: {n} problems')
        if p['part_empty']:
            got.add(f"{mode} group: per_block={p['per_block']}, a workgroup part empty")
    return got
