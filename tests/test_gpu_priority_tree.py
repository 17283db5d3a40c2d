"""The priority tree of csrc/priority.hip on the GPU against tests/prioritized_ref.py (NumPy float64).

Sample: the device block is filled from the reference tree (float32 leaves, float64 ascending sums — the block's
defined content), so the descent is tested on its own: indices must equal the reference's EXACTLY.  The draws are
chosen from the float64 reference alone (prioritized_ref.safe_uniforms: 1e-9 * total from every prefix boundary on
the path, 10^4 times the association-order bound; closer draws are replaced, u = 0 and u = 1 - 2^-53 are kept).
Weights: against float64, tolerance WEIGHT_RTOL below.  Store / update: the sums the DEVICE computes, read back,
against float64 sums of the read-back children; duplicates, out-of-capacity indices, the wrap of a row, max_leaf.
"""
import functools

import numpy as np
import pytest

import prioritized_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

GUARD = 64
BETA = 0.4
# powf's largest relative error on these inputs, measured: profiles/prioritized_replay_accuracy.md (float32 quotient,
# float32 powf, against the float64 power of the float64 quotient).  The tolerance is 4 x that, never above 1e-5.
POWF_MEASURED = 2.81e-7
WEIGHT_RTOL = min(4 * POWF_MEASURED, 1e-5)
# (loss + epsilon)^alpha as float32 against the float64 power of the same float32 sum: the same powf, one rounding more
LEAF_RTOL = WEIGHT_RTOL

CAPACITIES = (1, 63, 64, 65, 4097, 262145)
LEAF_SETS = ('equal', 'prefix', 'spike', 'span', 'last')
measured = {}                    # what the weight checks saw, printed by the last test of this file


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def check(status, lib):
    assert status == 0, lib.tonic_last_error().decode()


def stream():
    return torch.cuda.current_stream().cuda_stream


def leaf_set(name, capacity, rng):
    """float32 leaves, so that the device's block holds exactly what the float64 reference sums."""
    leaves = np.zeros(capacity, np.float32)
    if name == 'equal':
        leaves[:] = 0.37
    elif name == 'prefix':                    # a store that is not full yet
        filled = (capacity * 3 + 4) // 5
        leaves[:filled] = rng.uniform(0.5, 1.5, filled)
    elif name == 'spike':                     # one leaf 10^6 times the rest
        leaves[:] = 1e-3
        leaves[capacity // 3] = 1e3
    elif name == 'span':                      # 2^-20 .. 2^20
        leaves[:] = np.exp2(rng.uniform(-20, 20, capacity))
        leaves[0], leaves[-1] = 2.0 ** -20, 2.0 ** 20
    elif name == 'last':                      # a single non-zero leaf at the last index
        leaves[-1] = 0.75
    return leaves


@functools.lru_cache(maxsize=None)
def reference_tree(capacity, name):
    rng = np.random.RandomState(capacity * 7 + LEAF_SETS.index(name))
    return ref.Tree(capacity, leaf_set(name, capacity, rng))


@functools.lru_cache(maxsize=None)
def reference_draws(capacity, name, B):
    """(uniforms, indices) of the float64 reference, computed once per case."""
    tree = reference_tree(capacity, name)
    rng = np.random.RandomState(B * 1000 + capacity % 997)
    uniforms = ref.safe_uniforms(tree, B, rng, keep=(0.0, 1 - 2.0 ** -53))
    return uniforms, tree.sample(uniforms)


def block_of(tree):
    """The device block holding `tree`: header, float32 leaves, float64 sums at the documented offsets."""
    raw = np.zeros(ref.tree_bytes(tree.capacity), np.uint8)
    raw[:4] = np.frombuffer(np.float32(tree.max_leaf).tobytes(), np.uint8)
    for level, offset in enumerate(ref.level_offsets(tree.capacity)):
        values = tree.levels[level].astype(np.float32 if level == 0 else np.float64)
        raw[offset:offset + values.nbytes] = np.frombuffer(values.tobytes(), np.uint8)
    return torch.as_tensor(raw).cuda()


def read_back(block, capacity):
    """(max_leaf, [levels as float64]) of a device block."""
    raw = block.cpu().numpy()
    sizes, levels = ref.level_sizes(capacity), []
    for level, offset in enumerate(ref.level_offsets(capacity)):
        kind, width = (np.float32, 4) if level == 0 else (np.float64, 8)
        values = np.frombuffer(raw[offset:offset + width * ref.pad64(sizes[level])].tobytes(), kind)
        levels.append(values.astype(np.float64))
    return np.frombuffer(raw[:4].tobytes(), np.float32)[0], levels


def guarded(count, dtype, fill):
    arena = torch.full((count + 2 * GUARD,), fill, dtype=dtype, device='cuda')
    return arena, arena[GUARD:GUARD + count]


def untouched(arena, fill):
    values = arena.cpu().numpy()
    outside = np.concatenate([values[:GUARD], values[-GUARD:]])
    return np.all(np.isnan(outside)) if isinstance(fill, float) and np.isnan(fill) else np.all(outside == fill)


def device_sample(lib, block, capacity, uniforms, beta=BETA, want_weights=True):
    B = len(uniforms)
    u = torch.as_tensor(uniforms, dtype=torch.float64).cuda()
    index_arena, indices = guarded(B, torch.int64, -7)
    weight_arena, weights = guarded(B, torch.float32, float('nan'))
    check(lib.tonic_priority_sample(block.data_ptr(), block.numel(), capacity, u.data_ptr(), indices.data_ptr(),
                                    weights.data_ptr() if want_weights else None, B, beta, stream()), lib)
    torch.cuda.synchronize()
    assert untouched(index_arena, -7) and untouched(weight_arena, float('nan')), 'a write outside [0, B)'
    return indices.cpu().numpy(), weights.cpu().numpy()


def check_weights(what, got, tree, indices, beta):
    want = tree.weights(indices, beta)
    error = float(np.max(np.abs(got.astype(np.float64) - want) / want))
    measured[what] = error
    print(f'{what}: largest relative error of the weights {error:.3e} (tolerance {WEIGHT_RTOL:.3e})')
    assert error <= WEIGHT_RTOL, (what, error)
    assert got.max() <= 1.0 + WEIGHT_RTOL and got.min() > 0


@pytest.mark.parametrize('name', LEAF_SETS)
@pytest.mark.parametrize('B', [1, 33, 256])
@pytest.mark.parametrize('capacity', CAPACITIES)
def test_sample(lib, capacity, B, name):
    tree = reference_tree(capacity, name)
    uniforms, want = reference_draws(capacity, name, B)
    assert uniforms[0] == 0.0 and (B == 1 or uniforms[1] == 1 - 2.0 ** -53)
    live = np.flatnonzero(tree.leaves > 0)
    assert want[0] == live[0] and (B == 1 or want[1] == live[-1])        # the first and the last non-zero leaf
    assert (tree.leaves[want] > 0).all()
    block = block_of(tree)
    before = block.clone()
    indices, weights = device_sample(lib, block, capacity, uniforms)
    assert torch.equal(block, before), 'the sample wrote into the tree'
    assert np.array_equal(indices, want), (np.flatnonzero(indices != want)[:5], indices[:5], want[:5])
    check_weights(f'sample {capacity} {B} {name}', weights, tree, want, BETA)
    # the indices do not depend on the weights being asked for
    alone, nothing = device_sample(lib, block, capacity, uniforms, want_weights=False)
    assert np.array_equal(alone, want) and np.isnan(nothing).all()


@pytest.mark.parametrize('beta', [0.0, 1.0])
def test_weights_at_the_ends_of_beta(lib, beta):
    tree = reference_tree(4097, 'span')
    uniforms, want = reference_draws(4097, 'span', 256)
    indices, weights = device_sample(lib, block_of(tree), 4097, uniforms, beta=beta)
    assert np.array_equal(indices, want)
    check_weights(f'beta {beta}', weights, tree, want, beta)
    if beta == 0.0:
        assert (weights == 1.0).all()


def assert_sums(levels, capacity, what):
    """Every inner node equals the float64 ascending sum of its read-back children to within 1 ulp."""
    for level in range(1, len(levels)):
        want = ref.ascending_sums(levels[level - 1].reshape(-1, 64))
        got = levels[level]
        assert (got[len(want):] == 0).all(), f'{what}: level {level} written behind its nodes'
        off = np.abs(got[:len(want)] - want)
        worst = int(np.argmax(off / np.spacing(np.maximum(want, np.finfo(np.float64).tiny))))
        assert (off <= np.spacing(want)).all(), (what, level, worst, got[worst], want[worst])


def run_sequence(lib, capacity, W, B):
    """init -> rows stored -> an update with duplicates and indices outside the capacity -> an update that must not
    move max_leaf -> the first row stored again (the wrap) -> a sample.  Asserts every state on the way; returns the
    final block's bytes and the sample, for the bit-identity of two runs."""
    rng = np.random.RandomState(capacity + B)
    size = lib.tonic_priority_tree_bytes(capacity)
    assert size == ref.tree_bytes(capacity)
    arena = torch.full((size + 2 * 512,), 0xAB, dtype=torch.uint8, device='cuda')
    block = arena[512:512 + size]

    def state(what):
        torch.cuda.synchronize()
        host = arena.cpu().numpy()
        assert (host[:512] == 0xAB).all() and (host[-512:] == 0xAB).all(), f'{what}: a write outside the block'
        max_leaf, levels = read_back(block, capacity)
        assert (levels[0][capacity:] == 0).all(), f'{what}: a leaf behind the capacity'
        assert_sums(levels, capacity, what)
        return max_leaf, levels

    check(lib.tonic_priority_tree_init(block.data_ptr(), size, capacity, stream()), lib)
    max_leaf, levels = state('init')
    assert max_leaf == 1.0 and all((level == 0).all() for level in levels)

    rows = min(capacity // W, 40)
    firsts = [row * W for row in range(rows)]
    if capacity >= 4097:                      # rows that straddle a node of every level, and the last one
        firsts += [64 - 1, min(4096 - 2, capacity - W), capacity - W]
    for first in firsts:
        check(lib.tonic_priority_store(block.data_ptr(), size, capacity, first, W, stream()), lib)
    max_leaf, levels = state('store')
    stored = np.zeros(capacity, bool)
    for first in firsts:
        stored[first:first + W] = True
    assert max_leaf == 1.0 and (levels[0][:capacity] == stored).all()

    # an update: indices among the stored leaves, every third position a repeat of an earlier one, losses distinct
    # per position so that the winner of a repeated index is known by its value
    live = np.flatnonzero(stored)
    indices = rng.choice(live, B)
    indices[2::3] = indices[:len(indices[2::3])]
    if B >= 33:
        indices[5], indices[7] = -1, capacity                      # outside the capacity: skipped
    losses = (0.5 + np.arange(B) * 0.25).astype(np.float32)
    alpha, epsilon = 0.6, 1e-6
    expected = ref.Tree(capacity, levels[0][:capacity], max_leaf)
    written = expected.update(indices, losses, alpha, epsilon)
    d_indices, d_losses = torch.as_tensor(indices).cuda(), torch.as_tensor(losses).cuda()
    check(lib.tonic_priority_update(block.data_ptr(), size, capacity, d_indices.data_ptr(), d_losses.data_ptr(), B,
                                    alpha, epsilon, stream()), lib)
    new_max, new_levels = state('update')
    touched = np.zeros(capacity, bool)
    touched[list(written)] = True
    assert (new_levels[0][:capacity][~touched] == levels[0][:capacity][~touched]).all(), 'an undrawn leaf moved'
    got, want = new_levels[0][:capacity][touched], expected.leaves[touched]
    error = float(np.max(np.abs(got - want) / want))
    print(f'update {capacity} {B}: largest relative error of the new leaves {error:.3e} (tolerance {LEAF_RTOL:.3e})')
    assert error <= LEAF_RTOL                 # (neighbouring positions' losses differ by >= 2e-3 relative)
    assert new_max == max(np.float32(1.0), np.float32(new_levels[0][:capacity][touched].max()))
    assert new_max >= max_leaf

    # max_leaf only grows: an update with small losses moves leaves and sums, not max_leaf
    small = torch.full((B,), 1e-3, dtype=torch.float32, device='cuda')
    check(lib.tonic_priority_update(block.data_ptr(), size, capacity, d_indices.data_ptr(), small.data_ptr(), B,
                                    alpha, epsilon, stream()), lib)
    same_max, small_levels = state('small update')
    assert same_max == new_max
    assert (small_levels[0][:capacity][touched] < 0.02).all()

    # the wrap: the first row stored again starts at the largest priority seen so far
    check(lib.tonic_priority_store(block.data_ptr(), size, capacity, 0, W, stream()), lib)
    wrap_max, wrap_levels = state('wrap')
    assert wrap_max == new_max and (wrap_levels[0][:W] == np.float64(new_max)).all()
    assert (wrap_levels[0][W:capacity] == small_levels[0][W:capacity]).all()

    # a sample after all that matches the reference rebuilt from the read-back leaves
    rebuilt = ref.Tree(capacity, wrap_levels[0][:capacity], wrap_max)
    uniforms = ref.safe_uniforms(rebuilt, 33, rng, keep=(0.0, 1 - 2.0 ** -53))
    sampled, weights = device_sample(lib, block, capacity, uniforms)
    assert np.array_equal(sampled, rebuilt.sample(uniforms))
    check_weights(f'after update {capacity} {B}', weights, rebuilt, sampled, BETA)
    return block.cpu().numpy().tobytes(), sampled.tobytes(), weights.tobytes()


@pytest.mark.parametrize('capacity, W, B', [(1, 1, 1), (64, 3, 33), (65, 3, 33), (4097, 3, 256), (4097, 64, 1024),
                                            (262145, 5, 256)])
def test_store_and_update(lib, capacity, W, B):
    first = run_sequence(lib, capacity, W, B)
    second = run_sequence(lib, capacity, W, B)
    assert first == second, 'the same sequence gave other bits'


def test_report():
    """Prints what the weight checks of this file measured (profiles/prioritized_replay_accuracy.md)."""
    assert measured
    worst = max(measured, key=measured.get)
    print(f'largest relative error of the weights over {len(measured)} cases: {measured[worst]:.3e} ({worst})')
