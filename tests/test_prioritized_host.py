"""Prioritized replay, the host side: the priority tree's size query, what its entries and the weighted critic steps
answer BEFORE any HIP call, PrioritizedBuffer's constructor and uniform stream, and the refusals by name.  No GPU:
every pointer is a fake non-NULL address nobody reads, every call is shaped to return before a launch."""
import math
import types

import numpy as np
import pytest

import prioritized_ref
from tonic_amd import _lib, parallel, replays
from tonic_amd.replays import PrioritizedBuffer

FAKE = 0x1000
INVALID, WORKSPACE = -1, -4


def _message(lib):
    return lib.tonic_last_error().decode()


@pytest.mark.parametrize('capacity', [1, 64, 65, 4096, 4097, 262145])
def test_tree_bytes(capacity):
    lib = _lib.load()
    # header + float32 leaves + float64 sums, every level padded to 64 entries, written out by hand ...
    expected = {1: 64 + 4 * 64, 64: 64 + 4 * 64, 65: 64 + 4 * 128 + 8 * 64, 4096: 64 + 4 * 4096 + 8 * 64,
                4097: 64 + 4 * 4160 + 8 * 128 + 8 * 64,
                262145: 64 + 4 * 262208 + 8 * 4160 + 8 * 128 + 8 * 64}[capacity]
    assert lib.tonic_priority_tree_bytes(capacity) == expected
    # ... and by the reference's statement of the levels
    assert prioritized_ref.tree_bytes(capacity) == expected


def test_tree_bytes_of_the_documented_capacity_and_of_no_capacity():
    lib = _lib.load()
    million = lib.tonic_priority_tree_bytes(10 ** 6)
    assert million == prioritized_ref.tree_bytes(10 ** 6)
    assert 4_000_000 <= million - 8 * (15680 + 256 + 64) <= 4_000_400      # 4 MB of leaves + 128 KB of sums
    assert lib.tonic_priority_tree_bytes(0) == 0 and lib.tonic_priority_tree_bytes(-5) == 0
    assert lib.tonic_priority_tree_bytes(2 ** 40 + 1) == 0


CAPACITY = 1000


def _call(lib, entry, **changes):
    size = lib.tonic_priority_tree_bytes(CAPACITY)
    arguments = {
        'tonic_priority_tree_init': dict(d_tree=FAKE, tree_bytes=size, capacity=CAPACITY, stream=None),
        'tonic_priority_store': dict(d_tree=FAKE, tree_bytes=size, capacity=CAPACITY, first=0, count=10, stream=None),
        'tonic_priority_sample': dict(d_tree=FAKE, tree_bytes=size, capacity=CAPACITY, d_uniforms=FAKE,
                                      d_indices=FAKE, d_weights=FAKE, B=32, beta=0.4, stream=None),
        'tonic_priority_update': dict(d_tree=FAKE, tree_bytes=size, capacity=CAPACITY, d_indices=FAKE,
                                      d_sample_losses=FAKE, B=32, alpha=0.6, epsilon=1e-6, stream=None),
    }[entry]
    assert set(changes) <= set(arguments), changes
    arguments.update(changes)
    return getattr(lib, entry)(*arguments.values())


TREE_ENTRIES = ('tonic_priority_tree_init', 'tonic_priority_store', 'tonic_priority_sample', 'tonic_priority_update')


@pytest.mark.parametrize('entry', TREE_ENTRIES)
def test_tree_entries_refuse_the_block(entry):
    lib = _lib.load()
    assert _call(lib, entry, d_tree=None) == INVALID
    assert _message(lib) == f'{entry}: d_tree is NULL'
    assert _call(lib, entry, d_tree=FAKE + 8) == INVALID
    assert _message(lib) == f'{entry}: d_tree is not 16-byte aligned'
    for capacity in (0, -1, 2 ** 40 + 1):
        assert _call(lib, entry, capacity=capacity) == INVALID
        assert _message(lib) == f'{entry}: capacity {capacity} (1 .. 2^40)'
    size = lib.tonic_priority_tree_bytes(CAPACITY)
    assert _call(lib, entry, tree_bytes=size - 1) == WORKSPACE
    assert _message(lib) == f'{entry}: a tree block of {size - 1} bytes, a capacity of {CAPACITY} needs {size}'


@pytest.mark.parametrize('first, count', [(-1, 4), (0, 0), (0, -3), (CAPACITY, 1), (CAPACITY - 3, 4),
                                          (0, CAPACITY + 1), (2 ** 62, 2 ** 62)])
def test_store_refuses_leaves_outside_the_capacity(first, count):
    lib = _lib.load()
    assert _call(lib, 'tonic_priority_store', first=first, count=count) == INVALID
    assert _message(lib) == (f'tonic_priority_store: leaves [{first}, {first} + {count}) of a capacity of '
                             f'{CAPACITY}')


def test_sample_refusals():
    lib = _lib.load()
    for name in ('d_uniforms', 'd_indices'):
        assert _call(lib, 'tonic_priority_sample', **{name: None}) == INVALID
        assert _message(lib) == f'tonic_priority_sample: {name} is NULL'
    for B in (0, -7, 2 ** 20 + 1):
        assert _call(lib, 'tonic_priority_sample', B=B) == INVALID
        assert _message(lib) == f'tonic_priority_sample: B = {B} (1 .. 2^20)'
    for beta, text in ((-0.5, '-0.5'), (math.inf, 'inf'), (math.nan, 'nan')):
        assert _call(lib, 'tonic_priority_sample', beta=beta) == INVALID
        assert _message(lib).replace('-nan', 'nan') == f'tonic_priority_sample: beta {text} (finite and >= 0)'


def test_update_refusals():
    lib = _lib.load()
    for name in ('d_indices', 'd_sample_losses'):
        assert _call(lib, 'tonic_priority_update', **{name: None}) == INVALID
        assert _message(lib) == f'tonic_priority_update: {name} is NULL'
    for B in (0, -1, 1025):
        assert _call(lib, 'tonic_priority_update', B=B) == INVALID
        assert _message(lib) == f'tonic_priority_update: B = {B} (1 .. 1024: one workgroup recomputes the ancestors)'
    for changes in (dict(alpha=-1.0), dict(alpha=math.inf), dict(epsilon=-1e-6), dict(epsilon=math.nan)):
        assert _call(lib, 'tonic_priority_update', **changes) == INVALID
        assert _message(lib).startswith('tonic_priority_update: alpha ')
        assert _message(lib).endswith('(finite and >= 0)')


def _weighted(lib, entry, B=17, NA=51, workspace_short=0):
    twin = 'twin' in entry
    O, H, A = 17, 64, 6
    query = lib.tonic_twin_distributional_workspace_bytes if twin else lib.tonic_distributional_workspace_bytes
    size = query(17, O, A, H, 51) - workspace_short
    head = [FAKE] * 5 + [5.0] + [FAKE] * (8 if twin else 7) + [B, O, H, A, NA]
    return getattr(lib, entry)(*head, *((0.2, 0.5) if twin else ()), FAKE, FAKE, FAKE, size, None)


@pytest.mark.parametrize('entry', ['tonic_weighted_distributional_q_grad',
                                   'tonic_weighted_twin_distributional_q_grad'])
def test_weighted_entries_refuse_like_the_plain_ones_under_their_own_name(entry):
    lib = _lib.load()
    for changes in (dict(B=0), dict(NA=1), dict(NA=65)):
        assert _weighted(lib, entry, **changes) == INVALID
        assert _message(lib) == f'{entry}: bad argument (2 <= atoms <= 64)'
    assert _weighted(lib, entry, workspace_short=1) == WORKSPACE
    assert _message(lib) == f'{entry}: workspace too small'


def test_constructor_and_uniform_stream():
    replay = PrioritizedBuffer(size=400, return_steps=5, batch_iterations=6, batch_size=20)
    assert isinstance(replay, replays.Buffer)
    assert (replay.alpha, replay.beta, replay.epsilon) == (0.6, 0.4, 1e-6)
    assert (replay.full_max_size, replay.return_steps, replay.batch_iterations, replay.batch_size) == (400, 5, 6, 20)
    replay = PrioritizedBuffer(batch_iterations=6, batch_size=20, alpha=0.7, beta=0.5, epsilon=1e-3)
    assert (replay.alpha, replay.beta, replay.epsilon) == (0.7, 0.5, 1e-3)
    replay.initialize(seed=11)
    expected = np.random.RandomState(11)
    first = replay.sample_uniforms()
    assert first.dtype == np.float64 and first.shape == (6, 20)
    assert np.array_equal(first, expected.random_sample((6, 20)))
    assert np.array_equal(replay.sample_uniforms(3), expected.random_sample((3, 20)))
    assert replay.graph_signature()[:3] == (0.7, 0.5, 1e-3)
    with pytest.raises(NotImplementedError, match='sample_uniforms'):
        replay.sample_indices()


@pytest.mark.parametrize('name', ['alpha', 'beta', 'epsilon'])
@pytest.mark.parametrize('value', [-0.1, math.inf, math.nan])
def test_constructor_refuses_hyperparameters(name, value):
    with pytest.raises(ValueError, match=f'PrioritizedBuffer: {name} = '):
        PrioritizedBuffer(**{name: value})


@pytest.mark.parametrize('batch_size', [0, 1025])
def test_constructor_refuses_batch_sizes(batch_size):
    with pytest.raises(ValueError, match='PrioritizedBuffer: batch_size = '):
        PrioritizedBuffer(batch_size=batch_size)


def test_several_ranks_are_refused_by_name(monkeypatch):
    monkeypatch.setattr(parallel, 'world_size', lambda: 2)
    with pytest.raises(NotImplementedError, match='PrioritizedBuffer on 2 ranks'):
        PrioritizedBuffer().initialize(seed=0)


def _spaces():
    box = lambda n: types.SimpleNamespace(shape=(n,), low=-np.ones(n, np.float32), high=np.ones(n, np.float32))
    return box(5), box(2)


@pytest.mark.parametrize('agent, updater', [('SAC', 'TwinCriticSoftQLearning'),
                                            ('DDPG', 'DeterministicQLearning'),
                                            ('TD3', 'TwinCriticDeterministicQLearning'),
                                            ('MPO', 'ExpectedSARSA')])
def test_other_agents_are_refused_by_name(agent, updater):
    from tonic_amd.torch import agents
    with pytest.raises(NotImplementedError) as refusal:
        getattr(agents, agent)(replay=PrioritizedBuffer()).initialize(*_spaces(), seed=0)
    text = str(refusal.value)
    assert f'PrioritizedBuffer with the critic updater {updater} is not served' in text
    assert 'DistributionalDeterministicQLearning and TwinCriticDistributionalDeterministicQLearning' in text


def test_reference_descent_rule():
    """The NumPy reference itself on a tree small enough to do by hand."""
    tree = prioritized_ref.Tree(4, [1.0, 0.0, 2.0, 1.0])
    assert tree.total == 4.0
    assert [tree.descend(u)[0] for u in (0.0, 0.2499, 0.25, 0.74, 0.75, 1 - 2.0 ** -53)] == [0, 0, 2, 2, 3, 3]
    assert np.allclose(tree.weights(np.array([0, 2, 3]), 0.5), [1.0, 0.5 ** 0.5, 1.0])
    written = tree.update(np.array([2, 0, 2]), np.array([1.0, 3.0, 8.0], np.float32), 1.0, 0.0)
    assert written == {2: np.float32(8.0), 0: np.float32(3.0)} and tree.max_leaf == np.float32(8.0)
    assert tree.total == 12.0
    wide = prioritized_ref.Tree(4097, np.ones(4097))
    assert wide.sizes == [4097, 65, 2] and wide.total == 4097.0
    assert wide.descend(4096.5 / 4097)[0] == 4096 and wide.descend(0.0)[0] == 0
