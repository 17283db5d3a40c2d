"""The host's half of a pushed collector step without a GPU (csrc/collector.hip tonic_collector_synthetic_step):
a block in ordinary memory, an ordinary-memory buffer standing in for the device window (as
tests/test_host_logic.py::test_push_protocol_of_the_block_header_on_ordinary_memory sets it up).  One call must
leave every byte of the block and of the window exactly where the order of operations BEFORE the chunked
publishing left it — that order is restated in NumPy here."""
import os

import numpy as np
import pytest

WORKERS = (1, 15, 16, 17, 33, 256, 300)
OBSERVATION_SIZES = (1, 3, 17, 28)
ACTION_SIZES = (1, 6, 8)
SENTINEL = 0xCD


def header_words():
    """Indices (in 8-byte words of the header) of `armed` and `command`, found as tests/test_host_logic.py finds
    them: arm a pattern through every zero 64-byte slot and see which one a ring moves, and where to."""
    from tonic_amd import _lib
    from tonic_amd.collector import Block
    lib = _lib.load()
    block = Block(2, 2, 2)
    head = np.frombuffer(block.memory, np.uint64, 512, 0)
    for slot in range(16, 512, 8):
        if head[slot] != 0:
            continue
        before = head.copy()
        head[slot] = (7 << 32) | 0x106
        if lib.tonic_collector_ring(block.address) == 1:
            command = [i for i in range(512) if head[i] != before[i] and head[i] == (7 << 32) | 0x106][0]
            return slot, command
        head[slot] = 0
    raise AssertionError('no armed word found in the block header')


@pytest.fixture(scope='module')
def words():
    armed, command = header_words()
    # (BlockHeader: act_seq is the 64-byte line in front of `command`, the window's address the line behind
    #  `armed`, its owner's pid the int32 behind the address)
    return dict(armed=armed, command=command, act_seq32=2 * (command - 8), window=armed + 8,
                pid32=2 * (armed + 8) + 2)


def placed(count, dtype, remainder):
    """`count` items of `dtype` in fresh memory whose address is `remainder` modulo 64."""
    raw = np.zeros(count * np.dtype(dtype).itemsize + 128, np.uint8)
    start = (remainder - raw.ctypes.data) % 64
    return raw[start:start + count * np.dtype(dtype).itemsize].view(dtype)


def rewards_left_to_right(actions):
    """-sum_k a[w][k]^2 in float32, one product and one addition at a time, k ascending."""
    total = np.zeros(actions.shape[0], np.float32)
    for k in range(actions.shape[1]):
        total = (total + actions[:, k] * actions[:, k]).astype(np.float32)
    return -total


class Case:
    """A block with recognisable contents, a window of sentinel bytes that this process owns (or not), and
    images of both that `parent_order` brings to what the call must leave."""

    def __init__(self, words, W, O, A, misaligned, seed, own_window=True):
        from tonic_amd import _lib
        from tonic_amd.collector import Block
        self.lib, self.words, self.W, self.O, self.A = _lib.load(), words, W, O, A
        rng = np.random.RandomState(seed)
        self.block = block = Block(W, O, A)
        block.actions[:] = rng.standard_normal((W, A)).astype(np.float32) * 3
        block.observations[:] = 11.0
        block.next_observations[:] = 12.0
        block.rewards[:] = 13.0
        self.rows = placed(W * O, np.float32, 4 if misaligned else 0).reshape(W, O)
        assert self.rows.ctypes.data % 64 == (4 if misaligned else 0)
        self.rows[:] = rng.standard_normal((W, O)).astype(np.float32)
        self.window = placed(block.nbytes, np.uint8, 0)
        self.window[:] = SENTINEL
        self.head = np.frombuffer(block.memory, np.uint64, 512, 0)
        self.head32 = np.frombuffer(block.memory, np.uint32, 1024, 0)
        if own_window is not None:
            self.head[words['window']] = self.window.ctypes.data
            self.head32[words['pid32']] = os.getpid() + (0 if own_window else 1)
        self.offset = {name: self.lib.tonic_collector_block_offset(block.address, index)
                       for name, index in (('observations', 1), ('next_observations', 2), ('rewards', 3))}

    def call(self, armed_word, ring, actions=None):
        self.head[self.words['armed']] = armed_word
        self.want_block = bytearray(self.block.memory[:])
        self.want_window = self.window.copy()
        self.parent_order(armed_word, ring, actions)
        status = self.lib.tonic_collector_synthetic_step(
            self.block.address, self.rows.ctypes.data, None if actions is None else actions.ctypes.data, ring)
        assert status == 0

    def parent_order(self, armed_word, ring, actions):
        """tonic_collector_synthetic_step as it was before the chunks: NEXT_OBSERVATIONS, [OBSERVATIONS when
        nothing is pushed], the rewards, [the window's rows, then] the armed command, [OBSERVATIONS]."""
        W, O, words = self.W, self.O, self.words
        image = np.frombuffer(self.want_block, np.uint8)
        head, head32 = image[:4096].view(np.uint64), image[:4096].view(np.uint32)
        field = lambda memory, name, count: memory[self.offset[name]:self.offset[name] + 4 * count].view(np.float32)
        owned = head[words['window']] != 0 and head32[words['pid32']] == os.getpid()
        foreign = head[words['window']] != 0 and not owned
        pushes = bool(ring) and armed_word != 0 and owned
        field(image, 'next_observations', W * O)[:] = self.rows.ravel()
        if not pushes:
            field(image, 'observations', W * O)[:] = self.rows.ravel()
        field(image, 'rewards', W)[:] = rewards_left_to_right(self.block.actions if actions is None else actions)
        if pushes:
            field(self.want_window, 'observations', W * O)[:] = self.rows.ravel()
        if ring and armed_word != 0 and not foreign:
            head[words['armed']] = 0
            head32[words['act_seq32']] = armed_word >> 32
            head[words['command']] = armed_word
            if owned:
                self.want_window[:4096].view(np.uint64)[words['command']] = armed_word
        if pushes:
            field(image, 'observations', W * O)[:] = self.rows.ravel()

    def check(self, what):
        got = np.frombuffer(self.block.memory, np.uint8)
        want = np.frombuffer(self.want_block, np.uint8)
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0])
            raise AssertionError(f'{what}: the block differs from the parent order first at byte {at}')
        if not np.array_equal(self.window, self.want_window):
            at = int(np.flatnonzero(self.window != self.want_window)[0])
            raise AssertionError(f'{what}: the window differs from the parent order first at byte {at}')


@pytest.mark.parametrize('misaligned', (False, True), ids=('aligned', 'source+4'))
@pytest.mark.parametrize('W', WORKERS)
def test_a_pushed_step_leaves_what_the_parent_order_left(words, W, misaligned):
    for O in OBSERVATION_SIZES:
        for A in ACTION_SIZES:
            what = f'W={W} O={O} A={A}'
            case = Case(words, W, O, A, misaligned, seed=W * 1000 + O * 10 + A)
            block, window, rows = case.block, case.window, case.rows
            word = (41 << 32) | 0x206
            case.call(word, 1)
            # field by field ...
            span = slice(case.offset['observations'], case.offset['observations'] + 4 * W * O)
            assert window[span].tobytes() == rows.tobytes(), what
            assert block.next_observations.tobytes() == rows.tobytes(), what
            assert block.observations.tobytes() == rows.tobytes(), what
            assert block.rewards.tobytes() == rewards_left_to_right(block.actions).tobytes(), what
            assert window[:4096].view(np.uint64)[words['command']] == word, what
            assert case.head[words['armed']] == 0 and case.head32[words['act_seq32']] == 41, what
            # ... nothing else of the window was touched ...
            rest = window.copy()
            rest[span] = SENTINEL
            rest[:4096].view(np.uint64)[words['command']] = np.uint64(0xCDCDCDCDCDCDCDCD)
            assert (rest == SENTINEL).all(), what
            # ... and every byte is where the parent's order of operations put it
            case.check(what)
            # a second step through the same block, with the actions handed over explicitly
            rows[:] = rows[::-1] * 0.5
            actions = np.random.RandomState(W + O + A).standard_normal((W, A)).astype(np.float32)
            case.call((42 << 32) | 0x306, 1, actions)
            assert block.rewards.tobytes() == rewards_left_to_right(actions).tobytes(), what
            assert case.head32[words['act_seq32']] == 42, what
            case.check(what + ' (explicit actions)')


@pytest.mark.parametrize('W', WORKERS)
def test_a_step_that_issues_nothing_leaves_the_window_alone(words, W):
    O, A = 17, 6
    for armed_word, ring, own_window in ((0, 1, True), ((9 << 32) | 0x206, 0, True), (0, 0, True),
                                         ((9 << 32) | 0x206, 1, False), ((9 << 32) | 0x206, 1, None)):
        what = f'W={W} armed={armed_word:#x} ring={ring} window={own_window}'
        case = Case(words, W, O, A, True, seed=W, own_window=own_window)
        case.call(armed_word, ring)
        assert (case.window == SENTINEL).all(), what
        assert case.block.observations.tobytes() == case.rows.tobytes(), what
        assert case.block.next_observations.tobytes() == case.rows.tobytes(), what
        assert case.block.rewards.tobytes() == rewards_left_to_right(case.block.actions).tobytes(), what
        issued = bool(ring) and armed_word != 0 and own_window is None          # (a pull collector's ring)
        assert case.head[words['armed']] == (0 if issued else armed_word), what
        assert case.head[words['command']] == (armed_word if issued else 0), what
        case.check(what)


@pytest.mark.parametrize('A', ACTION_SIZES)
def test_both_paths_of_the_synthetic_step_write_the_same_record(A):
    """SyntheticBatch.step handed the block's own actions (the host call) and handed a copy of them (NumPy)."""
    from tonic_amd import environments
    W, O = 33, 17
    envs = [environments.SyntheticBatch(W, O, A, pool=4) for _ in range(2)]
    rng = np.random.RandomState(A)
    for env in envs:
        env.initialize(seed=2)
        env.start()
    for t in range(5):
        actions = (rng.standard_normal((W, A)) * 3).astype(np.float32)
        for env in envs:
            env.block.actions[:] = actions
        envs[0].step(envs[0].block.out_actions)
        envs[1].step(actions.copy())
        for field in ('observations', 'next_observations', 'rewards'):
            assert getattr(envs[0].block, field).tobytes() == getattr(envs[1].block, field).tobytes(), (t, field)
        assert envs[0].block.rewards.tobytes() == rewards_left_to_right(actions).tobytes(), t
