"""The replay kernels held BIT FOR BIT at their chunk and launch edges: tonic_meanstd_record, tonic_segment_store,
tonic_buffer_store (its own launch and the store role of the acting launch), tonic_buffer_accumulate_n_steps,
tonic_buffer_gather and tonic_segment_gather.

The reference's Buffer.store, accumulate_n_steps, Segment.store, fancy-indexed gathers and MeanStd.record are
elementwise float32 in a fixed order, so the expected result is known exactly: plain NumPy copies,
numpy_port.buffer_discounts, numpy_port.BufferPort and numpy_port.MeanStdPort (each pinned on goldens of the reference
by tests/test_oracle_golden.py).  No comparison in this file has a tolerance.

The arena rule: every destination of a direct kernel call is a slice of one larger tensor pre-filled with NaN, with at
least 64 NaNs before and after it.  After the launch the destination equals the reference as uint32 (a NaN of the
reference must be a NaN, of any payload), and everything else in the arena is still NaN: a write outside `row`, past
W * O or into a neighbouring row is seen.
"""
import numpy as np
import pytest

import numpy_port as port
from test_oracle_golden import nstep_golden_cases

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

GUARD = 64                        # floats of NaN around every destination
F32 = np.float32
STORE_KEYS = ('observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations')


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda().contiguous()


def assert_bits(got, want, what):
    """`got` is `want` bit for bit; where `want` is NaN, `got` is a NaN."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f'{what}: {(~np.isnan(got[nan])).sum()} elements are not NaN where the reference is'
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    if differ.any():
        first = tuple(int(i) for i in np.argwhere(differ)[0])
        raise AssertionError(f'{what}: {differ.sum()} of {differ.size} elements differ, first at {first}: '
                             f'got {got[first]!r}, want {want[first]!r}')


class Arena:
    """Named destinations inside one NaN-filled device tensor, GUARD or more NaNs on either side of each (every
    destination starts on a 256-byte boundary, like an allocation of its own)."""

    def __init__(self, **shapes):
        self.slots, offset = {}, GUARD
        for name, shape in shapes.items():
            count = int(np.prod(shape))
            self.slots[name] = (offset, count, tuple(shape))
            offset += (count + GUARD + 63) // 64 * 64
        self.flat = torch.full((offset,), float('nan'), dtype=torch.float32, device='cuda')

    def __getitem__(self, name):
        offset, count, shape = self.slots[name]
        return self.flat[offset:offset + count].view(shape)

    def check(self, what, **expected):
        assert set(expected) == set(self.slots)
        got = self.flat.cpu().numpy()
        outside = np.ones(got.shape[0], bool)
        for name, (offset, count, shape) in self.slots.items():
            outside[offset:offset + count] = False
            assert_bits(got[offset:offset + count].reshape(shape), expected[name], f'{what}: {name}')
        assert outside.sum() >= GUARD * (len(self.slots) + 1)
        assert np.isnan(got[outside]).all(), f'{what}: {(~np.isnan(got[outside])).sum()} floats written outside'


def started_sums(size, rng):
    """A MeanStdPort that has recorded two rows already, and those sums as the kernels' float32[2 * size]."""
    ref = port.MeanStdPort((size,))
    ref.record((rng.standard_normal((2, size)) * 2 - 1).astype(F32))
    return ref, np.concatenate([ref.new_sum, ref.new_sum_sq]).astype(F32)


def sums_of(ref):
    return np.concatenate([ref.new_sum, ref.new_sum_sq]).astype(F32)


# ------------------------------------------------------------------------------------- (a) tonic_meanstd_record

def record_row_counts(size):
    """One, two and three chunks of per = 4096 // size rows (csrc/replay.hip: kQuarter / size), an even and an odd
    number of 16-row batches in a chunk, empty and non-empty tails; for sizes 1 and 2 the float counts either side of
    the 8-way unrolled fetch of the first chunk (256 threads: 2048 floats) and of a later one (128 threads: 1024)."""
    per = 4096 // size
    rows = [1, 15, 16, 17, 31, 32, 33, per - 1, per, per + 1, 2 * per, 2 * per + 17, 3 * per + 1]
    if size <= 2:
        for floats in (2047, 2048, 2049):
            rows += [floats // size, (floats + size - 1) // size]
        for floats in (1023, 1024, 1025):
            rows += [per + floats // size, per + (floats + size - 1) // size]
    return sorted(set(rows))


@pytest.mark.parametrize('size', [1, 2, 33, 63, 64])
def test_meanstd_record_at_every_chunk_and_batch_edge(lib, size):
    """tonic_meanstd_record == MeanStdPort.record from non-zero sums, at every row count of record_row_counts: the
    record is sequential, so the sums after n rows of one stream are the reference's state after its n-th row."""
    from tonic_amd import _lib
    counts = record_row_counts(size)
    if size == 1:
        assert {2047, 2048, 2049, 4096 + 1023, 4096 + 1024, 4096 + 1025} <= set(counts)
    if size == 2:
        assert {1023, 1024, 1025, 2048 + 511, 2048 + 512, 2048 + 513} <= set(counts)
    rng = np.random.RandomState(100 + size)
    values = (rng.standard_normal((counts[-1], size)) * 3 + 1).astype(F32)
    ref, start = started_sums(size, rng)
    want, done = {}, 0
    for n in counts:
        ref.record(values[done:n])
        done = n
        want[n] = sums_of(ref)
    d_values = dev(values)
    for n in counts:
        arena = Arena(sums=(2 * size,))
        arena['sums'].copy_(dev(start))
        _lib.check(lib.tonic_meanstd_record(d_values.data_ptr(), arena['sums'].data_ptr(), n, size, None),
                   'tonic_meanstd_record')
        arena.check(f'size {size}, {n} rows', sums=want[n])


# ------------------------------------------------------------------- (b) tonic_segment_store, tonic_buffer_store

# 16-row chunks (O = 1024, 1023: record_rows' unrolled body once, then with a tail), 252-row chunks (O = 65) either
# side of one and two chunks, two workgroups, and one shape past the cap of 256 workgroups
STORE_SHAPES = [(1, 1, 1), (16, 1024, 3), (17, 1024, 3), (33, 1023, 1), (251, 65, 7), (252, 65, 7), (253, 65, 7),
                (505, 65, 7), (300, 17, 6), (2100, 500, 20)]
T, ROW = 3, 1


def store_workgroups(W, O, A):
    return min(256, (W * (2 * O + A + 4) + 8 * 1024 - 1) // (8 * 1024))


def test_store_shapes_are_the_edges_they_are_meant_to_be():
    assert 16384 // 1024 == 16 and 16384 // 1023 == 16 and 16384 // 65 == 252
    assert store_workgroups(300, 17, 6) == 2
    assert 2100 * (2 * 500 + 20 + 4) > 256 * 8192 and store_workgroups(2100, 500, 20) == 256
    assert store_workgroups(1, 1, 1) == 1


def transition(W, O, A, rng, log_probs=False):
    """One time row on the host, float32, with a NaN, an infinity and zeros of both signs among the scalars."""
    row = dict(observations=(rng.standard_normal((W, O)) * 3 + 1).astype(F32),
               actions=rng.uniform(-1, 1, (W, A)).astype(F32),
               next_observations=rng.standard_normal((W, O)).astype(F32),
               rewards=rng.standard_normal(W).astype(F32),
               resets=(rng.uniform(size=W) < 0.3).astype(F32),
               terminations=(rng.uniform(size=W) < 0.4).astype(F32))
    row['terminations'][0], row['terminations'][-1] = 1.0, 0.0
    row['rewards'][0] = -0.0
    row['next_observations'][-1, -1] = np.inf
    if W > 2:
        row['rewards'][1], row['rewards'][2] = np.nan, 0.0
    if log_probs:
        row['log_probs'] = rng.standard_normal(W).astype(F32)
    return row


def in_row(values, shape):
    """A [T, ...] destination that holds `values` in row ROW and NaN elsewhere."""
    out = np.full((T,) + tuple(shape), np.nan, F32)
    out[ROW] = values
    return out


@pytest.mark.parametrize('W,O,A', STORE_SHAPES)
def test_segment_store_writes_one_row_and_records_bit_exact(lib, W, O, A):
    """tonic_segment_store into row 1 of a T = 3 Segment: the row is the transition, the other rows and the guard
    bands stay NaN, the sums are MeanStdPort's; with norm_acc == NULL the sums are untouched."""
    from tonic_amd import _lib
    rng = np.random.RandomState(W * 31 + O)
    row = transition(W, O, A, rng, log_probs=True)
    keys = STORE_KEYS + ('log_probs',)
    sources = [dev(row[k]) for k in keys]
    ref, start = started_sums(O, rng)
    ref.record(row['observations'])
    shapes = dict(observations=(T, W, O), actions=(T, W, A), next_observations=(T, W, O), rewards=(T, W),
                  resets=(T, W), terminations=(T, W), log_probs=(T, W))
    want = {k: in_row(row[k], shapes[k][1:]) for k in keys}
    for record in (True, False):
        arena = Arena(sums=(2 * O,), **shapes)
        arena['sums'].copy_(dev(start))
        _lib.check(lib.tonic_segment_store(
            *[arena[k].data_ptr() for k in keys], *[s.data_ptr() for s in sources],
            arena['sums'].data_ptr() if record else None, ROW, W, O, A, None), 'tonic_segment_store')
        arena.check(f'segment store {(W, O, A)} record={record}', sums=sums_of(ref) if record else start, **want)


@pytest.mark.parametrize('W,O,A', STORE_SHAPES)
def test_buffer_store_writes_one_row_discounts_and_records_bit_exact(lib, W, O, A):
    """tonic_buffer_store (its own launch: 1024 threads, up to 256 workgroups, a 16384-float tile): the same, plus
    discounts = float32(1 - terminations) * discount_factor for discount factors 0.99, 1 and 0."""
    from tonic_amd import _lib
    rng = np.random.RandomState(W * 37 + O)
    row = transition(W, O, A, rng)
    assert 0 < row['terminations'].sum() < W or W == 1
    sources = [dev(row[k]) for k in STORE_KEYS]
    ref, start = started_sums(O, rng)
    ref.record(row['observations'])
    shapes = dict(observations=(T, W, O), actions=(T, W, A), next_observations=(T, W, O), rewards=(T, W),
                  resets=(T, W), terminations=(T, W), discounts=(T, W))
    want = {k: in_row(row[k], shapes[k][1:]) for k in STORE_KEYS}
    keys = STORE_KEYS + ('discounts',)
    for discount_factor, record in ((0.99, True), (1.0, True), (0.0, True), (0.99, False)):
        discounts = port.buffer_discounts(row['terminations'] != 0, discount_factor)
        assert discounts.dtype == F32
        arena = Arena(sums=(2 * O,), **shapes)
        arena['sums'].copy_(dev(start))
        _lib.check(lib.tonic_buffer_store(
            *[arena[k].data_ptr() for k in keys], *[s.data_ptr() for s in sources],
            arena['sums'].data_ptr() if record else None, ROW, W, O, A, discount_factor, None), 'tonic_buffer_store')
        arena.check(f'buffer store {(W, O, A)} discount_factor={discount_factor} record={record}',
                    sums=sums_of(ref) if record else start, discounts=in_row(discounts, (W,)), **want)


# --------------------------------------------------------------------- (c) tonic_buffer_accumulate_n_steps

def device_buffer(W, max_size, return_steps, discount_factor=0.99):
    import tonic_amd
    replay = tonic_amd.replays.Buffer(size=max_size * W, return_steps=return_steps, discount_factor=discount_factor)
    replay.initialize(seed=0, device='cuda')
    return replay


def assert_buffers(replay, ref, what):
    assert (replay.index, replay.size, replay.max_size) == (ref.index, ref.size, ref.max_size), what
    for key in ref.KEYS:
        assert_bits(replay.buffers[key].cpu().numpy(), ref.buffers[key], f'{what}: {key}')


def replay_through_both(replay, ref, rows, what, after=None):
    """Every row through Buffer.store and BufferPort.store, every buffer compared after every store."""
    stacked = {k: dev(np.stack([np.asarray(r[k], F32) for r in rows])) for k in STORE_KEYS}
    for t, row in enumerate(rows):
        with np.errstate(invalid='ignore'):                   # (0 * inf where a test asks for it)
            ref.store(**row)
        replay.store(**{k: v[t] for k, v in stacked.items()})
        assert_buffers(replay, ref, f'{what}, store {t}')
        if after is not None:
            after(t)


RESETS = ('none', 'all', 'random', 'alternate')


def nstep_rows(W, O, stores, pattern, rng):
    rows = []
    for t in range(stores):
        resets = dict(none=np.zeros(W, bool), all=np.ones(W, bool), random=rng.uniform(size=W) < 0.25,
                      alternate=rng.uniform(size=W) < 0.1)[pattern]
        if pattern == 'alternate':
            resets[W // 2] = t % 2 == 1                        # a worker that resets on every second step
        rows.append(dict(observations=rng.standard_normal((W, O)).astype(F32),
                         actions=rng.uniform(-1, 1, (W, 2)).astype(F32),
                         next_observations=rng.standard_normal((W, O)).astype(F32),
                         rewards=rng.standard_normal(W).astype(F32),
                         resets=resets.astype(F32), terminations=(rng.uniform(size=W) < 0.15).astype(F32)))
    return rows


# W * O = 255, 256, 257, 258 and 513 threads (256 per workgroup), thin and wide
@pytest.mark.parametrize('W,O', [(1, 255), (85, 3), (256, 1), (4, 64), (1, 257), (257, 1), (3, 86), (129, 2),
                                 (19, 27), (1, 513)])
def test_n_step_accumulation_across_workgroups_and_the_wrap(W, O):
    """Buffer.store with return_steps 2, 3, 9 on max_size 2, 5, 12 (return_steps - 1 >= max_size: the chain runs the
    full circle) against BufferPort after each of 2 * max_size + 3 stores, under four reset patterns."""
    assert W * O in (255, 256, 257, 258, 513)
    for return_steps in (2, 3, 9):
        for max_size in (2, 5, 12):
            for pattern in RESETS:
                rng = np.random.RandomState(W * 1000 + O * 10 + return_steps + max_size)
                replay = device_buffer(W, max_size, return_steps)
                ref = port.BufferPort(max_size * W, W, return_steps=return_steps)
                rows = nstep_rows(W, O, 2 * max_size + 3, pattern, rng)
                replay_through_both(replay, ref, rows,
                                    f'W={W} O={O} return_steps={return_steps} max_size={max_size} resets={pattern}')
                assert replay.size == max_size and replay.index == (2 * max_size + 3) % max_size


@pytest.mark.parametrize('name', ['buffer_nstep', 'buffer_nstep_edges'])
def test_n_step_goldens_replayed_through_the_device_buffer(golden, name):
    """What the reference's own Buffer left behind (tests/golden/buffer_nstep*.npz: the edges are signed zero
    rewards, an infinite reward behind a cut chain — 0 * inf is NaN exactly where the reference's is, nothing
    selects it away —, a NaN next observation, return_steps - 1 >= max_size down to max_size 1, discount factors 1
    and 0) is what Buffer.store leaves on the device, bit for bit, early and at the end."""
    g = golden(name)
    for pre, workers, size, steps, index, filled, discount, rows in nstep_golden_cases(g):
        replay = device_buffer(workers, size // workers, steps, discount)
        ref = port.BufferPort(size, workers, return_steps=steps, discount_factor=discount)

        def early(t):
            if t == 3:
                for key in ref.KEYS:
                    assert_bits(replay.buffers[key].cpu().numpy(), g[pre + 'early_' + key], f'{name} {pre} early {key}')
        replay_through_both(replay, ref, rows, f'{name} {pre}', early)
        assert (replay.index, replay.size) == (index, filled)
        for key in ref.KEYS:
            assert_bits(replay.buffers[key].cpu().numpy(), g[pre + 'buf_' + key], f'{name} {pre} {key}')


# ------------------------------------------------------------------------------------------------ (d) gathers

GATHER_WIDTHS = [(1, 1), (64, 64), (65, 65), (130, 3), (3, 130)]      # either side of the 64-lane strides
BATCH_KEYS = ('observations', 'actions', 'next_observations', 'rewards', 'discounts')


def gather_indices(B, total, rng):
    """B indices with 0, the last transition and a duplicate among them as far as B allows."""
    indices = rng.randint(total, size=B)
    for at, value in enumerate((total - 1, 0, total - 1, total // 2, total // 2)[:B]):
        indices[at] = value
    return indices.astype(np.int64)


@pytest.mark.parametrize('O,A', GATHER_WIDTHS)
def test_buffer_gather_equals_fancy_indexing(O, A):
    """tonic_buffer_gather (4 waves per workgroup, one per sampled transition) through Buffer.gather and
    Buffer.gather_many into NaN arenas == buffers[k][idx // W, idx % W], for B either side of a workgroup."""
    import tonic_amd
    rows = 6
    for W in (1, 7):
        rng = np.random.RandomState(O * 100 + A + W)
        replay = tonic_amd.replays.Buffer(size=rows * W, batch_size=4)
        replay.initialize(seed=0, device='cuda')
        replay._allocate(W, O, A)
        host = {k: rng.standard_normal(tuple(v.shape)).astype(F32) for k, v in replay.buffers.items()}
        host['rewards'][0, 0], host['rewards'][-1, -1] = -0.0, np.inf
        for k, v in replay.buffers.items():
            v.copy_(dev(host[k]))
        replay.size = rows
        widths = dict(observations=(O,), actions=(A,), next_observations=(O,))

        def expected(indices):
            return {k: host[k][indices // W, indices % W] for k in BATCH_KEYS}
        for B in (1, 3, 4, 5, 9):
            indices = gather_indices(B, rows * W, rng)
            assert indices.min() == 0 and indices.max() == rows * W - 1 or B == 1
            arena = Arena(**{k: (B,) + widths.get(k, ()) for k in BATCH_KEYS})
            d_indices = dev(indices, torch.int64)
            replay.gather(d_indices, out={k: arena[k] for k in BATCH_KEYS})
            arena.check(f'gather O={O} A={A} W={W} B={B}', **expected(indices))
        for iterations, B in ((3, 5), (2, 9), (1, 1), (7, 3)):
            assert iterations * B % 4 != 0
            indices = np.stack([gather_indices(B, rows * W, rng) for _ in range(iterations)])
            arena = Arena(**{k: (iterations, B) + widths.get(k, ()) for k in BATCH_KEYS})
            replay._many = {k: arena[k] for k in BATCH_KEYS}      # (gather_many reuses a store of this shape)
            d_indices = dev(indices, torch.int64)
            out = replay.gather_many(d_indices)
            assert all(out[k].data_ptr() == arena[k].data_ptr() for k in BATCH_KEYS)
            want = expected(indices.reshape(-1))
            arena.check(f'gather_many O={O} A={A} W={W} {iterations}x{B}',
                        **{k: v.reshape((iterations, B) + v.shape[1:]) for k, v in want.items()})


@pytest.mark.parametrize('O,A', GATHER_WIDTHS)
def test_segment_gather_equals_fancy_indexing_and_skips_what_is_out_of_range(lib, O, A):
    """tonic_segment_gather == v[indices] (segments.py:64); a row whose index is -1 or N is skipped (csrc/replay.hip:
    `if (t < 0 || t >= g.N) return;`): it stays NaN, every other row is exact."""
    from tonic_amd import _lib
    N = 23
    rng = np.random.RandomState(O * 100 + A)
    keys = ('observations', 'actions', 'advantages', 'log_probs', 'returns')
    widths = dict(observations=(O,), actions=(A,))
    host = {k: rng.standard_normal((N,) + widths.get(k, ())).astype(F32) for k in keys}
    host['returns'][0], host['advantages'][N - 1] = -0.0, np.inf
    sources = [dev(host[k]) for k in keys]

    def run(indices, what):
        count = len(indices)
        valid = (indices >= 0) & (indices < N)
        arena = Arena(**{k: (count,) + widths.get(k, ()) for k in keys})
        d_indices = dev(indices, torch.int64)
        _lib.check(lib.tonic_segment_gather(
            d_indices.data_ptr(), *[s.data_ptr() for s in sources],
            *[arena[k].data_ptr() for k in keys], count, N, O, A, None), 'tonic_segment_gather')
        want = {}
        for k in keys:
            want[k] = np.full((count,) + widths.get(k, ()), np.nan, F32)
            want[k][valid] = host[k][indices[valid]]
        arena.check(f'segment gather O={O} A={A} {what}', **want)
    for count in (1, 3, 4, 5, 9):
        run(gather_indices(count, N, rng), f'count={count}')
    for count in (3, 5, 9):
        indices = gather_indices(count, N, rng)
        indices[1] = -1
        indices[count - 1] = N
        run(indices, f'count={count} with -1 and N')


# -------------------------------------------------------------- (e) the store role of the acting launch

def acting_tile_floats(O, H=256):
    """The floats of LDS the acting launch's store role stages the record through: img_lds(K1 = O, H).total / 4 of
    csrc/mlpimg_body.h (16 rows per workgroup; the policy tail's 3 x 16 x 64 floats; 160 floats of row maxima,
    partials and descale factors), restated."""
    def pad32(k):
        return (k + 31) & ~31
    rows, post_pitch = 16, 64
    pa, pb = pad32(max(O, H)) + 8, pad32(H) + 8
    tail = max(3 * rows * post_pitch, 2 * rows * (post_pitch + 4))
    total = 2 * rows * pa * 2 + 2 * rows * pb * 2 + (64 + 64 + 32) * 4 + tail * 4
    assert total <= 128 * 1024                                 # kImgLdsCap
    return total // 4


def acting_agent(kind, W, steps):
    import tonic_amd
    import tonic_amd.torch as tt
    replay = tonic_amd.replays.Buffer(size=W * (steps + 4), batch_iterations=1, batch_size=16,
                                      steps_before_batches=10 ** 9)      # beyond the run: no update interferes
    if kind == 'sac':
        return tt.agents.SAC(replay=replay, exploration=tonic_amd.explorations.NoActionNoise(start_steps=0))
    return tt.agents.TD3(replay=replay, exploration=tonic_amd.explorations.NormalActionNoise(start_steps=0))


def run_acting_store(kind, W, O, A, steps=8):
    """agent.step -> env.step -> agent.update on the environment's own arrays (the default 256-wide torso, the policy
    acting from the first step); BufferPort and MeanStdPort fed what the environment returned.  Returns (what the
    run left on the device, the two ports, whether the policy acted on the environment's block)."""
    import tonic_amd
    env = tonic_amd.environments.distribute(
        lambda: tonic_amd.environments.Synthetic(O, A, max_episode_steps=3), 1, W)
    env.initialize(seed=11)
    agent = acting_agent(kind, W, steps)
    agent.initialize(env.observation_space, env.action_space, seed=4)
    assert agent.hidden is not None                            # (a torso the HIP path serves)
    observations = env.start()
    on_block = agent._q.find(observations, agent.policy_kind) is not None
    ref = port.BufferPort(W * (steps + 4), W)
    sums = port.MeanStdPort((O,))
    for t in range(steps):
        before = observations.copy()
        actions = agent.step(observations, (t + 1) * W)        # steps > start_steps: the policy, never the warm-up
        executed = np.array(actions, F32)
        observations, infos = env.step(actions)
        row = dict(observations=before, actions=executed, next_observations=infos['observations'].copy(),
                   rewards=infos['rewards'].copy(), resets=infos['resets'].copy(),
                   terminations=infos['terminations'].copy())
        agent.update(**infos, steps=(t + 1) * W)
        ref.store(**row)
        sums.record(before)
    agent.settle()
    replay, normalizer = agent.replay, agent.model.observation_normalizer
    out = {k: v.cpu().numpy() for k, v in replay.buffers.items()}
    out.update(index=replay.index, size=replay.size, device_sums=normalizer.device_sums.cpu().numpy(),
               new_count=normalizer.new_count, return_steps=replay.return_steps)
    assert not hasattr(agent, 'last_infos'), 'a learner update ran'
    agent.close()
    return out, ref, sums, on_block


def check_acting_store(monkeypatch, kind, W, O, A, path, steps=8):
    import tonic_amd
    reserved = []
    reserve_row = tonic_amd.replays.Buffer.reserve_row
    monkeypatch.setattr(tonic_amd.replays.Buffer, 'reserve_row',
                        lambda self, *args, **kwargs: reserved.append(1) or reserve_row(self, *args, **kwargs))
    if path == 'block':
        monkeypatch.delenv('TONIC_AMD_Q_BLOCK', raising=False)
    else:
        monkeypatch.setenv('TONIC_AMD_Q_BLOCK', '0')
    out, ref, sums, on_block = run_acting_store(kind, W, O, A, steps)
    if path == 'block':
        # the first transition is stored by a launch of its own (it allocates the Buffer); every later one is
        # reserved and rides in the next acting launch, the last in the launch settle() issues
        assert on_block and len(reserved) == steps - 1, (on_block, len(reserved))
    else:
        assert not on_block and not reserved
    assert out['return_steps'] == 1 and (out['index'], out['size']) == (ref.index, ref.size) == (steps, steps)
    assert out['new_count'] == steps * W
    what = f'{kind} W={W} O={O} A={A} {path}'
    assert (ref.buffers['resets'][:steps] != 0).any() and not (ref.buffers['resets'][:steps] != 0).all()
    for key in ('observations', 'next_observations', 'resets', 'terminations', 'discounts', 'actions', 'rewards'):
        assert_bits(out[key], ref.buffers[key], f'{what}: {key}')
    assert_bits(out['device_sums'], sums_of(sums), f'{what}: device_sums')


@pytest.mark.parametrize('path', ['block', 'staged'])
@pytest.mark.parametrize('kind', ['sac', 'td3'])
def test_acting_launch_store_small_observations(monkeypatch, kind, path):
    """(W, O, A) = (5, 17, 6): buffer_store_body with 256 threads, parts = 1, one chunk, one pass of the k0 loop."""
    assert 5 * 17 <= acting_tile_floats(17)
    check_acting_store(monkeypatch, kind, 5, 17, 6, path)


WIDE_O = (376, 300, 257)


@pytest.mark.parametrize('path', ['block', 'staged'])
@pytest.mark.parametrize('kind', ['sac', 'td3'])
def test_acting_launch_store_more_columns_than_threads(lib, monkeypatch, kind, path):
    """O > 256 with W = 3: the k0 loop of buffer_store_body runs twice (columns [0, 256) and [256, O)).  O is the
    largest of 376, 300, 257 that the fused forward on weight images serves (tonic_mlp_actor_image_bytes > 0, the
    record's rows fit the launch's LDS): O = 376 is served, for SAC and TD3; the block path is asserted taken."""
    A = 6
    served = [O for O in WIDE_O if lib.tonic_mlp_actor_image_bytes(O, 256, A, 2 if kind == 'sac' else 1) > 0
              and O <= acting_tile_floats(O)]
    assert served and served[0] == 376, served
    O = served[0]
    assert O > 256 and 3 * O <= acting_tile_floats(O)
    check_acting_store(monkeypatch, kind, 3, O, A, path)


@pytest.mark.parametrize('path', ['block', 'staged'])
@pytest.mark.parametrize('kind', ['sac', 'td3'])
def test_acting_launch_store_more_rows_than_the_tile(monkeypatch, kind, path):
    """W * O larger than the launch's LDS: the record runs over two chunks, staged by 256 threads."""
    O, A = 17, 6
    tile = acting_tile_floats(O)
    W = tile // O + 13
    assert tile < W * O < 2 * tile
    check_acting_store(monkeypatch, kind, W, O, A, path)
