"""HBM-resident off-policy ``Buffer`` — API of ``tonic/replays/buffers.py``.

Circular float32 store ``[max_size = size // W, W, ...]`` for ``observations, actions,
next_observations, rewards, resets, terminations, discounts``, NaN-initialised like the
reference (buffers.py:45), 936 B per transition at O=111, A=8 (0.94 GB for 1 M transitions).
``store`` is one ``tonic_buffer_store`` launch (row write, ``discounts = float32(1 -
terminations) * discount_factor``, observation-normaliser record) plus, for ``return_steps > 1``,
one ``tonic_buffer_accumulate_n_steps`` launch (buffers.py:58-79, bit-exact); ``get`` draws the indices
with the host ``RandomState`` exactly like buffers.py:86 (bit-exact stream) and gathers the
batch with ``tonic_buffer_gather`` (one wavefront per sampled transition,
``rows = idx // W``, ``cols = idx % W``).
"""
import numpy as np
import torch

from tonic_amd import _lib, parallel

KEYS = ('observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations',
        'discounts')
BATCH_KEYS = ('observations', 'actions', 'next_observations', 'rewards', 'discounts')


class Buffer:
    def __init__(self, size=int(1e6), return_steps=1, batch_iterations=50, batch_size=100,
                 discount_factor=0.99, steps_before_batches=int(1e4), steps_between_batches=50):
        self.full_max_size = size
        self.return_steps = return_steps
        self.batch_iterations = batch_iterations
        self.batch_size = batch_size
        self.discount_factor = discount_factor
        self.steps_before_batches = steps_before_batches
        self.steps_between_batches = steps_between_batches

    def initialize(self, seed=None, device=None):
        self.np_random = np.random.RandomState(seed)
        self.device = torch.device(device if device is not None else 'cuda')
        self.buffers = None
        self.index = 0
        self.size = 0
        self.last_steps = 0
        self.lib = _lib.load()

    def ready(self, steps):
        if steps < self.steps_before_batches:
            return False
        return (steps - self.last_steps) >= self.steps_between_batches

    def _allocate(self, num_workers, observation_size, action_size):
        # Multi-GPU: this rank holds a contiguous shard of the GLOBAL worker axis (equal shards);
        # capacity and the index stream are those of the global [max_size, W_global] buffer.
        self.num_workers = num_workers
        self.rank, self.world = parallel.rank(), parallel.world_size()
        self.global_workers = num_workers * self.world
        self.max_size = self.full_max_size // self.global_workers
        self.observation_size, self.action_size = observation_size, action_size
        widths = dict(observations=(observation_size,), actions=(action_size,), next_observations=(observation_size,))
        self.buffers = {k: torch.full((self.max_size, num_workers) + widths.get(k, ()), float('nan'),
                                      dtype=torch.float32, device=self.device) for k in KEYS}
        self.batch = {k: torch.empty((self.batch_size,) + widths.get(k, ()), device=self.device) for k in BATCH_KEYS}

    def store(self, normalizer=None, **kwargs):
        """One time row from float32 device tensors [W, ...] (buffers.py:33-56)."""
        if self.buffers is None:
            self._allocate(kwargs['observations'].shape[0], kwargs['observations'].shape[1],
                           kwargs['actions'].shape[1])
        self.store_at(self.index, normalizer, **kwargs)
        if self.return_steps > 1:                                    # buffers.py:52-53
            b, p = self.buffers, _lib.ptr
            _lib.check(self.lib.tonic_buffer_accumulate_n_steps(
                p(b['next_observations']), p(b['rewards']), p(b['discounts']), p(b['resets']),
                p(kwargs['next_observations']), p(kwargs['rewards']), p(kwargs['terminations']),
                self.index, self.size, self.max_size, self.num_workers, self.observation_size,
                self.return_steps, float(self.discount_factor), _lib.current_stream()),
                'tonic_buffer_accumulate_n_steps')
        self._take_row(normalizer)

    def _take_row(self, normalizer):
        """The host half of a store (buffers.py:54-56): the circular index and the size advanced, the normaliser's
        record count noted.  Returns the row taken."""
        row = self.index
        if normalizer is not None:
            normalizer.note_device_rows(self.num_workers)
        self.index = (self.index + 1) % self.max_size
        self.size = min(self.size + 1, self.max_size)
        return row

    def reserve_row(self, normalizer=None):
        """The host half of `store` for a transition whose device write is issued later (the off-policy agents'
        acting launch carries it: tonic_collector_q_act): the row it will occupy.  Needs an allocated Buffer and
        return_steps == 1 (the n-step accumulation reads the stored row right away)."""
        assert self.buffers is not None and self.return_steps == 1
        return self._take_row(normalizer)

    def store_at(self, row, normalizer=None, **kwargs):
        """The device half of a store (tonic_buffer_store into `row`) — on its own: what the acting launch would
        have carried for a reserved transition, when no acting launch follows (an update is due first, the policy
        sits out)."""
        p = _lib.ptr
        sums = normalizer.device_sums if normalizer is not None else None
        _lib.check(self.lib.tonic_buffer_store(
            *self._pointers(self.buffers, KEYS), *self._pointers(kwargs, KEYS[:-1]), p(sums), row,
            self.num_workers, self.observation_size, self.action_size,
            float(self.discount_factor), _lib.current_stream()), 'tonic_buffer_store')

    def store_arguments(self, row, observations, normalizer=None):
        """tonic_q_store_t for `row` (see reserve_row): the Buffer's arrays, the observation rows' device copy."""
        sums = normalizer.device_sums if normalizer is not None else None
        return _lib.QStore(*self._pointers(self.buffers, KEYS), _lib.ptr(observations), _lib.ptr(sums),
                           row, float(self.discount_factor))

    @staticmethod
    def _pointers(arrays, keys):
        return [_lib.ptr(arrays[k]) for k in keys]

    def sample_indices(self, iterations=None):
        """The index stream of `iterations` successive Buffer.get draws (buffers.py:85-86)."""
        total = self.size * self.global_workers
        count = self.batch_iterations if iterations is None else iterations
        return np.stack([self.np_random.randint(total, size=self.batch_size)
                         for _ in range(count)])

    def shard_indices(self, indices):
        """Splits GLOBAL flat indices [iterations, B] (rows = idx // W_global, cols = idx %
        W_global, buffers.py:87-88) into this rank's part: returns (local flat indices into the
        [max_size, W_local] shard, positions inside the global batch, counts), the first two
        zero-padded to B per iteration.  Every rank draws the same global stream (same seed), so
        the union over ranks is exactly the single-process batch."""
        iterations, B = indices.shape
        rows, cols = indices // self.global_workers, indices % self.global_workers
        mine = (cols // self.num_workers) == self.rank
        local = np.zeros((iterations, B), np.int64)
        positions = np.zeros((iterations, B), np.int64)
        counts = mine.sum(axis=1)
        for it in range(iterations):
            pos = np.flatnonzero(mine[it])
            positions[it, :len(pos)] = pos
            local[it, :len(pos)] = (rows[it, pos] * self.num_workers
                                    + cols[it, pos] - self.rank * self.num_workers)
        return local, positions, counts

    def gather(self, device_indices, out=None):
        """Gathers one batch (int64 device indices [B]) into `out` (default: the reusable batch)."""
        out = out or self.batch
        count = device_indices.shape[0]
        self._gather(device_indices, count, out)
        if count != out['rewards'].shape[0]:
            return {k: v[:count] for k, v in out.items()}
        return out

    def gather_many(self, device_indices):
        """All batches of one learner update in ONE launch: int64 device indices [iterations, B] ->
        {key: [iterations, B, ...]} (the store does not change while an update runs, so the
        gathers of its iterations need not be interleaved with them)."""
        iterations, count = device_indices.shape
        store = getattr(self, '_many', None)
        if store is None or store['rewards'].shape != (iterations, count):
            store = self._many = {
                k: torch.empty((iterations, count) + tuple(v.shape[1:]), dtype=v.dtype,
                               device=self.device) for k, v in self.batch.items()}
        self._gather(device_indices, iterations * count, store)
        return store

    def _gather(self, device_indices, count, out):
        _lib.check(self.lib.tonic_buffer_gather(
            _lib.ptr(device_indices), *self._pointers(self.buffers, BATCH_KEYS), *self._pointers(out, BATCH_KEYS),
            self.num_workers, count, self.observation_size, self.action_size, _lib.current_stream()),
            'tonic_buffer_gather')

    def get(self, *keys, steps):
        """Generator form of the reference API (buffers.py:81-91): yields device-tensor batches.
        With several ranks every rank draws the same global index stream and yields ITS part of
        each batch (the rows whose worker column it owns, in batch order; possibly none) — the
        fused learner reduces gradient sums over ranks, so the union is the reference's batch."""
        for _ in range(self.batch_iterations):
            indices = self.sample_indices(1)
            if self.world > 1:                 # this rank's part of the global batch
                local, _, counts = self.shard_indices(indices)
                indices = local[:, :counts[0]]
            count = indices.shape[1]
            out = {k: torch.empty((count,) + tuple(v.shape[1:]), dtype=v.dtype, device=self.device)
                   for k, v in self.batch.items()}
            if count > 0:
                device_indices = torch.as_tensor(indices[0], device=self.device)
                out = self.gather(device_indices, out)
            yield {k: out[k] for k in keys}
        self.last_steps = steps


class PrioritizedBuffer(Buffer):
    """Proportional prioritized replay (Schaul et al. 2016, the third part of D4PG): P_i = p_i / sum_j p_j with
    p_i = (loss_i + epsilon)^alpha, importance weights w_i = (N P_i)^-beta over the batch's largest.  The
    priorities live in a sum tree on the device (csrc/priority.hip, include/tonic_hip.h) next to the store: the
    batch of iteration k + 1 depends on the losses of iteration k, so it is drawn there, between the critic steps,
    from uniforms the host drew ahead (`sample_uniforms`, the only host stream).  A stored row starts at the
    largest priority seen so far, a wrapped-around row again.  `alpha`, `beta`, `epsilon` are fixed for the
    lifetime (a captured update graph bakes them in).  One rank only; the priorities are not checkpointed."""

    def __init__(self, size=int(1e6), return_steps=1, batch_iterations=50, batch_size=100,
                 discount_factor=0.99, steps_before_batches=int(1e4), steps_between_batches=50,
                 alpha=0.6, beta=0.4, epsilon=1e-6):
        super().__init__(size, return_steps, batch_iterations, batch_size, discount_factor, steps_before_batches,
                         steps_between_batches)
        for name, value in (('alpha', alpha), ('beta', beta), ('epsilon', epsilon)):
            if not (np.isfinite(value) and value >= 0):
                raise ValueError(f'PrioritizedBuffer: {name} = {value!r} (finite and >= 0)')
        if not 0 < batch_size <= 1024:
            raise ValueError(f'PrioritizedBuffer: batch_size = {batch_size!r} (1 .. 1024: one workgroup recomputes '
                             'the sums above a batch\'s leaves)')
        self.alpha, self.beta, self.epsilon = float(alpha), float(beta), float(epsilon)

    def initialize(self, seed=None, device=None):
        if parallel.world_size() > 1:
            raise NotImplementedError(
                f'PrioritizedBuffer on {parallel.world_size()} ranks is not served: the shards of the store would '
                'need one global priority tree (use Buffer)')
        super().initialize(seed, device)
        self.tree = None

    def _allocate(self, num_workers, observation_size, action_size):
        super()._allocate(num_workers, observation_size, action_size)
        self.capacity = self.max_size * num_workers
        self.tree = torch.empty(self.lib.tonic_priority_tree_bytes(self.capacity), dtype=torch.uint8,
                                device=self.device)
        _lib.check(self.lib.tonic_priority_tree_init(_lib.ptr(self.tree), self.tree.numel(), self.capacity,
                                                     _lib.current_stream()), 'tonic_priority_tree_init')
        self._drawn = (torch.zeros(self.batch_size, dtype=torch.float64, device=self.device),
                       torch.zeros(self.batch_size, dtype=torch.int64, device=self.device),
                       torch.zeros(self.batch_size, dtype=torch.float32, device=self.device))

    def _take_row(self, normalizer):
        """... and the row's leaves set to the largest priority so far (a reserved row, whose data write rides in
        the acting launch, too: nothing samples before the update that follows both)."""
        row = super()._take_row(normalizer)
        _lib.check(self.lib.tonic_priority_store(_lib.ptr(self.tree), self.tree.numel(), self.capacity,
                                                 row * self.num_workers, self.num_workers, _lib.current_stream()),
                   'tonic_priority_store')
        return row

    def graph_signature(self):
        """What a captured update graph bakes in of this replay."""
        return (self.alpha, self.beta, self.epsilon, self.tree.data_ptr() if self.tree is not None else 0)

    def sample_uniforms(self, iterations=None):
        """The uniform stream of `iterations` successive batches, float64 [iterations, B] in [0, 1): drawn where
        Buffer.sample_indices draws, ahead of the update that turns them into indices on the device."""
        count = self.batch_iterations if iterations is None else iterations
        return self.np_random.random_sample((count, self.batch_size))

    def sample(self, uniforms, indices, weights=None):
        """One batch's draw on the device: float64 uniforms [B] -> int64 `indices` [B] and, when given, float32
        `weights` [B] (tonic_priority_sample)."""
        _lib.check(self.lib.tonic_priority_sample(
            _lib.ptr(self.tree), self.tree.numel(), self.capacity, _lib.ptr(uniforms), _lib.ptr(indices),
            _lib.ptr(weights), uniforms.shape[0], self.beta, _lib.current_stream()), 'tonic_priority_sample')

    def update_priorities(self, indices, sample_losses):
        """Closes the loop: the drawn transitions' priorities from their (unweighted) losses, device tensors [B]
        (tonic_priority_update)."""
        _lib.check(self.lib.tonic_priority_update(
            _lib.ptr(self.tree), self.tree.numel(), self.capacity, _lib.ptr(indices), _lib.ptr(sample_losses),
            indices.shape[0], self.alpha, self.epsilon, _lib.current_stream()), 'tonic_priority_update')

    def sample_indices(self, iterations=None):
        raise NotImplementedError('PrioritizedBuffer draws its indices on the device from `sample_uniforms` '
                                  '(`sample`): there is no host index stream')

    def get(self, *keys, steps):
        """The generator API for custom agents: batches drawn by priority; `keys` may name 'indices' and 'weights'
        besides the stored fields, and `update_priorities(batch['indices'], losses)` between two batches moves the
        priorities the next one is drawn from."""
        uniforms, indices, weights = self._drawn
        for _ in range(self.batch_iterations):
            uniforms.copy_(torch.as_tensor(self.sample_uniforms(1)[0]))
            self.sample(uniforms, indices, weights)
            out = {k: torch.empty_like(v) for k, v in self.batch.items()}
            out = self.gather(indices, out)
            out['indices'], out['weights'] = indices.clone(), weights.clone()
            yield {k: out[k] for k in keys}
        self.last_steps = steps
