"""The off-policy agents' acting and storing on the environment's collector block (``tonic_collector_q_act``,
DESIGN.md §4.5): ``QBlock`` is the state of one agent on one block, ``QBlocks`` the agent's registry of them."""
import ctypes
import os

import numpy as np
import torch

from tonic_amd import _lib
from tonic_amd.collector import Block, Collector


class DevicePointer:
    """A raw device address where `_lib.ptr` expects a contiguous float32 tensor: a page-locked block's field."""

    def __init__(self, address, shape):
        self.address, self.shape = address, tuple(shape)

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.address


class QBlock:
    """One agent on one block.  The acting launch reads the block's observations in place and leaves a device copy in
    one of two row buffers; a store reads outcome and executed actions in place, the observations from that copy.

    turn           the row buffer that holds the rows of the current step
    acted          the policy's launch ran on this block during the current step()
    fed            step() copied the executed actions into block.actions
    deferred       None or (reserved Buffer row, turn of its observation rows): written by a later launch
    store_pending  a store launch that reads the block in place is issued and not known complete

    begin_step     acted = fed = False
    act            (other blocks flush first) the acting launch writes row buffer turn ^ 1 and carries `deferred`; all
                   completion words waited for; deferred = None, store_pending = False, turn ^= 1, acted = True
    feed           the policy sat out: flush, synchronize if store_pending.  store_pending = False, the executed
                   actions into block.actions, fed = True; float32 actions go out as block.out_actions
    store          fed, the block's own outcome arrays: acted, Buffer allocated, return_steps == 1 -> deferred =
                   (reserve_row, turn); else [not acted: synchronize, last observations -> row buffer turn] store
                   now, store_pending = True.  Anything else: False (the staged path)
    flush          deferred -> a store launch of its own, store_pending = True (an update is due, the policy
                   sits out or is asked about other observations, settle)
    """

    __slots__ = ('registry', 'block', 'turn', 'acted', 'fed', 'deferred', 'store_pending', 'usable', 'collector',
                 'workspace', 'rows', 'row_pointers', 'fields', 'held', 'held_for', 'staged')

    def __init__(self, registry, block):
        self.registry, self.block = registry, block
        self.turn, self.acted, self.fed, self.deferred, self.store_pending = 0, False, False, None, False
        self.held = self.held_for = self.staged = None
        self._create_resources()

    # ------------------------------------------------------------------ transitions
    def act(self, kind, stochastic):
        # one launch on the environment's block, no copies: ddpg.py:45-52 / sac.py:40-51.  The transition of the step
        # before (reserved by store(), its sources still in the block) rides in it: one more workgroup stores it
        # while the tiles compute these actions
        self._act(kind, stochastic, self.deferred)
        self.deferred, self.store_pending = None, False
        self.turn, self.acted = self.turn ^ 1, True
        return self.block.eps[1].copy()

    def feed(self, actions):
        if not self.acted:
            # the policy sat this step out (warm-up: uniform actions): no acting launch carried the reserved
            # transition or was waited for behind a store launch — they read the block in place and must be
            # through before the environment overwrites it
            self.flush()
            if self.store_pending:
                self._synchronize()
        self.store_pending = False
        # the executed actions go into the environment's block (where the store launch reads them); policy
        # actions (float32) are handed out as the block's own view — value-identical, and the environments of
        # tonic_amd.environments take their one-call step then — the warm-up's float64 draws as they are
        np.copyto(self.block.actions, actions)
        self.fed = True
        return self.block.out_actions if actions.dtype == np.float32 else actions

    def store(self, observations, rewards, last_observations):
        """The transition straight from the environment's block (Buffer.store, buffers.py:33-56)."""
        block = self.block
        if not self.fed or observations is not block.out_next_observations or rewards is not block.out_rewards:
            return False
        replay = self.registry.agent.replay
        if self.acted and replay.buffers is not None and replay.return_steps == 1:
            # the usual step: the row is reserved now (Buffer bookkeeping, buffers.py:54-56) and written by the next
            # acting launch, which reads the block before the environment's next step can touch it
            assert self.deferred is None, 'a reserved transition was never written'
            self.deferred = (replay.reserve_row(self.registry.agent.model.observation_normalizer), self.turn)
            return True
        if not self.acted:       # (warm-up: the policy never saw these rows; the previous store may still read them)
            self._synchronize()
        self._store_now(None if self.acted else last_observations)
        self.store_pending = True
        return True

    def flush(self):
        if self.deferred is not None:
            self._store_at(*self.deferred)
            self.deferred, self.store_pending = None, True

    # ------------------------------------------------------------------ the device
    def _create_resources(self):
        agent, block = self.registry.agent, self.block
        W, O, A = block.workers, agent.observation_size, agent.action_size
        self.collector = Collector.for_block(block, 0)
        need = agent.lib.tonic_offpolicy_workspace_bytes(W, O, A, agent.hidden)
        self.workspace = torch.empty(need, dtype=torch.uint8, device=agent.device)
        self.rows = [torch.zeros(W, O, device=agent.device) for _ in range(2)]
        self.row_pointers = [_lib.ptr(r) for r in self.rows]

        # the block's fields as the GPU sees them (page-locked by the collector): the store reads them in place
        def mapped(view, shape):
            address = agent.lib.tonic_host_device_pointer(view.ctypes.data)
            return DevicePointer(address, shape) if address else None
        self.fields = dict(actions=mapped(block.actions, (W, A)),
                           next_observations=mapped(block.next_observations, (W, O)),
                           rewards=mapped(block.rewards, (W,)), resets=mapped(block.resets, (W,)),
                           terminations=mapped(block.terminations, (W,)))
        self.usable = all(v is not None for v in self.fields.values())

    def _act(self, kind, stochastic, carried):
        registry, agent, block = self.registry, self.registry.agent, self.block
        if stochastic:          # Normal.sample() of sac.py:43 == loc + scale * randn
            np.copyto(block.eps[0], agent._randn(block.workers, agent.action_size).numpy())
        # the images follow the float32 parameters: rebuilt after every learner update (raw-pointer writes: the
        # flag) and whenever torch has written the flat block in place since (load_state_dict, an optimizer of the
        # caller's: the tensor's version counter, which every in-place operation on a view of it advances)
        version = agent.model.flat_online._version
        stale = registry.images_stale or version != registry.images_version
        registry.images_version = version
        store = None
        if carried is not None:
            held = self.held        # (one tonic_q_store_t per block: two fields change per step)
            if held is None or self.held_for is not agent.replay.buffers:
                held = self.held = agent.replay.store_arguments(0, self.rows[0], agent.model.observation_normalizer)
                self.held_for = agent.replay.buffers
            held.row = carried[0]
            held.d_observations = self.row_pointers[carried[1]]
            store = ctypes.addressof(held)
        # (these rows' device copy: the buffer the pending store does not read)
        status = registry.launch(
            self.collector.handle, _lib.ptr(agent.model.flat_actor.flat), _lib.ptr(registry.images), int(stale), kind,
            agent.hidden, 0 if stochastic else -1, self.row_pointers[self.turn ^ 1], store, _lib.ptr(self.workspace),
            self.workspace.numel(), _lib.current_stream())
        if status != 0:
            _lib.check(status, 'tonic_collector_q_act')
        registry.images_stale = False
        self.collector.wait_actions()          # (every completion word, the store's included)

    def _store_at(self, row, turn):
        agent = self.registry.agent
        agent.replay.store_at(row, agent.model.observation_normalizer, observations=self.rows[turn], **self.fields)

    def _store_now(self, observations):
        # `observations`: rows the policy did not act on, copied through pinned memory first
        agent, rows = self.registry.agent, self.rows[self.turn]
        if observations is not None:
            if self.staged is None:
                self.staged = torch.zeros(rows.shape, dtype=torch.float32).pin_memory()
            self.staged.numpy()[:] = observations
            rows.copy_(self.staged, non_blocking=True)
        agent.replay.store(normalizer=agent.model.observation_normalizer, observations=rows, **self.fields)

    def _synchronize(self):
        torch.cuda.current_stream().synchronize()


class QBlocks:
    """An agent's QBlock per block, found by the observations array's identity, and the actor's weight images."""

    def __init__(self, agent):
        self.agent, self.blocks = agent, {}
        self.last = None          # (three look-ups per loop iteration: the same view each time)
        self.stepped = None       # the QBlock of the array the current step() saw
        self.launch = _lib.hot('tonic_collector_q_act')      # (per environment step: the vectorcall shim if built)
        self.images, self.images_stale, self.images_version = None, True, -1

    def find(self, observations, kind):
        """The QBlock of the block these observations are a view of (tonic_amd.environments hand such views out) when
        the policy can act on it in place (a torso the fused forward holds, mappable fields); None: staged copies."""
        last = self.last
        if last is not None and last[0] is observations and last[1] == kind:
            return last[2]
        if kind not in (0, 1) or self.agent.hidden is None or os.environ.get('TONIC_AMD_Q_BLOCK', '1') == '0':
            return None
        if self.images is None:          # (once: does the fused forward on weight images serve this policy?)
            self.images = self._create_images(kind)
        if self.images is False or not isinstance(observations, np.ndarray):
            return None
        block = Block.owner_of(observations)
        found = self.blocks.get(id(block))
        if found is None and block is not None:
            found = self.blocks[id(block)] = QBlock(self, block)
        if found is not None and not found.usable:
            found = None
        self.last = (observations, kind, found)
        return found

    def _create_images(self, kind):
        agent = self.agent
        need = agent.lib.tonic_mlp_actor_image_bytes(agent.observation_size, agent.hidden, agent.action_size,
                                                     2 if kind == 1 else 1)
        return torch.zeros(need, dtype=torch.uint8, device=agent.device) if need > 0 else False

    def parameters_changed(self):
        self.images_stale = True          # (the acting launch rebuilds its weight images after an update)

    def begin_step(self):
        for q in self.blocks.values():
            q.acted = q.fed = False

    def flush(self, but=None):
        """Reserved transitions no acting launch will carry in time go out now: all (an update samples them, settle)
        or those of the blocks other than the one about to act (test episodes, a second environment)."""
        for q in self.blocks.values():
            if q is not but:
                q.flush()

    def stores_through(self):
        for q in self.blocks.values():
            q.store_pending = False

    def settle(self):
        for q in self.blocks.values():
            q.flush()
            if q.store_pending:
                q._synchronize()
                q.store_pending = False

    def clear(self):
        """Lets go of the blocks, their registrations, workspaces and row buffers: found again on the next step."""
        self.blocks, self.last, self.stepped = {}, None, None
