"""A2C / PPO / TRPO / DDPG / TD3 / SAC / D4PG / MPO / TD4 / DMPO on the HIP engine — API of ``tonic/torch/agents/*.py``.

``step`` / ``update`` keep the reference signatures (NumPy in, NumPy out) so
``tonic.Trainer`` drives the agents unchanged.  The on-policy agents talk to the GPU through
the pinned-host collector (``tonic_amd.collector``, ``tonic_collector_*``): per environment
step ONE fused launch — policy forward + sample + log-prob of the block's observations,
Segment row store, ``MeanStd.record``, and the deferred store of the previous step's outcome —
reads the environment's shared block in place and writes the actions back into it; the host
waits on a completion word, not on the stream, and draws the next step's noise meanwhile.
``update`` only marks the outcome that sits in the block as pending.  Every ``Segment.size``
steps ``_update`` enqueues the whole learner update (2 x value forward, GAE scan,
``batch_iterations`` x [actor grad+Adam, critic grad+Adam]) without any host synchronisation —
the KL early stop of ppo.py:45-46 is a device flag — and reads the logged statistics back once.

The action noise is drawn on the host with ``torch.randn`` from the global CPU generator,
which consumes the same stream as the reference's ``Normal.sample()``, so
runs with equal seeds follow the reference's trajectory up to float32 rounding.  The draw for
step t+1 is made while the GPU works on step t; ``test_step`` (which draws from the same
generator, a2c.py:87-90) first rewinds the generator to where the reference would be.
"""
import os
import random
import weakref

import numpy as np
import torch

from tonic_amd import _lib, agents, explorations, logger, parallel, replays
from tonic_amd.critic_chain import CriticChain
from tonic_amd.policy_block import PolicyBlock
from tonic_amd.q_block import QBlocks
from tonic_amd.q_update import QUpdate, _check_chain, chunk_size, shard_noise      # noqa: F401 (for their importers)
from tonic_amd.torch import models, normalizers, updaters


def default_model():
    """tonic/torch/agents/a2c.py:7-17."""
    return models.ActorCritic(
        actor=models.Actor(
            encoder=models.ObservationEncoder(),
            torso=models.MLP((64, 64), torch.nn.Tanh),
            head=models.DetachedScaleGaussianPolicyHead()),
        critic=models.Critic(
            encoder=models.ObservationEncoder(),
            torso=models.MLP((64, 64), torch.nn.Tanh),
            head=models.ValueHead()),
        observation_normalizer=normalizers.MeanStd())


def _device():
    if not torch.cuda.is_available():
        raise _lib.TonicHipError(
            'tonic_amd agents need a ROCm GPU: the learner runs in hand-written HIP kernels '
            'and there is deliberately no CPU fallback')
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    device = torch.device('cuda', local_rank if local_rank < torch.cuda.device_count() else 0)
    parallel.bind_near_gpu(device)             # (the collect loop is PCIe round trips: stay on the GPU's socket)
    return device


class Agent(agents.Agent):
    """tonic/torch/agents/agent.py:10-26 (seeding and .pt checkpoints)."""

    def initialize(self, seed=None):
        parallel.init_from_env()          # one process per GPU under torch.distributed.run; else no-op
        self.seed = seed
        if seed is not None:
            np.random.seed(seed)
            random.seed(seed)
            torch.manual_seed(seed)

    def _replicate(self, buffers, own_noise):
        """Several ranks: rank 0's parameters everywhere (replicas must not hinge on equal seeds),
        then the ACTING noise of this rank's workers gets a stream of its own (seed + rank), unless
        TONIC_AMD_GLOBAL_NOISE asks for the single-process stream (parallel.global_noise):
        `own_noise` — the on-policy agents, whose torch generator feeds nothing but the action
        noise — re-seeds the global generator; the off-policy agents keep the global generator for
        the update's replicated noise stream (`_draw_noise`, which must stay in step across ranks)
        and act from a dedicated per-rank generator — otherwise worker i of every rank would
        explore with the very same draws."""
        self.rank, self.world = parallel.rank(), parallel.world_size()
        self.global_noise = self.world > 1 and parallel.global_noise()
        self._acting_generator = None
        if self.world == 1:
            return
        parallel.broadcast_from_first(buffers)
        if self.global_noise:
            return
        if own_noise:
            if self.seed is not None and self.rank > 0:
                torch.manual_seed(self.seed + self.rank)
            return
        self._acting_generator = torch.Generator()
        if self.seed is not None:
            self._acting_generator.manual_seed(self.seed + self.rank)
        else:
            self._acting_generator.seed()

    def _randn(self, workers, width, out=None):
        """Standard-normal action noise for this rank's `workers` workers (global_noise: rows
        [rank * workers, (rank + 1) * workers) of the draw for all of them)."""
        if not getattr(self, 'global_noise', False):
            generator = getattr(self, '_acting_generator', None)
            if out is not None:
                return torch.randn(workers, width, out=out, generator=generator)
            return torch.randn(workers, width, generator=generator)
        rows = torch.randn(self.world * workers, width)[self.rank * workers:(self.rank + 1) * workers]
        return rows if out is None else out.copy_(rows)

    def save(self, path):
        path = path + '.pt'
        logger.log(f'\nSaving weights to {path}')
        os.makedirs(os.path.dirname(path), exist_ok=True)
        # CPU tensors with the reference's key layout: loadable by the reference and tonic.play.
        torch.save({k: v.detach().cpu() for k, v in self.model.state_dict().items()}, path)

    def load(self, path):
        path = path + '.pt'
        logger.log(f'\nLoading weights from {path}')
        self.model.load_state_dict(torch.load(path, map_location='cpu'))


class _Staging:
    """One [W, ...] record per environment step in PINNED host memory that the kernels read and
    write IN PLACE (page-locked memory is mapped into the GPU's address space at the same
    address): no hipMemcpyAsync in either direction, no stream synchronisation — the host fills
    the fields, enqueues the kernels with these very pointers, records an event behind them and
    spins on it.  (`TONIC_AMD_STAGING=copy` restores explicit H2D / D2H copies through a device
    mirror.)"""

    def __init__(self, fields, device):
        self.offsets, total = {}, 0
        for name, shape in fields:
            size = int(np.prod(shape))
            self.offsets[name] = (total, size, tuple(shape))
            total += (size + 63) // 64 * 64              # fields on 256-byte boundaries
        self.host = torch.zeros(total, dtype=torch.float32).pin_memory()
        self.host_np = self.host.numpy()
        self.mapped = os.environ.get('TONIC_AMD_STAGING', 'mapped') != 'copy'
        if self.mapped:      # kernels must see the block at the address the host uses
            seen = _lib.load().tonic_host_device_pointer(self.host.data_ptr())
            self.mapped = seen == self.host.data_ptr()
        self.device = self.host if self.mapped else torch.empty(total, dtype=torch.float32,
                                                                device=device)
        self.done = None             # event behind the last kernels / copies that touched `host`

    def host_view(self, name):
        start, size, shape = self.offsets[name]
        return self.host_np[start:start + size].reshape(shape)

    def device_view(self, name):
        """What the kernels get: the pinned field itself, or its device mirror."""
        start, size, shape = self.offsets[name]
        return self.device[start:start + size].view(shape)

    def writable(self):
        """Blocks until the work recorded by mark() has consumed the pinned block: the host may
        not overwrite it earlier (nothing else orders consecutive update() calls while an agent
        is still warming up and never reads anything back)."""
        if self.done is not None:
            self.done.synchronize()
        return self

    def upload(self):
        if not self.mapped:
            self.device.copy_(self.host, non_blocking=True)

    def download(self):
        if not self.mapped:
            self.host.copy_(self.device, non_blocking=True)

    def mark(self):
        """Records the event behind everything enqueued so far that reads / writes this block."""
        if self.done is None:
            self.done = torch.cuda.Event()
        self.done.record()

    def wait(self):
        """Spins until the marked work is complete (results written in place are visible)."""
        done = self.done
        while not done.query():
            pass


def _read_back_actions(stage_in, stage_out):
    """The tail of a staged forward: the actions, once everything enqueued so far is through (both blocks free)."""
    stage_out.download()
    stage_out.mark()
    stage_in.done = stage_out.done
    stage_out.wait()
    return stage_out.host_view('actions').copy()


class _NoiseAhead:
    """The action noise of the collect loop, off its critical path (a2c.py:81 draws
    ``Normal.sample()`` = one ``torch.randn(W, A)`` per environment step: 5 - 9 us of host time per
    step at W = 256).  The draws of DEPTH steps are made by ONE call — the generator's stream is the
    same: ``normal_`` fills its output with consecutive uniforms and transforms them in blocks of
    16, so a [DEPTH * W, A] draw equals DEPTH consecutive [W, A] draws bit for bit as long as W * A
    is a multiple of 16 — into one of two buffers; a helper thread fills the next buffer (the GIL
    is released inside the draw) while the loop consumes the current one, 0.7 us per step for the
    copy into the block's noise slot.  The generator runs up to 2 * DEPTH steps ahead of the noise
    the agent has consumed; ``rewind`` puts it back where the reference's stream is (state at the
    start of the current buffer, re-advanced by the rows consumed) before anybody else — a test
    episode — draws from it.  Shapes the block draw does not reproduce (W * A not a multiple of
    16), several ranks slicing a global draw, or TONIC_AMD_NOISE_AHEAD=0: one draw per step with
    the generator state kept before it, as before."""

    DEPTH = 64

    def __init__(self, agent, workers, width):
        import threading
        import weakref
        # (a weak reference: the helper thread keeps THIS object alive, and must not keep the
        #  agent — its Segment, collector and page-locked block — alive with it)
        self._agent, self.workers, self.width = weakref.ref(agent), workers, width
        n = workers * width
        self.bulk = (n % 16 == 0 and n >= 16 and not agent.global_noise
                     and os.environ.get('TONIC_AMD_NOISE_AHEAD', '1') != '0')
        self.generator = getattr(agent, '_acting_generator', None)
        self.mark = None                    # per-step mode: generator state before the last draw
        if not self.bulk:
            return
        self.buffers = [torch.empty(self.DEPTH * workers, width) for _ in range(2)]
        self.rows = [b.numpy().reshape(self.DEPTH, workers, width) for b in self.buffers]
        self.states = [None, None]          # generator state before each buffer was drawn
        self.current, self.taken, self.valid, self.ahead = 0, self.DEPTH, False, False
        self.filling = False                # the helper owns buffers[current ^ 1]
        self.pending = False                # a fill has been asked for and not started yet
        self.request, self.ready = threading.Event(), threading.Event()
        self.closed = False
        self.thread = threading.Thread(target=self._helper, daemon=True, name='tonic-noise-ahead')
        self.thread.start()
        weakref.finalize(agent, self.close)
        # (a daemon thread that is inside torch.randn when the interpreter finalises is killed in
        #  C++ code — "terminate called without an active exception": end the helpers first)
        _NoiseAhead._live.add(self)
        if not _NoiseAhead._at_exit:
            import atexit
            atexit.register(_NoiseAhead._end_all)
            _NoiseAhead._at_exit = True

    _live, _at_exit = weakref.WeakSet(), False

    @staticmethod
    def _end_all():
        for helper in list(_NoiseAhead._live):
            helper.close()
            helper.thread.join(timeout=5.0)

    def close(self):
        """Ends the helper thread (the agent was closed or collected)."""
        if self.bulk and not self.closed:
            self.closed = True
            self.request.set()

    def _state(self):
        return self.generator.get_state() if self.generator is not None else torch.get_rng_state()

    def _set_state(self, state):
        if self.generator is not None:
            self.generator.set_state(state)
        else:
            torch.set_rng_state(state)

    def _fill(self, index):
        self.states[index] = self._state()
        torch.randn(self.buffers[index].shape, out=self.buffers[index], generator=self.generator)

    def _helper(self):
        while True:
            self.request.wait()
            self.request.clear()
            if self.pending:                # (a fill asked for before close() is still delivered)
                self.pending = False
                self._fill(self.current ^ 1)
                self.ready.set()
            if self.closed:
                return

    def _settle(self):
        if self.filling:
            self.ready.wait()
            self.ready.clear()
            self.filling = False

    def take(self, out):
        """The next step's draws -> `out` (the block's noise slot, a NumPy view [W, A])."""
        if not self.bulk:
            self.mark = self._state()
            self._agent()._randn(self.workers, self.width, out=torch.from_numpy(out))
            return
        if self.taken == self.DEPTH:
            if self.valid and self.ahead:   # the buffer drawn ahead takes over
                self._settle()
                self.current ^= 1
            else:                           # first use / after a rewind / no helper: draw here
                self._fill(self.current)
                self.valid = True
            self.taken = 0
            self.ahead = not self.closed    # (a closed helper draws nothing ahead)
            if self.ahead:
                self.filling = True         # the helper draws the buffer after this one
                self.pending = True
                self.request.set()
        np.copyto(out, self.rows[self.current][self.taken])
        self.taken += 1

    def rewind(self, unconsumed):
        """Generator back to the state right after the draws of the steps the agent has executed
        (`unconsumed`: 1 if the last `take` was for a step that has not run yet)."""
        if not self.bulk:
            if unconsumed and self.mark is not None:
                self._set_state(self.mark)
            return
        if not self.valid:
            return
        self._settle()
        consumed = self.taken - unconsumed
        self._set_state(self.states[self.current])
        if consumed > 0:
            torch.randn(consumed * self.workers, self.width, generator=self.generator)
        self.taken, self.valid, self.ahead = self.DEPTH, False, False


class A2C(Agent):
    """Acting / storing half shared by the on-policy agents (a2c.py:20-99)."""

    def __init__(self, model=None, replay=None, actor_updater=None, critic_updater=None):
        self.model = model or default_model()
        self.replay = replay or replays.Segment()
        self.actor_updater = actor_updater or updaters.StochasticPolicyGradient()
        self.critic_updater = critic_updater or updaters.VRegression()

    def initialize(self, observation_space, action_space, seed=None):
        super().initialize(seed=seed)
        self.device = _device()
        if not getattr(self, '_holds_affinity', False):
            self._holds_affinity = True
            parallel.hold_affinity()
        self.lib = _lib.load()
        self.model.initialize(observation_space, action_space)       # CPU init: seed parity
        self.model.pack(self.device)
        if self.model.observation_normalizer:
            self.model.observation_normalizer.attach(self.device)
        self.replay.initialize(seed, device=self.device)
        self.actor_updater.initialize(self.model)
        self.critic_updater.initialize(self.model)
        # acting (and the kernel updates) run the kernels' head: one they do not compute is refused by name.  A torso on
        # stock torch operators acts and learns through the module's own forward (`_act`, `_stock_grad`): any head
        if not getattr(self.actor_updater, 'stock', False):
            updaters.policy_head_rule(self.model.actor.head, 'on_policy')
        self.observation_size = observation_space.shape[0]
        self.action_size = action_space.shape[0]
        self._replicate([self.model.flat_actor.flat, self.model.flat_critic.flat], own_noise=True)
        self._staged_workers = self._test_workers = self._act_workspace = None       # (the staged path)
        # 3 (default): the act kernel stays RESIDENT for a rollout and the host pushes each step's
        # command, observation and noise rows into a device window (the collector falls back to 2 where
        # it cannot or should not: see tonic_collector_create); 2: resident, the kernel pulls everything
        # from the page-locked block over PCIe; 0: the same kernel launched once per step;
        # 1: hipMemcpyAsync around it (profiles/r02_collector_latency.md: 10.4 / 13.9 / 28.4 us per
        # round trip for 2 / 0 / 1)
        transport = int(os.environ.get('TONIC_AMD_COLLECTOR_TRANSPORT', '3'))
        if self._rollout is None:
            self._rollout = PolicyBlock(self, transport)
        else:
            self._rollout.reset(transport)

    # the rollout on the environment's collector block: all of its state (tonic_amd.policy_block)
    _rollout = None
    _chain = None            # (PPO: the critic's iterations under the next rollout, tonic_amd.critic_chain)
    transport = property(lambda self: self._rollout.transport,
                         lambda self, value: setattr(self._rollout, 'transport', value))
    transport_in_effect = property(lambda self: self._rollout.transport_in_effect)       # (absent until bound)
    steps_issued_by_environment = property(lambda self: self._rollout.issued_by_environment)
    # (what the GPU tests read of the rollout, under the names it had on the agent)
    _block = property(lambda self: self._rollout.block)
    _collector = property(lambda self: self._rollout.collector)
    _speculated = property(lambda self: self._rollout.speculated)

    def _settle(self):
        self._rollout.settle()

    def _draws_ahead(self, workers, width):
        return _NoiseAhead(self, workers, width)

    # ------------------------------------------------------------------ acting
    def _io(self, workers):
        W, O, A = workers, self.observation_size, self.action_size
        return (_Staging([('observations', (W, O)), ('eps', (W, A))], self.device),
                _Staging([('actions', (W, A)), ('log_probs', (W,))], self.device))

    def _act(self, observations, stage_in, stage_out, want_log_probs):
        """Stand-alone forward + sample (test episodes): staging copies and a stream sync."""
        W, A = observations.shape[0], self.action_size
        stage_in.writable()
        stage_out.writable()
        stage_in.host_view('observations')[:] = observations
        # Same generator draw as Normal.sample() in the reference (a2c.py:81).
        # (test episodes run on every rank alike: plain draws; training workers are a shard)
        draw = self._randn if want_log_probs else torch.randn
        stage_in.host_view('eps')[:] = draw(W, A).numpy()
        stage_in.upload()
        if getattr(self.actor_updater, 'stock', False):
            # any MLP(sizes, activation): the policy's forward as stock torch operators on the
            # device, the sample and its log-probability as a2c.py:75-85 forms them
            # (mapped staging hands the kernels pinned host fields: torch operators want device
            #  tensors, and write their results back with an asynchronous copy)
            with torch.no_grad():
                observations = stage_in.device_view('observations').to(self.device, non_blocking=True)
                eps = stage_in.device_view('eps').to(self.device, non_blocking=True)
                distribution = self.model.actor(observations)
                actions = distribution.loc + distribution.scale * eps
                stage_out.device_view('actions').copy_(actions, non_blocking=True)
                if want_log_probs:
                    stage_out.device_view('log_probs').copy_(
                        distribution.log_prob(actions).sum(dim=-1), non_blocking=True)
            return _read_back_actions(stage_in, stage_out)
        p = _lib.ptr
        torso = getattr(self.actor_updater, 'torso', None)
        if torso is not None:
            prefix, name = torso, 'tonic_ppo_act_torso'
            need = self.lib.tonic_ppo_torso_workspace_bytes(W, self.observation_size, A, 1, torso[0], torso[1])
        else:
            prefix, name = (), 'tonic_ppo_act_wide'
            need = self.lib.tonic_ppo_workspace_bytes(W, self.observation_size, A, 1)
        if self._act_workspace is None or self._act_workspace.numel() < need:
            self._act_workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        _lib.check(getattr(self.lib, name)(
            *prefix, p(self.model.flat_actor.flat), p(stage_in.device_view('observations')),
            p(stage_in.device_view('eps')), p(stage_out.device_view('actions')),
            p(stage_out.device_view('log_probs')) if want_log_probs else None,
            W, self.observation_size, A, p(self._act_workspace), self._act_workspace.numel(),
            _lib.current_stream()), name)
        return _read_back_actions(stage_in, stage_out)

    # -- shapes beyond the fused act kernel (O > 32 or A > 8): staged copies + separate launches
    def _wide(self):
        """Shapes beyond the fused act kernel go through the collector as well (layer-by-layer
        launches per step on the mapped block, csrc/mlpwide.hip wide_collect_step);
        TONIC_AMD_WIDE_STAGED=1 keeps the older path of staged copies and separate launches."""
        # (torsos outside the kernels' shapes act through stock torch operators, staged as well)
        # (... and torsos on the layer-by-layer HIP path, tonic_ppo_act_torso, staged too: the collector's
        #  per-step kernels hold the default torso)
        return getattr(self.actor_updater, 'stock', False) or \
            getattr(self.actor_updater, 'torso', None) is not None or (
                (self.observation_size > 32 or self.action_size > 8)
                and os.environ.get('TONIC_AMD_WIDE_STAGED', '0') == '1')

    def _step_staged(self, observations):
        observations = np.asarray(observations, np.float32)
        W, O = observations.shape[0], self.observation_size
        if self._staged_workers != W:
            self._staged_workers = W
            self._in, self._out = self._io(W)
            self._outcome = _Staging([('next_observations', (W, O)), ('rewards', (W,)),
                                      ('resets', (W,)), ('terminations', (W,))], self.device)
        actions = self._act(observations, self._in, self._out, True)
        self.last_observations, self.last_actions = observations, actions
        return actions

    def _update_staged(self, observations, rewards, resets, terminations):
        stage = self._outcome.writable()
        stage.host_view('next_observations')[:] = observations
        stage.host_view('rewards')[:] = rewards
        stage.host_view('resets')[:] = resets                 # bool -> float32 (segments.py:33)
        stage.host_view('terminations')[:] = terminations
        stage.upload()
        self.replay.store(
            normalizer=self.model.observation_normalizer,
            observations=self._in.device_view('observations'),
            actions=self._out.device_view('actions'),
            next_observations=stage.device_view('next_observations'),
            rewards=stage.device_view('rewards'), resets=stage.device_view('resets'),
            terminations=stage.device_view('terminations'),
            log_probs=self._out.device_view('log_probs'))
        stage.mark()                  # the store kernel reads the pinned fields in place
        self._in.done = self._out.done = stage.done
        if self.replay.ready():
            self._update()

    def step(self, observations, steps):
        # (once per environment step: the steady state of a block-fed loop first, PolicyBlock.step_ahead)
        rollout = self._rollout
        actions = rollout.step_ahead(observations)
        if actions is None:
            if self._wide():
                return self._step_staged(observations)
            actions = rollout.step(observations)
        self.last_observations = observations
        self.last_actions = actions
        return actions

    def close(self):
        """Releases what a live agent holds beyond its tensors (PolicyBlock.close: a step issued ahead, the
        generator, the noise helper thread, the collector).  The agent can be initialised again afterwards."""
        if self._rollout is not None:
            self._rollout.close()
        if getattr(self, '_holds_affinity', False):
            self._holds_affinity = False
            parallel.release_affinity()            # (bind_near_gpu: the last agent to close restores the CPU mask)

    def test_step(self, observations, steps):
        self._open_gates()      # (the current stream waits for the critic's iterations: let them start)
        self._rollout.rewind()
        observations = np.asarray(observations, np.float32)
        if self._test_workers != observations.shape[0]:
            self._test_workers = observations.shape[0]
            self._test_in, self._test_out = self._io(observations.shape[0])
        return self._act(observations, self._test_in, self._test_out, False)

    def _open_gates(self):
        """(PPO: the gates in front of critic chains, CriticChain.open_gates)"""

    # ---------------------------------------------------------------- learning
    def update(self, observations, rewards, resets, terminations, steps):
        """a2c.py:58-73 (PolicyBlock.update_ahead: the steady state; PolicyBlock.update ends the rollout with
        `self._update()`)."""
        rollout = self._rollout
        if rollout.update_ahead(observations, rewards, resets, terminations):
            return
        if self._wide():
            return self._update_staged(observations, rewards, resets, terminations)
        rollout.update(observations, rewards, resets, terminations)

    # -- the Return normaliser (a2c.py:68-69 records every step's rewards, :126-127 updates it)
    def _range_rewards(self):
        """The rollout is complete: its rewards' [min, max] (tonic_reward_range, stream-ordered) — merged over
        the ranks' worker shards — goes to the Return normaliser at the update's sync (_record_rewards).
        Return.record keeps only the running min / max, so the pair does what recording every reward
        does.  Launched before anything of the update touches the Segment."""
        if not self.model.return_normalizer:
            return
        if getattr(self, '_reward_range', None) is None:
            self._reward_range = torch.empty(2, dtype=torch.float32, device=self.device)
        rewards = self.replay.buffers['rewards']
        _lib.check(self.lib.tonic_reward_range(_lib.ptr(rewards), rewards.numel(),
                                               _lib.ptr(self._reward_range), _lib.current_stream()),
                   'tonic_reward_range')
        if parallel.exchanging():
            # MIN / MAX over the ranks as one MAX of (-min, max): an empty pair (+inf, -inf) is its identity
            self._reward_range[0].neg_()
            torch.distributed.all_reduce(self._reward_range, op=torch.distributed.ReduceOp.MAX)
            self._reward_range[0].neg_()

    def _record_rewards(self):
        """Reads the pair back (after the update's own sync: nothing left to wait for) and records it."""
        if not self.model.return_normalizer:
            return
        low, high = self._reward_range.cpu().numpy()
        if low <= high:                     # (min > max: no reward that is not NaN)
            self.model.return_normalizer.record(np.array([low, high], np.float32))

    def _update_normalizers(self):
        """a2c.py:123-127 / ppo.py:55-59 / trpo.py:93-97, after the critic's iterations."""
        if self.model.observation_normalizer:
            self.model.observation_normalizer.update()
        if self.model.return_normalizer:
            self.model.return_normalizer.update()

    def _evaluate(self):
        """a2c.py:92-99 on the HBM-resident segment: fills values / next_values in place."""
        b = self.replay.buffers
        critic = self.critic_updater
        critic.forward_values(replays.flatten_batch(b['observations']), b['values'].view(-1))
        critic.forward_values(replays.flatten_batch(b['next_observations']),
                              b['next_values'].view(-1))
        return b['values'], b['next_values']

    def _form_returns(self):
        """Evaluate, lambda-returns (a2c.py:101-106); returns how many iterations one pass over the Segment yields."""
        values, next_values = self._evaluate()
        self.replay.compute_returns(values, next_values)
        return self.replay.updates_per_get()

    def _begin_update(self, fresh=False):
        """The head of a kernel update: the returns formed, the statistic rows [2, updates, INFO_WIDTH] zeroed — the
        agent's own, or `fresh` ones for a critic chain that outlives the update and keeps them — and the actor's KL
        stop reset.  Returns the rows."""
        updates = self._form_returns()
        if fresh:
            infos = torch.zeros(2, updates, updaters.INFO_WIDTH, device=self.device)
        else:
            if getattr(self, '_infos', None) is None or self._infos.shape[1] != updates:
                self._infos = torch.zeros(2, updates, updaters.INFO_WIDTH, device=self.device)
            self._infos.zero_()
            infos = self._infos
        self.actor_updater.reset_stop()
        return infos

    def enqueue_update(self):
        """a2c.py:101-127 without a host sync: evaluate, lambda-returns, ONE actor step on the
        full batch, then the critic over `replay.get` (full batch `batch_iterations` times, or
        minibatches).  Returns the statistic rows: [0, 0] the actor's, [1, :] the critic's."""
        replay, actor, critic = self.replay, self.actor_updater, self.critic_updater
        self._begin_update()
        full = tuple(replays.flatten_batch(replay.buffers[k]) for k in replays.segments.LEARNER_KEYS)
        obs, act, raw_adv, log_probs, _ = full
        actor.enqueue(obs, act, raw_adv, replay.adv_stats, log_probs, self._infos[0, 0])
        for it, (obs, _, _, _, returns) in enumerate(replay.learner_batches()):
            critic.enqueue(obs, returns, self._infos[1, it])
        return self._infos

    def _update(self):
        self._range_rewards()
        infos = self.enqueue_update().cpu().numpy()          # the only sync of the update
        parallel.check_one_shot()
        for i, key in enumerate(updaters.ACTOR_INFO):
            if key in ('loss', 'kl', 'entropy', 'std'):
                logger.store('actor/' + key, infos[0, 0, i])
        for row in infos[1]:
            logger.store('critic/loss', row[0])
            logger.store('critic/v', row[1])      # mean of the value batch (log-equivalent)
        self.last_infos = infos
        self._record_rewards()
        self._update_normalizers()


class TRPO(A2C):
    """tonic/torch/agents/trpo.py:7-97.  Acting, storing, evaluation, lambda-returns and the
    critic regression are the A2C / PPO machinery (fused collector, HBM-resident Segment, HIP
    kernels); the actor step is TrustRegionPolicyGradient (stock-torch autograd on the device,
    SURVEY.md §8(f4)).  The behaviour policy's locs / scales are not stored per step
    (trpo.py:27-28,41-43): the parameters are those of the rollout until this update moves them,
    so the updater recomputes them from the stored observations."""

    def __init__(self, model=None, replay=None, actor_updater=None, critic_updater=None):
        super().__init__(model=model, replay=replay,
                         actor_updater=actor_updater or updaters.TrustRegionPolicyGradient(),
                         critic_updater=critic_updater)

    def _update(self):
        replay, critic = self.replay, self.critic_updater
        self._range_rewards()
        updates = self._form_returns()
        batch = replay.get_full('observations', 'actions', 'log_probs', 'advantages')
        for key, value in self.actor_updater(**batch).items():
            logger.store('actor/' + key, value.numpy())
        # (the actor's step is the updater's own: no KL stop to reset, and the critic's rows alone, behind it)
        infos = torch.zeros(updates, updaters.INFO_WIDTH, device=self.device)
        for it, (obs, _, _, _, returns) in enumerate(replay.learner_batches()):
            critic.enqueue(obs, returns, infos[it])
        infos = infos.cpu().numpy()
        parallel.check_one_shot()
        for row in infos:
            logger.store('critic/loss', row[0])
            logger.store('critic/v', row[1])
        logger.store('critic/iterations', updates)
        self.last_infos = infos
        self._record_rewards()
        self._update_normalizers()


class PPO(A2C):
    """tonic/torch/agents/ppo.py:7-67."""

    def __init__(self, model=None, replay=None, actor_updater=None, critic_updater=None):
        super().__init__(model=model, replay=replay,
                         actor_updater=actor_updater or updaters.ClippedRatio(),
                         critic_updater=critic_updater)

    def initialize(self, observation_space, action_space, seed=None):
        super().initialize(observation_space, action_space, seed=seed)
        if self._chain is None:
            self._chain = CriticChain(self)

    def _form_returns(self):
        self.critic_updater.max_workgroups = self._critic_width()
        return super()._form_returns()

    def enqueue_update(self):
        """Enqueues one whole learner update on the current stream (no host sync)."""
        self.settle()
        replay, actor, critic = self.replay, self.actor_updater, self.critic_updater
        infos = self._begin_update()
        # Full batch (ppo.py:40-47 over segments.py:55-57) or shuffled minibatches
        # (segments.py:58-65); the advantages stay raw and are normalised in-register with the
        # GLOBAL statistics, exactly what get_full computes before the reference slices.
        # Several ranks: every iteration exchanges [gradient sums | 8 statistics] of both networks
        # (RCCL over xGMI).  After the KL stop the actor half is zero-filled on every rank alike and
        # its step is skipped by the same device flag everywhere.  The schedules
        # (TONIC_AMD_EXCHANGE), A/B-measured through RCCL with a one-rank group:
        #   one-shot         tonic_allreduce_f32 behind each grad launch: one ~10 us launch per exchange,
        #                    nothing to hide it behind
        #   joint (default)  one all-reduce of both halves per iteration, both Adam steps in one
        #                    launch: +8.6 ms per 80-iteration update over the exchange-free path;
        #   overlap          one asynchronous all-reduce per network, each hidden behind the OTHER
        #                    network's fused grad kernel
        #                      actor grad i | AR(actor i) over critic grad i | Adam(actor i)
        #                      critic grad i | AR(critic i) over Adam(actor i) + actor grad i+1 | Adam(critic i)
        #                    : +12.4 ms — the stream hand-overs of 160 collectives cost more than
        #                    the latency of 80 they hide when there is no link latency to hide.
        # The first three are ONE loop: what follows the actor's grad launch, what the critic's.
        after_actor = after_critic = None
        if parallel.exchanging():
            one_shot = parallel.one_shot(max(actor.count, critic.count) + updaters.INFO_WIDTH)
            if one_shot is not None:
                def after_actor():
                    one_shot.all_reduce(actor.grad_sums)

                def after_critic():
                    one_shot.all_reduce(critic.grad_sums)
            elif os.environ.get('TONIC_AMD_EXCHANGE', 'joint') == 'joint':
                # ONE synchronous all-reduce of [actor sums | 8 | critic sums | 8] per iteration, both
                # optimizer steps in one launch (half the collectives, none of them hidden)
                if getattr(self, '_joint_grads', None) is None:
                    na, nc = actor.count + updaters.INFO_WIDTH, critic.count + updaters.INFO_WIDTH
                    self._joint_grads = torch.zeros(na + nc, device=self.device)
                    actor.share_gradient_buffer(self._joint_grads[:na])
                    critic.share_gradient_buffer(self._joint_grads[na:])

                def after_critic():
                    torch.distributed.all_reduce(self._joint_grads)
            else:
                return self._enqueue_overlapped_exchange(infos)
        for it, (obs, act, raw_adv, log_probs, returns) in enumerate(replay.learner_batches()):
            actor.enqueue_grad(obs, act, raw_adv, replay.adv_stats, log_probs)
            if after_actor is not None:
                after_actor()
            critic.enqueue_grad(obs, returns)
            if after_critic is not None:
                after_critic()
            updaters.enqueue_step_pair(actor, critic, obs.shape[0], replay.adv_stats, infos[0, it], infos[1, it])
        return infos

    def _enqueue_overlapped_exchange(self, infos):
        """TONIC_AMD_EXCHANGE=overlap (see enqueue_update): its pipelining is a loop of its own."""
        replay, actor, critic = self.replay, self.actor_updater, self.critic_updater
        all_reduce = torch.distributed.all_reduce
        pending = None                           # (work handle, rows, info row) of the critic
        for it, (obs, act, raw_adv, log_probs, returns) in enumerate(replay.learner_batches()):
            n = obs.shape[0]
            actor.enqueue_grad(obs, act, raw_adv, replay.adv_stats, log_probs)
            actor_sums = all_reduce(actor.grad_sums, async_op=True)
            if pending is not None:
                pending[0].wait()
                critic.enqueue_step(pending[1], pending[2], allreduce=False)
            critic.enqueue_grad(obs, returns)
            pending = (all_reduce(critic.grad_sums, async_op=True), n, infos[1, it])
            actor_sums.wait()
            actor.enqueue_step(n, replay.adv_stats, infos[0, it], allreduce=False)
        if pending is not None:
            pending[0].wait()
            critic.enqueue_step(pending[1], pending[2], allreduce=False)
        return infos

    # -- the critic's iterations under the next rollout (tonic_amd.critic_chain) --------------
    # On one GPU with full-batch iterations update() runs the actor's 80 iterations, hands the critic's 80
    # to a second HIP stream BEHIND them and returns (on the compute units the resident collect kernel
    # leaves, less 16 to spare: 219 of 256 at 256 workers).  Everything that reads the critic waits first
    # (settle(): the next update, save / load, close, `last_infos`, the logger's dump — and the current
    # stream itself waits, so parameters read through torch are final).
    # TONIC_AMD_CRITIC_OVERLAP=0: the interleaved launches of enqueue_update.
    OVERLAP_BLOCKS = None       # (developer override of the critic's workgroups per launch)
    MIN_OVERLAP_BLOCKS = 128    # below this width the critic's chain does not go under a rollout
    GATE_MARGIN_MS = 1.0        # (CriticChain.arm_gate: the chain ends this long before the rollout does)
    GATE_ROLLOUT_US = 100e3     # (... and no gate in a rollout longer than this)

    def _critic_blocks(self):
        """Workgroups of the critic's launches while a rollout is collected: what the resident
        collect kernel leaves of the 256 compute units (one workgroup per 16 workers + 4 copy + 1
        record, and a few to spare)."""
        if self.OVERLAP_BLOCKS is not None:
            return int(self.OVERLAP_BLOCKS)
        return min(256, max(8, 256 - self._collect_workgroups() - 16))

    def _critic_width(self):
        """`max_workgroups` of the critic's grad launches in this update: what they get under a
        rollout whenever the configuration is one whose critic MAY run there — whether or not it
        does (TONIC_AMD_CRITIC_OVERLAP) — so that the switch moves the critic's iterations in time
        and changes no bit of what they compute; the kernel's own width otherwise."""
        return self._critic_blocks() if self._overlap_eligible() else 0

    def _collect_workgroups(self):
        workers = getattr(self.replay, 'num_workers', None) or 0
        return (workers + 15) // 16 + 5

    def _overlap(self):
        return os.environ.get('TONIC_AMD_CRITIC_OVERLAP', '1') != '0' and self._overlap_eligible()

    def _overlap_eligible(self):
        """Everything but the switch: the updates of such a configuration give the critic's launches
        the width they have under a rollout (`_critic_blocks`) whether or not they run there, so the
        switch changes WHEN the critic's iterations run and not one bit of what they compute."""
        return (self.replay.batch_size is None
                and not self.actor_updater.stock and not self.critic_updater.stock
                and self.observation_size <= 32 and self.action_size <= 8
                # the collect kernel must leave the critic at least half of the chip: with thousands of
                # workers per GPU (cfg 5 on one GPU: 645 collect workgroups) a chain squeezed into the
                # few units left over would run many times longer than the rollout it hides under —
                # such configurations keep the full-width interleaved launches
                and self._critic_blocks() >= self.MIN_OVERLAP_BLOCKS
                and self._rollout.collector is not None
                # only behind a rollout that came through the collector (it binds the Segment's
                # buffers anew every rollout; anybody else — rollout.DeviceRollout's captured graph —
                # may hold their addresses, and the overlap swaps the observation buffer)
                and self._rollout.host_rollout)

    # (what the benchmark and the tests read of the chain: None / 0 before the first one)
    _critic_stream = property(lambda self: self._chain and self._chain.stream)
    _gate_ticket = property(lambda self: self._chain.gate_ticket if self._chain else 0)
    critic_chain_ms = property(lambda self: self._chain and self._chain.chain_ms)

    @property
    def _critic_pending(self):
        """The chain in flight as the tests read it: None, or its `done` event."""
        chain = self._chain
        return None if chain is None or chain.done is None else dict(done=chain.done)

    @property
    def last_infos(self):
        self.settle()
        return self._last_infos

    @last_infos.setter
    def last_infos(self, value):
        self._last_infos = value

    def _open_gates(self):
        CriticChain.open_gates()

    def settle(self):
        """Waits for the critic iterations a previous update left running and logs their rows."""
        rows = self._chain.settle() if self._chain is not None else CriticChain.open_gates()
        if rows is None:
            return
        log_ppo_critic_rows(rows)
        logger.store('critic/iterations', len(rows))
        log_learning_rate('critic', self.critic_updater, self)
        if getattr(self, '_last_infos', None) is not None:
            self._last_infos[1] = rows

    def save(self, path):
        self.settle()
        super().save(path)

    def load(self, path):
        self.settle()
        super().load(path)

    def close(self):
        self.settle()
        super().close()

    def _update(self):
        self.settle()
        self._range_rewards()
        if not self._overlap():
            infos = self.enqueue_update().cpu().numpy()          # the only sync of the update
            parallel.check_one_shot()
            log_ppo_update(infos)
            log_learning_rate('actor', self.actor_updater, self)
            log_learning_rate('critic', self.critic_updater, self)
            self.last_infos = infos
            self._record_rewards()
            self._update_normalizers()
            return
        replay, actor, chain = self.replay, self.actor_updater, self._chain
        infos = self._begin_update(fresh=True)
        updates = infos.shape[1]
        buffers = replay.buffers
        obs, act, raw_adv, log_probs, returns = (
            replays.flatten_batch(buffers[k]) for k in replays.segments.LEARNER_KEYS)
        replay.index = 0
        n = obs.shape[0]
        first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        first.record()
        for it in range(updates):
            actor.enqueue_grad(obs, act, raw_adv, replay.adv_stats, log_probs)
            actor.enqueue_step(n, replay.adv_stats, infos[0, it])
        last.record()
        normalizer = self.model.observation_normalizer
        ahead = normalizer if parallel.exchanging() and normalizer else None      # (see CriticChain.launch)
        if chain.launch(obs, returns, infos, normalizer_first=ahead):
            # Whoever reads the critic through torch — a forward pass of the module, state_dict() — finds it
            # final: both settle first, and so does the logger's dump (the package's own readers call settle())
            logger.before_dump(self, 'settle')
            self.model.critic.register_forward_pre_hook(lambda module, args: self.settle())     # (settle: None)
            self.model.register_state_dict_pre_hook(lambda module, prefix, keep_vars: self.settle())
        rows = infos[0].cpu().numpy()                    # waits for the actor's iterations only
        self.actor_chain_ms = first.elapsed_time(last)   # (bench.py reports it)
        parallel.check_one_shot()
        logger.store('actor/iterations', log_ppo_actor_rows(rows))
        log_learning_rate('actor', self.actor_updater, self)
        self._last_infos = np.stack([rows, np.zeros_like(rows)])
        if normalizer and ahead is None:
            normalizer.update()
        self._record_rewards()
        if self.model.return_normalizer:
            self.model.return_normalizer.update()
        chain.hand_over(self._rollout)


def log_ppo_update(infos):
    """The keys ppo.py:46-67 logs for one learner update, from the statistics rows the device
    wrote: infos[0] = actor rows {loss, kl, entropy, clip_fraction, std, stop, ran}, one per
    iteration that ran before the KL stop; infos[1] = critic rows {loss, v}."""
    ran = log_ppo_actor_rows(infos[0])
    log_ppo_critic_rows(infos[1])
    logger.store('actor/iterations', ran)
    logger.store('critic/iterations', len(infos[1]))


def log_ppo_actor_rows(rows):
    """Stores the rows of the iterations that ran before the KL stop; returns how many did."""
    actor_rows = rows[rows[:, 6] > 0]
    for row in actor_rows:
        for i, key in enumerate(updaters.ACTOR_INFO):
            value = row[i] > 0.5 if key == 'stop' else row[i]
            logger.store('actor/' + key, value)
    return len(actor_rows)


def log_ppo_critic_rows(rows):
    for row in rows:
        logger.store('critic/loss', row[0])
        logger.store('critic/v', row[1])      # mean of the value batch (log-equivalent)


# ----------------------------------------------------------------- off-policy (SAC / TD3)

def _twin_model(head, critic_head=None):
    return models.ActorTwinCriticWithTargets(
        actor=models.Actor(
            encoder=models.ObservationEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=head),
        critic=models.Critic(
            encoder=models.ObservationActionEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=critic_head or models.ValueHead()),
        observation_normalizer=normalizers.MeanStd())


def _ddpg_model():
    """tonic/torch/agents/ddpg.py:7-17."""
    return models.ActorCriticWithTargets(
        actor=models.Actor(
            encoder=models.ObservationEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=models.DeterministicPolicyHead()),
        critic=models.Critic(
            encoder=models.ObservationActionEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=models.ValueHead()),
        observation_normalizer=normalizers.MeanStd())


class DDPG(Agent):
    """tonic/torch/agents/ddpg.py:20-112: acting / storing / update scheduling; TD3 and SAC build
    on this class like in the reference."""

    policy_kind = 0          # tonic_policy_forward kind used by `_policy`
    # ActorCriticWithTargets(..., return_normalizer=Return(...)): served by the updaters' *_ranged entries (DDPG, TD3,
    # SAC); an agent whose updaters have no squashed form (MPO) keeps raising at its first update
    serves_return_normalizer = True

    def __init__(self, model=None, replay=None, exploration=None, actor_updater=None,
                 critic_updater=None):
        self.model = model or _ddpg_model()
        self.replay = replay or replays.Buffer()
        self.exploration = exploration or explorations.NormalActionNoise()
        self.actor_updater = actor_updater or updaters.DeterministicPolicyGradient()
        self.critic_updater = critic_updater or updaters.DeterministicQLearning()

    # the critic updaters whose steps take a prioritized batch's weights and return its rows' losses
    _PRIORITIZED = (updaters.DistributionalDeterministicQLearning,
                    updaters.TwinCriticDistributionalDeterministicQLearning)

    def initialize(self, observation_space, action_space, seed=None):
        if isinstance(self.replay, replays.PrioritizedBuffer) and type(self.critic_updater) not in self._PRIORITIZED:
            raise NotImplementedError(
                f'PrioritizedBuffer with the critic updater {type(self.critic_updater).__name__} is not served: the '
                f'weighted critic steps are those of {" and ".join(c.__name__ for c in self._PRIORITIZED)} '
                '(D4PG, TD4)')
        super().initialize(seed=seed)
        self.device = _device()
        if not getattr(self, '_holds_affinity', False):
            self._holds_affinity = True
            parallel.hold_affinity()
        self.lib = _lib.load()
        self.model.initialize(observation_space, action_space)      # CPU init: seed parity
        self.model.pack(self.device)
        if self.model.observation_normalizer:
            self.model.observation_normalizer.attach(self.device)
        self.replay.initialize(seed, device=self.device)
        self.exploration.initialize(self._policy, action_space, seed)
        self.actor_updater.initialize(self.model)
        self.critic_updater.initialize(self.model)
        self.observation_size = observation_space.shape[0]
        self.action_size = action_space.shape[0]
        self.hidden = self.critic_updater.hidden
        # (the torch generator also feeds the update's GLOBAL noise stream here: it stays in step)
        self._replicate([self.model.flat_online, self.model.flat_target], own_noise=False)
        self._workers = None
        self._policy_io = {}
        self._q = QBlocks(self)      # acting / storing on the environments' own blocks (tonic_amd.q_block)
        self._u = QUpdate(self)      # how an update call reaches the GPU (tonic_amd.q_update); anew: re-captures

    def close(self):
        """Stores what is still deferred and lets go of the environments' blocks; gives back what the agent holds
        beyond its tensors (the process's CPU binding: parallel.bind_near_gpu)."""
        if getattr(self, '_q', None) is not None:
            self._q.settle()
            self._q.clear()
        if getattr(self, '_holds_affinity', False):
            self._holds_affinity = False
            parallel.release_affinity()

    # ------------------------------------------------------------------ acting
    def settle(self):
        """Everything this agent has deferred is on the device: reserved transitions stored, their launches through
        (readers of `replay.buffers` between two steps call this; `close` does)."""
        if getattr(self, '_q', None) is not None:
            self._q.settle()

    def _forward_policy(self, observations, kind, stochastic):
        q = self._q.find(observations, kind)
        self._q.flush(but=q)      # (a transition reserved on another block does not wait for that block's next launch)
        if q is not None:
            return q.act(kind, stochastic)
        return self._forward_staged(observations, kind, stochastic)

    def _forward_staged(self, observations, kind, stochastic):
        observations = np.asarray(observations, np.float32)
        W = observations.shape[0]
        io = self._policy_io.get(W)
        if io is None:
            need = 16 if self.hidden is None else self.lib.tonic_offpolicy_workspace_bytes(
                W, self.observation_size, self.action_size, self.hidden)
            io = (_Staging([('observations', (W, self.observation_size)),
                            ('eps', (W, self.action_size))], self.device),
                  _Staging([('actions', (W, self.action_size))], self.device),
                  torch.empty(need, dtype=torch.uint8, device=self.device))
            self._policy_io[W] = io
        stage_in, stage_out, workspace = io
        stage_in.host_view('observations')[:] = observations
        if stochastic:      # Normal.sample() of sac.py:43 == loc + scale * randn
            stage_in.host_view('eps')[:] = self._randn(W, self.action_size).numpy()
        stage_in.upload()
        if self.hidden is None:
            # any MLP(sizes, activation): the policy's forward as stock torch operators (updaters.
            # _StockTorch); kind 0 tanh head, 1 squashed Gaussian (greedy: its loc), 2 Gaussian
            with torch.no_grad():
                out = self.model.actor(
                    stage_in.device_view('observations').to(self.device, non_blocking=True))
                eps = stage_in.device_view('eps').to(self.device, non_blocking=True)
                if kind == 0:
                    actions = out
                elif kind == 1:
                    normal = out._distribution
                    actions = torch.tanh(normal.mean + normal.stddev * eps) if stochastic else out.loc
                else:
                    actions = out.loc + out.scale * eps if stochastic else out.loc
                stage_out.device_view('actions').copy_(actions, non_blocking=True)
            return _read_back_actions(stage_in, stage_out)
        p = _lib.ptr
        _lib.check(self.lib.tonic_policy_forward(
            p(self.model.flat_actor.flat), p(stage_in.device_view('observations')),
            p(stage_in.device_view('eps')) if stochastic else None,
            p(stage_out.device_view('actions')), kind, W, self.observation_size, self.hidden,
            self.action_size, p(workspace), workspace.numel(), _lib.current_stream()),
            'tonic_policy_forward')
        return _read_back_actions(stage_in, stage_out)

    def _greedy_actions(self, observations):
        return self._forward_policy(observations, self.policy_kind, False)

    def _policy(self, observations):
        return self._greedy_actions(observations)

    def step(self, observations, steps):
        self._q.begin_step()
        actions = self.exploration(observations, steps)
        self.last_observations = observations.copy()
        self.last_actions = actions.copy()
        q = self._q.stepped = self._q.find(observations, self.policy_kind)
        return actions if q is None else q.feed(actions)

    def test_step(self, observations, steps):
        return self._greedy_actions(observations)

    # ---------------------------------------------------------------- learning
    def update(self, observations, rewards, resets, terminations, steps):
        q = self._q.stepped
        if q is None or not q.store(observations, rewards, self.last_observations):
            self._store_staged(observations, rewards, resets, terminations)
        if self.model.return_normalizer:
            if not self.serves_return_normalizer:
                raise NotImplementedError('return normalisers are not supported')
            record_reward_range(self.model.return_normalizer, rewards)      # ddpg.py:69-70
        if self.replay.ready(steps):
            self._q.flush()              # the update samples the reserved transitions too
            self._update(steps)          # (ends with a read-back: the store launches are through)
            self._q.stores_through()
        self.exploration.update(resets)

    def _store_staged(self, observations, rewards, resets, terminations):
        W = len(rewards)
        if self._workers != W:
            self._workers = W
            O, A = self.observation_size, self.action_size
            fields = [('observations', (W, O)), ('actions', (W, A)), ('next_observations', (W, O)),
                      ('rewards', (W,)), ('resets', (W,)), ('terminations', (W,))]
            # two pinned blocks used in turn: the copy of step t may still be in flight while the
            # host fills the block of step t+1
            self._transitions = (_Staging(fields, self.device), _Staging(fields, self.device))
            self._transition_turn = 0
        self._transition_turn ^= 1
        stage = self._transitions[self._transition_turn].writable()
        record = dict(observations=self.last_observations, actions=self.last_actions, next_observations=observations,
                      rewards=rewards, resets=resets, terminations=terminations)
        for key, value in record.items():
            stage.host_view(key)[:] = value          # (actions: float64 warm-up -> float32)
        stage.upload()
        self.replay.store(normalizer=self.model.observation_normalizer,
                          **{key: stage.device_view(key) for key in record})
        stage.mark()                  # the store kernel(s) read the pinned fields in place

    def _actor_due(self, iteration):
        return True                       # ddpg.py:105-112: actor + targets every iteration

    def _draw_subsets(self, iterations):
        """int32 [iterations]: one word per learner iteration for a critic step that reads one (REDQ's subset
        masks); None: this agent's critic step reads none."""
        return None

    def enqueue_update(self, indices, eps, graph=None, subsets=None):
        """Enqueues `indices.shape[0]` learner iterations (no host sync).  indices: int64
        [iterations, B] host array (with a PrioritizedBuffer: its `sample_uniforms`, float64 [iterations, B] — the
        indices are drawn on the device between the critic steps); eps: float32 [iterations, draws, B, A] host array with the
        standard-normal draws in the order the reference consumes them.  With `graph` (default:
        on unless TONIC_AMD_NO_GRAPH=1) the launch sequence — gather, the fused forward / backward /
        grouped weight-gradient launches, Adam + polyak: 13 per SAC iteration — is captured once into a hipGraph
        reading fixed index / noise buffers and replayed on later calls (tonic_amd.q_update).
        subsets: int [iterations], REDQ's subset masks (bit z: target critic z + 1 is in the minimum), one per
        iteration; None: drawn by `_draw_subsets`."""
        return self._u.enqueue(indices, eps, graph, subsets=subsets)

    # -- the whole iteration through tonic_q_iteration (5 launches instead of 13)
    _FUSED = {updaters.DeterministicQLearning: (2, updaters.DeterministicPolicyGradient),
              updaters.TwinCriticDeterministicQLearning: (0, updaters.DeterministicPolicyGradient),
              updaters.TwinCriticSoftQLearning: (1, updaters.TwinCriticSoftDeterministicPolicyGradient)}

    def _fused_kind(self):
        """The `kind` of tonic_q_iteration when it serves this agent (QUpdate.route), else None."""
        return self._u.route().fused_kind

    def _fused_in_phases(self):
        """The fused iteration in two halves around what has to see the complete gradient sums (QUpdate.route)."""
        return self._u.route().in_phases

    # read-only, under the names other code knows: the last update's route and the current Slot's graph, noise
    # buffer and statistics rows
    _phased_update = property(lambda self: self._u.phased)
    _graph = property(lambda self: self._u.slot.graph)
    _static_eps = property(lambda self: self._u.slot.eps)
    _mpo_stats = property(lambda self: self._u.slot.stats)

    def _stats_width(self):
        """Floats per iteration the actor updater writes besides its statistics row (Slot.stats)."""
        return 0

    def _graph_signature(self):
        parts = []
        for updater in (self.actor_updater, self.critic_updater):
            hyper = updater.hyper
            noise = getattr(updater, 'target_action_noise', None)
            rule = getattr(updater, 'loss_rule', None)
            parts.append((tuple(sorted(hyper.items())),
                          (rule.kind, rule.param) if rule is not None else None,
                          float(getattr(updater, 'entropy_coeff', 0.0)),
                          float(getattr(updater, 'gradient_clip', 0.0) or 0.0),
                          int(getattr(updater, 'num_samples', 0)),
                          tuple(float(v) for v in getattr(updater, 'scale_bounds', None) or ()),
                          (noise.scale, noise.clip) if noise is not None else None,
                          # (the packed schedules: replays follow the device's step counters, so a scheduled
                          #  agent captures once)
                          updater.schedule_signature(),
                          dual.signature() if (dual := getattr(updater, 'dual_schedule', None)) is not None else None))
        norm = self.model.observation_normalizer
        # (the Return normaliser's _low / _high are read through their pointers by the captured launches)
        value_range = self.model.return_normalizer or None
        return (tuple(parts), float(self.model.target_coeff), getattr(self, 'delay_steps', 1),
                norm._mean.data_ptr() if norm is not None else 0,
                (value_range._low.data_ptr(), value_range._high.data_ptr()) if value_range is not None else None)

    def _noise_samples(self, draws):
        """Rows per state in each draw of `_draw_noise`: each updater reads the first c * samples rows of its own."""
        return (1,) * draws

    def _draw_noise(self, iterations):
        # DeterministicQLearning / DeterministicPolicyGradient draw nothing (one unused slot)
        return np.zeros((iterations, 1, self.replay.batch_size, self.action_size), np.float32)

    def _update_chunk(self, iterations, route=None):
        """Iterations per graph of an update call in chunks, 0: one graph (q_update.chunk_size).  A subclass with
        an enqueue_update or _update of its own gets none."""
        overridden = type(self)._update is not DDPG._update or type(self).enqueue_update is not DDPG.enqueue_update
        return chunk_size(iterations, int(getattr(self, 'delay_steps', 1) or 1), route or self._u.route(), overridden)

    def _update(self, steps):
        infos, stats = self._u.run()
        self.replay.last_steps = steps
        self._log_update(infos, stats)
        if self.model.observation_normalizer:
            self.model.observation_normalizer.update()
        if self.model.return_normalizer and self.serves_return_normalizer:
            # ddpg.py:102-103 / td3.py:54-55: behind the last iteration (the copies into _low / _high are enqueued
            # on the stream every graph replay of this update — chunks included — went to, and the infos were
            # read back above), the ranks' ranges merged first
            merge_reward_ranges(self.model.return_normalizer)
            self.model.return_normalizer.update()

    def _log_update(self, infos, stats):
        # (an ensemble of N critics logs one q, the mean over its critics: models.ActorCriticEnsembleWithTargets)
        twin = hasattr(self.model, 'critic_2') and not hasattr(self.model, 'num_critics')
        for row in infos[0]:
            logger.store('critic/loss', row[0])
            if twin:
                logger.store('critic/q1', row[1])    # batch means (log-equivalent)
                logger.store('critic/q2', row[2])
            elif not getattr(self.critic_updater, 'atoms', 0):
                logger.store('critic/q', row[1])
        for row in infos[1][infos[1][:, 6] > 0]:
            logger.store('actor/loss', row[0])
        self.last_infos = infos
        log_learning_rate('actor', self.actor_updater, self)
        log_learning_rate('critic', self.critic_updater, self)


def log_learning_rate(name, updater, agent):
    """With a scheduler on `updater`: one more key per update, `<name>/learning_rate`, the rate of the last step
    taken — tonic_lr_schedule_value at the device's step count less one, read behind the update's statistics
    read-back (the stream has drained: four bytes, no wait of its own).  Without a scheduler no key is added.
    The agent's `last_learning_rates` keeps {name: (rate, steps taken)}."""
    if getattr(updater, 'schedule', None) is None:
        return
    kept = agent.__dict__.setdefault('last_learning_rates', {})
    taken = int(updater.state[0])
    rate = updater.learning_rate(max(taken - 1, 0))
    logger.store(f'{name}/learning_rate', rate)
    kept[name] = (rate, taken)


def record_reward_range(normalizer, rewards):
    """ddpg.py:69-70 (`return_normalizer.record(rewards)`) as ONE record of the step's [min, max]: Return.record only
    keeps a running min / max, so the pair does what recording every reward does (the argument of
    tonic_reward_range, include/tonic_hip.h).  NaN is skipped — the reference's `<` / `>` are false for it — and
    a step whose rewards are all NaN records nothing; +-inf is kept."""
    rewards = np.asarray(rewards, np.float32).reshape(-1)
    rewards = rewards[~np.isnan(rewards)]
    if rewards.size:
        normalizer.record(np.array([rewards.min(), rewards.max()], np.float32))


def merge_reward_ranges(normalizer):
    """Several ranks: every rank's Return normaliser ends with the union of the ranks' (min_reward, max_reward) —
    what one process that saw every worker's rewards holds — as one all_reduce(MAX) of (-min, max), like
    A2C._range_rewards.  A rank that recorded nothing holds the initial (-1, 1), inside every range."""
    if not (torch.distributed.is_available() and torch.distributed.is_initialized()) \
            or torch.distributed.get_world_size() == 1:
        return
    pair = torch.tensor([-float(normalizer.min_reward), float(normalizer.max_reward)], dtype=torch.float32)
    if torch.distributed.get_backend() != 'gloo':
        pair = pair.to(_device())
    torch.distributed.all_reduce(pair, op=torch.distributed.ReduceOp.MAX)
    low, high = pair.cpu().numpy()
    normalizer.min_reward, normalizer.max_reward = np.float32(-low), np.float32(high)


def _d4pg_model():
    """tonic/torch/agents/d4pg.py:7-18 (support for the control suite with 0.99 discount)."""
    return models.ActorCriticWithTargets(
        actor=models.Actor(
            encoder=models.ObservationEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=models.DeterministicPolicyHead()),
        critic=models.Critic(
            encoder=models.ObservationActionEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU),
            head=models.DistributionalValueHead(-150., 150., 51)),
        observation_normalizer=normalizers.MeanStd())


class D4PG(DDPG):
    """tonic/torch/agents/d4pg.py:21-37: DDPG's acting / storing / scheduling with a categorical
    critic on 5-step returns (the HBM Buffer accumulates them, buffers.py:58-79)."""

    def __init__(self, model=None, replay=None, exploration=None, actor_updater=None,
                 critic_updater=None):
        super().__init__(
            model or _d4pg_model(), replay or replays.Buffer(return_steps=5), exploration,
            actor_updater or updaters.DistributionalDeterministicPolicyGradient(),
            critic_updater or updaters.DistributionalDeterministicQLearning())


def _mpo_model():
    """tonic/torch/agents/mpo.py:7-18."""
    return models.ActorCriticWithTargets(
        actor=models.Actor(
            encoder=models.ObservationEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=models.GaussianPolicyHead()),
        critic=models.Critic(
            encoder=models.ObservationActionEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=models.ValueHead()),
        observation_normalizer=normalizers.MeanStd())


class MPO(DDPG):
    """tonic/torch/agents/mpo.py:21-109: acts by sampling the Gaussian policy (no exploration
    object), stores 5-step returns, and per batch runs ExpectedSARSA, the MPO actor / dual step
    and the target update — DDPG's staging, HBM Buffer, hipGraph capture and schedule."""

    policy_kind = 2
    serves_return_normalizer = False     # (ExpectedSARSA and the E-step have no squashed form)

    def __init__(self, model=None, replay=None, actor_updater=None, critic_updater=None):
        super().__init__(
            model or _mpo_model(), replay or replays.Buffer(return_steps=5),
            explorations.NoActionNoise(start_steps=0),
            actor_updater or updaters.MaximumAPosterioriPolicyOptimization(),
            critic_updater or updaters.ExpectedSARSA())

    def step(self, observations, steps):
        actions = self._forward_policy(observations, 2, True)       # mpo.py:38-46, 77-80
        self.last_observations = observations.copy()
        self.last_actions = actions.copy()
        return actions

    def _noise_samples(self, draws):
        return (self.critic_updater.num_samples, self.actor_updater.num_samples)

    def _draw_noise(self, iterations):
        # per iteration: rsample((S_c,)) of ExpectedSARSA (critics.py:260), then sample((S_a,)) of the
        # actor step (actors.py:359) — [S, B, A] standard normals each, kept as the first S * B rows of a
        # [max(S_c, S_a) * B, A] block (the rows behind them zero, never read)
        B, A = self.replay.batch_size, self.action_size
        S_c, S_a = self._noise_samples(2)
        eps = np.zeros((iterations, 2, max(S_c, S_a) * B, A), np.float32)
        for it in range(iterations):
            eps[it, 0, :S_c * B] = torch.randn(S_c, B, A).numpy().reshape(S_c * B, A)
            eps[it, 1, :S_a * B] = torch.randn(S_a, B, A).numpy().reshape(S_a * B, A)
        return eps

    def _stats_width(self):
        return 9 + 2 * self.actor_updater.constraints

    def _log_update(self, infos, stats):
        for row, actor_row in zip(infos[0], stats):                 # mpo.py:92-97
            logger.store('critic/loss', row[0])
            logger.store('critic/q', row[1])
            for key, value in self.actor_updater.infos(actor_row).items():
                logger.store('actor/' + key, value)
        self.last_infos, self.last_actor_infos = infos, stats
        log_learning_rate('actor', self.actor_updater, self)
        log_learning_rate('critic', self.critic_updater, self)


def _dmpo_model():
    """MPO's model with the categorical critic head D4PG and TD4 default to."""
    model = _mpo_model()
    return models.ActorCriticWithTargets(
        actor=model.actor,
        critic=models.Critic(
            encoder=models.ObservationActionEncoder(), torso=model.critic.torso,
            head=models.DistributionalValueHead(-150., 150., 51)),
        observation_normalizer=model.observation_normalizer)


class DMPO(MPO):
    """Distributional MPO, an agent the library does not have: MPO's acting, actor and dual step on D4PG's
    categorical critic.  The critic step is DistributionalExpectedSARSA; the E-step reads the means of the target
    critic's distributions (MaximumAPosterioriPolicyOptimization on a critic with atoms).  Everything else — the
    noise draws, 5-step returns, scheduling, graph capture, several ranks — is MPO's."""

    def __init__(self, model=None, replay=None, actor_updater=None, critic_updater=None):
        super().__init__(model or _dmpo_model(), replay, actor_updater,
                         critic_updater or updaters.DistributionalExpectedSARSA())


class TD3(DDPG):
    """tonic/torch/agents/td3.py:20-55."""

    policy_kind = 0

    def __init__(self, model=None, replay=None, exploration=None, actor_updater=None,
                 critic_updater=None, delay_steps=2):
        super().__init__(
            model=model or _twin_model(models.DeterministicPolicyHead()), replay=replay,
            exploration=exploration,
            actor_updater=actor_updater or updaters.DeterministicPolicyGradient(),
            critic_updater=critic_updater or updaters.TwinCriticDeterministicQLearning())
        self.delay_steps = delay_steps
        self.model.critic = self.model.critic_1        # td3.py:36 (also a checkpoint alias)

    def _actor_due(self, iteration):
        return (iteration + 1) % self.delay_steps == 0     # td3.py:43-46 (quirk Q8)

    def _draw_noise(self, iterations):
        # TargetActionNoise: one torch.randn_like(actions) per critic update (critics.py:131)
        B, A = self.replay.batch_size, self.action_size
        return np.stack([torch.randn(B, A).numpy()[None] for _ in range(iterations)])


class TD4(TD3):
    """tonic/tensorflow/agents/td4.py:5-32, the one agent of the library without a torch form: TD3 — twin critics,
    clipped target-action noise, delayed actor and target updates — on D4PG's categorical critics and 5-step
    returns.  The actor ascends critic_1's mean (`model.critic`, the alias TD3 sets)."""

    def __init__(self, model=None, replay=None, exploration=None, actor_updater=None,
                 critic_updater=None, delay_steps=2):
        super().__init__(
            model=model or _twin_model(models.DeterministicPolicyHead(),
                                       models.DistributionalValueHead(-150., 150., 51)),
            replay=replay or replays.Buffer(return_steps=5), exploration=exploration,
            actor_updater=actor_updater or updaters.DistributionalDeterministicPolicyGradient(),
            critic_updater=critic_updater or updaters.TwinCriticDistributionalDeterministicQLearning(),
            delay_steps=delay_steps)


class SAC(DDPG):
    """tonic/torch/agents/sac.py:22-51.  `entropy_coeff_updater=updaters.EntropyCoeffTuning()` (None, the default:
    the reference's fixed coefficients, nothing changes) learns the entropy coefficient: per iteration the critic
    step and the actor step with alpha_t, then the coefficient's own step to alpha_{t+1} from the actor step's
    log-probabilities — on the updaters' split entries (tonic_tempered_*_q_grad), the updaters' own `entropy_coeff`
    floats unused."""

    policy_kind = 1

    def __init__(self, model=None, replay=None, exploration=None, actor_updater=None,
                 critic_updater=None, entropy_coeff_updater=None):
        self.entropy_coeff_updater = entropy_coeff_updater
        head = models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                         distribution=models.SquashedMultivariateNormalDiag)
        super().__init__(
            model=model or _twin_model(head), replay=replay,
            exploration=exploration or explorations.NoActionNoise(),
            actor_updater=actor_updater or updaters.TwinCriticSoftDeterministicPolicyGradient(),
            critic_updater=critic_updater or updaters.TwinCriticSoftQLearning())

    def _policy(self, observations):
        return self._forward_policy(observations, 1, True)        # sac.py:40-46

    def _draw_noise(self, iterations):
        # per iteration: rsample of the critic step, then rsample of the actor step
        B, A = self.replay.batch_size, self.action_size
        return np.stack([np.stack([torch.randn(B, A).numpy(), torch.randn(B, A).numpy()])
                         for _ in range(iterations)])

    # the updaters whose entries read a learned coefficient on the device: (critic, actor)
    _TEMPERED = (updaters.TwinCriticSoftQLearning, updaters.TwinCriticSoftDeterministicPolicyGradient)

    def initialize(self, observation_space, action_space, seed=None):
        tuner = self.entropy_coeff_updater
        if tuner is not None:       # (before anything is built: the tempered entries are these two updaters')
            for role, updater, served in (('critic_updater', self.critic_updater, self._TEMPERED[0]),
                                          ('actor_updater', self.actor_updater, self._TEMPERED[1])):
                if type(updater) is not served:
                    raise NotImplementedError(
                        f'{type(self).__name__}(entropy_coeff_updater=...) with {role}={type(updater).__name__}: a '
                        f'learned entropy coefficient is read on the device by {served.__name__} only')
        super().initialize(observation_space, action_space, seed=seed)
        if tuner is not None:
            tuner.initialize(self.model, self.action_size)
            self.critic_updater.entropy_coeff_updater = tuner
            self.actor_updater.entropy_coeff_updater = tuner

    def _stats_width(self):
        # the coefficient's statistics row {loss, mean log-prob, alpha before the step, ...} per iteration
        return updaters.INFO_WIDTH if self.entropy_coeff_updater is not None else 0

    def _graph_signature(self):
        signature, tuner = super()._graph_signature(), self.entropy_coeff_updater
        if tuner is None:
            return signature
        # (the coefficient itself is read through its pointer by the captured launches)
        return signature + ((tuple(sorted(tuner.hyper.items())), float(tuner.target_entropy),
                             tuner.log_entropy_coeff.data_ptr(), tuner.schedule_signature()),)

    def _log_update(self, infos, stats):
        super()._log_update(infos, stats)
        if self.entropy_coeff_updater is not None and stats is not None:
            for row in stats:
                logger.store('entropy_coeff/loss', row[0])
                logger.store('entropy_coeff/value', row[2])          # alpha the iteration's two steps used
                logger.store('entropy_coeff/entropy', -row[1])       # mean -log pi of the actor step's sample
            self.last_entropy_coeff_infos = stats
        if self.entropy_coeff_updater is not None:
            log_learning_rate('entropy_coeff', self.entropy_coeff_updater, self)

    def save(self, path):
        super().save(path)          # the .pt of the reference, as ever
        if self.entropy_coeff_updater is not None:
            torch.save(self.entropy_coeff_updater.state_dict(), path + '.entropy_coeff.pt')

    def load(self, path):
        super().load(path)
        sibling = path + '.entropy_coeff.pt'
        if self.entropy_coeff_updater is not None and os.path.exists(sibling):   # (absent: the initial value stays)
            self.entropy_coeff_updater.load_state_dict(torch.load(sibling, map_location='cpu'))


class TQC(SAC):
    """Truncated quantile critics (Kuznetsov et al. 2020; the reference has no such agent): SAC — acting, noise
    draws, scheduling, checkpoints, log keys and the optional `entropy_coeff_updater` — on two critics of 25 quantiles
    each, whose pooled target quantiles are sorted and truncated at the top (updaters.TruncatedQuantileQLearning,
    updaters.TwinCriticQuantileSoftPolicyGradient).  The updaters run the split route.  The paper's 5 critics:
    `model=models.ActorCriticEnsembleWithTargets(actor, critic, num_critics=5, ...)`, 2 .. 8 critics with
    num_critics x num_quantiles <= 256; the log then carries critic/q, the mean over the critics, for critic/q1, q2."""

    _TEMPERED = (updaters.TruncatedQuantileQLearning, updaters.TwinCriticQuantileSoftPolicyGradient)

    def __init__(self, model=None, replay=None, exploration=None, actor_updater=None,
                 critic_updater=None, entropy_coeff_updater=None):
        head = models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                         distribution=models.SquashedMultivariateNormalDiag)
        super().__init__(
            model=model or _twin_model(head, models.QuantileValueHead(25)), replay=replay, exploration=exploration,
            actor_updater=actor_updater or updaters.TwinCriticQuantileSoftPolicyGradient(),
            critic_updater=critic_updater or updaters.TruncatedQuantileQLearning(),
            entropy_coeff_updater=entropy_coeff_updater)

    def _graph_signature(self):
        return super()._graph_signature() + (getattr(self.critic_updater, 'top_quantiles_to_drop_per_net', None),)


def _redq_model(head):
    """SAC's default networks with 5 scalar critics."""
    return models.ActorCriticEnsembleWithTargets(
        actor=models.Actor(
            encoder=models.ObservationEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=head),
        critic=models.Critic(
            encoder=models.ObservationActionEncoder(),
            torso=models.MLP((256, 256), torch.nn.ReLU), head=models.ValueHead()),
        num_critics=5, observation_normalizer=normalizers.MeanStd())


class REDQ(SAC):
    """Randomized ensembled double Q-learning (Chen et al. 2021; the reference has no such agent): SAC — acting, noise
    draws, scheduling, checkpoints and the optional `entropy_coeff_updater` — on an ensemble of 5 scalar critics
    (models.ActorCriticEnsembleWithTargets, 2 .. 8 critics).  Every learner iteration draws `subset_size` (2) of the
    target critics, whose minimum forms the TD target of ALL the online critics (updaters.EnsembleSoftQLearning); the
    actor ascends the mean of all of them (updaters.EnsembleSoftPolicyGradient).  The default replay runs 20 learner
    iterations per environment step (an update-to-data ratio of 20).  The updaters run the split route.

    The subsets come from a generator of the agent's own, seeded from `initialize(seed=...)` — not torch's global
    stream, not the replay's — one draw per iteration: chunked updates and SAC's noise order cannot move it, and every
    rank of several holds the same subsets (equal seeds, like the index stream).  They reach the GPU as one int32 per
    iteration in the update's Slot, uploaded with the noise; the critic step's loss kernel reads its word, so one
    captured graph serves every draw.  The log carries critic/loss, critic/q (the mean over the critics) and
    actor/loss."""

    _TEMPERED = (updaters.EnsembleSoftQLearning, updaters.EnsembleSoftPolicyGradient)

    def __init__(self, model=None, replay=None, exploration=None, actor_updater=None,
                 critic_updater=None, entropy_coeff_updater=None):
        head = models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                         distribution=models.SquashedMultivariateNormalDiag)
        super().__init__(
            model=model or _redq_model(head),
            replay=replay or replays.Buffer(batch_size=256, batch_iterations=20, steps_between_batches=1),
            exploration=exploration,
            actor_updater=actor_updater or updaters.EnsembleSoftPolicyGradient(),
            critic_updater=critic_updater or updaters.EnsembleSoftQLearning(),
            entropy_coeff_updater=entropy_coeff_updater)

    SUBSET_STREAM = 0x52454451       # what the subsets' seed adds to the agent's, apart from the replay's index stream

    def initialize(self, observation_space, action_space, seed=None):
        super().initialize(observation_space, action_space, seed=seed)
        self._seed_subsets(seed)

    def _seed_subsets(self, seed):
        self._subset_generator = np.random.RandomState(None if seed is None else (seed + self.SUBSET_STREAM) % 2 ** 32)

    def _draw_subsets(self, iterations):
        critic = self.critic_updater
        if not getattr(critic, 'takes_subset', False):
            return None
        return updaters.draw_subset_masks(self._subset_generator, iterations, self.model.num_critics,
                                          critic.subset_size)

    def _graph_signature(self):
        return super()._graph_signature() + ((getattr(self.model, 'num_critics', None),
                                              getattr(self.critic_updater, 'subset_size', None)),)
