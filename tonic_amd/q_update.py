"""How one update call of the off-policy agents reaches the GPU: ``QUpdate`` is an agent's
scheduler — route, captured graphs, chunks — ``Slot`` one set of what a captured graph reads and writes."""
import ctypes
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from tonic_amd import _lib, parallel


class Route(NamedTuple):
    """The routing decision of one update call.

    fused_kind  the `kind` of tonic_q_iteration when it serves the agent, None: the updaters' split entry points
    in_phases   something has to see the complete gradient sums before the step — the exchange between ranks, a
                gradient-norm clip — and TONIC_AMD_FUSED_PHASES lets the fused iteration run in two halves round it"""
    fused_kind: Optional[int]
    in_phases: bool

    @property
    def phased(self):
        return self.fused_kind is not None and self.in_phases


def shard_noise(eps, positions, counts, global_batch, samples=None):
    """The rows of the GLOBAL noise draws that belong to this rank's part of each batch.
    eps [iterations, draws, S * B, A]: S draws per state of the global batch, sample-major (row
    s * B + m; S = 1 for everything but MPO).  positions[it, :counts[it]] = the batch positions m
    this rank owns.  Returns the same shape with row s * c + j = eps row s * B + positions[j]
    (c = counts[it]) in front and zeros behind: what the kernels see as a batch of c states.
    samples: S of each draw when the draws differ (draw d fills its first samples[d] * B rows, MPO with two
    sample counts); default: every draw fills the rows."""
    local = np.zeros_like(eps)
    draws, width = eps.shape[1], eps.shape[3]
    if samples is None:
        samples = (eps.shape[2] // global_batch,) * draws
    for it in range(eps.shape[0]):
        c = counts[it]
        for d, per_sample in enumerate(samples):
            kept = eps[it, d, :per_sample * global_batch].reshape(per_sample, global_batch, width)
            local[it, d, :per_sample * c] = kept[:, positions[it, :c]].reshape(per_sample * c, width)   # (c may be 0)
    return local


def ride_plan(due, ahead_supported):
    """(stage, slot, rides) of every fused iteration of one update call.  With delayed actor updates (td3.py:43-46)
    the policy passes (launch 1) of iteration k + 1 — they read the actor, the target actor, ITS batch and noise,
    none of which a critic step writes — ride as more workgroups in the critic-step launch of an iteration k that
    does not step the actor (tonic_q_iteration_t.ahead: the workspace's other set of launch-1 outputs; iteration
    k + 1 then starts behind them, stage 2).  At B = 100 a launch fills a ninth of the chip: one launch and its
    dispatch less per pair of iterations.  due[it]: iteration it steps the actor; ahead_supported(it): the kernels
    can run iteration it + 1's passes in iteration it's critic step (asked only where they would)."""
    plan, slot, behind = [], 0, False
    for it in range(len(due)):
        rides = not due[it] and it + 1 < len(due) and bool(ahead_supported(it))
        plan.append((2 if behind else 0, slot, rides))
        if rides:
            slot ^= 1                # (the passes ahead write the other set: the next iteration's)
        behind = rides
    return plan


def adam_table(iterations, due, critic_hyper, actor_hyper, critic_steps, actor_steps, schedules=(None, None)):
    """The optimizer steps' float64 constants, formed on the host like the reference's Python floats:
    [iteration, {critic, actor}, {step_size, bias_correction2_sqrt}] as float32 (an actor row that is not due stays
    zero), and the two step counters behind the last iteration.  `schedules`: the (critic's, actor's) packed
    tonic_lr_schedule_t or None — step number `step` (1-based) is taken at the rate of `step - 1` steps taken:
    step_size = F32(tonic_lr_schedule_value(schedule, lr, step - 1) / bias_correction1)."""
    from tonic_amd.torch.updaters import adam_step_constants, lr_schedule_value

    def constants(hyper, schedule, step):
        if schedule is not None:
            hyper = dict(hyper, lr=lr_schedule_value(schedule, hyper['lr'], step - 1))
        return adam_step_constants(hyper, step)

    table = np.zeros((iterations, 2, 2), np.float32)
    for it in range(iterations):
        critic_steps += 1
        table[it, 0] = constants(critic_hyper, schedules[0], critic_steps)
        if due[it]:
            actor_steps += 1
            table[it, 1] = constants(actor_hyper, schedules[1], actor_steps)
    return table, critic_steps, actor_steps


def chunk_size(iterations, delay, route, overridden):
    """How many iterations one graph of a chunked update holds (0: one graph for the whole call).  The streams
    are drawn in the reference's order either way (indices: the Buffer's RandomState, noise: torch's CPU
    generator, both only consumed by this call while it runs) — chunking only moves WHEN the host draws them:
    7.6 -> ~6 ms per SAC update call of 50 iterations, whose 2 ms of host draws ran in front of 5.4 ms of GPU
    work (profiles/r06_offpolicy_pmc.md).  Needs the fused iteration, whole, in a hipGraph (several ranks and an
    exercised exchange are in `route`: they need the complete sums); chunks hold a whole number of actor delays;
    `overridden`: a subclass with its own enqueue_update / _update.  TONIC_AMD_UPDATE_CHUNK=0: off; =n: n
    iterations per chunk."""
    chunk = int(os.environ.get('TONIC_AMD_UPDATE_CHUNK', '10'))
    if (chunk <= 0 or iterations < 2 * chunk or iterations % chunk or chunk % delay or overridden
            or os.environ.get('TONIC_AMD_NO_GRAPH', '0') == '1' or route.fused_kind is None or route.in_phases):
        return 0
    return chunk


def _check_chain(infos):
    """A chained launch whose workgroups waited 250 ms for a value of a peer that never came (a GPU
    shared with something that starves the launch, a lost workgroup) does not hang and does not step:
    the iteration's optimizer epilogues wrote nothing and marked their statistic rows (slot 7).  The
    parameters are intact; the update is incomplete, which is an error and not a log line."""
    gave_up = np.argwhere(infos[..., 7] > 0)
    if len(gave_up):
        raise _lib.TonicHipError(
            f'{len(gave_up)} optimizer steps of this update were skipped: a chained launch gave up '
            f'waiting for a peer workgroup (first: updater {gave_up[0][0]}, iteration '
            f'{gave_up[0][1]}); parameters, moments and targets are those of the last complete '
            'iteration (TONIC_AMD_TUNING=q_chain=0 runs one launch per pass)')


class Slot:
    """Everything a captured update graph reads and writes; two of them, so that one is replayed while the host
    fills the other (an update call in chunks).

    key      what the graph bakes in — shapes, the replay's storage, the agent's `_graph_signature()` — a change of
             any of it allocates `indices`, `eps`, `infos` anew and drops the graph
    indices  int64 [iterations, B]: the replay rows of every batch
    eps      float32 [iterations, draws, S * B, A]: the standard-normal draws
    adam     float32 [iterations, 2, 2] (`adam_table`) or None: only the whole fused iteration reads it
    infos    float32 [2, iterations, INFO_WIDTH]: the critic's and the actor's statistics rows
    stats    float32 [iterations, width] or None: the agent's `_stats_width()` more per iteration (MPO; SAC with
             a learned entropy coefficient: the coefficient's statistics rows)
    subsets  int32 [iterations] or None: one word per iteration that the critic step reads on the device (REDQ: the
             mask of the target critics in the minimum), uploaded with the noise; iteration `it`'s step gets the
             pointer to element `it`
    graph    the captured hipGraph; None: the next call through a graph captures
    With a PrioritizedBuffer `indices` is an OUTPUT of the graph, and there are three more:
    uniforms       float64 [iterations, B]: the host's draws, uploaded like `indices` otherwise
    weights        float32 [iterations, B]: the batches' importance weights
    sample_losses  float32 [iterations, B]: the rows' unweighted critic losses, the next priorities"""

    __slots__ = ('key', 'indices', 'eps', 'adam', 'infos', 'stats', 'graph', 'uniforms', 'weights', 'sample_losses',
                 'subsets')

    def __init__(self):
        self.key = self.indices = self.eps = self.adam = self.infos = self.stats = self.graph = None
        self.uniforms = self.weights = self.sample_losses = self.subsets = None


class QUpdate:
    """One agent's update scheduler.

    slots         the two Slots; `slot` is the one the next `enqueue` fills and replays
    workspace     tonic_q_iteration's workspace (its first word: the failure word of an update in phases), grown on
                  demand; None before the first fused iteration
    phased        the last `enqueue` ran the fused iteration in phases
    mirror_valid  the updaters' `steps_enqueued` equal the device's step counters: only behind a whole fused
                  iteration whose launches all went out.  The split entries (whose captured graphs step the device
                  counter on every replay), the phases, an exception on the way to the launches and a skipped step
                  leave the device the authority: the next Adam table starts with one read-back of `state[0]`
    """

    def __init__(self, agent):
        self.agent = agent
        self.slots = (Slot(), Slot())
        self.slot = self.slots[0]
        self.workspace, self.phased, self.mirror_valid = None, False, False

    @property
    def prioritized(self):
        """The replay draws by priority: the split route in its prioritized form (`_issue_prioritized`)."""
        from tonic_amd.replays import PrioritizedBuffer
        return isinstance(self.agent.replay, PrioritizedBuffer)

    def route(self):
        """tonic_q_iteration serves the plain DDPG / TD3 / SAC updaters (`agent._FUSED`) with plain Adam, no
        Return normaliser (no squashed value head there), no learned entropy coefficient (no tempered form) and shapes inside the fused kernels; what needs the
        complete sums gets it in phases, or the split entry points with TONIC_AMD_FUSED_PHASES=0.
        TONIC_AMD_FUSED_ITERATION=0 keeps the split entry points (the tests compare the two)."""
        agent, critic, actor = self.agent, self.agent.critic_updater, self.agent.actor_updater
        complete = parallel.exchanging() or critic.world_size > 1 or critic.gradient_clip > 0 \
            or actor.gradient_clip > 0
        in_phases = complete and os.environ.get('TONIC_AMD_FUSED_PHASES', '1') != '0'
        kind, actor_class = agent._FUSED.get(type(critic), (None, None))
        if kind is None or type(actor) is not actor_class or critic.stock or actor.stock \
                or agent.model.return_normalizer or not (critic.plain and actor.plain) \
                or getattr(agent, 'entropy_coeff_updater', None) is not None \
                or os.environ.get('TONIC_AMD_FUSED_ITERATION', '1') == '0' \
                or not agent.lib.tonic_q_iteration_supported(agent.observation_size, agent.hidden, agent.action_size,
                                                             2 if kind == 1 else 1) \
                or (complete and not in_phases):
            kind = None
        return Route(kind, in_phases)

    # ------------------------------------------------------------------ one update call
    def run(self):
        """Draws the index and noise streams, enqueues the update — in chunks when `chunk_size` says so: the host
        draws chunk k + 1's streams while the GPU runs chunk k — and reads the statistics back: (infos, stats)."""
        agent, replay = self.agent, self.agent.replay
        route, parts, stats = self.route(), [], None
        chunk = agent._update_chunk(replay.batch_iterations, route)
        if chunk:
            for k in range(replay.batch_iterations // chunk):
                indices = replay.sample_indices(chunk)         # (host: while the GPU runs the chunk before)
                eps = agent._draw_noise(chunk)
                self.slot = self.slots[k & 1]
                parts.append(self.enqueue(indices, eps, route=route).clone())
            self.slot = self.slots[0]
            infos = torch.cat(parts, dim=1).cpu().numpy()
        else:
            indices = replay.sample_uniforms() if self.prioritized else replay.sample_indices()
            eps = agent._draw_noise(indices.shape[0])
            infos = agent.enqueue_update(indices, eps).cpu().numpy()
            if self.slot.stats is not None:
                stats = self.slot.stats.cpu().numpy()
        parallel.check_one_shot()
        if self.phased and int(self.workspace[:4].view(torch.int32)[0]):
            # (in phases the steps are the updaters' own launches: nothing held them back)
            raise _lib.TonicHipError(
                'a chained launch of this update gave up waiting for a peer workgroup (250 ms): its gradient '
                'sums were incomplete and have been stepped on — the parameters are no longer valid '
                '(TONIC_AMD_TUNING=q_chain=0 runs one launch per pass)')
        try:
            _check_chain(infos)
        except _lib.TonicHipError:
            self.mirror_valid = False          # skipped steps: the device's counters decide
            raise
        return infos, stats

    def enqueue(self, indices, eps, graph=None, route=None, subsets=None):
        """`agent.enqueue_update`: shard, fill the current slot, issue the iterations or replay their graph.
        With a PrioritizedBuffer `indices` are its uniforms (float64 [iterations, B]).  subsets: the iterations'
        words of a critic step that reads one (REDQ), int [iterations]; None: the agent draws them — from a stream
        of its own, the same on every rank, so neither the chunks nor the shards move it."""
        agent = self.agent
        prioritized = self.prioritized
        iterations, global_batch = indices.shape
        subsets = self._subsets(subsets, iterations)
        agent._q.parameters_changed()
        counts = None
        if agent.critic_updater.world_size > 1:
            # every rank draws the same GLOBAL index / noise stream and keeps the
            # samples whose worker column lives in its shard (binomial split, mean B / world);
            # gradient SUMS are all-reduced and scaled by 1 / B_global, so the update equals the
            # single-process one on the global buffer.
            indices, positions, counts = agent.replay.shard_indices(indices)
            eps = shard_noise(eps, positions, counts, global_batch, agent._noise_samples(eps.shape[1]))
        slot = self._prepare(indices, eps, subsets)
        if graph is None:
            graph = os.environ.get('TONIC_AMD_NO_GRAPH', '0') != '1'
        route = route or self.route()
        due = [bool(agent._actor_due(it)) for it in range(iterations)]
        self.phased = route.phased
        if route.phased:
            self._workspace_for(max(indices.shape[1], 1))[:4].zero_()   # the update's failure word
        elif route.fused_kind is not None:
            self._upload_adam_table(slot, due)

        def issue():
            slot.infos.zero_()
            if prioritized:
                return self._issue_prioritized(due)
            # the store does not change during an update: the batches of ALL its iterations are
            # gathered by one launch (the rows a rank does not own are padding, never read)
            batches = agent.replay.gather_many(slot.indices)
            if route.fused_kind is None:
                self._issue_split(batches, due, counts, global_batch)
            elif route.phased:
                self._issue_phased(route.fused_kind, batches, due, counts, global_batch)
            else:
                self._issue_fused(route.fused_kind, batches, due)
        stock = agent.critic_updater.stock or agent.actor_updater.stock    # (autograd: no capture)
        if not graph or stock or parallel.exchanging():      # collectives sit between the kernels
            issue()
        else:
            if slot.graph is None:
                self._capture(slot, route, indices.shape[1], issue, gathers_many=not prioritized)
            slot.graph.replay()
        self.mirror_valid = route.fused_kind is not None and not route.phased
        return slot.infos

    def _subsets(self, subsets, iterations):
        """The iterations' words as int32 [iterations]: those given, else the agent's draw (None: it has none)."""
        agent = self.agent
        if not getattr(agent.critic_updater, 'takes_subset', False):
            if subsets is not None:
                raise ValueError(f'subsets= goes with a critic updater that reads one per iteration (REDQ\'s '
                                 f'EnsembleSoftQLearning), not with {type(agent.critic_updater).__name__}')
            return None
        if subsets is None:
            return agent._draw_subsets(iterations)
        given = np.asarray(subsets)
        if given.shape != (iterations,) or given.dtype.kind not in 'iu':
            raise ValueError(f'subsets: an int array of one mask per iteration, shape ({iterations},), got '
                             f'{given.dtype} {given.shape}')
        return given.astype(np.int32)

    def _prepare(self, indices, eps, subsets=None):
        agent, slot, iterations = self.agent, self.slot, indices.shape[0]
        # everything a captured graph bakes in: shapes, the replay's storage, the updaters'
        # hyper-parameters and schedules — a change of any of them re-captures
        prioritized = self.prioritized
        key = (iterations, tuple(eps.shape), agent.replay.buffers['observations'].data_ptr(),
               agent.replay.max_size, agent._graph_signature(),
               agent.replay.graph_signature() if prioritized else None)
        if slot.key != key:
            from tonic_amd.torch.updaters import INFO_WIDTH      # (tonic_amd.torch imports this module)
            slot.key = key
            slot.indices = torch.zeros(indices.shape, dtype=torch.int64, device=agent.device)
            slot.eps = torch.zeros(eps.shape, dtype=torch.float32, device=agent.device)
            slot.infos = torch.zeros(2, iterations, INFO_WIDTH, device=agent.device)
            slot.graph = None
            slot.uniforms = slot.weights = slot.sample_losses = None
            slot.subsets = None if subsets is None else torch.zeros(iterations, dtype=torch.int32, device=agent.device)
            if prioritized:
                slot.uniforms = torch.zeros(indices.shape, dtype=torch.float64, device=agent.device)
                slot.weights = torch.zeros(indices.shape, dtype=torch.float32, device=agent.device)
                slot.sample_losses = torch.zeros(indices.shape, dtype=torch.float32, device=agent.device)
        width = agent._stats_width()
        if width and (slot.stats is None or tuple(slot.stats.shape) != (iterations, width)):
            slot.stats = torch.zeros(iterations, width, device=agent.device)
            slot.graph = None
        (slot.uniforms if prioritized else slot.indices).copy_(torch.as_tensor(indices), non_blocking=True)
        slot.eps.copy_(torch.as_tensor(eps), non_blocking=True)
        if subsets is not None:
            slot.subsets.copy_(torch.as_tensor(subsets), non_blocking=True)
        return slot

    def _upload_adam_table(self, slot, due):
        critic, actor = self.agent.critic_updater, self.agent.actor_updater
        if not self.mirror_valid:            # (one read-back, then none again)
            critic.steps_enqueued = int(critic.state[0])
            actor.steps_enqueued = int(actor.state[0])
        self.mirror_valid = False            # until this update's launches are out
        table, critic.steps_enqueued, actor.steps_enqueued = adam_table(
            len(due), due, critic.hyper, actor.hyper, critic.steps_enqueued, actor.steps_enqueued,
            schedules=(critic.schedule, actor.schedule))
        if slot.adam is None or slot.adam.shape != table.shape:
            slot.adam = torch.zeros(table.shape, device=self.agent.device)
            slot.graph = None
        slot.adam.copy_(torch.as_tensor(table), non_blocking=True)

    def _capture(self, slot, route, batch_size, issue, gathers_many=True):
        agent = self.agent
        agent.critic_updater._offpolicy_workspace(batch_size)    # allocate outside the capture
        agent.actor_updater._offpolicy_workspace(batch_size)
        if gathers_many:
            agent.replay.gather_many(slot.indices)
        if route.fused_kind is not None:
            self._workspace_for(batch_size)
        torch.cuda.synchronize()
        slot.graph = torch.cuda.CUDAGraph()
        with _lib.capturing(slot.graph):
            issue()

    # ------------------------------------------------------------------ the iterations of one call, per route
    def _targets(self):
        # update_targets() (ddpg.py:112) rides in the actor's optimizer launch
        model = self.agent.model
        return (model.flat_target, model.flat_online, 0, model.target_coeff)

    def _actor_step(self, observations, eps, it, n_global):
        """The actor updater's own entry (observations None: this rank drew none of the global batch)."""
        actor, slot = self.agent.actor_updater, self.slot
        tuner = getattr(self.agent, 'entropy_coeff_updater', None)     # (SAC: slot.stats rows are the coefficient's)
        more = {} if slot.stats is None or tuner is not None else {'stats_row': slot.stats[it]}
        if observations is None:
            actor.enqueue_empty(slot.infos[1, it], n_global, self._targets(), **more)
        else:
            actor.enqueue(observations, eps, slot.infos[1, it], n_global, self._targets(), **more)
        if tuner is not None:       # alpha_t -> alpha_{t+1} from this actor step's sums, ahead of the next critic step
            if observations is None:
                tuner.enqueue_empty(slot.stats[it], n_global)
            else:
                tuner.enqueue_step(slot.stats[it], n_global or observations.shape[0] * tuner.world_size)

    def _issue_split(self, batches, due, counts, global_batch):
        critic, slot = self.agent.critic_updater, self.slot
        draws = slot.eps.shape[1]
        samples = self.agent._noise_samples(draws)     # rows per state of each draw (MPO: its updater's num_samples)
        n_global = None if counts is None else global_batch
        for it in range(len(due)):
            c = global_batch if counts is None else int(counts[it])
            if c > 0:
                batch = {k: v[it, :c] for k, v in batches.items()}
                more = {} if slot.subsets is None else {'subset': slot.subsets[it:it + 1]}
                critic.enqueue(batch, slot.eps[it, 0, :c * samples[0]], slot.infos[0, it], n_global, **more)
            else:
                critic.enqueue_empty(slot.infos[0, it], n_global)
            if due[it]:
                actor_eps = slot.eps[it, 1, :c * samples[1]] if c > 0 and draws > 1 else None
                self._actor_step(batch['observations'] if c > 0 else None, actor_eps, it, n_global)

    def _issue_prioritized(self, due):
        """The split route on a PrioritizedBuffer (one rank): the batch of iteration k + 1 depends on the losses of
        iteration k, so every iteration draws and gathers its own — sample -> single-batch gather -> weighted
        critic step -> priority update -> actor step when due — all of it inside the captured graph."""
        critic, slot, replay = self.agent.critic_updater, self.slot, self.agent.replay
        draws = slot.eps.shape[1]
        for it in range(len(due)):
            replay.sample(slot.uniforms[it], slot.indices[it], slot.weights[it])
            batch = replay.gather(slot.indices[it])
            critic.enqueue(batch, slot.eps[it, 0], slot.infos[0, it], None, weights=slot.weights[it],
                           sample_losses=slot.sample_losses[it])
            replay.update_priorities(slot.indices[it], slot.sample_losses[it])
            if due[it]:
                self._actor_step(batch['observations'], slot.eps[it, 1] if draws > 1 else None, it, None)

    def _issue_phased(self, kind, batches, due, counts, global_batch):
        """An iteration as [policy passes + critic step + critics' weight gradients] -> exchange / clip + Adam
        -> [actor step + actor's weight gradients] -> exchange / clip + Adam + polyak (tonic_q_iteration_t.phase
        1 / 2, the steps through the updaters' own `_step` like the split entry points): 3 + 1 + 2 + 1 launches
        around the two exchanges instead of the split entry points' 4 + 1 + 5 + 1."""
        critic, actor, slot = self.agent.critic_updater, self.agent.actor_updater, self.slot
        n_global = None if counts is None else global_batch
        for it in range(len(due)):
            c = global_batch if counts is None else int(counts[it])
            if c == 0:                                  # this rank drew none of the global batch
                critic.enqueue_empty(slot.infos[0, it], n_global)
                if due[it]:
                    self._actor_step(None, None, it, n_global)
                continue
            batch = {k: v[it, :c] for k, v in batches.items()}
            n = n_global or c * critic.world_size
            self._launch(self._arguments(kind, batch, it, due[it], phase=1))
            critic._step(n, slot.infos[0, it])
            if due[it]:
                self._launch(self._arguments(kind, batch, it, due[it], phase=2))
                actor._step(n, slot.infos[1, it], targets=self._targets())

    def _issue_fused(self, kind, batches, due):
        """The whole iteration per tonic_q_iteration call (5 launches instead of 13), the next iteration's policy
        passes riding ahead where `ride_plan` says so.  Same kernels' code on the same inputs: the same bits
        (TONIC_AMD_POLICY_AHEAD=0: every iteration by itself; the tests compare)."""
        agent = self.agent
        B, nets = batches['observations'].shape[1], 1 if kind == 2 else 2
        ahead_on = os.environ.get('TONIC_AMD_POLICY_AHEAD', '1') != '0'

        def ahead_supported(it):
            return ahead_on and agent.lib.tonic_q_iteration_ahead_supported(
                B, agent.observation_size, agent.hidden, agent.action_size, nets, 2 if due[it + 1] else 1)
        plan = ride_plan(due, ahead_supported)
        args = [self._arguments(kind, {k: v[it] for k, v in batches.items()}, it, due[it], stage=stage, slot=slot)
                for it, (stage, slot, _) in enumerate(plan)]
        for it, (_, _, rides) in enumerate(plan):
            if rides:
                args[it].ahead = ctypes.addressof(args[it + 1])      # (read during this call only; `args` lives on)
            self._launch(args[it])

    def _launch(self, arguments):
        _lib.check(self.agent.lib.tonic_q_iteration(ctypes.byref(arguments), _lib.current_stream()),
                   'tonic_q_iteration')

    def _workspace_for(self, batch_size):
        agent = self.agent
        need = agent.lib.tonic_q_iteration_workspace_bytes(batch_size, agent.observation_size, agent.action_size,
                                                           agent.hidden)
        if self.workspace is None or self.workspace.numel() < need:
            # (zero-filled: its head holds the arrival words of the chained launches)
            self.workspace = torch.zeros(need, dtype=torch.uint8, device=agent.device)
        return self.workspace

    def _arguments(self, kind, batch, iteration, actor_due, phase=0, stage=0, slot=0):
        agent, own, p = self.agent, self.slot, _lib.ptr
        critic, actor, model = agent.critic_updater, agent.actor_updater, agent.model
        B = batch['observations'].shape[0]
        ws = self._workspace_for(B)
        mean, std = critic.norm_tensors()
        noise = getattr(critic, 'target_action_noise', None)
        eps = own.eps

        def optimizer(updater, info_row, constants):
            h = updater.hyper
            return _lib.QOptimizer(p(updater.grad_sums), p(updater.exp_avg), p(updater.exp_avg_sq),
                                   p(updater.state), p(info_row), p(constants), h['lr'],
                                   h['betas'][0], h['betas'][1], h['eps'])
        return _lib.QIteration(
            kind=kind, actor_due=int(bool(actor_due)), B=B, O=agent.observation_size, H=agent.hidden,
            A=agent.action_size, global_batch=B,
            d_actor=p(model.flat_actor.flat), d_critics=p(model.flat_critics.flat),
            d_target_actor=p(model.flat_target_actor.flat),
            d_target_critics=p(model.flat_target_critics.flat),
            d_norm_mean=p(mean), d_norm_std=p(std), norm_clip=critic.norm_clip(),
            d_observations=p(batch['observations']), d_actions=p(batch['actions']),
            d_next_observations=p(batch['next_observations']), d_rewards=p(batch['rewards']),
            d_discounts=p(batch['discounts']),
            d_eps_critic=p(eps[iteration, 0]) if kind != 2 else None,
            d_eps_actor=p(eps[iteration, 1]) if kind == 1 else None,
            critic_entropy_coeff=float(getattr(critic, 'entropy_coeff', 0.0)),
            actor_entropy_coeff=float(getattr(actor, 'entropy_coeff', 0.0)),
            noise_scale=float(noise.scale if noise else 0.0),
            noise_clip=float(noise.clip if noise else 0.0),
            target_coeff=float(model.target_coeff),
            critic=optimizer(critic, own.infos[0, iteration], own.adam[iteration, 0] if phase == 0 else None),
            actor=optimizer(actor, own.infos[1, iteration], own.adam[iteration, 1] if phase == 0 else None),
            d_workspace=p(ws), workspace_bytes=ws.numel(), phase=phase, stage=stage, slot=slot,
            critic_loss=critic.loss_rule,
            # the workspace's fp16x2 weight images follow the optimizer epilogues INSIDE an update call; between
            # calls anybody may have written parameters (load_state_dict, another path): rebuilt on iteration 0
            refresh_images=int(iteration == 0 or phase != 0))
