"""PPO's critic iterations under the next rollout: ``CriticChain`` is one agent's chain on the
process's side stream, the record of the one in flight and the gate that holds it back."""
import math
import os
import time
import weakref

import torch

from tonic_amd import _lib, parallel

_SIDE_STREAMS = {}


def _side_stream(name):
    """One stream per purpose and device for the whole process, not one per agent: HIP maps the
    streams of a process onto a handful of hardware queues in creation order, and two streams on one
    queue run one after the other — an agent whose critic stream landed on its collector's queue
    would get no overlap at all (seen in a process that had built a dozen agents before)."""
    key = (name, torch.cuda.current_device())
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream()
    return _SIDE_STREAMS[key]


def gate_row(rows, chain_ms, step_us, margin_ms, rollout_us):
    """The row of a `rows`-row rollout (host time `step_us` per row) from which a chain of `chain_ms` just finishes
    before the rollout does, or None: nothing measured yet; the chain needs the whole rollout; a rollout much longer
    than the device's ramp (`rollout_us`) — nothing to gain, and a polling wave must not sit in a hardware queue for
    long (HIP streams share a handful of them: whatever another stream launches into that queue waits behind it)."""
    if not chain_ms or not step_us:
        return None
    row = rows - math.ceil((1.1 * chain_ms + margin_ms) * 1e3 / step_us)
    if row <= 0 or rows * step_us > rollout_us:
        return None
    return row


class CriticChain:
    """The two networks of an update share nothing (ppo.py:33-46: advantages and returns are formed before the first
    iteration), and a rollout needs the ACTOR only.  So on one GPU with full-batch iterations PPO._update runs the
    actor's iterations, hands the critic's to a second HIP stream BEHIND them and returns: the critic's kernels run on
    the compute units the resident collect kernel leaves while the host drives the next rollout, whose collect loop is
    latency-bound.  Everything that reads the critic settles first; what the chain still reads is kept out of the
    rollout's way: the rollout writes its observations to a spare buffer (PolicyBlock.behind), the normalisers are
    snapshot.  The launches are enqueued at once but need not START there: behind a lightly loaded phase the next
    update's first launches run 10 - 25 % slower until the device's power management has followed the load
    (profiles/r04_clock_ramp.md).  A gate (tonic_stream_gate: one polling wave) holds the chain back until the row of
    the NEXT rollout from which it just finishes before that rollout does; the host opens it with a plain store.
    Timing only.  TONIC_AMD_CRITIC_GATE=0: the chain starts at once.

    stream, marker     the process's critic stream; the stream that carries "actor and normaliser are final" to the
                       next begin_rollout.  None before the first chain
    done, clock        events behind and in front of the chain in flight; done is None: nothing in flight
    infos, keep        its statistic rows [2, updates, INFO_WIDTH] and the tensors it reads (batch, normaliser and
                       value-range snapshots), alive until it is settled
    chain_ms           device time of the last settled chain (None before)
    gate_word, gate_view   the page-locked word the gate polls, and its NumPy view
    gate_ticket        the value that opens the gate armed last (0 before the first)
    gate_row           the rollout row at which `note_row` opens the gate; None: no gate armed

    launch         clones the snapshots, [several ranks: the normaliser's update first], the side stream behind the
                   current one, [arm_gate], clock, `updates` x [critic grad, critic step], done; the record kept
    arm_gate       gate_row(...) is a row, the gate is not switched off and no ranks exchange: gate_ticket += 1,
                   tonic_stream_gate on the side stream, gate_row = the row, the chain joins the armed ones
    open_gates     every armed chain's ticket stored into its word, gate_row = None (the side stream is shared)
    note_row       a rollout row was stored: open_gates at gate_row
    hand_over      the marker stream ordered behind the current one -> rollout.behind; not gated: the current stream
                   waits for `done`; rollout.started = now
    settle         open_gates; in flight: the current stream behind `done`, the critic's rows read back, chain_ms
                   measured, the record dropped; returns the rows (None: nothing was in flight)
    """

    __slots__ = ('_agent', 'stream', 'marker', 'done', 'clock', 'infos', 'keep', 'chain_ms', 'gate_word', 'gate_view',
                 'gate_ticket', 'gate_row', '__weakref__')

    _armed = weakref.WeakSet()      # chains that wait behind a tonic_stream_gate

    def __init__(self, agent):
        self._agent = weakref.ref(agent)
        self.stream = self.marker = self.done = self.clock = self.infos = self.keep = None
        self.chain_ms = self.gate_word = self.gate_view = self.gate_row = None
        self.gate_ticket = 0

    agent = property(lambda self: self._agent())

    def launch(self, obs, returns, infos, normalizer_first=None):
        """The critic's iterations: same inputs, the normalisers as they are NOW, their own stream.  Returns whether
        this is the agent's first chain (its readers are guarded then)."""
        critic, n, updates = self.agent.critic_updater, obs.shape[0], infos.shape[1]
        snapshot = tuple(t.clone() for t in critic.norm_tensors())
        value_range = critic.range_tensors()
        if value_range is not None:       # (the Return normaliser is refreshed under the chain)
            value_range = tuple(t.clone() for t in value_range)
        if normalizer_first is not None:
            # Several ranks: the normaliser's update is a collective + a read-back on THIS stream; issued
            # after the critic's chain it would queue behind the chain's 80 all-reduces on the
            # communicator (one rank's host blocked for the whole chain).  It depends on neither
            # network (a2c.py:126-127 merges the rollout's recorded sums), the chain reads the snapshot:
            # it goes first.
            normalizer_first.update()
        ready = torch.cuda.Event()
        ready.record()
        first = self.stream is None
        if first:
            self.stream = _side_stream('critic')
        side = self.stream
        side.wait_event(ready)
        clock, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            self.arm_gate(side)
            clock.record(side)
            for it in range(updates):
                critic.enqueue_grad(obs, returns, norm=snapshot, value_range=value_range)
                critic.enqueue_step(n, infos[1, it])
            done.record(side)
        # (Enqueued HERE, while the GPU is busy with the actor's chain and the host has nothing else
        #  to do.  Round 4 also tried it late — from agent.update at the Segment row from which the
        #  chain just finishes before the rollout does, so that the next update's first launches find
        #  the chip at its working clock (profiles/r04_clock_ramp.md): the 160 enqueues then sit on the
        #  host-bound collect loop's critical path, 82.3 against 80.9 ms per step.)
        self.done, self.clock, self.infos = done, clock, infos
        self.keep = (obs, returns, snapshot, value_range)
        return first

    def arm_gate(self, side):
        agent = self.agent
        self.gate_row = None
        if os.environ.get('TONIC_AMD_CRITIC_GATE', '1') == '0':
            return
        if parallel.exchanging():
            # The chain's iterations all-reduce their gradient sums: a collective issued on the main
            # stream meanwhile (the normaliser's statistics) queues BEHIND them on the communicator,
            # and with a host-synchronous backend the first of them blocks the host — the only party
            # that can open a gate.  Ranks that exchange never hold the chain back.
            return
        step_us = agent._rollout.step_us
        row = gate_row(agent.replay.max_size, self.chain_ms, step_us, agent.GATE_MARGIN_MS, agent.GATE_ROLLOUT_US)
        if row is None:
            return
        if self.gate_word is None:
            self.gate_word = torch.zeros(1, dtype=torch.int32).pin_memory()
            self.gate_view = self.gate_word.numpy()
        self.gate_ticket += 1
        # (its own limit: twice the time the host needs to that row — nobody who synchronises the device
        #  without asking the agent first waits longer than that)
        limit = max(0.01, 2.0 * row * step_us * 1e-6 + 0.005)
        _lib.check(_lib.load().tonic_stream_gate(self.gate_word.data_ptr(), self.gate_ticket, limit,
                                                 side.cuda_stream), 'stream gate')
        self.gate_row = row
        CriticChain._armed.add(self)

    @staticmethod
    def open_gates():
        # The critic stream is shared by the agents of a process (_side_stream): whatever another
        # agent has parked there holds THIS agent's chain too, so every armed gate is opened.
        armed = CriticChain._armed
        for chain in list(armed):
            if chain.gate_row is not None:
                chain.gate_view[0] = chain.gate_ticket
                chain.gate_row = None
        armed.clear()

    def note_row(self, index):
        if self.gate_row is not None and index >= self.gate_row:
            self.open_gates()

    def hand_over(self, rollout):
        """What the next rollout depends on — the actor, the normaliser — is on the current stream up to here: a
        stream of its own carries that point to the collector (PolicyBlock -> begin_rollout), which also moves the
        rollout's observations to the spare buffer.  Everything ELSE that follows on the current stream waits for
        the critic's iterations as well — unless they are parked behind a gate: the gate opens late in the next
        rollout, and user work on this stream (a `current_stream().synchronize()` after agent.update) would stall for
        most of a rollout.  Whoever reads the critic is ordered behind the chain by settle()."""
        if self.marker is None:
            self.marker = _side_stream('rollout marker')
        ordered = torch.cuda.Event()
        ordered.record()
        self.marker.wait_event(ordered)
        rollout.behind = self.marker
        if self.gate_row is None:
            torch.cuda.current_stream().wait_event(self.done)
        rollout.started = time.perf_counter()

    def settle(self):
        self.open_gates()
        done, clock, infos, keep = self.done, self.clock, self.infos, self.keep     # (alive until the rows are here)
        if done is None:
            return None
        self.done = self.clock = self.infos = self.keep = None
        torch.cuda.current_stream().wait_event(done)   # whoever reads the critic next is behind it
        rows = infos[1].cpu().numpy()
        self.chain_ms = clock.elapsed_time(done)
        return rows
