"""The on-policy agents' rollout on the environment's collector block (``tonic_collector_ppo_step``, DESIGN.md §4.2 /
§4.3): ``PolicyBlock`` is the state of one agent (A2C / PPO / TRPO) on one block."""
import os
import time
import weakref

import numpy as np
import torch

from tonic_amd.collector import Block, Collector


class PolicyBlock:
    """One agent on one block.  Per environment step ONE command (policy forward + sample + log-prob of the block's
    observations, Segment row store, normaliser record, the deferred store of the step before's outcome) reads the
    block in place and writes the actions back into it; the host waits on a completion word and draws the next step's
    noise meanwhile.  A loop that hands over the block's own arrays ("block-fed") gets the next step's command issued
    from `update`, or from the environment itself, before the trainer's loop comes back to `step`.

    block, collector   the block bound to (the environment's, or a private one foreign arrays are copied into) and its
                       GPU handle; None: unbound
    noise              the draws of the steps ahead (agent._draws_ahead), kept over a re-bind of the same shape
    slot               the noise slot the next command reads
    eps_ahead          that slot already holds the next step's draws
    pending            the last outcome lies in the block and no command has carried it into the Segment yet: the
                       `store_previous` of the next ppo_step
    rollout_open       begin_rollout was issued and end_rollout was not
    speculated         a command for row replay.index is in flight and no step() has collected it
    armed              a command was left with the environment (Collector.arm)
    fed                the last step() was handed the block's own arrays
    speculate, arm_steps   TONIC_AMD_SPECULATE / TONIC_AMD_ARM as they stood when the block was bound
    behind             the stream the next begin_rollout is ordered behind (CriticChain.hand_over), taken once; with
                       it the rollout's observations go to `spare_observations`, swapped with the Segment's buffer
    host_rollout       the update that is running follows a rollout that came through this collector
    started, step_us   when the update before let the rollout start; host microseconds per row of the last rollout
    issued_by_environment   steps whose command the environment issued (agent.steps_issued_by_environment)
    chain              the agent's CriticChain (PPO) or None: `update` opens its gate at the gate's row

    Legal combinations: speculated and armed exclude each other, and either needs rollout_open; armed needs fed and
    eps_ahead; pending and speculated exclude each other (the command in flight carries the outcome); unbound, every
    flag is False.

    bind           (first step, new worker count) the block the observations are a view of, or a private one; its
                   collector; the Segment allocated for W workers; every flag False, slot 0
    adopt          (step, replay.index == 0, rollout not open, the observations are ANOTHER live block's) settle, bind;
                   the draws made ahead move into the new block's slot, eps_ahead stays
    step_ahead     the steady state: speculated, eps_ahead, the block's own observations.  speculated = False; draws
                   into slot ^ 1, slot ^= 1; arm(index + 1, slot, True) while index + 2 < max_size -> armed;
                   wait_actions; fed = True.  Anything else: None
    step           claim; bind / adopt; foreign observations copied in; a speculated command is kept (fed, eps_ahead) or
                   waited out.  Not kept: [rollout not open: bind_segment, begin_rollout(behind), rollout_open = True]
                   [not eps_ahead: draws into slot] ppo_step(index, slot, pending), pending = False.  Then draws into
                   slot ^ 1, slot ^= 1, eps_ahead = True; wait_actions; fed = the block's own arrays
    update_ahead   the steady state: fed, the block's own outcome arrays, eps_ahead, speculate, index + 2 < max_size.
                   armed: claim (True: the environment issued it) else ppo_step(index + 1, slot, True); speculated =
                   True, armed = pending = False, index += 1, the gate opened at its row.  Anything else: False
    update         claim.  Block-fed: ppo_step(index + 1, slot, True) if eps_ahead, speculate, index + 2 <= max_size
                   and nothing in flight -> speculated.  Else settle, the outcome copied in.  index += 1, the gate,
                   pending = not speculated.  Segment full: end_rollout(index - 1), pending = rollout_open = False,
                   agent._update() with host_rollout set
    claim          armed = False; the environment had issued the command: speculated = True
    settle         claim; speculated: wait_actions, speculated = False
    rewind         (a test episode draws from the generator) settle; the generator back behind the executed steps'
                   draws, eps_ahead = False
    close          settle; generator back, noise helper ended; the collector destroyed; unbound
    """

    __slots__ = ('_agent', 'replay', 'model', 'transport', 'transport_in_effect', 'speculate', 'arm_steps', 'block', 'collector',
                 'chain', 'noise', 'slot', 'eps_ahead', 'pending', 'rollout_open', 'speculated', 'armed', 'fed',
                 'behind', 'spare_observations', 'host_rollout', 'started', 'step_us', 'issued_by_environment')

    def __init__(self, agent, transport):
        self._agent = weakref.ref(agent)      # (weak: the agent goes when its last user lets go, not at a collection)
        self.noise = self.spare_observations = self.started = self.step_us = None
        self.reset(transport)

    def reset(self, transport):
        """agent.initialize: unbound (a collector that was not closed stays with its block)."""
        agent = self.agent
        self.replay, self.model, self.transport, self.host_rollout, self.behind = \
            agent.replay, agent.model, transport, False, None
        self._unbound()

    agent = property(lambda self: self._agent())

    def _unbound(self):
        self.block = self.collector = self.chain = None
        self.slot, self.issued_by_environment = 0, 0
        self.eps_ahead = self.pending = self.rollout_open = self.speculated = self.armed = self.fed = False
        self.speculate = self.arm_steps = False

    # ------------------------------------------------------------------ transitions
    def bind(self, observations):
        """First step (or a new worker count): find the environment's block — the arrays of
        tonic_amd.environments ARE views of one — or make a private one, page-lock it and point
        the collector at the Segment."""
        agent, replay = self.agent, self.replay
        W, O, A = observations.shape[0], agent.observation_size, agent.action_size
        self._unbound()
        self.block = block = Block.owner_of(observations) or Block(W, O, A)
        self.collector = Collector.for_block(block, self.transport)
        self.transport_in_effect = self.collector.transport
        self.chain = agent._chain
        if replay.buffers is None or replay.num_workers != W:
            replay._allocate(W, O, A)
        noise = self.noise
        if noise is None or (noise.workers, noise.width) != (W, A):
            if noise is not None:
                noise.rewind(0)
            self.noise = agent._draws_ahead(W, A)
        # update() may issue the NEXT step's launch itself (see there), and step() may leave the one after with
        # the environment (Block.ring issues it)
        self.speculate = os.environ.get('TONIC_AMD_SPECULATE', '1') != '0'
        self.arm_steps = self.speculate and os.environ.get('TONIC_AMD_ARM', '1') != '0'

    def step_ahead(self, observations):
        # The steady state of a block-fed loop (every attribute lookup of this call is host time between the
        # simulator's step and the next command to the GPU): update() has issued this step with the block's own
        # observations and the noise drawn ahead.
        if not (self.speculated and self.eps_ahead and observations is self.block.out_observations):
            return None
        block, slot = self.block, self.slot
        self.speculated = False
        self.noise.take(block.eps[slot ^ 1])      # the step after this one
        self.slot = slot ^ 1
        # ... whose command is left with the ENVIRONMENT: it issues it the moment its step
        # record is complete (Block.ring), update() only confirms (see there)
        replay = self.replay
        if self.arm_steps and replay.index + 2 < replay.max_size:
            self.armed = self.collector.arm(replay.index + 1, slot ^ 1, True)
        self.collector.wait_actions()
        self.fed = True
        return block.out_actions

    def step(self, observations):
        self.claim()
        block = self.block
        if self.collector is None or block.workers != len(observations):
            self.settle()
            self.bind(observations)
            block = self.block
        fed = observations is block.out_observations or observations is block.observations
        if not fed and self.replay.index == 0 and not self.rollout_open:
            # between two rollouts: another environment of tonic_amd.environments took over (its
            # observations are the view of ANOTHER live block) -> adopt that block, stay zero-copy
            owner = Block.owner_of(observations)
            if owner is not None and owner is not block:
                self.settle()
                ahead = self.eps_ahead and block.eps[self.slot].copy()
                self.bind(observations)
                block, fed = self.block, True
                if ahead is not False:        # the noise drawn ahead moves along (same stream)
                    np.copyto(block.eps[self.slot], ahead)
                    self.eps_ahead = True
        if not fed:
            np.copyto(block.observations, observations)
        collector = self.collector
        launched = False
        if self.speculated:
            # update() already issued this step with the block's contents and the noise drawn
            # ahead.  Still what the reference would compute?  (Other observations, or a test
            # episode in between whose draws come first in the generator's order: no.)
            self.speculated = False
            if fed and self.eps_ahead:
                launched = True
            else:
                collector.wait_actions()          # discard; a step is idempotent (collector.hip)
        if not launched:
            if not self.rollout_open:
                self._begin_rollout()
            if not self.eps_ahead:
                self.noise.take(block.eps[self.slot])                                # a2c.py:81
            collector.ppo_step(self.replay.index, self.slot, self.pending)
            self.pending = False
        slot = self.slot
        # The next step's noise goes into the other slot while the GPU works on this one (drawn
        # ahead by _NoiseAhead; a test episode rewinds the generator: its own draws come first in the
        # reference's stream order).
        self.noise.take(block.eps[slot ^ 1])
        self.slot, self.eps_ahead = slot ^ 1, True
        collector.wait_actions()
        self.fed = fed
        # An environment that lives in the block consumes the actions at once (and may take them
        # from the block itself): it gets the block's read-only view; anybody else a fresh array.
        return block.out_actions if fed else block.actions.copy()

    def _begin_rollout(self):
        replay, norm = self.replay, self.model.observation_normalizer
        behind = None
        if self.behind is not None:
            # the update left the critic's iterations running (CriticChain): this rollout writes its
            # observations to the spare buffer and is ordered behind what it depends on
            # (the actor, the normaliser) — the current stream waits for the critic as well
            behind, self.behind = self.behind.cuda_stream, None
            buffers = replay.buffers
            spare = self.spare_observations
            if spare is None or spare.shape != buffers['observations'].shape:
                spare = torch.empty_like(buffers['observations'])
            self.spare_observations, buffers['observations'] = buffers['observations'], spare
        self.collector.bind_segment(replay.buffers, norm.device_sums if norm is not None else None, replay.max_size)
        self.collector.begin_rollout(self.model.flat_actor.flat, behind)
        self.rollout_open = True

    def _own_outcome(self, observations, rewards, resets, terminations):
        # (identity: the arrays tonic_amd.environments hand out ARE the block's fields)
        block = self.block
        return (self.fed and observations is block.out_next_observations and rewards is block.out_rewards
                and resets is block.out_resets and terminations is block.out_terminations)

    def update_ahead(self, observations, rewards, resets, terminations):
        block, replay = self.block, self.replay
        if not (self.fed and observations is block.out_next_observations
                and rewards is block.out_rewards and resets is block.out_resets
                and terminations is block.out_terminations and self.eps_ahead and self.speculate
                and replay.index + 2 < replay.max_size):
            return False
        # the steady state of a block-fed loop (the general form is `update`): the next step's
        # command goes out first, the bookkeeping runs while the GPU works
        index = replay.index
        if self.armed:
            # step() left this command with the environment, which normally has issued it
            # from inside its own step call, before the trainer's loop even got here
            self.armed = False
            if self.collector.claim():
                self.issued_by_environment += 1
            else:
                self.collector.ppo_step(index + 1, self.slot, True)
        else:
            self.collector.ppo_step(index + 1, self.slot, True)
        self.speculated = True
        replay.index = index + 1
        chain = self.chain
        if chain is not None:
            gate = chain.gate_row
            if gate is not None and index >= gate:
                chain.open_gates()
        normalizer = self.model.observation_normalizer
        if normalizer:
            normalizer.new_count += block.workers             # (note_device_rows)
        self.pending = False
        return True

    def update(self, observations, rewards, resets, terminations):
        """a2c.py:58-73.  The outcome stays in the block; the NEXT step's launch (or
        end_rollout) moves it into the Segment row of the step it belongs to."""
        block, replay = self.block, self.replay
        self.claim()
        if self._own_outcome(observations, rewards, resets, terminations):
            # The environment lives in the block: the outcome is in place and so are the next
            # step's observations (distributed.py:136-155 returns them with these infos).  With
            # its noise drawn ahead, the next step's launch goes out FIRST — the rest of this call,
            # the trainer's bookkeeping and the head of the next agent.step run while the GPU
            # works.  step() issues it again if it turns out to be obsolete.
            if (self.eps_ahead and self.speculate and replay.index + 2 <= replay.max_size
                    and not self.speculated):
                self.collector.ppo_step(replay.index + 1, self.slot, True)
                self.speculated = True
        else:
            self.settle()      # (a step the environment issued reads the block: not under it)
            if (observations is not block.out_next_observations
                    and observations is not block.next_observations):
                np.copyto(block.next_observations, observations)
            if rewards is not block.out_rewards and rewards is not block.rewards:
                np.copyto(block.rewards, rewards)
            if resets is not block.out_resets and resets is not block.resets_bool:
                np.copyto(block.resets, resets)             # bool -> float32 (segments.py:33)
            if terminations is not block.out_terminations and \
                    terminations is not block.terminations_bool:
                np.copyto(block.terminations, terminations)
        replay.index += 1
        if self.chain is not None:
            self.chain.note_row(replay.index - 1)
        normalizer = self.model.observation_normalizer
        if normalizer:
            normalizer.note_device_rows(block.workers)
        self.pending = not self.speculated
        if replay.ready():
            self._end_rollout()

    def _end_rollout(self):
        replay = self.replay
        if self.started is not None:          # host time per environment step of the rollout that ends here
            self.step_us = (time.perf_counter() - self.started) * 1e6 / replay.max_size
        self.collector.end_rollout(replay.index - 1)
        self.pending, self.rollout_open = False, False
        # (this rollout came through the collector, which binds the Segment's buffers anew at
        #  every rollout: the update may swap them — see CriticChain)
        self.host_rollout = True
        try:
            self.agent._update()           # (through the instance: probes and the benchmark wrap it there)
        finally:
            self.host_rollout = False

    def claim(self):
        """Takes back a command that step() left with the environment: issued meanwhile = a step
        in flight like one update() issued early; not issued = withdrawn."""
        if self.armed:
            self.armed = False
            if self.collector.claim():
                self.speculated = True

    def settle(self):
        """Waits out a step that update() issued early and nobody asked for yet (the Segment row it
        wrote lies beyond the rows stored so far and is rewritten by the real step)."""
        self.claim()
        if self.speculated:
            self.collector.wait_actions()
            self.speculated = False

    def rewind(self):
        """A test episode draws from the same generator (a2c.py:87-90): its draws come first."""
        if self.noise is not None:
            self.settle()          # (a step issued ahead reads the slot: let it finish first)
            self.noise.rewind(1 if self.eps_ahead else 0)
            self.eps_ahead = False

    def close(self):
        """Waits out a step issued ahead, puts the generator back where the reference's stream is, ends the noise
        helper thread and destroys the collector (its stream, its resident kernel, the page-lock on the
        environment's block)."""
        if self.collector is None:
            return
        self.settle()
        if self.noise is not None:
            self.noise.rewind(1 if self.eps_ahead else 0)
            self.noise.close()
            self.noise = None
        self.collector.close()
        self.block._collectors.pop(self.collector.requested, None)
        self.behind = None
        self._unbound()
