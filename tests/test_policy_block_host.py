"""CPU test of the on-policy agents' rollout on the environment's collector block (tonic_amd.policy_block) and of the
gate row of PPO's critic chain (tonic_amd.critic_chain): A2C's own step / update / test_step / close drive the
state machine against a recording stand-in for the Collector, a Segment that only keeps books and real collector
blocks (plain shared memory).  The expected commands and flags were taken from the agent before the state moved
into PolicyBlock: only `world`'s fixture part knows where the state lives."""
import math
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

W, O, A, T = 3, 5, 2, 6


class Books:
    """What the rollout asks of replays.Segment, as bookkeeping."""

    def __init__(self):
        self.max_size, self.index, self.buffers, self.num_workers, self.allocated = T, 0, None, None, []

    def _allocate(self, workers, observation_size, action_size):
        self.num_workers = workers
        self.buffers = dict(observations=torch.zeros(T, workers, observation_size))
        self.allocated.append(workers)

    def ready(self):
        return self.index == self.max_size


class Normalizer:
    device_sums = 'sums'

    def __init__(self):
        self.new_count = 0

    def note_device_rows(self, rows):
        self.new_count += rows


class Recorder:
    """Collector's face; every command lands in `log`.  A command left with the environment (`arm`) is issued by
    `ring`, the environment's side, when `rings` is set."""
    log, rings = None, True

    def __init__(self, block, transport):
        self.block, self.requested, self.transport = block, transport, transport
        self.left, self.issued, self.closed = None, False, False

    @classmethod
    def for_block(cls, block, transport=0):
        if transport not in block._collectors:
            block._collectors[transport] = cls(block, transport)
        return block._collectors[transport]

    def bind_segment(self, buffers, norm_acc, rows):
        self.log.append(('bind_segment', self.block, buffers['observations'].data_ptr(), norm_acc, rows))

    def begin_rollout(self, actor_params, stream=None):
        self.log.append(('begin_rollout', self.block, actor_params, stream))

    def ppo_step(self, row, slot, store_previous, by='agent'):
        assert not self.closed
        self.log.append(('ppo_step', self.block, row, slot, bool(store_previous), by))
        self.block.actions[:] = row + 1

    def arm(self, row, slot, store_previous):
        self.left, self.issued = (row, slot, store_previous), False
        self.log.append(('arm', self.block, row, slot, bool(store_previous)))
        return True

    def ring(self):
        if self.left is not None and self.rings:
            self.ppo_step(*self.left, by='environment')
            self.left, self.issued = None, True

    def claim(self):
        issued, self.left, self.issued = self.issued, None, False
        self.log.append(('claim', self.block, issued))
        return issued

    def wait_actions(self):
        self.log.append(('wait_actions', self.block))

    def end_rollout(self, last_row):
        self.log.append(('end_rollout', self.block, last_row))

    def close(self):
        self.closed = True
        self.log.append(('close', self.block))


@pytest.fixture
def world(monkeypatch):
    from tonic_amd import policy_block
    from tonic_amd.collector import Block
    from tonic_amd.torch import agents
    log = Recorder.log = []
    Recorder.rings = True
    for name in ('TONIC_AMD_SPECULATE', 'TONIC_AMD_ARM', 'TONIC_AMD_WIDE_STAGED'):
        monkeypatch.delenv(name, raising=False)

    class Agent(agents.A2C):
        def _update(self):
            log.append(('update', self.replay.index))
            self.replay.index = 0

        def _io(self, workers):
            return 'in', 'out'

        def _act(self, observations, stage_in, stage_out, want_log_probs):       # (test episodes: the staged path)
            assert (stage_in, stage_out, want_log_probs) == ('in', 'out', False)
            self.test_draws.append(torch.randn(observations.shape[0], A))
            return np.zeros((observations.shape[0], A), np.float32)

    # ---- the fixture part: where the collector is patched in and where the state lives --------------------------
    monkeypatch.setattr(policy_block, 'Collector', Recorder)

    def agent():
        agent = Agent(model=types.SimpleNamespace(observation_normalizer=Normalizer(), return_normalizer=None,
                                                  flat_actor=types.SimpleNamespace(flat='actor')),
                      replay=Books(), actor_updater=types.SimpleNamespace(stock=False, torso=None), critic_updater=1)
        agent.observation_size, agent.action_size, agent.test_draws = O, A, []
        agent.global_noise, agent._acting_generator = False, None
        agent._staged_workers = agent._test_workers = agent._act_workspace = None
        # (what A2C.initialize leaves, less the device)
        agent._rollout = policy_block.PolicyBlock(agent, 3)
        return agent

    def flags(agent):
        r = agent._rollout
        return r.slot, r.eps_ahead, r.pending, r.rollout_open, r.speculated, r.armed, r.fed

    def unbound(agent):
        r = agent._rollout
        return (r.collector is None and r.block is None and r.behind is None
                and flags(agent) == (0, False, False, False, False, False, False))

    def bound(agent):
        return agent._rollout.block, agent._rollout.collector

    def set_behind(agent, stream):
        agent._rollout.behind = stream

    def spare(agent):
        return agent._rollout.spare_observations
    # --------------------------------------------------------------------------------------------------------------

    def take():
        events = list(log)
        del log[:]
        return events
    return types.SimpleNamespace(agent=agent, flags=flags, unbound=unbound, bound=bound, set_behind=set_behind,
                                 spare=spare, take=take, S=Block(W, O, A), S2=Block(W, O, A))


def fed_step(world, agent, block):
    """agent.step on the block's own arrays -> the environment (completes its record and rings) -> the outcome."""
    actions = agent.step(block.out_observations, 0)
    assert actions is block.out_actions
    collector = world.bound(agent)[1]
    return actions, collector.ring, lambda: agent.update(**block.infos, steps=0)


def foreign_step(agent, block, workers=W):
    observations = np.full((workers, O), 0.5, np.float32)
    actions = agent.step(observations, 0)
    infos = dict(observations=np.full((workers, O), 0.25, np.float32), rewards=np.full(workers, 2.0, np.float32),
                 resets=np.array([True] + [False] * (workers - 1)), terminations=np.zeros(workers, bool))
    return observations, actions, infos


def fed_rollout(world, agent, block, rows=T):
    for _ in range(rows):
        _, ring, update = fed_step(world, agent, block)
        ring()
        update()


def commands(events, *kinds):
    return [e for e in events if e[0] in kinds]


def test_first_step_on_foreign_arrays_copies_in_and_hands_out_a_fresh_array(world):
    agent = world.agent()
    observations, actions, infos = foreign_step(agent, None)
    P, collector = world.bound(agent)
    assert P is not world.S and P is not world.S2 and P.workers == W and agent.replay.allocated == [W]
    assert agent.transport_in_effect == 3 and isinstance(collector, Recorder)
    pointer = agent.replay.buffers['observations'].data_ptr()
    assert world.take() == [('bind_segment', P, pointer, 'sums', T), ('begin_rollout', P, 'actor', None),
                            ('ppo_step', P, 0, 0, False, 'agent'), ('wait_actions', P)]
    np.testing.assert_array_equal(P.observations, observations)
    assert actions is not P.out_actions and actions is not P.actions and actions.flags.writeable
    np.testing.assert_array_equal(actions, np.full((W, A), 1, np.float32))
    assert agent.last_observations is observations and agent.last_actions is actions
    assert world.flags(agent) == (1, True, False, True, False, False, False)
    agent.update(**infos, steps=0)
    assert world.take() == [] and world.flags(agent) == (1, True, True, True, False, False, False)
    np.testing.assert_array_equal(P.next_observations, infos['observations'])
    np.testing.assert_array_equal(P.rewards, infos['rewards'])
    np.testing.assert_array_equal(P.resets, [1, 0, 0])
    np.testing.assert_array_equal(P.terminations, [0, 0, 0])
    assert agent.replay.index == 1 and agent.model.observation_normalizer.new_count == W
    # the outcome rides in the next step's command
    _, actions, infos = foreign_step(agent, None)
    assert world.take() == [('ppo_step', P, 1, 1, True, 'agent'), ('wait_actions', P)]
    assert world.flags(agent) == (0, True, False, True, False, False, False)
    np.testing.assert_array_equal(actions, np.full((W, A), 2, np.float32))


@pytest.mark.parametrize('mode', ['rung', 'not_rung', 'no_arm', 'no_speculation'])
def test_block_fed_rollout(world, monkeypatch, mode):
    """A whole rollout on the block's own arrays and the first step of the next: the steady state and its general
    form at the rollout's two ends.  The commands are the same whoever issues them."""
    if mode == 'no_arm':
        monkeypatch.setenv('TONIC_AMD_ARM', '0')
    if mode == 'no_speculation':
        monkeypatch.setenv('TONIC_AMD_SPECULATE', '0')
    Recorder.rings = mode == 'rung'
    agent, S = world.agent(), world.S
    arms, speculates = mode in ('rung', 'not_rung'), mode != 'no_speculation'
    issued, slot = [], 0
    for row in range(T):
        _, ring, update = fed_step(world, agent, S)
        events = world.take()
        issued += commands(events, 'ppo_step')
        armed = arms and 1 <= row and row + 2 < T
        ahead = speculates and row >= 1                 # update() issued this row already
        want = []
        if row == 0:
            want += [('bind_segment', S, agent.replay.buffers['observations'].data_ptr(), 'sums', T),
                     ('begin_rollout', S, 'actor', None)]
        if not ahead:
            want += [('ppo_step', S, row, slot, row > 0, 'agent')]
        if armed:
            want += [('arm', S, row + 1, slot ^ 1, True)]
        assert events == want + [('wait_actions', S)], row
        slot ^= 1
        assert world.flags(agent) == (slot, True, False, True, False, armed, True), row
        assert agent.last_observations is S.out_observations and agent.last_actions is S.out_actions
        ring()
        issued += commands(world.take(), 'ppo_step')
        update()
        events = world.take()
        issued += commands(events, 'ppo_step')
        next_issued = speculates and row + 2 <= T
        want = []
        if armed:
            want += [('claim', S, mode == 'rung')]
        if next_issued and not (armed and mode == 'rung'):
            want += [('ppo_step', S, row + 1, slot, True, 'agent')]
        if row == T - 1:
            want += [('end_rollout', S, T - 1), ('update', T)]
            assert world.flags(agent) == (slot, True, False, False, False, False, True)
        else:
            assert world.flags(agent) == (slot, True, not next_issued, True, next_issued, False, True), row
        assert events == want, row
    assert [e[:5] for e in issued] == [('ppo_step', S, row, row % 2, row > 0) for row in range(T)]
    assert [e[5] for e in issued].count('environment') == (3 if mode == 'rung' else 0)
    assert agent.steps_issued_by_environment == (3 if mode == 'rung' else 0)
    assert agent.model.observation_normalizer.new_count == T * W and agent.replay.index == 0
    # the next rollout opens with the noise drawn ahead and nothing to store
    fed_step(world, agent, S)
    assert world.take() == [('bind_segment', S, agent.replay.buffers['observations'].data_ptr(), 'sums', T),
                            ('begin_rollout', S, 'actor', None), ('ppo_step', S, 0, slot, False, 'agent'),
                            ('wait_actions', S)]
    assert world.flags(agent) == (slot ^ 1, True, False, True, False, False, True)


def test_foreign_observations_in_a_block_fed_rollout_issue_the_step_again(world):
    agent, S = world.agent(), world.S
    fed_rollout(world, agent, S, 1)
    assert world.flags(agent) == (1, True, False, True, True, False, True)        # row 1 is in flight
    world.take()
    observations, actions, infos = foreign_step(agent, S)
    # the step issued early is waited out (it read the block's old rows) and issued again: its outcome went along
    # with the first issue
    assert world.take() == [('wait_actions', S), ('ppo_step', S, 1, 1, False, 'agent'), ('wait_actions', S)]
    np.testing.assert_array_equal(S.observations, observations)
    assert actions is not S.out_actions and world.flags(agent) == (0, True, False, True, False, False, False)
    agent.update(**infos, steps=0)
    assert world.take() == [] and world.flags(agent) == (0, True, True, True, False, False, False)
    # back on the block's arrays: the general step, then the steady state again
    _, ring, update = fed_step(world, agent, S)
    assert world.take() == [('ppo_step', S, 2, 0, True, 'agent'), ('wait_actions', S)]
    update()
    assert world.take() == [('ppo_step', S, 3, 1, True, 'agent')]
    assert world.flags(agent) == (1, True, False, True, True, False, True)


@pytest.mark.parametrize('rung', [True, False])
def test_a_foreign_outcome_takes_back_the_command_left_with_the_environment(world, rung):
    Recorder.rings = rung
    agent, S = world.agent(), world.S
    fed_rollout(world, agent, S, 1)
    _, ring, _ = fed_step(world, agent, S)
    assert world.flags(agent) == (0, True, False, True, False, True, True)
    ring()
    world.take()
    infos = {k: v.copy() for k, v in S.infos.items()}
    agent.update(**infos, steps=0)
    # (a step the environment issued reads the block: the outcome is not copied in under it)
    assert world.take() == [('claim', S, rung)] + ([('wait_actions', S)] if rung else [])
    assert world.flags(agent) == (0, True, True, True, False, False, True) and agent.replay.index == 2
    assert agent.steps_issued_by_environment == 0


def test_a_test_episode_between_update_and_step_keeps_the_noise_order(world):
    agent, S = world.agent(), world.S
    torch.manual_seed(11)
    want = [torch.randn(W, A).numpy() for _ in range(5)]
    torch.manual_seed(11)
    fed_rollout(world, agent, S, 1)
    np.testing.assert_array_equal(S.eps[0], want[0])
    np.testing.assert_array_equal(S.eps[1], want[1])           # drawn ahead for row 1, which is in flight
    world.take()
    agent.test_step(np.zeros((W, O), np.float32), 0)
    assert world.take() == [('wait_actions', S)]
    assert world.flags(agent) == (1, False, False, True, False, False, True)
    np.testing.assert_array_equal(agent.test_draws[0].numpy(), want[1])      # the test episode's draw comes first
    agent.test_step(np.zeros((W, O), np.float32), 0)
    assert world.take() == []
    np.testing.assert_array_equal(agent.test_draws[1].numpy(), want[2])
    fed_step(world, agent, S)
    assert world.take() == [('ppo_step', S, 1, 1, False, 'agent'), ('wait_actions', S)]
    assert world.flags(agent) == (0, True, False, True, False, False, True)
    np.testing.assert_array_equal(S.eps[1], want[3])           # a fresh draw for row 1
    np.testing.assert_array_equal(S.eps[0], want[4])           # ... and row 2's ahead of it


def test_the_last_rows_of_a_rollout_do_not_speculate_past_it(world):
    agent, S = world.agent(), world.S
    called = []
    agent._update = lambda: (called.append(agent.replay.index), setattr(agent.replay, 'index', 0))
    fed_rollout(world, agent, S, T - 2)
    world.take()
    _, ring, update = fed_step(world, agent, S)                 # row T - 2, issued by the update before
    assert world.take() == [('wait_actions', S)]
    update()
    assert world.take() == [('ppo_step', S, T - 1, 1, True, 'agent')]
    assert world.flags(agent) == (1, True, False, True, True, False, True)
    _, ring, update = fed_step(world, agent, S)                 # row T - 1
    assert world.take() == [('wait_actions', S)]
    update()
    assert world.take() == [('end_rollout', S, T - 1)] and called == [T]      # (_update through the instance)
    assert world.flags(agent) == (0, True, False, False, False, False, True)


def test_another_environments_block_is_adopted_between_rollouts_with_the_noise_ahead(world):
    agent, S, S2 = world.agent(), world.S, world.S2
    torch.manual_seed(5)
    want = [torch.randn(W, A).numpy() for _ in range(T + 3)]
    torch.manual_seed(5)
    fed_rollout(world, agent, S)
    np.testing.assert_array_equal(S.eps[0], want[T])           # row 0 of the next rollout, drawn ahead
    assert world.flags(agent) == (0, True, False, False, False, False, True)
    world.take()
    old = world.bound(agent)[1]
    fed_step(world, agent, S2)
    assert world.bound(agent) == (S2, S2._collectors[3]) and world.bound(agent)[1] is not old
    assert world.take() == [('bind_segment', S2, agent.replay.buffers['observations'].data_ptr(), 'sums', T),
                            ('begin_rollout', S2, 'actor', None), ('ppo_step', S2, 0, 0, False, 'agent'),
                            ('wait_actions', S2)]
    np.testing.assert_array_equal(S2.eps[0], want[T])
    np.testing.assert_array_equal(S2.eps[1], want[T + 1])
    assert world.flags(agent) == (1, True, False, True, False, False, True)
    assert agent.replay.allocated == [W] and agent.steps_issued_by_environment == 0
    # in the middle of a rollout another block's arrays are foreign ones: copied in
    agent.update(**S2.infos, steps=0)
    world.take()
    actions = agent.step(S.out_observations, 0)
    assert world.bound(agent)[0] is S2 and actions is not S2.out_actions
    assert world.take() == [('wait_actions', S2), ('ppo_step', S2, 1, 1, False, 'agent'), ('wait_actions', S2)]


def test_a_new_worker_count_binds_anew(world):
    agent, S = world.agent(), world.S
    fed_rollout(world, agent, S)
    world.take()
    _, actions, infos = foreign_step(agent, None, workers=4)
    P = world.bound(agent)[0]
    assert P is not S and P.workers == 4 and agent.replay.allocated == [W, 4] and actions.shape == (4, A)
    assert world.take() == [('bind_segment', P, agent.replay.buffers['observations'].data_ptr(), 'sums', T),
                            ('begin_rollout', P, 'actor', None), ('ppo_step', P, 0, 0, False, 'agent'),
                            ('wait_actions', P)]
    assert world.flags(agent) == (1, True, False, True, False, False, False)


def test_the_update_orders_the_next_rollout_behind_a_stream_once(world):
    agent, S = world.agent(), world.S
    fed_rollout(world, agent, S)
    world.take()
    first = agent.replay.buffers['observations']
    world.set_behind(agent, types.SimpleNamespace(cuda_stream=77))
    fed_step(world, agent, S)
    second = agent.replay.buffers['observations']
    assert second is not first and second.shape == first.shape and world.spare(agent) is first
    assert world.take()[:2] == [('bind_segment', S, second.data_ptr(), 'sums', T), ('begin_rollout', S, 'actor', 77)]
    agent.update(**S.infos, steps=0)
    fed_rollout(world, agent, S, T - 1)
    world.take()
    fed_step(world, agent, S)                    # no stream left behind: the current one, the buffers as they are
    assert world.take()[:2] == [('bind_segment', S, second.data_ptr(), 'sums', T), ('begin_rollout', S, 'actor', None)]
    assert agent.replay.buffers['observations'] is second and world.spare(agent) is first
    agent.update(**S.infos, steps=0)
    fed_rollout(world, agent, S, T - 1)
    world.take()
    world.set_behind(agent, types.SimpleNamespace(cuda_stream=78))       # the two buffers take turns
    fed_step(world, agent, S)
    assert world.take()[:2] == [('bind_segment', S, first.data_ptr(), 'sums', T), ('begin_rollout', S, 'actor', 78)]
    assert agent.replay.buffers['observations'] is first and world.spare(agent) is second


def test_close_waits_out_the_step_in_flight_and_gives_the_noise_back(world):
    agent, S = world.agent(), world.S
    agent.close()                                # nothing bound: nothing to do
    assert world.take() == [] and world.unbound(agent)
    torch.manual_seed(3)
    want = [torch.randn(W, A).numpy() for _ in range(3)]
    torch.manual_seed(3)
    fed_rollout(world, agent, S, 1)
    _, ring, _ = fed_step(world, agent, S)       # row 1 collected, row 2 left with the environment
    ring()
    assert world.flags(agent) == (0, True, False, True, False, True, True)
    world.take()
    agent.close()
    assert world.take() == [('claim', S, True), ('wait_actions', S), ('close', S)]
    assert world.unbound(agent) and S._collectors == {}
    state = torch.get_rng_state()
    np.testing.assert_array_equal(torch.randn(W, A).numpy(), want[2])       # the draw made ahead is the next one
    torch.set_rng_state(state)
    agent.close()
    assert world.take() == []
    # bound again from scratch by the next step
    agent.replay.index = 0
    fed_step(world, agent, S)
    assert world.bound(agent)[0] is S and world.bound(agent)[1] is not None
    assert world.take() == [('bind_segment', S, agent.replay.buffers['observations'].data_ptr(), 'sums', T),
                            ('begin_rollout', S, 'actor', None), ('ppo_step', S, 0, 0, False, 'agent'),
                            ('wait_actions', S)]
    assert world.flags(agent) == (1, True, False, True, False, False, True)
    assert agent.steps_issued_by_environment == 0
    np.testing.assert_array_equal(S.eps[0], want[2])


# ---------------------------------------------------------------------------------------------- the gate's row
def parent_gate_row(rows, chain_ms, step_us, margin_ms=1.0, rollout_us=100e3):
    """PPO._arm_gate's arithmetic as it stood before it became a function."""
    if not chain_ms or not step_us:
        return None
    row = rows - int(np.ceil((1.1 * chain_ms + margin_ms) * 1e3 / step_us))
    if row <= 0 or rows * step_us > rollout_us:
        return None
    return row


GATE_CASES = [
    # rows, chain_ms, step_us
    (1024, None, 10.3), (1024, 0.0, 10.3), (1024, 15.4, None), (1024, 15.4, 0.0),       # nothing measured yet
    (1024, 15.4, 70.7), (1024, 22.7, 80.9), (2048, 18.5, 12.9), (64, 0.31, 31.7), (1024, 15.4, 40.3),     # armed
    (1024, 15.4, 10.3), (1024, 95.3, 70.7), (16, 15.4, 70.7),                           # the chain needs the rollout
    (1024, 15.4, 105.3), (4096, 15.4, 30.3),                                            # a rollout beyond the ramp
]


@pytest.mark.parametrize('rows,chain_ms,step_us', GATE_CASES)
def test_gate_row_is_the_parents_expression(rows, chain_ms, step_us):
    from tonic_amd.critic_chain import gate_row
    if chain_ms and step_us:          # (no quotient near an integer: ceil cannot flip on a rounding)
        quotient = (1.1 * chain_ms + 1.0) * 1e3 / step_us
        assert abs(quotient - round(quotient)) > 1e-9
    want = parent_gate_row(rows, chain_ms, step_us)
    assert gate_row(rows, chain_ms, step_us, 1.0, 100e3) == want
    assert want is None or 0 < want < rows


def test_gate_row_reaches_every_branch():
    wants = [parent_gate_row(*case) for case in GATE_CASES]
    assert wants == [None] * 4 + [770, 702, 392, 21, 578] + [None] * 5
    assert wants[4] == 1024 - math.ceil(17940 / 70.7)
