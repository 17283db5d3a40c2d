"""CPU test of the off-policy agents' update scheduler (tonic_amd.q_update).  The plain functions against tables
written by hand; then the agents' own enqueue_update / _update / _fused_kind / _fused_in_phases / _update_chunk
with the library, the updaters' entries and the graph capture replaced by recorders, tensors on the CPU and a
stand-in Buffer: which launches go out, in which order, with which tonic_q_iteration_t fields."""
import contextlib
import ctypes
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

O, A, B, H = 5, 2, 4, 32
F, T = False, True


# ---------------------------------------------------------------------------------------------- the plain functions
def test_ride_plan_tables():
    from tonic_amd.q_update import ride_plan
    always = lambda it: 1                                                       # noqa: E731
    assert ride_plan([F, T, F, T], always) == [(0, 0, T), (2, 1, F), (0, 1, T), (2, 0, F)]
    assert ride_plan([F, F, T, F, F, T], always) == [(0, 0, T), (2, 1, T), (2, 0, F), (0, 0, T), (2, 1, T), (2, 0, F)]
    assert ride_plan([T, T, T], always) == [(0, 0, F)] * 3
    assert ride_plan([T, F], always) == [(0, 0, F), (0, 0, F)]                  # nothing behind the last to ride
    assert ride_plan([F, F], always) == [(0, 0, T), (2, 1, F)]
    asked = []
    refuses_2 = lambda it: asked.append(it) or it != 2                          # noqa: E731
    assert ride_plan([F, T, F, T], refuses_2) == [(0, 0, T), (2, 1, F), (0, 1, F), (0, 1, F)]
    assert asked == [0, 2]                     # only where an iteration that does not step the actor has a successor
    assert ride_plan([], always) == []


def test_adam_table_follows_a_td3_schedule():
    from tonic_amd.q_update import adam_table
    from tonic_amd.torch.updaters import adam_step_constants
    critic = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    actor = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-8)
    table, critic_steps, actor_steps = adam_table(4, [F, T, F, T], critic, actor, 7, 3)
    assert table.shape == (4, 2, 2) and table.dtype == np.float32 and (critic_steps, actor_steps) == (11, 5)
    want = np.zeros((4, 2, 2), np.float32)
    for it in range(4):
        want[it, 0] = adam_step_constants(critic, 8 + it)
    want[1, 1], want[3, 1] = adam_step_constants(actor, 4), adam_step_constants(actor, 5)
    np.testing.assert_array_equal(table, want)
    assert (table[0, 1] == 0).all() and (table[2, 1] == 0).all() and table[3, 0, 0] != table[0, 0, 0]


def test_chunk_size_terms(monkeypatch):
    from tonic_amd.q_update import Route, chunk_size
    for name in ('TONIC_AMD_UPDATE_CHUNK', 'TONIC_AMD_NO_GRAPH'):
        monkeypatch.delenv(name, raising=False)
    whole = Route(0, False)
    assert chunk_size(40, 2, whole, False) == 10 and chunk_size(20, 1, whole, False) == 10
    assert chunk_size(19, 1, whole, False) == 0             # fewer than two chunks
    assert chunk_size(45, 1, whole, False) == 0             # no whole number of chunks
    assert chunk_size(40, 3, whole, False) == 0             # a chunk is no whole number of actor delays
    assert chunk_size(40, 2, whole, True) == 0              # a subclass's own enqueue_update / _update
    assert chunk_size(40, 2, Route(None, False), False) == 0            # the split entries
    assert chunk_size(40, 2, Route(0, True), False) == 0                # in phases (several ranks, an exchange, a clip)
    monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    assert chunk_size(40, 2, whole, False) == 0
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH')
    monkeypatch.setenv('TONIC_AMD_UPDATE_CHUNK', '0')
    assert chunk_size(40, 2, whole, False) == 0
    monkeypatch.setenv('TONIC_AMD_UPDATE_CHUNK', '4')
    assert chunk_size(40, 2, whole, False) == 4 and chunk_size(40, 3, whole, False) == 0


# ------------------------------------------------------------------------------------ the scheduler behind the agent
class Counter:
    """An updater's `state`: the device's step counter, reads of which are logged."""

    def __init__(self, log, name):
        self.log, self.name, self.value, self.memory = log, name, 0, torch.zeros(2, dtype=torch.int32)

    def __getitem__(self, index):
        self.log.append(('read_state', self.name))
        return self.value

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.memory.data_ptr()


class Books:
    """replays.Buffer as far as an update reads it: index streams that count up, batches of zeros."""

    def __init__(self, log, iterations):
        self.log, self.batch_size, self.batch_iterations, self.max_size = log, B, iterations, 100
        self.buffers = {'observations': torch.zeros(1)}
        self.counts, self.drawn, self.last_steps = None, 0, None

    def initialize(self, seed, device=None):
        pass

    def sample_indices(self, iterations=None):
        iterations = iterations or self.batch_iterations
        self.drawn += 1
        self.log.append(('indices', iterations))
        return np.full((iterations, B), self.drawn, np.int64)

    def shard_indices(self, indices):
        positions = np.tile(np.arange(B), (len(indices), 1))
        return indices, positions, np.asarray(self.counts)

    def gather_many(self, indices):
        self.log.append(('gather', int(indices[0, 0])))
        n = indices.shape[0]
        return dict(observations=torch.zeros(n, B, O), actions=torch.zeros(n, B, A),
                    next_observations=torch.zeros(n, B, O), rewards=torch.zeros(n, B), discounts=torch.zeros(n, B))


def floats(address, count):
    return tuple(np.ctypeslib.as_array((ctypes.c_float * count).from_address(address)).tolist()) if address else None


@pytest.fixture
def world(monkeypatch):
    """make(kind): an initialised agent whose every launch lands in `log`."""
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd import _lib, parallel
    from tonic_amd.torch import agents, updaters
    log = []
    knobs = types.SimpleNamespace(supported=1, no_ahead_at=None, give_up_at=None)

    class Library:
        def tonic_q_iteration(self, reference, stream):
            a = reference._obj
            it = len([e for e in log if e[0] == 'q' and e[1] in (0, 1)])          # (since the last take())
            if a.phase != 2 and knobs.give_up_at == it:          # (the critic's epilogue marks its row)
                ctypes.c_float.from_address(a.critic.d_info_row + 7 * 4).value = 1.0
            log.append(('q', a.phase, a.stage, a.slot, a.actor_due, a.refresh_images, a.ahead,
                        floats(a.critic.d_step_constants, 2), floats(a.actor.d_step_constants, 2),
                        ctypes.addressof(a), a.kind))
            return 0

        def tonic_q_iteration_supported(self, *shape):
            return knobs.supported

        def tonic_q_iteration_ahead_supported(self, batch, o, h, a, nets, passes):
            asked = len([e for e in log if e[0] == 'ahead?'])
            log.append(('ahead?', nets, passes))
            return int(knobs.no_ahead_at != asked)

        def tonic_q_iteration_workspace_bytes(self, *shape):
            return 64

    class Graph:
        def replay(self):
            log.append(('replayed', self.name))

    graphs = []

    def new_graph():
        graph = Graph()
        graph.name = len(graphs)
        graphs.append(graph)
        return graph

    @contextlib.contextmanager
    def capturing(graph, **kwargs):
        log.append(('captured', graph.name))
        yield

    monkeypatch.setattr(agents, '_device', lambda: torch.device('cpu'))
    monkeypatch.setattr(_lib, 'current_stream', lambda: 0)
    monkeypatch.setattr(_lib, 'capturing', capturing)
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', new_graph)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda: None)
    monkeypatch.setattr(agents.logger, 'store', lambda key, value: log.append(('log', key)))
    for name in ('TONIC_AMD_FUSED_ITERATION', 'TONIC_AMD_FUSED_PHASES', 'TONIC_AMD_POLICY_AHEAD',
                 'TONIC_AMD_UPDATE_CHUNK', 'TONIC_AMD_NO_GRAPH', 'WORLD_SIZE', 'TONIC_AMD_EXERCISE_EXCHANGE'):
        monkeypatch.delenv(name, raising=False)

    def recorder(name, updater):
        def record(*args, **kwargs):
            if name == '_step':
                updater.steps_enqueued += 1
            shown = [tuple(a.shape) if isinstance(a, torch.Tensor) else a for a in args
                     if a is None or isinstance(a, (int, torch.Tensor))]
            log.append((updater.role + '.' + name, *shown, *sorted(kwargs)))
        return record

    def prepare(updater, role, clip, lr):
        updater.role, updater.initialize = role, lambda model, *more: None
        updater.hyper, updater.plain, updater.world_size = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8), True, 1
        updater.gradient_clip, updater.hidden, updater.steps_enqueued = float(clip), H, 0
        updater.state, updater.normalizer, updater._unit = Counter(log, role), None, (torch.zeros(O), torch.ones(O))
        updater.grad_sums = updater.exp_avg = updater.exp_avg_sq = torch.zeros(8)
        for name in ('enqueue', 'enqueue_empty', '_step', '_offpolicy_workspace'):
            setattr(updater, name, recorder(name, updater))
        return updater

    pairs = dict(ddpg=(tt.agents.DDPG, updaters.DeterministicQLearning, updaters.DeterministicPolicyGradient),
                 td3=(tt.agents.TD3, updaters.TwinCriticDeterministicQLearning, updaters.DeterministicPolicyGradient),
                 sac=(tt.agents.SAC, updaters.TwinCriticSoftQLearning,
                      updaters.TwinCriticSoftDeterministicPolicyGradient),
                 d4pg=(tt.agents.D4PG, updaters.DistributionalDeterministicQLearning,
                       updaters.DistributionalDeterministicPolicyGradient),
                 mpo=(tt.agents.MPO, updaters.ExpectedSARSA, updaters.MaximumAPosterioriPolicyOptimization))

    def make(kind, iterations=4, critic_clip=0, actor_clip=0, agent_class=None):
        default_class, critic_class, actor_class = pairs[kind]
        flat = lambda: types.SimpleNamespace(flat=torch.zeros(8))                # noqa: E731
        model = types.SimpleNamespace(
            initialize=lambda *spaces: None, pack=lambda device: None, observation_normalizer=None,
            return_normalizer=None, critic_1=None, target_coeff=0.005, flat_online=torch.zeros(8),
            flat_target=torch.zeros(8), flat_actor=flat(), flat_critics=flat(), flat_target_actor=flat(),
            flat_target_critics=flat())
        arguments = dict(model=model, replay=Books(log, iterations),
                         critic_updater=prepare(critic_class(), 'critic', critic_clip, 1e-3),
                         actor_updater=prepare(actor_class(), 'actor', actor_clip, 3e-4))
        if kind != 'mpo':
            arguments['exploration'] = tonic_amd.explorations.NoActionNoise(0)
        agent = (agent_class or default_class)(**arguments)
        if kind == 'mpo':
            agent.actor_updater.constraints, agent.actor_updater.num_samples = 1, 3
            agent.critic_updater.num_samples = 2
        box = types.SimpleNamespace(shape=(O,)), types.SimpleNamespace(shape=(A,))
        agent.initialize(*box, seed=0)
        agent.lib = Library()
        agent.close()                                   # (gives the process's CPU binding back; nothing is deferred)
        return agent

    def take():
        events = list(log)
        del log[:]
        return events
    return types.SimpleNamespace(make=make, take=take, knobs=knobs, graphs=graphs, parallel=parallel,
                                 updaters=updaters, agents=agents, monkeypatch=monkeypatch)


def streams(agent, iterations=4, value=1):
    return np.full((iterations, B), value, np.int64), agent._draw_noise(iterations)


def launches(events):
    """The tonic_q_iteration calls of a log as (phase, stage, slot, actor_due, refresh_images, ahead set)."""
    return [(*e[1:6], bool(e[6])) for e in events if e[0] == 'q']


def names(events):
    return [e[0] for e in events]


def constants(hyper, step):
    from tonic_amd.torch.updaters import adam_step_constants
    return tuple(np.asarray(adam_step_constants(hyper, step), np.float32).tolist())


@pytest.mark.parametrize('kind, fused', [('ddpg', 2), ('td3', 0), ('sac', 1), ('mpo', None), ('d4pg', None)])
def test_the_routing_decision(world, kind, fused):
    set_environment = world.monkeypatch.setenv
    agent = world.make(kind)
    assert agent._fused_kind() == fused and not agent._fused_in_phases()
    for clips in (dict(critic_clip=0.5), dict(actor_clip=0.5)):
        clipped = world.make(kind, **clips)
        assert clipped._fused_kind() == fused and clipped._fused_in_phases()
        set_environment('TONIC_AMD_FUSED_PHASES', '0')
        assert clipped._fused_kind() is None and not clipped._fused_in_phases()
        assert agent._fused_kind() == fused and not agent._fused_in_phases()
        world.monkeypatch.delenv('TONIC_AMD_FUSED_PHASES')
    set_environment('TONIC_AMD_FUSED_ITERATION', '0')
    assert agent._fused_kind() is None and not agent._fused_in_phases() and clipped._fused_in_phases()
    world.monkeypatch.delenv('TONIC_AMD_FUSED_ITERATION')
    agent.model.return_normalizer = object()
    assert agent._fused_kind() is None
    agent.model.return_normalizer = None
    for holder, name, value in ((agent.critic_updater, 'plain', False), (agent.actor_updater, 'plain', False),
                                (agent.critic_updater, 'stock', True), (agent.actor_updater, 'stock', True),
                                (world.knobs, 'supported', 0)):
        before = getattr(holder, name)
        setattr(holder, name, value)
        assert agent._fused_kind() is None
        setattr(holder, name, before)
    assert agent._fused_kind() == fused
    agent.critic_updater.world_size = 2
    assert agent._fused_kind() == fused and agent._fused_in_phases()
    agent.critic_updater.world_size = 1
    world.monkeypatch.setattr(world.parallel, 'exchanging', lambda: True)
    assert agent._fused_kind() == fused and agent._fused_in_phases()


def test_a_foreign_actor_updater_takes_the_split_entries(world):
    agent = world.make('td3')
    agent.actor_updater.__class__ = world.updaters.TwinCriticSoftDeterministicPolicyGradient
    assert agent._fused_kind() is None


def test_update_chunk_on_the_agent(world):
    agent = world.make('td3', iterations=40)
    assert agent._update_chunk(40) == 10 and agent._update_chunk(30) == 10 and agent._update_chunk(10) == 0
    agent.delay_steps = 3
    assert agent._update_chunk(40) == 0
    agent.delay_steps = 2
    agent.critic_updater.world_size = 2
    assert agent._update_chunk(40) == 0
    agent.critic_updater.world_size = 1
    assert world.make('td3', critic_clip=1)._update_chunk(40) == 0 and world.make('mpo')._update_chunk(40) == 0

    class OwnUpdate(world.agents.TD3):
        def _update(self, steps):
            return super()._update(steps)

    class OwnEnqueue(world.agents.TD3):
        def enqueue_update(self, indices, eps, graph=None):
            return super().enqueue_update(indices, eps, graph)
    assert world.make('td3', agent_class=OwnUpdate)._update_chunk(40) == 0
    assert world.make('td3', agent_class=OwnEnqueue)._update_chunk(40) == 0
    world.monkeypatch.setattr(world.parallel, 'exchanging', lambda: True)
    assert agent._update_chunk(40) == 0


def test_the_split_route(world):
    agent = world.make('td3')
    world.monkeypatch.setenv('TONIC_AMD_FUSED_ITERATION', '0')
    world.take()
    infos = agent.enqueue_update(*streams(agent))
    assert tuple(infos.shape) == (2, 4, 8) and not agent._phased_update
    batch, row = (B, A), (8,)
    critic, actor = ('critic.enqueue', batch, row, None), ('actor.enqueue', (B, O), None, row, None)
    assert world.take() == [
        ('critic._offpolicy_workspace', B), ('actor._offpolicy_workspace', B), ('gather', 1), ('captured', 0),
        ('gather', 1), critic, critic, actor, critic, critic, actor, ('replayed', 0)]
    # (TD3's actor step draws nothing; SAC's takes the second draw)
    sac = world.make('sac', iterations=1)
    world.take()
    sac.enqueue_update(*streams(sac, 1), graph=False)
    assert world.take() == [('gather', 1), critic, ('actor.enqueue', (B, O), batch, row, None)]


def test_the_split_route_hands_mpo_its_statistics_rows(world):
    agent = world.make('mpo', iterations=2)
    world.take()
    agent.enqueue_update(*streams(agent, 2), graph=False)
    assert world.take() == [('gather', 1)] + 2 * [('critic.enqueue', (2 * B, A), (8,), None),
                                                  ('actor.enqueue', (B, O), (3 * B, A), (8,), None, 'stats_row')]


def test_the_fused_route(world):
    agent = world.make('sac')
    world.take()
    agent.critic_updater.state.value, agent.actor_updater.state.value = 10, 20
    agent.enqueue_update(*streams(agent))
    events = world.take()
    assert names(events) == ['read_state', 'read_state', 'critic._offpolicy_workspace', 'actor._offpolicy_workspace',
                             'gather', 'captured', 'gather', 'q', 'q', 'q', 'q', 'replayed']
    assert launches(events) == [(0, 0, 0, 1, 1, F), (0, 0, 0, 1, 0, F), (0, 0, 0, 1, 0, F), (0, 0, 0, 1, 0, F)]
    rows = [e for e in events if e[0] == 'q']
    for it, row in enumerate(rows):
        assert row[7] == constants(agent.critic_updater.hyper, 11 + it) and row[10] == 1
        assert row[8] == constants(agent.actor_updater.hyper, 21 + it)
    assert (agent.critic_updater.steps_enqueued, agent.actor_updater.steps_enqueued) == (14, 24)
    assert not agent._phased_update


def test_the_fused_route_with_policy_passes_riding_ahead(world):
    agent = world.make('td3')
    world.take()
    agent.enqueue_update(*streams(agent), graph=False)
    events = world.take()
    assert names(events) == ['read_state', 'read_state', 'gather', 'ahead?', 'ahead?', 'q', 'q', 'q', 'q']
    assert [e for e in events if e[0] == 'ahead?'] == [('ahead?', 2, 2)] * 2          # twin critics, a due successor
    assert launches(events) == [(0, 0, 0, 0, 1, T), (0, 2, 1, 1, 0, F), (0, 0, 1, 0, 0, T), (0, 2, 0, 1, 0, F)]
    rows = [e for e in events if e[0] == 'q']
    assert rows[0][6] == rows[1][9] and rows[2][6] == rows[3][9]                      # `ahead`: the next arguments
    assert [row[7] for row in rows] == [constants(agent.critic_updater.hyper, 1 + it) for it in range(4)]
    assert [row[8] for row in rows] == [(0.0, 0.0), constants(agent.actor_updater.hyper, 1),
                                        (0.0, 0.0), constants(agent.actor_updater.hyper, 2)]
    assert (agent.critic_updater.steps_enqueued, agent.actor_updater.steps_enqueued) == (4, 2)
    # the kernels refuse the second pair; the switch: every iteration by itself, and nobody is asked
    world.knobs.no_ahead_at = 1
    agent.enqueue_update(*streams(agent), graph=False)
    assert launches(world.take()) == [(0, 0, 0, 0, 1, T), (0, 2, 1, 1, 0, F), (0, 0, 1, 0, 0, F), (0, 0, 1, 1, 0, F)]
    world.monkeypatch.setenv('TONIC_AMD_POLICY_AHEAD', '0')
    agent.enqueue_update(*streams(agent), graph=False)
    events = world.take()
    assert launches(events) == [(0, 0, 0, 0, 1, F), (0, 0, 0, 1, 0, F), (0, 0, 0, 0, 0, F), (0, 0, 0, 1, 0, F)]
    assert 'ahead?' not in names(events)
    # an iteration that does not step the actor at the end of the call has nothing to carry
    world.monkeypatch.delenv('TONIC_AMD_POLICY_AHEAD')
    world.knobs.no_ahead_at = None
    agent.enqueue_update(*streams(agent, 3), graph=False)
    assert launches(world.take()) == [(0, 0, 0, 0, 1, T), (0, 2, 1, 1, 0, F), (0, 0, 1, 0, 0, F)]


def test_the_fused_route_in_phases(world):
    agent = world.make('td3', critic_clip=0.5)
    world.take()
    agent.enqueue_update(*streams(agent), graph=False)
    events = world.take()
    assert agent._phased_update
    first = [('q', 1), ('critic._step', B, (8,))]
    both = first + [('q', 2), ('actor._step', B, (8,), 'targets')]
    assert [e[:2] if e[0] == 'q' else e for e in events] == [('gather', 1)] + first + both + first + both
    # every half rebuilds the weight images, carries no Adam constants and rides nowhere
    assert launches(events) == [(1, 0, 0, 0, 1, F), (1, 0, 0, 1, 1, F), (2, 0, 0, 1, 1, F),
                                (1, 0, 0, 0, 1, F), (1, 0, 0, 1, 1, F), (2, 0, 0, 1, 1, F)]
    assert all(e[7] is None and e[8] is None for e in events if e[0] == 'q')


def test_an_empty_shard_takes_the_same_steps(world):
    for phases, launched in (('1', True), ('0', False)):
        world.monkeypatch.setenv('TONIC_AMD_FUSED_PHASES', phases)
        agent = world.make('td3', iterations=2)
        agent.critic_updater.world_size = agent.actor_updater.world_size = 2
        agent.replay.counts = [0, 3]
        world.take()
        agent.enqueue_update(*streams(agent, 2), graph=False)
        events = world.take()
        assert agent._phased_update == launched and events[0] == ('gather', 1)
        assert events[1] == ('critic.enqueue_empty', (8,), B)
        if launched:
            assert [e[:2] if e[0] == 'q' else e for e in events[2:]] == [
                ('q', 1), ('critic._step', B, (8,)), ('q', 2), ('actor._step', B, (8,), 'targets')]
        else:
            assert events[2:] == [('critic.enqueue', (3, A), (8,), B), ('actor.enqueue', (3, O), None, (8,), B)]
        agent.replay.counts = [3, 0]
        agent.enqueue_update(*streams(agent, 2), graph=False)
        assert world.take()[-1] == ('actor.enqueue_empty', (8,), B)


def test_replay_and_what_captures_again(world):
    agent = world.make('sac')
    agent.enqueue_update(*streams(agent))
    assert 'captured' in names(world.take())
    agent.enqueue_update(*streams(agent, value=2))
    events = world.take()
    assert names(events) == ['replayed'] and len(world.graphs) == 1          # (no read-back of the counters either)
    agent.critic_updater.hyper['lr'] = 2e-3                                  # a changed hyper-parameter
    agent.enqueue_update(*streams(agent))
    assert names(world.take()).count('captured') == 1 and len(world.graphs) == 2
    indices, eps = streams(agent)
    agent.enqueue_update(indices, np.concatenate([eps, eps], axis=2))        # a changed noise shape
    assert names(world.take()).count('captured') == 1 and len(world.graphs) == 3
    agent.enqueue_update(indices, eps[:2].copy()[[0, 1, 0, 1]])
    assert names(world.take()).count('captured') == 1 and len(world.graphs) == 4
    agent.enqueue_update(indices, eps)
    assert names(world.take()) == ['replayed']
    world.monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    agent.enqueue_update(indices, eps)
    assert names(world.take()) == ['gather', 'q', 'q', 'q', 'q']


def test_a_changed_mpo_statistics_width_captures_again(world):
    agent = world.make('mpo', iterations=2)
    agent.enqueue_update(*streams(agent, 2))
    agent.enqueue_update(*streams(agent, 2))
    assert names(world.take())[-1] == 'replayed' and len(world.graphs) == 1
    agent.actor_updater.constraints = 2
    agent.enqueue_update(*streams(agent, 2))
    assert names(world.take()).count('captured') == 1 and len(world.graphs) == 2


def test_update_reads_back_logs_and_keeps_last_infos(world):
    agent = world.make('mpo', iterations=2)
    world.take()
    agent._update(steps=123)
    events = world.take()
    assert events[0] == ('indices', 2) and agent.replay.last_steps == 123
    logged = [e[1] for e in events if e[0] == 'log']
    assert logged[:2] == ['critic/loss', 'critic/q'] and logged.count('critic/loss') == 2
    assert 'actor/alpha_mean' in logged
    assert agent.last_infos.shape == (2, 2, 8) and agent.last_actor_infos.shape == (2, 11)
    agent = world.make('td3')
    world.take()
    agent._update(steps=7)
    logged = [e[1] for e in world.take() if e[0] == 'log']
    assert logged == ['critic/loss', 'critic/q'] * 4 and agent.last_infos.shape == (2, 4, 8)


def test_chunks_alternate_two_sets_of_graph_inputs(world):
    agent = world.make('td3', iterations=40)
    world.take()
    agent._update(steps=1)
    events = world.take()
    assert [e for e in events if e[0] in ('indices', 'captured', 'replayed')] == [
        ('indices', 10), ('captured', 0), ('replayed', 0), ('indices', 10), ('captured', 1), ('replayed', 1),
        ('indices', 10), ('replayed', 0), ('indices', 10), ('replayed', 1)]
    # each graph reads its own index buffer (the stand-in Buffer's k-th draw holds k) ...
    assert [e[1] for e in events if e[0] == 'gather'] == [1, 1, 2, 2]
    # ... and its own Adam constants: the table of every chunk goes on where the chunk before ended
    rows = [e for e in events if e[0] == 'q']
    assert len(rows) == 20 and rows[0][7] == constants(agent.critic_updater.hyper, 1)
    assert rows[10][7] == constants(agent.critic_updater.hyper, 11)
    assert rows[19][8] == constants(agent.actor_updater.hyper, 10)
    assert (agent.critic_updater.steps_enqueued, agent.actor_updater.steps_enqueued) == (40, 20)
    assert agent.last_infos.shape == (2, 40, 8) and names(events).count('read_state') == 2
    # the next call replays both and reads no counter back; a single-graph call afterwards uses the first set
    agent._update(steps=2)
    events = world.take()
    assert [e for e in events if e[0] in ('captured', 'replayed')] == [('replayed', 0), ('replayed', 1)] * 2
    assert 'read_state' not in names(events) and agent.critic_updater.steps_enqueued == 80
    agent.critic_updater.hyper['lr'] = 5e-4                    # both sets notice, each at its own next turn
    agent._update(steps=3)
    assert [e[1] for e in world.take() if e[0] == 'captured'] == [2, 3]
    world.monkeypatch.setenv('TONIC_AMD_UPDATE_CHUNK', '0')
    agent._update(steps=4)
    events = world.take()
    assert [e for e in events if e[0] in ('indices', 'captured', 'replayed')] == [
        ('indices', 40), ('captured', 4), ('replayed', 4)]


def test_the_step_mirror_is_read_back_only_when_the_device_decides(world):
    agent = world.make('sac', iterations=2)
    reads = lambda: names(world.take()).count('read_state')                # noqa: E731
    agent._update(steps=1)
    assert reads() == 2                                        # a new scheduler trusts the device
    agent._update(steps=2)
    agent.enqueue_update(*streams(agent, 2), graph=False)
    assert reads() == 0
    world.monkeypatch.setenv('TONIC_AMD_FUSED_ITERATION', '0')
    agent.enqueue_update(*streams(agent, 2), graph=False)      # an eager update on the split entries
    world.monkeypatch.delenv('TONIC_AMD_FUSED_ITERATION')
    assert reads() == 0
    agent.critic_updater.state.value, agent.actor_updater.state.value = 50, 60
    agent._update(steps=3)
    assert reads() == 2 and (agent.critic_updater.steps_enqueued, agent.actor_updater.steps_enqueued) == (52, 62)
    agent._update(steps=4)
    assert reads() == 0
    world.knobs.give_up_at = 1                                 # a chained launch gave up: steps were skipped
    world.monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    from tonic_amd._lib import TonicHipError
    with pytest.raises(TonicHipError, match='1 optimizer steps of this update were skipped'):
        agent._update(steps=5)
    assert agent.replay.last_steps == 4 and reads() == 0
    world.knobs.give_up_at = None
    agent._update(steps=6)
    assert reads() == 2 and agent.replay.last_steps == 6
