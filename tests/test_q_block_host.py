"""CPU test of the off-policy agents' acting / storing on the environment's block (tonic_amd.q_block): DDPG's
own step / test_step / update / settle / close drive QBlock and QBlocks with the device methods replaced by
recorders, a stand-in Buffer that only keeps books, and real collector blocks (plain shared memory)."""
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

W, O, A = 3, 5, 2
START = 100            # the exploration's start_steps: the policy acts on steps > START


class Books:
    """reserve_row / store_at / store / ready of replays.Buffer as bookkeeping (rows count up, no wrap)."""

    def __init__(self, return_steps=1):
        self.return_steps, self.buffers, self.index, self.size = return_steps, None, 0, 0
        self.reserved, self.written, self.due = [], [], False

    def reserve_row(self, normalizer=None):
        assert self.buffers is not None and self.return_steps == 1
        self.reserved.append(self.index)
        self.index += 1
        return self.index - 1

    def store_at(self, row, normalizer=None, **kwargs):
        self.written.append(row)

    def store(self, normalizer=None, **kwargs):
        self.buffers = self.buffers or {'allocated': True}
        self.store_at(self.index)
        self.index += 1

    def ready(self, steps):
        return self.due


@pytest.fixture
def world(monkeypatch):
    """An agent whose every device operation lands in `log`, and two environments' blocks."""
    import tonic_amd
    from tonic_amd import q_block
    from tonic_amd.collector import Block
    from tonic_amd.torch.agents import DDPG
    log, created = [], []

    def create_resources(self):
        created.append(self.block)
        self.usable, self.rows, self.fields = True, ['rows0', 'rows1'], {}

    def act(self, kind, stochastic, carried):
        log.append(('act', self.block, carried, self.turn ^ 1))
        if carried is not None:
            self.registry.agent.replay.store_at(carried[0])

    def store_at(self, row, turn):
        log.append(('store_at', self.block, row, turn))
        self.registry.agent.replay.store_at(row)

    def store_now(self, observations):
        log.append(('store_now', self.block, observations is not None, self.turn))
        self.registry.agent.replay.store()
    monkeypatch.setattr(q_block.QBlock, '_create_resources', create_resources)
    monkeypatch.setattr(q_block.QBlock, '_act', act)
    monkeypatch.setattr(q_block.QBlock, '_store_at', store_at)
    monkeypatch.setattr(q_block.QBlock, '_store_now', store_now)
    monkeypatch.setattr(q_block.QBlock, '_synchronize', lambda self: log.append(('sync', self.block)))
    monkeypatch.setattr(q_block.QBlocks, '_create_images', lambda self, kind: 'images')
    monkeypatch.delenv('TONIC_AMD_Q_BLOCK', raising=False)

    class Agent(DDPG):
        def _forward_staged(self, observations, kind, stochastic):
            log.append(('staged_forward',))
            return np.zeros((len(observations), A), np.float32)

        def _store_staged(self, observations, rewards, resets, terminations):
            log.append(('staged_store',))
            self.replay.store()

        def _update(self, steps):
            # the update samples every transition taken so far: all of them are written
            assert sorted(self.replay.written) == list(range(self.replay.index))
            log.append(('update',))

    def agent(return_steps=1):
        agent = Agent(model=types.SimpleNamespace(observation_normalizer=None, return_normalizer=None),
                      replay=Books(return_steps), exploration=tonic_amd.explorations.NoActionNoise(START),
                      actor_updater=1, critic_updater=1)
        agent.exploration.initialize(agent._policy, types.SimpleNamespace(shape=(A,)), seed=0)
        agent.hidden, agent.observation_size, agent.action_size = 32, O, A
        agent._q = q_block.QBlocks(agent)
        return agent

    def take():
        events = list(log)
        del log[:]
        return events
    return types.SimpleNamespace(agent=agent, take=take, created=created, train=Block(W, O, A), test=Block(W, O, A))


def state(q):
    return q.turn, q.acted, q.fed, q.deferred, q.store_pending


def train_step(agent, block, steps, foreign=False):
    """agent.step -> (the environment) -> agent.update on the block's own arrays, or on copies of them."""
    observations = block.out_observations.copy() if foreign else block.out_observations
    actions = agent.step(observations, steps)
    infos = {k: v.copy() for k, v in block.infos.items()} if foreign else dict(block.infos)
    return actions, lambda: agent.update(**infos, steps=steps)


def test_warm_up_stores_now_and_synchronizes_before_the_next_copy(world):
    agent, S = world.agent(), world.train
    for t in range(3):
        actions, update = train_step(agent, S, steps=t)
        q = agent._q.stepped
        # (the first step has nothing pending; later ones wait for the store that reads the block in place)
        assert world.take() == ([('sync', S)] if t else [])
        assert actions.dtype == np.float64 and actions is not S.out_actions       # the draws as they are
        np.testing.assert_array_equal(S.actions, actions.astype(np.float32))
        assert state(q) == (0, False, True, None, False)
        update()
        assert world.take() == [('sync', S), ('store_now', S, True, 0)]
        assert state(q) == (0, False, True, None, True)
    assert agent.replay.written == [0, 1, 2] and agent.replay.reserved == []


def test_steady_state_reserves_and_the_next_launch_carries_that_row_and_turn(world):
    agent, S = world.agent(), world.train
    _, update = train_step(agent, S, steps=0)             # one warm-up step: the Buffer is allocated
    update()
    world.take()
    carried, turn = None, 0
    for t in range(6):
        actions, update = train_step(agent, S, steps=START + 1 + t)
        q = agent._q.stepped
        turn ^= 1
        assert world.take() == [('act', S, carried, turn)]       # (waits for the warm-up's store too: no sync)
        assert actions is S.out_actions and state(q) == (turn, True, True, None, False)
        update()
        carried = (1 + t, turn)
        assert world.take() == [] and state(q) == (turn, True, True, carried, False)
    assert agent.replay.reserved == [1, 2, 3, 4, 5, 6] and agent.replay.written == [0, 1, 2, 3, 4, 5]


def test_first_policy_step_on_an_unallocated_buffer_stores_now(world):
    agent, S = world.agent(), world.train
    _, update = train_step(agent, S, steps=START + 1)
    update()
    assert world.take() == [('act', S, None, 1), ('store_now', S, False, 1)]
    assert state(agent._q.stepped) == (1, True, True, None, True)
    _, update = train_step(agent, S, steps=START + 2)
    assert world.take() == [('act', S, None, 0)] and state(agent._q.stepped) == (0, True, True, None, False)


def test_a_due_update_flushes_the_reserved_row_first(world):
    agent, S = world.agent(), world.train
    train_step(agent, S, steps=0)[1]()
    train_step(agent, S, steps=START + 1)[1]()
    world.take()
    agent.replay.due = True
    _, update = train_step(agent, S, steps=START + 2)
    assert world.take() == [('act', S, (1, 1), 0)]
    update()
    assert world.take() == [('store_at', S, 2, 0), ('update',)]
    assert state(agent._q.stepped) == (0, True, True, None, False)
    agent.replay.due = False
    train_step(agent, S, steps=START + 3)
    assert world.take() == [('act', S, None, 1)]             # nothing rides


def test_a_forward_on_another_block_flushes_instead_of_carrying(world):
    agent, S, T = world.agent(), world.train, world.test
    train_step(agent, S, steps=0)[1]()
    train_step(agent, S, steps=START + 1)[1]()
    world.take()
    q = agent._q.stepped
    for _ in range(2):
        actions = agent.test_step(T.out_observations, START + 1)
        assert actions is not T.out_actions
    assert world.take() == [('store_at', S, 1, 1), ('act', T, None, 1), ('act', T, None, 0)]
    assert state(q) == (1, True, True, None, True)
    train_step(agent, S, steps=START + 2)
    assert world.take() == [('act', S, None, 0)] and state(q) == (0, True, True, None, False)
    assert len(agent._q.blocks) == 2 and agent.replay.written == [0, 1]


def test_foreign_arrays_take_the_staged_path_and_lose_no_reserved_row(world):
    agent, S = world.agent(), world.train
    train_step(agent, S, steps=0)[1]()
    train_step(agent, S, steps=START + 1)[1]()
    world.take()
    q = agent._q.stepped
    # the policy is asked about foreign arrays: the reserved row goes out first, then the staged forward
    _, update = train_step(agent, S, steps=START + 2, foreign=True)
    assert agent._q.stepped is None
    update()
    assert world.take() == [('store_at', S, 1, 1), ('staged_forward',), ('staged_store',)]
    assert state(q) == (1, False, False, None, True) and agent.replay.written == [0, 1, 2]
    train_step(agent, S, steps=START + 3)[1]()
    assert world.take() == [('act', S, None, 0)] and state(q) == (0, True, True, (3, 0), False)
    # a foreign step the policy sits out touches nothing: the row stays reserved for the next launch
    _, update = train_step(agent, S, steps=0, foreign=True)
    update()
    assert world.take() == [('staged_store',)] and state(q) == (0, False, False, (3, 0), False)
    train_step(agent, S, steps=START + 4)
    assert world.take() == [('act', S, (3, 0), 1)] and sorted(agent.replay.written) == [0, 1, 2, 3, 4]
    # the block's arrays handed back after a step on foreign ones are not this step's transition
    agent.step(S.out_observations.copy(), START + 5)
    agent.update(**S.infos, steps=START + 5)
    assert world.take() == [('staged_forward',), ('staged_store',)]


def test_the_switch_and_other_policy_kinds_take_the_staged_path(world, monkeypatch):
    agent, S = world.agent(), world.train
    assert agent._q.find(S.out_observations, 2) is None            # (MPO's Gaussian head)
    monkeypatch.setenv('TONIC_AMD_Q_BLOCK', '0')
    train_step(agent, S, steps=START + 1)[1]()
    assert world.take() == [('staged_forward',), ('staged_store',)] and not agent._q.blocks


def test_n_step_returns_never_reserve(world):
    agent, S = world.agent(return_steps=2), world.train
    train_step(agent, S, steps=0)[1]()
    world.take()
    for t in range(4):
        train_step(agent, S, steps=START + 1 + t)[1]()
        turn = (t + 1) % 2
        assert world.take() == [('act', S, None, turn), ('store_now', S, False, turn)]
        assert state(agent._q.stepped) == (turn, True, True, None, True)
    assert agent.replay.reserved == [] and agent.replay.written == [0, 1, 2, 3, 4]


def test_settle_and_close(world):
    agent, S, T = world.agent(), world.train, world.test
    train_step(agent, S, steps=0)[1]()
    train_step(agent, T, steps=START + 1)[1]()         # a second training environment: reserved on T
    train_step(agent, S, steps=START + 2)[1]()         # flushes T's (pending), reserves on S
    world.take()
    qs = list(agent._q.blocks.values())
    assert [q.block for q in qs] == [S, T] and state(qs[0])[3:] == ((2, 1), False) and state(qs[1])[3:] == (None, True)
    agent.settle()
    assert world.take() == [('store_at', S, 2, 1), ('sync', S), ('sync', T)]
    assert all(state(q)[3:] == (None, False) for q in qs)
    agent.settle()
    assert world.take() == []
    train_step(agent, S, steps=START + 3)[1]()
    world.take()
    agent.close()
    assert world.take() == [('store_at', S, 3, 0), ('sync', S)]
    assert agent._q.blocks == {} and agent._q.last is None and agent._q.stepped is None
    assert agent.replay.written == [0, 1, 2, 3]
    before = len(world.created)
    train_step(agent, S, steps=START + 4)[1]()         # found again, from scratch
    assert len(world.created) == before + 1 and world.take() == [('act', S, None, 1)]


def test_every_reserved_row_is_written_once_in_order(world):
    agent, S, T = world.agent(), world.train, world.test
    random = np.random.RandomState(7)
    train_step(agent, S, steps=0)[1]()
    kinds = {}
    for _ in range(400):
        kind = random.choice(['train', 'train', 'train', 'sits_out', 'foreign', 'test', 'test_foreign', 'settle'])
        kinds[kind] = kinds.get(kind, 0) + 1
        agent.replay.due = random.uniform() < 0.2
        if kind in ('train', 'sits_out', 'foreign'):
            unwritten = set(agent.replay.reserved) - set(agent.replay.written)
            assert len(unwritten) <= 1
            train_step(agent, S, steps=0 if kind == 'sits_out' else START + 1, foreign=kind == 'foreign')[1]()
            acts = [e for e in world.take() if e[0] == 'act']
            # an acting launch carries exactly the row that was reserved and not yet written
            assert [e[2][0] for e in acts if e[2] is not None] == (sorted(unwritten) if kind == 'train' else [])
        elif kind == 'test':
            for _ in range(random.randint(1, 4)):
                agent.test_step(T.out_observations, START + 1)
        elif kind == 'test_foreign':
            agent.test_step(T.out_observations.copy(), START + 1)
        else:
            agent.settle()
            assert sorted(agent.replay.written) == list(range(agent.replay.index))
        written = agent.replay.written
        assert written == sorted(written) and len(set(written)) == len(written)
    assert min(kinds.values()) >= 20 and len(agent.replay.reserved) >= 100
    agent.close()
    assert agent.replay.written == list(range(agent.replay.index))
    assert set(agent.replay.reserved) <= set(agent.replay.written)
