"""The optimizer family through the updaters and the agents (updaters._FlatUpdater._step -> tonic_optimizer_step).

Updaters: the step under test is taken from gradient sums the EXISTING grad kernels produced and left in
`updater.grad_sums` (the optimizer only reads them): parameters and every state buffer afterwards must equal the rule's
statement (tests/optim_family_ref.py) applied to the read-back sums, BIT FOR BIT — the same property
test_gpu_optim_family.py holds the C entry to, here with the launch arguments the updaters form (grad_scale = 1 / N, the
statistics kind, the stop flag as skip flag, the polyak targets).  Shapes: the smallest that still cover a ragged tile —
PPO on 2 workers x 8 rows (N = 16 of a 64-row tile), O = 3, A = 2; DDPG at B = 17; SAC at B = 24, 32-unit torso; MPO
at B = 16.

Agents: PPO and DDPG built with such factories initialise (NotImplementedError before this entry existed), take two
updates on `Synthetic` environments, save a checkpoint in the reference's layout that a default-built agent loads, and
a second construction reproduces the run bit for bit."""
import numpy as np
import pytest

import numpy_port as port
import optim_family_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


def optim(name, **kwargs):
    return lambda params: getattr(torch.optim, name)(params, **kwargs)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def host(tensor):
    torch.cuda.synchronize()
    return tensor.detach().cpu().numpy().copy()


def assert_moment_views(updater):
    """`exp_avg` / `exp_avg_sq` are the first two state slots, not buffers of their own."""
    assert updater.exp_avg.data_ptr() == updater.slots.data_ptr()
    assert updater.exp_avg_sq.data_ptr() == updater.slots.data_ptr() + 4 * updater.count


class Follow:
    """An updater's parameters and state buffers, advanced by the statement from the sums the updater holds."""

    def __init__(self, updater):
        self.u, self.rule = updater, updater.hyper
        assert not updater.plain and not updater.stock
        assert (updater.exp_avg is None) == (self.rule['kind'] in ('sgd', 'rmsprop'))
        if updater.exp_avg is not None:
            assert_moment_views(updater)
        self.names = ref.slot_names(self.rule)
        assert (updater.slots.numel() if updater.slots is not None else 0) == len(self.names) * updater.count
        self.p, self.slots, self.step = host(updater.flat.flat), self.read_slots(), 0

    def read_slots(self):
        return list(host(self.u.slots).reshape(-1, self.u.count)) if self.u.slots is not None else []

    def advance(self, n):
        """The statement's step from the sums now in the updater's buffer (mean over `n` rows)."""
        self.step += 1
        sums = host(self.u.grad_sums)[:self.u.count]
        assert np.isfinite(sums).all() and np.abs(sums).max() > 0
        self.p, self.slots = ref.family_statement(self.rule, self.p, sums, self.slots, self.step, 1.0 / n)

    def check(self, what):
        got = [host(self.u.flat.flat)] + self.read_slots()
        for name, g, want in zip(['parameters'] + self.names, got, [self.p] + self.slots):
            differ = np.flatnonzero(bits(g) != bits(want))
            assert differ.size == 0, (f'{what}: {name} differ from the statement in {differ.size} of {g.size} '
                                      f'elements, first [{differ[0]}]: {g[differ[0]]!r} != {want[differ[0]]!r}')
        assert int(self.u.state[0]) == self.step, (what, host(self.u.state))


# ------------------------------------------------------------------ PPO's updaters

def ppo_agent(actor_optimizer, critic_optimizer, kl_threshold=0.015, iterations=2, O=3, A=2, size=8, spaces=True):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    agent = tt.agents.PPO(
        replay=tonic_amd.replays.Segment(size=size, batch_iterations=iterations),
        actor_updater=tt.updaters.ClippedRatio(optimizer=actor_optimizer, kl_threshold=kl_threshold),
        critic_updater=tt.updaters.VRegression(optimizer=critic_optimizer))
    if spaces:
        agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=4)
    return agent


def test_ppo_updaters_step_by_the_statement(lib):
    """ClippedRatio with AdamW + amsgrad, VRegression with RMSprop, N = 2 x 8 rows, O = 3, A = 2, the default torso.
    Two iterations; the first actor step is taken and its KL (the threshold is below any KL) raises the stop flag, so
    the second must not step: parameters, all three state buffers and the counter keep their bits and its row stays
    unwritten.  The critic has no stop: it steps twice."""
    from tonic_amd.torch import updaters
    N, O, A = 16, 3, 2
    agent = ppo_agent(optim('AdamW', lr=3e-4, amsgrad=True), optim('RMSprop', lr=1e-3), kl_threshold=-1e9)
    actor, critic = agent.actor_updater, agent.critic_updater
    assert actor.hyper == dict(kind='adamw', lr=3e-4, weight_decay=1e-2, maximize=False, betas=(0.9, 0.999), eps=1e-8,
                               amsgrad=True)
    assert critic.hyper['kind'] == 'rmsprop' and len(ref.slot_names(actor.hyper)) == 3
    rng = np.random.RandomState(41)
    dev = lambda a: torch.as_tensor(np.asarray(a, F32)).cuda()                         # noqa: E731
    observations, actions = dev(rng.normal(size=(N, O))), dev(rng.uniform(-1, 1, (N, A)))
    advantages, log_probs = dev(rng.normal(size=N)), dev(rng.normal(size=N) - 2.0)
    returns = dev(rng.normal(size=N))
    adv_stats = dev([0.0, 1.0, 0.0, 0.0])
    infos = torch.zeros(2, 2, updaters.INFO_WIDTH, device='cuda')
    follow_actor, follow_critic = Follow(actor), Follow(critic)
    actor.reset_stop()
    for it in range(2):
        actor.enqueue(observations, actions, advantages, adv_stats, log_probs, infos[0, it])
        critic.enqueue(observations, returns, infos[1, it])
        if it == 0:
            follow_actor.advance(N)
        follow_critic.advance(N)
        follow_actor.check(f'actor, iteration {it + 1}')
        follow_critic.check(f'critic, iteration {it + 1}')
        assert host(actor.state).tolist()[:2] == [1, 1]
    rows = host(infos)
    assert rows[0, 0, 5] == 1.0 and rows[0, 0, 6] == 1.0 and not rows[0, 1].any(), rows[0]
    assert rows[1, :, 6].tolist() == [1.0, 1.0] and np.isfinite(rows).all()
    assert (follow_actor.slots[2] >= follow_actor.slots[1]).all()
    agent.close()


# ------------------------------------------------------------------ the off-policy updaters

def q_agent(kind, O, A, B, hidden, actor_optimizer=None, critic_optimizer=None, iterations=1, **replay):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    relu = torch.nn.ReLU
    head = {'sac': lambda: tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                                        distribution=tt.models.SquashedMultivariateNormalDiag),
            'mpo': tt.models.GaussianPolicyHead, 'ddpg': tt.models.DeterministicPolicyHead}[kind]()
    container = tt.models.ActorTwinCriticWithTargets if kind == 'sac' else tt.models.ActorCriticWithTargets
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP((hidden, hidden), relu),
                              head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(),
                                torso=tt.models.MLP((hidden, hidden), relu), head=tt.models.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())
    buffer = tonic_amd.replays.Buffer(batch_iterations=iterations, batch_size=B, **(replay or dict(size=1000)))
    u = tt.updaters
    if kind == 'mpo':
        agent = tt.agents.MPO(model=model, replay=buffer,
                              actor_updater=u.MaximumAPosterioriPolicyOptimization(actor_optimizer=actor_optimizer),
                              critic_updater=u.ExpectedSARSA(optimizer=critic_optimizer))
    elif kind == 'sac':
        agent = tt.agents.SAC(model=model, replay=buffer,
                              actor_updater=u.TwinCriticSoftDeterministicPolicyGradient(optimizer=actor_optimizer),
                              critic_updater=u.TwinCriticSoftQLearning(optimizer=critic_optimizer))
    else:
        agent = tt.agents.DDPG(model=model, replay=buffer,
                               actor_updater=u.DeterministicPolicyGradient(optimizer=actor_optimizer),
                               critic_updater=u.DeterministicQLearning(optimizer=critic_optimizer))
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=6)
    assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
    return agent


def q_batch(rng, B, O, A):
    dev = lambda a: torch.as_tensor(np.asarray(a, F32)).cuda()                         # noqa: E731
    return dict(observations=dev(rng.normal(size=(B, O))), actions=dev(rng.uniform(-1, 1, (B, A))),
                next_observations=dev(rng.normal(size=(B, O))), rewards=dev(rng.normal(size=B) * 2),
                discounts=dev(np.full(B, 0.99) * (rng.uniform(size=B) > 0.1)))


def test_ddpg_updaters_with_sgd_momentum_and_polyak_targets(lib):
    """DeterministicQLearning + DeterministicPolicyGradient with SGD(momentum), B = 17, two iterations (the first
    sets the momentum buffer to the gradient, the second damps it).  The actor's step carries the polyak update:
    every target entry follows `numpy_port.polyak` of the new online buffer.  Such an agent reports no fused kind."""
    O, A, B = 17, 6, 17
    sgd = optim('SGD', lr=1e-2, momentum=0.9, dampening=0.1)
    agent = q_agent('ddpg', O, A, B, 256, actor_optimizer=sgd, critic_optimizer=sgd)
    assert agent._fused_kind() is None
    plain = q_agent('ddpg', O, A, B, 256)
    assert plain._fused_kind() == 2 and plain.actor_updater.plain
    assert plain.actor_updater.slots.numel() == 2 * plain.actor_updater.count
    assert_moment_views(plain.actor_updater)
    model, critic, actor = agent.model, agent.critic_updater, agent.actor_updater
    coeff = float(model.target_coeff)
    assert 0 < coeff < 1
    rng = np.random.RandomState(42)
    follow_critic, follow_actor = Follow(critic), Follow(actor)
    info = torch.zeros(2, 8, device='cuda')
    target = host(model.flat_target)
    for it in range(2):
        batch = q_batch(rng, B, O, A)
        critic.enqueue(batch, None, info[0])
        follow_critic.advance(B)
        follow_critic.check(f'critic, iteration {it + 1}')
        actor.enqueue(batch['observations'], None, info[1],
                      targets=(model.flat_target, model.flat_online, 0, model.target_coeff))
        follow_actor.advance(B)
        follow_actor.check(f'actor, iteration {it + 1}')
        online = host(model.flat_online)
        assert np.array_equal(bits(online[:actor.count]), bits(follow_actor.p))
        target = port.polyak([target], [online], coeff)[0]
        differ = np.flatnonzero(bits(host(model.flat_target)) != bits(target))
        assert differ.size == 0, f'iteration {it + 1}: {differ.size} target entries differ, first [{differ[0]}]'
    rows = host(info)
    assert rows[:, 6].tolist() == [1.0, 1.0] and np.isfinite(rows).all()


def test_sac_critic_with_adam_weight_decay(lib):
    """TwinCriticSoftQLearning with Adam(weight_decay): both critics' block, B = 24 on a 32-unit torso, two steps."""
    O, A, B = 11, 3, 24
    agent = q_agent('sac', O, A, B, 32, critic_optimizer=optim('Adam', lr=1e-3, weight_decay=1e-2))
    assert agent._fused_kind() is None and agent.actor_updater.plain
    critic = agent.critic_updater
    assert critic.hyper['weight_decay'] == 1e-2 and critic.slots.numel() == 2 * critic.count
    rng = np.random.RandomState(43)
    follow = Follow(critic)
    info = torch.zeros(8, device='cuda')
    for it in range(2):
        eps = torch.as_tensor(rng.normal(size=(B, A)).astype(F32)).cuda()
        critic.enqueue(q_batch(rng, B, O, A), eps, info)
        follow.advance(B)
        follow.check(f'iteration {it + 1}')
    assert host(info)[6] == 1.0


def test_mpo_actor_and_duals_with_rmsprop(lib):
    """MaximumAPosterioriPolicyOptimization with RMSprop: `actor_optimizer` also builds the DUAL optimizer
    (actors.py:291-292), so the duals' step goes through tonic_optimizer_step too — from `dual_grads` with
    grad_scale 1.  B = 16, two iterations."""
    O, A, B, S = 17, 2, 16, 20
    rms = optim('RMSprop', lr=1e-3, centered=True, momentum=0.5)
    agent = q_agent('mpo', O, A, B, 256, actor_optimizer=rms)
    actor = agent.actor_updater
    assert actor.hyper == actor.dual_hyper and actor.hyper['kind'] == 'rmsprop'
    assert actor.dual_exp_avg is None and actor.dual_slots.numel() == 3 * (2 * A + 2)
    rng = np.random.RandomState(44)
    follow = Follow(actor)
    duals, dual_slots = host(actor.duals), list(host(actor.dual_slots).reshape(3, -1))
    info = torch.zeros(8, device='cuda')
    for it in range(2):
        observations = torch.as_tensor(rng.normal(size=(B, O)).astype(F32)).cuda()
        eps = torch.as_tensor(rng.normal(size=(S * B, A)).astype(F32)).cuda()
        actor.enqueue(observations, eps, info)
        follow.advance(B)
        follow.check(f'actor, iteration {it + 1}')
        dual_sums = host(actor.dual_grads)[:2 * A + 2]
        assert np.abs(dual_sums).max() > 0
        duals, dual_slots = ref.family_statement(actor.dual_hyper, duals, dual_sums, dual_slots, it + 1, 1.0)
        for name, got, want in zip(['duals'] + ref.slot_names(actor.dual_hyper),
                                   [host(actor.duals)] + list(host(actor.dual_slots).reshape(3, -1)),
                                   [duals] + dual_slots):
            assert np.array_equal(bits(got), bits(want)), (it, name, got, want)
        assert int(actor.dual_state[0]) == it + 1


# ------------------------------------------------------------------ the agents

PPO_KEYS = {'actor.torso.model.0.weight', 'actor.torso.model.0.bias', 'actor.torso.model.2.weight',
            'actor.torso.model.2.bias', 'actor.head.log_scale', 'actor.head.loc_layer.0.weight',
            'actor.head.loc_layer.0.bias', 'critic.torso.model.0.weight', 'critic.torso.model.0.bias',
            'critic.torso.model.2.weight', 'critic.torso.model.2.bias', 'critic.head.v_layer.weight',
            'critic.head.v_layer.bias', 'observation_normalizer._mean', 'observation_normalizer._std'}


def run_agent(kind, seed=3):
    """Two updates on `Synthetic` -> (agent, state_dict as arrays, the updaters' state buffers)."""
    import tonic_amd
    O, A, W = 3, 2, 2
    env = tonic_amd.environments.distribute(lambda: tonic_amd.environments.Synthetic(O, A, max_episode_steps=5), 1, W)
    env.initialize(seed=seed)
    if kind == 'ppo':
        agent, steps = ppo_agent(optim('AdamW', lr=3e-4, amsgrad=True), optim('RMSprop', lr=1e-3), spaces=False), 16
    else:
        agent = q_agent_for_loop(W)
        steps = 12
    agent.initialize(env.observation_space, env.action_space, seed=seed)
    observations = env.start()
    for t in range(steps):
        actions = agent.step(observations, t * W)
        assert np.isfinite(actions).all()
        observations, infos = env.step(actions)
        agent.update(**infos, steps=t * W)
    state = {k: host(v) for k, v in agent.model.state_dict().items()}
    slots = [host(u.slots) for u in (agent.actor_updater, agent.critic_updater)]
    counters = [int(u.state[0]) for u in (agent.actor_updater, agent.critic_updater)]
    return agent, state, slots, counters


def q_agent_for_loop(W):
    import tonic_amd
    import tonic_amd.torch as tt
    sgd = optim('SGD', lr=1e-2, momentum=0.9, nesterov=True)
    replay = tonic_amd.replays.Buffer(size=200, batch_iterations=2, batch_size=17, steps_before_batches=W * 4,
                                      steps_between_batches=W * 4)
    return tt.agents.DDPG(replay=replay, actor_updater=tt.updaters.DeterministicPolicyGradient(optimizer=sgd),
                          critic_updater=tt.updaters.DeterministicQLearning(
                              optimizer=optim('Adam', lr=1e-3, weight_decay=1e-2)))


@pytest.mark.parametrize('kind', ['ppo', 'ddpg'])
def test_agents_run_save_and_reproduce(lib, tmp_path, kind):
    import tonic_amd.torch as tt
    agent, state, slots, counters = run_agent(kind)
    assert not agent.actor_updater.plain and not agent.critic_updater.plain
    assert min(counters) >= 2 and all(np.isfinite(v).all() for v in state.values())
    assert all(np.isfinite(s).all() and np.abs(s).max() > 0 for s in slots)
    path = str(tmp_path / 'agent')
    agent.save(path)
    saved = torch.load(path + '.pt', map_location='cpu')
    if kind == 'ppo':
        assert PPO_KEYS <= set(saved)
    fresh = tt.agents.PPO() if kind == 'ppo' else tt.agents.DDPG()         # (default optimizers: the layout is the model's)
    from tonic_amd.environments import Box
    fresh.initialize(Box(-np.inf, np.inf, (3,)), Box(-1, 1, (2,)), seed=99)
    fresh.load(path)
    loaded = fresh.model.state_dict()
    assert sorted(loaded) == sorted(state)
    for key, value in state.items():
        assert np.array_equal(bits(host(loaded[key])), bits(value)), key
    agent.close()
    fresh.close()
    again, state2, slots2, counters2 = run_agent(kind)
    assert counters2 == counters
    for key, value in state.items():
        assert np.array_equal(bits(state2[key]), bits(value)), f'{key} differs on a second construction'
    for a, b in zip(slots, slots2):
        assert np.array_equal(bits(a), bits(b))
    again.close()
