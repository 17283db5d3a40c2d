"""Learning-rate schedules through the updaters and the agents, on every route a step takes: PPO's pair launch, the
fused off-policy iteration, the split entries (polyak riding in the actor's launch), a stock-torch torso, MPO's dual
block, SAC's entropy-coefficient tuner, captured graphs.

(a) `ConstantLR(factor=1.0, total_iters=1)` on every updater is the agent without a scheduler, bit for bit, over two
    update calls: parameters, targets, moments, state words and statistics rows.
(b) `SequentialLR([LinearLR(0.1, 1.0, 4), CosineAnnealingLR(T_max=9, eta_min=1e-5)], [4])`: the fused iteration (its
    rates formed on the host into the Adam table) equals the split entries (formed on the device), the captured
    update equals the eager one, the second call replays the same graph, and the logged `*/learning_rate` is
    tonic_lr_schedule_value at the counted step.
(c) PPO whose KL threshold stops the actor early: the actor's and the critic's logged rates follow their own counts.

PPO: W = 4 workers, T = 16 steps, the fused (64, 64) torso; DDPG, TD3 and SAC: B = 20, 6 iterations, O = 17, A = 6."""
import numpy as np
import pytest

import lr_schedule_ref as sref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

O, A, B, ITERATIONS, ROWS, W = 17, 6, 20, 6, 30, 4
WARM = 'warmup-cosine'


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


def constant(optimizer):
    return torch.optim.lr_scheduler.ConstantLR(optimizer, factor=1.0, total_iters=1)


@pytest.fixture
def logged(monkeypatch):
    from tonic_amd.torch import agents
    store = {}
    monkeypatch.setattr(agents.logger, 'store', lambda key, value: store.setdefault(key, []).append(value))
    return store


# ------------------------------------------------------------------------------------------------ off-policy agents

def q_agent(kind, scheduler, sizes=None, tuner=False):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    u, more = tt.updaters, {}
    keyword = dict(lr_scheduler=scheduler)
    if kind == 'sac':
        head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                            distribution=tt.models.SquashedMultivariateNormalDiag)
        relu = torch.nn.ReLU
        more['model'] = tt.models.ActorTwinCriticWithTargets(
            actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(),
                                  torso=tt.models.MLP(sizes or (256, 256), relu), head=head),
            critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(),
                                    torso=tt.models.MLP(sizes or (256, 256), relu), head=tt.models.ValueHead()),
            observation_normalizer=tt.normalizers.MeanStd())
        if tuner:
            more['entropy_coeff_updater'] = u.EntropyCoeffTuning(**keyword)
    cls, critic, actor = {
        'ddpg': (tt.agents.DDPG, u.DeterministicQLearning, u.DeterministicPolicyGradient),
        'td3': (tt.agents.TD3, u.TwinCriticDeterministicQLearning, u.DeterministicPolicyGradient),
        'sac': (tt.agents.SAC, u.TwinCriticSoftQLearning, u.TwinCriticSoftDeterministicPolicyGradient),
        'd4pg': (tt.agents.D4PG, u.DistributionalDeterministicQLearning, u.DistributionalDeterministicPolicyGradient),
        'mpo': (tt.agents.MPO, u.ExpectedSARSA, u.MaximumAPosterioriPolicyOptimization)}[kind]
    actor_keyword = dict(actor_lr_scheduler=scheduler, dual_lr_scheduler=scheduler) if kind == 'mpo' else keyword
    agent = cls(replay=tonic_amd.replays.Buffer(size=ROWS * W, batch_iterations=ITERATIONS, batch_size=B,
                                                steps_before_batches=0, steps_between_batches=1),
                critic_updater=critic(**keyword), actor_updater=actor(**actor_keyword), **more)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=7)
    rng = np.random.RandomState(321)
    for _ in range(ROWS - 3):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        row = {k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()}
        agent.replay.store(normalizer=agent.model.observation_normalizer, **row)
    return agent


def q_state(agent):
    tensors = [agent.model.flat_online, agent.model.flat_target]
    blocks = [agent.critic_updater.optim, agent.actor_updater.optim]
    if getattr(agent.actor_updater, 'dual_optim', None) is not None:
        blocks.append(agent.actor_updater.dual_optim)
        tensors.append(agent.actor_updater.duals)
    tuner = getattr(agent, 'entropy_coeff_updater', None)
    if tuner is not None:
        blocks.append(tuner.optim)
        tensors.append(tuner.log_entropy_coeff)
    for block in blocks:
        tensors += [block.state] + ([block.slots] if block.slots is not None else [])
    if agent.critic_updater.stock:
        for updater in (agent.critic_updater, agent.actor_updater):
            for state in updater.torch_optimizer.state.values():
                tensors += [state['exp_avg'], state['exp_avg_sq']]
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().tobytes() for t in tensors]


def q_updates(agent, calls=2):
    """`calls` update calls on streams of their own -> per call (infos, state bytes, graph, steps taken)."""
    rng, out = np.random.RandomState(5), []
    shape = agent._draw_noise(ITERATIONS).shape
    for _ in range(calls):
        indices = rng.randint(0, agent.replay.size * agent.replay.global_workers, size=(ITERATIONS, B)).astype(np.int64)
        eps = rng.normal(size=shape).astype(np.float32)
        infos = agent.enqueue_update(indices, eps).cpu().numpy().copy()
        stats = agent._u.slot.stats.cpu().numpy().copy() if agent._u.slot.stats is not None else None
        out.append(dict(infos=infos, stats=stats, state=q_state(agent), graph=agent._u.slot.graph,
                        counts=(int(agent.critic_updater.state[0]), int(agent.actor_updater.state[0]))))
    return out


def same_runs(a, b, what):
    for call, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x['infos'].view(np.int32), y['infos'].view(np.int32)), f'{what}, call {call}: infos'
        if x['stats'] is not None:
            assert np.array_equal(x['stats'].view(np.int32), y['stats'].view(np.int32)), f'{what}, call {call}: stats'
        assert x['state'] == y['state'], f'{what}, call {call}: parameters, moments or state words'
        assert x['counts'] == y['counts']


ROUTES = [('ddpg', 'fused'), ('td3', 'fused'), ('sac', 'fused'), ('ddpg', 'split'), ('td3', 'split'),
          ('sac', 'split'), ('sac', 'tuned'), ('sac', 'stock'), ('d4pg', 'split'), ('mpo', 'split')]


def on_route(monkeypatch, kind, route, scheduler):
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH', raising=False)
    monkeypatch.setenv('TONIC_AMD_FUSED_ITERATION', '0' if route == 'split' else '1')
    agent = q_agent(kind, scheduler, sizes=(48, 40, 32, 24, 16) if route == 'stock' else None, tuner=route == 'tuned')
    assert (agent._u.route().fused_kind is not None) == (route == 'fused'), (kind, route)
    assert agent.critic_updater.stock == (route == 'stock')
    return agent


@pytest.mark.parametrize('kind, route', ROUTES)
def test_a_constant_schedule_is_no_schedule(lib, monkeypatch, kind, route):
    """(a) on the fused iteration, the split entries, the tuner's block, a stock-torch torso, D4PG and MPO."""
    plain = on_route(monkeypatch, kind, route, None)
    scheduled = on_route(monkeypatch, kind, route, constant)
    assert plain.critic_updater.schedule is None and scheduled.critic_updater.schedule is not None
    assert scheduled.actor_updater.schedule is not None
    same_runs(q_updates(plain), q_updates(scheduled), f'{kind} / {route}')
    plain.close()
    scheduled.close()


def check_logged(agent, logged, run, schedule):
    """`*/learning_rate`: one value per update, the rate of the last step taken."""
    logged.clear()
    agent._log_update(run['infos'], run['stats'])
    critic_count, actor_count = run['counts']
    for name, updater, count in (('critic', agent.critic_updater, critic_count),
                                 ('actor', agent.actor_updater, actor_count)):
        want = sref.value(schedule, updater.hyper['lr'], count - 1)
        assert logged[f'{name}/learning_rate'] == [want], (name, logged.get(f'{name}/learning_rate'), want)
        assert agent.last_learning_rates[name] == (want, count)
        assert updater.learning_rate() == sref.value(schedule, updater.hyper['lr'], count)


@pytest.mark.parametrize('kind', ['ddpg', 'td3', 'sac'])
def test_warmup_cosine_fused_split_captured_eager(lib, monkeypatch, logged, kind):
    """(b).  The table's step sizes are formed from the host's rates, the split entries' on the device: the steps
    compared are safe ones (the reference alone: F32(lr_t / bias1) is the same at lr_t (1 +- 2^-44) for every step
    of the two calls — asserted, at the updaters' default rates)."""
    schedule = sref.SCHEDULES[WARM][1]
    scheduler = sref.factory(WARM)
    fused = on_route(monkeypatch, kind, 'fused', scheduler)
    for updater in (fused.critic_updater, fused.actor_updater):
        assert sref.unpack(updater.schedule) == schedule
        beta1 = updater.hyper['betas'][0]
        for t in range(2 * ITERATIONS):
            assert sref.safe(lambda x, t=t: np.float32(x / (1.0 - beta1 ** (t + 1))),
                             sref.value(schedule, updater.hyper['lr'], t)), (kind, t)
    fused_runs = q_updates(fused)
    assert fused_runs[0]['graph'] is not None and fused_runs[1]['graph'] is fused_runs[0]['graph'], \
        'the second call captured again'
    assert fused_runs[1]['counts'][0] == 2 * ITERATIONS
    split = on_route(monkeypatch, kind, 'split', scheduler)
    split_runs = q_updates(split)
    assert split_runs[1]['graph'] is split_runs[0]['graph'] is not None
    same_runs(fused_runs, split_runs, f'{kind}: fused against split')
    monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    eager = q_agent(kind, scheduler)
    eager_runs = q_updates(eager)
    assert all(run['graph'] is None for run in eager_runs)
    same_runs(split_runs, eager_runs, f'{kind}: captured against eager')
    unscheduled = on_route(monkeypatch, kind, 'fused', None)
    assert q_updates(unscheduled, 1)[0]['state'] != fused_runs[0]['state'], 'the schedule moved nothing'
    check_logged(fused, logged, fused_runs[-1], schedule)
    check_logged(split, logged, split_runs[-1], schedule)
    logged.clear()
    unscheduled._log_update(fused_runs[0]['infos'], None)
    assert logged and not any(key.endswith('learning_rate') for key in logged)      # without a scheduler: no key
    for agent in (fused, split, eager, unscheduled):
        agent.close()


def test_the_tuners_rate_is_logged(lib, monkeypatch, logged):
    schedule = sref.SCHEDULES[WARM][1]
    agent = on_route(monkeypatch, 'sac', 'tuned', sref.factory(WARM))
    runs = q_updates(agent)
    assert runs[1]['graph'] is runs[0]['graph'] is not None
    agent._log_update(runs[1]['infos'], runs[1]['stats'])
    tuner = agent.entropy_coeff_updater
    count = int(tuner.state[0])
    assert count == 2 * ITERATIONS
    assert logged['entropy_coeff/learning_rate'] == [sref.value(schedule, tuner.hyper['lr'], count - 1)]
    agent.close()


# ------------------------------------------------------------------------------------------------ PPO

def ppo_run(scheduler, updates=2, kl_threshold=0.015, iterations=5, T=16, critic_scheduler=False, torso=None):
    """`updates` PPO updates on the Synthetic environment -> the agent, and per update its state and rates.
    `torso` = (sizes, activation): a model of its own (None: the default, the fused (64, 64) Tanh torso)."""
    import tonic_amd
    import tonic_amd.torch as tt
    env = tonic_amd.environments.distribute(lambda: tonic_amd.environments.Synthetic(O, A, max_episode_steps=5), 1, W)
    env.initialize(seed=0)
    critic_scheduler = scheduler if critic_scheduler is False else critic_scheduler
    more, models = {}, tt.models
    if torso is not None:
        sizes, act = torso
        more['model'] = models.ActorCritic(
            actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, act),
                               head=models.DetachedScaleGaussianPolicyHead()),
            critic=models.Critic(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, act),
                                 head=models.ValueHead()),
            observation_normalizer=tt.normalizers.MeanStd())
    agent = tt.agents.PPO(
        **more,
        replay=tonic_amd.replays.Segment(size=T, batch_iterations=iterations),
        actor_updater=tt.updaters.ClippedRatio(kl_threshold=kl_threshold, lr_scheduler=scheduler),
        critic_updater=tt.updaters.VRegression(lr_scheduler=critic_scheduler))
    agent.initialize(env.observation_space, env.action_space, seed=0)
    observations, out = env.start(), []
    for t in range(updates * T):
        actions = agent.step(observations, t * W)
        observations, infos = env.step(actions)
        agent.update(**infos, steps=t * W)
        if (t + 1) % T == 0:
            agent.settle()
            tensors = [agent.model.flat_actor.flat, agent.model.flat_critic.flat]
            for updater in (agent.actor_updater, agent.critic_updater):
                tensors += [updater.exp_avg, updater.exp_avg_sq, updater.state]
            torch.cuda.synchronize()
            out.append(dict(state=[x.detach().cpu().numpy().tobytes() for x in tensors],
                            infos=np.array(agent.last_infos).copy(),
                            counts=(int(agent.actor_updater.state[0]), int(agent.critic_updater.state[0])),
                            rates=dict(getattr(agent, 'last_learning_rates', {}))))
    return agent, out


def test_ppo_constant_schedule_is_no_schedule(lib, logged):
    """(a) on the pair launch, both networks scheduled and the critic alone."""
    plain_agent, plain = ppo_run(None)
    assert 'actor/learning_rate' not in logged and 'critic/learning_rate' not in logged
    for critic_scheduler in (False, constant):
        actor_scheduler = constant if critic_scheduler is False else None
        agent, scheduled = ppo_run(actor_scheduler, critic_scheduler=critic_scheduler)
        assert agent.critic_updater.schedule is not None and not agent.critic_updater.stock
        for call, (x, y) in enumerate(zip(plain, scheduled)):
            assert x['state'] == y['state'], f'update {call}: parameters, moments or state words'
            assert np.array_equal(x['infos'].view(np.int32), y['infos'].view(np.int32)), f'update {call}: infos'
        agent.close()
    assert plain[1]['counts'][1] == 10 and len(logged['critic/learning_rate']) == 4
    plain_agent.close()


@pytest.mark.parametrize('route', ['layers', 'stock'])
def test_ppo_torsos_off_the_fused_kernels(lib, logged, route):
    """(a) on the layer-by-layer entries ((48, 32) ReLU: separate steps through `_OptimizerState.enqueue`) and on a
    stock-torch torso (five layers: the real torch scheduler behind each `optimizer.step()`); under warm-up + cosine
    both log the schedule's rate at their own counts."""
    torso = ((48, 32), torch.nn.ReLU) if route == 'layers' else ((32, 32, 32, 32, 32), torch.nn.ReLU)
    plain_agent, plain = ppo_run(None, torso=torso)
    agent, scheduled = ppo_run(constant, torso=torso)
    assert agent.actor_updater.stock == agent.critic_updater.stock == (route == 'stock')
    assert (agent.actor_updater.torso is not None) == (route == 'layers')
    for call, (x, y) in enumerate(zip(plain, scheduled)):
        assert x['state'] == y['state'] and x['counts'] == y['counts'], f'update {call}'
        assert np.array_equal(x['infos'].view(np.int32), y['infos'].view(np.int32)), f'update {call}: infos'
    logged.clear()
    schedule = sref.SCHEDULES[WARM][1]
    warm_agent, runs = ppo_run(sref.factory(WARM), torso=torso)
    assert runs[1]['state'] != plain[1]['state']
    for run, actor_rate, critic_rate in zip(runs, logged['actor/learning_rate'], logged['critic/learning_rate']):
        actor_count, critic_count = run['counts']
        assert actor_rate == sref.value(schedule, 3e-4, actor_count - 1)
        assert critic_rate == sref.value(schedule, 1e-3, critic_count - 1)
    if route == 'stock':        # the chainable rate the torch optimizer holds is the closed form's, to rounding
        held = warm_agent.actor_updater.learning_rate()
        assert abs(held - sref.value(schedule, 3e-4, runs[1]['counts'][0])) <= 1e-13 * held
    for each in (plain_agent, agent, warm_agent):
        each.close()


def test_ppo_rates_follow_each_networks_own_count(lib, logged):
    """(c): a KL threshold below any KL stops the actor behind its first iteration of every update while the critic
    takes all five; each logged rate is the schedule's value at its own network's last step, and the scheduled run
    moves the parameters off the unscheduled one."""
    schedule = sref.SCHEDULES[WARM][1]
    agent, runs = ppo_run(sref.factory(WARM), kl_threshold=-1e9)
    assert [run['counts'] for run in runs] == [(1, 5), (2, 10)]
    for run, (actor_rate, critic_rate) in zip(runs, zip(logged['actor/learning_rate'], logged['critic/learning_rate'])):
        actor_count, critic_count = run['counts']
        assert actor_rate == sref.value(schedule, 3e-4, actor_count - 1)
        assert critic_rate == sref.value(schedule, 1e-3, critic_count - 1)
        assert run['rates'] == {'actor': (actor_rate, actor_count), 'critic': (critic_rate, critic_count)}
    assert agent.actor_updater.learning_rate() == sref.value(schedule, 3e-4, 2)
    assert agent.critic_updater.learning_rate() == sref.value(schedule, 1e-3, 10)
    plain_agent, plain = ppo_run(None, kl_threshold=-1e9)
    assert [run['counts'] for run in plain] == [(1, 5), (2, 10)] and plain[0]['state'] != runs[0]['state']
    agent.close()
    plain_agent.close()
