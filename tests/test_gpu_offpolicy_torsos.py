"""GPU tests of the off-policy agents on torsos of 1 .. 4 layers (tonic_mlp_torso): the reference goldens of all
five agents, one critic step and one actor step at realistic shapes against float64 autograd, the captured update
against the launches one by one, and D4PG / MPO end to end with a save / load round trip."""
import numpy as np
import pytest

import test_gpu_offpolicy as base

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

TORSO_CASES = [('sac_deep3_small', 'sac'), ('td3_single_small', 'td3'), ('ddpg_deep4_small', 'ddpg'),
               ('d4pg_uneven_small', 'd4pg'), ('d4pg_tanh3_small', 'd4pg'), ('mpo_elu_small', 'mpo'),
               ('mpo_deep3_small', 'mpo')]
ACTIVATIONS = {'ReLU': torch.nn.ReLU, 'Tanh': torch.nn.Tanh, 'ELU': torch.nn.ELU}


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.mark.parametrize('name,kind', TORSO_CASES)
def test_torso_update_matches_reference(lib, golden, name, kind):
    """The first learner update of the reference agent with this torso (scripts/make_torso_goldens.py), on the HIP
    entries: neither updater falls back to stock torch operators."""
    g = golden(name)
    agent = base._agent_from_golden(g, kind)
    for updater in (agent.critic_updater, agent.actor_updater):
        assert updater.stock is False and updater.hidden is not None, type(updater).__name__
    base.test_offpolicy_update_matches_reference(lib, golden, name, kind)


# ---------------------------------------------------------------- one step against float64 autograd

def _model(kind, sizes, activation, atoms=None):
    import tonic_amd.torch as tt
    act = ACTIVATIONS[activation]
    if kind == 'sac':
        head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                            distribution=tt.models.SquashedMultivariateNormalDiag)
    elif kind == 'mpo':
        head = tt.models.GaussianPolicyHead()
    else:
        head = tt.models.DeterministicPolicyHead()
    critic_head = tt.models.DistributionalValueHead(*atoms) if kind == 'd4pg' else tt.models.ValueHead()
    container = tt.models.ActorTwinCriticWithTargets if kind in ('sac', 'td3') else tt.models.ActorCriticWithTargets
    return container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=critic_head),
        observation_normalizer=tt.normalizers.MeanStd())


def _f64(module):
    """float64 CPU leaves of a network's weights / biases (models.network_variables order)."""
    from tonic_amd.torch.models import network_variables
    return [p.detach().cpu().double().requires_grad_() for p in network_variables(module)]


def _torso(params, x, layers, activation):
    act = {'ReLU': torch.relu, 'Tanh': torch.tanh, 'ELU': torch.nn.functional.elu}[activation]
    for l in range(layers):
        x = act(torch.nn.functional.linear(x, params[2 * l], params[2 * l + 1]))
    return x


def _linear(params, h, i):
    return torch.nn.functional.linear(h, params[i], params[i + 1])


def _scale(pre):
    return torch.clamp(torch.nn.functional.softplus(pre), 1e-4, 1.0)


def _grad_sums(modules, sums, B):
    """The mean gradients of `modules` out of a flat gradient-sum block (the padded off-policy layout)."""
    from tonic_amd.torch.models import FlatNetwork
    out, at = [], 0
    for p, n, ld in FlatNetwork.slots(modules, padded=True):
        block = sums[at:at + n]
        out.append((block.view(p.shape[0], ld)[:, :p.shape[1]] if ld else block[:p.numel()].view(p.shape)) / B)
        at += n
    return out


def _compare(got, leaves, names):
    for name, g, leaf in zip(names, got, leaves):
        want = leaf.grad.numpy()
        scale = max(np.abs(want).max(), 1e-30)
        np.testing.assert_allclose(g.double().cpu().numpy(), want, rtol=0, atol=1e-5 * scale, err_msg=name)


@pytest.mark.parametrize('kind,sizes,activation,B,extra', [
    ('sac', (400, 300, 200), 'ReLU', 256, None), ('td3', (400, 300, 200), 'ReLU', 256, None),
    ('d4pg', (400, 300), 'ReLU', 256, 51), ('mpo', (256, 256, 256), 'ELU', 256, 20),
    ('sac', (1024,), 'ReLU', 256, None), ('td3', (33, 7, 100), 'Tanh', 33, None)])
def test_one_step_vs_float64(lib, kind, sizes, activation, B, extra):
    """One critic step and one actor step (MPO: its ExpectedSARSA critic step) from identical parameters, batch and
    noise: the gradient sums of the HIP entries / B against float64 autograd of the reference's losses
    (updaters/critics.py, updaters/actors.py), each tensor within 1e-5 of its largest element."""
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    O, A, L = 17, 6, len(sizes)
    atoms = (-10.0, 10.0, extra) if kind == 'd4pg' else None
    model = _model(kind, sizes, activation, atoms)
    replay = tonic_amd.replays.Buffer(size=1000, batch_iterations=1, batch_size=B)
    if kind == 'mpo':
        agent = tt.agents.MPO(model=model, replay=replay,
                              actor_updater=tt.updaters.MaximumAPosterioriPolicyOptimization(num_samples=extra),
                              critic_updater=tt.updaters.ExpectedSARSA(num_samples=extra))
    else:
        agent = dict(sac=tt.agents.SAC, td3=tt.agents.TD3, d4pg=tt.agents.D4PG)[kind](model=model, replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=9)
    critic_u, actor_u = agent.critic_updater, agent.actor_updater
    assert critic_u.stock is False and actor_u.stock is False and critic_u.hidden != sizes[0]
    rng = np.random.RandomState(3)
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))              # noqa: E731
    batch = dict(observations=f32(rng.normal(size=(B, O))), actions=f32(rng.uniform(-1, 1, (B, A))),
                 next_observations=f32(rng.normal(size=(B, O))), rewards=f32(rng.normal(size=B) * 2),
                 discounts=f32(np.full(B, 0.99) * (rng.uniform(size=B) > 0.1)))
    S = extra if kind == 'mpo' else 1
    eps = f32(rng.normal(size=(S * B, A)))
    eps_actor = f32(rng.normal(size=(B, A)))
    gpu = {k: v.cuda() for k, v in batch.items()}
    m = model
    twin = kind in ('sac', 'td3')
    critics = [m.critic_1, m.critic_2] if twin else [m.critic]
    targets = [m.target_critic_1, m.target_critic_2] if twin else [m.target_critic]
    actor, target_actor = _f64(m.actor), _f64(m.target_actor)
    online = [_f64(c) for c in critics]
    frozen = [_f64(c) for c in targets]
    d = {k: v.double() for k, v in batch.items()}

    def policy(params, obs):                      # (torso, head outputs)
        h = _torso(params, obs, L, activation)
        if kind in ('sac', 'mpo'):
            loc = _linear(params, h, 2 * L)
            return (torch.tanh(loc) if kind == 'mpo' else loc), _scale(_linear(params, h, 2 * L + 2))
        return torch.tanh(_linear(params, h, 2 * L)), None

    def critic(params, obs, act):
        h = _torso(params, torch.cat([obs, act], -1), L, activation)
        out = _linear(params, h, 2 * L)
        return out if kind == 'd4pg' else out.squeeze(-1)

    def squashed(loc, scale, noise):
        raw = loc + scale * noise
        a = torch.tanh(raw)
        logp = torch.distributions.Normal(loc, scale).log_prob(raw) - torch.log(1 - a ** 2 + 1e-6)
        return a, logp.sum(-1)

    # ---- critic step (critics.py)
    with torch.no_grad():
        if kind == 'sac':                                                   # :202-235
            loc, scale = policy(actor, d['next_observations'])
            a, logp = squashed(loc, scale, eps.double())
            nxt = torch.min(*[critic(p, d['next_observations'], a) for p in frozen]) - critic_u.entropy_coeff * logp
        elif kind == 'td3':                                                 # :125-134, :156-182
            noise = critic_u.target_action_noise
            a = policy(target_actor, d['next_observations'])[0]
            a = torch.clamp(a + torch.clamp(noise.scale * eps.double(), -noise.clip, noise.clip), -1, 1)
            nxt = torch.min(*[critic(p, d['next_observations'], a) for p in frozen])
        elif kind == 'mpo':                                                 # :238-282
            loc, scale = policy(target_actor, d['next_observations'])
            a = (loc[None] + scale[None] * eps.double().view(S, B, A)).reshape(S * B, A)
            nxt = critic(frozen[0], d['next_observations'].repeat(S, 1), a).view(S, B).mean(0)
        if kind != 'd4pg':
            returns = d['rewards'] + d['discounts'] * nxt
    if kind == 'd4pg':                                                      # :89-122
        values = torch.linspace(*atoms[:2], atoms[2]).double()
        with torch.no_grad():
            a = policy(target_actor, d['next_observations'])[0]
            p_next = torch.softmax(critic(frozen[0], d['next_observations'], a), -1)
            returns = d['rewards'][:, None] + d['discounts'][:, None] * values[None]
            above = (torch.cat([values[1:], values[:1]]) - values)[None, :, None]
            below = (values - torch.cat([values[-1:], values[:-1]]))[None, :, None]
            delta = torch.clamp(returns, values[0], values[-1])[:, None] - values[None, :, None]
            up = (delta >= 0).double()
            hat = (up * delta / above) - ((1 - up) * delta / below)
            target = (torch.clamp(1 - hat, 0, 1) * p_next[:, None]).sum(2)
        logits = critic(online[0], d['observations'], d['actions'])
        loss = -(target * torch.log_softmax(logits, -1)).sum(-1).mean()
    else:
        loss = sum(((critic(p, d['observations'], d['actions']) - returns) ** 2).mean() for p in online)
    loss.backward()
    info = torch.zeros(8, device='cuda')
    critic_u.enqueue(gpu, eps.cuda(), info)
    torch.cuda.synchronize()
    got = _grad_sums(critics, critic_u.grad_sums, B)
    _compare(got, [leaf for p in online for leaf in p], [f'critic {i}' for i in range(len(got))])
    if kind == 'mpo':
        return
    # ---- actor step (actors.py), through the critics the critic step has just moved
    online = [_f64(c) for c in critics]
    if kind == 'sac':                                                       # :238-267
        loc, scale = policy(actor, d['observations'])
        a, logp = squashed(loc, scale, eps_actor.double())
        q = torch.min(*[critic(p, d['observations'], a) for p in online])
        loss = (actor_u.entropy_coeff * logp - q).mean()
    elif kind == 'td3':                                                     # :170-189
        loss = -critic(online[0], d['observations'], policy(actor, d['observations'])[0]).mean()
    else:                                                                   # :203-224
        logits = critic(online[0], d['observations'], policy(actor, d['observations'])[0])
        values = torch.linspace(*atoms[:2], atoms[2]).double()
        loss = -(torch.softmax(logits, -1) * values).sum(-1).mean()
    loss.backward()
    actor_u.enqueue(gpu['observations'], eps_actor.cuda() if kind == 'sac' else None, info)
    torch.cuda.synchronize()
    _compare(_grad_sums([m.actor], actor_u.grad_sums, B), actor, [f'actor {i}' for i in range(len(actor))])


# ---------------------------------------------------------------- capture

@pytest.mark.parametrize('kind,sizes,activation', [('sac', (64, 48, 40, 32), 'ReLU'), ('mpo', (48, 40, 32), 'ELU')])
def test_captured_update_equals_the_launches(lib, monkeypatch, kind, sizes, activation):
    """An update call of 20 iterations captured in a hipGraph (the default) and launched one by one
    (TONIC_AMD_NO_GRAPH=1): parameters, targets, Adam moments, step counters and the logged statistics are
    bit-identical, twice in a row."""
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    O, A, W, B, rows, iterations = 23, 5, 2, 64, 40, 20
    rng = np.random.RandomState(21)
    host = dict(observations=rng.normal(size=(rows, W, O)), actions=rng.uniform(-1, 1, (rows, W, A)),
                next_observations=rng.normal(size=(rows, W, O)), rewards=rng.normal(size=(rows, W)),
                resets=rng.uniform(size=(rows, W)) < 0.1, terminations=rng.uniform(size=(rows, W)) < 0.05)
    host = {k: np.asarray(v, np.float32) for k, v in host.items()}
    results = {}
    for mode, no_graph in (('graph', '0'), ('launches', '1')):
        monkeypatch.setenv('TONIC_AMD_NO_GRAPH', no_graph)
        replay = tonic_amd.replays.Buffer(size=rows * W, batch_iterations=iterations, batch_size=B)
        model = _model(kind, sizes, activation)
        if kind == 'mpo':
            agent = tt.agents.MPO(model=model, replay=replay)
        else:
            agent = tt.agents.SAC(model=model, replay=replay)
        agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=5)
        assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
        norm = agent.model.observation_normalizer
        for t in range(rows):
            replay.store(normalizer=norm, **{k: base.dev(v[t]) for k, v in host.items()})
        infos = []
        for call in range(2):
            agent._update(steps=100000 + 50 * call)
            infos.append(np.array(agent.last_infos, copy=True))
            for t in range(3):
                replay.store(normalizer=norm, **{k: base.dev(v[t]) for k, v in host.items()})
        results[mode] = dict(
            infos0=infos[0], infos1=infos[1], online=agent.model.flat_online.cpu().numpy(),
            target=agent.model.flat_target.cpu().numpy(),
            critic_m=agent.critic_updater.exp_avg.cpu().numpy(), actor_v=agent.actor_updater.exp_avg_sq.cpu().numpy(),
            steps=np.array([int(agent.critic_updater.state[0]), int(agent.actor_updater.state[0])]))
    assert results['graph']['steps'][0] == 2 * iterations
    for key, want in results['launches'].items():
        got = results['graph'][key]
        assert np.array_equal(got, want, equal_nan=True), (key, np.abs(got - want).max())


# ---------------------------------------------------------------- end to end

@pytest.mark.parametrize('kind,sizes,activation', [('d4pg', (64, 48, 32), 'ReLU'), ('mpo', (40, 40, 32, 24), 'Tanh')])
def test_deep_torso_agents_end_to_end(lib, tmp_path, kind, sizes, activation):
    """D4PG and MPO with deep torsos through the drop-in loop on environments.Synthetic: acting, storing, learner
    updates; then save / load restores the same state_dict."""
    import tonic_amd
    import tonic_amd.torch as tt
    O, A, W = 6, 2, 4
    atoms = (-10.0, 10.0, 21) if kind == 'd4pg' else None
    replay = tonic_amd.replays.Buffer(size=2000, batch_iterations=4, batch_size=32, steps_before_batches=W * 10,
                                      steps_between_batches=W * 10, return_steps=3)
    model = _model(kind, sizes, activation, atoms)
    agent = tt.agents.D4PG(model=model, replay=replay) if kind == 'd4pg' else tt.agents.MPO(model=model, replay=replay)
    env = tonic_amd.environments.distribute(lambda: tonic_amd.environments.Synthetic(O, A, max_episode_steps=7), 1, W)
    env.initialize(seed=3)
    agent.initialize(env.observation_space, env.action_space, seed=3)
    assert agent.critic_updater.hidden is not None and agent.critic_updater.hidden != sizes[0]
    before = {k: v.detach().cpu().numpy().copy() for k, v in agent.model.state_dict().items()}
    observations = env.start()
    for t in range(40):
        actions = agent.step(observations, t * W)
        assert actions.shape == (W, A) and np.isfinite(actions).all()
        observations, infos = env.step(actions)
        agent.update(**infos, steps=t * W)
    assert hasattr(agent, 'last_infos') and np.isfinite(np.asarray(agent.last_infos)).all()
    state = {k: v.detach().cpu().numpy().copy() for k, v in agent.model.state_dict().items()}
    assert any(not np.array_equal(state[k], before[k]) for k in state if 'actor' in k)
    path = str(tmp_path / 'agent')
    agent.save(path)
    other = (tt.agents.D4PG(model=_model(kind, sizes, activation, atoms), replay=tonic_amd.replays.Buffer(return_steps=3))
             if kind == 'd4pg' else tt.agents.MPO(model=_model(kind, sizes, activation)))
    other.initialize(env.observation_space, env.action_space, seed=11)
    other.load(path)
    loaded = other.model.state_dict()
    assert sorted(loaded) == sorted(state)
    for key, value in state.items():
        assert np.array_equal(loaded[key].detach().cpu().numpy(), value), key
