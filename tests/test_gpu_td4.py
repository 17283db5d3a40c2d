"""GPU tests of TD4: tonic_twin_distributional_q_grad, the updater and the agent against tests/td4_ref.py.

The target distribution of a row is that of the target critic with the smaller mean: a discontinuous choice, which
a float32 mean that differs from the float64 one in its last bits could make the other way.  So every comparison
with the restatement first asserts td4_ref.precondition ON THE REFERENCE ALONE — every row's |mu_1 - mu_2| at least
1e-4 of the support's range, 25 times the error of a float32 mean, and from 32 rows on each critic selected on at
least a fifth of the rows — and no row is ever left out of a comparison.  The batches' seeds are searched on the CPU
until the reference satisfies it, with the target critics' head weights scaled up so that their means differ
visibly from row to row (`_spread_targets`).

Gradient sums are held by the convention of tests/test_gpu_offpolicy_grads.py: every tensor of both critic blocks
to 1e-5 of its largest element, the statistic slot to the count B, the logged loss / q1 / q2 to float64 at rtol 1e-5."""
import numpy as np
import pytest

import td4_ref
from test_gpu_offpolicy_grads import _batch, _check, _check_stat, _set_normalizer
from test_gpu_offpolicy_torsos import ACTIVATIONS, _grad_sums

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SUPPORT = (-10.0, 10.0)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


# ---------------------------------------------------------------- agents, batches and the seed search

def _model(tt, twin, sizes, activation, atoms, normalizer=None):
    act = ACTIVATIONS[activation]
    container = tt.models.ActorTwinCriticWithTargets if twin else tt.models.ActorCriticWithTargets
    return container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act),
                              head=tt.models.DeterministicPolicyHead()),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=tt.models.DistributionalValueHead(*atoms)),
        observation_normalizer=normalizer if normalizer is not None else tt.normalizers.MeanStd())


def _agent(O, A, sizes, activation, B, NA, noise=None, normalizer=None, seed=9, twin=True, atoms=None, replay=None,
           **more):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    model = _model(tt, twin, sizes, activation, atoms or (*SUPPORT, NA), normalizer)
    replay = replay or tonic_amd.replays.Buffer(size=1000, batch_iterations=1, batch_size=B)
    if twin:
        critic_updater = tt.updaters.TwinCriticDistributionalDeterministicQLearning(
            target_action_noise=tt.updaters.TargetActionNoise(*noise) if noise else None)
        agent = tt.agents.TD4(model=model, replay=replay, critic_updater=critic_updater, **more)
    else:
        agent = tt.agents.D4PG(model=model, replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=seed)
    assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
    return agent


def _spread_targets(agent, layers=2, activation='ReLU', gain=8.0, balance=True):
    """The target critics' head weights times `gain`: freshly initialised heads give nearly uniform distributions
    whose means hardly move from row to row.  One critic's mean would still lie below the other's on nearly every
    row, so target_critic_2's head bias is tilted along the support (bias_i += c z_i / vmax, which moves its mean
    monotonically) until the float64 restatement selects each critic on half of 512 probe rows — all on the CPU."""
    model = agent.model
    with torch.no_grad():
        for critic in (model.target_critic_1, model.target_critic_2):
            critic.head.distributional_layer.weight.mul_(gain)
    if not balance:
        return
    noise, rng = agent.critic_updater.target_action_noise, np.random.RandomState(0)
    probe = {k: v.double() for k, v in _batch(rng, 512, agent.observation_size, agent.action_size).items()}
    eps = torch.as_tensor(rng.normal(size=(512, agent.action_size)))
    bias = model.target_critic_2.head.distributional_layer.bias
    base, z = bias.detach().cpu().clone(), model.target_critic_2.head.values.cpu()
    low, high = -20.0, 20.0
    for _ in range(24):
        c = 0.5 * (low + high)
        with torch.no_grad():
            bias.copy_(base + c * z / z[-1])
        out = td4_ref.critic_targets(td4_ref.Networks.of_model(model, layers, activation), probe, eps, noise.scale,
                                     noise.clip)
        if float((out['mu_1'] - out['mu_2']).median()) > 0:
            low = c
        else:
            high = c


def _copy_network(source, destination):
    with torch.no_grad():
        for s, d in zip(td4_ref.weights(source), td4_ref.weights(destination)):
            d.copy_(s)


def _case(nets, seed, B, O, A, scale, clip, edit=None):
    rng = np.random.RandomState(seed)
    batch = _batch(rng, B, O, A)
    if edit is not None:
        edit(rng, batch)
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
    d = {k: v.double() for k, v in batch.items()}
    return batch, eps, d, td4_ref.critic_targets(nets, d, eps, scale, clip)


def _search(nets, B, O, A, noise, first_seed, edit=None):
    """The first batch seed from `first_seed` on at which the float64 reference satisfies the precondition."""
    for seed in range(first_seed, first_seed + 400):
        batch, eps, d, out = _case(nets, seed, B, O, A, noise.scale, noise.clip, edit)
        if td4_ref.precondition(out, nets.values, B):
            return batch, eps, d
    raise AssertionError('no batch seed satisfies the precondition')


def _critic_sums(agent, batch, eps):
    """One call of the critic updater's entry: (gradient sums and statistics as left for the optimizer, a clone),
    the parameters put back behind the optimizer step that follows it."""
    updater, model = agent.critic_updater, agent.model
    online = model.flat_online.clone()
    updater.enqueue({k: v.cuda() for k, v in batch.items()}, eps.cuda(), torch.zeros(8, device='cuda'))
    torch.cuda.synchronize()
    sums = updater.grad_sums.clone()
    model.flat_online.copy_(online)
    return sums


def _compare_with_float64(agent, layers, activation, batch, eps, d, label):
    """The entry's sums against float64 autograd of the restatement, the precondition asserted first."""
    m, updater, B = agent.model, agent.critic_updater, batch['observations'].shape[0]
    noise = updater.target_action_noise
    nets = td4_ref.Networks.of_model(m, layers, activation)
    out = td4_ref.critic_step(nets, d, eps, noise.scale, noise.clip)
    assert td4_ref.precondition(out, nets.values, B), (out['mu_1'] - out['mu_2']).abs().min()
    sums = _critic_sums(agent, batch, eps)
    stats = sums[updater.count:].cpu().numpy()
    assert stats[5] == B and not stats[[3, 4, 6, 7]].any(), stats
    got = _grad_sums([m.critic_1, m.critic_2], sums, B)
    leaves = nets.params['critic_1'] + nets.params['critic_2']
    # (loss = mean(loss_1) + mean(loss_2): the gradients of the means, like the sums / B)
    err = _check(got, leaves, [f'critic tensor {i}' for i in range(len(leaves))])
    _check_stat(stats[0] / B, out['loss'], out['terms'], 'loss')
    _check_stat(stats[1] / B, out['q1'].mean(), out['q1'], 'q1')
    _check_stat(stats[2] / B, out['q2'].mean(), out['q2'], 'q2')
    share = float(out['second'].double().mean())
    print(f'td4 {label}: largest relative error {err:.2e}, critic 2 selected on {share:.0%} of the rows, smallest '
          f'|mu_1 - mu_2| {float((out["mu_1"] - out["mu_2"]).abs().min()):.2e}')
    return out


# ---------------------------------------------------------------- 1. gradient sums against float64

GRAD_CASES = [
    # O, A, sizes, activation, B, NA, noise, normaliser's clip
    pytest.param(3, 1, (32, 32), 'ReLU', 1, 2, None, None, id='lone-wave-2-atoms'),
    pytest.param(17, 6, (32, 32), 'ReLU', 5, 51, None, None, id='ragged-workgroup'),
    pytest.param(17, 6, (32, 32), 'ReLU', 37, 64, None, None, id='lane-is-last-atom'),
    pytest.param(11, 3, (32, 32), 'ReLU', 64, 17, None, None, id='row-wider-than-atoms'),
    pytest.param(17, 6, (48, 40, 32), 'Tanh', 37, 51, None, None, id='registered-torso'),
    pytest.param(17, 6, (32, 32), 'ReLU', 37, 51, None, 1.0, id='normaliser-clip'),
    pytest.param(11, 3, (32, 32), 'ReLU', 64, 17, (2.0, 1.5), None, id='both-clips-bind'),
]


@pytest.mark.parametrize('O,A,sizes,activation,B,NA,noise,norm_clip', GRAD_CASES)
def test_critic_grads_vs_float64(lib, O, A, sizes, activation, B, NA, noise, norm_clip):
    """A lone wave in a workgroup (B = 1), a ragged last workgroup (B = 5, 37), lane = the last atom (NA = 64), a
    padded logit row wider than NA (17 in 32, 51 in 64, 2 in 16), a registered three-layer Tanh torso, a normaliser
    whose clip binds, and noise under which both the noise clip and the action clip bind on a tenth of the elements
    at least (asserted on the reference)."""
    import tonic_amd.torch as tt
    normalizer = tt.normalizers.MeanStd(clip=norm_clip) if norm_clip else None
    agent = _agent(O, A, sizes, activation, B, NA, noise=noise, normalizer=normalizer)
    assert (agent.critic_updater.hidden == 32) == (len(sizes) == 2)
    rng = np.random.RandomState(O * 7 + NA)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, np.exp(rng.uniform(-0.5, 0.5, O)))
    _spread_targets(agent, len(sizes), activation)
    nets = td4_ref.Networks.of_model(agent.model, len(sizes), activation)
    batch, eps, d = _search(nets, B, O, A, agent.critic_updater.target_action_noise, 100 * B + NA)
    if norm_clip:
        x = (d['observations'] - nets.mean) / nets.std
        assert float((x.abs() > norm_clip).double().mean()) > 0.1
    out = _compare_with_float64(agent, len(sizes), activation, batch, eps, d, f'{sizes} {activation} B={B} NA={NA}')
    if noise:
        assert out['noise_clipped'] >= 0.1 and out['action_clipped'] >= 0.1, (out['noise_clipped'],
                                                                              out['action_clipped'])


# ---------------------------------------------------------------- 2. the projection's edges

def test_projection_edges_vs_float64(lib):
    """A support of integers 1 apart, integer rewards, discounts of 0, 1 and 0.99: returns below vmin, above vmax
    and exactly on atoms (the projection's delta >= 0 branch at delta = 0), rows whose atoms all collapse onto
    the reward."""
    O, A, B, NA = 17, 6, 37, 17
    agent = _agent(O, A, (32, 32), 'ReLU', B, NA, atoms=((1 - NA) / 2, (NA - 1) / 2, NA))
    values = agent.model.critic_1.head.values.double()
    assert np.array_equal(values.numpy(), np.arange(NA) - (NA - 1) / 2)
    _spread_targets(agent)
    nets = td4_ref.Networks.of_model(agent.model, 2, 'ReLU')

    def edit(rng, batch):
        rewards = rng.randint(-3, 4, B).astype(np.float64)
        rewards[rng.uniform(size=B) < 0.3] *= 7.0                     # far past either end of the support
        batch['rewards'] = torch.as_tensor(rewards, dtype=torch.float32)
        batch['discounts'] = torch.as_tensor(rng.choice([0.0, 1.0, 0.99], B, p=[0.25, 0.5, 0.25]),
                                             dtype=torch.float32)
    batch, eps, d = _search(nets, B, O, A, agent.critic_updater.target_action_noise, 7, edit)
    returns = d['rewards'][:, None] + d['discounts'][:, None] * values[None]
    on_atoms = (returns[:, :, None] == values[None, None]).any(-1)
    assert (returns < values[0]).any() and (returns > values[-1]).any() and on_atoms.any()
    between = d['discounts'] == float(np.float32(0.99))                # (the batch holds float32 discounts)
    assert (d['discounts'] == 0).any() and (d['discounts'] == 1).any() and between.any()
    assert (between[:, None] & ~on_atoms).any()                        # ... and returns strictly between atoms
    _compare_with_float64(agent, 2, 'ReLU', batch, eps, d, 'projection edges')


# ---------------------------------------------------------------- 3. reduction to D4PG

def test_identical_twins_without_noise_are_two_d4pg_steps(lib):
    """critic_2 := critic_1, target_critic_2 := target_critic_1 and noise scale 0: each critic block of the sums
    equals tonic_distributional_q_grad's sums for that critic bit for bit (one statement of the arithmetic serves
    both entries; a + clamp(0 * eps) is a), the loss sum is twice D4PG's (the equal means select critic 1: no
    precondition is needed, both choices are the same numbers)."""
    O, A, B, NA, sizes = 17, 6, 37, 51, (32, 32)
    twin = _agent(O, A, sizes, 'ReLU', B, NA, noise=(0.0, 0.5))
    single = _agent(O, A, sizes, 'ReLU', B, NA, twin=False)
    _spread_targets(twin, balance=False)
    m, s = twin.model, single.model
    _copy_network(m.critic_1, m.critic_2)
    _copy_network(m.target_critic_1, m.target_critic_2)
    for source, destination in ((m.actor, s.actor), (m.target_actor, s.target_actor), (m.critic_1, s.critic),
                                (m.target_critic_1, s.target_critic)):
        _copy_network(source, destination)
    rng = np.random.RandomState(3)
    for agent in (twin, single):
        _set_normalizer(agent, np.linspace(-0.3, 0.3, O), np.linspace(0.7, 1.4, O))
    batch = _batch(rng, B, O, A)
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
    got = _critic_sums(twin, batch, eps)
    single.critic_updater.enqueue({k: v.cuda() for k, v in batch.items()}, None, torch.zeros(8, device='cuda'))
    torch.cuda.synchronize()
    want = single.critic_updater.grad_sums
    count = single.critic_updater.count
    assert twin.critic_updater.count == 2 * count
    for block in (0, 1):
        mine = got[block * count:(block + 1) * count]
        assert torch.equal(mine, want[:count]), (block, float((mine - want[:count]).abs().max()))
    stats, d4pg = got[2 * count:].cpu().numpy(), want[count:].cpu().numpy()
    assert stats[5] == d4pg[5] == B
    np.testing.assert_allclose(stats[0], 2 * d4pg[0], rtol=1e-5)
    np.testing.assert_allclose(stats[1], stats[2], rtol=1e-5)         # the same critic twice: q1 = q2


# ---------------------------------------------------------------- 4. additivity over ranks

def test_sums_add_up_over_parts_of_a_batch(lib):
    """What several ranks rely on, without processes: the entry on rows [0, 20) and on rows [20, 37) of a batch adds
    up to the whole batch's sums to 1e-5 of the largest element; the statistics add exactly in B."""
    O, A, B, NA = 17, 6, 37, 51
    agent = _agent(O, A, (32, 32), 'ReLU', B, NA)
    _spread_targets(agent)
    rng = np.random.RandomState(11)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, np.exp(rng.uniform(-0.5, 0.5, O)))
    batch = _batch(rng, B, O, A)
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
    whole = _critic_sums(agent, batch, eps)
    parts = [_critic_sums(agent, {k: v[a:b].contiguous() for k, v in batch.items()}, eps[a:b].contiguous())
             for a, b in ((0, 20), (20, 37))]
    count = agent.critic_updater.count
    assert [float(p[count + 5]) for p in parts] == [20.0, 17.0] and float(whole[count + 5]) == 37.0
    total = parts[0] + parts[1]
    scale = float(whole[:count].abs().max())
    assert float((total[:count] - whole[:count]).abs().max()) <= 1e-5 * scale
    for slot in (0, 1, 2):                                              # loss, q1, q2: sums over the rows
        np.testing.assert_allclose(float(total[count + slot]), float(whole[count + slot]), rtol=1e-5)


# ---------------------------------------------------------------- 5. the actor step on the twin model

def test_actor_step_reads_critic_1_only(lib):
    """DistributionalDeterministicPolicyGradient on the twin model is bit-identical with the same updater on a
    single-critic model that holds critic_1's parameters — sums, statistics and the stepped actor — and changing
    critic_2 alone does not change a bit."""
    O, A, B, NA, sizes = 17, 6, 37, 51, (32, 32)
    rng = np.random.RandomState(4)
    observations = torch.as_tensor(rng.normal(size=(B, O)), dtype=torch.float32).cuda()
    results = []
    source = _agent(O, A, sizes, 'ReLU', B, NA, seed=9).model          # (never stepped: what every case starts from)
    for case in ('twin', 'single', 'other critic_2'):
        agent = _agent(O, A, sizes, 'ReLU', B, NA, twin=case != 'single', seed=9)
        _copy_network(source.actor, agent.model.actor)
        if case == 'single':
            _copy_network(source.critic_1, agent.model.critic)
        else:
            _copy_network(source.critic_1, agent.model.critic_1)
            _copy_network(source.critic_2, agent.model.critic_2)
        if case == 'other critic_2':
            with torch.no_grad():
                for p in td4_ref.weights(agent.model.critic_2):
                    p.add_(0.25)
        _set_normalizer(agent, np.linspace(-0.3, 0.3, O), np.linspace(0.7, 1.4, O))
        updater = agent.actor_updater
        assert type(updater).__name__ == 'DistributionalDeterministicPolicyGradient'
        info = torch.zeros(8, device='cuda')
        updater.enqueue(observations, None, info)
        torch.cuda.synchronize()
        results.append((updater.grad_sums.cpu().numpy(), agent.model.flat_actor.flat.cpu().numpy(),
                        info.cpu().numpy()))
    assert np.abs(results[0][0][:-8]).max() > 0 and results[0][0][-3] == B
    for other in results[1:]:
        for got, want in zip(other, results[0]):
            assert np.array_equal(got, want)


# ---------------------------------------------------------------- 6. whole update calls

def _filled_agent(seed, rows=40, **more):
    """O = 17, A = 6, hidden 32, B = 37, NA = 51, W = 2: an initialised agent whose Buffer holds `rows` rows."""
    import tonic_amd
    O, A, W, B, NA = 17, 6, 2, 37, 51
    replay = tonic_amd.replays.Buffer(size=rows * W, batch_iterations=4, batch_size=B)
    agent = _agent(O, A, (32, 32), 'ReLU', B, NA, replay=replay, seed=seed, **more)
    rng = np.random.RandomState(seed)
    _set_normalizer(agent, rng.normal(size=O) * 0.3, np.exp(rng.uniform(-0.5, 0.5, O)))
    _spread_targets(agent)
    host = dict(observations=rng.normal(size=(rows, W, O)), actions=rng.uniform(-1, 1, (rows, W, A)),
                next_observations=rng.normal(size=(rows, W, O)), rewards=rng.normal(size=(rows, W)) * 2,
                resets=rng.uniform(size=(rows, W)) < 0.1, terminations=rng.uniform(size=(rows, W)) < 0.05)
    for t in range(rows):
        replay.store(**{k: torch.as_tensor(np.asarray(v[t], np.float32)).cuda() for k, v in host.items()})
    torch.cuda.synchronize()
    return agent, rows * W


def test_update_call_matches_the_float32_restatement(lib):
    """agent.enqueue_update for 4 iterations with delay_steps = 2 — critic steps on all four, actor steps and the
    polyak update of all targets on iterations 1 and 3 — with indices and eps fed explicitly, against td4_ref.Learner
    in float32 on the CPU: parameter deltas of the actor, both critics and all targets within atol 1e-5, the infos
    within rtol 1e-5 / atol 1e-5 (the bounds of test_gpu_offpolicy.py::test_offpolicy_update_matches_reference).
    The precondition is asserted at every iteration of the reference."""
    iterations, W = 4, 2
    agent, transitions = _filled_agent(seed=6)
    model, B, A = agent.model, agent.replay.batch_size, agent.action_size
    noise = agent.critic_updater.target_action_noise
    stored = {k: agent.replay.buffers[k].cpu() for k in ('observations', 'actions', 'next_observations', 'rewards',
                                                         'discounts')}

    def reference(seed):
        rng = np.random.RandomState(seed)
        indices = rng.randint(transitions, size=(iterations, B))
        eps = rng.normal(size=(iterations, 1, B, A)).astype(np.float32)
        learner = td4_ref.Learner(model, 2, 'ReLU', noise, delay_steps=2, target_coeff=model.target_coeff)
        before, rows, holds = learner.snapshot(), [], True
        for it in range(iterations):
            batch = {k: v[indices[it] // W, indices[it] % W] for k, v in stored.items()}
            out, actor_loss = learner.iteration(it, batch, torch.as_tensor(eps[it, 0]))
            holds = holds and td4_ref.precondition(out, learner.nets.values, B)
            rows.append((float(out['loss']), float(out['q1'].mean()), float(out['q2'].mean()), actor_loss))
        return indices, eps, learner, before, rows, holds
    for seed in range(400):
        indices, eps, learner, before, rows, holds = reference(seed)
        if holds:
            break
    assert holds, 'no seed satisfies the precondition at every iteration'
    start = {name: [p.detach().cpu().numpy().copy() for p in td4_ref.weights(getattr(model, name))]
             for name in td4_ref.NAMES}
    infos = agent.enqueue_update(indices, eps).cpu().numpy()
    np.testing.assert_allclose(infos[0][:, 0], [r[0] for r in rows], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(infos[0][:, 1], [r[1] for r in rows], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(infos[0][:, 2], [r[2] for r in rows], rtol=1e-5, atol=1e-5)
    ran = infos[1][:, 6] > 0
    assert ran.tolist() == [False, True, False, True]
    np.testing.assert_allclose(infos[1][ran, 0], [float(r[3]) for r in rows if r[3] is not None], rtol=1e-5, atol=1e-5)
    after, worst, moved = learner.snapshot(), 0.0, 0.0
    for name in td4_ref.NAMES:
        for i, p in enumerate(td4_ref.weights(getattr(model, name))):
            got = p.detach().cpu().numpy() - start[name][i]
            want = after[name][i] - before[name][i]
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-5, err_msg=f'{name} {i}')
            worst, moved = max(worst, float(np.abs(got - want).max())), max(moved, float(np.abs(want).max()))
    assert moved > 1e-3                                                  # (four Adam steps of 1e-3)
    print(f'td4 update call: largest |delta - reference| {worst:.2e} of deltas up to {moved:.2e}')


# ---------------------------------------------------------------- 7. scheduling, the Buffer, checkpoints

def _loop(monkeypatch, environment):
    import tonic_amd
    import tonic_amd.torch as tt
    for key in ('TONIC_AMD_NO_GRAPH', 'TONIC_AMD_UPDATE_CHUNK'):
        monkeypatch.delenv(key, raising=False)
    for key, value in environment.items():
        monkeypatch.setenv(key, value)
    O, A, W, NA = 6, 2, 2, 21
    replay = tonic_amd.replays.Buffer(size=2000, batch_iterations=4, batch_size=16, steps_before_batches=W * 8,
                                      steps_between_batches=W * 4, return_steps=5)
    agent = tt.agents.TD4(model=_model(tt, True, (32, 32), 'ReLU', (*SUPPORT, NA)), replay=replay,
                          exploration=tonic_amd.explorations.NormalActionNoise(start_steps=W * 5))
    env = tonic_amd.environments.distribute(lambda: tonic_amd.environments.Synthetic(O, A, max_episode_steps=7), 1, W)
    env.initialize(seed=3)
    agent.initialize(env.observation_space, env.action_space, seed=3)
    observations, calls, stored = env.start(), 0, []
    for t in range(18):
        actions = agent.step(observations, t * W)
        observations, infos = env.step(actions)
        # the one-step transition as the agent is given it (copies: the environment's block is written in place)
        stored.append(dict(next_observations=np.array(infos['observations'], np.float32),
                           rewards=np.array(infos['rewards'], np.float32),
                           resets=np.array(infos['resets'], np.float32),
                           terminations=np.array(infos['terminations'], np.float32)))
        had = getattr(agent, 'last_infos', None)
        agent.update(**infos, steps=t * W)
        calls += getattr(agent, 'last_infos', None) is not had
    agent.settle()
    torch.cuda.synchronize()
    assert calls == 3
    return agent, stored, env


def test_scheduling_buffer_and_checkpoints(lib, monkeypatch, tmp_path, golden):
    """The same step / update loop on a synthetic environment of two workers, three update calls of four
    iterations: by default (captured in a hipGraph), launch by launch (TONIC_AMD_NO_GRAPH=1) and with
    TONIC_AMD_UPDATE_CHUNK=0 — parameters, targets, Adam moments and the logged rows are bit-identical.  The Buffer
    holds 5-step returns (a row against the one-step transitions accumulated on the host by buffers.py:58-79);
    save / load round-trips; the state-dict keys are those recorded from the reference's torch TD3 model with the
    value head's layer renamed to the distributional head's, the `critic.*` alias among them."""
    import tonic_amd.torch as tt
    results = {}
    for mode, environment in (('graph', {}), ('launches', {'TONIC_AMD_NO_GRAPH': '1'}),
                              ('unchunked', {'TONIC_AMD_UPDATE_CHUNK': '0'})):
        agent, stored, env = _loop(monkeypatch, environment)
        results[mode] = dict(
            online=agent.model.flat_online.cpu().numpy(), target=agent.model.flat_target.cpu().numpy(),
            critic_m=agent.critic_updater.exp_avg.cpu().numpy(), actor_v=agent.actor_updater.exp_avg_sq.cpu().numpy(),
            infos=np.array(agent.last_infos, copy=True),
            steps=np.array([int(agent.critic_updater.state[0]), int(agent.actor_updater.state[0])]))
        if mode == 'graph':
            assert agent._graph is not None
            kept = agent, stored, env
    assert results['graph']['steps'].tolist() == [12, 6]
    assert np.isfinite(results['graph']['infos']).all() and np.abs(results['graph']['infos'][0][:, 0]).min() > 0
    for mode in ('launches', 'unchunked'):
        for key, want in results['graph'].items():
            assert np.array_equal(results[mode][key], want, equal_nan=True), (mode, key)
    agent, stored, env = kept
    # 5-step returns: row t takes rows t + 1 .. t + 4 while no reset lies in between (buffers.py:58-79)
    buffers = {k: v.cpu().numpy() for k, v in agent.replay.buffers.items()}
    gamma, checked = np.float32(agent.replay.discount_factor), 0
    for t in (0, 3, 7):
        for w in range(2):
            reward = np.float32(stored[t]['rewards'][w])
            discount = np.float32(1 - stored[t]['terminations'][w]) * gamma
            nxt, mask = stored[t]['next_observations'][w], np.float32(1)
            for later in range(t + 1, t + 5):
                mask = mask * np.float32(1 - stored[later - 1]['resets'][w])
                new_reward = reward + discount * np.float32(stored[later]['rewards'][w])
                reward = (1 - mask) * reward + mask * new_reward
                new_discount = discount * (np.float32(1 - stored[later]['terminations'][w]) * gamma)
                discount = (1 - mask) * discount + mask * new_discount
                nxt = (1 - mask) * nxt + mask * stored[later]['next_observations'][w]
            np.testing.assert_allclose(buffers['rewards'][t, w], reward, rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(buffers['discounts'][t, w], discount, rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(buffers['next_observations'][t, w], nxt, rtol=1e-6, atol=1e-7)
            checked += bool(mask)
    assert checked > 0                                   # (some row did take all five steps)
    # checkpoints
    state = {k: v.detach().cpu().numpy().copy() for k, v in agent.model.state_dict().items()}
    recorded = golden('reference_dropin')
    td3 = {k[len('state/TD3/'):] for k in recorded.files if k.startswith('state/TD3/')}
    assert any(k.startswith('critic.') for k in td3)
    assert set(state) == {k.replace('head.v_layer', 'head.distributional_layer') for k in td3}
    path = str(tmp_path / 'agent')
    agent.save(path)
    other = tt.agents.TD4(model=_model(tt, True, (32, 32), 'ReLU', (*SUPPORT, 21)))
    other.initialize(env.observation_space, env.action_space, seed=11)
    other.load(path)
    loaded = other.model.state_dict()
    assert sorted(loaded) == sorted(state)
    for key, value in state.items():
        assert np.array_equal(loaded[key].detach().cpu().numpy(), value), key
