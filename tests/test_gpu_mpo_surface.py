"""GPU tests of MPO's constructor surface on the HIP entries: the joint KL constraint (per_dim_constraining=False,
`joint_kl` of the tonic_mpo_*_joint entries), 1 .. 256 samples per state (the E-step's register slots) and different
sample counts in ExpectedSARSA and the actor step.

1. the joint constraint against the float64 restatement (tests/mpo_surface_reference.py, held to the unmodified
   reference in tests/test_mpo_surface_host.py), under the stress and the bounds of test_gpu_offpolicy_grads;
2. invariants without tolerance: A = 1 (both constraints are one), replicated alphas at A = 6, and joint_kl = 0
   through the new entries against the entries that were there before;
3. 65 .. 256 samples against float64, for both constraints and for ExpectedSARSA; 257 refused with the bound;
4. the sharded form under the joint constraint at 100 samples;
5. the agent with (3, 7) samples against the split entries by hand, its graph replayed and re-captured;
6. the first update of the unmodified reference (tests/golden/mpo_surface_small.npz).

Every float64 test prints the largest relative error it saw."""
import numpy as np
import pytest

from mpo_surface_reference import mpo_reference
from test_gpu_offpolicy_grads import MPO_TORSOS, _agent, _check, _check_stat, _f64, _mpo_call, _mpo_setup
from test_gpu_offpolicy_grads import test_expected_sarsa_grads_vs_float64 as _expected_sarsa_vs_float64
from test_gpu_offpolicy_torsos import _grad_sums

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

TONIC_ERR_INVALID_ARGUMENT = -1


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def _duals(K):
    """The stress of _mpo_setup for K constraints: a cold temperature, duals below the floor."""
    return np.concatenate([[-5.0], np.where(np.arange(K) % 2, -25.0, 1.0), np.where(np.arange(K) % 2, 10.0, -30.0),
                           [-20.0]]).astype(np.float32)


def _call(lib, agent, u, duals, obs, eps, joint, shard=None):
    """`_mpo_call` of test_gpu_offpolicy_grads on the *_joint entries: (gradient sums + slot, dual gradients + slot,
    statistics, the duals as the call left them)."""
    from tonic_amd import _lib
    p, m, A, S = _lib.ptr, agent.model, u.action_size, u.num_samples
    B, K = obs.shape[0], len(duals) // 2 - 1
    assert K == (1 if joint else A)
    mean, std = u.norm_tensors()
    d_duals = torch.as_tensor(duals).cuda()
    grads = torch.zeros(u.count + 8, device='cuda')
    dual_grads = torch.zeros(2 * K + 2 + 8, device='cuda')
    stats = torch.zeros(9 + 2 * K, device='cuda')
    obs, eps = obs.cuda(), eps.cuda().view(S, B, A)
    rest = (float(u.epsilon), float(u.epsilon_penalty), float(u.epsilon_mean), float(u.epsilon_std),
            int(bool(u.action_penalization)), int(joint))
    if shard is None:
        ws = u._offpolicy_workspace(B)
        _lib.check(lib.tonic_mpo_actor_grad_joint(
            p(m.flat_actor.flat), p(m.flat_target_actor.flat), p(m.flat_target_critics.flat), p(d_duals),
            float(u.min_log_dual), p(mean), p(std), u.norm_clip(), p(obs), p(eps.reshape(S * B, A)), p(grads),
            p(dual_grads), p(stats), B, u.observation_size, u.hidden, A, S, *rest, p(ws), ws.numel(),
            _lib.current_stream()), 'tonic_mpo_actor_grad_joint')
    else:
        columns = torch.zeros(6 + 2 * A, dtype=torch.float64, device='cuda')
        bounds = np.linspace(0, B, shard + 1).astype(int)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            part = torch.zeros(u.count + 8, device='cuda')
            cols = torch.zeros(6 + 2 * A, dtype=torch.float64, device='cuda')
            o, e = obs[lo:hi].contiguous(), eps[:, lo:hi].reshape(S * (hi - lo), A).contiguous()
            ws = u._offpolicy_workspace(hi - lo)
            _lib.check(lib.tonic_mpo_actor_grad_shard_joint(
                p(m.flat_actor.flat), p(m.flat_target_actor.flat), p(m.flat_target_critics.flat), p(d_duals),
                float(u.min_log_dual), p(mean), p(std), u.norm_clip(), p(o), p(e), p(part), p(cols), hi - lo,
                u.observation_size, u.hidden, A, S, int(bool(u.action_penalization)), int(joint), p(ws), ws.numel(),
                _lib.current_stream()), 'tonic_mpo_actor_grad_shard_joint')
            torch.cuda.synchronize()
            grads[:u.count] += part[:u.count]
            columns += cols
        _lib.check(lib.tonic_mpo_dual_step_joint(
            p(columns), p(d_duals), float(u.min_log_dual), p(dual_grads), p(stats), p(grads[u.count:]), B, B, A, S,
            *rest, _lib.current_stream()), 'tonic_mpo_dual_step_joint')
    torch.cuda.synchronize()
    return (grads.cpu().numpy(), dual_grads.cpu().numpy(), stats.cpu().numpy(), d_duals.cpu().numpy())


def _compare(agent, u, got, duals, obs, eps, ref, label, joint):
    """`_mpo_compare` of test_gpu_offpolicy_grads with K constraints in place of A: the same checks, the same
    bounds."""
    grads, dual_grads, stats, written = got
    m, A, S, B = agent.model, u.action_size, u.num_samples, obs.shape[0]
    K = 1 if joint else A
    actor, target_actor, frozen = _f64(m.actor), _f64(m.target_actor), _f64(m.target_critic)
    penal = bool(u.action_penalization)
    leaves, want_stats, actor_loss, floored, actions, temperature_scale, tempering = mpo_reference(
        ref, actor, target_actor, frozen, obs.double(), eps.double(), duals, u.min_log_dual, u, S, penal, not joint)
    outside = (actions.abs() > 1).double().mean()
    assert 0 < outside < 1, float(outside)                       # the penalty weights are not uniform
    # (the E-step weights are softmax_s(Q / T) of float32 Q values: see _mpo_compare)
    bound = max(1e-5, 64 * 2.0 ** -24 * tempering)
    err = _check(_grad_sums([m.actor], torch.as_tensor(grads), B), actor, [f'actor {i}' for i in range(len(actor))],
                 bound)
    names = ('log_temperature', 'log_alpha_mean', 'log_alpha_std', 'log_penalty_temperature')
    groups = [np.s_[:1], np.s_[1:1 + K], np.s_[1 + K:1 + 2 * K], np.s_[1 + 2 * K:2 * K + 2]]
    dual_err = 0.0
    for name, leaf, at in zip(names, leaves, groups):
        if name == 'log_penalty_temperature' and not penal:
            assert dual_grads[at][0] == 0.0
            continue
        if name in ('log_temperature', 'log_penalty_temperature'):
            epsilon = u.epsilon if name == 'log_temperature' else u.epsilon_penalty
            want = float(leaf.grad[0])
            scale = max(abs(want), float(torch.sigmoid(leaf.detach()[0])) * (abs(epsilon) + np.log(S)))
            assert abs(float(dual_grads[at][0]) - want) <= 1e-5 * scale, (name, float(dual_grads[at][0]), want)
            dual_err = max(dual_err, abs(float(dual_grads[at][0]) - want) / max(abs(want), 1e-30))
            continue
        dual_err = max(dual_err, _check([torch.as_tensor(dual_grads[at])], [leaf], [name]))
    assert dual_grads[2 * K + 2 + 5] == 1.0, dual_grads[2 * K + 2:]
    want_written = floored.astype(np.float32)
    if not penal:
        want_written[-1] = duals[-1]
    assert np.array_equal(written, want_written), (written, want_written)
    assert grads[u.count + 5] == B, grads[u.count:]
    _check_stat(grads[u.count] / B, actor_loss, None, 'actor loss slot')
    n = 8 + 2 * K + (1 if penal else 0)
    stat_err = max(_check_stat(stats[i], want_stats[i], torch.tensor([temperature_scale]) if i == 6 else None,
                               f'stat {i}') for i in range(n))
    print(f'mpo surface {label}: largest relative error actor {err:.2e} (bound {bound:.1e}) duals {dual_err:.2e} '
          f'stats {stat_err:.2e}')


# ---------------------------------------------------------------- 1. the joint constraint against float64

@pytest.mark.parametrize('torso', ['plain', 'elu3'])
@pytest.mark.parametrize('A', [1, 6, 64])
@pytest.mark.parametrize('B', [37, 256])
@pytest.mark.parametrize('penalization', [True, False])
def test_joint_kl_vs_float64(lib, torso, A, B, penalization):
    """tonic_mpo_actor_grad_joint with joint_kl = 1 against float64 of actors.py:318-464 with
    per_dim_constraining=False, under the stress of test_mpo_actor_grads_vs_float64."""
    agent, u, _, obs, eps, ref = _mpo_setup(lib, A, B, torso, penalization, -18.0)
    duals = _duals(1)
    got = _call(lib, agent, u, duals, obs, eps, joint=True)
    _compare(agent, u, got, duals, obs, eps, ref, f'joint {torso} A={A} B={B} penalization={penalization}', True)


def test_joint_kl_with_a_raised_dual_floor(lib):
    """min_log_dual = -3: the temperatures and one alpha sit on the floor, read through it and written back."""
    agent, u, _, obs, eps, ref = _mpo_setup(lib, 6, 100, 'plain', True, -3.0)
    duals = _duals(1)
    got = _call(lib, agent, u, duals, obs, eps, joint=True)
    assert (got[3] == np.float32(-3.0)).sum() == 3
    _compare(agent, u, got, duals, obs, eps, ref, 'joint floor -3', True)


# ---------------------------------------------------------------- 2. invariants, bit for bit

def _equal(a, b, what):
    for x, y, name in zip(a, b, ('gradient sums', 'dual gradients', 'statistics', 'written duals')):
        assert np.array_equal(x, y), (what, name, np.abs(x - y).max())


@pytest.mark.parametrize('penalization', [True, False])
def test_one_action_dimension_makes_the_two_constraints_one(lib, penalization):
    agent, u, duals, obs, eps, _ = _mpo_setup(lib, 1, 37, 'plain', penalization, -18.0)
    assert len(duals) == 4
    _equal(_call(lib, agent, u, duals, obs, eps, joint=True), _call(lib, agent, u, duals, obs, eps, joint=False),
           'A = 1')


def test_joint_gradients_equal_per_dimension_ones_with_replicated_alphas(lib):
    """The actor's gradient sums read the alphas only as factors of each dimension's KL gradient: the joint call
    equals the per-dimension call whose alpha_mean[a] / alpha_std[a] are the joint values."""
    A = 6
    agent, u, _, obs, eps, _ = _mpo_setup(lib, A, 37, 'plain', True, -18.0)
    for alpha_mean, alpha_std in ((1.0, -30.0), (-0.4, 2.5)):
        joint = np.array([-5.0, alpha_mean, alpha_std, -20.0], np.float32)
        per_dim = np.concatenate([[-5.0], [alpha_mean] * A, [alpha_std] * A, [-20.0]]).astype(np.float32)
        a, b = _call(lib, agent, u, joint, obs, eps, joint=True), _call(lib, agent, u, per_dim, obs, eps, joint=False)
        assert np.array_equal(a[0][:u.count], b[0][:u.count])
        assert a[0][u.count + 5] == b[0][u.count + 5] == obs.shape[0]


@pytest.mark.parametrize('S', [1, 20, 64])
@pytest.mark.parametrize('torso', ['plain', 'elu3'])
def test_joint_kl_zero_is_the_entries_that_were(lib, S, torso):
    """joint_kl = 0 through tonic_mpo_actor_grad_joint / _shard_joint / tonic_mpo_dual_step_joint against
    tonic_mpo_actor_grad / _shard / tonic_mpo_dual_step: every output, the single call and the sharded form."""
    agent, u, duals, obs, eps, _ = _mpo_setup(lib, 6, 37, torso, True, -18.0, S=S)
    _equal(_call(lib, agent, u, duals, obs, eps, joint=False), _mpo_call(lib, agent, u, duals, obs, eps), 'single')
    _equal(_call(lib, agent, u, duals, obs, eps, joint=False, shard=2),
           _mpo_call(lib, agent, u, duals, obs, eps, shard=2), 'sharded')


# ---------------------------------------------------------------- 3. more than one sample per lane

@pytest.mark.parametrize('joint', [False, True])
@pytest.mark.parametrize('S,B', [(65, 37), (100, 37), (128, 37), (129, 37), (256, 37), (100, 256)])
def test_sample_counts_beyond_a_wave_vs_float64(lib, S, B, joint):
    """Two to four register slots per lane in the E-step (65: one sample in the second slot; 128 / 129: the edge of
    the third; 256: all four full) against float64, both constraints.  S * B is no multiple of 16 at B = 37 with an
    odd S: the tiled rows end inside a padded block."""
    A = 6
    agent, u, duals, obs, eps, ref = _mpo_setup(lib, A, B, 'plain', True, -18.0, S=S)
    if joint:
        duals = _duals(1)
    got = _call(lib, agent, u, duals, obs, eps, joint=joint)
    _compare(agent, u, got, duals, obs, eps, ref, f'S={S} B={B} joint={joint}', joint)


@pytest.mark.parametrize('S', [65, 256])
def test_expected_sarsa_beyond_a_wave_vs_float64(lib, S):
    _expected_sarsa_vs_float64(lib, 'plain', S)


def test_257_samples_are_refused_with_the_bound(lib):
    from tonic_amd import _lib
    A, B, S = 6, 37, 256
    agent, u, duals, obs, eps, _ = _mpo_setup(lib, A, B, 'elu3', True, -18.0, S=S)
    p, m = _lib.ptr, agent.model
    mean, std = u.norm_tensors()
    ws = u._offpolicy_workspace(B)
    d_duals, obs, eps = torch.as_tensor(duals).cuda(), obs.cuda(), eps.cuda()
    grads, dual_grads = torch.zeros(u.count + 8, device='cuda'), torch.zeros(2 * A + 2 + 8, device='cuda')
    stats, columns = torch.zeros(9 + 2 * A, device='cuda'), torch.zeros(6 + 2 * A, dtype=torch.float64, device='cuda')
    front = (p(m.flat_actor.flat), p(m.flat_target_actor.flat), p(m.flat_target_critics.flat), p(d_duals),
             float(u.min_log_dual), p(mean), p(std), u.norm_clip(), p(obs), p(eps), p(grads))
    epsilons = (float(u.epsilon), float(u.epsilon_penalty), float(u.epsilon_mean), float(u.epsilon_std))
    tail = (p(ws), ws.numel(), _lib.current_stream())
    c = agent.critic_updater
    batch = {k: torch.zeros(B, n, device='cuda') if n else torch.zeros(B, device='cuda')
             for k, n in (('actions', A), ('rewards', 0), ('discounts', 0))}
    cws = c._offpolicy_workspace(B)
    calls = {
        'tonic_mpo_actor_grad': lambda S: lib.tonic_mpo_actor_grad(
            *front, p(dual_grads), p(stats), B, u.observation_size, u.hidden, A, S, *epsilons, 1, *tail),
        'tonic_mpo_actor_grad_joint': lambda S: lib.tonic_mpo_actor_grad_joint(
            *front, p(dual_grads), p(stats), B, u.observation_size, u.hidden, A, S, *epsilons, 1, 0, *tail),
        'tonic_mpo_actor_grad_shard': lambda S: lib.tonic_mpo_actor_grad_shard(
            *front, p(columns), B, u.observation_size, u.hidden, A, S, 1, *tail),
        'tonic_mpo_dual_step': lambda S: lib.tonic_mpo_dual_step(
            p(columns), p(d_duals), float(u.min_log_dual), p(dual_grads), p(stats), p(grads[u.count:]), B, B, A, S,
            *epsilons, 1, _lib.current_stream()),
        'tonic_expected_sarsa_grad': lambda S: lib.tonic_expected_sarsa_grad(
            p(m.flat_target_actor.flat), p(m.flat_target_critics.flat), p(c.flat.flat), p(mean), p(std),
            c.norm_clip(), p(obs), p(batch['actions']), p(obs), p(batch['rewards']), p(batch['discounts']), p(eps),
            p(c.grad_sums), B, c.observation_size, c.hidden, A, S, p(cws), cws.numel(), _lib.current_stream()),
    }
    for name, call in calls.items():
        for refused in (257, 0):
            assert call(refused) == TONIC_ERR_INVALID_ARGUMENT, (name, refused)
            assert b'256' in lib.tonic_last_error(), (name, lib.tonic_last_error())
        assert call(256) == 0, (name, lib.tonic_last_error())
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. the sharded form

def test_joint_sharded_step_equals_the_single_call(lib):
    """The batch in two halves through tonic_mpo_actor_grad_shard_joint and tonic_mpo_dual_step_joint with
    joint_kl = 1 at 100 samples: the criterion of test_mpo_sharded_step_equals_the_single_call."""
    agent, u, _, obs, eps, ref = _mpo_setup(lib, 6, 74, 'plain', True, -18.0, S=100)
    duals = _duals(1)
    single = _call(lib, agent, u, duals, obs, eps, joint=True)
    sharded = _call(lib, agent, u, duals, obs, eps, joint=True, shard=2)
    np.testing.assert_allclose(sharded[1][:4], single[1][:4], rtol=1e-6, atol=0)
    np.testing.assert_allclose(sharded[2], single[2], rtol=1e-6, atol=0)
    assert np.array_equal(sharded[3], single[3])
    assert sharded[0][u.count + 5] == single[0][u.count + 5] == obs.shape[0]
    _compare(agent, u, sharded, duals, obs, eps, ref, 'joint sharded S=100', True)


# ---------------------------------------------------------------- 5. two sample counts through the agent

def _store_rows(agent, first, rows):
    """Time rows first .. first + rows - 1 of one fixed stream of transitions (4 workers) into the agent's replay."""
    O, A, W = agent.observation_size, agent.action_size, 4
    for t in range(first, first + rows):
        rng = np.random.RandomState(1000 + t)
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, (W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        agent.replay.store(normalizer=agent.model.observation_normalizer,
                           **{k: torch.as_tensor(np.asarray(v, np.float32), device='cuda') for k, v in row.items()})


def _filled_agent(S_c, S_a, B, iterations):
    sizes, activation = MPO_TORSOS['elu3']
    agent = _agent('mpo', 17, 6, B, sizes=sizes, activation=activation, S=S_a, per_dim_constraining=False)
    agent.critic_updater.num_samples = S_c
    agent.replay.batch_iterations = iterations
    _store_rows(agent, 0, 40)
    return agent


def _update_by_hand(agent):
    """MPO._update on the split entries: the replay's index stream, the reference's order of draws
    (critics.py:260, then actors.py:359, per iteration), one enqueue per updater and iteration."""
    import tonic_amd.torch as tt
    critic, actor, model, replay = agent.critic_updater, agent.actor_updater, agent.model, agent.replay
    B, A = replay.batch_size, agent.action_size
    indices = replay.sample_indices()
    iterations = indices.shape[0]
    eps = [(torch.randn(critic.num_samples, B, A), torch.randn(actor.num_samples, B, A)) for _ in range(iterations)]
    batches = {k: v.clone() for k, v in replay.gather_many(torch.as_tensor(indices).cuda()).items()}
    infos = torch.zeros(2, iterations, tt.updaters.INFO_WIDTH, device='cuda')
    stats = torch.zeros(iterations, agent.actor_updater.mpo_stats.numel(), device='cuda')
    for it in range(iterations):
        batch = {k: v[it] for k, v in batches.items()}
        critic.enqueue(batch, eps[it][0].reshape(-1, A).cuda(), infos[0, it])
        actor.enqueue(batch['observations'], eps[it][1].reshape(-1, A).cuda(), infos[1, it],
                      targets=(model.flat_target, model.flat_online, 0, model.target_coeff), stats_row=stats[it])
    torch.cuda.synchronize()
    model.observation_normalizer.update()
    return infos.cpu().numpy(), stats.cpu().numpy()


def _same_state(a, b, what):
    for (key, x), y in zip(a.model.state_dict().items(), b.model.state_dict().values()):
        assert torch.equal(x, y), (what, key)
    assert torch.equal(a.actor_updater.duals, b.actor_updater.duals), what
    assert a.actor_updater.duals.numel() == 4


def test_agent_with_two_sample_counts_equals_the_split_entries_by_hand(lib):
    """ExpectedSARSA(num_samples=3) beside MaximumAPosterioriPolicyOptimization(num_samples=7,
    per_dim_constraining=False), B = 24, two iterations per update: parameters, duals and infos after agent._update
    equal those of the split entries called by hand on the same indices and noise rows; a second update replays
    the captured graph; (7, 3) re-captures and still matches."""
    B, iterations = 24, 2
    agent, hand = _filled_agent(3, 7, B, iterations), _filled_agent(3, 7, B, iterations)
    _same_state(agent, hand, 'initial')
    graphs = []
    for update, samples in enumerate([(3, 7), (3, 7), (7, 3)]):
        for one in (agent, hand):
            one.critic_updater.num_samples, one.actor_updater.num_samples = samples
            _store_rows(one, 40 + update, 1)       # (the normaliser's update at the end needs a new row)
        torch.manual_seed(40 + update)
        agent._update(steps=update)
        torch.manual_seed(40 + update)
        infos, stats = _update_by_hand(hand)
        assert agent._static_eps.shape == (iterations, 2, 7 * B, agent.action_size)
        assert np.array_equal(agent.last_infos, infos), update
        assert np.array_equal(agent.last_actor_infos, stats), update
        assert agent.last_actor_infos.shape == (iterations, 11) and np.isfinite(stats).all()
        _same_state(agent, hand, update)
        assert agent._graph is not None
        graphs.append(agent._graph)
    assert graphs[1] is graphs[0]               # the same counts: replayed
    assert graphs[2] is not graphs[1]           # (7, 3): the same noise block's shape, another graph


# ---------------------------------------------------------------- 6. the reference's first update

@pytest.mark.parametrize('case', ['a', 'b', 'c'])
def test_first_update_matches_the_reference(lib, golden, case):
    """One ExpectedSARSA step, one MPO actor / dual step and the target update of the unmodified reference
    (scripts/make_mpo_surface_golden.py) on the HIP entries, within the tolerances test_gpu_offpolicy.py holds
    mpo_small to: (a) the joint constraint at 4 samples, (b) joint at (3, 7), (c) per-dimension at 100."""
    import tonic_amd.torch as tt
    g = golden('mpo_surface_small')
    O, A, B, _ = (int(v) for v in g['cfg'])
    per_dim, (S_c, S_a) = bool(g[case + '/per_dim_constraining']), (int(v) for v in g[case + '/samples'])
    K = A if per_dim else 1
    initial = {k[len('duals/'):]: float(g[k]) for k in g.files if k.startswith('duals/')}
    agent = _agent('mpo', O, A, B, sizes=tuple(int(v) for v in g['torso_sizes']), activation='ReLU', S=S_a,
                   per_dim_constraining=per_dim, **initial)
    critic, actor, model = agent.critic_updater, agent.actor_updater, agent.model
    critic.num_samples = S_c
    state = {}
    for key in model.state_dict():         # (a target tensor that is not stored equals its online twin)
        stored = 'pre/' + key if 'pre/' + key in g.files else 'pre/' + key[len('target_'):]
        state[key] = torch.as_tensor(g[stored])
    model.load_state_dict(state)
    before = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    duals_before = actor.duals.cpu().numpy()
    assert np.array_equal(duals_before, g[case + '/duals_before'])
    batch = {k[len('batch/'):]: torch.as_tensor(g[k]).cuda() for k in g.files if k.startswith('batch/')}
    infos = torch.zeros(2, tt.updaters.INFO_WIDTH, device='cuda')
    stats = torch.zeros(9 + 2 * K, device='cuda')
    critic.enqueue(batch, torch.as_tensor(g[case + '/eps_critic']).cuda(), infos[0])
    actor.enqueue(batch['observations'], torch.as_tensor(g[case + '/eps_actor']).cuda(), infos[1],
                  targets=(model.flat_target, model.flat_online, 0, model.target_coeff), stats_row=stats)
    torch.cuda.synchronize()
    infos = infos.cpu().numpy()
    np.testing.assert_allclose(infos[0, 0], g[case + '/info/critic/loss'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(infos[0, 1], g[case + '/info/critic/q_mean'], rtol=1e-5, atol=1e-5)
    logged = actor.infos(stats.cpu().numpy())
    assert sorted(logged) == sorted(k[len(case + '/info/actor/'):] for k in g.files
                                    if k.startswith(case + '/info/actor/'))
    for key in tt.updaters.MPO_INFO:
        np.testing.assert_allclose(logged[key], np.asarray(g[f'{case}/info/actor/{key}']).reshape(()), rtol=2e-5,
                                   atol=2e-6, err_msg=key)
    for key in ('alpha_mean', 'alpha_std'):
        assert logged[key].shape == g[f'{case}/info/actor/{key}'].shape == (K,), key
        np.testing.assert_allclose(logged[key], g[f'{case}/info/actor/{key}'], rtol=1e-5, err_msg=key)
    np.testing.assert_allclose(logged['penalty_temperature'], g[case + '/info/actor/penalty_temperature'][0],
                               rtol=1e-5)
    after, at = model.state_dict(), 0
    for key in (str(k) for k in g['post_keys']):
        n = before[key].size
        want = g[case + '/post'][at:at + n].reshape(before[key].shape) - before[key]
        at += n
        np.testing.assert_allclose(after[key].detach().cpu().numpy() - before[key], want, rtol=0, atol=1e-5,
                                   err_msg=key)
        assert np.abs(want).max() > 0, key
    assert at == g[case + '/post'].size
    np.testing.assert_allclose(actor.duals.cpu().numpy() - duals_before,
                               g[case + '/duals_after'] - g[case + '/duals_before'], rtol=0, atol=1e-5)
