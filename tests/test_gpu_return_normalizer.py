"""The Return normaliser on the device: the *_ranged critic entries (squashed value head) against float64
autograd, their NULL-range form against the plain entries, tonic_reward_range against NumPy, and the
on-policy agents (A2C, PPO, TRPO) with ActorCritic(..., return_normalizer=Return(0.99)) against the
reference's runs (tests/golden/*_return_small.npz, scripts/make_return_goldens.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, 'tests', 'mp_return_worker.py')


@pytest.fixture(scope='module')
def lib():
    import tonic_amd  # noqa: F401
    from tonic_amd import _lib
    return _lib.load()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _critic(O, sizes, activation, seed):
    from tonic_amd.environments import Box
    from tonic_amd.torch import models
    torch.manual_seed(seed)
    critic = models.Critic(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, activation),
                           head=models.ValueHead())
    critic.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (1,)))
    return critic


class _Case:
    """A critic's flat block on the device, inputs, and the entries that serve its torso."""

    def __init__(self, lib, O, n, sizes=(64, 64), activation=torch.nn.Tanh, seed=0, bias=None, scale=1.0):
        from tonic_amd.torch import models, updaters
        self.lib, self.O, self.n = lib, O, n
        self.critic = _critic(O, sizes, activation, seed)
        if bias is not None:                      # a saturated head: z = bias for every sample
            with torch.no_grad():
                self.critic.head.v_layer.weight.zero_()
                self.critic.head.v_layer.bias.fill_(bias)
        self.flat = models.FlatNetwork(self.critic, 'cuda')
        rng = np.random.RandomState(seed + 1)
        self.obs = torch.as_tensor(rng.normal(size=(n, O)).astype(np.float32), device='cuda')
        self.ret = torch.as_tensor((rng.normal(size=n) * scale).astype(np.float32), device='cuda')
        self.mean = torch.zeros(O, device='cuda')
        self.std = torch.ones(O, device='cuda')
        torso = self.critic.torso
        self.torso = None if updaters.fused_ppo_torso(torso) else updaters.hip_ppo_torso(torso)
        assert updaters.fused_ppo_torso(torso) or self.torso is not None
        if self.torso is None:
            need = lib.tonic_ppo_workspace_bytes(n, O, 1, 0)
        else:
            need = lib.tonic_ppo_torso_workspace_bytes(n, O, 1, 0, self.torso[0], self.torso[1])
        self.ws = torch.zeros(max(int(need), 16), dtype=torch.uint8, device='cuda')
        self.P = self.flat.count

    def values(self, rng_pair, ranged=True):
        from tonic_amd import _lib
        out = torch.full((self.n,), -7.0, device='cuda')
        low, high = (None, None) if rng_pair is None else (_ptr(rng_pair[0]), _ptr(rng_pair[1]))
        common = (_ptr(self.flat.flat), _ptr(self.mean), _ptr(self.std), 0.0, _ptr(self.obs), _ptr(out),
                  self.n, self.O)
        if self.torso is not None:
            if ranged:
                rc = self.lib.tonic_value_forward_torso_ranged(*self.torso, *common, _ptr(self.ws), self.ws.numel(),
                                                               low, high, None)
            else:
                rc = self.lib.tonic_value_forward_torso(*self.torso, *common, _ptr(self.ws), self.ws.numel(), None)
        elif ranged:
            rc = self.lib.tonic_value_forward_wide_ranged(*common, _ptr(self.ws), self.ws.numel(), low, high, None)
        else:
            rc = self.lib.tonic_value_forward_wide(*common, _ptr(self.ws), self.ws.numel(), None)
        _lib.check(rc, 'value forward')
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def narrow_values(self, rng_pair, ranged=True):
        from tonic_amd import _lib
        out = torch.full((self.n,), -7.0, device='cuda')
        common = (_ptr(self.flat.flat), _ptr(self.mean), _ptr(self.std), 0.0, _ptr(self.obs), _ptr(out),
                  self.n, self.O)
        if ranged:
            low, high = (None, None) if rng_pair is None else (_ptr(rng_pair[0]), _ptr(rng_pair[1]))
            _lib.check(self.lib.tonic_value_forward_ranged(*common, low, high, None), 'forward')
        else:
            _lib.check(self.lib.tonic_value_forward(*common, None), 'forward')
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def grads(self, rng_pair, ranged=True):
        from tonic_amd import _lib
        sums = torch.full((self.P + 8,), 3.0, device='cuda')
        low, high = (None, None) if rng_pair is None else (_ptr(rng_pair[0]), _ptr(rng_pair[1]))
        common = (_ptr(self.flat.flat), _ptr(self.mean), _ptr(self.std), 0.0, _ptr(self.obs), _ptr(self.ret),
                  _ptr(sums), self.n, self.O)
        if self.torso is not None:
            if ranged:
                rc = self.lib.tonic_value_regression_grad_torso_ranged(
                    *self.torso, *common, _ptr(self.ws), self.ws.numel(), low, high, None)
            else:
                rc = self.lib.tonic_value_regression_grad_torso(*self.torso, *common, _ptr(self.ws),
                                                                self.ws.numel(), None)
        elif ranged:
            rc = self.lib.tonic_value_regression_grad_ranged(*common, 0, _ptr(self.ws), self.ws.numel(), low, high,
                                                             None)
        else:
            rc = self.lib.tonic_value_regression_grad(*common, 0, _ptr(self.ws), self.ws.numel(), None)
        _lib.check(rc, 'value regression grad')
        torch.cuda.synchronize()
        return sums.cpu().numpy()

    def reference(self, low, high, dtype=torch.float64):
        """autograd of sum((low + sigmoid(z) (high - low) - ret)^2) over the batch (float64; float32 is what
        the reference computes where the two differ by more than rounding: a saturated sigmoid)."""
        critic = _critic(self.O, tuple(self.critic.torso.sizes), self.critic.torso.activation, 0).to(dtype)
        critic.load_state_dict({k: v.detach().to(dtype).cpu() for k, v in self.critic.state_dict().items()})
        obs = self.obs.to(dtype).cpu()
        z = critic.head.v_layer(critic.torso(obs)).squeeze(-1)
        low, high = torch.tensor(float(low), dtype=dtype), torch.tensor(float(high), dtype=dtype)
        v = low + torch.sigmoid(z) * (high - low)
        loss = ((v - self.ret.to(dtype).cpu()) ** 2).sum()
        params = [p for name, p in critic.named_parameters() if 'normalizer' not in name]
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        flat = torch.cat([g.reshape(-1) for g in grads]).double().numpy()
        v = v.detach().double()
        return v.numpy(), flat, float(loss.detach()), float(v.sum())


def _pair(low, high):
    return (torch.tensor(low, dtype=torch.float32, device='cuda'),
            torch.tensor(high, dtype=torch.float32, device='cuda'))


def _check_against_reference(case, low, high, forward=None, dtype=torch.float64):
    forward = forward or case.values
    want_v, want_g, want_loss, want_vsum = case.reference(low, high, dtype)
    got_v = forward(_pair(low, high))
    scale = max(1.0, float(np.abs(want_v).max()))
    np.testing.assert_allclose(got_v, want_v, rtol=0, atol=2e-5 * scale)
    got = case.grads(_pair(low, high))
    g = got[:case.P]
    gmax = float(np.abs(want_g).max())
    assert np.abs(g - want_g).max() <= 2e-3 * gmax + 1e-6, (np.abs(g - want_g).max(), gmax)
    np.testing.assert_allclose(got[case.P], want_loss, rtol=2e-4)          # squared-error sum of the squashed v
    np.testing.assert_allclose(got[case.P + 1], want_vsum, rtol=2e-4, atol=1e-3 * scale)
    assert got[case.P + 5] == case.n


@pytest.mark.parametrize('O,n,sizes,activation', [
    (17, 3000, (64, 64), torch.nn.Tanh),             # per-step forward kernel
    (17, 40000, (64, 64), torch.nn.Tanh),            # the values16 form (n >= 32 768)
    (5, 700, (64, 64), torch.nn.Tanh),
    (111, 2000, (64, 64), torch.nn.Tanh),            # layer by layer (O > 32)
    (11, 1500, (96, 48, 32), torch.nn.Tanh),         # the tonic_*_torso entries
    (17, 1200, (256, 256), torch.nn.ReLU),
])
def test_ranged_entries_against_float64(lib, O, n, sizes, activation):
    case = _Case(lib, O, n, sizes, activation, seed=O + n, scale=30.0)
    for low, high in ((-100.0, 100.0), (-35.5, 2.25), (-3185.4, 100.0)):
        _check_against_reference(case, low, high)
    if case.torso is None and O <= 32:
        _check_against_reference(case, -35.5, 2.25, forward=case.narrow_values)


@pytest.mark.parametrize('bias', [30.0, -30.0, 100.0, -100.0])
def test_saturated_heads(lib, bias):
    for O in (17, 111):
        case = _Case(lib, O, 2048, seed=7, bias=bias, scale=50.0)
        # (float32: sigmoid(30) is 1 there, and so is the gradient of the reference's saturated head 0)
        _check_against_reference(case, -100.0, 100.0, dtype=torch.float32)


def test_wide_range_in_the_fp16x2_kernel(lib):
    """t = high - low = 2e4: the fp16x2 backward's unit must bound |err t s (1 - s)|, not |err|."""
    for n in (4096, 40000):
        case = _Case(lib, 17, n, seed=11, scale=8000.0)
        with torch.no_grad():                     # |z| of a few units (the weights are views of the flat block)
            case.critic.head.v_layer.weight.mul_(4.0)
        _check_against_reference(case, -1e4, 1e4)
        got = case.grads(_pair(-1e4, 1e4))
        assert np.isfinite(got).all()


def test_infinite_range_gives_the_reference_nan(lib):
    for O in (17, 111):
        case = _Case(lib, O, 1000, seed=3)
        for low, high in ((-np.inf, np.inf), (-np.inf, 5.0), (-5.0, np.inf)):
            want_v, _, _, _ = case.reference(low, high)
            got_v = case.values(_pair(low, high))
            assert np.array_equal(np.isnan(got_v), np.isnan(want_v)), (low, high)
            np.testing.assert_array_equal(got_v[~np.isnan(want_v)], want_v[~np.isnan(want_v)])
            _, want_g, want_loss, _ = case.reference(low, high)
            got = case.grads(_pair(low, high))
            # an infinite error: the reference's loss is inf (-5, inf) or NaN, its gradient NaN; the kernels'
            # statistic is not finite either (the fp16x2 kernel's is NaN: the unit of an infinite bound)
            assert not np.isfinite(want_loss) and not np.isfinite(got[case.P]), (low, high, got[case.P])
            assert np.isnan(want_g).any() and np.isnan(got[:case.P]).any()


@pytest.mark.parametrize('O,n,sizes,activation', [
    (17, 3000, (64, 64), torch.nn.Tanh), (17, 40000, (64, 64), torch.nn.Tanh),
    (111, 2000, (64, 64), torch.nn.Tanh), (11, 1500, (96, 48, 32), torch.nn.Tanh),
])
def test_null_range_is_the_plain_entry(lib, O, n, sizes, activation):
    case = _Case(lib, O, n, sizes, activation, seed=2)
    assert np.array_equal(case.values(None), case.values(None, ranged=False))
    assert np.array_equal(case.grads(None), case.grads(None, ranged=False))
    if case.torso is None and O <= 32:
        assert np.array_equal(case.narrow_values(None), case.narrow_values(None, ranged=False))
    one = torch.zeros((), device='cuda')
    from tonic_amd import _lib
    with pytest.raises(_lib.TonicHipError):
        _lib.check(lib.tonic_value_forward_ranged(_ptr(case.flat.flat), _ptr(case.mean), _ptr(case.std), 0.0,
                                                  _ptr(case.obs), _ptr(case.obs), n, O, _ptr(one), None, None),
                   'one range pointer')


def _reward_range(lib, values):
    from tonic_amd import _lib
    x = torch.as_tensor(np.asarray(values, np.float32).ravel(), device='cuda')
    out = torch.full((2,), 5.0, device='cuda')
    _lib.check(lib.tonic_reward_range(_ptr(x) if x.numel() else None, x.numel(), _ptr(out), None),
               'tonic_reward_range')
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_reward_range_against_numpy(lib):
    from tonic_amd import _lib
    rng = np.random.RandomState(0)
    arrays = [rng.normal(size=(24, 256)) * 3, rng.normal(size=1), rng.normal(size=(4096, 256)),
              rng.normal(size=1000003) * 100, np.full(77, np.nan), np.array([np.inf, np.nan, -2.0]),
              np.array([-np.inf, 1.0]), np.array([np.nan, np.inf]), np.array([-0.0, 0.0]), np.array([7.5])]
    x = rng.normal(size=(333, 17))
    x[rng.uniform(size=x.shape) < 0.4] = np.nan
    arrays.append(x)
    for n in (1, 2, 63, 64, 65, 255, 1023, 1025, 4097, 99991):
        arrays.append(rng.normal(size=n) * n)
    try:
        for values in arrays:
            values = np.asarray(values, np.float32)
            results = []
            for blocks in (0, 1, 3, 256):
                assert lib.tonic_set_tuning(b'range_blocks', blocks) == 0
                results.append(_reward_range(lib, values))
            for r in results[1:]:
                assert r.tobytes() == results[0].tobytes(), 'the launch width moved the result'
            got = results[0]
            if np.isnan(values).all():
                assert got[0] > got[1] and got[0] == np.inf and got[1] == -np.inf
            else:
                assert got[0] == np.nanmin(values) and got[1] == np.nanmax(values)
        assert tuple(_reward_range(lib, np.zeros(0))) == (np.inf, -np.inf)
    finally:
        lib.tonic_set_tuning(b'range_blocks', 0)
    with pytest.raises(_lib.TonicHipError):
        _lib.check(lib.tonic_reward_range(None, 4, None, None), 'null range')


# ------------------------------------------------------------------------------- agents

def _return_model(g):
    from tonic_amd.torch import models, normalizers
    sizes = tuple(int(s) for s in g['torso_sizes'])
    act = getattr(torch.nn, str(g['torso_activation']))
    return models.ActorCritic(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, act),
                           head=models.DetachedScaleGaussianPolicyHead()),
        critic=models.Critic(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, act),
                             head=models.ValueHead()),
        observation_normalizer=normalizers.MeanStd(), return_normalizer=normalizers.Return(0.99))


# golden -> (agent class, atol of the parameters after update 1 / after the later ones)
TRAJECTORIES = {
    'ppo_return_small': ('PPO', 3e-5, 2e-4),
    'a2c_return_small': ('A2C', 2e-5, 1e-4),
    'trpo_return_small': ('TRPO', 3e-5, 3e-4),
    'ppo_wide_return_small': ('PPO', 3e-5, 2e-4),
    'ppo_tanh3_return_small': ('PPO', 3e-5, 2e-4),
}


@pytest.mark.parametrize('name', sorted(TRAJECTORIES))
def test_drop_in_trajectory_with_return_normalizer(golden, lib, name):
    """agent.step / agent.update on the synthetic environment over three rollouts with Return(0.99), like the
    reference's run: actions, critic losses, the range after every update (exact) and the parameters."""
    import tonic_amd
    import tonic_amd.torch
    g = golden(name)
    kind, first_atol, later_atol = TRAJECTORIES[name]
    O, A, W, steps, seed, iterations, updates = (int(x) for x in g['cfg'])
    env = tonic_amd.environments.distribute(
        lambda: tonic_amd.environments.Synthetic(O, A, max_episode_steps=7), 1, W)
    env.initialize(seed=seed)
    agent = getattr(tonic_amd.torch.agents, kind)(
        model=_return_model(g), replay=tonic_amd.replays.Segment(size=steps, batch_iterations=iterations))
    agent.initialize(env.observation_space, env.action_space, seed=seed)
    state = agent.model.state_dict()
    for key in g.files:
        if key.startswith('init/'):
            assert np.array_equal(state[key[5:]].detach().cpu().numpy(), g[key]), key
    observations = env.start()
    rng = np.random.RandomState(seed + 1)
    for u in range(updates):
        for t in range(steps):
            i = u * steps + t
            np.testing.assert_allclose(observations, g['act/observations'][i], rtol=0,
                                       atol=0 if u == 0 else 1e-4)
            actions = agent.step(observations, i * W)
            np.testing.assert_allclose(actions, g['act/actions'][i], rtol=0, atol=3e-6 if u == 0 else 3e-4)
            observations, infos = env.step(g['act/actions'][i])
            infos['rewards'] = (infos['rewards'] * float(g['reward_scale']) +
                                rng.normal(size=W)).astype(np.float32)
            term = rng.uniform(size=W) < 0.05
            infos['terminations'] = term
            infos['resets'] = infos['resets'] | term
            agent.update(**infos, steps=i * W)
        infos = agent.last_infos
        rows = infos[:, 0] if kind == 'TRPO' else infos[1][:, 0]
        np.testing.assert_allclose(rows, g[f'u{u}/info/critic/loss'], rtol=1e-3 if u else 2e-4,
                                   err_msg=f'update {u}: critic loss')
        rn = agent.model.return_normalizer
        assert np.array_equal(np.array([rn.min_reward, rn.max_reward], np.float32), g[f'u{u}/return/range'])
        after = agent.model.state_dict()
        for key in ('return_normalizer._low', 'return_normalizer._high',
                    'critic.head.return_normalizer._low', 'critic.head.return_normalizer._high'):
            assert after[key].detach().cpu().numpy().tobytes() == g[f'post{u}/' + key].tobytes(), (u, key)
        for key, value in after.items():
            if 'normalizer' in key:
                continue
            np.testing.assert_allclose(value.detach().cpu().numpy(), g[f'post{u}/' + key], rtol=0,
                                       atol=first_atol if u == 0 else later_atol, err_msg=f'update {u}: {key}')
    agent.close()


def _run(mode, out, extra_env=None, world=1, port=29671):
    env = dict(os.environ)
    env.update(extra_env or {})
    if world == 1:
        for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
            env.pop(key, None)
        procs = [subprocess.Popen([sys.executable, WORKER, mode, out], env=env, stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True)]
    else:
        env.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world),
                   TONIC_AMD_BACKEND='gloo')
        procs = [subprocess.Popen([sys.executable, WORKER, mode, out],
                                  env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True) for r in range(world)]
    for p in procs:
        output = p.communicate(timeout=300)[0]
        assert p.returncode == 0, output[-3000:]
    return np.load(out)


@pytest.mark.parametrize('switch', ['TONIC_AMD_CRITIC_OVERLAP', 'TONIC_AMD_SPECULATE'])
def test_ppo_switches_compute_the_same(tmp_path, switch):
    """The critic's chain under the next rollout reads a snapshot of the range; the block-fed / speculating
    steps no longer step aside for the normaliser: switching either off changes no result."""
    base = _run('loop', str(tmp_path / 'default.npz'))
    other = _run('loop', str(tmp_path / 'off.npz'), {switch: '0'})
    assert np.array_equal(base['lows'], other['lows']) and np.array_equal(base['highs'], other['highs'])
    assert base['lows'][-1] != base['lows'][0] or base['highs'][-1] != base['highs'][0], 'the range must move'
    for key in base.files:
        assert np.array_equal(base[key], other[key]), key


def test_save_and_load_keep_the_range(tmp_path, lib):
    import tonic_amd
    import tonic_amd.torch
    from tonic_amd.environments import Box
    g = {'torso_sizes': np.array([64, 64]), 'torso_activation': np.array('Tanh')}
    agents = []
    for seed in (3, 4):
        agent = tonic_amd.torch.agents.PPO(model=_return_model(g),
                                           replay=tonic_amd.replays.Segment(size=8, batch_iterations=2))
        agent.initialize(Box(-np.inf, np.inf, (17,)), Box(-1, 1, (6,)), seed=seed)
        agents.append(agent)
    first, second = agents
    first.model.return_normalizer.record(np.array([-57.25, 3.5], np.float32))
    first.model.return_normalizer.update()
    path = str(tmp_path / 'checkpoint')
    first.save(path)
    second.load(path)
    for key in ('return_normalizer._low', 'return_normalizer._high', 'critic.head.return_normalizer._low',
                'critic.head.return_normalizer._high'):
        assert torch.equal(first.model.state_dict()[key], second.model.state_dict()[key]), key
    rn = first.model.return_normalizer
    assert float(second.model.return_normalizer._low) == float(torch.as_tensor(rn.coefficient * np.float32(-57.25),
                                                                                 dtype=torch.float32))
    obs = torch.as_tensor(np.random.RandomState(0).normal(size=(300, 17)).astype(np.float32), device='cuda')
    values = [torch.empty(300, device='cuda') for _ in agents]
    for agent, out in zip(agents, values):
        agent.critic_updater.forward_values(obs, out)
    torch.cuda.synchronize()
    assert torch.equal(values[0], values[1])
    with torch.no_grad():
        stock = second.model.critic(obs)
    np.testing.assert_allclose(values[1].cpu().numpy(), stock.cpu().numpy(), rtol=0, atol=2e-5 * 6000)
    for agent in agents:
        agent.close()


def test_two_ranks_reach_the_single_process_range(tmp_path):
    single = _run('segment', str(tmp_path / 'one.npz'))
    double = _run('segment', str(tmp_path / 'two.npz'), world=2, port=29673)
    assert np.array_equal(single['lows'], double['lows']) and np.array_equal(single['highs'], double['highs'])
    assert np.array_equal(single['range'], double['range'])
    for key in single.files:
        if key in ('lows', 'highs', 'range'):
            continue
        np.testing.assert_allclose(double[key], single[key], rtol=0, atol=2e-5, err_msg=key)
