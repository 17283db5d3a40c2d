"""GPU tests of Gaussian policy heads whose scale bounds are not the defaults: SAC and MPO with
``GaussianPolicyHead(..., scale_min, scale_max)``, the bounds carried by the `H` code (tonic_mlp_torso_head) into every
kernel that forms a scale.

1. gradient sums of one critic and one actor step against float64 autograd, bounds (0.2, 1.5), SAC and MPO (S = 3 and
   70, both KL constraints), every path, B = 33 and 100, with the scale head spread over both bounds;
2. degenerate bounds 0.3 = scale_min = scale_max: the sampled actions and the scale head's gradients, no tolerance;
3. acting: tonic_policy_forward kinds 1 and 2 against the float32 restatement (tests/policy_head_ref.py);
4. one path, not two: the fused iteration serves the bounded head, and equals the split entries and both graph modes;
5. the agents against the unmodified reference (tests/golden/{sac,mpo}_scale_small.npz): acting on the collector
   block / the staged forward, every update, checkpoints;
6. refusals reach the agents.

Every comparison with a tolerance prints the largest error it saw."""
import numpy as np
import pytest

import policy_head_ref as ph
from mpo_surface_reference import mpo_reference
from test_gpu_mpo_surface import _call as _mpo_joint_call
from test_gpu_mpo_surface import _compare as _mpo_compare
from test_gpu_offpolicy_grads import Ref, _batch, _check, _check_stat, _f64, _Images, _q_steps, _stats
from test_gpu_offpolicy_torsos import ACTIVATIONS, _grad_sums

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

O, A = 17, 6
LOW, HIGH = 0.2, 1.5
# path -> (torso, activation, q_images tuning: None = the layer-by-layer launches, which have no images)
PATHS = {'images': ((256, 256), 'ReLU', 1), 'float32': ((256, 256), 'ReLU', 0), 'tanh3': ((64, 48, 32), 'Tanh', None)}
ACTING_ATOL = 5e-6                  # test_gpu_offpolicy.test_offpolicy_agent_drop_in_trajectory


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def _head(kind, bounds, **extra):
    import tonic_amd.torch as tt
    limits = {} if bounds is None else dict(scale_min=bounds[0], scale_max=bounds[1])
    if kind == 'sac':
        return tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                            distribution=tt.models.SquashedMultivariateNormalDiag, **limits, **extra)
    return tt.models.GaussianPolicyHead(**limits, **extra)


def _model(kind, sizes, activation, bounds, **extra):
    import tonic_amd.torch as tt
    act = ACTIVATIONS[activation]
    container = tt.models.ActorTwinCriticWithTargets if kind == 'sac' else tt.models.ActorCriticWithTargets
    return container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act),
                              head=_head(kind, bounds, **extra)),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=tt.models.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())


def _agent(kind, sizes, activation, B, bounds=(LOW, HIGH), S=20, iterations=1, seed=9, o=O, a=A, rows=1000):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    replay = tonic_amd.replays.Buffer(size=rows, batch_iterations=iterations, batch_size=B)
    if kind == 'mpo':
        agent = tt.agents.MPO(model=_model(kind, sizes, activation, bounds), replay=replay,
                              actor_updater=tt.updaters.MaximumAPosterioriPolicyOptimization(num_samples=S),
                              critic_updater=tt.updaters.ExpectedSARSA(num_samples=S))
    else:
        agent = tt.agents.SAC(model=_model(kind, sizes, activation, bounds), replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (o,)), Box(-1, 1, (a,)), seed=seed)
    assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
    return agent


def _variables(module):
    from tonic_amd.torch.models import network_variables
    return list(network_variables(module))


def _set_normalizer(agent, rng):
    norm = agent.model.observation_normalizer
    size = norm._mean.shape[0]
    with torch.no_grad():
        norm._mean.copy_(torch.as_tensor(np.asarray(rng.normal(size=size) * 0.5, np.float32)))
        norm._std.copy_(torch.as_tensor(np.asarray(np.exp(rng.uniform(-1, 1, size)), np.float32)))


class BoundedRef(Ref):
    """The float64 networks of test_gpu_offpolicy_grads.Ref with policy_head_ref's head: the scale clamped to the
    head's own bounds (models/actors.py:94-98)."""

    def __init__(self, agent, kind, layers, activation, low, high):
        super().__init__(agent, kind, layers, activation)
        self.low, self.high = float(np.float32(low)), float(np.float32(high))

    def heads(self, params, obs):
        h, L = self._torso(params, obs), self.L
        return self._linear(params, h, 2 * L), self._linear(params, h, 2 * L + 2)

    def policy(self, params, obs):
        return ph.gaussian_head(*self.heads(params, obs), self.low, self.high, tanh_loc=self.kind == 'mpo')


def _spread_scale_heads(agent, ref, spread=2.0):
    """Multiplies the rows of the scale head's weights (of the actor and of the target actor, each by its own
    figures) until every action dimension's float64 pre-activation on standard-normal observations is centred with a
    standard deviation of `spread`: about 0.22 / 0.51 / 0.27 of them then lie below, inside and above the bounds
    (0.2, 1.5)."""
    m = agent.model
    size = m.observation_normalizer._mean.shape[0]
    sample = torch.as_tensor(np.random.RandomState(0).normal(size=(4096, size)))
    with torch.no_grad():
        for net in (m.actor, m.target_actor):
            w, b = _variables(net)[-2:]
            pre = ref.heads(_f64(net), sample)[1] - b.double().cpu()
            factor = spread / pre.std(0)
            w.mul_(factor.to(w)[:, None])
            b.copy_((-factor * pre.mean(0)).to(b))


def _conditioned(agent, kind, ref, B, S=1, first_seed=None, a=A):
    """A batch and its noise for which the condition on the inputs holds, from the float64 reference alone: on every
    (network, observations) pair the steps read, each of the three regimes of the clamp (softplus below scale_min,
    inside, above scale_max) holds at least 10 % of the (row, action) elements and no softplus lies within 1e-3 of
    a bound.  The seed is the first of 1000 + B, 1001 + B, ... that satisfies it."""
    m = agent.model
    size = m.observation_normalizer._mean.shape[0]
    pairs = [(m.actor, 'next_observations'), (m.actor, 'observations')] if kind == 'sac' else \
        [(m.target_actor, 'next_observations'), (m.target_actor, 'observations'), (m.actor, 'observations')]
    leaves = {id(net): _f64(net) for net, _ in pairs}
    start = 1000 + B if first_seed is None else first_seed
    for seed in range(start, start + 5000):
        rng = np.random.RandomState(seed)
        batch = _batch(rng, B, size, a)
        good = True
        with torch.no_grad():
            for net, key in pairs:
                below, inside, above, distance = ph.regimes(ref.heads(leaves[id(net)], batch[key].double())[1],
                                                            ref.low, ref.high)
                good = good and min(below, inside, above) >= 0.10 and distance >= 1e-3
        if good:
            eps = torch.as_tensor(rng.normal(size=(S * B, a)), dtype=torch.float32)
            eps_actor = torch.as_tensor(rng.normal(size=(S * B, a)), dtype=torch.float32)
            return seed, batch, eps, eps_actor
    raise AssertionError('no seed satisfies the condition on the inputs')


def _assert_condition(agent, kind, ref, batch):
    """The condition of `_conditioned`, asserted (on the float64 reference, before anything is compared)."""
    m = agent.model
    pairs = [(m.actor, 'next_observations'), (m.actor, 'observations')] if kind == 'sac' else \
        [(m.target_actor, 'next_observations'), (m.target_actor, 'observations'), (m.actor, 'observations')]
    shares = []
    with torch.no_grad():
        for net, key in pairs:
            below, inside, above, distance = ph.regimes(ref.heads(_f64(net), batch[key].double())[1], ref.low, ref.high)
            assert min(below, inside, above) >= 0.10, (key, below, inside, above)
            assert distance >= 1e-3, (key, distance)
            shares.append((round(below, 2), round(inside, 2), round(above, 2)))
    return shares


def _expected_code(lib, sizes, activation, low, high):
    import ctypes
    code = {'ReLU': 1, 'Tanh': 2, 'ELU': 3}[activation]
    return lib.tonic_mlp_torso_head(len(sizes), (ctypes.c_int32 * len(sizes))(*sizes), code, low, high)


# ---------------------------------------------------------------- 1. gradient sums vs float64

@pytest.mark.parametrize('B', [33, 100])
@pytest.mark.parametrize('path', list(PATHS))
def test_sac_gradient_sums_vs_float64(lib, path, B):
    """One critic step (tonic_twin_q_grad_loss) and one actor step (tonic_actor_q_grad) of SAC with head bounds
    (0.2, 1.5) against float64 autograd of the reference's losses: every tensor within 1e-5 of its largest element,
    loss / q1 / q2 / actor loss within 1e-5 (_check / _check_stat of test_gpu_offpolicy_grads).  B = 33: a ragged last
    tile.  The scale head is spread over both bounds (see _conditioned, asserted on the reference)."""
    sizes, activation, images = PATHS[path]
    with _Images(lib, 1 if images is None else images):
        agent = _agent('sac', sizes, activation, B)
        for updater in (agent.critic_updater, agent.actor_updater):
            assert updater.hidden == _expected_code(lib, sizes, activation, LOW, HIGH) and updater.hidden >= 1 << 30
            assert updater.scale_bounds == (np.float32(LOW), np.float32(HIGH))
        if images is not None:
            assert (lib.tonic_mlp_actor_image_bytes(O, agent.hidden, A, 2) > 0) == bool(images)
            assert agent.critic_updater.torso_code == sizes[0]
        _set_normalizer(agent, np.random.RandomState(B))
        ref = BoundedRef(agent, 'sac', len(sizes), activation, LOW, HIGH)
        _spread_scale_heads(agent, ref)
        seed, batch, eps, eps_actor = _conditioned(agent, 'sac', ref, B)
        shares = _assert_condition(agent, 'sac', ref, batch)
        out = _q_steps(agent, 'sac', batch, eps, eps_actor, ref)
    print(f'sac {path} B={B} seed {seed} regimes {shares}: largest relative error critic {out["critic"]:.2e} '
          f'actor {out["actor"]:.2e}')


MPO_DUALS = {False: lambda: np.concatenate([[1.0], np.full(A, 1.0), np.full(A, 2.0), [0.5]]).astype(np.float32),
             True: lambda: np.array([1.0, 1.0, 2.0, 0.5], np.float32)}


@pytest.mark.parametrize('joint', [False, True])
@pytest.mark.parametrize('S', [3, 70])
@pytest.mark.parametrize('B', [33, 100])
@pytest.mark.parametrize('path', list(PATHS))
def test_mpo_gradient_sums_vs_float64(lib, path, B, S, joint):
    """One critic step (tonic_expected_sarsa_grad_loss) and one actor step (tonic_mpo_actor_grad_joint, both
    joint_kl values) of MPO with head bounds (0.2, 1.5), S = 3 (one register slot) and 70 (two), against float64 of
    critics.py:238-282 / actors.py:318-464: every tensor within 1e-5 of its largest element.  The temperature is warm
    (log T = 1), so that the standing bound of the MPO actor step, max(1e-5, 64 2^-24 max |Q| / T), IS 1e-5 — asserted
    on the reference."""
    sizes, activation, images = PATHS[path]
    with _Images(lib, 1 if images is None else images):
        agent = _agent('mpo', sizes, activation, B, S=S)
        m, critic_u, u = agent.model, agent.critic_updater, agent.actor_updater
        assert u.hidden == critic_u.hidden == _expected_code(lib, sizes, activation, LOW, HIGH)
        rng = np.random.RandomState(S + B)
        _set_normalizer(agent, rng)
        with torch.no_grad():          # the online actor away from the target: every KL first order
            for p in _variables(m.actor):
                p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.02, dtype=torch.float32, device='cuda')
        ref = BoundedRef(agent, 'mpo', len(sizes), activation, LOW, HIGH)
        _spread_scale_heads(agent, ref)
        seed, batch, eps, eps_actor = _conditioned(agent, 'mpo', ref, B, S=S)
        shares = _assert_condition(agent, 'mpo', ref, batch)
        # ---- the critic step (test_expected_sarsa_grads_vs_float64 with the bounded head)
        target_actor, frozen, online = _f64(m.target_actor), _f64(m.target_critic), _f64(m.critic)
        d = {k: v.double() for k, v in batch.items()}
        with torch.no_grad():
            loc, scale = ref.policy(target_actor, d['next_observations'])
            a = (loc[None] + scale[None] * eps.double().view(S, B, A)).reshape(S * B, A)
            nxt = ref.critic(frozen, d['next_observations'].repeat(S, 1), a).view(S, B).mean(0)
            returns = d['rewards'] + d['discounts'] * nxt
        q = ref.critic(online, d['observations'], d['actions'])
        sq = (q - returns) ** 2
        sq.mean().backward()
        critic_u.enqueue({k: v.cuda() for k, v in batch.items()}, eps.cuda(), torch.zeros(8, device='cuda'))
        stats = _stats(critic_u)
        assert stats[5] == B, stats
        critic_err = _check(_grad_sums([m.critic], critic_u.grad_sums, B), online,
                            [f'critic {i}' for i in range(len(online))])
        _check_stat(stats[0] / B, sq.detach().mean(), sq.detach(), 'loss')
        _check_stat(stats[1] / B, q.detach().mean(), q.detach(), 'q')
        # ---- the actor step through the critic the critic step has just moved (its target is what it was)
        duals = MPO_DUALS[joint]()
        obs = batch['observations']
        *_, tempering = mpo_reference(ref, _f64(m.actor), _f64(m.target_actor), _f64(m.target_critic), obs.double(),
                                      eps_actor.double(), duals, u.min_log_dual, u, S, True, not joint)
        assert 64 * 2.0 ** -24 * tempering <= 1e-5, tempering           # the bound below is 1e-5
        got = _mpo_joint_call(lib, agent, u, duals, obs, eps_actor, joint=joint)
        print(f'mpo {path} B={B} S={S} joint={joint} seed {seed} regimes {shares}: critic {critic_err:.2e}')
        _mpo_compare(agent, u, got, duals, obs, eps_actor, ref, f'bounded {path} B={B} S={S} joint={joint}', joint)


# ---------------------------------------------------------------- 2. degenerate bounds

def _policy_forward(agent, kind, observations, eps, code=None):
    """tonic_policy_forward on device tensors; code: the `H` argument (default: the agent's)."""
    from tonic_amd import _lib
    lib, p = agent.lib, _lib.ptr
    W = observations.shape[0]
    H = agent.hidden if code is None else code
    ws = torch.empty(lib.tonic_offpolicy_workspace_bytes(W, agent.observation_size, agent.action_size, H),
                     dtype=torch.uint8, device='cuda')
    out = torch.full((W, agent.action_size), float('nan'), device='cuda')
    _lib.check(lib.tonic_policy_forward(
        p(agent.model.flat_actor.flat), p(observations), p(eps) if eps is not None else None, p(out), kind, W,
        agent.observation_size, H, agent.action_size, p(ws), ws.numel(), _lib.current_stream()),
        'tonic_policy_forward')
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('path', list(PATHS))
def test_degenerate_bounds_mpo_without_tolerance(lib, path):
    """scale_min == scale_max == 0.3: every sampled action IS loc + 0.3 * eps in float32 — loc the kernel's own greedy
    action, the product rounded before the sum — whatever the scale head says (its weights are spread as in test 1),
    and every gradient sum of the scale head's weights and bias is exactly 0 while the loc head's are not."""
    sizes, activation, images = PATHS[path]
    B, S = 33, 3
    with _Images(lib, 1 if images is None else images):
        agent = _agent('mpo', sizes, activation, B, bounds=(0.3, 0.3), S=S)
        rng = np.random.RandomState(4)
        _set_normalizer(agent, rng)
        _spread_scale_heads(agent, BoundedRef(agent, 'mpo', len(sizes), activation, LOW, HIGH))
        observations = torch.as_tensor(rng.normal(size=(B, O)), dtype=torch.float32).cuda()
        eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
        loc = _policy_forward(agent, 2, observations, None)
        got = _policy_forward(agent, 2, observations, eps.cuda())
        np.testing.assert_array_equal(got, loc + np.float32(0.3) * eps.numpy())
        assert not np.array_equal(got, _policy_forward(agent, 2, observations, eps.cuda(),
                                                       code=agent.critic_updater.torso_code))
        u = agent.actor_updater
        eps_actor = torch.as_tensor(rng.normal(size=(S * B, A)), dtype=torch.float32)
        for joint in (False, True):
            grads = _mpo_joint_call(lib, agent, u, MPO_DUALS[joint](), observations.cpu(), eps_actor, joint=joint)[0]
            tensors = _grad_sums([agent.model.actor], torch.as_tensor(grads), B)
            assert not np.asarray(tensors[-1].cpu()).any() and not np.asarray(tensors[-2].cpu()).any()
            assert np.abs(np.asarray(tensors[-3].cpu())).max() > 0 and np.isfinite(grads).all()


@pytest.mark.parametrize('path', list(PATHS))
def test_degenerate_bounds_sac_without_tolerance(lib, path):
    """scale_min == scale_max == 0.3 under the squashed head, a = tanh(loc + eps * 0.3).
    A SUBSTITUTE for "the last bit of the float32 restatement": the device's tanhf and NumPy's tanh differ in their
    last bits, so no host restatement of tanh(u) can be compared bit for bit.  What is compared bit for bit instead
    is the argument u and the kernel's own tanh of it; the host restatement (NumPy's tanh) is held at 5e-6, the
    acting tolerance.
    - with a loc head of zero weights loc IS its bias, so u = bias + eps * 0.3 is known in float32 to the last bit;
      the greedy forward of a network whose loc bias is set to a row's u gives tanh(u) by the kernel's own tanh, and
      the sampled actions of all 33 rows (the ragged last tile included) equal it bit for bit, whatever the (spread)
      scale head says;
    - on the network as initialised, replacing the scale head by other weights leaves every sampled action as it is,
      and the float32 restatement (NumPy's tanh) holds at the acting tolerance;
    - every gradient sum of the scale head's weights and bias is exactly 0 after the actor step."""
    sizes, activation, images = PATHS[path]
    B = 33
    with _Images(lib, 1 if images is None else images):
        agent = _agent('sac', sizes, activation, B, bounds=(0.3, 0.3))
        m = agent.model
        rng = np.random.RandomState(6)
        _set_normalizer(agent, rng)
        ref = BoundedRef(agent, 'sac', len(sizes), activation, 0.3, 0.3)
        _spread_scale_heads(agent, BoundedRef(agent, 'sac', len(sizes), activation, LOW, HIGH))
        batch = _batch(rng, B, O, A)
        observations = batch['observations'].cuda()
        eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
        # ---- the network as initialised
        got = _policy_forward(agent, 1, observations, eps.cuda())
        with torch.no_grad():
            loc_pre, scale_pre = ref.heads(_f64(m.actor), batch['observations'].double())
        want = ph.act32(loc_pre.numpy(), scale_pre.numpy(), eps.numpy(), 0.3, 0.3, squash=True)
        print(f'sac degenerate {path}: largest |action - restatement| {np.abs(got - want).max():.2e}')
        np.testing.assert_allclose(got, want, rtol=0, atol=ACTING_ATOL)
        assert not np.array_equal(got, _policy_forward(agent, 1, observations, eps.cuda(),
                                                       code=agent.critic_updater.torso_code))
        w_scale, b_scale = _variables(m.actor)[-2:]
        kept = w_scale.clone(), b_scale.clone()
        with torch.no_grad():
            w_scale.copy_(torch.as_tensor(rng.normal(size=tuple(w_scale.shape)), dtype=torch.float32))
            b_scale.copy_(torch.as_tensor(rng.normal(size=tuple(b_scale.shape)) * 3, dtype=torch.float32))
        np.testing.assert_array_equal(_policy_forward(agent, 1, observations, eps.cuda()), got)
        with torch.no_grad():
            w_scale.copy_(kept[0])
            b_scale.copy_(kept[1])
        # ---- the actor step: the scale head's gradient sums
        eps_actor = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
        agent.actor_updater.enqueue(observations, eps_actor.cuda(), torch.zeros(8, device='cuda'))
        torch.cuda.synchronize()
        tensors = _grad_sums([m.actor], agent.actor_updater.grad_sums, B)
        assert not np.asarray(tensors[-1].cpu()).any() and not np.asarray(tensors[-2].cpu()).any()
        assert np.abs(np.asarray(tensors[-3].cpu())).max() > 0
        # ---- loc = bias: the last bit
        w_loc, b_loc = _variables(m.actor)[-4:-2]
        bias = rng.normal(size=A).astype(np.float32)
        with torch.no_grad():
            w_loc.zero_()
            b_loc.copy_(torch.as_tensor(bias))
        agent._q.parameters_changed()
        got = _policy_forward(agent, 1, observations, eps.cuda())
        u = bias[None] + eps.numpy() * np.float32(0.3)
        for row in range(B):
            with torch.no_grad():
                b_loc.copy_(torch.as_tensor(u[row]))
            np.testing.assert_array_equal(got[row], _policy_forward(agent, 1, observations[:1], None)[0], err_msg=str(row))
        np.testing.assert_allclose(got, np.tanh(u), rtol=0, atol=ACTING_ATOL)


# ---------------------------------------------------------------- 3. acting

@pytest.mark.parametrize('kind,policy', [('sac', 1), ('mpo', 2)])
@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('W', [5, 40])
def test_policy_forward_vs_the_float32_restatement(lib, kind, policy, path, W):
    """tonic_policy_forward kind 1 (squashed Gaussian) and kind 2 (Gaussian, tanh loc) with head bounds (0.2, 1.5),
    stochastic and greedy, against policy_head_ref.act32 on the float64 heads' outputs at the acting tolerance of
    test_gpu_offpolicy (5e-6 absolute); the stochastic actions are NOT those of the torso's own code (the default
    bounds), the greedy ones are, bit for bit."""
    sizes, activation, images = PATHS[path]
    with _Images(lib, 1 if images is None else images):
        agent = _agent(kind, sizes, activation, 16)
        rng = np.random.RandomState(W)
        ref = BoundedRef(agent, kind, len(sizes), activation, LOW, HIGH)
        _spread_scale_heads(agent, ref)
        host = torch.as_tensor(rng.normal(size=(W, O)), dtype=torch.float32)
        eps = torch.as_tensor(rng.normal(size=(W, A)), dtype=torch.float32)
        with torch.no_grad():
            loc, _ = ref.policy(_f64(agent.model.actor), host.double())
            loc_pre, scale_pre = ref.heads(_f64(agent.model.actor), host.double())
            below, inside, above, _ = ph.regimes(scale_pre, LOW, HIGH)
        assert below > 0 and above > 0 and inside > 0
        loc_out = (loc_pre if kind == 'sac' else loc).numpy()
        plain = agent.critic_updater.torso_code
        worst = 0.0
        for noise in (eps, None):
            got = _policy_forward(agent, policy, host.cuda(), noise.cuda() if noise is not None else None)
            want = ph.act32(loc_out, scale_pre.numpy(), None if noise is None else noise.numpy(), LOW, HIGH,
                            squash=kind == 'sac')
            worst = max(worst, float(np.abs(got - want).max()))
            np.testing.assert_allclose(got, want, rtol=0, atol=ACTING_ATOL)
            default = _policy_forward(agent, policy, host.cuda(), noise.cuda() if noise is not None else None, code=plain)
            assert np.array_equal(got, default) == (noise is None)
        print(f'{kind} acting {path} W={W}: largest |action - restatement| {worst:.2e}')


# ---------------------------------------------------------------- 4. one path, not two

def test_fused_iteration_serves_the_bounded_head_and_equals_every_other_path(lib, monkeypatch):
    """A SAC agent with head bounds (0.2, 1.5) on the default torso takes the fused iteration (tonic_q_iteration); two
    update calls of four iterations leave the same bits in parameters, targets, moments, step counters and infos on
    the fused iteration and on the split entries (TONIC_AMD_FUSED_ITERATION=0), each launched eagerly
    (TONIC_AMD_NO_GRAPH=1) and replayed from a captured graph — and other bits than the default bounds."""
    o, a, W, B, rows, iterations = 23, 5, 2, 40, 24, 4
    rng = np.random.RandomState(11)
    host = dict(observations=rng.normal(size=(rows, W, o)), actions=rng.uniform(-1, 1, (rows, W, a)),
                next_observations=rng.normal(size=(rows, W, o)), rewards=rng.normal(size=(rows, W)),
                resets=rng.uniform(size=(rows, W)) < 0.1, terminations=rng.uniform(size=(rows, W)) < 0.05)
    host = {k: np.asarray(v, np.float32) for k, v in host.items()}
    eps = rng.normal(size=(iterations, 2, B, a)).astype(np.float32)
    indices = rng.randint(rows * W, size=(iterations, B))
    dev = lambda x: torch.as_tensor(x).cuda()       # noqa: E731
    results = {}
    for mode, fused, no_graph, bounds in (('fused-graph', '1', '0', (LOW, HIGH)), ('fused', '1', '1', (LOW, HIGH)),
                                          ('split-graph', '0', '0', (LOW, HIGH)), ('split', '0', '1', (LOW, HIGH)),
                                          ('default bounds', '1', '0', None)):
        monkeypatch.setenv('TONIC_AMD_FUSED_ITERATION', fused)
        monkeypatch.setenv('TONIC_AMD_NO_GRAPH', no_graph)
        agent = _agent('sac', (256, 256), 'ReLU', B, bounds=bounds, iterations=iterations, seed=5, o=o, a=a,
                       rows=rows * W)
        assert (agent._fused_kind() is not None) == (fused == '1')
        _set_normalizer(agent, np.random.RandomState(1))
        _spread_scale_heads(agent, BoundedRef(agent, 'sac', 2, 'ReLU', LOW, HIGH))
        for t in range(rows):
            agent.replay.store(**{k: dev(v[t]) for k, v in host.items()})
        infos = [agent.enqueue_update(indices, eps).cpu().numpy().copy() for _ in range(2)]
        assert (agent._graph is not None) == (no_graph == '0')
        results[mode] = dict(
            infos0=infos[0], infos1=infos[1], online=agent.model.flat_online.cpu().numpy(),
            target=agent.model.flat_target.cpu().numpy(),
            critic_m=agent.critic_updater.exp_avg.cpu().numpy(), critic_v=agent.critic_updater.exp_avg_sq.cpu().numpy(),
            actor_m=agent.actor_updater.exp_avg.cpu().numpy(), actor_v=agent.actor_updater.exp_avg_sq.cpu().numpy(),
            steps=np.array([int(agent.critic_updater.state[0]), int(agent.actor_updater.state[0])]))
    want = results['split']
    assert list(want['steps']) == [2 * iterations, 2 * iterations]
    assert np.isfinite(want['online']).all() and np.isfinite(want['infos1']).all()
    for mode in ('fused-graph', 'fused', 'split-graph'):
        for key, value in want.items():
            assert np.array_equal(results[mode][key], value), (mode, key, np.abs(results[mode][key] - value).max())
    assert not np.array_equal(results['default bounds']['online'], want['online'])
    assert not np.array_equal(results['default bounds']['infos0'], want['infos0'])


# ---------------------------------------------------------------- 5. the agents against the unmodified reference

UPDATES = 3


def _widen_scale_layer(module):
    """`scale_fn` of the goldens' heads (scripts/make_policy_head_goldens.py: SCALE_GAIN = 16)."""
    if isinstance(module, torch.nn.Linear):
        with torch.no_grad():
            module.weight.mul_(16.0)


def _golden_agent(g, kind):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    o, a, W, hidden, B, iterations, seed, loop_steps = (int(x) for x in g['cfg'])
    assert float(g['scale_gain']) == 16.0
    model = _model(kind, (hidden, hidden), 'ReLU', tuple(float(v) for v in g['scale_bounds']),
                   scale_fn=_widen_scale_layer)
    replay = tonic_amd.replays.Buffer(size=400, batch_iterations=iterations, batch_size=B,
                                      steps_before_batches=W * 10, steps_between_batches=W * 10,
                                      return_steps=int(g['return_steps']))
    if kind == 'sac':
        agent = tt.agents.SAC(model=model, replay=replay,
                              exploration=tonic_amd.explorations.NoActionNoise(start_steps=W * 5))
    else:
        samples = int(g['samples'])
        agent = tt.agents.MPO(model=model, replay=replay,
                              actor_updater=tt.updaters.MaximumAPosterioriPolicyOptimization(num_samples=samples),
                              critic_updater=tt.updaters.ExpectedSARSA(num_samples=samples))
    agent.initialize(Box(-np.inf, np.inf, (o,)), Box(-1, 1, (a,)), seed=seed)
    return agent


def _state(g, u):
    """The reference's state in front of update u: pre{u} is post{u-1}, init for the first (asserted by the
    generator)."""
    prefix = 'init/' if u == 0 else f'post{u - 1}/'
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


@pytest.mark.parametrize('name,kind', [('sac_scale_small', 'sac'), ('mpo_scale_small', 'mpo')])
def test_agents_match_the_unmodified_reference(lib, golden, name, kind, tmp_path):
    """The unmodified reference's SAC / MPO with GaussianPolicyHead(scale_min=0.2, scale_max=1.5) and a scale layer
    initialised 16 x wider (scripts/make_policy_head_goldens.py), 31 loop steps, three learner updates; the tonic_amd
    agent is built from the same seed (init/ equal bit for bit) and run in the same loop on the same environment.

    Acting, every step up to the first update: agent.step (SAC: on the environment's collector block) and
    agent.test_step against the reference's actions within 5e-6 — the tolerance of
    test_offpolicy_agent_drop_in_trajectory; the float32 restatement reproduces the reference's there too, and the
    default bounds would not (asserted on the recorded actions).  After EACH update, started from the reference's own
    state in front of it: the parameter change post - pre within 1e-5 absolute, the logged losses within rtol 1e-5 +
    1e-5 (MPO's eleven values at rtol 2e-5 + 2e-6, alphas at rtol 1e-5) — the tolerances of
    test_offpolicy_update_matches_reference.  A checkpoint saved after the last update loads strictly into a fresh
    agent, and the reference's state loads strictly into this one."""
    import tonic_amd
    import tonic_amd.torch as tt
    g = golden(name)
    o, a, W, hidden, B, iterations, seed, loop_steps = (int(x) for x in g['cfg'])
    low, high = (float(v) for v in g['scale_bounds'])
    agent = _golden_agent(g, kind)
    assert agent.actor_updater.scale_bounds == (np.float32(low), np.float32(high))
    state = agent.model.state_dict()
    for key in state:
        np.testing.assert_array_equal(state[key].cpu().numpy(), g['init/' + key], err_msg=key)
    assert sorted(state) == sorted(k[len('init/'):] for k in g.files if k.startswith('init/'))
    # the recorded actions are those of the bounds, not of the defaults (float32 restatement on the initial actor)
    first_update = int(g['updates'][0]) // W
    policy_steps = [t for t in range(first_update + 1) if kind == 'mpo' or t * W > W * 5]        # (SAC: after the warm-up)
    x = g['act/observations'][policy_steps].reshape(-1, o).astype(np.float32)
    for layer in (0, 2):
        x = np.maximum(x @ g[f'init/actor.torso.model.{layer}.weight'].T + g[f'init/actor.torso.model.{layer}.bias'], 0)
    loc_out = x @ g['init/actor.head.loc_layer.0.weight'].T + g['init/actor.head.loc_layer.0.bias']
    scale_pre = x @ g['init/actor.head.scale_layer.0.weight'].T + g['init/actor.head.scale_layer.0.bias']
    if kind == 'mpo':
        loc_out = np.tanh(loc_out)
    recorded_eps = g['act/policy_eps'][policy_steps].reshape(-1, a)
    recorded = g['act/actions'][policy_steps].reshape(-1, a)
    restated = ph.act32(loc_out, scale_pre, recorded_eps, low, high, squash=kind == 'sac')
    np.testing.assert_allclose(restated, recorded, rtol=0, atol=ACTING_ATOL)
    defaults = ph.act32(loc_out, scale_pre, recorded_eps, 1e-4, 1.0, squash=kind == 'sac')
    assert np.abs(defaults - recorded).max() > 1e-2
    env = tonic_amd.environments.distribute(lambda: tonic_amd.environments.Synthetic(o, a, max_episode_steps=5), 1, W)
    env.initialize(seed=seed)
    observations = env.start()
    worst, done = {}, []
    at = {}
    agent.replay.sample_indices = lambda *args: g[f'u{at["u"]}/indices']
    agent._draw_noise = lambda n: g[f'u{at["u"]}/eps'].astype(np.float32)

    def check(u):
        after = {k: v.detach().cpu().numpy() for k, v in agent.model.state_dict().items()}
        pre = _state(g, u)
        infos = agent.last_infos
        info = lambda key: g[f'u{u}/info/{key}']       # noqa: E731
        np.testing.assert_allclose(infos[0][:, 0], info('critic/loss'), rtol=1e-5, atol=1e-5)
        if kind == 'sac':
            np.testing.assert_allclose(infos[0][:, 1], info('critic/q1_mean'), rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(infos[0][:, 2], info('critic/q2_mean'), rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(infos[1][:, 0], info('actor/loss'), rtol=1e-5, atol=1e-5)
        else:
            np.testing.assert_allclose(infos[0][:, 1], info('critic/q_mean'), rtol=1e-5, atol=1e-5)
            stats = agent._mpo_stats.cpu().numpy()
            for i, key in enumerate(tt.updaters.MPO_INFO):
                suffix = '_mean' if key.startswith('temperature') else ''
                np.testing.assert_allclose(stats[:, i], info('actor/' + key + suffix), rtol=2e-5, atol=2e-6,
                                           err_msg=key)
            np.testing.assert_allclose(stats[:, 8:8 + a], info('actor/alpha_mean'), rtol=1e-5)
            np.testing.assert_allclose(stats[:, 8 + a:8 + 2 * a], info('actor/alpha_std'), rtol=1e-5)
            np.testing.assert_allclose(stats[:, 8 + 2 * a], info('actor/penalty_temperature_mean'), rtol=1e-5)
            np.testing.assert_allclose(agent.actor_updater.duals.cpu().numpy(), g[f'u{u}/duals_post'], rtol=1e-5,
                                       atol=1e-6)
        for key, value in after.items():
            if 'normalizer' not in key:
                got, want = value - pre[key], g[f'post{u}/{key}'] - pre[key]
                worst[u] = max(worst.get(u, 0.0), float(np.abs(got - want).max()))
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-5, err_msg=f'{u} {key}')
        print(f'{name} update {u}: largest |parameter change - reference\'s| {worst[u]:.2e}')
        # the next update starts from the reference's own state (rounding does not accumulate across updates)
        agent.model.load_state_dict({k: torch.as_tensor(v) for k, v in _state(g, u + 1).items()}, strict=True)
        if kind == 'mpo':
            agent.actor_updater.duals.copy_(torch.as_tensor(g[f'u{u}/duals_post']))
        agent._q.parameters_changed()

    acting = 0.0
    for t in range(loop_steps):
        np.testing.assert_array_equal(observations, g['act/observations'][t])
        if not done:          # (after the first update the parameters differ at rounding level)
            greedy = agent.test_step(observations.copy(), t * W)        # (a copy: the staged forward)
            np.testing.assert_allclose(greedy, g['act/greedy_actions'][t], rtol=0, atol=ACTING_ATOL)
        actions = agent.step(observations, t * W)
        if kind == 'sac' and t * W > W * 5:
            assert agent._q.stepped is not None                     # acting ran on the collector block
        if not done:
            acting = max(acting, float(np.abs(actions - g['act/actions'][t]).max()))
            np.testing.assert_allclose(actions, g['act/actions'][t], rtol=0, atol=ACTING_ATOL)
        # (the transition holds the recorded action: after the first update the agent's own noise stream is not the
        #  reference's, whose updaters drew from the same generator in between)
        agent.last_actions = g['act/actions'][t].astype(np.float32)
        observations, infos = env.step(g['act/actions'][t])
        # (the recorded outcome: the reference's environment adds its reward noise in float64, a last bit apart)
        np.testing.assert_array_equal(infos['observations'], g['act/next_observations'][t])
        infos['rewards'], infos['resets'], infos['terminations'] = \
            g['act/rewards'][t], g['act/resets'][t], g['act/terminations'][t]
        at['u'] = int(np.searchsorted(g['updates'], t * W))
        before = getattr(agent, 'last_infos', None)
        agent.update(**infos, steps=t * W)
        if getattr(agent, 'last_infos', None) is not before:
            assert g['updates'][at['u']] == t * W
            done.append(at['u'])
            check(at['u'])
    assert done == list(range(UPDATES))
    print(f'{name}: largest |action - reference\'s| before the first update {acting:.2e}')
    # checkpoints, both ways
    path = str(tmp_path / 'checkpoint' / 'step')
    agent.save(path)
    saved = torch.load(path + '.pt')
    assert sorted(saved) == sorted(k[len('init/'):] for k in g.files if k.startswith('init/'))
    fresh = _golden_agent(g, kind)
    fresh.load(path)
    for key, value in agent.model.state_dict().items():
        np.testing.assert_array_equal(fresh.model.state_dict()[key].cpu().numpy(), value.cpu().numpy(), err_msg=key)
    fresh.model.load_state_dict({k: torch.as_tensor(v) for k, v in _state(g, UPDATES).items()}, strict=True)
    agent.close()
    fresh.close()


# ---------------------------------------------------------------- 6. refusals reach the agents

def test_refused_heads_raise_at_initialize_by_name(lib):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    m = tt.models
    on_policy = m.ActorCritic(
        actor=m.Actor(encoder=m.ObservationEncoder(), torso=m.MLP((64, 64), torch.nn.Tanh),
                      head=m.DetachedScaleGaussianPolicyHead(scale_max=0.5)),
        critic=m.Critic(encoder=m.ObservationEncoder(), torso=m.MLP((64, 64), torch.nn.Tanh), head=m.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())
    with pytest.raises(NotImplementedError, match='scale_max=0.5'):
        tt.agents.PPO(model=on_policy).initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    deterministic = m.ActorTwinCriticWithTargets(
        actor=m.Actor(encoder=m.ObservationEncoder(), torso=m.MLP((256, 256), torch.nn.ReLU),
                      head=m.DeterministicPolicyHead(activation=torch.nn.Identity)),
        critic=m.Critic(encoder=m.ObservationActionEncoder(), torso=m.MLP((256, 256), torch.nn.ReLU),
                        head=m.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())
    with pytest.raises(NotImplementedError, match='activation=.*Identity'):
        tt.agents.TD3(model=deterministic).initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    # ... a TRPO head with other bounds on a kernel torso: its actor step falls back to autograd, acting does not
    trpo = m.ActorCritic(
        actor=m.Actor(encoder=m.ObservationEncoder(), torso=m.MLP((64, 64), torch.nn.Tanh),
                      head=m.DetachedScaleGaussianPolicyHead(scale_min=1e-2)),
        critic=m.Critic(encoder=m.ObservationEncoder(), torso=m.MLP((64, 64), torch.nn.Tanh), head=m.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())
    with pytest.raises(NotImplementedError, match='scale_min=0.01'):
        tt.agents.TRPO(model=trpo).initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    # ... and an MPO head (tanh loc, Normal) under SAC's updaters
    gaussian = m.ActorTwinCriticWithTargets(
        actor=m.Actor(encoder=m.ObservationEncoder(), torso=m.MLP((256, 256), torch.nn.ReLU),
                      head=m.GaussianPolicyHead(scale_max=2)),
        critic=m.Critic(encoder=m.ObservationActionEncoder(), torso=m.MLP((256, 256), torch.nn.ReLU),
                        head=m.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())
    with pytest.raises(NotImplementedError, match='loc_activation'):
        tt.agents.SAC(model=gaussian).initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)


@pytest.mark.parametrize('name', ['PPO', 'A2C'])
def test_on_policy_torsos_on_stock_operators_keep_any_head(lib, name):
    """A torso outside the on-policy kernels (two ReLU layers of 512) acts and learns through the module's own
    forward, which honours the head as it is: such an agent initialises with bounds and a loc activation the kernels
    would refuse, and its actions are those of the module — loc + scale * eps with the scale clamped to 0.5."""
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    m = tt.models
    head = m.DetachedScaleGaussianPolicyHead(loc_activation=torch.nn.Identity, scale_max=0.5, log_scale_init=1.0)
    model = m.ActorCritic(
        actor=m.Actor(encoder=m.ObservationEncoder(), torso=m.MLP((512, 512), torch.nn.ReLU), head=head),
        critic=m.Critic(encoder=m.ObservationEncoder(), torso=m.MLP((512, 512), torch.nn.ReLU), head=m.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())
    agent = getattr(tt.agents, name)(model=model)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=3)
    assert agent.actor_updater.stock is True
    observations = np.random.RandomState(2).normal(size=(4, O)).astype(np.float32)
    with torch.no_grad():
        distribution = agent.model.actor(torch.as_tensor(observations).cuda())
    assert float(distribution.scale.max()) == 0.5                    # softplus(1) = 1.31 on the head's own ceiling
    torch.manual_seed(11)
    eps = torch.randn(4, A).numpy()
    torch.manual_seed(11)
    actions = agent.test_step(observations, 0)
    want = distribution.loc.cpu().numpy() + distribution.scale.cpu().numpy() * eps
    np.testing.assert_allclose(actions, want, rtol=0, atol=ACTING_ATOL)
