"""GPU tests of the Return normaliser on the off-policy split entries (tonic_twin_q_grad_ranged /
tonic_actor_q_grad_ranged): DDPG, TD3 and SAC with ``return_normalizer=Return(discount)``, whose critics' value heads
publish v = low + sigmoid(z) (high - low) (csrc/mlpfwd.h: value_squash / value_squash_dz).

1. gradient sums of one critic and one actor step against float64 autograd, every kind x path, B = 100 and 33;
2. the published values and the head's gradient factor against tests/return_squash_ref.py, no tolerance but exp's;
3. NULL / NULL is the entry without the suffix, bit for bit, and the fused iteration still serves the plain model;
4. a moved range under graph replay;
5. the stock-torch torsos;
6. the three agents against the unmodified reference (tests/golden/*_return_small.npz), every update;
7. a checkpoint between two updates.

Every comparison with a tolerance prints the largest error it saw."""
import ctypes

import numpy as np
import pytest

import return_squash_ref as rs
from test_gpu_offpolicy_grads import Ref, _batch, _check, _check_stat, _f64, _Images, _q_steps
from test_gpu_offpolicy_torsos import ACTIVATIONS, _grad_sums

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

O, A = 17, 6
# path -> (torso, activation, q_images tuning: None = the layer-by-layer launches, which have no images)
PATHS = {'images': ((256, 256), 'ReLU', 1), 'float32': ((256, 256), 'ReLU', 0),
         'uneven': ((48, 32), 'ReLU', None), 'elu3': ((32, 32, 32), 'ELU', None)}
KINDS = ('sac', 'td3', 'ddpg')
RECORDED = (-5.725, 3.5)              # Return(0.99): [_low, _high] = [-572.5, 350] — asymmetric, not the default
LOW, HIGH = -572.5, 350.0
DISCOUNT = 0.99


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def _model(kind, sizes, activation, with_return=True):
    import tonic_amd.torch as tt
    act = ACTIVATIONS[activation]
    if kind == 'sac':
        head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                            distribution=tt.models.SquashedMultivariateNormalDiag)
    elif kind == 'mpo':
        head = tt.models.GaussianPolicyHead()
    else:
        head = tt.models.DeterministicPolicyHead()
    container = tt.models.ActorTwinCriticWithTargets if kind in ('sac', 'td3') else tt.models.ActorCriticWithTargets
    return container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=tt.models.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd(),
        return_normalizer=tt.normalizers.Return(DISCOUNT) if with_return else None)


def _agent(kind, sizes, activation, B, with_return=True, seed=9, iterations=1, recorded=RECORDED, **extra):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    replay = tonic_amd.replays.Buffer(size=1000, batch_iterations=iterations, batch_size=B)
    cls = dict(sac=tt.agents.SAC, td3=tt.agents.TD3, ddpg=tt.agents.DDPG, mpo=tt.agents.MPO)[kind]
    agent = cls(model=_model(kind, sizes, activation, with_return), replay=replay, **extra)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=seed)
    if with_return and recorded is not None:
        rn = agent.model.return_normalizer
        rn.record(np.array(recorded, np.float32))
        rn.update()
        assert (float(rn._low), float(rn._high)) == (LOW, HIGH) and rn._low.is_cuda
    return agent


def _set_normalizer(agent, rng):
    norm = agent.model.observation_normalizer
    with torch.no_grad():
        norm._mean.copy_(torch.as_tensor(np.asarray(rng.normal(size=O) * 0.5, np.float32)))
        norm._std.copy_(torch.as_tensor(np.asarray(np.exp(rng.uniform(-1, 1, O)), np.float32)))


class SquashedRef(Ref):
    """The float64 networks of test_gpu_offpolicy_grads.Ref with the Return normaliser on every critic's head,
    online and target (models/critics.py:17-19)."""

    def __init__(self, agent, kind, layers, activation, low, high):
        super().__init__(agent, kind, layers, activation)
        self.low, self.high = float(low), float(high)

    def z(self, params, obs, act):
        return super().critic(params, obs, act)

    def critic(self, params, obs, act):
        return rs.squash64(self.z(params, obs, act), self.low, self.high)


def _critics(agent, kind):
    m = agent.model
    if kind in ('sac', 'td3'):
        return [m.critic_1, m.critic_2], [m.target_critic_1, m.target_critic_2]
    return [m.critic], [m.target_critic]


def _variables(module):
    from tonic_amd.torch.models import network_variables
    return list(network_variables(module))


def _spread_heads(agent, kind, ref, batch, spread=2.5):
    """Scales each critic's head (its target's alike) so that the float64 pre-activations z on the batch are centred
    with a standard deviation of `spread`: both regimes of the squash are then in the batch.  Returns the online
    critics' float64 z afterwards."""
    online, targets = _critics(agent, kind)
    d = {k: v.double() for k, v in batch.items()}
    out = []
    for c, t in zip(online, targets):
        with torch.no_grad():
            z = ref.z(_f64(c), d['observations'], d['actions'])
            w, b = _variables(c)[-2:]
            f = spread / float(z.std())
            mean_wh = float(z.mean()) - float(b.double().cpu())
            for net in (c, t):
                nw, nb = _variables(net)[-2:]
                nw.mul_(f)
                nb.fill_(-f * mean_wh)
            out.append(ref.z(_f64(c), d['observations'], d['actions']))
    return out


def _regimes(zs):
    """The condition on the inputs (float64 reference alone): at least 10 % of the rows saturated (|z| > 3), at least
    10 % in the linear part (|z| < 0.5), for every online critic."""
    for z in zs:
        z = z.abs()
        assert float((z > 3).double().mean()) >= 0.10 and float((z < 0.5).double().mean()) >= 0.10, \
            (float((z > 3).double().mean()), float((z < 0.5).double().mean()))


# batch seeds: 1000 + B, except where that batch does not put 10 % of its rows into each regime of the sigmoid
# (_regimes — checked on the CPU, from the float64 reference alone, when these tests were written)
SEEDS = {('sac', 'uneven', 33): 2, ('td3', 'elu3', 100): 1, ('ddpg', 'elu3', 100): 1}


def _case(kind, path, B, seed=None):
    sizes, activation, images = PATHS[path]
    rng = np.random.RandomState(SEEDS.get((kind, path, B), 1000 + B) if seed is None else seed)
    batch = _batch(rng, B, O, A)
    # (rewards on the scale of the range: the TD errors are then neither all tiny nor all of one sign)
    batch['rewards'] = batch['rewards'] * 40
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
    eps_actor = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
    return sizes, activation, images, rng, batch, eps, eps_actor


# ---------------------------------------------------------------- 1. gradient sums vs float64

@pytest.mark.parametrize('B', [100, 33])
@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('kind', KINDS)
def test_gradient_sums_vs_float64(lib, kind, path, B):
    """One critic step and one actor step of the *_ranged entries against float64 autograd of the reference's losses
    on squashed critics (targets too), range [-572.5, 350]: every tensor within 1e-5 of its largest element, loss /
    q1 / q2 / actor loss within 1e-5 (test_gpu_offpolicy_grads' _check / _check_stat).  B = 33: a ragged last tile.
    The heads are scaled until float64 z is spread over both regimes of the sigmoid (asserted on the reference)."""
    sizes, activation, images, rng, batch, eps, eps_actor = _case(kind, path, B)
    with _Images(lib, 1 if images is None else images):
        agent = _agent(kind, sizes, activation, B)
        assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
        assert agent._fused_kind() is None
        heads = 2 if kind == 'sac' else 1
        if images is not None:
            assert (lib.tonic_mlp_actor_image_bytes(O, sizes[0], A, heads) > 0) == bool(images)
        else:
            assert agent.critic_updater.hidden >= 1024          # a tonic_mlp_torso code: layer by layer
        _set_normalizer(agent, rng)
        ref = SquashedRef(agent, kind, len(sizes), activation, LOW, HIGH)
        zs = _spread_heads(agent, kind, ref, batch)
        _regimes(zs)
        out = _q_steps(agent, kind, batch, eps if kind != 'ddpg' else None, eps_actor, ref)
    print(f'{kind} {path} B={B}: largest relative error critic {out["critic"]:.2e} actor {out["actor"]:.2e}')


# ---------------------------------------------------------------- the entries, called directly

def _critic_call(agent, gpu, eps, form, low=None, high=None):
    """tonic_twin_q_grad* on the agent's buffers WITHOUT the optimizer step; form: 'old' tonic_twin_q_grad, 'loss'
    tonic_twin_q_grad_loss, 'ranged' tonic_twin_q_grad_ranged with low / high (device scalars or None).  Returns the
    gradient-sum block with its statistic slots."""
    from tonic_amd import _lib
    u, p, lib = agent.critic_updater, _lib.ptr, agent.lib
    B = gpu['observations'].shape[0]
    ws = u._offpolicy_workspace(B)
    mean, std = u.norm_tensors()
    noise = getattr(u, 'target_action_noise', None)
    args = [u.kind, p(u._policy_params()), p(agent.model.flat_target_critics.flat), p(u.flat.flat), p(mean), p(std),
            u.norm_clip(), p(gpu['observations']), p(gpu['actions']), p(gpu['next_observations']), p(gpu['rewards']),
            p(gpu['discounts']), p(eps), p(u.grad_sums), B, u.observation_size, u.hidden, u.action_size,
            float(getattr(u, 'entropy_coeff', 0.0)), float(noise.scale if noise else 0.0),
            float(noise.clip if noise else 0.0)]
    tail = [p(ws), ws.numel(), _lib.current_stream()]
    u.grad_sums.zero_()
    if form == 'old':
        _lib.check(lib.tonic_twin_q_grad(*args, *tail), 'tonic_twin_q_grad')
    elif form == 'loss':
        _lib.check(lib.tonic_twin_q_grad_loss(*args, ctypes.addressof(u.loss_rule), *tail), 'tonic_twin_q_grad_loss')
    else:
        _lib.check(lib.tonic_twin_q_grad_ranged(*args, ctypes.addressof(u.loss_rule), p(low), p(high), *tail),
                   'tonic_twin_q_grad_ranged')
    torch.cuda.synchronize()
    return u.grad_sums.clone()


def _actor_call(agent, observations, eps, form, low=None, high=None):
    from tonic_amd import _lib
    u, p, lib = agent.actor_updater, _lib.ptr, agent.lib
    B = observations.shape[0]
    ws = u._offpolicy_workspace(B)
    mean, std = u.norm_tensors()
    args = [u.kind, p(u.flat.flat), p(agent.model.flat_critics.flat), p(mean), p(std), u.norm_clip(),
            p(observations), p(eps), p(u.grad_sums), B, u.observation_size, u.hidden, u.action_size,
            float(getattr(u, 'entropy_coeff', 0.0))]
    tail = [p(ws), ws.numel(), _lib.current_stream()]
    u.grad_sums.zero_()
    if form == 'plain':
        _lib.check(lib.tonic_actor_q_grad(*args, *tail), 'tonic_actor_q_grad')
    else:
        _lib.check(lib.tonic_actor_q_grad_ranged(*args, p(low), p(high), *tail), 'tonic_actor_q_grad_ranged')
    torch.cuda.synchronize()
    return u.grad_sums.clone()


# ---------------------------------------------------------------- 2. no tolerance

def _rows(agent, kind, gpu, eps, low, high):
    """Every row of the batch as a batch of ONE through the plain and the squashed entry: with B = 1 the statistic
    slots q1 / q2 ARE the row's head outputs and the head bias's gradient sum IS the row's dq — the kernels' own z,
    v and head gradient through the public outputs.  Returns z, v, dq [nets, B] (float32)."""
    online, _ = _critics(agent, kind)
    u, nets, B = agent.critic_updater, len(online), gpu['observations'].shape[0]
    z, v, dq = (np.zeros((nets, B), np.float32) for _ in range(3))
    for r in range(B):
        one = {k: t[r:r + 1].contiguous() for k, t in gpu.items()}
        e = eps[r:r + 1].contiguous() if eps is not None else None
        plain = _critic_call(agent, one, e, 'ranged')
        z[:, r] = plain[u.count + 1:u.count + 1 + nets].cpu().numpy()
        got = _critic_call(agent, one, e, 'ranged', low, high)
        v[:, r] = got[u.count + 1:u.count + 1 + nets].cpu().numpy()
        grads = _grad_sums(online, got, 1)
        per_net = len(grads) // nets
        dq[:, r] = [float(grads[(n + 1) * per_net - 1]) for n in range(nets)]
    return z, v, dq


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('kind', KINDS)
def test_values_and_head_gradient_factor_without_tolerance(lib, kind, path):
    """The published v and the head's gradient against return_squash_ref in float32, fed the kernel's own z (read
    from a NULL / NULL run of the same parameters and rows), row by row (see _rows) and then as one batch of 33.

    v: within 2 ulp — of the operands of its last addition, ulp(max(|low|, |s t|, |v|)): device and NumPy exp differ by
    an ulp, which s and s t carry at THEIR magnitude; where low + s t cancels, an ulp of the small v is below what
    any float32 evaluation of the sum can resolve.  dq = value_squash_dz(2 (v - r), v) with discounts = 0 (so that
    y = r exactly): no exp in it, bit for bit.  The batch's q sums are the float64 sums of the rows' v, bit for bit:
    a row's value does not depend on its neighbours.  Head bias +inf / -inf gives exactly high / low, NaN gives NaN
    and leaves the twin critic of the same launch alone."""
    B = 33
    sizes, activation, images, rng, batch, eps, _ = _case(kind, path, B, seed=73)
    batch['discounts'] = torch.zeros(B)
    with _Images(lib, 1 if images is None else images):
        agent = _agent(kind, sizes, activation, B)
        _set_normalizer(agent, rng)
        ref = SquashedRef(agent, kind, len(sizes), activation, LOW, HIGH)
        _regimes(_spread_heads(agent, kind, ref, batch))
        rn, u = agent.model.return_normalizer, agent.critic_updater
        low, high = rn._low.data, rn._high.data
        gpu = {k: t.cuda() for k, t in batch.items()}
        eps_gpu = eps.cuda() if kind != 'ddpg' else None
        z, v, dq = _rows(agent, kind, gpu, eps_gpu, low, high)
        nets = z.shape[0]
        want_v = rs.squash32(z, LOW, HIGH)
        t = np.float32(HIGH - LOW)
        s = np.float32(1) / (np.float32(1) + np.exp(-z, dtype=np.float32))
        scale = np.maximum(np.maximum(np.abs(want_v), np.abs(s * t)), np.float32(abs(LOW)))
        distance = np.abs(v.astype(np.float64) - want_v.astype(np.float64)) / np.spacing(scale).astype(np.float64)
        print(f'{kind} {path}: v up to {distance.max():.2f} ulp of the sum\'s operands, '
              f'{rs.ulps(v, want_v).max():.1f} ulp of v; z in [{z.min():.2f}, {z.max():.2f}]')
        assert distance.max() <= 2.0, distance.max()
        assert (v >= LOW).all() and (v <= HIGH).all()
        rewards = batch['rewards'].numpy()
        want_dq = rs.squash_dz32(np.float32(2) * (v - rewards[None]).astype(np.float32), v, LOW, HIGH)
        np.testing.assert_array_equal(dq, want_dq)
        assert np.abs(want_dq).max() > 0
        # the whole batch in one launch: its rows are those rows
        got = _critic_call(agent, gpu, eps_gpu, 'ranged', low, high)
        sums = got[u.count + 1:u.count + 1 + nets].cpu().numpy()
        np.testing.assert_array_equal(sums, v.astype(np.float64).sum(1).astype(np.float32))
        # z = +inf / -inf / NaN through the head's bias (twin: the second critic keeps its own)
        online, _ = _critics(agent, kind)
        one = {k: t[:1].contiguous() for k, t in gpu.items()}
        e = eps_gpu[:1].contiguous() if eps_gpu is not None else None
        bias = _variables(online[0])[-1]
        for value, want in ((np.inf, HIGH), (-np.inf, LOW), (np.nan, np.nan)):
            with torch.no_grad():
                bias.fill_(value)
            z0 = _critic_call(agent, one, e, 'ranged')[u.count + 1].item()
            assert np.isnan(z0) if np.isnan(value) else z0 == value, (value, z0)
            got = _critic_call(agent, one, e, 'ranged', low, high)[u.count + 1:u.count + 1 + nets].cpu().numpy()
            np.testing.assert_array_equal(got[0], np.float32(want))
            if nets == 2:
                np.testing.assert_array_equal(got[1], v[1, 0])


# ---------------------------------------------------------------- 3. the plain head is what it was

@pytest.mark.parametrize('path', ['images', 'uneven'])
@pytest.mark.parametrize('kind', KINDS)
def test_null_range_is_the_plain_entry_bit_for_bit(lib, kind, path):
    """A model WITHOUT a Return normaliser: tonic_twin_q_grad_loss, tonic_twin_q_grad_ranged(..., NULL, NULL) and the
    pre-existing tonic_twin_q_grad leave the same bits in the gradient sums and the statistic slots; so do
    tonic_actor_q_grad and tonic_actor_q_grad_ranged(..., NULL, NULL).  (One of them squashed differs.)"""
    B = 100
    sizes, activation, images, rng, batch, eps, eps_actor = _case(kind, path, B, seed=5)
    with _Images(lib, 1 if images is None else images):
        agent = _agent(kind, sizes, activation, B, with_return=False)
        _set_normalizer(agent, rng)
        gpu = {k: t.cuda() for k, t in batch.items()}
        e = eps.cuda() if kind != 'ddpg' else None
        want = _critic_call(agent, gpu, e, 'loss').cpu().numpy()
        assert np.isfinite(want).all() and np.abs(want[:agent.critic_updater.count]).max() > 0
        for form in ('old', 'ranged'):
            np.testing.assert_array_equal(_critic_call(agent, gpu, e, form).cpu().numpy(), want, err_msg=form)
        ea = eps_actor.cuda() if kind == 'sac' else None
        want_actor = _actor_call(agent, gpu['observations'], ea, 'plain').cpu().numpy()
        assert np.isfinite(want_actor).all() and np.abs(want_actor[:agent.actor_updater.count]).max() > 0
        np.testing.assert_array_equal(_actor_call(agent, gpu['observations'], ea, 'ranged').cpu().numpy(), want_actor)
        low, high = torch.tensor(LOW, device='cuda'), torch.tensor(HIGH, device='cuda')
        assert not np.array_equal(_critic_call(agent, gpu, e, 'ranged', low, high).cpu().numpy(), want)
        assert not np.array_equal(_actor_call(agent, gpu['observations'], ea, 'ranged', low, high).cpu().numpy(),
                                  want_actor)


@pytest.mark.parametrize('kind', KINDS)
def test_fused_iteration_still_serves_the_model_without_a_normaliser(lib, kind):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    agent = dict(sac=tt.agents.SAC, td3=tt.agents.TD3, ddpg=tt.agents.DDPG)[kind]()
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=1)
    assert agent._fused_kind() is not None
    assert agent.critic_updater.return_normalizer is None and agent.actor_updater.return_normalizer is None


# ---------------------------------------------------------------- 4. a moved range under graph replay

def _filled(B, iterations, seed=5, rows=24, W=4):
    """A SAC agent with a Return normaliser (default range) on a filled buffer + two sets of index / noise streams."""
    agent = _agent('sac', (256, 256), 'ReLU', B, iterations=iterations, seed=seed, recorded=None)
    rng = np.random.RandomState(11)
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32)).cuda()       # noqa: E731
    host = dict(observations=rng.normal(size=(rows, W, O)), actions=rng.uniform(-1, 1, (rows, W, A)),
                next_observations=rng.normal(size=(rows, W, O)), rewards=rng.normal(size=(rows, W)) * 40,
                resets=rng.uniform(size=(rows, W)) < 0.1, terminations=rng.uniform(size=(rows, W)) < 0.05)
    for t in range(rows):
        agent.replay.store(**{k: dev(v[t]) for k, v in host.items()})
    streams = [(rng.randint(rows * W, size=(iterations, B)),
                rng.normal(size=(iterations, 2, B, A)).astype(np.float32)) for _ in range(2)]
    return agent, streams


def _snapshot(agent, infos):
    torch.cuda.synchronize()
    return dict(infos=infos.cpu().numpy().copy(), online=agent.model.flat_online.cpu().numpy(),
                target=agent.model.flat_target.cpu().numpy(),
                moments=agent.critic_updater.exp_avg.cpu().numpy())


def _two_calls(move):
    agent, streams = _filled(40, 2)
    assert agent._fused_kind() is None
    out = [_snapshot(agent, agent.enqueue_update(*streams[0]))]
    if move:
        rn = agent.model.return_normalizer
        rn.record(np.array([-9.0, 7.0], np.float32))
        rn.update()
        assert float(rn._low) < -800 and float(rn._high) > 600
    out.append(_snapshot(agent, agent.enqueue_update(*streams[1])))
    return out, agent


def test_a_moved_range_under_graph_replay(lib, monkeypatch):
    """Two SAC agents from identical seeds (B = 40, two iterations per update), one replaying a captured hipGraph,
    one with TONIC_AMD_NO_GRAPH=1: enqueue_update, record + update() with a wider range, enqueue_update again.
    Parameters, targets, moments and infos are the same bits after both calls — the kernels read _low / _high from
    the device, the graph is not re-captured — and the second call is not that of a range that did not move."""
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH', raising=False)
    graphed, agent = _two_calls(move=True)
    assert agent._graph is not None
    kept, _ = _two_calls(move=False)
    monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    launched, agent = _two_calls(move=True)
    assert agent._graph is None
    for call in range(2):
        for key in graphed[call]:
            np.testing.assert_array_equal(graphed[call][key], launched[call][key], err_msg=f'call {call} {key}')
        assert np.isfinite(graphed[call]['online']).all() and np.isfinite(graphed[call]['infos']).all()
    np.testing.assert_array_equal(graphed[0]['online'], kept[0]['online'])
    assert not np.array_equal(graphed[1]['online'], kept[1]['online'])
    assert not np.array_equal(graphed[1]['infos'], kept[1]['infos'])


# ---------------------------------------------------------------- 5. stock torsos

def test_stock_torsos_with_a_return_normaliser_vs_float64(lib):
    """A five-layer torso runs on stock torch operators (updater.stock), whose ValueHead squashes by itself: one TD3
    iteration (critic step, actor step) against the float64 restatement at the bound of test 1.

    Width and seed come from the float32 arithmetic of stock torch itself, measured on the CPU against the same
    float64 restatement (seeds 1 .. 12 that pass _regimes): five ReLU layers sit at 1.4e-6 .. 2.5e-6 of a tensor's
    largest element at widths 64 .. 256 (4.7e-6 .. 6.3e-6 at width 32), with outliers of 2e-5 .. 1e-4 at seeds where
    a pre-activation lies within float32 rounding of zero, so that its ReLU mask differs from float64's: no float32
    evaluation agrees with float64 there.  Width 64, seed 3: 1.5e-6 on the CPU, no such unit."""
    kind, sizes, B = 'td3', (64, 64, 64, 64, 64), 33
    rng = np.random.RandomState(3)
    batch = _batch(rng, B, O, A)
    batch['rewards'] = batch['rewards'] * 40
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
    agent = _agent(kind, sizes, 'ReLU', B)
    critic_u, actor_u = agent.critic_updater, agent.actor_updater
    assert critic_u.stock is True and actor_u.stock is True
    _set_normalizer(agent, rng)
    ref = SquashedRef(agent, kind, len(sizes), 'ReLU', LOW, HIGH)
    _regimes(_spread_heads(agent, kind, ref, batch))
    m = agent.model
    d = {k: v.double() for k, v in batch.items()}
    gpu = {k: v.cuda() for k, v in batch.items()}
    online = [_f64(m.critic_1), _f64(m.critic_2)]
    frozen = [_f64(m.target_critic_1), _f64(m.target_critic_2)]
    actor, target_actor = _f64(m.actor), _f64(m.target_actor)
    with torch.no_grad():
        noise = critic_u.target_action_noise
        a = ref.policy(target_actor, d['next_observations'])[0]
        a = torch.clamp(a + torch.clamp(noise.scale * eps.double(), -noise.clip, noise.clip), -1, 1)
        returns = d['rewards'] + d['discounts'] * torch.min(*[ref.critic(p, d['next_observations'], a) for p in frozen])
    qs = [ref.critic(p, d['observations'], d['actions']) for p in online]
    loss = sum(((q - returns) ** 2).mean() for q in qs)
    loss.backward()
    info = torch.zeros(8, device='cuda')
    critic_u.enqueue(gpu, eps.cuda(), info)
    got = [p.grad for p in critic_u.variables]
    leaves = [leaf for p in online for leaf in p]
    worst = _check(got, leaves, [f'critic {i}' for i in range(len(got))])
    row = info.cpu().numpy()
    _check_stat(row[0], loss.detach(), sum((q.detach() - returns) ** 2 for q in qs), 'critic loss')
    for i, q in enumerate(qs):
        _check_stat(row[1 + i], q.detach().mean(), q.detach(), f'q{i + 1}')
    online = [_f64(m.critic_1)]
    terms = -ref.critic(online[0], d['observations'], ref.policy(actor, d['observations'])[0])
    terms.mean().backward()
    actor_u.enqueue(gpu['observations'], None, info)
    worst_actor = _check([p.grad for p in actor_u.variables], actor, [f'actor {i}' for i in range(len(actor))])
    _check_stat(info.cpu().numpy()[0], terms.detach().mean(), terms.detach(), 'actor loss')
    print(f'stock td3: largest relative error critic {worst:.2e} actor {worst_actor:.2e}')


# ---------------------------------------------------------------- 6. the agents against the unmodified reference

GOLDENS = [('sac_return_small', 'sac'), ('td3_return_small', 'td3'), ('ddpg_return_small', 'ddpg')]
UPDATES = 3


def _golden_agent(g, kind):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    o, a, W, hidden, B, iterations, seed, loop_steps = (int(x) for x in g['cfg'])
    model = _model(kind, (hidden, hidden), 'ReLU')
    replay = tonic_amd.replays.Buffer(size=400, batch_iterations=iterations, batch_size=B,
                                      steps_before_batches=W * 10, steps_between_batches=W * 10)
    if kind == 'sac':
        agent = tt.agents.SAC(model=model, replay=replay,
                              exploration=tonic_amd.explorations.NoActionNoise(start_steps=W * 5))
    else:
        cls = {'ddpg': tt.agents.DDPG, 'td3': tt.agents.TD3}[kind]
        agent = cls(model=model, replay=replay,
                    exploration=tonic_amd.explorations.NormalActionNoise(start_steps=W * 5))
    agent.initialize(Box(-np.inf, np.inf, (o,)), Box(-1, 1, (a,)), seed=seed)
    return agent


def _state(g, u):
    """The reference's state in front of update u: nothing moves the model between two updates (asserted by
    scripts/make_offpolicy_return_goldens.py), so pre{u} is post{u-1}, init for the first."""
    prefix = 'init/' if u == 0 else f'post{u - 1}/'
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def _drive(agent, g, first, last, check=None):
    """agent.update over the recorded loop steps [first, last) with the recorded transitions; the learner updates
    triggered on the way draw the recorded index and noise streams of that update.  check(u): called after update u.
    Returns the updates that ran."""
    W = int(g['cfg'][2])
    at, done = {}, []
    agent.replay.sample_indices = lambda *a: g[f'u{at["u"]}/indices']
    agent._draw_noise = lambda iterations: g[f'u{at["u"]}/eps'].astype(np.float32)
    for t in range(first, last):
        at['u'] = int(np.searchsorted(g['updates'], t * W))        # the update this step triggers, if it triggers one
        agent.last_observations = g['act/observations'][t].astype(np.float32)
        agent.last_actions = g['act/actions'][t].astype(np.float32)
        agent._q.begin_step()
        before = getattr(agent, 'last_infos', None)
        agent.update(observations=g['act/next_observations'][t].astype(np.float32), rewards=g['act/rewards'][t],
                     resets=g['act/resets'][t], terminations=g['act/terminations'][t], steps=t * W)
        if getattr(agent, 'last_infos', None) is not before:
            assert g['updates'][at['u']] == t * W
            done.append(at['u'])
            if check is not None:
                check(at['u'])
    return done


@pytest.mark.parametrize('name,kind', GOLDENS)
def test_agents_match_the_unmodified_reference_every_update(lib, golden, name, kind):
    """The unmodified reference's SAC / TD3 / DDPG with Return(0.99) on rewards scaled by 3 (scripts/
    make_offpolicy_return_goldens.py), three learner updates; the tonic_amd agent is built from the same seed (init/
    equal bit for bit) and driven through agent.update with the recorded transitions.  After EACH update, started
    from the reference's own state in front of it: _low / _high and every head's copy equal the reference's bit for
    bit (host arithmetic on the recorded rewards); the parameter change post - pre within 1e-5 absolute and the
    logged critic/loss, critic/q*, actor/loss within rtol 1e-5 + 1e-5 — the tolerances of the *_small trajectory
    tests (test_gpu_offpolicy.test_offpolicy_update_matches_reference)."""
    g = golden(name)
    agent = _golden_agent(g, kind)
    state = agent.model.state_dict()
    for key in state:
        np.testing.assert_array_equal(state[key].cpu().numpy(), g['init/' + key], err_msg=key)
    assert sorted(state) == sorted(k[len('init/'):] for k in g.files if k.startswith('init/'))
    worst = {}

    def check(u):
        after = {k: v.detach().cpu().numpy() for k, v in agent.model.state_dict().items()}
        pre = _state(g, u)
        rn = agent.model.return_normalizer
        np.testing.assert_array_equal(np.array([rn.min_reward, rn.max_reward], np.float32), g[f'u{u}/return/range'])
        infos = agent.last_infos
        keys = [('critic/loss', infos[0][:, 0])]
        keys += [('critic/q_mean', infos[0][:, 1])] if kind == 'ddpg' else \
            [('critic/q1_mean', infos[0][:, 1]), ('critic/q2_mean', infos[0][:, 2])]
        ran = infos[1][:, 6] > 0
        keys.append(('actor/loss', infos[1][ran, 0]))
        for key, got in keys:
            want = g[f'u{u}/info/{key}']
            print(f'{name} update {u} {key}: max relative error {np.abs(got / want - 1).max():.2e}')
        for key, value in after.items():
            if 'return_normalizer' in key:
                np.testing.assert_array_equal(value, g[f'post{u}/{key}'], err_msg=key)
            elif 'normalizer' not in key:
                got, want = value - pre[key], g[f'post{u}/{key}'] - pre[key]
                worst[u] = max(worst.get(u, 0.0), float(np.abs(got - want).max()))
        print(f'{name} update {u}: largest |parameter change - reference\'s| {worst[u]:.2e}')
        for key, got in keys:
            np.testing.assert_allclose(got, g[f'u{u}/info/{key}'], rtol=1e-5, atol=1e-5, err_msg=f'{u} {key}')
        for key, value in after.items():
            if 'normalizer' not in key:
                np.testing.assert_allclose(value - pre[key], g[f'post{u}/{key}'] - pre[key], rtol=0, atol=1e-5,
                                           err_msg=f'{u} {key}')
        # the next update starts from the reference's own state (rounding does not accumulate across updates)
        agent.model.load_state_dict({k: torch.as_tensor(v) for k, v in _state(g, u + 1).items()})
        agent._q.parameters_changed()

    done = _drive(agent, g, 0, int(g['cfg'][7]), check)
    assert done == list(range(UPDATES))
    # the range moved on the way: the later updates squash with another [_low, _high] than the first
    lows = {float(g[f'post{u}/return_normalizer._low']) for u in range(UPDATES)}
    highs = {float(g[f'post{u}/return_normalizer._high']) for u in range(UPDATES)}
    assert len(lows) + len(highs) > 2 and -100.0 not in lows


# ---------------------------------------------------------------- 7. checkpoint

def test_checkpoint_between_two_updates(lib, golden, tmp_path):
    """save after update 2, load, update 3.  A .pt holds the model alone (the reference's keys; Adam's moments and
    the buffer are not in it), so the agent that loads is a second one driven through the same first two updates —
    with its range knocked off before the load, which must restore it IN PLACE (the kernels and a captured graph
    read _low / _high through the pointers they had).  Update 3 is then bit-identical to the uninterrupted run."""
    g = golden('td3_return_small')
    steps, second = int(g['cfg'][7]), int(g['updates'][1]) // int(g['cfg'][2]) + 1
    straight, loaded = _golden_agent(g, 'td3'), _golden_agent(g, 'td3')
    assert _drive(straight, g, 0, second) == [0, 1]
    assert _drive(loaded, g, 0, second) == [0, 1]
    path = str(tmp_path / 'checkpoint' / 'step')
    straight.save(path)
    saved = torch.load(path + '.pt')
    for key in ('return_normalizer._low', 'return_normalizer._high', 'critic.head.return_normalizer._low',
                'critic_1.head.return_normalizer._low', 'critic_2.head.return_normalizer._high',
                'target_critic_1.head.return_normalizer._low', 'target_critic_2.head.return_normalizer._high'):
        assert key in saved and saved[key].shape == (), key
    rn = loaded.model.return_normalizer
    pointers = rn._low.data_ptr(), rn._high.data_ptr()
    with torch.no_grad():
        rn._low.fill_(-1.0)
        rn._high.fill_(1.0)
    loaded.load(path)
    assert (rn._low.data_ptr(), rn._high.data_ptr()) == pointers and rn._low.is_cuda
    assert float(rn._low) == float(saved['return_normalizer._low']) != -1.0
    assert loaded.model.critic_1.head.return_normalizer is rn and loaded.model.target_critic_2.head.return_normalizer is rn
    loaded._q.parameters_changed()
    assert _drive(straight, g, second, steps) == [2] and _drive(loaded, g, second, steps) == [2]
    a, b = straight.model.state_dict(), loaded.model.state_dict()
    for key in a:
        np.testing.assert_array_equal(a[key].cpu().numpy(), b[key].cpu().numpy(), err_msg=key)
    np.testing.assert_array_equal(straight.last_infos, loaded.last_infos)
    assert not np.array_equal(a['critic_1.head.v_layer.weight'].cpu().numpy(), saved['critic_1.head.v_layer.weight'].numpy())


# ---------------------------------------------------------------- MPO keeps raising where it did

def test_mpo_with_a_return_normaliser_raises_at_its_first_update(lib):
    """MPO's updaters have no squashed form: it constructs, initialises and acts, and its first agent.update raises
    NotImplementedError('return normalisers are not supported') AFTER the store, as before."""
    import tonic_amd.torch as tt
    agent = _agent('mpo', (256, 256), 'ReLU', 16, recorded=None)
    assert tt.agents.MPO.serves_return_normalizer is False and tt.agents.SAC.serves_return_normalizer is True
    observations = np.zeros((2, O), np.float32)
    actions = agent.step(observations, 0)
    assert actions.shape == (2, A)
    with pytest.raises(NotImplementedError, match='return normalisers are not supported'):
        agent.update(observations=observations, rewards=np.ones(2, np.float32), resets=np.zeros(2, bool),
                     terminations=np.zeros(2, bool), steps=0)
    agent.settle()
    assert agent.replay.size == 1                                  # the transition was stored first
    rn = agent.model.return_normalizer
    assert (rn.min_reward, rn.max_reward) == (-1, 1)
