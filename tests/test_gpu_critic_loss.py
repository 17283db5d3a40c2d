"""GPU tests of `loss=` on the off-policy critic updaters (tonic_critic_loss_t: L1, smooth-L1 and Huber beside MSE).

1. gradient sums and the logged loss of SAC / TD3 / DDPG / MPO's ExpectedSARSA against float64 autograd of the torch
   loss OBJECT, on the image passes, the float32 passes and the layer-by-layer torsos, with the TD errors prescribed
   away from the kinks;
2. the kink itself without tolerance: the kernel's dq against the float32 restatement (tests/critic_loss_ref.py) of
   the kernel's own error, bit for bit, a NaN row included;
3. MSE is what it was: the old entries, the new ones with NULL and with an explicit MSE rule, bit for bit;
4. the fused iteration (whole, in phases, policy passes riding ahead, replayed from a graph) equals the split entries
   bit for bit under a Huber loss, and a changed loss re-captures;
5. the stock-torch form applies the same loss;
6. the agents take the updaters and log the float64 loss."""
import numpy as np
import pytest

import critic_loss_ref as rule
from test_gpu_offpolicy_grads import Ref, _agent, _batch, _check, _check_stat, _f64, _Images, _stats
from test_gpu_offpolicy_torsos import _grad_sums

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu
nn = torch.nn

O, A, S = 17, 6, 20
HUBER_DELTA = 0.75
LOSSES = {'l1': lambda: nn.L1Loss(), 'smooth': lambda: nn.SmoothL1Loss(beta=0.5),
          'smooth0': lambda: nn.SmoothL1Loss(beta=0), 'huber': lambda: nn.HuberLoss(delta=HUBER_DELTA)}
# (sizes, activation, q_images): the plain torso on the fp16x2 images and on the float32 passes (one-launch chains:
# mlpimg_body.h / mlp_backward_body + mlp_loss_stats), an uneven and a three-layer torso (layer by layer:
# critic_loss_kernel)
PATHS = {'images': ((256, 256), 'ReLU', 1), 'float32': ((256, 256), 'ReLU', 0), 'uneven': ((48, 32), 'ReLU', 1),
         'elu3': ((32, 32, 32), 'ELU', 1)}


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def dev(x):
    return torch.as_tensor(np.asarray(x, np.float32), device='cuda')


def _critics(agent, kind):
    m = agent.model
    if kind in ('sac', 'td3'):
        return [m.critic_1, m.critic_2], [m.target_critic_1, m.target_critic_2]
    return [m.critic], [m.target_critic]


def _next_values(agent, kind, ref, d, eps):
    """float64 value of the next state as the critic step of `kind` forms it (critics.py:72-79, 156-167, 202-221,
    253-270), from the agent's parameters."""
    m, u = agent.model, agent.critic_updater
    frozen = [_f64(c) for c in _critics(agent, kind)[1]]
    nxt_obs = d['next_observations']
    B = nxt_obs.shape[0]
    with torch.no_grad():
        if kind == 'sac':
            loc, scale = ref.policy(_f64(m.actor), nxt_obs)
            raw = loc + scale * eps.double()
            a = torch.tanh(raw)
            logp = (torch.distributions.Normal(loc, scale).log_prob(raw) - torch.log(1 - a ** 2 + 1e-6)).sum(-1)
            return torch.min(*[ref.critic(p, nxt_obs, a) for p in frozen]) - u.entropy_coeff * logp
        if kind == 'mpo':
            loc, scale = ref.policy(_f64(m.target_actor), nxt_obs)
            a = (loc[None] + scale[None] * eps.double().view(S, B, A)).reshape(S * B, A)
            return ref.critic(frozen[0], nxt_obs.repeat(S, 1), a).view(S, B).mean(0)
        a = ref.policy(_f64(m.target_actor), nxt_obs)[0]
        if kind == 'td3':
            noise = u.target_action_noise
            a = torch.clamp(a + torch.clamp(noise.scale * eps.double(), -noise.clip, noise.clip), -1, 1)
            return torch.min(*[ref.critic(p, nxt_obs, a) for p in frozen])
        return ref.critic(frozen[0], nxt_obs, a)


def _kinks(loss):
    kind, param = rule.rule_of(loss)
    return [0.0] if kind == rule.L1 or param == 0 else [-param, param]


def _branch(loss, e):
    """Which piece of the rule an error is on: the sign for L1, quadratic / linear otherwise."""
    kind, param = rule.rule_of(loss)
    return e > 0 if kind == rule.L1 or param == 0 else e.abs() < param


def _prescribed_errors(rng, loss, B, offsets):
    """|e_b| uniform in [0.05, 0.8 p] u [1.2 p, 4 p] (L1: [0.05, 3]), half of the rows in each part, signs at random
    places.  The signs are 55 : 45 in number, not 50 : 50: db3 is the plain sum of dq over the batch, and under these
    rules dq is a bounded sign-like quantity, so with balanced signs that one-element tensor cancels to ~1e-3 of its
    terms, below what float32 errors q - y carry into it (seen: 1.02e-5 of a sum that had fallen to 0.2 of 256
    terms); 55 : 45 keeps it at a tenth of its terms and every branch within 40 .. 60 %.
    `offsets`: q_z - q_1 of the other critics, whose errors e_b + offset must keep 0.04 from every kink as well: a
    row that does not is drawn again (same part, same sign)."""
    kind, param = rule.rule_of(loss)
    kinks = np.asarray(_kinks(loss))
    lower = np.arange(B) % 2 == 0
    signs = np.where(rng.permutation(B) < round(0.55 * B), 1.0, -1.0)

    def draw(n, low_part):
        if len(kinks) == 1:
            return rng.uniform(0.05, 3.0, n)
        return np.where(low_part, rng.uniform(0.05, 0.8 * param, n), rng.uniform(1.2 * param, 4 * param, n))

    def bad(e):
        every = np.stack([e] + [e + o for o in offsets])
        return (np.abs(every[:, :, None] - kinks[None, None, :]).min(-1) < 0.045).any(0)

    e = draw(B, lower) * signs
    for _ in range(200):
        again = bad(e)
        if not again.any():
            break
        e[again] = draw(int(again.sum()), lower[again]) * signs[again]
    return e


def _loss_case(agent, kind, ref, loss, B, seed):
    """One critic step under `loss` against float64 autograd of the loss object; returns the largest relative error."""
    u = agent.critic_updater
    rng = np.random.RandomState(seed)
    batch = _batch(rng, B, O, A)
    eps = torch.as_tensor(rng.normal(size=(S * B if kind == 'mpo' else B, A)), dtype=torch.float32)
    online_modules = _critics(agent, kind)[0]
    online = [_f64(c) for c in online_modules]
    d = {k: v.double() for k, v in batch.items()}
    nxt = _next_values(agent, kind, ref, d, eps)
    with torch.no_grad():
        q64 = [ref.critic(p, d['observations'], d['actions']) for p in online]
    e = _prescribed_errors(rng, loss, B, [(q - q64[0]).numpy() for q in q64[1:]])
    batch['rewards'] = (q64[0] - torch.as_tensor(e) - d['discounts'] * nxt).float()
    d['rewards'] = batch['rewards'].double()
    returns = d['rewards'] + d['discounts'] * nxt
    qs = [ref.critic(p, d['observations'], d['actions']) for p in online]
    # the reference's call: loss(values, returns), ExpectedSARSA loss(returns, values) (critics.py:79,175,227,275)
    terms = [loss(returns, q) if kind == 'mpo' else loss(q, returns) for q in qs]
    total = sum(terms)
    total.backward()
    # the float64 errors stand where they were prescribed: no row near a kink, every branch populated
    for q in qs:
        err = (q.detach() - returns)
        distance = min(float((err - k).abs().min()) for k in _kinks(loss))
        assert distance >= 0.04, (kind, distance)
        share = float(_branch(loss, err).double().mean())
        assert 0.4 <= share <= 0.6, (kind, share)
    u.loss = loss
    u.enqueue({k: v.cuda() for k, v in batch.items()}, eps.cuda() if kind != 'ddpg' else None,
              torch.zeros(8, device='cuda'))
    stats = _stats(u)
    assert stats[5] == B, stats
    got = _grad_sums(online_modules, u.grad_sums, B)
    leaves = [leaf for p in online for leaf in p]
    worst = _check(got, leaves, [f'critic {i}' for i in range(len(got))])
    functional = type(loss)(reduction='none', **{k: getattr(loss, k) for k in ('beta', 'delta') if hasattr(loss, k)})
    rows = sum(functional(q.detach(), returns) for q in qs)
    stat = _check_stat(stats[0] / B, total.detach(), rows, 'critic loss')
    for i, q in enumerate(qs):
        _check_stat(stats[1 + i] / B, q.detach().mean(), q.detach(), f'q{i + 1}')
    return max(worst, stat)


@pytest.mark.parametrize('B', [37, 256])
@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('kind', ['sac', 'td3', 'ddpg', 'mpo'])
def test_critic_loss_grads_vs_float64(lib, kind, path, B):
    """Gradient sums (every tensor within 1e-5 of its largest element) and the logged loss and q means (_check_stat)
    of one critic step under L1Loss(), SmoothL1Loss(beta=0.5), SmoothL1Loss(beta=0) and HuberLoss(delta=0.75) against
    float64 autograd of the loss object — the bound tests/test_gpu_offpolicy_grads.py holds MSE to.  O = 17, A = 6;
    B = 37 leaves 11 padded rows and a partly filled wave, B = 256 is several tiles.  The gradient of every rule jumps
    or bends at its kinks, where a float32 error on the other side of float64's would differ by O(1): the rewards are
    set from the float64 values so that every error is the prescribed one, at least 0.04 from a kink (asserted), half
    of the rows on each branch (asserted)."""
    sizes, activation, images = PATHS[path]
    errors = {}
    with _Images(lib, images):
        agent = _agent(kind, O, A, B, sizes=sizes, activation=activation, S=S)
        plain = sizes == (256, 256)
        assert (agent.critic_updater.hidden == 256) == plain
        if plain and kind != 'mpo':
            assert (lib.tonic_mlp_actor_image_bytes(O, 256, A, 2 if kind == 'sac' else 1) > 0) == bool(images)
        rng = np.random.RandomState(B + len(sizes))
        norm = agent.model.observation_normalizer
        with torch.no_grad():
            norm._mean.copy_(dev(rng.normal(size=O) * 0.3))
            norm._std.copy_(dev(np.exp(rng.uniform(-0.5, 0.5, O))))
        ref = Ref(agent, kind, len(sizes), activation)
        for seed, (name, make) in enumerate(LOSSES.items()):
            errors[name] = _loss_case(agent, kind, ref, make(), B, 100 + seed)
    print(f'{kind} {path} B={B}: largest relative error', {k: f'{v:.1e}' for k, v in errors.items()})


# ---------------------------------------------------------------- 2. the kink, bit for bit

def _find_rows(workspace, want, tolerance=1e-3):
    """Offset (in floats) of the len(want) consecutive floats of a workspace that equal `want` within `tolerance`:
    where the entry keeps dq (its layout is the entry's own business)."""
    ws = workspace.view(torch.float32).cpu().numpy()
    with np.errstate(invalid='ignore'):
        starts = np.flatnonzero(np.abs(ws[:len(ws) - len(want)] - want[0]) < tolerance)
        hits = [int(s) for s in starts if np.all(np.abs(ws[s:s + len(want)] - want) < tolerance)]
    assert len(hits) == 1, hits
    return hits[0]


@pytest.mark.parametrize('path', ['images', 'float32', 'uneven'])
def test_dq_at_the_kink_is_the_float32_rule_bit_for_bit(lib, path):
    """DDPG, B = 37.  The MSE rule writes dq = 2 e with e the kernel's own float32 error q - y (exact), so e is read
    back from the entry's workspace; the rewards of some rows are then moved so that e lands on +-param and next to
    it, one row's reward is NaN, and e is read again.  Under Huber, smooth-L1 (beta > 0 and beta = 0) and L1 the dq
    the kernels write must be the restatement of tests/critic_loss_ref.py on that e, every bit of every row; the NaN
    row gives NaN (0 where the rule is the sign alone) and the logged loss is NaN."""
    B, param = 37, 0.5
    sizes, activation, images = PATHS[path]
    with _Images(lib, images):
        agent = _agent('ddpg', O, A, B, sizes=sizes, activation=activation)
        u = agent.critic_updater
        rng = np.random.RandomState(3)
        batch = _batch(rng, B, O, A)
        ref = Ref(agent, 'ddpg', len(sizes), activation)
        d = {k: v.double() for k, v in batch.items()}
        nxt = _next_values(agent, 'ddpg', ref, d, None)
        with torch.no_grad():
            q64 = ref.critic(_f64(agent.model.critic), d['observations'], d['actions'])
        e64 = (q64 - d['rewards'] - d['discounts'] * nxt).numpy()

        parameters = agent.model.flat_online.clone()

        def run(loss, rewards):
            u.loss = loss
            gpu = {k: v.cuda() for k, v in batch.items()}
            gpu['rewards'] = dev(rewards)
            u.enqueue(gpu, None, torch.zeros(8, device='cuda'))
            torch.cuda.synchronize()
            agent.model.flat_online.copy_(parameters)         # (enqueue also steps the critic: every run from the same)
            return u.workspace.view(torch.float32)

        rewards = batch['rewards'].numpy().copy()
        at = _find_rows(run(None, rewards), (2 * e64).astype(np.float32))
        e = run(None, rewards)[at:at + B].cpu().numpy() / np.float32(2)
        np.testing.assert_allclose(e, e64, rtol=0, atol=1e-4)
        # rows 0 .. 7: the error moved onto +-param and a few float32 steps to either side (y moves with the reward)
        wanted = np.float32(param) * np.asarray([1, -1, 1, -1, 1, -1, 1, -1], np.float32)
        steps = np.asarray([0, 0, 1, 1, -1, -1, 3, -3], np.float32) * np.spacing(np.float32(param))
        rewards[:8] = rewards[:8] + (e[:8] - (wanted + steps))
        rewards[8] = np.nan
        e = run(None, rewards)[at:at + B].cpu().numpy() / np.float32(2)
        assert np.isnan(e[8]) and np.isnan(_stats(u)[0])
        # (the reward and the target round at their own magnitude, a few float32 steps of param)
        near = np.abs(np.abs(e[:8]) - np.float32(param)) <= 64 * np.spacing(np.float32(param))
        assert near.all(), e[:8]
        sides = np.abs(e[:8]) >= np.float32(param)
        assert sides.any() and not sides.all(), e[:8]          # both sides of the kink are hit
        for loss in (nn.HuberLoss(delta=param), nn.SmoothL1Loss(beta=param), nn.SmoothL1Loss(beta=0), nn.L1Loss()):
            kind, p = rule.rule_of(loss)
            got = run(loss, rewards)[at:at + B].cpu().numpy()
            want = rule.loss_dq(e, kind, p)
            sign_only = kind == rule.L1 or p == 0
            assert (got[8] == 0) if sign_only else np.isnan(got[8]), (type(loss).__name__, got[8])
            assert np.array_equal(got.view(np.uint32)[np.arange(B) != 8], want.view(np.uint32)[np.arange(B) != 8]), \
                (type(loss).__name__, e[got != want], got[got != want], want[got != want])
            assert np.isnan(_stats(u)[0]), type(loss).__name__
            # and the logged loss of the finite rows is the restatement's sum
            finite = rewards.copy()
            finite[8] = 0.0
            run(None, finite)
            e_finite = u.workspace.view(torch.float32)[at:at + B].cpu().numpy() / np.float32(2)
            run(loss, finite)
            want_sum = rule.loss_term(e_finite, kind, p).astype(np.float64).sum()
            assert abs(_stats(u)[0] - want_sum) <= 1e-6 * want_sum, (type(loss).__name__, _stats(u)[0], want_sum)


# ---------------------------------------------------------------- 3. MSE is untouched

class _Route:
    """The library with tonic_twin_q_grad_loss routed: 'old' = the entry without a loss argument, 'null' = NULL,
    'explicit' = the updater's own rule."""

    def __init__(self, lib, mode):
        self._lib, self._mode = lib, mode

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def tonic_twin_q_grad_loss(self, *args):
        if self._mode == 'old':
            return self._lib.tonic_twin_q_grad(*args[:21], *args[22:])
        if self._mode == 'null':
            return self._lib.tonic_twin_q_grad_loss(*args[:21], None, *args[22:])
        return self._lib.tonic_twin_q_grad_loss(*args)


def _filled_agent(kind, B, iterations, rows=24, W=4, delay_steps=None, critic=None, actor=None, sizes=None, seed=5):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    rng = np.random.RandomState(11)
    host = dict(observations=rng.normal(size=(rows, W, O)), actions=rng.uniform(-1, 1, (rows, W, A)),
                next_observations=rng.normal(size=(rows, W, O)), rewards=rng.normal(size=(rows, W)) * 2,
                resets=rng.uniform(size=(rows, W)) < 0.1, terminations=rng.uniform(size=(rows, W)) < 0.05)
    extra = dict(delay_steps=delay_steps) if delay_steps else {}
    if sizes is not None:
        from test_gpu_offpolicy_torsos import _model
        extra['model'] = _model(kind, sizes, 'ReLU')
    agent = dict(sac=tt.agents.SAC, td3=tt.agents.TD3, ddpg=tt.agents.DDPG, mpo=tt.agents.MPO)[kind](
        replay=tonic_amd.replays.Buffer(size=rows * W, batch_iterations=iterations, batch_size=B),
        critic_updater=critic, **(dict(actor_updater=actor) if actor is not None else {}), **extra)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=seed)
    norm = agent.model.observation_normalizer
    norm._mean.data.copy_(dev(np.random.RandomState(1).normal(size=O) * 0.3))
    norm._std.data.copy_(dev(np.abs(np.random.RandomState(2).normal(size=O)) + 0.5))
    for t in range(rows):
        agent.replay.store(**{k: dev(v[t]) for k, v in host.items()})
    draws = 2 if kind in ('sac', 'mpo') else 1
    per_row = S if kind == 'mpo' else 1
    eps = rng.normal(size=(iterations, draws, B * per_row, A)).astype(np.float32)
    indices = rng.randint(rows * W, size=(iterations, B))
    return agent, indices, eps


def _state(agent, infos):
    return dict(infos=np.stack(infos), online=agent.model.flat_online.cpu().numpy(),
                target=agent.model.flat_target.cpu().numpy(), sums=agent.critic_updater.grad_sums.cpu().numpy(),
                critic_m=agent.critic_updater.exp_avg.cpu().numpy(),
                steps=np.array([int(agent.critic_updater.state[0]), int(agent.actor_updater.state[0])]))


def _assert_same(got, want, label):
    for key in want:
        if not np.array_equal(got[key], want[key], equal_nan=True):
            where = np.argwhere(got[key] != want[key])
            raise AssertionError((label, key, len(where), tuple(where[0]), got[key][tuple(where[0])],
                                  want[key][tuple(where[0])]))


@pytest.mark.parametrize('kind', ['sac', 'td3'])
def test_mse_is_bit_identical_through_old_and_new_entries(lib, monkeypatch, kind):
    """loss=None and loss=MSELoss(), three iterations of the update path on the split entries: gradient sums with
    their statistic slots, logged rows, parameters and moments are the same bits through tonic_twin_q_grad (the
    entry as it was), tonic_twin_q_grad_loss with NULL and with an explicit {TONIC_LOSS_MSE} rule."""
    import tonic_amd.torch as tt
    monkeypatch.setenv('TONIC_AMD_FUSED_ITERATION', '0')
    critic = dict(sac=tt.updaters.TwinCriticSoftQLearning, td3=tt.updaters.TwinCriticDeterministicQLearning)[kind]
    results = {}
    for form in ('none', 'mse'):
        for mode in ('old', 'null', 'explicit'):
            agent, indices, eps = _filled_agent(kind, 100, 3, critic=critic(loss=None if form == 'none' else nn.MSELoss()))
            assert agent._fused_kind() is None and agent.critic_updater.loss_rule.kind == rule.MSE
            agent.critic_updater.lib = _Route(agent.critic_updater.lib, mode)
            infos = [agent.enqueue_update(indices, eps, graph=False).cpu().numpy().copy()]
            results[form, mode] = _state(agent, infos)
    want = results['none', 'old']
    assert np.isfinite(want['online']).all() and want['steps'][0] == 3
    assert np.abs(want['sums']).max() > 0
    for key, got in results.items():
        _assert_same(got, want, key)


# ---------------------------------------------------------------- 4. fused iteration = split entries

@pytest.mark.parametrize('kind,B,delay', [('sac', 256, None), ('td3', 100, 2)])
def test_fused_iteration_equals_split_entries_under_huber(lib, monkeypatch, kind, B, delay):
    """Four iterations under HuberLoss(delta=1) through tonic_q_iteration — whole (phase 0, replayed from a graph;
    TD3 with delay_steps = 2: the policy passes of every other iteration ride ahead, stage 2) and in phases 1 / 2
    (gradient clipping on both updaters) — against the split entries: parameters, targets, moments, sums, step
    counters and every info row bit for bit, as test_fused_iteration_equals_the_split_entry_points has it for MSE.
    Then ONLY the updater's loss changes: the captured graph must not be replayed under the old rule (the second call
    equals the split entries' again, which never capture)."""
    import tonic_amd.torch as tt
    critic, actor = dict(
        sac=(tt.updaters.TwinCriticSoftQLearning, tt.updaters.TwinCriticSoftDeterministicPolicyGradient),
        td3=(tt.updaters.TwinCriticDeterministicQLearning, tt.updaters.DeterministicPolicyGradient))[kind]
    monkeypatch.setenv('TONIC_AMD_UPDATE_CHUNK', '0')
    results = {}
    for mode, env, clip, graph in (('split', ('TONIC_AMD_FUSED_ITERATION', '0'), 0, False),
                                   ('fused', ('TONIC_AMD_FUSED_ITERATION', '1'), 0, True),
                                   ('split-clip', ('TONIC_AMD_FUSED_PHASES', '0'), 0.9, False),
                                   ('phases', ('TONIC_AMD_FUSED_PHASES', '1'), 0.9, False)):
        monkeypatch.setenv('TONIC_AMD_FUSED_ITERATION', '1')
        monkeypatch.setenv('TONIC_AMD_FUSED_PHASES', '1')
        monkeypatch.setenv(*env)
        agent, indices, eps = _filled_agent(kind, B, 4, delay_steps=delay,
                                            critic=critic(loss=nn.HuberLoss(delta=1.0), gradient_clip=clip),
                                            actor=actor(gradient_clip=clip))
        assert (agent._fused_kind() is not None) == (mode in ('fused', 'phases'))
        assert agent._fused_in_phases() == (mode == 'phases')
        if mode == 'fused' and delay:
            assert lib.tonic_q_iteration_ahead_supported(B, O, 256, A, 2, 2)
        infos = [agent.enqueue_update(indices, eps, graph=graph).cpu().numpy().copy()]
        first_graph = agent._graph
        agent.critic_updater.loss = nn.SmoothL1Loss(beta=0.5)
        infos.append(agent.enqueue_update(indices, eps, graph=graph).cpu().numpy().copy())
        if graph:
            assert first_graph is not None and agent._graph is not first_graph
        results[mode] = _state(agent, infos)
    assert np.isfinite(results['split']['online']).all() and np.isfinite(results['split']['infos']).all()
    # the loss rows are Huber's, not MSE's: the errors of this batch reach beyond delta
    assert list(results['split']['steps']) == [8, 8 if kind == 'sac' else 4]
    _assert_same(results['fused'], results['split'], 'fused')
    _assert_same(results['phases'], results['split-clip'], 'phases')


def test_huber_rows_differ_from_mse_rows(lib, monkeypatch):
    """(The power of the test above: on its batch the Huber rule is not the MSE rule.)"""
    import tonic_amd.torch as tt
    rows = {}
    for name, loss in (('mse', None), ('huber', nn.HuberLoss(delta=1.0))):
        agent, indices, eps = _filled_agent('sac', 256, 1, critic=tt.updaters.TwinCriticSoftQLearning(loss=loss))
        rows[name] = float(agent.enqueue_update(indices, eps, graph=False)[0, 0, 0])
    assert rows['huber'] < 0.8 * rows['mse'], rows


# ---------------------------------------------------------------- 5. the stock-torch form

def test_stock_torch_form_applies_the_same_loss(lib, monkeypatch):
    """SAC on a (48, 32) ReLU torso under SmoothL1Loss(beta=0.5): three updates on stock torch operators
    (TONIC_AMD_TORSO_STOCK=1) against the HIP entries, parameters within the 1e-5 both forms are held to against the
    reference's update (test_offpolicy_update_matches_reference / ..._as_stock_torch_operators)."""
    import tonic_amd.torch as tt
    results = {}
    for stock in ('0', '1'):
        monkeypatch.setenv('TONIC_AMD_TORSO_STOCK', stock)
        agent, indices, eps = _filled_agent('sac', 64, 3, sizes=(48, 32),
                                            critic=tt.updaters.TwinCriticSoftQLearning(loss=nn.SmoothL1Loss(beta=0.5)))
        assert agent.critic_updater.stock == (stock == '1') and agent.actor_updater.stock == (stock == '1')
        infos = agent.enqueue_update(indices, eps).cpu().numpy().copy()
        results[stock] = {k: v.detach().cpu().numpy().copy() for k, v in agent.model.state_dict().items()}, infos
    (hip, hip_infos), (stock, stock_infos) = results['0'], results['1']
    np.testing.assert_allclose(hip_infos[0][:, 0], stock_infos[0][:, 0], rtol=1e-5, atol=1e-5)
    worst = 0.0
    for key, want in stock.items():
        if 'normalizer' in key:
            continue
        np.testing.assert_allclose(hip[key], want, rtol=0, atol=1e-5, err_msg=key)
        worst = max(worst, float(np.abs(hip[key] - want).max()))
    print(f'stock vs HIP under smooth-L1: largest parameter difference {worst:.2e}')


# ---------------------------------------------------------------- 6. the agents

@pytest.mark.parametrize('kind', ['mpo', 'sac'])
def test_agents_take_the_updaters_and_log_the_float64_loss(lib, kind):
    """tt.agents.MPO(critic_updater=ExpectedSARSA(loss=HuberLoss())) and tt.agents.SAC(critic_updater=
    TwinCriticSoftQLearning(loss=SmoothL1Loss())) initialise on the HIP entries (stock is False), run one update, and
    the logged critic/loss is the float64 value of the loss object on the batch the update drew."""
    import tonic_amd.torch as tt
    B = 64
    if kind == 'mpo':
        loss = nn.HuberLoss()
        critic = tt.updaters.ExpectedSARSA(loss=loss)
    else:
        loss = nn.SmoothL1Loss()
        critic = tt.updaters.TwinCriticSoftQLearning(loss=loss)
    agent, indices, eps = _filled_agent(kind, B, 1, critic=critic)
    assert agent.critic_updater.stock is False and agent.actor_updater.stock is False
    assert agent.critic_updater.loss is loss
    flat = {k: v.flatten(0, 1) for k, v in agent.replay.buffers.items()}
    batch = {k: flat[k][torch.as_tensor(indices[0], device='cuda')].cpu() for k in
             ('observations', 'actions', 'next_observations', 'rewards', 'discounts')}
    d = {k: v.double() for k, v in batch.items()}
    ref = Ref(agent, kind, 2, 'ReLU')
    critic_eps = torch.as_tensor(eps[0, 0])
    nxt = _next_values(agent, kind, ref, d, critic_eps)
    returns = d['rewards'] + d['discounts'] * nxt
    with torch.no_grad():
        qs = [ref.critic(_f64(c), d['observations'], d['actions']) for c in _critics(agent, kind)[0]]
        want = sum(loss(returns, q) if kind == 'mpo' else loss(q, returns) for q in qs)
        rows = sum(type(loss)(reduction='none')(q, returns) for q in qs)
    infos = agent.enqueue_update(indices, eps).cpu().numpy()
    _check_stat(infos[0][0, 0], want, rows, 'critic/loss')
    assert want > 0
