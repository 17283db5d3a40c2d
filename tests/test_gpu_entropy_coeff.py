"""GPU tests of SAC's learned entropy coefficient (tonic_tempered_twin_q_grad / tonic_tempered_actor_q_grad,
updaters.EntropyCoeffTuning, agents.SAC(entropy_coeff_updater=...)).

1  bit identity: a coefficient pointer to 0.0f (expf(0) = 1 exactly) against the *_ranged entries with
   entropy_coeff = 1.0, and a NULL pointer against the *_ranged entries with 0.2 — every byte of both gradient-sum
   blocks, on the three routes (fp16x2 weight images, float32 one-launch, layer by layer), with and without a range;
2  both entries' gradient sums, their logged statistics and the coefficient's own sums against float64
   (tests/entropy_coeff_ref.py, tests/test_gpu_offpolicy_grads.py's rules) at log_alpha in {log 0.2, log 5, -10};
3  five iterations through the updaters: log_entropy_coeff bit for bit the optimizer family's statement from the sums
   read back (tests/test_gpu_optim_family_updaters.py's rule) and within a derived bound of the float64 trajectory;
4  a captured update graph follows the moving coefficient: replays equal eager updates bit for bit, no re-capture;
5  the agent on a synthetic environment: route, logs, checkpoint; a five-layer torso on stock operators;
6  two ranks equal one process.

Shapes are the smallest at which the kernels can go wrong (row tiles of 16: B in {1, 16, 17, 100}; (O, A) in
{(3, 1), (17, 6)}), not SAC's own."""
import ctypes
import math
import os

import numpy as np
import pytest

import entropy_coeff_ref as ref
import optim_family_ref as family
from test_gpu_offpolicy_grads import Ref, _agent, _batch, _check_stat, _f64, _Images, _q_steps, _set_normalizer

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROUTES = {'images': ((256, 256), 'ReLU', 1), 'float32': ((256, 256), 'ReLU', 0), 'layers': ((48, 32), 'Tanh', 1)}
BATCHES = (1, 16, 17, 100)
SHAPES = ((3, 1), (17, 6))
LOG_ALPHAS = (math.log(0.2), math.log(5.0), -10.0)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


def bits(tensor):
    torch.cuda.synchronize()
    return np.ascontiguousarray(tensor.detach().cpu().numpy()).view(np.int32)


def _tuner(agent, initial=1.0, optimizer=None, target_entropy=None):
    """An EntropyCoeffTuning attached to an initialised SAC agent's updaters (what SAC.initialize does)."""
    from tonic_amd.torch import updaters
    tuner = updaters.EntropyCoeffTuning(target_entropy=target_entropy, initial_entropy_coeff=initial,
                                        optimizer=optimizer)
    tuner.initialize(agent.model, agent.action_size)
    agent.entropy_coeff_updater = tuner
    agent.critic_updater.entropy_coeff_updater = agent.actor_updater.entropy_coeff_updater = tuner
    return tuner


def _set_log_alpha(tuner, value):
    with torch.no_grad():
        tuner.log_entropy_coeff.fill_(value)
    return float(tuner.log_entropy_coeff)          # (the float32 the kernels read)


def _route_agent(route, O, A, B):
    sizes, activation, _ = ROUTES[route]
    agent = _agent('sac', O, A, B, sizes=sizes, activation=activation)
    rng = np.random.RandomState(O * 11 + A)
    _set_normalizer(agent, rng.normal(size=O) * 0.5, np.exp(rng.uniform(-1, 1, O)))
    return agent, rng


# ---------------------------------------------------------------- 1. bit identity

def _twin(agent, entry, batch, eps, coeff, value_range=(None, None), log_alpha=()):
    """One call of a critic-step entry into a fresh gradient-sum block, NaN where the entry writes nothing (the layout's
    padding), and no optimizer step; `log_alpha`: () for the
    *_ranged entry, (tensor or None,) for the tempered one."""
    from tonic_amd import _lib
    u, p = agent.critic_updater, _lib.ptr
    B = batch['observations'].shape[0]
    ws, (mean, std) = u._offpolicy_workspace(B), u.norm_tensors()
    out = torch.full_like(u.grad_sums, float('nan'))
    _lib.check(getattr(u.lib, entry)(
        1, p(agent.model.flat_actor.flat), p(agent.model.flat_target_critics.flat), p(u.flat.flat), p(mean), p(std),
        u.norm_clip(), p(batch['observations']), p(batch['actions']), p(batch['next_observations']),
        p(batch['rewards']), p(batch['discounts']), p(eps), p(out), B, u.observation_size, u.hidden, u.action_size,
        float(coeff), 0.0, 0.0, ctypes.addressof(u.loss_rule), *[p(v) for v in value_range],
        *[p(v) for v in log_alpha], p(ws), ws.numel(), _lib.current_stream()), entry)
    return bits(out)


def _actor(agent, entry, batch, eps, coeff, value_range=(None, None), temper=None):
    """One call of an actor-step entry; `temper`: None for the *_ranged entry, (log_alpha, sums, target) else."""
    from tonic_amd import _lib
    u, p = agent.actor_updater, _lib.ptr
    B = batch['observations'].shape[0]
    ws, (mean, std) = u._offpolicy_workspace(B), u.norm_tensors()
    out = torch.full_like(u.grad_sums, float('nan'))
    more = () if temper is None else (p(temper[0]), p(temper[1]), float(temper[2]))
    _lib.check(getattr(u.lib, entry)(
        1, p(u.flat.flat), p(agent.model.flat_critics.flat), p(mean), p(std), u.norm_clip(), p(batch['observations']),
        p(eps), p(out), B, u.observation_size, u.hidden, u.action_size, float(coeff),
        *[p(v) for v in value_range], *more, p(ws), ws.numel(), _lib.current_stream()), entry)
    return bits(out)


def _identity_case(lib, route, O, A, B, value_range=(None, None)):
    with _Images(lib, ROUTES[route][2]):
        agent, rng = _route_agent(route, O, A, B)
        served = lib.tonic_mlp_actor_image_bytes(O, agent.critic_updater.hidden, A, 2) > 0
        assert served == (route == 'images'), (route, served)           # the route the case names is the one taken
        batch = {k: v.cuda() for k, v in _batch(rng, B, O, A).items()}
        eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32).cuda()
        eps_actor = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32).cuda()
        zero = torch.zeros(1, device='cuda')
        sums = torch.full((9,), float('nan'), device='cuda')
        # a pointer to 0.0f: alpha = expf(0) = 1
        want = _twin(agent, 'tonic_twin_q_grad_ranged', batch, eps, 1.0, value_range)
        got = _twin(agent, 'tonic_tempered_twin_q_grad', batch, eps, 0.2, value_range, (zero,))
        assert np.array_equal(got, want), ('critic', route, O, A, B)
        want = _actor(agent, 'tonic_actor_q_grad_ranged', batch, eps_actor, 1.0, value_range)
        got = _actor(agent, 'tonic_tempered_actor_q_grad', batch, eps_actor, 0.2, value_range, (zero, sums, -A))
        assert np.array_equal(got, want), ('actor', route, O, A, B)
        written = sums.cpu().numpy()
        assert np.isfinite(written).all() and written[6] == B and written[3] == B and written[1] == 0.0
        # a NULL pointer: the entropy_coeff argument, the *_ranged entry's launches and bits
        want = _twin(agent, 'tonic_twin_q_grad_ranged', batch, eps, 0.2, value_range)
        got = _twin(agent, 'tonic_tempered_twin_q_grad', batch, eps, 0.2, value_range, (None,))
        assert np.array_equal(got, want), ('critic, NULL', route, O, A, B)
        want = _actor(agent, 'tonic_actor_q_grad_ranged', batch, eps_actor, 0.2, value_range)
        got = _actor(agent, 'tonic_tempered_actor_q_grad', batch, eps_actor, 0.2, value_range, (None, None, -A))
        assert np.array_equal(got, want), ('actor, NULL', route, O, A, B)
        # ... and 1.0 is not 0.2: the comparison above can tell coefficients apart
        assert not np.array_equal(_actor(agent, 'tonic_actor_q_grad_ranged', batch, eps_actor, 1.0, value_range), want)


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('O,A', SHAPES)
@pytest.mark.parametrize('B', BATCHES)
def test_bit_identity_at_log_alpha_zero_and_with_null(lib, route, O, A, B):
    _identity_case(lib, route, O, A, B)


@pytest.mark.parametrize('route', ROUTES)
def test_bit_identity_with_a_value_range(lib, route):
    low, high = torch.tensor([-3.0], device='cuda'), torch.tensor([5.0], device='cuda')
    _identity_case(lib, route, 17, 6, 17, (low, high))


# ---------------------------------------------------------------- 2. against float64

@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('O,A', SHAPES)
@pytest.mark.parametrize('B', BATCHES)
def test_entries_and_coefficient_sums_vs_float64(lib, route, O, A, B):
    """Gradient sums of both entries per tensor within 1e-5 of the tensor's largest element and the logged statistics
    by `_check_stat` (through test_gpu_offpolicy_grads._q_steps, whose float64 statements read the coefficient off
    the updaters' floats: they are set to exp of the float32 the kernels read); the coefficient's sums by
    `_check_stat`, whose floor of the mean absolute term the sum of both signs needs."""
    sizes, activation, images = ROUTES[route]
    with _Images(lib, images):
        agent, rng = _route_agent(route, O, A, B)
        tuner = _tuner(agent)
        model_ref = Ref(agent, 'sac', len(sizes), activation)
        batch = _batch(rng, B, O, A)
        worst = {}
        for wanted in LOG_ALPHAS:
            log_alpha = _set_log_alpha(tuner, wanted)
            agent.critic_updater.entropy_coeff = agent.actor_updater.entropy_coeff = math.exp(log_alpha)
            eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
            eps_actor = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)
            actor64 = _f64(agent.model.actor)              # (the critic step leaves the actor alone)
            tuner.grad_sums.fill_(float('nan'))
            out = _q_steps(agent, 'sac', batch, eps, eps_actor, model_ref)
            with torch.no_grad():
                log_probs = ref.squashed_sample(*model_ref.policy(actor64, batch['observations'].double()),
                                                eps_actor.double())[1]
            want = ref.coeff_sums(log_alpha, log_probs, tuner.target_entropy)
            torch.cuda.synchronize()
            got = tuner.grad_sums.cpu().numpy()
            print(f'{route} O={O} A={A} B={B} log_alpha={log_alpha:.4f}: coefficient sums {got[:4]} want '
                  f'{float(want["grad"]):.9g} {float(want["loss"]):.9g} {float(want["log_prob"]):.9g}')
            assert got[6] == B and not got[[4, 5, 7, 8]].any(), got
            errors = [_check_stat(got[0], want['grad'], want['terms'], 'coefficient gradient sum'),
                      _check_stat(got[1], want['loss'], log_alpha * want['terms'], 'coefficient loss sum'),
                      _check_stat(got[2], want['log_prob'], log_probs, 'log-probability sum')]
            assert abs(got[3] - math.exp(log_alpha) * B) <= 1e-6 * math.exp(log_alpha) * B, got
            worst[round(wanted, 3)] = (out['critic'], out['actor'], max(errors))
        print(f'{route} O={O} A={A} B={B}: largest relative error (critic, actor, coefficient sums)', worst)


# ---------------------------------------------------------------- 3. the step

def _iterate(agent, tuner, batches, noises, model_ref, rule_name, k):
    """k iterations through the updaters (critic, actor, coefficient) on fixed batches.  Returns the trajectories of
    log_entropy_coeff: the device's, the family's float32 statement from the sums read back (with its state
    buffers), and the float64 restatement's, which reads the actor the device holds before each iteration."""
    info = torch.zeros(8, device='cuda')
    names = family.slot_names(tuner.hyper)
    p = tuner.log_entropy_coeff.cpu().numpy().copy()
    slots = [np.zeros(1, np.float32) for _ in names]
    coefficient = ref.Coefficient(float(p[0]), tuner.target_entropy, ref.OPTIMIZERS[rule_name])
    device, statement, restated, rows = [], [], [], []
    for it in range(k):
        batch, (eps, eps_actor) = batches[it % len(batches)], noises[it % len(noises)]
        B = batch['observations'].shape[0]
        actor64 = _f64(agent.model.actor)
        gpu = {key: v.cuda() for key, v in batch.items()}
        agent.critic_updater.enqueue(gpu, eps.cuda(), info)
        agent.actor_updater.enqueue(gpu['observations'], eps_actor.cuda(), info)
        row = torch.zeros(8, device='cuda')
        tuner.enqueue_step(row, B)
        torch.cuda.synchronize()
        sums = tuner.grad_sums.cpu().numpy()
        p, slots = family.family_statement(tuner.hyper, p, sums[:1], slots, it + 1, 1.0 / B)
        with torch.no_grad():
            log_probs = ref.squashed_sample(*model_ref.policy(actor64, batch['observations'].double()),
                                            eps_actor.double())[1]
        coefficient.step(log_probs)
        device.append(tuner.log_entropy_coeff.cpu().numpy().copy())
        statement.append(p.copy())
        restated.append(coefficient.value)
        rows.append(row.cpu().numpy())
    assert int(tuner.state[0]) == k
    return np.concatenate(device), np.concatenate(statement), np.array(restated), np.array(rows)


def _check_trajectory(device, statement, restated, start):
    """Bit for bit the statement from the read-back sums (the existing updater tests' rule for a stepped parameter).
    Against float64: per step 2^-22 max(1, |log_alpha|) — the float32 parameter and the rule's float32 constants, an
    ulp each — plus 1e-4 of the step: the gradient sum is within 1e-5 (test 2) and a rule of the family carries a
    relative gradient error into its step at most a few times over (Adam and RMSprop normalise it away, momentum
    averages it), rounded up to 1e-4; the allowances add up along the trajectory."""
    assert np.array_equal(device.view(np.int32), statement.view(np.int32)), (device, statement)
    allowed, before = 0.0, start
    for it, (got, want) in enumerate(zip(device, restated)):
        allowed += 2.0 ** -22 * max(1.0, abs(want)) + 1e-4 * abs(want - before)
        print(f'  iteration {it + 1}: log_entropy_coeff {got!r} float64 {want!r} allowed {allowed:.3g}')
        assert abs(float(got) - want) <= allowed, (it, float(got), want, allowed)
        before = want
    assert abs(device[-1] - start) > 1e-4         # it moved


@pytest.mark.parametrize('rule', ['adam_fast', 'sgd', 'rmsprop', 'adam'])
def test_coefficient_steps_by_the_rule(lib, rule):
    O, A, B, k = 17, 6, 17, 5
    agent, rng = _route_agent('images', O, A, B)
    tuner = _tuner(agent, initial=0.5, optimizer=ref.OPTIMIZERS[rule])
    start = float(tuner.log_entropy_coeff)
    batches = [_batch(rng, B, O, A) for _ in range(2)]
    noises = [(torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32),
               torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)) for _ in range(3)]
    device, statement, restated, rows = _iterate(agent, tuner, batches, noises, Ref(agent, 'sac', 2, 'ReLU'), rule, k)
    print(f'{rule}: ', end='')
    if rule == 'adam':          # lr = 3e-4, the default: five steps of ~lr
        assert np.array_equal(device.view(np.int32), statement.view(np.int32))
        np.testing.assert_allclose(device, restated, rtol=0, atol=5 * 2.0 ** -22 + 1e-4 * 5 * 3e-4)
    else:
        _check_trajectory(device, statement, restated, start)
    # the logged row: {loss, mean log-prob, alpha BEFORE the step}
    alphas = np.exp(np.concatenate([[start], device[:-1]]).astype(np.float64))
    np.testing.assert_allclose(rows[:, 2], alphas, rtol=1e-6)
    assert np.isfinite(rows).all() and (rows[:, 6] == 1.0).all()


# ---------------------------------------------------------------- 4. graph

def _filled_agent(B, iterations, sizes=(256, 256), tuner_kwargs=None, O=17, A=6, rows=30, W=4, tuned=True):
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    activation = torch.nn.ReLU
    head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                        distribution=tt.models.SquashedMultivariateNormalDiag)
    model = tt.models.ActorTwinCriticWithTargets(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, activation), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, activation),
                                head=tt.models.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())
    tuner = tt.updaters.EntropyCoeffTuning(**(tuner_kwargs or {})) if tuned else None
    agent = tt.agents.SAC(model=model, entropy_coeff_updater=tuner,
                          replay=tonic_amd.replays.Buffer(size=rows * W, batch_iterations=iterations, batch_size=B,
                                                          steps_before_batches=0, steps_between_batches=1))
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=7)
    rng = np.random.RandomState(321)
    for _ in range(rows - 3):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        row = {k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()}
        agent.replay.store(normalizer=agent.model.observation_normalizer, **row)
    return agent


def _updates(agent, calls, iterations, B, A):
    """`calls` update calls with indices and noise of their own; (rows of every call, the graphs seen)."""
    rng = np.random.RandomState(5)
    out, graphs = [], []
    for _ in range(calls):
        indices = rng.randint(0, agent.replay.size * agent.replay.global_workers, size=(iterations, B)).astype(np.int64)
        eps = rng.normal(size=(iterations, 2, B, A)).astype(np.float32)
        infos = agent.enqueue_update(indices, eps)
        torch.cuda.synchronize()
        out.append((infos.cpu().numpy().copy(), agent._u.slot.stats.cpu().numpy().copy(),
                    agent.entropy_coeff_updater.log_entropy_coeff.cpu().numpy().copy()))
        graphs.append(agent._u.slot.graph)
    return out, graphs


def test_captured_graph_follows_the_coefficient(lib, monkeypatch):
    B, iterations, A = 17, 3, 6
    fast = dict(initial_entropy_coeff=0.5, optimizer=lambda params: torch.optim.Adam(params, lr=0.05))
    monkeypatch.delenv('TONIC_AMD_NO_GRAPH', raising=False)
    captured = _filled_agent(B, iterations, tuner_kwargs=fast)
    assert captured._u.route().fused_kind is None
    got, graphs = _updates(captured, 5, iterations, B, A)        # the capture's own update, then four replays
    assert graphs[0] is not None and all(g is graphs[0] for g in graphs), 'the graph was captured again'
    monkeypatch.setenv('TONIC_AMD_NO_GRAPH', '1')
    eager = _filled_agent(B, iterations, tuner_kwargs=fast)
    want, none = _updates(eager, 5, iterations, B, A)
    assert all(g is None for g in none)
    for call, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(('infos', 'coefficient rows', 'log_entropy_coeff'), g, w):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (call, name)
    for key, value in captured.model.state_dict().items():
        assert np.array_equal(bits(value), bits(eager.model.state_dict()[key])), key
    trajectory = np.concatenate([g[2] for g in got])
    assert len(set(trajectory.tolist())) == 5 and np.isfinite(got[-1][0]).all()        # it moved on every replay
    captured.close()
    eager.close()


# ---------------------------------------------------------------- 5. the agent

def _run(agent, steps=12, O=3, A=2, W=2, seed=3):
    import tonic_amd
    from tonic_amd import logger
    env = tonic_amd.environments.distribute(lambda: tonic_amd.environments.Synthetic(O, A, max_episode_steps=5), 1, W)
    env.initialize(seed=seed)
    agent.initialize(env.observation_space, env.action_space, seed=seed)
    observations, updates, stored = env.start(), [], {}
    original = logger.store
    logger.store = lambda key, value, **kw: stored.setdefault(key, []).append(float(value))
    try:
        for t in range(steps):
            actions = agent.step(observations, t * W)
            assert np.isfinite(actions).all()
            observations, infos = env.step(actions)
            before = int(agent.critic_updater.state[0])
            agent.update(**infos, steps=t * W)
            if int(agent.critic_updater.state[0]) != before:
                updates.append(t)
    finally:
        logger.store = original
    return stored, updates


def _loop_agent(tuner, sizes=None, W=2):
    import tonic_amd
    import tonic_amd.torch as tt
    replay = tonic_amd.replays.Buffer(size=200, batch_iterations=2, batch_size=17, steps_before_batches=W * 4,
                                      steps_between_batches=W * 4)
    model = None
    if sizes is not None:
        head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                            distribution=tt.models.SquashedMultivariateNormalDiag)
        model = tt.models.ActorTwinCriticWithTargets(
            actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, torch.nn.ReLU),
                                  head=head),
            critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(),
                                    torso=tt.models.MLP(sizes, torch.nn.ReLU), head=tt.models.ValueHead()),
            observation_normalizer=tt.normalizers.MeanStd())
    return tt.agents.SAC(model=model, replay=replay, entropy_coeff_updater=tuner)


KEYS = ('entropy_coeff/loss', 'entropy_coeff/value', 'entropy_coeff/entropy')


def test_agent_with_a_tuner_on_a_synthetic_environment(lib, tmp_path):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    fast = lambda params: torch.optim.Adam(params, lr=0.01)             # noqa: E731
    agent = _loop_agent(tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=0.5, optimizer=fast))
    stored, updates = _run(agent)
    tuner = agent.entropy_coeff_updater
    assert len(updates) >= 2 and int(tuner.state[0]) == int(agent.actor_updater.state[0]) >= 4
    route = agent._u.route()
    assert route.fused_kind is None and not agent.critic_updater.stock and tuner.target_entropy == -2.0
    for key in KEYS:
        assert len(stored[key]) == int(tuner.state[0]) and np.isfinite(stored[key]).all(), key
    assert stored['entropy_coeff/value'][0] == pytest.approx(0.5, rel=1e-6)      # alpha before the first step
    assert len(set(stored['entropy_coeff/value'])) == len(stored['entropy_coeff/value'])
    final = bits(tuner.log_entropy_coeff)
    assert abs(float(tuner.log_entropy_coeff) - math.log(0.5)) > 1e-3            # alpha moved
    # save / load: the .pt as ever, the coefficient beside it
    path = str(tmp_path / 'agent')
    agent.save(path)
    assert sorted(torch.load(path + '.entropy_coeff.pt')) == ['log_entropy_coeff']
    assert sorted(torch.load(path + '.pt', map_location='cpu')) == sorted(agent.model.state_dict())
    spaces = Box(-np.inf, np.inf, (3,)), Box(-1, 1, (2,))
    fresh = _loop_agent(tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=2.0))
    fresh.initialize(*spaces, seed=99)
    fresh.load(path)
    assert np.array_equal(bits(fresh.entropy_coeff_updater.log_entropy_coeff), final)
    for key, value in agent.model.state_dict().items():
        assert np.array_equal(bits(fresh.model.state_dict()[key]), bits(value)), key
    os.remove(path + '.entropy_coeff.pt')           # a checkpoint without the sibling file (the reference's): the
    again = _loop_agent(tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=2.0))        # initial value stays
    again.initialize(*spaces, seed=99)
    again.load(path)
    assert float(again.entropy_coeff_updater.log_entropy_coeff) == float(np.float32(math.log(2.0)))
    # a plain SAC is what it was: the fused iteration, no file beside the .pt
    plain = _loop_agent(None)
    plain_stored, _ = _run(plain)
    assert plain._u.route().fused_kind == 1 and plain._stats_width() == 0
    assert not any(key.startswith('entropy_coeff/') for key in plain_stored)
    plain.save(str(tmp_path / 'plain'))
    assert not os.path.exists(str(tmp_path / 'plain') + '.entropy_coeff.pt')
    for a in (agent, fresh, again, plain):
        a.close()


def test_five_layer_torso_runs_on_stock_operators(lib):
    """A torso outside the kernels (five layers): the updaters' stock-torch forms with alpha = exp(log_entropy_coeff)
    kept a tensor, the coefficient's sums from the same log-probabilities, the step through tonic_optimizer_step."""
    import tonic_amd.torch as tt
    sizes = (24, 16, 24, 16, 8)
    fast = lambda params: torch.optim.Adam(params, lr=0.01)             # noqa: E731
    agent = _loop_agent(tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=0.5, optimizer=fast), sizes)
    stored, updates = _run(agent)
    tuner = agent.entropy_coeff_updater
    assert agent.critic_updater.stock and agent.actor_updater.stock and agent._u.route().fused_kind is None
    assert len(updates) >= 2 and int(tuner.state[0]) >= 4
    for key in KEYS:
        assert len(stored[key]) == int(tuner.state[0]) and np.isfinite(stored[key]).all(), key
    assert abs(float(tuner.log_entropy_coeff) - math.log(0.5)) > 1e-3
    # the trajectory against float64, five more iterations on fixed batches through the same updaters
    O, A, B = 3, 2, 17
    rng = np.random.RandomState(11)
    fresh = tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=0.5, optimizer=ref.OPTIMIZERS['adam_fast'])
    fresh.initialize(agent.model, A)
    agent.entropy_coeff_updater = fresh
    agent.critic_updater.entropy_coeff_updater = agent.actor_updater.entropy_coeff_updater = fresh
    start = float(fresh.log_entropy_coeff)
    batches = [_batch(rng, B, O, A) for _ in range(2)]
    noises = [(torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32),
               torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32)) for _ in range(3)]
    device, statement, restated, rows = _iterate(agent, fresh, batches, noises, Ref(agent, 'sac', len(sizes), 'ReLU'),
                                                 'adam_fast', 5)
    _check_trajectory(device, statement, restated, start)
    agent.close()


# ---------------------------------------------------------------- 6. two ranks

def test_two_ranks_equal_single_process(tmp_path):
    """Sharded Buffer + global index / noise streams: two ranks give the update one process holding the whole buffer
    gives, parameters and log_entropy_coeff (tests/test_gpu_multirank.py's launcher, time limit and tolerances)."""
    from test_gpu_multirank import launch
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mp_entropy_coeff_worker.py')
    outs = {}
    for world in (1, 2):
        outs[world] = str(tmp_path / f'tuned{world}.npz')
        launch(world, outs[world], 29911 + world, command=(worker,))
    a, b = np.load(outs[1]), np.load(outs[2])
    np.testing.assert_allclose(b['infos'], a['infos'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(b['coeff_infos'], a['coeff_infos'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(b['log_entropy_coeff'], a['log_entropy_coeff'], rtol=0, atol=2e-5)
    assert abs(float(a['log_entropy_coeff'][0]) - math.log(0.5)) > 1e-2
    for key in a.files:
        if key in ('infos', 'coeff_infos', 'log_entropy_coeff'):
            continue
        diff = np.abs(b[key] - a[key])          # (Adam and float32-noise gradient elements: test_gpu_multirank.py)
        assert diff.max() < 3e-3 and np.mean(diff > 2e-5) < 1e-3, (key, diff.max())
