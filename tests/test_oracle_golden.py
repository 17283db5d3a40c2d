"""Pins the CPU oracle (oracle/numpy_port.py) against golden vectors produced by the
unmodified reference (oracle/make_golden.py).  Runs on CPU, no reference checkout needed."""
import numpy as np
import pytest

import numpy_port as port

PPO_CASES = ['ppo_halfcheetah_small', 'ppo_pendulum_small', 'ppo_antbullet_small',
             'ppo_halfcheetah_w256', 'ppo_ant_wide', 'ppo_humanoid_wide']


def test_lambda_returns_bit_exact(golden):
    g = golden('lambda_returns')
    for i in range(int(g['n_cases'])):
        for j in range(4):
            k = f'c{i}_{j}_'
            ret = port.lambda_returns(g[k + 'next_values'], g[k + 'rewards'], g[k + 'resets'],
                                      g[k + 'terminations'], float(g[k + 'gamma']),
                                      float(g[k + 'lambda']))
            assert np.array_equal(ret, g[k + 'returns']), k
            adv = port.normalized_advantages(ret, g[k + 'values'])
            assert np.array_equal(adv, g[k + 'advantages'], equal_nan=True), k
            # affine form (what the chunked HIP scan composes) stays within fp32 rounding
            aff = port.lambda_returns_affine(g[k + 'next_values'], g[k + 'rewards'],
                                             g[k + 'resets'], g[k + 'terminations'],
                                             float(g[k + 'gamma']), float(g[k + 'lambda']))
            scale = max(1.0, np.abs(aff).max())
            assert np.abs(aff - ret).max() <= 2e-5 * scale, k
    const = port.normalized_advantages(np.full((4, 3), 2, np.float32), np.ones((4, 3), np.float32))
    assert np.array_equal(const.reshape(-1), g['const_advantages'])


def test_lambda_returns_f64_reference(golden):
    """lambda_returns_f64 is the float32 chain's recurrence with the float32 chain's scalars: it
    stays within float32 rounding of the chain on the goldens (per column, no floor), equals it
    exactly where every operation is exact in float32, and its output depends on the scalars'
    float32 rounding, not on their Python value."""
    g = golden('lambda_returns')
    for i in range(int(g['n_cases'])):
        for j in range(4):
            k = f'c{i}_{j}_'
            args = [g[k + n] for n in ('next_values', 'rewards', 'resets', 'terminations')]
            gamma, lam = float(g[k + 'gamma']), float(g[k + 'lambda'])
            ref = port.lambda_returns_f64(*args, gamma, lam)
            assert ref.dtype == np.float64
            err = np.abs(ref - g[k + 'returns']).max(axis=0)
            assert (err <= 1e-5 * np.abs(ref).max(axis=0)).all(), k
            nudged = port.lambda_returns_f64(*args, float(np.float32(gamma)), lam)
            assert np.array_equal(nudged, ref), k
    # small integers, gamma = lambda = 1: every product and sum is exact in both precisions
    rng = np.random.RandomState(3)
    nv, rew = (rng.randint(-8, 9, size=(40, 6)).astype(np.float32) for _ in range(2))
    rst = (rng.uniform(size=(40, 6)) < 0.2).astype(np.float32)
    term = rst * (rng.uniform(size=(40, 6)) < 0.5).astype(np.float32)
    assert np.array_equal(port.lambda_returns_f64(nv, rew, rst, term, 1.0, 1.0),
                          port.lambda_returns(nv, rew, rst, term, 1.0, 1.0).astype(np.float64))


ADAM_LR, ADAM_GRAD_SCALE = 3e-4, 1.0 / 37


def adam_case(n, steps, seed, warm=False):
    """Inputs of the optimizer tests here and in test_gpu_optim.py -> p, m, v, [gradient SUMS of each step].
    Parameters ~ N(0, 1); gradient means N(0, 1) x 10 ** U(-6, 1), drawn anew per step and element, with a block of
    exact zeros [n/2, n/2 + n/5) in every step; `warm`: moments as a long run leaves them (m ~ 0.3 s N(0, 1),
    v = (s U(0.5, 1.5)) ** 2 with s = 10 ** U(-6, 1) per element) instead of zeros."""
    rng = np.random.RandomState([n % 65521, steps, seed, int(warm)])
    p = rng.normal(size=n).astype(np.float32)
    sums = []
    for _ in range(steps):
        g = (rng.normal(size=n) * 10 ** rng.uniform(-6, 1, size=n) / ADAM_GRAD_SCALE).astype(np.float32)
        g[n // 2:n // 2 + n // 5] = 0.0
        sums.append(g)
    if warm:
        s = 10 ** rng.uniform(-6, 1, size=n)
        m = (rng.normal(size=n) * 0.3 * s).astype(np.float32)
        v = np.square(s * rng.uniform(0.5, 1.5, size=n)).astype(np.float32)
    else:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    return p, m, v, sums


def test_adam_statement_against_torch_and_float64():
    """`adam_statement` (the float32 expression of the HIP kernels) over 7 steps of 50 000 elements.

    Against `adam_f64`: the largest distance in `adam_f64_unit`s (one ulp of the parameter + lr * 2**-23) is
    MEASURED here and must not exceed `ADAM_F64_UNITS`, which the GPU tests double.  Measured (torch 2.10 / NumPy
    2.2): from zero state 0.9 / 1.2 / 1.7 / 2.5 / 2.7 / 2.6 / 2.9 units after steps 1 .. 7, from step 1000 with warm
    moments 1.6 / 2.5 / 4.1 / 7.0 / 5.1 / 8.0 / 8.0; the largest absolute error 7.9e-7 = 1.7 ulps of that parameter
    = 2.6e-3 x lr.

    Against torch.optim.Adam on the CPU: step 1 — `exp_avg` bit-identical, `exp_avg_sq` bit-identical for AdamPort
    and within 2 ulps for the statement (measured: 13 771 elements differ); later torch's `lerp_` fuses
    and matches neither (`exp_avg_sq`: the addend's ulp and one flipped rounding per step, so 2 ulps per step are
    allowed; measured 3 after 7).  Parameters: each step can flip the parameter's
    rounding (one ulp) and moves the update by a few ulps of lr, so the bound is 2 units per step; measured after
    7 steps 3.1 units, 2.4e-7 at most (one ulp of a parameter >= 2; the bound is one ulp of the largest)."""
    torch = pytest.importorskip('torch')
    n, steps = 50_000, 7
    worst_units = worst_abs = 0.0
    for start, warm in ((0, False), (999, True)):
        p, m, v, sums = adam_case(n, steps, 11, warm)
        if not warm:
            assert 4.0 < np.abs(p).max() < 8.0          # (the largest ulp: 4.8e-7)
        p64, m64, v64 = p, m, v
        for k in range(steps):
            before = p
            p, m, v = port.adam_statement(p, sums[k], m, v, start + k + 1, ADAM_GRAD_SCALE, ADAM_LR)
            p64, m64, v64 = port.adam_f64(p64, sums[k], m64, v64, start + k + 1, ADAM_GRAD_SCALE, ADAM_LR)
            assert p64.dtype == np.float64 and p.dtype == np.float32
            err = np.abs(p - p64)
            units = float((err / port.adam_f64_unit(p64, ADAM_LR)).max())
            i = int(err.argmax())
            print(f'adam_statement vs float64, start {start}, step {k + 1}: {units:.2f} units, largest error '
                  f'{err[i]:.2e} = {err[i] / np.spacing(np.abs(np.float32(p64[i]))):.2f} ulps = '
                  f'{err[i] / ADAM_LR:.2e} x lr')
            worst_units, worst_abs = max(worst_units, units), max(worst_abs, float(err[i]))
            zero = slice(n // 2, n // 2 + n // 5)
            if not warm:     # m = v = 0 and denom = eps: a zero gradient leaves the parameter where it is
                assert np.array_equal(p[zero], before[zero]) and not m[zero].any() and not v[zero].any()
    assert worst_units <= port.ADAM_F64_UNITS, worst_units
    assert worst_units >= 0.5 * port.ADAM_F64_UNITS, 'ADAM_F64_UNITS is a measurement: bring it down to it'
    assert worst_abs <= 1e-6

    p, m, v, sums = adam_case(n, steps, 11)
    ref = [torch.nn.Parameter(torch.tensor(p))]
    opt = torch.optim.Adam(ref, lr=ADAM_LR)
    adam_port, ported = port.AdamPort([p], ADAM_LR), [p]
    for k in range(steps):
        g = sums[k] * np.float32(ADAM_GRAD_SCALE)
        ref[0].grad = torch.tensor(g)
        opt.step()
        p, m, v = port.adam_statement(p, sums[k], m, v, k + 1, ADAM_GRAD_SCALE, ADAM_LR)
        ported = adam_port.step(ported, [g])
        state = opt.state[ref[0]]
        t_m, t_v, t_p = state['exp_avg'].numpy(), state['exp_avg_sq'].numpy(), ref[0].detach().numpy()
        if k == 0:
            assert np.array_equal(m, t_m) and np.array_equal(adam_port.exp_avg_sq[0], t_v)
            differ = int((v != t_v).sum())
            print(f'step 1: exp_avg_sq of the statement differs from torch in {differ} of {n} elements')
            assert 0 < differ and (np.abs(v - t_v) <= 2 * np.spacing(t_v)).all()
        units = float((np.abs(p - t_p) / port.adam_f64_unit(t_p, ADAM_LR)).max())
        print(f'adam_statement vs torch, step {k + 1}: {units:.2f} units, {np.abs(p - t_p).max():.2e}')
        assert units <= 2 * (k + 1)
        assert (np.abs(v - t_v) <= 2 * (k + 1) * np.spacing(t_v)).all()
    assert np.abs(p - t_p).max() <= np.spacing(np.float32(4.0))      # one ulp of the largest parameters


def test_clip_grad_norm_f64_reference():
    """clip_grad_norm_f64 against the float32 port (torch's clip_grad_norm_) and on cases with exact answers."""
    rng = np.random.RandomState(4)
    sums = (rng.standard_normal(4099) * 1000).astype(np.float32)
    for max_norm in (0.5, 4000.0):
        norm, coef, scaled = port.clip_grad_norm_f64(sums, 1.0 / 64, max_norm)
        (want,), total = port.clip_grad_norm([sums * np.float32(1.0 / 64)], max_norm)
        assert abs(norm - total) <= 4e-6 * norm and scaled.dtype == np.float64
        np.testing.assert_allclose(scaled * (1.0 / 64), want, rtol=4e-6, atol=0)
        assert (coef == 1.0) == (max_norm == 4000.0)
    norm, coef, scaled = port.clip_grad_norm_f64(np.array([3, 0, -4], np.float32), 0.5, 1.0)
    assert norm == 2.5 and coef == 1.0 / (2.5 + 1e-6) and np.array_equal(scaled, np.array([3, 0, -4]) * coef)
    norm, coef, scaled = port.clip_grad_norm_f64(np.zeros(5, np.float32), 1.0, 0.25)
    assert norm == 0.0 and coef == 1.0 and not scaled.any()


def test_meanstd_bit_exact(golden):
    g = golden('meanstd')
    norm = port.MeanStdPort((5,))
    for u in range(3):
        for s in range(4):
            norm.record(g[f'u{u}_s{s}_batch'])
        assert np.array_equal(norm.new_sum, g[f'u{u}_sum'])
        assert np.array_equal(norm.new_sum_sq, g[f'u{u}_sum_sq'])
        mean, std = norm.update()
        assert np.array_equal(mean, g[f'u{u}_mean'])
        assert np.array_equal(std, g[f'u{u}_std'])
        assert np.array_equal(norm.normalize(g[f'u{u}_x']), g[f'u{u}_normalized'])


def test_buffer_index_math_bit_exact(golden):
    g = golden('buffer')
    for case in range(3):
        pre = f'b{case}_'
        workers, size, batch = (int(x) for x in g[pre + 'cfg'])
        rng = np.random.RandomState(case)
        n_store = g[pre + 'in_rewards'].shape[0]
        max_size = size // workers
        assert max_size == int(g[pre + 'max_size'])
        assert n_store % max_size == int(g[pre + 'index'])
        disc = port.buffer_discounts(g[pre + 'in_terminations'][-1], 0.99)
        row = (n_store - 1) % max_size
        assert np.array_equal(disc, g[pre + 'buf_discounts'][row])
        cur = min(n_store, max_size)
        for it in range(3):
            flat, rows, cols = port.buffer_sample_indices(rng, cur, workers, batch)
            assert np.array_equal(flat, g[pre + f'get{it}_indices'])
            for key in ('observations', 'actions', 'next_observations', 'rewards', 'discounts'):
                assert np.array_equal(g[pre + 'buf_' + key][rows, cols],
                                      g[pre + f'get{it}_' + key], equal_nan=True)


def nstep_cases(g):
    for case in range(3):
        pre = f'n{case}_'
        workers, size, steps, index, filled = (int(x) for x in g[pre + 'cfg'])
        rows = [{k: g[pre + 'in_' + k][t] for k in (
            'observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations')}
            for t in range(g[pre + 'in_rewards'].shape[0])]
        yield pre, workers, size, steps, index, filled, rows


def nstep_golden_cases(g):
    """Every case of an n-step golden (buffer_nstep: three, discount factor 0.99; buffer_nstep_edges: `n_cases`, each
    with its own): (prefix, workers, size, return_steps, final index, final size, discount factor, stored rows)."""
    for case in range(int(g['n_cases']) if 'n_cases' in g.files else 3):
        pre = f'n{case}_'
        workers, size, steps, index, filled = (int(x) for x in g[pre + 'cfg'])
        discount = float(g[pre + 'discount']) if pre + 'discount' in g.files else 0.99
        rows = [{k: g[pre + 'in_' + k][t] for k in (
            'observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations')}
            for t in range(g[pre + 'in_rewards'].shape[0])]
        yield pre, workers, size, steps, index, filled, discount, rows


def test_buffer_n_step_accumulation_bit_exact(golden):
    """Buffer(return_steps > 1): store + accumulate_n_steps (buffers.py:33-79)."""
    g = golden('buffer_nstep')
    for pre, workers, size, steps, index, filled, rows in nstep_cases(g):
        buf = port.BufferPort(size, workers, return_steps=steps)
        for t, row in enumerate(rows):
            buf.store(**row)
            if t == 3:
                for k in buf.KEYS:
                    assert np.array_equal(buf.buffers[k], g[pre + 'early_' + k], equal_nan=True), k
        assert (buf.index, buf.size) == (index, filled)
        for k in buf.KEYS:
            assert np.array_equal(buf.buffers[k], g[pre + 'buf_' + k], equal_nan=True), k


def _buffer_port_equals_golden(g):
    """The helper and assertions of test_buffer_n_step_accumulation_bit_exact for any n-step golden, plus the sign of
    every zero."""
    for pre, workers, size, steps, index, filled, discount, rows in nstep_golden_cases(g):
        buf = port.BufferPort(size, workers, return_steps=steps, discount_factor=discount)
        for t, row in enumerate(rows):
            with np.errstate(invalid='ignore'):                # (the edge cases multiply 0 by inf, as recorded)
                buf.store(**row)
            if t == 3:
                for k in buf.KEYS:
                    assert np.array_equal(buf.buffers[k], g[pre + 'early_' + k], equal_nan=True), (pre, k)
        assert (buf.index, buf.size) == (index, filled)
        for k in buf.KEYS:
            assert np.array_equal(buf.buffers[k], g[pre + 'buf_' + k], equal_nan=True), (pre, k)
            held = ~np.isnan(g[pre + 'buf_' + k])               # (array_equal takes -0.0 for 0.0)
            assert np.array_equal(np.signbit(buf.buffers[k])[held], np.signbit(g[pre + 'buf_' + k])[held]), (pre, k)


def test_buffer_n_step_value_edges_bit_exact(golden):
    """The same at the value edges recorded from the reference in buffer_nstep_edges.npz: return_steps - 1 >=
    max_size (the chain ends on the row just written), signed zero rewards, an infinite reward behind a cut chain
    (0 * inf is NaN exactly where the reference's is), a NaN next observation, discount factors 1 and 0."""
    g = golden('buffer_nstep_edges')
    cases = list(nstep_golden_cases(g))
    assert len(cases) == 7
    assert any(steps - 1 >= size // workers for _, workers, size, steps, *_ in cases)
    assert any(size // workers == 1 for _, workers, size, *_ in cases)
    rewards = np.concatenate([g[pre + 'in_rewards'].ravel() for pre, *_ in cases])
    assert (np.signbit(rewards) & (rewards == 0)).any() and (~np.signbit(rewards) & (rewards == 0)).any()
    assert np.isinf(rewards).any()
    assert any(np.isnan(g[pre + 'in_next_observations']).any() for pre, *_ in cases)
    # the edges reach the stored rows: a NaN reward where a chain was cut before the infinite one, a zero of each sign
    assert any(np.isnan(g[pre + 'buf_rewards'][:filled]).any() for pre, _, _, _, _, filled, *_ in cases)
    _buffer_port_equals_golden(g)


def test_segment_minibatch_indices_bit_exact(golden):
    g = golden('segment_minibatch')
    rng = np.random.RandomState(int(g['seed']))
    got = np.concatenate(list(port.segment_minibatch_indices(
        rng, int(g['size']), int(g['batch_size']), int(g['iterations']))))
    assert np.array_equal(got, g['indices'])


def _params(g, prefix):
    actor = [g[prefix + 'actor.torso.model.0.weight'], g[prefix + 'actor.torso.model.0.bias'],
             g[prefix + 'actor.torso.model.2.weight'], g[prefix + 'actor.torso.model.2.bias'],
             g[prefix + 'actor.head.log_scale'], g[prefix + 'actor.head.loc_layer.0.weight'],
             g[prefix + 'actor.head.loc_layer.0.bias']]
    critic = [g[prefix + 'critic.torso.model.0.weight'], g[prefix + 'critic.torso.model.0.bias'],
              g[prefix + 'critic.torso.model.2.weight'], g[prefix + 'critic.torso.model.2.bias'],
              g[prefix + 'critic.head.v_layer.weight'], g[prefix + 'critic.head.v_layer.bias']]
    norm = (g[prefix + 'observation_normalizer._mean'], g[prefix + 'observation_normalizer._std'])
    return actor, critic, norm


@pytest.mark.parametrize('name', PPO_CASES)
def test_ppo_acting_matches_reference(golden, name):
    g = golden(name)
    actor, _, _ = _params(g, 'init/')
    steps = int(g['cfg'][3])
    for t in range(steps):      # first update window uses the initial parameters
        act, lp = port.ppo_act(actor, g['act/observations'][t], g['act/eps'][t])
        np.testing.assert_allclose(act, g['act/actions'][t], rtol=0, atol=2e-6)
        np.testing.assert_allclose(lp, g['act/log_probs'][t], rtol=0, atol=2e-5)


@pytest.mark.parametrize('name', PPO_CASES)
def test_ppo_update_matches_reference(golden, name):
    g = golden(name)
    updates = int(g['cfg'][6])
    actor_adam = critic_adam = None
    for u in range(updates):
        actor, critic, norm = _params(g, f'pre{u}/')
        seg = {k: g[f'u{u}/segment/{k}'] for k in (
            'observations', 'actions', 'next_observations', 'rewards', 'resets',
            'terminations', 'log_probs')}
        if actor_adam is None:
            actor_adam = port.AdamPort(actor, 3e-4)
            critic_adam = port.AdamPort(critic, 1e-3)
        new_actor, new_critic, infos, extra = port.ppo_update(
            actor, critic, norm, seg, batch_iterations=int(g['cfg'][5]), actor_adam=actor_adam,
            critic_adam=critic_adam)
        np.testing.assert_allclose(extra['returns'], g[f'u{u}/segment/returns'], atol=1e-5, rtol=1e-6)
        np.testing.assert_allclose(extra['advantages'].reshape(seg['rewards'].shape),
                                   g[f'u{u}/segment/advantages'], atol=1e-5, rtol=1e-5)
        n_actor = int(g[f'u{u}/info/actor/iterations'][0])
        assert sum('actor' in i for i in infos) == n_actor
        for key in ('loss', 'kl', 'entropy', 'clip_fraction', 'std'):
            got = np.array([i['actor'][key] for i in infos if 'actor' in i])
            np.testing.assert_allclose(got, g[f'u{u}/info/actor/{key}'], atol=1e-5, rtol=1e-5)
        stops = np.array([i['actor']['stop'] for i in infos if 'actor' in i])
        assert np.array_equal(stops, g[f'u{u}/info/actor/stop'])
        closs = np.array([i['critic']['loss'] for i in infos])
        np.testing.assert_allclose(closs, g[f'u{u}/info/critic/loss'], rtol=1e-5, atol=1e-5)
        vmean = np.array([i['critic']['v'].mean() for i in infos])
        np.testing.assert_allclose(vmean, g[f'u{u}/info/critic/v_mean'], rtol=1e-5, atol=1e-5)
        ref_actor, ref_critic, _ = _params(g, f'post{u}/')
        noise = _params(g, 'noise/')
        for got, want, before, floor in zip(new_actor + new_critic, ref_actor + ref_critic,
                                            actor + critic, noise[0] + noise[1]):
            # Parameter *deltas* within 1e-5 (north_star tolerance) after ALL iterations,
            # unless the reference itself moves by more than that when only its float32
            # summation order changes (golden 'noise/': reference vs reference on a
            # sample-permuted batch) — then the bound is a multiple of that floor.
            tol = max(1e-5, 50 * float(floor.max()))
            np.testing.assert_allclose(got - before, want - before, atol=tol, rtol=0)


def test_ppo_update_with_gradient_and_normaliser_clipping(golden):
    """`gradient_clip` on both updaters (actors.py:96-98, critics.py:24-25) and
    `MeanStd(clip=1.5)` (mean_stds.py:37-38): two consecutive reference updates, the second one
    with learnt normaliser statistics so that inputs beyond the clip exist."""
    g = golden('ppo_clipped_small')
    actor_clip, critic_clip, normalizer_clip = (float(x) for x in g['clips'])
    actor_adam = critic_adam = None
    for u in range(int(g['cfg'][6])):
        actor, critic, norm = _params(g, f'pre{u}/')
        seg = {k: g[f'u{u}/segment/{k}'] for k in (
            'observations', 'actions', 'next_observations', 'rewards', 'resets',
            'terminations', 'log_probs')}
        if actor_adam is None:
            actor_adam, critic_adam = port.AdamPort(actor, 3e-4), port.AdamPort(critic, 1e-3)
        new_actor, new_critic, infos, extra = port.ppo_update(
            actor, critic, norm, seg, batch_iterations=int(g['cfg'][5]), actor_adam=actor_adam,
            critic_adam=critic_adam, actor_clip=actor_clip, critic_clip=critic_clip,
            normalizer_clip=normalizer_clip)
        np.testing.assert_allclose(extra['returns'], g[f'u{u}/segment/returns'], atol=1e-5, rtol=1e-6)
        n_actor = int(g[f'u{u}/info/actor/iterations'][0])
        assert sum('actor' in i for i in infos) == n_actor
        kl = np.array([i['actor']['kl'] for i in infos if 'actor' in i])
        np.testing.assert_allclose(kl, g[f'u{u}/info/actor/kl'], atol=1e-5, rtol=1e-5)
        closs = np.array([i['critic']['loss'] for i in infos])
        np.testing.assert_allclose(closs, g[f'u{u}/info/critic/loss'], rtol=1e-5, atol=1e-5)
        ref_actor, ref_critic, _ = _params(g, f'post{u}/')
        for got, want, before in zip(new_actor + new_critic, ref_actor + ref_critic, actor + critic):
            np.testing.assert_allclose(got - before, want - before, atol=2e-5, rtol=0)
    # the clipping must actually bite in this golden
    x = (g['u1/segment/observations'] - norm[0]) / norm[1]
    assert (np.abs(x) > normalizer_clip).mean() > 0.01


def test_a2c_update_matches_reference(golden):
    """A2C (a2c.py:101-127): ONE StochasticPolicyGradient step with an entropy bonus on the full
    batch, then `batch_iterations` VRegression steps; two consecutive reference updates."""
    g = golden('a2c_small')
    entropy_coeff, iterations = float(g['entropy_coeff']), int(g['cfg'][5])
    actor_adam = critic_adam = None
    for u in range(int(g['cfg'][6])):
        actor, critic, norm = _params(g, f'pre{u}/')
        seg = {k: g[f'u{u}/segment/{k}'] for k in (
            'observations', 'actions', 'log_probs', 'advantages', 'returns')}
        flat = {k: port.flatten_time_major(v) for k, v in seg.items()}
        if actor_adam is None:
            actor_adam, critic_adam = port.AdamPort(actor, 3e-4), port.AdamPort(critic, 1e-3)
        grads, stats = port.clipped_ratio_grads(
            actor, flat['observations'], flat['actions'], flat['advantages'].reshape(-1),
            flat['log_probs'], entropy_coeff=entropy_coeff, plain=True)
        new_actor = actor_adam.step(actor, grads)
        for key in ('loss', 'kl', 'entropy', 'std'):
            np.testing.assert_allclose(stats[key], g[f'u{u}/info/actor/{key}'][0], rtol=1e-5, atol=1e-5)
        new_critic, losses = critic, []
        for _ in range(iterations):
            grads, stats = port.value_regression_grads(new_critic, norm[0], norm[1],
                                                       flat['observations'], flat['returns'].reshape(-1))
            new_critic = critic_adam.step(new_critic, grads)
            losses.append(stats['loss'])
        np.testing.assert_allclose(losses, g[f'u{u}/info/critic/loss'], rtol=1e-5, atol=1e-5)
        ref_actor, ref_critic, _ = _params(g, f'post{u}/')
        for got, want, before in zip(new_actor + new_critic, ref_actor + ref_critic, actor + critic):
            np.testing.assert_allclose(got - before, want - before, atol=1e-5, rtol=0)


@pytest.mark.parametrize('name', PPO_CASES)
def test_ppo_single_iteration_deltas_strict(golden, name):
    """One actor + one critic optimizer step: parameter deltas within 1e-5, strictly."""
    g = golden(name)
    actor, critic, norm = _params(g, 'pre0/')
    seg = {k: g[f'u0/segment/{k}'] for k in (
        'observations', 'actions', 'next_observations', 'rewards', 'resets',
        'terminations', 'log_probs')}
    new_actor, new_critic, _, extra = port.ppo_update(actor, critic, norm, seg, batch_iterations=1)
    ref_actor, ref_critic, _ = _params(g, 'iter1/')
    flat = {k: port.flatten_time_major(v) for k, v in seg.items()}
    g_actor, _ = port.clipped_ratio_grads(actor, flat['observations'], flat['actions'],
                                          extra['advantages'], flat['log_probs'])
    g_critic, _ = port.value_regression_grads(critic, norm[0], norm[1], flat['observations'],
                                              extra['returns'].reshape(-1))
    for got, want, before, grad in zip(new_actor + new_critic, ref_actor + ref_critic,
                                       actor + critic, g_actor + g_critic):
        # Adam's first step is lr * g / (|g| + 1e-8): where |g| is at float32 summation-noise
        # level the reference's own step has an arbitrary sign, so only the bound |step| <= lr
        # can be checked there; everywhere else the 1e-5 tolerance applies strictly.
        live = np.abs(grad) > 1e-6 * np.abs(grad).max()
        assert live.mean() > 0.99
        np.testing.assert_allclose((got - before)[live], (want - before)[live], atol=1e-5, rtol=0)
        assert np.abs(got - before).max() <= 1.01e-3


@pytest.mark.parametrize('name', ['ppo_halfcheetah_small', 'ppo_pendulum_small'])
def test_torch_port_matches_reference(golden, name):
    """oracle/torch_port.py (the timed CPU baseline) reproduces the reference's update."""
    import torch
    import torch_port
    torch.set_num_threads(1)
    g = golden(name)
    O, A, W, steps = (int(x) for x in g['cfg'][:4])
    actor, critic, norm = _params(g, 'pre0/')
    agent = torch_port.TorchPPO(O, A, steps=steps)
    agent.load(actor, critic, norm)
    agent.buffers = {k: g[f'u0/segment/{k}'].copy() for k in (
        'observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations',
        'log_probs')}
    agent.normalizer.new_count = 1
    agent.normalizer.new_sum = np.zeros(O, np.float32)
    agent.normalizer.new_sum_sq = np.zeros(O, np.float32)
    infos = agent.update()
    assert np.array_equal(agent.buffers['returns'], g['u0/segment/returns'])
    kl = np.array([float(i['actor']['kl']) for i in infos if 'actor' in i])
    np.testing.assert_allclose(kl, g['u0/info/actor/kl'], rtol=1e-6, atol=1e-7)
    closs = np.array([float(i['critic']['loss']) for i in infos])
    np.testing.assert_allclose(closs, g['u0/info/critic/loss'], rtol=1e-6, atol=1e-7)
    ref_actor, ref_critic, _ = _params(g, 'post0/')
    for got, want in zip(agent.actor_vars + agent.critic_vars, ref_actor + ref_critic):
        np.testing.assert_allclose(got.detach().numpy(), want, rtol=0, atol=1e-6)


def test_trpo_port_matches_reference(golden):
    """oracle/torch_port.TorchTRPO — conjugate gradient on Fisher-vector products, backtracking
    line search, critic regression — against two consecutive updates of the reference's TRPO agent."""
    import torch
    import torch_port
    torch.set_num_threads(1)
    g = golden('trpo_small')
    O, A, W, steps, seed, iterations, updates = (int(x) for x in g['cfg'])
    agent = torch_port.TorchTRPO(O, A, steps=steps, iterations=iterations)
    for u in range(updates):
        actor, critic, norm = _params(g, f'pre{u}/')
        agent.load(actor, critic, norm)
        agent.buffers = {k: g[f'u{u}/segment/{k}'].copy() for k in (
            'observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations',
            'log_probs')}
        agent.normalizer.new_count = 1
        agent.normalizer.new_sum = np.zeros(O, np.float32)
        agent.normalizer.new_sum_sq = np.zeros(O, np.float32)
        info = agent.update()
        assert np.array_equal(agent.buffers['returns'], g[f'u{u}/segment/returns'])
        assert info['actor']['backtrack_steps'] == int(g[f'u{u}/info/actor/backtrack_steps'][0])
        np.testing.assert_allclose(info['actor']['loss'], g[f'u{u}/info/actor/loss'][0], rtol=1e-5,
                                   atol=1e-7)
        np.testing.assert_allclose(info['actor']['kl'], g[f'u{u}/info/actor/kl'][0], rtol=1e-4,
                                   atol=1e-7)
        np.testing.assert_allclose([float(c['loss']) for c in info['critic']],
                                   g[f'u{u}/info/critic/loss'], rtol=1e-6, atol=1e-6)
        ref_actor, ref_critic, _ = _params(g, f'post{u}/')
        for got, want in zip(agent.actor_vars + agent.critic_vars, ref_actor + ref_critic):
            np.testing.assert_allclose(got.detach().numpy(), want, rtol=0, atol=2e-6)


def test_c_restatement_matches_golden(golden):
    """oracle/gae_ref.c (built by __graft_entry__.build()) is bit-exact with the reference."""
    import ctypes
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle',
                        'liboracle_gae.so')
    if not os.path.exists(path):
        pytest.skip('oracle C checker not built (run python __graft_entry__.py build)')
    lib = ctypes.CDLL(path)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.oracle_lambda_returns.argtypes = [fp] * 5 + [ctypes.c_int64] * 2 + [ctypes.c_double] * 2
    g = golden('lambda_returns')
    for i in range(int(g['n_cases'])):
        for j in range(4):
            k = f'c{i}_{j}_'
            arrays = [np.ascontiguousarray(g[k + n]) for n in
                      ('next_values', 'rewards', 'resets', 'terminations')]
            out = np.zeros_like(arrays[0])
            T, W = out.shape
            lib.oracle_lambda_returns(*[a.ctypes.data_as(fp) for a in arrays],
                                      out.ctypes.data_as(fp), T, W, float(g[k + 'gamma']),
                                      float(g[k + 'lambda']))
            assert np.array_equal(out, g[k + 'returns']), k


@pytest.mark.parametrize('name,kind', [('sac_small', 'sac'), ('td3_small', 'td3'),
                                       ('ddpg_small', 'ddpg'), ('d4pg_small', 'd4pg'),
                                       ('mpo_small', 'mpo')])
def test_offpolicy_port_matches_reference(golden, name, kind):
    """oracle/torch_port.OffPolicyPort replays the reference's first SAC / TD3 update from the
    golden buffer, index stream and normal draws (this also pins the RNG bookkeeping)."""
    import torch
    import torch_port
    torch.set_num_threads(1)
    g = golden(name)
    workers = int(g['cfg'][2])
    state = {k: g[k] for k in g.files}
    port_ = torch_port.OffPolicyPort(kind, state, 'pre/',
                                     atoms=g['atoms'] if kind == 'd4pg' else None,
                                     samples=int(g['samples']) if kind == 'mpo' else 20)
    buffers = {k[len('buffer/'):]: g[k] for k in g.files if k.startswith('buffer/')}
    # Buffer.store semantics (buffers.py:33-56): discounts, NaN padding beyond `size`
    size = int(g['buffer_size'])
    if kind not in ('d4pg', 'mpo'):   # (those: n-step returns, discounts accumulated, buffers.py:58-79)
        assert np.array_equal(buffers['discounts'][:size],
                              port.buffer_discounts(buffers['terminations'][:size] != 0, 0.99))
    assert np.isnan(buffers['rewards'][size:]).all()
    infos = port_.update(buffers, workers, g['indices'], g['eps'])
    np.testing.assert_allclose([i['critic']['loss'] for i in infos], g['info/critic/loss'], rtol=1e-6)
    if kind != 'd4pg':
        q_key = 'info/critic/q_mean' if kind in ('ddpg', 'mpo') else 'info/critic/q1_mean'
        np.testing.assert_allclose([i['critic']['q1'] for i in infos], g[q_key], rtol=1e-5, atol=1e-7)
    if kind == 'mpo':
        for key in ('policy_mean_loss', 'policy_std_loss', 'kl_mean_loss', 'kl_std_loss',
                    'alpha_mean_loss', 'alpha_std_loss', 'alpha_mean', 'alpha_std'):
            np.testing.assert_allclose([i['actor'][key] for i in infos], g['info/actor/' + key],
                                       rtol=1e-5, atol=1e-7, err_msg=key)
        for key in ('temperature_loss', 'temperature', 'penalty_temperature'):
            np.testing.assert_allclose([i['actor'][key] for i in infos],
                                       g['info/actor/' + key + '_mean'], rtol=1e-5, err_msg=key)
    else:
        np.testing.assert_allclose([i['actor']['loss'] for i in infos if 'actor' in i],
                                   g['info/actor/loss'], rtol=1e-5, atol=1e-7)
    for key, value in port_.state().items():
        np.testing.assert_allclose(value, g['post/' + key], rtol=0, atol=1e-7, err_msg=key)


def test_ppo_minibatch_update_matches_reference(golden):
    """Segment(batch_size=64): shuffled minibatches (segments.py:58-65), ragged last batch, KL stop
    in the middle of an iteration."""
    g = golden('ppo_minibatch_small')
    seed, iterations, bs = int(g['cfg'][4]), int(g['cfg'][5]), int(g['batch_size'])
    actor, critic, norm = _params(g, 'pre0/')
    seg = {k: g[f'u0/segment/{k}'] for k in (
        'observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations',
        'log_probs')}
    new_actor, new_critic, infos, _ = port.ppo_update(
        actor, critic, norm, seg, batch_iterations=iterations, batch_size=bs,
        np_random=np.random.RandomState(seed))
    assert len(infos) == int(g['u0/info/critic/iterations'][0])
    kl = np.array([i['actor']['kl'] for i in infos if 'actor' in i])
    np.testing.assert_allclose(kl, g['u0/info/actor/kl'], rtol=1e-5, atol=1e-5)
    assert np.array_equal([i['actor']['stop'] for i in infos if 'actor' in i], g['u0/info/actor/stop'])
    np.testing.assert_allclose([i['critic']['loss'] for i in infos], g['u0/info/critic/loss'],
                               rtol=1e-5, atol=1e-5)
    ref_actor, ref_critic, _ = _params(g, 'post0/')
    for got, want, before in zip(new_actor + new_critic, ref_actor + ref_critic, actor + critic):
        np.testing.assert_allclose(got - before, want - before, atol=2e-5, rtol=0)
