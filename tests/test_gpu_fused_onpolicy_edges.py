"""The FUSED route of the PPO / A2C entries — mlp64_grad16_kernel (csrc/mlp64x16.hip), the act / value kernels of
csrc/mlp64.hip and the packed collect kernel — PER PARAMETER TENSOR against float64, at the edges of its launch code:
every input instantiation <KS1, XT, XR> at its lowest and highest O, every head form (exact 1 / 6 / 8, padded 2 .. 5
and 7), the squashed critic, values16, row counts either side of a tile and of a workgroup, the tile stride with the
shrinking fp16x2 unit, the launch width.  DESIGN.md §4.2 maps each instantiation to its case here.

The plain entries (no `_torso`, no `_wide`) on the default torso are what reaches these kernels: the `*_torso` entries
run layer by layer even for (64, 64) Tanh.  The shipped library only, `grad_variant` at its default.

The reference is float64 torch autograd of the statements of test_gpu_layerwise_edges.py, the yardstick float32
autograd of the same statement on the device, the rule test_gpu_trpo_hip.assert_per_tensor:
max |hip - f64| <= max(1e-5 max |f64|, 2 max |f32 - f64|) for every tensor.  The problems are
test_gpu_trpo_hip.problem(O, A, n, 'default') and test_gpu_layerwise_edges.critic_problem / ppo_old on them;
n = 333 is 21 tiles of 16 rows, the last one of 13, in three workgroups of 8 waves."""
import functools

import numpy as np
import pytest
import torch

import numpy_port as port
import return_squash_ref as rs
import trpo_fisher_ref as ref
from test_gpu_layerwise_edges import (NORM_CLIP, RATIO_CLIP, SENTINEL, actor_statement, assert_guarded, cast,
                                      critic_problem, critic_statement, critic_values, guarded, normalised, policy,
                                      ppo_old, tensors)
from test_gpu_trpo_hip import assert_per_tensor, dev, problem

pytestmark = pytest.mark.gpu

# (O, A): every input form <1,0,4> O <= 4, <4,1,0> 5 .. 16, <5,1,1> 17, <5,1,4> 18 .. 20, <8,2,0> 21 .. 32 with its
# lowest and highest O; every head form (A = 1, 6, 8 exact; 2 .. 5 padded into the 6-build, 7 into the 8-build) with
# at least two input forms
TABLE = [(1, 1), (4, 5), (5, 2), (16, 6), (17, 6), (17, 7), (18, 3), (20, 8), (21, 1), (31, 4), (32, 8)]
CRITICS = {1: 1, 4: 5, 5: 2, 16: 6, 17: 6, 18: 3, 20: 8, 21: 1, 32: 8}     # O -> the A of TABLE's problem
N = 333
STRIDE = 256 * 128 + 17     # every workgroup full, the first two waves take a second tile, the last tile holds one row
RANGE = (-35.5, 2.25)
ACT_ROWS = (1, 31, 32, 33, 127, 128, 129, 333)     # either side of the act kernel's 32-row tile and of 4 waves of them
IDENTITY = (0.0, 1.0, 0.0, 0.0)                    # adv_stats: the advantages are final


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


# ------------------------------------------------------------------------ the statements and their references

def a2c_statement(p, old, coeff, dtype):
    """-> (gradient SUMS [P] in float64, statistics): StochasticPolicyGradient's loss (actors.py:20-51) times n,
    -sum(adv logp) with actor_statement's entropy term; kl is old - new."""
    t = tensors(p['theta'], p['slots'], dtype)
    dist = policy(p, t, cast(p['x'], dtype))
    logp = dist.log_prob(cast(p['actions'], dtype)).sum(-1)
    old, adv = cast(old, dtype), cast(p['adv'], dtype)
    entropy = dist.entropy().mean()
    loss = -(adv * logp).sum() - coeff * entropy * p['n']
    grads = torch.autograd.grad(loss, [t[name] for name, _, _ in p['slots']])
    stats = dict(loss=float(loss.detach()) / p['n'], kl=float((old - logp.detach()).mean()),
                 entropy=float(entropy.detach()), clip_fraction=0.0)
    return torch.cat([g.reshape(-1) for g in grads]).cpu().numpy().astype(np.float64), stats


def raw_advantages(p):
    """Advantages as tonic_gae_lambda_returns hands them over: raw float32 values, their mean and population std
    taken in float64 and rounded to float32."""
    raw = (p['adv'] * np.float32(2.5) + np.float32(0.7)).astype(np.float32)
    return raw, np.float32(raw.astype(np.float64).mean()), np.float32(raw.astype(np.float64).std())


@functools.lru_cache(maxsize=None)
def actor_reference(O, A, n, coeff, form='ppo'):
    """-> (float64 gradient sums, statistics, float32 gradient sums) of one case, shared by the tests that run it at
    several widths (read-only).  `form`: 'ppo', 'a2c', or 'norm' = ppo on (raw - float32 mean) / float32 std."""
    p, old = problem(O, A, n, 'default'), ppo_old(O, A, n, 'default')
    if form == 'norm':
        raw, mean, std = raw_advantages(p)
        p = dict(p, adv=(raw.astype(np.float64) - np.float64(mean)) / np.float64(std))
    statement = a2c_statement if form == 'a2c' else actor_statement
    want, info = statement(p, old, coeff, torch.float64)
    stock, _ = statement(p, old, coeff, torch.float32)
    return want, info, stock


@functools.lru_cache(maxsize=None)
def critic_reference(O, A, n, clip, value_range=None):
    c = critic_problem(O, A, n, 'default')
    want, info = critic_statement(c, clip, torch.float64, value_range)
    stock, _ = critic_statement(c, clip, torch.float32, value_range)
    return want, info, stock


# ------------------------------------------------------------------------ the entries

def actor_grad(lib, p, old, coeff, ratio_clip=RATIO_CLIP, adv=None, adv_stats=IDENTITY, rows=slice(None), width=0,
               skip=None):
    """tonic_ppo_actor_grad -> [P + 8] in float64.  The output lies between sentinel margins; with a skip flag it
    starts as NaN instead."""
    from tonic_amd import _lib
    O, A, P = p['O'], p['A'], p['P']
    keep = [dev(p['theta'])] + [dev(a[rows]) for a in (p['x'], p['actions'], p['adv'] if adv is None else adv)]
    keep += [dev(np.array(adv_stats, np.float32)), dev(old[rows])]
    n = keep[1].shape[0]
    assert lib.tonic_ppo_actor_param_count(O, A) == P
    need = lib.tonic_ppo_workspace_bytes(n, O, A, 1)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    if skip is None:
        whole, out = guarded(P + 8)
    else:
        whole = out = torch.full((P + 8,), float('nan'), device='cuda')
    _lib.check(lib.tonic_ppo_actor_grad(*[t.data_ptr() for t in keep], out.data_ptr(), n, O, A, ratio_clip, coeff,
                                        None if skip is None else skip.data_ptr(), width, ws.data_ptr(), ws.numel(),
                                        None), 'tonic_ppo_actor_grad')
    if skip is None:
        assert_guarded(whole, 'actor gradient sums')
    return out.cpu().numpy().astype(np.float64)


def critic_grad(lib, c, clip, value_range=None, width=0):
    """tonic_value_regression_grad[_ranged] -> [P + 8] in float64, the output between sentinel margins."""
    from tonic_amd import _lib
    O, P, n = c['O'], c['P'], c['n']
    keep = [dev(c[k]) for k in ('theta', 'mean', 'std', 'x', 'returns')]
    assert lib.tonic_v_critic_param_count(O) == P
    need = lib.tonic_ppo_workspace_bytes(n, O, 1, 0)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    whole, out = guarded(P + 8)
    common = (*[t.data_ptr() for t in keep[:3]], clip, keep[3].data_ptr(), keep[4].data_ptr(), out.data_ptr(), n, O,
              width, ws.data_ptr(), ws.numel())
    if value_range is None:
        _lib.check(lib.tonic_value_regression_grad(*common, None), 'tonic_value_regression_grad')
    else:
        low, high = (torch.tensor(v, dtype=torch.float32, device='cuda') for v in value_range)
        _lib.check(lib.tonic_value_regression_grad_ranged(*common, low.data_ptr(), high.data_ptr(), None),
                   'tonic_value_regression_grad_ranged')
    assert_guarded(whole, 'critic gradient sums')
    return out.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------ the checks

def check_actor(lib, O, A, n, coeff, form='ppo', width=0):
    p, old = problem(O, A, n, 'default'), ppo_old(O, A, n, 'default')
    want, info, stock = actor_reference(O, A, n, coeff, form)
    # preconditions, on the float64 reference alone
    if form != 'a2c':
        assert not ((np.abs(info['ratio'] - (1 - RATIO_CLIP)) < 1e-4) |
                    (np.abs(info['ratio'] - (1 + RATIO_CLIP)) < 1e-4)).any(), 'a ratio on a clip edge'
        if n >= 15:
            assert 0.05 <= info['clip_fraction'] <= 0.95, info['clip_fraction']
    if form == 'norm':
        raw, mean, std = raw_advantages(p)
        got = actor_grad(lib, p, old, coeff, adv=raw, adv_stats=(mean, std, 0.0, 1.0), width=width)
    else:
        got = actor_grad(lib, p, old, coeff, ratio_clip=-1.0 if form == 'a2c' else RATIO_CLIP, width=width)
    P = p['P']
    assert_per_tensor(p, got[:P], want, stock, f'fused {form} actor grad c={coeff} wg={width}')
    # the loss slot holds the surrogate's sum; the entropy bonus is the entropy slot's
    np.testing.assert_allclose((got[P] - coeff * got[P + 3]) / n, info['loss'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[P + 1] / n, info['kl'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[P + 3] / n, info['entropy'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[P + 2] / n, info['clip_fraction'], rtol=0, atol=1e-7)
    np.testing.assert_allclose(got[P + 4], n * p['sigma'].mean(), rtol=1e-5, atol=0)
    assert got[P + 5] == n and got[P + 6] == 0 and got[P + 7] == 0


def check_critic(lib, O, A, n, clip, value_range=None, width=0):
    c = critic_problem(O, A, n, 'default')
    want, info, stock = critic_reference(O, A, n, clip, value_range)
    if clip > 0:
        beyond = (np.abs(normalised(c['x'], c['mean'], c['std'], 0.0)) > clip).mean()
        assert beyond > 0.1, beyond
    got = critic_grad(lib, c, clip, value_range, width)
    P = c['P']
    what = 'fused critic grad' if value_range is None else f'fused ranged critic grad {value_range}'
    assert_per_tensor(c, got[:P], want, stock, f'{what} clip={clip} wg={width}')
    if value_range is None:
        np.testing.assert_allclose(got[P] / n, info['loss'], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got[P + 1] / n, info['v_mean'], rtol=1e-5, atol=2e-6)
    else:
        # v = low + s t: an error dz of the head's pre-activation moves v by s (1 - s) t dz <= t dz / 4, so the plain
        # head's absolute bound on the mean value scales by (high - low) / 4; the errors are of the size of v
        # (returns ~ N(0, 1) against v in (low, high)), so the loss keeps its relative bound
        np.testing.assert_allclose(got[P] / n, info['loss'], rtol=1e-5, atol=0)
        np.testing.assert_allclose(got[P + 1] / n, info['v_mean'], rtol=1e-5,
                                   atol=2e-6 * (value_range[1] - value_range[0]) / 4)
    assert got[P + 5] == n and not got[P + 2:P + 5].any() and not got[P + 6:].any()


# ------------------------------------------------------------------------ 1. the gradients, per tensor

@pytest.mark.parametrize('coeff', [0.0, 0.01])
@pytest.mark.parametrize('O,A', TABLE)
def test_ppo_actor_grad_per_tensor(lib, O, A, coeff):
    check_actor(lib, O, A, N, coeff)


@pytest.mark.parametrize('O,A', [(17, 6), (18, 3), (32, 8)])
def test_advantages_normalised_in_the_kernel(lib, O, A):
    """Raw advantages with adv_stats = [mean, std, 0, 1]: the kernel forms (adv - mean) / std in float32; the
    float64 statement divides by the same float32 pair."""
    check_actor(lib, O, A, N, 0.01, form='norm')


@pytest.mark.parametrize('coeff', [0.0, 0.01])
@pytest.mark.parametrize('O,A', [(4, 5), (17, 6), (21, 1)])
def test_a2c_policy_gradient_per_tensor(lib, O, A, coeff):
    """ratio_clip = -1: the plain policy gradient -sum(adv logp) (A2C), nothing clipped, no ratio."""
    check_actor(lib, O, A, N, coeff, form='a2c')


@pytest.mark.parametrize('clip', [0.0, NORM_CLIP])
@pytest.mark.parametrize('O', list(CRITICS))
def test_value_regression_grad_per_tensor(lib, O, clip):
    check_critic(lib, O, CRITICS[O], N, clip)


@pytest.mark.parametrize('O', [4, 16, 17, 20, 32])
def test_ranged_value_regression_grad_per_tensor(lib, O):
    """The five squashed instantiations (critic_squashed_by_inputs)."""
    check_critic(lib, O, CRITICS[O], N, NORM_CLIP, value_range=RANGE)


@pytest.mark.parametrize('n', [1, 15, 16, 17, 127, 128, 129])
@pytest.mark.parametrize('O,A', [(17, 6), (20, 7)])
def test_row_count_edges_per_tensor(lib, O, A, n):
    """Either side of a 16-row tile and of a workgroup's 8 tiles.  (A clip fraction has no range to lie in at one
    row: it is asserted from 15 rows.)"""
    check_actor(lib, O, A, n, 0.01)
    check_critic(lib, O, A, n, NORM_CLIP)


@pytest.mark.parametrize('width', [1, 2])
@pytest.mark.parametrize('O,A', [(17, 6), (5, 2)])
def test_narrow_launches_per_tensor(lib, O, A, width):
    """max_workgroups = 1: the 21 tiles on 8 waves, 2 - 3 tiles each — the tile stride, and the fp16x2 unit of a
    wave shrinking as it walks them; 2: 16 waves, the last five with one tile."""
    check_actor(lib, O, A, N, 0.01, width=width)
    check_critic(lib, O, A, N, NORM_CLIP, width=width)


def test_the_natural_tile_stride_per_tensor(lib):
    """n = 256 * 128 + 17 at the kernel's own width: 256 full workgroups, waves 0 and 1 of workgroup 0 take a second
    tile, the last tile holds one row."""
    check_actor(lib, 17, 6, STRIDE, 0.01)
    check_critic(lib, 17, 6, STRIDE, NORM_CLIP)
    check_critic(lib, 17, 6, STRIDE, NORM_CLIP, value_range=RANGE)


def test_actor_grad_is_additive_over_a_split(lib):
    """(17, 6) at n = 32 785 against its parts of 15 000 and 17 785 rows (118 and 139 workgroups), per tensor at
    test_gpu_layerwise_edges.test_actor_grad_is_additive_where_slabs_start_to_empty's bound."""
    p, old = problem(17, 6, STRIDE, 'default'), ppo_old(17, 6, STRIDE, 'default')
    P, n, h = p['P'], p['n'], 15000
    full = actor_grad(lib, p, old, 0.01)
    a = actor_grad(lib, p, old, 0.01, rows=slice(0, h))
    b = actor_grad(lib, p, old, 0.01, rows=slice(h, n))
    # the entropy bonus enters each call's log_scale gradient in proportion to its rows, so it is additive too
    both = a + b
    failures = []
    for name, shape, at in p['slots']:
        sl = slice(at, at + int(np.prod(shape)))
        err, scale = np.abs(both[sl] - full[sl]).max(), np.abs(full[sl]).max()
        print(f'ACC fused additivity n={n} torso={p["sizes"]} {name}: err/scale={err / scale:.2e}')
        if not err <= 2e-5 * scale:
            failures.append((name, err, scale))
    assert not failures, failures
    assert full[P + 5] == n and a[P + 5] == h and b[P + 5] == n - h


def test_the_skip_flag_zero_fills_the_output(lib):
    """*d_skip_flag != 0: all P + 8 floats of a NaN-filled output come back exactly 0.  (The flag is an argument of
    tonic_ppo_actor_grad alone: the critic's entries have none.)"""
    p, old = problem(17, 6, N, 'default'), ppo_old(17, 6, N, 'default')
    for value in (1, -3):
        flag = torch.full((1,), value, dtype=torch.int32, device='cuda')
        got = actor_grad(lib, p, old, 0.01, skip=flag)
        assert got.shape == (p['P'] + 8,) and np.array_equal(got, np.zeros_like(got))
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    got = actor_grad(lib, p, old, 0.01, skip=flag)
    assert np.isfinite(got).all() and got[p['P'] + 5] == N and np.abs(got[:p['P']]).max() > 0


# ------------------------------------------------------------------------ 2. the forward entries

@pytest.mark.parametrize('O,A', TABLE + [(3, 8), (17, 1)])
def test_ppo_act_vs_float64(lib, O, A):
    """tonic_ppo_act (no workspace) with noise and as the mode (d_eps = NULL), at the tolerances of
    test_gpu_layerwise_edges.test_forward_entries_vs_float64, the outputs between sentinel margins.  The act kernel
    has its own buckets, <KS1 = 2 (O <= 4), 9 (<= 18), 16> x <AP = 1, 6, 8>: (3, 8) and (17, 1) are the two of the
    nine that TABLE leaves out."""
    from tonic_amd import _lib
    for n in ACT_ROWS:
        p = problem(O, A, n, 'default')
        eps = np.random.RandomState(n + A).standard_normal((n, A)).astype(np.float32)
        theta, x, e = dev(p['theta']), dev(p['x']), dev(eps)
        for noise in (e, None):
            whole_a, actions = guarded(n, A)
            whole_l, lps = guarded(n)
            _lib.check(lib.tonic_ppo_act(theta.data_ptr(), x.data_ptr(), None if noise is None else noise.data_ptr(),
                                         actions.data_ptr(), lps.data_ptr(), n, O, A, None), 'tonic_ppo_act')
            what = f'O={O} A={A} n={n} ' + ('mode' if noise is None else 'sampled')
            assert_guarded(whole_a, what + ': actions')
            assert_guarded(whole_l, what + ': log-probabilities')
            got = actions.cpu().numpy()
            if noise is None:
                # the log-probability is that of the action returned
                want_actions, want_lp = p['mu'], ref.log_probs(p['mu'], p['sigma'], got.astype(np.float64))
            else:
                want_actions = p['mu'] + p['sigma'] * eps.astype(np.float64)
                want_lp = ref.log_probs(p['mu'], p['sigma'], want_actions)
            np.testing.assert_allclose(got, want_actions, rtol=1e-5, atol=1e-5, err_msg=what)
            np.testing.assert_allclose(lps.cpu().numpy(), want_lp, rtol=1e-5, atol=2e-5, err_msg=what)


@pytest.mark.parametrize('O', list(CRITICS))
def test_value_forwards_vs_float64(lib, O):
    """tonic_value_forward and tonic_value_forward_ranged: the per-step kernel up to 32 767 rows, values16 (the
    forward half of the regression kernel) from kValues16MinRows = 32 768.  The squashed values at
    test_gpu_return_normalizer._check_against_reference's form: atol = 2e-5 max(1, max |v|), no relative term."""
    from tonic_amd import _lib
    A = CRITICS[O]
    low, high = (torch.tensor(v, dtype=torch.float32, device='cuda') for v in RANGE)
    for n in ACT_ROWS + (32767, 32768, STRIDE):
        c = critic_problem(O, A, n, 'default')
        keep = [dev(c[k]) for k in ('theta', 'mean', 'std', 'x')]
        t64 = tensors(c['theta'], c['slots'], torch.float64)
        beyond = (np.abs(normalised(c['x'], c['mean'], c['std'], 0.0)) > NORM_CLIP).mean()
        assert n < 15 or beyond > 0.1, beyond
        for clip in (0.0, NORM_CLIP):
            with torch.no_grad():
                z = critic_values(c, t64, torch.float64, clip)
                want = {False: z.cpu().numpy(), True: rs.squash64(z, *RANGE).cpu().numpy()}
            common = (*[t.data_ptr() for t in keep[:3]], clip, keep[3].data_ptr())
            for ranged in (False, True):
                whole, values = guarded(n)
                if ranged:
                    _lib.check(lib.tonic_value_forward_ranged(*common, values.data_ptr(), n, O, low.data_ptr(),
                                                              high.data_ptr(), None), 'tonic_value_forward_ranged')
                else:
                    _lib.check(lib.tonic_value_forward(*common, values.data_ptr(), n, O, None), 'tonic_value_forward')
                what = f'O={O} n={n} clip={clip} ranged={ranged}'
                assert_guarded(whole, what)
                if ranged:
                    scale = max(1.0, float(np.abs(want[True]).max()))
                    np.testing.assert_allclose(values.cpu().numpy(), want[True], rtol=0, atol=2e-5 * scale,
                                               err_msg=what)
                else:
                    np.testing.assert_allclose(values.cpu().numpy(), want[False], rtol=2e-5, atol=2e-5, err_msg=what)


# the 3 x 3 pack forms: collect16_ks1 1 / 5 / 8 x collect16_ap 1 / 6 / 8
@pytest.mark.parametrize('O,A', [(4, 1), (4, 5), (3, 8), (17, 1), (17, 6), (20, 7), (32, 1), (21, 4), (32, 8)])
def test_packed_collect_steps_vs_float64(lib, O, A):
    """tonic_ppo_pack_actor + tonic_ppo_collect_steps_packed: two steps into rows 1 and 2 of a 4-row Segment whose
    rows 0 and 3 hold sentinels; W either side of the kernel's 16-row tile."""
    from tonic_amd import _lib
    fields = {'observations': (O,), 'actions': (A,), 'next_observations': (O,), 'rewards': (), 'resets': (),
              'terminations': (), 'log_probs': ()}
    for W in (1, 15, 16, 17, 333):
        p = problem(O, A, W, 'default')
        rng = np.random.RandomState(O * 100 + A * 10 + W)
        obs = (rng.standard_normal((3, W, O)) * 1.5).astype(np.float32)
        eps = rng.standard_normal((2, W, A)).astype(np.float32)
        rewards = rng.standard_normal((2, W)).astype(np.float32)
        resets = (rng.uniform(size=(2, W)) < 0.3).astype(np.float32)
        terms = (resets * (rng.uniform(size=(2, W)) < 0.5)).astype(np.float32)
        # MeanStd.record's sequential float32 sums, continuing from non-zero running sums
        record = port.MeanStdPort((O,))
        record.record(obs[2][:1])
        start = np.concatenate([record.new_sum, record.new_sum_sq]).astype(np.float32)
        record.record(obs[0])
        record.record(obs[1])
        packed = torch.zeros(lib.tonic_ppo_packed_actor_floats(O, A), device='cuda')
        theta = dev(p['theta'])
        _lib.check(lib.tonic_ppo_pack_actor(theta.data_ptr(), packed.data_ptr(), O, A, None), 'tonic_ppo_pack_actor')
        seg = {k: torch.full((4, W) + tail, SENTINEL, device='cuda') for k, tail in fields.items()}
        whole_acc, acc = guarded(2 * O)
        acc.copy_(dev(start))
        d = [dev(a) for a in (obs, eps, rewards, resets, terms)]
        _lib.check(lib.tonic_ppo_collect_steps_packed(
            packed.data_ptr(), *[t.data_ptr() for t in d], seg['observations'].data_ptr(), seg['actions'].data_ptr(),
            seg['next_observations'].data_ptr(), seg['rewards'].data_ptr(), seg['resets'].data_ptr(),
            seg['terminations'].data_ptr(), seg['log_probs'].data_ptr(), acc.data_ptr(), 1, 2, W, O, A, None),
            'tonic_ppo_collect_steps_packed')
        got = {k: v.cpu().numpy() for k, v in seg.items()}
        what = f'O={O} A={A} W={W}'
        for k, v in got.items():
            assert (v[0] == SENTINEL).all() and (v[3] == SENTINEL).all(), f'{what}: {k}: a row beside the steps written'
        for k, want in (('observations', obs[:2]), ('next_observations', obs[1:]), ('rewards', rewards),
                        ('resets', resets), ('terminations', terms)):
            assert np.array_equal(got[k][1:3], want), f'{what}: {k}'
        for t in range(2):
            _, mu, sigma, _ = ref.forward(p['theta'], obs[t], *p['args'])
            want_actions = mu + sigma * eps[t].astype(np.float64)
            np.testing.assert_allclose(got['actions'][1 + t], want_actions, rtol=1e-5, atol=1e-5, err_msg=what)
            np.testing.assert_allclose(got['log_probs'][1 + t], ref.log_probs(mu, sigma, want_actions), rtol=1e-5,
                                       atol=2e-5, err_msg=what)
        assert_guarded(whole_acc, what + ': d_norm_acc')
        sums = acc.cpu().numpy()
        assert np.array_equal(sums[:O], record.new_sum) and np.array_equal(sums[O:], record.new_sum_sq), what
