"""The PPO / A2C entries of the layer-by-layer path (csrc/mlpwide.hip, the tonic_*_torso entries) on the edge
torsos of test_gpu_trpo_hip.EDGES, PER PARAMETER TENSOR: what TRPO's loss gradient does not run — the clipped
ratio, the normaliser in the critic's first layer, the value head, the squashed value head, the acting and value
forwards — and the row counts either side of a tile and of a slab.

The reference is float64 torch autograd of the statement of test_gpu_parity.test_torso_grads_vs_float64_autograd,
the yardstick float32 autograd of the same statement on the device, the rule test_gpu_trpo_hip.assert_per_tensor:
max |hip - f64| <= max(1e-5 max |f64|, 2 max |f32 - f64|) for every tensor, log_scale and the narrow biases
included.  The problems (parameters, observations, actions, advantages) are test_gpu_trpo_hip.problem's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import return_squash_ref as rs
import trpo_fisher_ref as ref
from test_gpu_trpo_hip import CODES, EDGES, assert_per_tensor, dev, problem

pytestmark = pytest.mark.gpu

SMALL = ['min4', 'steps', 'k116', 'wide256', 'wide384']         # at their (O, A, n), n = 333
RATIO_CLIP = 0.2
NORM_CLIP = 1.2
SENTINEL, MARGIN = -7777.0, 64


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _lib.load()


def edge(name, n=None):
    O, A, rows = EDGES[name][2]
    return problem(O, A, rows if n is None else n, name)


def torso_args(p):
    sizes = p['sizes']
    return len(sizes), (ctypes.c_int32 * len(sizes))(*sizes), CODES[p['activation']]


# ------------------------------------------------------------------------ the problems

@functools.lru_cache(maxsize=32)
def ppo_old(O, A, n, torso):
    """The problem's old log-probabilities with every ratio off the clip edges: min(adv r, adv clamp(r)) changes
    branch at r = 0.8 and r = 1.2, and a row within float32 rounding of an edge has no defined branch.  Rows within
    1e-4 of an edge (float32 moves a ratio by ~1e-6) get a new draw; no row is ever left out of a comparison."""
    p = problem(O, A, n, torso)
    rng = np.random.RandomState(n + 11 * A)
    logp = ref.log_probs(p['mu'], p['sigma'], p['actions'].astype(np.float64))
    old = p['old'].copy()
    for _ in range(100):
        ratio = np.exp(logp - old)
        near = (np.abs(ratio - (1 - RATIO_CLIP)) < 1e-4) | (np.abs(ratio - (1 + RATIO_CLIP)) < 1e-4)
        if not near.any():
            break
        old[near] = (logp[near] + rng.standard_normal(int(near.sum())) * 0.3).astype(np.float32)
    return old


def critic_layout(O, sizes):
    out, at, fan_in = [], 0, O
    for l, size in enumerate(sizes):
        out.append((f'W{l}', (size, fan_in), at)); at += size * fan_in
        out.append((f'b{l}', (size,), at)); at += size
        fan_in = size
    out.append(('W_v', (1, fan_in), at)); at += fan_in
    out.append(('b_v', (1,), at)); at += 1
    return out, at


def normalised(x, mean, std, clip):
    xn = (np.asarray(x, np.float64) - mean) / std
    return np.clip(xn, -clip, clip) if clip > 0 else xn


@functools.lru_cache(maxsize=32)
def critic_problem(O, A, n, torso):
    """A critic on the problem's torso: parameters drawn as problem() draws them, a MeanStd normaliser with
    mean != 0 and std != 1, returns, and the problem's observations — for ReLU redrawn by problem()'s rule on the
    NORMALISED inputs, with the clip off and on (the mask must be defined in float32 for both)."""
    p = problem(O, A, n, torso)
    sizes, activation = p['sizes'], p['activation']
    rng = np.random.RandomState(O * 17 + n + 3 * len(sizes))
    slots, P = critic_layout(O, sizes)
    theta = np.zeros(P, np.float32)
    for name, shape, at in slots:
        scale = 0.1 if len(shape) == 1 else 0.6 / np.sqrt(shape[1])
        theta[at:at + int(np.prod(shape))] = rng.standard_normal(int(np.prod(shape))) * scale
    mean = (rng.standard_normal(O) * 0.2).astype(np.float32)
    std = (0.5 + rng.uniform(size=O)).astype(np.float32)
    returns = rng.standard_normal(n).astype(np.float32)
    x = p['x'].copy()
    t64 = {name: theta[at:at + int(np.prod(shape))].reshape(shape).astype(np.float64) for name, shape, at in slots}
    while activation == 'relu':
        close = np.zeros(n, bool)
        for clip in (0.0, NORM_CLIP):
            h = normalised(x, mean, std, clip)
            for l in range(len(sizes)):
                z = h @ t64[f'W{l}'].T + t64[f'b{l}']
                close |= (np.abs(z) < 1e-5).any(1)
                h = np.maximum(z, 0.0)
        if not close.any():
            break
        x[close] = (rng.standard_normal((int(close.sum()), O)) * 1.5).astype(np.float32)
    return dict(O=O, A=1, n=n, sizes=sizes, activation=activation, slots=slots, P=P, theta=theta, mean=mean, std=std,
                returns=returns, x=x)


# ------------------------------------------------------------------------ the statements, in any dtype

def tensors(theta, slots, dtype):
    return {name: torch.tensor(np.asarray(theta[at:at + int(np.prod(shape))]).reshape(shape), dtype=dtype,
                               device='cuda', requires_grad=True) for name, shape, at in slots}


def cast(x, dtype):
    return torch.tensor(np.asarray(x), device='cuda').to(dtype)


def body(x, t, layers, activation):
    fn = torch.tanh if activation == 'tanh' else torch.relu
    for l in range(layers):
        x = fn(x @ t[f'W{l}'].T + t[f'b{l}'])
    return x


def policy(p, t, x):
    loc = torch.tanh(body(x, t, len(p['sizes']), p['activation']) @ t['W_mu'].T + t['b_mu'])
    scale = (torch.nn.functional.softplus(t['log_scale']) + 1e-8).clamp(1e-4, 1.0)
    return torch.distributions.Normal(loc, scale)


def actor_statement(p, old, coeff, dtype):
    """-> (gradient SUMS [P] in float64, statistics): ClippedRatio's loss (actors.py:81-91) times n."""
    t = tensors(p['theta'], p['slots'], dtype)
    dist = policy(p, t, cast(p['x'], dtype))
    logp = dist.log_prob(cast(p['actions'], dtype)).sum(-1)
    old, adv = cast(old, dtype), cast(p['adv'], dtype)
    ratio = torch.exp(logp - old)
    surrogate = -torch.min(adv * ratio, adv * ratio.clamp(1 - RATIO_CLIP, 1 + RATIO_CLIP)).sum()
    entropy = dist.entropy().mean()
    loss = surrogate - coeff * entropy * p['n']
    grads = torch.autograd.grad(loss, [t[name] for name, _, _ in p['slots']])
    ratio, logp = ratio.detach(), logp.detach()
    stats = dict(loss=float(loss.detach()) / p['n'], kl=float((old - logp).mean()), entropy=float(entropy.detach()),
                 clip_fraction=float(((ratio > 1 + RATIO_CLIP) | (ratio < 1 - RATIO_CLIP)).double().mean()),
                 ratio=ratio.cpu().numpy())
    return torch.cat([g.reshape(-1) for g in grads]).cpu().numpy().astype(np.float64), stats


def critic_values(c, t, dtype, clip):
    xn = (cast(c['x'], dtype) - cast(c['mean'], dtype)) / cast(c['std'], dtype)
    if clip > 0:
        xn = xn.clamp(-clip, clip)
    return (body(xn, t, len(c['sizes']), c['activation']) @ t['W_v'].T + t['b_v'])[:, 0]


def critic_statement(c, clip, dtype, value_range=None):
    """-> (gradient SUMS [P] in float64, statistics): sum((v - returns)^2) (critics.py:18-24 times n), v through
    the Return normaliser's head where `value_range` = (low, high)."""
    t = tensors(c['theta'], c['slots'], dtype)
    v = critic_values(c, t, dtype, clip)
    if value_range is not None:
        v = rs.squash64(v, *value_range)
    loss = ((v - cast(c['returns'], dtype)) ** 2).sum()
    grads = torch.autograd.grad(loss, [t[name] for name, _, _ in c['slots']])
    stats = dict(loss=float(loss.detach()) / c['n'], v_mean=float(v.detach().mean()))
    return torch.cat([g.reshape(-1) for g in grads]).cpu().numpy().astype(np.float64), stats


# ------------------------------------------------------------------------ the entries

def actor_grad(lib, p, old, coeff, rows=slice(None)):
    from tonic_amd import _lib
    torso = torso_args(p)
    keep = [dev(p['theta'])] + [dev(a[rows]) for a in (p['x'], p['actions'], p['adv'])]
    keep += [dev(np.array([0, 1, 0, 0], np.float32)), dev(old[rows])]
    n = keep[1].shape[0]
    need = lib.tonic_ppo_torso_workspace_bytes(n, p['O'], p['A'], 1, torso[0], torso[1])
    assert need > 0 and lib.tonic_ppo_torso_param_count(p['O'], p['A'], 1, torso[0], torso[1]) == p['P']
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.full((p['P'] + 8,), float('nan'), device='cuda')
    _lib.check(lib.tonic_ppo_actor_grad_torso(*torso, *[t.data_ptr() for t in keep], out.data_ptr(), n, p['O'],
                                              p['A'], RATIO_CLIP, coeff, None, ws.data_ptr(), ws.numel(), None),
               'tonic_ppo_actor_grad_torso')
    return out.cpu().numpy().astype(np.float64)


def critic_grad(lib, c, clip, value_range=None):
    from tonic_amd import _lib
    torso = torso_args(c)
    keep = [dev(c[k]) for k in ('theta', 'mean', 'std', 'x', 'returns')]
    need = lib.tonic_ppo_torso_workspace_bytes(c['n'], c['O'], 1, 0, torso[0], torso[1])
    assert need > 0 and lib.tonic_ppo_torso_param_count(c['O'], 1, 0, torso[0], torso[1]) == c['P']
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.full((c['P'] + 8,), float('nan'), device='cuda')
    common = (*torso, *[t.data_ptr() for t in keep[:3]], clip, keep[3].data_ptr(), keep[4].data_ptr(),
              out.data_ptr(), c['n'], c['O'], ws.data_ptr(), ws.numel())
    if value_range is None:
        _lib.check(lib.tonic_value_regression_grad_torso(*common, None), 'tonic_value_regression_grad_torso')
    else:
        low, high = (torch.tensor(v, dtype=torch.float32, device='cuda') for v in value_range)
        _lib.check(lib.tonic_value_regression_grad_torso_ranged(*common, low.data_ptr(), high.data_ptr(), None),
                   'tonic_value_regression_grad_torso_ranged')
    return out.cpu().numpy().astype(np.float64)


def guarded(*shape):
    """An output filled with a sentinel between two sentinel margins of 64 floats."""
    count = int(np.prod(shape))
    whole = torch.full((count + 2 * MARGIN,), SENTINEL, device='cuda')
    return whole, whole[MARGIN:MARGIN + count].view(*shape)


def assert_guarded(whole, what):
    whole = whole.cpu().numpy()
    assert (whole[:MARGIN] == SENTINEL).all() and (whole[-MARGIN:] == SENTINEL).all(), what + ': margin written'
    assert not (whole[MARGIN:-MARGIN] == SENTINEL).any(), what + ': element not written'


# ------------------------------------------------------------------------ the checks

def check_actor(lib, name, coeff, n=None, fraction=True):
    p = edge(name, n)
    old = ppo_old(p['O'], p['A'], p['n'], name)
    want, info = actor_statement(p, old, coeff, torch.float64)
    # preconditions, on the float64 reference alone
    assert not ((np.abs(info['ratio'] - (1 - RATIO_CLIP)) < 1e-4) |
                (np.abs(info['ratio'] - (1 + RATIO_CLIP)) < 1e-4)).any(), 'a ratio on a clip edge'
    if fraction:
        assert 0.05 <= info['clip_fraction'] <= 0.95, info['clip_fraction']
    stock, _ = actor_statement(p, old, coeff, torch.float32)
    got = actor_grad(lib, p, old, coeff)
    P, n = p['P'], p['n']
    assert_per_tensor(p, got[:P], want, stock, f'ppo actor grad c={coeff}')
    # the loss slot holds the surrogate's sum; the entropy bonus is the entropy slot's
    np.testing.assert_allclose((got[P] - coeff * got[P + 3]) / n, info['loss'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[P + 1] / n, info['kl'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[P + 3] / n, info['entropy'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got[P + 2] / n, info['clip_fraction'], rtol=0, atol=1e-7)
    assert got[P + 5] == n


def check_critic(lib, name, clip, n=None, value_range=None):
    p = edge(name, n)
    c = critic_problem(p['O'], p['A'], p['n'], name)
    want, info = critic_statement(c, clip, torch.float64, value_range)
    if clip > 0:
        beyond = (np.abs(normalised(c['x'], c['mean'], c['std'], 0.0)) > clip).mean()
        assert beyond > 0.1, beyond
    stock, _ = critic_statement(c, clip, torch.float32, value_range)
    got = critic_grad(lib, c, clip, value_range)
    P, n = c['P'], c['n']
    what = 'critic grad' if value_range is None else f'ranged critic grad {value_range}'
    assert_per_tensor(c, got[:P], want, stock, f'{what} clip={clip}')
    if value_range is None:
        np.testing.assert_allclose(got[P] / n, info['loss'], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got[P + 1] / n, info['v_mean'], rtol=1e-5, atol=2e-6)
    assert got[P + 5] == n


# ------------------------------------------------------------------------ 1. the two gradients, per tensor

@pytest.mark.parametrize('coeff', [0.0, 0.01])
@pytest.mark.parametrize('name', SMALL)
def test_ppo_actor_grad_per_tensor(lib, name, coeff):
    check_actor(lib, name, coeff)


@pytest.mark.parametrize('clip', [0.0, NORM_CLIP])
@pytest.mark.parametrize('name', SMALL)
def test_value_regression_grad_per_tensor(lib, name, clip):
    check_critic(lib, name, clip)


def test_the_tile_stride_in_both_gradients(lib):
    """`stride`: 2048 * 64 + 17 rows — the grid-stride regime of dense_kernel with a two-chunk K (4 <- 68)."""
    check_actor(lib, 'stride', 0.01)
    check_critic(lib, 'stride', NORM_CLIP)


def test_ranged_value_regression_grad_per_tensor(lib):
    """The squashed value head (the Return normaliser, tests/return_squash_ref.py) on `steps`."""
    check_critic(lib, 'steps', NORM_CLIP, value_range=(-35.5, 2.25))


@pytest.mark.parametrize('n', [1, 15, 16, 17, 63, 64, 65])
def test_row_count_edges_per_tensor(lib, n):
    """Either side of a 16-row tile and of a workgroup's four tiles / one 64-row slab, on `steps`.  (A clip
    fraction has no range to lie in at one row: only the clip-edge precondition is asserted here.)"""
    check_actor(lib, 'steps', 0.01, n, fraction=False)
    check_critic(lib, 'steps', NORM_CLIP, n)


# ------------------------------------------------------------------------ 2. the forward entries

@pytest.mark.parametrize('name,n', [(name, n) for name in SMALL for n in (1, 333)] + [('stride', None)])
def test_forward_entries_vs_float64(lib, name, n):
    """tonic_value_forward_torso and tonic_ppo_act_torso at the tolerances of test_torso_grads_vs_float64_autograd;
    the outputs lie between sentinel margins: the stores of a ragged last tile are what can overrun."""
    from tonic_amd import _lib
    p = edge(name, n)
    n, O, A = p['n'], p['O'], p['A']
    c = critic_problem(O, A, n, name)
    torso = torso_args(p)
    ws = torch.empty(max(lib.tonic_ppo_torso_workspace_bytes(n, O, A, 1, torso[0], torso[1]),
                         lib.tonic_ppo_torso_workspace_bytes(n, O, 1, 0, torso[0], torso[1])),
                     dtype=torch.uint8, device='cuda')
    keep = [dev(c[k]) for k in ('theta', 'mean', 'std', 'x')]
    for clip in (0.0, NORM_CLIP):
        with torch.no_grad():
            want = critic_values(c, tensors(c['theta'], c['slots'], torch.float64), torch.float64, clip)
        whole, values = guarded(n)
        _lib.check(lib.tonic_value_forward_torso(*torso, *[t.data_ptr() for t in keep[:3]], clip, keep[3].data_ptr(),
                                                 values.data_ptr(), n, O, ws.data_ptr(), ws.numel(), None), 'values')
        assert_guarded(whole, f'values clip={clip}')
        np.testing.assert_allclose(values.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-5)
    eps = np.random.RandomState(n + A).standard_normal((n, A)).astype(np.float32)
    want_actions = p['mu'] + p['sigma'] * eps.astype(np.float64)
    want_lp = ref.log_probs(p['mu'], p['sigma'], want_actions)
    whole_a, actions = guarded(n, A)
    whole_l, lps = guarded(n)
    theta, x, e = dev(p['theta']), dev(p['x']), dev(eps)
    _lib.check(lib.tonic_ppo_act_torso(*torso, theta.data_ptr(), x.data_ptr(), e.data_ptr(), actions.data_ptr(),
                                       lps.data_ptr(), n, O, A, ws.data_ptr(), ws.numel(), None), 'act')
    assert_guarded(whole_a, 'actions')
    assert_guarded(whole_l, 'log-probabilities')
    np.testing.assert_allclose(actions.cpu().numpy(), want_actions, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(lps.cpu().numpy(), want_lp, rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------ 3. the slab regime change

def test_actor_grad_is_additive_where_slabs_start_to_empty(lib):
    """`k116` at n = 65 537: slab = 68, slabs 964 .. 1023 are empty; the two parts (30 000 and 35 537 rows) run
    469 and 556 full-width slabs.  test_config5_size_properties' bound, per tensor."""
    p = edge('k116', 65537)
    old = ppo_old(p['O'], p['A'], p['n'], 'k116')
    P, n, h = p['P'], p['n'], 30000
    full = actor_grad(lib, p, old, 0.01)
    a = actor_grad(lib, p, old, 0.01, slice(0, h))
    b = actor_grad(lib, p, old, 0.01, slice(h, n))
    # the entropy bonus enters each call's log_scale gradient in proportion to its rows, so it is additive too
    both = a + b
    failures = []
    for name, shape, at in p['slots']:
        sl = slice(at, at + int(np.prod(shape)))
        err, scale = np.abs(both[sl] - full[sl]).max(), np.abs(full[sl]).max()
        print(f'ACC additivity n={n} torso={p["sizes"]} {name}: err/scale={err / scale:.2e}')
        if not err <= 2e-5 * scale:
            failures.append((name, err, scale))
    assert not failures, failures
    assert full[P + 5] == n and a[P + 5] == h and b[P + 5] == n - h
