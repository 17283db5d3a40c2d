"""Entries of one on-policy operation that must be the SAME launches give the same bits: a *_wide entry at a
fused shape and the entry without a workspace; the plain / *_wide entry at the first wide shapes and its *_torso
form called with the default torso (2 layers of 64, Tanh); `max_workgroups` 0 and any width above the kernel's
own.  (The statuses and routes of the same entries without a device: test_onpolicy_entries_host.py.)"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (ctypes.c_int32 * 2)(64, 64)
DEFAULT_TORSO = (2, SIZES, 1)                     # layers, sizes, activation (1: Tanh)


@pytest.fixture(scope='module')
def lib():
    import tonic_amd  # noqa: F401
    from tonic_amd import _lib
    return _lib.load()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _pair(low, high):
    return (torch.tensor(low, dtype=torch.float32, device='cuda'),
            torch.tensor(high, dtype=torch.float32, device='cuda'))


class _Network:
    """A default-torso critic (A = None) or actor from `models` as a flat block on the device, with inputs."""

    def __init__(self, lib, O, A, n, seed):
        from tonic_amd.environments import Box
        from tonic_amd.torch import models
        self.lib, self.O, self.A, self.n = lib, O, A, n
        torch.manual_seed(seed)
        torso = models.MLP((64, 64), torch.nn.Tanh)
        if A is None:
            self.module = models.Critic(encoder=models.ObservationEncoder(), torso=torso, head=models.ValueHead())
        else:
            self.module = models.Actor(encoder=models.ObservationEncoder(), torso=torso,
                                       head=models.DetachedScaleGaussianPolicyHead())
        self.module.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A or 1,)))
        self.flat = models.FlatNetwork(self.module, 'cuda')
        self.P = self.flat.count
        rng = np.random.RandomState(seed + 1)

        def device(*shape, scale=1.0):
            return torch.as_tensor((rng.normal(size=shape) * scale).astype(np.float32), device='cuda')
        self.obs = device(n, O)
        self.mean, self.std = torch.zeros(O, device='cuda'), torch.ones(O, device='cuda')
        self.ret = device(n, scale=3.0)
        if A is not None:
            self.eps, self.actions, self.adv, self.old_logp = device(n, A), device(n, A, scale=0.5), device(n), \
                device(n, scale=0.1) - A
            self.adv_stats = torch.tensor([0.1, 1.2, 0.0, 1.0], device='cuda')    # mean, std, all_zero, normalise
        actor = 0 if A is None else 1
        need = max(lib.tonic_ppo_workspace_bytes(n, O, A or 1, actor),
                   lib.tonic_ppo_torso_workspace_bytes(n, O, A or 1, actor, 2, SIZES))
        assert need > 0
        self.workspace_bytes = int(need)

    def call(self, entry, prefix, leading, trailing, outputs):
        """One call of `entry` into fresh outputs and a fresh workspace; the outputs on the host."""
        from tonic_amd import _lib
        ws = torch.zeros(self.workspace_bytes, dtype=torch.uint8, device='cuda')
        trailing = [(_ptr(ws), ws.numel()) if t == 'workspace' else (t,) for t in trailing]
        args = [*prefix, *leading, *(_ptr(o) for o in outputs), self.n, self.O,
                *([] if self.A is None else [self.A]), *(x for t in trailing for x in t), None]
        _lib.check(getattr(self.lib, entry)(*args), entry)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outputs]

    def values(self, entry, value_range=None, torso=(), workspace=True):
        out = torch.full((self.n,), -7.0, device='cuda')
        trailing = (['workspace'] if workspace else []) + \
            ([_ptr(value_range[0]), _ptr(value_range[1])] if entry.endswith('_ranged') else [])
        return self.call(entry, torso, [_ptr(self.flat.flat), _ptr(self.mean), _ptr(self.std), 0.0, _ptr(self.obs)],
                         trailing, [out])

    def value_grads(self, entry, value_range=None, torso=(), max_workgroups=0):
        sums = torch.full((self.P + 8,), 3.0, device='cuda')
        trailing = ([] if torso else [max_workgroups]) + ['workspace'] + \
            ([_ptr(value_range[0]), _ptr(value_range[1])] if entry.endswith('_ranged') else [])
        return self.call(entry, torso, [_ptr(self.flat.flat), _ptr(self.mean), _ptr(self.std), 0.0, _ptr(self.obs),
                                        _ptr(self.ret)], trailing, [sums])

    def act(self, entry, torso=(), workspace=True):
        actions = torch.full((self.n, self.A), -7.0, device='cuda')
        log_probs = torch.full((self.n,), -7.0, device='cuda')
        return self.call(entry, torso, [_ptr(self.flat.flat), _ptr(self.obs), _ptr(self.eps)],
                         ['workspace'] if workspace else [], [actions, log_probs])

    def actor_grads(self, entry, torso=()):
        sums = torch.full((self.P + 8,), 3.0, device='cuda')
        trailing = [0.2, 0.01, None] + ([] if torso else [0]) + ['workspace']
        return self.call(entry, torso, [_ptr(self.flat.flat), _ptr(self.obs), _ptr(self.actions), _ptr(self.adv),
                                        _ptr(self.adv_stats), _ptr(self.old_logp)], trailing, [sums])


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.isfinite(g).all() and not (g == -7.0).all() and not (g == 3.0).all()
        assert np.array_equal(g, w), float(np.abs(g - w).max())


@pytest.mark.parametrize('O,n', [(5, 700), (32, 700), (17, 32768)])       # 32 768: the first values16 size
def test_value_forward_wide_is_the_plain_entry_at_fused_shapes(lib, O, n):
    net = _Network(lib, O, None, n, seed=O + n)
    _same(net.values('tonic_value_forward_wide'), net.values('tonic_value_forward', workspace=False))
    value_range = _pair(-35.5, 2.25)
    _same(net.values('tonic_value_forward_wide_ranged', value_range),
          net.values('tonic_value_forward_ranged', value_range, workspace=False))


@pytest.mark.parametrize('O,A,n', [(17, 6, 700), (32, 8, 700)])
def test_act_wide_is_the_plain_entry_at_fused_shapes(lib, O, A, n):
    net = _Network(lib, O, A, n, seed=O + A)
    _same(net.act('tonic_ppo_act_wide'), net.act('tonic_ppo_act', workspace=False))


def test_default_torso_is_the_wide_critic_at_the_first_wide_shape(lib):
    net = _Network(lib, 33, None, 700, seed=33)
    value_range = _pair(-35.5, 2.25)
    _same(net.values('tonic_value_forward_wide'), net.values('tonic_value_forward_torso', torso=DEFAULT_TORSO))
    _same(net.values('tonic_value_forward_wide_ranged', value_range),
          net.values('tonic_value_forward_torso_ranged', value_range, torso=DEFAULT_TORSO))
    _same(net.value_grads('tonic_value_regression_grad'),
          net.value_grads('tonic_value_regression_grad_torso', torso=DEFAULT_TORSO))
    _same(net.value_grads('tonic_value_regression_grad_ranged', value_range),
          net.value_grads('tonic_value_regression_grad_torso_ranged', value_range, torso=DEFAULT_TORSO))


def test_default_torso_is_the_wide_actor_at_the_first_wide_shape(lib):
    net = _Network(lib, 17, 9, 700, seed=9)
    _same(net.act('tonic_ppo_act_wide'), net.act('tonic_ppo_act_torso', torso=DEFAULT_TORSO))
    _same(net.actor_grads('tonic_ppo_actor_grad'), net.actor_grads('tonic_ppo_actor_grad_torso', torso=DEFAULT_TORSO))


def test_max_workgroups_reaches_the_fused_grad_only_below_its_own_width(lib):
    net = _Network(lib, 17, None, 700, seed=17)
    full, = net.value_grads('tonic_value_regression_grad')
    wider, = net.value_grads('tonic_value_regression_grad', max_workgroups=4096)
    assert np.isfinite(full).all() and full[net.P + 5] == net.n
    assert np.array_equal(wider, full)
    one, = net.value_grads('tonic_value_regression_grad', max_workgroups=1)
    # another grouping of the float32 partial sums: rounding level relative to the largest element, the bound
    # of test_gpu_parity.test_value_regression_grad_width_is_an_argument
    assert np.abs(one - full).max() <= 2e-6 * np.abs(full).max()
