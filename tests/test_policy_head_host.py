"""Host tests of the policy heads' surface (no device): the `H` codes that carry a Gaussian head's scale bounds
(tonic_mlp_torso_head), the rule that serves or refuses a head by name (updaters.policy_head_rule), the float64
restatement tests/policy_head_ref.py held to the unmodified reference where its checkout is present, and the
committed fixtures tests/golden/{sac,mpo}_scale_small.npz against their generator."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_head_ref as ph

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
REGISTERED = 1 << 30 | 1 << 29
TORSOS = [((48,), 1), ((256, 256), 1), ((400, 300), 1), ((64, 64), 2), ((64, 48, 32), 2), ((32, 32, 32, 16), 3)]


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def _plain(lib, sizes, activation):
    return lib.tonic_mlp_torso(len(sizes), (ctypes.c_int32 * len(sizes))(*sizes), activation)


def _code(lib, sizes, activation, low, high):
    return lib.tonic_mlp_torso_head(len(sizes), (ctypes.c_int32 * len(sizes))(*sizes), activation, low, high)


# ---------------------------------------------------------------- codes

@pytest.mark.parametrize('sizes,activation', TORSOS)
def test_codes_of_one_to_four_layer_torsos(lib, sizes, activation):
    """Default bounds (as float32) give tonic_mlp_torso's code; other bounds a registered code, two-layer torsos
    included; the same descriptor the same code, another descriptor another."""
    plain = _plain(lib, sizes, activation)
    assert plain > 0
    assert _code(lib, sizes, activation, 1e-4, 1.0) == plain
    assert _code(lib, sizes, activation, float(np.float32(1e-4)), 1) == plain
    bounded = _code(lib, sizes, activation, 0.2, 1.5)
    assert bounded > 0 and bounded & REGISTERED == REGISTERED and bounded != plain
    assert _code(lib, sizes, activation, 0.2, 1.5) == bounded
    assert _code(lib, sizes, activation, float(np.float32(0.2)), 1.5) == bounded        # what the kernels see
    other = _code(lib, sizes, activation, 0.2, 1.25)
    assert other > 0 and other not in (bounded, plain)
    assert _plain(lib, sizes, activation) == plain                          # a bounded descriptor is not the torso's
    # sizes and parameter counts are the torso's, whatever the bounds
    for O, A in ((17, 6), (3, 1)):
        for heads in (1, 2):
            assert lib.tonic_mlp_actor_param_count(O, bounded, A, heads) == \
                lib.tonic_mlp_actor_param_count(O, plain, A, heads) > 0
        assert lib.tonic_q_critic_param_count(O, A, bounded) == lib.tonic_q_critic_param_count(O, A, plain) > 0
        assert lib.tonic_offpolicy_workspace_bytes(33, O, A, bounded) == \
            lib.tonic_offpolicy_workspace_bytes(33, O, A, plain)
        assert lib.tonic_mpo_workspace_bytes(33, O, A, bounded, 7) == lib.tonic_mpo_workspace_bytes(33, O, A, plain, 7)


@pytest.mark.parametrize('low,high', [(0.0, 1.0), (0.5, 0.4), (float('nan'), 1.0), (0.1, float('nan')),
                                      (0.1, float('inf')), (float('inf'), float('inf')), (-0.1, 1.0), (1e-60, 1.0)])
def test_invalid_bounds_are_refused_with_both_values(lib, low, high):
    assert _code(lib, (256, 256), 1, low, high) == -1
    message = lib.tonic_last_error().decode()
    assert 'tonic_mlp_torso_head' in message and 'scale_min' in message and 'scale_max' in message, message
    assert f'{low:g}' in message and f'{high:g}' in message, message


def test_an_unrepresentable_torso_is_refused_as_by_tonic_mlp_torso(lib):
    assert _code(lib, (256, 256, 256, 256, 256), 1, 0.2, 1.5) < 0
    assert _code(lib, (4096, 16), 1, 0.2, 1.5) < 0
    assert _code(lib, (64, 64), 4, 0.2, 1.5) < 0
    assert lib.tonic_mlp_torso_head(2, None, 1, 0.2, 1.5) < 0


def test_a_plain_torso_with_bounds_is_served_like_the_plain_width(lib):
    """(256, 256) ReLU with bounds (0.2, 1.5): every size, support and image query answers as at H = 256."""
    H = 256
    code = _code(lib, (H, H), 1, 0.2, 1.5)
    assert code & REGISTERED == REGISTERED
    for O, A in ((17, 6), (111, 8), (67, 21), (9, 33)):
        for heads in (1, 2):
            assert lib.tonic_mlp_actor_param_count(O, code, A, heads) == lib.tonic_mlp_actor_param_count(O, H, A, heads)
            assert lib.tonic_q_iteration_supported(O, code, A, heads) == lib.tonic_q_iteration_supported(O, H, A, heads)
            assert lib.tonic_mlp_actor_image_bytes(O, code, A, heads) == lib.tonic_mlp_actor_image_bytes(O, H, A, heads)
        assert lib.tonic_q_critic_param_count(O, A, code) == lib.tonic_q_critic_param_count(O, A, H)
        for B in (1, 33, 100, 1024):
            assert lib.tonic_offpolicy_workspace_bytes(B, O, A, code) == lib.tonic_offpolicy_workspace_bytes(B, O, A, H)
            assert lib.tonic_q_iteration_workspace_bytes(B, O, A, code) == \
                lib.tonic_q_iteration_workspace_bytes(B, O, A, H)
            assert lib.tonic_mpo_workspace_bytes(B, O, A, code, 20) == lib.tonic_mpo_workspace_bytes(B, O, A, H, 20)
            assert lib.tonic_distributional_workspace_bytes(B, O, A, code, 51) == \
                lib.tonic_distributional_workspace_bytes(B, O, A, H, 51)
            for nets in (1, 2):
                for passes in (1, 2):
                    assert lib.tonic_q_iteration_ahead_supported(B, O, code, A, nets, passes) == \
                        lib.tonic_q_iteration_ahead_supported(B, O, H, A, nets, passes)
    assert lib.tonic_mlp_actor_image_bytes(17, code, 6, 2) > 0
    assert lib.tonic_q_iteration_supported(17, code, 6, 2) == 1 and lib.tonic_q_iteration_supported(111, code, 8, 2) == 1
    assert lib.tonic_q_iteration_ahead_supported(100, 17, code, 6, 2, 2) == 1
    # an uneven two-layer torso with bounds: the packed code's answers (no fused iteration, no images)
    uneven, packed = _code(lib, (400, 300), 1, 0.2, 1.5), lib.tonic_mlp_hidden(400, 300, 1)
    assert lib.tonic_q_iteration_supported(17, uneven, 6, 2) == lib.tonic_q_iteration_supported(17, packed, 6, 2) == 0
    assert lib.tonic_mlp_actor_image_bytes(17, uneven, 6, 2) == 0
    assert lib.tonic_offpolicy_workspace_bytes(33, 17, 6, uneven) == lib.tonic_offpolicy_workspace_bytes(33, 17, 6, packed)


# ---------------------------------------------------------------- served or refused by name

def _heads():
    import tonic_amd.torch as tt
    return tt.models


def _served(family, **changes):
    m = _heads()
    if family == 'sac':
        arguments = dict(loc_activation=torch.nn.Identity, distribution=m.SquashedMultivariateNormalDiag)
        cls = m.GaussianPolicyHead
    elif family == 'mpo':
        arguments, cls = {}, m.GaussianPolicyHead
    elif family == 'deterministic':
        arguments, cls = {}, m.DeterministicPolicyHead
    else:
        arguments, cls = {}, m.DetachedScaleGaussianPolicyHead
    arguments.update(changes)
    return cls(**arguments)


REFUSED = [
    ('sac', 'loc_activation', dict(loc_activation=torch.nn.Tanh)),
    ('sac', 'scale_activation', dict(scale_activation=torch.nn.ReLU)),
    ('sac', 'distribution', dict(distribution=torch.distributions.normal.Normal)),
    ('sac', 'scale_min', dict(scale_min=0.0)),
    ('sac', 'scale_max', dict(scale_min=0.5, scale_max=0.4)),
    ('sac', 'scale_max', dict(scale_max=float('inf'))),
    ('sac', 'scale_min', dict(scale_min=float('nan'))),
    ('mpo', 'loc_activation', dict(loc_activation=torch.nn.Identity)),
    ('mpo', 'scale_activation', dict(scale_activation=torch.nn.Sigmoid)),
    ('mpo', 'distribution', dict(distribution=torch.distributions.laplace.Laplace)),
    ('mpo', 'scale_min', dict(scale_min=-1.0)),
    ('deterministic', 'activation', dict(activation=torch.nn.Identity)),
    ('deterministic', 'activation', dict(activation=torch.nn.Sigmoid)),
    ('on_policy', 'loc_activation', dict(loc_activation=torch.nn.Identity)),
    ('on_policy', 'distribution', dict(distribution=torch.distributions.laplace.Laplace)),
    ('on_policy', 'scale_max', dict(scale_max=0.5)),
    ('on_policy', 'scale_max', dict(scale_max=2)),
    ('on_policy', 'scale_min', dict(scale_min=1e-2)),
]


@pytest.mark.parametrize('family,argument,changes', REFUSED)
def test_a_head_the_kernels_do_not_compute_is_refused_by_name(family, argument, changes):
    from tonic_amd.torch.updaters import policy_head_rule
    with pytest.raises(NotImplementedError) as error:
        policy_head_rule(_served(family, **changes), family)
    message = str(error.value)
    assert argument in message and family in message and 'serve' in message, message
    assert f'got {argument}={changes[argument]!r}' in message, message


@pytest.mark.parametrize('family', ['sac', 'mpo', 'deterministic', 'on_policy'])
def test_subclasses_and_other_heads_are_refused(family):
    from tonic_amd.torch.updaters import policy_head_rule
    base = type(_served(family))
    sub = type('Mine', (base,), {})
    arguments = dict(loc_activation=torch.nn.Identity, distribution=_heads().SquashedMultivariateNormalDiag) \
        if family == 'sac' else {}
    with pytest.raises(NotImplementedError, match='Mine'):
        policy_head_rule(sub(**arguments), family)
    other = 'deterministic' if family != 'deterministic' else 'mpo'
    with pytest.raises(NotImplementedError, match=type(_served(other)).__name__):
        policy_head_rule(_served(other), family)


def test_served_heads_pass_with_their_float32_bounds():
    from tonic_amd.torch.updaters import policy_head_rule
    default = (np.float32(1e-4), np.float32(1))
    assert policy_head_rule(_served('sac'), 'sac') == default
    assert policy_head_rule(_served('mpo'), 'mpo') == default
    assert policy_head_rule(_served('deterministic'), 'deterministic') is None
    assert policy_head_rule(_served('on_policy'), 'on_policy') == default
    assert policy_head_rule(_served('on_policy', log_scale_init=-1.0, loc_fn=lambda m: None), 'on_policy') == default
    for family in ('sac', 'mpo'):
        got = policy_head_rule(_served(family, scale_min=0.2, scale_max=1.5, scale_fn=lambda m: None,
                                       loc_fn=lambda m: None), family)
        assert got == (np.float32(0.2), np.float32(1.5)) and all(type(v) is np.float32 for v in got)
        assert policy_head_rule(_served(family, scale_min=0.3, scale_max=0.3), family) == (np.float32(0.3),) * 2
    assert policy_head_rule(_served('deterministic', fn=lambda m: None), 'deterministic') is None


def test_the_actor_code_keeps_torso_width_and_adds_the_bounds(lib):
    """_torso_width is what it was; _actor_code is it for default bounds and tonic_mlp_torso_head's code otherwise."""
    import tonic_amd.torch as tt
    from tonic_amd.torch.updaters import _actor_code, _torso_width
    for sizes, activation, name in (((256, 256), 1, 'ReLU'), ((64, 48, 32), 2, 'Tanh'), ((400, 300), 1, 'ReLU')):
        torso = tt.models.MLP(sizes, getattr(torch.nn, name))
        width = _torso_width(torso)
        assert width == _plain(lib, sizes, activation)
        assert _actor_code(torso, None) == width
        assert _actor_code(torso, (np.float32(1e-4), np.float32(1))) == width
        assert _actor_code(torso, (np.float32(0.2), np.float32(1.5))) == _code(lib, sizes, activation, 0.2, 1.5)


# ---------------------------------------------------------------- the restatement against the reference

def _reference_present():
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    try:
        import reference_loader
        return reference_loader.reference_available()
    finally:
        sys.path.pop(0)


needs_reference = pytest.mark.skipif(not _reference_present(), reason='the reference checkout is not present')
LOW, HIGH = 0.2, 1.5


def _reference():
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import reference_loader as rl
    return rl, rl.load_reference()


def _close(got, want, name):
    got, want = np.asarray(got.detach() if torch.is_tensor(got) else got, np.float64), \
        np.asarray(want.detach() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * max(np.abs(want).max(), 1e-30), err_msg=name)


def _widen(scale_layers, gain=20.0):
    """Scales the scale layers' weights so that their pre-activations spread over both bounds."""
    with torch.no_grad():
        for layer in scale_layers:
            layer[0].weight.mul_(gain)


@needs_reference
@pytest.mark.parametrize('family', ['sac', 'mpo'])
def test_restated_head_equals_the_reference_forward(family):
    """gaussian_head against GaussianPolicyHead.forward of the unmodified reference with bounds (0.2, 1.5), float64:
    loc and scale equal bit for bit (the same torch operations), scales on both bounds and inside; the gradient of
    sum(scale) through the clamp as well."""
    rl, tonic = _reference()
    models = tonic.torch.models
    torch.manual_seed(4)
    if family == 'sac':
        head = models.GaussianPolicyHead(loc_activation=torch.nn.Identity, scale_min=LOW, scale_max=HIGH,
                                         distribution=models.SquashedMultivariateNormalDiag)
    else:
        head = models.GaussianPolicyHead(scale_min=LOW, scale_max=HIGH)
    head.initialize(24, 5)
    head.double()
    _widen([head.scale_layer])
    inputs = torch.randn(64, 24, dtype=torch.float64)
    distribution = head(inputs)
    normal = distribution._distribution if family == 'sac' else distribution
    loc_pre = head.loc_layer[0](inputs)
    scale_pre = head.scale_layer[0](inputs).detach().requires_grad_()
    loc, scale = ph.gaussian_head(loc_pre, scale_pre, LOW, HIGH, tanh_loc=family == 'mpo')
    assert torch.equal(loc, normal.loc) and torch.equal(scale, normal.scale)
    below, inside, above, _ = ph.regimes(scale_pre, LOW, HIGH)
    assert min(below, inside, above) >= 0.10, (below, inside, above)
    assert float(scale.detach().min()) == LOW and float(scale.detach().max()) == HIGH
    scale.sum().backward()
    raw = torch.nn.functional.softplus(scale_pre.detach())
    gate = (raw >= LOW) & (raw <= HIGH)
    assert torch.equal(scale_pre.grad != 0, gate)
    _close(scale_pre.grad, gate.double() * torch.sigmoid(scale_pre.detach()), 'd scale / d pre')
    # the float32 NumPy statement of sigma, on the same pre-activations: within float32 rounding of float64's
    sigma = ph.head32(scale_pre.detach().numpy().astype(np.float32), LOW, HIGH)
    assert sigma.dtype == np.float32 and sigma.min() == np.float32(LOW) and sigma.max() == np.float32(HIGH)
    np.testing.assert_allclose(sigma, scale.detach().numpy(), rtol=3e-7, atol=0)


def _model(tonic, rl, family, O, A, sizes):
    models = tonic.torch.models
    critic = models.Critic(encoder=models.ObservationActionEncoder(), torso=models.MLP(sizes, torch.nn.ReLU),
                           head=models.ValueHead())
    if family == 'sac':
        head = models.GaussianPolicyHead(loc_activation=torch.nn.Identity, scale_min=LOW, scale_max=HIGH,
                                         distribution=models.SquashedMultivariateNormalDiag)
        container = models.ActorTwinCriticWithTargets
    else:
        head = models.GaussianPolicyHead(scale_min=LOW, scale_max=HIGH)
        container = models.ActorCriticWithTargets
    model = container(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, torch.nn.ReLU), head=head),
        critic=critic, observation_normalizer=tonic.torch.normalizers.MeanStd())
    model.initialize(rl.SyntheticSpace(-np.inf, np.inf, (O,)), rl.SyntheticSpace(-1, 1, (A,)))
    return model


def _weights(net):
    return [p for name, p in net.named_parameters() if 'normalizer' not in name]


def _leaves(net):
    return [p.detach().clone().requires_grad_() for p in _weights(net)]


@needs_reference
def test_restated_sac_actor_step_equals_the_reference_updater():
    """sac_actor_terms against TwinCriticSoftDeterministicPolicyGradient.__call__ of the unmodified reference, both
    in float64 on the CPU, head bounds (0.2, 1.5) with the scale head widened over both bounds: the loss and every
    actor gradient within 1e-9 of the tensor's largest element."""
    rl, tonic = _reference()
    O, A, B, sizes = 9, 3, 40, (16, 12)
    torch.manual_seed(6)
    model = _model(tonic, rl, 'sac', O, A, sizes)
    u = tonic.torch.updaters.TwinCriticSoftDeterministicPolicyGradient(entropy_coeff=0.2)
    u.initialize(model)
    rng = np.random.RandomState(2)
    model.observation_normalizer.record(rng.normal(size=(30, O)).astype(np.float32) * 2 + 0.5)
    model.observation_normalizer.update()
    model.double()
    _widen([model.actor.head.scale_layer])
    obs = torch.as_tensor(rng.normal(size=(B, O)))
    networks = ph.Networks(len(sizes), model.observation_normalizer._mean.detach().double(),
                           model.observation_normalizer._std.detach().double(), LOW, HIGH, tanh_loc=False)
    actor = _leaves(model.actor)
    critics = [_leaves(model.critic_1), _leaves(model.critic_2)]
    below, inside, above, _ = ph.regimes(networks.heads(actor, obs)[1], LOW, HIGH)
    assert min(below, inside, above) >= 0.10, (below, inside, above)
    torch.manual_seed(17)
    noise = torch.randn(B, A, dtype=torch.float64)           # Normal.rsample: standard normals of loc's dtype
    terms = ph.sac_actor_terms(networks, actor, critics, obs, noise, u.entropy_coeff)
    terms.mean().backward()
    torch.manual_seed(17)
    infos = u(obs)
    _close(infos['loss'], terms.mean(), 'loss')
    for i, (p, leaf) in enumerate(zip(_weights(model.actor), actor)):
        _close(p.grad, leaf.grad, f'actor {i}')
    assert float(actor[-1].grad.abs().max()) > 0 and float(actor[-2].grad.abs().max()) > 0


@needs_reference
@pytest.mark.parametrize('per_dim', [True, False])
def test_restated_mpo_actor_step_equals_the_reference_updater(per_dim):
    """mpo_reference (tests/mpo_surface_reference.py) on policy_head_ref.Networks with bounds (0.2, 1.5) against
    MaximumAPosterioriPolicyOptimization.__call__ of the unmodified reference in float64: the actor's gradients, the
    logged losses.  Bound: 1e-9 of each tensor's largest element (the temperature loss carries the reference's
    float32 log S, see tests/test_mpo_surface_host.py)."""
    from mpo_surface_reference import mpo_reference
    rl, tonic = _reference()
    O, A, B, S, sizes, floor = 9, 3, 23, 5, (16, 12), -18.0
    torch.manual_seed(8)
    model = _model(tonic, rl, 'mpo', O, A, sizes)
    action_space = rl.SyntheticSpace(-1, 1, (A,))
    u = tonic.torch.updaters.MaximumAPosterioriPolicyOptimization(num_samples=S, per_dim_constraining=per_dim,
                                                                  min_log_dual=floor)
    u.initialize(model, action_space)
    rng = np.random.RandomState(3)
    model.observation_normalizer.record(rng.normal(size=(30, O)).astype(np.float32) * 2 + 0.5)
    model.observation_normalizer.update()
    model.double()
    with torch.no_grad():
        for p in model.actor.parameters():
            p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.05)
    _widen([model.actor.head.scale_layer, model.target_actor.head.scale_layer])
    K = A if per_dim else 1
    duals = np.concatenate([[0.5], np.full(K, 1.0), np.full(K, 2.0), [0.0]])
    u.min_log_dual = u.min_log_dual.double()
    at = 0
    for variable in u.dual_variables:
        n = variable.numel()
        variable.data = torch.as_tensor(duals[at:at + n]).double()
        at += n
    obs = torch.as_tensor(rng.normal(size=(B, O)))
    networks = ph.Networks(len(sizes), model.observation_normalizer._mean.detach().double(),
                           model.observation_normalizer._std.detach().double(), LOW, HIGH, tanh_loc=True)
    actor, target_actor, frozen = _leaves(model.actor), _leaves(model.target_actor), _leaves(model.target_critic)
    for leaves in (actor, target_actor):
        below, inside, above, _ = ph.regimes(networks.heads(leaves, obs)[1], LOW, HIGH)
        assert min(below, inside, above) >= 0.10, (below, inside, above)
    torch.manual_seed(17)
    eps = torch.randn(S, B, A, dtype=torch.float64)
    _, want_stats, _, _, _, _, _ = mpo_reference(networks, actor, target_actor, frozen, obs, eps.reshape(S * B, A),
                                                 duals, floor, u, S, True, per_dim)
    torch.manual_seed(17)
    infos = u(obs)
    for i, (p, leaf) in enumerate(zip(_weights(model.actor), actor)):
        _close(p.grad, leaf.grad, f'actor {i}')
    for i, name in enumerate(('policy_mean_loss', 'policy_std_loss', 'kl_mean_loss', 'kl_std_loss')):
        _close(np.asarray(infos[name]).reshape(()), np.asarray(want_stats[i]), name)


# ---------------------------------------------------------------- the committed fixtures

@pytest.mark.parametrize('name,sibling', [('sac_scale_small', 'sac_return_small'),
                                          ('mpo_scale_small', 'sac_return_small')])
def test_the_fixtures_are_small_and_hold_bounds_that_matter(name, sibling):
    path = os.path.join(GOLDEN, name + '.npz')
    assert os.path.getsize(path) < os.path.getsize(os.path.join(GOLDEN, sibling + '.npz'))
    g = np.load(path)
    small = np.load(os.path.join(GOLDEN, name.replace('_scale', '') + '.npz'))
    assert np.array_equal(g['cfg'][:7], small['cfg'][:7]) and tuple(g['torso_sizes']) == (32, 32)
    assert tuple(g['scale_bounds']) == (0.2, 1.5) and len(g['updates']) == 3
    steps, W, A = int(g['cfg'][7]), int(g['cfg'][2]), int(g['cfg'][1])
    assert g['act/actions'].shape == g['act/greedy_actions'].shape == g['act/policy_eps'].shape == (steps, W, A)
    for u in range(3):
        assert f'post{u}/actor.head.scale_layer.0.weight' in g.files and f'u{u}/indices' in g.files
    # the acting steps' scales leave the default bounds on both sides (float32 restatement of the initial actor)
    x = g['act/observations'].reshape(-1, g['act/observations'].shape[-1]).astype(np.float32)
    for layer in (0, 2):
        x = np.maximum(x @ g[f'init/actor.torso.model.{layer}.weight'].T + g[f'init/actor.torso.model.{layer}.bias'], 0)
    raw = ph.softplus32(x @ g['init/actor.head.scale_layer.0.weight'].T + g['init/actor.head.scale_layer.0.bias'])
    assert (raw < 0.2).mean() >= 0.05 and (raw > 1.0).mean() >= 0.05, ((raw < 0.2).mean(), (raw > 1.0).mean())


@needs_reference
def test_the_committed_fixtures_equal_their_generator(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'scripts', 'make_policy_head_goldens.py'),
                           '--out', str(tmp_path)], stdout=subprocess.DEVNULL)
    for name in ('sac_scale_small', 'mpo_scale_small'):
        want = np.load(os.path.join(GOLDEN, name + '.npz'))
        got = np.load(str(tmp_path / (name + '.npz')))
        assert sorted(want.files) == sorted(got.files)
        for key in want.files:
            assert np.array_equal(want[key], got[key]), (name, key)
