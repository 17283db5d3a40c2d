"""QRegression without a GPU: the updater's surface, the tests' restatement (tests/q_regression_ref.py) against the
unmodified reference's own class where that is present, what tonic_q_regression_grad answers before any HIP call,
and what the updater refuses or routes to stock torch operators."""
import inspect
import os
import sys

import numpy as np
import pytest

import q_regression_ref as ref
from test_offpolicy_entries_host import (BAD_LOSSES, FAKE, INVALID, TORSOS, UNKNOWN_H, WORKSPACE, expect, loss_rule,
                                         torso_code)

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'tonic_q_regression_grad'
ARGUMENTS = ('d_critic d_norm_mean d_norm_std norm_clip d_observations d_actions d_returns d_grad_sums B O H A loss '
             'd_value_low d_value_high d_workspace workspace_bytes stream').split()
DEFAULTS = dict(norm_clip=5.0, B=17, O=17, H=64, A=6, loss=None, d_value_low=None, d_value_high=None, stream=None,
                workspace_bytes=None)


def _reference_present():
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    try:
        import reference_loader
        return reference_loader.reference_available()
    finally:
        sys.path.pop(0)


needs_reference = pytest.mark.skipif(not _reference_present(), reason='the reference checkout is not present')


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- 1. the surface

def test_updater_has_the_reference_signature():
    """updaters.QRegression(loss=None, optimizer=None, gradient_clip=0), initialize(model) and
    __call__(observations, actions, returns): critics.py:31-43."""
    import tonic_amd.torch as tt
    cls = tt.updaters.QRegression
    init = inspect.signature(cls.__init__).parameters
    assert list(init) == ['self', 'loss', 'optimizer', 'gradient_clip']
    assert [init[k].default for k in ('loss', 'optimizer', 'gradient_clip')] == [None, None, 0]
    assert list(inspect.signature(cls.initialize).parameters) == ['self', 'model']
    assert list(inspect.signature(cls.__call__).parameters) == ['self', 'observations', 'actions', 'returns']
    assert list(inspect.signature(cls.enqueue).parameters) == ['self', 'batch', 'info_row', 'n_global']
    updater = cls()
    assert (updater.stats_kind, updater.stock_capable, updater.default_lr) == (3, True, 1e-3)
    assert updater.loss is None and updater.loss_rule.kind == 0
    huber = torch.nn.HuberLoss(delta=0.5)
    updater.loss = huber
    assert updater.loss is huber and (updater.loss_rule.kind, updater.loss_rule.param) == (3, 0.5)


# ---------------------------------------------------------------- 2. the restatement against the reference

@needs_reference
@pytest.mark.parametrize('activation,loss,ranged,clip', [('ReLU', ('mse', None), False, None),
                                                          ('Tanh', ('huber', 0.5), True, 1.0),
                                                          ('ELU', ('smooth_l1', 2.0), False, None),
                                                          ('ReLU', ('l1', None), True, None)])
def test_restatement_is_the_reference_step(activation, loss, ranged, clip):
    """The unmodified reference's QRegression.__call__ in float32 on the CPU against the restatement in float64 from
    the same state_dict: loss and values to rtol 1e-6 (float32 rounding of sums of ~ten terms), the gradients it
    leaves on the critic to 1e-6 of each tensor's largest element, and its Adam step against torch.optim.Adam fed
    the restatement's gradients to atol 1e-6 — a thousandth of the 1e-3 a first Adam step moves an element by, which
    a gradient holds unless it is within 1e-3 of itself in float32 (none is, in nets this small)."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import reference_loader as rl
    tonic = rl.load_reference()
    models, normalizers = tonic.torch.models, tonic.torch.normalizers
    O, A, B, sizes = 7, 3, 13, (16, 12)
    torch.manual_seed(5)
    act = getattr(torch.nn, activation)
    model = models.ActorCriticWithTargets(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP((8,), torch.nn.Tanh),
                           head=models.DeterministicPolicyHead()),
        critic=models.Critic(encoder=models.ObservationActionEncoder(), torso=models.MLP(sizes, act),
                             head=models.ValueHead()),
        observation_normalizer=normalizers.MeanStd(clip=clip),
        return_normalizer=normalizers.Return(0.9) if ranged else None)
    model.initialize(rl.SyntheticSpace(-np.inf, np.inf, (O,)), rl.SyntheticSpace(-1, 1, (A,)))
    rng = np.random.RandomState(2)
    model.observation_normalizer.record(rng.normal(size=(30, O)).astype(np.float32) * 2 + 0.5)
    model.observation_normalizer.update()
    updater = tonic.torch.updaters.QRegression(loss=ref.torch_loss(*loss))
    updater.initialize(model)
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))              # noqa: E731
    observations, actions = f32(rng.normal(size=(B, O)) * 2), f32(rng.uniform(-1, 1, (B, A)))
    returns = f32(rng.normal(size=B) * (3 if ranged else 1))
    state = {k: v.detach().clone() for k, v in model.critic.state_dict().items()}
    norm = model.observation_normalizer
    if clip is not None:
        x = (observations - norm._mean) / norm._std
        assert float((x.abs() > clip).float().mean()) > 0.05
    low, high = (model.return_normalizer._low, model.return_normalizer._high) if ranged else (None, None)
    want = ref.step(state, observations, actions, returns, activation, loss, norm._mean, norm._std, clip, low, high)
    infos = updater(observations, actions, returns)
    np.testing.assert_allclose(float(infos['loss']), float(want['loss']), rtol=1e-6)
    np.testing.assert_allclose(infos['q'].numpy(), want['values'].numpy(), rtol=1e-6,
                               atol=1e-6 * float(want['values'].abs().max()))
    variables = models.trainable_variables(model.critic)
    assert [tuple(p.shape) for p in variables] == [tuple(p.shape) for p in want['params']]
    for i, (p, g) in enumerate(zip(variables, want['grads'])):
        np.testing.assert_allclose(p.grad.numpy(), g.numpy(), rtol=0, atol=1e-6 * float(g.abs().max()),
                                   err_msg=f'gradient {i}')
    stepped = [p.detach().float().clone().requires_grad_() for p in want['params']]
    adam = torch.optim.Adam(stepped, lr=1e-3)
    for p, g in zip(stepped, want['grads']):
        p.grad = g.float()
    adam.step()
    for i, (p, s) in enumerate(zip(variables, stepped)):
        np.testing.assert_allclose(p.detach().numpy(), s.detach().numpy(), rtol=0, atol=1e-6, err_msg=f'tensor {i}')


# ---------------------------------------------------------------- 3. the entry's statuses

def call(lib, **changes):
    values = dict(DEFAULTS, **changes)
    if values['workspace_bytes'] is None:
        values['workspace_bytes'] = lib.tonic_q_regression_workspace_bytes(values['B'], values['O'], values['A'],
                                                                           values['H'])
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ARGUMENTS]
    return getattr(lib, ENTRY)(*args), lib.tonic_last_error()


def test_entry_answers_before_any_gpu_work(lib):
    """Every pointer NULL in turn, B <= 0, unknown torso codes: -1 with the entry's "bad argument", also when the
    workspace is too small as well; every bad loss rule with the rule's message, ahead of a null pointer; one bound
    of the range without the other, ahead of both; a workspace of 16 bytes and one a byte short: -4.  Every pointer
    is a fake address nobody reads: each call returns before a launch."""
    from tonic_amd import _lib
    assert len(ARGUMENTS) == len(_lib.SIGNATURES[ENTRY][1])
    bad = (ENTRY + ': bad argument').encode()
    small = (ENTRY + ': workspace too small').encode()
    for pointer in (name for name in ARGUMENTS if name.startswith('d_') and 'value' not in name):
        expect(call(lib, **{pointer: None}), INVALID, bad)
        expect(call(lib, **{pointer: None}, workspace_bytes=16), INVALID, bad)
    for B in (0, -1):
        expect(call(lib, B=B), INVALID, bad)
        expect(call(lib, B=B, workspace_bytes=16), INVALID, bad)
    for code in UNKNOWN_H:
        expect(call(lib, H=code, workspace_bytes=1 << 40), INVALID, bad)
    for rule, message in BAD_LOSSES.values():
        expect(call(lib, loss=loss_rule(*rule)), INVALID, message)
        expect(call(lib, loss=loss_rule(*rule), d_critic=None), INVALID, message)
        expect(call(lib, loss=loss_rule(*rule), B=0, workspace_bytes=16), INVALID, message)
    for rule in ((0, 0.0), (1, 0.0), (2, 0.0), (2, 1.5), (3, 1.0)):
        expect(call(lib, loss=loss_rule(*rule), workspace_bytes=16), WORKSPACE, small)
    for pair, missing in ((dict(d_value_low=FAKE), b'd_value_high is NULL'),
                          (dict(d_value_high=FAKE), b'd_value_low is NULL')):
        message = ENTRY.encode() + b': ' + missing
        expect(call(lib, **pair), INVALID, message)
        expect(call(lib, d_grad_sums=None, **pair), INVALID, message)
        expect(call(lib, loss=loss_rule(4, 1.0), **pair), INVALID, message)
    expect(call(lib, d_value_low=FAKE, d_value_high=FAKE, workspace_bytes=16), WORKSPACE, small)
    expect(call(lib, workspace_bytes=16), WORKSPACE, small)
    expect(call(lib, workspace_bytes=0), WORKSPACE, small)


@pytest.mark.parametrize('torso', TORSOS)
def test_workspace_query(lib, torso):
    """Plain, deep and single-layer codes: the query is positive, no larger than tonic_offpolicy_workspace_bytes for
    the same shape, and one byte less is refused."""
    H = torso_code(lib, torso)
    small = (ENTRY + ': workspace too small').encode()
    for B, O, A in ((1, 3, 1), (17, 17, 6), (256, 17, 17), (100, 111, 8)):
        need = lib.tonic_q_regression_workspace_bytes(B, O, A, H)
        assert 0 < need <= lib.tonic_offpolicy_workspace_bytes(B, O, A, H), (B, O, A)
        expect(call(lib, B=B, O=O, A=A, H=H, workspace_bytes=need - 1), WORKSPACE, small)


def test_head_code_is_read_as_its_torso(lib):
    """A tonic_mlp_torso_head code (an actor's scale bounds): the critic ignores the bounds, the query answers what
    it answers for the torso's own code."""
    import ctypes
    sizes = (ctypes.c_int32 * 2)(64, 64)
    code = lib.tonic_mlp_torso_head(2, ctypes.cast(sizes, ctypes.c_void_p), 1, 1e-3, 2.0)
    assert code > 0 and code != 64
    assert lib.tonic_q_regression_workspace_bytes(17, 17, 6, code) == lib.tonic_q_regression_workspace_bytes(17, 17, 6, 64)
    expect(call(lib, H=code, workspace_bytes=16), WORKSPACE)


# ---------------------------------------------------------------- 4. the updater's refusals and routes

def _model(container=None, head=None, sizes=(32, 32), activation=None, actor_sizes=None, actor_head=None, O=5, A=2,
           pack=True, **more):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    activation = activation or torch.nn.ReLU
    container = container or tt.models.ActorCriticWithTargets
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(),
                              torso=tt.models.MLP(actor_sizes or sizes, activation if actor_sizes is None else torch.nn.Tanh),
                              head=actor_head or tt.models.DeterministicPolicyHead()),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, activation),
                                head=head or tt.models.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd(), **more)
    model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    return model.pack('cpu') if pack else model


def test_updater_refuses_by_name():
    import tonic_amd.torch as tt
    updater = tt.updaters.QRegression()
    twin = _model(tt.models.ActorTwinCriticWithTargets, pack=False)
    with pytest.raises(NotImplementedError, match='QRegression.*critic_1 / critic_2'):
        updater.initialize(twin)
    distributional = _model(head=tt.models.DistributionalValueHead(-10., 10., 21), pack=False)
    with pytest.raises(NotImplementedError, match='QRegression.*DistributionalValueHead'):
        updater.initialize(distributional)
    with pytest.raises(NotImplementedError, match='QRegression.*model.pack'):
        updater.initialize(_model(pack=False))
    with pytest.raises(NotImplementedError, match='BCELoss.*does not run on the HIP engine'):
        tt.updaters.QRegression(loss=torch.nn.BCELoss())
    with pytest.raises(NotImplementedError, match="reduction='sum'"):
        tt.updaters.QRegression(loss=torch.nn.MSELoss(reduction='sum'))
    with pytest.raises(NotImplementedError, match='delta > 0'):
        tt.updaters.QRegression().loss = torch.nn.HuberLoss(delta=0.0)
    with pytest.raises(NotImplementedError, match='Adagrad'):
        tt.updaters.QRegression(optimizer=lambda p: torch.optim.Adagrad(p)).initialize(_model())


def test_routes(monkeypatch, lib):
    """The HIP entry: a packed critic on a torso inside the kernels' envelope, whatever the actor is.  Stock torch
    operators: a five-layer torso, TONIC_AMD_TORSO_STOCK=1 on a torso the layer-by-layer route serves, a plain
    ActorCritic with a Q-critic."""
    import tonic_amd.torch as tt
    monkeypatch.delenv('TONIC_AMD_TORSO_STOCK', raising=False)

    def routed(model, **arguments):
        updater = tt.updaters.QRegression(**arguments)
        updater.initialize(model)
        trained = tt.models.trainable_variables(model.critic)
        assert len(updater.variables) == len(trained) and all(a is b for a, b in zip(updater.variables, trained))
        return updater
    plain = routed(_model())
    assert plain.stock is False and plain.hidden == 32 and (plain.observation_size, plain.action_size) == (5, 2)
    assert plain.flat is plain.model.flat_critics and plain.count == lib.tonic_q_critic_param_count(5, 2, 32)
    other_actor = routed(_model(actor_sizes=(24,), actor_head=tt.models.GaussianPolicyHead(scale_min=1e-3)))
    assert other_actor.stock is False and other_actor.hidden == 32
    layered = routed(_model(sizes=(40,), activation=torch.nn.Tanh), loss=torch.nn.L1Loss(), gradient_clip=1.0)
    assert layered.stock is False and layered.hidden == lib.tonic_mlp_torso(
        1, ctypes_sizes(40), 2) and layered.gradient_clip == 1.0
    ranged = routed(_model(return_normalizer=tt.normalizers.Return(0.99)))
    assert ranged.stock is False and None not in ranged.range_pointers()
    assert plain.range_pointers() == (None, None)
    deep = routed(_model(sizes=(16,) * 5))
    assert deep.stock is True and deep.hidden is None and isinstance(deep.torch_optimizer, torch.optim.Adam)
    monkeypatch.setenv('TONIC_AMD_TORSO_STOCK', '1')
    assert routed(_model(sizes=(40,), activation=torch.nn.Tanh)).stock is True
    assert routed(_model()).stock is False                    # (the plain torso has no stock switch, as for DDPG)
    monkeypatch.delenv('TONIC_AMD_TORSO_STOCK')
    unpadded = routed(_model(tt.models.ActorCritic), optimizer=lambda p: torch.optim.SGD(p, lr=0.1, momentum=0.9))
    assert unpadded.stock is True and unpadded.flat is unpadded.model.flat_critic
    assert isinstance(unpadded.torch_optimizer, torch.optim.SGD)


def ctypes_sizes(*sizes):
    import ctypes
    return ctypes.cast((ctypes.c_int32 * len(sizes))(*sizes), ctypes.c_void_p)


def test_stock_route_is_the_reference_arithmetic_on_the_cpu():
    """The stock route needs no device: four calls on a five-layer torso against torch autograd on a copy of the
    critic with torch.optim.Adam, every parameter and the logged loss / q to float32 rounding."""
    import copy
    import tonic_amd.torch as tt
    torch.manual_seed(3)
    model = _model(sizes=(16,) * 5, activation=torch.nn.Tanh)
    twin = copy.deepcopy(model.critic)
    for p in twin.parameters():
        p.data = p.data.clone()
    variables = [p for name, p in twin.named_parameters() if 'normalizer' not in name]
    for p in variables:
        p.requires_grad_(True)
    adam = torch.optim.Adam(variables, lr=1e-3)
    updater = tt.updaters.QRegression(loss=torch.nn.SmoothL1Loss(beta=0.5), gradient_clip=0.5)
    updater.initialize(model)
    rng = np.random.RandomState(0)
    for _ in range(4):
        f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))          # noqa: E731
        observations, actions, returns = f32(rng.normal(size=(9, 5))), f32(rng.uniform(-1, 1, (9, 2))), \
            f32(rng.normal(size=9))
        adam.zero_grad()
        values = twin(observations, actions)
        loss = torch.nn.functional.smooth_l1_loss(values, returns, beta=0.5)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(variables, 0.5)
        adam.step()
        infos = updater(observations, actions, returns)
        np.testing.assert_allclose(float(infos['loss']), float(loss.detach()), rtol=1e-6)
        np.testing.assert_allclose(float(infos['q']), float(values.detach().mean()), rtol=1e-5, atol=1e-7)
    for p, q in zip(tt.models.trainable_variables(model.critic), variables):
        np.testing.assert_allclose(p.detach().numpy(), q.detach().numpy(), rtol=0, atol=1e-6)
