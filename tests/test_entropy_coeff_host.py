"""SAC's learned entropy coefficient without a device: `updaters.EntropyCoeffTuning`'s constructor and refusals, what
`agents.SAC(entropy_coeff_updater=...)` refuses before it builds anything, the two C entries' declarations and the
statuses they answer before any HIP call (the method of tests/test_offpolicy_entries_host.py: fake pointers, calls
shaped to return before a launch), and tests/entropy_coeff_ref.py against the reference's own statements of the SAC
steps when the coefficient is frozen."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import entropy_coeff_ref as ref
from test_offpolicy_entries_host import _ACTOR, _TWIN, _WS, DEFAULTS, FAKE, INVALID, OK, WORKSPACE

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    'tonic_tempered_twin_q_grad': (_TWIN + ' loss d_value_low d_value_high d_log_entropy_coeff' + _WS).split(),
    'tonic_tempered_actor_q_grad': (_ACTOR + ' d_value_low d_value_high d_log_entropy_coeff d_entropy_coeff_sums '
                                    'target_entropy' + _WS).split(),
}
VALUES = dict(DEFAULTS, target_entropy=-6.0)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def call(lib, entry, **changes):
    values = dict(VALUES, **changes)
    if values['workspace_bytes'] is None:
        values['workspace_bytes'] = lib.tonic_offpolicy_workspace_bytes(values['B'], values['O'], values['A'],
                                                                        values['H'])
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ENTRIES[entry]]
    return getattr(lib, entry)(*args), lib.tonic_last_error()


# ---------------------------------------------------------------------------------- the updater

def test_constructor_defaults_and_refusals():
    from tonic_amd.torch import updaters
    tuner = updaters.EntropyCoeffTuning()
    assert tuner.target_entropy is None and tuner.initial_entropy_coeff == 1.0 and tuner.optimizer is None
    assert tuner.hyper == dict(kind='adam', lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                               maximize=False)
    assert tuner.stats_kind == 3 and tuner.log_entropy_coeff is None
    for bad in (0, 0.0, -0.2, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match='initial_entropy_coeff'):
            updaters.EntropyCoeffTuning(initial_entropy_coeff=bad)
    for bad in (math.nan, math.inf):
        with pytest.raises(ValueError, match='target_entropy'):
            updaters.EntropyCoeffTuning(target_entropy=bad)
    sgd = updaters.EntropyCoeffTuning(optimizer=lambda params: torch.optim.SGD(params, lr=0.1, momentum=0.5))
    assert sgd.hyper['kind'] == 'sgd' and sgd.hyper['lr'] == 0.1 and sgd.hyper['momentum'] == 0.5
    rms = updaters.EntropyCoeffTuning(optimizer=lambda params: torch.optim.RMSprop(params, lr=0.01))
    assert rms.hyper['kind'] == 'rmsprop'
    # the usual refusals of optimizer_hyperparameters, by name
    with pytest.raises(NotImplementedError, match='Adagrad'):
        updaters.EntropyCoeffTuning(optimizer=lambda params: torch.optim.Adagrad(params))
    with pytest.raises(NotImplementedError, match='tensor lr'):
        updaters.EntropyCoeffTuning(optimizer=lambda params: torch.optim.Adam(params, lr=torch.tensor(1e-3)))


def _host_model(action_size):
    head = types.SimpleNamespace(loc_layer=[torch.nn.Linear(4, action_size)])
    return types.SimpleNamespace(flat_online=torch.zeros(1), actor=types.SimpleNamespace(head=head))


@pytest.mark.parametrize('action_size', [1, 6])
def test_target_entropy_resolves_to_minus_the_action_size(lib, action_size):
    from tonic_amd.torch import updaters
    tuner = updaters.EntropyCoeffTuning(initial_entropy_coeff=0.2)
    tuner.initialize(_host_model(action_size))
    assert tuner.target_entropy == -float(action_size)
    value = tuner.log_entropy_coeff
    assert value.dtype == torch.float32 and tuple(value.shape) == (1,)
    assert float(value) == float(np.float32(math.log(0.2)))
    assert tuner.grad_sums.numel() == 1 + updaters.INFO_WIDTH and tuner.count == 1
    assert abs(tuner.entropy_coeff - 0.2) < 1e-7
    given = updaters.EntropyCoeffTuning(target_entropy=-1.5)
    given.initialize(_host_model(action_size), action_size)
    assert given.target_entropy == -1.5 and float(given.log_entropy_coeff) == 0.0
    # the checkpoint's form
    state = tuner.state_dict()
    assert list(state) == ['log_entropy_coeff'] and state['log_entropy_coeff'].device.type == 'cpu'
    given.load_state_dict(state)
    assert given.log_entropy_coeff.view(torch.int32).item() == value.view(torch.int32).item()


def test_stock_sums_have_the_entrys_layout(lib):
    from tonic_amd.torch import updaters
    tuner = updaters.EntropyCoeffTuning(initial_entropy_coeff=0.5, target_entropy=-3.0)
    tuner.initialize(_host_model(3))
    log_probs = torch.tensor([1.5, -2.0, 4.25, 0.5])
    tuner.stock_sums(log_probs)
    log_alpha = float(tuner.log_entropy_coeff)
    excess = float((log_probs.double() - 3.0).sum())
    want = [-excess, -log_alpha * excess, float(log_probs.sum()), math.exp(log_alpha) * 4, 0, 0, 4, 0, 0]
    np.testing.assert_allclose(tuner.grad_sums.numpy(), want, rtol=1e-6, atol=0)


def test_sac_refuses_other_updaters_by_name():
    """Before anything is built: no device is needed to be told."""
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    spaces = Box(-np.inf, np.inf, (5,)), Box(-1, 1, (3,))
    agent = tt.agents.SAC(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning(),
                          actor_updater=tt.updaters.DeterministicPolicyGradient(),
                          critic_updater=tt.updaters.TwinCriticSoftQLearning())
    with pytest.raises(NotImplementedError, match='actor_updater=DeterministicPolicyGradient'):
        agent.initialize(*spaces, seed=0)
    agent = tt.agents.SAC(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning(),
                          critic_updater=tt.updaters.TwinCriticDeterministicQLearning())
    with pytest.raises(NotImplementedError, match='critic_updater=TwinCriticDeterministicQLearning'):
        agent.initialize(*spaces, seed=0)

    class Mine(tt.updaters.TwinCriticSoftQLearning):        # exactly the class: a subclass may compute anything
        pass
    agent = tt.agents.SAC(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning(), critic_updater=Mine())
    with pytest.raises(NotImplementedError, match='critic_updater=Mine'):
        agent.initialize(*spaces, seed=0)
    assert tt.agents.SAC().entropy_coeff_updater is None


# ---------------------------------------------------------------------------------- the C ABI

def test_entries_are_declared_prototyped_and_exported(lib):
    """Fails on ABI 21: neither symbol exists there."""
    from tonic_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tonic_hip.h')).read()
    assert re.search(r'#define TONIC_ABI_VERSION 22\b', header)
    assert _lib.ABI_VERSION == 22 and lib.tonic_abi_version() == 22
    assert re.search(r'\b22 = tonic_tempered_twin_q_grad / tonic_tempered_actor_q_grad', header)      # the history
    exported = ctypes.CDLL(_lib.LIBRARY_PATH)
    for entry, names in ENTRIES.items():
        declared = re.search(r'\bint %s\s*\(([^;{}()]*)\)\s*;' % entry, header)
        assert declared, entry
        assert declared.group(1).count(',') + 1 == len(names) == len(_lib.SIGNATURES[entry][1]), entry
        for name in names:
            assert re.search(r'\b%s\b' % name, declared.group(1)), (entry, name)
        assert hasattr(exported, entry), entry
    # the argument lists of the *_ranged entries plus the coefficient's
    for entry, base in (('tonic_tempered_twin_q_grad', 'tonic_twin_q_grad_ranged'),
                        ('tonic_tempered_actor_q_grad', 'tonic_actor_q_grad_ranged')):
        ranged, tempered = _lib.SIGNATURES[base][1], _lib.SIGNATURES[entry][1]
        extra = len(tempered) - len(ranged)
        assert tempered[:len(ranged) - 3] == ranged[:-3] and tempered[-3:] == ranged[-3:] and extra in (1, 3)


@pytest.mark.parametrize('entry', ENTRIES)
def test_statuses_before_any_launch(lib, entry):
    actor = entry == 'tonic_tempered_actor_q_grad'
    short = dict(workspace_bytes=16)
    # valid arguments reach the workspace check (the last one ahead of the device)
    status, error = call(lib, entry, **short)
    assert status == WORKSPACE and b'workspace too small' in error
    # NULL coefficient: the *_ranged entry's checks, nothing more (the actor entry: the sums NULL with it)
    none = dict(d_log_entropy_coeff=None, **(dict(d_entropy_coeff_sums=None) if actor else {}))
    assert call(lib, entry, **none, **short)[0] == WORKSPACE
    for kind in (0, 2) if not actor else (0,):
        assert call(lib, entry, kind=kind, **none, **short)[0] == WORKSPACE        # (as the *_ranged entry serves them)
        # a coefficient with a kind that has no entropy term: refused, also when the workspace is short as well
        for more in ({}, short):
            status, error = call(lib, entry, kind=kind, **more)
            assert status == INVALID and b'has no entropy term' in error and entry.encode() in error, error
    # half a value range still answers first, as in the *_ranged entries
    status, error = call(lib, entry, d_value_low=FAKE, **short)
    assert status == INVALID and b'both or neither' in error
    if actor:
        for missing in ('d_log_entropy_coeff', 'd_entropy_coeff_sums'):
            status, error = call(lib, entry, **{missing: None}, **short)
            assert status == INVALID and missing.encode() in error and b'both or neither' in error, error
        for bad in (math.nan, math.inf):
            status, error = call(lib, entry, target_entropy=bad, **short)
            assert status == INVALID and b'target_entropy' in error
    assert OK == 0


# ---------------------------------------------------------------------------------- the float64 restatement

def _model(O, A, sizes=(24, 16)):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                        distribution=tt.models.SquashedMultivariateNormalDiag)
    model = tt.models.ActorTwinCriticWithTargets(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, torch.nn.Tanh),
                              head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, torch.nn.Tanh),
                                head=tt.models.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd())
    torch.manual_seed(3)
    model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    with torch.no_grad():                       # targets that differ from the online critics
        for p in list(model.target_critic_1.parameters()) + list(model.target_critic_2.parameters()):
            p.add_(0.05 * torch.randn_like(p))
    return model.double()


def test_frozen_coefficient_is_the_reference_sac_step():
    """tests/entropy_coeff_ref.py at log_alpha = log 0.2, stepped by nobody, against the statements of the
    reference's updaters (critics.py:202-235, actors.py:238-267, entropy_coeff = 0.2) on the package's own modules
    with autograd, float64: targets, both losses and every gradient."""
    from tonic_amd.torch.updaters import squashed_sample
    O, A, B, coeff = 5, 3, 19, 0.2
    model = _model(O, A)
    rng = np.random.RandomState(0)
    f64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))             # noqa: E731
    batch = dict(observations=f64(rng.normal(size=(B, O))), actions=f64(rng.uniform(-1, 1, (B, A))),
                 next_observations=f64(rng.normal(size=(B, O))), rewards=f64(rng.normal(size=B)),
                 discounts=f64(0.99 * (rng.uniform(size=B) > 0.2)))
    eps_critic, eps_actor = f64(rng.normal(size=(B, A))), f64(rng.normal(size=(B, A)))

    # the reference's statements
    with torch.no_grad():
        actions, log_probs = squashed_sample(model.actor(batch['next_observations']), eps_critic)
        next_values = torch.min(model.target_critic_1(batch['next_observations'], actions),
                                model.target_critic_2(batch['next_observations'], actions))
        returns = batch['rewards'] + batch['discounts'] * (next_values - coeff * log_probs)
    mse = torch.nn.MSELoss()
    want_critic = mse(model.critic_1(batch['observations'], batch['actions']), returns) + \
        mse(model.critic_2(batch['observations'], batch['actions']), returns)
    critic_variables = [p for p in list(model.critic_1.parameters()) + list(model.critic_2.parameters())
                        if p.requires_grad]           # (the encoder holds the normaliser's statistics)
    want_critic_grads = torch.autograd.grad(want_critic, critic_variables)
    actions, log_probs = squashed_sample(model.actor(batch['observations']), eps_actor)
    values = torch.min(model.critic_1(batch['observations'], actions), model.critic_2(batch['observations'], actions))
    want_actor = (coeff * log_probs - values).mean()
    actor_variables = [p for p in model.actor.parameters() if p.requires_grad]
    want_actor_grads = torch.autograd.grad(want_actor, actor_variables)

    # the restatement, the coefficient frozen (an optimizer that does not move it)
    def policy(observations):
        normal = model.actor(observations)._distribution
        return normal.mean, normal.stddev
    frozen = ref.Coefficient(math.log(coeff), -A, lambda params: torch.optim.SGD(params, lr=0.0))
    out = ref.iteration(policy, [model.critic_1, model.critic_2], [model.target_critic_1, model.target_critic_2],
                        batch, eps_critic, eps_actor, frozen)
    assert out['next_log_alpha'] == out['log_alpha'] == math.log(coeff)
    np.testing.assert_allclose(out['returns'].numpy(), returns.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(float(out['critic_loss']), float(want_critic), rtol=1e-12)
    np.testing.assert_allclose(float(out['actor_loss']), float(want_actor), rtol=1e-12)
    np.testing.assert_allclose(out['log_probs'].numpy(), log_probs.detach().numpy(), rtol=1e-12, atol=1e-12)
    for got, want in zip(torch.autograd.grad(out['critic_loss'], critic_variables), want_critic_grads):
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-10, atol=1e-14)
    for got, want in zip(torch.autograd.grad(out['actor_loss'], actor_variables), want_actor_grads):
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-10, atol=1e-14)
    # the coefficient's loss and sums: J = -log_alpha mean(logp + target), dJ / d log_alpha = -mean(logp + target)
    excess = log_probs.detach() - A
    np.testing.assert_allclose(out['coeff_loss'], -math.log(coeff) * float(excess.mean()), rtol=1e-12)
    np.testing.assert_allclose(float(out['coeff_sums']['grad']), -float(excess.sum()), rtol=1e-12)
    np.testing.assert_allclose(float(frozen.log_alpha.grad), -float(excess.mean()), rtol=1e-12)


@pytest.mark.parametrize('rule', ['adam', 'sgd', 'rmsprop'])
def test_coefficient_descends_towards_the_target_entropy(rule):
    """log-probabilities above -target (entropy below the target) raise alpha, below lower it — whatever the rule."""
    for log_probs, sign in ((torch.full((8,), 5.0, dtype=torch.float64), 1), (torch.full((8,), -5.0, dtype=torch.float64), -1)):
        coefficient = ref.Coefficient(0.0, -3.0, ref.OPTIMIZERS[rule])
        for _ in range(3):
            coefficient.step(log_probs)
        assert sign * coefficient.value > 0
