"""TQC on an ensemble of 2 .. 8 critics without a GPU: models.ActorCriticEnsembleWithTargets, what the updaters refuse
by name, what the tonic_ensemble_quantile_* entries answer before any HIP call, the restatement
(tests/tqc_ensemble_ref.py) on a row computed by hand, and that agents.TQC() still builds the twin model."""
import os

import numpy as np
import pytest

import tqc_ensemble_ref
from test_offpolicy_entries_host import FAKE, INVALID, WORKSPACE, expect, torso_code
from test_tqc_host import _model as _twin_style_model, _sac_head

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('tonic_ensemble_quantile_workspace_bytes', 'tonic_ensemble_quantile_q_grad',
           'tonic_ensemble_quantile_actor_grad')
ENTRIES = {
    'tonic_ensemble_quantile_q_grad':
        'd_actor d_target_critics d_critics d_norm_mean d_norm_std norm_clip d_observations d_actions '
        'd_next_observations d_rewards d_discounts d_eps d_grad_sums B O H A M N drop_per_net entropy_coeff '
        'd_log_entropy_coeff d_workspace workspace_bytes stream',
    'tonic_ensemble_quantile_actor_grad':
        'd_actor d_critics d_norm_mean d_norm_std norm_clip d_observations d_eps d_grad_sums B O H A M N entropy_coeff '
        'd_log_entropy_coeff d_entropy_coeff_sums target_entropy d_workspace workspace_bytes stream',
}
ENTRIES = {name: spec.split() for name, spec in ENTRIES.items()}
TUNER = ('d_log_entropy_coeff', 'd_entropy_coeff_sums')
DEFAULTS = dict(norm_clip=5.0, B=17, O=17, H=64, A=6, M=25, N=5, drop_per_net=2, entropy_coeff=0.2,
                target_entropy=-6.0, d_log_entropy_coeff=None, d_entropy_coeff_sums=None, stream=None,
                workspace_bytes=None)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def query(lib, v):
    return lib.tonic_ensemble_quantile_workspace_bytes(v['B'], v['O'], v['A'], v['H'], v['M'], v['N'])


def call(lib, entry, **changes):
    values = dict(DEFAULTS, **changes)
    if values['workspace_bytes'] is None:
        values['workspace_bytes'] = query(lib, values)
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ENTRIES[entry]]
    return getattr(lib, entry)(*args), lib.tonic_last_error()


def ensemble(head, num_critics=5, **kwargs):
    import tonic_amd.torch as tt
    container = lambda **parts: tt.models.ActorCriticEnsembleWithTargets(num_critics=num_critics, **parts)   # noqa: E731
    return _twin_style_model(container, head, **kwargs)


# ---------------------------------------------------------------- 1. the model class

def _parts():
    import tonic_amd.torch as tt
    return dict(actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(),
                                      torso=tt.models.MLP((32, 32), torch.nn.ReLU), head=_sac_head()),
                critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(),
                                        torso=tt.models.MLP((32, 32), torch.nn.ReLU),
                                        head=tt.models.QuantileValueHead(7)))


def test_model_holds_n_independent_critics_in_order():
    import tonic_amd.torch as tt
    assert issubclass(tt.models.ActorCriticEnsembleWithTargets, tt.models.ActorCriticWithTargets)
    parts = _parts()
    model = tt.models.ActorCriticEnsembleWithTargets(**parts)
    assert model.num_critics == 5 and model.target_coeff == 0.005                   # the paper's default
    assert model.observation_normalizer is None and model.return_normalizer is None
    assert model.critic_1 is parts['critic'] and model.actor is parts['actor']
    for N in (2, 3, 8):
        model = tt.models.ActorCriticEnsembleWithTargets(num_critics=N, **_parts())
        assert model.num_critics == N and isinstance(model.num_critics, int)
        online = [getattr(model, f'critic_{z}') for z in range(1, N + 1)]
        targets = [getattr(model, f'target_critic_{z}') for z in range(1, N + 1)]
        assert not hasattr(model, f'critic_{N + 1}') and not hasattr(model, f'target_critic_{N + 1}')
        assert not hasattr(model, 'critic') and not hasattr(model, 'critic_0')
        assert len({id(net) for net in online + targets}) == 2 * N                  # independent objects
        nets = model._networks()
        assert [net for net, _ in nets] == [model.actor] + online + [model.target_actor] + targets
        assert [is_critic for _, is_critic in nets] == ([False] + [True] * N) * 2
    model = ensemble(tt.models.QuantileValueHead(7), num_critics=3)
    keys = sorted(model.state_dict())
    assert 'critic_3.head.quantile_layer.weight' in keys and 'target_critic_3.torso.model.0.bias' in keys
    assert not any(key.startswith(('critic_4.', 'target_critic_4.', 'critic.')) for key in keys)
    assert model.critic_3(torch.zeros(4, 5), torch.zeros(4, 2)).shape == (4, 7)
    # independent parameters: moving one critic moves no other
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        model.critic_2.head.quantile_layer.bias.add_(1.0)
    moved = [k for k, v in model.state_dict().items() if not torch.equal(v, before[k])]
    assert moved == ['critic_2.head.quantile_layer.bias']


@pytest.mark.parametrize('bad', [1, 9, 2.5, 0, -3, None, '5', True])
def test_model_refuses_a_count_outside_two_to_eight(bad):
    import tonic_amd.torch as tt
    with pytest.raises(ValueError, match='2 <= num_critics <= 8'):
        tt.models.ActorCriticEnsembleWithTargets(num_critics=bad, **_parts())


def test_targets_equal_the_online_networks_after_initialize():
    import tonic_amd.torch as tt
    model = ensemble(tt.models.QuantileValueHead(7), num_critics=4)
    state = model.state_dict()
    for z in range(1, 5):
        pairs = [(k, 'target_' + k) for k in state if k.startswith(f'critic_{z}.')]
        assert len(pairs) >= 6                              # (three layers' weight and bias, and the encoder's buffers)
        for online, target in pairs:
            assert torch.equal(state[online], state[target]), online
    for key in (k for k in state if k.startswith('actor.')):
        assert torch.equal(state[key], state['target_' + key]), key
    assert len(model.online_variables) == len(model.target_variables) == 8 + 4 * 6
    assert all(not p.requires_grad for p in model.target_variables)
    # (the deep copies are initialised one by one: the critics differ from each other, as the twin model's do)
    assert not torch.equal(state['critic_1.head.quantile_layer.weight'], state['critic_2.head.quantile_layer.weight'])


# ---------------------------------------------------------------- 2. the updaters

def test_tqc_updaters_refuse_by_name(monkeypatch):
    import tonic_amd.torch as tt
    quantile = tt.models.QuantileValueHead
    for make in (tt.updaters.TruncatedQuantileQLearning, tt.updaters.TwinCriticQuantileSoftPolicyGradient):
        name = make.__name__
        with pytest.raises(NotImplementedError, match=name + '.*twin critics.*ActorCriticEnsembleWithTargets'):
            make().initialize(_twin_style_model(tt.models.ActorCriticWithTargets, quantile(5)))
        with pytest.raises(NotImplementedError, match=name + '.*QuantileValueHead'):
            make().initialize(ensemble(tt.models.ValueHead(), 3))
        mixed = ensemble(quantile(5), 3)
        mixed.target_critic_3.head.num_quantiles = 6
        with pytest.raises(NotImplementedError, match=name + '.*same num_quantiles in all 6.*5, 5, 5, 5, 5, 6'):
            make().initialize(mixed)
        mixed = ensemble(quantile(5), 3)
        mixed.critic_3.head.num_quantiles = 4               # (a twin-only count of four heads would not see this one)
        with pytest.raises(NotImplementedError, match=name + '.*same num_quantiles.*5, 5, 4, 5, 5, 5'):
            make().initialize(mixed)
        with pytest.raises(NotImplementedError, match=f'{name}.*num_quantiles = 1 .. 32, got 33'):
            make().initialize(ensemble(quantile(33), 3))
        with pytest.raises(NotImplementedError, match=name + '.*Return normaliser'):
            make().initialize(ensemble(quantile(5), 3, return_normalizer=tt.normalizers.Return(0.99)))
        with pytest.raises(NotImplementedError, match='sac kernels serve GaussianPolicyHead.*DeterministicPolicyHead'):
            make().initialize(ensemble(quantile(5), 3, policy_head=tt.models.DeterministicPolicyHead()))
        with pytest.raises(NotImplementedError, match='torsos of 1 .. 4 layers'):
            make().initialize(ensemble(quantile(5), 3, sizes=(8, 8, 8, 8, 8)))
        # N M <= 256: 8 critics of 32 quantiles reach the bound and no served pair passes it, so the refusal is shown
        # under a smaller bound
        assert tt.updaters.POOLED_MAX == 256 == 8 * tt.updaters.QUANTILES_MAX
        with monkeypatch.context() as patch:
            patch.setattr(tt.updaters, 'POOLED_MAX', 128)
            with pytest.raises(NotImplementedError, match=f'{name}.*<= 128 values, got 5 x 32 = 160'):
                make().initialize(ensemble(quantile(32), 5))
    with pytest.raises(NotImplementedError, match='top_quantiles_to_drop_per_net = 0 .. num_quantiles - 1 = 4'):
        tt.updaters.TruncatedQuantileQLearning(top_quantiles_to_drop_per_net=5).initialize(ensemble(quantile(5), 3))


def test_other_updaters_refuse_an_ensemble_by_name():
    """Before, an ensemble reached a parameter-count mismatch (or a twin / single-critic message)."""
    import tonic_amd.torch as tt
    u, deterministic, mpo = tt.updaters, tt.models.DeterministicPolicyHead, tt.models.GaussianPolicyHead
    cases = [(u.TwinCriticSoftQLearning, None), (u.TwinCriticSoftDeterministicPolicyGradient, None),
             (u.TwinCriticDeterministicQLearning, deterministic), (u.DeterministicPolicyGradient, deterministic),
             (u.DeterministicQLearning, deterministic), (u.QRegression, deterministic),
             (u.DistributionalDeterministicQLearning, deterministic),
             (u.DistributionalDeterministicPolicyGradient, deterministic),
             (u.TwinCriticDistributionalDeterministicQLearning, deterministic),
             (u.ExpectedSARSA, mpo), (u.DistributionalExpectedSARSA, mpo),
             (u.MaximumAPosterioriPolicyOptimization, mpo)]
    heads = (lambda: tt.models.QuantileValueHead(5), tt.models.ValueHead,
             lambda: tt.models.DistributionalValueHead(-10., 10., 21))
    for make, head in cases:
        for critic_head in heads:
            model = ensemble(critic_head(), 3, policy_head=head() if head else None)
            with pytest.raises(NotImplementedError, match=f'{make.__name__} does not serve a '
                                                          'ActorCriticEnsembleWithTargets of 3 critics.*'
                                                          'TruncatedQuantileQLearning and '
                                                          'TwinCriticQuantileSoftPolicyGradient'):
                make().initialize(model)


def test_agent_still_builds_the_twin_model_and_takes_an_ensemble():
    import tonic_amd.torch as tt
    model = tt.agents.TQC().model
    assert type(model) is tt.models.ActorTwinCriticWithTargets and not hasattr(model, 'num_critics')
    assert model.critic_2.head.num_quantiles == 25 and not hasattr(model, 'critic_3')
    given = tt.models.ActorCriticEnsembleWithTargets(observation_normalizer=tt.normalizers.MeanStd(), **_parts())
    agent = tt.agents.TQC(model=given)
    assert agent.model is given
    assert type(agent.critic_updater) is tt.updaters.TruncatedQuantileQLearning
    assert type(agent.actor_updater) is tt.updaters.TwinCriticQuantileSoftPolicyGradient


# ---------------------------------------------------------------- 3. the C interface

def test_symbols_are_in_the_table_and_the_headers(lib):
    from tonic_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tonic_hip.h')).read()
    for symbol in SYMBOLS:
        assert symbol in _lib.SIGNATURES and f' {symbol}(' in header, symbol
        assert getattr(lib, symbol) is not None
    dev = open(os.path.join(ROOT, 'include', 'tonic_hip_dev.h')).read()
    assert 'tonic_debug_ensemble_quantile_loss' in _lib.SIGNATURES and ' tonic_debug_ensemble_quantile_loss(' in dev
    for entry, names in ENTRIES.items():
        assert len(names) == len(_lib.SIGNATURES[entry][1]), entry
    assert len(_lib.SIGNATURES['tonic_ensemble_quantile_workspace_bytes'][1]) == 6
    assert len(_lib.SIGNATURES['tonic_debug_ensemble_quantile_loss'][1]) == 17
    assert lib.tonic_abi_version() == 22                                       # additive


@pytest.mark.parametrize('entry', ENTRIES)
def test_entries_answer_before_any_gpu_work(lib, entry):
    """Every failure has its own message with the numbers, and the call returns before a launch: every pointer is a
    fake address nobody reads (the method of tests/test_offpolicy_entries_host.py)."""
    name = entry.encode()
    for pointer in (p for p in ENTRIES[entry] if p.startswith('d_') and p not in TUNER):
        expect(call(lib, entry, **{pointer: None}), INVALID, name + b': a NULL pointer')
    for N in (1, 0, -2, 9, 64):
        expect(call(lib, entry, N=N, workspace_bytes=1 << 40), INVALID, b'%d critics (2 <= N <= 8)' % N)
    for M in (0, -3, 33, 64):
        expect(call(lib, entry, M=M, drop_per_net=0, workspace_bytes=1 << 40), INVALID,
               b'%d quantiles (1 <= M <= 32)' % M)
    for B in (0, -1):
        expect(call(lib, entry, B=B, workspace_bytes=1 << 40), INVALID, b'B %d' % B)
    if 'drop_per_net' in ENTRIES[entry]:
        for M, drop in ((25, 25), (25, -1), (1, 1), (32, 40)):
            expect(call(lib, entry, M=M, drop_per_net=drop), INVALID,
                   b'%d quantiles dropped per critic (0 <= drop_per_net < M = %d)' % (drop, M))
        expect(call(lib, entry, d_log_entropy_coeff=FAKE, workspace_bytes=16), WORKSPACE)
    else:
        expect(call(lib, entry, d_log_entropy_coeff=FAKE), INVALID,
               b'd_entropy_coeff_sums is NULL and the other is not')
        expect(call(lib, entry, d_entropy_coeff_sums=FAKE), INVALID,
               b'd_log_entropy_coeff is NULL and the other is not')
        expect(call(lib, entry, target_entropy=float('nan')), INVALID, b'target_entropy is not finite')
    for H in (64, 256, torso_code(lib, 'relu32x3')):
        for B, M, N in ((1, 1, 2), (17, 25, 5), (37, 32, 8)):
            need = query(lib, dict(DEFAULTS, B=B, H=H, M=M, N=N))
            expect(call(lib, entry, B=B, H=H, M=M, N=N, drop_per_net=0, workspace_bytes=need - 1), WORKSPACE,
                   name + b': workspace of %d bytes, %d needed' % (need - 1, need))


def test_queries(lib):
    """The ensemble's query grows with N, answers 0 outside 2 .. 8, and the twin query is the ensemble's at N = 2: no
    more than the twin layout of its own asked for (the figures below), so a caller that sized by those still fits."""
    for H in (64, 256):
        sizes = [lib.tonic_ensemble_quantile_workspace_bytes(37, 17, 6, H, 25, N) for N in range(2, 9)]
        assert all(b > a > 0 for a, b in zip(sizes, sizes[1:])), sizes
    for N in (1, 0, 9, -1):
        assert lib.tonic_ensemble_quantile_workspace_bytes(37, 17, 6, 64, 25, N) == 0
    for key, before in TWIN_QUERY.items():
        answer = lib.tonic_quantile_workspace_bytes(*key)
        assert answer == lib.tonic_ensemble_quantile_workspace_bytes(*key, 2), key
        assert 0 < answer <= before, key


# tonic_quantile_workspace_bytes(B, O, A, H, M) as the twin layout of its own answered (two target hidden regions)
TWIN_QUERY = {(1, 3, 1, 64, 1): 76544, (17, 17, 6, 64, 25): 170496, (37, 17, 6, 256, 32): 771840,
              (256, 17, 6, 256, 25): 4113408}


def test_loss_kernel_entry_refuses_before_a_launch(lib):
    entry = lib.tonic_debug_ensemble_quantile_loss

    def run(ld=32, M=25, N=5, drop=2, B=5, Bp=16, **null):
        p = lambda name: None if name in null else FAKE                    # noqa: E731
        status = entry(p('t'), p('th'), ld, p('r'), p('d'), p('logp'), M, N, drop, 0.2, None, p('g'), p('sample_m'), B,
                       Bp, 0, None)
        return status, lib.tonic_last_error()
    for name in ('t', 'th', 'r', 'd', 'logp', 'g', 'sample_m'):
        expect(run(**{name: True}), INVALID, b'a NULL pointer')
    for N in (1, 9):
        expect(run(N=N), INVALID, b'%d critics (2 <= N <= 8)' % N)
    for M in (0, 33):
        expect(run(M=M), INVALID, b'%d quantiles (1 <= M <= 32)' % M)
    for bad in (dict(drop=25), dict(drop=-1), dict(ld=24), dict(ld=48), dict(B=0), dict(B=17, Bp=16)):
        expect(run(**bad), INVALID, b'0 <= drop < M, M <= ld <= 32, 0 < B <= Bp')


# ---------------------------------------------------------------- 4. the restatement, by hand

def test_restatement_on_a_row_computed_by_hand():
    """N = 3, M = 2, d = 1: the pool {3, 1}, {2, 5}, {0, 4} sorts to 0 1 2 3 4 5 from critics 2 0 1 0 2 1; K = 3 keeps
    {0, 1, 2}; r = 0.5, disc = 0.5, alpha logp' = 1: y = {0, 0.5, 1}."""
    f = lambda *v: torch.tensor([list(v)], dtype=torch.float64)            # noqa: E731
    one = lambda v: torch.tensor([v], dtype=torch.float64)                 # noqa: E731
    targets = [f(3, 1), f(2, 5), f(0, 4)]
    y, source = tqc_ensemble_ref.truncated_targets(targets, one(0.5), one(0.5), one(2.0), 0.5, 1)
    assert y.tolist() == [[0.0, 0.5, 1.0]] and source.tolist() == [[2, 0, 1, 0, 2, 1]]
    thetas = [f(0, 3), f(0.75, 0.75), f(-2, 0.25)]
    loss, grads, q = tqc_ensemble_ref.critic_rows_with_gradients(targets, thetas, one(0.5), one(0.5), one(2.0), 0.5, 1)
    # theta 0, tau 1/4: u = {0, 0.5, 1}, clamp the same; theta 3, tau 3/4: u = {-3, -2.5, -2}, weight 1/4, clamp -1
    assert grads[0].tolist() == [[-(0.25 * 1.5) / 6, -(0.25 * -3.0) / 6]]
    # theta -2: u = {2, 2.5, 3} under tau 1/4: clamp 1 each
    assert grads[2][0, 0].item() == -(0.25 * 3.0) / 6
    assert q.tolist() == [(1.5 + 0.75 + (-1.75 / 2)) / 3]
    import tqc_ref
    want = sum(float(tqc_ref.quantile_huber_rows(theta, y)) for theta in thetas)
    assert float(loss) == pytest.approx(want, rel=1e-15)
    assert tqc_ensemble_ref.actor_rows(thetas, one(2.0), 0.5).tolist() == [1.0 - (1.5 + 0.75 - 0.875) / 3]
