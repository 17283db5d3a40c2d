"""TQC without a GPU: the tests' restatement (tests/tqc_ref.py) pinned on hand-computed rows, what the
tonic_truncated_quantile_* entries answer before any HIP call, what the updaters and the agent refuse by name, the
QuantileValueHead's shapes and the agent's defaults."""
import itertools

import numpy as np
import pytest

import tqc_ref
from test_offpolicy_entries_host import FAKE, INVALID, SHAPES, TORSOS, UNKNOWN_H, WORKSPACE, expect, torso_code

torch = pytest.importorskip('torch')

ENTRIES = {
    'tonic_truncated_quantile_q_grad':
        'd_actor d_target_critics d_critics d_norm_mean d_norm_std norm_clip d_observations d_actions '
        'd_next_observations d_rewards d_discounts d_eps d_grad_sums B O H A M drop_per_net entropy_coeff '
        'd_log_entropy_coeff d_workspace workspace_bytes stream',
    'tonic_truncated_quantile_actor_grad':
        'd_actor d_critics d_norm_mean d_norm_std norm_clip d_observations d_eps d_grad_sums B O H A M entropy_coeff '
        'd_log_entropy_coeff d_entropy_coeff_sums target_entropy d_workspace workspace_bytes stream',
}
ENTRIES = {name: spec.split() for name, spec in ENTRIES.items()}
TUNER = ('d_log_entropy_coeff', 'd_entropy_coeff_sums')            # optional: NULL is the float coefficient
DEFAULTS = dict(norm_clip=5.0, B=17, O=17, H=64, A=6, M=25, drop_per_net=2, entropy_coeff=0.2, target_entropy=-6.0,
                d_log_entropy_coeff=None, d_entropy_coeff_sums=None, stream=None, workspace_bytes=None)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def query(lib, v):
    return lib.tonic_quantile_workspace_bytes(v['B'], v['O'], v['A'], v['H'], v['M'])


def call(lib, entry, **changes):
    values = dict(DEFAULTS, **changes)
    if values['workspace_bytes'] is None:
        values['workspace_bytes'] = query(lib, values)
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ENTRIES[entry]]
    return getattr(lib, entry)(*args), lib.tonic_last_error()


# ---------------------------------------------------------------- 1. the restatement, by hand

def test_restatement_on_a_row_computed_by_hand():
    """M = 2, d = 1: pool {3, 1} and {2, 5} sorts to 1 2 3 5, K = 2 keeps {1, 2}; r = 0.5, disc = 0.5, alpha logp' = 1:
    y = {0.5, 1.0}.  theta_1 = {0, 3}: tau = {1/4, 3/4}."""
    f = lambda *v: torch.tensor([list(v)], dtype=torch.float64)            # noqa: E731
    one = lambda v: torch.tensor([v], dtype=torch.float64)                 # noqa: E731
    y, source = tqc_ref.truncated_targets(f(3, 1), f(2, 5), one(0.5), one(0.5), one(2.0), 0.5, 1)
    assert y.tolist() == [[0.5, 1.0]] and source.tolist() == [[0, 1, 0, 1]]
    # theta 0: u = {0.5, 1}, both >= 0, weight 1/4, huber {0.125, 0.5}; theta 3: u = {-2.5, -2}, weight 1 - 3/4,
    # huber {2, 1.5}: (0.25 (0.625) + 0.25 (3.5)) / (M K = 4)
    rows = tqc_ref.quantile_huber_rows(f(0, 3), y)
    assert rows.tolist() == [(0.25 * 0.625 + 0.25 * 3.5) / 4]
    loss, g1, g2, q1, q2 = tqc_ref.critic_rows_with_gradients(f(3, 1), f(2, 5), f(0, 3), f(0.75, 0.75), one(0.5),
                                                              one(0.5), one(2.0), 0.5, 1)
    # d/d theta = -(1 / (M K)) sum_j weight clamp(u, -1, 1)
    assert g1.tolist() == [[-(0.25 * 0.5 + 0.25 * 1.0) / 4, -(0.25 * -1.0 + 0.25 * -1.0) / 4]]
    # theta 0.75 under both taus: u = {-0.25, 0.25}
    want = [-((1 - tau) * -0.25 + tau * 0.25) / 4 for tau in (0.25, 0.75)]
    np.testing.assert_allclose(g2.numpy(), [want], rtol=1e-15)
    assert (q1.tolist(), q2.tolist()) == ([1.5], [0.75])
    assert float(loss) == pytest.approx(float(rows) + float(tqc_ref.quantile_huber_rows(f(0.75, 0.75), y)), rel=1e-15)
    assert tqc_ref.actor_rows(f(0, 3), f(0.75, 0.75), one(2.0), 0.5).tolist() == [1.0 - (1.5 + 0.75) / 2]


def test_dropping_nothing_keeps_the_pool_and_twins_do_not_matter():
    rng = np.random.RandomState(0)
    t = torch.as_tensor(rng.normal(size=(4, 5)))
    zeros = torch.zeros(4, dtype=torch.float64)
    y, _ = tqc_ref.truncated_targets(t, t, zeros, zeros + 1, zeros, 0.0, 0)
    assert torch.equal(y, torch.sort(torch.cat([t, t], 1), 1)[0])
    y, _ = tqc_ref.truncated_targets(t, t, zeros, zeros + 1, zeros, 0.0, 2)
    assert torch.equal(y, torch.sort(t, 1)[0][:, :3].repeat_interleave(2, dim=1))


# ---------------------------------------------------------------- 2. the entries' statuses and the query

@pytest.mark.parametrize('entry', ENTRIES)
def test_entries_answer_before_any_gpu_work(lib, entry):
    """Every failure has its own message, and the call returns before a launch: every pointer is a fake address
    nobody reads (the method of tests/test_offpolicy_entries_host.py)."""
    from tonic_amd import _lib
    name = entry.encode()
    assert len(ENTRIES[entry]) == len(_lib.SIGNATURES[entry][1])
    for pointer in (p for p in ENTRIES[entry] if p.startswith('d_') and p not in TUNER):
        expect(call(lib, entry, **{pointer: None}), INVALID, name + b': a NULL pointer')
        expect(call(lib, entry, **{pointer: None}, workspace_bytes=16), INVALID, name + b': a NULL pointer')
    for B in (0, -1):
        expect(call(lib, entry, B=B, workspace_bytes=1 << 40), INVALID, b'B %d' % B)
    for code in UNKNOWN_H:
        expect(call(lib, entry, H=code, workspace_bytes=1 << 40), INVALID, b'H %d is not a torso' % code)
    for M in (0, -3, 33, 64):
        expect(call(lib, entry, M=M, drop_per_net=0, workspace_bytes=1 << 40), INVALID,
               b'%d quantiles (1 <= M <= 32)' % M)
        expect(call(lib, entry, M=M, drop_per_net=0, workspace_bytes=16), INVALID, b'1 <= M <= 32')
    if 'drop_per_net' in ENTRIES[entry]:
        for M, drop in ((25, 25), (25, -1), (1, 1), (32, 40)):
            expect(call(lib, entry, M=M, drop_per_net=drop), INVALID,
                   b'%d quantiles dropped per critic (0 <= drop_per_net < M = %d)' % (drop, M))
        for M, drop in ((25, 24), (25, 0), (1, 0), (32, 31)):
            expect(call(lib, entry, M=M, drop_per_net=drop, workspace_bytes=16), WORKSPACE)
        # the coefficient's pointer alone is the device form of alpha: accepted
        expect(call(lib, entry, d_log_entropy_coeff=FAKE, workspace_bytes=16), WORKSPACE)
    else:
        expect(call(lib, entry, d_log_entropy_coeff=FAKE), INVALID,
               b'd_entropy_coeff_sums is NULL and the other is not')
        expect(call(lib, entry, d_entropy_coeff_sums=FAKE), INVALID,
               b'd_log_entropy_coeff is NULL and the other is not')
        expect(call(lib, entry, d_log_entropy_coeff=FAKE, d_entropy_coeff_sums=FAKE, workspace_bytes=16), WORKSPACE)
        for bad in (float('nan'), float('inf'), -float('inf')):
            expect(call(lib, entry, target_entropy=bad), INVALID, b'target_entropy is not finite')
            expect(call(lib, entry, target_entropy=bad, d_log_entropy_coeff=FAKE, d_entropy_coeff_sums=FAKE), INVALID,
                   b'target_entropy is not finite')
    expect(call(lib, entry, workspace_bytes=16), WORKSPACE,
           name + b': workspace of 16 bytes, %d needed' % query(lib, DEFAULTS))
    for H in (64, 256, lib.tonic_mlp_hidden(40, 24, 2), torso_code(lib, 'relu32x3'), torso_code(lib, 'one256')):
        for B, M in ((1, 1), (17, 25), (37, 32)):
            need = query(lib, dict(DEFAULTS, B=B, H=H, M=M))
            expect(call(lib, entry, B=B, H=H, M=M, drop_per_net=0, workspace_bytes=need - 1), WORKSPACE,
                   name + b': workspace of %d bytes, %d needed' % (need - 1, need))


@pytest.mark.parametrize('torso', TORSOS)
def test_query_is_monotone_in_rows_and_quantiles(lib, torso):
    H = torso_code(lib, torso)
    for O, A in ((3, 1), (17, 6)):
        table = [[lib.tonic_quantile_workspace_bytes(B, O, A, H, M) for M in (1, 2, 16, 17, 25, 32)]
                 for B in (1, 5, 16, 17, 37, 256)]
        assert all(v > 0 for row in table for v in row)
        for row in table:                      # more quantiles never need less
            assert all(b >= a for a, b in zip(row, row[1:])), row
        for column in zip(*table):             # nor do more rows
            assert all(b >= a for a, b in zip(column, column[1:])), column
        assert table[-1][-1] > table[0][0] and table[0][3] > table[0][2] and table[3][0] > table[2][0]


def test_query_is_a_function_of_its_arguments(lib):
    import ctypes
    answers = lambda: [lib.tonic_quantile_workspace_bytes(B, O, A, torso_code(lib, torso), M)         # noqa: E731
                       for (B, O, A), M, torso in itertools.product(SHAPES, (1, 25), TORSOS)]
    want, saved = answers(), {}
    try:
        for name in ('q_images', 'policy_tail', 'q_chain'):
            value = ctypes.c_int32(0)
            assert lib.tonic_get_tuning(name.encode(), ctypes.addressof(value)) == 0, name
            saved[name] = value.value
            assert lib.tonic_set_tuning(name.encode(), 0) == 0, name
        assert answers() == want
    finally:
        for name, value in saved.items():
            lib.tonic_set_tuning(name.encode(), value)


def test_loss_kernel_entry_refuses_before_a_launch(lib):
    """The developer entry in the twin form: N = 2 and the twin row {loss, q1, q2}."""
    entry = lib.tonic_debug_ensemble_quantile_loss

    def run(ld=32, M=25, N=2, drop=2, B=5, Bp=16, twin_row=1, **null):
        p = lambda name: None if name in null else FAKE                    # noqa: E731
        status = entry(p('targets'), p('thetas'), ld, p('r'), p('d'), p('logp'), M, N, drop, 0.2, None, p('dlogits'),
                       p('sample_m'), B, Bp, twin_row, None)
        return status, lib.tonic_last_error()
    for name in ('targets', 'thetas', 'r', 'd', 'logp', 'dlogits', 'sample_m'):
        expect(run(**{name: True}), INVALID, b'a NULL pointer')
    for M in (0, 33):
        expect(run(M=M), INVALID, b'%d quantiles (1 <= M <= 32)' % M)
    for bad in (dict(drop=25), dict(drop=-1), dict(ld=24), dict(ld=48), dict(B=0), dict(B=17, Bp=16)):
        expect(run(**bad), INVALID, b'0 <= drop < M, M <= ld <= 32, 0 < B <= Bp')
    for N in (3, 8):
        expect(run(N=N), INVALID, b'the twin row {loss, q1, q2} is that of 2 critics, not of %d' % N)
    expect(run(N=3, twin_row=0, sample_m=True), INVALID, b'a NULL pointer')    # (N = 3 itself is served)


# ---------------------------------------------------------------- 3. the head, the updaters and the agent

def _sac_head():
    import tonic_amd.torch as tt
    return tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                        distribution=tt.models.SquashedMultivariateNormalDiag)


def _model(container, head, policy_head=None, O=5, A=2, sizes=(32, 32), return_normalizer=None):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, torch.nn.ReLU),
                              head=policy_head or _sac_head()),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(),
                                torso=tt.models.MLP(sizes, torch.nn.ReLU), head=head),
        observation_normalizer=tt.normalizers.MeanStd(), return_normalizer=return_normalizer)
    model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    return model


def test_quantile_value_head():
    import tonic_amd.torch as tt
    head = tt.models.QuantileValueHead()
    assert head.num_quantiles == 25 and head.fn is None and not hasattr(head, 'num_atoms')
    seen = []
    head = tt.models.QuantileValueHead(num_quantiles=7, fn=lambda layer: seen.append(layer))
    head.initialize(12)
    assert seen == [head.quantile_layer] and isinstance(head.quantile_layer, torch.nn.Linear)
    assert sorted(head.state_dict()) == ['quantile_layer.bias', 'quantile_layer.weight']
    assert head.quantile_layer.weight.shape == (7, 12) and head.quantile_layer.bias.shape == (7,)
    out = head(torch.zeros(3, 12))
    assert out.shape == (3, 7) and torch.equal(out, head.quantile_layer.bias.expand(3, 7))
    model = _model(tt.models.ActorTwinCriticWithTargets, tt.models.QuantileValueHead(7), O=5, A=2)
    values = model.critic_1(torch.zeros(4, 5), torch.zeros(4, 2))
    assert values.shape == (4, 7)
    assert [tuple(p.shape) for p in tt.models.network_variables(model.critic_2)] == \
        [(32, 7), (32,), (32, 32), (32,), (7, 32), (7,)]


def test_updaters_refuse_by_name():
    import tonic_amd.torch as tt
    twin, single = tt.models.ActorTwinCriticWithTargets, tt.models.ActorCriticWithTargets
    quantile = tt.models.QuantileValueHead
    critic, actor = tt.updaters.TruncatedQuantileQLearning, tt.updaters.TwinCriticQuantileSoftPolicyGradient
    u = critic()
    assert (u.entropy_coeff, u.top_quantiles_to_drop_per_net, u.gradient_clip, u.optimizer, u.lr_scheduler) == \
        (0.2, 2, 0, None, None)
    assert (u.stats_kind, u.stock_capable, u.head_family, u.default_lr) == (3, False, 'sac', 3e-4)
    u = actor()
    assert (u.entropy_coeff, u.gradient_clip, u.optimizer, u.lr_scheduler) == (0.2, 0, None, None)
    assert (u.stats_kind, u.stock_capable, u.head_family, u.default_lr) == (4, False, 'sac', 3e-4)
    for make in (critic, actor):
        name = make.__name__
        with pytest.raises(NotImplementedError, match=name + '.*twin critics'):
            make().initialize(_model(single, quantile(5)))
        with pytest.raises(NotImplementedError, match=name + '.*QuantileValueHead'):
            make().initialize(_model(twin, tt.models.ValueHead()))
        with pytest.raises(NotImplementedError, match=name + '.*QuantileValueHead'):
            make().initialize(_model(twin, tt.models.DistributionalValueHead(-10., 10., 21)))
        mixed = _model(twin, quantile(5))
        mixed.target_critic_2.head.num_quantiles = 6
        with pytest.raises(NotImplementedError, match=name + '.*same num_quantiles.*5, 5, 5, 6'):
            make().initialize(mixed)
        for M in (33, 64):
            with pytest.raises(NotImplementedError, match=f'{name}.*num_quantiles = 1 .. 32, got {M}'):
                make().initialize(_model(twin, quantile(M)))
        zero = _model(twin, quantile(3))
        for net in (zero.critic_1, zero.critic_2, zero.target_critic_1, zero.target_critic_2):
            net.head.num_quantiles = 0
        with pytest.raises(NotImplementedError, match=f'{name}.*num_quantiles = 1 .. 32, got 0'):
            make().initialize(zero)
        with pytest.raises(NotImplementedError, match='sac kernels serve GaussianPolicyHead.*DeterministicPolicyHead'):
            make().initialize(_model(twin, quantile(5), policy_head=tt.models.DeterministicPolicyHead()))
        with pytest.raises(NotImplementedError, match='sac kernels serve.*loc_activation'):
            make().initialize(_model(twin, quantile(5), policy_head=tt.models.GaussianPolicyHead()))
        with pytest.raises(NotImplementedError, match=name + '.*Return normaliser'):
            make().initialize(_model(twin, quantile(5), return_normalizer=tt.normalizers.Return(0.99)))
        with pytest.raises(NotImplementedError, match='torsos of 1 .. 4 layers'):
            make().initialize(_model(twin, quantile(5), sizes=(8, 8, 8, 8, 8)))
    for M, drop in ((5, 5), (5, -1), (1, 1), (25, 30), (5, 1.5)):
        with pytest.raises(NotImplementedError, match='TruncatedQuantileQLearning.*top_quantiles_to_drop_per_net = 0 '
                                                      f'.. num_quantiles - 1 = {M - 1}'):
            critic(top_quantiles_to_drop_per_net=drop).initialize(_model(twin, quantile(M)))


def test_other_updaters_refuse_a_quantile_head_by_name():
    """The scalar and categorical updaters name the head; before, such a critic failed on a parameter count."""
    import tonic_amd.torch as tt
    twin, single = tt.models.ActorTwinCriticWithTargets, tt.models.ActorCriticWithTargets
    u, deterministic, mpo = tt.updaters, tt.models.DeterministicPolicyHead, tt.models.GaussianPolicyHead
    cases = [(u.TwinCriticSoftQLearning, twin, None), (u.TwinCriticSoftDeterministicPolicyGradient, twin, None),
             (u.TwinCriticDeterministicQLearning, twin, deterministic), (u.DeterministicPolicyGradient, twin, deterministic),
             (u.DeterministicQLearning, single, deterministic), (u.QRegression, single, deterministic),
             (u.DistributionalDeterministicQLearning, single, deterministic),
             (u.DistributionalDeterministicPolicyGradient, single, deterministic),
             (u.TwinCriticDistributionalDeterministicQLearning, twin, deterministic),
             (u.ExpectedSARSA, single, mpo), (u.DistributionalExpectedSARSA, single, mpo),
             (u.MaximumAPosterioriPolicyOptimization, single, mpo)]
    for make, container, head in cases:
        model = _model(container, tt.models.QuantileValueHead(5), policy_head=head() if head else None)
        with pytest.raises(NotImplementedError, match='QuantileValueHead'):
            make().initialize(model)


def test_agent_defaults():
    import tonic_amd
    import tonic_amd.torch as tt
    agent = tt.agents.TQC()
    assert isinstance(agent, tt.agents.SAC) and agent.policy_kind == 1 and agent.entropy_coeff_updater is None
    model, sac = agent.model, tt.agents.SAC().model
    assert type(model) is tt.models.ActorTwinCriticWithTargets
    for critic in (model.critic_1, model.critic_2, model.target_critic_1, model.target_critic_2):
        assert type(critic.head) is tt.models.QuantileValueHead and critic.head.num_quantiles == 25
        assert (critic.torso.sizes, critic.torso.activation) == (sac.critic_1.torso.sizes, sac.critic_1.torso.activation)
        assert isinstance(critic.encoder, tt.models.ObservationActionEncoder)
    for actor in (model.actor, model.target_actor):
        assert type(actor.head) is tt.models.GaussianPolicyHead and actor.head.loc_activation is torch.nn.Identity
        assert actor.head.distribution is tt.models.SquashedMultivariateNormalDiag
        assert (actor.torso.sizes, actor.torso.activation) == (sac.actor.torso.sizes, sac.actor.torso.activation)
    assert isinstance(model.observation_normalizer, tt.normalizers.MeanStd) and model.return_normalizer is None
    assert type(agent.replay) is tonic_amd.replays.Buffer and agent.replay.return_steps == 1
    assert type(agent.exploration) is type(tt.agents.SAC().exploration)
    assert type(agent.actor_updater) is tt.updaters.TwinCriticQuantileSoftPolicyGradient
    assert type(agent.critic_updater) is tt.updaters.TruncatedQuantileQLearning
    assert type(agent.critic_updater) not in tt.agents.DDPG._FUSED and agent._actor_due(0) and agent._actor_due(1)
    given = tt.updaters.TruncatedQuantileQLearning(top_quantiles_to_drop_per_net=5)
    assert tt.agents.TQC(critic_updater=given).critic_updater is given
    tuner = tt.updaters.EntropyCoeffTuning()
    assert tt.agents.TQC(entropy_coeff_updater=tuner).entropy_coeff_updater is tuner


def test_agent_refusals():
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    spaces = Box(-np.inf, np.inf, (5,)), Box(-1, 1, (2,))
    agent = tt.agents.TQC(replay=tonic_amd.replays.PrioritizedBuffer())
    with pytest.raises(NotImplementedError, match='PrioritizedBuffer with the critic updater '
                                                  'TruncatedQuantileQLearning is not served.*\\(D4PG, TD4\\)'):
        agent.initialize(*spaces, seed=0)
    # a tuner goes with exactly the two quantile updaters; SAC's own check reads as it did
    agent = tt.agents.TQC(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning(),
                          critic_updater=tt.updaters.TwinCriticSoftQLearning())
    with pytest.raises(NotImplementedError, match='TQC\\(entropy_coeff_updater=...\\) with critic_updater='
                                                  'TwinCriticSoftQLearning.*TruncatedQuantileQLearning only'):
        agent.initialize(*spaces, seed=0)
    agent = tt.agents.TQC(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning(),
                          actor_updater=tt.updaters.TwinCriticSoftDeterministicPolicyGradient())
    with pytest.raises(NotImplementedError, match='with actor_updater=TwinCriticSoftDeterministicPolicyGradient.*'
                                                  'TwinCriticQuantileSoftPolicyGradient only'):
        agent.initialize(*spaces, seed=0)
    agent = tt.agents.SAC(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning(),
                          critic_updater=tt.updaters.TruncatedQuantileQLearning())
    with pytest.raises(NotImplementedError, match='SAC\\(entropy_coeff_updater=...\\) with critic_updater='
                                                  'TruncatedQuantileQLearning: a learned entropy coefficient is read '
                                                  'on the device by TwinCriticSoftQLearning only'):
        agent.initialize(*spaces, seed=0)
