"""REDQ without a GPU: what the two updaters refuse by name, the agent's defaults, the subset stream, the restatement
(tests/redq_ref.py) on rows computed by hand, and what the C entries answer before any HIP call."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import redq_ref
from test_offpolicy_entries_host import FAKE, INVALID, UNKNOWN_H, WORKSPACE, expect, torso_code
from test_tqc_ensemble_host import ensemble
from test_tqc_host import _model as _twin_style_model

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'tonic_ensemble_subset_q_grad'
ARGUMENTS = ('d_actor d_target_critics d_critics d_norm_mean d_norm_std norm_clip d_observations d_actions '
             'd_next_observations d_rewards d_discounts d_eps d_grad_sums B O H A N d_subset entropy_coeff '
             'd_log_entropy_coeff loss d_workspace workspace_bytes stream').split()
DEFAULTS = dict(norm_clip=5.0, B=17, O=17, H=64, A=6, N=5, entropy_coeff=0.2, d_log_entropy_coeff=None, loss=None,
                stream=None, workspace_bytes=None)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def query(lib, v):
    return lib.tonic_ensemble_q_workspace_bytes(v['B'], v['O'], v['A'], v['H'], v['N'])


def call(lib, **changes):
    values = dict(DEFAULTS, **changes)
    if values['workspace_bytes'] is None:
        values['workspace_bytes'] = query(lib, values)
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ARGUMENTS]
    return getattr(lib, ENTRY)(*args), lib.tonic_last_error()


_RULES = []


def rule(kind, param=0.0):
    """A tonic_critic_loss_t that outlives the call its address goes to."""
    from tonic_amd import _lib
    _RULES.append(_lib.CriticLoss(kind=kind, param=param))
    return _RULES[-1]


# ---------------------------------------------------------------- 1. the updaters

def test_updaters_defaults():
    import tonic_amd.torch as tt
    u = tt.updaters.EnsembleSoftQLearning()
    assert (u.loss, u.optimizer, u.entropy_coeff, u.subset_size, u.gradient_clip, u.lr_scheduler) == \
        (None, None, 0.2, 2, 0, None)
    assert (u.stats_kind, u.stock_capable, u.head_family, u.default_lr, u.loss_rule.kind) == (3, False, 'sac', 3e-4, 0)
    u = tt.updaters.EnsembleSoftPolicyGradient()
    assert (u.optimizer, u.entropy_coeff, u.gradient_clip, u.lr_scheduler) == (None, 0.2, 0, None)
    assert (u.stats_kind, u.stock_capable, u.head_family, u.default_lr) == (4, False, 'sac', 3e-4)
    huber = tt.updaters.EnsembleSoftQLearning(loss=torch.nn.HuberLoss(delta=0.5))
    assert (huber.loss_rule.kind, huber.loss_rule.param) == (3, 0.5)


def test_updaters_refuse_by_name():
    import tonic_amd.torch as tt
    value, models = tt.models.ValueHead, tt.models
    for make in (tt.updaters.EnsembleSoftQLearning, tt.updaters.EnsembleSoftPolicyGradient):
        name = make.__name__
        for container in (models.ActorTwinCriticWithTargets, models.ActorCriticWithTargets):
            with pytest.raises(NotImplementedError, match=f'{name} needs an ensemble.*ActorCriticEnsembleWithTargets.*'
                                                          f'{container.__name__}'):
                make().initialize(_twin_style_model(container, value()))
        with pytest.raises(NotImplementedError, match=name + '.*ValueHead.*all 6.*QuantileValueHead'):
            make().initialize(ensemble(models.QuantileValueHead(5), 3))
        with pytest.raises(NotImplementedError, match=name + '.*ValueHead.*DistributionalValueHead'):
            make().initialize(ensemble(models.DistributionalValueHead(-10., 10., 21), 3))
        mixed = ensemble(value(), 3)
        mixed.target_critic_3.head = models.QuantileValueHead(1)              # (one of the six is enough)
        with pytest.raises(NotImplementedError, match=name + ".*'ValueHead', 'QuantileValueHead'\\]"):
            make().initialize(mixed)
        with pytest.raises(NotImplementedError, match=name + '.*Return normaliser.*Return'):
            make().initialize(ensemble(value(), 3, return_normalizer=tt.normalizers.Return(0.99)))
        with pytest.raises(NotImplementedError, match=name + '.*torso.*1 .. 4 layers.*\\(8, 8, 8, 8, 8\\)'):
            make().initialize(ensemble(value(), 3, sizes=(8, 8, 8, 8, 8)))
        with pytest.raises(NotImplementedError, match='sac kernels serve GaussianPolicyHead.*DeterministicPolicyHead'):
            make().initialize(ensemble(value(), 3, policy_head=models.DeterministicPolicyHead()))
    name = 'EnsembleSoftQLearning'
    for bad in (0, 4, -1, 1.5, None, '2', True):
        with pytest.raises(NotImplementedError, match=f'{name}: subset_size is a whole number in 1 .. num_critics = 3, '
                                                      f'got {bad!r}'):
            tt.updaters.EnsembleSoftQLearning(subset_size=bad).initialize(ensemble(value(), 3))

    class Own(torch.nn.MSELoss):
        pass
    for bad, told in ((torch.nn.BCELoss(), 'BCELoss'), (Own(), 'Own'), (torch.nn.MSELoss(reduction='sum'), "'sum'"),
                      (lambda a, b: 0, 'lambda'), (torch.nn.HuberLoss(delta=float('inf')), 'not finite')):
        with pytest.raises(NotImplementedError, match=f'{name}: .*{told}'):
            tt.updaters.EnsembleSoftQLearning(loss=bad).initialize(ensemble(value(), 3))
    late = tt.updaters.EnsembleSoftQLearning()
    late._loss = torch.nn.BCELoss()                       # (past the setter: `initialize` looks again)
    with pytest.raises(NotImplementedError, match=f'{name}: .*BCELoss'):
        late.initialize(ensemble(value(), 3))


def test_the_other_updaters_message_is_as_it_was():
    import tonic_amd.torch as tt
    with pytest.raises(NotImplementedError, match='TwinCriticSoftQLearning does not serve a '
                                                  'ActorCriticEnsembleWithTargets of 3 critics.*'
                                                  'TruncatedQuantileQLearning and TwinCriticQuantileSoftPolicyGradient'):
        tt.updaters.TwinCriticSoftQLearning().initialize(ensemble(tt.models.ValueHead(), 3))
    for make in (tt.updaters.TruncatedQuantileQLearning, tt.updaters.TwinCriticQuantileSoftPolicyGradient):
        with pytest.raises(NotImplementedError, match=make.__name__ + '.*QuantileValueHead'):
            make().initialize(ensemble(tt.models.ValueHead(), 3))


# ---------------------------------------------------------------- 2. the agent

def test_agent_defaults():
    import tonic_amd
    import tonic_amd.torch as tt
    agent = tt.agents.REDQ()
    assert isinstance(agent, tt.agents.SAC) and agent.policy_kind == 1 and agent.entropy_coeff_updater is None
    model, sac = agent.model, tt.agents.SAC().model
    assert type(model) is tt.models.ActorCriticEnsembleWithTargets and model.num_critics == 5
    assert model.target_coeff == sac.target_coeff
    for critic in model.critics() + model.critics(target=True):
        assert type(critic.head) is tt.models.ValueHead
        assert (critic.torso.sizes, critic.torso.activation) == (sac.critic_1.torso.sizes, sac.critic_1.torso.activation)
        assert isinstance(critic.encoder, tt.models.ObservationActionEncoder)
    for actor in (model.actor, model.target_actor):
        assert type(actor.head) is tt.models.GaussianPolicyHead and actor.head.loc_activation is torch.nn.Identity
        assert actor.head.distribution is tt.models.SquashedMultivariateNormalDiag
        assert (actor.torso.sizes, actor.torso.activation) == (sac.actor.torso.sizes, sac.actor.torso.activation)
    assert isinstance(model.observation_normalizer, tt.normalizers.MeanStd) and model.return_normalizer is None
    replay = agent.replay
    assert type(replay) is tonic_amd.replays.Buffer
    assert (replay.batch_size, replay.batch_iterations, replay.steps_between_batches, replay.return_steps) == \
        (256, 20, 1, 1)                                                           # an update-to-data ratio of 20
    assert type(agent.exploration) is type(tt.agents.SAC().exploration)
    assert type(agent.actor_updater) is tt.updaters.EnsembleSoftPolicyGradient
    assert type(agent.critic_updater) is tt.updaters.EnsembleSoftQLearning and agent.critic_updater.subset_size == 2
    assert agent._TEMPERED == (tt.updaters.EnsembleSoftQLearning, tt.updaters.EnsembleSoftPolicyGradient)
    assert type(agent.critic_updater) not in tt.agents.DDPG._FUSED and agent._actor_due(0) and agent._actor_due(1)
    assert tt.agents.REDQ.enqueue_update is tt.agents.DDPG.enqueue_update          # chunking's condition
    assert tt.agents.REDQ._update is tt.agents.DDPG._update
    given = tt.updaters.EnsembleSoftQLearning(subset_size=3)
    assert tt.agents.REDQ(critic_updater=given).critic_updater is given
    tuner = tt.updaters.EntropyCoeffTuning()
    assert tt.agents.REDQ(entropy_coeff_updater=tuner).entropy_coeff_updater is tuner
    assert tt.agents.SAC()._draw_subsets(4) is None and tt.agents.TQC()._draw_subsets(4) is None


def test_agent_refusals():
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    spaces = Box(-np.inf, np.inf, (5,)), Box(-1, 1, (2,))
    agent = tt.agents.REDQ(replay=tonic_amd.replays.PrioritizedBuffer())
    with pytest.raises(NotImplementedError, match='PrioritizedBuffer with the critic updater '
                                                  'EnsembleSoftQLearning is not served.*\\(D4PG, TD4\\)'):
        agent.initialize(*spaces, seed=0)
    agent = tt.agents.REDQ(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning(),
                           critic_updater=tt.updaters.TwinCriticSoftQLearning())
    with pytest.raises(NotImplementedError, match='REDQ\\(entropy_coeff_updater=...\\) with critic_updater='
                                                  'TwinCriticSoftQLearning.*EnsembleSoftQLearning only'):
        agent.initialize(*spaces, seed=0)
    agent = tt.agents.REDQ(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning(),
                           actor_updater=tt.updaters.TwinCriticQuantileSoftPolicyGradient())
    with pytest.raises(NotImplementedError, match='with actor_updater=TwinCriticQuantileSoftPolicyGradient.*'
                                                  'EnsembleSoftPolicyGradient only'):
        agent.initialize(*spaces, seed=0)


# ---------------------------------------------------------------- 3. the subset stream

def popcount(mask):
    return bin(int(mask)).count('1')


def test_subset_stream_is_seeded_uniform_and_chunk_proof():
    import tonic_amd.torch as tt
    torch_state, numpy_state = torch.get_rng_state(), np.random.get_state()[1].copy()
    agent = tt.agents.REDQ()
    agent._seed_subsets(7)
    masks = agent._draw_subsets(2000)
    assert masks.dtype == np.int32 and masks.shape == (2000,)
    assert all(popcount(m) == 2 and 0 < m < 32 for m in masks)                    # exactly |S| of the low N bits
    pairs = {redq_ref.mask_of(pair) for pair in itertools.combinations(range(5), 2)}
    assert len(pairs) == 10 and set(masks.tolist()) == pairs                      # all 10 pairs occur
    counts = np.array([np.sum(masks == pair) for pair in sorted(pairs)])
    assert counts.min() > 140 and counts.max() < 260, counts                      # 200 +- 4.5 sigma of a uniform draw
    # seeded and reproducible; another seed, another stream
    again = tt.agents.REDQ()
    again._seed_subsets(7)
    assert np.array_equal(again._draw_subsets(2000), masks)
    other = tt.agents.REDQ()
    other._seed_subsets(8)
    assert not np.array_equal(other._draw_subsets(2000), masks)
    # one call of 40 or four of 10: the same stream
    whole, parts = tt.agents.REDQ(), tt.agents.REDQ()
    whole._seed_subsets(3)
    parts._seed_subsets(3)
    assert np.array_equal(whole._draw_subsets(40), np.concatenate([parts._draw_subsets(10) for _ in range(4)]))
    # a generator of the agent's own: neither torch's global stream nor numpy's moved
    assert torch.equal(torch.get_rng_state(), torch_state) and np.array_equal(np.random.get_state()[1], numpy_state)
    # every size of subset
    for N, size in ((2, 1), (3, 1), (3, 2), (8, 7), (8, 1)):
        drawn = tt.updaters.draw_subset_masks(np.random.RandomState(N), 300, N, size)
        assert all(popcount(m) == size and 0 < m < (1 << N) for m in drawn)
        assert {z for m in drawn for z in redq_ref.subset_of(m, N)} == set(range(N))


def test_the_whole_ensemble_consumes_no_draw():
    import tonic_amd.torch as tt
    agent = tt.agents.REDQ(critic_updater=tt.updaters.EnsembleSoftQLearning(subset_size=5))
    agent._seed_subsets(7)
    before = agent._subset_generator.get_state()[1].copy()
    masks = agent._draw_subsets(50)
    assert masks.dtype == np.int32 and (masks == 31).all()
    assert np.array_equal(agent._subset_generator.get_state()[1], before)
    assert (tt.updaters.draw_subset_masks(None, 3, 8, 8) == 255).all()           # (no generator is asked)


# ---------------------------------------------------------------- 4. the restatement, by hand

def test_restatement_on_rows_computed_by_hand():
    one = lambda *v: torch.tensor(list(v), dtype=torch.float64)                    # noqa: E731
    nan, inf = float('nan'), float('inf')
    assert redq_ref.subset_of(0b00110, 5) == [1, 2] and redq_ref.subset_of(0, 3) == [0, 1, 2]
    assert redq_ref.subset_of(0b11000, 3) == [0, 1, 2] and redq_ref.subset_of(0b11101, 3) == [0, 2]
    assert redq_ref.mask_of([0, 4]) == 17
    targets = [one(3, 1, nan, 2), one(2, 5, 1, inf), one(0, 4, 0, nan)]
    low, who = redq_ref.subset_min(targets, [0, 1])
    assert low[:2].tolist() == [2, 1] and torch.isnan(low[2]) and low[3] == 2     # a NaN inside S stays, inf loses
    assert who.tolist() == [1, 0, -1, 0]
    low, _ = redq_ref.subset_min(targets, [1, 2])
    assert low[:3].tolist() == [0, 4, 0] and torch.isnan(low[3])                  # (row 2's NaN is outside this S)
    # r = 0.5, disc = 0.5, alpha logp' = 1, S = {0, 1}: y = 0.5 + 0.5 (min - 1) = {1, 0.5}
    t2 = [t[:2] for t in targets]
    y = redq_ref.td_target(t2, one(0.5, 0.5), one(0.5, 0.5), one(2, 2), 0.5, [0, 1])
    assert y.tolist() == [1.0, 0.5]
    qs = [one(2, 0.5), one(1, 0.75), one(-2, 0.25)]                               # errors {1, 0, -3}, {0, 0.25, -0.25}
    loss, grads, q = redq_ref.critic_rows_with_gradients(t2, qs, one(0.5, 0.5), one(0.5, 0.5), one(2, 2), 0.5, [0, 1])
    assert loss.tolist() == [1 + 0 + 9, 0 + 0.0625 + 0.0625]
    assert [g.tolist() for g in grads] == [[2, 0], [0, 0.5], [-6, -0.5]]
    assert q.tolist() == [1 / 3, 0.5]
    huber = redq_ref.critic_rows_with_gradients(t2, qs, one(0.5, 0.5), one(0.5, 0.5), one(2, 2), 0.5, [0, 1],
                                                redq_ref.HUBER, 1.0)
    assert huber[0].tolist() == [0.5 + 0 + 2.5, 0 + 0.03125 + 0.03125]
    assert [g.tolist() for g in huber[1]] == [[1, 0], [0, 0.25], [-1, -0.25]]      # (e = delta: the linear branch)
    for kind, param in ((0, 0.0), (1, 0.0), (2, 0.5), (2, 0.0), (3, 0.7)):
        leaves = [q.clone().requires_grad_() for q in qs]
        redq_ref.critic_rows(t2, leaves, one(0.5, 0.5), one(0.5, 0.5), one(2, 2), 0.5, [0, 1], kind, param).sum().backward()
        closed = redq_ref.critic_rows_with_gradients(t2, qs, one(0.5, 0.5), one(0.5, 0.5), one(2, 2), 0.5, [0, 1], kind,
                                                     param)[1]
        for leaf, want in zip(leaves, closed):
            assert torch.equal(leaf.grad, want), (kind, param)
    functional = torch.nn.functional
    e, zero = torch.linspace(-2, 2, 41, dtype=torch.float64), torch.zeros(41, dtype=torch.float64)
    assert torch.equal(redq_ref.loss_terms(e, 3, 0.7), functional.huber_loss(e, zero, reduction='none', delta=0.7))
    assert torch.equal(redq_ref.loss_terms(e, 2, 0.5), functional.smooth_l1_loss(e, zero, reduction='none', beta=0.5))
    assert torch.equal(redq_ref.loss_terms(e, 1, 0.0), functional.l1_loss(e, zero, reduction='none'))
    assert redq_ref.actor_rows(qs, one(2, 2), 0.5).tolist() == [1 - 1 / 3, 0.5]


# ---------------------------------------------------------------- 5. the C interface

def test_symbols_are_in_the_table_and_the_headers(lib):
    import re
    from tonic_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tonic_hip.h')).read()
    dev = open(os.path.join(ROOT, 'include', 'tonic_hip_dev.h')).read()
    counts = {'tonic_ensemble_q_workspace_bytes': (header, 5), ENTRY: (header, len(ARGUMENTS)),
              'tonic_debug_ensemble_subset_loss': (dev, 16)}
    for symbol, (text, count) in counts.items():
        assert symbol in _lib.SIGNATURES and getattr(lib, symbol) is not None
        found = re.findall(r'\b%s\s*\(([^;{}()]*)\)\s*;' % symbol, text)
        assert len(found) == 1, symbol
        assert found[0].count(',') + 1 == count == len(_lib.SIGNATURES[symbol][1]), symbol
    assert 'tonic_debug_ensemble_subset_loss' not in header
    assert lib.tonic_abi_version() == 22 == _lib.ABI_VERSION                     # additive


def test_critic_entry_answers_before_any_gpu_work(lib):
    """Every failure has its own message with the numbers, and the call returns before a launch: every pointer is a
    fake address nobody reads (the method of tests/test_offpolicy_entries_host.py)."""
    name = ENTRY.encode()
    for pointer in (p for p in ARGUMENTS if p.startswith('d_') and p != 'd_log_entropy_coeff'):
        expect(call(lib, **{pointer: None}), INVALID, name + b': a NULL pointer')
        expect(call(lib, **{pointer: None}, workspace_bytes=16), INVALID, name + b': a NULL pointer')
    for B in (0, -1):
        expect(call(lib, B=B, workspace_bytes=1 << 40), INVALID, b'B %d' % B)
    for O, A in ((0, 6), (17, 0), (-1, 6)):
        expect(call(lib, O=O, A=A, workspace_bytes=1 << 40), INVALID, b'O %d, A %d (each >= 1)' % (O, A))
    for code in UNKNOWN_H:
        expect(call(lib, H=code, workspace_bytes=1 << 40), INVALID, b'H %d is not a torso' % code)
    for N in (1, 0, -2, 9, 64):
        expect(call(lib, N=N, workspace_bytes=1 << 40), INVALID, name + b': %d critics (2 <= N <= 8)' % N)
    for kind in (-1, 4, 99):
        expect(call(lib, loss=ctypes.addressof(rule(kind))), INVALID, b'unknown kind %d' % kind)
    for kind, param, told in ((3, float('nan'), b'delta'), (3, float('inf'), b'delta'), (2, float('nan'), b'beta'),
                              (2, -float('inf'), b'beta')):
        expect(call(lib, loss=ctypes.addressof(rule(kind, param))), INVALID, told + b' = ')
    expect(call(lib, loss=ctypes.addressof(rule(3, 0.0))), INVALID, b'Huber needs delta > 0')
    expect(call(lib, loss=ctypes.addressof(rule(2, -1.0))), INVALID, b'smooth-L1 needs beta >= 0')
    # what is served reaches the workspace check: every rule, the coefficient's pointer, every N
    for served in (None, rule(0), rule(1), rule(2, 0.0), rule(2, 0.5), rule(3, 1.0)):
        loss = None if served is None else ctypes.addressof(served)
        expect(call(lib, loss=loss, workspace_bytes=16), WORKSPACE,
               name + b': workspace of 16 bytes, %d needed' % query(lib, DEFAULTS))
    expect(call(lib, d_log_entropy_coeff=FAKE, workspace_bytes=16), WORKSPACE)
    for H in (64, 256, torso_code(lib, 'relu32x3')):
        for B, N in ((1, 2), (17, 5), (37, 8)):
            need = query(lib, dict(DEFAULTS, B=B, H=H, N=N))
            expect(call(lib, B=B, H=H, N=N, workspace_bytes=need - 1), WORKSPACE,
                   name + b': workspace of %d bytes, %d needed' % (need - 1, need))


def test_queries(lib):
    """A function of its arguments alone: the quantile layout at M = 1; 0 outside 2 .. 8; growing with N."""
    for H in (64, 256, torso_code(lib, 'relu32x3')):
        sizes = [lib.tonic_ensemble_q_workspace_bytes(37, 17, 6, H, N) for N in range(2, 9)]
        assert all(b > a > 0 for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes == [lib.tonic_ensemble_quantile_workspace_bytes(37, 17, 6, H, 1, N) for N in range(2, 9)]
    for N in (1, 9, 0, -1):
        assert lib.tonic_ensemble_q_workspace_bytes(37, 17, 6, 64, N) == 0
    want, saved = lib.tonic_ensemble_q_workspace_bytes(256, 17, 6, 256, 5), {}
    try:
        for name in ('q_images', 'policy_tail', 'q_chain'):
            value = ctypes.c_int32(0)
            assert lib.tonic_get_tuning(name.encode(), ctypes.addressof(value)) == 0, name
            saved[name] = value.value
            assert lib.tonic_set_tuning(name.encode(), 0) == 0, name
        assert lib.tonic_ensemble_q_workspace_bytes(256, 17, 6, 256, 5) == want
    finally:
        for name, value in saved.items():
            lib.tonic_set_tuning(name.encode(), value)


def test_loss_kernel_entry_refuses_before_a_launch(lib):
    entry = lib.tonic_debug_ensemble_subset_loss

    def run(ld=16, N=5, B=5, Bp=16, loss=None, **null):
        p = lambda name: None if name in null else FAKE                    # noqa: E731
        status = entry(p('t'), p('q'), ld, p('r'), p('d'), p('logp'), N, p('subset'), 0.2, None, loss, p('dq'),
                       p('sample_m'), B, Bp, None)
        return status, lib.tonic_last_error()
    for name in ('t', 'q', 'r', 'd', 'logp', 'subset', 'dq', 'sample_m'):
        expect(run(**{name: True}), INVALID, b'tonic_debug_ensemble_subset_loss: a NULL pointer')
    for N in (1, 9, 0, 33):
        expect(run(N=N), INVALID, b'%d critics (2 <= N <= 8)' % N)
    for bad in (dict(ld=0), dict(ld=33), dict(B=0), dict(B=17, Bp=16)):
        expect(run(**bad), INVALID, b'1 <= ld <= 32, 0 < B <= Bp')
    expect(run(loss=ctypes.addressof(rule(7))), INVALID, b'unknown kind 7')
    expect(run(loss=ctypes.addressof(rule(3, float('nan')))), INVALID, b'delta')
