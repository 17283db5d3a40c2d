"""TD4 without a GPU: the tests' restatement (tests/td4_ref.py) against the unmodified reference where the two
meet, what tonic_twin_distributional_q_grad answers before any HIP call, what the updater refuses, and the agent's
defaults."""
import math
import os
import sys

import numpy as np
import pytest

import td4_ref
from test_offpolicy_entries_host import FAKE, INVALID, UNKNOWN_H, WORKSPACE, expect, torso_code

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'tonic_twin_distributional_q_grad'
ARGUMENTS = ('d_target_actor d_target_critics d_critics d_norm_mean d_norm_std norm_clip d_observations d_actions '
             'd_next_observations d_rewards d_discounts d_eps d_values d_grad_sums B O H A NA noise_scale noise_clip '
             'd_workspace workspace_bytes stream').split()
DEFAULTS = dict(norm_clip=5.0, B=17, O=17, H=64, A=6, NA=51, noise_scale=0.2, noise_clip=0.5, stream=None,
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


# ---------------------------------------------------------------- 1. the restatement

@needs_reference
def test_restatement_with_identical_twins_is_the_reference_d4pg_step():
    """critic_2 := critic_1, target_critic_2 := target_critic_1 and noise scale 0 make TD4's critic step two copies
    of D4PG's: against DistributionalDeterministicQLearning.__call__ of the unmodified reference (critics.py:100-122),
    both in float64 on the CPU, the loss is exactly twice the reference's and each critic's gradient equals the
    reference's to 1e-12.  The support is integers 1 apart, so that the reference's float32 support and its float64
    copy space the atoms by the same numbers."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import reference_loader as rl
    tonic = rl.load_reference()
    models, updaters = tonic.torch.models, tonic.torch.updaters
    O, A, B, sizes = 7, 3, 13, (16, 12)
    torch.manual_seed(5)
    model = models.ActorCriticWithTargets(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, torch.nn.ReLU),
                           head=models.DeterministicPolicyHead()),
        critic=models.Critic(encoder=models.ObservationActionEncoder(), torso=models.MLP(sizes, torch.nn.ReLU),
                             head=models.DistributionalValueHead(-5., 5., 11)),
        observation_normalizer=tonic.torch.normalizers.MeanStd())
    model.initialize(rl.SyntheticSpace(-np.inf, np.inf, (O,)), rl.SyntheticSpace(-1, 1, (A,)))
    updater = updaters.DistributionalDeterministicQLearning()
    updater.initialize(model)
    rng = np.random.RandomState(2)
    model.observation_normalizer.record(rng.normal(size=(30, O)).astype(np.float32) * 2 + 0.5)
    model.observation_normalizer.update()
    model.double()
    with torch.no_grad():
        for net in (model.target_actor, model.target_critic):       # the targets away from the online networks
            for p in td4_ref.weights(net):
                p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.3)
    assert np.array_equal(model.critic.head.values.numpy(), np.arange(-5.0, 6.0))
    batch = dict(observations=rng.normal(size=(B, O)), actions=rng.uniform(-1, 1, (B, A)),
                 next_observations=rng.normal(size=(B, O)), rewards=rng.normal(size=B) * 3,
                 discounts=0.99 * (rng.uniform(size=B) > 0.2))
    batch = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in batch.items()}
    twin = dict(actor=model.actor, critic_1=model.critic, critic_2=model.critic, target_actor=model.target_actor,
                target_critic_1=model.target_critic, target_critic_2=model.target_critic)
    nets = td4_ref.Networks(twin, model.observation_normalizer, model.critic.head.values, len(sizes))
    out = td4_ref.critic_step(nets, batch, torch.randn(B, A), 0.0, 0.5)
    assert not out['second'].any()                                   # equal means: the first critic
    infos = updater(**batch)                                         # (steps the optimizer: the gradients stay)
    assert float(out['loss']) == 2 * float(infos['loss'])
    for name in ('critic_1', 'critic_2'):
        for i, (leaf, p) in enumerate(zip(nets.params[name], td4_ref.weights(model.critic))):
            want = p.grad.numpy()
            np.testing.assert_allclose(leaf.grad.numpy(), want, rtol=0, atol=1e-12 * max(np.abs(want).max(), 1e-30),
                                       err_msg=f'{name} {i}')


def test_selection_rule_on_hand_made_logits():
    """mu_2 < mu_1 selects critic 2, mu_2 > mu_1 and an exact tie critic 1, a NaN mean critic 1: the targets are the
    projection of exactly that critic's distribution."""
    values = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)
    logits_1 = torch.tensor([[0.0, 0.0, 2.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    logits_2 = torch.tensor([[2.0, 0.0, 0.0], [0.0, 0.0, 2.0], [1.0, 0.0, 1.0], [math.nan, 0.0, 0.0]],
                            dtype=torch.float64)
    returns = torch.tensor([0.3, -0.2, 0.0, 0.5], dtype=torch.float64)[:, None] + 0.9 * values[None]
    targets, second, mu_1, mu_2 = td4_ref.select_targets(values, logits_1, logits_2, returns)
    assert mu_2[0] < mu_1[0] and mu_2[1] > mu_1[1] and mu_2[2] == mu_1[2] and torch.isnan(mu_2[3])
    assert second.tolist() == [True, False, False, False]
    want_1 = td4_ref.categorical(values, logits_1).project(returns)
    want_2 = td4_ref.categorical(values, logits_2).project(returns)
    assert not torch.equal(want_1[2], want_2[2])                     # (the tie's two candidates differ)
    assert torch.equal(targets[0], want_2[0])
    for row in (1, 2, 3):
        assert torch.equal(targets[row], want_1[row]), row


# ---------------------------------------------------------------- 2. the entry's statuses

def call(lib, **changes):
    values = dict(DEFAULTS, **changes)
    if values['workspace_bytes'] is None:
        values['workspace_bytes'] = lib.tonic_twin_distributional_workspace_bytes(
            values['B'], values['O'], values['A'], values['H'], values['NA'])
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ARGUMENTS]
    return getattr(lib, ENTRY)(*args), lib.tonic_last_error()


def test_entry_answers_before_any_gpu_work(lib):
    """Every pointer NULL in turn, B <= 0, atoms outside 2 .. 64, unknown torso codes, negative or non-finite noise
    parameters: -1 with a message that names the entry, also when the workspace is too small as well; a 16-byte
    workspace and one a byte short: -4.  Every pointer is a fake address nobody reads: each call returns before a
    launch (the method of tests/test_offpolicy_entries_host.py)."""
    from tonic_amd import _lib
    assert len(ARGUMENTS) == len(_lib.SIGNATURES[ENTRY][1])
    bad = (ENTRY + ': bad argument').encode()
    for pointer in (name for name in ARGUMENTS if name.startswith('d_')):
        expect(call(lib, **{pointer: None}), INVALID, bad)
        expect(call(lib, **{pointer: None}, workspace_bytes=16), INVALID, bad)
    for B in (0, -1):
        expect(call(lib, B=B), INVALID, bad)
    for NA in (1, 65):
        expect(call(lib, NA=NA, workspace_bytes=16), INVALID, bad)
    for code in UNKNOWN_H:
        expect(call(lib, H=code, workspace_bytes=1 << 40), INVALID, bad)
    for noise in (dict(noise_clip=-0.5), dict(noise_scale=-0.2), dict(noise_clip=math.nan),
                  dict(noise_scale=math.inf)):
        expect(call(lib, **noise), INVALID, (ENTRY + ': noise scale').encode())
        expect(call(lib, **noise, workspace_bytes=16), INVALID, (ENTRY + ': noise scale').encode())
    expect(call(lib, noise_scale=0.0, noise_clip=0.0, workspace_bytes=16), WORKSPACE)    # (zero noise is served)
    small = (ENTRY + ': workspace too small').encode()
    expect(call(lib, workspace_bytes=16), WORKSPACE, small)
    for H in (64, 256, lib.tonic_mlp_hidden(40, 24, 2), torso_code(lib, 'relu32x3'), torso_code(lib, 'one256')):
        for B, NA in ((1, 2), (17, 51), (37, 64)):
            need = lib.tonic_twin_distributional_workspace_bytes(B, 17, 6, H, NA)
            assert need > 0 and need >= lib.tonic_distributional_workspace_bytes(B, 17, 6, H, NA)
            expect(call(lib, B=B, H=H, NA=NA, workspace_bytes=need - 1), WORKSPACE, small)


# ---------------------------------------------------------------- 3. the updater and the agent

def _model(container, head, O=5, A=2):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP((32, 32), torch.nn.ReLU),
                              head=tt.models.DeterministicPolicyHead()),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(),
                                torso=tt.models.MLP((32, 32), torch.nn.ReLU), head=head),
        observation_normalizer=tt.normalizers.MeanStd())
    model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    return model


def test_updater_refuses_by_name():
    import tonic_amd.torch as tt
    name = 'TwinCriticDistributionalDeterministicQLearning'
    updater = getattr(tt.updaters, name)()
    assert (updater.stats_kind, updater.stock_capable) == (3, False)
    assert (updater.target_action_noise.scale, updater.target_action_noise.clip) == (0.2, 0.5)
    single = _model(tt.models.ActorCriticWithTargets, tt.models.DistributionalValueHead(-10., 10., 21))
    with pytest.raises(NotImplementedError, match=name + '.*twin critics'):
        updater.initialize(single)
    plain = _model(tt.models.ActorTwinCriticWithTargets, tt.models.ValueHead())
    with pytest.raises(NotImplementedError, match=name + '.*DistributionalValueHead'):
        updater.initialize(plain)
    uneven = _model(tt.models.ActorTwinCriticWithTargets, tt.models.DistributionalValueHead(-10., 10., 21))
    uneven.target_critic_2.head.values = uneven.target_critic_2.head.values * 0.5
    with pytest.raises(NotImplementedError, match=name + '.*same support'):
        updater.initialize(uneven)
    fewer = _model(tt.models.ActorTwinCriticWithTargets, tt.models.DistributionalValueHead(-10., 10., 21))
    fewer.critic_2.head.values = fewer.critic_2.head.values[:20]
    with pytest.raises(NotImplementedError, match=name + '.*same support'):
        updater.initialize(fewer)


def test_agent_defaults():
    """The defaults of the library's td4.py: the twin model with DistributionalValueHead(-150, 150, 51) on
    (256, 256) ReLU torsos and a MeanStd normaliser, 5-step returns, the distributional actor step, the new critic
    step, delay_steps = 2; TD3's schedule and `critic` alias; a Return normaliser is refused by the head."""
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    agent = tt.agents.TD4()
    assert isinstance(agent, tt.agents.TD3) and agent.delay_steps == 2
    model = agent.model
    assert type(model) is tt.models.ActorTwinCriticWithTargets and model.critic is model.critic_1
    for critic in (model.critic_1, model.critic_2, model.target_critic_1, model.target_critic_2):
        assert isinstance(critic.head, tt.models.DistributionalValueHead) and critic.head.num_atoms == 51
        assert torch.equal(critic.head.values, torch.linspace(-150., 150., 51))
        assert critic.torso.sizes == (256, 256) and critic.torso.activation is torch.nn.ReLU
    assert isinstance(model.actor.head, tt.models.DeterministicPolicyHead)
    assert model.actor.torso.sizes == (256, 256) and model.actor.torso.activation is torch.nn.ReLU
    assert isinstance(model.observation_normalizer, tt.normalizers.MeanStd) and model.return_normalizer is None
    assert agent.replay.return_steps == 5
    assert type(agent.actor_updater) is tt.updaters.DistributionalDeterministicPolicyGradient
    assert type(agent.critic_updater) is tt.updaters.TwinCriticDistributionalDeterministicQLearning
    assert [agent._actor_due(it) for it in range(4)] == [False, True, False, True]
    assert tt.agents.TD4(delay_steps=3).delay_steps == 3
    assert tt.agents.TD4(replay=tonic_amd.replays.Buffer(return_steps=1)).replay.return_steps == 1
    ranged = tt.agents.TD4().model
    ranged.return_normalizer = tt.normalizers.Return(0.99)
    with pytest.raises(ValueError, match='distributional value heads'):
        ranged.initialize(Box(-np.inf, np.inf, (5,)), Box(-1, 1, (2,)))
