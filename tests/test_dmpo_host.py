"""DMPO without a GPU: the tests' restatement (tests/dmpo_ref.py) pinned where it meets TD4's / D4PG's, what the
tonic_distributional_mpo_* entries answer before any HIP call, what the updaters and the agent refuse, and the
agent's defaults."""
import ctypes
import itertools

import numpy as np
import pytest

import dmpo_ref
import td4_ref
from test_offpolicy_entries_host import FAKE, INVALID, SHAPES, TORSOS, UNKNOWN_H, WORKSPACE, expect, torso_code

torch = pytest.importorskip('torch')

_NETWORKS = 'd_norm_mean d_norm_std norm_clip'
_TAIL = ' d_workspace workspace_bytes stream'
ENTRIES = {
    'tonic_distributional_expected_sarsa_grad':
        'd_target_actor d_target_critic d_critic ' + _NETWORKS + ' d_observations d_actions d_next_observations '
        'd_rewards d_discounts d_eps d_values d_grad_sums B O H A S NA' + _TAIL,
    'tonic_distributional_mpo_actor_grad':
        'd_actor_params d_target_actor d_target_critic d_duals min_log_dual ' + _NETWORKS + ' d_observations d_eps '
        'd_values d_grad_sums d_dual_grads d_stats B O H A S NA epsilon epsilon_penalty epsilon_mean epsilon_std '
        'action_penalization joint_kl' + _TAIL,
    'tonic_distributional_mpo_actor_grad_shard':
        'd_actor_params d_target_actor d_target_critic d_duals min_log_dual ' + _NETWORKS + ' d_observations d_eps '
        'd_values d_grad_sums d_column_sums B O H A S NA action_penalization joint_kl' + _TAIL,
}
ENTRIES = {name: spec.split() for name, spec in ENTRIES.items()}
DEFAULTS = dict(norm_clip=5.0, B=17, O=17, H=64, A=6, S=20, NA=51, min_log_dual=-18.0, epsilon=0.1,
                epsilon_penalty=1e-3, epsilon_mean=1e-3, epsilon_std=1e-6, action_penalization=1, joint_kl=0,
                stream=None, workspace_bytes=None)


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def query(lib, v):
    return lib.tonic_distributional_mpo_workspace_bytes(v['B'], v['O'], v['A'], v['H'], v['S'], v['NA'])


def call(lib, entry, **changes):
    values = dict(DEFAULTS, **changes)
    if values['workspace_bytes'] is None:
        values['workspace_bytes'] = query(lib, values)
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ENTRIES[entry]]
    return getattr(lib, entry)(*args), lib.tonic_last_error()


# ---------------------------------------------------------------- 1. the restatement

def _cpu_model(O, A, sizes, atoms, seed):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    torch.manual_seed(seed)
    model = tt.models.ActorCriticWithTargets(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, torch.nn.ReLU),
                              head=tt.models.GaussianPolicyHead()),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, torch.nn.ReLU),
                                head=tt.models.DistributionalValueHead(*atoms)),
        observation_normalizer=tt.normalizers.MeanStd())
    model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    rng = np.random.RandomState(seed)
    model.observation_normalizer.record(rng.normal(size=(30, O)).astype(np.float32) * 2 + 0.5)
    model.observation_normalizer.update()
    with torch.no_grad():
        for net in (model.target_actor, model.target_critic):       # the targets away from the online networks
            for p in td4_ref.weights(net):
                p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.3, dtype=torch.float32)
        model.target_critic.head.distributional_layer.weight.mul_(8.0)
    return model, rng


def _cpu_batch(rng, B, O, A):
    batch = dict(observations=rng.normal(size=(B, O)), actions=rng.uniform(-1, 1, (B, A)),
                 next_observations=rng.normal(size=(B, O)), rewards=rng.normal(size=B) * 3,
                 discounts=0.99 * (rng.uniform(size=B) > 0.2))
    return {k: torch.as_tensor(v, dtype=torch.float64) for k, v in batch.items()}


def test_one_sample_of_a_scaleless_actor_is_the_d4pg_step():
    """S = 1 and a target actor whose scale is forced to 0: a' = loc_t(s'), the mixture is the one distribution, and
    the critic loss and gradients equal td4_ref's with identical twins and no noise (which tests/test_td4_host.py
    holds to the reference's D4PG step) — each critic's gradient, and half of its loss, to float64 rounding."""
    O, A, B, sizes = 7, 3, 13, (16, 12)
    model, rng = _cpu_model(O, A, sizes, (-5.0, 5.0, 11), seed=5)
    batch = _cpu_batch(rng, B, O, A)
    nets = dmpo_ref.Networks.of_model(model, len(sizes))
    nets.scale_bounds = (0.0, 0.0)
    eps = torch.as_tensor(rng.normal(size=(B, A)))
    out = dmpo_ref.critic_step(nets, batch, eps, 1)
    twin = td4_ref.Networks({name: getattr(model, attribute) for name, attribute in dmpo_ref.SINGLE.items()},
                            model.observation_normalizer, model.target_critic.head.values, len(sizes))
    # td4_ref's deterministic policy reads the first head, the Gaussian head's loc layer: tanh(loc) both ways
    want = td4_ref.critic_step(twin, batch, eps, 0.0, 0.5)
    assert torch.equal(nets.gaussian('target_actor', batch['next_observations'])[0],
                       twin.policy('target_actor', batch['next_observations']))
    np.testing.assert_allclose(float(out['loss']), float(want['loss']) / 2, rtol=1e-14)
    np.testing.assert_allclose(out['targets'].numpy(), want['targets'].numpy(), rtol=0, atol=1e-15)
    for i, (mine, theirs) in enumerate(zip(nets.params['critic_1'], twin.params['critic_1'])):
        scale = max(float(theirs.grad.abs().max()), 1e-30)
        np.testing.assert_allclose(mine.grad.numpy(), theirs.grad.numpy(), rtol=0, atol=1e-12 * scale, err_msg=str(i))
    assert all(p.grad is None for p in nets.params['critic_2'])


def test_the_projection_is_linear_in_the_distribution():
    """project(mean_s p_s) == mean_s project(p_s) to float64 rounding: what lets the kernel project the mixture
    once per row instead of every sample."""
    rng = np.random.RandomState(1)
    S, B, NA = 7, 9, 17
    values = torch.linspace(-4.0, 4.0, NA, dtype=torch.float64)
    samples = torch.softmax(torch.as_tensor(rng.normal(size=(S, B, NA)) * 3), -1)
    returns = torch.as_tensor(rng.normal(size=(B, 1)) * 3) + 0.97 * values[None]
    assert (returns < values[0]).any() and (returns > values[-1]).any()
    of_mean = dmpo_ref.project(values, samples.mean(0), returns)
    mean_of = torch.stack([dmpo_ref.project(values, samples[s], returns) for s in range(S)]).mean(0)
    np.testing.assert_allclose(of_mean.numpy(), mean_of.numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(of_mean.sum(-1).numpy(), 1.0, rtol=0, atol=1e-14)


def test_critic_targets_mix_the_samples_of_a_row():
    """Row m's mixture is the mean over s of the distributions at rows s * B + m of the tiled batch."""
    O, A, B, S, sizes = 7, 3, 5, 4, (16, 12)
    model, rng = _cpu_model(O, A, sizes, (-5.0, 5.0, 11), seed=2)
    batch = _cpu_batch(rng, B, O, A)
    nets = dmpo_ref.Networks.of_model(model, len(sizes))
    eps = torch.as_tensor(rng.normal(size=(S * B, A)))
    out = dmpo_ref.critic_targets(nets, batch, eps, S)
    loc, scale = nets.gaussian('target_actor', batch['next_observations'])
    for m in (0, B - 1):
        rows = []
        for s in range(S):
            action = loc[m] + scale[m] * eps[s * B + m]
            rows.append(torch.softmax(nets.logits('target_critic_1', batch['next_observations'][m:m + 1],
                                                  action[None]), -1)[0])
        np.testing.assert_allclose(out['mixture'][m].detach().numpy(), torch.stack(rows).mean(0).detach().numpy(),
                                   rtol=0, atol=1e-15)
    spread = out['samples'].std(0).max()
    assert float(spread) > 1e-3                              # (the samples' distributions do differ)


# ---------------------------------------------------------------- 2. the entries' statuses and the query

@pytest.mark.parametrize('entry', ENTRIES)
def test_entries_answer_before_any_gpu_work(lib, entry):
    """Every pointer NULL in turn, B <= 0, atoms 1 and 65, samples 0 and 257, unknown torso codes, joint_kl 2: -1,
    also when the workspace is too small as well (the pointer check wins); a workspace one byte short: -4.  Every
    pointer is a fake address nobody reads: each call returns before a launch (the method of
    tests/test_offpolicy_entries_host.py)."""
    from tonic_amd import _lib
    assert len(ENTRIES[entry]) == len(_lib.SIGNATURES[entry][1])
    for pointer in (name for name in ENTRIES[entry] if name.startswith('d_')):
        message = b'null column sums' if pointer == 'd_column_sums' else b'bad argument'      # (the shard's own check)
        expect(call(lib, entry, **{pointer: None}), INVALID, message)
        expect(call(lib, entry, **{pointer: None}, workspace_bytes=16), INVALID, message)
    for B in (0, -1):
        expect(call(lib, entry, B=B, workspace_bytes=1 << 40), INVALID, b'bad argument')
    for NA in (1, 65):
        expect(call(lib, entry, NA=NA, workspace_bytes=1 << 40), INVALID, b'2 <= atoms <= 64')
        expect(call(lib, entry, NA=NA, workspace_bytes=16), INVALID, b'2 <= atoms <= 64')
    for S in (0, 257):
        expect(call(lib, entry, S=S, workspace_bytes=1 << 40), INVALID, b'256')
    for code in UNKNOWN_H:
        expect(call(lib, entry, H=code, workspace_bytes=1 << 40), INVALID, b'bad argument')
    if 'joint_kl' in ENTRIES[entry]:
        for joint in (2, -1):
            expect(call(lib, entry, joint_kl=joint), INVALID, b'bad argument')
    expect(call(lib, entry, workspace_bytes=16), WORKSPACE, b'workspace too small')
    for H in (64, 256, lib.tonic_mlp_hidden(40, 24, 2), torso_code(lib, 'relu32x3'), torso_code(lib, 'one256')):
        for B, S, NA in ((1, 1, 2), (17, 20, 51), (37, 256, 64)):
            need = query(lib, dict(DEFAULTS, B=B, H=H, S=S, NA=NA))
            expect(call(lib, entry, B=B, H=H, S=S, NA=NA, workspace_bytes=need - 1), WORKSPACE,
                   b'workspace too small')
            # (one byte short of the scalar entries' workspace as well: the categorical arrays lie behind it)
            expect(call(lib, entry, B=B, H=H, S=S, NA=NA,
                        workspace_bytes=lib.tonic_mpo_workspace_bytes(B, 17, 6, H, S)), WORKSPACE)


def _answers(lib, torso):
    H = torso_code(lib, torso)
    return [lib.tonic_distributional_mpo_workspace_bytes(B, O, A, H, S, NA)
            for (B, O, A), S, NA in itertools.product(SHAPES, (1, 65), (2, 51))]


@pytest.mark.parametrize('torso', TORSOS)
def test_query_is_positive_and_never_below_the_scalar_one(lib, torso):
    H = torso_code(lib, torso)
    got = _answers(lib, torso)
    scalar = [lib.tonic_mpo_workspace_bytes(B, O, A, H, S)
              for (B, O, A), S, NA in itertools.product(SHAPES, (1, 65), (2, 51))]
    for mine, theirs in zip(got, scalar):
        assert mine > 0 and mine >= theirs, (mine, theirs)
    # a wider support never needs less
    for a, b in zip(got[0::2], got[1::2]):
        assert b >= a


def test_query_is_a_function_of_its_arguments(lib):
    """The run-time switches decide what an entry launches, never what the query answers."""
    want = {torso: _answers(lib, torso) for torso in TORSOS}
    saved = {}
    try:
        for name in ('q_images', 'policy_tail', 'q_chain'):
            value = ctypes.c_int32(0)
            assert lib.tonic_get_tuning(name.encode(), ctypes.addressof(value)) == 0, name
            saved[name] = value.value
            assert lib.tonic_set_tuning(name.encode(), 0) == 0, name
        assert {torso: _answers(lib, torso) for torso in TORSOS} == want
    finally:
        for name, value in saved.items():
            lib.tonic_set_tuning(name.encode(), value)


# ---------------------------------------------------------------- 3. the updaters and the agent

def _model(container, head, policy_head=None, O=5, A=2):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP((32, 32), torch.nn.ReLU),
                              head=policy_head or tt.models.GaussianPolicyHead()),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(),
                                torso=tt.models.MLP((32, 32), torch.nn.ReLU), head=head),
        observation_normalizer=tt.normalizers.MeanStd())
    model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
    return model


def test_updaters_refuse_by_name():
    import tonic_amd.torch as tt
    name = 'DistributionalExpectedSARSA'
    updater = tt.updaters.DistributionalExpectedSARSA()
    assert (updater.stats_kind, updater.stock_capable, updater.head_family) == (3, False, 'mpo')
    assert updater.num_samples == 20 and updater.default_lr == 3e-4 and updater.gradient_clip == 0
    plain = _model(tt.models.ActorCriticWithTargets, tt.models.ValueHead())
    with pytest.raises(NotImplementedError, match=name + '.*DistributionalValueHead'):
        updater.initialize(plain)
    uneven = _model(tt.models.ActorCriticWithTargets, tt.models.DistributionalValueHead(-10., 10., 21))
    uneven.target_critic.head.values = uneven.target_critic.head.values * 0.5
    with pytest.raises(NotImplementedError, match=name + '.*same support'):
        updater.initialize(uneven)
    fewer = _model(tt.models.ActorCriticWithTargets, tt.models.DistributionalValueHead(-10., 10., 21))
    fewer.target_critic.head.values = fewer.target_critic.head.values[:20]
    with pytest.raises(NotImplementedError, match=name + '.*same support'):
        updater.initialize(fewer)
    twin = _model(tt.models.ActorTwinCriticWithTargets, tt.models.DistributionalValueHead(-10., 10., 21))
    with pytest.raises(NotImplementedError, match=name + '.*twin critics'):
        updater.initialize(twin)
    for samples in (0, 257):
        with pytest.raises(NotImplementedError, match=f'{name}.*num_samples={samples}.*256'):
            tt.updaters.DistributionalExpectedSARSA(num_samples=samples)
    # the scalar critic step on a categorical critic: refused, naming the updater that serves it
    categorical = _model(tt.models.ActorCriticWithTargets, tt.models.DistributionalValueHead(-10., 10., 21))
    with pytest.raises(NotImplementedError, match='ExpectedSARSA.*DistributionalExpectedSARSA'):
        tt.updaters.ExpectedSARSA().initialize(categorical)


def test_agent_defaults():
    """MPO's actor and the head D4PG and TD4 default to on MPO's critic torso, 5-step returns, the new critic step
    beside MPO's actor step; MPO's schedule, noise draws and refusal of a Return normaliser."""
    import tonic_amd
    import tonic_amd.torch as tt
    agent = tt.agents.DMPO()
    assert isinstance(agent, tt.agents.MPO) and agent.policy_kind == 2 and agent.serves_return_normalizer is False
    model, mpo = agent.model, tt.agents.MPO().model
    assert type(model) is tt.models.ActorCriticWithTargets
    for critic in (model.critic, model.target_critic):
        assert isinstance(critic.head, tt.models.DistributionalValueHead) and critic.head.num_atoms == 51
        assert torch.equal(critic.head.values, torch.linspace(-150., 150., 51))
        assert isinstance(critic.encoder, tt.models.ObservationActionEncoder)
        assert (critic.torso.sizes, critic.torso.activation) == (mpo.critic.torso.sizes, mpo.critic.torso.activation)
        assert critic.torso.sizes == (256, 256) and critic.torso.activation is torch.nn.ReLU
    for actor in (model.actor, model.target_actor):
        assert isinstance(actor.head, tt.models.GaussianPolicyHead)
        assert (actor.torso.sizes, actor.torso.activation) == (mpo.actor.torso.sizes, mpo.actor.torso.activation)
    assert isinstance(model.observation_normalizer, tt.normalizers.MeanStd) and model.return_normalizer is None
    assert type(agent.replay) is tonic_amd.replays.Buffer and agent.replay.return_steps == 5
    assert type(agent.actor_updater) is tt.updaters.MaximumAPosterioriPolicyOptimization
    assert type(agent.critic_updater) is tt.updaters.DistributionalExpectedSARSA
    assert (agent.actor_updater.num_samples, agent.critic_updater.num_samples) == (20, 20)
    assert agent._noise_samples(2) == (20, 20) and agent._actor_due(0) and agent._actor_due(1)
    assert tt.agents.DMPO(replay=tonic_amd.replays.Buffer(return_steps=1)).replay.return_steps == 1
    given = tt.updaters.DistributionalExpectedSARSA(num_samples=3)
    assert tt.agents.DMPO(critic_updater=given).critic_updater is given


def test_a_prioritized_buffer_is_refused_with_the_message_that_was():
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    agent = tt.agents.DMPO(replay=tonic_amd.replays.PrioritizedBuffer(return_steps=5))
    with pytest.raises(NotImplementedError, match='PrioritizedBuffer with the critic updater '
                                                  'DistributionalExpectedSARSA is not served.*\\(D4PG, TD4\\)'):
        agent.initialize(Box(-np.inf, np.inf, (5,)), Box(-1, 1, (2,)), seed=0)
