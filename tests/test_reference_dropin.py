"""The drop-in claims held against what the REFERENCE's own code computed, recorded by oracle/make_golden.py
in tests/golden/reference_dropin.npz: the reference agents' strict load accepts a checkpoint written by this
package (same keys, same shapes), CategoricalWithSupport equals the reference's bit for bit, and the
explorations and scripted agents follow the reference's random streams.  (The checks that run the reference
itself — its `tonic.train` driving this package's agents, the fixtures regenerated — are
oracle/reference_checks.py.)"""
import numpy as np
import pytest

import reference_streams

AGENTS = ('PPO', 'A2C', 'TRPO', 'SAC', 'TD3', 'DDPG', 'D4PG', 'MPO')


@pytest.fixture(scope='module')
def recorded(golden):
    return golden('reference_dropin')


@pytest.mark.parametrize('name', AGENTS)
def test_reference_agents_load_this_packages_checkpoints(tmp_path, name, recorded):
    """tonic/torch/agents/agent.py:23-26: the reference agent's strict load_state_dict accepts a
    `.pt` written by this package's Agent.save exactly when it holds the reference's keys with the
    reference's shapes (recorded from the reference's agent at O=11, A=3); what it loads is what was saved."""
    import torch
    import tonic_amd
    import tonic_amd.torch
    from tonic_amd.environments import Box
    observation_space, action_space = Box(-np.inf, np.inf, (11,)), Box(-1, 1, (3,))
    prefix = f'state/{name}/'
    reference = {k[len(prefix):]: tuple(int(n) for n in recorded[k])
                 for k in recorded.files if k.startswith(prefix)}
    assert reference, name
    mine = getattr(tonic_amd.torch.agents, name)()
    mine.model.initialize(observation_space, action_space)         # CPU parameters suffice
    torch.manual_seed(1)
    for parameter in mine.model.parameters():
        parameter.data.copy_(torch.randn(parameter.shape))
    mine.save(str(tmp_path / 'step_1'))
    saved = torch.load(tmp_path / 'step_1.pt', map_location='cpu')
    assert set(saved) == set(reference)
    for key, value in saved.items():
        assert tuple(value.shape) == reference[key], key
        assert value.dtype == torch.float32, key
    want = mine.model.state_dict()
    assert set(want) == set(saved)
    for key in want:
        assert torch.equal(saved[key], want[key].cpu()), key


def test_categorical_with_support_equals_the_reference(recorded):
    """models.CategoricalWithSupport / DistributionalValueHead (critics.py:23-66): same support,
    probabilities, mean and projection as the reference's, bit for bit, on returns inside, outside
    and exactly on the support."""
    import torch
    import tonic_amd.torch as tt
    mine = tt.models.DistributionalValueHead(-7.5, 4.0, 23)
    assert torch.equal(mine.values, torch.from_numpy(recorded['categorical/values']))
    logits = torch.from_numpy(recorded['categorical/logits'])
    returns = torch.from_numpy(recorded['categorical/returns'])
    assert torch.equal(returns[0], mine.values)                   # exactly on the atoms
    b = tt.models.CategoricalWithSupport(mine.values, logits)
    assert torch.equal(b.probabilities, torch.from_numpy(recorded['categorical/probabilities']))
    assert torch.equal(b.mean(), torch.from_numpy(recorded['categorical/mean']))
    assert torch.equal(b.project(returns), torch.from_numpy(recorded['categorical/project']))


def test_explorations_and_scripted_agents_follow_the_reference_streams(recorded):
    """tonic/explorations/noisy.py and tonic/agents/basic.py (host logic either side of the policy
    forward; `--agent 'tonic.agents.UniformRandom()'` is part of the reference's command line): same
    constructor arguments, same NumPy RandomState stream, same per-worker reset
    handling — bit-identical action sequences over warm-up, policy steps and resets."""
    import tonic_amd
    from tonic_amd.environments import Box
    ours = reference_streams.records(tonic_amd, Box(-1, 1, (3,)))
    theirs = {k[len('streams/'):]: recorded[k] for k in recorded.files if k.startswith('streams/')}
    assert list(ours) == sorted(theirs, key=list(ours).index) and set(ours) == set(theirs)
    for key, a in ours.items():
        b = theirs[key]
        assert a.dtype == b.dtype and np.array_equal(a, b), key
