"""Host-side tests (no GPU) of the Return normaliser on the off-policy agents: the float64 restatement against the
unmodified reference, the C ABI's argument check, the per-step [min, max] record, the merge of the ranks' ranges and
the state-dict keys.  The kernels: tests/test_gpu_offpolicy_return.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import return_squash_ref as rs

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NAMES = ('sac_return_small', 'td3_return_small', 'ddpg_return_small')


def _reference_present():
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    try:
        import reference_loader
        return reference_loader.reference_available()
    finally:
        sys.path.pop(0)


def _reference():
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    try:
        import reference_loader
        return reference_loader, reference_loader.load_reference()
    finally:
        sys.path.pop(0)


needs_reference = pytest.mark.skipif(not _reference_present(), reason='the reference checkout is not present')


# ---------------------------------------------------------------- the restatement

@needs_reference
def test_restatement_equals_the_reference_value_head():
    """return_squash_ref on random z against the unmodified reference's ValueHead + Return.forward, the range moved
    by record / update: float64 to rounding, float32 to an ulp of the sum's operands (torch's sigmoid is not the
    1 / (1 + exp(-z)) of the kernels bit for bit), and the derivative against autograd."""
    _, tonic = _reference()
    rn = tonic.torch.normalizers.Return(0.99)
    rn.record(np.array([-5.725, 0.25, 3.5], np.float32))
    rn.update()
    low, high = float(rn._low), float(rn._high)
    assert (low, high) == (-572.5, 350.0)
    head = tonic.torch.models.ValueHead()
    head.initialize(8, return_normalizer=rn)
    rng = np.random.RandomState(0)
    h = torch.as_tensor(rng.normal(size=(257, 8)) * 12, dtype=torch.float32)
    with torch.no_grad():
        z = head.v_layer(h).squeeze(-1)
        want = head(h)
    assert float(z.abs().max()) > 6 and float(z.abs().min()) < 0.1
    got64 = rs.squash64(z.double(), low, high)
    np.testing.assert_allclose(got64.numpy(), want.double().numpy(), rtol=0, atol=2 * np.spacing(np.float32(922.5)))
    got32 = rs.squash32(z.numpy(), low, high)
    assert np.abs(got32.astype(np.float64) - want.numpy()).max() <= 2 * np.spacing(np.float32(922.5))
    # the derivative: float64 autograd of the reference's forward against the float32 factor from the published v
    z64 = z.double().requires_grad_()
    rs.squash64(z64, low, high).sum().backward()
    factor = rs.squash_dz32(np.ones_like(got32), got32, low, high)
    assert np.abs(factor - z64.grad.numpy()).max() <= 1e-6 * np.abs(z64.grad.numpy()).max()
    # +-inf and NaN
    edge = rs.squash32(np.array([np.inf, -np.inf, np.nan], np.float32), low, high)
    assert edge[0] == np.float32(high) and edge[1] == np.float32(low) and np.isnan(edge[2])


# ---------------------------------------------------------------- C ABI

def _call_ranged(lib, name, low, high):
    from tonic_amd import _lib
    restype, argtypes = _lib.SIGNATURES[name]
    args = []
    for i, kind in enumerate(argtypes):
        args.append(None if kind is _lib.c_vp else (0.0 if kind is _lib.c_f64 else 0))
    # the two bounds sit in front of (workspace, bytes, stream)
    args[-5], args[-4] = low, high
    return getattr(lib, name)(*args)


@pytest.mark.parametrize('name', ['tonic_twin_q_grad_ranged', 'tonic_actor_q_grad_ranged'])
def test_ranged_entries_refuse_exactly_one_bound(name):
    """The library exports both entries; with exactly one of d_value_low / d_value_high NULL they return
    TONIC_ERR_INVALID_ARGUMENT and tonic_last_error names the missing argument — before anything touches the device
    (every other argument here is NULL / 0; the bound that is given is a host address nobody reads)."""
    from tonic_amd import _lib
    lib = _lib.load()
    assert lib.tonic_abi_version() >= 18
    bound = ctypes.c_float(1.0)
    address = ctypes.addressof(bound)
    assert _call_ranged(lib, name, None, address) == -1
    message = lib.tonic_last_error().decode()
    assert name in message and 'd_value_low' in message, message
    assert _call_ranged(lib, name, address, None) == -1
    message = lib.tonic_last_error().decode()
    assert name in message and 'd_value_high' in message, message
    # both NULL passes this check and fails the next one (the entry without the suffix's own argument check)
    assert _call_ranged(lib, name, None, None) == -1
    assert 'd_value' not in lib.tonic_last_error().decode()


# ---------------------------------------------------------------- the per-step record

STEPS = {
    'random': [np.random.RandomState(s).normal(size=5).astype(np.float32) * 3 for s in range(12)],
    'a NaN among them': [np.array([0.5, np.nan, -2.5, 4.0], np.float32), np.array([np.nan, 7.0], np.float32),
                         np.array([-3.0, np.nan], np.float32)],
    'all NaN': [np.array([np.nan, np.nan], np.float32), np.array([2.0, -0.5], np.float32),
                np.array([np.nan], np.float32)],
    'infinities': [np.array([1.5, np.inf], np.float32), np.array([-np.inf, 0.0], np.float32),
                   np.array([3.0], np.float32)],
    'inside the initial range': [np.array([0.25, -0.5], np.float32)],
}


@needs_reference
@pytest.mark.parametrize('case', list(STEPS))
def test_step_pair_record_equals_the_reference_loop(case):
    """agents.record_reward_range (ONE record of the step's [min, max], NaN skipped, nothing for an all-NaN step)
    against the reference's Return.record over every reward of every step: min_reward / max_reward bit for bit
    after each step, and _low / _high after update()."""
    from tonic_amd.torch import agents, normalizers
    _, tonic = _reference()
    want = tonic.torch.normalizers.Return(0.99)
    got = normalizers.Return(0.99)
    with np.errstate(invalid='ignore'):
        for rewards in STEPS[case]:
            want.record(rewards)
            before = (got.min_reward, got.max_reward)
            agents.record_reward_range(got, rewards)
            if np.isnan(rewards).all():
                assert (got.min_reward, got.max_reward) == before
            for a, b in ((got.min_reward, want.min_reward), (got.max_reward, want.max_reward)):
                assert np.float32(a).tobytes() == np.float32(b).tobytes(), (case, a, b)
        want.update()
        got.update()
    assert torch.equal(got._low.data, want._low.data) and torch.equal(got._high.data, want._high.data)


def test_step_pair_record_without_the_reference():
    """The same properties from the definition (kept when the reference checkout is absent)."""
    from tonic_amd.torch import agents, normalizers
    rn = normalizers.Return(0.99)
    agents.record_reward_range(rn, np.array([np.nan, np.nan], np.float32))
    assert (rn.min_reward, rn.max_reward) == (-1, 1)
    agents.record_reward_range(rn, np.array([0.5, np.nan, -2.5, 4.0], np.float32))
    assert (rn.min_reward, rn.max_reward) == (np.float32(-2.5), np.float32(4.0))
    agents.record_reward_range(rn, np.array([np.inf, -3.0], np.float32))
    assert (rn.min_reward, rn.max_reward) == (np.float32(-3.0), np.float32(np.inf))


# ---------------------------------------------------------------- the rank merge

MERGE_WORKER = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tonic_amd import parallel
from tonic_amd.torch import agents, normalizers
rank, world = parallel.init_from_env(backend='gloo')
assert world == 2
rn = normalizers.Return(0.99)
# rank 0 saw rewards down to -4.25, rank 1 up to 6.5: both end with the union
agents.record_reward_range(rn, np.array([-4.25, 0.5] if rank == 0 else [0.25, 6.5], np.float32))
agents.merge_reward_ranges(rn)
assert (rn.min_reward, rn.max_reward) == (np.float32(-4.25), np.float32(6.5)), (rn.min_reward, rn.max_reward)
assert type(rn.min_reward) is np.float32 and type(rn.max_reward) is np.float32
# a rank that recorded nothing changes nothing: rank 1 holds the initial (-1, 1)
rn = normalizers.Return(0.99)
if rank == 0:
    agents.record_reward_range(rn, np.array([-2.0, 3.0], np.float32))
agents.merge_reward_ranges(rn)
assert (rn.min_reward, rn.max_reward) == (np.float32(-2.0), np.float32(3.0)), (rn.min_reward, rn.max_reward)
# nobody recorded: the initial range
rn = normalizers.Return(0.99)
agents.merge_reward_ranges(rn)
assert (rn.min_reward, rn.max_reward) == (-1, 1)
rn.update()
assert (float(rn._low), float(rn._high)) == (-100.0, 100.0)
print('rank', rank, 'ok')
'''


def test_two_ranks_end_with_the_union_of_their_ranges_gloo(tmp_path):
    script = tmp_path / 'worker.py'
    script.write_text(MERGE_WORKER)
    import socket
    with socket.socket() as probe:              # a port nobody holds (suites may run side by side on one host)
        probe.bind(('127.0.0.1', 0))
        port = probe.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='2', OMP_NUM_THREADS='1')
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, out
        assert f'rank {r} ok' in out


def test_one_process_merges_nothing():
    from tonic_amd.torch import agents, normalizers
    rn = normalizers.Return(0.99)
    agents.record_reward_range(rn, np.array([-2.0, 3.0], np.float32))
    agents.merge_reward_ranges(rn)
    assert (rn.min_reward, rn.max_reward) == (np.float32(-2.0), np.float32(3.0))


# ---------------------------------------------------------------- state dict, packed block

def _td3_model(tt):
    from tonic_amd.environments import Box
    torch.manual_seed(3)
    model = tt.models.ActorTwinCriticWithTargets(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP((32, 32), torch.nn.ReLU),
                              head=tt.models.DeterministicPolicyHead()),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(),
                                torso=tt.models.MLP((32, 32), torch.nn.ReLU), head=tt.models.ValueHead()),
        observation_normalizer=tt.normalizers.MeanStd(), return_normalizer=tt.normalizers.Return(0.99))
    agent = tt.agents.TD3(model=model)
    assert agent.model.critic is agent.model.critic_1                # td3.py:36
    model.initialize(Box(-np.inf, np.inf, (9,)), Box(-1, 1, (4,)))
    return model


def test_state_dict_keys_are_those_of_the_reference_golden():
    """Keys and shapes of a tonic_amd TD3 model with a Return normaliser (CPU, before pack) against the reference's
    state dict recorded in td3_return_small.npz: return_normalizer._low / _high, critic*.head.return_normalizer.*,
    target_critic*.head.return_normalizer.* — one shared module."""
    import tonic_amd.torch as tt
    g = np.load(os.path.join(GOLDEN, 'td3_return_small.npz'))
    model = _td3_model(tt)
    state = model.state_dict()
    want = {k[len('init/'):]: g[k].shape for k in g.files if k.startswith('init/')}
    assert {k: tuple(v.shape) for k, v in state.items()} == want
    for prefix in ('', 'critic.head.', 'critic_1.head.', 'critic_2.head.', 'target_critic_1.head.',
                   'target_critic_2.head.'):
        for name in ('_low', '_high'):
            assert prefix + 'return_normalizer.' + name in state
    rn = model.return_normalizer
    for net in (model.critic_1, model.critic_2, model.target_critic_1, model.target_critic_2):
        assert net.head.return_normalizer is rn
    assert model.actor.head is not None and not hasattr(model.actor.head, 'return_normalizer')


@needs_reference
def test_state_dicts_load_into_each_other_strictly():
    import tonic_amd.torch as tt
    rl, tonic = _reference()
    ours = _td3_model(tt)
    env = rl.SyntheticEnvironment(9, 4, max_episode_steps=5)
    torch.manual_seed(4)
    models = tonic.torch.models
    theirs = models.ActorTwinCriticWithTargets(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP((32, 32), torch.nn.ReLU),
                           head=models.DeterministicPolicyHead()),
        critic=models.Critic(encoder=models.ObservationActionEncoder(), torso=models.MLP((32, 32), torch.nn.ReLU),
                             head=models.ValueHead()),
        observation_normalizer=tonic.torch.normalizers.MeanStd(),
        return_normalizer=tonic.torch.normalizers.Return(0.99))
    agent = tonic.torch.agents.TD3(model=theirs)
    agent.initialize(env.observation_space, env.action_space, seed=4)
    theirs = agent.model
    a, b = ours.state_dict(), theirs.state_dict()
    assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()}
    theirs.return_normalizer.record(np.array([-3.0, 2.0], np.float32))
    theirs.return_normalizer.update()
    ours.load_state_dict(theirs.state_dict(), strict=True)
    assert float(ours.return_normalizer._low) == float(theirs.return_normalizer._low) != -100.0
    ours.return_normalizer.record(np.array([-7.0, 9.0], np.float32))
    ours.return_normalizer.update()
    theirs.load_state_dict(ours.state_dict(), strict=True)
    assert float(theirs.return_normalizer._high) == float(ours.return_normalizer._high) != 100.0
    assert float(theirs.critic_2.head.return_normalizer._high) == float(ours.return_normalizer._high)


def test_packed_blocks_and_polyak_leave_the_range_out():
    """network_variables — what FlatNetwork packs, Adam steps and the polyak update mixes — holds no normaliser
    parameter, like the reference's trainable_variables; the two parameters do not require gradients."""
    import tonic_amd.torch as tt
    from tonic_amd.torch.models import FlatNetwork, network_variables
    model = _td3_model(tt)
    rn = model.return_normalizer
    for net in (model.critic_1, model.target_critic_2):
        assert all(p is not rn._low and p is not rn._high for p in network_variables(net))
        flat = [p for p, _, _ in FlatNetwork.slots(net, padded=False)]
        assert len(flat) == 6 and all(p is not rn._low and p is not rn._high for p in flat)
    assert all(p is not rn._low and p is not rn._high for p in model.online_variables + model.target_variables)
    assert not rn._low.requires_grad and not rn._high.requires_grad


# ---------------------------------------------------------------- the fixtures

@needs_reference
def test_committed_goldens_equal_the_generator(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'scripts', 'make_offpolicy_return_goldens.py'),
                           '--out', str(tmp_path)] + list(NAMES), stdout=subprocess.DEVNULL)
    for name in NAMES:
        want, got = np.load(os.path.join(GOLDEN, name + '.npz')), np.load(str(tmp_path / (name + '.npz')))
        assert sorted(want.files) == sorted(got.files), name
        for key in want.files:
            assert np.array_equal(want[key], got[key]), (name, key)
