"""CPU tests of the off-policy torso codes (no device): tonic_mlp_torso against tonic_mlp_hidden and the plain
width, its argument limits, the packed parameter counts of 1 .. 4 layer torsos against the layout FlatNetwork
writes, the updaters' routing of torsos, and the committed torso goldens against their generator."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NAMES = ('sac_deep3_small', 'td3_single_small', 'ddpg_deep4_small', 'd4pg_uneven_small', 'd4pg_tanh3_small',
         'mpo_elu_small', 'mpo_deep3_small')
ACTIVATIONS = {1: torch.nn.ReLU, 2: torch.nn.Tanh, 3: torch.nn.ELU}


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def torso_code(lib, sizes, activation):
    return lib.tonic_mlp_torso(len(sizes), (ctypes.c_int32 * len(sizes))(*sizes), activation)


def test_two_layer_codes_are_the_hidden_codes(lib):
    for sizes, activation in (((256, 256), 1), ((1024, 1024), 1), ((4000, 4000), 1), ((400, 300), 1),
                              ((256, 256), 2), ((48, 40), 3), ((1, 4095), 2)):
        code = torso_code(lib, sizes, activation)
        assert code == lib.tonic_mlp_hidden(sizes[0], sizes[1], activation) > 0, (sizes, activation)
        assert not code & (1 << 29)
    assert torso_code(lib, (256, 256), 1) == 256            # the plain width, as it is


def test_descriptor_codes_are_stable(lib):
    cases = [((64, 48, 32), 1), ((40,), 2), ((32, 32, 24, 16), 3), ((1024,), 1), ((33, 7, 100), 2),
             ((4095, 1, 4095, 1), 1)]
    codes = [torso_code(lib, sizes, activation) for sizes, activation in cases]
    for code in codes:
        assert code > 0 and code & (1 << 30) and code & (1 << 29)
    assert len(set(codes)) == len(codes)
    assert [torso_code(lib, sizes, activation) for sizes, activation in cases] == codes   # same torso, same code
    assert torso_code(lib, (64, 48, 32), 2) not in codes                                 # activation counts


def test_bad_arguments_are_negative(lib):
    for sizes, layers, activation in (((), 0, 1), ((8,) * 5, 5, 1), ((0,), 1, 1), ((4096,), 1, 1),
                                      ((16, 0, 16), 3, 1), ((16, 16, 4096), 3, 2), ((16,), 1, 4),
                                      ((16,), 1, 0), ((16, 16, 16), 3, -1)):
        array = (ctypes.c_int32 * max(len(sizes), 1))(*sizes)
        assert lib.tonic_mlp_torso(layers, array, activation) < 0, (sizes, layers, activation)
        assert lib.tonic_last_error()
    assert lib.tonic_mlp_torso(3, None, 1) < 0
    assert lib.tonic_mlp_torso(2, (ctypes.c_int32 * 2)(4096, 16), 1) < 0


def _networks(kind, sizes, activation, O, A, atoms=21):
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    act = ACTIVATIONS[activation]
    critic_head = tt.models.DistributionalValueHead(-6.0, 6.0, atoms) if kind == 'd4pg' else tt.models.ValueHead()
    if kind == 'sac':
        head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                            distribution=tt.models.SquashedMultivariateNormalDiag)
    elif kind == 'mpo':
        head = tt.models.GaussianPolicyHead()
    else:
        head = tt.models.DeterministicPolicyHead()
    actor = tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act), head=head)
    critic = tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                              head=critic_head)
    observation_space, action_space = Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,))
    actor.initialize(observation_space, action_space)
    critic.initialize(observation_space, action_space)
    return actor, critic


@pytest.mark.parametrize('kind', ['sac', 'td3', 'd4pg', 'mpo'])
@pytest.mark.parametrize('sizes,activation', [((40,), 2), ((64, 48, 32), 1), ((32, 32, 24, 16), 3),
                                              ((400, 300, 200), 1), ((33, 7, 100), 2), ((60, 40), 1),
                                              ((1024,), 1), ((256, 256), 1)])
def test_param_counts_match_the_padded_layout(lib, kind, sizes, activation):
    from tonic_amd.torch.models import FlatNetwork
    O, A = 17, 6
    actor, critic = _networks(kind, sizes, activation, O, A)
    H = torso_code(lib, sizes, activation)
    heads = 2 if kind in ('sac', 'mpo') else 1
    assert lib.tonic_mlp_actor_param_count(O, H, A, heads) == FlatNetwork.length(actor, padded=True)
    if kind == 'd4pg':
        assert lib.tonic_mlp_actor_param_count(O + A, H, 21, 1) == FlatNetwork.length(critic, padded=True)
    else:
        assert lib.tonic_q_critic_param_count(O, A, H) == FlatNetwork.length(critic, padded=True)


def test_workspace_queries(lib):
    """The two-layer queries do not move with the new codes; deeper torsos ask for more, and the fused-only
    queries keep refusing every code but a plain width."""
    B, O, A = 256, 17, 6
    deep = torso_code(lib, (256, 256, 256), 1)
    single = torso_code(lib, (256,), 1)
    for query in (lambda H: lib.tonic_offpolicy_workspace_bytes(B, O, A, H),
                  lambda H: lib.tonic_distributional_workspace_bytes(B, O, A, H, 51),
                  lambda H: lib.tonic_mpo_workspace_bytes(B, O, A, H, 20)):
        assert query(deep) > query(lib.tonic_mlp_hidden(256, 256, 2)) > 0
        assert query(single) > 0
    for H in (deep, single, lib.tonic_mlp_hidden(400, 300, 1)):
        assert lib.tonic_q_iteration_supported(O, H, A, 1) == 0
        assert lib.tonic_q_iteration_ahead_supported(B, O, H, A, 2, 1) == 0
        assert lib.tonic_mlp_actor_image_bytes(O, H, A, 1) == 0


def test_updaters_route_torsos(monkeypatch):
    """Every off-policy updater takes 1 .. 4 layer torsos to the HIP entries; beyond that SAC / TD3 / DDPG fall
    back to stock torch operators and D4PG / MPO raise, with the envelope in the message."""
    from tonic_amd.torch import updaters

    class Torso:
        def __init__(self, sizes, activation):
            self.sizes, self.activation = sizes, activation

    code = updaters._torso_width(Torso((64, 48, 32), torch.nn.ReLU))
    assert code > 0 and code & (1 << 29)
    assert updaters._torso_width(Torso((64, 64), torch.nn.ReLU)) == 64
    assert updaters._torso_width(Torso((40,), torch.nn.Tanh), True) & (1 << 29)
    for bad in (Torso((8,) * 5, torch.nn.ReLU), Torso((64, 64, 64), torch.nn.Sigmoid),
                Torso((4096, 64), torch.nn.ReLU)):
        for generic in (False, True):
            with pytest.raises(NotImplementedError, match='1 .. 4 layers'):
                updaters._torso_width(bad, generic)
    monkeypatch.setenv('TONIC_AMD_TORSO_STOCK', '1')
    with pytest.raises(NotImplementedError):
        updaters._torso_width(Torso((64, 48, 32), torch.nn.ReLU), True)        # SAC / TD3 / DDPG: stock
    assert updaters._torso_width(Torso((64, 48, 32), torch.nn.ReLU)) == code   # D4PG / MPO: no stock form
    for cls in (updaters.DistributionalDeterministicQLearning, updaters.DistributionalDeterministicPolicyGradient,
                updaters.ExpectedSARSA, updaters.MaximumAPosterioriPolicyOptimization):
        assert cls.stock_capable is False


def test_goldens_are_small_and_carry_their_torso():
    for name in NAMES:
        path = os.path.join(GOLDEN, name + '.npz')
        assert os.path.getsize(path) < 1 << 20, name
        g = np.load(path)
        sizes = tuple(int(v) for v in g['torso_sizes'])
        assert max(sizes) <= 64 and str(g['torso_activation']) in ('ReLU', 'Tanh', 'ELU'), name
        plain = len(sizes) == 2 and sizes[0] == sizes[1] and str(g['torso_activation']) == 'ReLU'
        assert not plain, name


def _reference_present():
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    try:
        import reference_loader
        return reference_loader.reference_available()
    finally:
        sys.path.pop(0)


@pytest.mark.skipif(not _reference_present(), reason='the reference checkout is not present')
def test_committed_goldens_equal_the_generator(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'scripts', 'make_torso_goldens.py'),
                           '--out', str(tmp_path)] + list(NAMES), stdout=subprocess.DEVNULL)
    for name in NAMES:
        want, got = np.load(os.path.join(GOLDEN, name + '.npz')), np.load(str(tmp_path / (name + '.npz')))
        assert sorted(want.files) == sorted(got.files), name
        for key in want.files:       # (the replay buffers' unwritten rows hold NaN)
            numeric = want[key].dtype.kind in 'fc'
            assert np.array_equal(want[key], got[key], equal_nan=numeric), (name, key)
