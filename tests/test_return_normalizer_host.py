"""CPU tests of the Return normaliser (tonic/torch/normalizers/returns.py): the host class against a
line-by-line restatement of the reference, the pair record the on-policy agents rely on, the state-dict
layout of a model that carries it, and the committed goldens against their generator."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NAMES = ('ppo_return_small', 'a2c_return_small', 'trpo_return_small', 'ppo_wide_return_small',
         'ppo_tanh3_return_small')


class _ReferenceReturn:
    """returns.py:6-41, line by line (host state only)."""

    def __init__(self, discount_factor):
        assert 0 <= discount_factor < 1
        self.coefficient = 1 / (1 - discount_factor)
        self.min_reward = np.float32(-1)
        self.max_reward = np.float32(1)
        self._low = torch.as_tensor(self.coefficient * self.min_reward, dtype=torch.float32)
        self._high = torch.as_tensor(self.coefficient * self.max_reward, dtype=torch.float32)

    def record(self, values):
        for val in values:
            if val < self.min_reward:
                self.min_reward = np.float32(val)
            elif val > self.max_reward:
                self.max_reward = np.float32(val)

    def update(self):
        self._low = torch.as_tensor(self.coefficient * self.min_reward, dtype=torch.float32)
        self._high = torch.as_tensor(self.coefficient * self.max_reward, dtype=torch.float32)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.tobytes() == b.tobytes()


def _pair(values):
    """What tonic_reward_range hands the agent: [nanmin, nanmax], or None when nothing is not NaN."""
    values = np.asarray(values, np.float32).ravel()
    finite = values[~np.isnan(values)]
    if finite.size == 0:
        return None
    return np.array([finite.min(), finite.max()], np.float32)


def _reward_batches(rng):
    yield rng.normal(size=(24, 8)).astype(np.float32) * 3
    yield (rng.normal(size=(5, 3)) * 200).astype(np.float32)
    x = rng.normal(size=(7, 5)).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.3] = np.nan
    yield x
    x = rng.normal(size=(6, 4)).astype(np.float32)
    x[0, 1], x[3, 2] = np.inf, -np.inf
    yield x
    yield np.full((3, 4), np.nan, np.float32)
    yield np.array([[0.5]], np.float32)
    yield np.array([[np.inf, np.nan]], np.float32)
    yield np.array([[-np.inf]], np.float32)


def test_return_matches_reference_restatement():
    from tonic_amd.torch.normalizers import Return
    rng = np.random.RandomState(0)
    for discount in (0.0, 0.9, 0.99):
        ours, ref = Return(discount), _ReferenceReturn(discount)
        assert _same(ours._low.data, ref._low) and _same(ours._high.data, ref._high)
        assert isinstance(ours._low, torch.nn.Parameter) and not ours._low.requires_grad
        assert ours._low.dim() == 0 and ours._low.dtype == torch.float32
        for batch in _reward_batches(rng):
            for row in batch:
                ours.record(row)
                ref.record(row)
            assert type(ours.min_reward) is np.float32 and type(ours.max_reward) is np.float32
            assert _same(ours.min_reward, ref.min_reward) and _same(ours.max_reward, ref.max_reward)
            ours.update()
            ref.update()
            assert _same(ours._low.data, ref._low) and _same(ours._high.data, ref._high)
    with pytest.raises(AssertionError):
        Return(1.0)


def test_return_forward_is_the_squashed_head():
    from tonic_amd.torch.normalizers import Return
    rn = Return(0.99)
    rn._update(np.float32(-3.5), np.float32(7.25))
    z = torch.linspace(-40, 40, 101)
    want = rn._low + torch.sigmoid(z) * (rn._high - rn._low)
    assert torch.equal(rn(z), want)


def test_recording_the_pair_equals_recording_every_value():
    """The agents record [nanmin, nanmax] of a rollout instead of every reward (tonic_reward_range)."""
    from tonic_amd.torch.normalizers import Return
    rng = np.random.RandomState(1)
    for trial in range(40):
        every, pair = Return(0.99), Return(0.99)
        for batch in _reward_batches(rng):
            if trial % 3 == 0:
                batch = batch * np.float32(0.1)          # inside the initial [-1, 1]: nothing moves
            for row in batch:
                every.record(row)
            p = _pair(batch)
            if p is not None:
                pair.record(p)
            assert _same(every.min_reward, pair.min_reward) and _same(every.max_reward, pair.max_reward)
            every.update()
            pair.update()
            assert _same(every._low.data, pair._low.data) and _same(every._high.data, pair._high.data)


def test_state_dict_keys_match_the_golden():
    import tonic_amd.torch  # noqa: F401
    from tonic_amd.environments import Box
    from tonic_amd.torch import models, normalizers
    for name in NAMES:
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        O, A = int(g['cfg'][0]), int(g['cfg'][1])
        sizes, act = tuple(int(s) for s in g['torso_sizes']), getattr(torch.nn, str(g['torso_activation']))
        model = models.ActorCritic(
            actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, act),
                               head=models.DetachedScaleGaussianPolicyHead()),
            critic=models.Critic(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, act),
                                 head=models.ValueHead()),
            observation_normalizer=normalizers.MeanStd(), return_normalizer=normalizers.Return(0.99))
        model.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)))
        want = sorted(k[len('init/'):] for k in g if k.startswith('init/'))
        assert sorted(model.state_dict()) == want, name
        for key in ('return_normalizer._low', 'return_normalizer._high',
                    'critic.head.return_normalizer._low', 'critic.head.return_normalizer._high'):
            assert key in model.state_dict()
            assert _same(model.state_dict()[key], g['init/' + key]), key


def test_flat_critic_block_leaves_the_range_out():
    """FlatNetwork packs network_variables, which drops every `normalizer` parameter: the critic's flat block
    and its parameter count are those of the model without the Return normaliser."""
    from tonic_amd.environments import Box
    from tonic_amd.torch import models, normalizers
    counts = []
    for rn in (None, normalizers.Return(0.99)):
        torch.manual_seed(0)
        critic = models.Critic(encoder=models.ObservationEncoder(), torso=models.MLP((64, 64), torch.nn.Tanh),
                               head=models.ValueHead())
        critic.initialize(Box(-np.inf, np.inf, (17,)), Box(-1, 1, (6,)), None, rn)
        flat = models.FlatNetwork(critic, 'cpu')
        assert all('normalizer' not in n for n, p in critic.named_parameters()
                   if any(p is q for q in flat.params))
        counts.append((flat.count, flat.shapes(), flat.flat.clone()))
    assert counts[0][0] == counts[1][0] == 64 * 17 + 64 + 64 * 64 + 64 + 64 + 1
    assert counts[0][1] == counts[1][1]
    assert torch.equal(counts[0][2], counts[1][2])


def _reference_present():
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    try:
        import reference_loader
        return reference_loader.reference_available()
    finally:
        sys.path.pop(0)


@pytest.mark.skipif(not _reference_present(), reason='the reference checkout is not present')
def test_committed_goldens_equal_the_generator(tmp_path):
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'scripts', 'make_return_goldens.py'),
                           '--out', str(tmp_path)] + list(NAMES), stdout=subprocess.DEVNULL)
    for name in NAMES:
        want, got = np.load(os.path.join(GOLDEN, name + '.npz')), np.load(str(tmp_path / (name + '.npz')))
        assert sorted(want.files) == sorted(got.files), name
        for key in want.files:
            assert np.array_equal(want[key], got[key]), (name, key)
