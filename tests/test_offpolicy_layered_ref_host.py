"""CPU tests of what tests/test_gpu_offpolicy_layered_edges.py stands on (tests/offpolicy_layered_ref.py), without a
GPU and without an agent:

- the float64 restatement (Ref.policy, Ref.critic of test_gpu_offpolicy_grads.py: 1 .. 4 layers, ReLU / Tanh / ELU,
  the normaliser on the critics' inputs only) against the stock torch modules' own forward in float64, within 1e-12,
  on every network of every case's model — the reference is pinned independently of the kernels;
- the seed search: every case finds inputs that meet its preconditions within the cap, and the seeds fixed in the
  file are the search's own."""
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import offpolicy_layered_ref as layered                                     # noqa: E402
from test_gpu_offpolicy_grads import Ref, _f64                              # noqa: E402

IDS = [layered.case_id(c) for c in layered.CASES]


def _close(got, want, name):
    scale = max(float(want.abs().max()), 1.0)
    assert float((got - want).abs().max()) <= 1e-12 * scale, (name, float((got - want).abs().max()), scale)


@pytest.mark.parametrize('case', layered.CASES, ids=IDS)
def test_restatement_equals_the_stock_modules_in_float64(case):
    model = layered.build_model(case)
    inputs = layered.draw(case, layered.seed_of(case), model)
    layered.install(model, inputs)
    ref = Ref(types.SimpleNamespace(model=model), case.kind, len(case.sizes), case.activation)
    leaves = {name: _f64(net) for name, net in model.named_children() if 'normalizer' not in name}
    assert len(leaves) == len(layered.networks(model))
    model.double()
    rng = np.random.RandomState(1)
    obs = torch.as_tensor(rng.normal(size=(case.B, case.O)) * 2)
    act = torch.as_tensor(rng.uniform(-1, 1, (case.B, case.A)))
    assert obs.dtype == torch.float64
    with torch.no_grad():
        for name, net in model.named_children():
            if 'normalizer' in name:
                continue
            if 'actor' in name:
                stock, (loc, scale) = net(obs), ref.policy(leaves[name], obs)
                if case.kind in ('sac', 'mpo'):
                    normal = stock._distribution if case.kind == 'sac' else stock
                    _close(loc, normal.mean, name + ' loc')
                    _close(scale, normal.stddev, name + ' scale')
                else:
                    assert scale is None
                    _close(loc, stock, name)
            else:
                stock, got = net(obs, act), ref.critic(leaves[name], obs, act)
                _close(got, stock.logits if case.family == 'd4pg' else stock, name)
                assert got.shape == ((case.B, case.NA) if case.family == 'd4pg' else (case.B,))


@pytest.mark.parametrize('case', layered.CASES, ids=IDS)
def test_seed_search_ends_within_its_cap_on_the_fixed_seed(case):
    seed = layered.search(case)
    assert seed < layered.SEARCH_CAP and seed == layered.seed_of(case), (seed, layered.seed_of(case))


def test_case_table():
    """Every case once, no seed fixed for a case that does not exist, and the axes the table is meant to hold."""
    assert len(set(IDS)) == len(IDS) and set(layered.SEEDS) <= set(IDS)
    q = [c for c in layered.Q_CASES]
    assert {c.B for c in q if c.sizes == (40, 24)} == {1, 15, 16, 17, 100, 1100}
    assert {(c.O, c.A) for c in q if c.sizes == (48, 40, 32)} == set(layered.INPUT_AXIS)
    assert {c.kind for c in q if c.sizes == (4095,)} == {'td3'} and {c.kind for c in q if c.B == 1100} == {'td3', 'sac'}
    assert sum(layered.plain(c) for c in q) == 4 * 3
    assert (len(layered.Q_CASES), len(layered.D4PG_CASES), len(layered.SARSA_CASES), len(layered.MPO_CASES)) == \
        (72, 24, 8, 16)
