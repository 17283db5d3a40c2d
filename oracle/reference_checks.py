"""Checks against the REFERENCE's own code, run by hand where a reference checkout is present (they are not
part of the test suite, which holds this package against the fixtures in tests/golden/ instead):

    TONIC_REFERENCE_ROOT=<reference checkout> python -m pytest oracle/reference_checks.py

`tonic.train.train()` drives an agent of this package and the learner statistics land in the reference's
log.csv; the learning-curve fixture and every committed golden are what the unmodified reference computes
now (oracle/make_learning_curves.py, oracle/make_golden.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle'), ROOT):
    if path not in sys.path:
        sys.path.insert(0, path)
import reference_loader  # noqa: E402

pytestmark = pytest.mark.skipif(not reference_loader.reference_available(),
                                reason='needs the reference checkout (TONIC_REFERENCE_ROOT)')

PPO_KEYS = ('actor/loss', 'actor/kl', 'actor/entropy', 'actor/clip_fraction', 'actor/std',
            'actor/stop', 'actor/iterations', 'critic/loss', 'critic/v', 'critic/iterations')


def test_reference_train_logs_this_packages_learner_keys(tmp_path, monkeypatch):
    """tonic/train.py:76-133 end to end with `--header 'import tonic_amd as amd'`: the agent logs
    through tonic_amd.logger, the reference initialised tonic.logger — one log.csv, one
    checkpoint folder, under the reference's environment/name/seed path."""
    tonic = reference_loader.load_reference()
    import tonic.train
    import tonic_amd
    from tonic_amd.utils import logger as amd_logger
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(amd_logger, 'current_logger', None)        # nobody initialised ours
    monkeypatch.setattr(tonic.logger, 'current_logger', None)
    tonic.train.train(
        header='import tonic_amd as amd, tonic_amd.torch, stub_agents',
        agent='stub_agents.LoggingOnlyPPO(update_every=8, iterations=3)',
        environment='__import__("tonic_amd").environments.Synthetic(5, 2, max_episode_steps=7)',
        test_environment=None,
        trainer='tonic.Trainer(steps=96, epoch_steps=48, save_steps=96, show_progress=False)',
        before_training=None, after_training=None, parallel=1, sequential=4, seed=3,
        name=None, environment_name=None, checkpoint='last', path=None)
    run = tmp_path / 'synthetic-5-2' / 'LoggingOnlyPPO-1x4' / '3'
    header = (run / 'log.csv').read_text().split('\n')[0].split(',')
    for key in PPO_KEYS + ('train/episode_score/mean', 'test/episode_score/mean',
                           'train/steps_per_second'):
        assert key in header, (key, header)
    assert (run / 'config.yaml').exists()
    assert (run / 'checkpoints' / 'step_96.pt').exists()
    assert amd_logger.current_logger is None, 'the reference logger must stay the only one'
    rows = (run / 'log.csv').read_text().strip().split('\n')
    assert len(rows) == 3                                           # header + two epochs


def test_this_packages_trainer_under_the_reference_logger(tmp_path, monkeypatch):
    """`--trainer 'amd.Trainer(...)'` with the reference's logger: same single log."""
    tonic = reference_loader.load_reference()
    import tonic.train
    from tonic_amd.utils import logger as amd_logger
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(amd_logger, 'current_logger', None)
    monkeypatch.setattr(tonic.logger, 'current_logger', None)
    tonic.train.train(
        header='import tonic_amd as amd, tonic_amd.torch, stub_agents',
        agent='stub_agents.LoggingOnlyPPO(update_every=8, iterations=3)',
        environment='__import__("tonic_amd").environments.Synthetic(5, 2, max_episode_steps=7)',
        test_environment=None,
        trainer='amd.Trainer(steps=96, epoch_steps=48, save_steps=96, show_progress=False)',
        before_training=None, after_training=None, parallel=1, sequential=4, seed=3,
        name='run', environment_name='env', checkpoint='last', path=None)
    header = (tmp_path / 'env' / 'run' / '3' / 'log.csv').read_text().split('\n')[0].split(',')
    for key in PPO_KEYS + ('train/episode_score/mean', 'test/episode_length/mean'):
        assert key in header, key
    assert (tmp_path / 'env' / 'run' / '3' / 'checkpoints' / 'step_96.pt').exists()


def test_install_puts_the_collector_under_the_reference_cli(tmp_path, monkeypatch):
    """`tonic_amd.install()` from the header: the reference's train() then builds its
    environments with this package's distribute (forked workers writing into the shared block)
    and the agent receives the block's views."""
    tonic = reference_loader.load_reference()
    import tonic.train
    import stub_agents
    from tonic_amd.utils import logger as amd_logger
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(amd_logger, 'current_logger', None)
    monkeypatch.setattr(tonic.logger, 'current_logger', None)
    monkeypatch.setattr(tonic.environments, 'distribute', tonic.environments.distribute)
    seen = []
    original = stub_agents.LoggingOnlyPPO.update

    def spy(self, *args, **kwargs):
        seen.append(self.saw_block_views)
        return original(self, *args, **kwargs)
    monkeypatch.setattr(stub_agents.LoggingOnlyPPO, 'update', spy)
    tonic.train.train(
        header='import tonic_amd as amd, tonic_amd.torch, stub_agents; amd.install()',
        agent='stub_agents.LoggingOnlyPPO(update_every=8, iterations=3)',
        environment='__import__("tonic_amd").environments.Synthetic(5, 2, max_episode_steps=7)',
        test_environment=None,
        trainer='tonic.Trainer(steps=48, epoch_steps=48, save_steps=48, show_progress=False)',
        before_training=None, after_training=None, parallel=2, sequential=3, seed=3,
        name='run', environment_name='env', checkpoint='last', path=None)
    assert seen and all(seen), 'the agent must be handed views of the shared block'
    assert (tmp_path / 'env' / 'run' / '3' / 'log.csv').exists()


def test_learning_curve_fixture_is_what_the_reference_does(tmp_path):
    """tests/golden/learning_curves.json (what tests/test_gpu_learning.py holds this package's agents
    against) is regenerated for one cheap case by training the unmodified reference here, and must
    come out identical: the fixture is pinned on the reference, not on a past run of this package."""
    import json
    import reach_task
    tonic = reference_loader.load_reference()
    import tonic.torch
    import torch
    torch.set_num_threads(8)                    # as oracle/make_learning_curves.py
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'learning_curves.json')))
    assert set(golden['curves']) == set(reach_task.CASES)
    agent = reach_task.build_agent(tonic, tonic.torch.agents, 'A2C')
    curve = reach_task.train(tonic, agent, 'A2C', str(tmp_path))
    np.testing.assert_allclose(curve, golden['curves']['A2C'], rtol=0, atol=1e-6)


def test_committed_goldens_are_what_their_generator_writes(tmp_path):
    """oracle/make_golden.py run NOW on the unmodified reference (in a subprocess: one torch
    thread, its own generator state) writes exactly tests/golden/*.npz — same keys, same bits.
    A generator that gained a field (or a reference / torch build that computes something else)
    fails here instead of leaving the committed fixtures silently behind."""
    import subprocess
    root = ROOT
    code = ('import sys; sys.path.insert(0, %r); import make_golden; make_golden.OUT = %r; '
            'sys.argv = sys.argv[:1]; make_golden.main()'
            % (os.path.join(root, 'oracle'), str(tmp_path)))
    subprocess.run([sys.executable, '-c', code], check=True, capture_output=True, timeout=600)
    committed = os.path.join(root, 'tests', 'golden')
    fresh = sorted(f for f in os.listdir(tmp_path) if f.endswith('.npz'))
    assert fresh == sorted(f for f in os.listdir(committed) if f.endswith('.npz'))
    for name in fresh:
        got = np.load(os.path.join(tmp_path, name), allow_pickle=True)
        want = np.load(os.path.join(committed, name), allow_pickle=True)
        assert sorted(got.files) == sorted(want.files), name
        for key in got.files:
            a, b = got[key], want[key]
            same = (np.array_equal(a, b, equal_nan=True) if a.dtype.kind in 'fc'
                    else np.array_equal(a, b))
            assert same, (name, key)
