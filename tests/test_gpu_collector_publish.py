"""What a rollout leaves behind does not depend on how the host publishes a step (csrc/collector.hip
tonic_collector_synthetic_step): one rollout through SyntheticBatch and the PPO agent with the
push transport (rows and command stored into the device window, in chunks), the same rollout with
TONIC_AMD_COLLECTOR_PUSH=0 (the resident kernel pulls them from the block) and a third one whose simulator is
handed a COPY of the actions (the NumPy path of SyntheticBatch.step; the block-level ring publishes the rows) must
agree bit for bit.  One collector per process: every run is a fresh child (this file run as a script) under its
own time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, A, T = 17, 6, 32
FIELDS = ('observations', 'next_observations', 'actions', 'log_probs', 'rewards')
MODES = ('push', 'pull', 'copied_actions')


def rollout(mode, W, path):
    """The child: T steps, the learner update of the T-th included (it closes the rollout: the last outcome row
    and the normaliser's sums are final), then the Segment and the sums as the update found them -> path."""
    sys.path.insert(0, ROOT)
    import torch
    import tonic_amd
    import tonic_amd.torch
    from tonic_amd import environments
    env = environments.SyntheticBatch(W, O, A, max_episode_steps=1000, pool=4)
    env.initialize(seed=5)
    agent = tonic_amd.torch.agents.PPO(replay=tonic_amd.replays.Segment(size=T, batch_iterations=1))
    agent.initialize(env.observation_space, env.action_space, seed=7)
    norm = agent.model.observation_normalizer
    kept = {}
    update = norm.update

    def update_and_keep():
        kept['normalizer_sums'] = norm.device_sums.cpu().numpy().copy()
        kept['normalizer_rows'] = np.array([norm.new_count])
        for key in FIELDS:
            kept[key] = agent.replay.buffers[key].cpu().numpy().copy()
        return update()
    norm.update = update_and_keep
    observations = env.start()
    for t in range(T):
        actions = agent.step(observations, t * W)
        observations, infos = env.step(actions.copy() if mode == 'copied_actions' else actions)
        agent.update(**infos, steps=t * W)
    torch.cuda.synchronize()
    kept['transport'] = np.array([agent.transport_in_effect])
    kept['issued_by_environment'] = np.array([agent.steps_issued_by_environment])
    kept['normalizer_mean'], kept['normalizer_std'] = norm.mean, norm.std
    agent.close()
    np.savez(path, **kept)


@pytest.mark.gpu
@pytest.mark.parametrize('W', (1, 16, 17, 33))
def test_a_rollout_is_bit_identical_however_the_step_is_published(W, tmp_path):
    children = {}
    for mode in MODES:
        env = dict(os.environ)
        env.pop('TONIC_AMD_COLLECTOR_PUSH', None)
        env.pop('TONIC_AMD_COLLECTOR_TRANSPORT', None)
        if mode == 'pull':
            env['TONIC_AMD_COLLECTOR_PUSH'] = '0'
        children[mode] = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), mode, str(W), str(tmp_path / (mode + '.npz'))],
            cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    failed = []
    for mode, child in children.items():
        try:
            output, _ = child.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            child.kill()
            output, _ = child.communicate()
            failed.append(f'{mode}: no end within 120 s\n{output[-2000:]}')
            continue
        if child.returncode != 0:
            failed.append(f'{mode}: exit status {child.returncode}\n{output[-2000:]}')
    assert not failed, '\n'.join(failed)
    runs = {mode: np.load(tmp_path / (mode + '.npz')) for mode in MODES}
    push = runs['push']
    assert int(runs['pull']['transport'][0]) == 2
    assert int(push['transport'][0]) == 3 and int(runs['copied_actions']['transport'][0]) == 3, \
        'the push transport is not in effect: the comparison would be the pull transport with itself'
    # (the synthetic step issued the armed commands itself only where it was handed the block's own actions)
    assert int(push['issued_by_environment'][0]) >= T // 2 and int(runs['pull']['issued_by_environment'][0]) >= T // 2
    assert int(push['normalizer_rows'][0]) == T * W
    assert np.isfinite(push['rewards']).all() and push['rewards'].any() and push['observations'].any()
    for mode in ('pull', 'copied_actions'):
        for key in FIELDS + ('normalizer_sums', 'normalizer_rows', 'normalizer_mean', 'normalizer_std'):
            assert push[key].tobytes() == runs[mode][key].tobytes(), (mode, key)


if __name__ == '__main__':
    rollout(sys.argv[1], int(sys.argv[2]), sys.argv[3])
