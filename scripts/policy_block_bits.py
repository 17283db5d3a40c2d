"""The sha256 of everything three rollouts and updates of PPO, A2C and TRPO leave behind on the collector path
(tonic_amd.policy_block, tonic_amd.critic_chain) at (O, A, W, T) = (6, 3, 12, 10) over Sequential, Parallel and
SyntheticBatch, with test episodes, one step on foreign observations and one outcome in foreign arrays in between as in
tests/test_gpu_collector.py (PPO with TONIC_AMD_CRITIC_OVERLAP=0 and =1): every step's actions, the Segment's buffers at
each rollout's end, every logged value in order, the final state_dict.  One JSON object on stdout; two checkouts on
the same library compute the same bits exactly when their outputs are identical:

    PROBE_LIBRARY=<a libtonic_hip.so> python scripts/policy_block_bits.py > bits.json

(PROBE_LIBRARY as in scripts/determinism_probe.py; unset: this checkout's library.)  One fresh process per checkout."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tonic_amd import _lib   # noqa: E402

if os.environ.get('PROBE_LIBRARY'):            # a variant build of the library (developer)
    _lib.LIBRARY_PATH = os.environ['PROBE_LIBRARY']
import numpy as np           # noqa: E402
import torch                 # noqa: E402
import tonic_amd             # noqa: E402
import tonic_amd.torch       # noqa: E402
from tonic_amd import environments          # noqa: E402
from tonic_amd.utils import logger          # noqa: E402

O, A, W, T = 6, 3, 12, 10
SEGMENT = ('observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations', 'log_probs')


def sha(array):
    return hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()


def environment(kind):
    if kind == 'batch':
        return environments.SyntheticBatch(W, O, A, max_episode_steps=7, pool=5)
    groups = 2 if kind == 'parallel' else 1
    return environments.distribute(lambda: environments.Synthetic(O, A, max_episode_steps=4), groups, W // groups)


def run(agent_name, kind, overlap):
    os.environ['TONIC_AMD_CRITIC_OVERLAP'] = overlap
    logged = []
    logger.get_current_logger().store = lambda key, value, *a, **k: logged.append(
        (key, sha(np.asarray(value, np.float64))))
    env = environment(kind)
    env.initialize(seed=3)
    agent = getattr(tonic_amd.torch.agents, agent_name)(replay=tonic_amd.replays.Segment(size=T, batch_iterations=2))
    agent.initialize(env.observation_space, env.action_space, seed=9)
    segments, update = [], agent._update

    def recording_update():
        torch.cuda.synchronize()
        segments.append({k: sha(agent.replay.buffers[k].cpu().numpy()) for k in SEGMENT})
        update()
    agent._update = recording_update
    observations = env.start()
    test_obs = np.random.RandomState(1).standard_normal((2, O)).astype(np.float32)
    actions_of, tests = [], []
    for t in range(3 * T + 3):
        if t == 5:                                   # foreign observations: a copy of the block's
            observations = observations.copy()
        actions = agent.step(observations, t * W)
        actions_of.append(sha(actions))
        observations, infos = env.step(actions)
        if t == 15:                                  # foreign infos after the environment rang
            infos = {k: v.copy() for k, v in infos.items()}
        if t == 17:                                  # a test episode between step and update
            tests.append(sha(agent.test_step(test_obs, t * W)))
        agent.update(**infos, steps=t * W)
        if t in (2, 7, 13, 24):                      # test episodes between update and step
            tests.append(sha(agent.test_step(test_obs, t * W)))
    torch.cuda.synchronize()
    state = {k: sha(v.detach().cpu().numpy()) for k, v in agent.model.state_dict().items()}
    issued = int(agent.steps_issued_by_environment)
    overlapped = getattr(agent, '_critic_stream', None) is not None
    agent.close()
    if hasattr(env, 'close'):
        env.close()
    assert len(segments) == 3
    return dict(actions=actions_of, test_actions=tests, segments=segments, logged=logged, state=state,
                steps_issued_by_environment=issued, critic_under_next_rollout=overlapped)


def main():
    bits = {}
    for agent_name, overlaps in (('PPO', ('0', '1')), ('A2C', ('1',)), ('TRPO', ('1',))):
        for kind in ('sequential', 'parallel', 'batch'):
            for overlap in overlaps:
                name = f'{agent_name}/{kind}' + (f'/overlap{overlap}' if agent_name == 'PPO' else '')
                bits[name] = run(agent_name, kind, overlap)
                print(name, 'done', file=sys.stderr, flush=True)
    json.dump(dict(abi=int(_lib.load().tonic_abi_version()), runs=len(bits), sha256=bits), sys.stdout, indent=0)
    print()


if __name__ == '__main__':
    main()
