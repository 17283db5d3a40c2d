"""REDQ beside SAC on the task of tests/test_gpu_learning.py (tests/reach_task.py: reward = 1 - mean((a - tanh(M obs))^2),
6 observations, 3 actions, 4 workers, 6000 steps, the Buffer and the exploration of its SAC case — so REDQ runs the
task's update-to-data ratio, SAC's, not its own default of 20): the mean training reward of every tenth of the run, one
fresh process per agent, the same seeds.  REDQ runs 5 critics, subsets of 2, entropy_coeff 0.2.  A record, not a test:
no threshold is asserted.

    python scripts/redq_reach.py [--out profiles/redq_reach.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def one(name):
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    import reach_task
    replay = tonic_amd.replays.Buffer(**reach_task.BUFFER)
    exploration = tonic_amd.explorations.NoActionNoise(start_steps=reach_task.START_STEPS)
    agent = getattr(tt.agents, name)(replay=replay, exploration=exploration)
    with tempfile.TemporaryDirectory() as path:
        curve = reach_task.train(tonic_amd, agent, 'SAC', path)
    torch.cuda.synchronize()
    print('RESULT ' + json.dumps(dict(agent=name, mean_reward_per_tenth=[round(v, 4) for v in curve])))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=('SAC', 'REDQ'))
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'redq_reach.json'))
    args = parser.parse_args()
    if args.one:
        return one(args.one)
    runs = []
    for name in ('SAC', 'REDQ'):
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', name], capture_output=True,
                              text=True, timeout=400)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{name}: exit status {done.returncode}')
        runs.append(json.loads([l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):]))
        print(runs[-1], flush=True)
    with open(args.out, 'w') as out:
        json.dump(dict(what='mean training reward of every tenth of 6000 steps on tests/reach_task.py (6 observations, '
                            '3 actions, 4 workers, B = 100, 20 iterations per update, 1-step returns, discount 0.9), '
                            'seeds as tests/test_gpu_learning.py; REDQ: 5 critics, subsets of 2, on the task\'s Buffer '
                            '(SAC\'s update-to-data ratio); one fresh process per agent, one run each; no threshold '
                            'asserted',
                       runs=runs), out, indent=1)


if __name__ == '__main__':
    main()
