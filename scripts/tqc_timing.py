"""What does a TQC learner iteration cost, and did serving it move SAC's?  Three figures on one MI355X, one fresh
process per run, the builds alternating (and who goes first), measured the way scripts/dmpo_timing.py does:

  a  the parent commit's SAC iteration on the split route (TONIC_AMD_FUSED_ITERATION=0: the updaters' own entries, the
     route TQC runs);
  b  the same on this commit;
  c  this commit's TQC iteration (25 quantiles per critic, 2 dropped per critic: the agent's defaults).

Each run: the agent's default (256, 256) torso, O = 17, A = 6, B = 256, one update call of 200 iterations captured as
a hipGraph; device events round 7 replays (new indices and draws each), microseconds per iteration, the median of the
7.  Checked when the figures are written: b's median inside the parent's own spread between its two processes (and
within the spread of a's windows of a's median).  c is reported beside them, not judged.

    python scripts/tqc_timing.py --parent <built checkout of the parent commit> [--rounds 2] [--out FILE]

A run that fails or runs out of time ends the whole measurement (nothing is started behind it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, A, W, B, M, ITERATIONS, WINDOWS = 17, 6, 16, 256, 25, 200, 7


def build(quantile):
    sys.path.insert(0, os.getcwd())              # (the tree the driver started this run in)
    import numpy as np
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    replay = tonic_amd.replays.Buffer(size=10 ** 5, batch_iterations=ITERATIONS, batch_size=B,
                                      steps_before_batches=0, steps_between_batches=1)
    agent = (tt.agents.TQC if quantile else tt.agents.SAC)(replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    assert agent.critic_updater.hidden == 256 and agent._u.route().fused_kind is None      # the split route
    assert getattr(agent.critic_updater, 'quantiles', 0) == (M if quantile else 0)
    rng = np.random.RandomState(0)
    for _ in range(400):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        agent.replay.store(normalizer=agent.model.observation_normalizer,
                           **{k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()})
    total = agent.replay.size * agent.replay.global_workers

    def draw():
        eps = rng.normal(size=(ITERATIONS, 2, B, A)).astype(np.float32)
        return rng.randint(0, total, size=(ITERATIONS, B)).astype(np.int64), eps
    return agent, draw, torch


def one_time(quantile):
    agent, draw, torch = build(quantile)
    for _ in range(2):                           # the capture and one replay
        agent.enqueue_update(*draw())
    torch.cuda.synchronize()
    assert agent._u.slot.graph is not None
    graph, windows = agent._u.slot.graph, []
    for _ in range(WINDOWS):
        first, eps = draw()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        infos = agent.enqueue_update(first, eps)
        end.record()
        end.synchronize()
        windows.append(start.elapsed_time(end) * 1e3 / ITERATIONS)
    assert agent._u.slot.graph is graph and bool(torch.isfinite(infos).all())
    print('RESULT ' + json.dumps(dict(quantile=quantile, iterations_per_window=ITERATIONS,
                                      us_per_iteration_windows=[round(w, 3) for w in windows],
                                      us_per_iteration=round(statistics.median(windows), 3))))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=('time',))
    parser.add_argument('--quantile', action='store_true')
    parser.add_argument('--parent')
    parser.add_argument('--rounds', type=int, default=2)
    parser.add_argument('--out', default='profiles/tqc_timing.json')
    args = parser.parse_args()
    if args.one == 'time':
        return one_time(args.quantile)
    trees = {'a': os.path.abspath(args.parent), 'b': ROOT, 'c': ROOT}

    def run(figure):
        command = [sys.executable, os.path.abspath(__file__), '--one', 'time']
        if figure == 'c':
            command.append('--quantile')
        env = dict(os.environ, TONIC_AMD_FUSED_ITERATION='0')
        env.pop('TONIC_AMD_NO_GRAPH', None)
        done = subprocess.run(command, cwd=trees[figure], env=env, capture_output=True, text=True, timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{figure}: exit status {done.returncode}')
        return json.loads([l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):])

    runs, summary = [], {}

    def write():
        result = dict(
            what='SAC (split route, TONIC_AMD_FUSED_ITERATION=0) and TQC learner iterations, (256, 256) torso, O = 17, '
                 'A = 6, B = 256, one MI355X, one fresh process per run, the builds alternating: a = the parent '
                 'commit\'s SAC, b = this commit\'s SAC, c = this commit\'s TQC (25 quantiles per critic, 2 dropped '
                 'per critic); microseconds per iteration, device events round 7 replays of a captured update call of '
                 f'{ITERATIONS} iterations, the median of the 7 per run',
            runs=runs, summary=summary)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as out:
            json.dump(result, out, indent=1)

    for round_ in range(1, args.rounds + 1):
        for figure in (('a', 'b', 'c') if round_ % 2 else ('c', 'b', 'a')):
            runs.append({**run(figure), 'figure': figure, 'round': round_})
            print(runs[-1], flush=True)
            write()
    windows = {f: [w for r in runs if r['figure'] == f for w in r['us_per_iteration_windows']] for f in 'abc'}
    medians = {f: statistics.median(w) for f, w in windows.items()}
    per_process = [r['us_per_iteration'] for r in runs if r['figure'] == 'a']
    spread = max(windows['a']) - min(windows['a'])
    summary.update(
        a_median=round(medians['a'], 3), a_min=round(min(windows['a']), 3), a_max=round(max(windows['a']), 3),
        a_spread=round(spread, 3), a_process_medians=per_process, b_median=round(medians['b'], 3),
        c_median=round(medians['c'], 3), b_minus_a=round(medians['b'] - medians['a'], 3),
        c_minus_b=round(medians['c'] - medians['b'], 3), c_over_b=round(medians['c'] / medians['b'], 4),
        b_within_a_spread_of_a=bool(abs(medians['b'] - medians['a']) <= spread),
        b_within_a_process_medians=bool(min(per_process) <= medians['b'] <= max(per_process)))
    write()
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
