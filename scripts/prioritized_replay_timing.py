"""What does prioritized replay cost per D4PG learner iteration, and did adding its route move the uniform one?  Three
figures on one MI355X, one fresh process per run, the builds alternating (and who goes first):

  a  the parent commit's D4PG iteration on the uniform `Buffer`;
  b  the same on this commit;
  c  this commit's iteration on a `PrioritizedBuffer` with a capacity of 10^6 transitions: per iteration the sample,
     a gather of its own, the weighted critic step, the priority update (and the actor step) instead of one gather
     for the whole call in front of the iterations.

Each run: D4PG on the default (256, 256) torso and 51 atoms, O = 17, A = 6, one update call of 200 iterations captured
as a hipGraph; device events round 7 replays (new indices or uniforms each), microseconds per iteration, the median of
the 7.  At B = 100 and 256.  Checked when the figures are written: b's median within the spread (max - min) of a's own
windows of a's median.  c is reported with its difference from b and that difference's share of c, not gated.

    python scripts/prioritized_replay_timing.py --parent <built checkout of the parent commit> [--rounds 2] [--out FILE]

A run that fails or runs out of time ends the whole measurement (nothing is started behind it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, A, W, ITERATIONS, WINDOWS, CAPACITY = 17, 6, 16, 200, 7, 10 ** 6


def build(batch, prioritized):
    sys.path.insert(0, os.getcwd())              # (the tree the driver started this run in)
    import numpy as np
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    kind = tonic_amd.replays.PrioritizedBuffer if prioritized else tonic_amd.replays.Buffer
    replay = kind(size=CAPACITY, return_steps=5, batch_iterations=ITERATIONS, batch_size=batch, steps_before_batches=0,
                  steps_between_batches=1)
    agent = tt.agents.D4PG(replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    assert agent._u.route().fused_kind is None and agent.critic_updater.hidden == 256
    rng = np.random.RandomState(0)
    for _ in range(400):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        agent.replay.store(normalizer=agent.model.observation_normalizer,
                           **{k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()})
    total = agent.replay.size * agent.replay.global_workers
    if prioritized:
        assert agent.replay.capacity == CAPACITY // W * W

    def draw():
        eps = np.zeros((ITERATIONS, 1, batch, A), np.float32)
        if prioritized:
            return rng.random_sample((ITERATIONS, batch)), eps
        return rng.randint(0, total, size=(ITERATIONS, batch)).astype(np.int64), eps
    return agent, draw, torch


def one_time(batch, prioritized):
    agent, draw, torch = build(batch, prioritized)
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
    if prioritized:
        drawn = agent._u.slot.indices.cpu().numpy()
        assert drawn.min() >= 0 and drawn.max() < agent.replay.size * W
    print('RESULT ' + json.dumps(dict(batch=batch, prioritized=prioritized, iterations_per_window=ITERATIONS,
                                      us_per_iteration_windows=[round(w, 3) for w in windows],
                                      us_per_iteration=round(statistics.median(windows), 3))))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=('time',))
    parser.add_argument('--batch', type=int, default=256)
    parser.add_argument('--prioritized', action='store_true')
    parser.add_argument('--parent')
    parser.add_argument('--rounds', type=int, default=2)
    parser.add_argument('--out', default='profiles/prioritized_replay_timing.json')
    args = parser.parse_args()
    if args.one == 'time':
        return one_time(args.batch, args.prioritized)
    trees = {'a': os.path.abspath(args.parent), 'b': ROOT, 'c': ROOT}

    def run(figure, batch):
        command = [sys.executable, os.path.abspath(__file__), '--one', 'time', '--batch', str(batch)]
        if figure == 'c':
            command.append('--prioritized')
        env = dict(os.environ)
        env.pop('TONIC_AMD_NO_GRAPH', None)
        done = subprocess.run(command, cwd=trees[figure], env=env, capture_output=True, text=True, timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{figure} B={batch}: exit status {done.returncode}')
        return json.loads([l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):])

    runs, summary = [], {}

    def write():
        result = dict(
            what='D4PG learner iteration, (256, 256) torso, 51 atoms, O = 17, A = 6, 5-step returns, one MI355X, one '
                 'fresh process per run, the builds alternating: a = the parent commit on the uniform Buffer, b = this '
                 'commit on the uniform Buffer, c = this commit on a PrioritizedBuffer with a capacity of 10^6 '
                 'transitions (sample, single-batch gather, weighted critic step, priority update per iteration); '
                 'microseconds per iteration, device events round 7 replays of a captured update call of '
                 f'{ITERATIONS} iterations, the median of the 7 per run',
            runs=runs, summary=summary)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as out:
            json.dump(result, out, indent=1)

    for batch in (100, 256):
        for round_ in range(1, args.rounds + 1):
            for figure in (('a', 'b', 'c') if round_ % 2 else ('c', 'b', 'a')):
                runs.append({**run(figure, batch), 'figure': figure, 'round': round_})
                print(runs[-1], flush=True)
                write()
        windows = {f: [w for r in runs if (r['figure'], r['batch']) == (f, batch) for w in r['us_per_iteration_windows']]
                   for f in 'abc'}
        medians = {f: statistics.median(w) for f, w in windows.items()}
        spread = max(windows['a']) - min(windows['a'])
        summary[f'B={batch}'] = dict(
            a_median=round(medians['a'], 3), a_min=round(min(windows['a']), 3), a_max=round(max(windows['a']), 3),
            a_spread=round(spread, 3), b_median=round(medians['b'], 3), c_median=round(medians['c'], 3),
            b_minus_a=round(medians['b'] - medians['a'], 3), c_minus_b=round(medians['c'] - medians['b'], 3),
            prioritized_share_of_c=round((medians['c'] - medians['b']) / medians['c'], 4),
            b_within_a_spread_of_a=bool(abs(medians['b'] - medians['a']) <= spread))
        write()
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
