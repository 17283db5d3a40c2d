"""What does SAC's learned entropy coefficient cost per learner iteration, and did adding it move the fixed-coefficient
split iteration?  Three figures on one MI355X, one fresh process per run, the builds alternating (and who goes first):

  a  the parent commit's split-entry SAC iteration at the fixed coefficient (TONIC_AMD_FUSED_ITERATION=0);
  b  the same on this commit;
  c  this commit's iteration with `entropy_coeff_updater=EntropyCoeffTuning()` (the tempered entries + the
     coefficient's optimizer step).

Each run: SAC on the default (256, 256) torso, O = 17, A = 6, one update call of 200 iterations captured as a hipGraph;
device events round 7 replays (new indices and noise each), microseconds per iteration, the median of the 7.  `count`
runs count the kernel launches of an eager iteration with torch.profiler (the difference between update calls of 20
and of 10 iterations, over 10; everything the profiler sees on the stream, the replay's gather included), where the
profiler is available.  Bounds, checked when the figures are written: b's median within the spread (max - min) of a's own
windows of a's median; c above b by no more than the share of the launches it adds plus that spread.

    python scripts/entropy_coeff_timing.py --parent <built checkout of the parent commit> [--rounds 2] [--out FILE]

A run that fails or runs out of time ends the whole measurement (nothing is started behind it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, A, ITERATIONS, WINDOWS = 17, 6, 200, 7


def build(batch, tuned, iterations):
    sys.path.insert(0, os.getcwd())              # (the tree the driver started this run in)
    import numpy as np
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    replay = tonic_amd.replays.Buffer(size=20000, batch_iterations=iterations, batch_size=batch, steps_before_batches=0,
                                      steps_between_batches=1)
    more = dict(entropy_coeff_updater=tt.updaters.EntropyCoeffTuning()) if tuned else {}
    agent = tt.agents.SAC(replay=replay, **more)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    assert agent._u.route().fused_kind is None, 'the split entries are what is timed'
    rng, W = np.random.RandomState(0), 16
    for _ in range(200):
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        agent.replay.store(normalizer=agent.model.observation_normalizer,
                           **{k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in row.items()})
    total = agent.replay.size * agent.replay.global_workers

    def draw(count):
        return (rng.randint(0, total, size=(count, batch)).astype(np.int64),
                rng.normal(size=(count, 2, batch, A)).astype(np.float32))
    return agent, draw, torch


def one_time(batch, tuned):
    agent, draw, torch = build(batch, tuned, ITERATIONS)
    for _ in range(2):                           # the capture and one replay
        agent.enqueue_update(*draw(ITERATIONS))
    torch.cuda.synchronize()
    assert agent._u.slot.graph is not None
    graph, windows = agent._u.slot.graph, []
    for _ in range(WINDOWS):
        indices, eps = draw(ITERATIONS)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        infos = agent.enqueue_update(indices, eps)
        end.record()
        end.synchronize()
        windows.append(start.elapsed_time(end) * 1e3 / ITERATIONS)
    assert agent._u.slot.graph is graph and bool(torch.isfinite(infos).all())
    print('RESULT ' + json.dumps(dict(batch=batch, tuned=tuned, iterations_per_window=ITERATIONS,
                                      us_per_iteration_windows=[round(w, 3) for w in windows],
                                      us_per_iteration=round(statistics.median(windows), 3))))


def one_count(batch, tuned):
    """Kernel launches per eager iteration; null when the profiler gives no device events here."""
    agent, draw, torch = build(batch, tuned, 20)
    agent.enqueue_update(*draw(10), graph=False)
    torch.cuda.synchronize()
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        counted = []
        for count in (10, 20):
            arguments = draw(count)
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as trace:
                agent.enqueue_update(*arguments, graph=False)
                torch.cuda.synchronize()
            kernels = [e for e in trace.events() if str(e.device_type).endswith('CUDA') and 'emcpy' not in e.name
                       and 'emset' not in e.name]
            counted.append(len(kernels))
        if counted[0] > 0:
            launches = (counted[1] - counted[0]) / 10
    except Exception as error:                   # noqa: BLE001 (a profiler that is not there is not a failure of the run)
        print('profiler unavailable:', error)
    print('RESULT ' + json.dumps(dict(batch=batch, tuned=tuned, launches_per_iteration=launches)))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=('time', 'count'))
    parser.add_argument('--batch', type=int, default=256)
    parser.add_argument('--tuned', action='store_true')
    parser.add_argument('--parent')
    parser.add_argument('--rounds', type=int, default=2)
    parser.add_argument('--out', default='profiles/entropy_coeff_timing.json')
    args = parser.parse_args()
    if args.one == 'time':
        return one_time(args.batch, args.tuned)
    if args.one == 'count':
        return one_count(args.batch, args.tuned)
    trees = {'a': os.path.abspath(args.parent), 'b': ROOT, 'c': ROOT}

    def run(figure, batch, what='time'):
        command = [sys.executable, os.path.abspath(__file__), '--one', what, '--batch', str(batch)]
        if figure == 'c':
            command.append('--tuned')
        env = dict(os.environ, TONIC_AMD_FUSED_ITERATION='0')
        env.pop('TONIC_AMD_NO_GRAPH', None)
        done = subprocess.run(command, cwd=trees[figure], env=env, capture_output=True, text=True, timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{figure} B={batch} {what}: exit status {done.returncode}')
        return json.loads([l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):])

    runs, summary, launches = [], {}, {}

    def write():
        result = dict(
            what='SAC learner iteration on the split entries (TONIC_AMD_FUSED_ITERATION=0), (256, 256) torso, O = 17, '
                 'A = 6, one MI355X, one fresh process per run, the builds alternating: a = the parent commit at the '
                 'fixed coefficient, b = this commit at the fixed coefficient, c = this commit with '
                 'EntropyCoeffTuning; microseconds per iteration, device events round 7 replays of a captured update '
                 f'call of {ITERATIONS} iterations, the median of the 7 per run',
            launches_per_iteration=launches, runs=runs, summary=summary)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as out:
            json.dump(result, out, indent=1)

    for figure in ('b', 'c'):
        launches[figure] = run(figure, 256, 'count')['launches_per_iteration']
    write()
    for batch in (256, 1024):
        for round_ in range(1, args.rounds + 1):
            for figure in (('a', 'b', 'c') if round_ % 2 else ('c', 'b', 'a')):
                runs.append({**run(figure, batch), 'figure': figure, 'round': round_})
                print(runs[-1], flush=True)
                write()
        windows = {f: [w for r in runs if (r['figure'], r['batch']) == (f, batch) for w in r['us_per_iteration_windows']]
                   for f in 'abc'}
        medians = {f: statistics.median(w) for f, w in windows.items()}
        spread = max(windows['a']) - min(windows['a'])
        added = (launches['c'] - launches['b']) / launches['b'] if launches['b'] and launches['c'] else 1 / 13
        summary[f'B={batch}'] = dict(
            a_median=round(medians['a'], 3), a_min=round(min(windows['a']), 3), a_max=round(max(windows['a']), 3),
            a_spread=round(spread, 3), b_median=round(medians['b'], 3), c_median=round(medians['c'], 3),
            b_minus_a=round(medians['b'] - medians['a'], 3), c_over_b=round(medians['c'] / medians['b'], 4),
            added_launch_share=round(added, 4),
            b_within_a_spread_of_a=bool(abs(medians['b'] - medians['a']) <= spread),
            c_within_added_launches_plus_spread=bool(medians['c'] <= medians['b'] * (1 + added) + spread))
        write()
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
