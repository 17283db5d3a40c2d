"""What does TQC on an ensemble of critics cost, and did serving it move the twin agent's iteration?  Figures on one
MI355X, one fresh process per run, two processes per figure, the order reversed in the second round, measured the way
scripts/tqc_timing.py does:

  a   the parent commit's TQC iteration (the twin model: 2 critics of 25 quantiles, 2 dropped per critic);
  b   the same on this commit (the twin entries: the same launches);
  e2  this commit's ensemble entries at N = 2 (models.ActorCriticEnsembleWithTargets, the same 25 / 2);
  e5  the ensemble at N = 5: the paper's configuration;
  k   the ensemble critic loss kernel alone (tonic_debug_ensemble_quantile_loss) at B = 256 and N M = 50 (2 x 25, one
      value per lane), 125 (5 x 25, two) and 256 (8 x 32, four), 2 dropped per critic;
  pe2, pe5, pk   e2, e5 and k on the parent commit, by the parent's own copy of this script (its developer entry may
      take other arguments).

a .. e5: the agent's default (256, 256) torso, O = 17, A = 6, B = 256, one update call of 200 iterations captured as a
hipGraph; device events round 7 replays (new indices and draws each), microseconds per iteration, the median of the 7.
k: 200 launches captured as one graph, device events round 7 replays, microseconds per launch.  Checked when the figures
are written: b's median inside the range of the parent's own windows, and inside the spread between its two processes;
each kernel figure inside the range of the parent's windows.  The rest is reported, not judged.

    python scripts/tqc_ensemble_timing.py --parent <built checkout of the parent commit> [--rounds 2] [--out FILE]

A run that fails or runs out of time ends the whole measurement (nothing is started behind it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, A, W, B, M, DROP, ITERATIONS, WINDOWS = 17, 6, 16, 256, 25, 2, 200, 7
KERNEL_POOLS = ((2, 25), (5, 25), (8, 32))              # (N, M): N M = 50, 125, 256


def build(critics):
    """critics = 0: agents.TQC() as it comes (the twin model); N >= 2: the ensemble model of N critics."""
    sys.path.insert(0, os.getcwd())              # (the tree the driver started this run in)
    import numpy as np
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    replay = tonic_amd.replays.Buffer(size=10 ** 5, batch_iterations=ITERATIONS, batch_size=B,
                                      steps_before_batches=0, steps_between_batches=1)
    model = None
    if critics:
        twin = tt.agents.TQC().model             # the default networks, N times
        model = tt.models.ActorCriticEnsembleWithTargets(twin.actor, twin.critic_1, num_critics=critics,
                                                         observation_normalizer=tt.normalizers.MeanStd())
    agent = tt.agents.TQC(model=model, replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    assert agent.critic_updater.hidden == 256 and agent._u.route().fused_kind is None      # the split route
    assert agent.critic_updater.quantiles == M and agent.critic_updater.top_quantiles_to_drop_per_net == DROP
    assert getattr(agent.model, 'num_critics', 0) == critics
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


def one_time(critics):
    agent, draw, torch = build(critics)
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
    print('RESULT ' + json.dumps(dict(critics=critics or 2, ensemble=bool(critics), iterations_per_window=ITERATIONS,
                                      us_per_iteration_windows=[round(w, 3) for w in windows],
                                      us_per_iteration=round(statistics.median(windows), 3))))


def one_kernel():
    sys.path.insert(0, os.getcwd())
    import torch
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lib, p, out = _lib.load(), _lib.ptr, {}
    generator = torch.Generator(device='cuda').manual_seed(0)
    for N, quantiles in KERNEL_POOLS:
        ld = (quantiles + 15) // 16 * 16
        targets, thetas = (5 + 3 * torch.randn(N, B, ld, device='cuda', generator=generator) for _ in range(2))
        rewards, logp = (torch.randn(B, device='cuda', generator=generator) for _ in range(2))
        discounts = torch.full((B,), 0.99, device='cuda')
        dlogits, sample_m = torch.empty_like(thetas), torch.empty(3, B, device='cuda')

        def launch():
            _lib.check(lib.tonic_debug_ensemble_quantile_loss(
                p(targets), p(thetas), ld, p(rewards), p(discounts), p(logp), quantiles, N, DROP, 0.2, None, p(dlogits),
                p(sample_m), B, B, 0, _lib.current_stream()), 'tonic_debug_ensemble_quantile_loss')
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            launch()                             # (outside the capture first)
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                for _ in range(ITERATIONS):
                    launch()
            graph.replay()
            stream.synchronize()
            windows = []
            for _ in range(WINDOWS):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                graph.replay()
                end.record()
                end.synchronize()
                windows.append(start.elapsed_time(end) * 1e3 / ITERATIONS)
        assert bool(torch.isfinite(dlogits).all()) and bool(torch.isfinite(sample_m).all())
        out[str(N * quantiles)] = dict(critics=N, quantiles=quantiles, us_per_launch_windows=[round(w, 3) for w in windows],
                                       us_per_launch=round(statistics.median(windows), 3))
    print('RESULT ' + json.dumps(dict(kernel=out, launches_per_window=ITERATIONS)))


FIGURES = {'a': 0, 'b': 0, 'e2': 2, 'e5': 5, 'pe2': 2, 'pe5': 5}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=('time', 'kernel'))
    parser.add_argument('--critics', type=int, default=0)
    parser.add_argument('--parent')
    parser.add_argument('--rounds', type=int, default=2)
    parser.add_argument('--out', default='profiles/tqc_ensemble_timing.json')
    args = parser.parse_args()
    if args.one == 'time':
        return one_time(args.critics)
    if args.one == 'kernel':
        return one_kernel()
    parent = os.path.abspath(args.parent)

    def run(figure):
        theirs = figure.startswith('p')
        script = os.path.join(parent, 'scripts', os.path.basename(__file__)) if theirs else os.path.abspath(__file__)
        command = [sys.executable, script, '--one']
        command += ['kernel'] if figure in ('k', 'pk') else ['time', '--critics', str(FIGURES[figure])]
        env = dict(os.environ)
        env.pop('TONIC_AMD_NO_GRAPH', None)
        done = subprocess.run(command, cwd=parent if figure == 'a' or theirs else ROOT, env=env, capture_output=True, text=True,
                              timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{figure}: exit status {done.returncode}')
        return json.loads([l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):])

    runs, summary = [], {}

    def write():
        result = dict(
            what='TQC learner iterations, (256, 256) torso, O = 17, A = 6, B = 256, 25 quantiles per critic, 2 dropped '
                 'per critic, one MI355X, one fresh process per run, the order reversed in the second round: a = the '
                 'parent commit\'s twin TQC, b = this commit\'s twin TQC, e2 = the ensemble entries at N = 2, e5 = at '
                 'N = 5, pe2 / pe5 / pk = e2 / e5 / k on the parent commit; microseconds per iteration, device events round 7 replays of a captured update call of '
                 f'{ITERATIONS} iterations, the median of the 7 per run.  k = the ensemble critic loss kernel alone at '
                 f'B = 256 and N M = 50, 125, 256: microseconds per launch, 7 replays of {ITERATIONS} captured launches',
            runs=runs, summary=summary)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as out:
            json.dump(result, out, indent=1)

    order = ('a', 'b', 'e2', 'e5', 'k', 'pe2', 'pe5', 'pk')
    for round_ in range(1, args.rounds + 1):
        for figure in (order if round_ % 2 else order[::-1]):
            runs.append({**run(figure), 'figure': figure, 'round': round_})
            print(runs[-1], flush=True)
            write()
    windows = {f: [w for r in runs if r['figure'] == f for w in r['us_per_iteration_windows']] for f in FIGURES}
    medians = {f: statistics.median(w) for f, w in windows.items()}
    per_process = [r['us_per_iteration'] for r in runs if r['figure'] == 'a']
    alone = {f: [r['kernel'] for r in runs if r['figure'] == f] for f in ('k', 'pk')}
    launches = {f: {pool: [w for r in alone[f] for w in r[pool]['us_per_launch_windows']] for pool in alone[f][0]}
                for f in alone}
    kernel = {f: {pool: round(statistics.median(w), 3) for pool, w in launches[f].items()} for f in launches}
    summary.update(
        a_median=round(medians['a'], 3), a_min=round(min(windows['a']), 3), a_max=round(max(windows['a']), 3),
        a_process_medians=per_process, b_median=round(medians['b'], 3), e2_median=round(medians['e2'], 3),
        e5_median=round(medians['e5'], 3), b_minus_a=round(medians['b'] - medians['a'], 3),
        e2_minus_b=round(medians['e2'] - medians['b'], 3), e5_over_b=round(medians['e5'] / medians['b'], 4),
        pe2_median=round(medians['pe2'], 3), pe5_median=round(medians['pe5'], 3),
        loss_kernel_us=kernel['k'], parent_loss_kernel_us=kernel['pk'],
        parent_loss_kernel_us_range={pool: [min(w), max(w)] for pool, w in launches['pk'].items()},
        loss_kernel_within_parent_windows={pool: bool(min(launches['pk'][pool]) <= kernel['k'][pool]
                                                      <= max(launches['pk'][pool])) for pool in kernel['k']},
        b_within_a_windows=bool(min(windows['a']) <= medians['b'] <= max(windows['a'])),
        b_within_a_process_medians=bool(min(per_process) <= medians['b'] <= max(per_process)))
    write()
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
