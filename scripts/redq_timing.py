"""What does REDQ cost, and did serving it move SAC's and TQC's iterations?  Figures on one MI355X, one fresh process
per run, two processes per figure, the order reversed in the second round, measured the way
scripts/tqc_ensemble_timing.py does:

  sac_p, sac_c   the split SAC iteration (TONIC_AMD_FUSED_ITERATION=0: the updaters' own entries) on the parent commit
                 and on this one;
  tqc_p, tqc_c   the twin TQC iteration (2 critics of 25 quantiles, 2 dropped per critic) on the parent and on this one;
  r2, r5, r8     REDQ at N = 2, 5, 8 critics, subsets of 2;
  k              the subset critic loss kernel alone (tonic_debug_ensemble_subset_loss) at B = 256, N = 2, 5, 8.

All agents: the default (256, 256) torso, O = 17, A = 6, B = 256, one update call of 200 iterations captured as a
hipGraph; device events round 7 replays (new indices, draws and subsets each), microseconds per iteration, the median of
the 7.  k: 200 launches captured as one graph, device events round 7 replays, microseconds per launch.  Checked when the
figures are written: sac_c's and tqc_c's medians inside the range of the parent's own windows.  The rest is reported, not
judged.

    python scripts/redq_timing.py --parent <built checkout of the parent commit> [--rounds 2] [--out FILE]

Every run has a time limit of its own, and a run that fails or runs out of time ends the whole measurement (nothing is
started behind it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, A, W, B, ITERATIONS, WINDOWS = 17, 6, 16, 256, 200, 7
KERNEL_CRITICS = (2, 5, 8)


def build(agent_name, critics):
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
    if agent_name == 'REDQ':
        default = tt.agents.REDQ().model         # the default networks, N times
        model = tt.models.ActorCriticEnsembleWithTargets(default.actor, default.critic_1, num_critics=critics,
                                                         observation_normalizer=tt.normalizers.MeanStd())
    agent = getattr(tt.agents, agent_name)(model=model, replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    assert agent.critic_updater.hidden == 256 and agent._u.route().fused_kind is None      # the split route
    assert getattr(agent.model, 'num_critics', 2) == critics
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


def one_time(agent_name, critics):
    agent, draw, torch = build(agent_name, critics)
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
        infos = agent.enqueue_update(first, eps)           # (REDQ: the subsets drawn and uploaded inside)
        end.record()
        end.synchronize()
        windows.append(start.elapsed_time(end) * 1e3 / ITERATIONS)
    assert agent._u.slot.graph is graph and bool(torch.isfinite(infos).all())
    print('RESULT ' + json.dumps(dict(agent=agent_name, critics=critics, iterations_per_window=ITERATIONS,
                                      us_per_iteration_windows=[round(w, 3) for w in windows],
                                      us_per_iteration=round(statistics.median(windows), 3))))


def one_kernel():
    sys.path.insert(0, os.getcwd())
    import torch
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lib, p, out, ld = _lib.load(), _lib.ptr, {}, 16
    generator = torch.Generator(device='cuda').manual_seed(0)
    for N in KERNEL_CRITICS:
        targets, qs = (5 + 3 * torch.randn(N, B, ld, device='cuda', generator=generator) for _ in range(2))
        rewards, logp = (torch.randn(B, device='cuda', generator=generator) for _ in range(2))
        discounts = torch.full((B,), 0.99, device='cuda')
        word = torch.tensor([0b11], dtype=torch.int32, device='cuda')
        dq, sample_m = torch.empty_like(qs), torch.empty(3, B, device='cuda')

        def launch():
            _lib.check(lib.tonic_debug_ensemble_subset_loss(
                p(targets), p(qs), ld, p(rewards), p(discounts), p(logp), N, p(word), 0.2, None, None, p(dq),
                p(sample_m), B, B, _lib.current_stream()), 'tonic_debug_ensemble_subset_loss')
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
        assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(sample_m).all())
        out[str(N)] = dict(critics=N, us_per_launch_windows=[round(w, 3) for w in windows],
                           us_per_launch=round(statistics.median(windows), 3))
    print('RESULT ' + json.dumps(dict(kernel=out, launches_per_window=ITERATIONS)))


# figure: (agent, critics, on the parent commit)
FIGURES = {'sac_p': ('SAC', 2, True), 'sac_c': ('SAC', 2, False), 'tqc_p': ('TQC', 2, True), 'tqc_c': ('TQC', 2, False),
           'r2': ('REDQ', 2, False), 'r5': ('REDQ', 5, False), 'r8': ('REDQ', 8, False)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=('time', 'kernel'))
    parser.add_argument('--agent', default='REDQ')
    parser.add_argument('--critics', type=int, default=5)
    parser.add_argument('--parent')
    parser.add_argument('--rounds', type=int, default=2)
    parser.add_argument('--out', default='profiles/redq_timing.json')
    args = parser.parse_args()
    if args.one == 'time':
        return one_time(args.agent, args.critics)
    if args.one == 'kernel':
        return one_kernel()
    parent = os.path.abspath(args.parent)

    def run(figure):
        command = [sys.executable, os.path.abspath(__file__), '--one']
        theirs = False
        if figure == 'k':
            command += ['kernel']
        else:
            agent, critics, theirs = FIGURES[figure]
            command += ['time', '--agent', agent, '--critics', str(critics)]
        env = dict(os.environ, TONIC_AMD_FUSED_ITERATION='0')          # (SAC: the split entries; the others' route)
        env.pop('TONIC_AMD_NO_GRAPH', None)
        done = subprocess.run(command, cwd=parent if theirs else ROOT, env=env, capture_output=True, text=True,
                              timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{figure}: exit status {done.returncode}')
        return json.loads([l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1][len('RESULT '):])

    runs, summary = [], {}

    def write():
        result = dict(
            what='learner iterations, (256, 256) torso, O = 17, A = 6, B = 256, one MI355X, one fresh process per run, '
                 'the order reversed in the second round: sac_p / sac_c = the split SAC iteration on the parent commit '
                 '/ on this one, tqc_p / tqc_c = the twin TQC iteration (25 quantiles, 2 dropped), r2 / r5 / r8 = REDQ '
                 'at N = 2, 5, 8 with subsets of 2; microseconds per iteration, device events round 7 replays of a '
                 f'captured update call of {ITERATIONS} iterations, the median of the 7 per run.  k = the subset '
                 f'critic loss kernel alone at B = 256, N = 2, 5, 8: microseconds per launch, 7 replays of {ITERATIONS} '
                 'captured launches',
            runs=runs, summary=summary)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as out:
            json.dump(result, out, indent=1)

    order = ('sac_p', 'sac_c', 'tqc_p', 'tqc_c', 'r2', 'r5', 'r8', 'k')
    for round_ in range(1, args.rounds + 1):
        for figure in (order if round_ % 2 else order[::-1]):
            runs.append({**run(figure), 'figure': figure, 'round': round_})
            print(runs[-1], flush=True)
            write()
    windows = {f: [w for r in runs if r['figure'] == f for w in r['us_per_iteration_windows']] for f in FIGURES}
    medians = {f: round(statistics.median(w), 3) for f, w in windows.items()}
    launches = {N: [w for r in runs if r['figure'] == 'k' for w in r['kernel'][N]['us_per_launch_windows']]
                for N in map(str, KERNEL_CRITICS)}
    summary.update(
        medians=medians,
        parent_window_ranges={f: [min(windows[f]), max(windows[f])] for f in ('sac_p', 'tqc_p')},
        sac_c_within_sac_p_windows=bool(min(windows['sac_p']) <= medians['sac_c'] <= max(windows['sac_p'])),
        tqc_c_within_tqc_p_windows=bool(min(windows['tqc_p']) <= medians['tqc_c'] <= max(windows['tqc_p'])),
        redq_n2_minus_split_sac=round(medians['r2'] - medians['sac_c'], 3),
        redq_us_per_added_critic=round((medians['r8'] - medians['r2']) / 6, 3),
        redq_us_per_added_critic_2_to_5=round((medians['r5'] - medians['r2']) / 3, 3),
        tqc_us_per_added_critic_recorded=69,
        loss_kernel_us={N: round(statistics.median(w), 3) for N, w in launches.items()})
    write()
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
