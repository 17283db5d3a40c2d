"""Did stating every off-policy workspace once (the entries now evaluate their measured query on every call) move
anything?  Two figures, parent commit and this one alternating on one MI355X, one fresh process per run — the method
of scripts/policy_head_timing.py:

  sac    learner updates/s of bench.offpolicy_loop, BASELINE config 3 (SAC B = 1 024, the fused iteration), each
         tree's own package;
  split  microseconds per tonic_twin_q_grad + tonic_actor_q_grad pair (SAC, B = 256, O = 17, A = 6, the plain
         (256, 256) torso — where host time shows), the same inputs fed to either tree's libtonic_hip.so.

The bound: this commit's median inside the parent's own min - max spread.

    python scripts/offpolicy_layout_timing.py --parent <built checkout of the parent commit> [--repeats 4] [--out FILE]

A run that fails or runs out of time ends the whole measurement (nothing is started behind it)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = {'sac': 'learner_updates_per_sec', 'split': 'us_per_pair'}


def one_split(library_path, pairs=1000, windows=7, warmup=300):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import torch
    import test_gpu_offpolicy_workspace as cases
    from tonic_amd import _lib
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    B, O, A = 256, 17, 6
    library = ctypes.CDLL(os.path.abspath(library_path)) if library_path else _lib.load()
    for name in ('tonic_twin_q_grad', 'tonic_actor_q_grad', 'tonic_abi_version', 'tonic_offpolicy_workspace_bytes'):
        getattr(library, name).restype, getattr(library, name).argtypes = _lib.SIGNATURES[name]
    lib, p = _lib.load(), _lib.ptr              # (the inputs: this checkout's, for both builds; the workspace: as the build asks)
    cases.TORSOS['plain256'] = ((256, 256), 1)
    d = cases.Data(lib, 'plain256', B, O, A)
    actor, targets, critics = d.actor(2), d.critics(2), d.critics(2)
    ws = torch.zeros(library.tonic_offpolicy_workspace_bytes(B, O, A, d.H), dtype=torch.uint8, device='cuda')
    critic_sums, actor_sums = cases.zeros(critics.numel() + 8), cases.zeros(actor.numel() + 8)
    stream = _lib.current_stream()
    twin = [1, p(actor), p(targets), p(critics), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.actions), p(d.next_obs),
            p(d.rewards), p(d.discounts), p(d.eps), p(critic_sums), B, O, d.H, A, 0.2, 0.2, 0.5, p(ws), ws.numel(), stream]
    act = [1, p(actor), p(critics), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.eps2), p(actor_sums), B, O, d.H, A, 0.2,
           p(ws), ws.numel(), stream]

    def run(count):
        for _ in range(count):
            assert library.tonic_twin_q_grad(*twin) == 0 and library.tonic_actor_q_grad(*act) == 0
    run(warmup)
    torch.cuda.synchronize()
    measured = []
    for _ in range(windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run(pairs)
        end.record()
        end.synchronize()
        measured.append(start.elapsed_time(end) * 1e3 / pairs)
    assert torch.isfinite(critic_sums).all() and torch.isfinite(actor_sums).all()
    print('RESULT ' + json.dumps(dict(abi=int(library.tonic_abi_version()), B=B, O=O, A=A, H=256, pairs_per_window=pairs,
                                      us_per_pair_windows=[round(w, 3) for w in measured],
                                      us_per_pair=round(statistics.median(measured), 3))))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=tuple(FIGURES))
    parser.add_argument('--library', default=None)
    parser.add_argument('--parent')
    parser.add_argument('--repeats', type=int, default=4)
    parser.add_argument('--out', default='profiles/offpolicy_layout_timing.json')
    args = parser.parse_args()
    if args.one == 'sac':
        from policy_head_timing import one_sac
        return one_sac()
    if args.one == 'split':
        return one_split(args.library)
    trees = {'parent': os.path.abspath(args.parent), 'child': ROOT}

    def run(side, what):
        command = [sys.executable, os.path.abspath(__file__), '--one', what]
        if what == 'split':
            command += ['--library', os.path.join(trees[side], 'tonic_amd', 'libtonic_hip.so')]
        env = dict(os.environ)
        env.pop('TONIC_AMD_FUSED_ITERATION', None)
        done = subprocess.run(command, cwd=trees[side] if what == 'sac' else ROOT, env=env, capture_output=True,
                              text=True, timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{side} {what}: exit status {done.returncode}')
        line = [l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1]
        return json.loads(line[len('RESULT '):])

    repeats, summary = [], {}

    def write():
        result = dict(
            what='one MI355X, one fresh process per run, parent and child alternating (and who goes first): sac = learner '
                 'updates/s of bench.offpolicy_loop, BASELINE config 3 (the fused iteration); split = microseconds per '
                 'tonic_twin_q_grad + tonic_actor_q_grad pair (SAC, B = 256, O = 17, A = 6, plain 256); the bound: the '
                 "child's median inside the parent's own min - max spread",
            parent='the commit before the off-policy workspace layouts (hand-summed size formulas)',
            child='the commit that states each layout once (the entries measure their query on every call)',
            repeats=repeats, summary=summary)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as out:
            json.dump(result, out, indent=1)

    for what, figure in FIGURES.items():
        for repeat in range(1, args.repeats + 1):
            # (who goes first alternates: a process that follows another finds the box as that one left it)
            for side in (('parent', 'child') if repeat % 2 else ('child', 'parent')):
                repeats.append({**run(side, what), 'what': what, 'side': side, 'repeat': repeat})
                print(repeats[-1], flush=True)
                write()
        values = {side: [r[figure] for r in repeats if (r['what'], r['side']) == (what, side)]
                  for side in ('parent', 'child')}
        parent, child = values['parent'], values['child']
        summary[what] = dict(
            figure=figure, parent_median=statistics.median(parent), parent_min=min(parent), parent_max=max(parent),
            parent_spread=round(max(parent) - min(parent), 3), child_median=statistics.median(child),
            child_min=min(child), child_max=max(child),
            child_minus_parent=round(statistics.median(child) - statistics.median(parent), 3),
            child_median_inside_parent_spread=bool(min(parent) <= statistics.median(child) <= max(parent)))
        write()
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
