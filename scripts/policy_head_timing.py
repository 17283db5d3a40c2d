"""Did carrying the policy heads' scale bounds into the kernels as arguments move anything on the DEFAULT heads?
Three figures, parent commit and this one alternating on one MI355X, one fresh process per run:

  sac      learner updates/s of bench.offpolicy_loop, BASELINE config 3 (SAC B = 1 024, the fused iteration);
  mpo      microseconds per tonic_mpo_actor_grad call at the default shape (scripts/mpo_actor_grad_timing.py);
  forward  microseconds per tonic_policy_forward kind 1 call (B = 256, O = 17, A = 6, the plain (256, 256) torso).

`sac` runs each tree's own package; `mpo` and `forward` feed the same inputs of this checkout into either tree's
libtonic_hip.so (the timed entries kept their signatures).  The bound: this commit's median inside the parent's own
min - max spread; a median that moved by less than that spread is not a finding.  The figures are written down with
the register counts of the touched kernels, which this script takes from csrc/resource_usage.py run on offpolicy.hip
and mlpfwd.hip of both trees (compiles only: no GPU).

    python scripts/policy_head_timing.py --parent <built checkout of the parent commit> [--repeats 5] [--out FILE]
    python scripts/policy_head_timing.py --parent <checkout> --only-resources   # the register table of --out, in place

A run that fails or runs out of time ends the whole measurement (nothing is started behind it)."""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAC = dict(kind='sac', o_dim=111, a_dim=8, batch=1024, workers=1, loop_iterations=2000)
FIGURES = {'sac': 'learner_updates_per_sec', 'mpo': 'us_per_call', 'forward': 'us_per_call'}


TOUCHED = ('sac_sample_kernel', 'gaussian_sample_kernel', 'gaussian_tile_kernel', 'mpo_state_kernel',
           'actor_head_backward_kernel', 'mlp_forward_kernel', 'mlp_backward_kernel', 'mlp_forward_ranged_kernel',
           'mlp_backward_ranged_kernel', 'q_critic_step_kernel', 'q_actor_step_kernel')


def kernel_resources(trees):
    """{kernel: {side: registers, spills, scratch, occupancy}} of the touched kernels, from the tables that
    tonic_amd/csrc/resource_usage.py prints for offpolicy.hip and mlpfwd.hip of each tree."""
    row = re.compile(r'(.*?)\s+vgpr=\s*(\d+) agpr=\s*(\d+)\s+spill=\s*(\d+) scratch=\s*(\d+) occ=(\d+) sgpr=(\d+)')
    jobs = {(side, source): subprocess.Popen([sys.executable, 'resource_usage.py', source],
                                             cwd=os.path.join(tree, 'tonic_amd', 'csrc'), stdout=subprocess.PIPE, text=True)
            for side, tree in trees.items() for source in ('offpolicy.hip', 'mlpfwd.hip')}
    kernels = {}
    for (side, source), job in jobs.items():
        table, _ = job.communicate()
        if job.returncode != 0:
            raise SystemExit(f'resource_usage.py {source} ({side}): exit status {job.returncode}')
        for line in table.splitlines():
            found = row.match(line)
            name = re.search(r'(\w+_kernel(?:<\w+>)?)', found.group(1)) if found else None
            if name and name.group(1).startswith(TOUCHED):
                keys = ('vgpr', 'agpr', 'spill', 'scratch', 'occupancy', 'sgpr')
                kernels.setdefault(name.group(1), {})[side] = dict(zip(keys, (int(v) for v in found.groups()[1:])))
    return dict(source='tonic_amd/csrc/resource_usage.py on offpolicy.hip and mlpfwd.hip (hipcc -Rpass-analysis='
                       'kernel-resource-usage, gfx950), parent and child; <true> = the fp16x2 weight-image pass',
                kernels=kernels)


def one_sac():
    sys.path.insert(0, os.getcwd())
    import bench
    build = bench.build_offpolicy

    def checked(*args, **kwargs):
        agent, replay = build(*args, **kwargs)
        assert agent._fused_kind() is not None
        return agent, replay
    bench.build_offpolicy = checked
    out = bench.offpolicy_loop(**SAC)
    print('RESULT ' + json.dumps(dict(learner_updates_per_sec=out['learner_updates_per_sec'],
                                      ms_per_update_call=out['ms_per_update_call'], update_calls=out['update_calls'])))


def one_forward(library_path, calls=2000, windows=7, warmup=500):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import tonic_amd.torch as tt
    from tonic_amd import _lib
    from tonic_amd.environments import Box
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    O, A, B = 17, 6, 256
    agent = tt.agents.SAC()
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    library = ctypes.CDLL(os.path.abspath(library_path)) if library_path else _lib.load()
    entry = library.tonic_policy_forward
    entry.restype, entry.argtypes = _lib.SIGNATURES['tonic_policy_forward']
    library.tonic_abi_version.restype = ctypes.c_int32
    rng = np.random.RandomState(0)
    obs = torch.as_tensor(rng.normal(size=(B, O)), dtype=torch.float32, device='cuda')
    eps = torch.as_tensor(rng.normal(size=(B, A)), dtype=torch.float32, device='cuda')
    out = torch.zeros(B, A, device='cuda')
    ws = torch.empty(agent.lib.tonic_offpolicy_workspace_bytes(B, O, A, agent.hidden), dtype=torch.uint8, device='cuda')
    p = _lib.ptr
    arguments = [p(agent.model.flat_actor.flat), p(obs), p(eps), p(out), 1, B, O, agent.hidden, A, p(ws), ws.numel(),
                 _lib.current_stream()]

    def run(count):
        for _ in range(count):
            status = entry(*arguments)
            assert status == 0, status
    run(warmup)
    torch.cuda.synchronize()
    measured = []
    for _ in range(windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run(calls)
        end.record()
        end.synchronize()
        measured.append(start.elapsed_time(end) * 1e3 / calls)
    assert torch.isfinite(out).all()
    print('RESULT ' + json.dumps(dict(entry='tonic_policy_forward', kind=1, abi=int(library.tonic_abi_version()), B=B,
                                      O=O, A=A, calls_per_window=calls,
                                      us_per_call_windows=[round(w, 3) for w in measured],
                                      us_per_call=round(statistics.median(measured), 3))))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=tuple(FIGURES))
    parser.add_argument('--library', default=None)
    parser.add_argument('--parent')
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--no-resources', action='store_true', help='timing only (--only-resources adds the table)')
    parser.add_argument('--only-resources', action='store_true',
                        help='no timing: (re)write the register table of --out in place')
    parser.add_argument('--out', default='profiles/policy_head_timing.json')
    args = parser.parse_args()
    if args.one == 'sac':
        return one_sac()
    if args.one == 'forward':
        return one_forward(args.library)
    trees = {'parent': os.path.abspath(args.parent), 'child': ROOT}
    if args.only_resources:
        with open(args.out) as out:
            result = json.load(out)
        result['kernel_resources'] = kernel_resources(trees)
        with open(args.out, 'w') as out:
            json.dump(result, out, indent=1)
        return

    def run(side, what):
        library = os.path.join(trees[side], 'tonic_amd', 'libtonic_hip.so')
        if what == 'sac':
            command, cwd = [sys.executable, os.path.abspath(__file__), '--one', 'sac'], trees[side]
        elif what == 'mpo':
            command = [sys.executable, os.path.join(ROOT, 'scripts', 'mpo_actor_grad_timing.py'), '--library', library,
                       '--label', side]
            cwd = ROOT
        else:
            command, cwd = [sys.executable, os.path.abspath(__file__), '--one', 'forward', '--library', library], ROOT
        env = dict(os.environ)
        env.pop('TONIC_AMD_FUSED_ITERATION', None)
        done = subprocess.run(command, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{side} {what}: exit status {done.returncode}')
        line = [l for l in done.stdout.splitlines() if l.startswith(('RESULT ', '{'))][-1]
        return json.loads(line[len('RESULT '):] if line.startswith('RESULT ') else line)

    repeats, summary = [], {}
    resources = None if args.no_resources else kernel_resources(trees)

    def write():
        result = dict(
            what='default policy heads on one MI355X, one fresh process per run, parent and child alternating (and who goes first): '
                 f'sac = learner updates/s of bench.offpolicy_loop ({SAC}); mpo = microseconds per tonic_mpo_actor_grad '
                 'call (scripts/mpo_actor_grad_timing.py: B = 256, S = 20, A = 6, O = 17); forward = microseconds per '
                 'tonic_policy_forward kind 1 call (B = 256, O = 17, A = 6); the bound: the child\'s median inside the '
                 'parent\'s own min - max spread',
            parent='the commit before tonic_mlp_torso_head (ABI 18: the bounds are literals in the kernels)',
            child='the commit that adds it (ABI 19: the bounds are kernel arguments)',
            repeats=repeats, summary=summary, kernel_resources=resources)
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
