"""What does the Return normaliser cost DDPG-family learners, and did the plain path move?  bench.offpolicy_loop for
BASELINE configs 3 and 4 (SAC B = 1 024, TD3 B = 100, default networks), one fresh process per run:

  (a) with return_normalizer=Return(0.99): the split entries with the squashed value heads (tonic_*_ranged);
  (b) without one and TONIC_AMD_FUSED_ITERATION=0: the same split launches, plain heads;
  (c) without one on the default path (the fused iteration).

(b) and (c) are also run on the parent commit's tree, parent and child alternating (the protocol of
profiles/critic_loss_timing.json).  (a) / (b) is the cost of the squash, (a) / (c) the cost of not having the fused
iteration; (b) and (c) against the parent, next to the parent's own run-to-run spread, say whether the plain path
moved.  No threshold: the figures are written down.

    python scripts/offpolicy_return_timing.py --parent <built checkout of the parent commit> [--repeats 3] [--out FILE]

A run that fails or runs out of time ends the whole measurement (nothing is started behind it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

CONFIGS = {'sac': dict(kind='sac', o_dim=111, a_dim=8, batch=1024, workers=1, loop_iterations=2000),
           'td3': dict(kind='td3', o_dim=67, a_dim=21, batch=100, workers=64, loop_iterations=300)}
VARIANTS = {'a': 'Return(0.99), split entries', 'b': 'no normaliser, TONIC_AMD_FUSED_ITERATION=0',
            'c': 'no normaliser, default path'}


def one(kind, variant):
    sys.path.insert(0, os.getcwd())
    import bench
    import tonic_amd.torch as tt
    if variant == 'a':
        plain = tt.agents._twin_model

        def with_return(head):
            model = plain(head)
            model.return_normalizer = tt.normalizers.Return(0.99)
            return model
        tt.agents._twin_model = with_return
        build = bench.build_offpolicy

        def checked(*args, **kwargs):
            agent, replay = build(*args, **kwargs)
            assert agent.model.return_normalizer is not None and agent._fused_kind() is None
            assert agent.critic_updater.return_normalizer is agent.model.return_normalizer
            return agent, replay
        bench.build_offpolicy = checked
    out = bench.offpolicy_loop(**CONFIGS[kind])
    print('RESULT ' + json.dumps(dict(
        learner_updates_per_sec=out['learner_updates_per_sec'], env_steps_per_sec=out['env_steps_per_sec'],
        ms_per_update_call=out['ms_per_update_call'], update_calls=out['update_calls'])))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=tuple(CONFIGS))
    parser.add_argument('--variant', choices=tuple(VARIANTS), default='c')
    parser.add_argument('--parent')
    parser.add_argument('--repeats', type=int, default=3)
    parser.add_argument('--out', default='profiles/offpolicy_return_timing.json')
    args = parser.parse_args()
    if args.one:
        return one(args.one, args.variant)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trees = {'parent': os.path.abspath(args.parent), 'child': here}

    def run(side, kind, variant):
        env = dict(os.environ)
        env.pop('TONIC_AMD_FUSED_ITERATION', None)
        if variant == 'b':
            env['TONIC_AMD_FUSED_ITERATION'] = '0'
        command = [sys.executable, os.path.abspath(__file__), '--one', kind, '--variant', variant]
        done = subprocess.run(command, cwd=trees[side], env=env, capture_output=True, text=True, timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{side} {kind} ({variant}): exit status {done.returncode}')
        line = [l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1]
        return json.loads(line[len('RESULT '):])

    runs = [('parent', 'b'), ('child', 'b'), ('parent', 'c'), ('child', 'c'), ('child', 'a')]
    repeats, summary = [], {}

    def write():
        result = dict(
            what='bench.offpolicy_loop on one MI355X, one fresh process per run, parent and child alternating '
                 f'({", ".join(f"{k}: {v}" for k, v in CONFIGS.items())}); learner updates/s',
            variants=VARIANTS, parent='the commit before the *_ranged entries', child='the commit that adds them',
            repeats=repeats, learner_updates_per_sec=summary)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as out:
            json.dump(result, out, indent=1)

    for kind in CONFIGS:
        for repeat in range(1, args.repeats + 1):
            for side, variant in runs:
                repeats.append(dict(side=side, variant=variant, repeat=repeat, kind=kind, **run(side, kind, variant)))
                print(repeats[-1], flush=True)
                write()
        rates = {(side, variant): [r['learner_updates_per_sec'] for r in repeats
                                   if (r['kind'], r['side'], r['variant']) == (kind, side, variant)]
                 for side, variant in runs}
        median = {key: statistics.median(values) for key, values in rates.items()}
        row = {}
        for variant in ('b', 'c'):
            parent = rates['parent', variant]
            row[variant] = dict(parent_median=median['parent', variant], parent_min=min(parent), parent_max=max(parent),
                                parent_spread=round(max(parent) - min(parent), 1),
                                child_median=median['child', variant], child_min=min(rates['child', variant]),
                                child_max=max(rates['child', variant]),
                                child_minus_parent=round(median['child', variant] - median['parent', variant], 1))
        child_a = rates['child', 'a']
        row['a'] = dict(child_median=median['child', 'a'], child_min=min(child_a), child_max=max(child_a))
        row['squash_cost_a_over_b'] = round(median['child', 'a'] / median['child', 'b'], 4)
        row['no_fused_iteration_a_over_c'] = round(median['child', 'a'] / median['child', 'c'], 4)
        summary[kind] = row
        write()
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
