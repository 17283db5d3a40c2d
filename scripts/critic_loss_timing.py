"""Does the default MSE critic loss pay for the loss rule (tonic_critic_loss_t)?  bench.offpolicy_loop for BASELINE
configs 3 and 4 (SAC B = 1 024, TD3 B = 100), the parent commit's tree and this one alternating, one fresh process
per repeat — the protocol of profiles/q_block_refactor_speed.json — plus one SAC run under HuberLoss() for information.

    python scripts/critic_loss_timing.py --parent <built checkout of the parent commit> [--repeats 3] [--out FILE]

A repeat that fails or runs out of time ends the whole measurement (nothing is started behind it)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

CONFIGS = {'sac': dict(kind='sac', o_dim=111, a_dim=8, batch=1024, workers=1, loop_iterations=2000),
           'td3': dict(kind='td3', o_dim=67, a_dim=21, batch=100, workers=64, loop_iterations=300)}


def one(kind, huber):
    sys.path.insert(0, os.getcwd())
    import bench
    if huber:
        import torch
        build = bench.build_offpolicy

        def with_huber(*args, **kwargs):
            agent, replay = build(*args, **kwargs)
            agent.critic_updater.loss = torch.nn.HuberLoss()
            return agent, replay
        bench.build_offpolicy = with_huber
    out = bench.offpolicy_loop(**CONFIGS[kind])
    print('RESULT ' + json.dumps(dict(
        learner_updates_per_sec=out['learner_updates_per_sec'], env_steps_per_sec=out['env_steps_per_sec'],
        ms_per_update_call=out['ms_per_update_call'], update_calls=out['update_calls'])))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--one', choices=tuple(CONFIGS))
    parser.add_argument('--huber', action='store_true')
    parser.add_argument('--parent')
    parser.add_argument('--repeats', type=int, default=3)
    parser.add_argument('--out', default='profiles/critic_loss_timing.json')
    args = parser.parse_args()
    if args.one:
        return one(args.one, args.huber)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trees = {'parent': os.path.abspath(args.parent), 'child': here}

    def run(side, kind, huber=False):
        command = [sys.executable, os.path.abspath(__file__), '--one', kind] + (['--huber'] if huber else [])
        done = subprocess.run(command, cwd=trees[side], capture_output=True, text=True, timeout=300)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f'{side} {kind}: exit status {done.returncode}')
        line = [l for l in done.stdout.splitlines() if l.startswith('RESULT ')][-1]
        return json.loads(line[len('RESULT '):])

    repeats, summary = [], {}
    for kind in CONFIGS:
        for repeat in range(1, args.repeats + 1):
            for side in ('parent', 'child'):
                repeats.append(dict(side=side, repeat=repeat, kind=kind, loss='default (MSE)', **run(side, kind)))
                print(repeats[-1], flush=True)
        rates = {side: [r['learner_updates_per_sec'] for r in repeats if r['kind'] == kind and r['side'] == side]
                 for side in trees}
        spread = max(rates['parent']) - min(rates['parent'])
        summary[kind] = dict(parent_median=statistics.median(rates['parent']), parent_min=min(rates['parent']),
                             parent_max=max(rates['parent']), parent_spread=round(spread, 1),
                             child_median=statistics.median(rates['child']),
                             child_within_parent_spread=bool(
                                 statistics.median(rates['child']) >= statistics.median(rates['parent']) - spread))
    huber = dict(side='child', kind='sac', loss='HuberLoss()', **run('child', 'sac', huber=True))
    print(huber, flush=True)
    result = dict(
        what='bench.offpolicy_loop on one MI355X, one fresh process per repeat, parent and child alternating '
             f'({", ".join(f"{k}: {v}" for k, v in CONFIGS.items())}); the bound: the child\'s median learner '
             'updates/s at most the parent\'s own min-max spread below the parent\'s median',
        parent='the commit before tonic_critic_loss_t', child='the commit that adds it',
        repeats=repeats, learner_updates_per_sec=summary, huber_for_information=huber)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
