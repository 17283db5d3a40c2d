"""Developer probe: the cost of the Return normaliser at the bench workload — the step of bench.py (T = 4096
environment steps of 256 workers + one PPO learner update) with the default model and with
ActorCritic(..., return_normalizer=Return(0.99)), one agent alive at a time, alternating on one box: ms per
step.  `python scripts/return_normalizer_ab.py [rounds]`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                      # noqa: E402
import time                                       # noqa: E402

plain_build = bench.build_agent


def return_build(steps=bench.T, iterations=bench.ITERATIONS, seed=0):
    import tonic_amd
    import tonic_amd.torch
    from tonic_amd.environments import Box
    from tonic_amd.torch import models, normalizers
    model = models.ActorCritic(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP((64, 64), torch.nn.Tanh),
                           head=models.DetachedScaleGaussianPolicyHead()),
        critic=models.Critic(encoder=models.ObservationEncoder(), torso=models.MLP((64, 64), torch.nn.Tanh),
                             head=models.ValueHead()),
        observation_normalizer=normalizers.MeanStd(), return_normalizer=normalizers.Return(0.99))
    agent = tonic_amd.torch.agents.PPO(
        model=model, replay=tonic_amd.replays.Segment(size=steps, batch_iterations=iterations))
    agent.initialize(Box(-np.inf, np.inf, (bench.O,)), Box(-1, 1, (bench.A,)), seed=seed)
    return agent


rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
times = {'plain': [], 'Return(0.99)': []}
for r in range(rounds):
    for variant, build in (('plain', plain_build), ('Return(0.99)', return_build)):
        bench.build_agent = build
        agent, loop, rollout, out = bench.measure_job(256, 0, 1, 1, 0, True, device_too=False)
        loop.run(bench.T - agent.replay.index)
        torch.cuda.synchronize()
        for _ in range(2):
            t0 = time.perf_counter()
            for _ in range(4):                    # (several steps between two device syncs, like bench.py)
                loop.run(bench.T)
            torch.cuda.synchronize()
            times[variant].append((time.perf_counter() - t0) * 1e3 / 4)
        print(variant, loop.breakdown(), flush=True)
        agent.close()
        del agent, loop, rollout
for variant, ts in times.items():
    median = float(np.median(ts))
    print(f'{variant:>13}: ms per step', ' '.join(f'{t:.1f}' for t in ts), '| median', round(median, 2), '->',
          round(bench.T * 256 / median / 1e3, 2), 'M env-steps/s')
print('cost of the Return normaliser:',
      f"{(np.median(times['Return(0.99)']) / np.median(times['plain']) - 1) * 100:+.2f} % per step")
