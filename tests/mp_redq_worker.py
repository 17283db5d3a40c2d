"""Worker of tests/test_gpu_redq.py: one rank of a world_size-N REDQ learner update (tests/mp_tqc_worker.py's method:
each rank owns a contiguous shard of the worker axis of a common synthetic Buffer, every rank draws the same GLOBAL
index, noise and subset streams and keeps its own samples).  One update call of four iterations with a learned entropy
coefficient; the batch is small against the shards, so the ranks' parts are uneven.  Every rank saves its masks."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tonic_amd                      # noqa: E402
import tonic_amd.torch                # noqa: E402
from tonic_amd import parallel        # noqa: E402
from tonic_amd.environments import Box  # noqa: E402


def run(out_path, rows=40, W=8, O=11, A=3, iterations=4, batch=24):
    rank, world = parallel.init_from_env()
    tt = tonic_amd.torch
    tuner = tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=0.5,
                                           optimizer=lambda params: torch.optim.Adam(params, lr=0.01))
    agent = tt.agents.REDQ(replay=tonic_amd.replays.Buffer(size=rows * W, batch_iterations=iterations,
                                                           batch_size=batch, steps_before_batches=0,
                                                           steps_between_batches=1),
                           entropy_coeff_updater=tuner)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=7)
    assert agent._u.route().fused_kind is None
    rng = np.random.RandomState(321)
    lo, hi = parallel.shard_bounds(W)
    norm = agent.model.observation_normalizer
    for _ in range(rows - 3):                       # partially filled circular buffer
        row = dict(observations=rng.normal(size=(W, O)), actions=rng.uniform(-1, 1, size=(W, A)),
                   next_observations=rng.normal(size=(W, O)), rewards=rng.normal(size=W),
                   resets=rng.uniform(size=W) < 0.1, terminations=rng.uniform(size=W) < 0.05)
        row = {k: torch.as_tensor(np.ascontiguousarray(np.asarray(v, np.float32)[lo:hi])).cuda()
               for k, v in row.items()}
        agent.replay.store(normalizer=norm, **row)
    agent._update(steps=rows * W)
    torch.cuda.synchronize()
    np.save(f'{out_path}.masks{rank}.npy', agent._u.slots[0].subsets.cpu().numpy())      # (every rank its own)
    if rank == 0:
        state = {k: v.detach().cpu().numpy() for k, v in agent.model.state_dict().items()}
        np.savez(out_path, infos=agent.last_infos, coeff_infos=agent.last_entropy_coeff_infos,
                 log_entropy_coeff=tuner.log_entropy_coeff.cpu().numpy(), **state)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    run(sys.argv[1])
