"""Worker of tests/test_gpu_trpo_hip.py::test_two_ranks_equal_one: one rank of a world_size-N TRPO actor step
(run with RANK / WORLD_SIZE / MASTER_* set).  Each rank owns a contiguous shard of the rows of the common
batch; rank 0 saves the step and the statistics."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tonic_amd                      # noqa: E402
import tonic_amd.torch                # noqa: E402
from tonic_amd import parallel        # noqa: E402
from tonic_amd.torch import updaters  # noqa: E402
from test_gpu_trpo_hip import step_problem  # noqa: E402


def run(out_path):
    rank, world = parallel.init_from_env()
    model, batch = step_problem(5, 1.0)
    model.pack('cuda')
    updater = updaters.TrustRegionPolicyGradient()
    updater.initialize(model)
    lo, hi = parallel.shard_bounds(batch['observations'].shape[0])
    start = model.flat_actor.flat.detach().cpu().numpy().copy()
    out = updater(**{k: torch.as_tensor(np.ascontiguousarray(v[lo:hi])).cuda() for k, v in batch.items()})
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out_path, hip=int(updater.hip), step=model.flat_actor.flat.detach().cpu().numpy() - start,
                 **{k: np.asarray(v.numpy()) for k, v in out.items()})
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    run(sys.argv[1])
