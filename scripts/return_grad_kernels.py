"""Developer probe for `rocprofv3 --kernel-trace --stats -- python scripts/return_grad_kernels.py`: the critic's
fused grad kernel at the bench shape (N = 4096 x 256 samples, O = 17), plain (tonic_value_regression_grad)
and with the Return normaliser's squashed head (tonic_value_regression_grad_ranged), `repeats` launches of
each, alternating; plus tonic_reward_range on the rollout's [4096, 256] rewards."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tonic_amd                                  # noqa: E402
from tonic_amd import _lib                        # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 40
lib = _lib.load()
O, n = 17, 4096 * 256
P = lib.tonic_v_critic_param_count(O)
rng = np.random.RandomState(0)
params = torch.as_tensor((rng.normal(size=P) * 0.1).astype(np.float32), device='cuda')
obs = torch.as_tensor(rng.normal(size=(n, O)).astype(np.float32), device='cuda')
ret = torch.as_tensor((rng.normal(size=n) * 30).astype(np.float32), device='cuda')
mean, std = torch.zeros(O, device='cuda'), torch.ones(O, device='cuda')
low, high = torch.tensor(-3185.4, device='cuda'), torch.tensor(100.0, device='cuda')
sums = torch.zeros(P + 8, device='cuda')
ws = torch.empty(lib.tonic_ppo_workspace_bytes(n, O, 1, 0), dtype=torch.uint8, device='cuda')
rng_out = torch.empty(2, device='cuda')
p = _lib.ptr
for _ in range(repeats):
    _lib.check(lib.tonic_value_regression_grad(p(params), p(mean), p(std), 0.0, p(obs), p(ret), p(sums), n, O, 0,
                                               p(ws), ws.numel(), None), 'plain')
    _lib.check(lib.tonic_value_regression_grad_ranged(p(params), p(mean), p(std), 0.0, p(obs), p(ret), p(sums), n,
                                                      O, 0, p(ws), ws.numel(), p(low), p(high), None), 'ranged')
    _lib.check(lib.tonic_reward_range(p(ret), n, p(rng_out), None), 'range')
torch.cuda.synchronize()
print('done', repeats, 'launches of each; range', rng_out.cpu().numpy())
