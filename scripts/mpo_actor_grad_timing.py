"""Times tonic_mpo_actor_grad (the E-step, the M-step gradients and the dual kernel of one MPO actor step) with
device events and prints one JSON line.  Developer tool behind profiles/mpo_surface_timing.json.

    python scripts/mpo_actor_grad_timing.py [--library PATH] [--samples S] [--joint] [--label NAME]

The networks, the batch and the workspace come from this checkout's package (B = 256, A = 6, O = 17, the plain
(256, 256) ReLU torso); the timed entry is taken from `--library`, so that a libtonic_hip.so built from another commit
can be measured on the same inputs, one fresh process per measurement.  Without --joint the entry is
tonic_mpo_actor_grad, which every ABI since 8 has with this signature; --joint calls tonic_mpo_actor_grad_joint with
joint_kl = 1.  Each of `--windows` windows times `--calls` back-to-back calls between two events after `--warmup`
calls; the figure is the median window's microseconds per call (launch overheads of its ~20 launches included)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--library', default=None)
    parser.add_argument('--samples', type=int, default=20)
    parser.add_argument('--joint', action='store_true')
    parser.add_argument('--label', default='this checkout')
    parser.add_argument('--calls', type=int, default=1000)
    parser.add_argument('--windows', type=int, default=7)
    parser.add_argument('--warmup', type=int, default=300)
    args = parser.parse_args()
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd import _lib
    from tonic_amd.environments import Box
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    O, A, B, S = 17, 6, 256, args.samples
    agent = tt.agents.MPO(
        replay=tonic_amd.replays.Buffer(size=1000, batch_iterations=1, batch_size=B),
        actor_updater=tt.updaters.MaximumAPosterioriPolicyOptimization(
            num_samples=S, per_dim_constraining=not args.joint),
        critic_updater=tt.updaters.ExpectedSARSA(num_samples=S))
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    u, m, p = agent.actor_updater, agent.model, _lib.ptr
    name = 'tonic_mpo_actor_grad_joint' if args.joint else 'tonic_mpo_actor_grad'
    library = ctypes.CDLL(os.path.abspath(args.library)) if args.library else _lib.load()
    entry = getattr(library, name)
    entry.restype, entry.argtypes = _lib.SIGNATURES[name]
    library.tonic_abi_version.restype = ctypes.c_int32
    rng = np.random.RandomState(0)
    obs = torch.as_tensor(rng.normal(size=(B, O)), dtype=torch.float32, device='cuda')
    eps = torch.as_tensor(rng.normal(size=(S * B, A)), dtype=torch.float32, device='cuda')
    mean, std = u.norm_tensors()
    ws = u._offpolicy_workspace(B)
    stats = torch.zeros_like(u.mpo_stats)
    arguments = [p(u.flat.flat), p(m.flat_target_actor.flat), p(m.flat_target_critics.flat), p(u.duals),
                 float(u.min_log_dual), p(mean), p(std), u.norm_clip(), p(obs), p(eps), p(u.grad_sums),
                 p(u.dual_grads), p(stats), B, O, u.hidden, A, S, float(u.epsilon), float(u.epsilon_penalty),
                 float(u.epsilon_mean), float(u.epsilon_std), 1] + ([1] if args.joint else []) + \
        [p(ws), ws.numel(), _lib.current_stream()]

    def run(calls):
        for _ in range(calls):
            status = entry(*arguments)
            assert status == 0, status
    run(args.warmup)
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run(args.calls)
        end.record()
        end.synchronize()
        windows.append(start.elapsed_time(end) * 1e3 / args.calls)
    assert torch.isfinite(u.grad_sums).all() and torch.isfinite(stats).all()
    print(json.dumps(dict(side=args.label, entry=name, abi=int(library.tonic_abi_version()), B=B, S=S, A=A, O=O,
                          joint_kl=int(args.joint), calls_per_window=args.calls,
                          us_per_call_windows=[round(w, 3) for w in windows],
                          us_per_call=round(statistics.median(windows), 3))))


if __name__ == '__main__':
    main()
