"""Developer probe: learner updates/s of the off-policy agents with a three-layer torso, MLP((256, 256, 256), ReLU),
at B = 256, O = 17, A = 6 (50 iterations per update call, a full HBM Buffer of synthetic transitions).

    python scripts/offpolicy_torso_rate.py [sizes...]      # e.g. 400 300: another torso

SAC and TD3 run twice: on the HIP entries (tonic_mlp_torso: layer by layer on gemm16 launches, the update call
captured in a hipGraph) and on stock torch operators (TONIC_AMD_TORSO_STOCK=1: autograd, no capture).  D4PG and MPO
have no stock form: HIP only.  One JSON line per run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

O, A, B, ITERATIONS, ROWS = 17, 6, 256, 50, 100000


def build(kind, sizes):
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd.environments import Box
    relu = torch.nn.ReLU
    if kind == 'sac':
        head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                            distribution=tt.models.SquashedMultivariateNormalDiag)
    elif kind == 'mpo':
        head = tt.models.GaussianPolicyHead()
    else:
        head = tt.models.DeterministicPolicyHead()
    critic_head = tt.models.DistributionalValueHead(-150., 150., 51) if kind == 'd4pg' else tt.models.ValueHead()
    container = tt.models.ActorTwinCriticWithTargets if kind in ('sac', 'td3') else tt.models.ActorCriticWithTargets
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, relu), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, relu),
                                head=critic_head),
        observation_normalizer=tt.normalizers.MeanStd())
    replay = tonic_amd.replays.Buffer(size=ROWS, batch_iterations=ITERATIONS, batch_size=B)
    agent = dict(sac=tt.agents.SAC, td3=tt.agents.TD3, d4pg=tt.agents.D4PG, mpo=tt.agents.MPO)[kind](
        model=model, replay=replay)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=0)
    replay._allocate(1, O, A)
    gen = torch.Generator(device=agent.device)
    gen.manual_seed(0)
    for key, buf in replay.buffers.items():       # (as bench.build_offpolicy fills its Buffer)
        if key in ('resets', 'terminations'):
            buf.copy_((torch.rand(buf.shape, device=agent.device, generator=gen) < 1e-3).float())
        elif key == 'discounts':
            buf.copy_((1 - replay.buffers['terminations']) * 0.99)
        elif key == 'actions':
            buf.copy_(torch.rand(buf.shape, device=agent.device, generator=gen) * 2 - 1)
        else:
            buf.copy_(torch.randn(buf.shape, device=agent.device, generator=gen))
    replay.size, replay.index = replay.max_size, 0
    return agent, replay


def rate(kind, sizes, stock):
    import torch
    os.environ['TONIC_AMD_TORSO_STOCK'] = '1' if stock else '0'
    agent, replay = build(kind, sizes)
    assert agent.critic_updater.stock == stock and agent.actor_updater.stock == stock

    def one_update():
        return agent.enqueue_update(replay.sample_indices(), agent._draw_noise(ITERATIONS))
    one_update()
    one_update()
    reps, dt = 3, float('inf')
    for _ in range(3):                            # best of three groups
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            infos = one_update()
        infos.cpu()
        dt = min(dt, (time.perf_counter() - t0) / reps)
    return {'kind': kind, 'torso': list(sizes), 'path': 'stock' if stock else 'hip', 'B': B, 'O': O, 'A': A,
            'learner_updates_per_sec': round(ITERATIONS / dt, 1), 'ms_per_update_call': round(dt * 1e3, 2)}


def main():
    sizes = tuple(int(v) for v in sys.argv[1:]) or (256, 256, 256)
    for kind in ('sac', 'td3', 'd4pg', 'mpo'):
        for stock in ((False, True) if kind in ('sac', 'td3') else (False,)):
            print(json.dumps(rate(kind, sizes, stock)), flush=True)


if __name__ == '__main__':
    main()
