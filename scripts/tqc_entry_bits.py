"""The sha256 of what TQC's entries write — tonic_truncated_quantile_q_grad and tonic_truncated_quantile_actor_grad
through updaters.TruncatedQuantileQLearning and TwinCriticQuantileSoftPolicyGradient on a twin model, and the
tonic_ensemble_quantile_* pair through the same updaters on models.ActorCriticEnsembleWithTargets (the cases with
an N) — at seeded inputs, as one JSON object: the sibling of
scripts/offpolicy_entry_bits.py for the entries its cases do not reach.  Two commits compute the same bits exactly when
their outputs here are identical (the two statistics rows are also kept as values, for a digest that differs):

    python scripts/tqc_entry_bits.py [--tree <a built checkout>] --out bits.json

(--tree: the checkout whose package and library run; unset: this one.  The script uses nothing a commit that has
agents.TQC and the ensemble model lacks.)  One fresh process per build."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    # name: (sizes, activation, B, M, drop, O, A[, N: an ensemble of N critics])
    'one_row': ((32, 32), 'ReLU', 1, 2, 1, 3, 1),
    'ragged': ((32, 32), 'ReLU', 5, 25, 2, 17, 6),
    'full_wave': ((32, 32), 'ReLU', 37, 32, 2, 17, 6),
    'tanh_layers': ((48, 40, 32), 'Tanh', 37, 25, 2, 17, 6),
    'wide': ((256, 256), 'ReLU', 37, 25, 2, 17, 6),
    'batch': ((256, 256), 'ReLU', 256, 25, 2, 17, 6),
    'nothing_dropped': ((64, 64), 'ReLU', 33, 7, 0, 17, 6),
    'ensemble_of_two': ((32, 32), 'ReLU', 5, 7, 2, 17, 6, 2),
    'ensemble_of_five': ((32, 32), 'ReLU', 37, 25, 2, 17, 6, 5),
    'ensemble_of_eight': ((32, 32), 'ReLU', 37, 32, 2, 17, 6, 8),
}


def digest(tensor):
    return hashlib.sha256(tensor.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(tt, tonic_amd, np, torch, case, tuned):
    from tonic_amd.environments import Box
    from tonic_amd.torch.models import network_variables
    sizes, activation, B, M, drop, O, A = CASES[case][:7]
    N = CASES[case][7] if len(CASES[case]) > 7 else 0
    act = getattr(torch.nn, activation)
    head = tt.models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                        distribution=tt.models.SquashedMultivariateNormalDiag)
    container = tt.models.ActorTwinCriticWithTargets
    if N:
        container = lambda **parts: tt.models.ActorCriticEnsembleWithTargets(num_critics=N, **parts)      # noqa: E731
    model = container(
        actor=tt.models.Actor(encoder=tt.models.ObservationEncoder(), torso=tt.models.MLP(sizes, act), head=head),
        critic=tt.models.Critic(encoder=tt.models.ObservationActionEncoder(), torso=tt.models.MLP(sizes, act),
                                head=tt.models.QuantileValueHead(M)),
        observation_normalizer=tt.normalizers.MeanStd())
    tuner = tt.updaters.EntropyCoeffTuning(initial_entropy_coeff=0.35, target_entropy=-2.5) if tuned else None
    agent = tt.agents.TQC(
        model=model,
        replay=tonic_amd.replays.Buffer(size=1000, batch_iterations=1, batch_size=B, steps_before_batches=0,
                                        steps_between_batches=1),
        critic_updater=tt.updaters.TruncatedQuantileQLearning(top_quantiles_to_drop_per_net=drop),
        actor_updater=tt.updaters.TwinCriticQuantileSoftPolicyGradient(), entropy_coeff_updater=tuner)
    agent.initialize(Box(-np.inf, np.inf, (O,)), Box(-1, 1, (A,)), seed=9)
    rng = np.random.RandomState(B + M)
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32)).cuda()              # noqa: E731
    with torch.no_grad():          # the targets away from the online critics and from each other: a sort with work to do
        for critic in (getattr(model, f'target_critic_{z}') for z in range(1, (N or 2) + 1)):
            for p in network_variables(critic):
                p += f32(rng.normal(size=tuple(p.shape)) * 0.1)
            critic.head.quantile_layer.weight.mul_(8.0)
            critic.head.quantile_layer.bias.add_(f32(rng.normal(size=M)))
        agent.model.observation_normalizer._mean.copy_(f32(rng.normal(size=O) * 0.3))
        agent.model.observation_normalizer._std.copy_(f32(0.5 + rng.uniform(size=O)))
    batch = dict(observations=f32(rng.normal(size=(B, O))), actions=f32(rng.uniform(-1, 1, (B, A))),
                 next_observations=f32(rng.normal(size=(B, O))), rewards=f32(rng.normal(size=B) * 2),
                 discounts=f32(np.full(B, 0.99) * (rng.uniform(size=B) > 0.1)))
    eps = f32(rng.normal(size=(2, B, A)))
    info, out = torch.zeros(8, device='cuda'), {}
    agent.critic_updater.enqueue(batch, eps[0], info)
    torch.cuda.synchronize()
    out['critic_grad_sums'], out['critic_info'] = digest(agent.critic_updater.grad_sums), digest(info)
    out['critic_info_values'] = info.double().tolist()
    agent.actor_updater.enqueue(batch['observations'], eps[1], info)
    torch.cuda.synchronize()
    out['actor_grad_sums'], out['actor_info'] = digest(agent.actor_updater.grad_sums), digest(info)
    out['actor_info_values'] = info.double().tolist()
    if tuned:
        out['coefficient_sums'] = digest(tuner.grad_sums)
    out['online_after_the_steps'] = digest(agent.model.flat_online)
    agent.close()
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--tree', default=ROOT)
    parser.add_argument('--out', required=True)
    args = parser.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    import tonic_amd
    import tonic_amd.torch as tt
    from tonic_amd import _lib
    assert os.path.abspath(tonic_amd.__file__).startswith(os.path.abspath(args.tree)), tonic_amd.__file__
    assert torch.cuda.is_available(), 'the entries run on the GPU'
    bits = {f'{case}-{"device" if tuned else "float"}': run_case(tt, tonic_amd, np, torch, case, tuned)
            for case in CASES for tuned in (False, True)}
    with open(args.out, 'w') as out:
        json.dump(dict(abi=int(_lib.load().tonic_abi_version()), cases=len(bits), sha256=bits), out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
