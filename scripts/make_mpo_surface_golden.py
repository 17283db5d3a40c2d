"""TEST INFRASTRUCTURE ONLY — golden vectors of MPO's constructor surface beyond the defaults.

Drives the *unmodified* reference's ``ExpectedSARSA`` and ``MaximumAPosterioriPolicyOptimization`` (through
``oracle/reference_loader.py``) directly, on the CPU, on one tiny fixed problem (O = 9, A = 3, torso (32, 32) ReLU,
B = 20, the shapes of ``mpo_small``): one critic step, one actor / dual step and the target update, in the order of
``agents/mpo.py:102-109``.  Writes ``tests/golden/mpo_surface_small.npz`` with three cases:

    a  per_dim_constraining=False, 4 samples in both updaters
    b  per_dim_constraining=False, 3 samples in ExpectedSARSA and 7 in the actor step
    c  per-dimension constraints, 100 samples in both

Every case starts from the same networks (``pre/``: the seeded initialisation with the ONLINE actor's head moved
away from the target's, so that both KLs are first order; a target network whose tensor is not stored equals the
online one), the same batch and the same initial duals.  Per case: the standard-normal draws in the order the
updaters consume them (regenerated from the generator state saved in front of the step, and verified: the
generator ends in the state the reference left it in, and a replay of the step from that state on fresh updaters
gives the same parameters), the duals before and after, every returned info and the online parameters after
(``<case>/post``: the tensors named by ``post_keys``, flattened, end to end).

    python scripts/make_mpo_surface_golden.py             # 1 torch thread
    python scripts/make_mpo_surface_golden.py --out DIR   # elsewhere (the host test compares)

Needs the reference checkout; the GPU tests read only the committed ``.npz`` file.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import reference_loader as rl       # noqa: E402

NAME = 'mpo_surface_small'
O, A, B, SIZES, SEED = 9, 3, 20, (32, 32), 61
# case -> (per_dim_constraining, ExpectedSARSA's samples, the actor step's samples)
CASES = {'a': (False, 4, 4), 'b': (False, 3, 7), 'c': (True, 100, 100)}
# initial log-duals away from the defaults, so that a swapped slot shows
DUALS = dict(initial_log_temperature=0.5, initial_log_alpha_mean=-0.7, initial_log_alpha_std=2.0)


def build(tonic, per_dim, S_c, S_a):
    """The model of agents/mpo.py:7-18 on the small torso and the two updaters, initialised from SEED."""
    models, updaters = tonic.torch.models, tonic.torch.updaters
    torch.manual_seed(SEED)
    model = models.ActorCriticWithTargets(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(SIZES, torch.nn.ReLU),
                           head=models.GaussianPolicyHead()),
        critic=models.Critic(encoder=models.ObservationActionEncoder(), torso=models.MLP(SIZES, torch.nn.ReLU),
                             head=models.ValueHead()),
        observation_normalizer=tonic.torch.normalizers.MeanStd())
    observation_space, action_space = rl.SyntheticSpace(-np.inf, np.inf, (O,)), rl.SyntheticSpace(-1, 1, (A,))
    model.initialize(observation_space, action_space)
    actor = updaters.MaximumAPosterioriPolicyOptimization(num_samples=S_a, per_dim_constraining=per_dim, **DUALS)
    critic = updaters.ExpectedSARSA(num_samples=S_c)
    actor.initialize(model, action_space)
    critic.initialize(model)
    return model, actor, critic


def problem():
    """The batch, the normaliser's statistics and the offsets of the online actor's head (data, one RandomState)."""
    rng = np.random.RandomState(SEED)
    f32 = lambda a: np.asarray(a, np.float32)                          # noqa: E731
    batch = dict(observations=f32(rng.normal(size=(B, O))), actions=f32(rng.uniform(-1, 1, (B, A))),
                 next_observations=f32(rng.normal(size=(B, O))), rewards=f32(rng.normal(size=B)),
                 discounts=f32(0.99 * (rng.uniform(size=B) > 0.15)))
    seen = f32(rng.normal(size=(50, O)) * 1.5 + 0.3)
    return batch, seen, rng


def prepare(model, seen, rng):
    model.observation_normalizer.record(seen)
    model.observation_normalizer.update()
    with torch.no_grad():
        for p in model.actor.head.parameters():
            p += torch.as_tensor(rng.normal(size=tuple(p.shape)) * 0.05, dtype=torch.float32)


def duals_of(actor):
    return np.concatenate([v.detach().numpy().ravel() for v in actor.dual_variables])


def step(model, actor, critic, batch):
    tensors = {k: torch.as_tensor(v) for k, v in batch.items()}
    critic_infos = critic(**tensors)
    actor_infos = actor(tensors['observations'])
    model.update_targets()
    return critic_infos, actor_infos


def online(prefix, model):
    return {prefix + k: v.detach().numpy().copy() for k, v in model.state_dict().items()
            if not k.startswith('target_')}


def trained(model):
    """The online actor's and critic's tensors in state-dict order: (names, one flat vector)."""
    items = [(k, v) for k, v in model.state_dict().items()
             if k.startswith(('actor.', 'critic.')) and 'normalizer' not in k]
    return np.array([k for k, _ in items]), np.concatenate([v.detach().numpy().ravel() for _, v in items])


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = parser.parse_args()
    torch.set_num_threads(1)
    tonic = rl.load_reference()
    out = dict(cfg=np.array([O, A, B, SEED], np.int64), torso_sizes=np.array(SIZES, np.int64),
               cases=np.array(sorted(CASES)))
    for key, value in DUALS.items():
        out['duals/' + key] = np.float64(value)
    for case, (per_dim, S_c, S_a) in sorted(CASES.items()):
        batch, seen, rng = problem()
        model, actor, critic = build(tonic, per_dim, S_c, S_a)
        prepare(model, seen, rng)
        pre = {k: v.detach().clone() for k, v in model.state_dict().items()}
        if case == 'a':
            for k, v in batch.items():
                out['batch/' + k] = v
            out.update(online('pre/', model))
            for k, v in pre.items():            # the target tensors that differ from their online twins
                if k.startswith('target_') and not torch.equal(v, pre[k[len('target_'):]]):
                    out['pre/' + k] = v.numpy().copy()
        torch.manual_seed(SEED + 1)
        start = torch.get_rng_state()
        duals_before = duals_of(actor)
        critic_infos, actor_infos = step(model, actor, critic, batch)
        end = torch.get_rng_state()
        # the draws, in the updaters' order (critics.py:260 rsample((S_c,)), actors.py:359 sample((S_a,)))
        torch.set_rng_state(start)
        eps_critic, eps_actor = torch.randn(S_c, B, A).numpy(), torch.randn(S_a, B, A).numpy()
        assert torch.equal(torch.get_rng_state(), end), 'the updaters consumed something else'
        # ... and a replay from the saved state on fresh updaters lands on the same parameters
        model2, actor2, critic2 = build(tonic, per_dim, S_c, S_a)
        model2.load_state_dict(pre)
        torch.set_rng_state(start)
        step(model2, actor2, critic2, batch)
        for (k, v), w in zip(model.state_dict().items(), model2.state_dict().values()):
            assert torch.equal(v, w), k
        assert np.array_equal(duals_of(actor), duals_of(actor2))
        at = f'{case}/'
        out[at + 'per_dim_constraining'], out[at + 'samples'] = np.bool_(per_dim), np.array([S_c, S_a], np.int64)
        out[at + 'eps_critic'], out[at + 'eps_actor'] = eps_critic.reshape(S_c * B, A), eps_actor.reshape(S_a * B, A)
        out[at + 'duals_before'], out[at + 'duals_after'] = duals_before, duals_of(actor)
        out[at + 'info/critic/loss'] = critic_infos['loss'].numpy()
        out[at + 'info/critic/q_mean'] = critic_infos['q'].numpy().mean()
        for k, v in actor_infos.items():
            out[at + 'info/actor/' + k] = v.numpy()
        # (one vector per case, the tensors of `post_keys` end to end: a member per tensor and case would weigh more
        #  than the numbers)
        out['post_keys'], out[at + 'post'] = trained(model)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, NAME + '.npz')
    np.savez_compressed(path, **out)
    print(f'{NAME}: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
