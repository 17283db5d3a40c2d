"""TEST INFRASTRUCTURE ONLY — golden vectors of the on-policy agents with a Return normaliser.

Runs the *unmodified* reference agents (through ``oracle/reference_loader.py``) with
``ActorCritic(..., return_normalizer=tonic.torch.normalizers.Return(0.99))`` in the loop of
``oracle/make_golden.run_ppo`` (same synthetic environment, reward noise and terminations) and writes
``tests/golden/*_return_small.npz``.  The rewards are scaled so that the recorded range grows from one
update to the next: updates 2 and 3 evaluate and regress with a moved ``[_low, _high]``.

    python scripts/make_return_goldens.py                  # every fixture, 1 torch thread
    python scripts/make_return_goldens.py --out DIR NAME   # one fixture, elsewhere (the host test compares)

Needs the reference checkout; the GPU tests read only the committed ``.npz`` files.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import make_golden as mg            # noqa: E402
import reference_loader as rl       # noqa: E402

# name -> run arguments (O, A, workers, steps, seed, iterations, updates, algorithm, reward scale, torso)
CASES = {
    'ppo_return_small': dict(obs_dim=17, act_dim=6, workers=8, steps=24, seed=31, iterations=8, updates=3,
                             algorithm='PPO', reward_scale=3.0),
    'a2c_return_small': dict(obs_dim=17, act_dim=6, workers=8, steps=24, seed=32, iterations=6, updates=3,
                             algorithm='A2C', reward_scale=3.0),
    'trpo_return_small': dict(obs_dim=17, act_dim=6, workers=8, steps=24, seed=33, iterations=6, updates=3,
                              algorithm='TRPO', reward_scale=3.0),
    'ppo_wide_return_small': dict(obs_dim=111, act_dim=8, workers=6, steps=16, seed=34, iterations=8,
                                  updates=3, algorithm='PPO', reward_scale=3.0),
    'ppo_tanh3_return_small': dict(obs_dim=11, act_dim=3, workers=6, steps=20, seed=35, iterations=8,
                                   updates=3, algorithm='PPO', reward_scale=3.0,
                                   torso=((96, 48, 32), 'Tanh')),
}
DISCOUNT = 0.99


def run(tonic, name, obs_dim, act_dim, workers, steps, seed, iterations, updates, algorithm, reward_scale,
        torso=None):
    """make_golden.run_ppo's loop with a Return normaliser on the model."""
    def builder():
        return rl.SyntheticEnvironment(obs_dim, act_dim, max_episode_steps=7)
    env = tonic.environments.distribute(builder, 1, workers)
    env.initialize(seed=seed)
    models, norms = tonic.torch.models, tonic.torch.normalizers
    sizes, activation = torso if torso is not None else ((64, 64), 'Tanh')
    act = getattr(torch.nn, activation)
    model = models.ActorCritic(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(tuple(sizes), act),
                           head=models.DetachedScaleGaussianPolicyHead()),
        critic=models.Critic(encoder=models.ObservationEncoder(), torso=models.MLP(tuple(sizes), act),
                             head=models.ValueHead()),
        observation_normalizer=norms.MeanStd(),
        return_normalizer=norms.Return(DISCOUNT))
    kwargs = dict(model=model)
    if algorithm == 'A2C':
        kwargs['actor_updater'] = tonic.torch.updaters.StochasticPolicyGradient()
    agent = getattr(tonic.torch.agents, algorithm)(
        replay=tonic.replays.Segment(size=steps, batch_iterations=iterations), **kwargs)
    agent.initialize(env.observation_space, env.action_space, seed=seed)
    out = mg.state_arrays('init/', agent.model.state_dict())
    out['torso_sizes'] = np.array(sizes, np.int64)
    out['torso_activation'] = np.array(activation)
    out['discount_factor'] = np.float64(DISCOUNT)
    out['reward_scale'] = np.float64(reward_scale)
    out['algorithm'] = np.array(algorithm)
    recorder = mg.RecordingLogger()
    tonic.logger.current_logger = recorder
    observations = env.start()
    act_all, obs_all = [], []
    rng = np.random.RandomState(seed + 1)
    for update in range(updates):
        for t in range(steps):
            actions = agent.step(observations, t * workers)
            act_all.append(actions.copy())
            obs_all.append(observations.copy())
            observations, infos = env.step(actions)
            infos['rewards'] = (infos['rewards'] * reward_scale +
                                rng.normal(size=workers)).astype(np.float32)
            term = rng.uniform(size=workers) < 0.05
            infos['terminations'] = term
            infos['resets'] = infos['resets'] | term
            if t == steps - 1:
                out.update(mg.state_arrays(f'pre{update}/', agent.model.state_dict()))
            agent.update(**infos, steps=t * workers)
        seg = {k: v.copy() for k, v in agent.replay.buffers.items()}
        pre = f'u{update}/'
        for k in ('rewards', 'values', 'returns'):
            out[pre + 'segment/' + k] = seg[k]
        out.update(mg.state_arrays(f'post{update}/', agent.model.state_dict()))
        for k, v in recorder.records.items():
            if k == 'critic/v':
                out[pre + 'info/critic/v_mean'] = np.array([x.mean() for x in v])
            else:
                out[pre + 'info/' + k] = np.array(v)
        recorder.records.clear()
        rn = agent.model.return_normalizer
        out[pre + 'return/range'] = np.array([rn.min_reward, rn.max_reward], np.float32)
    out['act/observations'] = np.array(obs_all)
    out['act/actions'] = np.array(act_all)
    out['cfg'] = np.array([obs_dim, act_dim, workers, steps, seed, iterations, updates], np.int64)
    mg.save(name, source='tonic/torch/agents/{a2c,ppo,trpo}.py with normalizers/returns.py:'
                         'Return(0.99) (models/critics.py:15-20)', **out)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('names', nargs='*', default=list(CASES))
    parser.add_argument('--out', default=None, help='directory to write to (default tests/golden)')
    args = parser.parse_args()
    torch.set_num_threads(1)
    if args.out:
        mg.OUT = args.out
    tonic = rl.load_reference()
    for name in args.names:
        run(tonic, name, **CASES[name])


if __name__ == '__main__':
    main()
