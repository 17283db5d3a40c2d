"""TEST INFRASTRUCTURE ONLY — golden vectors of DDPG / TD3 / SAC with a Return normaliser.

Runs the *unmodified* reference agents (through ``oracle/reference_loader.py``) with
``ActorCriticWithTargets / ActorTwinCriticWithTargets(..., return_normalizer=Return(0.99))`` in the loop of
``oracle/make_golden.run_offpolicy`` (same synthetic environment, reward noise and terminations, the small shapes of
``sac_small`` / ``td3_small`` / ``ddpg_small``) and writes ``tests/golden/{sac,td3,ddpg}_return_small.npz``.  The
rewards are scaled by 3 so that the recorded range leaves [-1, 1]; 31 loop steps run THREE learner updates, the
second and third with a moved ``[_low, _high]``.

Every update is captured: the index stream of ``Buffer.get`` and the updaters' standard-normal draws (regenerated
from the generator states saved in front of the update, as ``run_offpolicy`` does), the logged infos, the reward
range and the model's state after it.  Nothing touches the model between two updates (the normalisers only move in
``_update``), which the script asserts: ``pre{u}`` IS ``post{u-1}`` (``init`` for the first), so only ``init/`` and
``post{u}/`` are stored and the files stay the size of their ``*_small`` siblings.

    python scripts/make_offpolicy_return_goldens.py                  # every fixture, 1 torch thread
    python scripts/make_offpolicy_return_goldens.py --out DIR NAME   # one fixture, elsewhere

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

# name -> (kind, run arguments): the shapes and seeds of make_golden.main's *_small cases
CASES = {
    'sac_return_small': dict(kind='sac', obs_dim=11, act_dim=3, workers=4, hidden=32, batch=24, iterations=6, seed=0),
    'td3_return_small': dict(kind='td3', obs_dim=9, act_dim=4, workers=3, hidden=32, batch=20, iterations=6, seed=3),
    'ddpg_return_small': dict(kind='ddpg', obs_dim=7, act_dim=2, workers=2, hidden=32, batch=16, iterations=6,
                              seed=5),
}
DISCOUNT = 0.99
REWARD_SCALE = 3.0
LOOP_STEPS = 31


def run(tonic, name, kind, obs_dim, act_dim, workers, hidden, batch, iterations, seed):
    models = tonic.torch.models
    sizes = (hidden, hidden)

    def builder():
        return rl.SyntheticEnvironment(obs_dim, act_dim, max_episode_steps=5)
    env = tonic.environments.distribute(builder, 1, workers)
    env.initialize(seed=seed)
    critic = models.Critic(encoder=models.ObservationActionEncoder(), torso=models.MLP(sizes, torch.nn.ReLU),
                           head=models.ValueHead())
    if kind == 'sac':
        head = models.GaussianPolicyHead(loc_activation=torch.nn.Identity,
                                         distribution=models.SquashedMultivariateNormalDiag)
    else:
        head = models.DeterministicPolicyHead()
    container = models.ActorCriticWithTargets if kind == 'ddpg' else models.ActorTwinCriticWithTargets
    model = container(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, torch.nn.ReLU), head=head),
        critic=critic, observation_normalizer=tonic.torch.normalizers.MeanStd(),
        return_normalizer=tonic.torch.normalizers.Return(DISCOUNT))
    replay = tonic.replays.Buffer(size=400, batch_iterations=iterations, batch_size=batch,
                                  steps_before_batches=workers * 10, steps_between_batches=workers * 10)
    if kind == 'sac':
        agent = tonic.torch.agents.SAC(model=model, replay=replay,
                                       exploration=tonic.explorations.NoActionNoise(start_steps=workers * 5))
    else:
        cls = {'ddpg': tonic.torch.agents.DDPG, 'td3': tonic.torch.agents.TD3}[kind]
        agent = cls(model=model, replay=replay,
                    exploration=tonic.explorations.NormalActionNoise(start_steps=workers * 5))
    agent.initialize(env.observation_space, env.action_space, seed=seed)
    out = mg.state_arrays('init/', agent.model.state_dict())
    recorder = mg.RecordingLogger()
    tonic.logger.current_logger = recorder
    rng = np.random.RandomState(seed + 1)
    observations = env.start()
    steps = {k: [] for k in ('observations', 'actions', 'next_observations', 'rewards', 'resets', 'terminations',
                             'policy_eps')}
    draws = 2 if kind == 'sac' else 1
    updates = []
    last = {k: v.detach().numpy().copy() for k, v in agent.model.state_dict().items()}
    original_update = agent._update

    def capturing_update(at):
        u = len(updates)
        state = {k: v.detach().numpy() for k, v in agent.model.state_dict().items()}
        for k, v in state.items():          # pre{u} is post{u-1} (init): nothing moves the model between updates
            assert np.array_equal(v, last[k]), (u, k)
        torch_state = torch.get_rng_state()
        index_rng = np.random.RandomState()
        index_rng.set_state(agent.replay.np_random.get_state())
        size = agent.replay.size
        original_update(at)
        pre = f'u{u}/'
        out[pre + 'indices'] = np.array([index_rng.randint(size * workers, size=batch) for _ in range(iterations)])
        after = torch.get_rng_state()
        torch.set_rng_state(torch_state)
        out[pre + 'eps'] = np.array([[torch.randn(batch, act_dim).numpy() for _ in range(draws)]
                                     for _ in range(iterations)])
        if kind != 'ddpg':        # (DDPG's updaters draw nothing: the generator did not move)
            assert torch.equal(torch.get_rng_state(), after), 'the update drew something else'
        torch.set_rng_state(after)
        assert np.array_equal(index_rng.get_state()[1], agent.replay.np_random.get_state()[1])
        out[pre + 'buffer_size'] = np.int64(size)
        out[pre + 'step'] = np.int64(at)
        for k, v in recorder.records.items():
            v = np.array(v)
            out[pre + 'info/' + k + ('_mean' if v.ndim == 2 else '')] = v.mean(axis=1) if v.ndim == 2 else v
        recorder.records.clear()
        rn = agent.model.return_normalizer
        out[pre + 'return/range'] = np.array([rn.min_reward, rn.max_reward], np.float32)
        out.update(mg.state_arrays(f'post{u}/', agent.model.state_dict()))
        last.update({k: v.detach().numpy().copy() for k, v in agent.model.state_dict().items()})
        updates.append(at)
    agent._update = capturing_update
    for t in range(LOOP_STEPS):
        gen_state = torch.get_rng_state()
        actions = agent.step(observations, t * workers)
        after = torch.get_rng_state()
        torch.set_rng_state(gen_state)
        steps['policy_eps'].append(torch.randn(workers, act_dim).numpy())      # consumed only by SAC's policy
        torch.set_rng_state(after)
        steps['observations'].append(observations.copy())
        steps['actions'].append(np.array(actions, np.float64))
        observations, infos = env.step(actions)
        infos['rewards'] = (infos['rewards'] * REWARD_SCALE + rng.normal(size=workers)).astype(np.float32)
        term = rng.uniform(size=workers) < 0.1
        infos['terminations'] = term
        infos['resets'] = infos['resets'] | term
        steps['next_observations'].append(np.array(infos['observations']).copy())
        for k in ('rewards', 'resets', 'terminations'):
            steps[k].append(np.array(infos[k]).copy())
        agent.update(**infos, steps=t * workers)
    assert len(updates) == 3, updates
    for k, v in steps.items():
        out['act/' + k] = np.array(v)
    out['torso_sizes'] = np.array(sizes, np.int64)
    out['torso_activation'] = np.array('ReLU')
    out['discount_factor'] = np.float64(DISCOUNT)
    out['reward_scale'] = np.float64(REWARD_SCALE)
    out['updates'] = np.array(updates, np.int64)
    out['cfg'] = np.array([obs_dim, act_dim, workers, hidden, batch, iterations, seed, LOOP_STEPS], np.int64)
    mg.save(name, source='tonic/torch/agents/ddpg.py:45-112; td3.py:38-55; sac.py:40-51 with normalizers/returns.py:'
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
