"""TEST INFRASTRUCTURE ONLY — golden vectors of SAC and MPO with a Gaussian policy head whose scale bounds are not the
defaults: ``GaussianPolicyHead(..., scale_min=0.2, scale_max=1.5)``.

Runs the *unmodified* reference agents (through ``oracle/reference_loader.py``) in the loop of
``oracle/make_golden.run_offpolicy`` (same synthetic environment, reward noise and terminations, the small shapes of
``sac_small`` / ``mpo_small``) and writes ``tests/golden/{sac,mpo}_scale_small.npz``.  31 loop steps run THREE learner
updates.  ``scale_max`` lies above the default ceiling of 1 and ``scale_min`` above the default floor of 1e-4.  With
the default initialiser the scale head's softplus stays within 0.5 .. 0.85 on these trajectories, inside either pair
of bounds; the head's ``scale_fn`` (an initialiser, which the reference applies to the scale layer) therefore
multiplies the layer's initial weights by ``SCALE_GAIN``, without drawing anything, so that the softplus spans about
0.01 .. 4: a kernel that clamps to the defaults acts and learns differently from these files, which the script
asserts (shares of the acting steps' scales below 0.2 and above 1).

Every loop step records the stochastic action of ``agent.step`` (and the standard-normal draws behind it) and the
greedy one of ``agent.test_step``.  Every update is captured as in ``scripts/make_offpolicy_return_goldens.py``: the
index stream of ``Buffer.get``, the updaters' standard-normal draws (regenerated from the generator state saved in
front of the update and checked), the logged infos and the model's state after it — for MPO also the dual variables
in front of and after it.  Nothing touches the model between two updates, which the script asserts: ``pre{u}`` IS
``post{u-1}`` (``init`` for the first), so only ``init/`` and ``post{u}/`` are stored.  ``buffer/``: the filled rows
of the replay buffer in front of the first update.

    python scripts/make_policy_head_goldens.py                  # both fixtures, 1 torch thread
    python scripts/make_policy_head_goldens.py --out DIR NAME   # one fixture, elsewhere

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

# name -> run arguments: the shapes and seeds of make_golden.main's sac_small / mpo_small
CASES = {
    'sac_scale_small': dict(kind='sac', obs_dim=11, act_dim=3, workers=4, hidden=32, batch=24, iterations=6, seed=0,
                            return_steps=1, samples=1),
    'mpo_scale_small': dict(kind='mpo', obs_dim=9, act_dim=3, workers=3, hidden=32, batch=20, iterations=6, seed=11,
                            return_steps=2, samples=4),
}
SCALE_MIN, SCALE_MAX = 0.2, 1.5
SCALE_GAIN = 16.0


def widen_scale_layer(module):
    """`scale_fn` of the head: the scale layer's initial weights times SCALE_GAIN (tests build the same head)."""
    if isinstance(module, torch.nn.Linear):
        with torch.no_grad():
            module.weight.mul_(SCALE_GAIN)
LOOP_STEPS = 31
DUALS = ('log_temperature', 'log_alpha_mean', 'log_alpha_std', 'log_penalty_temperature')


def run(tonic, name, kind, obs_dim, act_dim, workers, hidden, batch, iterations, seed, return_steps, samples):
    models, updaters = tonic.torch.models, tonic.torch.updaters
    sizes = (hidden, hidden)

    def builder():
        return rl.SyntheticEnvironment(obs_dim, act_dim, max_episode_steps=5)
    env = tonic.environments.distribute(builder, 1, workers)
    env.initialize(seed=seed)
    critic = models.Critic(encoder=models.ObservationActionEncoder(), torso=models.MLP(sizes, torch.nn.ReLU),
                           head=models.ValueHead())
    if kind == 'sac':
        head = models.GaussianPolicyHead(loc_activation=torch.nn.Identity, scale_min=SCALE_MIN, scale_max=SCALE_MAX,
                                         scale_fn=widen_scale_layer,
                                         distribution=models.SquashedMultivariateNormalDiag)
    else:
        head = models.GaussianPolicyHead(scale_min=SCALE_MIN, scale_max=SCALE_MAX, scale_fn=widen_scale_layer)
    container = models.ActorTwinCriticWithTargets if kind == 'sac' else models.ActorCriticWithTargets
    model = container(
        actor=models.Actor(encoder=models.ObservationEncoder(), torso=models.MLP(sizes, torch.nn.ReLU), head=head),
        critic=critic, observation_normalizer=tonic.torch.normalizers.MeanStd())
    replay = tonic.replays.Buffer(size=400, batch_iterations=iterations, batch_size=batch,
                                  steps_before_batches=workers * 10, steps_between_batches=workers * 10,
                                  return_steps=return_steps)
    if kind == 'sac':
        agent = tonic.torch.agents.SAC(model=model, replay=replay,
                                       exploration=tonic.explorations.NoActionNoise(start_steps=workers * 5))
    else:
        agent = tonic.torch.agents.MPO(
            model=model, replay=replay,
            actor_updater=updaters.MaximumAPosterioriPolicyOptimization(num_samples=samples),
            critic_updater=updaters.ExpectedSARSA(num_samples=samples))
    agent.initialize(env.observation_space, env.action_space, seed=seed)
    out = mg.state_arrays('init/', agent.model.state_dict())
    recorder = mg.RecordingLogger()
    tonic.logger.current_logger = recorder
    rng = np.random.RandomState(seed + 1)
    observations = env.start()
    raw_scales = []
    steps = {k: [] for k in ('observations', 'actions', 'greedy_actions', 'next_observations', 'rewards', 'resets',
                             'terminations', 'policy_eps')}
    updates = []
    last = {k: v.detach().numpy().copy() for k, v in agent.model.state_dict().items()}
    original_update = agent._update

    def duals():
        return np.concatenate([getattr(agent.actor_updater, k).detach().numpy().reshape(-1) for k in DUALS])

    def capturing_update(at):
        u = len(updates)
        state = {k: v.detach().numpy() for k, v in agent.model.state_dict().items()}
        for k, v in state.items():          # pre{u} is post{u-1} (init): nothing moves the model between updates
            assert np.array_equal(v, last[k]), (u, k)
        torch_state = torch.get_rng_state()
        index_rng = np.random.RandomState()
        index_rng.set_state(agent.replay.np_random.get_state())
        size = agent.replay.size
        pre = f'u{u}/'
        if kind == 'mpo':
            out[pre + 'duals_pre'] = duals()
        if u == 0:
            for k, v in agent.replay.buffers.items():
                out['buffer/' + k] = v[:size].copy()
        original_update(at)
        out[pre + 'indices'] = np.array([index_rng.randint(size * workers, size=batch) for _ in range(iterations)])
        after = torch.get_rng_state()
        torch.set_rng_state(torch_state)
        # SAC: rsample of the critic step, of the actor step; MPO: rsample((S,)) of the critic step, sample((S,)) of
        # the actor step — standard normals of [B, A] / [S, B, A] each
        out[pre + 'eps'] = np.array([[torch.randn(samples, batch, act_dim).numpy().reshape(-1, act_dim)
                                      for _ in range(2)] for _ in range(iterations)])
        assert torch.equal(torch.get_rng_state(), after), 'the update drew something else'
        torch.set_rng_state(after)
        assert np.array_equal(index_rng.get_state()[1], agent.replay.np_random.get_state()[1])
        out[pre + 'buffer_size'] = np.int64(size)
        out[pre + 'step'] = np.int64(at)
        for k, v in recorder.records.items():
            v = np.array(v)
            if k.startswith('actor/alpha'):
                out[pre + 'info/' + k] = v
            else:
                out[pre + 'info/' + k + ('_mean' if v.ndim == 2 else '')] = v.mean(axis=1) if v.ndim == 2 else v
        recorder.records.clear()
        if kind == 'mpo':
            out[pre + 'duals_post'] = duals()
        out.update(mg.state_arrays(f'post{u}/', agent.model.state_dict()))
        last.update({k: v.detach().numpy().copy() for k, v in agent.model.state_dict().items()})
        updates.append(at)
    agent._update = capturing_update
    for t in range(LOOP_STEPS):
        with torch.no_grad():
            actor = agent.model.actor
            hidden_out = actor.torso(actor.encoder(torch.as_tensor(observations, dtype=torch.float32)))
            raw_scales.append(actor.head.scale_layer(hidden_out).numpy())
        steps['greedy_actions'].append(np.array(agent.test_step(observations, t * workers), np.float64))
        gen_state = torch.get_rng_state()
        actions = agent.step(observations, t * workers)
        after = torch.get_rng_state()
        torch.set_rng_state(gen_state)
        steps['policy_eps'].append(torch.randn(workers, act_dim).numpy())
        torch.set_rng_state(after)
        steps['observations'].append(observations.copy())
        steps['actions'].append(np.array(actions, np.float64))
        observations, infos = env.step(actions)
        infos['rewards'] = (infos['rewards'] + rng.normal(size=workers)).astype(np.float32)
        term = rng.uniform(size=workers) < 0.1
        infos['terminations'] = term
        infos['resets'] = infos['resets'] | term
        steps['next_observations'].append(np.array(infos['observations']).copy())
        for k in ('rewards', 'resets', 'terminations'):
            steps[k].append(np.array(infos[k]).copy())
        agent.update(**infos, steps=t * workers)
    assert len(updates) == 3, updates
    raw_scales = np.array(raw_scales)
    below, above = float((raw_scales < SCALE_MIN).mean()), float((raw_scales > 1.0).mean())
    print(f'{name}: softplus of the scale head {raw_scales.min():.3f} .. {raw_scales.max():.3f}, {below:.2f} below '
          f'{SCALE_MIN}, {above:.2f} above 1, {float((raw_scales > SCALE_MAX).mean()):.2f} above {SCALE_MAX}')
    assert below >= 0.05 and above >= 0.05, (below, above)
    for k, v in steps.items():
        out['act/' + k] = np.array(v)
    out['torso_sizes'] = np.array(sizes, np.int64)
    out['torso_activation'] = np.array('ReLU')
    out['scale_bounds'] = np.array([SCALE_MIN, SCALE_MAX], np.float64)
    out['scale_gain'] = np.float64(SCALE_GAIN)
    out['return_steps'] = np.int64(return_steps)
    out['samples'] = np.int64(samples)
    out['updates'] = np.array(updates, np.int64)
    out['cfg'] = np.array([obs_dim, act_dim, workers, hidden, batch, iterations, seed, LOOP_STEPS], np.int64)
    mg.save(name, source='tonic/torch/agents/sac.py:40-51; mpo.py:42-109 with models/actors.py:69-98 '
                         'GaussianPolicyHead(scale_min=0.2, scale_max=1.5)', **out)


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
