"""The action streams of the exploration wrappers and the scripted agents (tonic/explorations/noisy.py,
tonic/agents/basic.py) on one seeded sequence of observations and resets: `records(tonic)` runs them for
either package (`tonic` = tonic_amd or the reference's tonic) and returns every action array in call order.
oracle/make_golden.py stores the reference's records in tests/golden/reference_dropin.npz; the test
holds this package's records against them bit for bit."""
import numpy as np

EXPLORATIONS = (('NoActionNoise', dict(start_steps=3)),
                ('NormalActionNoise', dict(scale=0.3, start_steps=3)),
                ('OrnsteinUhlenbeckActionNoise', dict(scale=0.4, clip=1.5, start_steps=3)))
SCRIPTED = (('NormalRandom', dict(loc=0.1, scale=0.5)), ('UniformRandom', {}),
            ('OrnsteinUhlenbeck', dict(scale=0.3)), ('Constant', dict(constant=0.25)))


def records(tonic, action_space):
    """{'explore/<name>/<steps>', 'step/<name>/<steps>', 'test_step/<name>/<steps>': actions}: the
    same constructor arguments, seeds, observations and per-worker resets for either package."""
    out = {}
    policy = lambda observations: np.tanh(observations[:, :3] * 0.7).astype(np.float32)
    rng = np.random.RandomState(5)
    for name, kwargs in EXPLORATIONS:
        exploration = getattr(tonic.explorations, name)(**kwargs)
        exploration.initialize(policy, action_space, seed=11)
        for steps in range(12):
            observations = rng.standard_normal((4, 5)).astype(np.float32)
            out[f'explore/{name}/{steps}'] = exploration(observations, steps)
            exploration.update(rng.rand(4) < 0.3)
    for name, kwargs in SCRIPTED:
        agent = getattr(tonic.agents, name)(**kwargs)
        agent.initialize(None, action_space, seed=3)
        for steps in range(8):
            observations = np.zeros((4, 5), np.float32)
            out[f'step/{name}/{steps}'] = agent.step(observations, steps)
            out[f'test_step/{name}/{steps}'] = agent.test_step(observations, steps)
            resets = rng.rand(4) < 0.3
            outcome = (observations, np.zeros(4), resets, resets, steps)
            agent.update(*outcome)
            agent.test_update(*outcome)
    return out
