"""Learning-rate schedules on the host, no GPU: tonic_lr_schedule_value against the `math` restatement
(tests/lr_schedule_ref.py) and the installed torch classes, `updaters.lr_schedule_rule`'s probing and refusals,
tonic_lr_schedule_check, the updaters' signatures, `adam_table` with schedules and the fused route of a scheduled
plain-Adam agent (the stub agents of tests/test_q_update_host.py)."""
import ctypes
import inspect
import math
import struct
import warnings

import numpy as np
import pytest

import lr_schedule_ref as ref
from test_q_update_host import constants, streams, world      # noqa: F401  (`world`: the stub agents' fixture)

torch = pytest.importorskip('torch')

NAMES = list(ref.SCHEDULES)
LR = 3e-4


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def bits(x):
    return struct.pack('<d', x)


def torch_scheduler(name, lr=LR):
    optimizer = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    return optimizer, ref.factory(name)(optimizer)


# ------------------------------------------------------------------------------------------------ the value statement

@pytest.mark.parametrize('name', NAMES)
def test_value_is_the_restatement_bit_for_bit(lib, name):
    """tonic_lr_schedule_value == lr_schedule_ref.value at the edge steps and over the first 64, two base rates."""
    schedule = ref.SCHEDULES[name][1]
    packed = ref.pack(schedule)
    assert lib.tonic_lr_schedule_check(ctypes.byref(packed)) == 0, lib.tonic_last_error()
    for lr in (LR, 1e-3):
        for t in ref.edge_steps(name) + list(range(64)):
            got, want = lib.tonic_lr_schedule_value(ctypes.byref(packed), lr, t), ref.value(schedule, lr, t)
            assert bits(got) == bits(want), (name, lr, t, got, want)
            assert math.isfinite(got) and 0.0 <= got <= lr
    assert lib.tonic_lr_schedule_value(None, LR, 5) == LR            # NULL: the base rate


@pytest.mark.parametrize('name', [n for n in NAMES if len(ref.SCHEDULES[n][1][0]) == 1])
def test_value_is_torchs_closed_form_bit_for_bit(lib, name):
    """... and the installed class's own `_get_closed_form_lr()` at last_epoch = t."""
    packed = ref.pack(ref.SCHEDULES[name][1])
    _, scheduler = torch_scheduler(name)
    for t in ref.edge_steps(name) + list(range(64)):
        scheduler.last_epoch = t
        want = scheduler._get_closed_form_lr()[0]
        got = lib.tonic_lr_schedule_value(ctypes.byref(packed), LR, t)
        assert bits(got) == bits(float(want)), (name, t, got, want)


def test_two_segments_are_the_parts_closed_forms_around_the_milestone(lib):
    """SequentialLR has no closed form of its own: below the milestone the first part's at t, from it on the second
    part's at t - m, both from the same base rate."""
    name = 'warmup-cosine'
    packed = ref.pack(ref.SCHEDULES[name][1])
    _, scheduler = torch_scheduler(name)
    first, second = scheduler._schedulers
    milestone = scheduler._milestones[0]
    for t in ref.edge_steps(name) + list(range(64)):
        part, local = (first, t) if t < milestone else (second, t - milestone)
        part.last_epoch = local
        want = part._get_closed_form_lr()[0]
        assert bits(lib.tonic_lr_schedule_value(ctypes.byref(packed), LR, t)) == bits(float(want)), t


@pytest.mark.parametrize('name', NAMES)
def test_value_follows_the_chainable_steps(lib, name):
    """Within 1e-13 relative of `optimizer.param_groups[0]['lr']` with scheduler.step() after each optimizer.step(),
    over 200 steps (the closed form is the reference; the chainable recursion is not reproduced)."""
    packed = ref.pack(ref.SCHEDULES[name][1])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        optimizer, scheduler = torch_scheduler(name)
        worst = 0.0
        for t in range(200):
            stepped = optimizer.param_groups[0]['lr']
            got = lib.tonic_lr_schedule_value(ctypes.byref(packed), LR, t)
            worst = max(worst, abs(got - stepped) / max(abs(stepped), 1e-300) if stepped != got else 0.0)
            optimizer.step()
            scheduler.step()
    print(f'{name}: {worst:.2e} relative from the chainable rate over 200 steps')
    assert worst <= 1e-13, (name, worst)


# ------------------------------------------------------------------------------------------------ probing, refusals

@pytest.mark.parametrize('name', NAMES)
def test_probing_maps_each_served_class_to_its_struct(name):
    from tonic_amd.torch import updaters
    adam = lambda params: torch.optim.Adam(params, lr=LR)                       # noqa: E731
    for optimizer_factory in (None, adam):
        packed = updaters.lr_schedule_rule(ref.factory(name), optimizer_factory, LR)
        assert ref.unpack(packed) == ref.SCHEDULES[name][1]
        assert packed.reserved == 0 and all(s.reserved == 0 for s in packed.segment)
        assert packed.signature() == ref.pack(ref.SCHEDULES[name][1]).signature()
    assert updaters.lr_schedule_rule(None, adam, LR) is None
    assert updaters.lr_schedule_value(packed, LR, 3) == ref.value(ref.SCHEDULES[name][1], LR, 3)


def refused():
    s = torch.optim.lr_scheduler

    class Mine(s.StepLR):
        pass

    three = lambda o: s.SequentialLR(o, [s.ConstantLR(o, 0.5, 2), s.LinearLR(o, 0.5, 1.0, 3),    # noqa: E731
                                         s.ExponentialLR(o, 0.9)], milestones=[2, 5])
    nested = lambda o: s.SequentialLR(o, [s.ConstantLR(o, 0.5, 2),                               # noqa: E731
                                          s.SequentialLR(o, [s.LinearLR(o, 0.5, 1.0, 3), s.ExponentialLR(o, 0.9)],
                                                         milestones=[3])], milestones=[2])
    return {
        'LambdaLR': (lambda o: s.LambdaLR(o, lambda epoch: 0.5), 'LambdaLR'),
        'MultiplicativeLR': (lambda o: s.MultiplicativeLR(o, lambda epoch: 0.5), 'MultiplicativeLR'),
        'MultiStepLR': (lambda o: s.MultiStepLR(o, [3, 6]), 'MultiStepLR'),
        'OneCycleLR': (lambda o: s.OneCycleLR(o, max_lr=1e-2, total_steps=10), 'OneCycleLR'),
        'CyclicLR': (lambda o: s.CyclicLR(o, 1e-4, 1e-2, cycle_momentum=False), 'CyclicLR'),
        'CosineAnnealingWarmRestarts': (lambda o: s.CosineAnnealingWarmRestarts(o, 5), 'CosineAnnealingWarmRestarts'),
        'ReduceLROnPlateau': (lambda o: s.ReduceLROnPlateau(o), 'ReduceLROnPlateau'),
        'ChainedScheduler': (lambda o: s.ChainedScheduler([s.ConstantLR(o, 0.5, 2), s.ExponentialLR(o, 0.9)]),
                             'ChainedScheduler'),
        'a subclass': (lambda o: Mine(o, 5), 'Mine'),
        'three schedulers': (three, 'SequentialLR of 3'),
        'a nested SequentialLR': (nested, 'nested SequentialLR'),
        'gamma = nan': (lambda o: s.ExponentialLR(o, float('nan')), 'gamma'),
        'gamma = inf': (lambda o: s.StepLR(o, 5, float('inf')), 'gamma'),
        'eta_min = -inf': (lambda o: s.CosineAnnealingLR(o, 5, -float('inf')), 'eta_min'),
        'power = nan': (lambda o: s.PolynomialLR(o, 5, float('nan')), 'power'),
        'a fractional step_size': (lambda o: s.StepLR(o, 2.5), 'step_size'),
        'what torch rejects: factor': (lambda o: s.ConstantLR(o, factor=1.5), 'factor'),
        'what torch rejects: start_factor': (lambda o: s.LinearLR(o, start_factor=0.0), 'factor'),
        'T_max = 0': (lambda o: s.CosineAnnealingLR(o, 0), 'period 0'),
        'gamma < 0': (lambda o: s.ExponentialLR(o, -0.5), 'negative'),
    }


@pytest.mark.parametrize('case', list(refused()))
def test_refusals_by_name(case):
    from tonic_amd.torch import updaters
    factory, named = refused()[case]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(NotImplementedError) as error:
            updaters.lr_schedule_rule(factory, None, LR)
    assert named in str(error.value), str(error.value)


def test_updaters_refuse_at_construction_or_initialize():
    """Like the optimizer refusals: the entropy-coefficient tuner and MPO's duals at construction; a flat updater's
    `_setup` (its `initialize`) probes the same way."""
    from tonic_amd.torch import updaters
    bad = lambda o: torch.optim.lr_scheduler.MultiStepLR(o, [3])                # noqa: E731
    with pytest.raises(NotImplementedError, match='MultiStepLR'):
        updaters.EntropyCoeffTuning(lr_scheduler=bad)
    with pytest.raises(NotImplementedError, match='MultiStepLR'):
        updaters.MaximumAPosterioriPolicyOptimization(dual_lr_scheduler=bad)
    tuner = updaters.EntropyCoeffTuning(lr_scheduler=ref.factory('cosine'))
    assert tuner.lr_scheduler is not None and tuner.schedule is None            # (packed at `initialize`)


def test_schedule_check_rejects_what_the_header_says(lib):
    from tonic_amd import _lib

    def status(schedule, **fields):
        packed = ref.pack(schedule)
        for key, value in fields.items():
            holder, _, name = key.rpartition('__')
            setattr(packed.segment[int(holder[-1])] if holder else packed, name, value)
        return lib.tonic_lr_schedule_check(ctypes.byref(packed)), lib.tonic_last_error().decode()

    assert lib.tonic_lr_schedule_check(None) == 0
    cosine, warm = ref.SCHEDULES['cosine'][1], ref.SCHEDULES['warmup-cosine'][1]
    assert status(cosine)[0] == 0 and status(warm)[0] == 0
    for fields, named in ((dict(count=0), 'count'), (dict(count=3), 'count'), (dict(reserved=1), 'reserved'),
                          (dict(milestone=2), 'milestone'), (dict(segment1__period=3), 'segment[1]'),
                          (dict(segment0__kind=6), 'kind'), (dict(segment0__kind=-1), 'kind'),
                          (dict(segment0__reserved=1), 'reserved'), (dict(segment0__a=float('nan')), 'finite'),
                          (dict(segment0__a=float('inf')), 'finite'), (dict(segment0__b=0.5), 'not read'),
                          (dict(segment0__period=0), 'period'), (dict(segment0__a=-1e-9), 'negative')):
        code, message = status(cosine, **fields)
        assert code == -1 and named in message, (fields, code, message)
    for fields in (dict(milestone=0), dict(milestone=-1), dict(segment1__kind=9), dict(segment1__period=0),
                   dict(segment0__a=0.0), dict(segment0__a=1.5), dict(segment0__b=-0.1), dict(segment0__period=0)):
        assert status(warm, **fields)[0] == -1, fields
    for schedule in (([('constant', 5, 1.5, 0.0)], 0), ([('constant', -1, 0.5, 0.0)], 0),
                     ([('exponential', 3, 0.9, 0.0)], 0), ([('exponential', 0, -0.9, 0.0)], 0),
                     ([('step', 0, 0.5, 0.0)], 0), ([('polynomial', 5, -1.0, 0.0)], 0),
                     ([('polynomial', 0, 1.0, 0.0)], 0)):
        assert status(schedule)[0] == -1, schedule
    assert status(([('constant', 0, 1.0, 0.0)], 0))[0] == 0                     # ConstantLR(total_iters=0) is torch's
    bad = ref.pack(cosine)
    bad.count = 3
    assert math.isnan(lib.tonic_lr_schedule_value(ctypes.byref(bad), LR, 1))
    assert math.isnan(lib.tonic_lr_schedule_value(ctypes.byref(ref.pack(cosine)), LR, -1))
    # an invalid schedule is refused by the step entries before anything touches the device (no device here)
    rule = _lib.Optimizer(kind=2, lr=1e-3)
    assert lib.tonic_scheduled_optimizer_step(None, None, None, None, 4, 1.0, ctypes.byref(rule), 0, 0.0, 0.0, None,
                                              None, None, None, None, 0, 0, 0.0, ctypes.byref(bad), None) == -1
    assert 'count' in lib.tonic_last_error().decode()
    assert lib.tonic_scheduled_adam_step_pair(*([None] * 5), 4, 1e-3, 0, 0.0, 0.0, None, None, None, *([None] * 5), 4,
                                              1e-3, 0, None, 1.0, 0.9, 0.999, 1e-8, None, ctypes.byref(bad),
                                              None) == -1
    assert 'count' in lib.tonic_last_error().decode()


# ------------------------------------------------------------------------------------------------ signatures, routing

# (the reference's positional arguments, in order: tonic/torch/updaters/{actors,critics}.py)
POSITIONAL = {
    'ClippedRatio': ['optimizer', 'ratio_clip', 'kl_threshold', 'entropy_coeff', 'gradient_clip'],
    'StochasticPolicyGradient': ['optimizer', 'entropy_coeff', 'gradient_clip'],
    'VRegression': ['loss', 'optimizer', 'gradient_clip'],
    'DeterministicQLearning': ['loss', 'optimizer', 'gradient_clip'],
    'TwinCriticDeterministicQLearning': ['loss', 'optimizer', 'target_action_noise', 'gradient_clip'],
    'TwinCriticSoftQLearning': ['loss', 'optimizer', 'entropy_coeff', 'gradient_clip'],
    'DistributionalDeterministicQLearning': ['optimizer', 'gradient_clip'],
    'TwinCriticDistributionalDeterministicQLearning': ['optimizer', 'target_action_noise', 'gradient_clip'],
    'ExpectedSARSA': ['num_samples', 'loss', 'optimizer', 'gradient_clip'],
    'DeterministicPolicyGradient': ['optimizer', 'gradient_clip'],
    'DistributionalDeterministicPolicyGradient': ['optimizer', 'gradient_clip'],
    'TwinCriticSoftDeterministicPolicyGradient': ['optimizer', 'entropy_coeff', 'gradient_clip'],
    'EntropyCoeffTuning': ['target_entropy', 'initial_entropy_coeff', 'optimizer'],
}


@pytest.mark.parametrize('name', list(POSITIONAL))
def test_positional_signatures_are_unchanged_and_the_keyword_trails(name):
    from tonic_amd.torch import updaters
    parameters = inspect.signature(getattr(updaters, name).__init__).parameters
    assert list(parameters) == ['self'] + POSITIONAL[name] + ['lr_scheduler']
    assert parameters['lr_scheduler'].default is None
    updater = getattr(updaters, name)(lr_scheduler=ref.factory('linear'))
    assert updater.lr_scheduler is not None and updater.schedule is None


def test_mpo_and_trpo_and_q_regression_signatures():
    from tonic_amd.torch import updaters
    mpo = list(inspect.signature(updaters.MaximumAPosterioriPolicyOptimization.__init__).parameters)
    assert mpo[-5:] == ['actor_optimizer', 'dual_optimizer', 'gradient_clip', 'actor_lr_scheduler',
                        'dual_lr_scheduler']
    updater = updaters.MaximumAPosterioriPolicyOptimization(actor_lr_scheduler=ref.factory('linear'),
                                                            dual_lr_scheduler=ref.factory('cosine'))
    assert ref.unpack(updater.dual_schedule) == ref.SCHEDULES['cosine'][1] and updater.lr_scheduler is not None
    assert list(inspect.signature(updaters.TrustRegionPolicyGradient.__init__).parameters) == \
        ['self', 'optimizer', 'entropy_coeff']
    # QRegression keeps the reference's constructor argument for argument; its scheduler is an attribute
    assert list(inspect.signature(updaters.QRegression.__init__).parameters) == \
        ['self', 'loss', 'optimizer', 'gradient_clip']
    assert updaters.QRegression().lr_scheduler is None


def test_adam_table_with_schedules():
    """F32(lr_t / bias1) per row with lr_t at the steps TAKEN before the row's step; without schedules the old bits."""
    from tonic_amd.q_update import adam_table
    from tonic_amd.torch.updaters import adam_step_constants
    critic = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    actor = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-8)
    due = [False, True, False, True]
    warm, cosine = ref.SCHEDULES['warmup-cosine'][1], ref.SCHEDULES['cosine'][1]
    plain, _, _ = adam_table(4, due, critic, actor, 2, 3)
    same, _, _ = adam_table(4, due, critic, actor, 2, 3, schedules=(None, None))
    np.testing.assert_array_equal(plain, same)
    want = np.zeros((4, 2, 2), np.float32)
    for it in range(4):
        want[it, 0] = adam_step_constants(critic, 3 + it)
    want[1, 1], want[3, 1] = adam_step_constants(actor, 4), adam_step_constants(actor, 5)
    np.testing.assert_array_equal(plain, want)
    table, critic_steps, actor_steps = adam_table(4, due, critic, actor, 2, 3,
                                                  schedules=(ref.pack(warm), ref.pack(cosine)))
    assert (critic_steps, actor_steps) == (6, 5) and table.dtype == np.float32
    for it in range(4):
        step = 3 + it
        lr_t = ref.value(warm, critic['lr'], step - 1)
        assert table[it, 0, 0] == np.float32(lr_t / (1 - 0.9 ** step)) and table[it, 0, 1] == want[it, 0, 1]
    for it, step in ((1, 4), (3, 5)):
        lr_t = ref.value(cosine, actor['lr'], step - 1)
        assert table[it, 1, 0] == np.float32(lr_t / (1 - 0.8 ** step)) and table[it, 1, 1] == want[it, 1, 1]
    assert (table[0, 1] == 0).all() and (table[2, 1] == 0).all()
    # (the critic's third row is step 5, t = 4 = the milestone: the cosine segment starts at the base rate)
    assert (table[:, 0, 0] != plain[:, 0, 0]).tolist() == [True, True, False, True]
    only_actor, _, _ = adam_table(4, due, critic, actor, 2, 3, schedules=(None, ref.pack(cosine)))
    np.testing.assert_array_equal(only_actor[:, 0], plain[:, 0])
    np.testing.assert_array_equal(only_actor[:, 1], table[:, 1])


@pytest.mark.parametrize('kind, fused', [('ddpg', 2), ('td3', 0), ('sac', 1)])
def test_a_scheduled_plain_adam_agent_stays_on_the_fused_iteration(world, kind, fused):     # noqa: F811
    """`plain` is the rule, not the rate: with a schedule on both updaters the route is the fused kind, the table of
    the launches holds the scheduled step sizes, and the schedules are part of what the graph bakes in."""
    agent = world.make(kind)
    unscheduled = agent._graph_signature()
    warm, cosine = ref.SCHEDULES['warmup-cosine'][1], ref.SCHEDULES['cosine'][1]
    agent.critic_updater.schedule, agent.actor_updater.schedule = ref.pack(warm), ref.pack(cosine)
    assert agent._fused_kind() == fused and not agent._fused_in_phases()
    assert agent._graph_signature() != unscheduled
    world.take()
    agent.critic_updater.state.value, agent.actor_updater.state.value = 3, 1
    agent.enqueue_update(*streams(agent))
    rows = [e for e in world.take() if e[0] == 'q']
    assert len(rows) == 4
    actor_step = 1
    for it, row in enumerate(rows):
        hyper = dict(agent.critic_updater.hyper, lr=ref.value(warm, 1e-3, 3 + it))
        assert row[7] == constants(hyper, 4 + it)
        if row[4]:                                  # actor_due
            actor_step += 1
            hyper = dict(agent.actor_updater.hyper, lr=ref.value(cosine, 3e-4, actor_step - 1))
            assert row[8] == constants(hyper, actor_step)
    assert actor_step > 1
    again = agent._u.slot.graph
    agent.enqueue_update(*streams(agent))
    assert agent._u.slot.graph is again             # the second call replays the same graph
