"""The learning-rate schedules of the HIP optimizer steps, restated with `math` (csrc/lr_schedule.h: lr_schedule_value
behind tonic_lr_schedule_value and the scheduled instantiations of optimizer_kernel): torch's `_get_closed_form_lr`
of the six served classes, operation by operation on Python floats (float64), at t = the number of optimizer steps
taken so far.

A segment is (kind, period, a, b) as tonic_lr_segment_t holds it; a schedule is ([segments], milestone):

    constant      a = factor, period = total_iters              lr * (a + (t >= period) * (1 - a))
    linear        a = start_factor, b = end_factor,             lr * (a + (b - a) * min(period, t) / period)
                  period = total_iters
    exponential   a = gamma                                     lr * a ** t
    step          a = gamma, period = step_size                 lr * a ** (t // period)
    polynomial    a = power, period = total_iters               lr * (1.0 - min(period, t) / period) ** a
    cosine        a = eta_min, period = T_max                   a + (lr - a) * (1 + cos(pi * t / period)) / 2
    two segments, milestone m                                   t < m: the first at t; else the second at t - m

The safe-step rule of the bit comparisons with the DEVICE: its pow / cos may differ from the host's by a few float64
ulps (OpenCL's bound for double pow: 16 ulp = 2^-48 relative), so a case (schedule, base rate, step) is compared bit
for bit only where this reference alone shows that the float32 constant derived from lr_t is the same at
lr_t * (1 +- 2^-44) — `safe`.  `safe_rate` picks, from a fixed list and by the reference alone, a base rate at which
every step of a case is safe (a step is never dropped)."""
import math

KINDS = ('constant', 'linear', 'exponential', 'step', 'polynomial', 'cosine')

# name -> (torch.optim.lr_scheduler factory given the optimizer, ([segments], milestone), the period its edge steps
# are taken around).  The exponential schedule has no period of its own: its steps are those of a period of 10.
SCHEDULES = {
    'constant': (lambda s, o: s.ConstantLR(o, factor=0.25, total_iters=7), ([('constant', 7, 0.25, 0.0)], 0), 7),
    'linear': (lambda s, o: s.LinearLR(o, start_factor=0.1, end_factor=0.9, total_iters=12),
               ([('linear', 12, 0.1, 0.9)], 0), 12),
    'exponential': (lambda s, o: s.ExponentialLR(o, gamma=0.97), ([('exponential', 0, 0.97, 0.0)], 0), 10),
    'step': (lambda s, o: s.StepLR(o, step_size=5, gamma=0.5), ([('step', 5, 0.5, 0.0)], 0), 5),
    'polynomial': (lambda s, o: s.PolynomialLR(o, total_iters=11, power=1.5), ([('polynomial', 11, 1.5, 0.0)], 0), 11),
    'cosine': (lambda s, o: s.CosineAnnealingLR(o, T_max=12, eta_min=1e-5), ([('cosine', 12, 1e-5, 0.0)], 0), 12),
    'warmup-cosine': (lambda s, o: s.SequentialLR(o, [s.LinearLR(o, start_factor=0.1, end_factor=1.0, total_iters=4),
                                                      s.CosineAnnealingLR(o, T_max=9, eta_min=1e-5)], milestones=[4]),
                      ([('linear', 4, 0.1, 1.0), ('cosine', 9, 1e-5, 0.0)], 4), 9),
}

BASE_RATES = (1e-3, 3e-4, 7e-4, 2.5e-3, 1.1e-3)


def factory(name):
    """The `lr_scheduler=` argument of an updater for SCHEDULES[name]."""
    import torch
    return lambda optimizer: SCHEDULES[name][0](torch.optim.lr_scheduler, optimizer)


def edge_steps(name):
    """0, 1, period - 1, period, period + 1, 2 period + 3, m - 1, m, m + 1 (two segments) and 10^6."""
    _, (_, milestone), period = SCHEDULES[name]
    steps = [0, 1, period - 1, period, period + 1, 2 * period + 3]
    if milestone:
        steps += [milestone - 1, milestone, milestone + 1]
    return sorted(set(steps)) + [10 ** 6]


def segment_value(segment, lr, t):
    kind, period, a, b = segment
    if kind == 'constant':
        return lr * (a + (t >= period) * (1 - a))
    if kind == 'linear':
        return lr * (a + (b - a) * min(period, t) / period)
    if kind == 'exponential':
        return lr * a ** t
    if kind == 'step':
        return lr * a ** (t // period)
    if kind == 'polynomial':
        return lr * (1.0 - min(period, t) / period) ** a
    assert kind == 'cosine', kind
    return a + (lr - a) * (1 + math.cos(math.pi * t / period)) / 2


def value(schedule, lr, t):
    """THE statement: the rate of the step taken after t steps from the base rate `lr` (None: lr itself)."""
    if schedule is None:
        return lr
    segments, milestone = schedule
    if len(segments) == 2 and t >= milestone:
        return segment_value(segments[1], lr, t - milestone)
    return segment_value(segments[0], lr, t)


def pack(schedule):
    """([segments], milestone) as the tonic_lr_schedule_t of the C ABI (None -> None)."""
    from tonic_amd import _lib
    if schedule is None:
        return None
    segments, milestone = schedule
    packed = _lib.LrSchedule(count=len(segments), milestone=milestone)
    for k, (kind, period, a, b) in enumerate(segments):
        packed.segment[k] = _lib.LrSegment(kind=KINDS.index(kind), period=period, a=a, b=b)
    return packed


def unpack(packed):
    """A tonic_lr_schedule_t as ([segments], milestone)."""
    return ([(KINDS[s.kind], s.period, s.a, s.b) for s in packed.segment[:packed.count]], packed.milestone)


def safe(derive, lr_t):
    """The float32 constant(s) `derive(lr_t)` forms do not depend on the last bits of lr_t: the same at lr_t (1 +- 2^-44)."""
    import numpy as np
    around = [derive(lr_t * (1.0 + sign * 2.0 ** -44)) for sign in (-1.0, 0.0, 1.0)]
    return all(np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(around[1], np.float32).view(np.int32))
               for a in around)


def safe_rate(schedule, steps, derive, rates=BASE_RATES):
    """The first base rate of `rates` at which every step of `steps` is safe — `derive(lr_t, t)` -> the float32
    constant(s) the rule rounds from lr_t at step count t.  By the reference alone; no step is dropped."""
    for lr in rates:
        if all(safe(lambda x, t=t: derive(x, t), value(schedule, lr, t)) for t in steps):
            return lr
    raise AssertionError(f'no base rate of {rates} keeps every step of {steps} away from a float32 rounding boundary')
