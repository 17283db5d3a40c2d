"""The float32 statements of the optimizer family (csrc/optim.hip: optimizer_kernel behind tonic_optimizer_step), operation
by operation, in the kernels' order — what `numpy_port.adam_statement` is for plain Adam.  (oracle/ is frozen: these live
with the tests.)

A rule is the dict `updaters.optimizer_hyperparameters` returns.  `family_statement` takes one step of it in float32,
every operation rounded once (no FMA: the library is built with -ffp-contract=off; divide and sqrt are correctly
rounded); `family_f64` evaluates the same expressions in float64 with the statement's float32 scalars, like
`numpy_port.adam_f64`.  Line numbers: the single-tensor CPU paths of the installed torch (2.10),
torch/optim/{adam,sgd,rmsprop}.py.

    every rule    g = g_sum * F32(grad_scale)
                  g = -g                                        maximize (adam.py:397, sgd.py:344, rmsprop.py:302)
                  g = g + F32(wd) * p                           wd != 0, not AdamW (adam.py:429, sgd.py:356,
                                                                rmsprop.py:308)
    Adam / AdamW  p = p * F32(1 - lr * wd)                      AdamW with wd != 0 (adam.py:419)
                  m = m + w1 * (g - m)                          w1 = F32(1 - beta1) (:457)
                  v = v * F32(beta2) + w2 * (g * g)             w2 = F32(1 - beta2) (:476)
                  vmax = max(vmax, v)                           amsgrad (:540); v below is then vmax
                  denom = sqrt(v) / bias2_sqrt + F32(eps)       (:543 / :545)
                  p = p - step_size * (m / denom)               step_size = F32(lr / (1 - beta1 ** step)) (:547)
    SGD           buf = g                                       momentum != 0, the first step taken (sgd.py:361-363)
                  buf = buf * F32(mu) + F32(1 - dampening) * g  momentum != 0, later steps (:365)
                  d = g + F32(mu) * buf | buf | g               nesterov | momentum | neither (:367-370)
                  p = p - F32(lr) * d                           (:380)
    RMSprop       sq = sq * F32(alpha) + wa * (g * g)           wa = F32(1 - alpha) (rmsprop.py:316)
                  ga = ga + wa * (g - ga)                       centered (:322)
                  avg = sqrt(sq - ga * ga) + F32(eps)           centered (:323, :330); else sqrt(sq) + F32(eps)
                  buf = buf * F32(mu) + g / avg                 momentum > 0 (:336)
                  p = p - F32(lr) * buf                         momentum > 0 (:337); else p - F32(lr) * (g / avg) (:339)

As with Adam these differ from torch's float32 CPU results in known places (addcmul_ forms (w * g) * g, lerp_ fuses
from the second step on, `add_(x, alpha=a)` fuses): tests/test_optim_family_host.py measures each statement against the
installed torch.optim class stepping float64 tensors.  State buffers are listed in tonic_optimizer_state_slots' order.
"""
import math

import numpy as np

F32 = np.float32

# One configuration per served code path, as the reference-style factory builds it -> (class name, keyword arguments).
CONFIGURATIONS = {
    'adam-wd': ('Adam', dict(lr=3e-4, weight_decay=1e-2)),
    'adam-amsgrad': ('Adam', dict(lr=3e-4, amsgrad=True)),
    'adam-maximize': ('Adam', dict(lr=3e-4, maximize=True)),
    'adamw': ('AdamW', dict(lr=3e-4)),                                    # (torch's default weight_decay: 1e-2)
    'sgd': ('SGD', dict(lr=1e-3)),
    'sgd-momentum': ('SGD', dict(lr=1e-3, momentum=0.9, dampening=0.1)),
    'sgd-nesterov': ('SGD', dict(lr=1e-3, momentum=0.9, nesterov=True)),
    'rmsprop': ('RMSprop', dict(lr=1e-3)),
    'rmsprop-centered-momentum': ('RMSprop', dict(lr=1e-3, centered=True, momentum=0.9)),
}

# The statements' own distance from the installed torch.optim class stepping FLOAT64 CPU tensors, in units of one
# float32 ulp of the parameter + lr * 2**-23 (numpy_port.adam_f64_unit), over 7 steps of 1031 elements from step 0:
# measured by tests/test_optim_family_host.py and rounded up (plain Adam: 8.0).  The unit is Adam's: steps of about lr.
# SGD steps by lr * |g| and a first RMSprop step by lr / sqrt(1 - alpha) = 10 lr, which momentum then piles up, with
# gradient means up to ~40 in these inputs: the float32 roundings of such steps are that many times the unit.
FAMILY_F64_UNITS = {
    'adam-wd': 3.0, 'adam-amsgrad': 3.0, 'adam-maximize': 2.5, 'adamw': 7.0, 'sgd': 2.5, 'sgd-momentum': 9.0,
    'sgd-nesterov': 21.0, 'rmsprop': 15.0, 'rmsprop-centered-momentum': 41.0,
}                   # measured: 2.76, 2.67, 2.37, 6.61, 2.12, 8.88, 20.92, 14.21, 40.53


def factory(name):
    """The `optimizer=` argument of an updater for CONFIGURATIONS[name]."""
    import torch
    cls, kwargs = CONFIGURATIONS[name]
    return lambda params: getattr(torch.optim, cls)(params, **kwargs)


def slot_names(rule):
    """The rule's state buffers in tonic_optimizer_state_slots' order."""
    if rule['kind'] in ('adam', 'adamw'):
        return ['exp_avg', 'exp_avg_sq'] + (['max_exp_avg_sq'] if rule['amsgrad'] else [])
    if rule['kind'] == 'sgd':
        return ['momentum_buffer'] if rule['momentum'] != 0 else []
    return ['square_avg'] + (['grad_avg'] if rule['centered'] else []) + \
        (['momentum_buffer'] if rule['momentum'] > 0 else [])


def _step(rule, p, g_sum, slots, step, grad_scale, T):
    """One step in the arithmetic of dtype `T`; every scalar is the kernel's float32 constant."""
    c = lambda x: T(F32(x))                                   # formed in float64, rounded to float32 ONCE
    kind, lr, wd = rule['kind'], rule['lr'], rule['weight_decay']
    p = np.asarray(p, T)
    state = dict(zip(slot_names(rule), (np.asarray(s, T) for s in slots)))
    assert len(state) == len(slots)
    g = np.asarray(g_sum, F32).astype(T) * c(grad_scale)
    if rule['maximize']:
        g = -g
    if wd != 0 and kind != 'adamw':
        g = g + c(wd) * p
    if kind in ('adam', 'adamw'):
        beta1, beta2 = rule['betas']
        step_size = c(lr / (1.0 - beta1 ** step))
        bias2_sqrt = c(math.sqrt(1.0 - beta2 ** step))
        if kind == 'adamw' and wd != 0:
            p = p * c(1.0 - lr * wd)
        m, v = state['exp_avg'], state['exp_avg_sq']
        m = m + c(1.0 - beta1) * (g - m)
        v = v * c(beta2) + c(1.0 - beta2) * (g * g)
        state['exp_avg'], state['exp_avg_sq'] = m, v
        if rule['amsgrad']:
            v = state['max_exp_avg_sq'] = np.maximum(state['max_exp_avg_sq'], v)
        denom = np.sqrt(v) / bias2_sqrt + c(rule['eps'])
        p = p - step_size * (m / denom)
    elif kind == 'sgd':
        d = g
        if rule['momentum'] != 0:
            mu = c(rule['momentum'])
            buf = g if step == 1 else state['momentum_buffer'] * mu + c(1.0 - rule['dampening']) * g
            state['momentum_buffer'] = buf
            d = g + mu * buf if rule['nesterov'] else buf
        p = p - c(lr) * d
    else:
        alpha = rule['alpha']
        sq = state['square_avg'] * c(alpha) + c(1.0 - alpha) * (g * g)
        state['square_avg'] = sq
        if rule['centered']:
            ga = state['grad_avg']
            ga = state['grad_avg'] = ga + c(1.0 - alpha) * (g - ga)
            avg = np.sqrt(sq - ga * ga) + c(rule['eps'])
        else:
            avg = np.sqrt(sq) + c(rule['eps'])
        if rule['momentum'] > 0:
            buf = state['momentum_buffer'] = state['momentum_buffer'] * c(rule['momentum']) + g / avg
            p = p - c(lr) * buf
        else:
            p = p - c(lr) * (g / avg)
    out = [state[name] for name in slot_names(rule)]
    assert p.dtype == T and all(s.dtype == T for s in out)
    return p, out


def family_statement(rule, p, g_sum, slots, step, grad_scale):
    """THE float32 expression optimizer_kernel is for `rule` (module docstring).  `g_sum` holds gradient SUMS, `step` is the
    1-based step being taken (state[0] + 1; SGD's momentum buffer starts at step 1).  -> new p, [new state buffers]."""
    return _step(rule, p, g_sum, slots, step, grad_scale, F32)


def family_f64(rule, p, g_sum, slots, step, grad_scale):
    """The same update in float64 from the same inputs, with the statement's float32 scalars: the difference between
    the two is the rounding of the element-wise operations alone.  `p`, `slots`: float32 or an earlier call's float64."""
    return _step(rule, p, g_sum, slots, step, grad_scale, np.float64)


def warm_slots(rule, n, seed):
    """State buffers as a long run leaves them (the scales of test_oracle_golden.adam_case's warm moments): second
    moments (s U(0.5, 1.5)) ** 2 with s = 10 ** U(-6, 1) per element, first moments within them (a centered RMSprop
    takes the root of square_avg - grad_avg ** 2), amsgrad's maximum up to twice the second moment."""
    rng = np.random.RandomState([n % 65521, seed, 77])
    s = 10 ** rng.uniform(-6, 1, size=n)
    second = np.square(s * rng.uniform(0.5, 1.5, size=n)).astype(F32)
    made = {'exp_avg': (rng.normal(size=n) * 0.3 * s).astype(F32), 'exp_avg_sq': second, 'square_avg': second,
            'max_exp_avg_sq': (second * rng.uniform(1.0, 2.0, size=n)).astype(F32),
            'grad_avg': (np.sqrt(second) * rng.uniform(-0.5, 0.5, size=n)).astype(F32),
            'momentum_buffer': (rng.normal(size=n) * s).astype(F32)}
    return [made[name] for name in slot_names(rule)]
