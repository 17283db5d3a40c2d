"""The optimizer family on the host: the float32 statements of tests/optim_family_ref.py against the installed
torch.optim classes stepping float64 CPU tensors, and `updaters.optimizer_hyperparameters` in both directions."""
import numpy as np
import pytest

import numpy_port as port
import optim_family_ref as ref
from test_oracle_golden import ADAM_GRAD_SCALE as GRAD_SCALE
from test_oracle_golden import adam_case

torch = pytest.importorskip('torch')

N, STEPS = 1031, 7


def rule_of(name):
    from tonic_amd.torch import updaters
    return updaters.optimizer_hyperparameters(ref.factory(name), 1e-3)


@pytest.mark.parametrize('name', list(ref.CONFIGURATIONS))
def test_statement_against_torch_float64(name):
    """7 steps of 1031 elements from step 0 (zero state: SGD's first-step rule, amsgrad's maximum from nothing).  The
    reference is the installed torch.optim class itself on float64 tensors, fed float64(g_sum) * float64(F32(scale)):
    it holds the class's real hyper-parameters, so the statement's float32 constants count as error too.  The largest
    distance in `adam_f64_unit`s (one ulp of the parameter + lr * 2**-23) is MEASURED here; FAMILY_F64_UNITS is that
    measurement rounded up, not a bound chosen in advance: the test fails when the statement moves away from float64
    and when the recorded value is more than twice what is measured.  `family_f64` (the statement's own expressions
    in float64) is printed beside it: what is left there is the float32 rounding of the constants alone."""
    rule = rule_of(name)
    lr = rule['lr']
    p, _, _, sums = adam_case(N, STEPS, 21)
    slots = [np.zeros(N, np.float32) for _ in ref.slot_names(rule)]
    p64, slots64 = p, slots
    param = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    optimizer = ref.factory(name)([param])
    worst = worst_f64 = 0.0
    for k in range(STEPS):
        param.grad = torch.tensor(sums[k].astype(np.float64) * np.float64(np.float32(GRAD_SCALE)))
        optimizer.step()
        want = param.detach().numpy()
        p, slots = ref.family_statement(rule, p, sums[k], slots, k + 1, GRAD_SCALE)
        p64, slots64 = ref.family_f64(rule, p64, sums[k], slots64, k + 1, GRAD_SCALE)
        assert p.dtype == np.float32 and p64.dtype == np.float64 and np.isfinite(p).all()
        unit = port.adam_f64_unit(want, lr)
        units = float((np.abs(p - want) / unit).max())
        worst, worst_f64 = max(worst, units), max(worst_f64, float((np.abs(p64 - want) / unit).max()))
        print(f'{name} step {k + 1}: statement {units:.2f} units from torch float64, family_f64 '
              f'{float((np.abs(p64 - want) / unit).max()):.3f}')
    print(f'{name}: {worst:.2f} units over {STEPS} steps (recorded {ref.FAMILY_F64_UNITS[name]})')
    assert worst <= ref.FAMILY_F64_UNITS[name], worst
    assert worst >= 0.5 * ref.FAMILY_F64_UNITS[name], 'FAMILY_F64_UNITS is a measurement: bring it down to it'


def test_statement_slots_and_first_step():
    """What only shows at the edges: SGD's buffer IS the gradient after the first step and is damped afterwards;
    amsgrad's maximum never falls; maximize mirrors the step; an exactly zero gradient without decay moves nothing."""
    p, _, _, sums = adam_case(N, 3, 22)
    zero = slice(N // 2, N // 2 + N // 5)
    rule = rule_of('sgd-momentum')
    g = sums[0] * np.float32(GRAD_SCALE)
    p1, (buf,) = ref.family_statement(rule, p, sums[0], [np.full(N, 7.0, np.float32)], 1, GRAD_SCALE)
    assert np.array_equal(buf, g) and np.array_equal(p1, p - np.float32(rule['lr']) * g)
    _, (buf2,) = ref.family_statement(rule, p1, sums[1], [buf], 2, GRAD_SCALE)
    g2 = sums[1] * np.float32(GRAD_SCALE)
    assert np.array_equal(buf2, buf * np.float32(0.9) + np.float32(1.0 - 0.1) * g2)
    rule = rule_of('adam-amsgrad')
    slots = [np.zeros(N, np.float32)] * 3
    q = p
    for k, scale in enumerate((1.0, 1e-2, 1e-4)):             # shrinking gradients: v falls, the maximum stays
        before = slots[2]
        q, slots = ref.family_statement(rule, q, (sums[k] * np.float32(scale)), slots, k + 1, GRAD_SCALE)
        assert (slots[2] >= before).all() and (slots[2] >= slots[1]).all()
    assert (slots[2] > slots[1]).sum() > N // 2
    up, _ = ref.family_statement(rule_of('adam-maximize'), p, sums[0], [np.zeros(N, np.float32)] * 2, 1, GRAD_SCALE)
    plain = dict(rule_of('adam-maximize'), maximize=False)
    down, _ = ref.family_statement(plain, p, sums[0], [np.zeros(N, np.float32)] * 2, 1, GRAD_SCALE)
    opposite = np.sign(up - p) * np.sign(down - p)
    assert not (opposite > 0).any() and (opposite < 0).sum() > N // 2
    want_down = port.adam_statement(p, sums[0], np.zeros(N, np.float32), np.zeros(N, np.float32), 1, GRAD_SCALE, 3e-4)
    assert np.array_equal(down, want_down[0]), 'without its options the Adam rule is adam_statement'
    for name in ('adam-amsgrad', 'sgd', 'sgd-nesterov', 'rmsprop', 'rmsprop-centered-momentum'):
        rule = rule_of(name)
        moved, _ = ref.family_statement(rule, p, sums[0], [np.zeros(N, np.float32) for _ in ref.slot_names(rule)], 1,
                                        GRAD_SCALE)
        assert np.array_equal(moved[zero], p[zero]) and not np.array_equal(moved, p), name


SERVED = {
    'adam-wd': dict(kind='adam', lr=3e-4, weight_decay=1e-2, amsgrad=False, maximize=False, betas=(0.9, 0.999),
                    eps=1e-8),
    'adam-amsgrad': dict(kind='adam', lr=3e-4, weight_decay=0.0, amsgrad=True, maximize=False, betas=(0.9, 0.999),
                         eps=1e-8),
    'adam-maximize': dict(kind='adam', lr=3e-4, weight_decay=0.0, amsgrad=False, maximize=True, betas=(0.9, 0.999),
                          eps=1e-8),
    'adamw': dict(kind='adamw', lr=3e-4, weight_decay=1e-2, amsgrad=False, maximize=False, betas=(0.9, 0.999),
                  eps=1e-8),
    'sgd': dict(kind='sgd', lr=1e-3, weight_decay=0.0, maximize=False, momentum=0.0, dampening=0.0, nesterov=False),
    'sgd-momentum': dict(kind='sgd', lr=1e-3, weight_decay=0.0, maximize=False, momentum=0.9, dampening=0.1,
                         nesterov=False),
    'sgd-nesterov': dict(kind='sgd', lr=1e-3, weight_decay=0.0, maximize=False, momentum=0.9, dampening=0.0,
                         nesterov=True),
    'rmsprop': dict(kind='rmsprop', lr=1e-3, weight_decay=0.0, maximize=False, alpha=0.99, eps=1e-8, momentum=0.0,
                    centered=False),
    'rmsprop-centered-momentum': dict(kind='rmsprop', lr=1e-3, weight_decay=0.0, maximize=False, alpha=0.99, eps=1e-8,
                                      momentum=0.9, centered=True),
}


@pytest.mark.parametrize('name', list(ref.CONFIGURATIONS))
def test_parser_accepts_the_family(name):
    """Every served configuration comes out with the class's own values as Python floats (float64: 3e-4 is not
    F32(3e-4)), and only plain Adam counts as plain."""
    from tonic_amd.torch import updaters
    rule = rule_of(name)
    assert rule == SERVED[name], rule
    for key, value in rule.items():
        if key in ('kind', 'amsgrad', 'maximize', 'nesterov', 'centered'):
            assert type(value) is (str if key == 'kind' else bool), (key, value)
        else:
            assert all(type(v) is float for v in (value if key == 'betas' else (value,))), (key, value)
    assert rule['lr'] != float(np.float32(rule['lr']))
    assert not updaters.plain_adam(rule)
    packed = updaters.optimizer_rule(rule)
    assert packed.lr == rule['lr'] and packed.weight_decay == rule['weight_decay']


def test_parser_plain_adam_and_defaults():
    from tonic_amd.torch import updaters
    default = updaters.optimizer_hyperparameters(None, 3e-4)
    assert default == dict(kind='adam', lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                           maximize=False)
    given = updaters.optimizer_hyperparameters(lambda params: torch.optim.Adam(params, lr=1e-3, betas=(0.8, 0.99)),
                                               3e-4)
    assert given == dict(default, lr=1e-3, betas=(0.8, 0.99))
    assert updaters.plain_adam(default) and updaters.plain_adam(given)
    # what the Adam entries read from it is what adam_hyperparameters reads
    legacy = updaters.adam_hyperparameters(lambda params: torch.optim.Adam(params, lr=1e-3, betas=(0.8, 0.99)), 3e-4)
    assert {k: given[k] for k in legacy} == legacy
    assert updaters.optimizer_hyperparameters(lambda params: torch.optim.AdamW(params), 1.0)['weight_decay'] == 1e-2
    assert updaters.plain_adam(updaters.optimizer_hyperparameters(
        lambda params: torch.optim.AdamW(params, weight_decay=0.0), 1.0))


def test_parser_rejects_by_name():
    from tonic_amd.torch import updaters
    with pytest.raises(NotImplementedError, match='Adagrad'):
        updaters.optimizer_hyperparameters(lambda params: torch.optim.Adagrad(params), 1e-3)
    other = torch.nn.Parameter(torch.zeros(1))
    with pytest.raises(NotImplementedError, match='2 parameter groups'):
        updaters.optimizer_hyperparameters(
            lambda params: torch.optim.SGD([dict(params=params), dict(params=[other], lr=0.5)], lr=0.1), 1e-3)
    with pytest.raises(NotImplementedError, match='tensor lr'):
        updaters.optimizer_hyperparameters(lambda params: torch.optim.Adam(params, lr=torch.tensor(1e-3)), 1e-3)

    class Lion(torch.optim.SGD):
        pass
    with pytest.raises(NotImplementedError, match='Lion'):
        updaters.optimizer_hyperparameters(lambda params: Lion(params, lr=0.1), 1e-3)


def test_adam_hyperparameters_unchanged():
    """`adam_hyperparameters` raises exactly as before for everything but plain Adam."""
    from tonic_amd.torch import updaters
    assert updaters.adam_hyperparameters(None, 3e-4) == dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8)
    for name in ('adam-wd', 'adam-amsgrad', 'adam-maximize'):
        with pytest.raises(NotImplementedError, match='weight_decay / amsgrad / maximize is not fused'):
            updaters.adam_hyperparameters(ref.factory(name), 1e-3)
    for name in ('adamw', 'sgd', 'rmsprop'):
        with pytest.raises(NotImplementedError, match='only torch.optim.Adam is fused'):
            updaters.adam_hyperparameters(ref.factory(name), 1e-3)


def test_slot_query_matches_the_statements():
    """tonic_optimizer_state_slots (no GPU work) counts what `slot_names` lists, and refuses what is no rule."""
    import ctypes
    from tonic_amd import _lib
    from tonic_amd.torch import updaters
    lib = _lib.load()
    for name in ref.CONFIGURATIONS:
        rule = rule_of(name)
        packed = updaters.optimizer_rule(rule)
        assert lib.tonic_optimizer_state_slots(ctypes.byref(packed)) == len(ref.slot_names(rule)), name
    assert {len(ref.slot_names(rule_of(name))) for name in ref.CONFIGURATIONS} == {0, 1, 2, 3}
    assert lib.tonic_optimizer_state_slots(ctypes.byref(_lib.Optimizer(kind=7))) == -1
    assert lib.tonic_optimizer_state_slots(ctypes.byref(_lib.Optimizer(kind=2, flags=1))) == -1     # SGD + amsgrad
    assert lib.tonic_optimizer_state_slots(None) == -1
    status = lib.tonic_optimizer_step(None, None, None, None, 4, 1.0, ctypes.byref(_lib.Optimizer(kind=7)), 0, 0.0,
                                      0.0, None, None, None, None, None, 0, 0, 0.0, None)
    assert status == -1 and b'not a rule' in lib.tonic_last_error()
