"""CPU tests of the critic-loss rule (`loss=` of the off-policy critic updaters): the mapping of torch loss objects to
tonic_critic_loss_t, what is refused and how, the host-only validation of the C ABI, and the float32 restatement of
the rules (tests/critic_loss_ref.py) against torch.nn.functional bit for bit, kinks, infinities and NaN included."""
import ctypes

import numpy as np
import pytest

import critic_loss_ref as ref

torch = pytest.importorskip('torch')
nn = torch.nn


def _updaters():
    import tonic_amd.torch as tt
    return tt.updaters


CRITIC_UPDATERS = ('DeterministicQLearning', 'TwinCriticDeterministicQLearning', 'TwinCriticSoftQLearning',
                   'ExpectedSARSA')


@pytest.mark.parametrize('loss,kind,param', [
    (None, ref.MSE, 0.0), (nn.MSELoss(), ref.MSE, 0.0), (nn.L1Loss(), ref.L1, 0.0),
    (nn.SmoothL1Loss(), ref.SMOOTH_L1, 1.0), (nn.SmoothL1Loss(beta=0.3), ref.SMOOTH_L1, float(np.float32(0.3))),
    (nn.SmoothL1Loss(beta=0.0), ref.SMOOTH_L1, 0.0),
    (nn.HuberLoss(), ref.HUBER, 1.0), (nn.HuberLoss(delta=2.7), ref.HUBER, float(np.float32(2.7)))])
def test_loss_objects_map_to_the_rule(loss, kind, param):
    updaters = _updaters()
    rule = updaters.critic_loss_rule(loss)
    assert (rule.kind, rule.reserved, rule.param) == (kind, 0, param)
    assert ref.rule_of(loss) == (kind, param)
    for name in CRITIC_UPDATERS:                    # every updater keeps the object and carries the rule
        updater = getattr(updaters, name)(loss=loss)
        assert updater.loss is loss
        assert (updater.loss_rule.kind, updater.loss_rule.param) == (kind, param), name


class _MyHuber(nn.HuberLoss):
    pass


@pytest.mark.parametrize('loss,names', [
    (nn.MSELoss(reduction='sum'), "MSELoss(reduction='sum')"), (nn.HuberLoss(reduction='none'), "reduction='none'"),
    (nn.SmoothL1Loss(reduction='sum'), "SmoothL1Loss(reduction='sum')"), (_MyHuber(), '_MyHuber'),
    (nn.BCELoss(), 'BCELoss'), (lambda values, returns: ((values - returns) ** 2).mean(), '<lambda>')])
def test_other_losses_are_refused_by_name(loss, names):
    updaters = _updaters()
    for name in CRITIC_UPDATERS:
        with pytest.raises(NotImplementedError) as error:
            getattr(updaters, name)(loss=loss)
        text = str(error.value)
        assert names in text, text
        for served in ('MSELoss', 'L1Loss', 'SmoothL1Loss', 'HuberLoss', "reduction='mean'"):
            assert served in text, text
    # assigning later goes through the same check and leaves the updater as it was
    updater = updaters.TwinCriticSoftQLearning(loss=nn.L1Loss())
    with pytest.raises(NotImplementedError):
        updater.loss = loss
    assert type(updater.loss) is nn.L1Loss and updater.loss_rule.kind == ref.L1


def test_invalid_parameters_are_refused_at_construction():
    updaters = _updaters()
    loss = nn.HuberLoss()
    loss.delta = 0.0                                # (torch does not check)
    with pytest.raises(NotImplementedError, match='delta'):
        updaters.DeterministicQLearning(loss=loss)
    loss = nn.SmoothL1Loss()
    loss.beta = -1.0
    with pytest.raises(NotImplementedError, match='beta'):
        updaters.ExpectedSARSA(loss=loss)


def test_v_regression_keeps_refusing_another_loss():
    updaters = _updaters()
    with pytest.raises(NotImplementedError):
        updaters.VRegression(loss=nn.HuberLoss())
    updaters.VRegression(loss=nn.MSELoss())


def test_critic_loss_check_of_the_c_abi():
    from tonic_amd import _lib
    lib = _lib.load()
    check = lambda **fields: lib.tonic_critic_loss_check(ctypes.byref(_lib.CriticLoss(**fields)))   # noqa: E731
    message = lambda: lib.tonic_last_error().decode()                                                # noqa: E731
    invalid = -1                                    # TONIC_ERR_INVALID_ARGUMENT
    assert lib.tonic_critic_loss_check(None) == 0
    assert check() == 0 and check(kind=ref.L1, param=float('nan')) == 0        # (param ignored for MSE and L1)
    assert check(kind=ref.SMOOTH_L1, param=0.0) == 0 and check(kind=ref.SMOOTH_L1, param=0.5) == 0
    assert check(kind=ref.HUBER, param=1.0) == 0
    assert check(kind=7) == invalid and 'kind 7' in message()
    assert check(kind=-1) == invalid and 'kind -1' in message()
    assert check(kind=ref.SMOOTH_L1, param=-1.0) == invalid and 'beta' in message() and '-1' in message()
    assert check(kind=ref.HUBER, param=0.0) == invalid and 'delta' in message()
    assert check(kind=ref.HUBER, param=-2.0) == invalid and 'delta' in message()
    assert check(kind=ref.HUBER, param=float('nan')) == invalid and 'finite' in message()
    assert check(kind=ref.SMOOTH_L1, param=float('inf')) == invalid and 'finite' in message()
    assert check(kind=ref.HUBER, param=1e-60) == invalid       # 0 in the float32 the kernels compare with
    # the entries validate before anything else: a bad rule never reaches a launch
    bad = _lib.QIteration(kind=0, actor_due=0, B=100, O=67, H=256, A=21,
                          critic_loss=_lib.CriticLoss(kind=ref.HUBER, param=0.0))
    assert lib.tonic_q_iteration(ctypes.byref(bad), None) == invalid and 'delta' in message()
    assert ctypes.sizeof(_lib.CriticLoss) == 16


def _vector(param):
    p = np.float32(param)
    up, down = np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(0))
    values = [p, -p, up, -up, down, -down, 0.0, -0.0, 1e-30, -1e-30, 1e4, -1e4, np.inf, -np.inf, np.nan,
              0.25 * p, -0.75 * p, 3.0 * p, -1.5 * p, 0.1, -0.7, 1.0, -1.0]
    return np.asarray(values, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('loss', [nn.MSELoss(), nn.L1Loss(), nn.SmoothL1Loss(), nn.SmoothL1Loss(beta=0.5),
                                  nn.SmoothL1Loss(beta=0.3), nn.SmoothL1Loss(beta=0.0), nn.HuberLoss(),
                                  nn.HuberLoss(delta=0.5), nn.HuberLoss(delta=2.75), nn.HuberLoss(delta=2.7)],
                         ids=lambda loss: f'{type(loss).__name__}-{getattr(loss, "beta", getattr(loss, "delta", ""))}')
def test_float32_restatement_equals_torch_bit_for_bit(loss):
    """Loss terms and gradients of the restatement on e = q - y against torch.nn.functional in float32 (reduction
    'none' for the terms, 'sum' for the gradient, i.e. unscaled by 1 / B): equal bit for bit, NaN for NaN.
    torch keeps beta / delta as a Python float and its CPU kernels divide and multiply by that float64; the rule
    rounds `param` to float32 ONCE (include/tonic_hip.h).  For a parameter float32 holds exactly (0.5, 1, 2.75) the two
    are the same arithmetic and every bit must agree; for one it does not hold (0.3, 2.7) the parameter itself is
    2^-25 relative away, and with the one rounding of the result that is at most 2 units in the last place, in the
    kernel's branch choice at the kink at most the neighbouring float: held to 2 ulp there."""
    kind, param = ref.rule_of(loss)
    e = _vector(param if param > 0 else 1.0)
    targets = np.asarray([0.0, 0.5, -3.0], np.float32)
    for y in targets:
        # q = e + y exactly representable errors are only guaranteed for y = 0; the others exercise q - y as formed
        q = torch.tensor(e + y, requires_grad=True)
        returns = torch.tensor(np.full_like(e, y))
        errors = (q.detach() - returns).numpy()
        name = {ref.MSE: 'mse_loss', ref.L1: 'l1_loss', ref.SMOOTH_L1: 'smooth_l1_loss', ref.HUBER: 'huber_loss'}[kind]
        extra = {key: getattr(loss, key) for key in ('beta', 'delta') if hasattr(loss, key)}
        functional = getattr(torch.nn.functional, name)
        terms = functional(q, returns, reduction='none', **extra)
        functional(q, returns, reduction='sum', **extra).backward()
        got_terms, got_dq = ref.loss_term(errors, kind, param), ref.loss_dq(errors, kind, param)
        want_terms, want_dq = terms.detach().numpy(), q.grad.numpy()
        for what, got, want in (('term', got_terms, want_terms), ('dq', got_dq, want_dq)):
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (what, y, errors[np.isnan(got) != nan])
            same = _bits(got)[~nan] == _bits(want)[~nan]
            if float(np.float32(param)) != float(getattr(loss, 'beta', getattr(loss, 'delta', 0.0))):
                finite = np.isfinite(want[~nan])
                with np.errstate(invalid='ignore'):
                    same |= finite & (np.abs(got[~nan] - want[~nan]) <= 2 * np.spacing(np.abs(want[~nan])))
            assert same.all(), (what, y, errors[~nan][~same], got[~nan][~same], want[~nan][~same])
        # the NaN rows of the rule
        nan_rows = np.isnan(errors)
        assert nan_rows.any() and np.isnan(got_terms[nan_rows]).all()
        sign_only = kind == ref.L1 or (kind == ref.SMOOTH_L1 and param == 0)
        assert (got_dq[nan_rows] == 0).all() if sign_only else np.isnan(got_dq[nan_rows]).all()


def test_restatement_is_symmetric_in_the_error():
    """ExpectedSARSA calls self.loss(returns, values) (critics.py:243): every rule gives the same term for -e and the
    gradient with respect to the SECOND argument of loss(returns, values) is the rule's gradient on e = q - y."""
    e = _vector(0.5)
    e = e[~np.isnan(e)]
    for kind, param in ((ref.MSE, 0), (ref.L1, 0), (ref.SMOOTH_L1, 0.5), (ref.SMOOTH_L1, 0), (ref.HUBER, 0.5)):
        assert np.array_equal(_bits(ref.loss_term(e, kind, param)), _bits(ref.loss_term(-e, kind, param)))
        assert np.array_equal(ref.loss_dq(e, kind, param), -ref.loss_dq(-e, kind, param))
    values = torch.tensor(e, requires_grad=True)
    torch.nn.functional.huber_loss(torch.zeros_like(values), values, reduction='sum', delta=0.5).backward()
    assert np.array_equal(values.grad.numpy(), ref.loss_dq(e, ref.HUBER, 0.5))
