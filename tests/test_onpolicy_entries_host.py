"""What the fifteen on-policy actor / critic entries (and the two torso size queries) answer BEFORE any HIP
call: the status of every invalid input, which check wins when two apply, and, through the workspace message, the
route a valid call would take.  One table; no GPU.

Every pointer is a fake non-NULL address that the host side never dereferences (the torso's `sizes` array, which
it does read, is real), every call is shaped to return before a launch: an invalid argument, `n == 0` on a
forward, or a 16-byte workspace where the route's first statement is its workspace check —
    "grad workspace too small"                                              the fused kernels
    "wide critic grad" / "wide actor grad" / "wide value forward" / "wide act"   layer by layer (csrc/mlpwide.hip)
"""
import ctypes

import pytest

FAKE = 0x1000                     # a device pointer nobody reads
OK, INVALID, SHAPE, WORKSPACE = 0, -1, -2, -4

# entry -> (operation, takes a torso, takes a workspace, takes a value range)
ENTRIES = {
    'tonic_value_forward': ('value_forward', False, False, False),
    'tonic_value_forward_wide': ('value_forward', False, True, False),
    'tonic_value_forward_torso': ('value_forward', True, True, False),
    'tonic_value_forward_ranged': ('value_forward', False, False, True),
    'tonic_value_forward_wide_ranged': ('value_forward', False, True, True),
    'tonic_value_forward_torso_ranged': ('value_forward', True, True, True),
    'tonic_value_regression_grad': ('value_grad', False, True, False),
    'tonic_value_regression_grad_torso': ('value_grad', True, True, False),
    'tonic_value_regression_grad_ranged': ('value_grad', False, True, True),
    'tonic_value_regression_grad_torso_ranged': ('value_grad', True, True, True),
    'tonic_ppo_act': ('act', False, False, False),
    'tonic_ppo_act_wide': ('act', False, True, False),
    'tonic_ppo_act_torso': ('act', True, True, False),
    'tonic_ppo_actor_grad': ('actor_grad', False, True, False),
    'tonic_ppo_actor_grad_torso': ('actor_grad', True, True, False),
}
FUSED = b'grad workspace too small'
LAYERED = {'value_forward': b'wide value forward', 'value_grad': b'wide critic grad', 'act': b'wide act',
           'actor_grad': b'wide actor grad'}

_arrays = []                      # the `sizes` arrays stay alive for the session


def _sizes(sizes):
    if sizes is None:
        return None
    array = (ctypes.c_int32 * len(sizes))(*sizes)
    _arrays.append(array)
    return ctypes.cast(array, ctypes.c_void_p)


def arguments(entry, params=FAKE, n=16, O=17, A=6, layers=2, sizes=(64, 64), activation=1, low=None, high=None,
              max_workgroups=0, workspace_bytes=16):
    """The argument list of `entry` in the order of include/tonic_hip.h."""
    operation, torso, workspace, ranged = ENTRIES[entry]
    args = [layers, _sizes(sizes), activation] if torso else []
    if operation == 'act':
        args += [params, FAKE, FAKE, FAKE, FAKE, n, O, A]
    elif operation == 'value_forward':
        args += [params, FAKE, FAKE, 0.0, FAKE, FAKE, n, O]
    elif operation == 'value_grad':
        args += [params, FAKE, FAKE, 0.0, FAKE, FAKE, FAKE, n, O]
    else:
        args += [params, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, n, O, A, 0.2, 0.0, None]
    if operation in ('value_grad', 'actor_grad') and not torso:
        args += [max_workgroups]
    if workspace:
        args += [FAKE, workspace_bytes]
    if ranged:
        args += [low, high]
    return args + [None]


def table():
    """(id, entry, its argument list, status — or '>0' for a size —, substring of tonic_last_error() or None)."""
    rows = []

    def row(label, entry, status, message=None, **kwargs):
        rows.append(pytest.param(entry, arguments(entry, **kwargs), status, message, id=f'{entry[6:]}-{label}'))

    def query(label, status, O=17, A=6, actor=1, layers=2, sizes=(64, 64), n=16):
        shape = [O, A, actor, layers, _sizes(sizes)]
        rows.append(pytest.param('tonic_ppo_torso_param_count', shape, status, None, id=f'torso_param_count-{label}'))
        rows.append(pytest.param('tonic_ppo_torso_workspace_bytes', [n] + shape, status, None,
                                 id=f'torso_workspace_bytes-{label}'))

    for entry, (operation, torso, workspace, ranged) in ENTRIES.items():
        forward = operation in ('value_forward', 'act')
        actor = operation in ('act', 'actor_grad')
        layered = LAYERED[operation]
        # what a valid call with a 16-byte workspace at n = 16 answers: its route's workspace message; a forward
        # on the fused route would launch, so those shapes are asked with n = 0 instead
        fused_answer = dict(status=OK, n=0) if forward else dict(status=WORKSPACE, message=FUSED)
        wide_answer = (dict(status=WORKSPACE, message=layered) if workspace else dict(status=SHAPE, n=0))
        narrow_answer = dict(status=WORKSPACE, message=layered) if torso else fused_answer

        # the pointer / row-count check
        row('null', entry, INVALID, b'null' if entry == 'tonic_ppo_act' else None, params=None)
        row('null-beats-shape', entry, INVALID, params=None, O=0)
        row('n<0', entry, INVALID, n=-1)
        row('n=0', entry, OK if forward else INVALID, n=0)

        # the value range: one pointer alone is refused before anything else
        if ranged:
            for label, pair in (('low-only', dict(low=FAKE)), ('high-only', dict(high=FAKE))):
                row(label, entry, INVALID, b'both', **pair)
                row(label + '-beats-shape', entry, INVALID, b'both', O=0, **pair)
                row(label + '-beats-null', entry, INVALID, b'both', params=None, **pair)
                if torso:
                    row(label + '-beats-torso', entry, INVALID, b'both', layers=0, **pair)
            row('range-n=0', entry, OK if forward else INVALID, n=0, low=FAKE, high=FAKE)
            row('range-narrow', entry, **narrow_answer, low=FAKE, high=FAKE)
            row('range-O=111', entry, **wide_answer, O=111, low=FAKE, high=FAKE)

        # observation sizes: 32 is the last fused one, 384 the last one served
        row('O=0', entry, SHAPE, O=0)
        row('O=32', entry, **narrow_answer, O=32)
        for O in (33, 111, 384):
            row(f'O={O}', entry, **wide_answer, O=O)
        row('O=385', entry, SHAPE, O=385)
        row('O=17', entry, **narrow_answer)

        # action sizes: 8 is the last fused one, 32 the last one served
        if actor:
            row('A=0', entry, SHAPE, A=0)
            row('A=8', entry, **narrow_answer, A=8)
            for A in (9, 32):
                row(f'A={A}', entry, **wide_answer, A=A)
            row('A=33', entry, SHAPE, A=33)

        # the torso's requirements come after the pointers and before the shape
        if torso:
            row('layers=0', entry, SHAPE, b'hidden layers', layers=0, sizes=())
            row('layers=5', entry, SHAPE, b'hidden layers', layers=5, sizes=(64,) * 5)
            row('sizes=NULL', entry, SHAPE, b'hidden layers', sizes=None)
            row('size=66', entry, SHAPE, b'multiples of 4', sizes=(64, 66))
            row('activation=3', entry, SHAPE, b'multiples of 4', activation=3)
            row('torso-beats-shape', entry, SHAPE, b'hidden layers', layers=0, sizes=(), O=385)
            row('null-beats-torso', entry, INVALID, params=None, layers=0, sizes=())
            row('one-layer', entry, WORKSPACE, layered, layers=1, sizes=(64,))
            row('relu-4x', entry, WORKSPACE, layered, layers=4, sizes=(4, 384, 8, 64), activation=2)

        # max_workgroups reaches the fused route only
        if not forward and not torso:
            row('max_workgroups=-1', entry, INVALID, b'max_workgroups', max_workgroups=-1)
            row('max_workgroups=-1-wide', entry, WORKSPACE, layered, max_workgroups=-1, O=111)
            row('max_workgroups=1', entry, WORKSPACE, FUSED, max_workgroups=1)

    # the two size queries: -1 for everything the entries refuse
    query('actor', '>0')
    query('critic', '>0', A=1, actor=0)
    query('critic-has-no-action-size', '>0', A=33, actor=0)
    query('largest', '>0', O=384, A=32, layers=4, sizes=(4, 384, 8, 64))
    query('layers=0', INVALID, layers=0, sizes=())
    query('layers=5', INVALID, layers=5, sizes=(64,) * 5)
    query('sizes=NULL', INVALID, sizes=None)
    query('size=66', INVALID, sizes=(64, 66))
    for O in (0, 385):
        query(f'O={O}', INVALID, O=O)
    for A in (0, 33):
        query(f'A={A}', INVALID, A=A)
    rows.append(pytest.param('tonic_ppo_torso_workspace_bytes', [0, 17, 6, 1, 2, _sizes((64, 64))], INVALID, None,
                             id='torso_workspace_bytes-n=0'))
    return rows


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('entry, args, status, message', table())
def test_entry_answers_before_any_launch(lib, entry, args, status, message):
    got = getattr(lib, entry)(*args)
    error = lib.tonic_last_error()
    assert got > 0 if status == '>0' else got == status, (got, error)
    if message is not None:
        assert message in error, error


def test_all_fifteen_entries_are_in_the_table():
    from tonic_amd import _lib
    families = ('tonic_value_forward', 'tonic_value_regression_grad', 'tonic_ppo_act', 'tonic_ppo_actor_grad')
    named = {name for name in _lib.SIGNATURES
             if name.startswith(families) and 'param_count' not in name}
    assert named == set(ENTRIES) and len(ENTRIES) == 15
    for entry in ENTRIES:
        assert len(arguments(entry)) == len(_lib.SIGNATURES[entry][1]), entry


def test_default_torso_counts_as_the_fixed_network(lib):
    sizes = _sizes((64, 64))
    assert lib.tonic_ppo_torso_param_count(17, 6, 1, 2, sizes) == lib.tonic_ppo_actor_param_count(17, 6) == 5708
    assert lib.tonic_ppo_torso_param_count(17, 1, 0, 2, sizes) == lib.tonic_v_critic_param_count(17) == 5377
