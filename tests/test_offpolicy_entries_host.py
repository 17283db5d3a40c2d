"""What the off-policy entries of csrc/offpolicy.hip (and their four size queries) answer BEFORE any HIP call: the
status and message of every invalid input, which check wins when two apply, and the workspace check at exactly one
byte below the query.  One table; no GPU.

Every pointer is a fake non-NULL address that the host side never dereferences (the `sizes` arrays and the
tonic_critic_loss_t / tonic_q_iteration_t structures, which it does read, are real), and every call is shaped to
return before a launch: an invalid argument, or a workspace one byte short.  The method of
tests/test_onpolicy_entries_host.py.
"""
import ctypes
import itertools
import math

import pytest

FAKE = 0x1000                     # a device pointer nobody reads
OK, INVALID, SHAPE, WORKSPACE = 0, -1, -2, -4

# entry -> its arguments in the order of include/tonic_hip.h: `d_*` a pointer, `loss` a tonic_critic_loss_t*,
# anything else a number taken from DEFAULTS
_TWIN = ('kind d_policy_params d_target_critics d_critics d_norm_mean d_norm_std norm_clip d_observations d_actions '
         'd_next_observations d_rewards d_discounts d_eps d_grad_sums B O H A entropy_coeff noise_scale noise_clip')
_ACTOR = 'kind d_actor_params d_critics d_norm_mean d_norm_std norm_clip d_observations d_eps d_grad_sums B O H A entropy_coeff'
_SARSA = ('d_target_actor d_target_critic d_critic d_norm_mean d_norm_std norm_clip d_observations d_actions '
          'd_next_observations d_rewards d_discounts d_eps d_grad_sums B O H A S')
_MPO = ('d_actor_params d_target_actor d_target_critic d_duals min_log_dual d_norm_mean d_norm_std norm_clip '
        'd_observations d_eps d_grad_sums')
_MPO_FULL = _MPO + ' d_dual_grads d_stats B O H A S epsilon epsilon_penalty epsilon_mean epsilon_std action_penalization'
_MPO_SHARD = _MPO + ' d_column_sums B O H A S action_penalization'
_DUAL = ('d_column_sums d_duals min_log_dual d_dual_grads d_stats d_actor_stats B B_global A S epsilon '
         'epsilon_penalty epsilon_mean epsilon_std action_penalization')
_WS = ' d_workspace workspace_bytes stream'
ENTRIES = {
    'tonic_policy_forward': 'd_actor_params d_observations d_eps d_actions kind B O H A' + _WS,
    'tonic_twin_q_grad': _TWIN + _WS,
    'tonic_twin_q_grad_loss': _TWIN + ' loss' + _WS,
    'tonic_twin_q_grad_ranged': _TWIN + ' loss d_value_low d_value_high' + _WS,
    'tonic_actor_q_grad': _ACTOR + _WS,
    'tonic_actor_q_grad_ranged': _ACTOR + ' d_value_low d_value_high' + _WS,
    'tonic_expected_sarsa_grad': _SARSA + _WS,
    'tonic_expected_sarsa_grad_loss': _SARSA + ' loss' + _WS,
    'tonic_mpo_actor_grad': _MPO_FULL + _WS,
    'tonic_mpo_actor_grad_joint': _MPO_FULL + ' joint_kl' + _WS,
    'tonic_mpo_actor_grad_shard': _MPO_SHARD + _WS,
    'tonic_mpo_actor_grad_shard_joint': _MPO_SHARD + ' joint_kl' + _WS,
    'tonic_mpo_dual_step': _DUAL + ' stream',
    'tonic_mpo_dual_step_joint': _DUAL + ' joint_kl stream',
    'tonic_distributional_q_grad': ('d_target_actor d_target_critic d_critic d_norm_mean d_norm_std norm_clip '
                                    'd_observations d_actions d_next_observations d_rewards d_discounts d_values '
                                    'd_grad_sums B O H A NA' + _WS),
    'tonic_distributional_actor_grad': ('d_actor_params d_critic d_norm_mean d_norm_std norm_clip d_observations '
                                        'd_values d_grad_sums B O H A NA' + _WS),
}
ENTRIES = {name: spec.split() for name, spec in ENTRIES.items()}
DEFAULTS = dict(kind=1, B=17, O=17, H=64, A=6, S=20, NA=51, B_global=34, norm_clip=5.0, entropy_coeff=0.2,
                noise_scale=0.2, noise_clip=0.5, min_log_dual=-18.0, epsilon=0.1, epsilon_penalty=1e-3,
                epsilon_mean=1e-3, epsilon_std=1e-6, action_penalization=1, joint_kl=0, stream=None, loss=None,
                d_value_low=None, d_value_high=None, workspace_bytes=None)

# the name each family's messages print (the _ranged entries: the unsuffixed name but for the low / high pair)
FAMILY = {name: ('tonic_twin_q_grad' if name.startswith('tonic_twin_q_grad') else
                 'tonic_actor_q_grad' if name.startswith('tonic_actor_q_grad') else
                 'tonic_expected_sarsa_grad' if name.startswith('tonic_expected_sarsa') else
                 'tonic_mpo_actor_grad' if name.startswith('tonic_mpo_actor_grad') else
                 'tonic_mpo_dual_step' if name.startswith('tonic_mpo_dual_step') else name) for name in ENTRIES}

_alive = []                       # what ctypes must keep alive for the session


def _keep(thing):
    _alive.append(thing)
    return thing


def loss_rule(kind, param=0.0):
    from tonic_amd._lib import CriticLoss
    return ctypes.cast(ctypes.pointer(_keep(CriticLoss(kind, 0, param))), ctypes.c_void_p)


BAD_LOSSES = {'kind=4': ((4, 1.0), b'unknown kind 4'), 'nan': ((3, math.nan), b'is not finite'),
              'inf': ((2, math.inf), b'is not finite'), 'beta<0': ((2, -1.0), b'beta >= 0'),
              'delta=0': ((3, 0.0), b'delta > 0'), 'delta<0': ((3, -2.0), b'delta > 0')}

TORSOS = {'plain64': ((64, 64), 1), 'plain256': ((256, 256), 1), 'tanh40x24': ((40, 24), 2),
          'relu32x3': ((32, 32, 32), 1), 'one256': ((256,), 1)}
UNKNOWN_H = (0, -5, (1 << 30) | (1 << 29) | 255)      # the last: a descriptor nobody registered


def torso_code(lib, name):
    sizes, activation = TORSOS[name]
    array = _keep((ctypes.c_int32 * len(sizes))(*sizes))
    code = lib.tonic_mlp_torso(len(sizes), ctypes.cast(array, ctypes.c_void_p), activation)
    assert code > 0
    return code


def query(lib, entry, v):
    """The size query an entry checks its workspace against, at the values `v` of its arguments."""
    if entry.startswith('tonic_distributional'):
        return lib.tonic_distributional_workspace_bytes(v['B'], v['O'], v['A'], v['H'], v['NA'])
    if entry.startswith(('tonic_expected_sarsa', 'tonic_mpo_actor')):
        return lib.tonic_mpo_workspace_bytes(v['B'], v['O'], v['A'], v['H'], v['S'])
    return lib.tonic_offpolicy_workspace_bytes(v['B'], v['O'], v['A'], v['H'])


def call(lib, entry, **changes):
    """Calls `entry` with valid arguments but for `changes` (workspace_bytes: the query's answer unless given);
    returns (status, tonic_last_error())."""
    values = dict(DEFAULTS, **changes)
    if values['workspace_bytes'] is None and 'workspace_bytes' in ENTRIES[entry]:
        values['workspace_bytes'] = query(lib, entry, values)
    args = [values.get(name, FAKE) if name.startswith('d_') else values[name] for name in ENTRIES[entry]]
    status = getattr(lib, entry)(*args)
    return status, lib.tonic_last_error()


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


def pointers(entry):
    return [name for name in ENTRIES[entry] if name.startswith('d_') and name not in ('d_value_low', 'd_value_high')]


def expect(result, status, message=None):
    got, error = result
    assert got == status, (got, error)
    if message is not None:
        assert message in error, error


def test_every_entry_is_in_the_table():
    from tonic_amd import _lib
    for entry, names in ENTRIES.items():
        assert len(names) == len(_lib.SIGNATURES[entry][1]), entry
    families = ('tonic_policy_forward', 'tonic_twin_q_grad', 'tonic_actor_q_grad', 'tonic_expected_sarsa_grad',
                'tonic_mpo_actor_grad', 'tonic_mpo_dual_step', 'tonic_distributional_q_grad',
                'tonic_distributional_actor_grad')
    assert {name for name in _lib.SIGNATURES if name.startswith(families)} == set(ENTRIES) and len(ENTRIES) == 16


# ---------------------------------------------------------------------------------- the pointer / shape check

@pytest.mark.parametrize('entry', ENTRIES)
def test_null_pointers_and_bad_numbers(lib, entry):
    """Every pointer NULL in turn, B = 0, the kinds, unknown torso codes, the sample / atom / action bounds: -1
    with the family's "bad argument" — also when the workspace is too small as well (the pointer check wins)."""
    names = ENTRIES[entry]
    bad = (FAMILY[entry] + ': bad argument').encode()
    small = dict(workspace_bytes=16) if 'workspace_bytes' in names else {}
    for pointer in pointers(entry):
        # the pointers a kind does without: d_eps of the DDPG critic step and of the deterministic actor step;
        # the greedy tonic_policy_forward has no noise at all
        if pointer == 'd_eps' and entry == 'tonic_policy_forward':
            continue
        message = b'null column sums' if pointer == 'd_column_sums' and 'shard' in entry else bad
        expect(call(lib, entry, **{pointer: None}), INVALID, message)
        expect(call(lib, entry, **{pointer: None}, **small), INVALID, message)
    if entry.startswith('tonic_twin_q_grad'):
        expect(call(lib, entry, kind=0, d_eps=None), INVALID, bad)
        expect(call(lib, entry, kind=2, d_eps=None, workspace_bytes=16), WORKSPACE)     # DDPG: no noise
    if entry.startswith('tonic_actor_q_grad'):
        expect(call(lib, entry, kind=1, d_eps=None), INVALID, bad)
        expect(call(lib, entry, kind=0, d_eps=None, workspace_bytes=16), WORKSPACE)     # deterministic: no draw
        for kind in (-1, 3):        # (no kind check of its own: any other kind is the twin-critic step)
            expect(call(lib, entry, kind=kind, workspace_bytes=16), WORKSPACE)
    if entry == 'tonic_policy_forward':
        for kind in (0, 1, 2):
            expect(call(lib, entry, kind=kind, d_eps=None, workspace_bytes=16), WORKSPACE)
    expect(call(lib, entry, B=0 if 'dual_step' not in entry else -1), INVALID, bad)
    expect(call(lib, entry, B=-1), INVALID, bad)
    if entry.startswith('tonic_twin_q_grad'):
        for kind in (-1, 3):
            expect(call(lib, entry, kind=kind), INVALID, bad)
    if 'H' in names:
        for code in UNKNOWN_H:
            expect(call(lib, entry, H=code, workspace_bytes=1 << 40), INVALID, bad)
    if 'S' in names:
        for S in (0, 257, -1):
            expect(call(lib, entry, S=S, **small), INVALID, bad + b' (1 <= samples <= 256')
    if 'NA' in names:
        for NA in (1, 65):
            expect(call(lib, entry, NA=NA, **small), INVALID, bad)
    if entry.startswith('tonic_mpo'):
        for A in (0, 65):
            expect(call(lib, entry, A=A, **small), INVALID, bad)
    if 'joint_kl' in names:
        for joint_kl in (2, -1):
            expect(call(lib, entry, joint_kl=joint_kl, **small), INVALID, bad)
    if 'B_global' in names:
        expect(call(lib, entry, B_global=0), INVALID, bad)


def test_policy_forward_kinds_are_not_checked_on_the_host(lib):
    """kind -1 / 3 of tonic_policy_forward reach the workspace check like any other (it has no kind check)."""
    for kind in (-1, 3):
        expect(call(lib, 'tonic_policy_forward', kind=kind, workspace_bytes=16), WORKSPACE,
               b'tonic_policy_forward: workspace too small')


@pytest.mark.parametrize('entry', ['tonic_twin_q_grad_ranged', 'tonic_actor_q_grad_ranged'])
def test_value_range_pair(lib, entry):
    """One bound without the other is refused first of all, under the _ranged entry's own name."""
    for pair, missing in ((dict(d_value_low=FAKE), b'd_value_high is NULL'), (dict(d_value_high=FAKE), b'd_value_low is NULL')):
        message = entry.encode() + b': ' + missing
        expect(call(lib, entry, **pair), INVALID, message)
        expect(call(lib, entry, d_grad_sums=None, **pair), INVALID, message)            # beats a null pointer
        expect(call(lib, entry, B=0, workspace_bytes=16, **pair), INVALID, message)
        if 'loss' in ENTRIES[entry]:
            for (rule, _) in BAD_LOSSES.values():                                         # beats a bad loss
                expect(call(lib, entry, loss=loss_rule(*rule), **pair), INVALID, message)
    expect(call(lib, entry, d_value_low=FAKE, d_value_high=FAKE, workspace_bytes=16), WORKSPACE,
           (FAMILY[entry] + ': workspace too small').encode())


@pytest.mark.parametrize('entry', [name for name, names in ENTRIES.items() if 'loss' in names])
@pytest.mark.parametrize('label', BAD_LOSSES)
def test_bad_critic_loss(lib, entry, label):
    """A bad tonic_critic_loss_t: -1 with the rule's message, ahead of the pointer and workspace checks."""
    rule, message = BAD_LOSSES[label]
    expect(call(lib, entry, loss=loss_rule(*rule)), INVALID, message)
    expect(call(lib, entry, loss=loss_rule(*rule), d_critics=None, d_critic=None), INVALID, message)   # beats a null pointer
    expect(call(lib, entry, loss=loss_rule(*rule), B=0, workspace_bytes=16), INVALID, message)


@pytest.mark.parametrize('entry', [name for name, names in ENTRIES.items() if 'loss' in names])
def test_good_critic_losses_reach_the_workspace_check(lib, entry):
    for rule in ((0, 0.0), (1, math.nan), (2, 0.0), (2, 1.5), (3, 1.0)):
        expect(call(lib, entry, loss=loss_rule(*rule), workspace_bytes=16), WORKSPACE,
               (FAMILY[entry] + ': workspace too small').encode())


# ---------------------------------------------------------------------------------- the workspace boundary

SHAPES = list(itertools.product((1, 17, 256), (3, 17), (1, 6, 17)))      # B, O, A


@pytest.mark.parametrize('torso', TORSOS)
@pytest.mark.parametrize('entry', [name for name, names in ENTRIES.items() if 'workspace_bytes' in names])
def test_workspace_boundary(lib, entry, torso):
    """Every other argument valid and the workspace ONE byte below the query: the workspace status and message."""
    H = torso_code(lib, torso)
    message = (FAMILY[entry] + ': workspace too small').encode()
    kinds = (0, 1, 2) if entry == 'tonic_policy_forward' or entry.startswith('tonic_twin_q') else \
        (0, 1) if entry.startswith('tonic_actor_q') else (None,)
    extras = [dict(S=S) for S in (1, 65)] if 'S' in ENTRIES[entry] else \
        [dict(NA=NA) for NA in (2, 51)] if 'NA' in ENTRIES[entry] else [{}]
    for (B, O, A), kind, extra in itertools.product(SHAPES, kinds, extras):
        values = dict(B=B, O=O, A=A, H=H, **extra)
        if kind is not None:
            values['kind'] = kind
        need = query(lib, entry, dict(DEFAULTS, **values))
        assert need > 1
        expect(call(lib, entry, workspace_bytes=need - 1, **values), WORKSPACE, message)
        expect(call(lib, entry, workspace_bytes=0, **values), WORKSPACE, message)


# ---------------------------------------------------------------------------------- tonic_q_iteration

def iteration(lib, **changes):
    """A valid tonic_q_iteration_t but for `changes` (workspace_bytes: the query's answer unless given)."""
    from tonic_amd._lib import QIteration, QOptimizer
    it = _keep(QIteration())
    for name, kind in QIteration._fields_:
        if kind is ctypes.c_void_p and name != 'ahead':
            setattr(it, name, FAKE)
    for half in (it.critic, it.actor):
        for name, kind in QOptimizer._fields_:
            setattr(half, name, FAKE if kind is ctypes.c_void_p else 1e-3)
    it.kind, it.actor_due, it.B, it.O, it.H, it.A = 1, 1, 17, 17, 64, 6
    it.norm_clip, it.target_coeff = 5.0, 0.005
    optimizers = {}
    for name, value in changes.items():
        if '.' in name:
            optimizers[name] = value
        elif name != 'workspace_bytes':
            setattr(it, name, value)
    for name, value in optimizers.items():
        half, field = name.split('.')
        setattr(getattr(it, half), field, value)
    it.workspace_bytes = changes.get('workspace_bytes', lib.tonic_q_iteration_workspace_bytes(it.B, it.O, it.A, it.H))
    return ctypes.cast(ctypes.pointer(it), ctypes.c_void_p)


def iterate(lib, **changes):
    status = lib.tonic_q_iteration(iteration(lib, **changes), None)
    return status, lib.tonic_last_error()


def test_q_iteration_refusals(lib):
    from tonic_amd._lib import CriticLoss, QIteration, QOptimizer
    expect((lib.tonic_q_iteration(None, None), lib.tonic_last_error()), INVALID, b'tonic_q_iteration: null arguments')
    bad = b'tonic_q_iteration: bad argument'
    pointers = [name for name, kind in QIteration._fields_ if kind is ctypes.c_void_p and name != 'ahead']
    pointers += [f'{half}.{name}' for half in ('critic', 'actor') for name, kind in QOptimizer._fields_
                 if kind is ctypes.c_void_p and name not in ('d_info_row', 'd_step_constants')]
    for pointer in pointers:
        expect(iterate(lib, **{pointer: None}), INVALID, bad)
        expect(iterate(lib, **{pointer: None}, workspace_bytes=16), INVALID, bad)        # beats the workspace
    # the draws a kind does without
    expect(iterate(lib, kind=2, d_eps_critic=None, d_eps_actor=None, workspace_bytes=16), WORKSPACE)
    expect(iterate(lib, kind=0, d_eps_actor=None, workspace_bytes=16), WORKSPACE)
    expect(iterate(lib, kind=1, actor_due=0, d_eps_actor=None, workspace_bytes=16), WORKSPACE)
    for name in ('critic.d_info_row', 'critic.d_step_constants', 'actor.d_info_row', 'actor.d_step_constants'):
        expect(iterate(lib, **{name: None}, workspace_bytes=16), WORKSPACE)
    for changes in (dict(B=0), dict(B=-1), dict(kind=-1), dict(kind=3)):
        expect(iterate(lib, **changes), INVALID, bad)
    expect(iterate(lib, phase=3), INVALID, b'tonic_q_iteration: phase 3 (actor_due 1)')
    expect(iterate(lib, phase=-1), INVALID, b'tonic_q_iteration: phase -1')
    expect(iterate(lib, phase=2, actor_due=0), INVALID, b'tonic_q_iteration: phase 2 (actor_due 0)')
    expect(iterate(lib, stage=1), INVALID, b'tonic_q_iteration: stage 1, slot 0 (phase 0)')
    expect(iterate(lib, stage=2, phase=1), INVALID, b'tonic_q_iteration: stage 2, slot 0 (phase 1)')
    expect(iterate(lib, slot=2), INVALID, b'tonic_q_iteration: stage 0, slot 2 (phase 0)')
    for code in UNKNOWN_H + (lib.tonic_mlp_hidden(40, 24, 2), torso_code(lib, 'relu32x3'), torso_code(lib, 'one256')):
        expect(iterate(lib, H=code, workspace_bytes=1 << 40), SHAPE, b'outside the fused kernels')
    # which check wins: the loss, then the phase, then stage / slot, then the pointers, then the shape, then the workspace
    for (rule, message) in BAD_LOSSES.values():
        loss = CriticLoss(rule[0], 0, rule[1])
        expect(iterate(lib, critic_loss=loss), INVALID, message)
        expect(iterate(lib, critic_loss=loss, phase=3, d_actor=None, workspace_bytes=16), INVALID, message)
    expect(iterate(lib, phase=3, slot=2, d_actor=None), INVALID, b'phase 3')
    expect(iterate(lib, slot=2, d_actor=None), INVALID, b'slot 2')
    expect(iterate(lib, d_actor=None, H=400), INVALID, bad)
    expect(iterate(lib, H=400, workspace_bytes=16), SHAPE, b'outside the fused kernels')
    # the next iteration's passes: refused unless this one is a whole iteration that leaves the actor alone
    expect(iterate(lib, ahead=iteration(lib, slot=1)), INVALID, b'policy passes ahead')


@pytest.mark.parametrize('torso', ['plain64', 'plain256'])
def test_q_iteration_workspace_boundary(lib, torso):
    H = torso_code(lib, torso)
    for (B, O, A), kind, due, slot in itertools.product(SHAPES, (0, 1, 2), (0, 1), (0, 1)):
        need = lib.tonic_q_iteration_workspace_bytes(B, O, A, H)
        assert need > 1
        for phase in ((0, 1, 2) if due else (0, 1)):
            expect(iterate(lib, B=B, O=O, A=A, H=H, kind=kind, actor_due=due, slot=slot, phase=phase,
                           workspace_bytes=need - 1), WORKSPACE, b'tonic_q_iteration: workspace too small')


def test_collector_q_act_without_a_collector(lib):
    for kind in (0, 1):
        assert lib.tonic_collector_q_act(None, FAKE, FAKE, 0, kind, 64, -1, None, None, FAKE, 1 << 30, None) == INVALID
        assert b'tonic_collector_q_act: bad argument' in lib.tonic_last_error()


# ---------------------------------------------------------------------------------- the queries

# What the build BEFORE the layouts stated their own sizes answered (its hand-summed formulas with their slack), for
# every torso of TORSOS x SHAPES in that order; the measured layouts may ask for less, never for more.
# tonic_offpolicy_workspace_bytes(B, O, A, H) | tonic_q_iteration_workspace_bytes (plain torsos) |
# tonic_distributional_workspace_bytes(.., NA = 2, 51) | tonic_mpo_workspace_bytes(.., S = 1, 65)
BEFORE = {
    'plain64': {
        'offpolicy': [
            402624, 403264, 447424, 406464, 407104, 482496, 482176, 483456, 539008, 489856, 491136, 576384, 1595904,
            1606144, 1821184, 1657344, 1667584, 1890816
        ],
        'distributional': [
            57984, 67200, 58304, 67520, 64640, 73856, 60544, 69760, 60864, 70080, 66176, 75392, 109824, 128256,
            110464, 128896, 123136, 141568, 114944, 133376, 115584, 134016, 126208, 144640, 835584, 983040, 840704,
            988160, 942080, 1089536, 876544, 1024000, 881664, 1029120, 966656, 1114112
        ],
        'mpo': [
            70080, 109504, 71040, 111744, 81856, 130496, 72640, 117184, 73600, 119424, 83392, 135104, 131968,
            802176, 133888, 825856, 155520, 982400, 137088, 894336, 139008, 918016, 158592, 1037696, 998400,
            11090944, 1013760, 11433984, 1186816, 13638656, 1039360, 12442624, 1054720, 12785664, 1211392, 14449664
        ],
        'q_iteration': [
            447232, 449152, 508160, 454912, 456832, 545536, 566528, 570368, 655616, 581888, 585728, 697600, 2236672,
            2267392, 2720000, 2359552, 2390272, 2826496
        ],
    },
    'plain256': {
        'offpolicy': [
            3892416, 3893056, 4035520, 3896256, 3896896, 4168896, 4168576, 4169856, 4323712, 4176256, 4177536,
            4459392, 8034816, 8045056, 8358400, 8096256, 8106496, 8526336
        ],
        'distributional': [
            180864, 190080, 181184, 190400, 187520, 196736, 183424, 192640, 183744, 192960, 189056, 198272, 355584,
            374016, 356224, 374656, 368896, 387328, 360704, 379136, 361344, 379776, 371968, 390400, 2801664,
            2949120, 2806784, 2954240, 2908160, 3055616, 2842624, 2990080, 2847744, 2995200, 2932736, 3080192
        ],
        'mpo': [
            217536, 355264, 218496, 357504, 229312, 376256, 220096, 362944, 221056, 365184, 230848, 380864, 426880,
            2768256, 428800, 2791936, 450432, 2948480, 432000, 2860416, 433920, 2884096, 453504, 3003776, 3357696,
            38616064, 3373056, 38959104, 3546112, 41163776, 3398656, 39967744, 3414016, 40310784, 3570688, 41974784
        ],
        'q_iteration': [
            4010752, 4012672, 4169984, 4018432, 4020352, 4305664, 4400384, 4404224, 4587776, 4415744, 4419584,
            4728064, 9855232, 9885952, 10436864, 9978112, 10008832, 10641664
        ],
    },
    'tanh40x24': {
        'offpolicy': [
            62656, 63296, 74688, 66496, 67136, 76992, 113536, 114816, 137600, 121216, 122496, 142208, 825856,
            836096, 1018368, 887296, 897536, 1055232
        ],
        'distributional': [
            40064, 49280, 40384, 49600, 46720, 55936, 42624, 51840, 42944, 52160, 48256, 57472, 73984, 92416, 74624,
            93056, 87296, 105728, 79104, 97536, 79744, 98176, 90368, 108800, 548864, 696320, 553984, 701440, 655360,
            802816, 589824, 737280, 594944, 742400, 679936, 827392
        ],
        'mpo': [
            48576, 73664, 49536, 75904, 60352, 94656, 51136, 81344, 52096, 83584, 61888, 99264, 88960, 515456,
            90880, 539136, 112512, 695680, 94080, 607616, 96000, 631296, 115584, 750976, 654336, 7076864, 669696,
            7419904, 842752, 9624576, 695296, 8428544, 710656, 8771584, 867328, 10435584
        ],
    },
    'relu32x3': {
        'offpolicy': [
            76992, 77632, 89024, 80832, 81472, 91328, 142208, 143488, 166272, 149888, 151168, 170880, 1055232,
            1065472, 1247744, 1116672, 1126912, 1284608
        ],
        'distributional': [
            49024, 58240, 49344, 58560, 55680, 64896, 51584, 60800, 51904, 61120, 57216, 66432, 91904, 110336,
            92544, 110976, 105216, 123648, 97024, 115456, 97664, 116096, 108288, 126720, 692224, 839680, 697344,
            844800, 798720, 946176, 733184, 880640, 738304, 885760, 823296, 970752
        ],
        'mpo': [
            59328, 91584, 60288, 93824, 71104, 112576, 61888, 99264, 62848, 101504, 72640, 117184, 110464, 658816,
            112384, 682496, 134016, 839040, 115584, 750976, 117504, 774656, 137088, 894336, 826368, 9083904, 841728,
            9426944, 1014784, 11631616, 867328, 10435584, 882688, 10778624, 1039360, 12442624
        ],
    },
    'one256': {
        'offpolicy': [
            287936, 288576, 299968, 291776, 292416, 302272, 564096, 565376, 588160, 571776, 573056, 592768, 4430336,
            4440576, 4622848, 4491776, 4502016, 4659712
        ],
        'distributional': [
            180864, 190080, 181184, 190400, 187520, 196736, 183424, 192640, 183744, 192960, 189056, 198272, 355584,
            374016, 356224, 374656, 368896, 387328, 360704, 379136, 361344, 379776, 371968, 390400, 2801664,
            2949120, 2806784, 2954240, 2908160, 3055616, 2842624, 2990080, 2847744, 2995200, 2932736, 3080192
        ],
        'mpo': [
            217536, 355264, 218496, 357504, 229312, 376256, 220096, 362944, 221056, 365184, 230848, 380864, 426880,
            2768256, 428800, 2791936, 450432, 2948480, 432000, 2860416, 433920, 2884096, 453504, 3003776, 3357696,
            38616064, 3373056, 38959104, 3546112, 41163776, 3398656, 39967744, 3414016, 40310784, 3570688, 41974784
        ],
    },
}


def answers(lib, torso):
    H = torso_code(lib, torso)
    row = {'offpolicy': [lib.tonic_offpolicy_workspace_bytes(B, O, A, H) for B, O, A in SHAPES],
           'distributional': [lib.tonic_distributional_workspace_bytes(B, O, A, H, NA)
                              for (B, O, A), NA in itertools.product(SHAPES, (2, 51))],
           'mpo': [lib.tonic_mpo_workspace_bytes(B, O, A, H, S) for (B, O, A), S in itertools.product(SHAPES, (1, 65))]}
    if torso.startswith('plain'):
        row['q_iteration'] = [lib.tonic_q_iteration_workspace_bytes(B, O, A, H) for B, O, A in SHAPES]
    return row


@pytest.mark.parametrize('torso', TORSOS)
def test_queries_are_positive_and_never_above_the_hand_summed_ones(lib, torso):
    now = answers(lib, torso)
    assert set(now) == set(BEFORE[torso])
    for name, values in now.items():
        assert len(values) == len(BEFORE[torso][name])
        for got, before in zip(values, BEFORE[torso][name]):
            assert 0 < got <= before, (name, got, before)


def test_queries_are_functions_of_their_arguments(lib):
    """The run-time switches (weight images, fused policy tail, chained launches) decide what an entry carves,
    never what a query answers."""
    want = {torso: answers(lib, torso) for torso in TORSOS}
    switches = ('q_images', 'policy_tail', 'q_chain')
    saved = {}
    try:
        for name in switches:
            value = ctypes.c_int32(0)
            assert lib.tonic_get_tuning(name.encode(), ctypes.addressof(value)) == OK, name
            saved[name] = value.value
            assert lib.tonic_set_tuning(name.encode(), 0) == OK, name
        assert {torso: answers(lib, torso) for torso in TORSOS} == want
    finally:
        for name, value in saved.items():
            lib.tonic_set_tuning(name.encode(), value)
