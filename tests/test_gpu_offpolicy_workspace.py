"""Nothing an off-policy entry launches writes past the size its query answers: every layout and route of
csrc/offpolicy.hip runs in a workspace of exactly `query` bytes with 64 KiB of a byte pattern behind it; the pattern
must come back intact and every output finite.

CASES / run_case are also what scripts/offpolicy_entry_bits.py feeds to a given build of the library to print the
sha256 of every output buffer.
"""
import ctypes
import itertools

import pytest
import torch

GUARD, PATTERN = 65536, 0xA5
TORSOS = {'plain64': ((64, 64), 1),            # the fused kernels, weight images
          'tanh40x24': ((40, 24), 2),          # layer by layer
          'relu32x3': ((32, 32, 32), 1)}       # layer by layer, three layers per region
_alive = []


def torso_code(lib, torso):
    sizes, activation = TORSOS[torso]
    array = (ctypes.c_int32 * len(sizes))(*sizes)
    _alive.append(array)
    code = lib.tonic_mlp_torso(len(sizes), ctypes.cast(array, ctypes.c_void_p), activation)
    assert code > 0
    return code


def _pack(lib, gen, layers):
    """A network in the padded layout (csrc/offpolicy.hip: actor_count): per layer W [rows, weight_ld(cols)] and
    b [slot4(rows)], the padding zero."""
    parts = []
    for rows, cols in layers:
        W = torch.zeros(rows, lib.tonic_mlp_weight_stride(cols))
        W[:, :cols] = torch.randn(rows, cols, generator=gen) * 0.2
        b = torch.zeros((rows + 3) // 4 * 4)
        b[:rows] = torch.randn(rows, generator=gen) * 0.1
        parts += [W.reshape(-1), b]
    return torch.cat(parts).cuda()


def _chain(inputs, sizes):
    return list(zip(sizes, (inputs,) + tuple(sizes[:-1])))


class Data:
    """Seeded inputs of one case: networks of `torso`, a batch, noise, the normaliser."""

    def __init__(self, lib, torso, B, O, A, samples=1, atoms=0):
        gen = torch.Generator().manual_seed(B * 1000 + O * 100 + A)
        sizes = TORSOS[torso][0]
        self.lib, self.H, self.B, self.O, self.A = lib, torso_code(lib, torso), B, O, A

        def actor(heads):
            flat = _pack(lib, gen, _chain(O, sizes) + [(A, sizes[-1])] * heads)
            assert flat.numel() == lib.tonic_mlp_actor_param_count(O, self.H, A, heads)
            return flat

        def critics(nets, outputs=1):
            flat = torch.cat([_pack(lib, gen, _chain(O + A, sizes) + [(outputs, sizes[-1])]) for _ in range(nets)])
            count = lib.tonic_q_critic_param_count(O, A, self.H) if outputs == 1 else \
                lib.tonic_mlp_actor_param_count(O + A, self.H, outputs, 1)
            assert flat.numel() == nets * count
            return flat

        self.actor, self.critics = actor, critics
        rand = lambda *shape: torch.randn(*shape, generator=gen).cuda()           # noqa: E731
        self.obs, self.next_obs = rand(B, O), rand(B, O)
        self.actions = torch.tanh(rand(B, A))
        self.rewards, self.discounts = rand(B), torch.full((B,), 0.99).cuda()
        self.eps, self.eps2 = rand(samples * B, A), rand(B, A)
        self.mean, self.std = rand(O) * 0.1, 1.0 + rand(O).abs() * 0.1
        self.low, self.high = torch.tensor([-3.0]).cuda(), torch.tensor([4.0]).cuda()
        self.values = torch.linspace(-10.0, 10.0, max(atoms, 2)).cuda()
        # importance weights > 0 and SAC's log entropy coefficient, from a generator of their own: `gen` goes on to draw
        # the networks, which keep their values
        more = torch.Generator().manual_seed(B * 1000 + O * 100 + A + 7)
        self.weights = (torch.rand(B, generator=more) + 0.1).cuda()
        self.log_coeff = (torch.randn(1, generator=more) * 0.5 - 1.0).cuda()


def guarded(need):
    """A zero-filled workspace of `need` bytes with the guard behind it."""
    assert need > 0
    buffer = torch.zeros(need + GUARD, dtype=torch.uint8, device='cuda')
    buffer[need:] = PATTERN
    return buffer


def zeros(n, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype, device='cuda')


# ------------------------------------------------------------------ one function per family: (status, outputs, ws, need)

def policy_forward(lib, p, kind, torso, B, O, A):
    d = Data(lib, torso, B, O, A)
    need = lib.tonic_offpolicy_workspace_bytes(B, O, A, d.H)
    ws, out = guarded(need), zeros(B * A)
    status = lib.tonic_policy_forward(p(d.actor(1 if kind == 0 else 2)), p(d.obs), p(d.eps), p(out), kind, B, O, d.H, A,
                                      p(ws), need, None)
    return status, {'actions': out}, ws, need


def twin_q(lib, p, kind, torso, B, O, A, ranged):
    d = Data(lib, torso, B, O, A)
    nets = 1 if kind == 2 else 2
    policy, targets, critics = d.actor(2 if kind == 1 else 1), d.critics(nets), d.critics(nets)
    need = lib.tonic_offpolicy_workspace_bytes(B, O, A, d.H)
    ws, out = guarded(need), zeros(critics.numel() + 8)
    status = lib.tonic_twin_q_grad_ranged(
        kind, p(policy), p(targets), p(critics), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.actions), p(d.next_obs),
        p(d.rewards), p(d.discounts), p(d.eps), p(out), B, O, d.H, A, 0.2, 0.2, 0.5, None,
        p(d.low) if ranged else None, p(d.high) if ranged else None, p(ws), need, None)
    return status, {'grad_sums': out}, ws, need


def actor_q(lib, p, kind, torso, B, O, A, ranged):
    d = Data(lib, torso, B, O, A)
    actor, critics = d.actor(1 if kind == 0 else 2), d.critics(1 if kind == 0 else 2)
    need = lib.tonic_offpolicy_workspace_bytes(B, O, A, d.H)
    ws, out = guarded(need), zeros(actor.numel() + 8)
    status = lib.tonic_actor_q_grad_ranged(
        kind, p(actor), p(critics), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.eps), p(out), B, O, d.H, A, 0.2,
        p(d.low) if ranged else None, p(d.high) if ranged else None, p(ws), need, None)
    return status, {'grad_sums': out}, ws, need


def tempered_twin_q(lib, p, torso, B, O, A, ranged):
    d = Data(lib, torso, B, O, A)
    policy, targets, critics = d.actor(2), d.critics(2), d.critics(2)
    need = lib.tonic_offpolicy_workspace_bytes(B, O, A, d.H)
    ws, out = guarded(need), zeros(critics.numel() + 8)
    status = lib.tonic_tempered_twin_q_grad(
        1, p(policy), p(targets), p(critics), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.actions), p(d.next_obs),
        p(d.rewards), p(d.discounts), p(d.eps), p(out), B, O, d.H, A, 0.2, 0.2, 0.5, None,
        p(d.low) if ranged else None, p(d.high) if ranged else None, p(d.log_coeff), p(ws), need, None)
    return status, {'grad_sums': out}, ws, need


def tempered_actor_q(lib, p, torso, B, O, A, ranged):
    d = Data(lib, torso, B, O, A)
    actor, critics = d.actor(2), d.critics(2)
    need = lib.tonic_offpolicy_workspace_bytes(B, O, A, d.H)
    ws, out, coeff_sums = guarded(need), zeros(actor.numel() + 8), zeros(1 + 8)
    status = lib.tonic_tempered_actor_q_grad(
        1, p(actor), p(critics), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.eps), p(out), B, O, d.H, A, 0.2,
        p(d.low) if ranged else None, p(d.high) if ranged else None, p(d.log_coeff), p(coeff_sums), -float(A), p(ws),
        need, None)
    return status, {'grad_sums': out, 'entropy_coeff_sums': coeff_sums}, ws, need


def q_regression(lib, p, torso, B, O, A, ranged):
    d = Data(lib, torso, B, O, A)
    critic = d.critics(1)
    need = lib.tonic_q_regression_workspace_bytes(B, O, A, d.H)
    ws, out = guarded(need), zeros(critic.numel() + 8)
    status = lib.tonic_q_regression_grad(
        p(critic), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.actions), p(d.rewards), p(out), B, O, d.H, A, None,
        p(d.low) if ranged else None, p(d.high) if ranged else None, p(ws), need, None)
    return status, {'grad_sums': out}, ws, need


def distributional_q(lib, p, torso, B, O, A, NA, weighted=False):
    d = Data(lib, torso, B, O, A, atoms=NA)
    target_actor, target_critic, critic = d.actor(1), d.critics(1, NA), d.critics(1, NA)
    need = lib.tonic_distributional_workspace_bytes(B, O, A, d.H, NA)
    ws, out = guarded(need), zeros(critic.numel() + 8)
    head = [p(target_actor), p(target_critic), p(critic), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.actions),
            p(d.next_obs), p(d.rewards), p(d.discounts), p(d.values), p(out), B, O, d.H, A, NA]
    if not weighted:
        return lib.tonic_distributional_q_grad(*head, p(ws), need, None), {'grad_sums': out}, ws, need
    losses = zeros(B)
    status = lib.tonic_weighted_distributional_q_grad(*head, p(d.weights), p(losses), p(ws), need, None)
    return status, {'grad_sums': out, 'sample_losses': losses}, ws, need


def twin_distributional_q(lib, p, torso, B, O, A, NA, weighted=False):
    d = Data(lib, torso, B, O, A, atoms=NA)
    target_actor, target_critics, critics = d.actor(1), d.critics(2, NA), d.critics(2, NA)
    need = lib.tonic_twin_distributional_workspace_bytes(B, O, A, d.H, NA)
    ws, out = guarded(need), zeros(critics.numel() + 8)
    head = [p(target_actor), p(target_critics), p(critics), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.actions),
            p(d.next_obs), p(d.rewards), p(d.discounts), p(d.eps), p(d.values), p(out), B, O, d.H, A, NA, 0.2, 0.5]
    if not weighted:
        return lib.tonic_twin_distributional_q_grad(*head, p(ws), need, None), {'grad_sums': out}, ws, need
    losses = zeros(B)
    status = lib.tonic_weighted_twin_distributional_q_grad(*head, p(d.weights), p(losses), p(ws), need, None)
    return status, {'grad_sums': out, 'sample_losses': losses}, ws, need


def distributional_actor(lib, p, torso, B, O, A, NA):
    d = Data(lib, torso, B, O, A, atoms=NA)
    actor, critic = d.actor(1), d.critics(1, NA)
    need = lib.tonic_distributional_workspace_bytes(B, O, A, d.H, NA)
    ws, out = guarded(need), zeros(actor.numel() + 8)
    status = lib.tonic_distributional_actor_grad(
        p(actor), p(critic), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.values), p(out), B, O, d.H, A, NA, p(ws), need,
        None)
    return status, {'grad_sums': out}, ws, need


def expected_sarsa(lib, p, torso, B, O, A, S):
    d = Data(lib, torso, B, O, A, samples=S)
    target_actor, target_critic, critic = d.actor(2), d.critics(1), d.critics(1)
    need = lib.tonic_mpo_workspace_bytes(B, O, A, d.H, S)
    ws, out = guarded(need), zeros(critic.numel() + 8)
    status = lib.tonic_expected_sarsa_grad_loss(
        p(target_actor), p(target_critic), p(critic), p(d.mean), p(d.std), 5.0, p(d.obs), p(d.actions), p(d.next_obs),
        p(d.rewards), p(d.discounts), p(d.eps), p(out), B, O, d.H, A, S, None, p(ws), need, None)
    return status, {'grad_sums': out}, ws, need


def mpo_actor(lib, p, torso, B, O, A, S, joint_kl, shard):
    d = Data(lib, torso, B, O, A, samples=S)
    actor, target_actor, target_critic = d.actor(2), d.actor(2), d.critics(1)
    need = lib.tonic_mpo_workspace_bytes(B, O, A, d.H, S)
    ws, out, duals = guarded(need), zeros(actor.numel() + 8), zeros(2 * A + 2)
    head = [p(actor), p(target_actor), p(target_critic), p(duals), -18.0, p(d.mean), p(d.std), 5.0, p(d.obs), p(d.eps),
            p(out)]
    if shard:
        sums = zeros(6 + 2 * A, torch.float64)
        status = lib.tonic_mpo_actor_grad_shard_joint(*head, p(sums), B, O, d.H, A, S, 1, joint_kl, p(ws), need, None)
        return status, {'grad_sums': out, 'column_sums': sums, 'duals': duals}, ws, need
    dual_grads, stats = zeros(2 * A + 2 + 8), zeros(7 + 2 * A + 2)
    status = lib.tonic_mpo_actor_grad_joint(*head, p(dual_grads), p(stats), B, O, d.H, A, S, 0.1, 1e-3, 1e-3, 1e-6, 1,
                                            joint_kl, p(ws), need, None)
    return status, {'grad_sums': out, 'dual_grads': dual_grads, 'stats': stats, 'duals': duals}, ws, need


def q_iteration(lib, p, kind, due, slot, torso='plain64', B=17, O=3, A=17):
    from tonic_amd._lib import QIteration
    d = Data(lib, torso, B, O, A)
    nets, heads = (1 if kind == 2 else 2), (2 if kind == 1 else 1)
    it = QIteration()
    it.kind, it.actor_due, it.B, it.O, it.H, it.A = kind, due, B, O, d.H, A
    nets_ = {'d_actor': d.actor(heads), 'd_critics': d.critics(nets), 'd_target_actor': d.actor(heads),
             'd_target_critics': d.critics(nets)}
    inputs = {'d_norm_mean': d.mean, 'd_norm_std': d.std, 'd_observations': d.obs, 'd_actions': d.actions,
              'd_next_observations': d.next_obs, 'd_rewards': d.rewards, 'd_discounts': d.discounts,
              'd_eps_critic': d.eps, 'd_eps_actor': d.eps2}
    for name, tensor in {**nets_, **inputs}.items():
        setattr(it, name, p(tensor))
    it.norm_clip, it.critic_entropy_coeff, it.actor_entropy_coeff = 5.0, 0.2, 0.2
    it.noise_scale, it.noise_clip, it.target_coeff = 0.2, 0.5, 0.005
    outputs = dict(nets_)
    for half, params in ((it.critic, nets_['d_critics']), (it.actor, nets_['d_actor'])):
        state = {'d_grad_sums': zeros(params.numel() + 8), 'd_exp_avg': zeros(params.numel()),
                 'd_exp_avg_sq': zeros(params.numel()), 'd_state': zeros(4, torch.int32), 'd_info_row': zeros(8)}
        for name, tensor in state.items():
            setattr(half, name, p(tensor))
            outputs[f'{"critic" if half is it.critic else "actor"}.{name}'] = tensor
        half.lr, half.beta1, half.beta2, half.eps = 3e-4, 0.9, 0.999, 1e-8
    need = lib.tonic_q_iteration_workspace_bytes(B, O, A, d.H)
    ws = guarded(need)             # (zero-filled: the failure words)
    it.d_workspace, it.workspace_bytes = p(ws), need
    it.refresh_images, it.slot = 1, slot
    status = lib.tonic_q_iteration(ctypes.cast(ctypes.pointer(it), ctypes.c_void_p), None)
    return status, outputs, ws, need


def _cases():
    cases = []

    def add(function, **kwargs):
        label = '-'.join(f'{k}={v}' for k, v in kwargs.items())
        cases.append(pytest.param(function, kwargs, id=f'{function.__name__}-{label}'))

    shapes = [dict(torso=t, B=B, O=3, A=A) for t, B, A in itertools.product(TORSOS, (1, 17), (1, 17))]
    for shape in shapes:
        for kind in (0, 1, 2):
            add(policy_forward, kind=kind, **shape)
            for ranged in (False, True):
                add(twin_q, kind=kind, ranged=ranged, **shape)
                if kind < 2:
                    add(actor_q, kind=kind, ranged=ranged, **shape)
        for ranged in (False, True):
            add(q_regression, ranged=ranged, **shape)
            add(tempered_twin_q, ranged=ranged, **shape)
            add(tempered_actor_q, ranged=ranged, **shape)
    for torso in TORSOS:
        shape = dict(torso=torso, B=17, O=3, A=17)
        for NA in (2, 51, 64):                  # 2: a row of 2 in a pitch of 16; 64: lane 63 is the last atom
            add(distributional_q, NA=NA, **shape)
            add(distributional_q, NA=NA, weighted=True, **shape)
            add(twin_distributional_q, NA=NA, **shape)
            add(twin_distributional_q, NA=NA, weighted=True, **shape)
            add(distributional_actor, NA=NA, **shape)
        for S in (1, 65):                       # 65: two register slots in the state kernel
            add(expected_sarsa, S=S, **shape)
            for joint_kl, shard in itertools.product((0, 1), (False, True)):
                add(mpo_actor, S=S, joint_kl=joint_kl, shard=shard, **shape)
    for B in (1, 5):                            # the loss kernels place 4 samples per block: a lone wave, a ragged block
        shape = dict(torso='plain64', B=B, O=3, A=17, NA=51)
        for function, weighted in itertools.product((distributional_q, twin_distributional_q), (False, True)):
            add(function, weighted=weighted, **shape)
    for kind, due, slot in itertools.product((0, 1, 2), (0, 1), (0, 1)):
        add(q_iteration, kind=kind, due=due, slot=slot)
    return cases


CASES = _cases()


def run_case(lib, function, kwargs):
    """Runs one case; returns (outputs, the guard's bytes) after the stream has drained."""
    from tonic_amd import _lib
    status, outputs, ws, need = function(lib, _lib.ptr, **kwargs)
    _lib.check(status, function.__name__)
    torch.cuda.synchronize()
    return outputs, ws[need:]


@pytest.fixture(scope='module')
def lib():
    from tonic_amd import _lib
    return _lib.load()


@pytest.mark.gpu
@pytest.mark.parametrize('function, kwargs', CASES)
def test_nothing_is_written_past_the_query(lib, function, kwargs):
    outputs, guard = run_case(lib, function, kwargs)
    assert guard.numel() == GUARD and bool((guard == PATTERN).all()), 'a launch wrote behind the workspace'
    for name, tensor in outputs.items():
        assert bool(torch.isfinite(tensor.double()).all()), name
