"""GPU tests of the off-policy LAYER-BY-LAYER route (csrc/offpolicy.hip: actor_forward, critics_forward,
critics_backward, critics_weight_gradients, actor_shaped_backward, actor_weight_gradients as launch_gemm /
launch_gemm_group calls, and the stand-alone tail kernels) against float64 at its edges.  Every case runs one critic
step and one actor step through the updaters' `enqueue`, both from the same parameters, batch and noise (the online
parameters are put back behind the critic step's optimizer), with a MeanStd of non-trivial mean and std, and asserts:

- the route: `stock is False`, `hidden == sizes[0]` exactly for a plain torso, no weight images where the case is
  meant to run without them;
- the preconditions of its inputs (tests/offpolicy_layered_ref.py), on the float64 reference, before the GPU runs;
- every gradient tensor within 1e-5 of the float64 tensor's largest element, critics and actor alike;
- the logged statistics (`_check_stat`), slot 5 == B and the unused slots zero;
- the padding floats of both gradient-sum blocks exactly zero.

The cases, their inputs and the seeds are tests/offpolicy_layered_ref.py's; tests/test_offpolicy_layered_ref_host.py
pins the float64 restatement to the stock modules.  Results: profiles/offpolicy_layered_edges_accuracy.md.

Which launches a shape takes (read from offpolicy.hip; nets = 2 for SAC / TD3, 1 for DDPG; L = layers):

LAYERED — every torso here but (64, 64) ReLU: the non-plain ones, and the plain (8, 8), (24, 24), (272, 272), which
mlp_forward_supported / mlp_backward_supported refuse (H < 16, H % 16, H > 256); images_serve refuses them too.
  critic step (tonic_twin_q_grad_loss):
    actor_forward: L launch_gemm('c', 'c') with bias + activation, one more per head (2 for SAC); the hidden arrays'
      pitch is weight_ld(widest layer), so a narrower layer ((15, 17), (17, 15), (33, 1, 33)) leaves columns unused;
    the tail on its own: td3_target_action_kernel / copy_actions_kernel / sac_sample_kernel (groups of
      sample_group(A) <= 32 lanes; A = 33, 65 loop), then encode_kernel with grid.y = 2: (s', a') -> X, (s, a) -> X2;
    critics_forward, two passes (targets on X, online on X2): per pass L launch_gemm over nets in blockIdx.z
      (strideB = strideBias = count, strideC = hs, strideA = 0 then hs) and the value head (N = 1, ldc = 1,
      strideC = Bp);
    critic_loss_kernel <<<1, 1024>>> (B = 1100: its m += blockDim.x loop);
    the chain: launch_gemm('c', 's') dq w3 under the activation's mask, L - 1 more down to dz1;
    critics_weight_gradients: one launch_gemm_group('s', 's') of L + 1 problems x nets, bias gradients as column sums.
  actor step (tonic_actor_q_grad):
    actor_forward as above, copy_actions_kernel / sac_sample_kernel (with sigma), encode_kernel (grid.y = 1);
    critics_forward, one pass; actor_loss_kernel <<<1, 1024>>>; the critics' chain as above without weight gradients,
      then dxa = dz1 W1[:, O : O + A] (B operand at W1 + O, pitch ld1; C pitch pad16(A); strideC = Bp pad16(A));
    actor_head_backward_kernel (both critics' dxa added for SAC);
    actor_shaped_backward: one masked launch_gemm per head (the second accumulates), L - 1 more, then
      actor_weight_gradients: one launch_gemm_group of heads + L problems.
MIXED — (64, 64) ReLU at A = 65, O = 3 (q_images at its default; images_serve refuses A > 64, so float32 passes):
  critic step: the actor layer by layer (heads * ceil(65 / 16) > 4) with its stand-alone tail and encode_kernel; the
    four critics' forward in ONE fused launch_mlp_forward; the chain with the TD loss in ONE launch_mlp_backward
    (xa_count = 0); the weight-gradient group over the fused forward's h1 / h2.
  actor step: the actor layer by layer; the critics' forward fused; their chain LAYERED (xa_count = 65 > 64) with
    actor_loss_kernel, over the h1 / h2 the fused forward wrote — both sides take the pitch weight_ld(64) = 68; the
    actor's backward layer by layer (NH = 65 > 64).
D4PG (tonic_distributional_q_grad / _actor_grad): actor and categorical critics are both actor-shaped networks run by
  actor_forward / actor_shaped_backward (the critic's dxa at xa_first = O), with distributional_critic_loss_kernel /
  distributional_actor_loss_kernel, loss_stats_kernel and actor_head_backward_kernel between them.
MPO: tonic_expected_sarsa_grad — actor_forward (2 heads), gaussian_tile_kernel, critics_forward on S * B rows,
  sample_mean_kernel, encode_kernel, critics_forward / critics_backward of one critic; tonic_mpo_actor_grad — the same
  sampled values, the online actor_forward, mpo_state_kernel<ceil(S / 64)>, mpo_dual_kernel, actor_shaped_backward.
  The temperature's dual is log T = 1 here (test_gpu_offpolicy_grads.py runs the cold one, where the float32 E-step
  weights need a wider bound): these cases hold the actor to 1e-5 like every other."""
import pytest

import offpolicy_layered_ref as layered
from test_gpu_offpolicy_grads import (Ref, _agent, _d4pg_steps, _mpo_call, _mpo_compare, _q_hyper, _q_steps,
                                      _sarsa_step, lib)                     # noqa: F401  (lib: the fixture)
from test_gpu_q_regression import _padding

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

BOUND = 1e-5


def _ids(cases):
    return [layered.case_id(c) for c in cases]


def _prepare(lib, case, **mpo):
    """The case's agent with the drawn parameters and normaliser installed, its route asserted, its inputs'
    preconditions asserted on the float64 reference of the agent's own parameters: (agent, inputs, reference)."""
    agent = _agent(case.kind, case.O, case.A, case.B, sizes=case.sizes, activation=case.activation,
                   atoms=layered.atoms(case), S=max(case.S, 1), **mpo)
    model = agent.model
    inputs = layered.draw(case, layered.seed_of(case), model)
    layered.install(model, inputs)
    heads = 2 if case.kind in ('sac', 'mpo') else 1
    for updater in (agent.critic_updater, agent.actor_updater):
        assert updater.stock is False
        assert (updater.hidden == case.sizes[0]) == layered.plain(case), (updater.hidden, case.sizes)
    if layered.plain(case):
        # no weight images: the widths outside the fused kernels, and A = 65 on the fused width (A = 64 has them)
        assert lib.tonic_mlp_actor_image_bytes(case.O, case.sizes[0], case.A, heads) == 0
        if case.sizes == (64, 64):
            assert lib.tonic_mlp_actor_image_bytes(case.O, 64, 64, 1) > 0 and \
                lib.tonic_q_iteration_supported(case.O, 64, 64, 1) == 1 and \
                lib.tonic_q_iteration_supported(case.O, 64, case.A, heads) == 0
    out = layered.reference(model, case, inputs)
    if case.sizes == layered.WIDEST:
        out['float32'] = layered.float32_error(model, case, inputs, out)
    assert layered.violations(case, out) == [], layered.case_id(case)
    return agent, inputs, out


def _slots_and_padding(case, agent, out, used):
    """Slot 5 == B and every statistic slot outside `used` zero; the padding floats of both blocks zero."""
    m = agent.model
    for part, block, modules in (('critic', 'grads', [c for n, c in m.named_children()
                                                     if n.startswith('critic')]),
                                 ('actor', 'actor_grads', [m.actor])):
        if block not in out:
            continue
        stats = out[part + '_stats']
        zero = [i for i in range(8) if i != 5 and i not in used[part]]
        assert stats[5] == case.B and not stats[zero].any(), (part, stats)
        sums = torch.as_tensor(out[block])
        assert sums.numel() % len(modules) == 0
        each = sums.numel() // len(modules)
        for k, module in enumerate(modules):
            assert not _padding(module, sums[k * each:(k + 1) * each]).any(), (part, k)


@pytest.mark.parametrize('case', layered.Q_CASES, ids=_ids(layered.Q_CASES))
def test_q_layered_edges_vs_float64(lib, case):
    """SAC / TD3 / DDPG: tonic_twin_q_grad and tonic_actor_q_grad on the torso, batch and input axes and the mixed
    routes.  The (4095,) case's bound is bound_from_float32 of the float32 CPU autograd's own error (measured:
    4.8e-7 and 1.3e-6 of the largest element on two hosts, below 2.5e-6, so the project's 1e-5 stands;
    profiles/offpolicy_layered_edges_accuracy.md)."""
    agent, inputs, want = _prepare(lib, case)
    # (the updaters' hyperparameters are the ones the CPU search ran on)
    assert all(v == layered.Q_HYPER[k.replace('actor_', '')] for k, v in _q_hyper(agent, case.kind).items())
    bound = BOUND
    if case.sizes == layered.WIDEST:
        bound = layered.bound_from_float32(want['float32'])
        print(f'{layered.case_id(case)}: float32 CPU autograd {want["float32"]:.2e} of the largest element, '
              f'bound {bound:.2e}')
    assert bound == BOUND or case.sizes == layered.WIDEST
    eps = inputs['eps'] if case.kind != 'ddpg' else None
    out = _q_steps(agent, case.kind, inputs['batch'], eps, inputs['eps_actor'],
                   Ref(agent, case.kind, len(case.sizes), case.activation), bound=bound, restore=True)
    twin = case.kind != 'ddpg'
    _slots_and_padding(case, agent, out, dict(critic=(0, 1, 2) if twin else (0, 1), actor=(0,)))
    print(f'{layered.case_id(case)} seed {layered.seed_of(case)}: largest relative error critic {out["critic"]:.2e} '
          f'actor {out["actor"]:.2e}')


@pytest.mark.parametrize('case', layered.D4PG_CASES, ids=_ids(layered.D4PG_CASES))
def test_d4pg_layered_edges_vs_float64(lib, case):
    """D4PG: tonic_distributional_q_grad and tonic_distributional_actor_grad on (15, 17) ReLU and (33, 1, 33) ELU,
    atoms 2 / 17 / 64, A 6 / 17, B 1 / 37, the returns of the 'edges' generator."""
    agent, inputs, _ = _prepare(lib, case)
    values = agent.model.target_critic.head.values.double()
    batch = inputs['batch']
    ret = batch['rewards'].double()[:, None] + batch['discounts'].double()[:, None] * values[None]
    assert (ret[:, 0] < values[0]).any() or case.B == 1
    out = _d4pg_steps(agent, batch, Ref(agent, 'd4pg', len(case.sizes), case.activation), restore=True)
    _slots_and_padding(case, agent, out, dict(critic=(0,), actor=(0,)))
    print(f'{layered.case_id(case)} seed {layered.seed_of(case)}: largest relative error critic {out["critic"]:.2e} '
          f'actor {out["actor"]:.2e}')


@pytest.mark.parametrize('case', layered.SARSA_CASES, ids=_ids(layered.SARSA_CASES))
def test_expected_sarsa_layered_edges_vs_float64(lib, case):
    """MPO's critic: tonic_expected_sarsa_grad on (15, 17) ReLU and (17, 15) Tanh, A 1 / 17, S 3 / 70."""
    agent, inputs, _ = _prepare(lib, case)
    out = _sarsa_step(agent, inputs['batch'], inputs['eps'], Ref(agent, 'mpo', len(case.sizes), case.activation),
                      case.S)
    _slots_and_padding(case, agent, out, dict(critic=(0, 1)))
    print(f'{layered.case_id(case)} seed {layered.seed_of(case)}: largest relative error critic {out["critic"]:.2e}')


@pytest.mark.parametrize('case', layered.MPO_CASES, ids=_ids(layered.MPO_CASES))
def test_mpo_actor_layered_edges_vs_float64(lib, case):
    """MPO's actor: tonic_mpo_actor_grad on (15, 17) ReLU and (17, 15) Tanh, A 1 / 17, S 3 / 70, with and without
    penalization; the actor's tensors to 1e-5 (log T = 1), duals, statistics and floored duals as _mpo_compare holds
    them."""
    agent, inputs, _ = _prepare(lib, case, action_penalization=case.penalization, min_log_dual=layered.MPO_FLOOR)
    u = agent.actor_updater
    assert {k: getattr(u, k) for k in layered.MPO_HYPER} == layered.MPO_HYPER
    obs, eps, duals = inputs['batch']['observations'], inputs['eps'], inputs['duals']
    got = _mpo_call(lib, agent, u, duals, obs, eps)
    ref = Ref(agent, 'mpo', len(case.sizes), case.activation)
    err, dual_err, stat_err = _mpo_compare(agent, u, got, duals, obs, eps, ref, layered.case_id(case), bound=BOUND)
    out = dict(actor_grads=got[0][:u.count], actor_stats=got[0][u.count:])
    _slots_and_padding(case, agent, out, dict(actor=(0,)))
    print(f'{layered.case_id(case)} seed {layered.seed_of(case)}: largest relative error actor {err:.2e} '
          f'duals {dual_err:.2e} stats {stat_err:.2e}')
