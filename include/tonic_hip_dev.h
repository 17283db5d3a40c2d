/*
 * Developer entry points of libtonic_hip.so — NOT part of the drop-in boundary (include/tonic_hip.h).
 * They exist for the parity tests and the profiling scripts of this repository: a process-wide
 * tuning switch between kernel variants that compute the same thing, one stand-alone GEMM of the
 * small-batch building block (and the block's batched / grouped launches, for its own tests), and a cycle probe of the fused grad kernel.  Nothing in the product
 * path (the tonic_amd package itself, as opposed to tests, scripts and bench) may depend on the knobs being set.
 */
#ifndef TONIC_HIP_DEV_H
#define TONIC_HIP_DEV_H

#include <stdint.h>

#include "tonic_hip.h" /* tonic_critic_loss_t */

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning knobs (process-wide atomics: a setting takes effect for launches issued after the call;
 * call before sizing workspaces).  Keys:
 *   "grad_waves" = 4       waves per workgroup of the 32x32x2-tile fused grad kernel;
 *   "grad_variant" = 0 .. 3 | -1  fused grad kernel: 0 = 32x32x2 fp32 tiles, 1 wave/SIMD;
 *                          1 = 16x16x4 fp32 tiles, 2 waves/SIMD; 2 = 1 with the two 64x64
 *                          hidden-layer products of a tile computed on bf16x3 terms (each fp32
 *                          operand = hi + mid + lo bf16 exactly; six bf16 MFMAs per product, fp32
 *                          accumulation: fp32-equivalent results, 2.4x less MFMA time); 3 (default)
 *                          = 2 with the 64x64 weight-gradient product dW2 on bf16x3 terms as well;
 *                          -1 restores the default;
 *   "grad_skew" = 0..64    start delay of half of the waves of variant 1 (experiment, default 0);
 *   "chain_fault" = 1      the NEXT chained critic step loses its first workgroup (test hook);
 *   "q_chain" = 0 | 1      off-policy iteration as chained launches (1, default) or one launch per pass;
 *   "gae_stream" = 0..4    which bit-exact GAE kernel serves small W (developer probe);
 *   "range_blocks" = 0..256  workgroups of the reward-range reduction: at most this many (0, default: by n); same bits;
 *   "policy_tail" = 0 | 1  off-policy actors: sampling / target noise / dense copy in the tail of
 *                          the forward launch (1, default) or in their own launches (0); same bits. */
int tonic_set_tuning(const char* key, int32_t value);
int tonic_get_tuning(const char* key, int32_t* value);

/* Developer tool: per-phase cycle totals (s_memtime) of the 8 waves of workgroup 0 of the
 * 16x16x4 fused actor grad kernel; d_phase_cycles = uint64[8][12]. */
int tonic_debug_grad16_phases(const float* d_actor_params, const float* d_observations,
                              const float* d_actions, const float* d_advantages,
                              const float* d_adv_stats, const float* d_old_log_probs, int64_t n,
                              int32_t O, int32_t A, void* d_workspace, int64_t workspace_bytes,
                              uint64_t* d_phase_cycles, void* stream);

/* Developer tool: wall-clock stamps (10 ns ticks) of workgroup (0, 0) of the fused off-policy
 * forward at its phase boundaries {entry, loads issued, layer 1, epilogue + barrier, layer 2,
 * epilogue + barrier, heads / output, policy tail}; d_stamps = uint64[8 launches][16] (wall clock | shader cycles), filled in
 * rotation by the launches that follow, then uint64[8 launches][8] of the weight-gradient group
 * {entry, requests out, main loop, partials exchanged, folded, -, end}; null switches the probe off
 * (scripts/forward_stamps.py). */
int tonic_debug_forward_stamps(uint64_t* d_stamps);

/* Developer / test entry: one GEMM of the small-batch fp32 MFMA building block
 * (mode "NT" | "NN" | "TN"; act 0 none, 1 relu, 2 tanh; d_mask multiplies by (mask > 0)). */
int tonic_gemm_f32(const char* mode, const float* d_a, const float* d_b, float* d_c,
                   const float* d_bias, const float* d_mask, float* d_colsum, int32_t M,
                   int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, int32_t act,
                   int32_t accumulate, double alpha, void* stream);

/* Developer / test entry: the WHOLE building block — every field of a problem, the batch dimension and the
 * grouped launches (tests/test_gpu_gemm_block.py).  One problem is
 *   C[z] = [C[z] +] mask'(act(alpha * op(A[z]) op(B[z]) + bias[z])),   z = 0 .. batch - 1,
 * with operand X[z] = x + z * stride_x (floats; a stride of 0 shares the operand among the batch), row pitches
 * lda / ldb / ldc / ldmask (floats), act 0 none, 1 relu, 2 tanh, 3 elu; the mask holds act(z) of another layer and
 * multiplies by that activation's derivative, chosen by mask_act: 0 / 1 (mask > 0), 2 (1 - mask^2), 3 (mask > 0 ? 1 :
 * mask + 1).  bias, mask and colsum may be null; colsum[z][m] = sum_k A[z][k][m], mode "TN" only.
 * count == 1: the single launch; count = 2 .. 4: one grouped launch of problems that share mode and K; count = 5, 6:
 * the plain "TN" form only (no bias, mask or activation).  Everything else is refused with
 * TONIC_ERR_INVALID_ARGUMENT before any launch.  No optimizer epilogue, weight images or value range. */
typedef struct {
  const float *a, *b; float *c; const float *bias, *mask; float *colsum;
  int32_t M, N, K, lda, ldb, ldc, ldmask;
  int64_t stride_a, stride_b, stride_c, stride_bias, stride_mask, stride_colsum;
  int32_t act, mask_act, accumulate; float alpha;
} tonic_gemm_problem;
int tonic_gemm_group_f32(const char* mode, const tonic_gemm_problem* problems,
                         int32_t count, int32_t batch, void* stream);

/* Test tool: `workgroups` workgroups that each hold a compute unit to themselves (100 KB of LDS:
 * neither a collect nor a grad workgroup fits beside one) and spin for `milliseconds` of the
 * 100 MHz wall clock — a foreign kernel that occupies part of the chip, for the tests of what the
 * resident collect kernel does when not all of its workgroups find a compute unit. */
int tonic_debug_occupy(int32_t workgroups, double milliseconds, void* stream);

/* Test entry: the critic loss kernel of TQC alone (step 4 of tonic_ensemble_quantile_q_grad and, at N = 2 with
 * twin_row, of tonic_truncated_quantile_q_grad; include/tonic_hip.h) on given rows.  d_targets / d_thetas [N][B][ld]
 * (the target and the online critics' quantiles; M <= ld <= 32, columns past M ignored; 2 <= N <= 8, N M <= 256),
 * d_rewards / d_discounts / d_logp [B]; alpha = entropy_coeff, or expf(*d_log_entropy_coeff) when given.
 * Out: d_dlogits [N][B][ld] (the row losses' gradients, 0 on the columns past M) and d_sample_m [3][Bp] =
 * {loss_m, (1 / N) sum_z mean_i theta_zi, 0}, or with twin_row != 0 (N = 2 only: TONIC_ERR_INVALID_ARGUMENT
 * otherwise) the twin row {loss_m, q1, q2}, q_z = mean_i theta_zi. */
int tonic_debug_ensemble_quantile_loss(const float* d_targets, const float* d_thetas, int32_t ld,
                                       const float* d_rewards, const float* d_discounts, const float* d_logp,
                                       int32_t M, int32_t N, int32_t drop_per_net, double entropy_coeff,
                                       const float* d_log_entropy_coeff, float* d_dlogits, float* d_sample_m,
                                       int32_t B, int32_t Bp, int32_t twin_row, void* stream);

/* Test entry: the critic loss kernel of REDQ alone (step 4 of tonic_ensemble_subset_q_grad; include/tonic_hip.h) on
 * given rows.  d_targets / d_qs [N][Bp][ld] (the target and the online critics' values in column 0; 1 <= ld <= 32,
 * the columns behind it ignored; 2 <= N <= 8), d_rewards / d_discounts / d_logp [B]; d_subset: ONE int32 on the
 * device, bit z = target critic z in the minimum (bits at and above N ignored, none of the low N set: all N);
 * alpha = entropy_coeff, or expf(*d_log_entropy_coeff) when given; loss: the rule (NULL: MSE).
 * Out: d_dq [N][Bp][ld] (rows below B: column 0 the row losses' gradients, 0 behind it; rows from B on untouched) and
 * d_sample_m [3][Bp] = {loss_m, (1 / N) sum_z Q_z, 0}. */
int tonic_debug_ensemble_subset_loss(const float* d_targets, const float* d_qs, int32_t ld, const float* d_rewards,
                                     const float* d_discounts, const float* d_logp, int32_t N,
                                     const int32_t* d_subset, double entropy_coeff,
                                     const float* d_log_entropy_coeff, const tonic_critic_loss_t* loss, float* d_dq,
                                     float* d_sample_m, int32_t B, int32_t Bp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TONIC_HIP_DEV_H */
