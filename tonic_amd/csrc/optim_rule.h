// The optimizer step's device statements, written ONCE: optimizer_kernel (optim.hip) and the optimizer epilogue
// of the weight-gradient kernels (gemm16.hip) both call these.  WHICH float32 expression Adam is, operation by
// operation, is oracle/numpy_port.py's adam_statement; -ffp-contract=off keeps every operation rounded on its own.
#pragma once
#include "common.h"

namespace tonic {

// The step's constants: bias corrections and step size are formed in float64 like the reference's Python floats
// and only then rounded (adam.py:530-536).  `formed`: {step_size, bias2_sqrt} of THIS step as the host formed them
// the same way (no float64 pow on the device); null: formed here for step f.state[0] + 1.  Args: an argument struct
// with state, beta1_d, beta2_d, lr_d — by reference, its fields read where they are used: handing them over as
// values, or forming the null branch in a function of its own, changes the register allocation of the
// weight-gradient kernels (gemm16.hip) around it.
struct AdamConsts { float step_size, bias2_sqrt, w1, w2; };

template <typename Args>
__device__ __forceinline__ AdamConsts adam_step_consts(const float* formed, const Args& f) {
  if (formed != nullptr) {
    AdamConsts c;
    c.step_size = formed[0]; c.bias2_sqrt = formed[1];
    c.w1 = (float)(1.0 - f.beta1_d); c.w2 = (float)(1.0 - f.beta2_d);
    return c;
  }
  const int step = f.state[0] + 1;
  const double bias1 = 1.0 - pow(f.beta1_d, (double)step);
  const double bias2 = 1.0 - pow(f.beta2_d, (double)step);
  AdamConsts c;
  c.step_size = (float)(f.lr_d / bias1);                             // adam.py:534
  c.bias2_sqrt = (float)sqrt(bias2);                                 // :536
  c.w1 = (float)(1.0 - f.beta1_d); c.w2 = (float)(1.0 - f.beta2_d);
  return c;
}

// One element: gradient g -> new parameter, the moments updated in place.  `seen` (amsgrad: the running maximum
// of v, updated too) may be null.  One ulp of `v` away from torch's addcmul_ order, which forms (w2 * g) * g.
__device__ __forceinline__ float adam_element(float g, float p, float& m, float& v, float* seen, float beta2,
                                              float eps, const AdamConsts& c) {
  m = m + c.w1 * (g - m);                                            // lerp_, adam.py:457
  v = v * beta2 + c.w2 * (g * g);                                    // mul_().addcmul_(), :476
  float root = v;
  if (seen != nullptr) {
    root = (v > *seen || v != v) ? v : *seen;                        // torch.maximum (NaN propagates), :540
    *seen = root;
  }
  const float denom = sqrtf(root) / c.bias2_sqrt + eps;              // :543 / :545
  return p - c.step_size * (m / denom);                              // addcdiv_, :547
}

// t = t*(1-c) + c*o with three roundings (actor_critics.py:126-130); used by SAC / TD3 / DDPG.
__device__ __forceinline__ float polyak(float target, float online, float keep, float mix) {
  const float scaled = target * keep;
  const float add = mix * online;
  return scaled + add;
}

// The logged row of a step from the eight statistic sums behind its gradient block, by stats_kind: 2 V critic,
// 3 twin Q critics, 4 Q actor (1, the PPO actor's, needs the step's own state: adam_finalize in optim.hip).
__device__ __forceinline__ void stats_row_v(const float* st, float grad_scale, float* info_row) {
  info_row[0] = st[0] * grad_scale;            // MSE loss
  info_row[1] = st[1] * grad_scale;            // mean of the pre-step values ('v')
  info_row[6] = 1.f;
}

__device__ __forceinline__ void stats_row_twin_q(const float* st, float grad_scale, float* info_row) {
  info_row[0] = st[0] * grad_scale;            // loss_1 + loss_2 (critics.py:172,224)
  info_row[1] = st[1] * grad_scale;            // mean q1
  info_row[2] = st[2] * grad_scale;            // mean q2
  info_row[6] = 1.f;
}

__device__ __forceinline__ void stats_row_q_actor(const float* st, float grad_scale, float* info_row) {
  info_row[0] = st[0] * grad_scale;            // actor loss (actors.py:179,257)
  info_row[6] = 1.f;
}

}  // namespace tonic
