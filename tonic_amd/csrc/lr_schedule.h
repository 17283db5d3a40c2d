// The learning rate of optimizer step t, written ONCE: tonic_lr_schedule_value (the host: the Adam table of the
// fused off-policy iteration, the logged rates) and the scheduled instantiations of optimizer_kernel (optim.hip)
// both call lr_schedule_value.  The expressions are torch.optim.lr_scheduler's `_get_closed_form_lr` of ConstantLR,
// LinearLR, ExponentialLR, StepLR, PolynomialLR and CosineAnnealingLR, operation by operation in float64 (Python
// floats), with t = the number of optimizer steps TAKEN so far (torch's `scheduler.step()` after each
// `optimizer.step()`: last_epoch).  -ffp-contract=off keeps every operation rounded on its own; pow and cos are the
// only operations whose last bits may differ between the host's and the device's library.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/tonic_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TONIC_LR_FN __host__ __device__ inline
#else
#define TONIC_LR_FN inline
#endif

namespace tonic {

// One segment at its own step count t >= 0 from the base rate `lr`.
TONIC_LR_FN double lr_segment_value(const tonic_lr_segment_t& s, double lr, int64_t t) {
  const double capped = (double)(t < s.period ? t : s.period);         // min(total_iters, last_epoch)
  switch (s.kind) {
    case TONIC_LR_CONSTANT:                                            // factor + (t >= total_iters) * (1 - factor)
      return lr * (s.a + (t >= s.period ? 1.0 : 0.0) * (1.0 - s.a));
    case TONIC_LR_LINEAR:                                              // start + (end - start) * min(..) / total_iters
      return lr * (s.a + (s.b - s.a) * capped / (double)s.period);
    case TONIC_LR_EXPONENTIAL:                                         // gamma ** t
      return lr * pow(s.a, (double)t);
    case TONIC_LR_STEP:                                                // gamma ** (t // step_size)
      return lr * pow(s.a, (double)(t / s.period));
    case TONIC_LR_POLYNOMIAL:                                          // (1.0 - min(..) / total_iters) ** power
      return lr * pow(1.0 - capped / (double)s.period, s.a);
    default: {                                                         // TONIC_LR_COSINE, periodic beyond T_max
      const double pi = 3.141592653589793;                             // math.pi
      return s.a + (lr - s.a) * (1.0 + cos(pi * (double)t / (double)s.period)) / 2.0;
    }
  }
}

// The rate of step t: one segment, or the first below the milestone and the second, counted from the milestone
// and from the same base rate, at and beyond it (SequentialLR of two).
TONIC_LR_FN double lr_schedule_value(const tonic_lr_schedule_t& s, double lr, int64_t t) {
  if (s.count == 2 && t >= s.milestone) return lr_segment_value(s.segment[1], lr, t - s.milestone);
  return lr_segment_value(s.segment[0], lr, t);
}

}  // namespace tonic
