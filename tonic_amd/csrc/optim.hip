// The flat fused optimizer step (one kernel template: optimizer_kernel) + PPO statistic finalisation (gfx950).
//
// Restates the single-tensor CPU paths of torch.optim.Adam / AdamW (torch/optim/adam.py:395-547), SGD
// (sgd.py:343-380) and RMSprop (rmsprop.py:287-339), applied to ONE flat buffer per network.  Plain Adam (betas
// (0.9, 0.999), eps 1e-8, no weight decay / amsgrad, as constructed by tonic/torch/updaters/actors.py:58-59 and
// critics.py:9-10) is the AdamRule<false> instantiation: 28 B/param of HBM traffic (read p,g,m,v, write p,m,v).
// WHICH float32 expression Adam is, operation by operation, is oracle/numpy_port.py's adam_statement (the
// statements themselves: optim_rule.h); tests/test_gpu_optim.py holds the kernel to it bit for bit.  It is NOT
// bit-identical with torch's CPU Adam, and nothing unfused can be: torch's lerp_ fuses from the second step on, and
// its addcmul_ forms (w2 * g) * g where adam_element forms w2 * (g * g) — one ulp of exp_avg_sq in a third of the
// elements, at most one ulp of a parameter after 7 steps.  The other rules, operation by operation, are tests/optim_family_ref.py;
// tests/test_gpu_optim_family.py holds the kernels to it bit for bit.  The file also holds the tail of
// ClippedRatio.__call__ (actors.py:101-112: loss/kl/entropy/clip_fraction/std/stop) and of
// VRegression.__call__ (critics.py:28).  The optimizer step counter and the PPO early-stop
// flag live on the device so the 80-iteration loop of ppo.py:33-46 needs no host sync.
// scheduled_optimizer_kernel is the same step at the rate of a learning-rate schedule (lr_schedule.h), formed from
// the device's step counter.
// Bytes of HBM traffic per parameter (p and g read, p written = 12, + 8 per state buffer): Adam / AdamW 28, with
// amsgrad 36; SGD 12, with momentum 20; RMSprop 20, + 8 centered, + 8 with momentum.
#include "common.h"
#include "optim_rule.h"
#include "lr_schedule.h"

namespace tonic {

struct OptimArgs {
  float* params;
  const float* grad_sums;
  float* slot[3];            // the rule's state buffers (tonic_optimizer_state_slots' order; Adam: exp_avg, exp_avg_sq)
  int32_t* state;            // {step_count, stop_flag, -, arrivals}
  int64_t n;
  float grad_scale, lr, beta2, eps;
  double beta1_d, beta2_d, lr_d;
  int stats_kind;            // 0 none, 1 PPO actor, 2 V critic, 3 twin Q critics, 4 Q actor
  float kl_threshold, entropy_coeff;
  const float* adv_stats;
  float* info_row;
  const int32_t* skip;
  // optional target-network update in the same launch: `params` is the block
  // [polyak_offset, polyak_offset + n) of the online buffer `polyak_online`
  float* polyak_target;
  const float* polyak_online;
  int64_t polyak_total, polyak_offset;
  float polyak_keep, polyak_mix;
  int adam_blocks;
  int decoupled, nesterov, maximize;
  float weight_decay;         // 0: no `g += wd * p` (adam.py:429, sgd.py:356, rmsprop.py:308)
  float decay_keep;           // AdamW: F32(1 - lr * wd) (adam.py:419)
  float momentum, undamped;   // SGD / RMSprop: mu; SGD: F32(1 - dampening)
  float alpha, unalpha;       // RMSprop: alpha, F32(1 - alpha)
};

// Up to two independent optimizer steps in one launch (blockIdx.y): PPO steps its actor and its
// critic together.
struct OptimPair { OptimArgs net[2]; };

// One thread: bump the step counter, turn the statistic sums into the logged values.
__device__ void adam_finalize(const OptimArgs& a) {
  const float* st = a.grad_sums + a.n;
  const bool all_zero = a.stats_kind == 1 && a.adv_stats != nullptr && a.adv_stats[2] != 0.f;
  if (!all_zero) a.state[0] += 1;
  if (a.info_row == nullptr) return;
  if (a.stats_kind == 1) {
    const float entropy = st[3] * a.grad_scale, std = st[4] * a.grad_scale;
    float loss = st[0] * a.grad_scale, kl = st[1] * a.grad_scale;
    float clip_fraction = st[2] * a.grad_scale;
    if (a.entropy_coeff != 0.f) loss -= a.entropy_coeff * entropy;   // actors.py:92-93
    if (all_zero) { loss = 0.f; kl = 0.f; clip_fraction = 0.f; }
    const bool stop = kl > a.kl_threshold;                           // actors.py:112
    a.info_row[0] = loss;
    a.info_row[1] = kl;
    a.info_row[2] = entropy;
    a.info_row[3] = clip_fraction;
    a.info_row[4] = std;
    a.info_row[5] = stop ? 1.f : 0.f;
    a.info_row[6] = 1.f;
    a.info_row[7] = 0.f;
    if (stop) a.state[1] = 1;
  } else if (a.stats_kind == 2) {
    stats_row_v(st, a.grad_scale, a.info_row);
  } else if (a.stats_kind == 3) {
    stats_row_twin_q(st, a.grad_scale, a.info_row);
  } else if (a.stats_kind == 4) {
    stats_row_q_actor(st, a.grad_scale, a.info_row);
  }
}

// The LAST optimizer workgroup to get here finalises (step counter, logged statistics, KL stop
// flag) — it used to be a launch of its own (4.6 us for an 8-float row).  Every workgroup has
// read state[0] / the skip flag before it arrives, so the writes below race with nobody: the
// barrier in front of the arrival is a workgroup-scope fence (s_waitcnt vmcnt(0) in every wave:
// all of this workgroup's loads have returned and its stores are acknowledged by L2) and the
// counter is an agent-scope atomic performed at L2; what the finaliser READS was written by
// earlier launches.  (A release / acquire pair at agent scope instead would be an L2 write-back
// + invalidate per workgroup.)
__device__ __forceinline__ void last_arrival_finalizes(const OptimArgs& a, int64_t grid) {
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned* arrivals = reinterpret_cast<unsigned*>(a.state + 3);
    const unsigned before = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
    if (before == (unsigned)grid - 1) {
      __hip_atomic_store(arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      adam_finalize(a);
    }
  }
}

// The rules as types: what is known at compile time decides which state buffers an instantiation streams.  Every
// rule LOADS all of its state before it stores any of it: the buffers may alias as far as the compiler knows, so a
// load behind a store waits for it, and each thread walks ~n / 32 768 elements one after the other.  With one
// round trip per element instead of one per buffer, at n = 4 194 304: SGD with momentum 75.0 -> 49.7 us, centered
// RMSprop with momentum 114.9 -> 66.3 us (profiles/optim_family_timing.json).
template <bool kAmsgrad>
struct AdamRule {
  AdamConsts c;
  __device__ void prepare(const OptimArgs& a) { c = adam_step_consts(nullptr, a); }
  __device__ float apply(const OptimArgs& a, int64_t i, float p, float g) const {
    float m = a.slot[0][i], v = a.slot[1][i];
    float seen = kAmsgrad ? a.slot[2][i] : 0.f;
    if (a.decoupled) p = p * a.decay_keep;                           // AdamW: param.mul_(1 - lr * wd), adam.py:419
    p = adam_element(g, p, m, v, kAmsgrad ? &seen : nullptr, a.beta2, a.eps, c);
    a.slot[0][i] = m;
    a.slot[1][i] = v;
    if (kAmsgrad) a.slot[2][i] = seen;
    return p;
  }
};

template <bool kMomentum>
struct SgdRule {
  bool first;
  __device__ void prepare(const OptimArgs& a) { first = a.state[0] == 0; }        // no step taken yet
  __device__ float apply(const OptimArgs& a, int64_t i, float p, float g) const {
    float d = g;
    if (kMomentum) {
      const float kept = a.slot[0][i] * a.momentum + a.undamped * g; // mul_().add_(alpha = 1 - dampening), sgd.py:365
      const float buf = first ? g : kept;                            // buf = grad.clone(), :361-363 (a select: what
      a.slot[0][i] = buf;                                            //  the buffer held before the first step is unused)
      d = a.nesterov ? g + a.momentum * buf : buf;                   // :367-370
    }
    return p - a.lr * d;                                             // param.add_(grad, alpha = -lr), :380
  }
};

template <bool kCentered, bool kMomentum>
struct RmspropRule {
  __device__ void prepare(const OptimArgs&) {}
  __device__ float apply(const OptimArgs& a, int64_t i, float p, float g) const {
    float* const momentum_slot = a.slot[kCentered ? 2 : 1];
    float sq = a.slot[0][i];
    float ga = kCentered ? a.slot[1][i] : 0.f;
    const float held = kMomentum ? momentum_slot[i] : 0.f;
    sq = sq * a.alpha + a.unalpha * (g * g);                         // mul_().addcmul_(), rmsprop.py:316
    float avg;
    if (kCentered) {
      ga = ga + a.unalpha * (g - ga);                                // lerp_, :322
      avg = sqrtf(sq - ga * ga) + a.eps;                             // addcmul(value = -1).sqrt_(), add_(eps), :323-330
    } else {
      avg = sqrtf(sq) + a.eps;                                       // :325-330
    }
    a.slot[0][i] = sq;
    if (kCentered) a.slot[1][i] = ga;
    if (kMomentum) {
      const float buf = held * a.momentum + g / avg;                 // mul_().addcdiv_(), :336
      momentum_slot[i] = buf;
      return p - a.lr * buf;                                         // :337
    }
    return p - a.lr * (g / avg);                                     // addcdiv_(value = -lr), :339
  }
};

template <typename Rule>
__global__ __launch_bounds__(256) void optimizer_kernel(OptimPair pair) {
  const OptimArgs& a = blockIdx.y == 0 ? pair.net[0] : pair.net[1];
  if (a.polyak_target != nullptr && (int)blockIdx.x >= a.adam_blocks) {
    // the target entries OUTSIDE this optimizer block: their online values are final already
    const int64_t first = (int64_t)((int)blockIdx.x - a.adam_blocks) * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)((int)gridDim.x - a.adam_blocks) * blockDim.x;
    for (int64_t i = first; i < a.polyak_total; i += stride) {
      if (i >= a.polyak_offset && i < a.polyak_offset + a.n) continue;
      a.polyak_target[i] = polyak(a.polyak_target[i], a.polyak_online[i], a.polyak_keep, a.polyak_mix);
    }
    return;
  }
  if (a.skip != nullptr && *a.skip != 0) return;
  // (pairs: the shorter network's spare workgroups walk nothing and arrive like the others)
  const int64_t grid = a.polyak_target != nullptr ? a.adam_blocks : (int64_t)gridDim.x;
  const bool all_zero = a.stats_kind == 1 && a.adv_stats != nullptr && a.adv_stats[2] != 0.f;  // actors.py:71
  if (!all_zero) {
    Rule rule;
    rule.prepare(a);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += grid * blockDim.x) {
      const float before = a.params[i];
      float g = a.grad_sums[i] * a.grad_scale;
      if (a.maximize) g = -g;                                        // adam.py:397, sgd.py:344, rmsprop.py:302
      if (a.weight_decay != 0.f && !a.decoupled) g = g + a.weight_decay * before;   // grad.add(param, alpha = wd)
      const float p = rule.apply(a, i, before, g);
      a.params[i] = p;
      if (a.polyak_target != nullptr) {                               // this entry's target, same thread
        float* t = a.polyak_target + a.polyak_offset + i;
        *t = polyak(*t, p, a.polyak_keep, a.polyak_mix);
      }
    }
  }
  last_arrival_finalizes(a, grid);
}

// The schedule of one network beside its OptimArgs (lr_schedule.h): `active` 0 leaves the network's rate what
// optim_fill packed; `weight_decay`: AdamW's, in float64 as decay_keep is formed from it.
struct LrScheduleArg { tonic_lr_schedule_t schedule; double weight_decay; int32_t active, reserved; };
struct LrSchedulePair { LrScheduleArg net[2]; };

// The same step at the rate of a schedule.  The schedules travel beside the OptimPair, as an argument of kernels of
// their own (the convention of ValueRangeArg): optimizer_kernel above is not touched — sharing its body through a
// function changes its instantiations' code — so the walk is stated here a second time, behind a copy of the
// network's arguments that holds the rate of THIS step: lr_t from the device's own step count in float64, and what
// optim_fill rounds from lr rounded the same way.  Every workgroup reads state[0] before it arrives
// (last_arrival_finalizes), so the count is the one the launch began with in all of them.
template <typename Rule>
__global__ __launch_bounds__(256) void scheduled_optimizer_kernel(OptimPair pair, LrSchedulePair schedules) {
  const OptimArgs& packed = blockIdx.y == 0 ? pair.net[0] : pair.net[1];
  const LrScheduleArg& s = blockIdx.y == 0 ? schedules.net[0] : schedules.net[1];
  if (packed.polyak_target != nullptr && (int)blockIdx.x >= packed.adam_blocks) {
    const int64_t first = (int64_t)((int)blockIdx.x - packed.adam_blocks) * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)((int)gridDim.x - packed.adam_blocks) * blockDim.x;
    for (int64_t i = first; i < packed.polyak_total; i += stride) {
      if (i >= packed.polyak_offset && i < packed.polyak_offset + packed.n) continue;
      packed.polyak_target[i] = polyak(packed.polyak_target[i], packed.polyak_online[i], packed.polyak_keep,
                                       packed.polyak_mix);
    }
    return;
  }
  if (packed.skip != nullptr && *packed.skip != 0) return;
  const int64_t grid = packed.polyak_target != nullptr ? packed.adam_blocks : (int64_t)gridDim.x;
  const bool all_zero = packed.stats_kind == 1 && packed.adv_stats != nullptr && packed.adv_stats[2] != 0.f;
  if (!all_zero) {
    OptimArgs a = packed;
    if (s.active) {
      const double lr_t = lr_schedule_value(s.schedule, packed.lr_d, (int64_t)packed.state[0]);
      a.lr_d = lr_t;                                                 // Adam / AdamW: step_size = F32(lr_t / bias1)
      a.lr = (float)lr_t;                                            // SGD / RMSprop
      a.decay_keep = (float)(1.0 - lr_t * s.weight_decay);           // AdamW (adam.py:419)
    }
    Rule rule;
    rule.prepare(a);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += grid * blockDim.x) {
      const float before = a.params[i];
      float g = a.grad_sums[i] * a.grad_scale;
      if (a.maximize) g = -g;
      if (a.weight_decay != 0.f && !a.decoupled) g = g + a.weight_decay * before;
      const float p = rule.apply(a, i, before, g);
      a.params[i] = p;
      if (a.polyak_target != nullptr) {
        float* t = a.polyak_target + a.polyak_offset + i;
        *t = polyak(*t, p, a.polyak_keep, a.polyak_mix);
      }
    }
  }
  last_arrival_finalizes(packed, grid);
}

// ---- gradient-norm clipping: torch.nn.utils.clip_grad_norm_ on the flat gradient-sum block ----
// Norm and factor are formed in float64 and rounded once (torch: float32 throughout): within one
// float32 ulp of numpy_port.clip_grad_norm_f64, the scaled sums within two (tests/test_gpu_optim.py).
// Pass 1: fixed-order partial sums of squares (float64) of a contiguous slice per workgroup.
constexpr int kClipBlocks = 64;

__global__ __launch_bounds__(256) void clip_partials_kernel(const float* sums, int64_t n,
                                                            double* partials,
                                                            const int32_t* skip) {
  __shared__ double red[256];
  if (skip != nullptr && *skip != 0) return;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = blockIdx.x * per, hi = min(n, lo + per);
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const double g = (double)sums[i];
    acc += g * g;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// Pass 2: every workgroup folds the partials in index order (same bits everywhere) into ||g|| and
// the factor min(1, max_norm / (||g|| + 1e-6)), then scales its slice of the sums in place.
__global__ __launch_bounds__(256) void clip_scale_kernel(float* sums, int64_t n,
                                                         const double* partials, int blocks,
                                                         double grad_scale, float max_norm,
                                                         float* report, const int32_t* skip) {
  __shared__ float coef_shared;
  if (skip != nullptr && *skip != 0) return;
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int b = 0; b < blocks; ++b) total += partials[b];
    const double norm = sqrt(total) * grad_scale;                 // norm of the MEAN gradient
    // clip_grad.py: clip_coef, clamped to 1 — formed in float64 like the norm and rounded ONCE.  (From the
    // float32 norm with a float32 add and divide, as torch forms it, it was up to 1.2 ulps from the exact
    // factor: tests/test_gpu_optim.py holds norm and factor to one ulp of numpy_port.clip_grad_norm_f64.)
    const double c = (double)max_norm / (norm + 1e-6);
    coef_shared = (float)(c < 1.0 ? c : 1.0);
    if (blockIdx.x == 0 && report != nullptr) { report[0] = coef_shared; report[1] = (float)norm; }
  }
  __syncthreads();
  const float coef = coef_shared;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    sums[i] = sums[i] * coef;
}

__global__ __launch_bounds__(256) void polyak_kernel(float* target, const float* online,
                                                     int64_t n, float keep, float mix) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    target[i] = polyak(target[i], online[i], keep, mix);
}

}  // namespace tonic

using namespace tonic;

namespace {

// Few, fat workgroups: every optimizer workgroup ends with one agent-scope atomic on the same
// counter (the last arriver finalises), and those serialise at ~10 ns each — 760 of them cost more
// than the finalisation launch they replaced (11.8 vs 10.3 us at 200 k parameters).
int adam_blocks_for(int64_t param_count) {
  const int64_t blocks = (param_count + 255) / 256;
  return (int)(blocks > 128 ? 128 : blocks);
}

bool family_rule_valid(const tonic_optimizer_t* rule) {
  if (rule == nullptr || rule->kind < TONIC_OPT_ADAM || rule->kind > TONIC_OPT_RMSPROP) return false;
  const int32_t allowed = TONIC_OPT_MAXIMIZE |
      (rule->kind <= TONIC_OPT_ADAMW ? TONIC_OPT_AMSGRAD
                                     : rule->kind == TONIC_OPT_SGD ? TONIC_OPT_NESTEROV : TONIC_OPT_CENTERED);
  if (rule->flags & ~allowed) return false;
  // sgd.py:57-58: Nesterov momentum requires a momentum and zero dampening
  if ((rule->flags & TONIC_OPT_NESTEROV) && (rule->momentum <= 0.0 || rule->dampening != 0.0)) return false;
  return rule->lr >= 0.0 && rule->weight_decay >= 0.0 && rule->momentum >= 0.0;
}

int state_slots(const tonic_optimizer_t& rule) {
  switch (rule.kind) {
    case TONIC_OPT_SGD: return rule.momentum != 0.0 ? 1 : 0;
    case TONIC_OPT_RMSPROP:
      return 1 + ((rule.flags & TONIC_OPT_CENTERED) ? 1 : 0) + (rule.momentum > 0.0 ? 1 : 0);
    default: return (rule.flags & TONIC_OPT_AMSGRAD) ? 3 : 2;
  }
}

// What tonic_adam_step* take as four numbers: torch.optim.Adam without weight decay / amsgrad / maximize.
tonic_optimizer_t plain_adam(double lr, double beta1, double beta2, double eps) {
  tonic_optimizer_t rule{};
  rule.kind = TONIC_OPT_ADAM;
  rule.lr = lr; rule.beta1 = beta1; rule.beta2 = beta2; rule.eps = eps;
  return rule;
}

// The optional target-network update of a step: `d_params` is the block [offset, offset + n) of `online`.
struct PolyakTail {
  float* target;
  const float* online;
  int64_t total, offset;
  double coeff;
};

// Validates and fills ONE network's arguments (`what`: the entry, for the messages); -> `blocks`: the
// workgroups its launch needs, the polyak tail's included.
int optim_fill(OptimArgs& a, unsigned& blocks, const char* what, float* d_params, const float* d_grad_sums,
               float* const slot[3], int32_t* d_state, int64_t param_count, double grad_scale,
               const tonic_optimizer_t& rule, int32_t stats_kind, double kl_threshold, double entropy_coeff,
               const float* d_adv_stats, float* d_info_row, const int32_t* d_skip_flag,
               const PolyakTail& tail = PolyakTail{}) {
  const int slots = state_slots(rule);
  bool held = true;
  for (int k = 0; k < slots; ++k) held = held && slot[k] != nullptr;
  TONIC_REQUIRE(d_params && d_grad_sums && held && d_state && param_count > 0, TONIC_ERR_INVALID_ARGUMENT,
                "%s: bad argument", what);
  TONIC_REQUIRE(stats_kind >= 0 && stats_kind <= 4, TONIC_ERR_INVALID_ARGUMENT,
                "%s: stats_kind %d", what, stats_kind);
  a = OptimArgs{};
  a.params = d_params; a.grad_sums = d_grad_sums; a.state = d_state; a.n = param_count;
  for (int k = 0; k < slots; ++k) a.slot[k] = slot[k];
  // Hyper-parameters are Python floats in the reference: bias corrections and step size are
  // formed in float64 and only then rounded to float32 (adam.py:530-547).
  a.grad_scale = (float)grad_scale; a.lr = (float)rule.lr; a.beta2 = (float)rule.beta2; a.eps = (float)rule.eps;
  a.beta1_d = rule.beta1; a.beta2_d = rule.beta2; a.lr_d = rule.lr;
  a.stats_kind = stats_kind; a.kl_threshold = (float)kl_threshold;
  a.entropy_coeff = (float)entropy_coeff;
  a.adv_stats = d_adv_stats; a.info_row = d_info_row; a.skip = d_skip_flag;
  a.decoupled = rule.kind == TONIC_OPT_ADAMW && rule.weight_decay != 0.0;
  a.nesterov = (rule.flags & TONIC_OPT_NESTEROV) != 0;
  a.maximize = (rule.flags & TONIC_OPT_MAXIMIZE) != 0;
  a.weight_decay = (float)rule.weight_decay;
  a.decay_keep = (float)(1.0 - rule.lr * rule.weight_decay);
  a.momentum = (float)rule.momentum; a.undamped = (float)(1.0 - rule.dampening);
  a.alpha = (float)rule.alpha; a.unalpha = (float)(1.0 - rule.alpha);
  a.adam_blocks = adam_blocks_for(param_count);
  int64_t extra = 0;
  if (tail.target != nullptr) {
    TONIC_REQUIRE(tail.online && tail.offset >= 0 && tail.offset + param_count <= tail.total &&
                      d_params == tail.online + tail.offset,
                  TONIC_ERR_INVALID_ARGUMENT, "%s: block [%lld, +%lld) of %lld", what,
                  (long long)tail.offset, (long long)param_count, (long long)tail.total);
    a.polyak_target = tail.target; a.polyak_online = tail.online; a.polyak_total = tail.total;
    a.polyak_offset = tail.offset; a.polyak_keep = (float)(1.0 - tail.coeff); a.polyak_mix = (float)tail.coeff;
    extra = (tail.total - param_count + 255) / 256;
    if (extra > 2048) extra = 2048;
  }
  blocks = (unsigned)(a.adam_blocks + extra);
  return TONIC_OK;
}

// `schedules` null: the rule's own kernel; otherwise its scheduled instantiation.
template <typename Rule>
void launch_as(const OptimPair& pair, const LrSchedulePair* schedules, dim3 grid, hipStream_t st) {
  if (schedules == nullptr) hipLaunchKernelGGL(optimizer_kernel<Rule>, grid, dim3(256), 0, st, pair);
  else hipLaunchKernelGGL(scheduled_optimizer_kernel<Rule>, grid, dim3(256), 0, st, pair, *schedules);
}

int optim_launch(const tonic_optimizer_t& rule, const OptimPair& pair, dim3 grid, void* stream, const char* what,
                 const LrSchedulePair* schedules = nullptr) {
  hipStream_t st = as_stream(stream);
  const bool momentum = rule.momentum != 0.0, centered = (rule.flags & TONIC_OPT_CENTERED) != 0;
  if (rule.kind == TONIC_OPT_SGD) {
    if (momentum) launch_as<SgdRule<true>>(pair, schedules, grid, st);
    else launch_as<SgdRule<false>>(pair, schedules, grid, st);
  } else if (rule.kind == TONIC_OPT_RMSPROP) {
    if (centered && momentum) launch_as<RmspropRule<true, true>>(pair, schedules, grid, st);
    else if (centered) launch_as<RmspropRule<true, false>>(pair, schedules, grid, st);
    else if (momentum) launch_as<RmspropRule<false, true>>(pair, schedules, grid, st);
    else launch_as<RmspropRule<false, false>>(pair, schedules, grid, st);
  } else if (rule.flags & TONIC_OPT_AMSGRAD) {
    launch_as<AdamRule<true>>(pair, schedules, grid, st);
  } else {
    launch_as<AdamRule<false>>(pair, schedules, grid, st);
  }
  TONIC_CHECK_LAUNCH(what);
  return TONIC_OK;
}

bool finite_in(double v, double low, double high) { return v == v && v >= low && v <= high; }

// What the header says tonic_lr_schedule_check rejects, one segment (`which`: for the messages).
int lr_segment_check(const tonic_lr_segment_t& s, int which) {
  TONIC_REQUIRE(s.kind >= TONIC_LR_CONSTANT && s.kind <= TONIC_LR_COSINE, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_lr_schedule_t: segment[%d].kind %d is not a TONIC_LR_* kind", which, s.kind);
  TONIC_REQUIRE(s.reserved == 0, TONIC_ERR_INVALID_ARGUMENT, "tonic_lr_schedule_t: segment[%d].reserved %d", which,
                s.reserved);
  const double huge = 1.7976931348623157e308;
  TONIC_REQUIRE(finite_in(s.a, -huge, huge) && finite_in(s.b, -huge, huge), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_lr_schedule_t: segment[%d] a %g, b %g: not finite", which, s.a, s.b);
  const bool reads_period = s.kind != TONIC_LR_EXPONENTIAL, reads_b = s.kind == TONIC_LR_LINEAR;
  TONIC_REQUIRE((reads_period || s.period == 0) && (reads_b || s.b == 0.0), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_lr_schedule_t: segment[%d] of kind %d: period %lld / b %g is not read and must be zero", which,
                s.kind, (long long)s.period, s.b);
  TONIC_REQUIRE(!reads_period || s.period >= (s.kind == TONIC_LR_CONSTANT ? 0 : 1), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_lr_schedule_t: segment[%d].period %lld (total_iters / step_size / T_max)", which,
                (long long)s.period);
  switch (s.kind) {
    case TONIC_LR_CONSTANT:
      TONIC_REQUIRE(finite_in(s.a, 0.0, 1.0), TONIC_ERR_INVALID_ARGUMENT,
                    "tonic_lr_schedule_t: segment[%d].a %g: ConstantLR's factor lies in [0, 1]", which, s.a);
      break;
    case TONIC_LR_LINEAR:
      TONIC_REQUIRE(s.a > 0.0 && s.a <= 1.0 && finite_in(s.b, 0.0, 1.0), TONIC_ERR_INVALID_ARGUMENT,
                    "tonic_lr_schedule_t: segment[%d] a %g, b %g: LinearLR's start_factor lies in (0, 1], its "
                    "end_factor in [0, 1]", which, s.a, s.b);
      break;
    default:
      TONIC_REQUIRE(s.a >= 0.0, TONIC_ERR_INVALID_ARGUMENT,
                    "tonic_lr_schedule_t: segment[%d].a %g (gamma / power / eta_min) is negative", which, s.a);
  }
  return TONIC_OK;
}

// One network's schedule beside its OptimArgs; null: inactive.
int lr_schedule_fill(LrScheduleArg& s, const tonic_lr_schedule_t* schedule, const tonic_optimizer_t& rule) {
  s = LrScheduleArg{};
  if (schedule == nullptr) return TONIC_OK;
  if (int rc = tonic_lr_schedule_check(schedule)) return rc;
  s.schedule = *schedule;
  s.weight_decay = rule.weight_decay;
  s.active = 1;
  return TONIC_OK;
}

// One network's step: fill, launch.
int optim_step(const char* what, float* d_params, const float* d_grad_sums, float* const slot[3],
               int32_t* d_state, int64_t param_count, double grad_scale, const tonic_optimizer_t& rule,
               int32_t stats_kind, double kl_threshold, double entropy_coeff, const float* d_adv_stats,
               float* d_info_row, const int32_t* d_skip_flag, const PolyakTail& tail, void* stream) {
  OptimPair pair{};
  unsigned blocks = 0;
  if (int rc = optim_fill(pair.net[0], blocks, what, d_params, d_grad_sums, slot, d_state, param_count,
                          grad_scale, rule, stats_kind, kl_threshold, entropy_coeff, d_adv_stats, d_info_row,
                          d_skip_flag, tail))
    return rc;
  return optim_launch(rule, pair, dim3(blocks), stream, what);
}

}  // namespace

extern "C" int32_t tonic_optimizer_state_slots(const tonic_optimizer_t* rule) {
  return family_rule_valid(rule) ? state_slots(*rule) : -1;
}

extern "C" int tonic_optimizer_step(float* d_params, const float* d_grad_sums, float* d_slots,
                                    int32_t* d_state, int64_t param_count, double grad_scale,
                                    const tonic_optimizer_t* rule, int32_t stats_kind,
                                    double kl_threshold, double entropy_coeff, const float* d_adv_stats,
                                    float* d_info_row, const int32_t* d_skip_flag, float* d_target,
                                    const float* d_online, int64_t total_count, int64_t block_offset,
                                    double coeff, void* stream) {
  const int slots = tonic_optimizer_state_slots(rule);
  TONIC_REQUIRE(slots >= 0, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_optimizer_step: not a rule of the family (kind %d, flags %d)",
                rule ? rule->kind : -1, rule ? rule->flags : -1);
  float* slot[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < slots && d_slots != nullptr; ++k) slot[k] = d_slots + (int64_t)k * param_count;
  return optim_step("tonic_optimizer_step", d_params, d_grad_sums, slot, d_state, param_count, grad_scale, *rule,
                    stats_kind, kl_threshold, entropy_coeff, d_adv_stats, d_info_row, d_skip_flag,
                    PolyakTail{d_target, d_online, total_count, block_offset, coeff}, stream);
}

extern "C" int tonic_lr_schedule_check(const tonic_lr_schedule_t* s) {
  if (s == nullptr) return TONIC_OK;
  TONIC_REQUIRE(s->count == 1 || s->count == 2, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_lr_schedule_t: count %d (one segment, or two around a milestone)", s->count);
  TONIC_REQUIRE(s->reserved == 0, TONIC_ERR_INVALID_ARGUMENT, "tonic_lr_schedule_t: reserved %d", s->reserved);
  TONIC_REQUIRE(s->count == 2 ? s->milestone >= 1 : s->milestone == 0, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_lr_schedule_t: milestone %lld with %d segment(s)", (long long)s->milestone, s->count);
  if (int rc = lr_segment_check(s->segment[0], 0)) return rc;
  if (s->count == 2) return lr_segment_check(s->segment[1], 1);
  const tonic_lr_segment_t& spare = s->segment[1];
  TONIC_REQUIRE(spare.kind == 0 && spare.reserved == 0 && spare.period == 0 && spare.a == 0.0 && spare.b == 0.0,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_lr_schedule_t: segment[1] is not zero with count 1");
  return TONIC_OK;
}

extern "C" double tonic_lr_schedule_value(const tonic_lr_schedule_t* schedule, double base_lr, int64_t step) {
  if (schedule == nullptr) return base_lr;
  if (tonic_lr_schedule_check(schedule) != TONIC_OK) return (double)NAN;
  if (step < 0) {
    set_error("tonic_lr_schedule_value: step %lld", (long long)step);
    return (double)NAN;
  }
  return lr_schedule_value(*schedule, base_lr, step);
}

extern "C" int tonic_scheduled_optimizer_step(float* d_params, const float* d_grad_sums, float* d_slots,
                                              int32_t* d_state, int64_t param_count, double grad_scale,
                                              const tonic_optimizer_t* rule, int32_t stats_kind,
                                              double kl_threshold, double entropy_coeff, const float* d_adv_stats,
                                              float* d_info_row, const int32_t* d_skip_flag, float* d_target,
                                              const float* d_online, int64_t total_count, int64_t block_offset,
                                              double coeff, const tonic_lr_schedule_t* schedule, void* stream) {
  if (schedule == nullptr)
    return tonic_optimizer_step(d_params, d_grad_sums, d_slots, d_state, param_count, grad_scale, rule, stats_kind,
                                kl_threshold, entropy_coeff, d_adv_stats, d_info_row, d_skip_flag, d_target,
                                d_online, total_count, block_offset, coeff, stream);
  const char* what = "tonic_scheduled_optimizer_step";
  const int slots = tonic_optimizer_state_slots(rule);
  TONIC_REQUIRE(slots >= 0, TONIC_ERR_INVALID_ARGUMENT, "%s: not a rule of the family (kind %d, flags %d)", what,
                rule ? rule->kind : -1, rule ? rule->flags : -1);
  LrSchedulePair schedules{};
  if (int rc = lr_schedule_fill(schedules.net[0], schedule, *rule)) return rc;
  float* slot[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < slots && d_slots != nullptr; ++k) slot[k] = d_slots + (int64_t)k * param_count;
  OptimPair pair{};
  unsigned blocks = 0;
  if (int rc = optim_fill(pair.net[0], blocks, what, d_params, d_grad_sums, slot, d_state, param_count, grad_scale,
                          *rule, stats_kind, kl_threshold, entropy_coeff, d_adv_stats, d_info_row, d_skip_flag,
                          PolyakTail{d_target, d_online, total_count, block_offset, coeff}))
    return rc;
  return optim_launch(*rule, pair, dim3(blocks), stream, what, &schedules);
}

extern "C" int tonic_scheduled_adam_step_pair(
    float* d_params_a, const float* d_grad_sums_a, float* d_exp_avg_a, float* d_exp_avg_sq_a,
    int32_t* d_state_a, int64_t param_count_a, double lr_a, int32_t stats_kind_a,
    double kl_threshold, double entropy_coeff, const float* d_adv_stats, float* d_info_row_a,
    const int32_t* d_skip_flag_a,
    float* d_params_b, const float* d_grad_sums_b, float* d_exp_avg_b, float* d_exp_avg_sq_b,
    int32_t* d_state_b, int64_t param_count_b, double lr_b, int32_t stats_kind_b,
    float* d_info_row_b,
    double grad_scale, double beta1, double beta2, double eps, const tonic_lr_schedule_t* schedule_a,
    const tonic_lr_schedule_t* schedule_b, void* stream) {
  if (schedule_a == nullptr && schedule_b == nullptr)
    return tonic_adam_step_pair(d_params_a, d_grad_sums_a, d_exp_avg_a, d_exp_avg_sq_a, d_state_a, param_count_a,
                                lr_a, stats_kind_a, kl_threshold, entropy_coeff, d_adv_stats, d_info_row_a,
                                d_skip_flag_a, d_params_b, d_grad_sums_b, d_exp_avg_b, d_exp_avg_sq_b, d_state_b,
                                param_count_b, lr_b, stats_kind_b, d_info_row_b, grad_scale, beta1, beta2, eps,
                                stream);
  OptimPair pair{};
  LrSchedulePair schedules{};
  unsigned blocks_a = 0, blocks_b = 0;
  float* const slot_a[3] = {d_exp_avg_a, d_exp_avg_sq_a, nullptr};
  float* const slot_b[3] = {d_exp_avg_b, d_exp_avg_sq_b, nullptr};
  const tonic_optimizer_t rule_a = plain_adam(lr_a, beta1, beta2, eps), rule_b = plain_adam(lr_b, beta1, beta2, eps);
  if (int rc = lr_schedule_fill(schedules.net[0], schedule_a, rule_a)) return rc;
  if (int rc = lr_schedule_fill(schedules.net[1], schedule_b, rule_b)) return rc;
  if (int rc = optim_fill(pair.net[0], blocks_a, "tonic_scheduled_adam_step_pair (first)", d_params_a,
                          d_grad_sums_a, slot_a, d_state_a, param_count_a, grad_scale, rule_a, stats_kind_a,
                          kl_threshold, entropy_coeff, d_adv_stats, d_info_row_a, d_skip_flag_a))
    return rc;
  if (int rc = optim_fill(pair.net[1], blocks_b, "tonic_scheduled_adam_step_pair (second)", d_params_b,
                          d_grad_sums_b, slot_b, d_state_b, param_count_b, grad_scale, rule_b, stats_kind_b, 0.0,
                          0.0, nullptr, d_info_row_b, nullptr))
    return rc;
  return optim_launch(rule_a, pair, dim3(blocks_a > blocks_b ? blocks_a : blocks_b, 2), stream,
                      "tonic_scheduled_adam_step_pair", &schedules);
}

extern "C" int tonic_adam_step_pair(
    float* d_params_a, const float* d_grad_sums_a, float* d_exp_avg_a, float* d_exp_avg_sq_a,
    int32_t* d_state_a, int64_t param_count_a, double lr_a, int32_t stats_kind_a,
    double kl_threshold, double entropy_coeff, const float* d_adv_stats, float* d_info_row_a,
    const int32_t* d_skip_flag_a,
    float* d_params_b, const float* d_grad_sums_b, float* d_exp_avg_b, float* d_exp_avg_sq_b,
    int32_t* d_state_b, int64_t param_count_b, double lr_b, int32_t stats_kind_b,
    float* d_info_row_b,
    double grad_scale, double beta1, double beta2, double eps, void* stream) {
  OptimPair pair{};
  unsigned blocks_a = 0, blocks_b = 0;
  float* const slot_a[3] = {d_exp_avg_a, d_exp_avg_sq_a, nullptr};
  float* const slot_b[3] = {d_exp_avg_b, d_exp_avg_sq_b, nullptr};
  const tonic_optimizer_t rule_a = plain_adam(lr_a, beta1, beta2, eps);
  if (int rc = optim_fill(pair.net[0], blocks_a, "tonic_adam_step_pair (first)", d_params_a, d_grad_sums_a,
                          slot_a, d_state_a, param_count_a, grad_scale, rule_a, stats_kind_a, kl_threshold,
                          entropy_coeff, d_adv_stats, d_info_row_a, d_skip_flag_a))
    return rc;
  if (int rc = optim_fill(pair.net[1], blocks_b, "tonic_adam_step_pair (second)", d_params_b, d_grad_sums_b,
                          slot_b, d_state_b, param_count_b, grad_scale, plain_adam(lr_b, beta1, beta2, eps),
                          stats_kind_b, 0.0, 0.0, nullptr, d_info_row_b, nullptr))
    return rc;
  return optim_launch(rule_a, pair, dim3(blocks_a > blocks_b ? blocks_a : blocks_b, 2), stream,
                      "tonic_adam_step_pair");
}

extern "C" int tonic_adam_step(float* d_params, const float* d_grad_sums, float* d_exp_avg,
                               float* d_exp_avg_sq, int32_t* d_state, int64_t param_count,
                               double grad_scale, double lr, double beta1, double beta2,
                               double eps, int32_t stats_kind, double kl_threshold,
                               double entropy_coeff,
                               const float* d_adv_stats, float* d_info_row,
                               const int32_t* d_skip_flag, void* stream) {
  float* const slot[3] = {d_exp_avg, d_exp_avg_sq, nullptr};
  return optim_step("tonic_adam_step", d_params, d_grad_sums, slot, d_state, param_count, grad_scale,
                    plain_adam(lr, beta1, beta2, eps), stats_kind, kl_threshold, entropy_coeff, d_adv_stats,
                    d_info_row, d_skip_flag, PolyakTail{}, stream);
}

extern "C" int tonic_adam_polyak_step(float* d_online, const float* d_grad_sums, float* d_exp_avg,
                                      float* d_exp_avg_sq, int32_t* d_state, int64_t block_offset,
                                      int64_t param_count, int64_t total_count, double grad_scale,
                                      double lr, double beta1, double beta2, double eps,
                                      int32_t stats_kind, float* d_info_row, float* d_target,
                                      double coeff, void* stream) {
  TONIC_REQUIRE(d_online && d_target && block_offset >= 0 && param_count > 0 &&
                    block_offset + param_count <= total_count,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_adam_polyak_step: block [%lld, +%lld) of %lld",
                (long long)block_offset, (long long)param_count, (long long)total_count);
  float* const slot[3] = {d_exp_avg, d_exp_avg_sq, nullptr};
  return optim_step("tonic_adam_polyak_step", d_online + block_offset, d_grad_sums, slot, d_state, param_count,
                    grad_scale, plain_adam(lr, beta1, beta2, eps), stats_kind, 0.0, 0.0, nullptr, d_info_row,
                    nullptr, PolyakTail{d_target, d_online, total_count, block_offset, coeff}, stream);
}

extern "C" int64_t tonic_clip_workspace_bytes(int64_t n) {
  (void)n;
  return kClipBlocks * (int64_t)sizeof(double) + 16;
}

extern "C" int tonic_clip_grad_norm(float* d_grad_sums, int64_t n, double grad_scale,
                                    double max_norm, const int32_t* d_skip_flag,
                                    void* d_workspace, int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_grad_sums && d_workspace && n > 0 && max_norm > 0, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_clip_grad_norm: bad argument");
  TONIC_REQUIRE(workspace_bytes >= tonic_clip_workspace_bytes(n), TONIC_ERR_WORKSPACE,
                "tonic_clip_grad_norm: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)tonic_clip_workspace_bytes(n));
  int64_t blocks = (n + 1023) / 1024;
  if (blocks > kClipBlocks) blocks = kClipBlocks;
  double* partials = static_cast<double*>(d_workspace);
  float* report = reinterpret_cast<float*>(partials + kClipBlocks);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(clip_partials_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_grad_sums, n,
                     partials, d_skip_flag);
  int64_t scale_blocks = (n + 255) / 256;
  if (scale_blocks > 1024) scale_blocks = 1024;
  hipLaunchKernelGGL(clip_scale_kernel, dim3((unsigned)scale_blocks), dim3(256), 0, st,
                     d_grad_sums, n, partials, (int)blocks, grad_scale, (float)max_norm, report,
                     d_skip_flag);
  TONIC_CHECK_LAUNCH("tonic_clip_grad_norm");
  return TONIC_OK;
}

extern "C" int tonic_polyak_update(float* d_target, const float* d_online, int64_t n,
                                   double coeff, void* stream) {
  TONIC_REQUIRE(d_target && d_online && n > 0, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_polyak_update: bad argument");
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     d_target, d_online, n, (float)(1.0 - coeff), (float)coeff);
  TONIC_CHECK_LAUNCH("tonic_polyak_update");
  return TONIC_OK;
}
