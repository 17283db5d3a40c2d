// Off-policy learner path (SAC / TD3 / DDPG / D4PG / MPO), gfx950.
//
// Restates (paths relative to the reference checkout):
//   tonic/torch/updaters/critics.py:31-53 (QRegression), :125-134 (TargetActionNoise), :156-182
//     (TwinCriticDeterministicQLearning), :202-235 (TwinCriticSoftQLearning),
//   tonic/torch/updaters/actors.py:170-189 (DeterministicPolicyGradient), :238-267
//     (TwinCriticSoftDeterministicPolicyGradient),
//   tonic/torch/models/actors.py:7-34 (SquashedMultivariateNormalDiag), :94-98
//     (GaussianPolicyHead.forward), :113-115 (DeterministicPolicyHead), critics.py:15-20,
//     encoders.py:28-31 (ObservationActionEncoder), normalizers/mean_stds.py:34-39,
//   tonic/replays/buffers.py:33-56 (store), :81-91 (get: rows = idx // W, cols = idx % W).
//
// Every dense layer is one gemm16 launch (gemm16.h) with bias / ReLU / ReLU-mask / bias-
// gradient fused in its epilogue; the twin critics run as batch-2 launches over a flat
// [critic_1 | critic_2] parameter block.  The glue (sampling, squashing, targets, loss
// gradients) is a handful of tiny element-wise kernels.  Gradients are written as SUMS over the
// batch straight into the flat gradient buffer (same layout as the parameters), so
// tonic_adam_step / an RCCL all-reduce consume them exactly like the PPO path.
#include "gemm16.h"
#include "mlpfwd.h"
#include "collector_q.h"
#include "bufstore.h"

#include <algorithm>
#include <mutex>

namespace tonic {

// Torso: MLP(sizes, activation) of tonic/torch/models/utils.py:4-23.  The fused kernels (mlpfwd.hip) hold the
// reference's shape — two ReLU layers of one width (H2 = 0 = "as H", act = ACT_RELU); every other torso (unequal
// widths: the (400, 300) class; Tanh; ELU; 1, 3 or 4 layers) runs layer by layer on gemm16 launches — `plain()`
// tells.  L: hidden layers (1 .. kTorsoMaxLayers), of H, h2(), H3, H4 units.
constexpr int kTorsoMaxLayers = 4;
struct ActorShape {                              // heads: 1 = deterministic (TD3), 2 = loc+scale (SAC)
  int O, H, A, heads; int H2 = 0; int act = ACT_RELU;
  int L = 2; int H3 = 0, H4 = 0;
  float scale_lo = kScaleMin, scale_hi = kScaleMax;     // heads == 2: the bounds of the Gaussian head's scale
  __host__ __device__ int h2() const { return H2 > 0 ? H2 : H; }
  __host__ __device__ int width(int l) const { return l == 0 ? H : l == 1 ? h2() : l == 2 ? H3 : H4; }
  __host__ __device__ int last() const { return width(L - 1); }              // the heads' input width
  __host__ __device__ int hp() const {                                        // pitch of every hidden array
    int w = 0;
    for (int l = 0; l < L; ++l) w = width(l) > w ? width(l) : w;
    return weight_ld(w);
  }
  bool plain() const { return L == 2 && h2() == H && act == ACT_RELU; }
};
struct CriticShape {
  int O, A, H; int H2 = 0; int act = ACT_RELU;
  int L = 2; int H3 = 0, H4 = 0;
  __host__ __device__ int h2() const { return H2 > 0 ? H2 : H; }
  __host__ __device__ int width(int l) const { return l == 0 ? H : l == 1 ? h2() : l == 2 ? H3 : H4; }
  __host__ __device__ int last() const { return width(L - 1); }
  __host__ __device__ int hp() const {
    int w = 0;
    for (int l = 0; l < L; ++l) w = width(l) > w ? width(l) : w;
    return weight_ld(w);
  }
  bool plain() const { return L == 2 && h2() == H && act == ACT_RELU; }
};

// The C ABI passes ONE int32 `H`: the width of a plain torso (any width: bit 30 clear), tonic_mlp_hidden(H1, H2,
// activation) = 1 << 30 | H1 | H2 << 12 | activation << 24 (two layers, widths below 4096; activation: GemmAct), or
// for 1, 3 or 4 layers a descriptor that tonic_mlp_torso registered: 1 << 30 | 1 << 29 | its index in a small
// process-wide table.  A descriptor also carries the bounds of the actor's Gaussian scale head; a torso of any depth
// with bounds other than the defaults is registered (tonic_mlp_torso_head), and a critic ignores them.  The codes are
// unpacked here, on the host; no kernel sees one.
constexpr int32_t kHiddenPacked = 1 << 30;
constexpr int32_t kTorsoRegistered = 1 << 29;
constexpr int kTorsoTableSize = 256;
struct Torso {                                          // L == 0: not a torso this library knows
  int L, width[kTorsoMaxLayers], act;
  float scale_lo = kScaleMin, scale_hi = kScaleMax;
};

struct TorsoTable {
  std::mutex lock;
  Torso entry[kTorsoTableSize];
  int count = 0;
};
TorsoTable& torso_table() {
  static TorsoTable table;
  return table;
}

inline Torso unpack_torso(int32_t code) {
  if ((code & kHiddenPacked) == 0) return Torso{2, {code, code, 0, 0}, ACT_RELU};
  if (code & kTorsoRegistered) {
    TorsoTable& t = torso_table();
    const int index = code & (kTorsoRegistered - 1);
    std::lock_guard<std::mutex> guard(t.lock);
    return index < t.count ? t.entry[index] : Torso{0, {0, 0, 0, 0}, 0};
  }
  Torso h{2, {code & 4095, (code >> 12) & 4095, 0, 0}, (code >> 24) & 7};
  if (h.width[1] == 0) h.width[1] = h.width[0];
  if (h.act == 0) h.act = ACT_RELU;
  return h;
}
inline ActorShape actor_shape(int O, int32_t code, int A, int heads) {
  const Torso t = unpack_torso(code);
  return ActorShape{O, t.width[0], A, heads, t.L >= 2 && t.width[1] != t.width[0] ? t.width[1] : 0, t.act, t.L,
                    t.width[2], t.width[3], t.scale_lo, t.scale_hi};
}
// The torso's own code: a registered two-layer descriptor (one that carries bounds) as the width or the packed code
// of its torso, so that whatever serves that torso — the fused kernels and weight images of the plain width among
// them — decides and sizes as it does there.  Every other code is its own.
inline int32_t torso_code(int32_t code) {
  if ((code & kHiddenPacked) == 0 || (code & kTorsoRegistered) == 0) return code;
  const Torso t = unpack_torso(code);
  if (t.L != 2) return code;
  return t.width[0] == t.width[1] && t.act == ACT_RELU ? t.width[0]
                                                       : kHiddenPacked | t.width[0] | (t.width[1] << 12) | (t.act << 24);
}
inline CriticShape critic_shape(int O, int A, int32_t code) {
  const Torso t = unpack_torso(code);
  return CriticShape{O, A, t.width[0], t.L >= 2 && t.width[1] != t.width[0] ? t.width[1] : 0, t.act, t.L,
                     t.width[2], t.width[3]};
}
inline int hidden_pitch(int32_t code) {
  const Torso t = unpack_torso(code);
  int w = 0;
  for (int l = 0; l < t.L; ++l) w = t.width[l] > w ? t.width[l] : w;
  return weight_ld(w);
}
inline bool hidden_plain(int32_t code) {
  const Torso t = unpack_torso(code);
  return t.L == 2 && t.width[0] == t.width[1] && t.act == ACT_RELU;
}
inline bool hidden_known(int32_t code) { return code > 0 && unpack_torso(code).L > 0; }
// Layers of hidden activations the workspaces hold per network and pass: two at least, so that the two-layer
// layouts (and every workspace size of a two-layer torso) stay what they are.
inline int hidden_layers(int32_t code) {
  const int L = unpack_torso(code).L;
  return L > 2 ? L : 2;
}

// Floats of one network in the padded layout (mlpfwd.h: weight_ld / slot4), layer by layer:
//   actor : W1 [H, O] b1 [H] W2 [H2, H] b2 [H2] ... then per head Wh [A, H_L] bh [A]
//   critic: W1 [H, O + A] b1 [H] W2 [H2, H] b2 [H2] ... w3 [1, H_L] b3 [1]
__host__ __device__ inline int64_t actor_count(ActorShape s) {
  int64_t n = 0;
  int in = s.O;
  for (int l = 0; l < s.L; ++l) {
    n += (int64_t)s.width(l) * weight_ld(in) + slot4(s.width(l));
    in = s.width(l);
  }
  return n + (int64_t)s.heads * ((int64_t)s.A * weight_ld(in) + slot4(s.A));
}
__host__ __device__ inline int64_t critic_count(CriticShape s) {
  int64_t n = 0;
  int in = s.O + s.A;
  for (int l = 0; l < s.L; ++l) {
    n += (int64_t)s.width(l) * weight_ld(in) + slot4(s.width(l));
    in = s.width(l);
  }
  return n + weight_ld(in) + slot4(1);
}

// Hidden activations of the layer-by-layer passes: the callers take a network's L layers as ONE region and pass
// its first two layers (h1, h2): layer l lies at h1 + l (h2 - h1).  The input-gradient chains run the other way
// and are passed (dh2, dh1) = (dz of the last layer, dz of the one below): dz of layer l lies at
// dh2 + (L - 1 - l) (dh1 - dh2).  For two layers these are the arrays the fused kernels take.
template <typename T>
inline T* layer_at(T* first, T* second, int l) { return first + (int64_t)l * (second - first); }

// ------------------------------------------------------------------ element-wise kernels

// X[m] = [ (obs[m] - mean) / std , actions[m] ]   (encoders.py:28-31 + mean_stds.py:36)
// blockIdx.y == 1 encodes a second (obs, act) pair into X2 in the same launch.
__global__ void encode_kernel(const float* obs, const float* act, const float* mean,
                              const float* std, float clip, float* X, int B, int O, int A, int ldx,
                              const float* obs2 = nullptr, const float* act2 = nullptr,
                              float* X2 = nullptr) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * (O + A)) return;
  if (blockIdx.y == 1) { obs = obs2; act = act2; X = X2; }
  const int m = idx / (O + A), c = idx - m * (O + A);
  X[(int64_t)m * ldx + c] =
      c < O ? __builtin_amdgcn_fmed3f((obs[(int64_t)m * O + c] - mean[c]) / std[c], -clip, clip)
            : act[(int64_t)m * A + (c - O)];
}

// SAC: u = loc + sigma * eps, a = tanh(u), logp = sum_a [N(u; loc, sigma) - log(1 - a^2 + 1e-6)]
// with sigma = clamp(softplus(spre), scale_lo, scale_hi) (actors.py:11-16,94-98).  A group of G = 2^k >= A
// lanes (G <= 32; wider heads loop) owns one sample and folds the log-probability terms with a
// fixed xor tree, so the dozen transcendental calls per action run in parallel, not in a loop.
__global__ void sac_sample_kernel(const float* loc, const float* spre, const float* eps, int ld,
                                  float* act, float* logp, float* sigma_out, int B, int A,
                                  int G, float scale_lo, float scale_hi) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = tid / G, lane_a = tid - m * G;
  const bool sample_ok = m < B;
  float lp = 0.f;
  for (int a = lane_a; a < A; a += G) {
    if (!sample_ok) break;
    const SquashedSample sm = squashed_sample(loc[(int64_t)m * ld + a], spre[(int64_t)m * ld + a],
                                              eps ? eps[(int64_t)m * A + a] : 0.f, eps != nullptr, scale_lo,
                                              scale_hi);
    lp += sm.logp_term;
    act[(int64_t)m * A + a] = sm.action;
    if (sigma_out) sigma_out[(int64_t)m * A + a] = sm.sigma;
  }
  for (int off = G >> 1; off >= 1; off >>= 1) lp += __shfl_xor(lp, off, 64);
  if (logp && sample_ok && lane_a == 0) logp[m] = lp;
}

// TD3 target actions: clamp(a + clamp(scale * eps, -clip, clip), -1, 1)  (critics.py:130-134)
__global__ void td3_target_action_kernel(const float* loc, int ld, const float* eps, float* act,
                                         int B, int A, float scale, float clip) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * A) return;
  const int m = idx / A, a = idx - m * A;
  act[idx] = noisy_target_action(loc[(int64_t)m * ld + a], eps[idx], scale, clip);
}

// dense actions out of a padded head buffer (deterministic policy: tanh already applied)
__global__ void copy_actions_kernel(const float* loc, int ld, float* act, int B, int A) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * A) return;
  act[idx] = loc[(int64_t)(idx / A) * ld + (idx % A)];
}

// y = r + disc * (min(q1', q2') - alpha * logp')  (critics.py:219-221; alpha = 0 and logp = null
// give TD3's critics.py:166-167), then dq_z = loss'(q_z - y) (critic_loss_dq, mlpfwd.h; MSE: 2 (q_z - y)) and the
// statistics.  nets == 1 (DDPG, critics.py:72-79): y = r + disc * q', one critic, statistics {loss_terms, q, 0}.
// (critic_loss_rows: the kernel's whole body, shared with the form that reads alpha from the device)
__device__ __forceinline__ void critic_loss_rows(const float* rewards, const float* discounts,
                                                 const float* tq, const float* logp_next, float alpha,
                                                 const float* q, float* dq, float* stats, int B, int Bp,
                                                 int nets, CriticLoss loss, const float* v_low, const float* v_high) {
  const ValueRange vrange = value_range(v_low, v_high);     // the Return normaliser's head: q / tq are squashed values
  float s_loss = 0.f, s_q1 = 0.f, s_q2 = 0.f;
  for (int m = threadIdx.x; m < B; m += blockDim.x) {
    const float y = td_target(rewards, discounts, tq, logp_next, alpha, m, ValueLines{Bp, 16}, nets);
    if (nets == 1) {
      const float e1 = q[m] - y;
      dq[m] = value_squash_dz(critic_loss_dq(e1, loss.kind, loss.param), q[m], vrange);
      s_loss += critic_loss_term(e1, loss.kind, loss.param);
      s_q1 += q[m];
      continue;
    }
    const float e1 = q[m] - y, e2 = q[Bp + m] - y;
    dq[m] = value_squash_dz(critic_loss_dq(e1, loss.kind, loss.param), q[m], vrange);
    dq[Bp + m] = value_squash_dz(critic_loss_dq(e2, loss.kind, loss.param), q[Bp + m], vrange);
    s_loss += critic_loss_term(e1, loss.kind, loss.param) + critic_loss_term(e2, loss.kind, loss.param);
    s_q1 += q[m];
    s_q2 += q[Bp + m];
  }
  double a = s_loss, b = s_q1, c = s_q2;
  block_sum3(a, b, c);
  if (threadIdx.x == 0) {
    stats[0] = (float)a; stats[1] = (float)b; stats[2] = (float)c; stats[3] = 0.f;
    stats[4] = 0.f; stats[5] = (float)B; stats[6] = 0.f; stats[7] = 0.f;
  }
}
__global__ void critic_loss_kernel(const float* rewards, const float* discounts,
                                   const float* tq, const float* logp_next, float alpha,
                                   const float* q, float* dq, float* stats, int B, int Bp,
                                   int nets, CriticLoss loss, const float* v_low, const float* v_high) {
  critic_loss_rows(rewards, discounts, tq, logp_next, alpha, q, dq, stats, B, Bp, nets, loss, v_low, v_high);
}
// ... with SAC's coefficient read from the device (TemperArg, mlpfwd.h): alpha = expf(*log_alpha), once
__global__ void critic_loss_tempered_kernel(const float* rewards, const float* discounts,
                                            const float* tq, const float* logp_next, const float* log_alpha,
                                            const float* q, float* dq, float* stats, int B, int Bp,
                                            int nets, CriticLoss loss, const float* v_low, const float* v_high) {
  const float alpha = expf(*log_alpha);
  critic_loss_rows(rewards, discounts, tq, logp_next, alpha, q, dq, stats, B, Bp, nets, loss, v_low, v_high);
}

// QRegression (critics.py:31-53): y = returns[m] as given, one critic — dq = loss'(q - y) at the head's
// pre-activation and the statistics row critic_loss_kernel writes for one critic (LOSS_REGRESSION, mlpfwd.h).
__global__ void regression_loss_kernel(const float* returns, const float* q, float* dq, float* stats, int B,
                                       CriticLoss loss, const float* v_low, const float* v_high) {
  const ValueRange vrange = value_range(v_low, v_high);     // the Return normaliser's head: q holds squashed values
  float s_loss = 0.f, s_q = 0.f;
  for (int m = threadIdx.x; m < B; m += blockDim.x) {
    const float e = q[m] - returns[m];
    dq[m] = value_squash_dz(critic_loss_dq(e, loss.kind, loss.param), q[m], vrange);
    s_loss += critic_loss_term(e, loss.kind, loss.param);
    s_q += q[m];
  }
  double a = s_loss, b = s_q, unused = 0;
  block_sum3(a, b, unused);
  if (threadIdx.x == 0) {
    stats[0] = (float)a; stats[1] = (float)b;
    for (int i = 2; i < 8; ++i) stats[i] = i == 5 ? (float)B : 0.f;
  }
}

// Actor objective: SAC  loss = mean(alpha * logp - min(q1, q2))  (actors.py:254-257)
//                  TD3  loss = -mean(q1)                          (actors.py:177-179)
// d loss / d q_z (unscaled by 1/B): -1 on the smaller critic, -1/2 each on ties.
__device__ __forceinline__ void actor_loss_rows(const float* q, const float* logp, float alpha, int twin,
                                                float* dq, float* stats, int B, int Bp, const float* v_low,
                                                const float* v_high) {
  const ValueRange vrange = value_range(v_low, v_high);     // the Return normaliser's head: q holds squashed values
  float s = 0.f;
  for (int m = threadIdx.x; m < B; m += blockDim.x) {
    const float q1 = q[m];
    dq[m] = value_squash_dz(actor_dq(q, m, ValueLines{Bp, 16}, twin, 0), q1, vrange);
    if (twin) {
      dq[Bp + m] = value_squash_dz(actor_dq(q, m, ValueLines{Bp, 16}, twin, 1), q[Bp + m], vrange);
      s += alpha * logp[m] - fminf(q1, q[Bp + m]);
    } else {
      s += -q1;
    }
  }
  double a = s, unused1 = 0, unused2 = 0;
  block_sum3(a, unused1, unused2);
  if (threadIdx.x == 0) {
    stats[0] = (float)a;
    for (int i = 1; i < 8; ++i) stats[i] = i == 5 ? (float)B : 0.f;
  }
}
__global__ void actor_loss_kernel(const float* q, const float* logp, float alpha, int twin,
                                  float* dq, float* stats, int B, int Bp, const float* v_low,
                                  const float* v_high) {
  actor_loss_rows(q, logp, alpha, twin, dq, stats, B, Bp, v_low, v_high);
}
// ... with SAC's coefficient read from the device, and the coefficient's own block (entropy_coeff_sums) formed from
// the same logp by the same workgroup: no launch more
__global__ void actor_loss_tempered_kernel(const float* q, const float* logp, TemperArg temper, int twin,
                                           float* dq, float* stats, int B, int Bp, const float* v_low,
                                           const float* v_high) {
  const float log_alpha = *temper.log_alpha;
  const float alpha = expf(log_alpha);
  actor_loss_rows(q, logp, alpha, twin, dq, stats, B, Bp, v_low, v_high);
  if (temper.sums != nullptr) {
    __syncthreads();                                  // (block_sum3's wave partials are free again)
    entropy_coeff_sums(logp, B, log_alpha, alpha, temper.target_entropy, temper.sums);
  }
}

// ---- distributional critic (models/critics.py:23-66, D4PG): one wave per sample, lane = atom.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// softmax over the NA lanes of a wave (torch.nn.functional.softmax: exp(x - max) / sum)
__device__ __forceinline__ float wave_softmax(float logit, bool live, float* log_norm) {
  const float mx = wave_max(live ? logit : -INFINITY);
  const float e = live ? expf(logit - mx) : 0.f;
  const float sum = wave_sum(e);
  if (log_norm != nullptr) *log_norm = mx + logf(sum);
  return e / sum;
}

// The wave's row of a [B, ld] logits array: sample m, lane = atom; a lane past the support reads atom NA - 1 and is
// not `live`.  False: no row for this wave (the ragged last workgroup).
struct AtomRow { int lane, m, i; bool live; float z; };
__device__ __forceinline__ bool atom_row(const float* values, int NA, int B, AtomRow& r) {
  r.lane = threadIdx.x & 63;
  r.m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r.m >= B) return false;
  r.live = r.lane < NA;
  r.i = r.live ? r.lane : NA - 1;
  r.z = values[r.i];
  return true;
}

// CategoricalWithSupport.project (critics.py:32-46, restated with the same float32 expressions): atom i's share of
// the distribution p_next (lane = atom) moved to the returns r + disc * z_j; 0 on a lane that is not live.
__device__ __forceinline__ float projected_target(const AtomRow& r, const float* values, int NA, float reward,
                                                  float discount, float p_next) {
  const float z = r.z, vmin = values[0], vmax = values[NA - 1];
  const float ret = reward + discount * z;
  const float clipped = fminf(fmaxf(ret, vmin), vmax);
  const float d_pos = (r.i + 1 < NA ? values[r.i + 1] : vmin) - z;  // critics.py:34-35
  const float d_neg = z - (r.i > 0 ? values[r.i - 1] : vmax);       // critics.py:36-37
  float target = 0.f;
  for (int j = 0; j < NA; ++j) {
    const float delta = __shfl(clipped, j, 64) - z;                 // critics.py:40
    const float sign = delta >= 0.f ? 1.f : 0.f;
    const float hat = (sign * delta / d_pos) - ((1.f - sign) * delta / d_neg);
    target += fminf(fmaxf(1.f - hat, 0.f), 1.f) * __shfl(p_next, j, 64);
  }
  return r.live ? target : 0.f;
}

// One online critic (its logit on this lane) against the row's target T (total = sum_i T_i): the softmax,
// loss = -sum_i T_i log_softmax(logits)_i and grad = d loss / d logits_i = softmax_i total - T_i (0 on a padded lane).
// No memory access: the kernels load before and store after, so that no store stands between two critics' loads.
struct CriticRow { float p, loss, grad; };
__device__ __forceinline__ CriticRow critic_row(const AtomRow& r, float logit, float target, float total) {
  float log_norm;
  const float p = wave_softmax(logit, r.live, &log_norm);
  const float loss = -wave_sum(r.live ? target * (logit - log_norm) : 0.f);
  return CriticRow{p, loss, r.live ? p * total - target : 0.f};
}

// Prioritized replay: `weights` [B] scales a row's dlogits (in the kernels) and, here on lane 0, its loss_m — the
// statistics then sum w_m loss_m — and `sample_losses` [B] receives the unweighted loss; each may be null, both null:
// the bits as before.
__device__ __forceinline__ void store_row_loss(int m, float loss, const float* weights, float* loss_m,
                                               float* sample_losses) {
  loss_m[m] = weights != nullptr ? weights[m] * loss : loss;
  if (sample_losses != nullptr) sample_losses[m] = loss;
}

// DistributionalDeterministicQLearning (critics.py:100-122):
//   returns_j = r + disc * z_j ; targets = CategoricalWithSupport.project(returns) of the TARGET
//   critic's distribution ;
//   loss = -sum_i targets_i log_softmax(logits)_i ; d loss / d logits_i = softmax_i sum_k targets_k - targets_i
// (gradient of the SUM over the batch; the optimizer step divides by B).  loss_m: per-sample losses.
__global__ __launch_bounds__(256) void distributional_critic_loss_kernel(
    const float* target_logits, const float* logits, int ld, const float* rewards,
    const float* discounts, const float* values, int NA, float* dlogits, float* loss_m, int B,
    const float* weights, float* sample_losses) {
  AtomRow r;
  if (!atom_row(values, NA, B, r)) return;
  const float p_next = wave_softmax(target_logits[(int64_t)r.m * ld + r.i], r.live, nullptr);
  const float target = projected_target(r, values, NA, rewards[r.m], discounts[r.m], p_next);
  const CriticRow c = critic_row(r, logits[(int64_t)r.m * ld + r.i], target, wave_sum(target));
  float grad = c.grad;
  if (weights != nullptr) grad *= weights[r.m];
  if (r.lane < ld) dlogits[(int64_t)r.m * ld + r.lane] = grad;
  if (r.lane == 0) store_row_loss(r.m, c.loss, weights, loss_m, sample_losses);
}

// TD4 (the library's TwinCriticDistributionalDeterministicQLearning): two target critics and two online critics over
// ONE support.  p_k = softmax(target_logits_k), mu_k = sum_i p_k,i z_i; the row's target distribution is that of the
// target critic with the smaller mean — critic 2 only when mu_2 < mu_1, so a tie and a NaN mean select critic 1 —
// projected as above.  The triangular weights depend on the returns and the support alone, so the loop runs once, on
// the selected p_next.  Each online critic takes the cross-entropy against the same target;
// sample_m [3][Bp] = {loss_1 + loss_2, q1, q2} per sample, q_k = sum_i softmax(logits_k)_i z_i the ONLINE critics'
// means (the logged critic/q1, critic/q2).  Prioritized replay: both dlogits and sample_m's first entry take w_m,
// q1 / q2 do not; sample_losses receives loss_1 + loss_2.
__global__ __launch_bounds__(256) void twin_distributional_critic_loss_kernel(
    const float* target_logits_1, const float* target_logits_2, const float* logits_1, const float* logits_2, int ld,
    const float* rewards, const float* discounts, const float* values, int NA, float* dlogits_1, float* dlogits_2,
    float* sample_m, int B, int Bp, const float* weights, float* sample_losses) {
  AtomRow r;
  if (!atom_row(values, NA, B, r)) return;
  const float p1 = wave_softmax(target_logits_1[(int64_t)r.m * ld + r.i], r.live, nullptr);
  const float p2 = wave_softmax(target_logits_2[(int64_t)r.m * ld + r.i], r.live, nullptr);
  const float mu1 = wave_sum(r.live ? p1 * r.z : 0.f), mu2 = wave_sum(r.live ? p2 * r.z : 0.f);
  const float p_next = mu2 < mu1 ? p2 : p1;                          // (wave-uniform: every lane holds both sums)
  const float target = projected_target(r, values, NA, rewards[r.m], discounts[r.m], p_next);
  const float total = wave_sum(target);
  const CriticRow c1 = critic_row(r, logits_1[(int64_t)r.m * ld + r.i], target, total);
  const CriticRow c2 = critic_row(r, logits_2[(int64_t)r.m * ld + r.i], target, total);
  const float q1 = wave_sum(r.live ? c1.p * r.z : 0.f), q2 = wave_sum(r.live ? c2.p * r.z : 0.f);
  float grad_1 = c1.grad, grad_2 = c2.grad;
  if (weights != nullptr) { grad_1 *= weights[r.m]; grad_2 *= weights[r.m]; }
  if (r.lane < ld) {
    dlogits_1[(int64_t)r.m * ld + r.lane] = grad_1;
    dlogits_2[(int64_t)r.m * ld + r.lane] = grad_2;
  }
  if (r.lane == 0) {
    store_row_loss(r.m, c1.loss + c2.loss, weights, sample_m, sample_losses);
    sample_m[Bp + r.m] = q1; sample_m[2 * Bp + r.m] = q2;
  }
}

// the 8 statistics {sum loss_1 + loss_2, sum q1, sum q2, 0, 0, B, 0, 0} (the stats_kind 3 row) from the per-sample
// values sample_m [3][Bp] (fixed order, float64); TQC's {sum loss, sum q, 0, ...} row is the same sums over a third
// row of zeros
__global__ void twin_loss_stats_kernel(const float* sample_m, float* stats, int B, int Bp) {
  double a = 0, b = 0, c = 0;
  for (int m = threadIdx.x; m < B; m += blockDim.x) { a += sample_m[m]; b += sample_m[Bp + m]; c += sample_m[2 * Bp + m]; }
  block_sum3(a, b, c);
  if (threadIdx.x == 0) {
    stats[0] = (float)a; stats[1] = (float)b; stats[2] = (float)c; stats[3] = 0.f;
    stats[4] = 0.f; stats[5] = (float)B; stats[6] = 0.f; stats[7] = 0.f;
  }
}

// DistributionalDeterministicPolicyGradient (actors.py:203-224): value = sum_i softmax(logits)_i z_i,
// loss = -mean(value): d(-value) / d logits_i = -p_i (z_i - value).
__global__ __launch_bounds__(256) void distributional_actor_loss_kernel(
    const float* logits, int ld, const float* values, int NA, float* dlogits, float* loss_m,
    int B) {
  AtomRow r;
  if (!atom_row(values, NA, B, r)) return;
  const float p = wave_softmax(logits[(int64_t)r.m * ld + r.i], r.live, nullptr);
  const float value = wave_sum(r.live ? p * r.z : 0.f);
  if (r.lane < ld) dlogits[(int64_t)r.m * ld + r.lane] = r.live ? -(p * (r.z - value)) : 0.f;
  if (r.lane == 0) loss_m[r.m] = -value;
}

// the 8 statistics {loss_sum, 0, 0, 0, 0, B, 0, 0} from per-sample losses (fixed order, float64)
__global__ void loss_stats_kernel(const float* loss_m, float* stats, int B) {
  double a = 0, unused1 = 0, unused2 = 0;
  for (int m = threadIdx.x; m < B; m += blockDim.x) a += loss_m[m];
  block_sum3(a, unused1, unused2);
  if (threadIdx.x == 0) {
    stats[0] = (float)a;
    for (int i = 1; i < 8; ++i) stats[i] = i == 5 ? (float)B : 0.f;
  }
}

// ---- TQC (Kuznetsov et al. 2020, truncated quantile critics): SAC on 2 <= N <= 8 critics (the paper's default is 5;
// the twin model is N = 2) of M <= 32 quantile outputs each, one wave per sample.  The pool of P = N M <= 256 values
// need not fit one value per lane: a lane holds R = 1, 2 or 4 values, element e = 64 r + lane in register r.  The N
// critics' [B, ld] arrays (ld = pad16(M)) lie `stride` floats apart (critic z at base + z stride).
constexpr int kMaxQuantiles = 32, kMaxCritics = 8, kMaxPooled = 64 * 4;

// 64 R values ascending in e: the bitonic network over the wave's lanes, continued over the registers.  A step of
// partner distance below 64 is a __shfl_xor on each register, one of distance 64 d an exchange between registers r and
// r + d of the same lane: 21 steps at R = 1, 28 at 2, 36 at 4, fully unrolled — a fixed sequence whatever the values
// are (a NaN may displace a value; it cannot stop or lengthen the network).
template <int R>
__device__ __forceinline__ void wave_sort(float (&v)[R], int lane) {
#pragma unroll
  for (int k = 2; k <= 64 * R; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1) {
      if (j < 64) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float other = __shfl_xor(v[r], j, 64);
          const bool ascending = ((64 * r + lane) & k) == 0, lower = (lane & j) == 0;
          v[r] = ascending == lower ? fminf(v[r], other) : fmaxf(v[r], other);
        }
      } else {
        const int d = j >> 6;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if ((r & d) == 0 && r + d < R) {
            const float lo = fminf(v[r], v[r + d]), hi = fmaxf(v[r], v[r + d]);
            const bool ascending = ((64 * r) & k) == 0;       // (k >= 128: the register's bits decide)
            v[r] = ascending ? lo : hi;
            v[r + d] = ascending ? hi : lo;
          }
        }
      }
    }
  }
}

// TruncatedQuantileQLearning on N critics.  The N TARGET critics' values at (s', a') pooled in critic order (element
// e = z M + i, +inf behind them), sorted, the K = N (M - drop) smallest kept: rank j sits in register j / 64 of lane
// j % 64, y_j = r + disc (Z_j - alpha logp').  A lane owns the online quantiles e = 64 r + lane < P (critic e / M,
// quantile i = e % M, tau_i = (2 i + 1) / (2 M)) and walks the K targets in ascending j, u = y_j - theta, each y_j read
// from a wave-uniform lane of a compile-time register; the trip counts depend on K alone:
//   rho = |tau - 1{u < 0}| huber_1(u) ;  d rho / d theta = -|tau - 1{u < 0}| clamp(u, -1, 1)
//   loss_m = sum_z (1 / (M K)) sum_i sum_j rho (at N = 2 the twin convention loss_1 + loss_2) ;
//   dlogits: its gradient, 0 on a padded column ;
//   sample_m [3][Bp] = {loss_m, (1 / N) sum_z mean_i theta_zi, 0}, or with twin_row (wave-uniform; N = 2, so R = 1)
//   the twin row {loss_m, q1, q2}, q_z = mean_i theta_zi, each from a wave_sum of its own over critic z's quantiles.
// alpha = expf(*log_alpha) when that pointer is given, read once at entry like M and drop.
// The targets, the errors and the two sums over j are float64: a quantile's gradient is a sum of terms of both signs
// (with M = 1, +1/2 clamp(u_0) + 1/2 clamp(u_1)), and float32 targets of magnitude ~10 leave it an error of 1e-6 of
// a term however far the terms cancel.  At most 256 steps per row: the cost does not show beside the networks' passes.
template <int R>
__global__ __launch_bounds__(256) void quantile_critic_loss_kernel(
    const float* targets, const float* thetas, int64_t stride, int ld, const float* rewards, const float* discounts,
    const float* logp_next, int M, int N, int drop, float alpha, const float* log_alpha, float* dlogits,
    float* sample_m, int twin_row, int B, int Bp) {
  if (log_alpha != nullptr) alpha = expf(*log_alpha);
  const int lane = threadIdx.x & 63, m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= B) return;
  const int P = N * M, K = N * (M - drop);
  const int64_t row = (int64_t)m * ld;
  float pooled[R];
  double theta[R], tau[R], loss[R], grad[R];
  int64_t at[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = 64 * r + lane;
    const bool live = e < P;
    const int z = live ? e / M : 0, i = live ? e - z * M : 0;
    at[r] = z * stride + row + i;
    pooled[r] = live ? targets[at[r]] : INFINITY;
    theta[r] = live ? (double)thetas[at[r]] : 0.0;
    tau[r] = (double)(2 * i + 1) / (double)(2 * M);
    loss[r] = 0.0; grad[r] = 0.0;
  }
  wave_sort<R>(pooled, lane);
  const double reward = (double)rewards[m], discount = (double)discounts[m];
  const double bonus = (double)alpha * (double)logp_next[m];
#pragma unroll
  for (int s = 0; s < R; ++s) {
    const double y = reward + discount * ((double)pooled[s] - bonus);
    const int y_hi = __double2hiint(y), y_lo = __double2loint(y);
    const int count = min(64, K - 64 * s);                     // (wave-uniform; <= 0: nothing kept in this register)
    for (int j = 0; j < count; ++j) {
      const double y_j = __hiloint2double(__builtin_amdgcn_readlane(y_hi, j), __builtin_amdgcn_readlane(y_lo, j));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double u = y_j - theta[r];
        const double weight = u < 0.0 ? 1.0 - tau[r] : tau[r];
        const double a = fabs(u);
        loss[r] += weight * (a <= 1.0 ? 0.5 * (u * u) : a - 0.5);
        grad[r] += weight * fmin(fmax(u, -1.0), 1.0);
      }
    }
  }
  const double scale = 1.0 / (double)(M * K);
  double lane_loss = 0.0, lane_theta = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (64 * r + lane < P) {
      dlogits[at[r]] = (float)-(grad[r] * scale);
      lane_loss += loss[r]; lane_theta += theta[r];
    }
  }
  const int pad = ld - M;                                        // the padded columns of the N rows: exact 0
  for (int t = lane; t < N * pad; t += 64) {
    const int z = t / pad;
    dlogits[z * stride + row + M + (t - z * pad)] = 0.f;
  }
  // each form's sums in one block of its own, so that their cross-lane steps overlap
  if (twin_row) {                                                // (theta[0] is 0.0 on a lane past the pool)
    const double q1 = wave_sum(lane < M ? theta[0] : 0.0) / (double)M;
    const double q2 = wave_sum(lane >= M ? theta[0] : 0.0) / (double)M;
    const double row_loss = wave_sum(lane_loss) * scale;
    if (lane == 0) { sample_m[m] = (float)row_loss; sample_m[Bp + m] = (float)q1; sample_m[2 * Bp + m] = (float)q2; }
    return;
  }
  const double row_loss = wave_sum(lane_loss) * scale, q = wave_sum(lane_theta) / (double)P;
  if (lane == 0) { sample_m[m] = (float)row_loss; sample_m[Bp + m] = (float)q; sample_m[2 * Bp + m] = 0.f; }
}

// the launch for a pool of P = N M values: as many registers per lane as the pool needs
static void launch_quantile_critic_loss(hipStream_t st, const float* targets, const float* thetas, int64_t stride, int ld,
                                        const float* rewards, const float* discounts, const float* logp_next, int M,
                                        int N, int drop, float alpha, const float* log_alpha, float* dlogits,
                                        float* sample_m, int twin_row, int B, int Bp) {
  const int P = N * M;
  auto kernel = P <= 64 ? quantile_critic_loss_kernel<1>
                        : P <= 128 ? quantile_critic_loss_kernel<2> : quantile_critic_loss_kernel<4>;
  hipLaunchKernelGGL(kernel, dim3((B + 3) / 4), dim3(256), 0, st, targets, thetas, stride, ld, rewards, discounts,
                     logp_next, M, N, drop, alpha, log_alpha, dlogits, sample_m, twin_row, B, Bp);
}

// TwinCriticQuantileSoftPolicyGradient on N critics: Q = (1 / (N M)) sum_z sum_i theta_zi(s, a) on the (frozen) online
// critics, loss_m = alpha logp - Q: dlogits = -1 / (N M) on the live columns, 0 on the padding; the wave walks the N
// rows' N ld columns.  With a tuner (temper.sums) workgroup 0, whole, also forms the coefficient's block, as
// actor_loss_tempered_kernel does.
__global__ __launch_bounds__(256) void quantile_actor_loss_kernel(
    const float* thetas, int64_t stride, int ld, const float* logp, int M, int N, float alpha, TemperArg temper,
    float* dlogits, float* loss_m, int B) {
  float log_alpha = 0.f;
  if (temper.log_alpha != nullptr) { log_alpha = *temper.log_alpha; alpha = expf(log_alpha); }
  const int lane = threadIdx.x & 63, m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m < B) {
    const int64_t row = (int64_t)m * ld;
    float sum = 0.f;
    for (int t = lane; t < N * ld; t += 64) {
      const int z = t / ld, c = t - z * ld;
      const int64_t at = z * stride + row + c;
      if (c < M) sum += thetas[at];
      dlogits[at] = c < M ? -1.f / (float)(N * M) : 0.f;
    }
    const float q = wave_sum(sum) / (float)(N * M);
    if (lane == 0) loss_m[m] = alpha * logp[m] - q;
  }
  if (temper.sums != nullptr && blockIdx.x == 0)
    entropy_coeff_sums(logp, B, log_alpha, alpha, temper.target_entropy, temper.sums);
}

// d loss / d action of critics 2 .. N added into critic 2's block (fixed order), so that SAC's head backward, which adds
// two blocks, serves N: blocks [N][count], block 1 += block 2 + ... + block N - 1.
__global__ void ensemble_action_grad_sum_kernel(float* blocks, int N, int64_t count) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= count) return;
  float sum = blocks[count + idx];
  for (int z = 2; z < N; ++z) sum += blocks[z * count + idx];
  blocks[count + idx] = sum;
}

// ---- REDQ (Chen et al. 2021, randomized ensembled double Q-learning): SAC on 2 <= N <= 8 SCALAR critics — TQC's
// layout at one output, so the value of critic z at row m is column 0 of its [Bp, ld] block — one wave per sample.
// EnsembleSoftQLearning: S = the target critics whose bit is set in the ONE device word *subset (read here, so a
// captured graph follows a new draw; bits at and above N ignored; none of the low N set: all N — no value of the word
// reaches a block outside the N):
//   y = r + disc (min_{z in S} Qt_z(s', a') - alpha logp') ;  loss_m = sum_z l(Q_z(s, a) - y) over ALL N online critics ;
//   dq: column 0 = l'(Q_z - y) (critic_loss_term / critic_loss_dq, mlpfwd.h), 0 on every column behind it ;
//   sample_m [3][Bp] = {loss_m, (1 / N) sum_z Q_z, 0}: the ensemble row of quantile_critic_loss_kernel.
// The minimum walks S in ascending z on every lane (wave-uniform loads, N <= 8) and keeps a NaN once it meets one, as
// torch.min does (fminf would drop it); a target critic outside S is never read.  y and the errors are float64 (a
// float32 y of magnitude ~10 would leave a small error 1e-6 / |e| of itself); lane z < N owns online critic z, and
// the two sums over the critics are wave_sums of float64: no atomics, the same inputs give the same bits.
// alpha = expf(*log_alpha) when that pointer is given, read once at entry.
__global__ __launch_bounds__(256) void ensemble_subset_critic_loss_kernel(
    const float* targets, const float* qs, int64_t stride, int ld, const float* rewards, const float* discounts,
    const float* logp_next, int N, const int32_t* subset, float alpha, const float* log_alpha, CriticLoss loss,
    float* dq, float* sample_m, int B, int Bp) {
  if (log_alpha != nullptr) alpha = expf(*log_alpha);
  const int all = (1 << N) - 1;
  int mask = *subset & all;
  if (mask == 0) mask = all;
  const int lane = threadIdx.x & 63, m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= B) return;
  const int64_t row = (int64_t)m * ld;
  float low = INFINITY;
  for (int z = 0; z < N; ++z) {
    if (((mask >> z) & 1) == 0) continue;
    const float t = targets[z * stride + row];
    low = (t < low || t != t) ? t : low;                         // (a NaN `low` fails both tests: it stays)
  }
  const double y = (double)rewards[m] + (double)discounts[m] * ((double)low - (double)alpha * (double)logp_next[m]);
  const bool live = lane < N;
  const float q = live ? qs[lane * stride + row] : 0.f;
  const float e = (float)((double)q - y);
  if (live) dq[lane * stride + row] = critic_loss_dq(e, loss.kind, loss.param);
  const int pad = ld - 1;                                        // the padded columns of the N rows: exact 0
  for (int t = lane; t < N * pad; t += 64) {
    const int z = t / pad;
    dq[z * stride + row + 1 + (t - z * pad)] = 0.f;
  }
  const double row_loss = wave_sum(live ? (double)critic_loss_term(e, loss.kind, loss.param) : 0.0);
  const double q_mean = wave_sum(live ? (double)q : 0.0) / (double)N;
  if (lane == 0) { sample_m[m] = (float)row_loss; sample_m[Bp + m] = (float)q_mean; sample_m[2 * Bp + m] = 0.f; }
}

// what REDQ's critic step adds to TQC's: where the subset's word lies and the rule of `loss=`
struct SubsetLoss { const int32_t* subset; CriticLoss rule; };

static void launch_subset_critic_loss(hipStream_t st, const float* targets, const float* qs, int64_t stride, int ld,
                                      const float* rewards, const float* discounts, const float* logp_next, int N,
                                      const SubsetLoss& s, float alpha, const float* log_alpha, float* dq,
                                      float* sample_m, int B, int Bp) {
  hipLaunchKernelGGL(ensemble_subset_critic_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, st, targets, qs, stride, ld,
                     rewards, discounts, logp_next, N, s.subset, alpha, log_alpha, s.rule, dq, sample_m, B, Bp);
}

// ---- DMPO: MPO's sampled actions on the categorical critic.  The target critic's logits on the S * B tiled rows
// (row s * B + m), one wave per row, lane = atom: the row's mean value sum_i softmax(logits)_i z_i -> tq — what the
// E-step reads where the scalar critic leaves its output — and, log_norm != null, the row's log-normaliser
// max + log(sum_i exp(logit_i - max)), which the mixture kernel below turns logits into probabilities with.
__global__ __launch_bounds__(256) void distributional_value_kernel(const float* logits, int ld, const float* values,
                                                                   int NA, float* tq, float* log_norm, int rows) {
  AtomRow r;
  if (!atom_row(values, NA, rows, r)) return;
  float ln;
  const float p = wave_softmax(logits[(int64_t)r.m * ld + r.i], r.live, &ln);
  const float value = wave_sum(r.live ? p * r.z : 0.f);
  if (r.lane == 0) {
    tq[r.m] = value;
    if (log_norm != nullptr) log_norm[r.m] = ln;
  }
}

// The distributional Expected-SARSA loss, one wave per state m, lane = atom:
//   p_bar = (1 / S) sum_s softmax(target_logits[s * B + m])   (the mixture of the S sampled actions' distributions;
//                                                              the projection is linear in p: it runs once, on p_bar)
//   T = project(r + disc * z, p_bar) ; loss = -sum_i T_i log_softmax(logits)_i ; dlogits_i = softmax_i sum T - T_i
// The loop over s reads each row's log-normaliser from distributional_value_kernel, exp(logit - log_norm), so it
// holds no cross-lane step however many samples there are.  sample_m [2][Bp] = {loss, q} per state,
// q = sum_i softmax(logits)_i z_i the ONLINE critic's mean (the logged critic/q).
__global__ __launch_bounds__(256) void mixture_critic_loss_kernel(
    const float* target_logits, const float* target_log_norm, const float* logits, int ld, const float* rewards,
    const float* discounts, const float* values, int NA, float* dlogits, float* sample_m, int B, int Bp, int S) {
  AtomRow r;
  if (!atom_row(values, NA, B, r)) return;
  float mix = 0.f;
  for (int s = 0; s < S; ++s) {
    const int64_t row = (int64_t)s * B + r.m;
    mix += expf(target_logits[row * ld + r.i] - target_log_norm[row]);
  }
  const float p_next = r.live ? mix / (float)S : 0.f;
  const float target = projected_target(r, values, NA, rewards[r.m], discounts[r.m], p_next);
  const CriticRow c = critic_row(r, logits[(int64_t)r.m * ld + r.i], target, wave_sum(target));
  const float q = wave_sum(r.live ? c.p * r.z : 0.f);
  if (r.lane < ld) dlogits[(int64_t)r.m * ld + r.lane] = c.grad;
  if (r.lane == 0) { sample_m[r.m] = c.loss; sample_m[Bp + r.m] = q; }
}

// the 8 statistics {sum loss, sum q, 0, 0, 0, B, 0, 0} (ExpectedSARSA's row) from sample_m [2][Bp] (fixed order,
// float64)
__global__ void mixture_loss_stats_kernel(const float* sample_m, float* stats, int B, int Bp) {
  double a = 0, b = 0, unused = 0;
  for (int m = threadIdx.x; m < B; m += blockDim.x) { a += sample_m[m]; b += sample_m[Bp + m]; }
  block_sum3(a, b, unused);
  if (threadIdx.x == 0) {
    stats[0] = (float)a; stats[1] = (float)b;
    for (int i = 2; i < 8; ++i) stats[i] = i == 5 ? (float)B : 0.f;
  }
}

// ---- MPO (agents/mpo.py; updaters/critics.py:238-282, updaters/actors.py:270-464)
// GaussianPolicyHead (models/actors.py:69-98): loc = tanh(.) (applied by the forward), sigma =
// clamp(softplus(spre), scale_lo, scale_hi).
__device__ __forceinline__ float gaussian_sigma(float spre, float scale_lo, float scale_hi) {
  return fminf(fmaxf(softplus_f(spre), scale_lo), scale_hi);
}

// Normal.sample / rsample: a = loc + sigma * eps (eps == null: the greedy loc, mpo.py:82-85)
__global__ void gaussian_sample_kernel(const float* loc, const float* spre, const float* eps,
                                       int ld, float* act, int B, int A, float scale_lo, float scale_hi) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * A) return;
  const int m = idx / A, a = idx - m * A;
  const float l = loc[(int64_t)m * ld + a];
  act[idx] = eps ? l + gaussian_sigma(spre[(int64_t)m * ld + a], scale_lo, scale_hi) * eps[idx] : l;
}

// S samples per state, tiled like updaters.tile + merge_first_two_dims (row s * B + m):
//   act[s, m] = loc[m] + sigma[m] * eps[s, m] ;  X[s * B + m] = [ norm(obs[m]) | act[s, m] ]
__global__ void gaussian_tile_kernel(const float* obs, const float* loc, const float* spre,
                                     const float* eps, int ldh, const float* mean,
                                     const float* std, float clip, float* act, float* X, int B,
                                     int O, int A, int S, int ldx, float scale_lo, float scale_hi) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)S * B * (O + A)) return;
  const int64_t r = idx / (O + A);
  const int c = (int)(idx - r * (O + A));
  const int m = (int)(r % B);
  if (c < O) {
    X[r * ldx + c] = __builtin_amdgcn_fmed3f((obs[(int64_t)m * O + c] - mean[c]) / std[c], -clip, clip);
  } else {
    const int a = c - O;
    const float v = loc[(int64_t)m * ldh + a] +
                    gaussian_sigma(spre[(int64_t)m * ldh + a], scale_lo, scale_hi) * eps[r * A + a];
    act[r * A + a] = v;
    X[r * ldx + c] = v;
  }
}

// next_values.view(S, -1).mean(dim=0) (critics.py:269-270)
__global__ void sample_mean_kernel(const float* q, float* out, int B, int S) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= B) return;
  float sum = 0.f;
  for (int s = 0; s < S; ++s) sum += q[(int64_t)s * B + m];
  out[m] = sum / (float)S;
}

// E-step samples per state: lane l of the state's wave holds samples l, l + 64, ... in kMpoMaxSlots register
// slots (a condition of mpo_state_kernel's layout, not a tuned figure)
constexpr int kMpoMaxSlots = 4;
constexpr int kMpoMaxSamples = 64 * kMpoMaxSlots;
constexpr int kMpoStats = 16;    // per-state partials: see mpo_state_kernel

// duals [2 K + 2] = {log_temperature, log_alpha_mean[K], log_alpha_std[K], log_penalty_temperature}, K = A
// (per_dim_constraining) or K = 1 (joint_kl: one alpha pair on the KLs of the Independent normals, actors.py:300-316);
// value = softplus(log) + 1e-8 (actors.py:378-383)
__device__ __forceinline__ float dual_value(float log_dual) { return softplus_f(log_dual) + 1e-8f; }

// E-step weights and the M-step gradients at the head outputs, one WAVE per state: lane = sample for
// the weights, lane = action dimension for the gradients (actors.py:384-432).  SUMS over the batch
// (the optimizer step divides by B):
//   d/d loc   = -sum_s W_s (a_s - loc) / sigma_t^2 + alpha_mean (loc - loc_t) / sigma_t^2
//   d/d sigma = -sum_s W_s ((a_s - loc_t)^2 / sigma^3 - 1 / sigma) + alpha_std (1 / sigma - sigma_t^2 / sigma^3)
// with W = softmax_s(q / T) + softmax_s(bound cost / T_penalty).  part[m][.] = {policy_mean, policy_std,
// LSE, LSE - sum_s w q / T, LSE_penalty, LSE_penalty - sum_s w_p cost / T_p}; klm / kls [m][a] = the
// per-dimension KLs (joint_kl: the dual kernel sums them over a; every dimension reads the one alpha pair).
// The temperatures' gradients need the differences LSE - sum_s w x (the entropy of w, in
// [0, log S]): they are formed here in the max-shifted frame, log(sum) - sum_s w (x - max), because at a cold
// temperature LSE and sum_s w x are each of the order of |x| (~1e7 for a penalty temperature on the dual floor)
// and their difference would be lost to float32 rounding.
// SLOTS = ceil(S / 64): lane l holds samples l + 64 k in slot k (arrays indexed by unrolled constants only, so
// they stay in registers); a reduction runs over the lane's slots in ascending k, then across the wave.
// SLOTS = 1 is the one-sample-per-lane kernel operation for operation.
template <int SLOTS>
__global__ __launch_bounds__(256) void mpo_state_kernel(
    const float* q, const float* act, const float* loc_t, const float* spre_t, const float* loc,
    const float* spre, int ldh, const float* duals, float floor, int penalize, int joint_kl, float* dloc,
    float* dspre, float* part, float* klm, float* kls, int B, int A, int S, float scale_lo, float scale_hi) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= B) return;
  const int K = joint_kl ? 1 : A;
  // (every log-dual is read through the floor the reference clamps it to, in place, at the head of its call —
  //  actors.py:347-356; mpo_dual_kernel, the last reader ahead of the duals' optimizer step, writes the
  //  clamped values back)
  const float T = dual_value(fmaxf(duals[0], floor)), Tp = dual_value(fmaxf(duals[2 * K + 1], floor));
  // softmax over the samples of x (-inf in the slots past S): w[k], LSE and the entropy-like difference
  auto softmax = [&](const float (&x)[SLOTS], float (&w)[SLOTS], float* lse) {
    float mx = x[0];
#pragma unroll
    for (int k = 1; k < SLOTS; ++k) mx = fmaxf(mx, x[k]);
    mx = wave_max(mx);
    float e[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) e[k] = lane + 64 * k < S ? expf(x[k] - mx) : 0.f;
    float sum = e[0];
#pragma unroll
    for (int k = 1; k < SLOTS; ++k) sum += e[k];
    sum = wave_sum(sum);
    *lse = mx + logf(sum);
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) w[k] = e[k] / sum;
    float wx = lane < S ? w[0] * (x[0] - mx) : 0.f;
#pragma unroll
    for (int k = 1; k < SLOTS; ++k) wx += lane + 64 * k < S ? w[k] * (x[k] - mx) : 0.f;
    return logf(sum) - wave_sum(wx);
  };
  // weights_and_temperature_loss (actors.py:325-338): softmax over the samples of q / T
  float x[SLOTS], w[SLOTS];
#pragma unroll
  for (int k = 0; k < SLOTS; ++k)
    x[k] = lane + 64 * k < S ? q[(int64_t)(lane + 64 * k) * B + m] / T : -INFINITY;
  float lse;
  const float wq = softmax(x, w, &lse);
  float lse_p = 0.f, wc = 0.f;
  if (penalize) {                                              // actors.py:388-398
    float wp[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      const int s = lane + 64 * k;
      float n2 = 0.f;
      if (s < S) {
        for (int a = 0; a < A; ++a) {
          const float v = act[((int64_t)s * B + m) * A + a];
          const float d = v - fminf(fmaxf(v, -1.f), 1.f);
          n2 += d * d;
        }
      }
      x[k] = s < S ? -sqrtf(n2) / Tp : -INFINITY;
    }
    wc = softmax(x, wp, &lse_p);
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) w[k] += wp[k];
  }
  // lane = action dimension: the sums over the samples in sample order
  const bool live = lane < A;
  const int a = live ? lane : A - 1;
  const float lt = loc_t[(int64_t)m * ldh + a], st = gaussian_sigma(spre_t[(int64_t)m * ldh + a], scale_lo, scale_hi);
  const float lo = loc[(int64_t)m * ldh + a], pre = spre[(int64_t)m * ldh + a];
  const float sg = gaussian_sigma(pre, scale_lo, scale_hi);
  float pm = 0.f, ps = 0.f, g_loc = 0.f, g_sigma = 0.f;
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) {
    const int n = min(64, S - 64 * k);
    for (int j = 0; j < n; ++j) {
      const float ws = __shfl(w[k], j, 64);
      const float v = act[((int64_t)(64 * k + j) * B + m) * A + a];
      const float d_mean = v - lo, d_std = v - lt;
      // Normal.log_prob: -(x - mu)^2 / (2 var) - log(sigma) - log(sqrt(2 pi))
      pm += ws * (-(d_mean * d_mean) / (2.f * (st * st)) - logf(st) - kHalfLog2Pi);
      ps += ws * (-(d_std * d_std) / (2.f * (sg * sg)) - logf(sg) - kHalfLog2Pi);
      g_loc -= ws * d_mean / (st * st);
      g_sigma -= ws * (d_std * d_std / (sg * sg * sg) - 1.f / sg);
    }
  }
  pm = wave_sum(live ? pm : 0.f);
  ps = wave_sum(live ? ps : 0.f);
  if (live) {
    // kl_divergence(Normal(lt, st), Normal(lo, st)) and (.., Normal(lt, sg)) (actors.py:416-421)
    const float ratio = st / sg;
    klm[(int64_t)m * A + a] = 0.5f * ((lt - lo) / st) * ((lt - lo) / st);
    kls[(int64_t)m * A + a] = 0.5f * (ratio * ratio - 1.f - logf(ratio * ratio));
    const int k = joint_kl ? 0 : a;
    const float alpha_mean = dual_value(fmaxf(duals[1 + k], floor)),
                alpha_std = dual_value(fmaxf(duals[1 + K + k], floor));
    g_loc += alpha_mean * (lo - lt) / (st * st);
    g_sigma += alpha_std * (1.f / sg - st * st / (sg * sg * sg));
    const float raw = softplus_f(pre);
    const bool inside = raw >= scale_lo && raw <= scale_hi;
    dloc[(int64_t)m * ldh + a] = g_loc * (1.f - lo * lo);                  // tanh loc head
    dspre[(int64_t)m * ldh + a] = inside ? g_sigma / (1.f + expf(-pre)) : 0.f;
  }
  if (lane == 0) {
    float* out = part + (int64_t)m * kMpoStats;
    out[0] = pm; out[1] = ps; out[2] = lse; out[3] = wq; out[4] = lse_p; out[5] = wc;
  }
}

// Batch means -> the logged losses, the dual variables' values and their gradients (one workgroup).
// stats [7 + 2 K + 2] = {policy_mean_loss, policy_std_loss, kl_mean_loss, kl_std_loss, alpha_mean_loss,
// alpha_std_loss, temperature_loss, temperature, alpha_mean[K], alpha_std[K], penalty_temperature};
// dual_grads [2 K + 2 + 8]: d loss / d log-duals + the statistics slot of the optimizer step.  K = A, or 1 with
// joint_kl: the one alpha pair constrains the KLs summed over the action dimensions (actors.py:319-323 on KLs of
// shape [B] with an alpha of shape [1]).
//
// Several ranks (each holds B of the B_norm states of the global batch): everything below is a
// function of the column MEANS, so the kernel runs in two halves around one all-reduce —
// out_sums != null: only the local column sums [6 + 2 A] (float64) are written; in_sums != null: the
// columns are taken from there (the all-reduced sums) instead of the per-state arrays.
__global__ void mpo_dual_kernel(const float* part, const float* klm, const float* kls,
                                float* duals, float floor, int penalize, int joint_kl, float epsilon,
                                float epsilon_penalty, float epsilon_mean, float epsilon_std,
                                float* dual_grads, float* stats, float* actor_stats, int B, int A,
                                int S, const double* in_sums, double* out_sums, int B_norm) {
  __shared__ double col[2 * 64 + 6];
  const int tid = threadIdx.x;
  // column means in fixed order: columns 0..5 the six partials, 6..6+A-1 kl_mean, then kl_std; one
  // wave per column, the lanes stride over the batch
  const int columns = 6 + 2 * A, lane = tid & 63, waves = blockDim.x >> 6;
  for (int c = tid >> 6; c < columns; c += waves) {
    double sum = 0;
    if (in_sums != nullptr) {
      sum = in_sums[c];
    } else {
      for (int m = lane; m < B; m += 64)
        sum += c < 6 ? part[(int64_t)m * kMpoStats + c]
                     : c < 6 + A ? klm[(int64_t)m * A + (c - 6)] : kls[(int64_t)m * A + (c - 6 - A)];
      sum = wave_sum(sum);
    }
    if (lane == 0) {
      if (out_sums != nullptr) out_sums[c] = sum;
      col[c] = sum / B_norm;
    }
  }
  if (out_sums != nullptr) return;                    // (uniform)
  __syncthreads();
  if (tid >= 64) return;                              // wave 0: lane = constraint (action dimension, or the one)
  const int K = joint_kl ? 1 : A;
  const float log_T = fmaxf(duals[0], floor), log_Tp = fmaxf(duals[2 * K + 1], floor);
  const float T = dual_value(log_T), Tp = dual_value(log_Tp);
  const float log_S = logf((float)S);
  auto sigmoid = [](float x) { return 1.f / (1.f + expf(-x)); };
  float kl_mean_loss = 0.f, kl_std_loss = 0.f, alpha_mean_loss = 0.f, alpha_std_loss = 0.f;
  if (tid < K) {
    const int a = tid;
    const float log_am = fmaxf(duals[1 + a], floor), log_as = fmaxf(duals[1 + K + a], floor);
    const float am = dual_value(log_am), as = dual_value(log_as);
    float km, ks;
    if (joint_kl) {                                   // the KL of the Independent normals: summed over a
      double sm = 0, ss = 0;
      for (int i = 0; i < A; ++i) { sm += col[6 + i]; ss += col[6 + A + i]; }
      km = (float)sm; ks = (float)ss;
    } else {
      km = (float)col[6 + a]; ks = (float)col[6 + A + a];
    }
    kl_mean_loss = am * km; kl_std_loss = as * ks;                        // actors.py:319-323
    alpha_mean_loss = am * (epsilon_mean - km);
    alpha_std_loss = as * (epsilon_std - ks);
    dual_grads[1 + a] = (epsilon_mean - km) * sigmoid(log_am);
    dual_grads[1 + K + a] = (epsilon_std - ks) * sigmoid(log_as);
    duals[1 + a] = log_am; duals[1 + K + a] = log_as;      // the reference's in-place clamp (actors.py:347-356)
    stats[8 + a] = am; stats[8 + K + a] = as;
  }
  kl_mean_loss = wave_sum(kl_mean_loss); kl_std_loss = wave_sum(kl_std_loss);
  alpha_mean_loss = wave_sum(alpha_mean_loss); alpha_std_loss = wave_sum(alpha_std_loss);
  if (tid != 0) return;
  // temperature * (epsilon + mean(logsumexp) - log S): d / dT = epsilon + mean(LSE - sum_s w q / T) - log S
  float temperature_loss = T * (epsilon + (float)col[2] - log_S);
  dual_grads[0] = (epsilon + (float)col[3] - log_S) * sigmoid(log_T);
  duals[0] = log_T;
  if (penalize) duals[2 * K + 1] = log_Tp;
  dual_grads[2 * K + 1] = 0.f;
  if (penalize) {
    temperature_loss += Tp * (epsilon_penalty + (float)col[4] - log_S);
    dual_grads[2 * K + 1] =
        (epsilon_penalty + (float)col[5] - log_S) * sigmoid(log_Tp);
  }
  for (int i = 0; i < 8; ++i) dual_grads[2 * K + 2 + i] = i == 5 ? 1.f : 0.f;
  stats[0] = -(float)col[0]; stats[1] = -(float)col[1]; stats[2] = kl_mean_loss; stats[3] = kl_std_loss;
  stats[4] = alpha_mean_loss; stats[5] = alpha_std_loss; stats[6] = temperature_loss; stats[7] = T;
  stats[8 + 2 * K] = Tp;
  // the actor's statistics slot {loss_sum = B * (policy losses + KL losses), 0, 0, 0, 0, B, 0, 0}
  actor_stats[0] = (float)B * (stats[0] + stats[1] + kl_mean_loss + kl_std_loss);
  for (int i = 1; i < 8; ++i) actor_stats[i] = i == 5 ? (float)B : 0.f;
}

// Back through the squashed Gaussian head (SAC) or the tanh head (TD3).
//   da[m][a] = d loss / d action (the action columns of the critics' input gradients, [B, pad16(A)])
// SAC: u = loc + sigma eps, a = tanh(u):
//   d loss/d u   = da (1 - a^2) + alpha * 2 a (1 - a^2) / (1 - a^2 + 1e-6)
//   d loss/d loc = d loss/d u ;  d loss/d sigma = d loss/d u * eps - alpha / sigma
//   d sigma/d spre = sigmoid(spre) inside the clamp, else 0.
// TD3: a = tanh(z):  d loss/d z = da (1 - a^2).
__device__ __forceinline__ void actor_head_backward_element(const float* dxa0, const float* dxa1, int ldxa,
                                                            const float* act,
                                                            const float* eps, const float* sigma,
                                                            const float* spre, int ld, float alpha, int sac,
                                                            float* dloc, float* dspre, int B, int A, float scale_lo,
                                                            float scale_hi) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * A) return;
  const int m = idx / A, a = idx - m * A;
  // d loss / d action = sum over the critics of the action columns of their input gradient
  float da = dxa0[(int64_t)m * ldxa + a];
  if (dxa1 != nullptr) da = da + dxa1[(int64_t)m * ldxa + a];
  const float t = act[idx];
  const float one_m = 1.f - t * t;
  if (!sac) {
    dloc[(int64_t)m * ld + a] = da * one_m;
    return;
  }
  const float du = da * one_m + alpha * (2.f * t * one_m / (one_m + kSacLogEps));
  const float sg = sigma[idx];
  const float dsigma = du * eps[idx] - alpha / sg;
  const float pre = spre[(int64_t)m * ld + a];
  const float raw = softplus_f(pre);
  const bool inside = raw >= scale_lo && raw <= scale_hi;
  dloc[(int64_t)m * ld + a] = du;
  dspre[(int64_t)m * ld + a] = inside ? dsigma / (1.f + expf(-pre)) : 0.f;
}
__global__ void actor_head_backward_kernel(const float* dxa0, const float* dxa1, int ldxa,
                                           const float* act,
                                           const float* eps, const float* sigma,
                                           const float* spre, int ld, float alpha, int sac,
                                           float* dloc, float* dspre, int B, int A, float scale_lo,
                                           float scale_hi) {
  actor_head_backward_element(dxa0, dxa1, ldxa, act, eps, sigma, spre, ld, alpha, sac, dloc, dspre, B, A, scale_lo,
                              scale_hi);
}
// ... the squashed Gaussian head with SAC's coefficient read from the device (TemperArg, mlpfwd.h)
__global__ void actor_head_backward_tempered_kernel(const float* dxa0, const float* dxa1, int ldxa,
                                                    const float* act,
                                                    const float* eps, const float* sigma,
                                                    const float* spre, int ld, const float* log_alpha,
                                                    float* dloc, float* dspre, int B, int A, float scale_lo,
                                                    float scale_hi) {
  const float alpha = expf(*log_alpha);
  actor_head_backward_element(dxa0, dxa1, ldxa, act, eps, sigma, spre, ld, alpha, 1, dloc, dspre, B, A, scale_lo,
                              scale_hi);
}

// Buffer.get gather (buffers.py:84-91): one wave per sampled transition.
struct GatherArgs {
  const int64_t* indices;
  const float* obs; const float* act; const float* next; const float* rew; const float* disc;
  float* o_obs; float* o_act; float* o_next; float* o_rew; float* o_disc;
  int64_t W;
  int B, O, A;
};

__global__ __launch_bounds__(256) void buffer_gather_kernel(GatherArgs g) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= g.B) return;
  const int64_t idx = g.indices[b];
  const int64_t row = idx / g.W, col = idx - row * g.W;       // rows = idx // W, cols = idx % W
  const int64_t t = row * g.W + col;
  for (int k = lane; k < g.O; k += 64) {
    g.o_obs[(int64_t)b * g.O + k] = g.obs[t * g.O + k];
    g.o_next[(int64_t)b * g.O + k] = g.next[t * g.O + k];
  }
  for (int k = lane; k < g.A; k += 64) g.o_act[(int64_t)b * g.A + k] = g.act[t * g.A + k];
  if (lane == 0) { g.o_rew[b] = g.rew[t]; g.o_disc[b] = g.disc[t]; }
}

// Buffer.accumulate_n_steps (buffers.py:58-79) after the row write of one store: thread = one
// (worker, next-observation feature) element; the reset mask chain of a worker is recomputed per
// thread (at most return_steps - 1 reads).  Every expression keeps the reference's separate
// float32 roundings — `(1 - m) * old + m * new` is NOT replaced by a select, so that even the
// sign of a zero comes out as in NumPy.
struct NStepArgs {
  float* b_next; float* b_rew; float* b_disc; const float* b_rst;
  const float* next; const float* rew; const float* term;
  int64_t row, size, max_size, W;
  int O, back;
  float discount;
};

__global__ __launch_bounds__(256) void buffer_nstep_kernel(NStepArgs a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.W * a.O) return;
  const int64_t w = e / a.O;
  const int k = (int)(e - w * a.O);
  const float reward = a.rew[w];
  const float discount = (1.f - a.term[w]) * a.discount;             // buffers.py:34-36
  const float next = a.next[e];
  float mask = 1.f;
  for (int i = 0; i < a.back; ++i) {
    int64_t index = (a.row - i - 1) % a.max_size;
    if (index < 0) index += a.max_size;                              // Python modulo
    const int64_t at = index * a.W + w;
    mask = mask * (1.f - a.b_rst[at]);
    const float keep = 1.f - mask;
    if (k == 0) {
      const float r_old = a.b_rew[at], d_old = a.b_disc[at];
      const float scaled = d_old * reward;
      const float new_reward = r_old + scaled;
      const float r_keep = keep * r_old, r_take = mask * new_reward;
      a.b_rew[at] = r_keep + r_take;
      const float new_discount = d_old * discount;
      const float d_keep = keep * d_old, d_take = mask * new_discount;
      a.b_disc[at] = d_keep + d_take;
    }
    const float o_keep = keep * a.b_next[at * a.O + k], o_take = mask * next;
    a.b_next[at * a.O + k] = o_keep + o_take;
  }
}

// Buffer.store row write (buffers.py:33-52) + MeanStd.record (mean_stds.py:44-48): bufstore.h
__global__ __launch_bounds__(1024) void buffer_store_kernel(BufferStoreArgs a) {
  __shared__ float tile[16384];
  buffer_store_body(a, tile, 16384, (int)blockIdx.x, (int)gridDim.x);
}

// --------------------------------------------------------------------------- host helpers

namespace {

inline int pad16(int x) { return (x + 15) / 16 * 16; }
// Row pitch of the batch-major scratch matrices the weight-gradient GEMMs walk along the batch
// (hidden activations, their gradients, the critics' input): never a multiple of 128 bytes
// (profiles/r01_ubench_row_stride.md).
inline int pitch16(int x) { return weight_ld(pad16(x)); }

// Pointers into one actor's block of a flat buffer (parameters, or the gradient sums of the same
// layout); ld1 / ldH: row strides of W1 and of the H-column weights; W[l] / b[l] / ld[l]: layer l of any depth.
template <typename T>
struct ActorBlock {
  T *W1, *b1, *W2, *b2, *Wh;                    // Wh: first head; the second follows head_stride on
  T *W[kTorsoMaxLayers], *b[kTorsoMaxLayers];   // (W1 = W[0], W2 = W[1])
  int ld[kTorsoMaxLayers];                      // row pitch of W[l]: weight_ld of the layer's input width
  ActorShape s;
  int ld1, ldH;
  int64_t head_stride;
  int ldO;                                       // row pitch of the heads (their inputs: the last layer)
  ActorBlock(T* p, ActorShape sh) : s(sh), ldO(weight_ld(sh.last())) {
    T* at = p;
    int in = s.O;
    for (int l = 0; l < kTorsoMaxLayers; ++l) {
      W[l] = b[l] = nullptr;
      ld[l] = 0;
      if (l >= s.L) continue;
      ld[l] = weight_ld(in);
      W[l] = at; b[l] = at + (int64_t)s.width(l) * ld[l]; at = b[l] + slot4(s.width(l));
      in = s.width(l);
    }
    W1 = W[0]; b1 = b[0]; W2 = W[1]; b2 = b[1]; ld1 = ld[0]; ldH = ld[1];
    Wh = at;
    head_stride = (int64_t)s.A * ldO + slot4(s.A);
  }
  T* head_w(int h) const { return Wh + h * head_stride; }
  T* head_b(int h) const { return head_w(h) + (int64_t)s.A * ldO; }
};
using ActorParams = ActorBlock<const float>;

struct CriticOffsets {
  int64_t W1, b1, W2, b2, w3, b3, count;
  int64_t W[kTorsoMaxLayers], b[kTorsoMaxLayers];   // layer l of any depth (W1 = W[0], W2 = W[1])
  int ld[kTorsoMaxLayers];
  int ld1, ldH, ldO;                             // ldO: pitch of the value head's row (last layer wide)
  explicit CriticOffsets(CriticShape s) : ldO(weight_ld(s.last())) {
    int64_t at = 0;
    int in = s.O + s.A;
    for (int l = 0; l < kTorsoMaxLayers; ++l) {
      W[l] = b[l] = 0;
      ld[l] = 0;
      if (l >= s.L) continue;
      ld[l] = weight_ld(in);
      W[l] = at; b[l] = at + (int64_t)s.width(l) * ld[l]; at = b[l] + slot4(s.width(l));
      in = s.width(l);
    }
    W1 = W[0]; b1 = b[0]; W2 = W[1]; b2 = b[1]; ld1 = ld[0]; ldH = ld[1];
    w3 = at; b3 = w3 + ldO; count = b3 + slot4(1);
  }
};

GemmArgs gemm(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N,
              int K) {
  GemmArgs g{};
  g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  g.alpha = 1.f;
  return g;
}

#define TRY(expr)                    \
  do {                               \
    const int rc__ = (expr);         \
    if (rc__ != TONIC_OK) return rc__; \
  } while (0)

// The fp16x2 weight images of a network (mlpimg.h): `block` = this network's (the first of `nets` critics,
// the others `v.bytes` on), `target` = its polyak target's (where the optimizer epilogue keeps those up to date),
// `second` = the images of a launch's second parameter set (critics_forward's params2).  Null block = float32 passes.
struct ActorImg { char* block; char* target; ActorImages v; };
struct CriticImg { char* block; char* target; char* second; CriticImages v; };

// build_weight_images: every image of one actor / of `nets` critics from the float32 parameters
void add_actor_images(ImgBuild& b, const float* params, ActorShape s, const ActorImg& img) {
  const ActorBlock<const float> p(params, s);
  b.add(p.W1, p.ld1, s.H, s.O, img.block, img.v.f1);
  b.add(p.W2, p.ldH, s.H, s.H, img.block, img.v.f2);
  b.add(p.W2, p.ldH, s.H, s.H, img.block, img.v.t2, true, 0, s.H);
  for (int h = 0; h < s.heads; ++h) {
    b.add(p.head_w(h), p.ldO, s.A, s.H, img.block, img.v.fh[h]);
    b.add(p.head_w(h), p.ldO, s.A, s.H, img.block, img.v.th[h], true, 0, s.H);
  }
}
void add_critic_images(ImgBuild& b, const float* params, CriticShape s, int nets, char* block,
                       const CriticImages& v) {
  const CriticOffsets o(s);
  for (int z = 0; z < nets; ++z) {
    const float* p = params + z * o.count;
    char* at = block + z * v.bytes;
    b.add(p + o.W1, o.ld1, s.H, s.O + s.A, at, v.f1);
    b.add(p + o.W2, o.ldH, s.H, s.H, at, v.f2);
    b.add(p + o.W2, o.ldH, s.H, s.H, at, v.t2, true, 0, s.H);
    b.add(p + o.W1, o.ld1, s.H, s.O + s.A, at, v.t1a, true, s.O, s.A);
  }
}
bool images_serve(int O, int A, int H) {
  return g_q_images.load() != 0 && H >= 16 && H <= 256 && H % 16 == 0 && A <= 64 &&
         mlp_image_pass_supported(O + A, H);
}

// actor torso + heads: h1, h2 [Bp, H]; head h -> out_h [Bp, ldh] (pre-activation unless `tanh_head`)
// What follows the heads (sampling / target noise / dense copy); folded into the forward launch
// when the fused kernel can (then *tail_done = true), else the caller launches its own kernel.
struct PolicyTail {
  int post;                    // PolicyPost
  const float* eps;
  float* actions; float* sigma; float* logp;
  float noise_scale, noise_clip;
  // optional: the critics' input rows [normalised observations | these actions] -> enc_out, and a
  // second pair from stored actions -> enc_out2 (see MlpFwdArgs)
  const float* enc_obs; const float* enc_obs2; const float* enc_act2;
  const float* enc_mean; const float* enc_std;
  float enc_clip;
  float* enc_out; float* enc_out2;
  int enc_ld;
};

// The fused form's arguments (a plain torso, mlp_forward_supported(H, A, heads)); tail != null: folded into the
// launch (mlp_policy_tail_supported(H, A)); img: the weight images the products run on (null, or a null block: none).
MlpFwdArgs actor_forward_args(const float* params, ActorShape s, const float* obs, int ldx, int B, float* h1,
                              float* h2, float* head0, float* head1, int ldh, bool tanh_head,
                              const PolicyTail* tail, const ActorImg* img) {
  const ActorParams p(params, s);
  MlpFwdArgs f{};
  f.X = obs; f.ldx = ldx; f.K1 = s.O;
  f.W1 = p.W1; f.b1 = p.b1; f.W2 = p.W2; f.b2 = p.b2; f.ldw1 = p.ld1; f.ldw2 = p.ldH;
  f.Wh[0] = p.head_w(0); f.bh[0] = p.head_b(0);
  f.Wh[1] = p.head_w(s.heads - 1); f.bh[1] = p.head_b(s.heads - 1);
  f.heads = s.heads; f.NH = s.A;
  f.h1 = h1; f.h2 = h2; f.ldh = s.hp();
  f.out[0] = head0; f.out[1] = s.heads == 2 ? head1 : head0; f.ldo = ldh;
  f.act[0] = tanh_head ? ACT_TANH : ACT_NONE; f.act[1] = ACT_NONE;
  f.B = B; f.H = s.H; f.split = 1 << 30;
  if (img != nullptr && img->block != nullptr)
    f.img = FwdImages{img->block, img->v.f1, img->v.f2, {img->v.fh[0], img->v.fh[s.heads - 1]}, 0, 0};
  if (tail != nullptr) {
    f.post = tail->post; f.post_eps = tail->eps; f.post_actions = tail->actions;
    f.post_sigma = tail->sigma; f.post_logp = tail->logp;
    f.noise_scale = tail->noise_scale; f.noise_clip = tail->noise_clip;
    f.scale_lo = s.scale_lo; f.scale_hi = s.scale_hi;
    f.enc_obs = tail->enc_obs; f.enc_obs2 = tail->enc_obs2; f.enc_act2 = tail->enc_act2;
    f.enc_mean = tail->enc_mean; f.enc_std = tail->enc_std; f.enc_clip = tail->enc_clip;
    f.enc_out = tail->enc_out; f.enc_out2 = tail->enc_out2; f.enc_O = s.O; f.enc_ld = tail->enc_ld;
  }
  return f;
}

int actor_forward(const float* params, ActorShape s, const float* obs, int B, float* h1,
                  float* h2, float* head0, float* head1, int ldh, bool tanh_head,
                  hipStream_t st, const PolicyTail* tail = nullptr, bool* tail_done = nullptr,
                  int ldx = 0, const ActorImg* img = nullptr, const CollectorStep* step = nullptr,
                  float* rows_out = nullptr, const BufferStoreArgs* store = nullptr) {
  ActorParams p(params, s);
  if (ldx <= 0) ldx = s.O;                      // dense observation rows unless told otherwise
  if (tail_done != nullptr) *tail_done = false;
  const int HP = s.hp();
  if (s.plain() && mlp_forward_supported(s.H, s.A, s.heads)) {      // one launch for torso + heads
    const bool fuse_tail = tail != nullptr && g_policy_tail != 0 && mlp_policy_tail_supported(s.H, s.A);
    MlpFwdArgs f = actor_forward_args(params, s, obs, ldx, B, h1, h2, head0, head1, ldh, tanh_head,
                                      fuse_tail ? tail : nullptr, img);
    if (step != nullptr) {       // a step of a collector's block: completion words, the rows' device copy
      f.done_flags = step->done_flags; f.done_seq = step->seq; f.rows_out = rows_out; f.rows_ld = s.O;
      if (store != nullptr) { f.store = *store; f.store_on = 1; }
    }
    if (tail_done != nullptr) *tail_done = fuse_tail;
    return launch_mlp_forward(f, 1, st);
  }
  // layer by layer: one launch per layer (bias + activation in the epilogue), then one per head
  GemmArgs g;
  for (int l = 0; l < s.L; ++l) {
    g = l == 0 ? gemm(obs, ldx, p.W[0], p.ld[0], h1, HP, B, s.H, s.O)
               : gemm(layer_at(h1, h2, l - 1), HP, p.W[l], p.ld[l], layer_at(h1, h2, l), HP, B, s.width(l),
                      s.width(l - 1));
    g.bias = p.b[l]; g.act = s.act;
    TRY(launch_gemm('c', 'c', g, 1, st));
  }
  const float* top = layer_at(h1, h2, s.L - 1);
  g = gemm(top, HP, p.head_w(0), p.ldO, head0, ldh, B, s.A, s.last());
  g.bias = p.head_b(0); g.act = tanh_head ? ACT_TANH : ACT_NONE;
  TRY(launch_gemm('c', 'c', g, 1, st));
  if (s.heads == 2) {
    g = gemm(top, HP, p.head_w(1), p.ldO, head1, ldh, B, s.A, s.last());
    g.bias = p.head_b(1);
    TRY(launch_gemm('c', 'c', g, 1, st));
  }
  return TONIC_OK;
}

// One policy pass: the forward with its tail, and — where the tail did not fuse — what the tail says as launches of
// their own: the stand-alone kernel of tail.post on the head outputs, then the critics' input rows (tail.enc_out; a
// second pair with tail.enc_out2).  The launch error, if any, is the caller's TONIC_CHECK_LAUNCH to report.
int policy_pass(const float* params, ActorShape s, const float* obs, int B, float* h1, float* h2, float* head0,
                float* head1, int ldh, bool tanh_head, hipStream_t st, const PolicyTail& tail,
                const ActorImg* img = nullptr) {
  bool tail_done = false;
  TRY(actor_forward(params, s, obs, B, h1, h2, head0, head1, ldh, tanh_head, st, &tail, &tail_done, 0, img));
  if (tail_done) return TONIC_OK;
  const int threads = 256, A = s.A;
  if (tail.post == POST_TARGET_NOISE) {
    hipLaunchKernelGGL(td3_target_action_kernel, dim3((B * A + threads - 1) / threads), dim3(threads), 0, st,
                       head0, ldh, tail.eps, tail.actions, B, A, tail.noise_scale, tail.noise_clip);
  } else if (tail.post == POST_COPY) {
    hipLaunchKernelGGL(copy_actions_kernel, dim3((B * A + threads - 1) / threads), dim3(threads), 0, st, head0,
                       ldh, tail.actions, B, A);
  } else {
    hipLaunchKernelGGL(sac_sample_kernel, dim3((B * sample_group(A) + threads - 1) / threads), dim3(threads), 0,
                       st, head0, head1, tail.eps, ldh, tail.actions, tail.logp, tail.sigma, B, A, sample_group(A),
                       s.scale_lo, s.scale_hi);
  }
  if (tail.enc_out != nullptr) {
    hipLaunchKernelGGL(encode_kernel, dim3((B * (s.O + A) + threads - 1) / threads, tail.enc_out2 != nullptr ? 2 : 1),
                       dim3(threads), 0, st, tail.enc_obs, tail.actions, tail.enc_mean, tail.enc_std, tail.enc_clip,
                       tail.enc_out, B, s.O, A, tail.enc_ld, tail.enc_obs2, tail.enc_act2, tail.enc_out2);
  }
  return TONIC_OK;
}

// `nets` critics batched over blockIdx.z; X shared ([Bp, ldx]); h1/h2 [nets][Bp][H]; q [nets][Bp]
// params2 / X2 != null: `nets` more critics (e.g. the online ones next to the targets) with their
// own input, appended to the same launch: h1/h2 [2 nets][Bp][H], q [2 nets][Bp].
// The fused form's arguments (mlp_forward_supported(H, 1, 1)); *launch_nets = networks in the launch.
MlpFwdArgs critics_forward_args(const float* params, CriticShape s, int nets, const float* X,
                                int ldx, int B, int Bp, float* h1, float* h2, float* q,
                                const float* params2, const float* X2, int* launch_nets,
                                const CriticImg* img = nullptr) {
  const CriticOffsets o(s);
  const int HP = weight_ld(s.H);
  MlpFwdArgs f{};
  f.X = X; f.ldx = ldx; f.K1 = s.O + s.A;
  f.W1 = params + o.W1; f.b1 = params + o.b1; f.W2 = params + o.W2; f.b2 = params + o.b2;
  f.ldw1 = o.ld1; f.ldw2 = o.ldH;
  f.Wh[0] = f.Wh[1] = params + o.w3; f.bh[0] = f.bh[1] = params + o.b3;
  f.heads = 1; f.NH = 1;
  f.h1 = h1; f.h2 = h2; f.ldh = HP; f.out[0] = f.out[1] = q; f.ldo = 1;
  f.act[0] = f.act[1] = ACT_NONE;
  f.B = B; f.H = s.H; f.split = 1 << 30;
  f.stride_params = o.count; f.stride_hidden = (int64_t)Bp * HP; f.stride_out = Bp;
  *launch_nets = nets;
  if (params2 != nullptr) {          // a second set of `nets` critics on a second input
    f.split = nets;
    f.second_params = (params2 - params) - (int64_t)nets * o.count;
    f.X2 = X2;
    *launch_nets = 2 * nets;
  }
  if (img != nullptr && img->block != nullptr) {
    f.img = FwdImages{img->block, img->v.f1, img->v.f2, {ImgView{}, ImgView{}}, img->v.bytes, 0};
    if (params2 != nullptr) f.img.second = (img->second - img->block) - (int64_t)nets * img->v.bytes;
  }
  return f;
}

int critics_forward(const float* params, CriticShape s, int nets, const float* X, int ldx, int B,
                    int Bp, float* h1, float* h2, float* q, hipStream_t st,
                    const float* params2 = nullptr, const float* X2 = nullptr,
                    const CriticImg* img = nullptr, const float* v_low = nullptr,
                    const float* v_high = nullptr) {      // (v_low / v_high: the Return normaliser's head, ValueRangeArg)
  const CriticOffsets o(s);
  const int in = s.O + s.A;
  const int HP = s.hp();
  const int64_t hs = (int64_t)Bp * HP;
  if (s.plain() && mlp_forward_supported(s.H, 1, 1)) {              // one launch for all `nets` critics
    int launch_nets = 0;
    MlpFwdArgs f = critics_forward_args(params, s, nets, X, ldx, B, Bp, h1, h2, q, params2,
                                        X2, &launch_nets, img);
    if (params2 != nullptr) f.hidden_from = nets;   // (the first set = the targets: forward only)
    return launch_mlp_forward(f, launch_nets, st, ValueRangeArg{v_low, v_high});
  }
  if (params2 != nullptr) {            // unfused path: one pass per parameter set
    TRY(critics_forward(params, s, nets, X, ldx, B, Bp, h1, h2, q, st, nullptr, nullptr, nullptr, v_low, v_high));
    return critics_forward(params2, s, nets, X2, ldx, B, Bp, h1 + nets * hs, h2 + nets * hs,
                           q + (int64_t)nets * Bp, st, nullptr, nullptr, nullptr, v_low, v_high);
  }
  GemmArgs g;
  for (int l = 0; l < s.L; ++l) {
    g = l == 0 ? gemm(X, ldx, params + o.W[0], o.ld[0], h1, HP, B, s.H, in)
               : gemm(layer_at(h1, h2, l - 1), HP, params + o.W[l], o.ld[l], layer_at(h1, h2, l), HP, B,
                      s.width(l), s.width(l - 1));
    g.bias = params + o.b[l]; g.act = s.act;
    g.strideA = l == 0 ? 0 : hs; g.strideB = o.count; g.strideBias = o.count; g.strideC = hs;
    TRY(launch_gemm('c', 'c', g, nets, st));
  }
  g = gemm(layer_at(h1, h2, s.L - 1), HP, params + o.w3, o.ldO, q, 1, B, 1, s.last());
  g.bias = params + o.b3;
  g.strideA = hs; g.strideB = o.count; g.strideBias = o.count; g.strideC = Bp;
  TRY(launch_gemm('c', 'c', g, nets, st, ValueRangeArg{v_low, v_high}));
  return TONIC_OK;
}

// Backward of `nets` critics from dq [nets][Bp].  grads != null: weight/bias gradient SUMS into
// the flat layout (stride = critic param count).  dxa != null: the ACTION columns of the input
// gradient, [nets][Bp][pad16(A)] (all the actor step needs of dX; the caller adds the critics).
// loss != null: dq is not given but FORMED from the forward outputs by the step's loss (LOSS_TD /
// LOSS_ACTOR / LOSS_REGRESSION, mlpfwd.h) and written to `dq`, the logged sums to loss->stats — inside the backward
// launch when the one-launch chain applies, by the stand-alone loss kernel otherwise.
struct StepLoss {
  int kind;                                   // LOSS_TD | LOSS_ACTOR | LOSS_REGRESSION
  const float* rewards; const float* discounts; const float* tq; const float* logp;
  float alpha;
  const float* q; float* stats;
  CriticLoss rule;                            // LOSS_TD, LOSS_REGRESSION: tonic_critic_loss_t (all-zero: MSE)
  const float* v_low; const float* v_high;    // the Return normaliser's head (q / tq are squashed values); null: plain
  const float* returns;                       // LOSS_REGRESSION: the targets [B] (one critic; all it reads beside q)
  TemperArg temper;                           // log_alpha != null (SAC, twin critics): exp(*log_alpha) stands for alpha
};

// The one-launch chain's arguments (mlp_backward_supported(H, 1, 0, dxa ? A : 0)).
MlpBwdArgs critics_chain_args(const float* params, CriticShape s, int nets, int B, int Bp,
                              const float* h1, const float* h2, float* dq, float* dh2, float* dh1,
                              float* dxa, const StepLoss* loss, const CriticImg* img = nullptr) {
  const CriticOffsets o(s);
  const int HP = weight_ld(s.H), ldxa = pad16(s.A);
  MlpBwdArgs b{};
  b.heads = 0; b.dq = dq; b.w3 = params + o.w3;
  if (loss) {
    b.loss = loss->kind; b.l_rewards = loss->rewards; b.l_discounts = loss->discounts;
    b.l_tq = loss->tq; b.l_logp = loss->logp; b.l_alpha = loss->alpha; b.l_q = loss->q;
    b.l_stats = loss->stats; b.l_nets = nets; b.l_Bp = Bp;
    b.l_tq_at = b.l_q_at = ValueLines{Bp, 16};
    b.l_kind = loss->rule.kind; b.l_param = loss->rule.param;
  }
  b.W2 = params + o.W2; b.W1 = params + o.W1; b.K1 = s.O + s.A; b.ldw1 = o.ld1; b.ldw2 = o.ldH;
  b.xa_first = s.O; b.xa_count = dxa ? s.A : 0;
  b.h1 = h1; b.h2 = h2; b.dz2 = dh2; b.dz1 = dh1; b.dxa = dxa; b.ldhid = HP;
  b.B = B; b.H = s.H;
  b.ldxa = ldxa;
  b.stride_params = o.count; b.stride_hidden = (int64_t)Bp * HP; b.stride_dq = Bp;
  b.stride_dxa = (int64_t)Bp * ldxa;
  if (img != nullptr && img->block != nullptr)
    b.img = BwdImages{img->block, img->v.t2, {ImgView{}, ImgView{}}, img->v.t1a, img->v.bytes};
  return b;
}

// The weight gradients of `nets` critics (all contract over the batch) in ONE launch:
//   dw3[1,H] = dq^T h2, db3 = sum dq ; dW2[H,H] = dz2^T h1, db2 ; dW1[H,in] = dz1^T X, db1
// (L layers: the value head, then dW_l = dz_l^T h_{l-1} from the top layer down; L + 1 problems)
int critics_weight_gradients(CriticShape s, int nets, const float* X, int ldx, int B, int Bp,
                             const float* h1, const float* h2, const float* dq, const float* dh2,
                             const float* dh1, float* grads, hipStream_t st, const AdamFold* fold,
                             const CriticImg* img = nullptr) {
  const CriticOffsets o(s);
  const int in = s.O + s.A;
  const int HP = s.hp();
  const int64_t hs = (int64_t)Bp * HP;
  GemmArgs w[kTorsoMaxLayers + 1];
  w[0] = gemm(dq, 1, layer_at(h1, h2, s.L - 1), HP, grads + o.w3, o.ldO, 1, s.last(), B);
  w[0].colsum = grads + o.b3; w[0].strideColsum = o.count;
  w[0].strideA = Bp; w[0].strideB = hs; w[0].strideC = o.count;
  for (int l = s.L - 1; l >= 0; --l) {
    GemmArgs& g = w[s.L - l];
    const float* dz = layer_at(dh2, dh1, s.L - 1 - l);
    g = l > 0 ? gemm(dz, HP, layer_at(h1, h2, l - 1), HP, grads + o.W[l], o.ld[l], s.width(l), s.width(l - 1), B)
              : gemm(dz, HP, X, ldx, grads + o.W[0], o.ld[0], s.H, in, B);
    g.colsum = grads + o.b[l]; g.strideColsum = o.count;
    g.strideA = hs; g.strideB = l > 0 ? hs : 0; g.strideC = o.count;
  }
  if (fold != nullptr && img != nullptr && img->block != nullptr) {      // (images: the plain torso, L == 2)
    // the optimizer epilogue keeps the stepped tensors' weight images (and their targets') up to date
    const int64_t to_target = img->target != nullptr ? img->target - img->block : 0;
    w[1].img = ImgTarget{img->block + img->v.f2.off, img->v.f2.chunks, img->block + img->v.t2.off,
                         img->v.t2.chunks, 0, s.H, img->v.bytes, to_target};
    w[2].img = ImgTarget{img->block + img->v.f1.off, img->v.f1.chunks, img->block + img->v.t1a.off,
                         img->v.t1a.chunks, s.O, s.A, img->v.bytes, to_target};
  }
  return launch_gemm_group('s', 's', w, s.L + 1, nets, st, fold);
}

int critics_backward(const float* params, CriticShape s, int nets, const float* X, int ldx, int B,
                     int Bp, const float* h1, const float* h2, float* dq, float* dh2,
                     float* dh1, float* grads, float* dxa, hipStream_t st,
                     const StepLoss* loss = nullptr, const AdamFold* fold = nullptr,
                     const CriticImg* img = nullptr) {
  const CriticOffsets o(s);
  const bool one_launch = s.plain() && mlp_backward_supported(s.H, 1, 0, dxa ? s.A : 0);
  if (loss && !one_launch) {
    if (loss->kind == LOSS_REGRESSION) {
      hipLaunchKernelGGL(regression_loss_kernel, dim3(1), dim3(1024), 0, st, loss->returns, loss->q, dq, loss->stats,
                         B, loss->rule, loss->v_low, loss->v_high);
    } else if (loss->temper.log_alpha != nullptr && loss->kind == LOSS_TD) {
      hipLaunchKernelGGL(critic_loss_tempered_kernel, dim3(1), dim3(1024), 0, st, loss->rewards,
                         loss->discounts, loss->tq, loss->logp, loss->temper.log_alpha, loss->q, dq,
                         loss->stats, B, Bp, nets, loss->rule, loss->v_low, loss->v_high);
    } else if (loss->temper.log_alpha != nullptr) {
      hipLaunchKernelGGL(actor_loss_tempered_kernel, dim3(1), dim3(1024), 0, st, loss->q, loss->logp,
                         loss->temper, nets == 2 ? 1 : 0, dq, loss->stats, B, Bp, loss->v_low, loss->v_high);
    } else if (loss->kind == LOSS_TD) {
      hipLaunchKernelGGL(critic_loss_kernel, dim3(1), dim3(1024), 0, st, loss->rewards,
                         loss->discounts, loss->tq, loss->logp, loss->alpha, loss->q, dq,
                         loss->stats, B, Bp, nets, loss->rule, loss->v_low, loss->v_high);
    } else {
      hipLaunchKernelGGL(actor_loss_kernel, dim3(1), dim3(1024), 0, st, loss->q, loss->logp,
                         loss->alpha, nets == 2 ? 1 : 0, dq, loss->stats, B, Bp, loss->v_low, loss->v_high);
    }
  }
  const int HP = s.hp();
  const int64_t hs = (int64_t)Bp * HP;
  const int ldxa = pad16(s.A);
  GemmArgs g;
  // the input-gradient chain first ...
  if (one_launch) {                                               // ... in ONE launch
    MlpBwdArgs b = critics_chain_args(params, s, nets, B, Bp, h1, h2, dq, dh2, dh1, dxa, loss, img);
    b.skip_dz = grads == nullptr ? 1 : 0;          // (a frozen critic's chain: only its action columns are read)
    if (loss && loss->temper.log_alpha != nullptr)
      TRY(launch_mlp_backward_tempered(b, nets, st, ValueRangeArg{loss->v_low, loss->v_high}, loss->temper));
    else TRY(launch_mlp_backward(b, nets, st, loss ? ValueRangeArg{loss->v_low, loss->v_high} : ValueRangeArg{nullptr, nullptr},
                            loss ? loss->returns : nullptr));
  } else {
    // dz_top = (dq w3) * act'(h_top)   (two layers: dz2, with h2)
    g = gemm(dq, 1, params + o.w3, o.ldO, dh2, HP, B, s.last(), 1);
    g.mask = layer_at(h1, h2, s.L - 1); g.ldmask = HP; g.mask_act = s.act;
    g.strideA = Bp; g.strideB = o.count; g.strideC = hs; g.strideMask = hs;
    TRY(launch_gemm('c', 's', g, nets, st));
    // dz_{l-1} = (dz_l W_l) * act'(h_{l-1})   (two layers: dz1 = (dz2 W2) * act'(h1))
    for (int l = s.L - 1; l >= 1; --l) {
      g = gemm(layer_at(dh2, dh1, s.L - 1 - l), HP, params + o.W[l], o.ld[l], layer_at(dh2, dh1, s.L - l), HP, B,
               s.width(l - 1), s.width(l));
      g.mask = layer_at(h1, h2, l - 1); g.ldmask = HP; g.mask_act = s.act;
      g.strideA = hs; g.strideB = o.count; g.strideC = hs; g.strideMask = hs;
      TRY(launch_gemm('c', 's', g, nets, st));
    }
    if (dxa) {     // dxa = dz1 W1[:, O : O + A]
      g = gemm(layer_at(dh2, dh1, s.L - 1), HP, params + o.W1 + s.O, o.ld1, dxa, ldxa, B, s.A, s.H);
      g.strideA = hs; g.strideB = o.count; g.strideC = (int64_t)Bp * ldxa;
      TRY(launch_gemm('c', 's', g, nets, st));
    }
  }
  if (grads)       // ... then the three weight gradients in ONE launch
    TRY(critics_weight_gradients(s, nets, X, ldx, B, Bp, h1, h2, dq, dh2, dh1, grads, st, fold, img));
  return TONIC_OK;
}

// One workspace, one layout type: its constructor performs the takes, in their order, and keeps the pointers.  A
// size query runs the same constructor over a workspace with a null base (measure) and returns `used`, so that no
// size is stated twice and no take sequence can outgrow what its query answered.
struct Workspace {
  char* base;                  // null: a size query — the takes only count
  int64_t used;
  float* take(int64_t floats) {
    float* p = base != nullptr ? reinterpret_cast<float*>(base + used) : nullptr;
    used += round_up(floats * 4, 256);
    return p;
  }
};
// the second of two arrays taken as one region (null with the region: a size query)
inline float* behind(float* p, int64_t floats) { return p != nullptr ? p + floats : nullptr; }
template <typename Layout, typename... Args>
int64_t measure(Args... args) {
  Workspace ws{nullptr, 0};
  const Layout layout(ws, args...);
  return ws.used;
}

// The six networks' image blocks [actor | target actor | two critics | two target critics] in 256-byte slots, carved
// from the END of a workspace's takes (so that nothing else moves).
struct ImageSet {
  ActorImg actor, target_actor;
  CriticImg critics, target_critics;       // (critics.second / .target = the targets and vice versa, as needed)
  bool on;
};
ImageSet take_images(Workspace& ws, int O, int A, int H, int heads, bool on) {
  ImageSet im{};
  im.on = on;
  if (!on) return im;
  const ActorImages av = actor_images(O, H, A, heads);
  const CriticImages cv = critic_images(O, A, H);
  char* a0 = reinterpret_cast<char*>(ws.take(round_up(av.bytes, 256) / 4));
  char* a1 = reinterpret_cast<char*>(ws.take(round_up(av.bytes, 256) / 4));
  char* c0 = reinterpret_cast<char*>(ws.take(round_up(2 * cv.bytes, 256) / 4));
  char* c1 = reinterpret_cast<char*>(ws.take(round_up(2 * cv.bytes, 256) / 4));
  im.actor = ActorImg{a0, a1, av};
  im.target_actor = ActorImg{a1, nullptr, av};
  im.critics = CriticImg{c0, c1, nullptr, cv};
  im.target_critics = CriticImg{c1, nullptr, c0, cv};
  return im;
}

// The layouts of tonic_offpolicy_workspace_bytes' four users.  H: the torso's own code (torso_code).  A network's
// hidden activations are ONE region of hidden_layers(H) layers (layer_at), hs floats each; `images`: the entry's
// run-time decision — the query measures with what a plain torso may ask for (a Gaussian policy's images).
struct PolicyForwardLayout {             // tonic_policy_forward
  float *h1, *h2, *head0, *head1;
  PolicyForwardLayout(Workspace& ws, int B, int A, int32_t H) {
    const int64_t Bp = pad16(B), hs = Bp * hidden_pitch(H);
    h1 = ws.take(hidden_layers(H) * hs); h2 = behind(h1, hs);
    head0 = ws.take(Bp * pad16(A)); head1 = ws.take(Bp * pad16(A));
  }
};
struct CollectorActLayout {              // tonic_collector_q_act (the fused forward: a plain torso)
  float *h1, *h2, *head0, *head1;
  CollectorActLayout(Workspace& ws, int B, int A, int32_t H) {
    const int64_t Bp = pad16(B), hs = Bp * hidden_pitch(H);
    h1 = ws.take(hs); h2 = ws.take(hs);
    head0 = ws.take(Bp * pad16(A)); head1 = ws.take(Bp * pad16(A));
  }
};
struct TwinQLayout {                     // the critic step (tonic_twin_q_grad*)
  float *a_h1, *a_h2, *head0, *head1, *next_act, *logp, *X, *X2, *h1_all, *h2_all, *q_all, *dq, *dh2, *dh1;
  ImageSet im;
  TwinQLayout(Workspace& ws, int B, int O, int A, int32_t H, int heads, bool images) {
    const int64_t Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), hs = Bp * hidden_pitch(H), L = hidden_layers(H);
    a_h1 = ws.take(L * hs); a_h2 = behind(a_h1, hs);
    head0 = ws.take(Bp * ldh); head1 = ws.take(Bp * ldh);
    next_act = ws.take(Bp * A); logp = ws.take(Bp);
    // target critics on (s', a') and online critics on (s, a) share ONE forward launch: inputs X /
    // X2, activations and values laid out [targets | online]
    X = ws.take(Bp * ldx); X2 = ws.take(Bp * ldx);
    h1_all = ws.take(L * 4 * hs); h2_all = behind(h1_all, 4 * hs);
    q_all = ws.take(4 * Bp);
    dq = ws.take(2 * Bp);
    dh2 = ws.take(L * 2 * hs); dh1 = behind(dh2, 2 * hs);
    im = take_images(ws, O, A, H, heads, images);
  }
};
struct ActorQLayout {                    // the actor step through the critics (tonic_actor_q_grad*)
  float *a_h1, *a_h2, *head0, *head1, *act, *sigma, *logp, *X, *c_h1, *c_h2, *q, *dq, *dh2, *dh1, *dxa, *dloc,
      *dspre, *da_h2, *da_h1;
  ImageSet im;
  ActorQLayout(Workspace& ws, int B, int O, int A, int32_t H, int heads, bool images) {
    const int64_t Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), hs = Bp * hidden_pitch(H), L = hidden_layers(H);
    a_h1 = ws.take(L * hs); a_h2 = behind(a_h1, hs);
    head0 = ws.take(Bp * ldh); head1 = ws.take(Bp * ldh);
    act = ws.take(Bp * A); sigma = ws.take(Bp * A);
    logp = ws.take(Bp);
    X = ws.take(Bp * ldx);
    c_h1 = ws.take(L * 2 * hs); c_h2 = behind(c_h1, 2 * hs);
    q = ws.take(2 * Bp); dq = ws.take(2 * Bp);
    dh2 = ws.take(L * 2 * hs); dh1 = behind(dh2, 2 * hs);
    dxa = ws.take(2 * Bp * ldh);                  // action columns of the critics' input gradients
    dloc = ws.take(Bp * ldh); dspre = ws.take(Bp * ldh);
    da_h2 = ws.take(L * hs); da_h1 = behind(da_h2, hs);
    im = take_images(ws, O, A, H, heads, images);
  }
};
// Regression of one critic on given returns (tonic_q_regression_grad): the critic's input, one network's activations,
// values and chain, and — `images` — this critic's weight images alone.  A query of its own
// (tonic_q_regression_workspace_bytes): every take is one TwinQLayout makes as well, at least as large.
struct QRegressionLayout {
  float *X, *h1, *h2, *q, *dq, *dh2, *dh1;
  CriticImg img;                         // block null: the float32 passes
  QRegressionLayout(Workspace& ws, int B, int O, int A, int32_t H, bool images) {
    const int64_t Bp = pad16(B), ldx = pitch16(O + A), hs = Bp * hidden_pitch(H), L = hidden_layers(H);
    X = ws.take(Bp * ldx);
    h1 = ws.take(L * hs); h2 = behind(h1, hs);
    q = ws.take(Bp); dq = ws.take(Bp);
    dh2 = ws.take(L * hs); dh1 = behind(dh2, hs);
    img = CriticImg{};
    if (images) {
      const CriticImages cv = critic_images(O, A, H);
      img = CriticImg{reinterpret_cast<char*>(ws.take(round_up(cv.bytes, 256) / 4)), nullptr, nullptr, cv};
    }
  }
};

}  // namespace
}  // namespace tonic

using namespace tonic;

extern "C" int64_t tonic_offpolicy_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H) {
  H = torso_code(H);
  // the largest of its four users' layouts, with the images wherever a torso may have them (a plain one: never by
  // the run-time switches — a query is a function of its arguments) and a Gaussian policy's two heads
  const bool images = hidden_plain(H);
  return std::max({measure<TwinQLayout>(B, O, A, H, 2, images), measure<ActorQLayout>(B, O, A, H, 2, images),
                   measure<PolicyForwardLayout>(B, A, H), measure<CollectorActLayout>(B, A, H)});
}

extern "C" int32_t tonic_mlp_weight_stride(int32_t cols) { return weight_ld(cols); }

extern "C" int64_t tonic_mlp_actor_param_count(int32_t O, int32_t H, int32_t A, int32_t heads) {
  return actor_count(actor_shape(O, H, A, heads));
}
extern "C" int64_t tonic_q_critic_param_count(int32_t O, int32_t A, int32_t H) {
  return critic_count(critic_shape(O, A, H));
}

// The `H` argument of the off-policy entries for a torso other than two ReLU layers of one width:
// MLP((H1, H2), activation) with activation 1 = ReLU, 2 = Tanh, 3 = ELU (GemmAct).  -1: not representable.
extern "C" int32_t tonic_mlp_hidden(int32_t H1, int32_t H2, int32_t activation) {
  if (H1 < 1 || H1 > 4095 || H2 < 1 || H2 > 4095 || activation < ACT_RELU || activation > ACT_ELU) return -1;
  if (H1 == H2 && activation == ACT_RELU) return H1;
  return kHiddenPacked | H1 | (H2 << 12) | (activation << 24);
}

namespace {
// MLP(sizes[0 .. layers), activation) as a descriptor, or false (tonic_last_error says why)
bool torso_descriptor(int32_t layers, const int32_t* sizes, int32_t activation, Torso* t) {
  if (layers < 1 || layers > kTorsoMaxLayers || sizes == nullptr || activation < ACT_RELU || activation > ACT_ELU) {
    set_error("tonic_mlp_torso: %d layers, activation %d (1 .. %d layers; 1 ReLU, 2 Tanh, 3 ELU)", layers,
              activation, kTorsoMaxLayers);
    return false;
  }
  *t = Torso{layers, {0, 0, 0, 0}, activation};
  for (int l = 0; l < layers; ++l) {
    if (sizes[l] < 1 || sizes[l] > 4095) {
      set_error("tonic_mlp_torso: layer %d has %d units (1 .. 4095)", l, sizes[l]);
      return false;
    }
    t->width[l] = sizes[l];
  }
  return true;
}
// the code of a descriptor in the process-wide table: the one it has, or a new one
int32_t registered_code(const Torso& t) {
  TorsoTable& table = torso_table();
  std::lock_guard<std::mutex> guard(table.lock);
  for (int i = 0; i < table.count; ++i) {
    const Torso& e = table.entry[i];
    bool same = e.L == t.L && e.act == t.act && e.scale_lo == t.scale_lo && e.scale_hi == t.scale_hi;
    for (int l = 0; l < kTorsoMaxLayers; ++l) same = same && e.width[l] == t.width[l];
    if (same) return kHiddenPacked | kTorsoRegistered | i;
  }
  if (table.count == kTorsoTableSize) {
    set_error("tonic_mlp_torso: %d distinct torsos registered already", kTorsoTableSize);
    return -1;
  }
  table.entry[table.count] = t;
  return kHiddenPacked | kTorsoRegistered | table.count++;
}
}  // namespace

// The `H` argument for MLP(sizes[0 .. layers), activation), 1 .. 4 layers: two layers give tonic_mlp_hidden's
// code; 1, 3 or 4 a descriptor registered in a process-wide table (the same torso: the same code).  Negative:
// not representable, or the table is full (tonic_last_error says which).
extern "C" int32_t tonic_mlp_torso(int32_t layers, const int32_t* sizes, int32_t activation) {
  Torso t;
  if (!torso_descriptor(layers, sizes, activation, &t)) return -1;
  if (layers == 2) return tonic_mlp_hidden(sizes[0], sizes[1], activation);
  return registered_code(t);
}

// ... for an ACTOR whose Gaussian head clamps its scale to [scale_min, scale_max] (GaussianPolicyHead, models/
// actors.py:69-98): the reference's defaults (1e-4, 1 as float32) give tonic_mlp_torso's code; other bounds register
// torso + bounds — two-layer torsos too — and every entry that forms a Gaussian scale from the code's actor clamps to
// them.  A critic ignores the bounds of the code it is given.  -1: the torso is not representable, the bounds are
// not 0 < scale_min <= scale_max (finite, as float32), or the table is full (tonic_last_error says which).
extern "C" int32_t tonic_mlp_torso_head(int32_t layers, const int32_t* sizes, int32_t activation, double scale_min,
                                        double scale_max) {
  const float lo = (float)scale_min, hi = (float)scale_max;              // what the kernels see
  if (!(lo > 0.f && lo <= hi && hi - hi == 0.f)) {
    set_error("tonic_mlp_torso_head: scale_min = %g, scale_max = %g (0 < scale_min <= scale_max, both finite)",
              scale_min, scale_max);
    return -1;
  }
  if (lo == kScaleMin && hi == kScaleMax) return tonic_mlp_torso(layers, sizes, activation);
  Torso t;
  if (!torso_descriptor(layers, sizes, activation, &t)) return -1;
  t.scale_lo = lo; t.scale_hi = hi;
  return registered_code(t);
}

// Policy forward for acting / evaluation.  kind: 0 = deterministic tanh head (TD3,
// actors.py:113-115), 1 = squashed Gaussian sample tanh(loc + sigma * eps) (SAC
// `_stochastic_actions`, sac.py:40-43; eps = NULL gives the greedy `loc` of sac.py:48-51).
extern "C" int tonic_policy_forward(const float* d_actor_params, const float* d_observations,
                                    const float* d_eps, float* d_actions, int32_t kind, int32_t B,
                                    int32_t O, int32_t H, int32_t A, void* d_workspace,
                                    int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_actor_params && d_observations && d_actions && d_workspace && B > 0 && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_policy_forward: bad argument");
  TONIC_REQUIRE(workspace_bytes >= tonic_offpolicy_workspace_bytes(B, O, A, H),
                TONIC_ERR_WORKSPACE, "tonic_policy_forward: workspace too small");
  hipStream_t st = as_stream(stream);
  const int ldh = pad16(A);
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const PolicyForwardLayout w(ws, B, A, H);
  const ActorShape s = actor_shape(O, H, A, kind == 0 ? 1 : 2);     // (with the scale's bounds of the code)
  const int threads = 256;
  if (kind == 2) {       // Gaussian head with a tanh loc (MPO, mpo.py:77-85): a = loc + sigma * eps
    TRY(actor_forward(d_actor_params, s, d_observations, B, w.h1, w.h2, w.head0, w.head1, ldh, true, st));
    hipLaunchKernelGGL(gaussian_sample_kernel, dim3((B * A + threads - 1) / threads), dim3(threads),
                       0, st, w.head0, w.head1, d_eps, ldh, d_actions, B, A, s.scale_lo, s.scale_hi);
    TONIC_CHECK_LAUNCH("tonic_policy_forward");
    return TONIC_OK;
  }
  PolicyTail tail{};
  tail.post = kind == 0 ? POST_COPY : POST_SQUASHED_SAMPLE; tail.eps = d_eps; tail.actions = d_actions;
  TRY(policy_pass(d_actor_params, s, d_observations, B, w.h1, w.h2, w.head0, w.head1, ldh, kind == 0, st, tail));
  TONIC_CHECK_LAUNCH("tonic_policy_forward");
  return TONIC_OK;
}

// Acting on a collector's block (the off-policy agents' step when the environment writes its observations into a
// shared pinned block, tonic_amd/collector.py): ONE launch reads the W observation rows in place (page-locked host
// memory, no staging copy), runs the policy of tonic_policy_forward (kind 0 deterministic tanh head, 1 squashed
// Gaussian: eps_slot 0 = the block's first noise field holds the standard-normal draws, -1 = the greedy loc), writes
// the actions into the block's second noise field (host-visible) and one completion word per 16 rows at system
// scope; the host waits with tonic_collector_wait_actions — no event, no copy back.  d_rows_out [W, O] (may be
// NULL): a device copy of the observation rows for the transition the agent stores after the environment's step
// (the block's own rows are overwritten by then).  replaces: tonic/torch/agents/ddpg.py:45-52,
// sac.py:40-51 (`_policy` / `_greedy_actions`) for observations that live in a collector block.
extern "C" int64_t tonic_mlp_actor_image_bytes(int32_t O, int32_t H, int32_t A, int32_t heads) {
  H = torso_code(H);
  if (!hidden_plain(H) || heads < 1 || heads > 2 || !images_serve(O, A, H) || !mlp_forward_supported(H, A, heads))
    return 0;
  return round_up(actor_images(O, H, A, heads).bytes, 256);
}

extern "C" int tonic_collector_q_act(tonic_collector_t* collector, const float* d_actor_params,
                                     void* d_actor_images, int32_t rebuild_images, int32_t kind,
                                     int32_t H, int32_t eps_slot, float* d_rows_out,
                                     const tonic_q_store_t* store, void* d_workspace,
                                     int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(collector && d_actor_params && d_actor_images && d_workspace && (kind == 0 || kind == 1),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_collector_q_act: bad argument");
  TONIC_REQUIRE(kind == 1 || eps_slot < 0, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_collector_q_act: the deterministic policy takes no noise");
  int64_t W; int O, A;
  collector_shape(collector, &W, &O, &A);      // (shapes first: nothing is opened before the arguments are known good)
  const ActorShape s = actor_shape(O, H, A, kind == 0 ? 1 : 2);
  H = torso_code(H);                           // (the bounds are in s; what follows sizes by the torso)
  TONIC_REQUIRE(tonic_mlp_actor_image_bytes(O, H, A, s.heads) > 0 && mlp_policy_tail_supported(s.H, s.A) &&
                    g_policy_tail != 0 && mlp_image_pass_supported(O, s.H),
                TONIC_ERR_UNSUPPORTED_SHAPE, "tonic_collector_q_act: O=%d H=%d A=%d outside the fused forward", O, H, A);
  TONIC_REQUIRE(workspace_bytes >= tonic_offpolicy_workspace_bytes((int32_t)W, O, A, H), TONIC_ERR_WORKSPACE,
                "tonic_collector_q_act: workspace too small");
  hipStream_t st = as_stream(stream);
  const int B = (int)W, ldh = pad16(A);
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const CollectorActLayout w(ws, B, A, H);
  // the actor's weight images (mlpimg.h): the caller's buffer, rebuilt here when it says the parameters moved
  const ActorImg img{static_cast<char*>(d_actor_images), nullptr, actor_images(O, s.H, A, s.heads)};
  if (rebuild_images != 0) {
    ImgBuild build;
    add_actor_images(build, d_actor_params, s, img);
    TRY(launch_build_images(build, st));
  }
  TONIC_REQUIRE(store == nullptr ||
                    (store->d_buf_observations && store->d_buf_actions && store->d_buf_next_observations &&
                     store->d_buf_rewards && store->d_buf_resets && store->d_buf_terminations &&
                     store->d_buf_discounts && store->d_observations && store->row >= 0),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_collector_q_act: bad store argument");
  CollectorStep step{};
  TRY(collector_begin_q_step(collector, eps_slot, store != nullptr ? 1 : 0, &step));
  BufferStoreArgs st_args{};
  if (store != nullptr) {      // the previous step's transition: the block's outcome fields, read in place
    st_args = BufferStoreArgs{store->d_buf_observations, store->d_buf_actions, store->d_buf_next_observations,
                              store->d_buf_rewards, store->d_buf_resets, store->d_buf_terminations,
                              store->d_buf_discounts, store->d_observations, step.actions, step.next_observations,
                              step.rewards, step.resets, step.terminations, store->d_norm_acc, store->row, W, O, A,
                              (float)store->discount_factor};
  }
  PolicyTail tail{};
  tail.post = kind == 0 ? POST_COPY : POST_SQUASHED_SAMPLE; tail.eps = step.eps; tail.actions = step.actions_out;
  bool tail_done = false;
  TRY(actor_forward(d_actor_params, s, step.observations, B, w.h1, w.h2, w.head0, w.head1, ldh, kind == 0, st,
                    &tail, &tail_done, 0, &img, &step, d_rows_out, store != nullptr ? &st_args : nullptr));
  TONIC_REQUIRE(tail_done, TONIC_ERR_UNSUPPORTED_SHAPE, "tonic_collector_q_act: the policy tail did not fuse");
  TONIC_CHECK_LAUNCH("tonic_collector_q_act");
  return TONIC_OK;
}

// Q-learning gradients.  kind 0 = TD3 (critics.py:156-175: target actor + clipped noise),
// 1 = SAC (critics.py:202-227: online actor sample, entropy term), 2 = DDPG (critics.py:68-86:
// ONE critic, target actor, no noise; gradient sums for [critic] + 8 statistics).  Writes gradient SUMS
// for [critic_1 | critic_2] + 8 statistics {sq_err_sum(both), q1_sum, q2_sum, 0, 0, B, 0, 0}
// into d_grad_sums; the caller follows with tonic_adam_step(grad_scale = 1/B).
// The rule of `loss=` (tonic_critic_loss_t): host-only validation.  NULL: MSE.
extern "C" int tonic_critic_loss_check(const tonic_critic_loss_t* loss) {
  if (loss == nullptr) return TONIC_OK;
  const int kind = loss->kind;
  TONIC_REQUIRE(kind >= TONIC_LOSS_MSE && kind <= TONIC_LOSS_HUBER, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_critic_loss_t: unknown kind %d (0 MSE, 1 L1, 2 smooth-L1, 3 Huber)", kind);
  if (kind == TONIC_LOSS_MSE || kind == TONIC_LOSS_L1) return TONIC_OK;      // (param is ignored)
  const float param = (float)loss->param;             // what the kernels see
  TONIC_REQUIRE(param - param == 0.f, TONIC_ERR_INVALID_ARGUMENT, "tonic_critic_loss_t: %s = %g is not finite",
                kind == TONIC_LOSS_HUBER ? "delta" : "beta", loss->param);
  TONIC_REQUIRE(kind != TONIC_LOSS_SMOOTH_L1 || param >= 0.f, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_critic_loss_t: smooth-L1 needs beta >= 0, got %g", loss->param);
  TONIC_REQUIRE(kind != TONIC_LOSS_HUBER || param > 0.f, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_critic_loss_t: Huber needs delta > 0, got %g", loss->param);
  return TONIC_OK;
}

namespace {
int twin_q_grad(int32_t kind, const float* d_policy_params, const float* d_target_critics, const float* d_critics,
                const float* d_norm_mean, const float* d_norm_std, double norm_clip, const float* d_observations,
                const float* d_actions, const float* d_next_observations, const float* d_rewards,
                const float* d_discounts, const float* d_eps, float* d_grad_sums, int32_t B, int32_t O, int32_t H,
                int32_t A, double entropy_coeff, double noise_scale, double noise_clip,
                const tonic_critic_loss_t* loss, const float* d_value_low, const float* d_value_high,
                void* d_workspace, int64_t workspace_bytes, void* stream,
                const float* d_log_entropy_coeff = nullptr) {
  TONIC_REQUIRE((d_value_low == nullptr) == (d_value_high == nullptr), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_twin_q_grad_ranged: %s is NULL and the other bound is not (both or neither)",
                d_value_low == nullptr ? "d_value_low" : "d_value_high");
  TONIC_REQUIRE(d_log_entropy_coeff == nullptr || kind == 1, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_tempered_twin_q_grad: kind %d has no entropy term (d_log_entropy_coeff goes with kind 1, SAC)",
                kind);
  TRY(tonic_critic_loss_check(loss));
  TONIC_REQUIRE(d_policy_params && d_target_critics && d_critics && d_norm_mean && d_norm_std && d_observations &&
                    d_actions && d_next_observations && d_rewards && d_discounts && (d_eps || kind == 2) &&
                    d_grad_sums && d_workspace && B > 0 && kind >= 0 && kind <= 2 && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_twin_q_grad: bad argument");
  TONIC_REQUIRE(workspace_bytes >= tonic_offpolicy_workspace_bytes(B, O, A, H), TONIC_ERR_WORKSPACE,
                "tonic_twin_q_grad: workspace too small");
  hipStream_t st = as_stream(stream);
  const ActorShape as = actor_shape(O, H, A, kind == 1 ? 2 : 1);
  H = torso_code(H);                           // (the bounds are in `as`; what follows sizes by the torso)
  const int Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A);
  const CriticShape cs = critic_shape(O, A, H);
  const int64_t Pc = critic_count(cs), hs = (int64_t)Bp * hidden_pitch(H);
  const int nets = kind == 2 ? 1 : 2;
  // the fused passes' weight images (mlpimg.h), formed from the float32 parameters by THIS call: the policy's,
  // the target critics' and the critics' — the same conversion as the fused iteration's, so the same bits
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const TwinQLayout w(ws, B, O, A, H, as.heads,
                      hidden_plain(H) && images_serve(O, A, H) && mlp_forward_supported(H, A, as.heads) &&
                          mlp_backward_supported(H, 1, 0, 0));
  const ImageSet& im = w.im;
  float* c_h1 = w.h1_all + nets * hs; float* c_h2 = w.h2_all + nets * hs;
  float* tq = w.q_all; float* q = w.q_all + (int64_t)nets * Bp;

  // ---- targets (no grad)
  if (im.on) {
    ImgBuild build;
    add_actor_images(build, d_policy_params, as, im.actor);
    add_critic_images(build, d_critics, cs, nets, im.critics.block, im.critics.v);
    add_critic_images(build, d_target_critics, cs, nets, im.target_critics.block, im.target_critics.v);
    TRY(launch_build_images(build, st));
  }
  // the policy's tail also encodes both critic inputs: (s', a') from its own actions -> X, the
  // stored (s, a) -> X2
  PolicyTail tail{};
  tail.post = kind == 0 ? POST_TARGET_NOISE : kind == 2 ? POST_COPY : POST_SQUASHED_SAMPLE;
  tail.eps = d_eps; tail.actions = w.next_act; tail.logp = kind == 1 ? w.logp : nullptr;
  tail.noise_scale = (float)noise_scale; tail.noise_clip = (float)noise_clip;
  tail.enc_obs = d_next_observations; tail.enc_obs2 = d_observations; tail.enc_act2 = d_actions;
  tail.enc_mean = d_norm_mean; tail.enc_std = d_norm_std; tail.enc_clip = clip_bound(norm_clip);
  tail.enc_out = w.X; tail.enc_out2 = w.X2; tail.enc_ld = ldx;
  TRY(policy_pass(d_policy_params, as, d_next_observations, B, w.a_h1, w.a_h2, w.head0, w.head1, ldh, kind != 1,
                  st, tail, im.on ? &im.actor : nullptr));
  // ---- the targets on (s', a') and the online critics on (s, a): one four-network forward
  TRY(critics_forward(d_target_critics, cs, nets, w.X, ldx, B, Bp, w.h1_all, w.h2_all, w.q_all, st,
                      d_critics, w.X2, im.on ? &im.target_critics : nullptr, d_value_low, d_value_high));
  const StepLoss td{LOSS_TD, d_rewards, d_discounts, tq, kind == 1 ? w.logp : (const float*)nullptr,
                    (float)entropy_coeff, q, d_grad_sums + nets * Pc, critic_loss_rule(loss),
                    d_value_low, d_value_high, nullptr, TemperArg{d_log_entropy_coeff, nullptr, 0.f}};
  TRY(critics_backward(d_critics, cs, nets, w.X2, ldx, B, Bp, c_h1, c_h2, w.dq, w.dh2, w.dh1, d_grad_sums,
                       nullptr, st, &td, nullptr, im.on ? &im.critics : nullptr));
  TONIC_CHECK_LAUNCH("tonic_twin_q_grad");
  return TONIC_OK;
}
}  // namespace

extern "C" int tonic_twin_q_grad(
    int32_t kind, const float* d_policy_params, const float* d_target_critics, const float* d_critics,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip, const float* d_observations,
    const float* d_actions, const float* d_next_observations, const float* d_rewards, const float* d_discounts,
    const float* d_eps, float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, double entropy_coeff,
    double noise_scale, double noise_clip, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return twin_q_grad(kind, d_policy_params, d_target_critics, d_critics, d_norm_mean, d_norm_std, norm_clip,
                     d_observations, d_actions, d_next_observations, d_rewards, d_discounts, d_eps, d_grad_sums, B, O,
                     H, A, entropy_coeff, noise_scale, noise_clip, nullptr, nullptr, nullptr, d_workspace,
                     workspace_bytes, stream);
}

// ... with the critic's loss (`loss=` of the reference's updaters, critics.py:58,142,189): NULL = MSE
extern "C" int tonic_twin_q_grad_loss(
    int32_t kind, const float* d_policy_params, const float* d_target_critics, const float* d_critics,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip, const float* d_observations,
    const float* d_actions, const float* d_next_observations, const float* d_rewards, const float* d_discounts,
    const float* d_eps, float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, double entropy_coeff,
    double noise_scale, double noise_clip, const tonic_critic_loss_t* loss, void* d_workspace,
    int64_t workspace_bytes, void* stream) {
  return twin_q_grad(kind, d_policy_params, d_target_critics, d_critics, d_norm_mean, d_norm_std, norm_clip,
                     d_observations, d_actions, d_next_observations, d_rewards, d_discounts, d_eps, d_grad_sums, B, O,
                     H, A, entropy_coeff, noise_scale, noise_clip, loss, nullptr, nullptr, d_workspace,
                     workspace_bytes, stream);
}

// ... for critics whose value heads squash into the Return normaliser's [low, high] (models/critics.py:17-19):
// online and target critics publish v, the TD loss, its gradient and the logged sums are those of v.  NULL / NULL:
// the plain heads, the launches and bits of tonic_twin_q_grad_loss.
extern "C" int tonic_twin_q_grad_ranged(
    int32_t kind, const float* d_policy_params, const float* d_target_critics, const float* d_critics,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip, const float* d_observations,
    const float* d_actions, const float* d_next_observations, const float* d_rewards, const float* d_discounts,
    const float* d_eps, float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, double entropy_coeff,
    double noise_scale, double noise_clip, const tonic_critic_loss_t* loss, const float* d_value_low,
    const float* d_value_high, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return twin_q_grad(kind, d_policy_params, d_target_critics, d_critics, d_norm_mean, d_norm_std, norm_clip,
                     d_observations, d_actions, d_next_observations, d_rewards, d_discounts, d_eps, d_grad_sums, B, O,
                     H, A, entropy_coeff, noise_scale, noise_clip, loss, d_value_low, d_value_high, d_workspace,
                     workspace_bytes, stream);
}

// ... SAC (kind 1) with a LEARNED entropy coefficient: d_log_entropy_coeff is one float32 on the device and the TD
// target's alpha is expf(*d_log_entropy_coeff), read by the kernels — the host never sees it, so a captured graph
// follows the coefficient as it moves.  NULL: tonic_twin_q_grad_ranged with `entropy_coeff`, launches and bits.
extern "C" int tonic_tempered_twin_q_grad(
    int32_t kind, const float* d_policy_params, const float* d_target_critics, const float* d_critics,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip, const float* d_observations,
    const float* d_actions, const float* d_next_observations, const float* d_rewards, const float* d_discounts,
    const float* d_eps, float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, double entropy_coeff,
    double noise_scale, double noise_clip, const tonic_critic_loss_t* loss, const float* d_value_low,
    const float* d_value_high, const float* d_log_entropy_coeff, void* d_workspace, int64_t workspace_bytes,
    void* stream) {
  return twin_q_grad(kind, d_policy_params, d_target_critics, d_critics, d_norm_mean, d_norm_std, norm_clip,
                     d_observations, d_actions, d_next_observations, d_rewards, d_discounts, d_eps, d_grad_sums, B, O,
                     H, A, entropy_coeff, noise_scale, noise_clip, loss, d_value_low, d_value_high, d_workspace,
                     workspace_bytes, stream, d_log_entropy_coeff);
}

// QRegression.__call__ (tonic/torch/updaters/critics.py:31-53): values = critic(s, a), loss(values, returns) on
// returns the caller computed — the encoder, the online critic's forward and its backward with LOSS_REGRESSION.
// No policy pass, no target network, no next observations; weight images of this critic only.  The routes are
// twin_q_grad's: images where images_serve says so, the float32 one-launch passes for any other plain torso, layer
// by layer otherwise.
extern "C" int64_t tonic_q_regression_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H) {
  H = torso_code(H);
  return measure<QRegressionLayout>(B, O, A, H, hidden_plain(H));      // (a function of its arguments, as above)
}

extern "C" int tonic_q_regression_grad(
    const float* d_critic, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_returns, float* d_grad_sums, int32_t B,
    int32_t O, int32_t H, int32_t A, const tonic_critic_loss_t* loss, const float* d_value_low,
    const float* d_value_high, void* d_workspace, int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE((d_value_low == nullptr) == (d_value_high == nullptr), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_q_regression_grad: %s is NULL and the other bound is not (both or neither)",
                d_value_low == nullptr ? "d_value_low" : "d_value_high");
  TRY(tonic_critic_loss_check(loss));
  TONIC_REQUIRE(d_critic && d_norm_mean && d_norm_std && d_observations && d_actions && d_returns && d_grad_sums &&
                    d_workspace && B > 0 && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_q_regression_grad: bad argument");
  TONIC_REQUIRE(workspace_bytes >= tonic_q_regression_workspace_bytes(B, O, A, H), TONIC_ERR_WORKSPACE,
                "tonic_q_regression_grad: workspace too small");
  hipStream_t st = as_stream(stream);
  H = torso_code(H);                           // (a head code's bounds: a critic ignores them)
  const int Bp = pad16(B), ldx = pitch16(O + A);
  const CriticShape cs = critic_shape(O, A, H);
  const int64_t Pc = critic_count(cs);
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const QRegressionLayout w(ws, B, O, A, H,
                            hidden_plain(H) && images_serve(O, A, H) && mlp_forward_supported(H, 1, 1) &&
                                mlp_backward_supported(H, 1, 0, 0));
  const CriticImg* img = w.img.block != nullptr ? &w.img : nullptr;
  if (img != nullptr) {
    ImgBuild build;
    add_critic_images(build, d_critic, cs, 1, w.img.block, w.img.v);
    TRY(launch_build_images(build, st));
  }
  const int threads = 256;
  hipLaunchKernelGGL(encode_kernel, dim3((B * (O + A) + threads - 1) / threads), dim3(threads), 0, st, d_observations,
                     d_actions, d_norm_mean, d_norm_std, clip_bound(norm_clip), w.X, B, O, A, ldx, nullptr, nullptr,
                     nullptr);
  TRY(critics_forward(d_critic, cs, 1, w.X, ldx, B, Bp, w.h1, w.h2, w.q, st, nullptr, nullptr, img, d_value_low,
                      d_value_high));
  const StepLoss regression{LOSS_REGRESSION, nullptr, nullptr, nullptr, nullptr, 0.f, w.q, d_grad_sums + Pc,
                            critic_loss_rule(loss), d_value_low, d_value_high, d_returns};
  TRY(critics_backward(d_critic, cs, 1, w.X, ldx, B, Bp, w.h1, w.h2, w.dq, w.dh2, w.dh1, d_grad_sums, nullptr, st,
                       &regression, nullptr, img));
  TONIC_CHECK_LAUNCH("tonic_q_regression_grad");
  return TONIC_OK;
}

namespace {

// Backward of an actor-shaped network (torso + `heads` linear heads) from the gradients at its head
// outputs: the input-gradient chain (dz2, dz1; optionally the columns [xa_first, xa_first + xa_count)
// of the input gradient -> dxa), then all weight / bias gradient SUMS into the flat layout `grads`
// (null: none — a frozen network) in one grouped launch.  X: the network's input rows, ldx apart.
MlpBwdArgs actor_chain_args(const float* params, ActorShape as, int B, const float* a_h1,
                            const float* a_h2, const float* dloc, const float* dspre, int ldh,
                            float* da_h2, float* da_h1, float* dxa, int xa_first, int xa_count,
                            const MlpBwdArgs* head_fold, const ActorImg* img = nullptr) {
  const int H = as.H, A = as.A, HP = as.hp();
  ActorParams p(params, as);
  MlpBwdArgs b{};
  b.heads = as.heads; b.NH = A; b.ldh = ldh;
  b.dhead[0] = dloc; b.dhead[1] = dspre ? dspre : dloc;
  b.Wh[0] = p.head_w(0); b.Wh[1] = p.head_w(as.heads - 1);
  b.W2 = p.W2; b.W1 = p.W1; b.K1 = as.O; b.ldw1 = p.ld1; b.ldw2 = p.ldH;
  b.xa_first = xa_first; b.xa_count = dxa ? xa_count : 0;
  b.h1 = a_h1; b.h2 = a_h2; b.dz2 = da_h2; b.dz1 = da_h1; b.dxa = dxa; b.ldhid = HP;
  b.ldxa = pad16(xa_count > 0 ? xa_count : 1);
  b.B = B; b.H = H;
  if (head_fold != nullptr) {          // dloc / dspre are FORMED by this launch (hb_* of MlpBwdArgs)
    b.hb_dxa0 = head_fold->hb_dxa0; b.hb_dxa1 = head_fold->hb_dxa1; b.hb_ldxa = head_fold->hb_ldxa;
    b.hb_act = head_fold->hb_act; b.hb_eps = head_fold->hb_eps; b.hb_sigma = head_fold->hb_sigma;
    b.hb_spre = head_fold->hb_spre; b.hb_sac = head_fold->hb_sac; b.hb_alpha = head_fold->hb_alpha;
    b.hb_scale_lo = as.scale_lo; b.hb_scale_hi = as.scale_hi;
  }
  if (img != nullptr && img->block != nullptr && b.xa_count == 0)     // (no image of W1^T's columns for actors)
    b.img = BwdImages{img->block, img->v.t2, {img->v.th[0], img->v.th[as.heads - 1]}, ImgView{}, 0};
  return b;
}

// All weight gradients of an actor-shaped network (they contract over the batch) in ONE launch:
//   dWh[A,H] = dhead^T h2, dbh (per head) ; dW2 = dz2^T h1, db2 ; dW1 = dz1^T X, db1
// (L layers: dW_l = dz_l^T h_{l-1} from the top layer down; heads + L problems, up to 6)
int actor_weight_gradients(ActorShape as, const float* X, int ldx, int B, const float* a_h1,
                           const float* a_h2, const float* dloc, const float* dspre, int ldh,
                           const float* da_h2, const float* da_h1, float* grads, hipStream_t st,
                           const AdamFold* fold, const ActorImg* img = nullptr) {
  const int H = as.H, A = as.A, HP = as.hp(), top = as.last();
  const ActorBlock<float> gp(grads, as);               // the gradient sums share the layout
  GemmArgs w[2 + kTorsoMaxLayers];
  int count = 0;
  // (images: the plain torso, L == 2)
  const bool images = fold != nullptr && img != nullptr && img->block != nullptr;
  const int64_t to_target = images && img->target != nullptr ? img->target - img->block : 0;
  for (int h = 0; h < as.heads; ++h) {
    const float* dhead = h == 0 ? dloc : dspre;
    w[count] = gemm(dhead, ldh, layer_at(a_h1, a_h2, as.L - 1), HP, gp.head_w(h), gp.ldO, A, top, B);
    if (images)
      w[count].img = ImgTarget{img->block + img->v.fh[h].off, img->v.fh[h].chunks, img->block + img->v.th[h].off,
                               img->v.th[h].chunks, 0, top, 0, to_target};
    w[count++].colsum = gp.head_b(h);
  }
  for (int l = as.L - 1; l >= 1; --l) {
    w[count] = gemm(layer_at(da_h2, da_h1, as.L - 1 - l), HP, layer_at(a_h1, a_h2, l - 1), HP, gp.W[l], gp.ld[l],
                    as.width(l), as.width(l - 1), B);
    if (images)
      w[count].img = ImgTarget{img->block + img->v.f2.off, img->v.f2.chunks, img->block + img->v.t2.off,
                               img->v.t2.chunks, 0, H, 0, to_target};
    w[count++].colsum = gp.b[l];
  }
  w[count] = gemm(layer_at(da_h2, da_h1, as.L - 1), HP, X, ldx, gp.W1, gp.ld1, H, as.O, B);
  if (images) w[count].img = ImgTarget{img->block + img->v.f1.off, img->v.f1.chunks, nullptr, 0, 0, 0, 0, to_target};
  w[count++].colsum = gp.b1;
  return launch_gemm_group('s', 's', w, count, 1, st, fold);
}

int actor_shaped_backward(const float* params, ActorShape as, const float* X, int ldx, int B,
                          const float* a_h1, const float* a_h2, const float* dloc,
                          const float* dspre, int ldh, float* da_h2, float* da_h1, float* grads,
                          float* dxa, int xa_first, int xa_count, hipStream_t st,
                          const MlpBwdArgs* head_fold = nullptr, const AdamFold* fold = nullptr,
                          const ActorImg* img = nullptr) {
  const int H = as.H, A = as.A, HP = as.hp();
  ActorParams p(params, as);
  GemmArgs g;
  // the input-gradient chain first: dz2 = (dloc Wloc [+ dspre Wscale]) * act'(h2) ; dz1
  if (as.plain() && mlp_backward_supported(H, A, as.heads, xa_count)) {
    const MlpBwdArgs b = actor_chain_args(params, as, B, a_h1, a_h2, dloc, dspre, ldh, da_h2, da_h1,
                                          dxa, xa_first, xa_count, head_fold, img);
    TRY(launch_mlp_backward(b, 1, st));
  } else {
    // (L layers: dz of the top layer from the heads, then dz_{l-1} = (dz_l W_l) * act'(h_{l-1}) down to dz1)
    for (int h = 0; h < as.heads; ++h) {
      const float* dhead = h == 0 ? dloc : dspre;
      g = gemm(dhead, ldh, p.head_w(h), p.ldO, da_h2, HP, B, as.last(), A);
      g.mask = layer_at(a_h1, a_h2, as.L - 1); g.ldmask = HP; g.accumulate = h > 0; g.mask_act = as.act;
      TRY(launch_gemm('c', 's', g, 1, st));
    }
    for (int l = as.L - 1; l >= 1; --l) {
      g = gemm(layer_at(da_h2, da_h1, as.L - 1 - l), HP, p.W[l], p.ld[l], layer_at(da_h2, da_h1, as.L - l), HP, B,
               as.width(l - 1), as.width(l));
      g.mask = layer_at(a_h1, a_h2, l - 1); g.ldmask = HP; g.mask_act = as.act;
      TRY(launch_gemm('c', 's', g, 1, st));
    }
    if (dxa) {
      g = gemm(layer_at(da_h2, da_h1, as.L - 1), HP, p.W1 + xa_first, p.ld1, dxa, pad16(xa_count), B, xa_count, H);
      TRY(launch_gemm('c', 's', g, 1, st));
    }
  }
  if (grads == nullptr) return TONIC_OK;
  return actor_weight_gradients(as, X, ldx, B, a_h1, a_h2, dloc, dspre, ldh, da_h2, da_h1, grads, st,
                                fold, img);
}

// Actor gradient through the (frozen) critics.  kind 0 = DeterministicPolicyGradient on
// critic_1 only (actors.py:170-189 with td3.py:36), 1 = TwinCriticSoftDeterministicPolicyGradient
// (actors.py:238-267).  Gradient SUMS for the actor + 8 statistics {loss_sum, 0.., B, ..}.
int actor_q_grad(int32_t kind, const float* d_actor_params, const float* d_critics, const float* d_norm_mean,
                 const float* d_norm_std, double norm_clip, const float* d_observations, const float* d_eps,
                 float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, double entropy_coeff,
                 const float* d_value_low, const float* d_value_high, void* d_workspace, int64_t workspace_bytes,
                 void* stream, TemperArg temper = TemperArg{nullptr, nullptr, 0.f}) {
  TONIC_REQUIRE((d_value_low == nullptr) == (d_value_high == nullptr), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_actor_q_grad_ranged: %s is NULL and the other bound is not (both or neither)",
                d_value_low == nullptr ? "d_value_low" : "d_value_high");
  TONIC_REQUIRE((temper.log_alpha == nullptr) == (temper.sums == nullptr), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_tempered_actor_q_grad: %s is NULL and the other is not (both or neither)",
                temper.log_alpha == nullptr ? "d_log_entropy_coeff" : "d_entropy_coeff_sums");
  TONIC_REQUIRE(temper.log_alpha == nullptr || kind == 1, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_tempered_actor_q_grad: kind %d has no entropy term (d_log_entropy_coeff goes with kind 1, SAC)",
                kind);
  TONIC_REQUIRE(temper.log_alpha == nullptr || temper.target_entropy - temper.target_entropy == 0.f,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_tempered_actor_q_grad: target_entropy is not finite");
  TONIC_REQUIRE(d_actor_params && d_critics && d_norm_mean && d_norm_std && d_observations &&
                    d_grad_sums && d_workspace && B > 0 && (kind == 0 || d_eps) && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_actor_q_grad: bad argument");
  TONIC_REQUIRE(workspace_bytes >= tonic_offpolicy_workspace_bytes(B, O, A, H),
                TONIC_ERR_WORKSPACE, "tonic_actor_q_grad: workspace too small");
  hipStream_t st = as_stream(stream);
  const ActorShape as = actor_shape(O, H, A, kind == 0 ? 1 : 2);
  H = torso_code(H);                           // (the bounds are in `as`; what follows sizes by the torso)
  const int Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), threads = 256;
  const int nets = kind == 0 ? 1 : 2;
  const CriticShape cs = critic_shape(O, A, H);
  const int64_t Pa = actor_count(as);
  // the weight images of the actor and the critics (mlpimg.h), formed by this call (see twin_q_grad)
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const ActorQLayout w(ws, B, O, A, H, as.heads,
                       hidden_plain(H) && images_serve(O, A, H) && mlp_forward_supported(H, A, as.heads) &&
                           mlp_backward_supported(H, A, as.heads, 0) && mlp_backward_supported(H, 1, 0, A));
  const ImageSet& im = w.im;
  if (im.on) {
    ImgBuild build;
    add_actor_images(build, d_actor_params, as, im.actor);
    add_critic_images(build, d_critics, cs, nets, im.critics.block, im.critics.v);
    TRY(launch_build_images(build, st));
  }

  PolicyTail tail{};                             // the tail also encodes the critics' input (s, a)
  tail.post = kind == 0 ? POST_COPY : POST_SQUASHED_SAMPLE; tail.eps = d_eps; tail.actions = w.act;
  tail.sigma = kind == 0 ? nullptr : w.sigma; tail.logp = kind == 0 ? nullptr : w.logp;
  tail.enc_obs = d_observations; tail.enc_mean = d_norm_mean; tail.enc_std = d_norm_std;
  tail.enc_clip = clip_bound(norm_clip); tail.enc_out = w.X; tail.enc_ld = ldx;
  TRY(policy_pass(d_actor_params, as, d_observations, B, w.a_h1, w.a_h2, w.head0, w.head1, ldh, kind == 0, st,
                  tail, im.on ? &im.actor : nullptr));
  TRY(critics_forward(d_critics, cs, nets, w.X, ldx, B, Bp, w.c_h1, w.c_h2, w.q, st, nullptr, nullptr,
                      im.on ? &im.critics : nullptr, d_value_low, d_value_high));
  const StepLoss objective{LOSS_ACTOR, nullptr, nullptr, nullptr, w.logp, (float)entropy_coeff, w.q,
                           d_grad_sums + Pa, CriticLoss{TONIC_LOSS_MSE, 0.f}, d_value_low, d_value_high, nullptr, temper};
  TRY(critics_backward(d_critics, cs, nets, w.X, ldx, B, Bp, w.c_h1, w.c_h2, w.dq, w.dh2, w.dh1, nullptr, w.dxa,
                       st, &objective, nullptr, im.on ? &im.critics : nullptr));
  if (temper.log_alpha != nullptr)
    hipLaunchKernelGGL(actor_head_backward_tempered_kernel, dim3((B * A + threads - 1) / threads), dim3(threads), 0, st,
                       w.dxa, w.dxa + (int64_t)Bp * ldh, ldh, w.act, d_eps, w.sigma, w.head1, ldh, temper.log_alpha,
                       w.dloc, w.dspre, B, A, as.scale_lo, as.scale_hi);
  else hipLaunchKernelGGL(actor_head_backward_kernel, dim3((B * A + threads - 1) / threads), dim3(threads), 0, st, w.dxa,
                     nets == 2 ? w.dxa + (int64_t)Bp * ldh : (float*)nullptr, ldh, w.act, d_eps, w.sigma, w.head1, ldh,
                     (float)entropy_coeff, kind == 1 ? 1 : 0, w.dloc, w.dspre, B, A, as.scale_lo, as.scale_hi);
  TRY(actor_shaped_backward(d_actor_params, as, d_observations, O, B, w.a_h1, w.a_h2, w.dloc,
                            kind == 1 ? w.dspre : nullptr, ldh, w.da_h2, w.da_h1, d_grad_sums, nullptr, 0, 0, st,
                            nullptr, nullptr, im.on ? &im.actor : nullptr));
  TONIC_CHECK_LAUNCH("tonic_actor_q_grad");
  return TONIC_OK;
}

}  // namespace

extern "C" int tonic_actor_q_grad(
    int32_t kind, const float* d_actor_params, const float* d_critics, const float* d_norm_mean,
    const float* d_norm_std, double norm_clip, const float* d_observations, const float* d_eps, float* d_grad_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, double entropy_coeff, void* d_workspace, int64_t workspace_bytes,
    void* stream) {
  return actor_q_grad(kind, d_actor_params, d_critics, d_norm_mean, d_norm_std, norm_clip, d_observations, d_eps,
                      d_grad_sums, B, O, H, A, entropy_coeff, nullptr, nullptr, d_workspace, workspace_bytes, stream);
}

// ... through critics whose value heads squash (tonic_twin_q_grad_ranged): the objective and its logged sum are
// those of v, the gradient that enters each head is multiplied by dv/dz.  NULL / NULL: tonic_actor_q_grad.
extern "C" int tonic_actor_q_grad_ranged(
    int32_t kind, const float* d_actor_params, const float* d_critics, const float* d_norm_mean,
    const float* d_norm_std, double norm_clip, const float* d_observations, const float* d_eps, float* d_grad_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, double entropy_coeff, const float* d_value_low,
    const float* d_value_high, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return actor_q_grad(kind, d_actor_params, d_critics, d_norm_mean, d_norm_std, norm_clip, d_observations, d_eps,
                      d_grad_sums, B, O, H, A, entropy_coeff, d_value_low, d_value_high, d_workspace, workspace_bytes,
                      stream);
}

// ... SAC (kind 1) with a LEARNED entropy coefficient (tonic_tempered_twin_q_grad): alpha = expf(*d_log_entropy_coeff)
// in the objective, its logged sum and the head backward, and the coefficient's own block
// d_entropy_coeff_sums [1 + 8] = {-sum(logp + target_entropy) | -log_alpha sum(logp + target_entropy), sum logp,
// alpha B, 0, 0, B, 0, 0} from the log-probabilities of THIS step's sample (formed by the workgroup that forms the
// objective's logged sum: no launch more) — the gradient SUM of J = -mean(log_alpha (logp + target_entropy)) and its
// statistics, stepped by tonic_optimizer_step on a block of one.  Both pointers or neither; NULL / NULL:
// tonic_actor_q_grad_ranged with `entropy_coeff`, launches and bits.
extern "C" int tonic_tempered_actor_q_grad(
    int32_t kind, const float* d_actor_params, const float* d_critics, const float* d_norm_mean,
    const float* d_norm_std, double norm_clip, const float* d_observations, const float* d_eps, float* d_grad_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, double entropy_coeff, const float* d_value_low,
    const float* d_value_high, const float* d_log_entropy_coeff, float* d_entropy_coeff_sums, double target_entropy,
    void* d_workspace, int64_t workspace_bytes, void* stream) {
  return actor_q_grad(kind, d_actor_params, d_critics, d_norm_mean, d_norm_std, norm_clip, d_observations, d_eps,
                      d_grad_sums, B, O, H, A, entropy_coeff, d_value_low, d_value_high, d_workspace, workspace_bytes,
                      stream, TemperArg{d_log_entropy_coeff, d_entropy_coeff_sums, (float)target_entropy});
}

// ------------------------------------------------------------------ one whole learner iteration
// ddpg.py:95-112 / td3.py:38-55 / sac.py with the launches of the two updaters merged where they do
// not depend on each other, and the optimizer steps folded into the weight-gradient launches:
//   1  policy passes of BOTH steps: net 0 = the critic step's policy on s' (TD3 / DDPG: target actor
//      [+ clipped noise], SAC: online actor sample + log-prob) whose tail also encodes the critics'
//      inputs (s', a') and (s, a); net 1 (actor due) = the online actor on s with the actor step's
//      sample, whose tail encodes (s, a_new).  The critic step does not touch the actor, so net 1
//      sees the parameters the reference's actor step would see.
//   2  target critics on (s', a') + online critics on (s, a)
//   3  TD loss + the online critics' input-gradient chain
//   4  the critics' weight gradients + Adam [+ polyak of the critics when the targets move]
//   5  (actor due) the UPDATED critics on (s, a_new)
//   6  actor objective + the critics' chain down to the action columns
//   7  head backward + the actor's input-gradient chain
//   8  the actor's weight gradients + Adam + polyak of the actor
// 13 launches of the split path (gather, 4 forwards, 3 backwards, head backward, 2 weight-gradient
// groups, 2 optimizer launches) become 8 (4 when the actor is not due).
namespace {

// The one word of the chained launches that must be ZERO when a launch starts (a reader sets it when
// a value never came, the launch's last workgroup reports and clears it) lives at the START of the
// workspace, so that it stays where it is whatever batch size the workspace is used with next.
constexpr int64_t kChainSyncArea = 64;               // floats

// Everything launch 1 writes — the chained launches' exchange area (the value lines of the tiles, then the
// critics' action-column gradients: ONE span, emptied by the policy launch of every iteration), the policy
// passes' activations and head outputs [net 0 | net 1], the actions / log-probabilities, the critics' input
// rows — twice: an iteration works on set `slot`, the passes it runs ahead for the next one on the other
struct PolicySet {
  float *xq, *dxa, *exchange_end, *p_h1, *p_h2, *head0, *head1, *next_act, *logp_next, *act, *sigma, *logp,
      *X, *X2, *X3;
};
// tonic_q_iteration's workspace (H: a plain width): the failure words first, the images last
struct QIterationLayout {
  // (one failure word per set: the passes that run ahead clear THEIR word while this iteration's launches may set its)
  unsigned* failed_words;
  PolicySet sets[2];
  float *h1_all, *h2_all, *q_all, *dq, *dh2, *dh1, *dloc, *dspre, *da_h2, *da_h1;
  ImageSet im;
  QIterationLayout(Workspace& ws, int B, int O, int A, int H, int heads, bool images) {
    const int64_t Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), hs = Bp * weight_ld(H);
    failed_words = reinterpret_cast<unsigned*>(ws.take(kChainSyncArea));
    for (PolicySet& t : sets) {
      t.xq = ws.take((Bp / 16) * kExchangeTileFloats);
      t.dxa = ws.take(2 * Bp * ldh);
      t.exchange_end = ws.take(0);
      t.p_h1 = ws.take(2 * hs); t.p_h2 = ws.take(2 * hs);
      t.head0 = ws.take(2 * Bp * ldh); t.head1 = ws.take(2 * Bp * ldh);
      t.next_act = ws.take(Bp * A); t.logp_next = ws.take(Bp);
      t.act = ws.take(Bp * A); t.sigma = ws.take(Bp * A);
      t.logp = ws.take(Bp);
      t.X = ws.take(Bp * ldx); t.X2 = ws.take(Bp * ldx);
      t.X3 = ws.take(Bp * ldx);
    }
    h1_all = ws.take(4 * hs); h2_all = ws.take(4 * hs);
    q_all = ws.take(4 * Bp);
    dq = ws.take(2 * Bp);
    dh2 = ws.take(2 * hs); dh1 = ws.take(2 * hs);
    dloc = ws.take(Bp * ldh); dspre = ws.take(Bp * ldh);
    da_h2 = ws.take(hs); da_h1 = ws.take(hs);
    im = take_images(ws, O, A, H, heads, images);
  }
};

// torch.optim.Adam of one block (`n` parameters at `params`) in the epilogue of its weight-gradient launch
AdamFold adam_fold(const tonic_q_optimizer& o, float* params, int64_t n, float grad_scale, int stats_kind,
                   const unsigned* skip) {
  AdamFold f{};
  f.grads = o.d_grad_sums; f.params = params; f.exp_avg = o.d_exp_avg;
  f.exp_avg_sq = o.d_exp_avg_sq; f.state = o.d_state; f.n = n;
  f.grad_scale = grad_scale; f.beta2 = (float)o.beta2; f.eps = (float)o.eps;
  f.beta1_d = o.beta1; f.beta2_d = o.beta2; f.lr_d = o.lr;
  f.stats_kind = stats_kind; f.info_row = o.d_info_row; f.consts = o.d_step_constants;
  f.skip = skip;
  return f;
}

}  // namespace

extern "C" int64_t tonic_q_iteration_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H) {
  return measure<QIterationLayout>(B, O, A, torso_code(H), 2, true);       // (the images: always, a Gaussian policy's)
}

extern "C" int tonic_q_iteration_ahead_supported(int32_t B, int32_t O, int32_t H, int32_t A, int32_t nets,
                                                 int32_t passes) {
  if (B <= 0 || nets < 1 || nets > 2 || passes < 1 || passes > 2) return 0;
  H = torso_code(H);
  if (g_q_chain.load() == 0 || !hidden_plain(H) || !images_serve(O, A, H) || !mlp_image_pass_supported(O, H)) return 0;
  const int tiles = (B + 15) / 16;
  return tiles * (2 * nets + passes) + 1 <= 256;      // one workgroup per compute unit: all of them at once
}

extern "C" int tonic_q_iteration_supported(int32_t O, int32_t H, int32_t A, int32_t heads) {
  H = torso_code(H);
  return hidden_plain(H) && mlp_forward_supported(H, A, heads) && mlp_policy_tail_supported(H, A) &&
         mlp_forward_supported(H, 1, 1) && mlp_backward_supported(H, 1, 0, A) &&
         mlp_backward_supported(H, A, heads, 0) && O > 0 ? 1 : 0;
}

extern "C" int tonic_q_iteration(const tonic_q_iteration_t* it, void* stream) {
  TONIC_REQUIRE(it != nullptr, TONIC_ERR_INVALID_ARGUMENT, "tonic_q_iteration: null arguments");
  const tonic_q_iteration_t& a = *it;
  TRY(tonic_critic_loss_check(&a.critic_loss));
  const int kind = a.kind, B = a.B, O = a.O, H = torso_code(a.H), A = a.A;     // (a.H: also the scale's bounds)
  const bool due = a.actor_due != 0;
  const int phase = a.phase;                 // 0 whole iteration | 1 critic half | 2 actor half (sums only)
  TONIC_REQUIRE(phase >= 0 && phase <= 2 && (phase != 2 || due), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_q_iteration: phase %d (actor_due %d)", phase, (int)due);
  const int stage = a.stage, slot = a.slot;  // 0 whole | 2 behind the policy passes; the set of launch-1 outputs
  TONIC_REQUIRE((stage == 0 || stage == 2) && (stage == 0 || phase == 0) && (slot == 0 || slot == 1),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_q_iteration: stage %d, slot %d (phase %d)", stage, slot, phase);
  const tonic_q_iteration_t* next = a.ahead;           // the iteration whose policy passes ride in this critic step
  TONIC_REQUIRE(next == nullptr ||
                    (phase == 0 && !due && next->kind == kind && next->B == B && next->O == O && next->H == a.H &&
                     next->A == A && next->slot == (slot ^ 1) && next->d_workspace == a.d_workspace &&
                     next->d_actor == a.d_actor && next->d_target_actor == a.d_target_actor &&
                     next->d_next_observations && next->d_observations && next->d_actions &&
                     (next->d_eps_critic || kind == 2) && (next->d_eps_actor || kind != 1 || !next->actor_due) &&
                     tonic_q_iteration_ahead_supported(B, O, H, A, kind == 2 ? 1 : 2, next->actor_due ? 2 : 1)),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_q_iteration: policy passes ahead (actor_due %d)", (int)due);
  TONIC_REQUIRE(kind >= 0 && kind <= 2 && B > 0 && a.d_actor && a.d_critics && a.d_target_actor &&
                    a.d_target_critics && a.d_norm_mean && a.d_norm_std && a.d_observations &&
                    a.d_actions && a.d_next_observations && a.d_rewards && a.d_discounts &&
                    (a.d_eps_critic || kind == 2) && (a.d_eps_actor || kind != 1 || !due) &&
                    a.critic.d_grad_sums && a.critic.d_exp_avg && a.critic.d_exp_avg_sq &&
                    a.critic.d_state && a.actor.d_grad_sums && a.actor.d_exp_avg &&
                    a.actor.d_exp_avg_sq && a.actor.d_state && a.d_workspace,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_q_iteration: bad argument");
  const int heads = kind == 1 ? 2 : 1;
  TONIC_REQUIRE(tonic_q_iteration_supported(O, H, A, heads), TONIC_ERR_UNSUPPORTED_SHAPE,
                "tonic_q_iteration: O=%d H=%d A=%d outside the fused kernels", O, H, A);
  TONIC_REQUIRE(a.workspace_bytes >= tonic_q_iteration_workspace_bytes(B, O, A, H),
                TONIC_ERR_WORKSPACE, "tonic_q_iteration: workspace too small");
  hipStream_t st = as_stream(stream);
  const int Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), HP = weight_ld(H);
  const int nets = kind == 2 ? 1 : 2;                  // critics
  const CriticShape cs{O, A, H};
  const ActorShape as = actor_shape(O, a.H, A, heads);
  const int64_t Pc = critic_count(cs), Pa = actor_count(as), hs = (int64_t)Bp * HP;
  Workspace ws{static_cast<char*>(a.d_workspace), 0};
  const QIterationLayout w(ws, B, O, A, H, heads, images_serve(O, A, H));
  unsigned* failed = w.failed_words + slot;
  const PolicySet& mine = w.sets[slot];
  const bool chain = g_q_chain.load() != 0;
  float* c_h1 = w.h1_all + nets * hs; float* c_h2 = w.h2_all + nets * hs;
  float* tq = w.q_all; float* q = w.q_all + (int64_t)nets * Bp;
  // the weight images of the six networks (mlpimg.h): rebuilt from the float32 parameters when the caller says
  // they may have changed since this workspace last saw them (the first iteration of an update call; every call
  // in phases, where the caller's own optimizer launches step the parameters), kept up to date by the optimizer
  // epilogues of this call otherwise
  const ImageSet& im = w.im;
  if (im.on && (a.refresh_images != 0 || phase != 0)) {
    ImgBuild build;
    add_actor_images(build, a.d_actor, as, im.actor);
    add_actor_images(build, a.d_target_actor, as, im.target_actor);
    add_critic_images(build, a.d_critics, cs, nets, im.critics.block, im.critics.v);
    add_critic_images(build, a.d_target_critics, cs, nets, im.target_critics.block, im.target_critics.v);
    TRY(launch_build_images(build, st));
  }
  const ActorImg* actor_img = im.on ? &im.actor : nullptr;
  const CriticImg* critics_img = im.on ? &im.critics : nullptr;

  // ---- 1: the policy passes (of iteration `it` into set `t`: this one's, or the next one's ahead of time)
  auto policy_passes = [&](const tonic_q_iteration_t& it, const PolicySet& t, unsigned* failed_word) {
    const bool it_due = it.actor_due != 0;
    const float* policy = kind == 1 ? it.d_actor : it.d_target_actor;
    PolicyTail tail{};           // net 0: the critic step's policy on s', its tail encodes (s', a') and (s, a)
    tail.post = kind == 0 ? POST_TARGET_NOISE : kind == 2 ? POST_COPY : POST_SQUASHED_SAMPLE;
    tail.eps = it.d_eps_critic; tail.actions = t.next_act; tail.logp = kind == 1 ? t.logp_next : nullptr;
    tail.noise_scale = (float)it.noise_scale; tail.noise_clip = (float)it.noise_clip;
    tail.enc_obs = it.d_next_observations; tail.enc_obs2 = it.d_observations; tail.enc_act2 = it.d_actions;
    tail.enc_mean = it.d_norm_mean; tail.enc_std = it.d_norm_std; tail.enc_clip = clip_bound(it.norm_clip);
    tail.enc_out = t.X; tail.enc_out2 = t.X2; tail.enc_ld = ldx;
    const ActorImg* pi = !im.on ? nullptr : kind == 1 ? &im.actor : &im.target_actor;
    MlpFwdArgs f = actor_forward_args(policy, as, it.d_next_observations, O, B, t.p_h1, t.p_h2, t.head0, t.head1,
                                      ldh, kind != 1, &tail, pi);
    f.stride_hidden = hs; f.stride_out = (int64_t)Bp * ldh;
    // (phases: the failure word is the caller's to clear — it stands for the whole update)
    if (chain) { f.reset_area = t.xq; f.reset_floats = t.exchange_end - t.xq; f.reset_failed = phase == 0 ? failed_word : nullptr; }
    if (it_due) {
      f.split = 1;
      f.second_params = it.d_actor - policy;           // (0 for SAC: the same network on s)
      f.X2 = it.d_observations;
      f.tail2.post = kind == 1 ? POST_SQUASHED_SAMPLE : POST_COPY;
      f.tail2.eps = kind == 1 ? it.d_eps_actor : nullptr;
      f.tail2.actions = t.act; f.tail2.sigma = kind == 1 ? t.sigma : nullptr;
      f.tail2.logp = kind == 1 ? t.logp : nullptr;
      f.tail2.enc_obs = it.d_observations; f.tail2.enc_out = t.X3;
    }
    if (pi != nullptr) {
      if (it_due) f.img.second = im.actor.block - pi->block;
      f.hidden_from = 1;             // (net 0, the critic step's policy, has no backward)
    }
    return f;
  };
  if (phase != 2 && stage != 2) TRY(launch_mlp_forward(policy_passes(a, mine, failed), due ? 2 : 1, st));
  // ---- 2: targets on (s', a') and online critics on (s, a)
  // ---- 3 + 4: TD loss, backward chain, weight gradients + Adam (+ polyak of the critics)
  const float grad_scale = (float)(1.0 / (a.global_batch > 0 ? a.global_batch : B));
  AdamFold cf = adam_fold(a.critic, a.d_critics, nets * Pc, grad_scale, 3, chain ? failed : nullptr);
  if (due) {
    cf.target = a.d_target_critics;
    cf.polyak_keep = (float)(1.0 - a.target_coeff); cf.polyak_mix = (float)a.target_coeff;
  }
  const StepLoss td{LOSS_TD, a.d_rewards, a.d_discounts, tq,
                    kind == 1 ? mine.logp_next : (const float*)nullptr, (float)a.critic_entropy_coeff, q,
                    a.critic.d_grad_sums + nets * Pc, critic_loss_rule(&a.critic_loss)};
  const AdamFold* critic_fold = phase == 0 ? &cf : nullptr;       // phases: gradient sums only
  if (phase == 2) {
    // (the critic half ran in an earlier call)
  } else if (chain) {
    // 2 + 3 as ONE launch: the online critics' workgroups go on to the TD loss and their chain as
    // soon as the targets of their 16 rows have arrived (q_critic_step_kernel)
    QCriticStep step{};
    int launch_nets = 0;
    step.fwd = critics_forward_args(a.d_target_critics, cs, nets, mine.X, ldx, B, Bp, w.h1_all, w.h2_all,
                                    w.q_all, a.d_critics, mine.X2, &launch_nets, im.on ? &im.target_critics : nullptr);
    step.fwd.xq = mine.xq;
    step.fwd.hidden_from = nets;     // (the targets: forward only)
    step.bwd = critics_chain_args(a.d_critics, cs, nets, B, Bp, c_h1, c_h2, w.dq, w.dh2, w.dh1, nullptr, &td,
                                  critics_img);
    step.bwd.exchange_failed = failed;   // targets: lines 0, 1 of the tile; the online critics: lines 2, 3
    step.bwd.l_tq = mine.xq; step.bwd.l_tq_at = ValueLines{32, kExchangeTileFloats};
    step.bwd.l_q = mine.xq + 64; step.bwd.l_q_at = ValueLines{32, kExchangeTileFloats};
    step.nets = nets;
    if (next != nullptr) {            // the next iteration's policy passes: more workgroups of this launch
      step.ahead = policy_passes(*next, w.sets[slot ^ 1], w.failed_words + (slot ^ 1));
      step.ahead_nets = next->actor_due ? 2 : 1;
    }
    TRY(launch_q_critic_step(step, st));
    TRY(critics_weight_gradients(cs, nets, mine.X2, ldx, B, Bp, c_h1, c_h2, w.dq, w.dh2, w.dh1,
                                 a.critic.d_grad_sums, st, critic_fold, critics_img));
  } else {
    TONIC_REQUIRE(next == nullptr, TONIC_ERR_INVALID_ARGUMENT, "tonic_q_iteration: passes ahead need the chained launches");
    TRY(critics_forward(a.d_target_critics, cs, nets, mine.X, ldx, B, Bp, w.h1_all, w.h2_all, w.q_all, st,
                        a.d_critics, mine.X2, im.on ? &im.target_critics : nullptr));
    TRY(critics_backward(a.d_critics, cs, nets, mine.X2, ldx, B, Bp, c_h1, c_h2, w.dq, w.dh2, w.dh1,
                         a.critic.d_grad_sums, nullptr, st, &td, critic_fold, critics_img));
  }
  if (!due || phase == 1) {
    TONIC_CHECK_LAUNCH("tonic_q_iteration");
    return TONIC_OK;
  }
  // ---- 5 + 6: the updated critics on (s, a_new), the actor objective, down to the action columns
  const int used = kind == 1 ? 2 : 1;                  // TD3 / DDPG: critic_1 only (td3.py:36)
  const StepLoss objective{LOSS_ACTOR, nullptr, nullptr, nullptr, mine.logp,
                           (float)a.actor_entropy_coeff, q, a.actor.d_grad_sums + Pa};
  // ---- 7 + 8: head backward + actor chain, weight gradients + Adam + polyak of the actor
  MlpBwdArgs hb{};
  hb.hb_dxa0 = mine.dxa; hb.hb_dxa1 = used == 2 ? mine.dxa + (int64_t)Bp * ldh : nullptr; hb.hb_ldxa = ldh;
  hb.hb_act = mine.act; hb.hb_eps = a.d_eps_actor; hb.hb_sigma = mine.sigma;
  hb.hb_spre = mine.head1 + (int64_t)Bp * ldh;              // net 1's scale head
  hb.hb_sac = kind == 1 ? 1 : 0; hb.hb_alpha = (float)a.actor_entropy_coeff;
  AdamFold af = adam_fold(a.actor, a.d_actor, Pa, grad_scale, 4, chain ? failed : nullptr);
  af.target = a.d_target_actor;
  af.polyak_keep = (float)(1.0 - a.target_coeff); af.polyak_mix = (float)a.target_coeff;
  const AdamFold* actor_fold = phase == 0 ? &af : nullptr;
  if (chain) {
    // 5 + 6 + 7 as ONE launch (q_actor_step_kernel): critics forward -> objective (the twins
    // exchange q) -> their chain to the action columns -> head backward + the actor's chain
    QActorStep step{};
    int launch_nets = 0;
    step.fwd = critics_forward_args(a.d_critics, cs, used, mine.X3, ldx, B, Bp, c_h1, c_h2, q, nullptr,
                                    nullptr, &launch_nets, critics_img);
    step.fwd.xq = mine.xq + 128;              // the critics' q: lines 4, 5 of the tile
    step.bwd = critics_chain_args(a.d_critics, cs, used, B, Bp, c_h1, c_h2, w.dq, w.dh2, w.dh1, mine.dxa,
                                  &objective, critics_img);
    step.bwd.exchange_failed = failed;
    step.bwd.skip_dz = 1;            // (the critics are frozen in the actor step: only dxa leaves their chain)
    step.bwd.l_q = mine.xq + 128; step.bwd.l_q_at = ValueLines{32, kExchangeTileFloats};
    step.actor = actor_chain_args(a.d_actor, as, B, mine.p_h1 + hs, mine.p_h2 + hs, w.dloc,
                                  kind == 1 ? w.dspre : nullptr, ldh, w.da_h2, w.da_h1, nullptr, 0, 0, &hb, actor_img);
    step.actor.exchange_failed = failed;
    step.used = used;
    TRY(launch_q_actor_step(step, st));
    TRY(actor_weight_gradients(as, a.d_observations, O, B, mine.p_h1 + hs, mine.p_h2 + hs, w.dloc,
                               kind == 1 ? w.dspre : nullptr, ldh, w.da_h2, w.da_h1, a.actor.d_grad_sums,
                               st, actor_fold, actor_img));
  } else {
    TRY(critics_forward(a.d_critics, cs, used, mine.X3, ldx, B, Bp, c_h1, c_h2, q, st, nullptr, nullptr, critics_img));
    TRY(critics_backward(a.d_critics, cs, used, mine.X3, ldx, B, Bp, c_h1, c_h2, w.dq, w.dh2, w.dh1, nullptr,
                         mine.dxa, st, &objective, nullptr, critics_img));
    TRY(actor_shaped_backward(a.d_actor, as, a.d_observations, O, B, mine.p_h1 + hs, mine.p_h2 + hs, w.dloc,
                              kind == 1 ? w.dspre : nullptr, ldh, w.da_h2, w.da_h1, a.actor.d_grad_sums,
                              nullptr, 0, 0, st, &hb, actor_fold, actor_img));
  }
  TONIC_CHECK_LAUNCH("tonic_q_iteration");
  return TONIC_OK;
}

// ------------------------------------------------------------------ D4PG (distributional critic)
// The critic is an actor-shaped network: input [normalised observation | action] (O + A columns),
// two ReLU layers, ONE linear head of NA logits (models/critics.py:49-66) — same packed layout as
// tonic_mlp_actor_param_count(O + A, H, NA, 1).

namespace {

// Every (h1, h2) / (dz2, dz1) pair is the first two layers of a region of hidden_layers(H) layers (see layer_at).
// One critic's arrays, target (t_) and online (c_): the hidden regions, the logits and the online logits' gradient.
struct DistributionalCritic {
  float *t_h1, *t_h2, *c_h1, *c_h2, *t_logits, *logits, *dlogits;
  void take(Workspace& ws, int64_t hid, int64_t region, int64_t rows) {
    t_h1 = ws.take(region); t_h2 = behind(t_h1, hid); c_h1 = ws.take(region); c_h2 = behind(c_h1, hid);
    t_logits = ws.take(rows); logits = ws.take(rows); dlogits = ws.take(rows);
  }
};
// nets == 1: D4PG's arrays.  nets == 2 (TD4): the same — a workspace of that size serves
// tonic_distributional_actor_grad as well — and behind them the second critic's and sample_m; the policy pass, X / X2
// and the chain's (dz2, dz1), which the two backward passes use one after the other, exist once.
struct DistributionalBuffers {
  float *a_h1, *a_h2, *head, *act, *X, *X2, *loss_m, *dz2, *dz1, *dxa, *dloc, *da_h2, *da_h1, *sample_m;
  DistributionalCritic k[2];
  DistributionalBuffers(Workspace& ws, int B, int O, int A, int32_t H, int NA, int nets = 1) : sample_m(nullptr), k{} {
    const int64_t Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), ldl = pad16(NA);
    const int64_t hid = Bp * hidden_pitch(H), region = hid * hidden_layers(H);
    a_h1 = ws.take(region); a_h2 = behind(a_h1, hid);
    head = ws.take(Bp * ldh); act = ws.take(Bp * A);
    X = ws.take(Bp * ldx); X2 = ws.take(Bp * ldx);
    k[0].take(ws, hid, region, Bp * ldl); loss_m = ws.take(Bp);
    dz2 = ws.take(region); dz1 = behind(dz2, hid);
    dxa = ws.take(Bp * ldh); dloc = ws.take(Bp * ldh);
    da_h2 = ws.take(region); da_h1 = behind(da_h2, hid);
    if (nets == 2) { k[1].take(ws, hid, region, Bp * ldl); sample_m = ws.take(3 * Bp); }
  }
};

}  // namespace

extern "C" int64_t tonic_distributional_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H,
                                                        int32_t NA) {
  return measure<DistributionalBuffers>(B, O, A, H, NA);
}

// TD4: TD3's twin critics, clipped target-action noise and delayed actor steps on D4PG's categorical critic.  The
// flat blocks are [critic_1 | critic_2]; the actor step is tonic_distributional_actor_grad on the first, critic_1.
extern "C" int64_t tonic_twin_distributional_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H,
                                                             int32_t NA) {
  return measure<DistributionalBuffers>(B, O, A, H, NA, 2);
}

namespace {

// The critic step of D4PG (nets == 1) and TD4 (nets == 2: the flat blocks [critic_1 | critic_2]) and their weighted
// forms, one body (`what`: the entry's name in the messages).  d_eps == null: the target actor's action as it is;
// else TD3's clipped target-action noise on it.
int distributional_q_grad(
    const char* what, int nets, const float* d_target_actor, const float* d_target_critics, const float* d_critics,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_eps, const float* d_values,
    float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t NA, double noise_scale,
    double noise_clip, const float* d_weights, float* d_sample_losses, void* d_workspace, int64_t workspace_bytes,
    void* stream) {
  TONIC_REQUIRE(d_target_actor && d_target_critics && d_critics && d_norm_mean && d_norm_std &&
                    d_observations && d_actions && d_next_observations && d_rewards &&
                    d_discounts && (d_eps || nets == 1) && d_values && d_grad_sums && d_workspace && B > 0 &&
                    NA >= 2 && NA <= 64 && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT, "%s: bad argument (2 <= atoms <= 64)", what);
  TONIC_REQUIRE(d_eps == nullptr ||
                    (std::isfinite(noise_scale) && std::isfinite(noise_clip) && noise_scale >= 0 && noise_clip >= 0),
                TONIC_ERR_INVALID_ARGUMENT,
                "%s: noise scale %g, clip %g (finite and >= 0)", what, noise_scale, noise_clip);
  TONIC_REQUIRE(workspace_bytes >= measure<DistributionalBuffers>(B, O, A, H, NA, nets),
                TONIC_ERR_WORKSPACE, "%s: workspace too small", what);
  hipStream_t st = as_stream(stream);
  const int Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), ldl = pad16(NA);
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const DistributionalBuffers w(ws, B, O, A, H, NA, nets);
  const ActorShape as = actor_shape(O, H, A, 1), cs = actor_shape(O + A, H, NA, 1);
  const int64_t Pc = actor_count(cs);
  // 1  a' = target_actor(s') (critics.py:104) [TD4: clamp(a' + clamp(scale eps, -clip, clip), -1, 1)]; the tail
  //    encodes (s', a') -> X and the stored (s, a) -> X2
  PolicyTail tail{};
  tail.post = POST_COPY; tail.actions = w.act;
  if (d_eps != nullptr) {
    tail.post = POST_TARGET_NOISE; tail.eps = d_eps;
    tail.noise_scale = (float)noise_scale; tail.noise_clip = (float)noise_clip;
  }
  tail.enc_obs = d_next_observations; tail.enc_obs2 = d_observations; tail.enc_act2 = d_actions;
  tail.enc_mean = d_norm_mean; tail.enc_std = d_norm_std; tail.enc_clip = clip_bound(norm_clip);
  tail.enc_out = w.X; tail.enc_out2 = w.X2; tail.enc_ld = ldx;
  TRY(policy_pass(d_target_actor, as, d_next_observations, B, w.a_h1, w.a_h2, w.head, w.head, ldh, true, st, tail));
  // 2  the target critics on (s', a'), then  3  the online critics on (s, a)
  for (int k = 0; k < nets; ++k)
    TRY(actor_forward(d_target_critics + k * Pc, cs, w.X, B, w.k[k].t_h1, w.k[k].t_h2, w.k[k].t_logits,
                      w.k[k].t_logits, ldl, false, st, nullptr, nullptr, ldx));
  for (int k = 0; k < nets; ++k)
    TRY(actor_forward(d_critics + k * Pc, cs, w.X2, B, w.k[k].c_h1, w.k[k].c_h2, w.k[k].logits, w.k[k].logits, ldl,
                      false, st, nullptr, nullptr, ldx));
  // 4 + 5  the loss [TD4: on the target distribution of the smaller mean] and the statistics behind the gradient blocks
  if (nets == 1) {
    hipLaunchKernelGGL(distributional_critic_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, st, w.k[0].t_logits,
                       w.k[0].logits, ldl, d_rewards, d_discounts, d_values, NA, w.k[0].dlogits, w.loss_m, B,
                       d_weights, d_sample_losses);
    hipLaunchKernelGGL(loss_stats_kernel, dim3(1), dim3(1024), 0, st, w.loss_m, d_grad_sums + Pc, B);
  } else {
    hipLaunchKernelGGL(twin_distributional_critic_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, st, w.k[0].t_logits,
                       w.k[1].t_logits, w.k[0].logits, w.k[1].logits, ldl, d_rewards, d_discounts, d_values, NA,
                       w.k[0].dlogits, w.k[1].dlogits, w.sample_m, B, Bp, d_weights, d_sample_losses);
    hipLaunchKernelGGL(twin_loss_stats_kernel, dim3(1), dim3(1024), 0, st, w.sample_m, d_grad_sums + 2 * Pc, B, Bp);
  }
  // 6  each online critic's backward into its own block of the sums
  for (int k = 0; k < nets; ++k)
    TRY(actor_shaped_backward(d_critics + k * Pc, cs, w.X2, ldx, B, w.k[k].c_h1, w.k[k].c_h2, w.k[k].dlogits, nullptr,
                              ldl, w.dz2, w.dz1, d_grad_sums + k * Pc, nullptr, 0, 0, st));
  TONIC_CHECK_LAUNCH(what);
  return TONIC_OK;
}

}  // namespace

extern "C" int tonic_distributional_q_grad(
    const float* d_target_actor, const float* d_target_critic, const float* d_critic,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_values, float* d_grad_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, int32_t NA, void* d_workspace,
    int64_t workspace_bytes, void* stream) {
  return distributional_q_grad("tonic_distributional_q_grad", 1, d_target_actor, d_target_critic, d_critic,
                               d_norm_mean, d_norm_std, norm_clip, d_observations, d_actions, d_next_observations,
                               d_rewards, d_discounts, nullptr, d_values, d_grad_sums, B, O, H, A, NA, 0.0, 0.0, nullptr,
                               nullptr, d_workspace, workspace_bytes, stream);
}

// ... on a prioritized batch: the rows' importance weights in, the unweighted row losses out (each may be NULL)
extern "C" int tonic_weighted_distributional_q_grad(
    const float* d_target_actor, const float* d_target_critic, const float* d_critic,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_values, float* d_grad_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, int32_t NA, const float* d_weights, float* d_sample_losses,
    void* d_workspace, int64_t workspace_bytes, void* stream) {
  return distributional_q_grad("tonic_weighted_distributional_q_grad", 1, d_target_actor, d_target_critic, d_critic,
                               d_norm_mean, d_norm_std, norm_clip, d_observations, d_actions, d_next_observations,
                               d_rewards, d_discounts, nullptr, d_values, d_grad_sums, B, O, H, A, NA, 0.0, 0.0,
                               d_weights, d_sample_losses, d_workspace, workspace_bytes, stream);
}

extern "C" int tonic_distributional_actor_grad(
    const float* d_actor_params, const float* d_critic, const float* d_norm_mean,
    const float* d_norm_std, double norm_clip, const float* d_observations, const float* d_values,
    float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t NA, void* d_workspace,
    int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_actor_params && d_critic && d_norm_mean && d_norm_std && d_observations &&
                    d_values && d_grad_sums && d_workspace && B > 0 && NA >= 2 && NA <= 64 && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_distributional_actor_grad: bad argument");
  TONIC_REQUIRE(workspace_bytes >= tonic_distributional_workspace_bytes(B, O, A, H, NA),
                TONIC_ERR_WORKSPACE, "tonic_distributional_actor_grad: workspace too small");
  hipStream_t st = as_stream(stream);
  const int ldx = pitch16(O + A), ldh = pad16(A), ldl = pad16(NA), threads = 256;
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const DistributionalBuffers w(ws, B, O, A, H, NA);
  const ActorShape as = actor_shape(O, H, A, 1), cs = actor_shape(O + A, H, NA, 1);
  PolicyTail tail{};                              // a = actor(s); the tail encodes (s, a) -> X
  tail.post = POST_COPY; tail.actions = w.act;
  tail.enc_obs = d_observations; tail.enc_mean = d_norm_mean; tail.enc_std = d_norm_std;
  tail.enc_clip = clip_bound(norm_clip); tail.enc_out = w.X; tail.enc_ld = ldx;
  TRY(policy_pass(d_actor_params, as, d_observations, B, w.a_h1, w.a_h2, w.head, w.head, ldh, true, st, tail));
  const DistributionalCritic& c = w.k[0];
  TRY(actor_forward(d_critic, cs, w.X, B, c.c_h1, c.c_h2, c.logits, c.logits, ldl, false, st,
                    nullptr, nullptr, ldx));
  hipLaunchKernelGGL(distributional_actor_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, st,
                     c.logits, ldl, d_values, NA, c.dlogits, w.loss_m, B);
  hipLaunchKernelGGL(loss_stats_kernel, dim3(1), dim3(1024), 0, st, w.loss_m,
                     d_grad_sums + actor_count(as), B);
  // through the frozen critic to the action columns of its input, then the tanh head and the actor
  TRY(actor_shaped_backward(d_critic, cs, w.X, ldx, B, c.c_h1, c.c_h2, c.dlogits, nullptr, ldl,
                            w.dz2, w.dz1, nullptr, w.dxa, O, A, st));
  hipLaunchKernelGGL(actor_head_backward_kernel, dim3((B * A + threads - 1) / threads),
                     dim3(threads), 0, st, w.dxa, (const float*)nullptr, ldh, w.act,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, ldh, 0.f,
                     0, w.dloc, (float*)nullptr, B, A, as.scale_lo, as.scale_hi);
  TRY(actor_shaped_backward(d_actor_params, as, d_observations, O, B, w.a_h1, w.a_h2, w.dloc,
                            nullptr, ldh, w.da_h2, w.da_h1, d_grad_sums, nullptr, 0, 0, st));
  TONIC_CHECK_LAUNCH("tonic_distributional_actor_grad");
  return TONIC_OK;
}

// ------------------------------------------------------------------ TD4 (twin distributional critics)
// The critic step of both online critics in one entry (distributional_q_grad with nets == 2).

extern "C" int tonic_twin_distributional_q_grad(
    const float* d_target_actor, const float* d_target_critics, const float* d_critics,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_eps, const float* d_values,
    float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t NA, double noise_scale,
    double noise_clip, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return distributional_q_grad("tonic_twin_distributional_q_grad", 2, d_target_actor, d_target_critics, d_critics,
                               d_norm_mean, d_norm_std, norm_clip, d_observations, d_actions, d_next_observations,
                               d_rewards, d_discounts, d_eps, d_values, d_grad_sums, B, O, H, A, NA, noise_scale,
                               noise_clip, nullptr, nullptr, d_workspace, workspace_bytes, stream);
}

// ... on a prioritized batch: the rows' importance weights in, the unweighted loss_1 + loss_2 out (each may be NULL)
extern "C" int tonic_weighted_twin_distributional_q_grad(
    const float* d_target_actor, const float* d_target_critics, const float* d_critics,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_eps, const float* d_values,
    float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t NA, double noise_scale,
    double noise_clip, const float* d_weights, float* d_sample_losses, void* d_workspace, int64_t workspace_bytes,
    void* stream) {
  return distributional_q_grad("tonic_weighted_twin_distributional_q_grad", 2, d_target_actor, d_target_critics,
                               d_critics, d_norm_mean, d_norm_std, norm_clip, d_observations, d_actions,
                               d_next_observations, d_rewards, d_discounts, d_eps, d_values, d_grad_sums, B, O, H, A, NA,
                               noise_scale, noise_clip, d_weights, d_sample_losses, d_workspace, workspace_bytes,
                               stream);
}

// ------------------------------------------------------------------ TQC (truncated quantile critics)
// SAC's frame on 2 <= N <= 8 quantile critics: each an actor-shaped network with ONE linear head of M quantiles (D4PG's
// layout, tonic_mlp_actor_param_count(O + A, H, M, 1)); the flat blocks are [critic_1 | ... | critic_N].  Every critic's
// passes are launches of their own and only the loss kernels see the ensemble whole.  The twin entries are N = 2.

namespace {

// Both steps' arrays (one query): SAC's policy pass with its sample, the critics' inputs, the critics' hidden regions,
// the rows' values, one chain (dz2, dz1) the backward passes use one after the other, and the actor step's action
// columns, head gradients and chain.  The N critics' target outputs, online outputs and their gradients are three
// arrays of N consecutive [Bp, ldl] blocks (the loss kernels address critic z at base + z `rows`); an online critic
// keeps its hidden region for its backward pass, the target critics, consumed one after the other, share one.
struct QuantileBuffers {
  float *a_h1, *a_h2, *head0, *head1, *act, *sigma, *logp, *X, *X2, *t_h1, *t_h2, *c_h1[kMaxCritics], *c_h2[kMaxCritics],
      *t_logits, *logits, *dlogits, *sample_m, *loss_m, *dz2, *dz1, *dxa, *dloc, *dspre, *da_h2, *da_h1;
  int64_t rows, action_rows;
  QuantileBuffers(Workspace& ws, int B, int O, int A, int32_t H, int M, int N) : c_h1{}, c_h2{} {
    const int64_t Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), ldl = pad16(M);
    const int64_t hid = Bp * hidden_pitch(H), region = hid * hidden_layers(H);
    rows = Bp * ldl; action_rows = Bp * ldh;
    a_h1 = ws.take(region); a_h2 = behind(a_h1, hid);
    head0 = ws.take(Bp * ldh); head1 = ws.take(Bp * ldh);
    act = ws.take(Bp * A); sigma = ws.take(Bp * A); logp = ws.take(Bp);
    X = ws.take(Bp * ldx); X2 = ws.take(Bp * ldx);
    t_h1 = ws.take(region); t_h2 = behind(t_h1, hid);
    for (int z = 0; z < N; ++z) { c_h1[z] = ws.take(region); c_h2[z] = behind(c_h1[z], hid); }
    t_logits = ws.take(N * rows); logits = ws.take(N * rows); dlogits = ws.take(N * rows);
    sample_m = ws.take(3 * Bp); loss_m = ws.take(Bp);
    dz2 = ws.take(region); dz1 = behind(dz2, hid);
    dxa = ws.take(N * action_rows);
    dloc = ws.take(Bp * ldh); dspre = ws.take(Bp * ldh);
    da_h2 = ws.take(region); da_h1 = behind(da_h2, hid);
  }
};

// what TQC asks of N and M, with the numbers
int quantile_counts_check(const char* what, int32_t M, int32_t N) {
  TONIC_REQUIRE(N >= 2 && N <= kMaxCritics, TONIC_ERR_INVALID_ARGUMENT, "%s: %d critics (2 <= N <= %d)", what, N,
                kMaxCritics);
  TONIC_REQUIRE(M >= 1 && M <= kMaxQuantiles, TONIC_ERR_INVALID_ARGUMENT, "%s: %d quantiles (1 <= M <= %d)", what, M,
                kMaxQuantiles);
  TONIC_REQUIRE(N * M <= kMaxPooled, TONIC_ERR_INVALID_ARGUMENT, "%s: %d critics of %d quantiles pool %d values (N M <= %d)",
                what, N, M, N * M, kMaxPooled);
  return TONIC_OK;
}

// ... and both steps of the shapes and the workspace, after their own pointer checks
int quantile_check(const char* what, int32_t B, int32_t O, int32_t A, int32_t H, int32_t M, int32_t N,
                   int64_t workspace_bytes) {
  TONIC_REQUIRE(B > 0 && O > 0 && A > 0, TONIC_ERR_INVALID_ARGUMENT, "%s: B %d, O %d, A %d (each >= 1)", what, B, O, A);
  TONIC_REQUIRE(hidden_known(H), TONIC_ERR_INVALID_ARGUMENT, "%s: H %d is not a torso this library knows", what, H);
  TRY(quantile_counts_check(what, M, N));
  const int64_t need = measure<QuantileBuffers>(B, O, A, H, M, N);
  TONIC_REQUIRE(workspace_bytes >= need, TONIC_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", what,
                (long long)workspace_bytes, (long long)need);
  return TONIC_OK;
}

// The critic step.  twin_row: the statistics row is the twin model's {loss, q1, q2} (N = 2), not {loss, q}.
// subset: REDQ's step — the same passes at M = 1 around the subset minimum's loss kernel; null: TQC's.
int quantile_q_grad(const char* what, int32_t N, int twin_row, const SubsetLoss* subset, const float* d_actor,
                    const float* d_target_critics,
                    const float* d_critics, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
                    const float* d_observations, const float* d_actions, const float* d_next_observations,
                    const float* d_rewards, const float* d_discounts, const float* d_eps, float* d_grad_sums, int32_t B,
                    int32_t O, int32_t H, int32_t A, int32_t M, int32_t drop_per_net, double entropy_coeff,
                    const float* d_log_entropy_coeff, void* d_workspace, int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_actor && d_target_critics && d_critics && d_norm_mean && d_norm_std && d_observations && d_actions &&
                    d_next_observations && d_rewards && d_discounts && d_eps && d_grad_sums && d_workspace,
                TONIC_ERR_INVALID_ARGUMENT, "%s: a NULL pointer (only d_log_entropy_coeff may be NULL)", what);
  TONIC_REQUIRE(M < 1 || M > kMaxQuantiles || (drop_per_net >= 0 && drop_per_net < M), TONIC_ERR_INVALID_ARGUMENT,
                "%s: %d quantiles dropped per critic (0 <= drop_per_net < M = %d)", what, drop_per_net, M);
  TRY(quantile_check(what, B, O, A, H, M, N, workspace_bytes));
  hipStream_t st = as_stream(stream);
  const int Bp = pad16(B), ldx = pitch16(O + A), ldh = pad16(A), ldl = pad16(M);
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const QuantileBuffers w(ws, B, O, A, H, M, N);
  const ActorShape as = actor_shape(O, H, A, 2), cs = actor_shape(O + A, torso_code(H), M, 1);
  const int64_t Pc = actor_count(cs);
  // 1  a' = rsample of the ONLINE actor at s' with logp' (as tonic_twin_q_grad, kind 1); the tail encodes (s', a') -> X
  //    and the stored (s, a) -> X2
  PolicyTail tail{};
  tail.post = POST_SQUASHED_SAMPLE; tail.eps = d_eps; tail.actions = w.act; tail.logp = w.logp;
  tail.enc_obs = d_next_observations; tail.enc_obs2 = d_observations; tail.enc_act2 = d_actions;
  tail.enc_mean = d_norm_mean; tail.enc_std = d_norm_std; tail.enc_clip = clip_bound(norm_clip);
  tail.enc_out = w.X; tail.enc_out2 = w.X2; tail.enc_ld = ldx;
  TRY(policy_pass(d_actor, as, d_next_observations, B, w.a_h1, w.a_h2, w.head0, w.head1, ldh, false, st, tail));
  // 2  the target critics on (s', a'), then  3  the online critics on (s, a)
  for (int z = 0; z < N; ++z)
    TRY(actor_forward(d_target_critics + z * Pc, cs, w.X, B, w.t_h1, w.t_h2, w.t_logits + z * w.rows,
                      w.t_logits + z * w.rows, ldl, false, st, nullptr, nullptr, ldx));
  for (int z = 0; z < N; ++z)
    TRY(actor_forward(d_critics + z * Pc, cs, w.X2, B, w.c_h1[z], w.c_h2[z], w.logits + z * w.rows,
                      w.logits + z * w.rows, ldl, false, st, nullptr, nullptr, ldx));
  // 4 + 5  the truncated quantile loss over the pool of N M (REDQ: the loss against the subset's minimum) and the
  //        statistics behind the gradient blocks
  if (subset != nullptr)
    launch_subset_critic_loss(st, w.t_logits, w.logits, w.rows, ldl, d_rewards, d_discounts, w.logp, N, *subset,
                              (float)entropy_coeff, d_log_entropy_coeff, w.dlogits, w.sample_m, B, Bp);
  else
    launch_quantile_critic_loss(st, w.t_logits, w.logits, w.rows, ldl, d_rewards, d_discounts, w.logp, M, N,
                                drop_per_net, (float)entropy_coeff, d_log_entropy_coeff, w.dlogits, w.sample_m,
                                twin_row, B, Bp);
  hipLaunchKernelGGL(twin_loss_stats_kernel, dim3(1), dim3(1024), 0, st, w.sample_m, d_grad_sums + N * Pc, B, Bp);
  // 6  each online critic's backward into its own block of the sums
  for (int z = 0; z < N; ++z)
    TRY(actor_shaped_backward(d_critics + z * Pc, cs, w.X2, ldx, B, w.c_h1[z], w.c_h2[z], w.dlogits + z * w.rows,
                              nullptr, ldl, w.dz2, w.dz1, d_grad_sums + z * Pc, nullptr, 0, 0, st));
  TONIC_CHECK_LAUNCH(what);
  return TONIC_OK;
}

// The actor step.
int quantile_actor_grad(const char* what, int32_t N, const float* d_actor, const float* d_critics,
                        const float* d_norm_mean, const float* d_norm_std, double norm_clip, const float* d_observations,
                        const float* d_eps, float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t M,
                        double entropy_coeff, const float* d_log_entropy_coeff, float* d_entropy_coeff_sums,
                        double target_entropy, void* d_workspace, int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_actor && d_critics && d_norm_mean && d_norm_std && d_observations && d_eps && d_grad_sums &&
                    d_workspace,
                TONIC_ERR_INVALID_ARGUMENT, "%s: a NULL pointer (only the tuner's pair may be NULL)", what);
  TONIC_REQUIRE((d_log_entropy_coeff == nullptr) == (d_entropy_coeff_sums == nullptr), TONIC_ERR_INVALID_ARGUMENT,
                "%s: %s is NULL and the other is not (both or neither)", what,
                d_log_entropy_coeff == nullptr ? "d_log_entropy_coeff" : "d_entropy_coeff_sums");
  TONIC_REQUIRE(std::isfinite(target_entropy), TONIC_ERR_INVALID_ARGUMENT, "%s: target_entropy is not finite", what);
  TRY(quantile_check(what, B, O, A, H, M, N, workspace_bytes));
  hipStream_t st = as_stream(stream);
  const int ldx = pitch16(O + A), ldh = pad16(A), ldl = pad16(M), threads = 256;
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const QuantileBuffers w(ws, B, O, A, H, M, N);
  const ActorShape as = actor_shape(O, H, A, 2), cs = actor_shape(O + A, torso_code(H), M, 1);
  const int64_t Pa = actor_count(as), Pc = actor_count(cs);
  const TemperArg temper{d_log_entropy_coeff, d_entropy_coeff_sums, (float)target_entropy};
  PolicyTail tail{};                              // a = rsample of the actor at s with logp; the tail encodes (s, a) -> X
  tail.post = POST_SQUASHED_SAMPLE; tail.eps = d_eps; tail.actions = w.act; tail.sigma = w.sigma; tail.logp = w.logp;
  tail.enc_obs = d_observations; tail.enc_mean = d_norm_mean; tail.enc_std = d_norm_std;
  tail.enc_clip = clip_bound(norm_clip); tail.enc_out = w.X; tail.enc_ld = ldx;
  TRY(policy_pass(d_actor, as, d_observations, B, w.a_h1, w.a_h2, w.head0, w.head1, ldh, false, st, tail));
  for (int z = 0; z < N; ++z)
    TRY(actor_forward(d_critics + z * Pc, cs, w.X, B, w.c_h1[z], w.c_h2[z], w.logits + z * w.rows,
                      w.logits + z * w.rows, ldl, false, st, nullptr, nullptr, ldx));
  hipLaunchKernelGGL(quantile_actor_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, st, w.logits, w.rows, ldl, w.logp, M,
                     N, (float)entropy_coeff, temper, w.dlogits, w.loss_m, B);
  hipLaunchKernelGGL(loss_stats_kernel, dim3(1), dim3(1024), 0, st, w.loss_m, d_grad_sums + Pa, B);
  // through each frozen critic to the action columns of its input; critics 2 .. N added up, then SAC's head (which adds
  // the two blocks left) and the actor
  for (int z = 0; z < N; ++z)
    TRY(actor_shaped_backward(d_critics + z * Pc, cs, w.X, ldx, B, w.c_h1[z], w.c_h2[z], w.dlogits + z * w.rows,
                              nullptr, ldl, w.dz2, w.dz1, nullptr, w.dxa + z * w.action_rows, O, A, st));
  if (N > 2)
    hipLaunchKernelGGL(ensemble_action_grad_sum_kernel, dim3((unsigned)((w.action_rows + threads - 1) / threads)),
                       dim3(threads), 0, st, w.dxa, N, w.action_rows);
  if (temper.log_alpha != nullptr)
    hipLaunchKernelGGL(actor_head_backward_tempered_kernel, dim3((B * A + threads - 1) / threads), dim3(threads), 0, st,
                       w.dxa, w.dxa + w.action_rows, ldh, w.act, d_eps, w.sigma, w.head1, ldh, temper.log_alpha,
                       w.dloc, w.dspre, B, A, as.scale_lo, as.scale_hi);
  else hipLaunchKernelGGL(actor_head_backward_kernel, dim3((B * A + threads - 1) / threads), dim3(threads), 0, st, w.dxa,
                     w.dxa + w.action_rows, ldh, w.act, d_eps, w.sigma, w.head1, ldh, (float)entropy_coeff, 1, w.dloc,
                     w.dspre, B, A, as.scale_lo, as.scale_hi);
  TRY(actor_shaped_backward(d_actor, as, d_observations, O, B, w.a_h1, w.a_h2, w.dloc, w.dspre, ldh, w.da_h2, w.da_h1,
                            d_grad_sums, nullptr, 0, 0, st));
  TONIC_CHECK_LAUNCH(what);
  return TONIC_OK;
}

}  // namespace

extern "C" int64_t tonic_ensemble_quantile_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H, int32_t M,
                                                           int32_t N) {
  if (N < 2 || N > kMaxCritics) return 0;                  // (the entries refuse such an N before they ask for a byte)
  return measure<QuantileBuffers>(B, O, A, H, M, N);
}

extern "C" int64_t tonic_quantile_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H, int32_t M) {
  return measure<QuantileBuffers>(B, O, A, H, M, 2);
}

extern "C" int tonic_truncated_quantile_q_grad(
    const float* d_actor, const float* d_target_critics, const float* d_critics, const float* d_norm_mean,
    const float* d_norm_std, double norm_clip, const float* d_observations, const float* d_actions,
    const float* d_next_observations, const float* d_rewards, const float* d_discounts, const float* d_eps,
    float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t M, int32_t drop_per_net,
    double entropy_coeff, const float* d_log_entropy_coeff, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return quantile_q_grad("tonic_truncated_quantile_q_grad", 2, 1, nullptr, d_actor, d_target_critics, d_critics,
                         d_norm_mean, d_norm_std, norm_clip, d_observations, d_actions, d_next_observations, d_rewards,
                         d_discounts, d_eps, d_grad_sums, B, O, H, A, M, drop_per_net, entropy_coeff,
                         d_log_entropy_coeff, d_workspace, workspace_bytes, stream);
}

extern "C" int tonic_ensemble_quantile_q_grad(
    const float* d_actor, const float* d_target_critics, const float* d_critics, const float* d_norm_mean,
    const float* d_norm_std, double norm_clip, const float* d_observations, const float* d_actions,
    const float* d_next_observations, const float* d_rewards, const float* d_discounts, const float* d_eps,
    float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t M, int32_t N, int32_t drop_per_net,
    double entropy_coeff, const float* d_log_entropy_coeff, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return quantile_q_grad("tonic_ensemble_quantile_q_grad", N, 0, nullptr, d_actor, d_target_critics, d_critics,
                         d_norm_mean, d_norm_std, norm_clip, d_observations, d_actions, d_next_observations, d_rewards,
                         d_discounts, d_eps, d_grad_sums, B, O, H, A, M, drop_per_net, entropy_coeff,
                         d_log_entropy_coeff, d_workspace, workspace_bytes, stream);
}

extern "C" int tonic_truncated_quantile_actor_grad(
    const float* d_actor, const float* d_critics, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A,
    int32_t M, double entropy_coeff, const float* d_log_entropy_coeff, float* d_entropy_coeff_sums,
    double target_entropy, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return quantile_actor_grad("tonic_truncated_quantile_actor_grad", 2, d_actor, d_critics, d_norm_mean, d_norm_std,
                             norm_clip, d_observations, d_eps, d_grad_sums, B, O, H, A, M, entropy_coeff,
                             d_log_entropy_coeff, d_entropy_coeff_sums, target_entropy, d_workspace, workspace_bytes,
                             stream);
}

extern "C" int tonic_ensemble_quantile_actor_grad(
    const float* d_actor, const float* d_critics, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A,
    int32_t M, int32_t N, double entropy_coeff, const float* d_log_entropy_coeff, float* d_entropy_coeff_sums,
    double target_entropy, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return quantile_actor_grad("tonic_ensemble_quantile_actor_grad", N, d_actor, d_critics, d_norm_mean, d_norm_std,
                             norm_clip, d_observations, d_eps, d_grad_sums, B, O, H, A, M, entropy_coeff,
                             d_log_entropy_coeff, d_entropy_coeff_sums, target_entropy, d_workspace, workspace_bytes,
                             stream);
}

// Test entry (include/tonic_hip_dev.h): the critic loss kernel alone on given rows, critic z's [B, ld] block at z B ld
// of each array; sample_m [3][Bp].
extern "C" int tonic_debug_ensemble_quantile_loss(
    const float* d_targets, const float* d_thetas, int32_t ld, const float* d_rewards, const float* d_discounts,
    const float* d_logp, int32_t M, int32_t N, int32_t drop_per_net, double entropy_coeff,
    const float* d_log_entropy_coeff, float* d_dlogits, float* d_sample_m, int32_t B, int32_t Bp, int32_t twin_row,
    void* stream) {
  const char* what = "tonic_debug_ensemble_quantile_loss";
  TONIC_REQUIRE(d_targets && d_thetas && d_rewards && d_discounts && d_logp && d_dlogits && d_sample_m,
                TONIC_ERR_INVALID_ARGUMENT, "%s: a NULL pointer (only d_log_entropy_coeff may be NULL)", what);
  TRY(quantile_counts_check(what, M, N));
  TONIC_REQUIRE(drop_per_net >= 0 && drop_per_net < M && ld >= M && ld <= kMaxQuantiles && B > 0 && Bp >= B,
                TONIC_ERR_INVALID_ARGUMENT,
                "%s: M %d, drop_per_net %d, ld %d, B %d, Bp %d (0 <= drop < M, M <= ld <= %d, 0 < B <= Bp)", what, M,
                drop_per_net, ld, B, Bp, kMaxQuantiles);
  TONIC_REQUIRE(twin_row == 0 || N == 2, TONIC_ERR_INVALID_ARGUMENT,
                "%s: the twin row {loss, q1, q2} is that of 2 critics, not of %d", what, N);
  launch_quantile_critic_loss(as_stream(stream), d_targets, d_thetas, (int64_t)B * ld, ld, d_rewards, d_discounts, d_logp,
                              M, N, drop_per_net, (float)entropy_coeff, d_log_entropy_coeff, d_dlogits, d_sample_m,
                              twin_row != 0, B, Bp);
  TONIC_CHECK_LAUNCH(what);
  return TONIC_OK;
}

// ------------------------------------------------------------------ REDQ (random-subset ensemble Q-learning)
// SAC on N scalar critics in TQC's layout at M = 1: the critic step is quantile_q_grad with the subset loss launch,
// the actor step tonic_ensemble_quantile_actor_grad at M = 1 as it stands, and the workspace TQC's layout at M = 1.
extern "C" int64_t tonic_ensemble_q_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H, int32_t N) {
  return tonic_ensemble_quantile_workspace_bytes(B, O, A, H, 1, N);
}

extern "C" int tonic_ensemble_subset_q_grad(
    const float* d_actor, const float* d_target_critics, const float* d_critics, const float* d_norm_mean,
    const float* d_norm_std, double norm_clip, const float* d_observations, const float* d_actions,
    const float* d_next_observations, const float* d_rewards, const float* d_discounts, const float* d_eps,
    float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t N, const int32_t* d_subset,
    double entropy_coeff, const float* d_log_entropy_coeff, const tonic_critic_loss_t* loss, void* d_workspace,
    int64_t workspace_bytes, void* stream) {
  const char* what = "tonic_ensemble_subset_q_grad";
  TONIC_REQUIRE(d_subset != nullptr, TONIC_ERR_INVALID_ARGUMENT,
                "%s: a NULL pointer (d_subset; only d_log_entropy_coeff may be NULL)", what);
  TRY(tonic_critic_loss_check(loss));
  const SubsetLoss subset{d_subset, critic_loss_rule(loss)};
  return quantile_q_grad(what, N, 0, &subset, d_actor, d_target_critics, d_critics, d_norm_mean, d_norm_std, norm_clip,
                         d_observations, d_actions, d_next_observations, d_rewards, d_discounts, d_eps, d_grad_sums, B,
                         O, H, A, 1, 0, entropy_coeff, d_log_entropy_coeff, d_workspace, workspace_bytes, stream);
}

// Test entry (include/tonic_hip_dev.h): REDQ's critic loss kernel alone on given rows, critic z's [Bp, ld] block at
// z Bp ld of each array; sample_m [3][Bp].
extern "C" int tonic_debug_ensemble_subset_loss(
    const float* d_targets, const float* d_qs, int32_t ld, const float* d_rewards, const float* d_discounts,
    const float* d_logp, int32_t N, const int32_t* d_subset, double entropy_coeff, const float* d_log_entropy_coeff,
    const tonic_critic_loss_t* loss, float* d_dq, float* d_sample_m, int32_t B, int32_t Bp, void* stream) {
  const char* what = "tonic_debug_ensemble_subset_loss";
  TONIC_REQUIRE(d_targets && d_qs && d_rewards && d_discounts && d_logp && d_subset && d_dq && d_sample_m,
                TONIC_ERR_INVALID_ARGUMENT, "%s: a NULL pointer (only d_log_entropy_coeff and loss may be NULL)", what);
  TONIC_REQUIRE(N >= 2 && N <= kMaxCritics, TONIC_ERR_INVALID_ARGUMENT, "%s: %d critics (2 <= N <= %d)", what, N,
                kMaxCritics);
  TONIC_REQUIRE(ld >= 1 && ld <= kMaxQuantiles && B > 0 && Bp >= B, TONIC_ERR_INVALID_ARGUMENT,
                "%s: ld %d, B %d, Bp %d (1 <= ld <= %d, 0 < B <= Bp)", what, ld, B, Bp, kMaxQuantiles);
  TRY(tonic_critic_loss_check(loss));
  launch_subset_critic_loss(as_stream(stream), d_targets, d_qs, (int64_t)Bp * ld, ld, d_rewards, d_discounts, d_logp, N,
                            SubsetLoss{d_subset, critic_loss_rule(loss)}, (float)entropy_coeff, d_log_entropy_coeff,
                            d_dq, d_sample_m, B, Bp);
  TONIC_CHECK_LAUNCH(what);
  return TONIC_OK;
}


// ------------------------------------------------------------------------------------- MPO
namespace {

struct MpoBuffers {
  float *a_h1, *a_h2, *loc_t, *spre_t, *loc, *spre, *o_h1, *o_h2, *act, *X, *X2, *t_h1, *t_h2, *tq,
      *tq_mean, *c_h1, *c_h2, *q, *dq, *dh2, *dh1, *dloc, *dspre, *da_h2, *da_h1, *part, *klm, *kls;
  // every (h1, h2) / (dh2, dh1) pair: the first two layers of a region of hidden_layers(H) layers (see layer_at)
  MpoBuffers(Workspace& ws, int B, int O, int A, int32_t H, int S) {
    const int64_t Bp = pad16(B), Rp = pad16(S * B), HP = hidden_pitch(H), hid = Bp * HP, layers = hidden_layers(H);
    const int64_t ldh = pad16(A), ldx = pitch16(O + A);
    a_h1 = ws.take(layers * hid); a_h2 = behind(a_h1, hid); o_h1 = ws.take(layers * hid); o_h2 = behind(o_h1, hid);
    loc_t = ws.take(Bp * ldh); spre_t = ws.take(Bp * ldh); loc = ws.take(Bp * ldh);
    spre = ws.take(Bp * ldh);
    act = ws.take(Rp * A); X = ws.take(Rp * ldx); X2 = ws.take(Bp * ldx);
    t_h1 = ws.take(layers * Rp * HP); t_h2 = behind(t_h1, Rp * HP); tq = ws.take(Rp); tq_mean = ws.take(Bp);
    c_h1 = ws.take(layers * hid); c_h2 = behind(c_h1, hid); q = ws.take(Bp); dq = ws.take(Bp);
    dh2 = ws.take(layers * hid); dh1 = behind(dh2, hid);
    dloc = ws.take(Bp * ldh); dspre = ws.take(Bp * ldh); da_h2 = ws.take(layers * hid); da_h1 = behind(da_h2, hid);
    part = ws.take(Bp * kMpoStats); klm = ws.take(Bp * A); kls = ws.take(Bp * A);
  }
};

// DMPO: MPO's arrays as they are, and behind them the categorical critic's — the target logits of the S * B tiled
// rows with their log-normalisers, the online critic's logits and their gradient, and sample_m [2][Bp].  The
// critics' hidden regions (t_h1, c_h1, dh2) are MPO's: a D4PG-shaped critic has the scalar critic's torso.
// NA == 0 (mpo_actor_grad on the scalar critic): MPO's arrays and nothing more.
struct DmpoBuffers : MpoBuffers {
  float *t_logits = nullptr, *t_log_norm = nullptr, *logits = nullptr, *dlogits = nullptr, *sample_m = nullptr;
  DmpoBuffers(Workspace& ws, int B, int O, int A, int32_t H, int S, int NA) : MpoBuffers(ws, B, O, A, H, S) {
    if (NA == 0) return;
    const int64_t Bp = pad16(B), Rp = pad16(S * B), ldl = pad16(NA);
    t_logits = ws.take(Rp * ldl); t_log_norm = ws.take(Rp);
    logits = ws.take(Bp * ldl); dlogits = ws.take(Bp * ldl); sample_m = ws.take(2 * Bp);
  }
};

// The categorical critic of a DMPO entry: its support, and where the tiled rows' logits and (null: not wanted)
// log-normalisers go.
struct SampledDistribution { const float* values; int NA; float* t_logits; float* t_log_norm; };

// target_actor(obs) -> S sampled actions per state -> target_critic on the tiled rows: tq [S * B].  dist != null:
// the critic is categorical — its logits on the tiled rows, then each row's mean into tq.
int mpo_sampled_values(const float* d_target_actor, const float* d_target_critic,
                       const float* d_norm_mean, const float* d_norm_std, double norm_clip,
                       const float* d_obs, const float* d_eps, int B, int O, int H, int A, int S,
                       const MpoBuffers& w, hipStream_t st, const SampledDistribution* dist = nullptr) {
  const int ldx = pitch16(O + A), ldh = pad16(A), threads = 256;
  const ActorShape as = actor_shape(O, H, A, 2);
  TRY(actor_forward(d_target_actor, as, d_obs, B, w.a_h1, w.a_h2, w.loc_t, w.spre_t, ldh, true, st));
  const int64_t items = (int64_t)S * B * (O + A);
  hipLaunchKernelGGL(gaussian_tile_kernel, dim3((unsigned)((items + threads - 1) / threads)),
                     dim3(threads), 0, st, d_obs, w.loc_t, w.spre_t, d_eps, ldh, d_norm_mean,
                     d_norm_std, clip_bound(norm_clip), w.act, w.X, B, O, A, S, ldx, as.scale_lo, as.scale_hi);
  if (dist == nullptr)
    return critics_forward(d_target_critic, critic_shape(O, A, H), 1, w.X, ldx, S * B, pad16(S * B),
                           w.t_h1, w.t_h2, w.tq, st);
  const int ldl = pad16(dist->NA), rows = S * B;
  TRY(actor_forward(d_target_critic, actor_shape(O + A, H, dist->NA, 1), w.X, rows, w.t_h1, w.t_h2, dist->t_logits,
                    dist->t_logits, ldl, false, st, nullptr, nullptr, ldx));
  hipLaunchKernelGGL(distributional_value_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, dist->t_logits, ldl,
                     dist->values, dist->NA, w.tq, dist->t_log_norm, rows);
  return TONIC_OK;
}

}  // namespace

extern "C" int64_t tonic_mpo_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H, int32_t S) {
  return measure<MpoBuffers>(B, O, A, H, S);
}

extern "C" int64_t tonic_distributional_mpo_workspace_bytes(int32_t B, int32_t O, int32_t A, int32_t H, int32_t S,
                                                            int32_t NA) {
  return measure<DmpoBuffers>(B, O, A, H, S, NA);
}

namespace {
int expected_sarsa_grad(
    const float* d_target_actor, const float* d_target_critic, const float* d_critic,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_eps, float* d_grad_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, const tonic_critic_loss_t* loss, void* d_workspace,
    int64_t workspace_bytes, void* stream) {
  TRY(tonic_critic_loss_check(loss));
  TONIC_REQUIRE(d_target_actor && d_target_critic && d_critic && d_norm_mean && d_norm_std &&
                    d_observations && d_actions && d_next_observations && d_rewards &&
                    d_discounts && d_eps && d_grad_sums && d_workspace && B > 0 && S >= 1 &&
                    S <= kMpoMaxSamples && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_expected_sarsa_grad: bad argument (1 <= samples <= 256)");
  TONIC_REQUIRE(workspace_bytes >= tonic_mpo_workspace_bytes(B, O, A, H, S), TONIC_ERR_WORKSPACE,
                "tonic_expected_sarsa_grad: workspace too small");
  hipStream_t st = as_stream(stream);
  const int Bp = pad16(B), ldx = pitch16(O + A), threads = 256;
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const MpoBuffers w(ws, B, O, A, H, S);
  const CriticShape cs = critic_shape(O, A, H);
  TRY(mpo_sampled_values(d_target_actor, d_target_critic, d_norm_mean, d_norm_std, norm_clip,
                         d_next_observations, d_eps, B, O, H, A, S, w, st));
  hipLaunchKernelGGL(sample_mean_kernel, dim3((B + threads - 1) / threads), dim3(threads), 0, st,
                     w.tq, w.tq_mean, B, S);
  hipLaunchKernelGGL(encode_kernel, dim3((B * (O + A) + threads - 1) / threads), dim3(threads), 0,
                     st, d_observations, d_actions, d_norm_mean, d_norm_std, clip_bound(norm_clip),
                     w.X2, B, O, A, ldx);
  TRY(critics_forward(d_critic, cs, 1, w.X2, ldx, B, Bp, w.c_h1, w.c_h2, w.q, st));
  const StepLoss td{LOSS_TD, d_rewards, d_discounts, w.tq_mean, nullptr, 0.f, w.q,
                    d_grad_sums + critic_count(cs), critic_loss_rule(loss)};
  TRY(critics_backward(d_critic, cs, 1, w.X2, ldx, B, Bp, w.c_h1, w.c_h2, w.dq, w.dh2, w.dh1,
                       d_grad_sums, nullptr, st, &td));
  TONIC_CHECK_LAUNCH("tonic_expected_sarsa_grad");
  return TONIC_OK;
}
}  // namespace

extern "C" int tonic_expected_sarsa_grad(
    const float* d_target_actor, const float* d_target_critic, const float* d_critic,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_eps, float* d_grad_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, void* d_workspace,
    int64_t workspace_bytes, void* stream) {
  return expected_sarsa_grad(d_target_actor, d_target_critic, d_critic, d_norm_mean, d_norm_std, norm_clip,
                             d_observations, d_actions, d_next_observations, d_rewards, d_discounts, d_eps,
                             d_grad_sums, B, O, H, A, S, nullptr, d_workspace, workspace_bytes, stream);
}

// ... with the critic's loss (critics.py:243: `self.loss(returns, values)`, symmetric in the error): NULL = MSE
extern "C" int tonic_expected_sarsa_grad_loss(
    const float* d_target_actor, const float* d_target_critic, const float* d_critic,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_eps, float* d_grad_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, const tonic_critic_loss_t* loss, void* d_workspace,
    int64_t workspace_bytes, void* stream) {
  return expected_sarsa_grad(d_target_actor, d_target_critic, d_critic, d_norm_mean, d_norm_std, norm_clip,
                             d_observations, d_actions, d_next_observations, d_rewards, d_discounts, d_eps,
                             d_grad_sums, B, O, H, A, S, loss, d_workspace, workspace_bytes, stream);
}

// DMPO's critic step: Expected SARSA on the categorical critic (D4PG's layout, tonic_mlp_actor_param_count(O + A, H,
// NA, 1)).  The target is the projection of the MIXTURE of the target critic's distributions at the S sampled next
// actions; the online critic takes the cross-entropy against it, as in tonic_distributional_q_grad.
extern "C" int tonic_distributional_expected_sarsa_grad(
    const float* d_target_actor, const float* d_target_critic, const float* d_critic,
    const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_actions, const float* d_next_observations,
    const float* d_rewards, const float* d_discounts, const float* d_eps, const float* d_values,
    float* d_grad_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, int32_t NA, void* d_workspace,
    int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_target_actor && d_target_critic && d_critic && d_norm_mean && d_norm_std &&
                    d_observations && d_actions && d_next_observations && d_rewards &&
                    d_discounts && d_eps && d_values && d_grad_sums && d_workspace && B > 0 && S >= 1 &&
                    S <= kMpoMaxSamples && NA >= 2 && NA <= 64 && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT,
                "tonic_distributional_expected_sarsa_grad: bad argument (1 <= samples <= 256, 2 <= atoms <= 64)");
  TONIC_REQUIRE(workspace_bytes >= tonic_distributional_mpo_workspace_bytes(B, O, A, H, S, NA), TONIC_ERR_WORKSPACE,
                "tonic_distributional_expected_sarsa_grad: workspace too small");
  hipStream_t st = as_stream(stream);
  const int Bp = pad16(B), ldx = pitch16(O + A), ldl = pad16(NA), threads = 256;
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const DmpoBuffers w(ws, B, O, A, H, S, NA);
  const ActorShape cs = actor_shape(O + A, H, NA, 1);
  const SampledDistribution dist{d_values, NA, w.t_logits, w.t_log_norm};
  TRY(mpo_sampled_values(d_target_actor, d_target_critic, d_norm_mean, d_norm_std, norm_clip,
                         d_next_observations, d_eps, B, O, H, A, S, w, st, &dist));
  hipLaunchKernelGGL(encode_kernel, dim3((B * (O + A) + threads - 1) / threads), dim3(threads), 0,
                     st, d_observations, d_actions, d_norm_mean, d_norm_std, clip_bound(norm_clip),
                     w.X2, B, O, A, ldx);
  TRY(actor_forward(d_critic, cs, w.X2, B, w.c_h1, w.c_h2, w.logits, w.logits, ldl, false, st, nullptr, nullptr,
                    ldx));
  hipLaunchKernelGGL(mixture_critic_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, st, w.t_logits, w.t_log_norm,
                     w.logits, ldl, d_rewards, d_discounts, d_values, NA, w.dlogits, w.sample_m, B, Bp, S);
  hipLaunchKernelGGL(mixture_loss_stats_kernel, dim3(1), dim3(1024), 0, st, w.sample_m,
                     d_grad_sums + actor_count(cs), B, Bp);
  TRY(actor_shaped_backward(d_critic, cs, w.X2, ldx, B, w.c_h1, w.c_h2, w.dlogits, nullptr, ldl, w.dh2, w.dh1,
                            d_grad_sums, nullptr, 0, 0, st));
  TONIC_CHECK_LAUNCH("tonic_distributional_expected_sarsa_grad");
  return TONIC_OK;
}

namespace {
static_assert(kMpoMaxSamples == 256, "the messages of the MPO entries name the bound");

// the state kernel on ceil(S / 64) register slots per lane
void launch_mpo_state(int slots, dim3 grid, hipStream_t st, const float* q, const float* act, const float* loc_t,
                      const float* spre_t, const float* loc, const float* spre, int ldh, const float* duals,
                      float floor, int penalize, int joint_kl, float* dloc, float* dspre, float* part, float* klm,
                      float* kls, int B, int A, int S, float scale_lo, float scale_hi) {
#define TONIC_MPO_STATE(SLOTS)                                                                                  \
  hipLaunchKernelGGL(mpo_state_kernel<SLOTS>, grid, dim3(256), 0, st, q, act, loc_t, spre_t, loc, spre, ldh,   \
                     duals, floor, penalize, joint_kl, dloc, dspre, part, klm, kls, B, A, S, scale_lo, scale_hi)
  switch (slots) {
    case 1: TONIC_MPO_STATE(1); break;
    case 2: TONIC_MPO_STATE(2); break;
    case 3: TONIC_MPO_STATE(3); break;
    default: TONIC_MPO_STATE(4); break;
  }
#undef TONIC_MPO_STATE
}

int mpo_actor_grad(
    const float* d_actor_params, const float* d_target_actor, const float* d_target_critic,
    float* d_duals, double min_log_dual, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, float* d_grad_sums, float* d_dual_grads,
    float* d_stats, int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, double epsilon,
    double epsilon_penalty, double epsilon_mean, double epsilon_std, int32_t action_penalization,
    int32_t joint_kl, void* d_workspace, int64_t workspace_bytes, void* stream, double* d_column_sums, bool shard,
    const float* d_values = nullptr, int32_t NA = 0) {
  // NA != 0 (the tonic_distributional_mpo_* entries, which check the pair): the E-step's q are the means of the
  // categorical target critic's distributions over the support d_values; nothing else differs
  // (a rank's shard of the batch: only the column sums leave, the duals' half follows the all-reduce — mpo_dual_step)
  TONIC_REQUIRE(!shard || d_column_sums != nullptr, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_mpo_actor_grad_shard: null column sums");
  TONIC_REQUIRE(d_actor_params && d_target_actor && d_target_critic && d_duals && d_norm_mean &&
                    d_norm_std && d_observations && d_eps && d_grad_sums &&
                    (d_column_sums || (d_dual_grads && d_stats)) &&
                    d_workspace && B > 0 && S >= 1 && S <= kMpoMaxSamples && A >= 1 && A <= 64 &&
                    (joint_kl == 0 || joint_kl == 1) && hidden_known(H),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_mpo_actor_grad: bad argument (1 <= samples <= 256, A <= 64)");
  TONIC_REQUIRE(workspace_bytes >= measure<DmpoBuffers>(B, O, A, H, S, NA), TONIC_ERR_WORKSPACE,
                "tonic_mpo_actor_grad: workspace too small");
  hipStream_t st = as_stream(stream);
  const int ldh = pad16(A);
  Workspace ws{static_cast<char*>(d_workspace), 0};
  const DmpoBuffers w(ws, B, O, A, H, S, NA);
  const ActorShape as = actor_shape(O, H, A, 2);
  const SampledDistribution dist{d_values, NA, w.t_logits, nullptr};       // (the E-step needs the rows' means alone)
  TRY(mpo_sampled_values(d_target_actor, d_target_critic, d_norm_mean, d_norm_std, norm_clip,
                         d_observations, d_eps, B, O, H, A, S, w, st, NA != 0 ? &dist : nullptr));
  TRY(actor_forward(d_actor_params, as, d_observations, B, w.o_h1, w.o_h2, w.loc, w.spre, ldh, true,
                    st));
  launch_mpo_state((S + 63) / 64, dim3((B + 3) / 4), st, w.tq, w.act, w.loc_t, w.spre_t, w.loc, w.spre, ldh, d_duals,
                   (float)min_log_dual, action_penalization, joint_kl, w.dloc, w.dspre, w.part, w.klm, w.kls, B, A,
                   S, as.scale_lo, as.scale_hi);
  hipLaunchKernelGGL(mpo_dual_kernel, dim3(1), dim3(1024), 0, st, w.part, w.klm, w.kls, d_duals,
                     (float)min_log_dual, action_penalization, joint_kl, (float)epsilon, (float)epsilon_penalty,
                     (float)epsilon_mean, (float)epsilon_std, d_dual_grads, d_stats,
                     d_grad_sums + actor_count(as), B, A, S, (const double*)nullptr, d_column_sums,
                     B);
  TRY(actor_shaped_backward(d_actor_params, as, d_observations, O, B, w.o_h1, w.o_h2, w.dloc,
                            w.dspre, ldh, w.da_h2, w.da_h1, d_grad_sums, nullptr, 0, 0, st));
  TONIC_CHECK_LAUNCH("tonic_mpo_actor_grad");
  return TONIC_OK;
}

int mpo_dual_step(const double* d_column_sums, float* d_duals, double min_log_dual, float* d_dual_grads,
                  float* d_stats, float* d_actor_stats, int32_t B, int32_t B_global, int32_t A, int32_t S,
                  double epsilon, double epsilon_penalty, double epsilon_mean, double epsilon_std,
                  int32_t action_penalization, int32_t joint_kl, void* stream) {
  TONIC_REQUIRE(d_column_sums && d_duals && d_dual_grads && d_stats && d_actor_stats && B >= 0 &&
                    B_global > 0 && A >= 1 && A <= 64 && S >= 1 && S <= kMpoMaxSamples &&
                    (joint_kl == 0 || joint_kl == 1),
                TONIC_ERR_INVALID_ARGUMENT, "tonic_mpo_dual_step: bad argument (1 <= samples <= 256, A <= 64)");
  hipLaunchKernelGGL(mpo_dual_kernel, dim3(1), dim3(1024), 0, as_stream(stream),
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, d_duals,
                     (float)min_log_dual, action_penalization, joint_kl, (float)epsilon, (float)epsilon_penalty,
                     (float)epsilon_mean, (float)epsilon_std, d_dual_grads, d_stats, d_actor_stats,
                     B, A, S, d_column_sums, (double*)nullptr, B_global);
  TONIC_CHECK_LAUNCH("tonic_mpo_dual_step");
  return TONIC_OK;
}
}  // namespace

extern "C" int tonic_mpo_actor_grad(
    const float* d_actor_params, const float* d_target_actor, const float* d_target_critic,
    float* d_duals, double min_log_dual, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, float* d_grad_sums, float* d_dual_grads,
    float* d_stats, int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, double epsilon,
    double epsilon_penalty, double epsilon_mean, double epsilon_std, int32_t action_penalization,
    void* d_workspace, int64_t workspace_bytes, void* stream) {
  return mpo_actor_grad(d_actor_params, d_target_actor, d_target_critic, d_duals, min_log_dual, d_norm_mean,
                        d_norm_std, norm_clip, d_observations, d_eps, d_grad_sums, d_dual_grads,
                        d_stats, B, O, H, A, S, epsilon, epsilon_penalty, epsilon_mean, epsilon_std,
                        action_penalization, 0, d_workspace, workspace_bytes, stream, nullptr, false);
}

// ... with joint_kl = 1: one alpha pair on the KLs summed over the action dimensions (duals [4], stats [11])
extern "C" int tonic_mpo_actor_grad_joint(
    const float* d_actor_params, const float* d_target_actor, const float* d_target_critic,
    float* d_duals, double min_log_dual, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, float* d_grad_sums, float* d_dual_grads,
    float* d_stats, int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, double epsilon,
    double epsilon_penalty, double epsilon_mean, double epsilon_std, int32_t action_penalization,
    int32_t joint_kl, void* d_workspace, int64_t workspace_bytes, void* stream) {
  return mpo_actor_grad(d_actor_params, d_target_actor, d_target_critic, d_duals, min_log_dual, d_norm_mean,
                        d_norm_std, norm_clip, d_observations, d_eps, d_grad_sums, d_dual_grads,
                        d_stats, B, O, H, A, S, epsilon, epsilon_penalty, epsilon_mean, epsilon_std,
                        action_penalization, joint_kl, d_workspace, workspace_bytes, stream, nullptr, false);
}

extern "C" int tonic_mpo_actor_grad_shard(
    const float* d_actor_params, const float* d_target_actor, const float* d_target_critic,
    float* d_duals, double min_log_dual, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, float* d_grad_sums, double* d_column_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, int32_t action_penalization,
    void* d_workspace, int64_t workspace_bytes, void* stream) {
  return mpo_actor_grad(d_actor_params, d_target_actor, d_target_critic, d_duals, min_log_dual, d_norm_mean,
                        d_norm_std, norm_clip, d_observations, d_eps, d_grad_sums, nullptr, nullptr, B, O, H, A, S,
                        0.0, 0.0, 0.0, 0.0, action_penalization, 0, d_workspace, workspace_bytes, stream, d_column_sums,
                        true);
}

extern "C" int tonic_mpo_actor_grad_shard_joint(
    const float* d_actor_params, const float* d_target_actor, const float* d_target_critic,
    float* d_duals, double min_log_dual, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, float* d_grad_sums, double* d_column_sums,
    int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, int32_t action_penalization, int32_t joint_kl,
    void* d_workspace, int64_t workspace_bytes, void* stream) {
  return mpo_actor_grad(d_actor_params, d_target_actor, d_target_critic, d_duals, min_log_dual, d_norm_mean,
                        d_norm_std, norm_clip, d_observations, d_eps, d_grad_sums, nullptr, nullptr, B, O, H, A, S,
                        0.0, 0.0, 0.0, 0.0, action_penalization, joint_kl, d_workspace, workspace_bytes, stream,
                        d_column_sums, true);
}

// DMPO's actor step: tonic_mpo_actor_grad_joint and its shard form on a categorical target critic (D4PG's layout) —
// the E-step's q[s * B + m] = sum_i softmax(target_critic(s_m, a_s))_i z_i; the dual half is tonic_mpo_dual_step_joint
extern "C" int tonic_distributional_mpo_actor_grad(
    const float* d_actor_params, const float* d_target_actor, const float* d_target_critic,
    float* d_duals, double min_log_dual, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, const float* d_values, float* d_grad_sums, float* d_dual_grads,
    float* d_stats, int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, int32_t NA, double epsilon,
    double epsilon_penalty, double epsilon_mean, double epsilon_std, int32_t action_penalization,
    int32_t joint_kl, void* d_workspace, int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_values != nullptr && NA >= 2 && NA <= 64, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_distributional_mpo_actor_grad: bad argument (2 <= atoms <= 64)");
  return mpo_actor_grad(d_actor_params, d_target_actor, d_target_critic, d_duals, min_log_dual, d_norm_mean,
                        d_norm_std, norm_clip, d_observations, d_eps, d_grad_sums, d_dual_grads,
                        d_stats, B, O, H, A, S, epsilon, epsilon_penalty, epsilon_mean, epsilon_std,
                        action_penalization, joint_kl, d_workspace, workspace_bytes, stream, nullptr, false, d_values,
                        NA);
}

extern "C" int tonic_distributional_mpo_actor_grad_shard(
    const float* d_actor_params, const float* d_target_actor, const float* d_target_critic,
    float* d_duals, double min_log_dual, const float* d_norm_mean, const float* d_norm_std, double norm_clip,
    const float* d_observations, const float* d_eps, const float* d_values, float* d_grad_sums,
    double* d_column_sums, int32_t B, int32_t O, int32_t H, int32_t A, int32_t S, int32_t NA,
    int32_t action_penalization, int32_t joint_kl, void* d_workspace, int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_values != nullptr && NA >= 2 && NA <= 64, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_distributional_mpo_actor_grad_shard: bad argument (2 <= atoms <= 64)");
  return mpo_actor_grad(d_actor_params, d_target_actor, d_target_critic, d_duals, min_log_dual, d_norm_mean,
                        d_norm_std, norm_clip, d_observations, d_eps, d_grad_sums, nullptr, nullptr, B, O, H, A, S,
                        0.0, 0.0, 0.0, 0.0, action_penalization, joint_kl, d_workspace, workspace_bytes, stream,
                        d_column_sums, true, d_values, NA);
}

extern "C" int tonic_mpo_dual_step(const double* d_column_sums, float* d_duals, double min_log_dual,
                                   float* d_dual_grads, float* d_stats, float* d_actor_stats,
                                   int32_t B, int32_t B_global, int32_t A, int32_t S,
                                   double epsilon, double epsilon_penalty, double epsilon_mean,
                                   double epsilon_std, int32_t action_penalization, void* stream) {
  return mpo_dual_step(d_column_sums, d_duals, min_log_dual, d_dual_grads, d_stats, d_actor_stats, B, B_global, A, S,
                       epsilon, epsilon_penalty, epsilon_mean, epsilon_std, action_penalization, 0, stream);
}

extern "C" int tonic_mpo_dual_step_joint(const double* d_column_sums, float* d_duals, double min_log_dual,
                                         float* d_dual_grads, float* d_stats, float* d_actor_stats,
                                         int32_t B, int32_t B_global, int32_t A, int32_t S,
                                         double epsilon, double epsilon_penalty, double epsilon_mean,
                                         double epsilon_std, int32_t action_penalization, int32_t joint_kl,
                                         void* stream) {
  return mpo_dual_step(d_column_sums, d_duals, min_log_dual, d_dual_grads, d_stats, d_actor_stats, B, B_global, A, S,
                       epsilon, epsilon_penalty, epsilon_mean, epsilon_std, action_penalization, joint_kl, stream);
}

extern "C" int tonic_buffer_gather(const int64_t* d_indices, const float* d_buf_observations,
                                   const float* d_buf_actions,
                                   const float* d_buf_next_observations,
                                   const float* d_buf_rewards, const float* d_buf_discounts,
                                   float* d_observations, float* d_actions,
                                   float* d_next_observations, float* d_rewards,
                                   float* d_discounts, int64_t W, int32_t B, int32_t O, int32_t A,
                                   void* stream) {
  TONIC_REQUIRE(d_indices && d_buf_observations && d_buf_actions && d_buf_next_observations &&
                    d_buf_rewards && d_buf_discounts && d_observations && d_actions &&
                    d_next_observations && d_rewards && d_discounts && W > 0 && B > 0 && O > 0 && A > 0,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_buffer_gather: bad argument");
  GatherArgs g{d_indices, d_buf_observations, d_buf_actions, d_buf_next_observations,
               d_buf_rewards, d_buf_discounts, d_observations, d_actions, d_next_observations,
               d_rewards, d_discounts, W, B, O, A};
  hipLaunchKernelGGL(buffer_gather_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(stream), g);
  TONIC_CHECK_LAUNCH("tonic_buffer_gather");
  return TONIC_OK;
}

extern "C" int tonic_buffer_accumulate_n_steps(float* d_buf_next_observations,
                                               float* d_buf_rewards, float* d_buf_discounts,
                                               const float* d_buf_resets,
                                               const float* d_next_observations,
                                               const float* d_rewards,
                                               const float* d_terminations, int64_t row,
                                               int64_t size, int64_t max_size, int64_t W,
                                               int32_t O, int32_t return_steps,
                                               double discount_factor, void* stream) {
  TONIC_REQUIRE(d_buf_next_observations && d_buf_rewards && d_buf_discounts && d_buf_resets &&
                    d_next_observations && d_rewards && d_terminations,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_buffer_accumulate_n_steps: null pointer");
  TONIC_REQUIRE(row >= 0 && row < max_size && size >= 0 && size <= max_size && W > 0 && O > 0 &&
                    return_steps >= 1,
                TONIC_ERR_INVALID_ARGUMENT,
                "tonic_buffer_accumulate_n_steps: row=%lld size=%lld max_size=%lld W=%lld O=%d "
                "return_steps=%d", (long long)row, (long long)size, (long long)max_size,
                (long long)W, O, return_steps);
  const int64_t back = size < return_steps - 1 ? size : return_steps - 1;      // buffers.py:64
  if (back == 0) return TONIC_OK;
  NStepArgs a{d_buf_next_observations, d_buf_rewards, d_buf_discounts, d_buf_resets,
              d_next_observations, d_rewards, d_terminations, row, size, max_size, W, O,
              (int)back, (float)discount_factor};
  const int64_t blocks = (W * O + 255) / 256;
  hipLaunchKernelGGL(buffer_nstep_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a);
  TONIC_CHECK_LAUNCH("tonic_buffer_accumulate_n_steps");
  return TONIC_OK;
}

extern "C" int tonic_buffer_store(float* d_buf_observations, float* d_buf_actions,
                                  float* d_buf_next_observations, float* d_buf_rewards,
                                  float* d_buf_resets, float* d_buf_terminations,
                                  float* d_buf_discounts, const float* d_observations,
                                  const float* d_actions, const float* d_next_observations,
                                  const float* d_rewards, const float* d_resets,
                                  const float* d_terminations, float* d_norm_acc, int64_t row,
                                  int64_t W, int32_t O, int32_t A, double discount_factor,
                                  void* stream) {
  TONIC_REQUIRE(d_buf_observations && d_buf_actions && d_buf_next_observations &&
                    d_buf_rewards && d_buf_resets && d_buf_terminations && d_buf_discounts &&
                    d_observations && d_actions && d_next_observations && d_rewards && d_resets &&
                    d_terminations && row >= 0 && W > 0 && O > 0 && O <= 1024 && A > 0,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_buffer_store: bad argument");
  BufferStoreArgs a{d_buf_observations, d_buf_actions, d_buf_next_observations, d_buf_rewards,
                    d_buf_resets, d_buf_terminations, d_buf_discounts, d_observations, d_actions,
                    d_next_observations, d_rewards, d_resets, d_terminations, d_norm_acc, row, W,
                    O, A, (float)discount_factor};
  int64_t blocks = (W * (2 * O + A + 4) + 8 * 1024 - 1) / (8 * 1024);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(buffer_store_kernel, dim3((unsigned)blocks), dim3(1024), 0,
                     as_stream(stream), a);
  TONIC_CHECK_LAUNCH("tonic_buffer_store");
  return TONIC_OK;
}
