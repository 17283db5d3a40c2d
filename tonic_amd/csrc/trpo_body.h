// TRPO's actor step (tonic/torch/updaters/actors.py:115-156, optimizers.py:25-115) on the layer-by-layer path.
// Included at the end of mlpwide.hip: it shares that file's dense / wgrad kernels, WideLayout, wide_forward and
// wide_backward.
//
// The parameters do not move while the conjugate-gradient loop runs, so ONE forward pass per update
// (tonic_trpo_prepare) leaves the hidden activations h_l, the locations mu_o and the scales sigma_o in the
// workspace; every Fisher-vector product reuses them.  With (mu_o, sigma_o) this very network's outputs the
// gradient of the KL with respect to (mu, sigma) vanishes, and the Hessian that the reference takes by double
// backward is the Gauss-Newton product F v = J^T M J v:
//
//   tangent_kernel      t'_l = act'(h_l) * (t'_{l-1} W_l^T + h_{l-1} V_l^T + v_b): ONE launch per layer, both
//                       products on fp32 MFMA 16x16x4 tiles into the same accumulators, W and V staged side by
//                       side in LDS as dense_kernel stages W (the first layer has t'_0 = 0 and is a dense_kernel
//                       launch over the observations; the head is the same kernel with act' = 1 - mu^2)
//   trpo_metric_kernel  dz_head = mu' / sigma_o^2 * (1 - mu^2) in place, and the log_scale slot of the partial
//                       images: rows * 2 sigma' / sigma_o^2 (reduce_partials_kernel applies softplus' and the
//                       clamp's convention, as for every actor gradient)
//   wide_backward       as for the loss gradient, from that head gradient
//   trpo_eval_kernel    a line-search trial: {sum of -ratio * adv, sum of (mu - mu_o)^2 / (2 sigma_o^2)} per slab
//                       in float64; trpo_eval_reduce_kernel folds the slabs in a fixed order and adds the terms
//                       that do not depend on the sample (entropy, the scales' share of the KL)
//
// The surrogate loss's gradient is ppo_loss_kernel with an unbounded clip range on the prepared activations.

namespace tonic {
namespace {

struct TangentArgs {
  const float* X1; const float* X2; int ldx;   // [N, K]: tangent and activations of the layer below
  const float* W; const float* V;              // [NOUT, K] each (row pitch K): the parameters, v's slice
  const float* bias;                           // [NOUT]: v's bias slice
  const float* D; int dkind;                   // [N, ldy]: this layer's activations; 1 tanh: 1 - D^2, 2 ReLU: D > 0
  float* Y; int ldy;
  int64_t N;
  int K, NOUT;                                 // K: a multiple of 4 (a hidden layer's width)
};

// TN = feature tiles of 16 outputs (NOUT <= 16 * TN).  Rows of X1 / X2 are 16-byte aligned multiples of four
// columns, so a lane's four k-steps are one 16-byte load (dense_kernel's `vec` form): k = 16 (st / 4) + 4 g + st % 4.
template <int TN>
__global__ __launch_bounds__(kWideThreads) void tangent_kernel(TangentArgs a) {
  extern __shared__ float wl[];                // [2][TN][KS][64]: A-operand images of W and of V
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KS = 4 * ((a.K + 15) >> 4);
  const int image = TN * KS * 64;
  for (int idx = tid; idx < 2 * image; idx += kWideThreads) wl[idx] = 0.f;
  __syncthreads();
  {
    const int total = a.NOUT * a.K;
    for (int m = 0; m < 2; ++m) {
      const float* src = m == 0 ? a.W : a.V;
      float* dst = wl + m * image;
      for (int base = tid; base < total; base += 16 * kWideThreads) {
        float w[16];
        int slot[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int f = base + u * kWideThreads;
          const bool live = f < total;
          const int j = live ? f / a.K : 0, k = live ? f - j * a.K : 0;
          w[u] = src[live ? f : 0];
          const int st = 4 * (k >> 4) + (k & 3), gg = (k >> 2) & 3;
          slot[u] = live ? ((j >> 4) * KS + st) * 64 + gg * 16 + (j & 15) : -1;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (slot[u] >= 0) dst[slot[u]] = w[u];
      }
    }
  }
  __syncthreads();
  const int s = lane & 15, g = lane >> 4;
  const int64_t tiles = (a.N + 15) >> 4, stride = (int64_t)gridDim.x * 4;
  constexpr int kChunk = 16;
  // (as in dense_kernel: the next chunk's loads are in flight under this chunk's MFMAs; addresses are clamped
  //  and the padding is masked at the consumer)
  auto load_chunk = [&](const float* X, int64_t t, int c0, float (&xv)[kChunk]) {
    const int64_t row = t * 16 + s;
    const float* x = X + (row < a.N ? row : a.N - 1) * a.ldx;
#pragma unroll
    for (int q = 0; q < kChunk / 4; ++q) {
      const int col = 16 * ((c0 >> 2) + q) + 4 * g;
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + (col < a.K ? col : 0));
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[4 * q + e] = v[e];
    }
  };
  float cur1[kChunk], cur2[kChunk], nxt1[kChunk], nxt2[kChunk];
  int64_t t = (int64_t)blockIdx.x * 4 + wave;
  int c0 = 0;
  if (t < tiles) {
    load_chunk(a.X1, t, 0, cur1);
    load_chunk(a.X2, t, 0, cur2);
  }
  f32x4 acc[TN];
#pragma unroll
  for (int T = 0; T < TN; ++T) acc[T] = f32x4{0.f, 0.f, 0.f, 0.f};
  while (t < tiles) {
    const bool last_chunk = c0 + kChunk >= KS;
    const int64_t t_next = last_chunk ? t + stride : t;
    const int c_next = last_chunk ? 0 : c0 + kChunk;
    if (t_next < tiles) {
      load_chunk(a.X1, t_next, c_next, nxt1);
      load_chunk(a.X2, t_next, c_next, nxt2);
    }
    const int64_t row = t * 16 + s;
    const bool valid = row < a.N;
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      const int st = c0 + u, k = 16 * (st >> 2) + 4 * g + (st & 3);
      if (st < KS) {                                   // (uniform)
        const bool live = valid && k < a.K;
        const float v1 = live ? cur1[u] : 0.f, v2 = live ? cur2[u] : 0.f;
#pragma unroll
        for (int T = 0; T < TN; ++T) {
          acc[T] = mfma16w(wl[(T * KS + st) * 64 + lane], v1, acc[T]);
          acc[T] = mfma16w(wl[image + (T * KS + st) * 64 + lane], v2, acc[T]);
        }
      }
    }
    if (last_chunk) {
      if (valid && (a.NOUT & 3) == 0 && (a.ldy & 3) == 0) {
#pragma unroll
        for (int T = 0; T < TN; ++T) {
          const int j = 16 * T + 4 * g;
          if (j < a.NOUT) {
            f32x4 v = acc[T];
            const f32x4 d = *reinterpret_cast<const f32x4*>(a.D + row * a.ldy + j);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = wide_derivative(v[r] + a.bias[j + r], d[r], a.dkind);
            *reinterpret_cast<f32x4*>(a.Y + row * a.ldy + j) = v;
          }
        }
      } else if (valid) {
#pragma unroll
        for (int T = 0; T < TN; ++T) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = 16 * T + 4 * g + r;
            if (j < a.NOUT)
              a.Y[row * a.ldy + j] = wide_derivative(acc[T][r] + a.bias[j], a.D[row * a.ldy + j], a.dkind);
          }
        }
      }
#pragma unroll
      for (int T = 0; T < TN; ++T) acc[T] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < kChunk; ++u) {
      cur1[u] = nxt1[u];
      cur2[u] = nxt2[u];
    }
    t = t_next;
    c0 = c_next;
  }
}

// Two weight images share the LDS: slices of 64 outputs up to 256 inputs (128 KB), of 32 beyond (96 KB).
constexpr int kTangentMaxLds = 2 * 4 * 64 * 64 * 4;

int launch_tangent_slice(const TangentArgs& a, hipStream_t st) {
  const int tiles_out = (a.NOUT + 15) / 16, ks = 4 * ((a.K + 15) / 16);
  const int tn = tiles_out <= 1 ? 1 : tiles_out == 2 ? 2 : 4;
  const int lds_bytes = 2 * tn * ks * 64 * 4;
  const int64_t tiles = (a.N + 15) / 16;
  int64_t blocks = (tiles + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  auto go = [&](auto kernel) {
    static thread_local bool configured = false;           // (one flag per instantiation)
    if (!configured) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, kTangentMaxLds);
      if (e != hipSuccess) {
        set_error("trpo: %d B of LDS for the weight images: %s", kTangentMaxLds, hipGetErrorString(e));
        return (int)TONIC_ERR_LAUNCH;
      }
      configured = true;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kWideThreads), lds_bytes, st, a);
    return (int)TONIC_OK;
  };
  int rc;
  if (tn <= 1) rc = go(tangent_kernel<1>);
  else if (tn == 2) rc = go(tangent_kernel<2>);
  else rc = go(tangent_kernel<4>);
  if (rc != TONIC_OK) return rc;
  TONIC_CHECK_LAUNCH("tangent_kernel");
  return TONIC_OK;
}

int launch_tangent(const TangentArgs& a, hipStream_t st) {
  const int width = a.K <= 256 ? 64 : 32;
  for (int j0 = 0; j0 < a.NOUT; j0 += width) {
    TangentArgs d = a;
    d.NOUT = a.NOUT - j0 < width ? a.NOUT - j0 : width;
    d.W = a.W + (int64_t)j0 * a.K; d.V = a.V + (int64_t)j0 * a.K;
    d.bias = a.bias + j0; d.D = a.D + j0; d.Y = a.Y + j0;
    if (int rc = launch_tangent_slice(d, st)) return rc;
  }
  return TONIC_OK;
}

// sigma = clamp(softplus(log_scale) + FLOAT_EPSILON, scale_min, scale_max) (actors.py:63-64), as every kernel
// of this file forms it
__device__ __forceinline__ float trpo_sigma(float ls) {
  const float sp = ls > 20.f ? ls : log1pf(expf(ls));
  return fminf(fmaxf(sp + 1e-8f, 1e-4f), 1.0f);
}

// The same in float64 from the float32 log_scale: a line-search trial's KL holds log(sigma_o / sigma) +
// sigma^2 / (2 sigma_o^2) - 1/2 ~ (d sigma / sigma)^2, where a float32 sigma's rounding alone is 1e-5 of the term
// at a step of 1e-2
__device__ __forceinline__ double trpo_sigma64(float ls) {
  const double s = (double)ls;
  const double sp = s > 40.0 ? s : log1p(exp(s));
  return fmin(fmax(sp + 1e-8, 1e-4), 1.0);
}

// prepare: sigma_o into the workspace (float32, and float64 for the trials' KL) and out, the constant {mean 0, std 1, not all zero, do not normalise}
// that ppo_loss_kernel reads its advantage statistics from
__global__ void trpo_sigma_kernel(const float* log_scale, int A, float* sigma_ws, double* sigma64_ws,
                                  float* adv_stats, float* sigma_out) {
  const int tid = threadIdx.x;
  if (tid < A) {
    const float sigma = trpo_sigma(log_scale[tid]);
    sigma_ws[tid] = sigma;
    sigma64_ws[tid] = trpo_sigma64(log_scale[tid]);
    if (sigma_out != nullptr) sigma_out[tid] = sigma;
  }
  if (tid < 4) adv_stats[tid] = tid == 1 ? 1.f : 0.f;
}

struct MetricArgs {
  float* dzh; const float* mu; int ld;         // [N, ld]: mu' in, d / d (pre-tanh) out; mu_o
  const float* sigma_o; const float* log_scale; const float* v_log_scale;
  float* image; int pstride; int ls_offset; int P;
  int64_t N, slab;
  int A;
};

__global__ __launch_bounds__(kWideThreads) void trpo_metric_kernel(MetricArgs a) {
  __shared__ float inv_var_s[kWideLd];
  const int tid = threadIdx.x;
  const int64_t r_begin = (int64_t)blockIdx.x * a.slab, r_end = min(a.N, r_begin + a.slab);
  const int64_t rows = r_end > r_begin ? r_end - r_begin : 0;
  if (tid < kWideLd) {
    const float so = tid < a.A ? a.sigma_o[tid] : 1.f;
    inv_var_s[tid] = 1.f / (so * so);
  }
  __syncthreads();
  float* image = a.image + (int64_t)blockIdx.x * a.pstride;
  if (tid < a.A) {
    // sigma' = d sigma / d log_scale * v: softplus' inside the clamp, 0 outside (reduce_partials_kernel's
    // convention at the edges); c_sigma = 2 sigma' / sigma_o^2 for each of this slab's rows
    const float ls = a.log_scale[tid];
    const float sp = ls > 20.f ? ls : log1pf(expf(ls));
    const float raw = sp + 1e-8f;
    const bool inside = raw >= 1e-4f && raw <= 1.0f;
    const float sigma_dot = inside ? a.v_log_scale[tid] / (1.f + expf(-ls)) : 0.f;
    image[a.ls_offset + tid] = (float)((double)rows * (double)(2.f * sigma_dot * inv_var_s[tid]));
  }
  if (tid < kStatSlots) image[a.P + tid] = 0.f;
  for (int64_t i = r_begin * a.ld + tid; i < r_end * a.ld; i += kWideThreads) {
    const int aa = (int)(i % a.ld);
    if (aa < a.A) {
      const float m = a.mu[i];
      a.dzh[i] = (a.dzh[i] * inv_var_s[aa]) * (1.f - m * m);
    }
  }
}

struct EvalArgs {
  const float* mu; const float* mu_o; int ld;  // [N, ld]: the trial's locations, the prepared ones
  const float* sigma_o; const float* log_scale;        // prepared scales; the TRIAL's log_scale
  const float* actions; const float* adv; const float* old_logp;
  double* partials;                            // [blocks][2]
  int64_t N, slab;
  int A;
};

__global__ __launch_bounds__(kWideThreads) void trpo_eval_kernel(EvalArgs a) {
  __shared__ float half_inv_var_s[kWideLd], logc_s[kWideLd], half_inv_var_o_s[kWideLd];
  __shared__ double red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < a.A) {
    const float sigma = trpo_sigma(a.log_scale[tid]), so = a.sigma_o[tid];
    half_inv_var_s[tid] = 1.0f / (2.0f * (sigma * sigma));
    logc_s[tid] = logf(sigma) + kLogSqrt2Pi;
    half_inv_var_o_s[tid] = 1.0f / (2.0f * (so * so));
  }
  __syncthreads();
  double loss = 0.0, kl = 0.0;
  const int64_t r_begin = (int64_t)blockIdx.x * a.slab, r_end = min(a.N, r_begin + a.slab);
  for (int64_t n = r_begin + tid; n < r_end; n += kWideThreads) {
    // The float32 terms are summed in float64: at A = 32 the log-probability is ~ -40, where every float32
    // addition rounds by 2e-6 — 32 of them left 5e-6 in each ratio and 1.1e-5 (c = 0) / 1.7e-5 (c = 0.01) of the
    // loss sum of 333 rows of (4, 32) on a (384, 260) torso, whose terms cancel to a thirtieth of their size.
    double logp = 0.0;
    float moved = 0.f;
    for (int aa = 0; aa < a.A; ++aa) {
      const float m = a.mu[n * a.ld + aa];
      const float dif = a.actions[n * a.A + aa] - m, dm = m - a.mu_o[n * a.ld + aa];
      logp += (double)(-(dif * dif) * half_inv_var_s[aa] - logc_s[aa]);
      moved += (dm * dm) * half_inv_var_o_s[aa];
    }
    loss -= (double)(a.adv[n] * __expf((float)(logp - (double)a.old_logp[n])));      // actors.py:145-147
    kl += (double)moved;
  }
  loss = wave_sum(loss); kl = wave_sum(kl);
  if (lane == 0) { red[wave][0] = loss; red[wave][1] = kl; }
  __syncthreads();
  if (tid < 2)
    a.partials[2 * (int64_t)blockIdx.x + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// {loss_sum, kl_sum}: the slabs' float64 partials in a fixed order, plus what no sample changes — per row
// -entropy_coeff * mean_A(entropy) (actors.py:148-149) and sum_A(log(sigma_o / sigma) + sigma^2 / (2 sigma_o^2)
// - 1/2) (the scales' share of Normal's kl_divergence)
__global__ __launch_bounds__(kWideThreads) void trpo_eval_reduce_kernel(
    const double* partials, int blocks, const double* sigma_o, const float* log_scale, int A, double rows,
    double entropy_coeff, float* out) {
  __shared__ double red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double loss = 0.0, kl = 0.0;
  for (int b = tid; b < blocks; b += kWideThreads) {
    loss += partials[2 * b];
    kl += partials[2 * b + 1];
  }
  loss = wave_sum(loss); kl = wave_sum(kl);
  if (lane == 0) { red[wave][0] = loss; red[wave][1] = kl; }
  __syncthreads();
  if (tid != 0) return;
  loss = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
  kl = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
  double entropy = 0.0, scales = 0.0;
  for (int aa = 0; aa < A; ++aa) {
    const double sigma = trpo_sigma64(log_scale[aa]), so = sigma_o[aa];
    entropy += (double)kEntropyConst + log(sigma);
    scales += log(so / sigma) + (sigma * sigma) / (2.0 * so * so) - 0.5;
  }
  out[0] = (float)(loss - entropy_coeff * (entropy / A) * rows);
  out[1] = (float)(kl + scales * rows);
}

// The workspace: WideLayout's scratch (prepared h_l and mu_o; head / hidden gradients and partial images that
// loss_grad and fisher_vector rewrite), the prepared sigma_o with ppo_loss_kernel's advantage constants, and
// two row buffers of the widest layer: the tangents of alternate layers, or a trial's hidden activations.
struct TrpoLayout {
  static_assert(kWideLd == 32, "the sigma block below holds kWideLd floats, 4 constants, kWideLd doubles");
  WideLayout L;
  int64_t off_sigma, off_t[2], bytes;
  TrpoLayout(int64_t n, int O, int A, const Torso& t) : L(n, O, A, true, t) {
    // mu and mu_o differ by the step only: tanh_fast's 2e-7 would be 1e-5 of (mu - mu_o)^2 at a step of 1e-2
    L.head_act = 3;
    int widest = 0;
    for (int l = 0; l < t.layers; ++l) widest = t.size[l] > widest ? t.size[l] : widest;
    off_sigma = L.bytes;
    off_t[0] = off_sigma + 512;            // float32 sigma_o [32], advantage constants [4]; float64 sigma_o [32]
    off_t[1] = off_t[0] + round_up(n * widest * 4, 256);
    bytes = off_t[1] + round_up(n * widest * 4, 256);
  }
  float* sigma(char* ws) const { return reinterpret_cast<float*>(ws + off_sigma); }
  float* adv_stats(char* ws) const { return reinterpret_cast<float*>(ws + off_sigma) + kWideLd; }
  double* sigma64(char* ws) const { return reinterpret_cast<double*>(ws + off_sigma + 256); }
};

int trpo_torso(const char* what, int32_t layers, const int32_t* sizes, int32_t activation, int64_t n,
               int32_t O, int32_t A, Torso& t) {
  if (int rc = parse_torso(what, layers, sizes, activation, t)) return rc;
  TONIC_REQUIRE(wide_supported(O, A, true), TONIC_ERR_UNSUPPORTED_SHAPE,
                "%s: %d observations / %d actions (1 .. 384 / 1 .. %d are served)", what, O, A, kWideLd);
  TONIC_REQUIRE(n > 0, TONIC_ERR_INVALID_ARGUMENT, "%s: %lld rows", what, (long long)n);
  return TONIC_OK;
}

}  // namespace
}  // namespace tonic

using namespace tonic;

extern "C" int64_t tonic_trpo_workspace_bytes(int64_t n, int32_t O, int32_t A, int32_t layers,
                                              const int32_t* sizes) {
  Torso t;
  if (trpo_torso("tonic_trpo_workspace_bytes", layers, sizes, 1, n, O, A, t) != TONIC_OK) return -1;
  return TrpoLayout(n, O, A, t).bytes;
}

extern "C" int tonic_trpo_prepare(int32_t layers, const int32_t* sizes, int32_t activation,
                                  const float* d_actor_params, const float* d_observations, int64_t n,
                                  int32_t O, int32_t A, float* d_locs, float* d_scales, void* d_workspace,
                                  int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_actor_params && d_observations, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_trpo_prepare: null argument");
  Torso t;
  if (int rc = trpo_torso("tonic_trpo_prepare", layers, sizes, activation, n, O, A, t)) return rc;
  const TrpoLayout T(n, O, A, t);
  TONIC_REQUIRE(d_workspace && workspace_bytes >= T.bytes, TONIC_ERR_WORKSPACE,
                "tonic_trpo_prepare: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)T.bytes);
  char* ws = static_cast<char*>(d_workspace);
  hipStream_t st = as_stream(stream);
  if (int rc = wide_forward(d_actor_params, T.L, d_observations, n, O, A, true, nullptr, nullptr, 0.f, ws,
                            nullptr, st))
    return rc;
  hipLaunchKernelGGL(trpo_sigma_kernel, dim3(1), dim3(64), 0, st, d_actor_params + T.L.ls, A, T.sigma(ws),
                     T.sigma64(ws), T.adv_stats(ws), d_scales);
  TONIC_CHECK_LAUNCH("trpo_sigma_kernel");
  if (d_locs != nullptr) {                     // [n, A] out of the scratch's rows of kWideLd
    int64_t blocks = (n + kWideThreads - 1) / kWideThreads;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)blocks), dim3(kWideThreads), 0, st,
                       reinterpret_cast<const float*>(ws + T.L.off_out), kWideLd, d_actor_params + T.L.ls,
                       (const float*)nullptr, d_locs, (float*)nullptr, n, A);
    TONIC_CHECK_LAUNCH("sample_kernel");
  }
  return TONIC_OK;
}

extern "C" int tonic_trpo_loss_grad(int32_t layers, const int32_t* sizes, int32_t activation,
                                    const float* d_actor_params, const float* d_observations,
                                    const float* d_actions, const float* d_advantages,
                                    const float* d_old_log_probs, float* d_grad_sums, int64_t n, int32_t O,
                                    int32_t A, double entropy_coeff, void* d_workspace,
                                    int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_actor_params && d_observations && d_actions && d_advantages && d_old_log_probs &&
                    d_grad_sums,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_trpo_loss_grad: null argument");
  Torso t;
  if (int rc = trpo_torso("tonic_trpo_loss_grad", layers, sizes, activation, n, O, A, t)) return rc;
  const TrpoLayout T(n, O, A, t);
  const WideLayout& L = T.L;
  TONIC_REQUIRE(d_workspace && workspace_bytes >= T.bytes, TONIC_ERR_WORKSPACE,
                "tonic_trpo_loss_grad: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)T.bytes);
  char* ws = static_cast<char*>(d_workspace);
  hipStream_t st = as_stream(stream);
  PpoLossArgs l{};
  l.loc = reinterpret_cast<float*>(ws + L.off_out);
  l.dz3 = reinterpret_cast<float*>(ws + L.off_dzh);
  l.ld = kWideLd; l.actions = d_actions; l.adv = d_advantages; l.adv_stats = T.adv_stats(ws);
  l.old_logp = d_old_log_probs; l.log_scale = d_actor_params + L.ls;
  l.image = reinterpret_cast<float*>(ws + L.off_image); l.pstride = (int)L.pstride;
  l.ls_offset = L.ls; l.P = L.P; l.N = n; l.slab = L.slab; l.A = A;
  l.clip_lo = -__builtin_huge_valf(); l.clip_hi = __builtin_huge_valf();    // actors.py:147: no clipping
  l.plain = 0; l.skip = nullptr;
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(L.blocks), dim3(kWideThreads), 0, st, l);
  TONIC_CHECK_LAUNCH("ppo_loss_kernel");
  if (int rc = wide_backward(d_actor_params, L, d_observations, n, O, A, true, nullptr, nullptr, 0.f, ws,
                             nullptr, st))
    return rc;
  return launch_reduce_partials(true, l.image, L.blocks, (int)L.pstride, L.P, d_actor_params, d_grad_sums,
                                O, A, (float)entropy_coeff, (double)n, nullptr, st, L.ls);
}

extern "C" int tonic_trpo_fisher_vector(int32_t layers, const int32_t* sizes, int32_t activation,
                                        const float* d_actor_params, const float* d_observations,
                                        const float* d_vector, float* d_out_sums, int64_t n, int32_t O,
                                        int32_t A, void* d_workspace, int64_t workspace_bytes,
                                        void* stream) {
  TONIC_REQUIRE(d_actor_params && d_observations && d_vector && d_out_sums, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_trpo_fisher_vector: null argument");
  Torso t;
  if (int rc = trpo_torso("tonic_trpo_fisher_vector", layers, sizes, activation, n, O, A, t)) return rc;
  const TrpoLayout T(n, O, A, t);
  const WideLayout& L = T.L;
  TONIC_REQUIRE(d_workspace && workspace_bytes >= T.bytes, TONIC_ERR_WORKSPACE,
                "tonic_trpo_fisher_vector: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)T.bytes);
  char* ws = static_cast<char*>(d_workspace);
  hipStream_t st = as_stream(stream);
  // t'_1 = act'(h_1) * (x V_1^T + v_b1): the tangent of the observations is zero
  {
    DenseArgs d{};
    d.X = d_observations; d.ldx = O; d.K = O; d.N = n;
    d.W = d_vector + L.W[0]; d.ldw = O; d.bias = d_vector + L.b[0];
    d.D = reinterpret_cast<const float*>(ws + L.off_h[0]); d.dkind = t.act;
    d.Y = reinterpret_cast<float*>(ws + T.off_t[0]); d.ldy = t.size[0]; d.NOUT = t.size[0];
    if (int rc = launch_dense(d, st)) return rc;
  }
  TangentArgs g{};
  g.N = n;
  for (int l = 1; l <= t.layers; ++l) {
    const bool head = l == t.layers;
    g.X1 = reinterpret_cast<const float*>(ws + T.off_t[(l - 1) & 1]);
    g.X2 = reinterpret_cast<const float*>(ws + L.off_h[l - 1]);
    g.ldx = g.K = t.size[l - 1];
    const int w = head ? L.Wh : L.W[l], b = head ? L.bh : L.b[l];
    g.W = d_actor_params + w; g.V = d_vector + w; g.bias = d_vector + b;
    g.D = reinterpret_cast<const float*>(ws + (head ? L.off_out : L.off_h[l]));
    g.dkind = head ? 1 : t.act;                // loc_activation Tanh: mu' = (1 - mu^2) * (...)
    g.Y = reinterpret_cast<float*>(ws + (head ? L.off_dzh : T.off_t[l & 1]));
    g.ldy = head ? kWideLd : t.size[l];
    g.NOUT = head ? A : t.size[l];
    if (int rc = launch_tangent(g, st)) return rc;
  }
  MetricArgs m{};
  m.dzh = reinterpret_cast<float*>(ws + L.off_dzh);
  m.mu = reinterpret_cast<const float*>(ws + L.off_out); m.ld = kWideLd;
  m.sigma_o = T.sigma(ws); m.log_scale = d_actor_params + L.ls; m.v_log_scale = d_vector + L.ls;
  m.image = reinterpret_cast<float*>(ws + L.off_image); m.pstride = (int)L.pstride;
  m.ls_offset = L.ls; m.P = L.P; m.N = n; m.slab = L.slab; m.A = A;
  hipLaunchKernelGGL(trpo_metric_kernel, dim3(L.blocks), dim3(kWideThreads), 0, st, m);
  TONIC_CHECK_LAUNCH("trpo_metric_kernel");
  if (int rc = wide_backward(d_actor_params, L, d_observations, n, O, A, true, nullptr, nullptr, 0.f, ws,
                             nullptr, st))
    return rc;
  return launch_reduce_partials(true, m.image, L.blocks, (int)L.pstride, L.P, d_actor_params, d_out_sums, O,
                                A, 0.f, (double)n, nullptr, st, L.ls);
}

extern "C" int tonic_trpo_evaluate(int32_t layers, const int32_t* sizes, int32_t activation,
                                   const float* d_trial_params, const float* d_observations,
                                   const float* d_actions, const float* d_advantages,
                                   const float* d_old_log_probs, int64_t n, int32_t O, int32_t A,
                                   double entropy_coeff, float* d_out, void* d_workspace,
                                   int64_t workspace_bytes, void* stream) {
  TONIC_REQUIRE(d_trial_params && d_observations && d_actions && d_advantages && d_old_log_probs && d_out,
                TONIC_ERR_INVALID_ARGUMENT, "tonic_trpo_evaluate: null argument");
  Torso t;
  if (int rc = trpo_torso("tonic_trpo_evaluate", layers, sizes, activation, n, O, A, t)) return rc;
  const TrpoLayout T(n, O, A, t);
  TONIC_REQUIRE(d_workspace && workspace_bytes >= T.bytes, TONIC_ERR_WORKSPACE,
                "tonic_trpo_evaluate: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)T.bytes);
  char* ws = static_cast<char*>(d_workspace);
  hipStream_t st = as_stream(stream);
  // forward at the trial parameters into scratch that fisher_vector rewrites anyway: hidden activations in
  // the tangent buffers, locations where the head gradient goes; h_l and mu_o stay as prepared
  WideLayout E = T.L;
  for (int l = 0; l < t.layers; ++l) E.off_h[l] = T.off_t[l & 1];
  E.off_out = T.L.off_dzh;
  if (int rc = wide_forward(d_trial_params, E, d_observations, n, O, A, true, nullptr, nullptr, 0.f, ws,
                            nullptr, st))
    return rc;
  EvalArgs e{};
  e.mu = reinterpret_cast<const float*>(ws + E.off_out);
  e.mu_o = reinterpret_cast<const float*>(ws + T.L.off_out); e.ld = kWideLd;
  e.sigma_o = T.sigma(ws); e.log_scale = d_trial_params + T.L.ls;
  e.actions = d_actions; e.adv = d_advantages; e.old_logp = d_old_log_probs;
  e.partials = reinterpret_cast<double*>(ws + T.L.off_image);      // (blocks * pstride * 4 >= blocks * 16 bytes)
  e.N = n; e.slab = T.L.slab; e.A = A;
  hipLaunchKernelGGL(trpo_eval_kernel, dim3(T.L.blocks), dim3(kWideThreads), 0, st, e);
  TONIC_CHECK_LAUNCH("trpo_eval_kernel");
  hipLaunchKernelGGL(trpo_eval_reduce_kernel, dim3(1), dim3(kWideThreads), 0, st, e.partials, T.L.blocks,
                     T.sigma64(ws), e.log_scale, A, (double)n, entropy_coeff, d_out);
  TONIC_CHECK_LAUNCH("trpo_eval_reduce_kernel");
  return TONIC_OK;
}
