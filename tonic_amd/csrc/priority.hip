// Priority tree of the prioritized replay (gfx950): proportional sampling P_i = leaf_i / sum_j leaf_j on the device,
// between the critic steps of one update call.
//
// One device block per replay:
//   [0, 64)          float32 max_leaf (the priority a freshly stored transition gets), initialised to 1
//   level 0          float32 [pad64(capacity)]: the leaves, one per flat transition index row * W + col;
//                    (loss + epsilon)^alpha, 0 for a slot never stored and for the padding
//   level l >= 1     float64 [pad64(n_l)], n_l = ceil(n_{l-1} / 64): node k is the sum of its 64 children
//                    64 k .. 64 k + 63 of level l - 1 IN ASCENDING ORDER, zero behind n_l
// The levels stop at the first one with <= 64 nodes (the leaves themselves for a capacity <= 64); the total is the
// ascending sum of that level.  A node is always RECOMPUTED from its children, never adjusted by a difference: no
// drift, no atomics, and the same inputs give the same bits.  Every level is padded to a multiple of 64 entries, so
// a scan of one node's 64 children never leaves the block.
#include <cmath>

#include "common.h"

namespace tonic {

constexpr int kTreeMaxLevels = 8;              // 64^8 leaves: more than any capacity the entries admit
constexpr int64_t kTreeMaxCapacity = (int64_t)1 << 40;
constexpr int kTreeHeaderBytes = 64;
constexpr int kPriorityThreads = 1024;
constexpr int kPriorityMaxBatch = 1024;        // tonic_priority_update: the batch's indices sit in LDS

struct TreeLayout {
  int levels;                                  // level 0 (the leaves) .. levels - 1 (the top, <= 64 nodes)
  int64_t n[kTreeMaxLevels];                   // nodes per level
  int64_t off[kTreeMaxLevels];                 // byte offset of each level in the block
  int64_t bytes;
};

inline int64_t pad64(int64_t v) { return (v + 63) / 64 * 64; }

inline TreeLayout tree_layout(int64_t capacity) {
  TreeLayout t{};
  t.n[0] = capacity;
  t.off[0] = kTreeHeaderBytes;
  int64_t end = t.off[0] + 4 * pad64(capacity);
  int l = 0;
  while (t.n[l] > 64 && l + 1 < kTreeMaxLevels) {
    t.n[l + 1] = (t.n[l] + 63) / 64;
    t.off[l + 1] = end;
    end += 8 * pad64(t.n[l + 1]);
    ++l;
  }
  t.levels = l + 1;
  t.bytes = end;
  return t;
}

__device__ __forceinline__ const float* tree_leaves(const char* tree, const TreeLayout& t) {
  return reinterpret_cast<const float*>(tree + t.off[0]);
}
__device__ __forceinline__ float* tree_leaves(char* tree, const TreeLayout& t) {
  return reinterpret_cast<float*>(tree + t.off[0]);
}
__device__ __forceinline__ const double* tree_level(const char* tree, const TreeLayout& t, int l) {
  return reinterpret_cast<const double*>(tree + t.off[l]);
}
__device__ __forceinline__ double* tree_level(char* tree, const TreeLayout& t, int l) {
  return reinterpret_cast<double*>(tree + t.off[l]);
}

// node `node` of level l >= 1 from its 64 children, ascending: ONE thread walks them (the loads are independent,
// the 64 additions a chain), so that a workgroup recomputes 1024 nodes at a time.  16-byte loads: the threads of a
// wave read 64 different cache lines per load instruction and one workgroup has one CU's load rate, so a quarter
// (float32 leaves) or half (float64 sums) of the scalar loads' instructions.  The block is 16-byte aligned (checked
// by the entries) and every level starts on a 64-byte boundary of it.
__device__ __forceinline__ void tree_recompute(char* tree, const TreeLayout& t, int l, int64_t node) {
  double sum = 0.0;
  if (l == 1) {
    const float4* children = reinterpret_cast<const float4*>(tree_leaves(tree, t) + node * 64);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const float4 v = children[c];
      sum += (double)v.x; sum += (double)v.y; sum += (double)v.z; sum += (double)v.w;
    }
  } else {
    const double2* children = reinterpret_cast<const double2*>(tree_level(tree, t, l - 1) + node * 64);
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      const double2 v = children[c];
      sum += v.x; sum += v.y;
    }
  }
  tree_level(tree, t, l)[node] = sum;
}

// The inclusive prefix sums of the wave's 64 values in ascending lane order, each the same chain of additions a
// sequential loop over the children makes (a shuffle scan would associate them differently); *total: lane 63's.
__device__ __forceinline__ double wave_prefix_ascending(double v, int lane, double* total) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  double run = 0.0, mine = 0.0;
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    run += __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
    if (lane == j) mine = run;
  }
  *total = run;
  return mine;
}

__global__ __launch_bounds__(256) void priority_init_kernel(char* tree, int64_t bytes) {
  // (the block is 8-byte aligned and its size a multiple of 8: 64 + 4 * 64 a + 8 * 64 b)
  uint64_t* words = reinterpret_cast<uint64_t*>(tree);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < bytes / 8; i += stride)
    words[i] = i == 0 ? (uint64_t)__float_as_uint(1.f) : 0;
}

// leaves [first, first + count) = max_leaf, then their ancestors level by level; one workgroup
__global__ __launch_bounds__(kPriorityThreads) void priority_store_kernel(char* tree, TreeLayout t, int64_t first,
                                                                          int64_t count) {
  const float fresh = *reinterpret_cast<const float*>(tree);
  float* leaves = tree_leaves(tree, t);
  for (int64_t i = threadIdx.x; i < count; i += blockDim.x) leaves[first + i] = fresh;
  int64_t lo = first, hi = first + count - 1;
  for (int l = 1; l < t.levels; ++l) {
    __syncthreads();                            // (level l - 1 is written)
    lo >>= 6; hi >>= 6;
    for (int64_t node = lo + threadIdx.x; node <= hi; node += blockDim.x) tree_recompute(tree, t, l, node);
  }
}

// One wave per draw: t = u * total, then from the top level down the smallest child whose inclusive prefix sum
// exceeds t (strictly), t less that child's exclusive prefix; where rounding leaves no such child, the last child
// with a non-zero value.  A zero leaf is never returned (a tree without any non-zero leaf answers index 0).
// leaf_out [B]: the drawn leaves, for the weights.
__global__ __launch_bounds__(256) void priority_sample_kernel(const char* tree, TreeLayout t, const double* uniforms,
                                                              int64_t* indices, float* leaf_out, int B) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (m >= B) return;
  int64_t node = 0;                             // the children scanned: 64 node .. 64 node + 63 of level l
  double target = 0.0, value = 0.0;
  for (int l = t.levels - 1; l >= 0; --l) {
    value = l == 0 ? (double)tree_leaves(tree, t)[node * 64 + lane] : tree_level(tree, t, l)[node * 64 + lane];
    double total;
    const double inclusive = wave_prefix_ascending(value, lane, &total);
    if (l == t.levels - 1) target = uniforms[m] * total;
    const unsigned long long above = __ballot(inclusive > target);
    const unsigned long long live = __ballot(value > 0.0);
    int child = 0;
    if (above != 0) child = __builtin_ctzll(above);
    else if (live != 0) child = 63 - __builtin_clzll(live);
    const double before = __shfl(inclusive, child > 0 ? child - 1 : 0, 64);
    if (child > 0) target -= before;
    value = __shfl(value, child, 64);
    node = node * 64 + child;
    if (node >= t.n[l]) node = t.n[l] - 1;      // (a zero child is never chosen, the padding is zero: never taken)
  }
  if (lane == 0) {
    indices[m] = node;
    if (leaf_out != nullptr) leaf_out[m] = (float)value;
  }
}

// w_i = (min_j leaf_j / leaf_i)^beta over the batch: (N P_i)^-beta over its maximum, in which N and the total cancel
__global__ __launch_bounds__(kPriorityThreads) void priority_weights_kernel(float* weights, int B, float beta) {
  __shared__ float part[kPriorityThreads / 64];
  float low = INFINITY;
  for (int m = threadIdx.x; m < B; m += blockDim.x) low = fminf(low, weights[m]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) low = fminf(low, __shfl_xor(low, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = low;
  __syncthreads();
  low = part[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) low = fminf(low, part[w]);
  for (int m = threadIdx.x; m < B; m += blockDim.x) weights[m] = powf(low / weights[m], beta);
}

// leaf[idx_m] = (loss_m + epsilon)^alpha, the highest batch position winning an index that occurs more than once;
// max_leaf = max(max_leaf, the leaves written); the touched leaves' ancestors recomputed level by level.  One
// workgroup: at most 1024 parents per level, a barrier between the levels.  An index outside the capacity is skipped.
__global__ __launch_bounds__(kPriorityThreads) void priority_update_kernel(
    char* tree, TreeLayout t, const int64_t* indices, const float* losses, int B, float alpha, float epsilon) {
  __shared__ int64_t drawn[kPriorityMaxBatch];
  __shared__ float part[kPriorityThreads / 64];
  const int m = threadIdx.x;
  int64_t idx = -1;
  if (m < B) {
    idx = indices[m];
    if (idx < 0 || idx >= t.n[0]) idx = -1;
    drawn[m] = idx;
  }
  __syncthreads();
  float written = 0.f;
  if (idx >= 0) {
    bool wins = true;
    for (int later = m + 1; later < B; ++later) wins = wins && drawn[later] != idx;
    if (wins) {
      written = powf(fmaxf(losses[m] + epsilon, 0.f), alpha);
      tree_leaves(tree, t)[idx] = written;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) written = fmaxf(written, __shfl_xor(written, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = written;
  __syncthreads();                              // (the leaves are written, the waves' maxima are in LDS)
  if (threadIdx.x == 0) {
    float high = *reinterpret_cast<float*>(tree);
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) high = fmaxf(high, part[w]);
    *reinterpret_cast<float*>(tree) = high;
  }
  for (int l = 1; l < t.levels; ++l) {
    if (l > 1) __syncthreads();                 // (level l - 1 is written)
    if (idx >= 0) {
      idx >>= 6;
      // (several positions under one parent write the same sum of the same children: the same bits)
      tree_recompute(tree, t, l, idx);
    }
  }
}

}  // namespace tonic

using namespace tonic;

namespace {

bool finite_non_negative(double v) { return std::isfinite(v) && v >= 0; }

}  // namespace

extern "C" int64_t tonic_priority_tree_bytes(int64_t capacity) {
  if (capacity <= 0 || capacity > kTreeMaxCapacity) return 0;
  return tree_layout(capacity).bytes;
}

#define PRIORITY_TREE_CHECK(what)                                                                                  \
  TONIC_REQUIRE(d_tree != nullptr, TONIC_ERR_INVALID_ARGUMENT, what ": d_tree is NULL");                           \
  TONIC_REQUIRE(reinterpret_cast<uintptr_t>(d_tree) % 16 == 0, TONIC_ERR_INVALID_ARGUMENT,                         \
                what ": d_tree is not 16-byte aligned");                                                           \
  TONIC_REQUIRE(capacity > 0 && capacity <= kTreeMaxCapacity, TONIC_ERR_INVALID_ARGUMENT,                          \
                what ": capacity %lld (1 .. 2^40)", (long long)capacity);                                          \
  TONIC_REQUIRE(tree_bytes >= tonic_priority_tree_bytes(capacity), TONIC_ERR_WORKSPACE,                            \
                what ": a tree block of %lld bytes, a capacity of %lld needs %lld", (long long)tree_bytes,         \
                (long long)capacity, (long long)tonic_priority_tree_bytes(capacity))

extern "C" int tonic_priority_tree_init(void* d_tree, int64_t tree_bytes, int64_t capacity, void* stream) {
  PRIORITY_TREE_CHECK("tonic_priority_tree_init");
  const TreeLayout t = tree_layout(capacity);
  int64_t blocks = (t.bytes / 8 + 256 * 8 - 1) / (256 * 8);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(priority_init_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     static_cast<char*>(d_tree), t.bytes);
  TONIC_CHECK_LAUNCH("tonic_priority_tree_init");
  return TONIC_OK;
}

extern "C" int tonic_priority_store(void* d_tree, int64_t tree_bytes, int64_t capacity, int64_t first, int64_t count,
                                    void* stream) {
  PRIORITY_TREE_CHECK("tonic_priority_store");
  TONIC_REQUIRE(first >= 0 && count > 0 && first < capacity && count <= capacity - first, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_priority_store: leaves [%lld, %lld + %lld) of a capacity of %lld", (long long)first,
                (long long)first, (long long)count, (long long)capacity);
  hipLaunchKernelGGL(priority_store_kernel, dim3(1), dim3(kPriorityThreads), 0, as_stream(stream),
                     static_cast<char*>(d_tree), tree_layout(capacity), first, count);
  TONIC_CHECK_LAUNCH("tonic_priority_store");
  return TONIC_OK;
}

extern "C" int tonic_priority_sample(const void* d_tree, int64_t tree_bytes, int64_t capacity,
                                     const double* d_uniforms, int64_t* d_indices, float* d_weights, int32_t B,
                                     double beta, void* stream) {
  PRIORITY_TREE_CHECK("tonic_priority_sample");
  TONIC_REQUIRE(d_uniforms != nullptr && d_indices != nullptr, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_priority_sample: %s is NULL", d_uniforms == nullptr ? "d_uniforms" : "d_indices");
  TONIC_REQUIRE(B > 0 && B <= (1 << 20), TONIC_ERR_INVALID_ARGUMENT, "tonic_priority_sample: B = %d (1 .. 2^20)", B);
  TONIC_REQUIRE(finite_non_negative(beta), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_priority_sample: beta %g (finite and >= 0)", beta);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(priority_sample_kernel, dim3((B + 3) / 4), dim3(256), 0, st, static_cast<const char*>(d_tree),
                     tree_layout(capacity), d_uniforms, d_indices, d_weights, B);
  if (d_weights != nullptr)
    hipLaunchKernelGGL(priority_weights_kernel, dim3(1), dim3(kPriorityThreads), 0, st, d_weights, B, (float)beta);
  TONIC_CHECK_LAUNCH("tonic_priority_sample");
  return TONIC_OK;
}

extern "C" int tonic_priority_update(void* d_tree, int64_t tree_bytes, int64_t capacity, const int64_t* d_indices,
                                     const float* d_sample_losses, int32_t B, double alpha, double epsilon,
                                     void* stream) {
  PRIORITY_TREE_CHECK("tonic_priority_update");
  TONIC_REQUIRE(d_indices != nullptr && d_sample_losses != nullptr, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_priority_update: %s is NULL", d_indices == nullptr ? "d_indices" : "d_sample_losses");
  TONIC_REQUIRE(B > 0 && B <= kPriorityMaxBatch, TONIC_ERR_INVALID_ARGUMENT,
                "tonic_priority_update: B = %d (1 .. %d: one workgroup recomputes the ancestors)", B,
                kPriorityMaxBatch);
  TONIC_REQUIRE(finite_non_negative(alpha) && finite_non_negative(epsilon), TONIC_ERR_INVALID_ARGUMENT,
                "tonic_priority_update: alpha %g, epsilon %g (finite and >= 0)", alpha, epsilon);
  hipLaunchKernelGGL(priority_update_kernel, dim3(1), dim3(kPriorityThreads), 0, as_stream(stream),
                     static_cast<char*>(d_tree), tree_layout(capacity), d_indices, d_sample_losses, B, (float)alpha,
                     (float)epsilon);
  TONIC_CHECK_LAUNCH("tonic_priority_update");
  return TONIC_OK;
}
