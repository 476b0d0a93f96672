// Trimmed class centroids on the GPU: the "trimmed-centroid support" that
// tools/outlier_cleaning.py:250-257 reserves compute_centroids(trim_frac=...) for.
// The definition (DESIGN "Trimmed class centroids") in short: from the plain
// centroid c_0, every round scores each row against its own class's centroid,
// ranks ALL rows of the class by (similarity ascending, sample index ascending),
// drops the drop[k] lowest-ranked ones and re-forms the centroid from the rest.
//
//   * own_sim_kernel         s_i = x_i . c[cls[i]]: one wave per row, N x D reads;
//     lane-strided fmaf, then the wave butterfly (row_norms_kernel's order);
//   * rank by counting       r_i = #{j in class : (s_j, j) < (s_i, i)}: exact and
//     order-independent, no sort, no scratch. A workgroup owns kRankBlock
//     consecutive CSR positions (they may straddle classes) and streams the
//     (s, index) pairs of every class it touches through LDS in tiles of
//     kTrimTile; a thread compares against its own class's part of each tile
//     (the same address for the whole class: an LDS broadcast). Cost sum n_k^2;
//     segment_rank_kernel stores the ranks, trim_keep_kernel turns them straight
//     into keep flags and counts the flags that flipped (an integer atomic);
//   * masked_class_sums_kernel   class_sums_kernel (scoring.hip) with the keep
//     flag: one thread per column, the kept rows in ascending sample order (the
//     order is the contract, so a class is walked serially; 32 rows in flight);
//   * trim_centroid_kernel       centroid_kernel dividing by n_k - drop[k].
// With drop == 0 everywhere the last two perform the operations of the plain
// pair in the same order, so the centroids are bit-identical to class_centroids.
// No float atomics: two runs are bit-identical. drop is clamped on the device to
// 0 .. n_k - 1, so every non-empty class keeps at least one row.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace miclip {
namespace {

constexpr int kRankBlock = 256;   // CSR positions (threads) per workgroup
constexpr int kSumBatch = 32;     // rows a column thread of the masked sum keeps in flight

struct __attribute__((aligned(8))) RankKey {
  float s;
  int32_t idx;
};

__device__ __forceinline__ int clamp_drop(int drop, int n) {
  return drop < 0 ? 0 : (drop > n - 1 ? (n > 0 ? n - 1 : 0) : drop);
}

__global__ __launch_bounds__(64) void own_sim_kernel(const float* __restrict__ x,
                                                     const float* __restrict__ cent,
                                                     const int32_t* __restrict__ cls, int K,
                                                     int D, float* __restrict__ sims) {
  const int i = blockIdx.x;
  const int k = cls[i];
  if ((unsigned)k >= (unsigned)K) {   // a label outside the layout: no centroid to score against
    if (threadIdx.x == 0) sims[i] = 0.f;
    return;
  }
  const float* row = x + (size_t)i * D;
  const float* c = cent + (size_t)k * D;
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += 64) s = fmaf(row[d], c[d], s);
  s = wave_sum(s);
  if (threadIdx.x == 0) sims[i] = s;
}

// 1 when (e.s, e.idx) < (s, idx), else 0: IEEE '<' / '==' on the values (-0 == +0), then the
// sample index. Bitwise, not short-circuit: no divergent branch per element.
__device__ __forceinline__ int key_less(const RankKey& e, float s, int idx) {
  return (int)(e.s < s) | ((int)(e.s == s) & (int)(e.idx < idx));
}

// the class of CSR position p: the largest k with offsets[k] <= p (empty classes repeat
// an offset and are stepped over), so offsets[k] <= p < offsets[k + 1]
__device__ __forceinline__ int class_of(const int32_t* __restrict__ offsets, int K, int p) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Rank of the key (my_s, my_i) among the rows of the class at CSR positions [c0, c1); a
// thread past the last row passes c0 == c1 and only helps staging. All threads of the
// workgroup call this together.
__device__ __forceinline__ int rank_in_class(const float* __restrict__ values,
                                             const int32_t* __restrict__ order,
                                             const int32_t* __restrict__ offsets, int K, int N,
                                             int c0, int c1, float my_s, int my_i,
                                             RankKey* tile) {
  // the span of positions this workgroup's classes cover (block-uniform)
  const int p_first = blockIdx.x * kRankBlock;
  const int p_last = min(p_first + kRankBlock, N) - 1;
  const int span0 = max(offsets[class_of(offsets, K, p_first)], 0);
  const int span1 = min(offsets[class_of(offsets, K, p_last) + 1], N);   // never read past order[N)
  int rank = 0;
  for (int t0 = span0; t0 < span1; t0 += kTrimTile) {
    const int t1 = min(t0 + kTrimTile, span1);
    for (int q = t0 + (int)threadIdx.x; q < t1; q += kRankBlock) {
      const int j = order[q];
      RankKey e;
      e.s = (unsigned)j < (unsigned)N ? values[j] : 0.f;
      e.idx = j;
      tile[q - t0] = e;
    }
    __syncthreads();
    // 8 independent LDS reads in flight per step: one wave per SIMD has nothing else to
    // hide the read latency behind
    const int a = max(t0, c0), b = min(t1, c1);
    int q = a;
    for (; q + 8 <= b; q += 8) {
      RankKey e[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) e[u] = tile[q - t0 + u];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        rank += key_less(e[u], my_s, my_i);
    }
    for (; q < b; ++q) {
      const RankKey e = tile[q - t0];
      rank += key_less(e, my_s, my_i);
    }
    __syncthreads();
  }
  return rank;
}

__global__ __launch_bounds__(kRankBlock) void segment_rank_kernel(
    const float* __restrict__ values, const int32_t* __restrict__ order,
    const int32_t* __restrict__ offsets, int K, int N, int32_t* __restrict__ rank_out) {
  __shared__ RankKey tile[kTrimTile];
  const int p = blockIdx.x * kRankBlock + threadIdx.x;
  int c0 = 0, c1 = 0, my_i = -1;
  float my_s = 0.f;
  if (p < N) {
    const int k = class_of(offsets, K, p);
    c0 = offsets[k];
    c1 = offsets[k + 1];
    my_i = order[p];
    if ((unsigned)my_i < (unsigned)N) my_s = values[my_i];
  }
  const int r = rank_in_class(values, order, offsets, K, N, c0, c1, my_s, my_i, tile);
  if (p < N && (unsigned)my_i < (unsigned)N) rank_out[my_i] = r;
}

// keep[i] = rank_i >= drop[class]; *changed += #{keep[i] != previous keep[i]} (first: the
// previous flags are all ones and keep is only written)
__global__ __launch_bounds__(kRankBlock) void trim_keep_kernel(
    const float* __restrict__ values, const int32_t* __restrict__ order,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ drop, int K, int N,
    int first, uint8_t* __restrict__ keep, int32_t* __restrict__ changed) {
  __shared__ RankKey tile[kTrimTile];
  const int p = blockIdx.x * kRankBlock + threadIdx.x;
  int c0 = 0, c1 = 0, my_i = -1, my_drop = 0;
  float my_s = 0.f;
  if (p < N) {
    const int k = class_of(offsets, K, p);
    c0 = offsets[k];
    c1 = offsets[k + 1];
    my_drop = clamp_drop(drop[k], c1 - c0);
    my_i = order[p];
    if ((unsigned)my_i < (unsigned)N) my_s = values[my_i];
  }
  const int r = rank_in_class(values, order, offsets, K, N, c0, c1, my_s, my_i, tile);
  bool flip = false;
  if (p < N && (unsigned)my_i < (unsigned)N) {
    const uint8_t now = r >= my_drop ? 1 : 0;
    const uint8_t before = first ? 1 : keep[my_i];
    keep[my_i] = now;
    flip = now != before;
  }
  const int n = __popcll(__ballot(flip));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(changed, n);
}

__global__ __launch_bounds__(64) void masked_class_sums_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ order,
    const int32_t* __restrict__ offsets, const uint8_t* __restrict__ keep, int D,
    float* __restrict__ sums) {
  const int k = blockIdx.y, col = blockIdx.x * 64 + threadIdx.x;
  if (col >= D) return;
  const int i0 = offsets[k], i1 = offsets[k + 1];
  float acc = 0.f;
  int i = i0;
  // the row is loaded whether it is kept or not, so the flag and the row travel together
  // (one dependent load behind order[], not two); kSumBatch rows in flight, added in order
  for (; i + kSumBatch <= i1; i += kSumBatch) {
    float v[kSumBatch];
    uint8_t kp[kSumBatch];
#pragma unroll
    for (int u = 0; u < kSumBatch; ++u) {
      const int r = order[i + u];
      kp[u] = keep[r];
      v[u] = x[(size_t)r * D + col];
    }
#pragma unroll
    for (int u = 0; u < kSumBatch; ++u) acc = kp[u] ? acc + v[u] : acc;
  }
  for (; i < i1; ++i) {
    const int r = order[i];
    const float v = x[(size_t)r * D + col];
    acc = keep[r] ? acc + v : acc;
  }
  sums[(size_t)k * D + col] = acc;
}

// centroid_kernel (scoring.hip) over the kept rows: means = sums / (n_k - drop[k]);
// out = means / max(||means||, eps). An empty class stays a row of zeros.
__global__ __launch_bounds__(64) void trim_centroid_kernel(const float* __restrict__ sums,
                                                           const int32_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ drop,
                                                           int D, float eps,
                                                           float* __restrict__ out) {
  const int k = blockIdx.x;
  const int n = offsets[k + 1] - offsets[k];
  const int kept = n - clamp_drop(drop[k], n);
  const float cnt = (float)(kept > 0 ? kept : 1);
  const float* s = sums + (size_t)k * D;
  float* o = out + (size_t)k * D;
  float n2 = 0.f;
  for (int d = threadIdx.x; d < D; d += 64) {
    const float m = s[d] / cnt;
    o[d] = m;
    n2 = fmaf(m, m, n2);
  }
  const float nrm = fmaxf(sqrtf(wave_sum(n2)), eps);
  for (int d = threadIdx.x; d < D; d += 64) o[d] = o[d] / nrm;
}

}  // namespace

hipError_t segment_rank(const float* values, const int32_t* order, const int32_t* offsets, int K,
                        int N, int32_t* rank_out, hipStream_t s) {
  if (K < 1 || N < 1 || N > kTrimMaxClassRows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(segment_rank_kernel, dim3((N + kRankBlock - 1) / kRankBlock),
                     dim3(kRankBlock), 0, s, values, order, offsets, K, N, rank_out);
  return hipGetLastError();
}

hipError_t trimmed_centroids(const float* x, const int32_t* order, const int32_t* offsets,
                             const int32_t* cls, const int32_t* drop, int K, int N, int D,
                             int rounds, float eps, float* sums, float* centroids,
                             uint8_t* keep, float* sims, int32_t* changed, hipStream_t s) {
  if (K < 1 || K > 65535 || N < 1 || N > kTrimMaxClassRows || D < 1 || rounds < 1 ||
      rounds > kTrimMaxRounds)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t) * rounds, s);
  if (e != hipSuccess) return e;
  e = class_centroids(x, order, offsets, K, D, eps, sums, centroids, s);   // c_0
  if (e != hipSuccess) return e;
  const dim3 rank_grid((N + kRankBlock - 1) / kRankBlock), sum_grid((D + 63) / 64, K);
  for (int t = 0; t < rounds; ++t) {
    hipLaunchKernelGGL(own_sim_kernel, dim3(N), dim3(64), 0, s, x, centroids, cls, K, D, sims);
    hipLaunchKernelGGL(trim_keep_kernel, rank_grid, dim3(kRankBlock), 0, s, sims, order, offsets,
                       drop, K, N, t == 0 ? 1 : 0, keep, changed + t);
    hipLaunchKernelGGL(masked_class_sums_kernel, sum_grid, dim3(64), 0, s, x, order, offsets,
                       keep, D, sums);
    hipLaunchKernelGGL(trim_centroid_kernel, dim3(K), dim3(64), 0, s, sums, offsets, drop, D,
                       eps, centroids);
  }
  return hipGetLastError();
}

}  // namespace miclip
