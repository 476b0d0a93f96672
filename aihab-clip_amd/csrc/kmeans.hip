// Device k-means for the multi-prototype outlier scorer (the per-class KMeans fit
// of tools/outlier_cleaning.py:511-541), all fp32. A launch runs Pn independent
// problems, one 256-thread workgroup each: problem p clusters the rows
// order[offsets[c] .. offsets[c+1]) of class c = prob_class[p] (the class layout
// of class_centroids) into k = prob_k[p] clusters (2 <= k <= 16). The restarts of
// a class are separate problems that name the same class; they share x and differ
// only in their state, so "the restart is a grid dimension".
//
//   * kmeans_seed_kernel: plain k-means++ (D^2 sampling, one candidate per step)
//     from host-supplied uniforms. mind[j] = min over the chosen centres of
//     |x_j - c|^2 (direct differences) lives in the scratch. Its sum runs in a
//     fixed order: thread t owns rows [t L, (t+1) L), L = ceil(n / 256), and sums
//     them left to right from 0; the 256 chunk sums are added left to right. The
//     inclusive prefix of row j is (sum of the chunks before) + (its chunk's running
//     sum), which is non-decreasing, and pick t is the first j whose prefix exceeds
//     u_t * total. A chosen row has mind == 0 exactly and can not be drawn again.
//   * kmeans_lloyd_kernel: the whole fit, scikit-learn's loop (_kmeans_single_lloyd)
//     rule for rule. Centres and cluster sums stay in LDS (2 x 16 x (D + 4) floats,
//     131,584 B at D = 1024 of the 160 KiB).
//       E-step  x . c_j on v_mfma_f32_16x16x4_f32, 16 rows x 16 centre slots per
//               tile (two row tiles per wave share the centre fragment), then
//               argmin_j |c_j|^2 - 2 x . c_j over the 16 lanes of a row; slots >= k
//               hold +inf, ties go to the lower index.
//       M-step  sums = onehot(labels)^T X on the same MFMA: a wave owns 64 columns
//               and walks the rows in ascending order, so a cluster's sum is the
//               strict left-to-right fp32 sum of its rows (0 * x adds nothing), as
//               in class_sums_kernel. Counts are integer LDS atomics.
//       empty   in ascending cluster order an empty cluster takes the row farthest
//               from its own (old) centre, the next one the next farthest (direct
//               distances into the scratch; lowest row among equals).
//       stop    labels unchanged ("strict"), else sum |c_new - c_old|^2 <= tol[p];
//               after a non-strict exit one more E-step; inertia from direct
//               differences on the returned labels and centres.
//
// Determinism: every reduction is a fixed butterfly or an index-ordered sum, the
// only atomics are on integers, and a problem reads x and its own slices only: its
// results are bit-identical run to run and wherever it stands in a launch.
// Non-finite input: every loop is bounded (max_iter, n, k) and every label / pick
// is clamped into range before it indexes anything.
// A problem whose table entry breaks the contract (k outside 2..16, n_c < k) is
// skipped: n_iter = -1 (lloyd), picks = -1 (seed), nothing else written.
#include <math.h>

#include "kernels.h"
#include "launch.h"
#include "mfma_f32.h"

namespace miclip {

namespace {

constexpr int kSlots = 16;   // centre slots per problem (k <= 16)

struct KmProblem {
  const int32_t* ord;   // the class's rows
  int n, k;
  size_t out0;          // offset into the per-row outputs / scratch
  bool ok;
};

MICLIP_DEV KmProblem km_problem(const int32_t* order, const int32_t* offsets,
                                const int32_t* prob_class, const int32_t* prob_k,
                                const int32_t* prob_off, int p) {
  KmProblem q;
  const int c = prob_class[p];
  const int r0 = offsets[c];
  q.ord = order + r0;
  q.n = offsets[c + 1] - r0;
  q.k = prob_k[p];
  q.out0 = (size_t)prob_off[p];
  q.ok = q.k >= 2 && q.k <= kSlots && q.n >= q.k && prob_off[p] >= 0;
  return q;
}

__global__ __launch_bounds__(256) void kmeans_seed_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ order,
    const int32_t* __restrict__ offsets, int D, const int32_t* __restrict__ prob_class,
    const int32_t* __restrict__ prob_k, const int32_t* __restrict__ prob_off,
    const float* __restrict__ u, float* mind_all, int32_t* __restrict__ picks,
    float* __restrict__ centres) {
  __shared__ float cs[256];
  __shared__ float base[257];
  __shared__ int s_picks[kSlots];
  __shared__ int s_pick, s_last;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const KmProblem q = km_problem(order, offsets, prob_class, prob_k, prob_off, p);
  if (!q.ok) {
    if (tid < kSlots) picks[p * kSlots + tid] = -1;
    return;
  }
  const int n = q.n, k = q.k;
  float* mind = mind_all + q.out0;
  float* cen = centres + (size_t)p * kSlots * D;
  const int L = (n + 255) / 256;
  const int b = min(tid * L, n), e = min(b + L, n);
  if (tid == 0) {
    const float f = fminf(fmaxf(floorf(u[p * kSlots] * (float)n), 0.f), (float)(n - 1));
    s_picks[0] = (int)f;
    picks[p * kSlots] = (int)f;
  }
  __syncthreads();
  for (int t = 1; t <= k; ++t) {
    const float* c = x + (size_t)q.ord[s_picks[t - 1]] * D;
    for (int d = tid; d < D; d += 256) cen[(size_t)(t - 1) * D + d] = c[d];
    if (t == k) break;
    for (int r = wave; r < n; r += 4) {
      const float* row = x + (size_t)q.ord[r] * D;
      float s = 0.f;
      for (int d = lane; d < D; d += 64) {
        const float df = row[d] - c[d];
        s = fmaf(df, df, s);
      }
      s = wave_sum(s);
      if (lane == 0) mind[r] = t == 1 ? s : fminf(mind[r], s);
    }
    if (tid == 0) {
      s_pick = -1;
      s_last = -1;
    }
    __syncthreads();
    {
      float s = 0.f;
      int last = -1;
      for (int j = b; j < e; ++j) {
        const float v = mind[j];
        s += v;
        if (v > 0.f) last = j;
      }
      cs[tid] = s;
      if (last >= 0) atomicMax(&s_last, last);
    }
    __syncthreads();
    if (tid == 0) {
      float run = 0.f;
      for (int i = 0; i < 256; ++i) {
        base[i] = run;
        run += cs[i];
      }
      base[256] = run;
    }
    __syncthreads();
    const float total = base[256];
    const float target = u[p * kSlots + t] * total;
    if (b < e && !(base[tid] > target) && base[tid + 1] > target) {
      float part = 0.f;
      for (int j = b; j < e; ++j) {
        part += mind[j];
        if (base[tid] + part > target) {
          s_pick = j;
          break;
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      int j = s_pick;
      if (j < 0 && total > 0.f) j = s_last;   // u_t * total rounded up to the total
      if (j < 0 || j >= n) {                  // total == 0 (or NaN): lowest row not yet chosen
        for (j = 0; j < n - 1; ++j) {
          bool taken = false;
          for (int a = 0; a < t; ++a) taken |= s_picks[a] == j;
          if (!taken) break;
        }
      }
      s_picks[t] = j;
      picks[p * kSlots + t] = j;
    }
    __syncthreads();
  }
}

// E-step of one workgroup: labels[r] = argmin_j cn[j] - 2 x_r . C_j. With TRACK the
// cluster counts and the "some label changed" flag are updated too.
template <bool VEC, bool TRACK>
MICLIP_DEV void km_estep(const float* __restrict__ x, const KmProblem& q, int D, int Dp, int ld,
                         const float* C, const float* cn, int* cnt, int* changed,
                         int32_t* labels) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int n = q.n, k = q.k;
  const int ntile = (n + 15) / 16;
  const float cni = i < k ? cn[i] : 0.f;
  bool diff = false;
  for (int t0 = wave * 2; t0 < ntile; t0 += 8) {
    const float* row0 = x + (size_t)q.ord[min(t0 * 16 + i, n - 1)] * D;
    const float* row1 = x + (size_t)q.ord[min(t0 * 16 + 16 + i, n - 1)] * D;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const float* crow = C + i * ld + 4 * g;
    for (int c0 = 0; c0 < Dp; c0 += 16) {
      const f32x4 bv = *(const f32x4*)(crow + c0);
      const f32x4 a0 = load4_clip<VEC>(row0, c0 + 4 * g, D);
      const f32x4 a1 = load4_clip<VEC>(row1, c0 + 4 * g, D);
      acc[0] = mfma4(a0, bv, acc[0]);
      acc[1] = mfma4(a1, bv, acc[1]);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = i < k ? fmaf(-2.f, acc[h][r], cni) : INFINITY;
        int idx = i;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float ov = __shfl_xor(v, o, 64);
          const int oi = __shfl_xor(idx, o, 64);
          if (ov < v || (ov == v && oi < idx)) {
            v = ov;
            idx = oi;
          }
        }
        const int row = (t0 + h) * 16 + 4 * g + r;
        if (i == 0 && row < n) {
          const int lab = min(max(idx, 0), k - 1);
          if constexpr (TRACK) {
            diff |= labels[row] != lab;
            atomicAdd(&cnt[lab], 1);
          }
          labels[row] = lab;
        }
      }
    }
  }
  if constexpr (TRACK) {
    if (diff) *changed = 1;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void kmeans_lloyd_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ order,
    const int32_t* __restrict__ offsets, int D, const int32_t* __restrict__ prob_class,
    const int32_t* __restrict__ prob_k, const int32_t* __restrict__ prob_off,
    const float* __restrict__ tol, int max_iter, float* dist_all, float* __restrict__ centres,
    int32_t* labels_all, float* __restrict__ inertia, int32_t* __restrict__ n_iter,
    int32_t* __restrict__ strict_out, int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const KmProblem q = km_problem(order, offsets, prob_class, prob_k, prob_off, p);
  if (!q.ok) {
    if (tid == 0) n_iter[p] = -1;
    return;
  }
  const int n = q.n, k = q.k;
  const int Dp = (D + 15) & ~15, ld = Dp + kLdsPad;
  float* C = (float*)smem;            // [16][ld] centres, columns >= D and slots >= k zero
  float* S = C + kSlots * ld;         // [16][ld] cluster sums, then the new means
  float* cn = S + kSlots * ld;        // [16] |c_j|^2
  int* cnt = (int*)(cn + kSlots);     // [16]
  float* red = (float*)(cnt + kSlots);   // [4] per-wave partials
  int* redi = (int*)(red + 4);           // [4]
  int* flag = redi + 4;                  // [0] label changed, [1] relocated row
  float* cen = centres + (size_t)p * kSlots * D;
  int32_t* labels = labels_all + q.out0;
  float* dist = dist_all + q.out0;
  const float tol_p = tol[p];

  for (int e = tid; e < kSlots * ld; e += 256) {
    const int j = e / ld, d = e - j * ld;
    C[e] = (j < k && d < D) ? cen[(size_t)j * D + d] : 0.f;
  }
  __syncthreads();
  const auto centre_norms = [&]() {
    for (int j = wave; j < k; j += 4) {
      float s = 0.f;
      for (int d = lane; d < D; d += 64) s = fmaf(C[j * ld + d], C[j * ld + d], s);
      s = wave_sum(s);
      if (lane == 0) cn[j] = s;
    }
  };
  centre_norms();

  int iters = 0;
  bool strict = false;
  for (int it = 0; it < max_iter; ++it) {
    if (tid < kSlots) cnt[tid] = 0;
    if (tid == 0) flag[0] = it == 0;   // no previous labels: never strict at the first pass
    __syncthreads();
    km_estep<VEC, true>(x, q, D, Dp, ld, C, cn, cnt, flag, labels);
    __syncthreads();
    const bool changed = flag[0] != 0;
    // M-step: S = onehot(labels)^T X, rows ascending, 64 columns per wave pass
    for (int c0 = wave * 64; c0 < Dp; c0 += 256) {
      f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                      {0.f, 0.f, 0.f, 0.f}};
      for (int m = 0; m < n; m += 16) {   // 4 MFMA k-steps of 4 rows, loads issued together
        float a[4], bv[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int row = m + 4 * s + g;
          const int rr = min(row, n - 1);
          const int lab = row < n ? labels[rr] : -1;
          a[s] = lab == i ? 1.f : 0.f;
          const float* rp = x + (size_t)q.ord[rr] * D;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int col = c0 + 16 * t + i;
            bv[s][t] = col < D ? rp[col] : 0.f;
          }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], bv[s][t], acc[t], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int col = c0 + 16 * t + i;
        if (col < Dp) {
#pragma unroll
          for (int r = 0; r < 4; ++r) S[(4 * g + r) * ld + col] = acc[t][r];
        }
      }
    }
    __syncthreads();
    // empty clusters (the list is taken once, before any row moves)
    unsigned empty = 0;
    for (int j = 0; j < k; ++j) empty |= (cnt[j] == 0 ? 1u : 0u) << j;
    if (empty) {
      for (int r = wave; r < n; r += 4) {
        const float* row = x + (size_t)q.ord[r] * D;
        const float* c = C + min(max(labels[r], 0), k - 1) * ld;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) {
          const float df = row[d] - c[d];
          s = fmaf(df, df, s);
        }
        s = wave_sum(s);
        if (lane == 0) dist[r] = s;
      }
      __syncthreads();
      for (int j = 0; j < k; ++j) {
        if (!((empty >> j) & 1u)) continue;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int r = tid; r < n; r += 256) {
          const float v = dist[r];
          if (v > bv || (v == bv && r < bi)) {
            bv = v;
            bi = r;
          }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
          }
        }
        if (lane == 0) {
          red[wave] = bv;
          redi[wave] = bi;
        }
        __syncthreads();
        if (tid == 0) {
          for (int w = 1; w < 4; ++w) {
            if (red[w] > bv || (red[w] == bv && redi[w] < bi)) {
              bv = red[w];
              bi = redi[w];
            }
          }
          if (bi < 0 || bi >= n) bi = 0;
          flag[1] = bi;
          dist[bi] = -1.f;   // taken: below every distance
        }
        __syncthreads();
        const int far = flag[1];
        const int old = min(max(labels[far], 0), k - 1);
        const float* row = x + (size_t)q.ord[far] * D;
        if (old != j) {
          for (int d = tid; d < D; d += 256) {
            const float v = row[d];
            S[old * ld + d] -= v;
            S[j * ld + d] = v;
          }
        }
        __syncthreads();
        if (tid == 0 && old != j) {
          cnt[j] = 1;
          cnt[old] -= 1;
        }
        __syncthreads();
      }
    }
    // means, centre shift, new centres
    float sh = 0.f;
    for (int e = tid; e < k * Dp; e += 256) {
      const int j = e / Dp, d = e - j * Dp;
      if (d < D) {
        const int cj = cnt[j];
        const float s = S[j * ld + d];
        const float c = cj > 0 ? s / (float)cj : s;
        const float df = c - C[j * ld + d];
        sh = fmaf(df, df, sh);
        C[j * ld + d] = c;
      }
    }
    sh = wave_sum(sh);
    if (lane == 0) red[wave] = sh;
    __syncthreads();
    const float shift = ((red[0] + red[1]) + red[2]) + red[3];
    centre_norms();
    __syncthreads();
    iters = it + 1;
    if (!changed) {
      strict = true;
      break;
    }
    if (shift <= tol_p) break;
  }
  if (!strict) {
    km_estep<VEC, false>(x, q, D, Dp, ld, C, cn, cnt, flag, labels);
  }
  if (tid < kSlots) cnt[tid] = 0;
  __syncthreads();
  for (int r = tid; r < n; r += 256) atomicAdd(&cnt[min(max(labels[r], 0), k - 1)], 1);
  float acc = 0.f;
  for (int r = wave; r < n; r += 4) {
    const float* row = x + (size_t)q.ord[r] * D;
    const float* c = C + min(max(labels[r], 0), k - 1) * ld;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float df = row[d] - c[d];
      s = fmaf(df, df, s);
    }
    acc += wave_sum(s);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    inertia[p] = ((red[0] + red[1]) + red[2]) + red[3];
    n_iter[p] = iters;
    if (strict_out) strict_out[p] = strict ? 1 : 0;
  }
  if (tid < kSlots) counts[p * kSlots + tid] = tid < k ? cnt[tid] : 0;
  for (int e = tid; e < k * D; e += 256) {
    const int j = e / D, d = e - j * D;
    cen[e] = C[j * ld + d];
  }
}

bool kmeans_shape_ok(int D, int Pn, int k_max) {
  return D >= 1 && D <= 1024 && Pn >= 1 && Pn <= 65535 && k_max >= 2 && k_max <= kSlots;
}

template <bool VEC>
hipError_t launch_lloyd(const float* x, const int32_t* order, const int32_t* offsets, int D,
                        const int32_t* prob_class, const int32_t* prob_k,
                        const int32_t* prob_off, int Pn, const float* tol, int max_iter,
                        float* scratch, float* centres, int32_t* labels, float* inertia,
                        int32_t* n_iter, int32_t* strict, int32_t* counts, hipStream_t s) {
  const int Dp = (D + 15) & ~15;
  const size_t lds = (size_t)(2 * kSlots * (Dp + kLdsPad) + 2 * kSlots + 16) * sizeof(float);
  // at most 131,776 B (D = 1024) of the 160 KiB
  const hipError_t attr = lds_opt_in((const void*)kmeans_lloyd_kernel<VEC>, lds);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(kmeans_lloyd_kernel<VEC>, dim3(Pn), dim3(256), lds, s, x, order, offsets, D,
                     prob_class, prob_k, prob_off, tol, max_iter, scratch, centres, labels,
                     inertia, n_iter, strict, counts);
  return hipGetLastError();
}

}  // namespace

hipError_t kmeans_seed(const float* x, const int32_t* order, const int32_t* offsets, int D,
                       const int32_t* prob_class, const int32_t* prob_k, const int32_t* prob_off,
                       int Pn, int k_max, const float* u, float* scratch, int32_t* picks,
                       float* centres, hipStream_t s) {
  if (!kmeans_shape_ok(D, Pn, k_max)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kmeans_seed_kernel, dim3(Pn), dim3(256), 0, s, x, order, offsets, D,
                     prob_class, prob_k, prob_off, u, scratch, picks, centres);
  return hipGetLastError();
}

hipError_t kmeans_lloyd(const float* x, const int32_t* order, const int32_t* offsets, int D,
                        const int32_t* prob_class, const int32_t* prob_k,
                        const int32_t* prob_off, int Pn, int k_max, const float* tol,
                        int max_iter, float* scratch, float* centres, int32_t* labels,
                        float* inertia, int32_t* n_iter, int32_t* strict, int32_t* counts,
                        hipStream_t s) {
  if (!kmeans_shape_ok(D, Pn, k_max) || max_iter < 1) return hipErrorInvalidValue;
  if (D % 4 == 0 && ((uintptr_t)x & 15) == 0)
    return launch_lloyd<true>(x, order, offsets, D, prob_class, prob_k, prob_off, Pn, tol,
                              max_iter, scratch, centres, labels, inertia, n_iter, strict, counts,
                              s);
  return launch_lloyd<false>(x, order, offsets, D, prob_class, prob_k, prob_off, Pn, tol, max_iter,
                             scratch, centres, labels, inertia, n_iter, strict, counts, s);
}

}  // namespace miclip
