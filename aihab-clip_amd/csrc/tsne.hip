// Exact t-SNE for the embedding-cache visualiser (the TSNE(n_components=2, ...) fit of
// feat_cache_vis/feat_vis.py:150-157): dense P, all-pairs repulsion, no tree and no
// neighbour truncation. Two embedding dimensions, so the Student-t
// has one degree of freedom. The rules are scikit-learn 1.7's (_t_sne.py,
// _utils._binary_search_perplexity), rule for rule; fp32 storage everywhere.
//
//   * row_norms (scoring.hip) + tsne_dist_kernel: dist [N, N], the quantity the perplexity
//     search is fed. x . x^T on v_mfma_f32_16x16x4_f32 (a wave owns a 32 x 32 block of
//     the Gram matrix, fragments straight from global memory, fp32 accumulation).
//     Cosine: clip(1 - x_i . x_j / (|x_i| |x_j|), 0, 2), diagonal 0, then squared
//     (_t_sne.py squares every non-euclidean metric). Euclidean: max(|x_i|^2 + |x_j|^2
//     - 2 x_i . x_j, 0), diagonal 0.
//   * tsne_perplexity_kernel: one 256-thread workgroup per row; the row of distances
//     is read once into LDS (4 N <= 64 KiB). _binary_search_perplexity as written:
//     beta = 1, at most 100 steps, stop at |H - log perplexity| <= 1e-5, double /
//     halve / bisect, sum 0 -> 1e-8, H = log sum + beta * sum(d p) / sum, diagonal
//     excluded. exp and the two sums run in fp64 (the kernel runs once per fit and this
//     keeps the search on scikit-learn's double path). Writes the conditional row
//     (fp32), beta, and the fp64 sum of the stored row.
//   * tsne_symmetrise_kernel: in place, P = max((C + C^T) / max(sum, eps), eps) off the
//     diagonal and 0 on it. A workgroup owns a 32 x 32 tile and its mirror image and
//     writes the same value to both, so P is bit-symmetric. The sum is the per-row sums
//     added in a fixed order (the same in every workgroup).
//   * tsne_forces_kernel: the per-iteration hot kernel. y [N, 2] staged in LDS, a wave
//     owns a row i, lanes stride over j (coalesced reads of P's row). With
//     w = 1 / (1 + |y_i - y_j|^2) (0 at j == i by a select): attr = sum p w (y_i - y_j),
//     rep = sum w^2 (y_i - y_j), z = sum w, and on error iterations sum pe log max(pe,
//     eps), sum pe log w, sum pe with pe = exaggeration * p. wave_sum, one row of 8
//     floats out.
//   * tsne_update_kernel: one 1024-thread workgroup. Z = sum z_i; g = 4 (exaggeration *
//     attr - rep / Z) (scikit-learn's 4 sum (P - Q) w (y_i - y_j) with Q unfloored);
//     _gradient_descent's gains / momentum rules in its order; on error iterations
//     stats = {KL, |g * gains|_2, Z, steps done}.
//
// Determinism: no float atomics (no atomics at all). Every reduction is a fixed
// butterfly or an index-ordered sum whose shape depends on N alone, so results are
// bit-identical run to run. Kernels never wait on another workgroup: forces -> update
// -> forces is ordered by the stream alone, two plain launches per iteration.
// Non-finite input: every loop is bounded by N or a constant; no index comes from data.
#include <math.h>

#include "kernels.h"
#include "mfma_f32.h"

namespace miclip {

namespace {

constexpr double kTsneEps = 2.220446049250313e-16;   // np.finfo(np.double).eps
constexpr int kRowOut = 8;                           // floats per row out of the forces kernel

MICLIP_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over a workgroup of NW waves, the same value in every thread: butterfly inside a
// wave, then the wave partials left to right. `red` holds NW doubles.
template <int NW>
MICLIP_DEV double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();   // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s += red[w];
  return s;
}

// A workgroup owns a 64 x 64 block of dist, each of its 4 waves a 32 x 32 quarter
// (2 x 2 MFMA tiles). Rows past N are clamped for the loads and masked at the store.
// nrm[i] = |x_i|.
template <bool VEC>
__global__ __launch_bounds__(256) void tsne_dist_kernel(const float* __restrict__ x, int N, int D,
                                                        int cosine, const float* __restrict__ nrm,
                                                        float* __restrict__ dist) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * 64 + (wave >> 1) * 32;
  const int n0 = blockIdx.x * 64 + (wave & 1) * 32;
  if (m0 >= N || n0 >= N) return;   // wave-uniform; no barrier below
  const float* ar[2] = {x + (size_t)min(m0 + i, N - 1) * D, x + (size_t)min(m0 + 16 + i, N - 1) * D};
  const float* br[2] = {x + (size_t)min(n0 + i, N - 1) * D, x + (size_t)min(n0 + 16 + i, N - 1) * D};
  f32x4 acc[2][2] = {{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}},
                     {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}};
  for (int c0 = 0; c0 < D; c0 += 16) {
    const int col = c0 + 4 * g;
    const f32x4 a0 = load4_clip<VEC>(ar[0], col, D), a1 = load4_clip<VEC>(ar[1], col, D);
    const f32x4 b0 = load4_clip<VEC>(br[0], col, D), b1 = load4_clip<VEC>(br[1], col, D);
    acc[0][0] = mfma4(a0, b0, acc[0][0]);
    acc[0][1] = mfma4(a0, b1, acc[0][1]);
    acc[1][0] = mfma4(a1, b0, acc[1][0]);
    acc[1][1] = mfma4(a1, b1, acc[1][1]);
  }
#pragma unroll
  for (int hm = 0; hm < 2; ++hm)
#pragma unroll
    for (int hn = 0; hn < 2; ++hn) {
      const int c = n0 + 16 * hn + i;
      if (c >= N) continue;
      const float nc = nrm[c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + 16 * hm + 4 * g + r;
        if (row >= N) continue;
        const float nr = nrm[row], dot = acc[hm][hn][r];
        float d;
        if (cosine) {   // a zero row has cosine 0 to everything, as sklearn's normalize leaves it
          const float den = nr * nc;
          d = fminf(fmaxf(1.f - (den > 0.f ? dot / den : 0.f), 0.f), 2.f);
          d *= d;
        } else {
          d = fmaxf(fmaf(-2.f, dot, fmaf(nr, nr, nc * nc)), 0.f);
        }
        dist[(size_t)row * N + c] = row == c ? 0.f : d;
      }
    }
}

// _binary_search_perplexity for row blockIdx.x. cond may be dist itself: a workgroup
// reads its row into LDS before it writes it, and touches no other row.
__global__ __launch_bounds__(256) void tsne_perplexity_kernel(const float* dist, int N,
                                                              float perplexity, float* cond,
                                                              float* __restrict__ beta_out,
                                                              double* __restrict__ row_sum) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double red[4];
  float* d = (float*)smem;   // [N]
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* src = dist + (size_t)row * N;
  for (int j = tid; j < N; j += 256) d[j] = src[j];
  __syncthreads();
  const double target = log((double)perplexity);
  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, sum_p = 1e-8;
  for (int step = 0; step < 100; ++step) {
    double sp = 0.0, sdp = 0.0;
    for (int j = tid; j < N; j += 256) {
      const double dj = (double)d[j];
      const double p = j == row ? 0.0 : exp(-dj * beta);
      sp += p;
      sdp = fma(dj, p, sdp);
    }
    sp = block_sum_f64<4>(sp, red);
    sdp = block_sum_f64<4>(sdp, red);
    if (sp == 0.0) sp = 1e-8;
    sum_p = sp;
    const double diff = log(sp) + beta * (sdp / sp) - target;
    if (fabs(diff) <= 1e-5) break;   // uniform: every thread holds the same sums
    if (step == 99) break;           // the row keeps the beta it was last evaluated at
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) * 0.5;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta * 0.5 : (beta + beta_min) * 0.5;
    }
  }
  double stored = 0.0;
  float* out = cond + (size_t)row * N;
  for (int j = tid; j < N; j += 256) {
    const float p = j == row ? 0.f : (float)(exp(-(double)d[j] * beta) / sum_p);
    out[j] = p;
    stored += (double)p;
  }
  stored = block_sum_f64<4>(stored, red);
  if (tid == 0) {
    beta_out[row] = (float)beta;
    row_sum[row] = stored;
  }
}

// In place: P[i][j] = P[j][i] = max((C[i][j] + C[j][i]) / max(sum, eps), eps), diagonal 0.
// grid (T, T) with T = ceil(N / 32); workgroups below the diagonal leave at once.
__global__ __launch_bounds__(256) void tsne_symmetrise_kernel(float* P, int N,
                                                              const double* __restrict__ row_sum) {
  __shared__ double red[4];
  __shared__ float A[32][33], B[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x, tid = threadIdx.x;
  if (bj < bi) return;
  double s = 0.0;
  for (int r = tid; r < N; r += 256) s += row_sum[r];
  // sum(C + C^T) = 2 sum C, as scikit-learn's np.sum(P) sees it
  const double total = fmax(2.0 * block_sum_f64<4>(s, red), kTsneEps);
  const int tx = tid & 31, ty = tid >> 5;   // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int ai = bi * 32 + r, aj = bj * 32 + tx;
    A[r][tx] = (ai < N && aj < N) ? P[(size_t)ai * N + aj] : 0.f;
    const int ci = bj * 32 + r, cj = bi * 32 + tx;
    B[r][tx] = (ci < N && cj < N) ? P[(size_t)ci * N + cj] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    {   // element (ai, aj) of the upper tile; its mirror is B[tx][r]
      const int ai = bi * 32 + r, aj = bj * 32 + tx;
      if (ai < N && aj < N) {
        const double v = fmax(((double)A[r][tx] + (double)B[tx][r]) / total, kTsneEps);
        P[(size_t)ai * N + aj] = ai == aj ? 0.f : (float)v;
      }
    }
    if (bj != bi) {   // element (ci, cj) of the mirror tile: the same sum, the same order
      const int ci = bj * 32 + r, cj = bi * 32 + tx;
      if (ci < N && cj < N) {
        const double v = fmax(((double)A[tx][r] + (double)B[r][tx]) / total, kTsneEps);
        P[(size_t)ci * N + cj] = (float)v;
      }
    }
  }
}

// rows [blockIdx.x * 4 * R, +4 R): wave w takes rows base + w, base + w + 4, ...
template <bool ERR>
__global__ __launch_bounds__(256) void tsne_forces_kernel(const float* __restrict__ P,
                                                          const float* __restrict__ y, int N, int R,
                                                          float exaggeration,
                                                          float* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f32x2* ys = (f32x2*)smem;   // [N]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < N; j += 256) ys[j] = ((const f32x2*)y)[j];
  __syncthreads();
  const int base = blockIdx.x * 4 * R;
  for (int q = 0; q < R; ++q) {
    const int i = base + 4 * q + wave;
    if (i >= N) break;   // wave-uniform, no barrier below
    const f32x2 yi = ys[i];
    const float* prow = P + (size_t)i * N;
    float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, z = 0.f, ea = 0.f, eb = 0.f, ep = 0.f;
#pragma unroll 4   // several loads of P in flight; a lane still adds its columns in order
    for (int j = lane; j < N; j += 64) {
      const float p = prow[j];
      const f32x2 yj = ys[j];
      const float dx = yi.x - yj.x, dy = yi.y - yj.y;
      const float w1 = 1.f / (1.f + fmaf(dx, dx, dy * dy));
      const float w = j == i ? 0.f : w1;
      const float pw = p * w, ww = w * w;
      ax = fmaf(pw, dx, ax);
      ay = fmaf(pw, dy, ay);
      rx = fmaf(ww, dx, rx);
      ry = fmaf(ww, dy, ry);
      z += w;
      if constexpr (ERR) {
        const float pe = p * exaggeration;   // 0 on the diagonal; log w1 = 0 there
        ea = fmaf(pe, logf(fmaxf(pe, (float)kTsneEps)), ea);
        eb = fmaf(pe, logf(w1), eb);
        ep += pe;
      }
    }
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    rx = wave_sum(rx);
    ry = wave_sum(ry);
    z = wave_sum(z);
    if constexpr (ERR) {
      ea = wave_sum(ea);
      eb = wave_sum(eb);
      ep = wave_sum(ep);
    }
    if (lane == 0) {
      float* o = rows + (size_t)i * kRowOut;
      o[0] = ax;
      o[1] = ay;
      o[2] = rx;
      o[3] = ry;
      o[4] = z;
      if constexpr (ERR) {
        o[5] = ea;
        o[6] = eb;
        o[7] = ep;
      }
    }
  }
}

// One workgroup of 1024 threads; thread t owns rows [t L, (t + 1) L), L = ceil(N / 1024).
template <bool ERR>
__global__ __launch_bounds__(1024) void tsne_update_kernel(const float* __restrict__ rows, int N,
                                                           float* __restrict__ y,
                                                           float* __restrict__ update,
                                                           float* __restrict__ gains,
                                                           float exaggeration, float momentum,
                                                           float lr, float min_gain, int steps_done,
                                                           float* __restrict__ stats) {
  __shared__ double red[16];
  const int tid = threadIdx.x;
  const int L = (N + 1023) / 1024;
  const int b = min(tid * L, N), e = min(b + L, N);
  double zs = 0.0;
  for (int i = b; i < e; ++i) zs += (double)rows[(size_t)i * kRowOut + 4];
  const double Zd = block_sum_f64<16>(zs, red);
  const float Z = (float)Zd;
  double g2 = 0.0, kl = 0.0, sp = 0.0;
  for (int i = b; i < e; ++i) {
    const float* o = rows + (size_t)i * kRowOut;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float g = 4.f * (exaggeration * o[c] - o[2 + c] / Z);
      const float u = update[2 * i + c];
      float gn = gains[2 * i + c];
      gn = u * g < 0.f ? gn + 0.2f : gn * 0.8f;
      gn = fmaxf(gn, min_gain);
      g *= gn;
      const float un = momentum * u - lr * g;
      gains[2 * i + c] = gn;
      update[2 * i + c] = un;
      y[2 * i + c] += un;
      if constexpr (ERR) g2 = fma((double)g, (double)g, g2);
    }
    if constexpr (ERR) {
      kl += (double)o[5] - (double)o[6];
      sp += (double)o[7];
    }
  }
  if constexpr (ERR) {
    g2 = block_sum_f64<16>(g2, red);
    kl = block_sum_f64<16>(kl, red);
    sp = block_sum_f64<16>(sp, red);
    if (tid == 0) {
      stats[0] = (float)(kl + log(Zd) * sp);
      stats[1] = (float)sqrt(g2);
      stats[2] = Z;
      stats[3] = (float)steps_done;
    }
  }
}

bool tsne_n_ok(int N) { return N >= 4 && N <= 16384; }

}  // namespace

hipError_t tsne_affinities(const float* x, int N, int D, int metric, float perplexity, float* P,
                           float* beta, float* dist, void* scratch, hipStream_t s) {
  if (!tsne_n_ok(N) || metric < 0 || metric > 2 || (metric != 2 && (D < 1 || D > 4096)))
    return hipErrorInvalidValue;
  double* row_sum = (double*)scratch;            // [N]
  float* nrm = (float*)(row_sum + N);            // [N]
  const float* d = x;                            // metric 2: the caller's matrix as it is
  if (metric != 2) {
    // without a dist buffer the distances go through P (a row is in LDS before it is overwritten)
    float* dd = dist ? dist : P;
    const hipError_t nr = row_norms(x, N, D, nrm, s);   // |x_i| (scoring.hip)
    if (nr != hipSuccess) return nr;
    const dim3 grid((N + 63) / 64, (N + 63) / 64);
    if (D % 4 == 0 && ((uintptr_t)x & 15) == 0)
      hipLaunchKernelGGL(tsne_dist_kernel<true>, grid, dim3(256), 0, s, x, N, D,
                         metric == 0 ? 1 : 0, nrm, dd);
    else
      hipLaunchKernelGGL(tsne_dist_kernel<false>, grid, dim3(256), 0, s, x, N, D,
                         metric == 0 ? 1 : 0, nrm, dd);
    d = dd;
  } else if (dist && dist != x) {
    const hipError_t c = hipMemcpyAsync(dist, x, (size_t)N * N * sizeof(float),
                                        hipMemcpyDeviceToDevice, s);
    if (c != hipSuccess) return c;
  }
  const size_t lds = (size_t)N * sizeof(float);
  if (lds > 48 * 1024) {   // at most 64 KiB of the 160 KiB
    const hipError_t attr = hipFuncSetAttribute((const void*)tsne_perplexity_kernel,
                                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                                64 * 1024);
    if (attr != hipSuccess) return attr;
  }
  hipLaunchKernelGGL(tsne_perplexity_kernel, dim3(N), dim3(256), lds, s, d, N, perplexity, P, beta,
                     row_sum);
  const int T = (N + 31) / 32;
  hipLaunchKernelGGL(tsne_symmetrise_kernel, dim3(T, T), dim3(256), 0, s, P, N, row_sum);
  return hipGetLastError();
}

hipError_t tsne_run(const float* P, int N, float* y, float* update, float* gains, int n_steps,
                    float exaggeration, float momentum, float lr, float min_gain, int error_every,
                    void* scratch, float* stats, hipStream_t s) {
  if (!tsne_n_ok(N) || n_steps < 1 || error_every < 0) return hipErrorInvalidValue;
  float* rows = (float*)scratch;   // [N, 8]
  const size_t lds = (size_t)N * 2 * sizeof(float);
  if (lds > 48 * 1024) {   // at most 128 KiB of the 160 KiB
    hipError_t attr = hipFuncSetAttribute((const void*)tsne_forces_kernel<false>,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    if (attr == hipSuccess)
      attr = hipFuncSetAttribute((const void*)tsne_forces_kernel<true>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    if (attr != hipSuccess) return attr;
  }
  // 4 rows per workgroup up to N = 4096 (N = 1398 -> 350 workgroups for 256 CUs), then
  // more rows per wave so that at most 1024 workgroups stage y
  const int R = N <= 4096 ? 1 : (N + 4095) / 4096;
  const int nwg = (N + 4 * R - 1) / (4 * R);
  for (int it = 0; it < n_steps; ++it) {
    const bool err = error_every > 0 ? (it + 1) % error_every == 0 : it == n_steps - 1;
    if (err) {
      hipLaunchKernelGGL(tsne_forces_kernel<true>, dim3(nwg), dim3(256), lds, s, P, y, N, R,
                         exaggeration, rows);
      hipLaunchKernelGGL(tsne_update_kernel<true>, dim3(1), dim3(1024), 0, s, rows, N, y, update,
                         gains, exaggeration, momentum, lr, min_gain, it + 1, stats);
    } else {
      hipLaunchKernelGGL(tsne_forces_kernel<false>, dim3(nwg), dim3(256), lds, s, P, y, N, R,
                         exaggeration, rows);
      hipLaunchKernelGGL(tsne_update_kernel<false>, dim3(1), dim3(1024), 0, s, rows, N, y, update,
                         gains, exaggeration, momentum, lr, min_gain, it + 1, stats);
    }
  }
  return hipGetLastError();
}

}  // namespace miclip
