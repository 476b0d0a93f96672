// Fine-tuning of the image tower's tail (methods/PEFT_openclip.py:139-384, the
// FTOpenCLIP loop): the kernels of the weight-gradient side and the optimiser.
//
//   * gemm_tn_kernel: G[Nn, K] (fp32) = sum_m A[m, Nn] * X[m, K], A and X in the
//     compute dtype, both contracted along their ROW index ("TN"): the shape of every
//     weight gradient dW = dY^T . X. The operands are staged row-major (coalesced
//     16-byte loads) into LDS, 32 rows at a time, and both MFMA fragments come out of
//     LDS through the transposing read ds_read_b64_tr_b16 (one 4-row x 16-column
//     block per 16-lane group), so neither operand is ever transposed in memory.
//     One workgroup owns a 64 x 64 output tile of one M-slice (wave w: rows 16 w ..
//     16 w + 15 of the tile, four 16 x 16 accumulators); rows past the slice and
//     columns past Nn / K are staged as zeros. The output is small and M long, so M
//     is split into slices (gemm_tn_plan, a function of the shape only) that land in
//     an fp32 workspace and are summed in ascending slice order (gemm_tn_reduce_kernel,
//     the splitk_reduce idiom), optionally times a device scalar that undoes the
//     power-of-two scale of a gradient operand.
//   * ft_amax_scale_kernel / ft_cast_scale_kernel: a gradient operand is scaled by the
//     power of two that puts its largest magnitude in [2^13, 2^14) before it is
//     rounded (RNE) to the compute dtype, and the product is unscaled in fp32 (as
//     ln_fold does for weights): small fp16 gradients do not fall into subnormals.
//   * ft_adam_kernel: torch.optim.Adam's single-tensor rule over one contiguous fp32
//     block (betas 0.9 / 0.999, bias correction by the 1-based step, no weight decay).
//   * ft_fold_kernel: the 16-row tile partials of prolip_grad -> {sum of row CE,
//     correct count}, ascending, one thread.
//   * the second half of the file: the last block, ln_post and proj behind the frozen
//     trunk (ft_grad) -- LayerNorm forward (saving xhat / rstd) and backward, CLS-query
//     attention forward (keeping p) and backward (packed dQKV), activation forward /
//     backward, chunked column sums, casts of the fp32 masters, and the closed-form
//     gradients of W_in / ln_1 from G = dQKV^T . xhat.
//   * ft_grad_rows: the same step on images picked out of a cache of trunk outputs. The
//     only two readers of x (ft_ln_fwd_kernel, ft_add_rows_kernel) take a row map, null
//     for ft_grad, so the batch is never gathered into a buffer of its own; the host's
//     indices are checked, then staged from launch arguments (stage_rows, launch.h).
//
// Determinism: every accumulation runs in ascending row order inside one wave,
// slices are added in index order, there are no atomics; the maximum behind the
// scale is order-independent.
#include <math.h>

#include "kernels.h"
#include "launch.h"

namespace miclip {

namespace {

constexpr int kTnTile = 64;       // output tile edge
constexpr int kTnRows = 32;       // contracted rows per LDS stage (one 16x16x32 k-step)
constexpr int kTnLd = 72;         // LDS row stride in elements: 144 B keeps 16-B stores and 8-B reads aligned
constexpr int kTnTargetWgs = 1024;
constexpr int kTnMaxSlices = 32;

// Rows 8 g .. 8 g + 7 (g = lane >> 4) of the staged tile, column col0 + (lane & 15):
// the 8 k-values of this lane's 16x16x32 fragment. Lane 4 q + p of a 16-lane group
// supplies the address of row q, columns 4 p .. 4 p + 3 of the block.
template <typename T>
MICLIP_DEV i16x8 tn_frag(const T* tile, int col0, int lane) {
  const int i = lane & 15, g = lane >> 4, q = i >> 2, p = i & 3;
  const LDS_AS char* a = (const LDS_AS char*)(tile + (8 * g + q) * kTnLd + col0 + 4 * p);
  const i16x4 lo = ds_read_tr16_b64(a);
  const i16x4 hi = ds_read_tr16_b64(a + 4 * kTnLd * (int)sizeof(T));
  return i16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <typename T>
__global__ __launch_bounds__(256) void gemm_tn_kernel(const T* __restrict__ A,
                                                      const T* __restrict__ X,
                                                      float* __restrict__ out, int M, int Nn,
                                                      int K, int slice_rows, int ntn) {
  __shared__ __attribute__((aligned(16))) T As[kTnRows * kTnLd];
  __shared__ __attribute__((aligned(16))) T Xs[kTnRows * kTnLd];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tn = blockIdx.x % ntn, tk = blockIdx.x / ntn, slice = blockIdx.y;
  const int n0 = tn * kTnTile, k0 = tk * kTnTile;
  const int m_begin = slice * slice_rows;
  const int m_end = m_begin + slice_rows < M ? m_begin + slice_rows : M;
  const int lr = tid >> 3, lc = (tid & 7) * 8;   // loader: row of the stage, first column
  const bool a_in = n0 + lc < Nn, x_in = k0 + lc < K;   // Nn, K % 8 == 0: a chunk is in or out whole
  const u32x4 zero = {0u, 0u, 0u, 0u};
  const f32x4 fz = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {fz, fz, fz, fz};

  u32x4 va = zero, vx = zero;
  {
    const int row = m_begin + lr;
    if (row < m_end && a_in) va = *(const u32x4*)(A + (size_t)row * Nn + n0 + lc);
    if (row < m_end && x_in) vx = *(const u32x4*)(X + (size_t)row * K + k0 + lc);
  }
  for (int m0 = m_begin; m0 < m_end; m0 += kTnRows) {
    __syncthreads();   // the previous stage's fragment reads are done
    *(u32x4*)(As + lr * kTnLd + lc) = va;
    *(u32x4*)(Xs + lr * kTnLd + lc) = vx;
    __syncthreads();
    va = zero;
    vx = zero;
    {   // the next stage's rows, in flight under the MFMAs
      const int row = m0 + kTnRows + lr;
      if (row < m_end && a_in) va = *(const u32x4*)(A + (size_t)row * Nn + n0 + lc);
      if (row < m_end && x_in) vx = *(const u32x4*)(X + (size_t)row * K + k0 + lc);
    }
    const i16x8 af = tn_frag<T>(As, 16 * w, lane);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = Mfma<T>::m16(af, tn_frag<T>(Xs, 16 * c, lane), acc[c]);
  }

  float* o = out + (size_t)slice * Nn * K;
  const int i = lane & 15, g = lane >> 4;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int kc = k0 + 16 * c + i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nn = n0 + 16 * w + 4 * g + j;
      if (nn < Nn && kc < K) o[(size_t)nn * K + kc] = acc[c][j];
    }
  }
}

__global__ __launch_bounds__(256) void gemm_tn_reduce_kernel(const float* __restrict__ ws,
                                                             float* __restrict__ G, size_t numel,
                                                             int slices,
                                                             const float* __restrict__ out_scale) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= numel) return;
  float s = ws[e];
  for (int k = 1; k < slices; ++k) s += ws[(size_t)k * numel + e];
  G[e] = out_scale ? s * *out_scale : s;
}

constexpr int kAmaxBlocks = 256;

// part[b] = max|x| over workgroup b's grid-strided elements (a maximum has no order)
__global__ __launch_bounds__(256) void ft_amax_part_kernel(const float* __restrict__ x,
                                                           size_t numel, float* __restrict__ part) {
  __shared__ float wmax[4];
  float mx = 0.f;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < numel; e += (size_t)gridDim.x * 256)
    mx = fmaxf(mx, fabsf(x[e]));
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// sc[0] = S, sc[1] = 1 / S with S the power of two that puts max|x| S in [2^(target-1),
// 2^target) (1 for an all-zero or non-finite block), from the numel partial maxima x.
__global__ __launch_bounds__(1024) void ft_amax_scale_kernel(const float* __restrict__ x,
                                                             size_t numel, float* __restrict__ sc,
                                                             int target) {
  __shared__ float wmax[16];
  float mx = 0.f;
  for (size_t e = threadIdx.x; e < numel; e += 1024) mx = fmaxf(mx, fabsf(x[e]));
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) mx = fmaxf(mx, wmax[k]);
    float S = 1.f, inv = 1.f;
    if (mx > 0.f && mx <= 3.0e38f) {
      int ex;
      frexpf(mx, &ex);   // mx = f * 2^ex, f in [0.5, 1)
      int sh = target - ex;  // mx * 2^sh in [2^(target-1), 2^target)
      sh = sh > 100 ? 100 : sh < -100 ? -100 : sh;
      S = ldexpf(1.f, sh);
      inv = ldexpf(1.f, -sh);
    }
    sc[0] = S;
    sc[1] = inv;
  }
}

constexpr int kScaleTarget = 14;

// out = {d[0], d[1] * *c_inv}: the scale of a tensor built on an already scaled one
__global__ void ft_scale_chain_kernel(const float* __restrict__ d, const float* __restrict__ c_inv,
                                      float* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  out[0] = d[0];
  out[1] = d[1] * *c_inv;
}

template <typename T>
__global__ __launch_bounds__(256) void ft_cast_scale_kernel(const float* __restrict__ in,
                                                            T* __restrict__ out, size_t numel,
                                                            const float* __restrict__ sc) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= numel) return;
  out[e] = to_t<T>(sc ? in[e] * sc[0] : in[e]);
}

// scale pair of x into sc; part: kAmaxBlocks floats of scratch
void amax_scale(const float* x, size_t numel, float* sc, float* part, int target, hipStream_t s) {
  size_t blocks = (numel + 1023) / 1024;
  blocks = blocks < 1 ? 1 : blocks > kAmaxBlocks ? kAmaxBlocks : blocks;
  hipLaunchKernelGGL(ft_amax_part_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, numel, part);
  hipLaunchKernelGGL(ft_amax_scale_kernel, dim3(1), dim3(1024), 0, s, (const float*)part, blocks,
                     sc, target);
}

struct FtAdamArgs {
  float step_size, bc2_sqrt, eps;
};

__global__ __launch_bounds__(256) void ft_adam_kernel(float* __restrict__ p,
                                                      const float* __restrict__ grad,
                                                      float* __restrict__ m, float* __restrict__ v,
                                                      size_t numel, FtAdamArgs a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= numel) return;
  const float g = grad[e], m0 = m[e], v0 = v[e];
  const float m1 = m0 + (g - m0) * 0.1f;                  // exp_avg.lerp_(grad, 1 - beta1)
  const float v1 = fmaf(0.001f, g * g, v0 * 0.999f);      // mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v1) / a.bc2_sqrt + a.eps;
  m[e] = m1;
  v[e] = v1;
  p[e] = p[e] - a.step_size * (m1 / denom);
}

// stats = {n * mean CE, correct}: prolip_grad's partials hold sums of row CE per tile
__global__ void ft_fold_kernel(const float* __restrict__ part, int ntiles,
                               float* __restrict__ stats) {
  if (threadIdx.x || blockIdx.x) return;
  float ce = 0.f, ok = 0.f;
  for (int t = 0; t < ntiles; ++t) {
    ce += part[2 * t];
    ok += part[2 * t + 1];
  }
  stats[0] = ce;
  stats[1] = ok;
}

}  // namespace

bool gemm_tn_shape_ok(int64_t M, int64_t Nn, int64_t K) {
  return M >= 1 && M <= 0x7fffffff - 64 && Nn >= 16 && K >= 16 && Nn % 16 == 0 && K % 16 == 0 &&
         Nn <= 65536 && K <= 65536;
}

void gemm_tn_plan(int M, int Nn, int K, int* slices, int* slice_rows) {
  const int tiles = ((Nn + kTnTile - 1) / kTnTile) * ((K + kTnTile - 1) / kTnTile);
  int S = (kTnTargetWgs + tiles - 1) / tiles;
  const int stages = (M + kTnRows - 1) / kTnRows;
  S = S > kTnMaxSlices ? kTnMaxSlices : S;
  S = S > stages ? stages : S;
  S = S < 1 ? 1 : S;
  int rows = (M + S - 1) / S;
  rows = (rows + kTnRows - 1) / kTnRows * kTnRows;
  *slice_rows = rows;
  *slices = (M + rows - 1) / rows;
}

size_t gemm_tn_ws_bytes(int M, int Nn, int K) {
  if (!gemm_tn_shape_ok(M, Nn, K)) return 0;
  int S, rows;
  gemm_tn_plan(M, Nn, K, &S, &rows);
  return (size_t)S * Nn * K * sizeof(float);
}

hipError_t gemm_tn(int dtype, const void* A, const void* X, float* G, int M, int Nn, int K,
                   float* ws, const float* out_scale, hipStream_t s) {
  if (!gemm_tn_shape_ok(M, Nn, K) || (dtype != kF16 && dtype != kBF16) || !A || !X || !G || !ws ||
      ((uintptr_t)A & 15) || ((uintptr_t)X & 15))
    return hipErrorInvalidValue;
  int S, rows;
  gemm_tn_plan(M, Nn, K, &S, &rows);
  const int ntn = (Nn + kTnTile - 1) / kTnTile, ntk = (K + kTnTile - 1) / kTnTile;
  const dim3 grid(ntn * ntk, S);
  if (dtype == kF16)
    hipLaunchKernelGGL(gemm_tn_kernel<_Float16>, grid, dim3(256), 0, s, (const _Float16*)A,
                       (const _Float16*)X, ws, M, Nn, K, rows, ntn);
  else
    hipLaunchKernelGGL(gemm_tn_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)A,
                       (const __bf16*)X, ws, M, Nn, K, rows, ntn);
  const size_t numel = (size_t)Nn * K;
  hipLaunchKernelGGL(gemm_tn_reduce_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, s,
                     ws, G, numel, S, out_scale);
  return hipGetLastError();
}

hipError_t ft_adam(float* params, const float* grads, float* m, float* v, int64_t numel, float lr,
                   int step, float eps, hipStream_t s) {
  if (numel < 1 || numel > ((int64_t)1 << 38) || step < 1 || !(eps >= 0.f) || !(lr >= 0.f))
    return hipErrorInvalidValue;
  // bias corrections in double, as torch's Python scalars (1 - beta ** step)
  const float bc1 = (float)(1.0 - pow(0.9, (double)step));
  const FtAdamArgs a = {lr / bc1, (float)sqrt(1.0 - pow(0.999, (double)step)), eps};
  hipLaunchKernelGGL(ft_adam_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, s,
                     params, grads, m, v, (size_t)numel, a);
  return hipGetLastError();
}

bool ft_proj_shape_ok(int64_t B, int64_t W, int64_t E, int64_t C) {
  return B >= 1 && B <= (1 << 24) && W >= 128 && W <= 1280 && W % 128 == 0 && E >= 16 &&
         E <= 1024 && E % 16 == 0 && C >= 1 && C <= 1024;
}

// scratch layout of ft_proj_grad (every piece 256-byte aligned)
struct FtProjScratch {
  size_t dz, part, sc, yc, dzc, ws, total;
};
static FtProjScratch ft_proj_layout(int B, int W, int E) {
  FtProjScratch L;
  size_t o = 0;
  L.dz = o;   o += align256((size_t)B * E * 4);
  L.part = o; o += align256((size_t)((B + 15) / 16) * 2 * 4);
  L.sc = o;   o += 256 + kAmaxBlocks * 4;   // scale pair, then the amax partials
  L.yc = o;   o += align256((size_t)B * W * 2);
  L.dzc = o;  o += align256((size_t)B * E * 2);
  L.ws = o;   o += align256(gemm_tn_ws_bytes(B, W, E));
  L.total = o;
  return L;
}

size_t ft_proj_scratch_bytes(int B, int W, int E, int C) {
  if (!ft_proj_shape_ok(B, W, E, C)) return 0;
  return ft_proj_layout(B, W, E).total;
}

hipError_t ft_proj_grad(int dtype, const float* y, const int64_t* labels, const float* tw,
                        const float* proj, int B, int W, int E, int C, float scale, float* dP,
                        void* scratch, float* stats, hipStream_t s) {
  if (!ft_proj_shape_ok(B, W, E, C) || (dtype != kF16 && dtype != kBF16) ||
      ((uintptr_t)scratch & 255) || ((uintptr_t)y & 15))
    return hipErrorInvalidValue;
  const FtProjScratch L = ft_proj_layout(B, W, E);
  char* base = (char*)scratch;
  float* dz = (float*)(base + L.dz);
  float* part = (float*)(base + L.part);
  float* sc = (float*)(base + L.sc);
  void* yc = base + L.yc;
  void* dzc = base + L.dzc;
  float* ws = (float*)(base + L.ws);
  hipError_t e = prolip_grad(kIn32, y, labels, tw, proj, dz, part, B, W, E, C, 1, scale, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ft_fold_kernel, dim3(1), dim3(64), 0, s, part, (B + 15) / 16, stats);
  const size_t ny = (size_t)B * W, nz = (size_t)B * E;
  amax_scale(dz, nz, sc, sc + 64, kScaleTarget, s);
  if (dtype == kF16) {
    hipLaunchKernelGGL(ft_cast_scale_kernel<_Float16>, dim3((unsigned)((ny + 255) / 256)),
                       dim3(256), 0, s, y, (_Float16*)yc, ny, (const float*)nullptr);
    hipLaunchKernelGGL(ft_cast_scale_kernel<_Float16>, dim3((unsigned)((nz + 255) / 256)),
                       dim3(256), 0, s, dz, (_Float16*)dzc, nz, sc);
  } else {
    hipLaunchKernelGGL(ft_cast_scale_kernel<__bf16>, dim3((unsigned)((ny + 255) / 256)), dim3(256),
                       0, s, y, (__bf16*)yc, ny, (const float*)nullptr);
    hipLaunchKernelGGL(ft_cast_scale_kernel<__bf16>, dim3((unsigned)((nz + 255) / 256)), dim3(256),
                       0, s, dz, (__bf16*)dzc, nz, sc);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return gemm_tn(dtype, yc, dzc, dP, B, W, E, ws, sc + 1, s);
}

// ======================================================================
// Group 2: the last ResidualAttentionBlock and ln_post behind the frozen trunk.
// Forward on the CLS rows only after the QKV GEMM (as run_block's cls_only), every
// GEMM operand rounded once to the compute dtype, everything else fp32; backward by
// the closed forms of DESIGN (no dgrad through the token rows: x carries no gradient).
// ======================================================================
namespace {

// sum over the workgroup (256 threads) in a fixed order: wave butterflies, then the
// four wave partials in index order; every thread gets the result
MICLIP_DEV float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
MICLIP_DEV float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

constexpr int kLnMaxPer = 8;   // D <= 2048 on 256 threads

// Source row of output row r = b * N + t under a row map: token t of image rows[b] of a
// cache of N-row blocks; the identity without a map.
MICLIP_DEV size_t ft_src_row(const int64_t* __restrict__ rows, size_t r, int N) {
  if (!rows) return r;
  const size_t b = r / (size_t)N;
  return (size_t)rows[b] * N + (r - b * N);
}

// LayerNorm of row r (read at x + ft_src_row(rows, r, N) * stride elements, written at
// row r), eps 1e-5, two-pass fp32 statistics. Any of the outputs may be null: xhat_t /
// h_t in the compute dtype, xhat_f / h_f fp32, rstd [R].
template <typename TI, typename T>
__global__ __launch_bounds__(256) void ft_ln_fwd_kernel(
    const TI* __restrict__ x, size_t stride, const int64_t* __restrict__ rows, int N,
    const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ xhat_t,
    T* __restrict__ h_t, float* __restrict__ xhat_f, float* __restrict__ h_f,
    float* __restrict__ rstd_out, int D) {
  __shared__ float red[4];
  const size_t r = blockIdx.x;
  const TI* xr = x + ft_src_row(rows, r, N) * stride;
  float v[kLnMaxPer];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kLnMaxPer; ++j) {
    const int k = threadIdx.x + 256 * j;
    v[j] = k < D ? to_f<TI>(xr[k]) : 0.f;
    s += v[j];
  }
  const float mean = block_sum(s, red) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < kLnMaxPer; ++j) {
    const int k = threadIdx.x + 256 * j;
    const float d = k < D ? v[j] - mean : 0.f;
    q = fmaf(d, d, q);
  }
  const float rstd = rsqrtf(block_sum(q, red) / (float)D + 1e-5f);
  if (rstd_out && threadIdx.x == 0) rstd_out[r] = rstd;
#pragma unroll
  for (int j = 0; j < kLnMaxPer; ++j) {
    const int k = threadIdx.x + 256 * j;
    if (k >= D) continue;
    const float xh = (v[j] - mean) * rstd, h = fmaf(xh, gamma[k], beta[k]);
    const size_t o = r * D + k;
    if (xhat_t) xhat_t[o] = to_t<T>(xh);
    if (h_t) h_t[o] = to_t<T>(h);
    if (xhat_f) xhat_f[o] = xh;
    if (h_f) h_f[o] = h;
  }
}

// dx = rstd (g - mean(g) - xhat mean(g xhat)) + resid with g = dy * (*dy_scale) * gamma
__global__ __launch_bounds__(256) void ft_ln_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ dy_scale,
    const float* __restrict__ xhat, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ resid, float* __restrict__ dx,
    int D) {
  __shared__ float red[4];
  const size_t r = blockIdx.x;
  const float sc = dy_scale ? *dy_scale : 1.f;
  float g[kLnMaxPer], xh[kLnMaxPer];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < kLnMaxPer; ++j) {
    const int k = threadIdx.x + 256 * j;
    g[j] = k < D ? dy[r * D + k] * sc * gamma[k] : 0.f;
    xh[j] = k < D ? xhat[r * D + k] : 0.f;
    s1 += g[j];
    s2 = fmaf(g[j], xh[j], s2);
  }
  const float m1 = block_sum(s1, red) / (float)D;
  const float m2 = block_sum(s2, red) / (float)D;
  const float rs = rstd[r];
#pragma unroll
  for (int j = 0; j < kLnMaxPer; ++j) {
    const int k = threadIdx.x + 256 * j;
    if (k >= D) continue;
    const float d = rs * (g[j] - m1 - xh[j] * m2);
    dx[r * D + k] = resid ? d + resid[r * D + k] : d;
  }
}

// dgamma[k] = sum_r dy[r,k] xhat[r,k], dbeta[k] = sum_r dy[r,k] (times *dy_scale), rows ascending
__global__ __launch_bounds__(256) void ft_ln_bwd_cols_kernel(
    const float* __restrict__ dy, const float* __restrict__ dy_scale,
    const float* __restrict__ xhat, float* __restrict__ dgamma, float* __restrict__ dbeta, int R,
    int D) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= D) return;
  float a = 0.f, b = 0.f;
  for (int r = 0; r < R; ++r) {
    const float d = dy[(size_t)r * D + k];
    a = fmaf(d, xhat[(size_t)r * D + k], a);
    b += d;
  }
  const float sc = dy_scale ? *dy_scale : 1.f;
  dgamma[k] = a * sc;
  dbeta[k] = b * sc;
}

// partial[c][k] = sum of rows [c * chunk, (c + 1) * chunk) of in [R, n], ascending
template <typename T>
__global__ __launch_bounds__(256) void ft_colsum_kernel(const T* __restrict__ in,
                                                        float* __restrict__ partial, int R, int n,
                                                        int chunk) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int r0 = blockIdx.y * chunk, r1 = r0 + chunk < R ? r0 + chunk : R;
  float a = 0.f;
  for (int r = r0; r < r1; ++r) a += to_f<T>(in[(size_t)r * n + k]);
  partial[(size_t)blockIdx.y * n + k] = a;
}

// CLS-query attention of one (image, head): p = softmax(q K^T / sqrt(dh)) kept in fp32
// [B, H, N], o = p V rounded to the compute dtype [B, W]. N <= 768, dh <= 80.
template <typename T>
__global__ __launch_bounds__(256) void ft_attn_fwd_kernel(const T* __restrict__ qkv,
                                                          T* __restrict__ o, float* __restrict__ p,
                                                          int N, int W, int dh, float inv_sqrt) {
  __shared__ float qs[80], ps[768], red[4];
  const int b = blockIdx.x, h = blockIdx.y, H = gridDim.y, tid = threadIdx.x;
  const T* base = qkv + (size_t)b * N * 3 * W + h * dh;
  if (tid < dh) qs[tid] = to_f<T>(base[tid]);
  __syncthreads();
  float mx = -INFINITY;
  for (int n = tid; n < N; n += 256) {
    const T* kr = base + (size_t)n * 3 * W + W;
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s = fmaf(qs[d], to_f<T>(kr[d]), s);
    s *= inv_sqrt;
    ps[n] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_max(mx, red);
  float se = 0.f;
  for (int n = tid; n < N; n += 256) {
    const float e = expf(ps[n] - mx);
    ps[n] = e;
    se += e;
  }
  se = block_sum(se, red);
  float* pr = p + ((size_t)b * H + h) * N;
  for (int n = tid; n < N; n += 256) {
    const float v = ps[n] / se;
    ps[n] = v;
    pr[n] = v;
  }
  __syncthreads();
  if (tid < dh) {
    const T* vr = base + 2 * W + tid;
    float a = 0.f;
    for (int n = 0; n < N; ++n) a = fmaf(ps[n], to_f<T>(vr[(size_t)n * 3 * W]), a);
    o[(size_t)b * W + h * dh + tid] = to_t<T>(a);
  }
}

// Backward of the same: with dO = d_o * (*mult), dP[n] = dO . V[n], dS = p (dP - sum p dP),
// dV[n] = p[n] dO, dK[n] = dS[n] q / sqrt(dh), dq = sum_n dS[n] K[n] / sqrt(dh); written in
// the packed qkv layout (Q rows other than the CLS row are zero).
template <typename T>
__global__ __launch_bounds__(256) void ft_attn_bwd_kernel(
    const T* __restrict__ qkv, const float* __restrict__ p, const float* __restrict__ d_o,
    const float* __restrict__ mult, T* __restrict__ dqkv, int N, int W, int dh, float inv_sqrt) {
  __shared__ float qs[80], dos[80], dqs[80], ps[768], dss[768], red[4];
  const int b = blockIdx.x, h = blockIdx.y, H = gridDim.y, tid = threadIdx.x;
  const size_t row0 = (size_t)b * N * 3 * W + h * dh;
  const T* base = qkv + row0;
  const float m = mult ? *mult : 1.f;
  if (tid < dh) {
    qs[tid] = to_f<T>(base[tid]);
    dos[tid] = d_o[(size_t)b * W + h * dh + tid] * m;
  }
  const float* pr = p + ((size_t)b * H + h) * N;
  __syncthreads();
  float part = 0.f;
  for (int n = tid; n < N; n += 256) {
    const T* vr = base + (size_t)n * 3 * W + 2 * W;
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s = fmaf(dos[d], to_f<T>(vr[d]), s);
    const float pn = pr[n];
    ps[n] = pn;
    dss[n] = s;
    part = fmaf(pn, s, part);
  }
  const float delta = block_sum(part, red);
  for (int n = tid; n < N; n += 256) dss[n] = ps[n] * (dss[n] - delta);
  __syncthreads();
  if (tid < dh) {
    const T* kr = base + W + tid;
    float a = 0.f;
    for (int n = 0; n < N; ++n) a = fmaf(dss[n], to_f<T>(kr[(size_t)n * 3 * W]), a);
    dqs[tid] = a * inv_sqrt;
  }
  __syncthreads();
  T* ob = dqkv + row0;
  for (int idx = tid; idx < N * dh; idx += 256) {
    const int n = idx / dh, d = idx - n * dh;
    T* orow = ob + (size_t)n * 3 * W + d;
    orow[0] = to_t<T>(n == 0 ? dqs[d] : 0.f);
    orow[W] = to_t<T>(dss[n] * qs[d] * inv_sqrt);
    orow[2 * W] = to_t<T>(ps[n] * dos[d]);
  }
}

MICLIP_DEV float act_fwd(float u, int act) {
  if (act == ACT_QUICKGELU) return u / (1.f + expf(-1.702f * u));
  return 0.5f * u * (1.f + erff(u * 0.70710678118654752f));
}
MICLIP_DEV float act_grad(float u, int act) {
  if (act == ACT_QUICKGELU) {
    const float sg = 1.f / (1.f + expf(-1.702f * u));
    return sg * (1.f + 1.702f * u * (1.f - sg));
  }
  return 0.5f * (1.f + erff(u * 0.70710678118654752f)) +
         u * 0.3989422804014327f * expf(-0.5f * u * u);
}

template <typename T>
__global__ __launch_bounds__(256) void ft_act_fwd_kernel(const float* __restrict__ u,
                                                         T* __restrict__ a, size_t numel, int act) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < numel) a[e] = to_t<T>(act_fwd(u[e], act));
}

// du = da * (*mult) * act'(u)
__global__ __launch_bounds__(256) void ft_act_bwd_kernel(const float* __restrict__ da,
                                                         const float* __restrict__ mult,
                                                         const float* __restrict__ u,
                                                         float* __restrict__ du, size_t numel,
                                                         int act) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < numel) du[e] = da[e] * *mult * act_grad(u[e], act);
}

// out[b, k] = a[b, k] + x[i * stride + k], i = rows[b] under a row map and b without one
// (the residual around the attention, CLS rows)
template <typename TI>
__global__ __launch_bounds__(256) void ft_add_rows_kernel(const float* __restrict__ a,
                                                          const TI* __restrict__ x, size_t stride,
                                                          const int64_t* __restrict__ rows,
                                                          float* __restrict__ out, int B, int D) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)B * D) return;
  const size_t b = e / D, k = e - b * D;
  const size_t i = rows ? (size_t)rows[b] : b;
  out[e] = a[e] + to_f<TI>(x[i * stride + k]);
}

__global__ __launch_bounds__(256) void ft_add_kernel(const float* __restrict__ a,
                                                     const float* __restrict__ b,
                                                     float* __restrict__ out, size_t numel) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < numel) out[e] = a[e] + b[e];
}

// out [C, R] = in [R, C] transposed, rounded to TO (fp32 -> fp32 copies)
template <typename TO>
__global__ __launch_bounds__(256) void ft_cast_t_kernel(const float* __restrict__ in,
                                                        TO* __restrict__ out, int R, int C) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  for (int j = ty; j < 32; j += 8)
    tile[j][tx] = (r0 + j < R && c0 + tx < C) ? in[(size_t)(r0 + j) * C + c0 + tx] : 0.f;
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (c0 + j < C && r0 + tx < R) {
      if constexpr (sizeof(TO) == 4) out[(size_t)(c0 + j) * R + r0 + tx] = tile[tx][j];
      else out[(size_t)(c0 + j) * R + r0 + tx] = to_t<TO>(tile[tx][j]);
    }
}

// dW_in = G * gamma (columns) + db (x) beta, in place on G [3W, W]
__global__ __launch_bounds__(256) void ft_win_grad_kernel(float* __restrict__ G,
                                                          const float* __restrict__ db,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          float* __restrict__ dW, size_t rows,
                                                          int W) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * W) return;
  const size_t n = e / W, k = e - n * W;
  dW[e] = fmaf(G[e], gamma[k], db[n] * beta[k]);
}

// dgamma1[k] = sum_n W_in[n,k] G[n,k], dbeta1[k] = sum_n W_in[n,k] db[n]: workgroup
// (x, c) sums rows [c * chunk, (c + 1) * chunk) ascending into part[c][0][k] / part[c][1][k];
// the chunks are then added in index order (gemm_tn_reduce_kernel)
__global__ __launch_bounds__(256) void ft_ln1_grad_kernel(const float* __restrict__ Win,
                                                          const float* __restrict__ G,
                                                          const float* __restrict__ db,
                                                          float* __restrict__ part, int rows,
                                                          int W, int chunk) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= W) return;
  const int n0 = blockIdx.y * chunk, n1 = n0 + chunk < rows ? n0 + chunk : rows;
  float a = 0.f, b = 0.f;
  for (int n = n0; n < n1; ++n) {
    const float w = Win[(size_t)n * W + k];
    a = fmaf(w, G[(size_t)n * W + k], a);
    b = fmaf(w, db[n], b);
  }
  part[(size_t)blockIdx.y * 2 * W + k] = a;
  part[(size_t)blockIdx.y * 2 * W + W + k] = b;
}

unsigned nblk(size_t n) { return (unsigned)((n + 255) / 256); }

struct Bump {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += align256(bytes);
    return o;
  }
};

constexpr int kColChunks = 64;

}  // namespace

void ft_layout(int W, int E, int64_t* off) {
  const int64_t w = W, sizes[kFtTensors] = {w, w, 3 * w * w, 3 * w, w * w, w, w, w, 4 * w * w, 4 * w,
                                            4 * w * w, w, w, w, w * (int64_t)E};
  int64_t o = 0;
  for (int i = 0; i < kFtTensors; ++i) {
    off[i] = o;
    o += sizes[i];
  }
  off[kFtTensors] = o;
}

bool ft_shape_ok(int64_t B, int64_t N, int64_t W, int64_t E, int64_t C, int64_t dh) {
  return ft_proj_shape_ok(B, W, E, C) && N >= 1 && N <= 768 && (dh == 64 || dh == 80) &&
         W % dh == 0 && B * N <= 0x7fffffff - 64;
}

struct FtScratch {
  size_t xhat, h, qkv, dqkv, p, o, x1, xhat2, rstd2, h2, u, a, tmp, x2, y, xhat3, rstd3, head,
      projT, dy, dx2, dxc, da, du, duc, dh2, dx1, d_o, win, wo, wfc, wpr, woT, wfcT, wprT, G, db,
      colp, tnws, sc, total;
};
static FtScratch ft_scratch_layout(int B, int N, int W, int E) {
  FtScratch L;
  Bump a;
  const size_t M = (size_t)B * N, w = W, b = B;
  L.xhat = a.take(M * w * 2);
  L.h = a.take(M * w * 2);
  L.qkv = a.take(M * 3 * w * 2);
  L.dqkv = a.take(M * 3 * w * 2);
  L.p = a.take(M * (w / 64 + 1) * 4);   // [B, H, N], H <= W / 64
  L.o = a.take(b * w * 2);
  L.x1 = a.take(b * w * 4);
  L.xhat2 = a.take(b * w * 4);
  L.rstd2 = a.take(b * 4);
  L.h2 = a.take(b * w * 2);
  L.u = a.take(b * 4 * w * 4);
  L.a = a.take(b * 4 * w * 2);
  L.tmp = a.take(b * w * 4);
  L.x2 = a.take(b * w * 4);
  L.y = a.take(b * w * 4);
  L.xhat3 = a.take(b * w * 4);
  L.rstd3 = a.take(b * 4);
  L.head = a.take(ft_proj_layout(B, W, E).total);
  L.projT = a.take(w * E * 4);
  L.dy = a.take(b * w * 4);
  L.dx2 = a.take(b * w * 4);
  L.dxc = a.take(b * w * 2);
  L.da = a.take(b * 4 * w * 4);
  L.du = a.take(b * 4 * w * 4);
  L.duc = a.take(b * 4 * w * 2);
  L.dh2 = a.take(b * w * 4);
  L.dx1 = a.take(b * w * 4);
  L.d_o = a.take(b * w * 4);
  L.win = a.take(3 * w * w * 2);
  L.wo = a.take(w * w * 2);
  L.wfc = a.take(4 * w * w * 2);
  L.wpr = a.take(4 * w * w * 2);
  L.woT = a.take(w * w * 2);
  L.wfcT = a.take(4 * w * w * 2);
  L.wprT = a.take(4 * w * w * 2);
  L.G = a.take(3 * w * w * 4);
  L.db = a.take(3 * w * 4);
  L.colp = a.take((size_t)kColChunks * 4 * w * 4);
  size_t ws = gemm_tn_ws_bytes(B, W, 4 * W);
  const size_t c[] = {gemm_tn_ws_bytes(B, 4 * W, W), gemm_tn_ws_bytes(B, W, W),
                      gemm_tn_ws_bytes((int)M, 3 * W, W)};
  for (size_t v : c) ws = v > ws ? v : ws;
  L.tnws = a.take(ws);
  L.sc = a.take(256 + kAmaxBlocks * 4);   // scale pairs, then the amax partials
  L.total = a.off;
  return L;
}

size_t ft_scratch_bytes(int B, int N, int W, int E, int C, int dh) {
  if (!ft_shape_ok(B, N, W, E, C, dh)) return 0;
  return ft_scratch_layout(B, N, W, E).total;
}

namespace {

template <typename T>
hipError_t colsum(const T* in, float* partial, float* out, int R, int n, const float* out_scale,
                  hipStream_t s) {
  int chunks = (R + 63) / 64;
  chunks = chunks > kColChunks ? kColChunks : chunks;
  const int chunk = (R + chunks - 1) / chunks;
  chunks = (R + chunk - 1) / chunk;
  hipLaunchKernelGGL(ft_colsum_kernel<T>, dim3(nblk(n), chunks), dim3(256), 0, s, in, partial, R,
                     n, chunk);
  hipLaunchKernelGGL(gemm_tn_reduce_kernel, dim3(nblk(n)), dim3(256), 0, s, partial, out,
                     (size_t)n, chunks, out_scale);
  return hipGetLastError();
}

template <typename T>
void cast_scaled(const float* in, void* out, size_t numel, float* sc, float* part, hipStream_t s) {
  amax_scale(in, numel, sc, part, kScaleTarget, s);
  hipLaunchKernelGGL(ft_cast_scale_kernel<T>, dim3(nblk(numel)), dim3(256), 0, s, in, (T*)out,
                     numel, (const float*)sc);
}

#define FT_TRY(expr)                     \
  do {                                   \
    const hipError_t e_ = (expr);        \
    if (e_ != hipSuccess) return e_;     \
  } while (0)

template <typename T, typename TI>
hipError_t ft_grad_t(int dtype, const TI* x, const int64_t* rows, const int64_t* labels,
                     const float* tw,
                     const float* P, int B, int N, int W, int E, int C, int dh, int act,
                     float scale, int groups, float* grads, char* base, float* stats,
                     float* y_out, hipStream_t s) {
  const FtScratch L = ft_scratch_layout(B, N, W, E);
  int64_t off[kFtTensors + 1];
  ft_layout(W, E, off);
  const int M = B * N, H = W / dh;
  const float inv_sqrt = 1.f / sqrtf((float)dh);
  const size_t bw = (size_t)B * W;
  auto F = [&](size_t o) { return (float*)(base + o); };
  auto Tp = [&](size_t o) { return (T*)(base + o); };
  const float *ln1g = P + off[0], *ln1b = P + off[1], *Win = P + off[2], *bin = P + off[3],
              *Wo = P + off[4], *bo = P + off[5], *ln2g = P + off[6], *ln2b = P + off[7],
              *Wfc = P + off[8], *bfc = P + off[9], *Wpr = P + off[10], *bpr = P + off[11],
              *lnpg = P + off[12], *lnpb = P + off[13], *proj = P + off[14];
  float* sc = F(L.sc);   // scale pairs {S, 1 / S}: [0] dx2, [2] du, [4] dx1, [6] d_o, [8] chained

  // ---- per-step casts of the fp32 masters ----
  const size_t w2 = (size_t)W * W;
  hipLaunchKernelGGL(ft_cast_scale_kernel<T>, dim3(nblk(3 * w2)), dim3(256), 0, s, Win, Tp(L.win),
                     3 * w2, (const float*)nullptr);
  hipLaunchKernelGGL(ft_cast_scale_kernel<T>, dim3(nblk(w2)), dim3(256), 0, s, Wo, Tp(L.wo), w2,
                     (const float*)nullptr);
  hipLaunchKernelGGL(ft_cast_scale_kernel<T>, dim3(nblk(4 * w2)), dim3(256), 0, s, Wfc, Tp(L.wfc),
                     4 * w2, (const float*)nullptr);
  hipLaunchKernelGGL(ft_cast_scale_kernel<T>, dim3(nblk(4 * w2)), dim3(256), 0, s, Wpr, Tp(L.wpr),
                     4 * w2, (const float*)nullptr);

  // ---- forward ----
  hipLaunchKernelGGL((ft_ln_fwd_kernel<TI, T>), dim3(M), dim3(256), 0, s, x, (size_t)W, rows, N,
                     ln1g, ln1b, Tp(L.xhat), Tp(L.h), (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, W);
  FT_TRY(gemm_store(dtype, Tp(L.h), Tp(L.win), bin, Tp(L.qkv), M, 3 * W, W, ACT_NONE, s));
  hipLaunchKernelGGL(ft_attn_fwd_kernel<T>, dim3(B, H), dim3(256), 0, s, Tp(L.qkv), Tp(L.o),
                     F(L.p), N, W, dh, inv_sqrt);
  FT_TRY(gemm_f32(dtype, Tp(L.o), Tp(L.wo), bo, F(L.tmp), B, W, W, s));
  hipLaunchKernelGGL(ft_add_rows_kernel<TI>, dim3(nblk(bw)), dim3(256), 0, s, F(L.tmp), x,
                     (size_t)N * W, rows, F(L.x1), B, W);
  hipLaunchKernelGGL((ft_ln_fwd_kernel<float, T>), dim3(B), dim3(256), 0, s, F(L.x1), (size_t)W,
                     (const int64_t*)nullptr, 1, ln2g, ln2b, (T*)nullptr, Tp(L.h2), F(L.xhat2),
                     (float*)nullptr, F(L.rstd2), W);
  FT_TRY(gemm_f32(dtype, Tp(L.h2), Tp(L.wfc), bfc, F(L.u), B, 4 * W, W, s));
  hipLaunchKernelGGL(ft_act_fwd_kernel<T>, dim3(nblk(4 * bw)), dim3(256), 0, s, F(L.u), Tp(L.a),
                     4 * bw, act);
  FT_TRY(gemm_f32(dtype, Tp(L.a), Tp(L.wpr), bpr, F(L.tmp), B, W, 4 * W, s));
  hipLaunchKernelGGL(ft_add_kernel, dim3(nblk(bw)), dim3(256), 0, s, F(L.tmp), F(L.x1), F(L.x2),
                     bw);
  hipLaunchKernelGGL((ft_ln_fwd_kernel<float, T>), dim3(B), dim3(256), 0, s, F(L.x2), (size_t)W,
                     (const int64_t*)nullptr, 1, lnpg, lnpb, (T*)nullptr, (T*)nullptr, F(L.xhat3),
                     F(L.y), F(L.rstd3), W);
  if (y_out)
    FT_TRY(hipMemcpyAsync(y_out, F(L.y), bw * 4, hipMemcpyDeviceToDevice, s));

  // ---- head: loss, correct count, dP, and dZ for the rest ----
  FT_TRY(ft_proj_grad(dtype, F(L.y), labels, tw, proj, B, W, E, C, scale, grads + off[14],
                      base + L.head, stats, s));
  if (groups < 2) return hipGetLastError();
  const FtProjScratch LH = ft_proj_layout(B, W, E);
  const float* dZ = (const float*)(base + L.head + LH.dz);

  // ---- backward ----
  hipLaunchKernelGGL(ft_cast_t_kernel<float>, dim3((E + 31) / 32, (W + 31) / 32), dim3(256), 0, s,
                     proj, F(L.projT), W, E);
  FT_TRY(rowvec_matmul(dZ, F(L.projT), F(L.dy), B, E, W, s));
  // ln_post
  hipLaunchKernelGGL(ft_ln_bwd_cols_kernel, dim3(nblk(W)), dim3(256), 0, s, F(L.dy),
                     (const float*)nullptr, F(L.xhat3), grads + off[12], grads + off[13], B, W);
  hipLaunchKernelGGL(ft_ln_bwd_kernel, dim3(B), dim3(256), 0, s, F(L.dy), (const float*)nullptr,
                     F(L.xhat3), F(L.rstd3), lnpg, (const float*)nullptr, F(L.dx2), W);
  // c_proj
  hipLaunchKernelGGL(ft_cast_t_kernel<T>, dim3((4 * W + 31) / 32, (W + 31) / 32), dim3(256), 0, s,
                     Wpr, Tp(L.wprT), W, 4 * W);
  cast_scaled<T>(F(L.dx2), Tp(L.dxc), bw, sc + 0, sc + 64, s);
  FT_TRY(gemm_tn(dtype, Tp(L.dxc), Tp(L.a), grads + off[10], B, W, 4 * W, F(L.tnws), sc + 1, s));
  FT_TRY(colsum<float>(F(L.dx2), F(L.colp), grads + off[11], B, W, nullptr, s));
  FT_TRY(gemm_f32(dtype, Tp(L.dxc), Tp(L.wprT), nullptr, F(L.da), B, 4 * W, W, s));
  hipLaunchKernelGGL(ft_act_bwd_kernel, dim3(nblk(4 * bw)), dim3(256), 0, s, F(L.da),
                     (const float*)(sc + 1), F(L.u), F(L.du), 4 * bw, act);
  // c_fc
  hipLaunchKernelGGL(ft_cast_t_kernel<T>, dim3((W + 31) / 32, (4 * W + 31) / 32), dim3(256), 0, s,
                     Wfc, Tp(L.wfcT), 4 * W, W);
  cast_scaled<T>(F(L.du), Tp(L.duc), 4 * bw, sc + 2, sc + 64, s);
  FT_TRY(gemm_tn(dtype, Tp(L.duc), Tp(L.h2), grads + off[8], B, 4 * W, W, F(L.tnws), sc + 3, s));
  FT_TRY(colsum<float>(F(L.du), F(L.colp), grads + off[9], B, 4 * W, nullptr, s));
  FT_TRY(gemm_f32(dtype, Tp(L.duc), Tp(L.wfcT), nullptr, F(L.dh2), B, W, 4 * W, s));
  // ln_2 and the residual
  hipLaunchKernelGGL(ft_ln_bwd_cols_kernel, dim3(nblk(W)), dim3(256), 0, s, F(L.dh2),
                     (const float*)(sc + 3), F(L.xhat2), grads + off[6], grads + off[7], B, W);
  hipLaunchKernelGGL(ft_ln_bwd_kernel, dim3(B), dim3(256), 0, s, F(L.dh2), (const float*)(sc + 3),
                     F(L.xhat2), F(L.rstd2), ln2g, (const float*)F(L.dx2), F(L.dx1), W);
  // out-proj
  hipLaunchKernelGGL(ft_cast_t_kernel<T>, dim3((W + 31) / 32, (W + 31) / 32), dim3(256), 0, s, Wo,
                     Tp(L.woT), W, W);
  cast_scaled<T>(F(L.dx1), Tp(L.dxc), bw, sc + 4, sc + 64, s);
  FT_TRY(gemm_tn(dtype, Tp(L.dxc), Tp(L.o), grads + off[4], B, W, W, F(L.tnws), sc + 5, s));
  FT_TRY(colsum<float>(F(L.dx1), F(L.colp), grads + off[5], B, W, nullptr, s));
  FT_TRY(gemm_f32(dtype, Tp(L.dxc), Tp(L.woT), nullptr, F(L.d_o), B, W, W, s));
  // attention: d_o holds dO * S(dx1); the power of two sc[6] puts max|d_o| sc[6] in [2^4, 2^5)
  // (dV = p dO stays that small, dK = dS q / sqrt(dh) has room to be larger) for the
  // compute-dtype dQKV, and sc[9] = 1 / (S(dx1) sc[6]) unscales what is built on it
  amax_scale(F(L.d_o), bw, sc + 6, sc + 64, 5, s);
  hipLaunchKernelGGL(ft_scale_chain_kernel, dim3(1), dim3(64), 0, s, sc + 6, sc + 5, sc + 8);
  hipLaunchKernelGGL(ft_attn_bwd_kernel<T>, dim3(B, H), dim3(256), 0, s, Tp(L.qkv), F(L.p),
                     F(L.d_o), (const float*)(sc + 8), Tp(L.dqkv), N, W, dh, inv_sqrt);
  FT_TRY(gemm_tn(dtype, Tp(L.dqkv), Tp(L.xhat), F(L.G), M, 3 * W, W, F(L.tnws), sc + 9, s));
  FT_TRY(colsum<T>(Tp(L.dqkv), F(L.colp), F(L.db), M, 3 * W, sc + 9, s));
  FT_TRY(hipMemcpyAsync(grads + off[3], F(L.db), (size_t)3 * W * 4, hipMemcpyDeviceToDevice, s));
  // ln_1.weight and ln_1.bias are adjacent in the block: one reduce writes both
  const int lchunk = (3 * W + kColChunks - 1) / kColChunks, lchunks = (3 * W + lchunk - 1) / lchunk;
  hipLaunchKernelGGL(ft_ln1_grad_kernel, dim3(nblk(W), lchunks), dim3(256), 0, s, Win, F(L.G),
                     F(L.db), F(L.colp), 3 * W, W, lchunk);
  hipLaunchKernelGGL(gemm_tn_reduce_kernel, dim3(nblk(2 * (size_t)W)), dim3(256), 0, s,
                     (const float*)F(L.colp), grads + off[0], (size_t)2 * W, lchunks,
                     (const float*)nullptr);
  hipLaunchKernelGGL(ft_win_grad_kernel, dim3(nblk(3 * w2)), dim3(256), 0, s, F(L.G), F(L.db),
                     ln1g, ln1b, grads + off[2], (size_t)3 * W, W);
  return hipGetLastError();
}

}  // namespace

// rows (device, nullable): the row map of ft_grad_rows; null reads x as it lies
static hipError_t ft_grad_any(int dtype, int x_dtype, const void* x, const int64_t* rows,
                              const int64_t* labels, const float* tw, const float* params, int B,
                              int N, int W, int E, int C, int dh, int act, float scale, int groups,
                              float* grads, void* scratch, float* stats, float* y_out,
                              hipStream_t s) {
  if (!ft_shape_ok(B, N, W, E, C, dh) || (dtype != kF16 && dtype != kBF16) ||
      (x_dtype != kF16 && x_dtype != kIn32) || (act != ACT_QUICKGELU && act != ACT_GELU) ||
      (groups != 1 && groups != 2) || ((uintptr_t)scratch & 255))
    return hipErrorInvalidValue;
  char* base = (char*)scratch;
#define FT_CALL(T, TI)                                                                         \
  return ft_grad_t<T, TI>(dtype, (const TI*)x, rows, labels, tw, params, B, N, W, E, C, dh,   \
                          act, scale, groups, grads, base, stats, y_out, s)
  if (dtype == kF16 && x_dtype == kF16) FT_CALL(_Float16, _Float16);
  if (dtype == kF16) FT_CALL(_Float16, float);
  if (x_dtype == kF16) FT_CALL(__bf16, _Float16);
  FT_CALL(__bf16, float);
#undef FT_CALL
}

hipError_t ft_grad(int dtype, int x_dtype, const void* x, const int64_t* labels, const float* tw,
                   const float* params, int B, int N, int W, int E, int C, int dh, int act,
                   float scale, int groups, float* grads, void* scratch, float* stats,
                   float* y_out, hipStream_t s) {
  return ft_grad_any(dtype, x_dtype, x, nullptr, labels, tw, params, B, N, W, E, C, dh, act, scale,
                     groups, grads, scratch, stats, y_out, s);
}

bool ft_rows_shape_ok(int64_t cache_images, int64_t B, int64_t N, int64_t W, int64_t E, int64_t C,
                      int64_t dh) {
  return ft_shape_ok(B, N, W, E, C, dh) && cache_images >= 1 &&
         cache_images <= (((int64_t)1 << 47) - 1) / (N * W);
}

size_t ft_rows_scratch_bytes(int B, int N, int W, int E, int C, int dh) {
  const size_t base = ft_scratch_bytes(B, N, W, E, C, dh);
  return base ? base + align256((size_t)B * sizeof(int64_t)) : 0;
}

hipError_t ft_grad_rows(int dtype, int x_dtype, const void* x_cache, int64_t cache_images,
                        const int64_t* rows_host, const int64_t* labels, const float* tw,
                        const float* params, int B, int N, int W, int E, int C, int dh, int act,
                        float scale, int groups, float* grads, void* scratch, float* stats,
                        float* y_out, hipStream_t s) {
  if (!ft_rows_shape_ok(cache_images, B, N, W, E, C, dh) || !rows_host || !scratch ||
      ((uintptr_t)scratch & 255))
    return hipErrorInvalidValue;
  for (int b = 0; b < B; ++b)   // before any launch: no kernel sees an index outside the cache
    if (rows_host[b] < 0 || rows_host[b] >= cache_images) return hipErrorInvalidValue;
  // the index area follows ft_grad's own scratch; each piece travels as launch arguments, so
  // the caller's array is free on return and the stream is never waited for
  int64_t* rows = (int64_t*)((char*)scratch + ft_scratch_bytes(B, N, W, E, C, dh));
  stage_rows(rows, B, s, [&](int b) { return rows_host[b]; });
  FT_TRY(hipGetLastError());
  return ft_grad_any(dtype, x_dtype, x_cache, rows, labels, tw, params, B, N, W, E, C, dh, act,
                     scale, groups, grads, scratch, stats, y_out, s);
}

}  // namespace miclip
