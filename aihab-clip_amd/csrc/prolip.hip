// ProLIP projector training on the cached pre-projection features
// (methods/ProLIP.py:165-259 and search_init_hp, :302-361), one optimiser step of
// G independent configurations per pair of launches. All fp32 on the f32-input
// MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation), X read
// as fp32 / fp16 / bf16 and widened in the load (exact). The two products that
// reach the softmax through scale (Z = X P and f W) keep their running sum as a
// compensated (hi, lo) pair (mfma_k_comp): their rounding, times scale, times
// Adam's first-step lr / eps, is what moves a trained weight away from fp64.
//
//   * prolip_grad_kernel (launch A), grid (ceil(n/16), G), one 16-row tile of one
//     configuration per workgroup:
//       Z = X P_g -> nrm = max(|z|, 1e-12), f = Z / nrm      (:232-233, F.normalize)
//       L = scale * f W                                       (:234)
//       softmax with the row maximum subtracted, CE, argmax   (:244, :248)
//       Gm = (softmax - onehot(y)) / n
//       dF = scale * Gm W^T,  dZ = (dF - f (f . dF)) / nrm    (the backward of
//     :232-234 written out). f . dF is taken as sum_c Gm[c] L[c] -- the same
//     number, since L = scale f W -- so it falls out of the softmax pass and the
//     dF tile never has to be held next to f. The f tile [16, E] and the logits /
//     Gm tile [16, C] stay in LDS; only dZ and two partials per tile (sum of CE,
//     number of rows with argmax == y) reach memory.
//   * prolip_adam_kernel (launch B), grid (ceil(E/32), ceil(D/32), G), one 32 x 32
//     tile of P_g per workgroup (one 16 x 16 tile per wave):
//       dP = X^T dZ_g + 2 lambda_g (P_g - P0)                 (:243-246, backward)
//       torch.optim.Adam's update of P_g, m_g, v_g in the epilogue (:165, :256),
//     dP stays in registers. Per tile: the partial of sum((P_g - P0)^2) on P
//     before the update (loss2, :243).
//   * prolip_fold_kernel, grid G: both launches' partials summed in a fixed order
//     into the history record {mean CE, MSE, correct} (loss1 / loss2 / acc of
//     :248-252, which the reference fetches with two .item() per step).
//
// Determinism: every k loop runs in ascending order over its full range inside
// one wave (waves split output tiles, never k), row and tile partials are folded
// by fixed butterflies or in index order, there are no atomics. A configuration
// reads only its own slice of P / m / v / dZ and the shared X, W, P0, so its
// result does not depend on G or on its index. Tail rows of the last 16-row tile
// are clamped on the load and masked to zero (launch A: Gm = 0 and no dZ store;
// launch B: zero operands behind every real row of the ascending k chain).
#include <math.h>

#include "kernels.h"
#include "launch.h"
#include "mfma_f32.h"

namespace miclip {

namespace {

// Error-free addition of p into the pair (hi, lo): hi + lo + p is preserved exactly
// (Knuth's TwoSum; no multiplications, so contraction cannot touch it).
MICLIP_DEV void two_sum(f32x4& hi, f32x4& lo, const f32x4 p) {
  const f32x4 s = hi + p;
  const f32x4 bb = s - hi;
  lo += (hi - (s - bb)) + (p - bb);
  hi = s;
}

// mfma_k (mfma_f32.h) with a compensated accumulator, for the two products whose rounding is
// multiplied by `scale` on its way into the softmax (Z = X P and f W): every MFMA
// (4 k) starts from zero and its result is added to a running (hi, lo) pair without
// error, so the only roundings left are inside the 4-term MFMA sums, at the size of
// those short sums rather than of the running total. MFMA s of every chunk feeds
// pair s (four independent chains, so neither the MFMAs nor the TwoSums of a chunk
// wait for one another); the pairs are merged in index order at the end. Ascending
// k within each chain.
template <typename FA, typename FB>
MICLIP_DEV f32x4 mfma_k_comp(int nch, FA fa, FB fb) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 h0 = zero, h1 = zero, h2 = zero, h3 = zero, l0 = zero, l1 = zero, l2 = zero, l3 = zero;
  const auto chunk = [&](const f32x4& a, const f32x4& b) {
    two_sum(h0, l0, __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, zero, 0, 0, 0));
    two_sum(h1, l1, __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, zero, 0, 0, 0));
    two_sum(h2, l2, __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, zero, 0, 0, 0));
    two_sum(h3, l3, __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, zero, 0, 0, 0));
  };
  int ch = 0;
  for (; ch + 2 <= nch; ch += 2) {   // the loads of two chunks are issued together
    const f32x4 a0 = fa(ch), b0 = fb(ch), a1 = fa(ch + 1), b1 = fb(ch + 1);
    chunk(a0, b0);
    chunk(a1, b1);
  }
  if (ch < nch) chunk(fa(ch), fb(ch));
  two_sum(h0, l0, h1);
  two_sum(h0, l0, h2);
  two_sum(h0, l0, h3);
  return h0 + ((l0 + l1) + (l2 + l3));
}

template <typename T>
__global__ __launch_bounds__(256) void prolip_grad_kernel(
    const T* __restrict__ x, const int64_t* __restrict__ y, const float* __restrict__ P,
    const float* __restrict__ W, float* __restrict__ dZ, float* __restrict__ part, int n, int D,
    int E, int C, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Cp = (C + 15) & ~15, ldz = E + kLdsPad, ldl = Cp + kLdsPad;
  float* Zs = (float*)smem;        // [16][ldz]  Z, then f
  float* Ls = Zs + 16 * ldz;       // [16][ldl]  logits, then Gm (columns C .. Cp-1 zero)
  float* rowv = Ls + 16 * ldl;     // [4][16]    nrm, f . dF, CE, correct
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, g = lane >> 4;
  const int r0 = blockIdx.x * 16, cfg = blockIdx.y;
  const float* Pg = P + (size_t)cfg * D * E;

  // Z = X P_g: wave w takes column tiles w, w + 4, ...
  {
    const int row = r0 + i < n ? r0 + i : n - 1;
    const T* xp = x + (size_t)row * D + 4 * g;
    for (int et = w; et < E / 16; et += 4) {
      const float* pp = Pg + (size_t)(4 * g) * E + et * 16 + i;
      const f32x4 acc = mfma_k_comp(
          D / 16, [&](int ch) { return load4<T>(xp + 16 * ch); },
          [&](int ch) {
            const float* q = pp + (size_t)(16 * ch) * E;
            return f32x4{q[0], q[E], q[2 * (size_t)E], q[3 * (size_t)E]};
          });
#pragma unroll
      for (int j = 0; j < 4; ++j) Zs[(4 * g + j) * ldz + et * 16 + i] = acc[j];
    }
  }
  __syncthreads();

  // row norms and f = Z / max(|Z|, 1e-12): 16 threads per row
  const int r = tid >> 4, sub = tid & 15;
  {
    float* zr = Zs + r * ldz;
    float s2 = 0.f;
    for (int e = sub; e < E; e += 16) s2 = fmaf(zr[e], zr[e], s2);
    const float nrm = fmaxf(sqrtf(sum16(s2)), 1e-12f);
    for (int e = sub; e < E; e += 16) zr[e] = zr[e] / nrm;
    if (sub == 0) rowv[r] = nrm;
  }
  __syncthreads();

  // L = scale * f W: wave w takes class tiles w, w + 4, ...
  for (int ct = w; ct < Cp / 16; ct += 4) {
    const int c = ct * 16 + i, col = c < C ? c : C - 1;
    const float* fp = Zs + i * ldz + 4 * g;
    const float* wp = W + (size_t)(4 * g) * C + col;
    const f32x4 acc = mfma_k_comp(
        E / 16, [&](int ch) { return *(const f32x4*)(fp + 16 * ch); },
        [&](int ch) {
          const float* q = wp + (size_t)(16 * ch) * C;
          return f32x4{q[0], q[C], q[2 * (size_t)C], q[3 * (size_t)C]};
        });
#pragma unroll
    for (int j = 0; j < 4; ++j) Ls[(4 * g + j) * ldl + c] = c < C ? scale * acc[j] : 0.f;
  }
  __syncthreads();

  // softmax (max subtracted), CE, first argmax, Gm and f . dF = sum_c Gm[c] L[c]
  {
    float* lr = Ls + r * ldl;
    const bool valid = r0 + r < n;
    const int64_t yl = valid ? y[r0 + r] : -1;
    const int yy = (yl >= 0 && yl < C) ? (int)yl : -1;
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int c = sub; c < C; c += 16) {
      const float v = lr[c];
      if (v > mx) { mx = v; am = c; }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float ov = __shfl_xor(mx, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (ov > mx || (ov == mx && oa < am)) { mx = ov; am = oa; }
    }
    const float ly = yy >= 0 ? lr[yy] : 0.f;
    float se = 0.f;
    for (int c = sub; c < C; c += 16) se += expf(lr[c] - mx);
    se = sum16(se);
    __syncthreads();   // every read of the logits row above precedes the Gm writes below
    const float fn = (float)n;
    float s = 0.f;
    for (int c = sub; c < C; c += 16) {
      const float v = lr[c];
      const float gm = valid ? (expf(v - mx) / se - (c == yy ? 1.f : 0.f)) / fn : 0.f;
      s = fmaf(gm, v, s);
      lr[c] = gm;
    }
    s = sum16(s);
    if (sub == 0) {
      rowv[16 + r] = s;
      rowv[32 + r] = valid ? (logf(se) + mx) - ly : 0.f;
      rowv[48 + r] = (valid && am == yy) ? 1.f : 0.f;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float ce = 0.f, ok = 0.f;
    for (int q = 0; q < 16; ++q) {
      ce += rowv[32 + q];
      ok += rowv[48 + q];
    }
    float* o = part + ((size_t)cfg * gridDim.x + blockIdx.x) * 2;
    o[0] = ce;
    o[1] = ok;
  }

  // dF = scale * Gm W^T and dZ = (dF - f (f . dF)) / nrm: wave w takes column tiles of E
  float* dZg = dZ + (size_t)cfg * n * E;
  for (int et = w; et < E / 16; et += 4) {
    const float* gp = Ls + i * ldl + 4 * g;
    const float* wr = W + (size_t)(et * 16 + i) * C;   // W^T[c][e] = W[e][c]
    const f32x4 acc = mfma_k(
        Cp / 16, [&](int ch) { return *(const f32x4*)(gp + 16 * ch); },
        [&](int ch) {
          const int c = 16 * ch + 4 * g;   // classes past C - 1 meet Gm = 0: clamp the read
          return f32x4{wr[c < C ? c : C - 1], wr[c + 1 < C ? c + 1 : C - 1],
                       wr[c + 2 < C ? c + 2 : C - 1], wr[c + 3 < C ? c + 3 : C - 1]};
        });
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rl = 4 * g + j, e = et * 16 + i;
      if (r0 + rl < n)
        dZg[(size_t)(r0 + rl) * E + e] =
            (scale * acc[j] - Zs[rl * ldz + e] * rowv[16 + rl]) / rowv[rl];
    }
  }
}

struct AdamArgs {
  float lr_factor, lambda_div, bc1, bc2_sqrt, eps;
};

template <typename T>
__global__ __launch_bounds__(256) void prolip_adam_kernel(
    const T* __restrict__ x, const float* __restrict__ dZ, const float* __restrict__ P0,
    float* __restrict__ P, float* __restrict__ m, float* __restrict__ v,
    const float* __restrict__ lr, const float* __restrict__ lam, float* __restrict__ part, int n,
    int D, int E, AdamArgs a) {
  __shared__ float wsq[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, g = lane >> 4;
  const int cfg = blockIdx.z;
  const int dt = blockIdx.y * 2 + (w & 1), et = blockIdx.x * 2 + (w >> 1);
  float sq = 0.f;
  if (dt < D / 16 && et < E / 16) {
    const T* xp = x + dt * 16 + i;                                   // X^T[d][r] = X[r][d]
    const float* zp = dZ + (size_t)cfg * n * E + et * 16 + i;
    const f32x4 acc = mfma_k(
        (n + 15) / 16,
        [&](int ch) {
          f32x4 o;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int rr = 16 * ch + 4 * g + s;
            const float val = to_f<T>(xp[(size_t)(rr < n ? rr : n - 1) * D]);
            o[s] = rr < n ? val : 0.f;
          }
          return o;
        },
        [&](int ch) {
          f32x4 o;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int rr = 16 * ch + 4 * g + s;
            const float val = zp[(size_t)(rr < n ? rr : n - 1) * E];
            o[s] = rr < n ? val : 0.f;
          }
          return o;
        });
    // torch.optim.Adam (single-tensor form, no weight decay, no amsgrad)
    const float lam2 = 2.f * (lam[cfg] / a.lambda_div);
    const float step_size = (lr[cfg] * a.lr_factor) / a.bc1;
    const size_t base = (size_t)cfg * D * E;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t idx = (size_t)(dt * 16 + 4 * g + j) * E + et * 16 + i;
      const float p = P[base + idx], diff = p - P0[idx];
      sq = fmaf(diff, diff, sq);
      const float grad = fmaf(lam2, diff, acc[j]);
      const float m0 = m[base + idx], v0 = v[base + idx];
      const float m1 = m0 + (grad - m0) * 0.1f;                  // exp_avg.lerp_(grad, 1 - beta1)
      const float v1 = fmaf(0.001f, grad * grad, v0 * 0.999f);   // mul_(beta2).addcmul_(g, g, 1 - beta2)
      const float denom = sqrtf(v1) / a.bc2_sqrt + a.eps;
      m[base + idx] = m1;
      v[base + idx] = v1;
      P[base + idx] = p - step_size * (m1 / denom);
    }
  }
  sq = wave_sum(sq);
  if (lane == 0) wsq[w] = sq;
  __syncthreads();
  if (tid == 0)
    part[(size_t)cfg * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] =
        (wsq[0] + wsq[1]) + (wsq[2] + wsq[3]);
}

// history[cfg] = {sum of CE partials / n, sum of MSE partials, sum of correct partials}:
// lane l adds partials l, l + 64, ... in ascending order, then a fixed butterfly
__global__ __launch_bounds__(64) void prolip_fold_kernel(const float* __restrict__ gpart, int ntA,
                                                         const float* __restrict__ mpart, int ntB,
                                                         int n, float* __restrict__ hist) {
  const int cfg = blockIdx.x, lane = threadIdx.x;
  float ce = 0.f, ok = 0.f, ms = 0.f;
  for (int t = lane; t < ntA; t += 64) {
    ce += gpart[((size_t)cfg * ntA + t) * 2];
    ok += gpart[((size_t)cfg * ntA + t) * 2 + 1];
  }
  for (int t = lane; t < ntB; t += 64) ms += mpart[(size_t)cfg * ntB + t];
  ce = wave_sum(ce);
  ok = wave_sum(ok);
  ms = wave_sum(ms);
  if (lane == 0) {
    hist[cfg * 3 + 0] = ce / (float)n;
    hist[cfg * 3 + 1] = ms;
    hist[cfg * 3 + 2] = ok;
  }
}

bool prolip_shape_ok(int n, int D, int E, int G) {
  return n >= 1 && G >= 1 && G <= 65535 && D >= 16 && D <= 1280 && D % 16 == 0 && E >= 16 &&
         E <= 1024 && E % 16 == 0;
}

template <typename T>
hipError_t launch_grad(const void* x, const int64_t* labels, const float* W, const float* P,
                       float* dZ, float* part, int n, int D, int E, int C, int G, float scale,
                       hipStream_t s) {
  const int Cp = (C + 15) & ~15;
  const size_t lds = (size_t)(16 * (E + kLdsPad) + 16 * (Cp + kLdsPad) + 64) * sizeof(float);
  // at most 131,840 B (E = C = 1024) of the 160 KiB
  const hipError_t attr = lds_opt_in((const void*)prolip_grad_kernel<T>, lds);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(prolip_grad_kernel<T>, dim3((n + 15) / 16, G), dim3(256), lds, s,
                     (const T*)x, labels, P, W, dZ, part, n, D, E, C, scale);
  return hipGetLastError();
}

}  // namespace

int prolip_adam_tiles(int D, int E) { return ((D + 31) / 32) * ((E + 31) / 32); }

hipError_t prolip_grad(int x_dtype, const void* x, const int64_t* labels, const float* W,
                       const float* P, float* dZ, float* part, int n, int D, int E, int C, int G,
                       float scale, hipStream_t s) {
  if (!prolip_shape_ok(n, D, E, G) || C < 1 || C > 1024 || ((uintptr_t)x & 15) ||
      !in_dtype_ok(x_dtype))
    return hipErrorInvalidValue;
  return dispatch_in_dtype(x_dtype, [&](auto tag) {
    return launch_grad<typename decltype(tag)::type>(x, labels, W, P, dZ, part, n, D, E, C, G,
                                                     scale, s);
  });
}

hipError_t prolip_adam(int x_dtype, const void* x, const float* dZ, const float* P0, float* P,
                       float* m, float* v, const float* lr, const float* lam,
                       const float* grad_part, float* mse_part, float* history, int n, int D,
                       int E, int G, float lr_factor, float lambda_div, int step, float eps,
                       hipStream_t s) {
  if (!prolip_shape_ok(n, D, E, G) || step < 1 || !(lambda_div > 0.f) || !(eps >= 0.f) ||
      !in_dtype_ok(x_dtype))
    return hipErrorInvalidValue;
  // bias corrections in double, as torch's Python scalars (1 - beta ** step)
  const AdamArgs a = {lr_factor, lambda_div, (float)(1.0 - pow(0.9, (double)step)),
                      (float)sqrt(1.0 - pow(0.999, (double)step)), eps};
  const dim3 grid((E + 31) / 32, (D + 31) / 32, G);
  dispatch_in_dtype(x_dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL(prolip_adam_kernel<T>, grid, dim3(256), 0, s, (const T*)x, dZ, P0, P, m, v,
                       lr, lam, mse_part, n, D, E, a);
  });
  hipLaunchKernelGGL(prolip_fold_kernel, dim3(G), dim3(64), 0, s, grad_part, (n + 15) / 16,
                     mse_part, prolip_adam_tiles(D, E), n, history);
  return hipGetLastError();
}

}  // namespace miclip
