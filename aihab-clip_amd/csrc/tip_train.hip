// Tip-Adapter-F: training the cache keys on cached joint-space features, one AdamW step
// of G independent configurations (lr, beta, alpha) per call. The adapter is a bias-free
// Linear(E, Nk) initialised to the cache keys, so adapter(f) = f K^T and only K [Nk, E]
// trains. All arithmetic is fp32 on exactly widened inputs (F fp32 / fp16 / bf16); both
// products run on the f32-input MFMA (v_mfma_f32_16x16x4_f32), in mfma_f32.h's k order.
//
// For the b batch rows named by the row map (F_b, Z_b, y_b are rows of F, Z, labels):
//   * stage_rows (launch.h): the host row map, already checked against [0, n), travels
//     in launch arguments (256 indices per launch) into the scratch; no gathered copy of
//     F is formed and the caller's array is free on return.
//   * tipf_forward_kernel, grid (ceil(b / 16), ceil(Nk / 64), G), one 16 x 16 tile per
//     wave: A = F_b K_g^T, the chain of tip_affinity_kernel, then
//     phi = exp(-(beta_g - beta_g A)) unfused as tip_grid_kernel rounds it, written to
//     phi [G, b, Nk] in the scratch.
//   * tipf_loss_kernel, grid (ceil(b / 16), G), 16 threads per row: the class sums
//     S[r, c] = sum of phi[r, k] over the keys of class c in ascending k (tip_sort's
//     order / offsets, computed once per fit by tipf_prepare), logits = Z + alpha_g S,
//     softmax with the row maximum subtracted, gm = (softmax - onehot(y)) / b into
//     gm [G, b, C], and the tile's partials {sum of CE, rows whose first argmax (NaN above
//     every number) is the label}.
//   * tipf_adamw_kernel, grid (ceil(Nk / 64), ceil(E / 64), G), a 64 x 64 tile of dK_g per
//     workgroup, wave w its 16 keys 16 w .. 16 w + 15 against four 16-wide column tiles:
//     dK = dA^T F_b with dA[r, k] = ((alpha_g beta_g) phi[r, k]) gm[r, cls(k)] formed in
//     the operand load (one float per lane: the transposed operand is only addressing),
//     then torch.optim.AdamW's step of K_g, m_g, v_g in the epilogue. dK reaches memory
//     only when the caller passes grad_out. Workgroup (0, 0, g) also folds the loss
//     partials of g in ascending tile order into history {mean CE, correct}.
//   * tipf_keep_kernel, grid (ceil(Nk E / 1024), G): the recipe's `if acc > best_acc` on
//     the device. The best count before epoch e is recomputed from the counts of epochs
//     0 .. e - 1 (and 0), which this kernel never writes, so every workgroup takes the same
//     decision without a fence; when counts[e, g] is strictly greater the keys of g are
//     copied to best_keys and workgroup 0 of g records the count and the epoch.
//
// Determinism: every float sum has an order fixed by the sizes and the labels (ascending
// k chains inside one wave, ascending key index inside a class, fixed butterflies,
// ascending tiles); there are no float atomics. A configuration reads only its own
// slices and the shared F, Z, labels, so its result depends neither on G nor on its index.
// Tail rows are clamped on the load and masked to zero operands; tail keys are clamped on
// the load and masked on the store. Nothing allocates or synchronises.
#include <math.h>

#include "kernels.h"
#include "launch.h"
#include "mfma_f32.h"

namespace miclip {

namespace {

// torch.topk's order: NaN above every number, the lower index first among equals
MICLIP_DEV bool ranks_above(float v, int c, float best, int arg) {
  if (v != v) return best == best || c < arg;
  if (best != best) return false;
  return v > best || (v == best && c < arg);
}

template <typename T>
__global__ __launch_bounds__(256) void tipf_forward_kernel(
    const T* __restrict__ F, const int32_t* __restrict__ rows, const float* __restrict__ K,
    const float* __restrict__ betas, float* __restrict__ phi, int b, int Nk, int E) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int cfg = blockIdx.z;
  const int q0 = blockIdx.x * 16, k0 = blockIdx.y * 64 + w * 16;
  if (k0 >= Nk) return;   // wave-uniform; the kernel has no barrier
  const int row = rows[q0 + i < b ? q0 + i : b - 1], col = k0 + i < Nk ? k0 + i : Nk - 1;
  const T* fp = F + (size_t)row * E + 4 * g;
  const float* kp = K + ((size_t)cfg * Nk + col) * E + 4 * g;   // K^T[e][col] = K[col][e]
  const f32x4 acc = mfma_k(
      E / 16, [&](int ch) { return load4<T>(fp + 16 * ch); },
      [&](int ch) { return load4<float>(kp + 16 * ch); });
  const float beta = betas[cfg];
  float* out = phi + (size_t)cfg * b * Nk;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int rr = q0 + 4 * g + j, cc = k0 + i;
    // unfused, as tip_grid_kernel evaluates -(beta - beta * affinity)
    if (rr < b && cc < Nk)
      out[(size_t)rr * Nk + cc] = expf(-__fsub_rn(beta, __fmul_rn(beta, acc[j])));
  }
}

__global__ __launch_bounds__(256) void tipf_loss_kernel(
    const float* __restrict__ phi, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ order, const int32_t* __restrict__ offsets,
    const float* __restrict__ Z, const int32_t* __restrict__ labels,
    const float* __restrict__ alphas, float* __restrict__ gm, float* __restrict__ part, int b,
    int Nk, int C) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ldl = C + kLdsPad;
  float* Ls = (float*)smem;       // [16][ldl] logits
  float* rowv = Ls + 16 * ldl;    // [2][16]   CE, correct
  const int tid = threadIdx.x, r = tid >> 4, sub = tid & 15;
  const int r0 = blockIdx.x * 16, cfg = blockIdx.y;
  const bool valid = r0 + r < b;
  const int rb = valid ? r0 + r : b - 1;   // row of the batch, clamped
  const int src = rows[rb];                // row of F / Z / labels
  const float alpha = alphas[cfg];
  const float* prow = phi + ((size_t)cfg * b + rb) * Nk;
  const float* zrow = Z + (size_t)src * C;
  float* lr = Ls + r * ldl;

  const int total = offsets[C] < Nk ? offsets[C] : Nk;
  for (int c = sub; c < C; c += 16) {
    int lo = offsets[c], hi = offsets[c + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > total ? total : hi;
    float s = 0.f;   // a class with no key stays 0
    for (int p = lo; p < hi; ++p) s += prow[order[p]];
    lr[c] = __fadd_rn(zrow[c], __fmul_rn(s, alpha));
  }
  // a thread reads back only the logits it wrote itself: no barrier needed here
  const int32_t yl = labels[src];
  const int yy = (yl >= 0 && yl < C) ? (int)yl : -1;
  float mx = -INFINITY;
  int am = 0x7fffffff;
  for (int c = sub; c < C; c += 16) {
    const float v = lr[c];
    if (am == 0x7fffffff || ranks_above(v, c, mx, am)) { mx = v; am = c; }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (oa != 0x7fffffff && (am == 0x7fffffff || ranks_above(ov, oa, mx, am))) { mx = ov; am = oa; }
  }
  float se = 0.f;
  for (int c = sub; c < C; c += 16) se += expf(lr[c] - mx);
  se = sum16(se);
  __syncthreads();   // lr[yy] below was written by another thread of the row
  // log-softmax as torch takes it, (l_y - max) - log(sum): no cancellation against the
  // size of the logits
  const float ly = yy >= 0 ? lr[yy] - mx : 0.f;
  const float fb = (float)b;
  float* grow = gm + ((size_t)cfg * b + rb) * C;
  if (valid)
    for (int c = sub; c < C; c += 16)
      grow[c] = (expf(lr[c] - mx) / se - (c == yy ? 1.f : 0.f)) / fb;
  if (sub == 0) {
    rowv[r] = valid ? logf(se) - ly : 0.f;
    rowv[16 + r] = (valid && am == yy) ? 1.f : 0.f;
  }
  __syncthreads();
  if (tid == 0) {
    float ce = 0.f, ok = 0.f;
    for (int q = 0; q < 16; ++q) {
      ce += rowv[q];
      ok += rowv[16 + q];
    }
    float* o = part + ((size_t)cfg * gridDim.x + blockIdx.x) * 2;
    o[0] = ce;
    o[1] = ok;
  }
}

struct AdamWArgs {
  float lr_factor, weight_decay, bc1, bc2_sqrt, eps;
};

template <typename T>
__global__ __launch_bounds__(256) void tipf_adamw_kernel(
    const T* __restrict__ F, const int32_t* __restrict__ rows, const float* __restrict__ phi,
    const float* __restrict__ gm, const int32_t* __restrict__ key_labels,
    const float* __restrict__ lrs, const float* __restrict__ betas,
    const float* __restrict__ alphas, float* __restrict__ K, float* __restrict__ m,
    float* __restrict__ v, float* __restrict__ grad_out, const float* __restrict__ part,
    float* __restrict__ history, int b, int Nk, int E, int C, AdamWArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, g = lane >> 4;
  const int cfg = blockIdx.z;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    const int nt = (b + 15) / 16;
    float ce = 0.f, ok = 0.f;
    for (int t = 0; t < nt; ++t) {   // ascending tile order
      ce += part[((size_t)cfg * nt + t) * 2];
      ok += part[((size_t)cfg * nt + t) * 2 + 1];
    }
    history[cfg * 2 + 0] = ce / (float)b;
    history[cfg * 2 + 1] = ok;
  }
  const int k0 = blockIdx.x * 64 + w * 16, e0 = blockIdx.y * 64;
  if (k0 >= Nk) return;   // wave-uniform; the kernel has no barrier
  const int net = (E - e0) / 16 < 4 ? (E - e0) / 16 : 4;   // live 16-wide column tiles
  const int key = k0 + i < Nk ? k0 + i : Nk - 1;
  const int32_t kl = key_labels[key];
  const bool owned = kl >= 0 && kl < C;   // a key outside [0, C) owns no class: no force
  const int cls = owned ? (int)kl : 0;
  const float ab = alphas[cfg] * betas[cfg];
  const float* pp = phi + (size_t)cfg * b * Nk + key;         // dA^T[k][r] = dA[r][k]
  const float* gp = gm + (size_t)cfg * b * C + cls;
  const T* fp = F + e0 + i;

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nch = (b + 15) / 16;
  for (int ch = 0; ch < nch; ++ch) {
    f32x4 da, fv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int rr = 16 * ch + 4 * g + s;
      const bool live = rr < b;
      const int rc = live ? rr : b - 1;
      const float d = (ab * pp[(size_t)rc * Nk]) * gp[(size_t)rc * C];
      da[s] = (live && owned) ? d : 0.f;
      const T* fr = fp + (size_t)rows[rc] * E;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float f = to_f<T>(fr[t < net ? 16 * t : 0]);
        fv[t][s] = live ? f : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = mfma4(da, fv[t], acc[t]);
  }

  // torch.optim.AdamW (single-tensor form, no amsgrad): decay, moments, step
  const float lr_t = lrs[cfg] * a.lr_factor;
  const float keep = 1.f - lr_t * a.weight_decay;
  const float step_size = lr_t / a.bc1;
  const size_t base = (size_t)cfg * Nk * E;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= net) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = k0 + 4 * g + j;
      if (kk >= Nk) continue;
      const size_t idx = base + (size_t)kk * E + e0 + 16 * t + i;
      const float grad = acc[t][j];
      if (grad_out) grad_out[idx] = grad;
      const float p = K[idx] * keep;
      const float m0 = m[idx], v0 = v[idx];
      const float m1 = m0 + (grad - m0) * 0.1f;                  // exp_avg.lerp_(grad, 1 - beta1)
      const float v1 = fmaf(0.001f, grad * grad, v0 * 0.999f);   // mul_(beta2).addcmul_(g, g, 1 - beta2)
      const float denom = sqrtf(v1) / a.bc2_sqrt + a.eps;
      m[idx] = m1;
      v[idx] = v1;
      K[idx] = p - step_size * (m1 / denom);
    }
  }
}

__global__ __launch_bounds__(256) void tipf_keep_kernel(
    const int32_t* __restrict__ counts, int epoch, int G, const float* __restrict__ keys,
    float* __restrict__ best_keys, int32_t* __restrict__ best_count,
    int32_t* __restrict__ best_epoch, size_t per) {
  const int cfg = blockIdx.y;
  int best = 0;   // the recipe's best_acc = 0
  for (int e = 0; e < epoch; ++e) {
    const int c = counts[(size_t)e * G + cfg];
    best = c > best ? c : best;
  }
  const int now = counts[(size_t)epoch * G + cfg];
  if (now <= best) return;   // uniform over the workgroups of cfg
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    best_count[cfg] = now;
    best_epoch[cfg] = epoch;
  }
  const size_t i4 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;   // per % 16 == 0
  if (i4 < per)
    *(f32x4*)(best_keys + (size_t)cfg * per + i4) = *(const f32x4*)(keys + (size_t)cfg * per + i4);
}

struct TipfScratch {
  int32_t *order, *offsets, *rows;
  float *phi, *gm, *part;
};

// head: tip_sort's layout (order, offsets); then rows [b], phi [G, b, Nk], gm [G, b, C],
// part [G, ceil(b / 16), 2]
size_t tipf_layout(void* scratch, int b, int Nk, int C, int G, TipfScratch* out) {
  size_t at = 0;
  char* base = (char*)scratch;
  const auto take = [&](size_t bytes) {
    char* p = base + at;
    at += align256(bytes);
    return p;
  };
  TipfScratch t;
  t.order = (int32_t*)take((size_t)Nk * 4);
  t.offsets = (int32_t*)take((size_t)(C + 1) * 4);
  t.rows = (int32_t*)take((size_t)b * 4);
  t.phi = (float*)take((size_t)G * b * Nk * 4);
  t.gm = (float*)take((size_t)G * b * C * 4);
  t.part = (float*)take((size_t)G * ((b + 15) / 16) * 2 * 4);
  if (out) *out = t;
  return at;
}

template <typename T>
hipError_t tipf_launch(const void* F, const int32_t* labels, const float* Z,
                       const int32_t* key_labels, float* K, float* m, float* v, const float* lrs,
                       const float* betas, const float* alphas, int b, int Nk, int E, int C,
                       int G, const AdamWArgs& a, float* history, float* grad_out,
                       const TipfScratch& t, hipStream_t s) {
  hipLaunchKernelGGL(tipf_forward_kernel<T>, dim3((b + 15) / 16, (Nk + 63) / 64, G), dim3(256), 0,
                     s, (const T*)F, t.rows, K, betas, t.phi, b, Nk, E);
  const size_t lds = (size_t)(16 * (C + kLdsPad) + 32) * sizeof(float);
  // 65,920 B at C = 1024
  const hipError_t attr = lds_opt_in((const void*)tipf_loss_kernel, lds);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(tipf_loss_kernel, dim3((b + 15) / 16, G), dim3(256), lds, s, t.phi, t.rows,
                     t.order, t.offsets, Z, labels, alphas, t.gm, t.part, b, Nk, C);
  hipLaunchKernelGGL(tipf_adamw_kernel<T>, dim3((Nk + 63) / 64, (E + 63) / 64, G), dim3(256), 0, s,
                     (const T*)F, t.rows, t.phi, t.gm, key_labels, lrs, betas, alphas, K, m, v,
                     grad_out, t.part, history, b, Nk, E, C, a);
  return hipGetLastError();
}

}  // namespace

const char* tipf_bad_arg(int64_t n, int64_t b, int64_t Nk, int64_t E, int64_t C, int64_t G) {
  if (n < 1 || n > ((int64_t)1 << 24)) return "n must be in 1..2^24";
  if (b < 1 || b > 4096) return "b must be in 1..4096";
  if (const char* bad = tip_bad_arg(kTipNk | kTipE | kTipC, 0, Nk, E, C, 0, 0)) return bad;
  if (G < 1 || G > 64) return "G must be in 1..64";
  return nullptr;
}

size_t tipf_scratch_bytes(int b, int Nk, int E, int C, int G) {
  if (tipf_bad_arg(1, b, Nk, E, C, G)) return 0;
  return tipf_layout(nullptr, b, Nk, C, G, nullptr);
}

hipError_t tipf_prepare(const int32_t* key_labels, int Nk, int C, void* scratch, hipStream_t s) {
  if (tip_bad_arg(kTipNk | kTipC, 0, Nk, 0, C, 0, 0) || !scratch || ((uintptr_t)scratch & 255))
    return hipErrorInvalidValue;
  // the head of the scratch is tip_sort's own layout: order at 0, offsets behind it
  if (tip_sort_offsets_at(Nk) != align256((size_t)Nk * 4)) return hipErrorInvalidValue;
  return tip_sort_keys(key_labels, Nk, C, scratch, s);
}

hipError_t tipf_step(int f_dtype, const void* F, int n, const int64_t* rows_host, int b,
                     const int32_t* labels, const float* Z, const int32_t* key_labels, float* K,
                     float* m, float* v, const float* lrs, const float* betas,
                     const float* alphas, int Nk, int E, int C, int G, float lr_factor,
                     float weight_decay, float eps, int step, float* history, float* grad_out,
                     void* scratch, hipStream_t s) {
  if (!in_dtype_ok(f_dtype) || tipf_bad_arg(n, b, Nk, E, C, G) || !rows_host || !scratch ||
      ((uintptr_t)scratch & 255) || ((uintptr_t)F & 15) || ((uintptr_t)K & 15) || step < 1 ||
      !isfinite(lr_factor) || !(weight_decay >= 0.f) || !isfinite(weight_decay) ||
      !(eps >= 0.f) || !isfinite(eps))
    return hipErrorInvalidValue;
  for (int r = 0; r < b; ++r)   // before any launch: no kernel sees a row outside [0, n)
    if (rows_host[r] < 0 || rows_host[r] >= n) return hipErrorInvalidValue;
  TipfScratch t;
  tipf_layout(scratch, b, Nk, C, G, &t);
  stage_rows(t.rows, b, s, [&](int r) { return (int32_t)rows_host[r]; });   // n <= 2^24
  // bias corrections in double, as torch's Python scalars (1 - beta ** step)
  const AdamWArgs a = {lr_factor, weight_decay, (float)(1.0 - pow(0.9, (double)step)),
                       (float)sqrt(1.0 - pow(0.999, (double)step)), eps};
  return dispatch_in_dtype(f_dtype, [&](auto tag) {
    return tipf_launch<typename decltype(tag)::type>(F, labels, Z, key_labels, K, m, v, lrs, betas,
                                                     alphas, b, Nk, E, C, G, a, history, grad_out,
                                                     t, s);
  });
}

hipError_t tipf_keep_best(const int32_t* counts, int epoch, const float* keys, float* best_keys,
                          int32_t* best_count, int32_t* best_epoch, int Nk, int E, int G,
                          hipStream_t s) {
  if (tip_bad_arg(kTipNk | kTipE, 0, Nk, E, 0, 0, 0) || G < 1 || G > 64 || epoch < 0 ||
      ((uintptr_t)keys & 15) || ((uintptr_t)best_keys & 15))
    return hipErrorInvalidValue;
  const size_t per = (size_t)Nk * E;
  hipLaunchKernelGGL(tipf_keep_kernel, dim3((unsigned)((per + 1023) / 1024), G), dim3(256), 0, s,
                     counts, epoch, G, keys, best_keys, best_count, best_epoch, per);
  return hipGetLastError();
}

}  // namespace miclip
