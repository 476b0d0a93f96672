// Tip-Adapter's training-free cache classifier and its (beta, alpha) search
// (methods/utils.py:23-62 build_cache_model, :64-94 search_hp_tip) on the device.
// All arithmetic is fp32 on exactly widened inputs (fp16 / bf16 / fp32 in the load);
// the three matrix products run on the f32-input MFMA (v_mfma_f32_16x16x4_f32: exact
// fp32 products, one fp32 fmaf chain per output element in mfma_f32.h's fixed order of k).
//
//   * tip_keys_kernel, grid ceil(Nk / 16), one 16-row tile of keys per workgroup:
//     for every view v in ascending order Z = x_v proj (MFMA), f = Z / max(|Z|, 1e-12)
//     (:38-39), added into the key rows; then keys = (sum / A) / |sum / A| (:47-48, a
//     plain division: an all-zero row gives 0 / 0 = NaN as in the reference). The
//     running sum lives in the output rows: every element is read and written by the
//     same thread from the first view to the last, so no fence is involved.
//   * tip_affinity_kernel, grid (ceil(Nq / 16), ceil(Nk / 64)), one 16 x 16 tile per
//     wave: Aff = scale * F keys^T (:79; with keys = clip_weights^T and scale 100 the
//     same kernel gives the CLIP logits of :82). Row and column tails are clamped on
//     the load and masked on the store.
//   * tip_sort_kernel, one workgroup: a stable counting sort of the key labels ->
//     order [Nk] (key indices grouped by class, ascending inside a class) and offsets
//     [C + 1]. A label outside [0, C) is left out (it owns no class; the host callers
//     refuse such labels), so no index derived from a label is ever out of range.
//   * tip_grid_kernel<false>, grid (ceil(Nq / 8), ceil(nb / bpb)): per query row and
//     beta the class sums s_c(beta) = sum_{k in class c} exp(-(beta - beta Aff_k)) (:81,
//     the product with the one-hot values written as a segmented sum), one exp per
//     (key, beta), summed in ascending key order inside the class; then for every
//     alpha the first argmax of Z_c + alpha s_c (:83, cls_acc :16-21) against the
//     label. The class sums stay in LDS, the per-(beta, alpha) counts of the
//     workgroup's rows in registers, and one integer atomic per pair and workgroup
//     adds them to correct [nb, na] (integer sums: any order gives the same value).
//   * tip_grid_kernel<true>: the same class sums for one (beta, alpha), written out as
//     the logits Z + alpha s [Nq, C]: bit-identical to what the grid compared.
//
// Determinism: every float sum has a shape fixed by the sizes and the labels alone
// (one fixed k order in one wave, ascending key index inside a class, fixed butterflies);
// there are no float atomics. Nothing allocates or synchronises.
#include <math.h>

#include "kernels.h"
#include "launch.h"
#include "mfma_f32.h"

namespace miclip {

namespace {

constexpr int kTipTile = 4096;  // sorted affinities staged per pass of tip_grid_kernel
constexpr int kTipRows = 8;     // query rows per workgroup of tip_grid_kernel
constexpr int kTipItems = 1024; // (class, beta) and (beta, alpha) items per workgroup
constexpr int kTipBetas = 512;  // betas per workgroup

template <typename T>
__global__ __launch_bounds__(256) void tip_keys_kernel(
    const void* const* __restrict__ views, const float* __restrict__ proj, float* keys, int Nk,
    int Wv, int E, int A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ldz = E + kLdsPad;
  float* Zs = (float*)smem;   // [16][ldz]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, g = lane >> 4;
  const int r0 = blockIdx.x * 16;
  const int row = r0 + i < Nk ? r0 + i : Nk - 1;
  // 16 threads per row for the norms; thread (r, sub) owns elements sub, sub + 16, ...
  // of key row r0 + r through every view and the final division
  const int r = tid >> 4, sub = tid & 15;
  const bool live = r0 + r < Nk;
  float* kr = keys + (size_t)(live ? r0 + r : Nk - 1) * E;
  const float* zr = Zs + r * ldz;

  for (int v = 0; v < A; ++v) {
    const T* xp = (const T*)views[v] + (size_t)row * Wv + 4 * g;
    for (int et = w; et < E / 16; et += 4) {
      const float* pp = proj + (size_t)(4 * g) * E + et * 16 + i;
      const f32x4 acc = mfma_k(
          Wv / 16, [&](int ch) { return load4<T>(xp + 16 * ch); },
          [&](int ch) {
            const float* q = pp + (size_t)(16 * ch) * E;
            return f32x4{q[0], q[E], q[2 * (size_t)E], q[3 * (size_t)E]};
          });
#pragma unroll
      for (int j = 0; j < 4; ++j) Zs[(4 * g + j) * ldz + et * 16 + i] = acc[j];
    }
    __syncthreads();
    float s2 = 0.f;
    for (int e = sub; e < E; e += 16) s2 = fmaf(zr[e], zr[e], s2);
    const float nrm = fmaxf(sqrtf(sum16(s2)), 1e-12f);
    if (live)
      for (int e = sub; e < E; e += 16) {
        const float f = zr[e] / nrm;
        kr[e] = v == 0 ? f : kr[e] + f;
      }
    __syncthreads();   // the next view overwrites Zs
  }

  const float fa = (float)A;
  float s2 = 0.f;
  for (int e = sub; e < E; e += 16) {
    const float m = live ? kr[e] / fa : 0.f;   // rows past Nk read nothing
    s2 = fmaf(m, m, s2);
  }
  const float nrm = sqrtf(sum16(s2));
  if (live)
    for (int e = sub; e < E; e += 16) kr[e] = (kr[e] / fa) / nrm;
}

template <typename T>
__global__ __launch_bounds__(256) void tip_affinity_kernel(
    const T* __restrict__ F, const float* __restrict__ keys, float* __restrict__ aff, int Nq,
    int Nk, int E, float scale) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, k0 = blockIdx.y * 64 + w * 16;
  if (k0 >= Nk) return;   // wave-uniform; the kernel has no barrier
  const int row = q0 + i < Nq ? q0 + i : Nq - 1, col = k0 + i < Nk ? k0 + i : Nk - 1;
  const T* fp = F + (size_t)row * E + 4 * g;
  const float* kp = keys + (size_t)col * E + 4 * g;   // keys^T[k][col] = keys[col][k]
  const f32x4 acc = mfma_k(
      E / 16, [&](int ch) { return load4<T>(fp + 16 * ch); },
      [&](int ch) { return load4<float>(kp + 16 * ch); });
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int rr = q0 + 4 * g + j, cc = k0 + i;
    if (rr < Nq && cc < Nk) aff[(size_t)rr * Nk + cc] = scale * acc[j];
  }
}

// Stable counting sort of the key labels, one workgroup of 1024 threads. Thread t
// owns (class c = t / S, segment sg = t % S) with S = 1024 / C segments of L =
// ceil(Nk / S) keys; the exclusive prefix over (c, sg) in that order is the position
// of the thread's first key, so keys of one class keep their ascending order.
__global__ __launch_bounds__(1024) void tip_sort_kernel(const int32_t* __restrict__ labels,
                                                        int Nk, int C,
                                                        int32_t* __restrict__ order,
                                                        int32_t* __restrict__ offsets) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* cnt = (int32_t*)smem;                     // [1024]
  unsigned short* lab = (unsigned short*)(cnt + 1024);   // [Nk], 0xffff = no class
  const int t = threadIdx.x;
  for (int k = t; k < Nk; k += 1024) {
    const int32_t l = labels[k];
    lab[k] = (l >= 0 && l < C) ? (unsigned short)l : (unsigned short)0xffff;
  }
  __syncthreads();
  const int S = 1024 / C, L = (Nk + S - 1) / S;
  const int c = t / S, sg = t - c * S;
  const bool live = c < C;
  const int lo = sg * L < Nk ? sg * L : Nk, hi = lo + L < Nk ? lo + L : Nk;
  int n = 0;
  if (live)
    for (int k = lo; k < hi; ++k) n += lab[k] == c;
  cnt[t] = live ? n : 0;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int q = 0; q < C * S; ++q) {
      if (q % S == 0) offsets[q / S] = run;
      const int m = cnt[q];
      cnt[q] = run;
      run += m;
    }
    offsets[C] = run;
  }
  __syncthreads();
  if (live) {
    int pos = cnt[t];   // <= Nk - n: the counts sum to at most Nk
    for (int k = lo; k < hi; ++k)
      if (lab[k] == c) order[pos++] = k;
  }
}

// kLogits false: correct [nb, na] += the workgroup's rows with the first argmax of
// Z + alpha s(beta) equal to the label. kLogits true (nb = na = bpb = 1): out [Nq, C] =
// Z + alpha1 s(beta1). Item (c, j) of the class sums and item (j, ia) of the argmax
// belong to thread item % 256; C * bpb, bpb * na <= kTipItems, bpb <= kTipBetas.
template <bool kLogits>
__global__ __launch_bounds__(256) void tip_grid_kernel(
    const float* __restrict__ aff, const int32_t* __restrict__ order,
    const int32_t* __restrict__ offsets, const float* __restrict__ Z,
    const int32_t* __restrict__ qlabels, const float* __restrict__ betas,
    const float* __restrict__ alphas, int32_t* correct, float* __restrict__ out, int Nq, int Nk,
    int C, int nb, int na, int bpb, float beta1, float alpha1) {
  __shared__ float sa[kTipTile];
  __shared__ float S[kTipItems];
  __shared__ float zrow[1024];
  __shared__ int32_t off[1025];
  __shared__ float sbeta[kTipBetas];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.y * bpb;
  const int nbl = nb - j0 < bpb ? nb - j0 : bpb;
  for (int c = tid; c <= C; c += 256) off[c] = offsets[c];
  for (int j = tid; j < nbl; j += 256) sbeta[j] = kLogits ? beta1 : betas[j0 + j];
  __syncthreads();
  const int total = off[C] < Nk ? off[C] : Nk;
  const int nitem = C * nbl, npair = nbl * na;
  int cnt[4] = {0, 0, 0, 0};

  for (int rr = 0; rr < kTipRows; ++rr) {
    const int q = blockIdx.x * kTipRows + rr;
    if (q >= Nq) break;   // uniform over the workgroup
    const float* arow = aff + (size_t)q * Nk;
    for (int it = tid; it < nitem; it += 256) S[it] = 0.f;   // a class with no key stays 0
    for (int c = tid; c < C; c += 256) zrow[c] = Z[(size_t)q * C + c];
    for (int t0 = 0; t0 < total; t0 += kTipTile) {
      const int m = total - t0 < kTipTile ? total - t0 : kTipTile;
      __syncthreads();   // the previous tile's readers are done
      for (int p = tid; p < m; p += 256) sa[p] = arow[order[t0 + p]];
      __syncthreads();
      for (int it = tid; it < nitem; it += 256) {
        const int c = it / nbl, j = it - c * nbl;
        const int lo = (off[c] > t0 ? off[c] : t0) - t0;
        const int hi = (off[c + 1] < t0 + m ? off[c + 1] : t0 + m) - t0;
        if (lo < hi) {
          const float b = sbeta[j];
          float acc = S[it];
          // unfused, as torch evaluates -(beta - beta * affinity): both instantiations
          // of this kernel then round the exponent alike whatever the compiler contracts
          for (int p = lo; p < hi; ++p) acc += expf(-__fsub_rn(b, __fmul_rn(b, sa[p])));
          S[it] = acc;
        }
      }
    }
    __syncthreads();
    if constexpr (kLogits) {
      for (int c = tid; c < C; c += 256)
        out[(size_t)q * C + c] = __fadd_rn(zrow[c], __fmul_rn(S[c], alpha1));
    } else {
      const int lab = qlabels[q];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int it = tid + 256 * u;
        if (it < npair) {
          const int j = it / na, ia = it - j * na;
          const float al = alphas[ia];
          // torch.topk's order (cls_acc): NaN above every number, the lower index first
          float best = -INFINITY;
          int arg = 0;
          for (int c = 0; c < C; ++c) {
            const float v = __fadd_rn(zrow[c], __fmul_rn(S[c * nbl + j], al));
            if (v > best || (v != v && best == best)) {
              best = v;
              arg = c;
            }
          }
          cnt[u] += arg == lab;
        }
      }
    }
    __syncthreads();   // the next row re-initialises S and zrow
  }
  if constexpr (!kLogits) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = tid + 256 * u;
      if (it < npair && cnt[u] > 0) {
        const int j = it / na, ia = it - j * na;
        atomicAdd(&correct[(size_t)(j0 + j) * na + ia], cnt[u]);
      }
    }
  }
}

size_t tip_order_bytes(int Nk) { return align256((size_t)Nk * 4); }

hipError_t tip_sort(const int32_t* key_labels, int Nk, int C, void* scratch, hipStream_t s) {
  const size_t lds = 1024 * sizeof(int32_t) + (((size_t)Nk * 2 + 15) & ~(size_t)15);
  // at most 135,168 B (Nk = 65536) of the 160 KiB
  const hipError_t attr = lds_opt_in((const void*)tip_sort_kernel, lds);
  if (attr != hipSuccess) return attr;
  int32_t* order = (int32_t*)scratch;
  int32_t* offsets = (int32_t*)((char*)scratch + tip_order_bytes(Nk));
  hipLaunchKernelGGL(tip_sort_kernel, dim3(1), dim3(1024), lds, s, key_labels, Nk, C, order,
                     offsets);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_keys(const void* const* views, const float* proj, float* keys, int Nk, int Wv,
                       int E, int A, hipStream_t s) {
  const size_t lds = (size_t)16 * (E + kLdsPad) * sizeof(float);
  // 65,792 B at E = 1024
  const hipError_t attr = lds_opt_in((const void*)tip_keys_kernel<T>, lds);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(tip_keys_kernel<T>, dim3((Nk + 15) / 16), dim3(256), lds, s, views, proj,
                     keys, Nk, Wv, E, A);
  return hipGetLastError();
}

}  // namespace

const char* tip_bad_arg(unsigned which, int64_t Nq, int64_t Nk, int64_t E, int64_t C, int64_t nb,
                        int64_t na) {
  if ((which & kTipNq) && (Nq < 1 || Nq > ((int64_t)1 << 24))) return "Nq must be in 1..2^24";
  if ((which & kTipNk) && (Nk < 1 || Nk > 65536)) return "Nk must be in 1..65536";
  if ((which & kTipE) && (E < 16 || E > 1024 || E % 16))
    return "E must be a multiple of 16 in 16..1024";
  if ((which & kTipC) && (C < 1 || C > 1024)) return "C must be in 1..1024";
  if ((which & kTipNb) && (nb < 1 || nb > 1024)) return "nb must be in 1..1024";
  if ((which & kTipNa) && (na < 1 || na > 1024)) return "na must be in 1..1024";
  if ((which & kTipNb) && (which & kTipNa) && nb * na > 65536)
    return "nb * na must be at most 65536";
  return nullptr;
}

size_t tip_sort_offsets_at(int Nk) { return tip_order_bytes(Nk); }

hipError_t tip_sort_keys(const int32_t* key_labels, int Nk, int C, void* scratch, hipStream_t s) {
  if (tip_bad_arg(kTipNk | kTipC, 0, Nk, 0, C, 0, 0)) return hipErrorInvalidValue;
  return tip_sort(key_labels, Nk, C, scratch, s);
}

size_t tip_scratch_bytes(int Nq, int Nk, int E, int C, int nb, int na) {
  if (tip_bad_arg(kTipAll, Nq, Nk, E, C, nb, na)) return 0;
  return tip_order_bytes(Nk) + align256((size_t)(C + 1) * 4);
}

hipError_t tip_keys(int x_dtype, const void* const* views, int A, const float* proj, float* keys,
                    int Nk, int Wv, int E, hipStream_t s) {
  if (!in_dtype_ok(x_dtype) || tip_bad_arg(kTipNk | kTipE, 0, Nk, E, 0, 0, 0) || A < 1 || A > 1024 ||
      Wv < 16 || Wv > 65536 || Wv % 16)
    return hipErrorInvalidValue;
  return dispatch_in_dtype(x_dtype, [&](auto tag) {
    return launch_keys<typename decltype(tag)::type>(views, proj, keys, Nk, Wv, E, A, s);
  });
}

hipError_t tip_affinity(int f_dtype, const void* F, const float* keys, float* aff, int Nq, int Nk,
                        int E, float scale, hipStream_t s) {
  if (!in_dtype_ok(f_dtype) || tip_bad_arg(kTipNq | kTipNk | kTipE, Nq, Nk, E, 0, 0, 0)) return hipErrorInvalidValue;
  const dim3 grid((Nq + 15) / 16, (Nk + 63) / 64);
  dispatch_in_dtype(f_dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL(tip_affinity_kernel<T>, grid, dim3(256), 0, s, (const T*)F, keys, aff, Nq,
                       Nk, E, scale);
  });
  return hipGetLastError();
}

hipError_t tip_grid(const float* aff, const int32_t* key_labels, const float* Z,
                    const int32_t* labels, const float* betas, const float* alphas,
                    int32_t* correct, int Nq, int Nk, int C, int nb, int na, void* scratch,
                    hipStream_t s) {
  if (tip_bad_arg(kTipAll & ~kTipE, Nq, Nk, 0, C, nb, na)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(correct, 0, (size_t)nb * na * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  e = tip_sort(key_labels, Nk, C, scratch, s);
  if (e != hipSuccess) return e;
  // betas per workgroup: about 512 (class, beta) items, at most kTipItems (beta, alpha) pairs
  int bpb = 512 / C < kTipItems / na ? 512 / C : kTipItems / na;
  bpb = bpb < 1 ? 1 : (bpb > nb ? nb : bpb);
  const int32_t* order = (const int32_t*)scratch;
  const int32_t* offsets = (const int32_t*)((const char*)scratch + tip_order_bytes(Nk));
  hipLaunchKernelGGL(tip_grid_kernel<false>, dim3((Nq + kTipRows - 1) / kTipRows,
                                                  (nb + bpb - 1) / bpb),
                     dim3(256), 0, s, aff, order, offsets, Z, labels, betas, alphas, correct,
                     (float*)nullptr, Nq, Nk, C, nb, na, bpb, 0.f, 0.f);
  return hipGetLastError();
}

hipError_t tip_logits(const float* aff, const int32_t* key_labels, const float* Z, float beta,
                      float alpha, float* out, int Nq, int Nk, int C, void* scratch,
                      hipStream_t s) {
  if (tip_bad_arg(kTipNq | kTipNk | kTipC, Nq, Nk, 0, C, 0, 0)) return hipErrorInvalidValue;
  const hipError_t e = tip_sort(key_labels, Nk, C, scratch, s);
  if (e != hipSuccess) return e;
  const int32_t* order = (const int32_t*)scratch;
  const int32_t* offsets = (const int32_t*)((const char*)scratch + tip_order_bytes(Nk));
  hipLaunchKernelGGL(tip_grid_kernel<true>, dim3((Nq + kTipRows - 1) / kTipRows, 1), dim3(256), 0,
                     s, aff, order, offsets, Z, (const int32_t*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, (int32_t*)nullptr, out, Nq, Nk, C, 1, 1, 1, beta,
                     alpha);
  return hipGetLastError();
}

}  // namespace miclip
