// Validation metrics on the GPU (methods/PEFT_openclip.py:50-136 `_run_validation`,
// aihab_utils/evaluation.py:80-331): one launch per batch does all the per-row work
// of the reference's loop body, a second one-workgroup launch folds the batch loss.
//
//   * eval_rows_kernel, grid ceil(B / 16), 256 threads, one 16-row tile per workgroup:
//       phase 0  (L2 roll-up with aggregated logits only) a CSR of the L3 -> L2 map in
//                LDS: per-group counts by LDS integer atomics, a one-wave exclusive
//                scan, and each class's rank inside its group (the number of lower L3
//                ids with the same group), so every group lists its L3 ids ascending.
//       phase 1  logits[16, C] = scale * (f . tw[:, c]) / max(|f|, 1e-12) into LDS, four
//                16-class tiles per round: head_logits_kernel's arithmetic (embed.hip) --
//                wave w takes k chunks [w nk / 4, (w + 1) nk / 4) of every tile, the
//                partial tiles are combined as (p0 + p1) + (p2 + p3) in wave order,
//                |f|^2 comes out of the first round's loop -- so a row's logits are
//                bitwise miclip_zero_shot's. The four tiles of a round are independent
//                MFMA chains in one wave and share the f loads; wave w combines tile w
//                of the round; two barriers per round. With MICLIP_EVAL_LOGITS_IN the
//                tile is loaded from `logits` instead.
//       phase 2  16 lanes per row (wave w owns rows 4w .. 4w + 3) over the LDS tile:
//                top-3 (value descending, lower index first: topk_rows_kernel's rule),
//                sum of exp(z - max), CE = (log(sum) + max) - z[y], the three softmax
//                probabilities; then the L2 logits of the row, group g on lane g % 16,
//                accumulated over the group's L3 ids in ascending order
//                (evaluation.py:125-140), and their top-3.
//       phase 3  integer accumulators: one vector atomic per row into the confusion
//                counts, the hit counts reduced in LDS first (one atomic per counter
//                and workgroup). Integer sums: exact, independent of arrival order.
//   * eval_finalise_kernel, one workgroup: the batch's row losses summed in a fixed
//     order (thread t adds rows t, t + 256, ... ascending, then a fixed tree), the
//     fp32 batch mean added to the float64 running sum (PEFT_openclip.py:93, 99).
//
// A row whose label is outside [0, C), or whose logits have no maximum (NaN), is
// skipped by every accumulator and counted in the `skipped` word; its loss is 0.
// Nothing is indexed by such a label or by a missing pick.
#include <math.h>

#include "kernels.h"
#include "launch.h"
#include "mfma_f32.h"

namespace miclip {

namespace {

constexpr int kPad = 4;        // LDS row stride = width + 4 floats
constexpr int kMaxC = 1024;

// the L3 -> L2 map by value in the kernel arguments (2 KiB): validated on the host,
// no device copy, no allocation
struct L2MapArg {
  uint16_t g[kMaxC];
};

struct EvalArgs {
  const void* f;
  const float* tw;
  const int64_t* labels;
  float* logits;
  float* row_loss;
  int32_t* row_pred;
  int32_t* row_top3;
  float* row_top3_prob;
  int32_t* l2_pred;
  int32_t* l2_top3;
  float* l2_logits;
  unsigned long long* state;
  int B, E, C, num_l2, l2_mode;
  float scale;
};

// embed.hip's mfma_chunks for four 16-class tiles at once, with the x element type as
// a parameter (widened exactly in the load). Per tile it is the same MFMA chain --
// ascending k chunks, x, y, z, w inside a chunk -- and the same fmaf chain for n2, so
// every tile's partial is bitwise mfma_chunks'; the x chunk is loaded once for the
// four tiles and the four chains are independent, which is what lets one wave per
// SIMD keep the f32 MFMA busy (40-cycle dependent latency, 32-cycle issue).
// wrow = W + 4g * ldw; col[t] = the lane's (clamped) class of tile t.
template <typename T, bool NORM>
MICLIP_DEV void mfma_chunks4(const T* __restrict__ xp, const float* __restrict__ wrow,
                             const int col[4], size_t ldw, int c0, int c1, f32x4 acc[4],
                             float& n2) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const auto loadw = [&](int ch, float bv[4][4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) bv[t][s2] = wrow[(size_t)(16 * ch + s2) * ldw + col[t]];
    }
  };
  const auto chunk = [&](const f32x4& a, const float bv[4][4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bv[t][0], acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bv[t][1], acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bv[t][2], acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bv[t][3], acc[t], 0, 0, 0);
    if (NORM) n2 = fmaf(a.w, a.w, fmaf(a.z, a.z, fmaf(a.y, a.y, fmaf(a.x, a.x, n2))));
  };
  int ch = c0;
  for (; ch + 2 <= c1; ch += 2) {   // the loads of two chunks are issued together
    const f32x4 a0 = load4<T>(xp + 16 * ch), a1 = load4<T>(xp + 16 * (ch + 1));
    float b0[4][4], b1[4][4];
    loadw(ch, b0);
    loadw(ch + 1, b1);
    chunk(a0, b0);
    chunk(a1, b1);
  }
  if (ch < c1) {
    const f32x4 a0 = load4<T>(xp + 16 * ch);
    float b0[4][4];
    loadw(ch, b0);
    chunk(a0, b0);
  }
}

// The top 3 of v[0 .. n) by the 16 lanes (sub = 0 .. 15) that share the row: value
// descending, the lower index first among equals (topk_rows_kernel's rule: pick j is
// the first entry strictly after pick j - 1 in that order). A pick that does not
// exist (n < 3, or NaN everywhere) is -1, and so is every later one.
MICLIP_DEV void top3_16(const float* v, int n, int sub, int idx[3], float val[3]) {
  float pv = INFINITY;
  int pi = -1;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float bv = -INFINITY;
    int bi = n;
    for (int c = sub; c < n; c += 16) {
      const float x = v[c];
      const bool after = x < pv || (x == pv && c > pi);
      if (after && (bi == n || x > bv)) { bv = x; bi = c; }   // ascending c: ties keep the lower
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi < n && (bi == n || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    idx[j] = bi < n ? bi : -1;
    val[j] = bv;
    pv = bi < n ? bv : -INFINITY;
    pi = bi;
  }
}

// torch.logaddexp's fp32 formula (aten LogAddExp.h)
MICLIP_DEV float logaddexp(float a, float b) {
  if (isinf(a) && a == b) return a;
  const float m = fmaxf(a, b);
  return m + log1pf(expf(-fabsf(a - b)));
}

// LDS carve (bytes), shared by the kernel and the launcher; every offset % 16 == 0
struct EvalLds {
  int red, nred, wgc, ls, l2s, off, cnt, mp, ord, total;
  __host__ __device__ EvalLds(int C, int L, bool agg) {
    const int Cp = (C + 15) & ~15, Lp = (L + 15) & ~15;
    int o = 0;
    red = o;  o += 4 * 4 * 64 * 16;          // f32x4 [4 tiles][4 waves][64] wave partials
    nred = o; o += 4 * 16 * 4;               // float [4][16] |f|^2 partials
    wgc = o;  o += 16 * 4;                   // int [8] workgroup counters
    ls = o;   o += 16 * (Cp + kPad) * 4;     // float [16][Cp + 4] L3 logits
    l2s = off = cnt = mp = ord = o;
    if (agg) {
      l2s = o; o += 16 * (Lp + kPad) * 4;    // float [16][Lp + 4] L2 logits
      off = o; o += (Lp + 16) * 4;           // int [L + 1] group offsets
      cnt = o; o += Lp * 4;                  // int [L] group sizes
      mp = o;  o += Cp * 2;                  // u16 [C] the map
      ord = o; o += Cp * 2;                  // u16 [C] L3 ids grouped by L2, ascending inside
    }
    total = o;
  }
};

template <typename T, bool LOGITS_IN>
__global__ __launch_bounds__(256) void eval_rows_kernel(const EvalArgs a, const L2MapArg map) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int B = a.B, C = a.C, L = a.num_l2;
  const int Cp = (C + 15) & ~15, ldl = Cp + kPad, ld2 = ((L + 15) & ~15) + kPad;
  const bool l2 = a.l2_mode != kEvalL2None, agg = a.l2_mode >= kEvalL2Sum;
  const EvalLds lay(C, L, agg);
  f32x4* red = (f32x4*)(smem + lay.red);
  float* nred = (float*)(smem + lay.nred);
  int* wgc = (int*)(smem + lay.wgc);
  float* Ls = (float*)(smem + lay.ls);
  float* L2s = (float*)(smem + lay.l2s);
  int* off = (int*)(smem + lay.off);
  int* cnt = (int*)(smem + lay.cnt);
  uint16_t* mp = (uint16_t*)(smem + lay.mp);
  uint16_t* ord = (uint16_t*)(smem + lay.ord);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, g = lane >> 4;
  const int b0 = blockIdx.x * 16;

  if (tid < 8) wgc[tid] = 0;

  // ---- phase 0: the map's CSR (groups in order, L3 ids ascending inside a group)
  if (agg) {
    for (int c = tid; c < C; c += 256) mp[c] = map.g[c];
    for (int q = tid; q < L; q += 256) cnt[q] = 0;
    __syncthreads();
    int rk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = tid + 256 * k;
      rk[k] = 0;
      if (c < C) {
        const int m = mp[c];
        int r = 0;
        for (int c2 = 0; c2 < c; ++c2) r += mp[c2] == m;
        rk[k] = r;
        atomicAdd(&cnt[m], 1);
      }
    }
    __syncthreads();
    if (w == 0) {   // exclusive scan of cnt: 16 groups per lane, then across the lanes
      int s = 0;
      for (int q = 16 * lane; q < 16 * lane + 16 && q < L; ++q) s += cnt[q];
      int incl = s;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      int run = incl - s;
      for (int q = 16 * lane; q < 16 * lane + 16 && q < L; ++q) {
        off[q] = run;
        run += cnt[q];
      }
      if (lane == 0) off[L] = C;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = tid + 256 * k;
      if (c < C) ord[off[mp[c]] + rk[k]] = (uint16_t)c;
    }
  }

  // ---- phase 1: the 16 x C logits tile
  if constexpr (LOGITS_IN) {
    for (int idx = tid; idx < 16 * C; idx += 256) {
      const int r = idx / C, c = idx - r * C;
      const int row = b0 + r < B ? b0 + r : B - 1;
      Ls[r * ldl + c] = a.logits[(size_t)row * C + c];
    }
  } else {
    const int E = a.E, nk = E / 16;
    const int row = b0 + i < B ? b0 + i : B - 1;
    const T* fp = (const T*)a.f + (size_t)row * E + 4 * g;
    const float* wrow = a.tw + (size_t)(4 * g) * C;
    const int k0 = w * nk / 4, k1 = (w + 1) * nk / 4;
    float inv[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ct0 = 0; ct0 < Cp / 16; ct0 += 4) {   // four class tiles per round
      int col[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) col[t] = (ct0 + t) * 16 + i < C ? (ct0 + t) * 16 + i : C - 1;
      f32x4 acc[4];
      float n2 = 0.f;
      if (ct0 == 0)
        mfma_chunks4<T, true>(fp, wrow, col, C, k0, k1, acc, n2);
      else
        mfma_chunks4<T, false>(fp, wrow, col, C, k0, k1, acc, n2);
      if (ct0 == 0) {
        n2 += __shfl_xor(n2, 16);   // (g0 + g1) + (g2 + g3) on every lane of row i
        n2 += __shfl_xor(n2, 32);
        if (g == 0) nred[w * 16 + i] = n2;
      } else {
        __syncthreads();            // the previous round's partials have been read
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) red[(t * 4 + w) * 64 + lane] = acc[t];
      __syncthreads();
      if (ct0 == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rl = 4 * g + j;
          const float nn = (nred[rl] + nred[16 + rl]) + (nred[32 + rl] + nred[48 + rl]);
          inv[j] = 1.0f / fmaxf(sqrtf(nn), 1e-12f);
        }
      }
      // wave w combines tile ct0 + w: wave 0's partial first, as head_logits_kernel does
      const int c = (ct0 + w) * 16 + i;
      const f32x4 p0 = red[(w * 4) * 64 + lane], p1 = red[(w * 4 + 1) * 64 + lane],
                  p2 = red[(w * 4 + 2) * 64 + lane], p3 = red[(w * 4 + 3) * 64 + lane];
      if (c < C) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          Ls[(4 * g + j) * ldl + c] = a.scale * (((p0[j] + p1[j]) + (p2[j] + p3[j])) * inv[j]);
      }
    }
  }
  __syncthreads();

  if (!LOGITS_IN && a.logits) {
    for (int idx = tid; idx < 16 * C; idx += 256) {
      const int r = idx / C, c = idx - r * C;
      if (b0 + r < B) a.logits[(size_t)(b0 + r) * C + c] = Ls[r * ldl + c];
    }
  }

  // ---- phase 2: per-row results, 16 lanes per row
  const int r = tid >> 4, sub = tid & 15, grow = b0 + r;
  const bool valid = grow < B;
  const float* lr = Ls + r * ldl;
  int t3[3];
  float tv[3];
  top3_16(lr, C, sub, t3, tv);
  const float mx = tv[0];
  float se = 0.f;
  for (int c = sub; c < C; c += 16) se += expf(lr[c] - mx);
  se = sum16(se);
  const int64_t yl = valid ? a.labels[grow] : -1;
  const int yy = (yl >= 0 && yl < C) ? (int)yl : -1;
  const bool counted = valid && yy >= 0 && t3[0] >= 0;
  if (valid && sub == 0) {
    a.row_loss[grow] = yy >= 0 ? (logf(se) + mx) - lr[yy] : 0.f;
    if (a.row_pred) a.row_pred[grow] = t3[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.row_top3) a.row_top3[(size_t)grow * 3 + k] = t3[k];
      if (a.row_top3_prob) a.row_top3_prob[(size_t)grow * 3 + k] = expf(tv[k] - mx) / se;
    }
  }
  const bool hit1 = counted && t3[0] == yy;
  const bool hit3 = counted && (t3[0] == yy || t3[1] == yy || t3[2] == yy);

  int p2 = -1, y2 = -1, q3[3] = {-1, -1, -1};
  if (l2) {
    if (yy >= 0) y2 = map.g[yy];
    if (agg) {
      float* l2r = L2s + r * ld2;
      for (int q = sub; q < L; q += 16) {
        const int j0 = off[q], j1 = off[q + 1];
        float s;
        if (a.l2_mode == kEvalL2LogSumExp) {
          s = -INFINITY;
          for (int j = j0; j < j1; ++j) s = logaddexp(s, lr[ord[j]]);
        } else {
          s = 0.f;
          for (int j = j0; j < j1; ++j) s += lr[ord[j]];
          if (a.l2_mode == kEvalL2Mean) s = s / (float)(j1 - j0 > 1 ? j1 - j0 : 1);
        }
        l2r[q] = s;
        if (valid && a.l2_logits) a.l2_logits[(size_t)grow * L + q] = s;
      }
      __syncthreads();
      float qv[3];
      top3_16(l2r, L, sub, q3, qv);
      p2 = q3[0];
    } else {
      p2 = t3[0] >= 0 ? (int)map.g[t3[0]] : -1;   // mode argmax: l3_to_l2[pred]
      q3[0] = p2;
    }
    if (valid && sub == 0) {
      if (a.l2_pred) a.l2_pred[grow] = p2;
      if (a.l2_top3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.l2_top3[(size_t)grow * 3 + k] = q3[k];
      }
    }
  }
  const bool ok2 = l2 && counted && p2 >= 0;
  const bool hit21 = ok2 && p2 == y2;
  const bool hit23 = ok2 && (q3[0] == y2 || q3[1] == y2 || q3[2] == y2);

  // ---- phase 3: integer accumulators
  if (sub == 0) {
    if (counted) {
      atomicAdd(&wgc[0], 1);
      atomicAdd(a.state + kEvalHeaderWords + (size_t)yy * C + t3[0], 1ull);
      if (ok2)
        atomicAdd(a.state + kEvalHeaderWords + (size_t)C * C + (size_t)y2 * L + p2, 1ull);
    } else if (valid) {
      atomicAdd(&wgc[5], 1);
    }
    if (hit1) atomicAdd(&wgc[1], 1);
    if (hit3) atomicAdd(&wgc[2], 1);
    if (hit21) atomicAdd(&wgc[3], 1);
    if (hit23) atomicAdd(&wgc[4], 1);
  }
  __syncthreads();
  if (tid < 6 && wgc[tid] != 0) {
    const int word = tid == 0 ? kEvalRows : tid == 5 ? kEvalSkipped : kEvalTop1 + tid - 1;
    atomicAdd(a.state + word, (unsigned long long)wgc[tid]);
  }
}

__global__ __launch_bounds__(256) void eval_finalise_kernel(const float* __restrict__ row_loss,
                                                            int B, unsigned long long* state) {
  __shared__ float part[256];
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int b = tid; b < B; b += 256) s += row_loss[b];
  part[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    double* loss = (double*)state;   // word kEvalLoss
    loss[kEvalLoss] += (double)(part[0] / (float)B);
    state[kEvalBatches] += 1ull;
  }
}

template <typename T, bool LOGITS_IN>
hipError_t launch_rows(const EvalArgs& a, const L2MapArg& map, hipStream_t s) {
  const EvalLds lay(a.C, a.num_l2, a.l2_mode >= kEvalL2Sum);
  // at most 160,640 B (C = num_l2 = 1024) of the 160 KiB
  const hipError_t attr = lds_opt_in((const void*)eval_rows_kernel<T, LOGITS_IN>, lay.total);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL((eval_rows_kernel<T, LOGITS_IN>), dim3((a.B + 15) / 16), dim3(256), lay.total,
                     s, a, map);
  return hipGetLastError();
}

}  // namespace

size_t eval_state_bytes(int C, int num_l2) {
  if (C < 3 || C > kMaxC || num_l2 < 1 || num_l2 > C) return 0;
  return sizeof(unsigned long long) * ((size_t)kEvalHeaderWords + (size_t)C * C + (size_t)num_l2 * num_l2);
}

bool eval_shape_ok(int B, int E, int C, int num_l2, int l2_mode, bool logits_in) {
  return B >= 1 && C >= 3 && C <= kMaxC && num_l2 >= 1 && num_l2 <= C && l2_mode >= kEvalL2None &&
         l2_mode <= kEvalL2LogSumExp && (logits_in || (E >= 16 && E <= 1024 && E % 16 == 0));
}

hipError_t eval_batch(int f_dtype, const void* f, const float* tw, const int64_t* labels, int B,
                      int E, int C, float scale, const int32_t* l3_to_l2_host, int num_l2,
                      int l2_mode, bool logits_in, void* state, float* logits, float* row_loss,
                      int32_t* row_pred, int32_t* row_top3, float* row_top3_prob, int32_t* l2_pred,
                      int32_t* l2_top3, float* l2_logits, hipStream_t s) {
  if (!eval_shape_ok(B, E, C, num_l2, l2_mode, logits_in) || !labels || !state || !row_loss ||
      ((uintptr_t)state & 7))
    return hipErrorInvalidValue;
  if (logits_in ? !logits : (!f || !tw || ((uintptr_t)f & 15) || !in_dtype_ok(f_dtype)))
    return hipErrorInvalidValue;
  if ((l2_mode != kEvalL2None) != (l3_to_l2_host != nullptr)) return hipErrorInvalidValue;
  L2MapArg map;
  for (int c = 0; c < kMaxC; ++c) map.g[c] = 0;
  if (l3_to_l2_host) {
    for (int c = 0; c < C; ++c) {
      if (l3_to_l2_host[c] < 0 || l3_to_l2_host[c] >= num_l2) return hipErrorInvalidValue;
      map.g[c] = (uint16_t)l3_to_l2_host[c];
    }
  }
  const EvalArgs a = {f, tw, labels, logits, row_loss, row_pred, row_top3, row_top3_prob,
                      l2_pred, l2_top3, l2_logits, (unsigned long long*)state, B, E, C, num_l2,
                      l2_mode, scale};
  const hipError_t e =
      logits_in ? launch_rows<float, true>(a, map, s)
                : dispatch_in_dtype(f_dtype, [&](auto tag) {
                    return launch_rows<typename decltype(tag)::type, false>(a, map, s);
                  });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(eval_finalise_kernel, dim3(1), dim3(256), 0, s, row_loss, B,
                     (unsigned long long*)state);
  return hipGetLastError();
}

hipError_t eval_reset(void* state, int C, int num_l2, hipStream_t s) {
  const size_t bytes = eval_state_bytes(C, num_l2);
  if (!state || !bytes || ((uintptr_t)state & 7)) return hipErrorInvalidValue;
  return hipMemsetAsync(state, 0, bytes, s);
}

}  // namespace miclip
