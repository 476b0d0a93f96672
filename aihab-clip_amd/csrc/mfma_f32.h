// The fp32-MFMA tile primitives of the cached-feature ops (tip, tip_train, prolip,
// kmeans, tsne, evaluate): exact fp32 products on v_mfma_f32_16x16x4_f32, fp32
// accumulation in one fixed, documented order. mfma_k's comment is the statement of the
// lane layout and the k order; the ops refer to it and do not restate it.
#pragma once
#include "common.h"

namespace miclip {

// LDS row stride of a [16][width] fp32 tile = width + 4 floats: 16 rows of float4 hit
// 16 bank groups
constexpr int kLdsPad = 4;

// 4 contiguous elements (fp32 / fp16 / bf16), widened exactly to fp32
template <typename T>
MICLIP_DEV f32x4 load4(const T* p) {
  if constexpr (sizeof(T) == 4) {
    return *(const f32x4*)p;
  } else {
    const u32x2 raw = *(const u32x2*)p;
    const T* e = (const T*)&raw;
    return f32x4{to_f<T>(e[0]), to_f<T>(e[1]), to_f<T>(e[2]), to_f<T>(e[3])};
  }
}

// row[col .. col + 3] of a row of D floats, zero past the end
template <bool VEC>
MICLIP_DEV f32x4 load4_clip(const float* row, int col, int D) {
  if constexpr (VEC) {   // D % 4 == 0: the 4 columns are all inside or all outside
    return col < D ? *(const f32x4*)(row + col) : f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    f32x4 v;
    v.x = col + 0 < D ? row[col + 0] : 0.f;
    v.y = col + 1 < D ? row[col + 1] : 0.f;
    v.z = col + 2 < D ? row[col + 2] : 0.f;
    v.w = col + 3 < D ? row[col + 3] : 0.f;
    return v;
  }
}

// One chunk of 16 k: four MFMAs of 4 k each, on .x .y .z .w in that order
MICLIP_DEV f32x4 mfma4(const f32x4& a, const f32x4& b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}

// One wave's 16 x 16 fp32 product over nch chunks of 16 k. Lane (i = lane & 15, g =
// lane >> 4) supplies fa(ch) = A[row i][16 ch + 4g + s] and fb(ch) = B[16 ch + 4g + s][col i]
// for s = 0..3 (the same k permutation on both operands), and ends with rows 4g .. 4g+3
// of column i. MFMA s of a chunk multiplies the pairs k = 16 ch + 4g + s over the four
// lane groups, so every output element is one fp32 fmaf chain in this order of k: chunks
// ascending, inside a chunk k = s, 4 + s, 8 + s, 12 + s for s = 0..3. The loads of two
// chunks are issued together; the accumulation order is unchanged.
template <typename FA, typename FB>
MICLIP_DEV f32x4 mfma_k(int nch, FA fa, FB fb) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int ch = 0;
  for (; ch + 2 <= nch; ch += 2) {
    const f32x4 a0 = fa(ch), b0 = fb(ch), a1 = fa(ch + 1), b1 = fb(ch + 1);
    acc = mfma4(a0, b0, acc);
    acc = mfma4(a1, b1, acc);
  }
  if (ch < nch) acc = mfma4(fa(ch), fb(ch), acc);
  return acc;
}

// sum over the 16 lanes that share a row (lanes 16 r .. 16 r + 15 of a wave), fixed butterfly
MICLIP_DEV float sum16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace miclip
