// On-device CLIP image preprocessing.
//
// Replaces the reference's per-image CPU transform
//   clip/clip.py:74-81 `_transform` / data/clip_transforms.py:50-55 (test split):
//   Resize(n, BICUBIC) on the shorter side -> CenterCrop(n) -> RGB -> ToTensor
//   -> Normalize(CLIP_MEAN, CLIP_STD)
// whose arithmetic is torchvision's size/anchor rules over Pillow's
// libImaging/Resample.c (8-bit two-pass separable cubic, a = -0.5, fixed point
// with 22 fractional bits). The kernels reproduce it bit for bit on uint8 HWC
// images already in HBM, computing only the crop window:
//   * `pre_tables_kernel` evaluates, once per distinct (H, W, n) geometry, the
//     crop window's horizontal and vertical coefficient tables in double with
//     FP contraction off, in Resample.c's operation order (the same doubles
//     the CPU computes), normalised to 22-bit fixed point; the handle caches
//     them (PreCache);
//   * `preprocess_kernel`, one workgroup per (image, band of 24 crop rows):
//     horizontal pass over the input rows the band's vertical taps need x
//     crop columns -> clip8 -> uint8 rows in LDS; vertical pass from LDS ->
//     clip8 -> float32 x/255, (x-mean)/std written planar [B,3,n,n] (or the
//     uint8 crop). Input pixels come through a per-image range-checked buffer
//     descriptor, 16 B per load (4 RGB taps), realigned with v_alignbyte and
//     accumulated with v_mad_i32_i24 (|coefficient| < 2^23, pixel < 2^8).
// HBM-bound in principle (each byte of the crop window is read about once;
// L1/L2 absorb the overlap of neighbouring taps).
//
// The train transform (data/clip_transforms.py:36-49,
// `preprocess_aug`) runs on the same resampler with host-drawn parameters:
//   * `aug_tables_kernel` writes every image's tables in one launch into a
//     per-call arena: RandomResizedCrop gives each image its own box, so the
//     box is resampled as an image of its own (crop, then resize) and nothing
//     is worth caching; BottomSquareCrop is the identity resize of its box;
//   * `preprocess_kernel<., true>` mirrors the store column for the flip;
//   * `rotate_kernel` gathers RandomRotation's nearest-neighbour source pixel
//     with Pillow's 16.16 fixed-point affine rule from the resized uint8 image
//     (a second pass: the gather crosses the bands).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <map>
#include <tuple>

#include "miclip.h"
#include "kernels.h"

namespace miclip {
namespace {

constexpr int kPB = 22;          // Resample.c PRECISION_BITS = 32 - 8 - 2
constexpr int kBand = 24;        // crop rows per workgroup (fewer shared input rows than 16)
constexpr int kThreads = 1024;   // 16 waves: the horizontal pass is load-latency bound
constexpr int kTmpBytes = 96 * 1024;   // LDS staging of horizontally resampled rows
constexpr int kMaxTaps = 64;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#pragma clang fp contract(off)
__device__ __host__ double cubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc for output index xx of
// an in_size -> out_size resize over the whole input: ksize fixed-point taps
// (zeros past the count), returns (xmin, count).
__device__ void coeffs(int in_size, int out_size, int xx, int ksize, int* k, int* bounds) {
  double filterscale, scale;
  filterscale = scale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 2.0 * filterscale;
  const double center = 0.0 + (xx + 0.5) * scale;
  double ww = 0.0;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  for (int x = 0; x < xmax; ++x) ww += cubic((x + xmin - center + 0.5) * ss);
  for (int x = 0; x < ksize; ++x) {
    int v = 0;
    if (x < xmax) {
      double c = cubic((x + xmin - center + 0.5) * ss);   // same double as the sum's term
      if (ww != 0.0) c /= ww;
      const double f = c * (double)(1 << kPB);
      v = c < 0 ? (int)(-0.5 + f) : (int)(0.5 + f);
    }
    k[x] = v;
  }
  bounds[0] = xmin;
  bounds[1] = xmax;
}

struct Geo {
  int nh, nw, top, left;
};

// torchvision: short side -> n, long side -> int(n * long / short); crop anchor
// int(round((size - n) / 2.0)) with Python's half-to-even round.
__host__ __device__ Geo geometry(int h, int w, int n) {
  Geo g;
  if (w <= h) {
    g.nw = n;
    g.nh = (int)((double)((long long)n * h) / w);
  } else {
    g.nh = n;
    g.nw = (int)((double)((long long)n * w) / h);
  }
  g.top = (int)rint((g.nh - n) / 2.0);
  g.left = (int)rint((g.nw - n) / 2.0);
  return g;
}

int ksize_for(int in_size, int out_size) {
  double fs = (double)in_size / out_size;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil(2.0 * fs) * 2 + 1;
}

// Geometry table: [KH, KV, 0 x 6] | hb [n][2] | hk [n][KH] | vb [n][2] | vk [n][KV]
int table_ints(int n, int KH, int KV) { return 8 + n * (4 + KH + KV); }

__global__ __launch_bounds__(256) void pre_tables_kernel(int H, int W, int n, int KH,
                                                              int KV, int* __restrict__ tab) {
  const Geo g = geometry(H, W, n);
  int* hb = tab + 8;
  int* hk = hb + 2 * n;
  int* vb = hk + n * KH;
  int* vk = vb + 2 * n;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    tab[0] = KH;
    tab[1] = KV;
    for (int e = 2; e < 8; ++e) tab[e] = 0;
  }
  if (i < n)
    coeffs(W, g.nw, g.left + i, KH, hk + i * KH, hb + 2 * i);
  else if (i < 2 * n)
    coeffs(H, g.nh, g.top + (i - n), KV, vk + (i - n) * KV, vb + 2 * (i - n));
}

// One image of a launch (device copy, built on the host per call).
struct PreImage {
  int64_t offset;     // byte offset of pixel (0, 0) from the pixels base
  uint32_t extent;    // bytes from pixel (0, 0) to the end of the last pixel
  int32_t H, W, C, stride;
  int32_t tab;        // int offset of its geometry table
};
static_assert(sizeof(PreImage) == 32, "PreImage layout");

__device__ __forceinline__ int clip8(int v) {
  v >>= kPB;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// d = a[23:0] * b[23:0] + c, signed 24-bit multiply at full VALU rate (hipcc
// lowers a plain int multiply to the quarter-rate v_mul_lo_u32 here)
__device__ __forceinline__ int mad24(int a, int b, int c) {
  int d;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

__device__ __forceinline__ int byte_of(uint32_t w, int i) {
  return (int)__builtin_amdgcn_ubfe(w, 8 * i, 8);
}

// One image's augmentation (device copy): what aug_tables_kernel resamples
// (in -> out size and the first output index of each axis, tap counts), the
// mirror of the resampled image and the rotation's 16.16 output -> source map.
struct AugImage {
  int32_t in_w, out_w, left, KH;
  int32_t in_h, out_h, top, KV;
  int32_t flip, rotate;
  int32_t a[6];
};
static_assert(sizeof(AugImage) == 64, "AugImage layout");

// OUT 0: float32 normalised planar [B,3,n,n]; 1: uint8 crop [B,n,n,3].
// AUG: `aug[b].flip` mirrors the store column (the resampled image is flipped).
template <int OUT, bool AUG>
__global__ __launch_bounds__(kThreads) void preprocess_kernel(
    const uint8_t* __restrict__ pix, const PreImage* __restrict__ imgs,
    const int* __restrict__ tabs, int n, int KH, int KV, void* __restrict__ out,
    const AugImage* __restrict__ aug) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* kh = (int*)smem;                      // [n][KH], KH % 16 == 0, zero-padded
  int* khb = kh + n * KH;                    // [n][2] xmin, count
  int* kv = khb + 2 * n;                     // [kBand][KV]
  int* kvb = kv + kBand * KV;                // [kBand][2]
  uint8_t* tmp = (uint8_t*)(kvb + 2 * kBand);

  const int b = blockIdx.x, i0 = blockIdx.y * kBand, tid = threadIdx.x;
  const PreImage d = imgs[b];
  const int C = d.C, stride = d.stride;
  const int* tab = tabs + d.tab;
  const int KHg = tab[0], KVg = tab[1];
  const int* hb = tab + 8;
  const int* hk = hb + 2 * n;
  const int* vb = hk + n * KHg;
  const int* vk = vb + 2 * n;
  const int nrows = n - i0 < kBand ? n - i0 : kBand;
  const bool flip = AUG && aug[b].flip != 0;

  for (int e = tid; e < n * KH; e += kThreads) {
    const int j = e / KH, t = e - j * KH;
    kh[e] = t < KHg ? hk[j * KHg + t] : 0;
  }
  for (int e = tid; e < 2 * n; e += kThreads) khb[e] = hb[e];
  for (int e = tid; e < nrows * KV; e += kThreads) {
    const int i = e / KV, t = e - i * KV;
    kv[e] = t < KVg ? vk[(i0 + i) * KVg + t] : 0;
  }
  for (int e = tid; e < 2 * nrows; e += kThreads) kvb[e] = vb[2 * i0 + e];
  __syncthreads();

  // per-image range-checked descriptor: loads past the image read 0, never fault
  const uint8_t* base = pix + d.offset;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, (int)d.extent, 0x00020000);
  const uint32_t extent = d.extent;

  const int rowb = n * C;                    // bytes of one staged row
  const int cap = kTmpBytes / rowb;          // staged rows that fit
  int s0 = 0;
  while (s0 < nrows) {
    // grow the sub-band while its input-row span fits the staging area
    const int ylo = kvb[2 * s0];
    int s1 = s0 + 1;
    while (s1 < nrows && kvb[2 * s1] + kvb[2 * s1 + 1] - ylo <= cap) ++s1;
    const int yhi = kvb[2 * (s1 - 1)] + kvb[2 * (s1 - 1) + 1];
    const int rows = yhi - ylo;

    // horizontal pass: staged[r][j][c] = clip8(half + sum_t in[ylo+r][xmin_j+t][c] * kh[j][t])
    for (int it = tid; it < rows * n; it += kThreads) {
      const int r = it / n, j = it - r * n;
      const int cnt = khb[2 * j + 1];
      const int* k = kh + j * KH;
      const uint32_t voff = (uint32_t)(ylo + r) * stride + (uint32_t)khb[2 * j] * C;
      const uint32_t al = voff & ~3u, sh = voff & 3u;
      const int ng = (cnt + 3) >> 2;                // groups of 4 taps
      if (C == 3) {
        int a0 = 1 << (kPB - 1), a1 = a0, a2 = a0;
        auto taps4 = [&](uint32_t w0, uint32_t w1, uint32_t w2, int4 kk) {
          a0 = mad24(byte_of(w0, 0), kk.x, a0);
          a1 = mad24(byte_of(w0, 1), kk.x, a1);
          a2 = mad24(byte_of(w0, 2), kk.x, a2);
          a0 = mad24(byte_of(w0, 3), kk.y, a0);
          a1 = mad24(byte_of(w1, 0), kk.y, a1);
          a2 = mad24(byte_of(w1, 1), kk.y, a2);
          a0 = mad24(byte_of(w1, 2), kk.z, a0);
          a1 = mad24(byte_of(w1, 3), kk.z, a1);
          a2 = mad24(byte_of(w2, 0), kk.z, a2);
          a0 = mad24(byte_of(w2, 1), kk.w, a0);
          a1 = mad24(byte_of(w2, 2), kk.w, a1);
          a2 = mad24(byte_of(w2, 3), kk.w, a2);
        };
        // fast path: every 16-B load of the item (4 groups per batch, the
        // batch's surplus groups meet zero coefficients) lies inside the image
        if (al + 48u * ((ng + 3) >> 2) + 16u <= extent) {
          for (int g = 0; g < ng; g += 4) {
            u32x4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
              v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, al + 12u * (g + q), 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              taps4(__builtin_amdgcn_alignbyte(v[q][1], v[q][0], sh),
                    __builtin_amdgcn_alignbyte(v[q][2], v[q][1], sh),
                    __builtin_amdgcn_alignbyte(v[q][3], v[q][2], sh),
                    *(const int4*)(k + 4 * (g + q)));
          }
        } else {   // the image's last bytes: byte loads, each range-checked
          for (int g = 0; g < ng; ++g) {
            uint32_t bb[12];
#pragma unroll
            for (int e = 0; e < 12; ++e)
              bb[e] = __builtin_amdgcn_raw_buffer_load_b8(rs, voff + 12u * g + e, 0, 0);
            taps4(bb[0] | bb[1] << 8 | bb[2] << 16 | bb[3] << 24,
                  bb[4] | bb[5] << 8 | bb[6] << 16 | bb[7] << 24,
                  bb[8] | bb[9] << 8 | bb[10] << 16 | bb[11] << 24, *(const int4*)(k + 4 * g));
          }
        }
        uint8_t* q = tmp + r * rowb + 3 * j;
        q[0] = (uint8_t)clip8(a0);
        q[1] = (uint8_t)clip8(a1);
        q[2] = (uint8_t)clip8(a2);
      } else {
        int a0 = 1 << (kPB - 1);
        auto taps4 = [&](uint32_t w, int4 kk) {
          a0 = mad24(byte_of(w, 0), kk.x, a0);
          a0 = mad24(byte_of(w, 1), kk.y, a0);
          a0 = mad24(byte_of(w, 2), kk.z, a0);
          a0 = mad24(byte_of(w, 3), kk.w, a0);
        };
        if (al + 16u * ((ng + 3) >> 2) + 8u <= extent) {
          for (int g = 0; g < ng; g += 4) {
            u32x4 v[2];
#pragma unroll
            for (int q = 0; q < 2; ++q)
              v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, al + 4u * g + 8u * q, 0, 0);
            taps4(__builtin_amdgcn_alignbyte(v[0][1], v[0][0], sh), *(const int4*)(k + 4 * g));
            taps4(__builtin_amdgcn_alignbyte(v[0][2], v[0][1], sh), *(const int4*)(k + 4 * g + 4));
            taps4(__builtin_amdgcn_alignbyte(v[0][3], v[0][2], sh), *(const int4*)(k + 4 * g + 8));
            taps4(__builtin_amdgcn_alignbyte(v[1][2], v[1][1], sh), *(const int4*)(k + 4 * g + 12));
          }
        } else {
          for (int g = 0; g < ng; ++g) {
            uint32_t bb[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
              bb[e] = __builtin_amdgcn_raw_buffer_load_b8(rs, voff + 4u * g + e, 0, 0);
            taps4(bb[0] | bb[1] << 8 | bb[2] << 16 | bb[3] << 24, *(const int4*)(k + 4 * g));
          }
        }
        tmp[r * rowb + j] = (uint8_t)clip8(a0);
      }
    }
    __syncthreads();

    // vertical pass + ToTensor/Normalize (or the uint8 crop)
    for (int it = tid; it < (s1 - s0) * n; it += kThreads) {
      const int ii = it / n, j = it - ii * n, i = s0 + ii;
      const int ymin = kvb[2 * i] - ylo, cnt = kvb[2 * i + 1];
      const int* k = kv + i * KV;
      int u[3];
      const uint8_t* q = tmp + ymin * rowb + j * C;
      if (C == 3) {
        int a0 = 1 << (kPB - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < cnt; ++t, q += rowb) {
          const int kt = k[t];
          a0 = mad24(q[0], kt, a0);
          a1 = mad24(q[1], kt, a1);
          a2 = mad24(q[2], kt, a2);
        }
        u[0] = clip8(a0);
        u[1] = clip8(a1);
        u[2] = clip8(a2);
      } else {
        int a0 = 1 << (kPB - 1);
        for (int t = 0; t < cnt; ++t, q += rowb) a0 = mad24(q[0], k[t], a0);
        u[0] = u[1] = u[2] = clip8(a0);   // convert("RGB") of an 'L' image
      }
      const int orow = i0 + i;
      const int ocol = AUG && flip ? n - 1 - j : j;
      if (OUT == 1) {
        uint8_t* o = (uint8_t*)out + (((size_t)b * n + orow) * n + ocol) * 3;
        o[0] = (uint8_t)u[0];
        o[1] = (uint8_t)u[1];
        o[2] = (uint8_t)u[2];
      } else {
        // float32(python float) constants, as torch builds the Normalize tensors
        const float mean[3] = {(float)0.48145466, (float)0.4578275, (float)0.40821073};
        const float stdv[3] = {(float)0.26862954, (float)0.26130258, (float)0.27577711};
        float* o = (float*)out + (size_t)b * 3 * n * n + (size_t)orow * n + ocol;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float x = (float)u[c] / 255.0f;
          o[(size_t)c * n * n] = (x - mean[c]) / stdv[c];
        }
      }
    }
    __syncthreads();
    s0 = s1;
  }
}

// Coefficient tables of a whole augmented batch in one launch: block (b, .)
// writes image b's table (pre_tables_kernel's layout and arithmetic) at
// imgs[b].tab of the per-call arena. Every image has its own box, so nothing
// here is worth caching.
__global__ __launch_bounds__(256) void aug_tables_kernel(const PreImage* __restrict__ imgs,
                                                         const AugImage* __restrict__ aug, int n,
                                                         int* __restrict__ arena) {
  const AugImage a = aug[blockIdx.x];
  int* tab = arena + imgs[blockIdx.x].tab;
  int* hb = tab + 8;
  int* hk = hb + 2 * n;
  int* vb = hk + n * a.KH;
  int* vk = vb + 2 * n;
  const int i = blockIdx.y * 256 + threadIdx.x;
  if (i == 0) {
    tab[0] = a.KH;
    tab[1] = a.KV;
    for (int e = 2; e < 8; ++e) tab[e] = 0;
  }
  if (i < n)
    coeffs(a.in_w, a.out_w, a.left + i, a.KH, hk + i * a.KH, hb + 2 * i);
  else if (i < 2 * n)
    coeffs(a.in_h, a.out_h, a.top + (i - n), a.KV, vk + (i - n) * a.KV, vb + 2 * (i - n));
}

// RandomRotation(30) = Image.rotate(NEAREST, expand=False, fillcolor=0) of the
// resized uint8 [B,n,n,3] image `src`: Geometry.c affine_fixed's gather
//   xin = (a2 + y*a1 + x*a0) >> 16, yin = (a5 + y*a4 + x*a3) >> 16
// with the sums in wrapping 32-bit arithmetic (unsigned here), 0 outside the
// image. One thread per output pixel; images of the batch that are not rotated
// are copied. Output as preprocess_kernel's.
template <int OUT>
__global__ __launch_bounds__(256) void rotate_kernel(const uint8_t* __restrict__ src,
                                                     const AugImage* __restrict__ aug, int n,
                                                     void* __restrict__ out) {
  const int b = blockIdx.x;
  const int p = blockIdx.y * 256 + threadIdx.x;
  if (p >= n * n) return;
  const int y = p / n, x = p - y * n;
  const AugImage a = aug[b];
  int xin = x, yin = y;
  if (a.rotate) {
    const uint32_t ux = (uint32_t)x, uy = (uint32_t)y;
    xin = (int)((uint32_t)a.a[2] + uy * (uint32_t)a.a[1] + ux * (uint32_t)a.a[0]) >> 16;
    yin = (int)((uint32_t)a.a[5] + uy * (uint32_t)a.a[4] + ux * (uint32_t)a.a[3]) >> 16;
  }
  int u[3] = {0, 0, 0};
  if (xin >= 0 && xin < n && yin >= 0 && yin < n) {
    const uint8_t* q = src + (((size_t)b * n + yin) * n + xin) * 3;
    u[0] = q[0];
    u[1] = q[1];
    u[2] = q[2];
  }
  if (OUT == 1) {
    uint8_t* o = (uint8_t*)out + ((size_t)b * n * n + p) * 3;
    o[0] = (uint8_t)u[0];
    o[1] = (uint8_t)u[1];
    o[2] = (uint8_t)u[2];
  } else {
    const float mean[3] = {(float)0.48145466, (float)0.4578275, (float)0.40821073};
    const float stdv[3] = {(float)0.26862954, (float)0.26130258, (float)0.27577711};
    float* o = (float*)out + (size_t)b * 3 * n * n + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = (float)u[c] / 255.0f;
      o[(size_t)c * n * n] = (v - mean[c]) / stdv[c];
    }
  }
}

hipError_t set_lds_attr(const void* f) {
  return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

}  // namespace

// Handle-owned state of miclip_preprocess: the geometry-table cache and the
// per-call image array (pinned staging + device copy).
struct PreCache {
  struct Entry {
    int off, KH, KV;
  };
  std::map<std::tuple<int, int, int>, Entry> geo;
  int* tabs = nullptr;
  size_t tab_cap = 0, tab_used = 0;   // ints
  PreImage* dev_imgs = nullptr;
  PreImage* host_imgs = nullptr;      // pinned
  int img_cap = 0;
  hipEvent_t copied = nullptr;        // last image-array upload done
  bool copy_pending = false;
  // preprocess_aug: per-call state, reused from call to call (stream-ordered)
  AugImage* dev_aug = nullptr;
  AugImage* host_aug = nullptr;       // pinned
  int aug_cap = 0;
  int* arena = nullptr;               // the batch's coefficient tables
  size_t arena_cap = 0;               // ints
  uint8_t* rot = nullptr;             // resized uint8 [B,n,n,3], input of the rotation
  size_t rot_cap = 0;                 // bytes
};

PreCache* pre_cache_create() { return new PreCache(); }

void pre_cache_destroy(PreCache* c) {
  if (!c) return;
  if (c->copied) (void)hipEventSynchronize(c->copied);
  if (c->tabs) (void)hipFree(c->tabs);
  if (c->dev_imgs) (void)hipFree(c->dev_imgs);
  if (c->host_imgs) (void)hipHostFree(c->host_imgs);
  if (c->dev_aug) (void)hipFree(c->dev_aug);
  if (c->host_aug) (void)hipHostFree(c->host_aug);
  if (c->arena) (void)hipFree(c->arena);
  if (c->rot) (void)hipFree(c->rot);
  if (c->copied) (void)hipEventDestroy(c->copied);
  delete c;
}

namespace {

// Image-array buffers for a batch of B, and the pinned staging free to write
// (the previous call's upload has left it).
hipError_t reserve_images(PreCache* c, int B, hipStream_t s) {
  hipError_t e;
  if (B > c->img_cap) {
    if (c->copy_pending && (e = hipEventSynchronize(c->copied)) != hipSuccess) return e;
    c->copy_pending = false;
    if (c->dev_imgs && (e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (c->dev_imgs) (void)hipFree(c->dev_imgs);
    if (c->host_imgs) (void)hipHostFree(c->host_imgs);
    c->dev_imgs = nullptr;
    c->host_imgs = nullptr;
    c->img_cap = 0;
    const int cap = B < 256 ? 256 : B;
    if ((e = hipMalloc(&c->dev_imgs, sizeof(PreImage) * cap)) != hipSuccess) return e;
    if ((e = hipHostMalloc(&c->host_imgs, sizeof(PreImage) * cap)) != hipSuccess) return e;
    c->img_cap = cap;
  }
  if (!c->copied && (e = hipEventCreateWithFlags(&c->copied, hipEventDisableTiming)) != hipSuccess)
    return e;
  if (c->copy_pending && (e = hipEventSynchronize(c->copied)) != hipSuccess) return e;
  c->copy_pending = false;
  return hipSuccess;
}

// Grows a handle-owned device buffer that earlier launches on `s` may still use.
template <typename T>
hipError_t grow_device(T** p, size_t* cap, size_t need, hipStream_t s) {
  if (need <= *cap) return hipSuccess;
  hipError_t e;
  if (*p) {
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
  }
  size_t n = *cap ? *cap : 1;
  while (n < need) n *= 2;
  if ((e = hipMalloc(p, n * sizeof(T))) != hipSuccess) return e;
  *cap = n;
  return hipSuccess;
}

bool valid_desc(const miclip_image_desc& d, int64_t* stride, int64_t* extent) {
  *stride = d.row_stride ? d.row_stride : (int64_t)d.width * d.channels;
  *extent = (int64_t)(d.height - 1) * *stride + (int64_t)d.width * d.channels;
  return !(d.height < 1 || d.width < 1 || (d.channels != 1 && d.channels != 3) || d.offset < 0 ||
           *stride < (int64_t)d.width * d.channels || *extent >= (1ll << 32) - 16);
}

}  // namespace

hipError_t preprocess(PreCache* c, const uint8_t* pixels, const miclip_image_desc* descs, int B,
                      int n, int out_kind, void* out, hipStream_t s, char* err, int errlen) {
  if (!c || B < 1 || n < 1 || n > 1024 || (out_kind != 0 && out_kind != 1)) {
    snprintf(err, errlen, "preprocess: bad batch %d / resolution %d / output kind %d", B, n,
             out_kind);
    return hipErrorInvalidValue;
  }
  hipError_t e;
  // validate, find or build each image's geometry table
  int KH = 4, KV = 1;
  if ((e = reserve_images(c, B, s)) != hipSuccess) return e;
  for (int i = 0; i < B; ++i) {
    const miclip_image_desc& d = descs[i];
    int64_t stride, extent;
    if (!valid_desc(d, &stride, &extent)) {
      snprintf(err, errlen, "preprocess: image %d has an invalid descriptor (%dx%dx%d, stride %d)",
               i, d.height, d.width, d.channels, d.row_stride);
      return hipErrorInvalidValue;
    }
    const Geo g = geometry(d.height, d.width, n);
    const int kh = ksize_for(d.width, g.nw), kv = ksize_for(d.height, g.nh);
    // a single crop row's vertical taps must fit the LDS staging area
    if (kh > kMaxTaps || kv > kMaxTaps || kv > kTmpBytes / (n * 3)) {
      snprintf(err, errlen,
               "preprocess: image %d (%dx%d) downscales too far for resolution %d (taps %d x %d, "
               "max %d)", i, d.height, d.width, n, kh, kv, kMaxTaps);
      return hipErrorInvalidValue;
    }
    const auto key = std::make_tuple(d.height, d.width, n);
    auto it = c->geo.find(key);
    if (it == c->geo.end()) {
      const size_t need = (size_t)table_ints(n, kh, kv);
      if (c->tab_used + need > c->tab_cap) {
        // grow (keeps every cached table: device-to-device copy, stream-ordered)
        size_t cap = c->tab_cap ? 2 * c->tab_cap : (size_t)1 << 20;
        while (cap < c->tab_used + need) cap *= 2;
        int* nt = nullptr;
        if ((e = hipMalloc(&nt, cap * sizeof(int))) != hipSuccess) return e;
        if (c->tabs) {
          if ((e = hipMemcpyAsync(nt, c->tabs, c->tab_used * sizeof(int),
                                  hipMemcpyDeviceToDevice, s)) != hipSuccess)
            return e;
          if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
          (void)hipFree(c->tabs);
        }
        c->tabs = nt;
        c->tab_cap = cap;
      }
      const int off = (int)c->tab_used;
      hipLaunchKernelGGL(pre_tables_kernel, dim3((2 * n + 255) / 256),
                         dim3(256), 0, s, d.height, d.width, n, kh, kv, c->tabs + off);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      c->tab_used += need;
      it = c->geo.emplace(key, PreCache::Entry{off, kh, kv}).first;
    }
    KH = it->second.KH > KH ? it->second.KH : KH;
    KV = it->second.KV > KV ? it->second.KV : KV;
    PreImage& p = c->host_imgs[i];
    p.offset = d.offset;
    p.extent = (uint32_t)extent;
    p.H = d.height;
    p.W = d.width;
    p.C = d.channels;
    p.stride = (int32_t)stride;
    p.tab = it->second.off;
  }
  KH = (KH + 15) & ~15;   // batches of 4 groups of 4 taps read whole 16-int rows
  const size_t lds = (size_t)(n * KH + 2 * n + kBand * KV + 2 * kBand) * 4 + kTmpBytes;
  if (lds > 160 * 1024) {
    snprintf(err, errlen, "preprocess: LDS need %zu B exceeds 160 KiB", lds);
    return hipErrorInvalidValue;
  }
  if ((e = hipMemcpyAsync(c->dev_imgs, c->host_imgs, sizeof(PreImage) * B,
                          hipMemcpyHostToDevice, s)) != hipSuccess)
    return e;
  if ((e = hipEventRecord(c->copied, s)) != hipSuccess) return e;
  c->copy_pending = true;
  const dim3 grid(B, (n + kBand - 1) / kBand);
  if (out_kind == 0) {
    static const hipError_t a0 = set_lds_attr((const void*)preprocess_kernel<0, false>);
    if (a0 != hipSuccess) return a0;
    hipLaunchKernelGGL((preprocess_kernel<0, false>), grid, dim3(kThreads), lds, s, pixels,
                       c->dev_imgs, c->tabs, n, KH, KV, out, (const AugImage*)nullptr);
  } else {
    static const hipError_t a1 = set_lds_attr((const void*)preprocess_kernel<1, false>);
    if (a1 != hipSuccess) return a1;
    hipLaunchKernelGGL((preprocess_kernel<1, false>), grid, dim3(kThreads), lds, s, pixels,
                       c->dev_imgs, c->tabs, n, KH, KV, out, (const AugImage*)nullptr);
  }
  return hipGetLastError();
}

// The reference's train transform (data/clip_transforms.py:36-49) with host-drawn
// parameters: per image a geometry (today's resize + centre crop, a box stretched
// to n x n = RandomResizedCrop, or a plain n x n crop = BottomSquareCrop), a
// mirror and a rotation. STRETCH and CROP are crop-then-resize, so the kernel
// sees the box as an image of its own: offset, extent and tables of the
// sub-rectangle (a CROP's tables are the identity, an exact copy). One tables
// launch and one resample launch per batch; a batch with a rotated image resamples
// into uint8 scratch and a gather launch writes the output.
hipError_t preprocess_aug(PreCache* c, const uint8_t* pixels, const miclip_image_desc* descs,
                          const miclip_aug_desc* augs, int B, int n, int out_kind, void* out,
                          hipStream_t s, char* err, int errlen) {
  if (!c || B < 1 || n < 1 || n > 1024 || (out_kind != 0 && out_kind != 1)) {
    snprintf(err, errlen, "preprocess_aug: bad batch %d / resolution %d / output kind %d", B, n,
             out_kind);
    return hipErrorInvalidValue;
  }
  hipError_t e;
  if ((e = reserve_images(c, B, s)) != hipSuccess) return e;
  if (B > c->aug_cap) {
    if (c->dev_aug && (e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (c->dev_aug) (void)hipFree(c->dev_aug);
    if (c->host_aug) (void)hipHostFree(c->host_aug);
    c->dev_aug = nullptr;
    c->host_aug = nullptr;
    c->aug_cap = 0;
    const int cap = B < 256 ? 256 : B;
    if ((e = hipMalloc(&c->dev_aug, sizeof(AugImage) * cap)) != hipSuccess) return e;
    if ((e = hipHostMalloc(&c->host_aug, sizeof(AugImage) * cap)) != hipSuccess) return e;
    c->aug_cap = cap;
  }
  int KH = 4, KV = 1;
  bool any_rot = false;
  size_t ints = 0;
  for (int i = 0; i < B; ++i) {
    const miclip_image_desc& d = descs[i];
    const miclip_aug_desc& g = augs[i];
    int64_t stride, extent;
    if (!valid_desc(d, &stride, &extent)) {
      snprintf(err, errlen,
               "preprocess_aug: image %d has an invalid descriptor (%dx%dx%d, stride %d)", i,
               d.height, d.width, d.channels, d.row_stride);
      return hipErrorInvalidValue;
    }
    PreImage& p = c->host_imgs[i];
    AugImage& a = c->host_aug[i];
    p.offset = d.offset;
    p.H = d.height;
    p.W = d.width;
    if (g.mode == MICLIP_AUG_RESIZE_CENTER) {
      const Geo q = geometry(d.height, d.width, n);
      a.in_w = d.width, a.out_w = q.nw, a.left = q.left;
      a.in_h = d.height, a.out_h = q.nh, a.top = q.top;
    } else if (g.mode == MICLIP_AUG_STRETCH || g.mode == MICLIP_AUG_CROP) {
      if (g.top < 0 || g.left < 0 || g.height < 1 || g.width < 1 ||
          (int64_t)g.top + g.height > d.height || (int64_t)g.left + g.width > d.width) {
        snprintf(err, errlen, "preprocess_aug: image %d: box (top %d, left %d, %dx%d) leaves the "
                 "%dx%d image", i, g.top, g.left, g.height, g.width, d.height, d.width);
        return hipErrorInvalidValue;
      }
      if (g.mode == MICLIP_AUG_CROP && (g.height != n || g.width != n)) {
        snprintf(err, errlen, "preprocess_aug: image %d: a CROP box is %dx%d, not %dx%d", i,
                 g.height, g.width, n, n);
        return hipErrorInvalidValue;
      }
      p.offset += (int64_t)g.top * stride + (int64_t)g.left * d.channels;
      p.H = g.height;
      p.W = g.width;
      extent = (int64_t)(g.height - 1) * stride + (int64_t)g.width * d.channels;
      a.in_w = g.width, a.out_w = n, a.left = 0;
      a.in_h = g.height, a.out_h = n, a.top = 0;
    } else {
      snprintf(err, errlen, "preprocess_aug: image %d: unknown mode %d", i, g.mode);
      return hipErrorInvalidValue;
    }
    a.KH = ksize_for(a.in_w, a.out_w);
    a.KV = ksize_for(a.in_h, a.out_h);
    // a single crop row's vertical taps must fit the LDS staging area
    if (a.KH > kMaxTaps || a.KV > kMaxTaps || a.KV > kTmpBytes / (n * 3)) {
      snprintf(err, errlen,
               "preprocess_aug: image %d (%dx%d) downscales too far for resolution %d (taps %d x "
               "%d, max %d)", i, a.in_h, a.in_w, n, a.KH, a.KV, kMaxTaps);
      return hipErrorInvalidValue;
    }
    a.flip = g.flip != 0;
    a.rotate = g.rotate != 0;
    for (int k = 0; k < 6; ++k) a.a[k] = g.affine[k];
    any_rot |= a.rotate != 0;
    p.extent = (uint32_t)extent;
    p.C = d.channels;
    p.stride = (int32_t)stride;
    p.tab = (int32_t)ints;
    ints += (size_t)table_ints(n, a.KH, a.KV);
    if (ints >= ((size_t)1 << 31)) {
      snprintf(err, errlen, "preprocess_aug: the coefficient tables of %d images exceed 2^31 "
               "entries", B);
      return hipErrorInvalidValue;
    }
    KH = a.KH > KH ? a.KH : KH;
    KV = a.KV > KV ? a.KV : KV;
  }
  KH = (KH + 15) & ~15;
  const size_t lds = (size_t)(n * KH + 2 * n + kBand * KV + 2 * kBand) * 4 + kTmpBytes;
  if (lds > 160 * 1024) {
    snprintf(err, errlen, "preprocess_aug: LDS need %zu B exceeds 160 KiB", lds);
    return hipErrorInvalidValue;
  }
  if ((e = grow_device(&c->arena, &c->arena_cap, ints, s)) != hipSuccess) return e;
  if (any_rot &&
      (e = grow_device(&c->rot, &c->rot_cap, (size_t)B * n * n * 3, s)) != hipSuccess)
    return e;
  if ((e = hipMemcpyAsync(c->dev_imgs, c->host_imgs, sizeof(PreImage) * B, hipMemcpyHostToDevice,
                          s)) != hipSuccess)
    return e;
  if ((e = hipMemcpyAsync(c->dev_aug, c->host_aug, sizeof(AugImage) * B, hipMemcpyHostToDevice,
                          s)) != hipSuccess)
    return e;
  if ((e = hipEventRecord(c->copied, s)) != hipSuccess) return e;
  c->copy_pending = true;
  hipLaunchKernelGGL(aug_tables_kernel, dim3(B, (2 * n + 255) / 256), dim3(256), 0, s,
                     c->dev_imgs, c->dev_aug, n, c->arena);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const dim3 grid(B, (n + kBand - 1) / kBand);
  if (any_rot || out_kind == 1) {
    static const hipError_t a1 = set_lds_attr((const void*)preprocess_kernel<1, true>);
    if (a1 != hipSuccess) return a1;
    hipLaunchKernelGGL((preprocess_kernel<1, true>), grid, dim3(kThreads), lds, s, pixels,
                       c->dev_imgs, c->arena, n, KH, KV, any_rot ? (void*)c->rot : out,
                       c->dev_aug);
  } else {
    static const hipError_t a0 = set_lds_attr((const void*)preprocess_kernel<0, true>);
    if (a0 != hipSuccess) return a0;
    hipLaunchKernelGGL((preprocess_kernel<0, true>), grid, dim3(kThreads), lds, s, pixels,
                       c->dev_imgs, c->arena, n, KH, KV, out, c->dev_aug);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (any_rot) {
    const dim3 rgrid(B, (n * n + 255) / 256);
    if (out_kind == 0)
      hipLaunchKernelGGL(rotate_kernel<0>, rgrid, dim3(256), 0, s, c->rot, c->dev_aug, n, out);
    else
      hipLaunchKernelGGL(rotate_kernel<1>, rgrid, dim3(256), 0, s, c->rot, c->dev_aug, n, out);
  }
  return hipGetLastError();
}

}  // namespace miclip
