// Host-side launcher helpers shared by the op files; none of them has a device effect
// beyond the one-line row-staging kernel.
#pragma once
#include "common.h"

namespace miclip {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the element types an op reads its features in (widened exactly in the load)
inline bool in_dtype_ok(int dtype) { return dtype == kIn32 || dtype == kF16 || dtype == kBF16; }

template <typename T>
struct TypeTag {
  typedef T type;
};

// f(TypeTag<T>{}) for the T that `dtype` names; the caller has checked in_dtype_ok(dtype)
template <typename F>
auto dispatch_in_dtype(int dtype, F f) {
  if (dtype == kIn32) return f(TypeTag<float>{});
  if (dtype == kF16) return f(TypeTag<_Float16>{});
  return f(TypeTag<__bf16>{});
}

// Compute units of the current device, asked once; 256 (an MI355X) where the query fails
inline int cu_count() {
  static int ncu = [] {
    int d = 0, n = 0;
    if (hipGetDevice(&d) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return ncu;
}

// A kernel that may need more than 64 KiB of dynamic LDS opts in to the full 160 KiB
inline hipError_t lds_opt_in(const void* fn, size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// Staging a host row map: in an unnamed namespace like every op's own kernels, so each
// file that stages rows carries its own copy.
namespace {

// dst[i] = c.v[i], i < n: a piece of a host array, carried by the launch's own arguments
constexpr int kStageRows = 256;
template <typename I>
struct RowChunk {
  I v[kStageRows];
};
template <typename I>
__global__ __launch_bounds__(kStageRows) void stage_rows_kernel(RowChunk<I> c,
                                                                I* __restrict__ dst, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}

// dst[r] = fill(r) for r < n on stream s, kStageRows indices per launch: the host array
// behind fill is free on return and the stream is never waited for
template <typename I, typename Fill>
void stage_rows(I* dst, int n, hipStream_t s, Fill fill) {
  for (int r0 = 0; r0 < n; r0 += kStageRows) {
    const int cnt = n - r0 < kStageRows ? n - r0 : kStageRows;
    RowChunk<I> c;
    for (int q = 0; q < kStageRows; ++q) c.v[q] = q < cnt ? fill(r0 + q) : 0;
    hipLaunchKernelGGL(stage_rows_kernel<I>, dim3(1), dim3(kStageRows), 0, s, c, dst + r0, cnt);
  }
}

}  // namespace

}  // namespace miclip
