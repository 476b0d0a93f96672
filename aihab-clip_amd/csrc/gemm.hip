// MFMA GEMM with fused epilogues for the ViT / text ResidualAttentionBlock.
//
// Replaces the torch Linear / packed in-projection / out-projection / conv1
// call sites of the reference (clip/model.py:171-175, 179-181, 204+217 and
// torch.nn.functional multi_head_attention_forward's in/out projections):
//   C[M,N] = A[M,K] . W[N,K]^T, A = activations (token rows), W = nn.Linear weight
//   layout [out, in] -- both operands K-contiguous ("NT"), so both MFMA
//   fragments are 16-byte row reads from LDS.
//
// CDNA4 design (cdna_hip_programming.md §5):
//   * 128x128x64 tile, 256 threads = 4 waves as 2(M) x 2(N), 64x64 per wave,
//     v_mfma_f32_16x16x32_{f16,bf16} with 4x4 fp32 accumulator tiles;
//   * global -> LDS by global_load_lds_dwordx4 (16 B per lane, 1 KiB per wave
//     instruction = 8 rows of 128 B), two LDS stages (64 KiB -> 2 WGs/CU);
//   * LDS image lane-linear, 16-B chunks XOR-swizzled by (row & 7) on the SOURCE
//     address and the same XOR on the ds_read_b128 address (rule 21, T2):
//     conflict-free for the 16x16x32 fragment reads;
//   * all fragments of a K-tile are read before the next tile's DMA is issued,
//     so no ds_read ever waits behind an in-flight LDS-DMA;
//   * bijective XCD-aware block remap so an XCD walks a contiguous range of
//     (A row-panel, W column-panel) tiles (T1).
// Epilogues are fused: bias, bias+QuickGELU (clip/model.py:160-162), bias +
// fp32 residual add (clip/model.py:184-185), and the patch-embed row remap +
// positional-embedding add (clip/model.py:217-221).
#include "common.h"
#include "epilogue.h"
#include "gemm_plan.h"
#include "kernels.h"
#include "launch.h"

#include <cstdlib>
#include <type_traits>
#include <utility>

// MICLIP_STAMPS_KLOOP (scripts/stamps/stamp_gemm_kloop.hip): the persistent
// kernel's main-loop vmcnt waits get a stamp segment of their own (6; the
// epilogue's staging-barrier segment then folds into 5)
#if defined(MICLIP_STAMPS) && defined(MICLIP_STAMPS_KLOOP)
#define MICLIP_KSTAMP(i) MICLIP_STAMP(i)
#define MICLIP_ESTAMP(i) MICLIP_STAMP(5)
#else
#define MICLIP_KSTAMP(i)
#define MICLIP_ESTAMP(i) MICLIP_STAMP(i)
#endif
// MICLIP_STAMPS_KPHASE (scripts/stamps/stamp_gemm_kphase.hip): the parts of each
// main-loop phase as segments (MICLIP_PSTAMP; that build folds every other stamp
// into segment 0)
#ifndef MICLIP_PSTAMP
#define MICLIP_PSTAMP(i)
#endif

namespace miclip {

namespace {

constexpr int BK = 64;

// ldk: row stride of A and W (elements); K: the k extent this workgroup reduces
// (ldk = K, except for the split-K partials below). bid: the tile (pre-remap).
template <typename T, int BM, int BN, class Epi>
MICLIP_DEV void gemm_nt_body(const T* __restrict__ A, const T* __restrict__ W, int M, int N,
                             int K, int ldk, Epi epi, int bid0) {
  constexpr int WN = 2;
  constexpr int TM = BM / 2, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int APW = BM / 8 / 4, BPW = BN / 8 / 4;  // 1 KiB pieces per wave
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int ntn = N / BN, ntm = (M + BM - 1) / BM;
  const int bid = xcd_remap(bid0, ntm * ntn);
  const int tm = bid / ntn, tn = bid - tm * ntn;
  const int m0 = tm * BM, n0 = tn * BN;

  // DMA sources: lane -> row (lane>>3) of an 8-row piece, physical chunk lane&7,
  // which holds logical chunk (lane&7) ^ (row&7).
  const int prow = lane >> 3, lchunk = (lane & 7) ^ prow;
  const T* a_src[APW];
  const T* b_src[BPW];
#pragma unroll
  for (int p = 0; p < APW; ++p) {
    int row = m0 + (wave * APW + p) * 8 + prow;
    row = row < M ? row : M - 1;
    a_src[p] = A + (size_t)row * ldk + lchunk * 8;
  }
#pragma unroll
  for (int p = 0; p < BPW; ++p) {
    const int row = n0 + (wave * BPW + p) * 8 + prow;
    b_src[p] = W + (size_t)row * ldk + lchunk * 8;
  }

  // fragment read offsets (bytes within a stage)
  const int fr = lane & 15, fk = lane >> 4;
  int a_off[FM][2], b_off[FN][2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
      a_off[i][s] = (wm * TM + i * 16 + fr) * 128 + (((4 * s + fk) ^ (fr & 7)) << 4);
#pragma unroll
    for (int j = 0; j < FN; ++j)
      b_off[j][s] = A_BYTES + (wn * TN + j * 16 + fr) * 128 + (((4 * s + fk) ^ (fr & 7)) << 4);
  }

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto stage = [&](int buf, int k0) {
    char* sa = smem + buf * STAGE;
#pragma unroll
    for (int p = 0; p < APW; ++p) glds16(a_src[p] + k0, sa + (wave * APW + p) * 1024);
#pragma unroll
    for (int p = 0; p < BPW; ++p)
      glds16(b_src[p] + k0, sa + A_BYTES + (wave * BPW + p) * 1024);
  };

  const int nk = K / BK;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int t = 0; t < nk; ++t) {
    const char* sb = smem + (t & 1) * STAGE;
    i16x8 af[2][FM], bf[2][FN];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < FM; ++i) af[s][i] = *(const i16x8*)(sb + a_off[i][s]);
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[s][j] = *(const i16x8*)(sb + b_off[j][s]);
    }
    if (t + 1 < nk) stage((t + 1) & 1, (t + 1) * BK);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = Mfma<T>::m16(af[s][i], bf[s][j], acc[i][j]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int col = n0 + wn * TN + j * 16 + fr;
    const float b = epi.bias1(col);
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * TM + i * 16 + fk * 4 + r;
        if (row < M) epi.put1(row, col, acc[i][j][r], b);
      }
    }
  }
}

template <typename T, int BM, int BN, class Epi>
__global__ __launch_bounds__(256) void gemm_nt_kernel(const T* __restrict__ A,
                                                      const T* __restrict__ W, int M, int N,
                                                      int K, Epi epi) {
  gemm_nt_body<T, BM, BN>(A, W, M, N, K, K, epi, blockIdx.x);
}

// Split-K for the small-M GEMMs of the CLS-only last block (M = images, K up to
// 4W: a few 128x128 tiles would each walk the whole K alone). Split s =
// blockIdx.y reduces k in [s*Ks, (s+1)*Ks) into an fp32 partial plane ws[s][M][N];
// splitk_reduce_kernel sums the S planes in ascending s (fixed order: deterministic,
// and the same for every M, so a row's result does not depend on the batch) and
// applies the epilogue's own put4 (bias, activation, folded LN, fp16 residual).
template <typename T>
__global__ __launch_bounds__(256) void gemm_nt_splitk_kernel(const T* __restrict__ A,
                                                             const T* __restrict__ W, int M,
                                                             int N, int K, int Ks,
                                                             float* __restrict__ ws) {
  const int sk = blockIdx.y;
  gemm_nt_body<T, 128, 128>(A + (size_t)sk * Ks, W + (size_t)sk * Ks, M, N, Ks, K,
                            EpiF32{ws + (size_t)sk * M * N, nullptr, N}, blockIdx.x);
}

template <class Epi>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, int S,
                                                            int M, int N, Epi epi) {
  const int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = N / 4;
  if (i4 >= (int64_t)M * n4) return;
  const int r = (int)(i4 / n4), c = (int)(i4 - (int64_t)r * n4) * 4;
  const size_t plane = (size_t)M * N, off = (size_t)r * N + c;
  float4 v = *(const float4*)(ws + off);
  for (int s = 1; s < S; ++s) {
    const float4 u = *(const float4*)(ws + s * plane + off);
    v = make_float4(v.x + u.x, v.y + u.y, v.z + u.z, v.w + u.w);
  }
  epi.put4(r, c, v, epi.bias4(c));
}


// ---------------------------------------------------------------------------
// 256x256x64 tile, 512 threads = 8 waves as 2(M) x 4(N), 128x64 per wave.
// LDS: 2 buffers x 4 half-tile slots {A0, A1, B0, B1} x 16 KiB = 128 KiB
// (1 workgroup per CU). Slot A_h holds tile rows {wr*128 + h*64 + 0..63},
// slot B_h tile cols {wc*64 + h*32 + 0..31}, so wave quadrant (qi, qj) reads
// exactly slots A_qi and B_qj. Each K-tile runs as 4 phases (quadrants
// Q0=(0,0) Q1=(0,1) Q2=(1,1) Q3=(1,0), 16 MFMAs each); every phase issues one
// half-tile of LDS-DMA (2 x global_load_lds_dwordx4 per lane) into a slot
// whose last reader finished before that phase's barrier:
//   phase 0: A1(t+1)   phase 1: B0(t+1)   phase 2: A0(t+2)   phase 3: B1(t+2)
// so one K-tile's data is in flight across the K-tile boundary and the only
// wait is a counted `s_waitcnt vmcnt(4)` once per K-tile (never 0 in the
// main loop; cdna_hip_programming.md §5 "Pipelining across barriers", T3/T4).
// ---------------------------------------------------------------------------
MICLIP_DEV void lds_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// SCHED 0: the half-tile schedule above (4 barriers per K-tile, ~1.5 K-tiles
// in flight, fragment reads right after each barrier). SCHED 1: fragment
// prefetch one quadrant ahead, one barrier per K-tile (see the branch below).
// 4x4 transpose inside each quad of lanes (DPP quad_perm): on entry lane jj of
// a quad holds column jj of a 4x4 block (a[r] = M[r][jj], the MFMA C layout);
// on exit it holds row jj (v[c] = M[jj][c]), i.e. 4 consecutive columns.
template <int CTRL>
MICLIP_DEV float dpp_f(float x) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}

MICLIP_DEV float4 quad_transpose(f32x4 a, int lane) {
  const bool odd = lane & 1, hi = lane & 2;
  // stage 1, partner jj^1 (quad_perm [1,0,3,2]): even lanes end with rows {0,2},
  // odd with rows {1,3}, each as a column pair (2u, 2u+1), u = jj >> 1
  const float t0 = dpp_f<0xB1>(odd ? a[0] : a[1]);
  const float t1 = dpp_f<0xB1>(odd ? a[2] : a[3]);
  const float x0 = odd ? t0 : a[0], y0 = odd ? a[1] : t0;
  const float x1 = odd ? t1 : a[2], y1 = odd ? a[3] : t1;
  // stage 2, partner jj^2 (quad_perm [2,3,0,1]): u = 0 keeps its low row, u = 1 its high
  const float r0 = dpp_f<0x4E>(hi ? x0 : x1);
  const float r1 = dpp_f<0x4E>(hi ? y0 : y1);
  return hi ? make_float4(r0, r1, x1, y1) : make_float4(x0, y0, r0, r1);
}

// Epilogue straight from the accumulators (no LDS): after the quad transpose
// each lane owns 4 consecutive columns of one row of every 16x16 fragment, so
// the epilogue functor's put4 (16-B aligned) applies unchanged. Rows are
// m0 + wr*128 + qi*64 + i*16 + fk*4 + jj, columns n0 + wc*64 + qj*32 + j*16 + 4q.
// A per-store row guard would make hipcc wait vmcnt(0) around every store --
// i.e. for the next tile's in-flight LDS-DMA in the persistent kernel -- so
// full tiles take a guard-free path (`full` is wave-uniform).
template <class Epi>
MICLIP_DEV void load_bias_regs(const Epi& epi, int n0, int wc, int lane, float4 (&bv)[2][2]) {
  const int q = (lane & 15) >> 2;
#pragma unroll
  for (int qj = 0; qj < 2; ++qj)
#pragma unroll
    for (int j = 0; j < 2; ++j) bv[qj][j] = epi.bias4nb(n0 + wc * 64 + qj * 32 + j * 16 + 4 * q);
}

// Residual epilogue, software-pipelined over the 8 row groups (qi, i): the 4
// x loads of group k+1 are issued before group k is combined and stored.
// Compiler-visible loads and stores, so hipcc counts them and emits exact
// vmcnt waits (it hoists the x loads and spills ~20 VGPRs: this path serves
// the non-default variants 260 and 3 only). (An inline-asm load with a VGPR destination counts as
// written at the end of its statement, so hipcc may reuse that register --
// e.g. for a store address -- before the data lands: an intermittent memory
// fault. cdna_hip_programming.md §5.7 item 1.)
template <bool GUARD>
MICLIP_DEV void epilogue_residual_regs(const f32x4 (&acc)[2][2][4][2],
                                       const float4 (&bv)[2][2], int m0, int n0, int wr,
                                       int wc, int lane, int M, const EpiResidual<float>& epi) {
  const int fk = lane >> 4, q = (lane & 15) >> 2, jj = lane & 3;
  auto row_of = [&](int k) {
    const int r = m0 + wr * 128 + (k >> 2) * 64 + (k & 3) * 16 + fk * 4 + jj;
    return GUARD ? (r < M ? r : M - 1) : r;
  };
  auto xptr = [&](int row, int qj, int j) {
    return epi.X + (size_t)row * epi.ldx + n0 + wc * 64 + qj * 32 + j * 16 + 4 * q;
  };
  f32x4 xa[4], xb[4];
  auto issue = [&](f32x4 (&x)[4], int k) {
    const int row = row_of(k);
#pragma unroll
    for (int f = 0; f < 4; ++f) x[f] = *(const f32x4*)xptr(row, f >> 1, f & 1);
  };
  issue(xa, 0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    f32x4 (&cur)[4] = (k & 1) ? xb : xa;
    f32x4 (&nxt)[4] = (k & 1) ? xa : xb;
    if (k + 1 < 8) issue(nxt, k + 1);
    const int qi = k >> 2, i = k & 3;
    const int r_true = m0 + wr * 128 + qi * 64 + i * 16 + fk * 4 + jj;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int qj = f >> 1, j = f & 1;
      const float4 v = quad_transpose(acc[qi][qj][i][j], lane);
      const float4 b = bv[qj][j];
      const f32x4 x = cur[f];
      const f32x4 y = {x[0] + (v.x + b.x), x[1] + (v.y + b.y), x[2] + (v.z + b.z),
                       x[3] + (v.w + b.w)};
      if (!GUARD || r_true < M) *(f32x4*)xptr(r_true, qj, j) = y;
    }
  }
}

template <bool GUARD, class Epi>
MICLIP_DEV void epilogue_regs_body(const f32x4 (&acc)[2][2][4][2], const float4 (&bv)[2][2],
                                   int m0, int n0, int wr, int wc, int lane, int M,
                                   const Epi& epi) {
  if constexpr (std::is_same_v<Epi, EpiResidual<float>>) {
    epilogue_residual_regs<GUARD>(acc, bv, m0, n0, wr, wc, lane, M, epi);
    return;
  }
  const int fk = lane >> 4, q = (lane & 15) >> 2, jj = lane & 3;
#pragma unroll
  for (int qi = 0; qi < 2; ++qi)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + wr * 128 + qi * 64 + i * 16 + fk * 4 + jj;
#pragma unroll
      for (int qj = 0; qj < 2; ++qj)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int col = n0 + wc * 64 + qj * 32 + j * 16 + 4 * q;
          const float4 v = quad_transpose(acc[qi][qj][i][j], lane);
          if (!GUARD || row < M) epi.template put4<true>(row, col, v, bv[qj][j]);
        }
    }
}

// bv: the tile's bias columns (load_bias_regs), loaded ahead by the caller.
template <class Epi>
MICLIP_DEV void epilogue_regs(const f32x4 (&acc)[2][2][4][2], const float4 (&bv)[2][2], int m0,
                              int n0, int wr, int wc, int lane, int M, const Epi& epi) {
  if (m0 + 256 <= M)
    epilogue_regs_body<false>(acc, bv, m0, n0, wr, wc, lane, M, epi);
  else
    epilogue_regs_body<true>(acc, bv, m0, n0, wr, wc, lane, M, epi);
}

// ---------------------------------------------------------------------------
// Tail of a 256x256 launch. M = 257 * images is never a multiple of 256 rows,
// so ceil(M/256) * N/256 tiles always leave a last round of a few tiles on a
// 256-CU chip (1028 tiles = 4 rounds + 4 tiles at N = 1024: the fifth round
// costs a whole tile time for 0.4 % of the work). The launch therefore
// covers only `ntm_dp` tile-rows (a whole number of rounds) with 256x256
// tiles, and the remaining <= 256 rows with extra workgroups that take this
// path: one 16-row x 64-column task per workgroup over the full K, a skinny
// GEMM streamed through LDS. Per K-tile (64 k) the A piece (16 rows, 2 KiB)
// and the W piece (64 columns, 8 KiB) are LDS-DMA'd into one of TS stages
// (every wave issues one W piece, waves 0-1 one A piece each; same 16-B chunk
// XOR swizzle as the tiles), TS-1 K-tiles in flight, one counted vmcnt and
// one barrier per K-tile; waves 0-3 each multiply the A fragments by the B
// fragments of 16 columns. Every output element accumulates the same
// v_mfma_f32_16x16x32 chain in the same k order as in the 256x256 tile (k
// chunks of 32 ascending, lane k-offset 8*(lane>>4)) and the epilogue applies
// the same functor, so results are bit-identical to an all-tile launch (the
// encode stays batch-invariant).
// ---------------------------------------------------------------------------
// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the count is an immediate)
MICLIP_DEV void wait_vmcnt(int n) {
  switch (n) {
#define MICLIP_VMC(k) \
  case k:           \
    asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    MICLIP_VMC(0) MICLIP_VMC(1) MICLIP_VMC(2) MICLIP_VMC(3) MICLIP_VMC(4) MICLIP_VMC(5)
    MICLIP_VMC(6) MICLIP_VMC(7) MICLIP_VMC(8) MICLIP_VMC(9) MICLIP_VMC(10) MICLIP_VMC(11)
    MICLIP_VMC(12) MICLIP_VMC(13) MICLIP_VMC(14) MICLIP_VMC(15) MICLIP_VMC(16)
#undef MICLIP_VMC
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// RG row groups of 16 x TN columns per workgroup: RG = 1, TN = 64 (waves 0-3
// own 16 columns each) or RG = 2, TN = 128 (wave = row group x 32 columns).
template <int RG, int TN>
struct TailShape {
  static constexpr int SA = RG * 2048, SB = TN * 128, STG = SA + SB;
  static constexpr int TS = 122880 / STG < 8 ? 122880 / STG : 8;   // stages (<= 120 KiB)
  static constexpr int NA = RG * 2, NB = TN / 8;                   // A / W pieces (1 KiB)
  static constexpr int CPW = RG == 1 ? 16 : 32;                    // columns per wave
};

// NW: waves of the calling workgroup (8: the 512-thread kernels; 4: gemm4s_kernel,
// where at RG = 2 every wave takes both row groups of its 32 columns).
template <typename T, class Epi, int RG, int TN, int NW = 8>
MICLIP_DEV void gemm_tail_wg(const T* __restrict__ A, const T* __restrict__ W, int M, int N,
                             int K, const Epi& epi, int m_start, int task, char* smem) {
  using S = TailShape<RG, TN>;
  static_assert(NW == 8 || NW == 4, "tail tasks run on 4 or 8 waves");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ncg = N / TN, rg = task / ncg;
  const int row0 = m_start + rg * 16 * RG, col0 = (task - rg * ncg) * TN;
  if (row0 >= M) return;   // whole workgroup (task is workgroup-uniform)
  const int nk = K / 64;
  // LDS-DMA pieces of 8 rows x 128 B: A pieces 0..NA-1 by waves 0..NA-1,
  // W pieces wave, wave+NW, ... (NB / NW per wave)
  const int lchunk = (lane & 7) ^ (lane >> 3);
  int ar = row0 + wave * 8 + (lane >> 3);
  ar = ar < M ? ar : M - 1;
  const T* asrc = A + (size_t)ar * K + lchunk * 8;
  const T* bsrc = W + (size_t)(col0 + wave * 8 + (lane >> 3)) * K + lchunk * 8;
  constexpr int BPW = S::NB / NW;
  const int per_stage = BPW + (wave < S::NA ? 1 : 0);   // LDS-DMA instructions per stage
  auto stage = [&](int t) {
    char* st = smem + (t % S::TS) * S::STG;
    if (wave < S::NA) glds16(asrc + t * 64, st + wave * 1024);
#pragma unroll
    for (int i = 0; i < BPW; ++i)
      glds16(bsrc + (size_t)i * NW * 8 * K + t * 64, st + S::SA + (wave + NW * i) * 1024);
  };
  const int fr = lane & 15, fk = lane >> 4;
  const int sw0 = ((0 + fk) ^ (fr & 7)) << 4, sw1 = ((4 + fk) ^ (fr & 7)) << 4;
  // row groups per wave: 2 when 4 waves cover RG = 2
  constexpr int NRW = (NW == 4 && RG == 2) ? 2 : 1;
  const int wrow = (RG == 1 || NW == 4) ? 0 : wave >> 2;   // this wave's first row group
  const int wcol = (RG == 1 ? wave : wave & 3) * S::CPW;
  const bool active = RG == 2 || wave < 4;
  constexpr int NJ = S::CPW / 16;
  f32x4 acc[NRW][NJ];
#pragma unroll
  for (int rr = 0; rr < NRW; ++rr)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[rr][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < S::TS - 1 && t < nk; ++t) stage(t);
  for (int t = 0; t < nk; ++t) {
    // retire stage t: the younger loads are stages t+1 .. min(t+TS-2, nk-1)
    const int younger = nk - 1 - t < S::TS - 2 ? nk - 1 - t : S::TS - 2;
    wait_vmcnt(younger * per_stage);
    lds_barrier();
    // refill the stage read in iteration t-1 (every wave passed this barrier)
    if (t + S::TS - 1 < nk) stage(t + S::TS - 1);
    if (active) {
      const char* st = smem + (t % S::TS) * S::STG;
#pragma unroll
      for (int rr = 0; rr < NRW; ++rr) {
        const char* sa = st + ((wrow + rr) * 16 + fr) * 128;
        const i16x8 a0 = *(const i16x8*)(sa + sw0);
        const i16x8 a1 = *(const i16x8*)(sa + sw1);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const char* sb = st + S::SA + (wcol + j * 16 + fr) * 128;
          acc[rr][j] = Mfma<T>::m16(a0, *(const i16x8*)(sb + sw0), acc[rr][j]);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const char* sb = st + S::SA + (wcol + j * 16 + fr) * 128;
          acc[rr][j] = Mfma<T>::m16(a1, *(const i16x8*)(sb + sw1), acc[rr][j]);
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  if (!active) return;
  // same register epilogue as the tiles: quad transpose -> 4 consecutive columns
  const int q = (lane & 15) >> 2, jj = lane & 3;
#pragma unroll
  for (int rr = 0; rr < NRW; ++rr) {
    const int row = row0 + (wrow + rr) * 16 + fk * 4 + jj;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = col0 + wcol + j * 16 + 4 * q;
      const float4 v = quad_transpose(acc[rr][j], lane);
      if (row < M) epi.put4(row, col, v, epi.bias4(col));
    }
  }
}

// ntm_dp: tile-rows covered by 256x256 tiles (blocks [0, ntm_dp*ntn)); blocks
// beyond them run the tail path over rows [ntm_dp*256, M) (see gemm_tail_wg).
template <typename T, class Epi, int SCHED, bool REGEPI = false>
__global__ __launch_bounds__(512) void gemm256_kernel(const T* __restrict__ A,
                                                      const T* __restrict__ W, int M, int N,
                                                      int K, Epi epi, int gm, int ntm_dp,
                                                      int tail_mode) {
  constexpr int HALF = 128 * 128;  // bytes of one half-tile slot
  constexpr int EPI_LD = 260;      // fp32 row stride of the epilogue staging (pad 4)
  constexpr int SMEM = 128 * EPI_LD * 4 > 8 * HALF ? 128 * EPI_LD * 4 : 8 * HALF;
  __shared__ __attribute__((aligned(1024))) char smem[SMEM];

  const int ntn = N / 256, ntm = ntm_dp;
  // Block roles. Plain: tiles [0, ntm*ntn), then the tail workgroups. With
  // TAIL_FIRST (bit 1 of tail_mode) the tail workgroups are interleaved with
  // the first tiles, 8 of each per 16 consecutive blocks (one of each per
  // XCD, so tile d keeps XCD d % 8 for xcd_remap): the CUs that draw tail
  // work start their tile sequence later, which staggers the rounds so that
  // one round's epilogue store burst overlaps other CUs' main loops instead of
  // every CU writing at once.
  const int ndp = ntm * ntn, bid = blockIdx.x;
  int dp = bid, tail = -1;
  if (tail_mode & 2) {
    const int nt8 = gridDim.x - ndp;   // tail blocks (a multiple of 8)
    if (bid < 2 * nt8) {
      const int g = bid >> 4, r = bid & 15;
      dp = r < 8 ? g * 8 + r : -1;
      tail = r < 8 ? -1 : g * 8 + r - 8;
    } else {
      dp = bid - nt8;
    }
  } else if (bid >= ndp) {
    dp = -1;
    tail = bid - ndp;
  }
  if (dp < 0) {
    if (tail_mode & 1)
      gemm_tail_wg<T, Epi, 2, 128>(A, W, M, N, K, epi, ntm * 256, tail, smem);
    else
      gemm_tail_wg<T, Epi, 1, 64>(A, W, M, N, K, epi, ntm * 256, tail, smem);
    return;
  }
  // Round stagger (tail_mode bits 8..15 = microseconds): half of the first
  // round's workgroups (every other one per XCD) start late, so the CUs run
  // their tile sequences offset and one half's epilogue store burst falls in
  // the other half's main loop instead of every CU writing at once.
  if ((tail_mode >> 8) && bid < 256 && ((bid >> 3) & 1)) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long ticks = (unsigned long long)(tail_mode >> 8) * 100;   // 100 MHz
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  int tm, tn;
  group_tile(xcd_remap(dp, ndp), ntm, ntn, gm, tm, tn);
  const int m0 = tm * 256, n0 = tn * 256;
  // LDS-DMA sources: slot row sr = piece*8 + (lane>>3), piece = wave*2 + pp
  const int lchunk = (lane & 7) ^ (lane >> 3);
  const T* asrc[2][2];
  const T* bsrc[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const int sr = (wave * 2 + pp) * 8 + (lane >> 3);
      int ar = m0 + (sr >> 6) * 128 + h * 64 + (sr & 63);
      ar = ar < M ? ar : M - 1;
      asrc[h][pp] = A + (size_t)ar * K + lchunk * 8;
      const int bc = n0 + (sr >> 5) * 64 + h * 32 + (sr & 31);
      bsrc[h][pp] = W + (size_t)bc * K + lchunk * 8;
    }
  // slot index: buf*4 + {0:A0, 1:A1, 2:B0, 3:B1}
  auto stage = [&](int slot_kind, int tile) {
    const int buf = tile & 1, k0 = tile * 64;
    char* dst = smem + (buf * 4 + slot_kind) * HALF + wave * 2048;
    const T* const* src = slot_kind < 2 ? asrc[slot_kind] : bsrc[slot_kind - 2];
    glds16(src[0] + k0, dst);
    glds16(src[1] + k0, dst + 1024);
  };
  const int fr = lane & 15, fk = lane >> 4;
  // byte offsets inside a slot for k-step s (swizzled 16-B chunk), per fragment row
  const int aoff = (wr * 64 + fr) * 128, boff = (wc * 32 + fr) * 128;
  const int sw0 = ((0 + fk) ^ (fr & 7)) << 4, sw1 = ((4 + fk) ^ (fr & 7)) << 4;

  f32x4 acc[2][2][4][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / 64;
  i16x8 af[2][4], bf[2][2];
  auto quadrant = [&](const char* sa, const char* sb, int qi, int qj, bool load_a,
                      bool load_b = true) {
    if (load_a) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[0][i] = *(const i16x8*)(sa + i * 2048 + sw0);
        af[1][i] = *(const i16x8*)(sa + i * 2048 + sw1);
      }
    }
    if (load_b) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bf[0][j] = *(const i16x8*)(sb + j * 2048 + sw0);
        bf[1][j] = *(const i16x8*)(sb + j * 2048 + sw1);
      }
    }
  };
  auto mfma_q = [&](int qi, int qj) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[qi][qj][i][j] = Mfma<T>::m16(af[s][i], bf[s][j], acc[qi][qj][i][j]);
    __builtin_amdgcn_s_setprio(0);
  };

  if constexpr (SCHED == 2) {
    // Staggered SCHED 0 (cdna_hip_programming.md §5 "256^2 8-phase template",
    // its `if (wr == 1) s_barrier`): each phase is [R: fragment reads + one
    // half-tile LDS-DMA + lgkmcnt(0)] barrier [M: 16 MFMAs] barrier, and waves
    // 4-7 (wr = 1, the partners of waves 0-3 on the same SIMDs) run one barrier
    // behind, so on every SIMD one wave reads LDS while its partner issues
    // MFMAs. Hazards, in barrier intervals (group 0 does R_j in interval 2j,
    // group 1 in 2j+1): every slot is restaged at least one interval after its
    // last read by either group; group 0 retires its LDS-DMA up to B0(t+1) with
    // vmcnt(4) at R of phase 0 of tile t+1, group 1 with vmcnt(2) at R of phase 3
    // of tile t, each before the barrier that precedes the other group's reads.
    stage(0, 0);
    stage(3, 0);
    stage(1, 0);
    stage(2, 0);
    if (nk > 1) {
      stage(0, 1);
      stage(3, 1);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    lds_barrier();
    if (wr == 1) lds_barrier();   // stagger (wr is wave-uniform: readfirstlane)
    for (int t = 0; t < nk; ++t) {
      const int buf = t & 1;
      const char* sA0 = smem + (buf * 4 + 0) * HALF + aoff;
      const char* sA1 = smem + (buf * 4 + 1) * HALF + aoff;
      const char* sB0 = smem + (buf * 4 + 2) * HALF + boff;
      const char* sB1 = smem + (buf * 4 + 3) * HALF + boff;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (p == 0 && wr == 0 && t > 0) {
          if (t + 1 < nk)
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (p == 3 && wr == 1 && t + 1 < nk) {
          if (t + 2 < nk)
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
          else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const int qi = (p >= 2) ? 1 : 0;
        const int qj = (p == 1 || p == 2) ? 1 : 0;
        quadrant(qi ? sA1 : sA0, qj ? sB1 : sB0, qi, qj, p == 0 || p == 2, p != 2);
        if (p == 0 && t + 1 < nk) stage(1, t + 1);
        if (p == 1 && t + 1 < nk) stage(2, t + 1);
        if (p == 2 && t + 2 < nk) stage(0, t + 2);
        if (p == 3 && t + 2 < nk) stage(3, t + 2);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        lds_barrier();
        mfma_q(qi, qj);
        lds_barrier();
      }
    }
    if (wr == 0) lds_barrier();   // balance the stagger barrier
  } else if constexpr (SCHED == 0) {
    // prologue: A0(0) B1(0) A1(0) B0(0) A0(1) B1(1)
    stage(0, 0);
    stage(3, 0);
    stage(1, 0);
    stage(2, 0);
    if (nk > 1) {
      stage(0, 1);
      stage(3, 1);
    }
    for (int t = 0; t < nk; ++t) {
      const int buf = t & 1;
      const char* sA0 = smem + (buf * 4 + 0) * HALF + aoff;
      const char* sA1 = smem + (buf * 4 + 1) * HALF + aoff;
      const char* sB0 = smem + (buf * 4 + 2) * HALF + boff;
      const char* sB1 = smem + (buf * 4 + 3) * HALF + boff;
      if (t + 1 < nk)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        lds_barrier();
        const int qi = (p >= 2) ? 1 : 0;
        const int qj = (p == 1 || p == 2) ? 1 : 0;
        quadrant(qi ? sA1 : sA0, qj ? sB1 : sB0, qi, qj, p == 0 || p == 2);
        if (p == 0 && t + 1 < nk) stage(1, t + 1);
        if (p == 1 && t + 1 < nk) stage(2, t + 1);
        if (p == 2 && t + 2 < nk) stage(0, t + 2);
        if (p == 3 && t + 2 < nk) stage(3, t + 2);
        mfma_q(qi, qj);
      }
    }
  } else {
    // Fragment-prefetch schedule: all four fragment sets live (A0/A1 32 VGPRs,
    // B0/B1 16 each); each set is read from LDS one quadrant before its first
    // MFMA, so LDS reads run under the previous quadrant's MFMAs. Quadrant order
    // Q0=(A0,B0) Q1=(A0,B1) Q2=(A1,B0) Q3=(A1,B1) frees A0 after Q1 and B0 after
    // Q2, where the next K-tile's A0/B0 are prefetched. One barrier per K-tile
    // (mid-tile): it retires the next K-tile's LDS-DMA (RAW) and every read of
    // this K-tile's buffer (WAR) before the K-tile after next is issued into it.
    i16x8 a0[2][4], a1[2][4], b0[2][2], b1[2][2];
    auto rdA = [&](i16x8 (&d)[2][4], const char* sa) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        d[0][i] = *(const i16x8*)(sa + i * 2048 + sw0);
        d[1][i] = *(const i16x8*)(sa + i * 2048 + sw1);
      }
    };
    auto rdB = [&](i16x8 (&d)[2][2], const char* sb) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        d[0][j] = *(const i16x8*)(sb + j * 2048 + sw0);
        d[1][j] = *(const i16x8*)(sb + j * 2048 + sw1);
      }
    };
    auto mm = [&](const i16x8 (&a)[2][4], const i16x8 (&b)[2][2], int qi, int qj) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[qi][qj][i][j] = Mfma<T>::m16(a[s][i], b[s][j], acc[qi][qj][i][j]);
      __builtin_amdgcn_s_setprio(0);
    };
    auto stage_all = [&](int tile) {
      stage(0, tile);
      stage(2, tile);
      stage(1, tile);
      stage(3, tile);
    };
    auto slot = [&](int buf, int kind) -> const char* {
      return smem + (buf * 4 + kind) * HALF + (kind < 2 ? aoff : boff);
    };
    stage_all(0);
    if (nk > 1) {
      stage_all(1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    lds_barrier();
    rdA(a0, slot(0, 0));
    rdB(b0, slot(0, 2));
    for (int t = 0; t < nk; ++t) {
      const int buf = t & 1;
      rdB(b1, slot(buf, 3));
      rdA(a1, slot(buf, 1));
      mm(a0, b0, 0, 0);
      mm(a0, b1, 0, 1);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      lds_barrier();
      if (t + 2 < nk) stage_all(t + 2);
      if (t + 1 < nk) rdA(a0, slot(buf ^ 1, 0));
      mm(a1, b0, 1, 0);
      if (t + 1 < nk) rdB(b0, slot(buf ^ 1, 2));
      mm(a1, b1, 1, 1);
    }
  }

  if constexpr (REGEPI) {
    float4 bv[2][2];
    load_bias_regs(epi, n0, wc, lane, bv);
    epilogue_regs(acc, bv, m0, n0, wr, wc, lane, M, epi);
    return;
  }
  // Epilogue through LDS: two passes (quadrant row qi), each stages the WG's
  // 128 x 256 fp32 accumulator rows {wr*128 + qi*64 + 0..63} in LDS (row stride
  // 260 floats: the 4 fk row groups of a ds_write_b32 land on distinct banks),
  // then every wave streams whole 1-KiB rows out: 16-B loads/stores per lane,
  // bias hoisted per column, residual/activation applied on the way out.
  float* stg = (float*)smem;
  const int ec = (tid & 63) * 4;            // this thread's 4 output columns
  const float4 bv = epi.bias4(n0 + ec);
  const bool full = m0 + 256 <= M;
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    lds_barrier();
    i16x4 xr[16];
    if constexpr (PrefetchX<Epi>::value) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int lr = (tid >> 6) + 8 * k;
        const int row = m0 + (lr >> 6) * 128 + qi * 64 + (lr & 63);
        xr[k] = epi.load4(row < M ? row : M - 1, n0 + ec);
      }
    }
#pragma unroll
    for (int qj = 0; qj < 2; ++qj)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int lr = wr * 64 + i * 16 + fk * 4 + r;      // staged row 0..127
            const int lc = wc * 64 + qj * 32 + j * 16 + fr;    // col 0..255
            stg[lr * EPI_LD + lc] = acc[qi][qj][i][j][r];
          }
    lds_barrier();
    if constexpr (PrefetchX<Epi>::value) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int lr = (tid >> 6) + 8 * k;
        const int row = m0 + (lr >> 6) * 128 + qi * 64 + (lr & 63);
        if (full || row < M)
          epi.put4x(row, n0 + ec, *(const float4*)(stg + lr * EPI_LD + ec), bv, xr[k]);
      }
    } else if (full) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int lr = (tid >> 6) + 8 * k;                      // 0..127
        const int row = m0 + (lr >> 6) * 128 + qi * 64 + (lr & 63);
        epi.put4(row, n0 + ec, *(const float4*)(stg + lr * EPI_LD + ec), bv);
      }
    } else {
#pragma unroll 4
      for (int k = 0; k < 16; ++k) {
        const int lr = (tid >> 6) + 8 * k;
        const int row = m0 + (lr >> 6) * 128 + qi * 64 + (lr & 63);
        if (row < M) epi.put4(row, n0 + ec, *(const float4*)(stg + lr * EPI_LD + ec), bv);
      }
    }
  }
}


// ---------------------------------------------------------------------------
// Persistent staggered kernel with the LDS-staged epilogue (variant 259). One
// workgroup per CU walks tiles blockIdx.x + i*gridDim.x (the same XCD-grouped
// rounds as the one-tile-per-workgroup launch); per tile the main loop is
// SCHED 2 unchanged. What changes is the tile boundary:
//   * the epilogue stages 64 accumulator rows per pass (4 passes) in the
//     buffer-1 half of LDS, so buffer 0 is free: right after the main loop the
//     next tile's whole first K-tile is LDS-DMA'd into it (hidden from hipcc,
//     so it does not wait vmcnt(0) before the staging ds_reads), under the
//     epilogue;
//   * the workgroup does not end after its stores: they drain while the next
//     tile's main loop starts (a retiring wave waits for its stores).
// At the next tile: K-tile 1 is staged into buffer 1 (freed by the last pass's
// barrier) and `vmcnt(4 + stores)` retires the prefetched K-tile 0 -- `stores`
// is the epilogue's global stores per lane after the prefetch (32 for a full
// tile; 0 for a partial tile, i.e. a full wait), never more than were issued.
// The row tail runs at the end on the same workgroups (gemm_tail_wg tasks).
// ---------------------------------------------------------------------------
// global stores per lane issued after the next-tile prefetch: the last 3 of the
// 4 passes x 8 rows, or with transposed accumulators 2 passes x 8 16-B stores
template <class Epi, bool TR> struct EpiStores { static constexpr int n = TR ? 16 : 24; };
// fp16 residual, transposed: after the prefetch come pass 0's 8 stores, pass 1's
// 8 residual loads and its 8 stores
template <> struct EpiStores<EpiResidual<_Float16>, true> { static constexpr int n = 24; };
// output of the transposed-accumulator epilogue: C, or the residual stream X
template <class Epi> MICLIP_DEV auto* tr_out(const Epi& e) {
  if constexpr (PrefetchX<Epi>::value) return e.X; else return e.C;
}
template <class Epi> MICLIP_DEV int tr_ld(const Epi& e) {
  if constexpr (PrefetchX<Epi>::value) return e.ldx; else return e.ldc;
}
template <bool TR> struct EpiStores<EpiNull, TR> { static constexpr int n = 0; };

// {mean, rstd} of rows r0, r0+8, ..., r0+56 (wave-uniform r0, all in bounds) by
// scalar loads: SGPR results, the lgkm counter only -- a vector load here would
// make hipcc wait vmcnt(0), draining the next tile's LDS-DMA prefetch and the
// previous pass's stores. Reads only (nothing is written through the scalar cache).
MICLIP_DEV void sload_stats8(const float2* r0, float2 (&st)[8]) {
  const unsigned long long a = (unsigned long long)r0;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const unsigned long long base = ((unsigned long long)hi << 32) | lo;
  unsigned long long v0, v1, v2, v3, v4, v5, v6, v7;
  asm volatile(
      "s_load_dwordx2 %0, %8, 0x0\n\t"
      "s_load_dwordx2 %1, %8, 0x40\n\t"
      "s_load_dwordx2 %2, %8, 0x80\n\t"
      "s_load_dwordx2 %3, %8, 0xc0\n\t"
      "s_load_dwordx2 %4, %8, 0x100\n\t"
      "s_load_dwordx2 %5, %8, 0x140\n\t"
      "s_load_dwordx2 %6, %8, 0x180\n\t"
      "s_load_dwordx2 %7, %8, 0x1c0\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&s"(v0), "=&s"(v1), "=&s"(v2), "=&s"(v3), "=&s"(v4), "=&s"(v5), "=&s"(v6), "=&s"(v7)
      : "s"(base)
      : "memory");
  const unsigned long long v[8] = {v0, v1, v2, v3, v4, v5, v6, v7};
#pragma unroll
  for (int k = 0; k < 8; ++k) st[k] = __builtin_bit_cast(float2, v[k]);
}

MICLIP_DEV void wait_vmcnt_tile(int n) {
  switch (n) {
    case 36: asm volatile("s_waitcnt vmcnt(36)" ::: "memory"); break;
    case 32: asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); break;
    case 28: asm volatile("s_waitcnt vmcnt(28)" ::: "memory"); break;
    case 22: asm volatile("s_waitcnt vmcnt(22)" ::: "memory"); break;
    case 21: asm volatile("s_waitcnt vmcnt(21)" ::: "memory"); break;
    case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
    case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
    case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

template <typename T, class Epi, bool TRQ = true, int RB = 4>
__global__ __launch_bounds__(512) void gemm256s_kernel(const T* __restrict__ A,
                                                       const T* __restrict__ W, int M, int N,
                                                       int K, Epi epi, int gm, int ntm_dp,
                                                       int ntail, int tail_wide) {
  // transposed accumulators (TrAcc epilogues): MFMA operands swapped, so each
  // lane's accumulator holds 4 consecutive output columns of one output row
  constexpr bool TR = TRQ && TrAcc<Epi>::value;
  // RB = 16-row blocks per wave quadrant: 4 -> 256-row tiles (the default), 3 ->
  // 192-row, 2 -> 128-row tiles (transposed-accumulator epilogues only; the
  // launcher picks them where 256-row tiles would leave CUs idle, e.g. ViT-B/32's
  // N = 768 GEMMs at M = 12 800, ViT-L/14's N = 1024 ones at 32-64 images). Same
  // MFMA chains and epilogue arithmetic per element: a row's result does not
  // depend on the tile height.
  static_assert(RB == 4 || ((RB == 3 || RB == 2) && TR),
                "192- / 128-row tiles: TR epilogues only");
  constexpr int QR = RB * 16;            // rows of one wave quadrant
  constexpr int SR = 2 * QR;             // rows of one A half-tile slot (both wave rows)
  constexpr int TM = 2 * SR;             // tile rows
  constexpr int APC = SR / 8;            // 1-KiB A pieces per slot (16 or 12)
  constexpr int HALF = 128 * 128;        // bytes of one half-tile slot
  constexpr int EPI_LD = 260;            // fp32 row stride of the epilogue staging
  constexpr int STG = 4 * HALF;          // staging: 64 rows in the buffer-1 half onward
  constexpr int SMEM0 = 8 * HALF > STG + 64 * EPI_LD * 4 ? 8 * HALF : STG + 64 * EPI_LD * 4;
  // TR staging: 128 rows of 256 outputs at a 520-B pitch (8-B skew per row); it
  // fits where the fp32 staging sits
  constexpr int TLD = 520;
  static_assert(STG + 128 * TLD <= SMEM0, "TR staging");
  // folded LayerNorm (EpiStoreLN): the tile's column sums after the staging; TR:
  // the tile's bias and column sums [64] float4 and row statistics [256] float2
  constexpr int SMEM = SMEM0 + (TR ? (IsLN<Epi>::value ? 4096 : 1024) : (IsLN<Epi>::value ? 1024 : 0));
  __shared__ __attribute__((aligned(1024))) char smem[SMEM];
  float4* lncs = (float4*)(smem + SMEM0);              // [64] column sums
  float4* tbias = (float4*)(smem + SMEM0);             // TR: [64] bias
  float4* tcs = (float4*)(smem + SMEM0 + 1024);        // TR LN: [64] column sums
  float2* tst = (float2*)(smem + SMEM0 + 2048);        // TR LN: [256] {mean, rstd}

  const int ntn = N / 256, ntm = ntm_dp, ndp = ntm * ntn, nk = K / 64;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int lchunk = (lane & 7) ^ (lane >> 3);
  const int fr = lane & 15, fk = lane >> 4;
  const int aoff = (wr * QR + fr) * 128, boff = (wc * 32 + fr) * 128;
  const int sw0 = ((0 + fk) ^ (fr & 7)) << 4, sw1 = ((4 + fk) ^ (fr & 7)) << 4;
  const int ec = (tid & 63) * 4;

  // A pieces of a slot: RB 4: 16 = 2 per wave (pieces 2w, 2w+1); RB 3: 12 = wave w's
  // piece w and, for waves 0-3 (wave row 0), piece w + 8; RB 2: 8 = piece w -- so a
  // wave's op count per A stage is a function of its wave row (2 or 1), which the
  // counted waits use (APW0 / APW1: A ops per stage of wave rows 0 / 1)
  auto apiece = [&](int pp) { return RB == 4 ? wave * 2 + pp : wave + 8 * pp; };
  auto ahas = [&](int pp) { return RB == 4 || pp == 0 || (RB == 3 && wave < 4); };   // wave-uniform
  constexpr int APW0 = RB == 2 ? 1 : 2, APW1 = RB == 4 ? 2 : 1;
  const int apw = wr == 0 ? APW0 : APW1;   // wave-uniform
  // LDS-DMA sources of tile `id` (slot row sr = piece*8 + (lane>>3))
  auto sources = [&](int id, int& m0_, int& n0_, const T* (&as)[2][2], const T* (&bs)[2][2]) {
    int tm_, tn_;
    group_tile(xcd_remap(id, ndp), ntm, ntn, gm, tm_, tn_);
    m0_ = tm_ * TM;
    n0_ = tn_ * 256;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        // A piece apiece(pp) of slot h: slot rows 0..QR-1 are wave row 0's quadrant
        // rows h*QR.., QR..SR-1 wave row 1's (tile rows SR + h*QR ..)
        const int ap = apiece(pp);
        const int asr = (ap < APC ? ap : 0) * 8 + (lane >> 3);
        int ar = m0_ + (asr / QR) * SR + h * QR + (asr % QR);
        ar = ar < M ? ar : M - 1;
        as[h][pp] = A + (size_t)ar * K + lchunk * 8;
        const int sr = (wave * 2 + pp) * 8 + (lane >> 3);
        const int bc = n0_ + (sr >> 5) * 64 + h * 32 + (sr & 31);
        bs[h][pp] = W + (size_t)bc * K + lchunk * 8;
      }
  };
  int m0, n0;
  const T* asrc[2][2];
  const T* bsrc[2][2];
  // Main-loop pieces by buffer_load_dwordx4 ... lds from per-tile buffer resources:
  // 32-bit offsets from the tile's first row / column (8 VGPRs) instead of eight 64-bit
  // source pointers live across the K loop and a 64-bit add per piece -- the
  // folded-LN kernels no longer spill (13-16 VGPRs before); +1.3 % in the model
  // (3 interleaved rounds, CHANGELOG r5). Same bytes: rows past M stay clamped to row
  // M - 1 (sources), whose offset lies inside the tile's resource.
  __amdgpu_buffer_rsrc_t rsA, rsB;
  unsigned aoff32[2][2], boff32[2][2];
  auto tile_rsrc = [&]() {
    const T* ab = A + (size_t)m0 * K;
    const T* bb = W + (size_t)n0 * K;
    const long long ra = (long long)(M - m0) * K * (long long)sizeof(T);
    rsA = __builtin_amdgcn_make_buffer_rsrc((void*)ab, (short)0,
                                            (int)(ra < 0x7fffffffll ? ra : 0x7fffffffll), 0x00020000);
    rsB = __builtin_amdgcn_make_buffer_rsrc((void*)bb, (short)0, 256 * K * (int)sizeof(T), 0x00020000);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        aoff32[h][pp] = (unsigned)((asrc[h][pp] - ab) * sizeof(T));
        boff32[h][pp] = (unsigned)((bsrc[h][pp] - bb) * sizeof(T));
      }
  };
  auto stage = [&](int slot_kind, int tile) {
    const int buf = tile & 1, k0 = tile * 64;
    char* slot = smem + (buf * 4 + slot_kind) * HALF;
    const unsigned kb = (unsigned)k0 * (unsigned)sizeof(T);
    if (slot_kind < 2) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_AS void*)(slot + apiece(0) * 1024), 16,
                                               aoff32[slot_kind][0] + kb, 0, 0, 0);
      if (ahas(1))
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_AS void*)(slot + apiece(1) * 1024), 16,
                                                 aoff32[slot_kind][1] + kb, 0, 0, 0);
    } else {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_AS void*)(slot + wave * 2048), 16,
                                               boff32[slot_kind - 2][0] + kb, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_AS void*)(slot + wave * 2048 + 1024), 16,
                                               boff32[slot_kind - 2][1] + kb, 0, 0, 0);
    }
  };

  f32x4 acc[2][2][RB][2];
  i16x8 af[2][RB], bf[2][2];
  // phase 2 = (A1, B1) finds B1 still in bf from phase 1 (same K-tile buffer):
  // load_b = false there, 28 fragment reads per K-tile instead of 32
  auto quadrant = [&](const char* sa, const char* sb, bool load_a, bool load_b) {
    if (load_a) {
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        af[0][i] = *(const i16x8*)(sa + i * 2048 + sw0);
        af[1][i] = *(const i16x8*)(sa + i * 2048 + sw1);
      }
    }
    if (load_b) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bf[0][j] = *(const i16x8*)(sb + j * 2048 + sw0);
        bf[1][j] = *(const i16x8*)(sb + j * 2048 + sw1);
      }
    }
  };
  // FIRST (K-tile 0): the k-step-0 MFMAs take a zero accumulator operand (the
  // inline constant 0), so a tile needs no 128 v_mov zeroing its accumulators
  auto mfma_q = [&](int qi, int qj, auto first_c) {
    constexpr bool FIRST = decltype(first_c)::value;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f32x4 c = (FIRST && s == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[qi][qj][i][j];
          if constexpr (TR)   // C^T = W . A^T: lane (fk, fr) = row fr, columns 4fk .. 4fk+3
            acc[qi][qj][i][j] = Mfma<T>::m16(bf[s][j], af[s][i], c);
          else
            acc[qi][qj][i][j] = Mfma<T>::m16(af[s][i], bf[s][j], c);
        }
    __builtin_amdgcn_s_setprio(0);
  };

  int prev_stores = -1;   // -1: first tile (full prologue)
  int id = blockIdx.x;
  MICLIP_STAMP_BEGIN;
  if (id < ndp) sources(id, m0, n0, asrc, bsrc);
  for (; id < ndp; id += gridDim.x) {
    tile_rsrc();
    if constexpr (TR) {
      // This tile's epilogue operands (bias, and for the folded LN the column
      // sums and the 256 row statistics) go to LDS by DMA now, one 1-KiB piece
      // per wave 0-3, ahead of the K-tile stages: the main loop's first counted
      // wait (wr = 0 waves, K-tile 1) retires them and its barriers publish
      // them, so the tile boundary waits on no load. (Their last readers, the
      // previous tile's epilogue, are past its closing barrier.) The 512
      // statistics words go one per lane over the 8 waves, each row clamped to
      // M - 1 (rows past M are never stored). The lane offset is made opaque
      // so hipcc builds each 64-bit source address at its DMA instead of
      // hoisting (and spilling) it.
      int lo = lane;
      asm volatile("" : "+v"(lo));
      if (wave == 0) {
        if (epi.bias) {
          glds16_hidden(epi.bias + n0 + lo * 4, tbias);
        } else {
          float z;   // materialised here (a hoisted zero vector got spilled)
          asm volatile("v_mov_b32 %0, 0" : "=v"(z));
          tbias[lane] = make_float4(z, z, z, z);
        }
      }
      if constexpr (IsLN<Epi>::value) {
        if (wave == 1) glds16_hidden(epi.colsum + n0 + lo * 4, tcs);
        const int d = wave * 64 + lo, r = m0 + (d >> 1);
        if (RB == 4 || wave < TM / 32)   // TM rows x 2 words, 64 per wave
          glds4_hidden((const float*)(epi.stats + (r < M ? r : M - 1)) + (d & 1),
                       (const char*)tst + wave * 256);
      }
    }
    if (prev_stores < 0) {
      stage(0, 0);
      stage(3, 0);
      stage(1, 0);
      stage(2, 0);
      stage(0, 1);
      stage(3, 1);
      if (apw == 2)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else   // one A piece per stage (RB 3 wave row 1, RB 2)
        asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    } else {
      // K-tile 0 was prefetched during the previous epilogue
      stage(0, 1);
      stage(3, 1);
      wait_vmcnt_tile(2 + apw + prev_stores);
    }
    lds_barrier();
    if (wr == 1) lds_barrier();   // stagger (wave-uniform)
    MICLIP_STAMP(0);              // tile top: K-tile 0/1 staging and its wait
    auto ktile = [&](int t, auto first_c) {
      const int buf = t & 1;
      const char* sA0 = smem + (buf * 4 + 0) * HALF + aoff;
      const char* sA1 = smem + (buf * 4 + 1) * HALF + aoff;
      const char* sB0 = smem + (buf * 4 + 2) * HALF + boff;
      const char* sB1 = smem + (buf * 4 + 3) * HALF + boff;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        MICLIP_PSTAMP(7);   // the previous phase's closing barrier
        if (p == 0 && wr == 0 && t > 0) {
          MICLIP_KSTAMP(1);
          if (t + 1 < nk) {
            if constexpr (APW0 == 2)   // A0(t+1) + B1(t+1) may stay in flight
              asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else
              asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
          } else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          MICLIP_KSTAMP(6);
        }
        if (p == 3 && wr == 1 && t + 1 < nk) {
          MICLIP_KSTAMP(1);
          if (t + 2 < nk) {
            if constexpr (APW1 == 2)   // A0(t+2) may stay in flight: 2 ops (RB 3 / 2: 1)
              asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else
              asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
          } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          }
          MICLIP_KSTAMP(6);
        }
        const int qi = (p >= 2) ? 1 : 0;
        const int qj = (p == 1 || p == 2) ? 1 : 0;
        MICLIP_PSTAMP(6);   // vmcnt wait
        quadrant(qi ? sA1 : sA0, qj ? sB1 : sB0, p == 0 || p == 2, p != 2);
        MICLIP_PSTAMP(1);   // fragment reads (the stamp waits for them)
        if (p == 0 && t + 1 < nk) stage(1, t + 1);
        if (p == 1 && t + 1 < nk) stage(2, t + 1);
        if (p == 2 && t + 2 < nk) stage(0, t + 2);
        if (p == 3 && t + 2 < nk) stage(3, t + 2);
        MICLIP_PSTAMP(2);   // LDS-DMA issue
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        MICLIP_PSTAMP(3);
        lds_barrier();
        MICLIP_PSTAMP(4);   // barrier before the MFMAs
        mfma_q(qi, qj, first_c);
        MICLIP_PSTAMP(5);   // MFMA issue
        lds_barrier();
      }
    };
    ktile(0, std::true_type{});   // nk >= 2 (the launcher requires K >= 128)
    for (int t = 1; t < nk; ++t) ktile(t, std::false_type{});
    if (wr == 0) lds_barrier();   // balance the stagger barrier
    MICLIP_STAMP(1);              // main loop

    // ---- tile boundary: prefetch the next tile's K-tile 0 into buffer 0 ----
    lds_barrier();                 // every wave is done with both buffers
    const int cm0 = m0, cn0 = n0;
    // the bias is loaded and retired here, before anything is in flight: a
    // load left pending on some path makes hipcc wait vmcnt(0) at the next
    // tile's first MFMA that reuses its registers (draining the prefetch/stores)
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (!TR) {
      bv = epi.bias4nb(cn0 + ec);   // branch-free (null bias -> zeros)
      asm volatile("" ::"v"(bv.x), "v"(bv.y), "v"(bv.z), "v"(bv.w));
    }
    if constexpr (IsLN<Epi>::value && !TR) {
      // the tile's column sums, retired here like the bias and parked in LDS
      // (read after the first pass's barrier). The row statistics are wave-
      // uniform per output row (a wave stores whole rows) and come in by
      // scalar loads in the passes below.
      const float4 sv = epi.colsum4nb(cn0 + ec);
      asm volatile("" ::"v"(sv.x), "v"(sv.y), "v"(sv.z), "v"(sv.w));
      if (tid < 64) lncs[tid] = sv;
    }
    const int nid = id + gridDim.x;
    auto prefetch_next = [&]() {
      if (nid < ndp) {
        sources(nid, m0, n0, asrc, bsrc);
#pragma unroll
        for (int kind = 0; kind < 4; ++kind) {
          char* slot = smem + kind * HALF;
          if (kind < 2) {
            glds16_hidden(asrc[kind][0], slot + apiece(0) * 1024);
            if (ahas(1)) glds16_hidden(asrc[kind][1], slot + apiece(1) * 1024);
          } else {
            glds16_hidden(bsrc[kind - 2][0], slot + wave * 2048);
            glds16_hidden(bsrc[kind - 2][1], slot + wave * 2048 + 1024);
          }
        }
      }
    };
    // Issued inside the epilogue (TR: after the first pass's staging writes;
    // otherwise after the first pass's stores), not here: hipcc puts a vmcnt(0)
    // in front of the epilogue's first LDS read (it still counts the main
    // loop's compiler-visible LDS-DMA as in flight), and issued here that wait
    // also drained this prefetch -- every tile's epilogue started one DMA round
    // trip late.
    const bool full = cm0 + TM <= M;
    MICLIP_STAMP(2);              // tile boundary: epilogue operands, prefetch issue
    if constexpr (TR) {
      // ---- transposed-accumulator epilogue: 2 passes of 128 rows (qi: tile rows
      // wr*128 + qi*64 + 0..63). Every wave converts its own accumulators in
      // registers (val4 / val4ln: put4's exact operations on 4 consecutive
      // columns of one row) and writes the 8 output bytes with one ds_write_b64
      // into a row-major image (pitch 520 B: the 16 rows of one write group land
      // on 16 distinct 8-B bank slots); after the barrier each wave reads 16
      // image rows back (ds_read_b64, 512 contiguous bytes per row) and stores
      // them as 512-B row segments. fp16 staging: half the LDS bytes of the
      // fp32 row staging, and no wave idles while another half stages.
      char* img = smem + STG;
      // The epilogue operands are read from LDS up front -- the lane's 4 column
      // quads of bias / column sums once per tile, its 4 row statistics once per
      // pass -- before the pass's first staging write: a read placed after a
      // ds_write to the same array waits for that write (hipcc cannot tell them
      // apart), which serialised every 4-element group behind one LDS round trip
      // and kept the exp -> rcp chains of different groups from interleaving.
      float4 tb[2][2], tc[2][2];
#pragma unroll
      for (int qj = 0; qj < 2; ++qj)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int c4 = wc * 16 + qj * 8 + j * 4 + fk;     // this lane's column quad
          tb[qj][j] = tbias[c4];
          tc[qj][j] = make_float4(0.f, 0.f, 0.f, 0.f);
          if constexpr (IsLN<Epi>::value) tc[qj][j] = tcs[c4];
        }
#pragma unroll
      for (int qi = 0; qi < 2; ++qi) {
        if (qi > 0) lds_barrier();   // pass 0's readers are done with the image
        float2 ts[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          ts[i] = make_float2(0.f, 0.f);
          if constexpr (IsLN<Epi>::value) ts[i] = tst[wr * SR + qi * QR + i * 16 + fr];
        }
        // fp16 residual stream: the 8 x pieces this lane adds at readback (row
        // R + h of each pair, columns 8li .. 8li+7: 16 B, row-contiguous), loaded
        // now so their latency hides under the staging math (after the LDS reads
        // above: hipcc's vmcnt(0) in front of the epilogue's first LDS read would
        // otherwise wait for them)
        // readback rows per wave and pass: SR / 8 (16, or 12 for RB 3)
        constexpr int RPW = SR / 8;
        u32x4 xq[RPW / 2];
        if constexpr (PrefetchX<Epi>::value) {
#pragma unroll
          for (int k = 0; k < RPW / 2; ++k) {
            const int ir = wave * RPW + 2 * k + (lane >> 5);
            const int row = cm0 + (ir / QR) * SR + qi * QR + (ir % QR);
            xq[k] = *(const u32x4*)(epi.X + (size_t)(row < M ? row : M - 1) * epi.ldx + cn0 +
                                    (lane & 31) * 8);
          }
        }
#pragma unroll
        for (int qj = 0; qj < 2; ++qj)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int c4 = wc * 16 + qj * 8 + j * 4 + fk;   // this lane's column quad
#pragma unroll
            for (int i = 0; i < RB; ++i) {
              const int ir = wr * QR + i * 16 + fr;         // image row
              const f32x4 a = acc[qi][qj][i][j];
              const float4 v = make_float4(a[0], a[1], a[2], a[3]);
              i16x4 o;
              if constexpr (IsLN<Epi>::value)
                o = epi.val4ln(v, tb[qj][j], tc[qj][j], ts[i]);
              else
                o = epi.val4(v, tb[qj][j]);
              *(i16x4*)(img + ir * TLD + (c4 & 1) * 256 + (c4 >> 1) * 8) = o;
            }
          }
        if (qi == 0) {
          // the residual pieces are waited for before the prefetch is issued:
          // waiting for them behind it would wait for the prefetch too (vmcnt
          // retires in issue order)
          if constexpr (PrefetchX<Epi>::value) {
#pragma unroll
            for (int k = 0; k < RPW / 2; ++k) asm volatile("" ::"v"(xq[k]));
          }
          prefetch_next();   // before this pass's stores (prev_stores: EpiStores)
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        MICLIP_STAMP(5);              // epilogue math + staging writes
        lds_barrier();
        MICLIP_ESTAMP(6);             // staging barrier
        // readback: wave w stores image rows 16w .. 16w+15 in pairs (R, R+1). Lane
        // (h, li) reads the 8 bytes at image half h of both rows (columns 8li + 4h
        // .. +3); one v_permlane32_swap per dword then leaves lanes 0-31 with row R
        // columns 8li .. 8li+7 and lanes 32-63 with row R+1 (guide T21): 16-B
        // stores, each half-wave writing one whole 512-B row segment.
        const int h = lane >> 5, li = lane & 31;
        auto* cb = tr_out(epi) + cn0 + li * 8;
#pragma unroll
        for (int p0 = 0; p0 < RPW / 2; p0 += 2) {
          i16x4 va[2], vb[2];
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const int R = wave * RPW + 2 * (p0 + p);
            va[p] = *(const i16x4*)(img + R * TLD + h * 256 + li * 8);
            vb[p] = *(const i16x4*)(img + (R + 1) * TLD + h * 256 + li * 8);
          }
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(va[0]), "+v"(va[1]), "+v"(vb[0]), "+v"(vb[1]));
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const u32x2 a = __builtin_bit_cast(u32x2, va[p]), b = __builtin_bit_cast(u32x2, vb[p]);
            const auto s0 = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
            u32x4 w = {s0[0], s1[0], s0[1], s1[1]};
            if constexpr (PrefetchX<Epi>::value) {   // x + t, 8 fp16 pairs of adds
              unsigned t[4] = {w[0], w[1], w[2], w[3]};
              const unsigned x[4] = {xq[p0 + p][0], xq[p0 + p][1], xq[p0 + p][2], xq[p0 + p][3]};
              Epi::template add_x<4>(t, x);
              w = (u32x4){t[0], t[1], t[2], t[3]};
            }
            const int ir = wave * RPW + 2 * (p0 + p) + h;
            const int row = cm0 + (ir / QR) * SR + qi * QR + (ir % QR);
            if (full || row < M) *(u32x4*)(cb + (size_t)row * tr_ld(epi)) = w;
          }
        }
        MICLIP_STAMP(7);              // readback + store issue
      }
    } else {
    // ---- epilogue: 4 passes of 64 rows staged at STG ----
    float* stg = (float*)(smem + STG);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (p > 0) lds_barrier();
      i16x4 xr[8];
      f32x4 xf[8];
      if constexpr (PrefetchX<Epi>::value) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int row = cm0 + p * 64 + (tid >> 6) + 8 * k;
          xr[k] = epi.load4(row < M ? row : M - 1, cn0 + ec);
        }
      }
      if constexpr (PrefetchXF<Epi>::value) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int row = cm0 + p * 64 + (tid >> 6) + 8 * k;
          xf[k] = epi.load4f(row < M ? row : M - 1, cn0 + ec);
        }
      }
      if (wr == (p >> 1)) {
#pragma unroll
        for (int qj = 0; qj < 2; ++qj)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int lr = i * 16 + fk * 4 + r;               // 0..63
                const int lc = wc * 64 + qj * 32 + j * 16 + fr;   // 0..255
                stg[lr * EPI_LD + lc] = acc[p & 1][qj][i][j][r];
              }
      }
      lds_barrier();
      if constexpr (IsLN<Epi>::value) {
        // row k of this wave is cm0 + p*64 + wave + 8k for all its lanes: its
        // {mean, rstd} is a scalar load (SGPRs, no LDS round trip, no VGPRs),
        // so the 8 rows unroll fully and their staging reads overlap
        const float4 cs = lncs[tid & 63];
        if (full) {
          float2 st[8];
          sload_stats8(epi.stats + cm0 + p * 64 + wave, st);
          // 4 staged rows read back-to-back, one wait, then their math and stores
          // (hipcc otherwise waits out each read's latency right before its row)
#pragma unroll
          for (int k0 = 0; k0 < 8; k0 += 4) {
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = *(const f32x4*)(stg + (wave + 8 * (k0 + k)) * EPI_LD + ec);
            asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
#pragma unroll
            for (int k = 0; k < 4; ++k)
              epi.put4ln(cm0 + p * 64 + wave + 8 * (k0 + k), cn0 + ec,
                         make_float4(v[k][0], v[k][1], v[k][2], v[k][3]), bv, cs, st[k0 + k]);
          }
        } else {
          // partial tile (rare): clamped vector loads, rows past M skipped
#pragma unroll 2
          for (int k = 0; k < 8; ++k) {
            const int lr = wave + 8 * k;
            const int row = cm0 + p * 64 + lr;
            if (row < M)
              epi.put4ln(row, cn0 + ec, *(const float4*)(stg + lr * EPI_LD + ec), bv, cs,
                         epi.stats[row]);
          }
        }
      }
      if constexpr (!IsLN<Epi>::value) {
        auto emit = [&](int k, float4 v) {
          const int row = cm0 + p * 64 + wave + 8 * k;
          if constexpr (PrefetchX<Epi>::value)
            epi.put4x(row, cn0 + ec, v, bv, xr[k]);
          else if constexpr (PrefetchXF<Epi>::value)
            epi.put4xf(row, cn0 + ec, v, bv, xf[k]);
          else
            epi.put4(row, cn0 + ec, v, bv);
        };
        if (full) {
          // unguarded: 4 staged rows read back-to-back, one wait, then their
          // math and stores (a per-row guard makes hipcc branch per row and
          // wait out each read's latency right before it)
#pragma unroll
          for (int k0 = 0; k0 < 8; k0 += 4) {
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              v[k] = *(const f32x4*)(stg + (wave + 8 * (k0 + k)) * EPI_LD + ec);
            asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
#pragma unroll
            for (int k = 0; k < 4; ++k)
              emit(k0 + k, make_float4(v[k][0], v[k][1], v[k][2], v[k][3]));
          }
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int lr = wave + 8 * k;
            if (cm0 + p * 64 + lr < M) emit(k, *(const float4*)(stg + lr * EPI_LD + ec));
          }
        }
      }
      if constexpr (PrefetchX<Epi>::value) {   // retire every residual load on every path
#pragma unroll
        for (int k = 0; k < 8; ++k) asm volatile("" ::"v"(xr[k]));
      }
      if constexpr (PrefetchXF<Epi>::value) {
#pragma unroll
        for (int k = 0; k < 8; ++k) asm volatile("" ::"v"(xf[k]));
      }
      // after the first pass's stores: hipcc's counted waits for the residual
      // loads assume no hidden operation younger than them, so a prefetch issued
      // before them made the first pass wait for it too (prev_stores = 24)
      if (p == 0) prefetch_next();
    }
    }
    lds_barrier();                 // staging (buffer-1 half) free for the next tile
    // RB 3 / 2: 12 / 8 rows per wave and pass instead of 16 (TR epilogues only)
    prev_stores = full ? EpiStores<Epi, TR>::n * RB / 4 : 0;
    MICLIP_STAMP(3);              // epilogue
  }
  // the row tail on the same workgroups, from the last one down (the workgroups
  // with one tile fewer when the tiles are not a whole number of rounds)
  for (int task = gridDim.x - 1 - blockIdx.x; task < ntail; task += gridDim.x) {
    lds_barrier();
    if (tail_wide)
      gemm_tail_wg<T, Epi, 2, 128>(A, W, M, N, K, epi, ntm * TM, task, smem);
    else
      gemm_tail_wg<T, Epi, 1, 64>(A, W, M, N, K, epi, ntm * TM, task, smem);
  }
  MICLIP_STAMP(4);                // row tail
  MICLIP_STAMP_END(blockIdx.x * 8 + wave);
}


// ---------------------------------------------------------------------------
// Persistent form of the staggered 256x256 kernel (SCHED 2): one workgroup per
// CU walks its tiles (ids blockIdx.x + i*gridDim.x, so every round covers the
// same XCD-grouped tile range as the one-tile-per-workgroup launch) as ONE
// continuous K-tile stream g = 0 .. tiles*nk-1. The half-tile LDS-DMA
// pipeline runs straight across tile boundaries: during a tile's last K-tiles
// the next tile's first ones are already staged, so a tile costs no prologue
// latency. The epilogue reads the accumulators directly (epilogue_regs, no
// LDS), so it needs none of the pipeline's LDS and its stores drain while
// the next tile's first K-tile computes.
// vmcnt after an epilogue (group 0, phase 0 of the next K-tile): the ops
// younger than the data it needs are A0/B1 of the K-tile after (4) plus the
// epilogue's own loads/stores (EPI_OPS), so vmcnt(min(4 + EPI_OPS, 63))
// retires exactly (or, capped, slightly more than) what is needed.
// ---------------------------------------------------------------------------
template <class Epi> struct EpiOps { static constexpr int n = 32 + 4; };   // stores + next bias
template <typename R> struct EpiOps<EpiResidual<R>> { static constexpr int n = 64 + 4; };  // + x loads
template <typename R> struct EpiOps<EpiPatch<R>> { static constexpr int n = 64 + 4; };  // pos + stores
template <class Epi> struct IsPatch : std::false_type {};
template <typename R> struct IsPatch<EpiPatch<R>> : std::true_type {};

template <typename T, class Epi>
__global__ __launch_bounds__(512) void gemm256p_kernel(const T* __restrict__ A,
                                                       const T* __restrict__ W, int M, int N,
                                                       int K, Epi epi, int gm) {
  constexpr int HALF = 128 * 128;  // bytes of one half-tile slot
  __shared__ __attribute__((aligned(1024))) char smem[8 * HALF];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int ntn = N / 256, ntm = (M + 255) / 256, ntiles = ntm * ntn;
  const int G = gridDim.x, bid = blockIdx.x;
  const int my = (ntiles - bid + G - 1) / G;
  if (my <= 0) return;
  const int nk = K / 64, total = my * nk;

  auto tile_mn = [&](int li, int& m0, int& n0) {
    int tm, tn;
    group_tile(xcd_remap(bid + li * G, ntiles), ntm, ntn, gm, tm, tn);
    m0 = tm * 256;
    n0 = tn * 256;
  };
  int cur = 0, cm0, cn0, nm0 = 0, nn0 = 0;
  tile_mn(0, cm0, cn0);
  if (my > 1) tile_mn(1, nm0, nn0);

  const int lchunk = (lane & 7) ^ (lane >> 3);
  const int sr0 = (wave * 2) * 8 + (lane >> 3), sr1 = sr0 + 8;
  // stage half-tile `kind` (0:A0 1:A1 2:B0 3:B1) of global K-tile g (tile cur or cur+1)
  auto stage = [&](int kind, int g) {
    const bool nxt = g >= (cur + 1) * nk;
    const int m0s = nxt ? nm0 : cm0, n0s = nxt ? nn0 : cn0;
    const int k0 = (g - (nxt ? cur + 1 : cur) * nk) * 64;
    char* dst = smem + ((g & 1) * 4 + kind) * HALF + wave * 2048;
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const int sr = pp ? sr1 : sr0;
      const T* src;
      if (kind < 2) {
        int ar = m0s + (sr >> 6) * 128 + kind * 64 + (sr & 63);
        ar = ar < M ? ar : M - 1;
        src = A + (size_t)ar * K + lchunk * 8 + k0;
      } else {
        const int bc = n0s + (sr >> 5) * 64 + (kind - 2) * 32 + (sr & 31);
        src = W + (size_t)bc * K + lchunk * 8 + k0;
      }
      glds16(src, dst + pp * 1024);
    }
  };

  const int fr = lane & 15, fk = lane >> 4;
  const int aoff = (wr * 64 + fr) * 128, boff = (wc * 32 + fr) * 128;
  const int sw0 = ((0 + fk) ^ (fr & 7)) << 4, sw1 = ((4 + fk) ^ (fr & 7)) << 4;

  f32x4 acc[2][2][4][2];
  auto zero = [&]() {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  zero();
  // the tile's bias columns, loaded at the tile's start so the epilogue has
  // no load of its own (hipcc counts these against the visible LDS-DMA exactly)
  float4 bv[2][2];
  load_bias_regs(epi, cn0, wc, lane, bv);
  i16x8 af[2][4], bf[2][2];
  // phase 2 = (A1, B1) finds B1 still in bf from phase 1 (same K-tile buffer):
  // load_b = false there, 28 fragment reads per K-tile instead of 32
  auto quadrant = [&](const char* sa, const char* sb, bool load_a, bool load_b) {
    if (load_a) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[0][i] = *(const i16x8*)(sa + i * 2048 + sw0);
        af[1][i] = *(const i16x8*)(sa + i * 2048 + sw1);
      }
    }
    if (load_b) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bf[0][j] = *(const i16x8*)(sb + j * 2048 + sw0);
        bf[1][j] = *(const i16x8*)(sb + j * 2048 + sw1);
      }
    }
  };
  auto mfma_q = [&](int qi, int qj) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[qi][qj][i][j] = Mfma<T>::m16(af[s][i], bf[s][j], acc[qi][qj][i][j]);
    __builtin_amdgcn_s_setprio(0);
  };

  // prologue: A0(0) B1(0) A1(0) B0(0) A0(1) B1(1) (SCHED 2 order)
  stage(0, 0);
  stage(3, 0);
  stage(1, 0);
  stage(2, 0);
  if (total > 1) {
    stage(0, 1);
    stage(3, 1);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  lds_barrier();
  if (wr == 1) lds_barrier();   // stagger: waves 4-7 one barrier behind
  bool after_epi = false;
  for (int g = 0; g < total; ++g) {
    const int buf = g & 1;
    const char* sA0 = smem + (buf * 4 + 0) * HALF + aoff;
    const char* sA1 = smem + (buf * 4 + 1) * HALF + aoff;
    const char* sB0 = smem + (buf * 4 + 2) * HALF + boff;
    const char* sB1 = smem + (buf * 4 + 3) * HALF + boff;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (p == 0 && wr == 0 && g > 0) {
        if (g + 1 >= total)
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (after_epi)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(EpiOps<Epi>::n + 4 < 63 ? EpiOps<Epi>::n + 4 : 63)
                       : "memory");
        else
          asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      }
      if (p == 3 && wr == 1 && g + 1 < total) {
        if (g + 2 < total)
          asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      const int qi = (p >= 2) ? 1 : 0;
      const int qj = (p == 1 || p == 2) ? 1 : 0;
      quadrant(qi ? sA1 : sA0, qj ? sB1 : sB0, p == 0 || p == 2, p != 2);
      if (p == 0 && g + 1 < total) stage(1, g + 1);
      if (p == 1 && g + 1 < total) stage(2, g + 1);
      if (p == 2 && g + 2 < total) stage(0, g + 2);
      if (p == 3 && g + 2 < total) stage(3, g + 2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      lds_barrier();
      mfma_q(qi, qj);
      lds_barrier();
    }
    after_epi = false;
    if (g + 1 == (cur + 1) * nk) {   // last K-tile of this tile
      // The bias loads were issued a whole tile ago; retire them here by hand,
      // naming them as asm outputs, so hipcc sees them defined and emits no
      // vmcnt(0) (which would also drain the next tile's in-flight LDS-DMA).
      // vmcnt(63) only waits for ops older than the 63 youngest.
      {
        f32x4 b0 = {bv[0][0].x, bv[0][0].y, bv[0][0].z, bv[0][0].w};
        f32x4 b1 = {bv[0][1].x, bv[0][1].y, bv[0][1].z, bv[0][1].w};
        f32x4 b2 = {bv[1][0].x, bv[1][0].y, bv[1][0].z, bv[1][0].w};
        f32x4 b3 = {bv[1][1].x, bv[1][1].y, bv[1][1].z, bv[1][1].w};
        asm volatile("s_waitcnt vmcnt(63)" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
        bv[0][0] = make_float4(b0[0], b0[1], b0[2], b0[3]);
        bv[0][1] = make_float4(b1[0], b1[1], b1[2], b1[3]);
        bv[1][0] = make_float4(b2[0], b2[1], b2[2], b2[3]);
        bv[1][1] = make_float4(b3[0], b3[1], b3[2], b3[3]);
      }
      epilogue_regs(acc, bv, cm0, cn0, wr, wc, lane, M, epi);
      zero();
      ++cur;
      cm0 = nm0;
      cn0 = nn0;
      if (cur + 1 < my) tile_mn(cur + 1, nm0, nn0);
      if (cur < my) load_bias_regs(epi, cn0, wc, lane, bv);
      after_epi = true;
    }
  }
  if (wr == 0) lds_barrier();   // balance the stagger barrier
}

// Which kernel runs, with which tile height, grid and row-tail split, is plan_gemm's
// decision (gemm_plan.h); this only carries it out, one launch per GemmKernel. The
// cases an epilogue has no kernel for stay behind `if constexpr`: plan_gemm never
// names them for such an epilogue.
template <typename T, class Epi>
hipError_t launch(const void* A, const void* W, int M, int N, int K, Epi epi, hipStream_t s,
                  int variant = 0, float* skws = nullptr, int sk = 1) {
  GemmPlan p;
  if (!plan_gemm(M, N, K, variant, sk, skws != nullptr, TrAcc<Epi>::value, IsPatch<Epi>::value,
                 cu_count(), &p))
    return hipErrorInvalidValue;
  const T* a = (const T*)A;
  const T* w = (const T*)W;
  const dim3 grid(p.grid), block(p.block);
#define MICLIP_GEMM_LAUNCH(kernel, ...) \
  hipLaunchKernelGGL(kernel, grid, block, 0, s, a, w, M, N, K, epi, ##__VA_ARGS__)
  switch (p.kernel) {
    case kGemmSplitK:
      hipLaunchKernelGGL((gemm_nt_splitk_kernel<T>), dim3(p.grid, sk), block, 0, s, a, w, M, N, K,
                         K / sk, skws);
      hipLaunchKernelGGL((splitk_reduce_kernel<Epi>), dim3(p.reduce_grid), dim3(256), 0, s,
                         (const float*)skws, sk, M, N, epi);
      break;
    case kGemmTile128:
      MICLIP_GEMM_LAUNCH((gemm_nt_kernel<T, 128, 128, Epi>));
      break;
    case kGemmTile256S0:
      MICLIP_GEMM_LAUNCH((gemm256_kernel<T, Epi, 0>), p.gm, p.ntm_dp, p.wide);
      break;
    case kGemmTile256S1:
      MICLIP_GEMM_LAUNCH((gemm256_kernel<T, Epi, 1>), p.gm, p.ntm_dp, p.wide);
      break;
    case kGemmTile256S2:
      MICLIP_GEMM_LAUNCH((gemm256_kernel<T, Epi, 2>), p.gm, p.ntm_dp, p.wide);
      break;
    case kGemmTile256S2Regs:
      MICLIP_GEMM_LAUNCH((gemm256_kernel<T, Epi, 2, true>), p.gm, p.ntm_dp, p.wide);
      break;
    case kGemmPersist256P:
      MICLIP_GEMM_LAUNCH((gemm256p_kernel<T, Epi>), p.gm);
      break;
    case kGemmRows256:
      MICLIP_GEMM_LAUNCH((gemm256s_kernel<T, Epi>), p.gm, p.ntm_dp, p.wgs, p.wide);
      break;
    case kGemmRows256Staged:
      if constexpr (TrAcc<Epi>::value)
        MICLIP_GEMM_LAUNCH((gemm256s_kernel<T, Epi, false>), p.gm, p.ntm_dp, p.wgs, p.wide);
      break;
    case kGemmRows192:
      if constexpr (TrAcc<Epi>::value && !IsPatch<Epi>::value)
        MICLIP_GEMM_LAUNCH((gemm256s_kernel<T, Epi, true, 3>), p.gm, p.ntm_dp, p.wgs, p.wide);
      break;
    case kGemmRows128:
      if constexpr (TrAcc<Epi>::value && !IsPatch<Epi>::value)
        MICLIP_GEMM_LAUNCH((gemm256s_kernel<T, Epi, true, 2>), p.gm, p.ntm_dp, p.wgs, p.wide);
      break;
  }
#undef MICLIP_GEMM_LAUNCH
  return hipGetLastError();
}

}  // namespace

// non-temporal stores of the GEMM output: measured level (A/B diagnostic), off
constexpr int gemm_nt() { return 0; }

template <typename T>
hipError_t gemm_store_t(const void* A, const void* W, const float* bias, void* C, int M, int N,
                        int K, int act, hipStream_t s, int v, float* skws, int sk) {
  const int nt = gemm_nt();
  switch (act) {
    case ACT_NONE:
      return launch<T>(A, W, M, N, K, EpiStore<T, ACT_NONE>{(T*)C, bias, N, nt}, s, v, skws, sk);
    case ACT_QUICKGELU:
      return launch<T>(A, W, M, N, K, EpiStore<T, ACT_QUICKGELU>{(T*)C, bias, N, nt}, s, v, skws, sk);
    case ACT_GELU:
      return launch<T>(A, W, M, N, K, EpiStore<T, ACT_GELU>{(T*)C, bias, N, nt}, s, v, skws, sk);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t gemm_store(int dtype, const void* A, const void* W, const float* bias, void* C, int M,
                      int N, int K, int act, hipStream_t s, int v, float* skws, int sk) {
  if (dtype == kF16) return gemm_store_t<_Float16>(A, W, bias, C, M, N, K, act, s, v, skws, sk);
  return gemm_store_t<__bf16>(A, W, bias, C, M, N, K, act, s, v, skws, sk);
}

template <typename T>
hipError_t gemm_store_ln_t(const void* A, const void* W, const float* c, const float* colsum,
                           const void* stats, void* C, int M, int N, int K, int act,
                           hipStream_t s, int v, float* skws, int sk) {
  const float2* st = (const float2*)stats;
  switch (act) {
    case ACT_NONE:
      return launch<T>(A, W, M, N, K, EpiStoreLN<T, ACT_NONE>{(T*)C, c, colsum, st, N}, s, v, skws, sk);
    case ACT_QUICKGELU:
      return launch<T>(A, W, M, N, K, EpiStoreLN<T, ACT_QUICKGELU>{(T*)C, c, colsum, st, N}, s,
                       v, skws, sk);
    case ACT_GELU:
      return launch<T>(A, W, M, N, K, EpiStoreLN<T, ACT_GELU>{(T*)C, c, colsum, st, N}, s, v, skws, sk);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t gemm_store_ln(int dtype, const void* A, const void* W, const float* c,
                         const float* colsum, const void* stats, void* C, int M, int N, int K,
                         int act, hipStream_t s, int v, float* skws, int sk) {
  if (!c || !colsum || !stats) return hipErrorInvalidValue;
  if (dtype == kF16)
    return gemm_store_ln_t<_Float16>(A, W, c, colsum, stats, C, M, N, K, act, s, v, skws, sk);
  return gemm_store_ln_t<__bf16>(A, W, c, colsum, stats, C, M, N, K, act, s, v, skws, sk);
}

hipError_t gemm_residual(int dtype, const void* A, const void* W, const float* bias, void* X,
                         int M, int N, int K, hipStream_t s, int v, int resid16, float* skws,
                         int sk) {
  if (resid16) {  // fp16 residual stream (fp16 or bf16 operands)
    if (dtype == kBF16)
      return launch<__bf16>(A, W, M, N, K, EpiResidual<_Float16>{(_Float16*)X, bias, N}, s, v,
                            skws, sk);
    return launch<_Float16>(A, W, M, N, K, EpiResidual<_Float16>{(_Float16*)X, bias, N}, s, v,
                            skws, sk);
  }
  if (dtype == kF16)
    return launch<_Float16>(A, W, M, N, K, EpiResidual<float>{(float*)X, bias, N}, s, v, skws,
                            sk);
  return launch<__bf16>(A, W, M, N, K, EpiResidual<float>{(float*)X, bias, N}, s, v, skws, sk);
}

hipError_t gemm_f32(int dtype, const void* A, const void* W, const float* bias, float* C, int M,
                    int N, int K, hipStream_t s, int v) {
  if (dtype == kF16) return launch<_Float16>(A, W, M, N, K, EpiF32{C, bias, N}, s, v);
  return launch<__bf16>(A, W, M, N, K, EpiF32{C, bias, N}, s, v);
}

hipError_t gemm_null(int dtype, const void* A, const void* W, float* C, int M, int N, int K,
                     hipStream_t s, int v) {
  if (dtype == kF16) return launch<_Float16>(A, W, M, N, K, EpiNull{C, 0}, s, v);
  return launch<__bf16>(A, W, M, N, K, EpiNull{C, 0}, s, v);
}

hipError_t gemm_patch(int dtype, const void* A, const void* W, const float* pos, void* X, int M,
                      int N, int K, int np, hipStream_t s, int resid16, int variant) {
  if (np <= 0 || M % np) return hipErrorInvalidValue;
  if (resid16) {   // patch embedding into the fp16 stream (fp16 or bf16 operands)
    if (dtype == kBF16)
      return launch<__bf16>(A, W, M, N, K, EpiPatch<_Float16>{(_Float16*)X, pos, N, np}, s,
                            variant);
    return launch<_Float16>(A, W, M, N, K, EpiPatch<_Float16>{(_Float16*)X, pos, N, np}, s,
                            variant);
  }
  if (dtype == kF16)
    return launch<_Float16>(A, W, M, N, K, EpiPatch<float>{(float*)X, pos, N, np}, s, variant);
  return launch<__bf16>(A, W, M, N, K, EpiPatch<float>{(float*)X, pos, N, np}, s, variant);
}

}  // namespace miclip
