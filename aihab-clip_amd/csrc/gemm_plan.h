// Which GEMM kernel serves which shape: the launcher's decision as a pure function of
// (M, N, K, variant, sk, epilogue class, CU count). Plain C++17 with no HIP type or call, so
// a host compiler takes it alone and a CPU test can sweep it (miclip_gemm_plan).
// gemm.hip's launch() asks plan_gemm for a GemmPlan and switches on its kernel; nothing
// else decides a kernel, a tile height, a grid or a row-tail split.
#pragma once

namespace miclip {

// Kernel variants and schedule switches are chosen by the op-level `variant`
// argument only (miclip_op_gemm: A/B benches); the model path runs variant 0,
// which picks by problem size. The library reads no environment variables.
// Tile-row group of the 256x256 kernel's grouped order (default 4; a variant >=
// 1000 carries another in its thousands digit).
constexpr int gemm_group() { return 4; }

// kGemmNoTail: every row in 256x256 tiles, no row-tail split (A/B benches).
constexpr int kGemmNoTail = 1 << 16;
// kGemmTailFirst: tail workgroups interleaved with the first tiles
// (gemm256_kernel, block roles)
constexpr int kGemmTailFirst = 1 << 17;
// kGemmStagger: 8-us round stagger, see gemm256_kernel
constexpr int kGemmStagger = 1 << 18;
// kGemmTrAccOff: the persistent kernel's fp32 row-staging epilogue instead of the
// transposed-accumulator one for EpiStore / EpiStoreLN (A/B)
constexpr int kGemmTrAccOff = 1 << 21;

// Split of a 256x256 launch into whole rounds of tiles plus a row tail
// (gemm_tail_wg). The tile-rows kept in tiles are the largest multiple of
// ncu / gcd(ntn, ncu) -- the tile count is then a whole number of rounds --
// provided at most 256 rows are left over; otherwise every row stays in tiles.
struct TailPlan {
  int ntm_dp, wgs, wide;
};

inline TailPlan plan_tail(int M, int N, int ncu, int TM = 256) {
  const int ntm = (M + TM - 1) / TM, ntn = N / 256;
  int a = ntn, b = ncu;
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  const int step = ncu / a;
  const int ntm_dp = ntm / step * step;
  const int rows = M - ntm_dp * TM;
  if (ntm_dp == 0 || rows <= 0 || rows > 256 || N % 64) return TailPlan{ntm, 0, 0};
  // gemm_tail_wg tasks: 32 x 128 or 16 x 64, whichever ends sooner: the tail
  // adds (tasks per workgroup) x (task time) to the launch, and a wide task
  // takes ~1.5x a narrow one (in-kernel stamps, K = 1024: 19.6k vs 12.8k cycles;
  // ViT-L/14 QKV at M = 32896: 384 narrow tasks = 2 per workgroup -> 96 wide
  // ones, the tail's share of the launch 5.2 -> 2.1 %)
  const int wide_tasks = (rows + 31) / 32 * (N / 128);
  const int narrow_tasks = (rows + 15) / 16 * (N / 64);
  const int wide_cost = (wide_tasks + ncu - 1) / ncu * 3;
  const int narrow_cost = (narrow_tasks + ncu - 1) / ncu * 2;
  if (N % 128 == 0 && wide_cost < narrow_cost) return TailPlan{ntm_dp, wide_tasks, 1};
  return TailPlan{ntm_dp, narrow_tasks, 0};
}

// Row plan of the persistent kernel: where a launch of 256-row tiles is a single
// partial round, the smallest tile height whose tiles still fit one round -- 128
// rows, else 192 -- otherwise 256-row tiles with the row tail (plan_tail). Every
// plan gives each row the same MFMA k order and epilogue functor, so the choice (a
// function of M) never changes a result bit. Measured op-level, interleaved rounds
// (profiles/r06/rows/rows_ops.jsonl): a 128- / 192-row tile costs 0.69-0.81 / 0.84-0.90
// of a 256-row one (its DMA pieces per K-tile shrink to 3/4 / 7/8, not 1/2 / 3/4),
// so splitting into two rounds or adding tail tasks to one round of smaller tiles
// never paid (ViT-L/14 at 32 images, out-proj: 192-row 0.0255 ms, 128-row + tail
// 0.0294, two rounds of 128-row 0.0378, 256-row 0.0284).
struct RowPlan {
  int rb;
  TailPlan tp;
};

inline RowPlan choose_rows(int M, int N, int ncu) {
  const int ntn = N / 256;
  if (((M + 255) / 256) * ntn <= ncu) {
    if (((M + 127) / 128) * ntn <= ncu) return RowPlan{2, TailPlan{(M + 127) / 128, 0, 0}};
    if (((M + 191) / 192) * ntn <= ncu) return RowPlan{3, TailPlan{(M + 191) / 192, 0, 0}};
  }
  return RowPlan{4, plan_tail(M, N, ncu, 256)};
}

// K in whole 64-wide K-tiles (BK), N in whole 128-column tiles
inline bool gemm_shape_ok(int M, int N, int K) {
  return M >= 1 && N >= 128 && K >= 64 && N % 128 == 0 && K % 64 == 0;
}

// What launch() can launch: one value per hipLaunchKernelGGL site (the values are part
// of miclip_gemm_plan's interface, include/miclip.h)
enum GemmKernel {
  kGemmSplitK = 0,        // gemm_nt_splitk_kernel + splitk_reduce_kernel
  kGemmTile128 = 1,       // gemm_nt_kernel 128x128
  kGemmTile256S0 = 2,     // gemm256_kernel SCHED 0
  kGemmTile256S1 = 3,     // gemm256_kernel SCHED 1
  kGemmTile256S2 = 4,     // gemm256_kernel SCHED 2, LDS-staged epilogue
  kGemmTile256S2Regs = 5, // gemm256_kernel SCHED 2, register epilogue
  kGemmPersist256P = 6,   // gemm256p_kernel
  kGemmRows256 = 7,       // gemm256s_kernel RB 4, TRQ on
  kGemmRows256Staged = 8, // gemm256s_kernel RB 4, TRQ off (fp32 row staging)
  kGemmRows192 = 9,       // gemm256s_kernel RB 3
  kGemmRows128 = 10       // gemm256s_kernel RB 2
};

// One launch: `grid` x `block` threads of `kernel`; gm, ntm_dp, wgs and wide are the
// kernel arguments of the same names (0 where the kernel takes none). Split-K launches
// grid x sk workgroups, then reduce_grid workgroups of the reduction.
struct GemmPlan {
  int kernel, grid, block, gm, ntm_dp, wgs, wide;
  unsigned reduce_grid;
};

// `variant` taken apart: the kernel code, the tile-row group and the four flag bits
struct GemmVariant {
  int code, group;
  bool no_tail, tail_first, stagger, tracc_off;
};

inline GemmVariant decode_variant(int variant) {
  const int v = variant & ~(kGemmNoTail | kGemmTailFirst | kGemmStagger | kGemmTrAccOff);
  return GemmVariant{v % 1000, v >= 1000 ? v / 1000 : gemm_group(),
                     (variant & kGemmNoTail) != 0, (variant & kGemmTailFirst) != 0,
                     (variant & kGemmStagger) != 0, (variant & kGemmTrAccOff) != 0};
}

inline bool gemm_code_known(int c) {   // an explicit variant never falls back silently
  return c == 0 || c == 3 || (c >= 128 && c <= 130) || c == 192 || (c >= 256 && c <= 260);
}

// The plan of launch<T, Epi>(M, N, K, variant, sk): tracc = TrAcc<Epi> (EpiStore,
// EpiStoreLN, the fp16 residual), patch = IsPatch<Epi>, has_ws = a split-K workspace was
// given. False exactly where the launcher refuses (hipErrorInvalidValue).
inline bool plan_gemm(int M, int N, int K, int variant, int sk, bool has_ws, bool tracc,
                      bool patch, int ncu, GemmPlan* plan) {
  if (!gemm_shape_ok(M, N, K)) return false;
  // split-K (small M, long K: the CLS-only last block), deterministic. Decided before
  // the variant is looked at: with sk > 1 any variant, a bad one included, is ignored.
  if (sk > 1) {
    if (!has_ws || K % (sk * 64) || N % 128) return false;
    const long long n4 = (long long)M * (N / 4);
    *plan = GemmPlan{kGemmSplitK, ((M + 127) / 128) * (N / 128), 256, 0, 0, 0, 0,
                     (unsigned)((n4 + 255) / 256)};
    return true;
  }
  const GemmVariant v = decode_variant(variant);
  if (!gemm_code_known(v.code)) return false;

  const int ntn = N / 256;
  // the persistent kernels need whole 256-column tiles and >= 2 K-tiles (the stream stages
  // at most one tile ahead); the patch-embed epilogue keeps the one-tile-per-workgroup kernel
  const bool persist_ok = !patch && N % 256 == 0 && K >= 128;
  // 192- / 128-row tiles exist for the transposed-accumulator epilogues only, so
  // kGemmTrAccOff switches them off, forced or chosen
  const bool rows_ok = persist_ok && tracc && !v.tracc_off;
  const bool half_round256 = 2 * ((M + 255) / 256) * ntn >= ncu;
  const bool half_round128 = 2 * ((M + 127) / 128) * ntn >= ncu;   // implied by half_round256
  // a persistent launch: as many workgroups as tiles or tail tasks, one per CU at most
  auto persistent = [&](int kernel, TailPlan tp) {
    const int ndp = tp.ntm_dp * ntn;
    const int want = ndp > tp.wgs ? ndp : tp.wgs;
    *plan = GemmPlan{kernel, want < ncu ? want : ncu, 512, v.group, tp.ntm_dp, tp.wgs,
                     tp.wide & 1, 0};
    return true;
  };
  const TailPlan whole256{(M + 255) / 256, 0, 0};

  // Code 0, the model's: resolved by size to one of the explicit codes below.
  // Default for full-size problems: the persistent staggered kernel (variant
  // 259; same-process A/B vs 258 on the ViT-L/14 shapes: QKV +1 %, out-proj +9 %,
  // c_fc +1 %, c_proj +1 %)
  // (from half a round of 256x256 tiles up: ViT-B/32 bs=128 QKV 225 tiles 0.047 ->
  // 0.028 ms, out-proj bs=256 150 tiles 0.051 -> 0.028 ms vs the 128x128 kernel)
  // Smaller row tiles (gemm256s_kernel RB 3 / 2, transposed-accumulator epilogues)
  // where 256-row tiles leave CUs idle for part of the launch (choose_rows; e.g.
  // ViT-B/32 bs=256 out-proj / c_proj: 150 -> 201 tiles of 192 rows on 256 CUs;
  // ViT-L/14 at 32 images, M = 8224, N = 1024: 132 tiles of 256 rows -> 256 of 128
  // plus the 32-row tail). The persistent kernel also takes launches below half a
  // round of 256-row tiles when 128-row tiles fill one (at 16 images).
  // Large problems otherwise: 256x256 tile (1 WG/CU, L2-friendly arithmetic intensity);
  // small ones (text tower, tiny batches) keep more workgroups with 128x128.
  int code = v.code;
  if (code == 0) {
    if (rows_ok && half_round128) {
      const RowPlan rp = choose_rows(M, N, ncu);
      if (rp.rb == 3) return persistent(kGemmRows192, rp.tp);
      if (rp.rb == 2) return persistent(kGemmRows128, rp.tp);
      code = 259;   // 256-row tiles won: persistent kernel
    } else if (persist_ok && half_round256) {
      code = 259;
    } else {
      code = N % 256 == 0 && half_round256 ? 258 : 128;
    }
  }

  switch (code) {
    // forced 192-row tiles / 128-row tiles / 128-row tiles + row tail: refused where the
    // smaller tiles do not exist. kGemmNoTail does not reach 130.
    case 192: case 129: case 130:
      if (!rows_ok) return false;
      if (code == 192) return persistent(kGemmRows192, TailPlan{(M + 191) / 192, 0, 0});
      return persistent(kGemmRows128, code == 129 ? TailPlan{(M + 127) / 128, 0, 0}
                                                  : plan_tail(M, N, ncu, 128));
    // persistent staggered kernel, LDS-staged epilogue + next-tile prefetch; kGemmTrAccOff
    // means something to a transposed-accumulator epilogue only
    case 259:
      if (persist_ok)
        return persistent(tracc && v.tracc_off ? kGemmRows256Staged : kGemmRows256,
                          v.no_tail ? whole256 : plan_tail(M, N, ncu));
      break;   // not applicable: an explicit 259 runs the one-tile kernel on SCHED 2 (forced)
    // persistent 256x256
    case 3:
      if (persist_ok) {
        const int tiles = ((M + 255) / 256) * ntn;
        *plan = GemmPlan{kGemmPersist256P, tiles < ncu ? tiles : ncu, 512, v.group, 0, 0, 0, 0};
        return true;
      }
      break;   // not applicable: an explicit 3 runs what the size test below picks
    default:
      break;
  }

  // One tile per workgroup. 256 .. 260 force the 256x256 kernel wherever N allows it
  // (elsewhere they run the 128x128 one); 3 takes it from half a round of tiles up.
  // The staggered schedule (SCHED 2) with the LDS-staged epilogue (full 512-B / 1-KiB
  // row stores) for every epilogue; 260 = the register epilogue, 256 / 257 = SCHED 0 / 1.
  // (The fp32 residual register epilogue was ~5 % faster with inline-asm x loads, but
  // an asm load's destination is free for hipcc to reuse before the data lands: it
  // faulted intermittently, so it is gone.)
  if (N % 256 == 0 && code != 128 && (code >= 256 || half_round256)) {
    TailPlan tp = v.no_tail ? whole256 : plan_tail(M, N, ncu);
    // kGemmTailFirst and kGemmStagger act on gemm256_kernel only
    if (tp.wgs && v.tail_first) {
      tp.wgs = (tp.wgs + 7) / 8 * 8;   // interleaved 8 per 16 blocks
      tp.wide |= 2;
    }
    if (v.stagger && tp.ntm_dp * ntn >= 2 * ncu) tp.wide |= 8 << 8;   // 8 us per round
    const int kernel = code == 260   ? kGemmTile256S2Regs
                       : code == 257 ? kGemmTile256S1
                       : code == 256 ? kGemmTile256S0
                                     : kGemmTile256S2;
    *plan = GemmPlan{kernel, tp.ntm_dp * ntn + tp.wgs, 512, v.group, tp.ntm_dp, tp.wgs, tp.wide, 0};
    return true;
  }
  *plan = GemmPlan{kGemmTile128, ((M + 127) / 128) * (N / 128), 256, 0, 0, 0, 0, 0};
  return true;
}

}  // namespace miclip
