"""float64 restatement of the GEMM family (csrc/gemm.hip, csrc/epilogue.h) and of the
patch-embedding / class-token / gathered-LayerNorm ops next to it: the yardstick of
tests/test_gpu_gemm_exact.py, checked on the CPU by tests/test_gemm_ref.py. Plain torch
(float64 unless a rounding is the point); it calls nothing under test and runs on whatever
device its arguments live on.

  ref64 / absdot        v = A . W^T + b in float64 and the error unit S = |A| |W|^T + |b|
  ref64_ln / absdot_ln  the folded-LN form rs (A . W^T - mu s) + c and its error unit
  emu_*                 what each epilogue SPECIFIES, bit for bit, on an fp32-exact v:
                        store (one RNE to T), f32, fp32 residual, fp16 residual (an IEEE fp16
                        add), patch rows, class-token rows, the folded-LN store's two fmas
  gelu64 / quick64      the activations in float64
  e_gelu / e_quick      the error the kernels' fp32 activation arithmetic is allowed
  interval_ok           out is the rounding of SOME value in [lo, hi] (RNE is monotone)
  fp16_grid             every fp16 pre-activation of the activation sweep
  plan_tail / choose_rows / launch_choice / launch_report
                        the launcher's host-side plan as functions of (M, N, K, ncu, variant)

T(x) for a float64 x means "x rounded to fp32, then RNE to T", the two steps an fp32
epilogue performs; both are monotone, so T is.
"""
import math

import torch

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
ACT_NONE, ACT_QUICKGELU, ACT_GELU = 0, 1, 2
FP32_MIN_NORMAL = 2.0 ** -126

# gemm.hip: variant flags
NO_TAIL = 1 << 16
TAIL_FIRST = 1 << 17
STAGGER = 1 << 18
ROW_STAGING = 1 << 21


# ------------------------------------------------------------------ float64 references
def ref64(A, W, bias=None):
    """v = A . W^T + b in float64 on the given (already rounded) operands."""
    v = A.double() @ W.double().t()
    return v if bias is None else v + bias.double()


def absdot(A, W, bias=None):
    """S = |A| |W|^T + |b|: every partial sum of v, in any order, is bounded by it."""
    s = A.double().abs() @ W.double().abs().t()
    return s if bias is None else s + bias.double().abs()


def ref64_ln(A, W, mu, rs, colsum, c):
    """rs (A . W^T - mu s) + c, float64; mu, rs [M], colsum, c [N]."""
    acc = A.double() @ W.double().t()
    return rs.double()[:, None] * (acc - mu.double()[:, None] * colsum.double()[None, :]) + c.double()


def absdot_ln(A, W, mu, rs, colsum, c):
    s = A.double().abs() @ W.double().abs().t()
    s = s + mu.double().abs()[:, None] * colsum.double().abs()[None, :]
    return rs.double().abs()[:, None] * s + c.double().abs()


def is_fp32_exact(v64):
    return bool((v64.float().double() == v64).all())


# ------------------------------------------------------------------ rounding
def to_T(x64, T):
    """T(x): float64 -> fp32 -> T, round to nearest even each."""
    x32 = x64.float()
    return x32 if T == F32 else x32.to(T)


def interval_ok(out, lo64, hi64, T):
    """Elementwise: T(lo) <= out <= T(hi). NaN in `out` is never accepted; -0 equals +0."""
    o = out.double()
    return (to_T(lo64, T).double() <= o) & (o <= to_T(hi64, T).double())


# ------------------------------------------------------------------ exact emulations
def emu_store(v64, T):
    """EpiStore, act none: one RNE of the fp32 value to T. v64 must be fp32-exact."""
    return v64.float().to(T)


def emu_f32(v64):
    return v64.float()


def emu_resid32(x0, v64):
    """fp32 residual stream: fp32(x0 + fp32(v))."""
    return (x0.double() + v64.float().double()).float()


def emu_resid16(x0_h, v64):
    """fp16 residual stream (fp16 and bf16 operands): t = half(v), then the IEEE fp16 add
    x0 + t. The sum of two fp16 values is exact in float64, so one rounding follows."""
    assert x0_h.dtype == F16
    t = v64.float().to(F16)
    return (x0_h.double() + t.double()).to(F16)


def patch_rows(M, npatch, device=None):
    """Row map of the patch GEMM: row r = b * np + p -> token row b * (np + 1) + 1 + p."""
    r = torch.arange(M, device=device)
    return (r // npatch) * (npatch + 1) + 1 + r % npatch


def emu_patch(acc64, pos, npatch, X0):
    """EpiPatch on a copy of X0 [B * (np + 1), N] (fp32 or fp16): token row of r receives
    fp32(acc + pos[1 + r % np]), rounded once more (RNE) on the fp16 stream. The class
    rows b * (np + 1) keep X0's content."""
    M = acc64.shape[0]
    r = torch.arange(M, device=acc64.device)
    y = (acc64.float().double() + pos.double()[1 + r % npatch]).float()
    X = X0.clone()
    X[patch_rows(M, npatch, acc64.device)] = y.to(X0.dtype)
    return X


def emu_class_token(cls, pos, ntok, X0):
    """class_token on a copy of X0 [B * ntok, D]: rows b * ntok = fp32(cls + pos[0])."""
    y = (cls.double() + pos.double()[0]).float().to(X0.dtype)
    X = X0.clone()
    X[::ntok] = y
    return X


def emu_ln_store(acc64, mu, rs, colsum, c):
    """EpiStoreLN before the activation: fma(rs, fma(-mu, s, acc), c) in fp32, returned as
    float64 (each fma rounded to fp32 once). The inner fma is exact in float64 for fp32
    inputs of moderate range; the outer one only where rs * inner + c is (checked by
    ln_grid_exact for the integer grid the exact tests use)."""
    inner = (acc64 - mu.double()[:, None] * colsum.double()[None, :]).float().double()
    return (rs.double()[:, None] * inner + c.double()[None, :]).float().double()


def ln_grid_exact(acc64, mu, rs, colsum, c):
    """True iff neither fma of the folded-LN store rounds: its fp32 result then IS
    rs (acc - mu s) + c, whatever the instruction order."""
    inner = acc64 - mu.double()[:, None] * colsum.double()[None, :]
    outer = rs.double()[:, None] * inner + c.double()[None, :]
    return is_fp32_exact(inner) and is_fp32_exact(outer)


# ------------------------------------------------------------------ activations
def gelu64(v64):
    """0.5 v erfc(-v / sqrt 2): no 1 + erf cancellation in the negative tail."""
    return 0.5 * v64 * torch.special.erfc(-v64 / math.sqrt(2.0))


def quick64(v64):
    """v sigmoid(1.702 v), as v / (1 + exp(-1.702 v)); exp overflowing to inf gives -0."""
    return v64 / (1.0 + torch.exp(-1.702 * v64))


def act64(v64, act):
    return v64 if act == ACT_NONE else quick64(v64) if act == ACT_QUICKGELU else gelu64(v64)


def e_gelu(v64, y64):
    """4 x the relative error epilogue.h documents for the erf fit (5e-6)."""
    return 2e-5 * y64.abs()


def e_quick(v64, y64):
    """v_exp_f32 and v_rcp_f32 at about 1 ulp each, three multiplies / adds, and the
    rounding of the base-2 exponent argument 1.702 log2(e) v (absolute error |t| 2^-24
    in the exponent, i.e. a relative 1.702 |v| 2^-24 on the power)."""
    return (8.0 + 2.5 * v64.abs()) * 2.0 ** -23 * y64.abs()


def e_act(v64, y64, act):
    if act == ACT_NONE:
        return torch.zeros_like(y64)
    return e_quick(v64, y64) if act == ACT_QUICKGELU else e_gelu(v64, y64)


ACT_LIPSCHITZ = 1.13     # max |act'|: GELU 1.129, QuickGELU 1.100 (test_gemm_ref.py)


def act_ok(out, v64, act, T, slack64=None):
    """The activation check: `out` is T of some value within e_act (+ Lipschitz-scaled
    slack on v) of act64(v). One exception: a result whose exact value is below the fp32
    normal range may come out as +-0 (the fp32 arithmetic flushes it)."""
    y = act64(v64, act)
    e = e_act(v64, y, act)
    if slack64 is not None:
        e = e + (ACT_LIPSCHITZ if act != ACT_NONE else 1.0) * slack64
    ok = interval_ok(out, y - e, y + e, T)
    return ok | ((y.abs() < FP32_MIN_NORMAL) & (out.double() == 0))


def ambiguous(v64, act, T):
    """Points where the reference alone cannot name the rounding: T(y - e) != T(y + e)."""
    y = act64(v64, act)
    e = e_act(v64, y, act)
    return to_T(y - e, T).double() != to_T(y + e, T).double()


def fp16_grid():
    """Every normal fp16 value with |v| <= 16 (36 866), then +-0, +-100, +-65504: float64."""
    bits = torch.arange(0x0400, 0x4C01, dtype=torch.int32).to(torch.int16)   # 2^-14 .. 16.0
    pos = bits.view(F16).double()
    extra = torch.tensor([0.0, -0.0, 100.0, -100.0, 65504.0, -65504.0], dtype=torch.float64)
    return torch.cat([pos, -pos, extra])


# ------------------------------------------------------------------ the launcher's plan
def _cdiv(a, b):
    return (a + b - 1) // b


def tail_step(N, ncu):
    """Tile-rows per whole round of 256-column tiles: ncu / gcd(N / 256, ncu)."""
    return ncu // math.gcd(N // 256, ncu)


def plan_tail(M, N, ncu, TM=256):
    """gemm.hip plan_tail: (tile-rows kept in tiles, tail tasks, wide)."""
    ntm = _cdiv(M, TM)
    step = tail_step(N, ncu)
    ntm_dp = ntm // step * step
    rows = M - ntm_dp * TM
    if ntm_dp == 0 or rows <= 0 or rows > 256 or N % 64:
        return (ntm, 0, 0)
    wide_tasks = _cdiv(rows, 32) * (N // 128)
    narrow_tasks = _cdiv(rows, 16) * (N // 64)
    wide_cost = _cdiv(wide_tasks, ncu) * 3
    narrow_cost = _cdiv(narrow_tasks, ncu) * 2
    if N % 128 == 0 and wide_cost < narrow_cost:
        return (ntm_dp, wide_tasks, 1)
    return (ntm_dp, narrow_tasks, 0)


def choose_rows(M, N, ncu):
    """gemm.hip choose_rows: (row blocks of 64 per tile, plan)."""
    ntn = N // 256
    if _cdiv(M, 256) * ntn <= ncu:
        if _cdiv(M, 128) * ntn <= ncu:
            return (2, (_cdiv(M, 128), 0, 0))
        if _cdiv(M, 192) * ntn <= ncu:
            return (3, (_cdiv(M, 192), 0, 0))
    return (4, plan_tail(M, N, ncu, 256))


def shape_ok(M, N, K):
    return M >= 1 and N >= 128 and K >= 64 and N % 128 == 0 and K % 64 == 0


# miclip_gemm_plan's kernel codes (include/miclip.h), by position
KERNELS = ("splitk", "tile128", "tile256_s0", "tile256_s1", "tile256", "tile256_regs",
           "persistent_p", "persistent", "persistent_staged", "rows192", "rows128")
CODES = (0, 3, 128, 129, 130, 192, 256, 257, 258, 259, 260)
DEFAULT_GROUP = 4


def launch_choice(M, N, K, ncu, tracc=True, patch=False, variant=0):
    """launch(): (kernel, plan), or None where it refuses the variant. At variant 0 kernel is
    one of 'rows128', 'rows192' (the persistent kernel's smaller tiles, transposed-accumulator
    epilogues only), 'persistent' (256-row tiles + tail), 'tile256' (one tile per workgroup
    + tail), 'tile128'. An explicit variant also reaches 'persistent_staged' (259 with
    ROW_STAGING), 'persistent_p' (3) and 'tile256_s0' / '_s1' / '_regs' (256 / 257 / 260).
    plan = the (ntm_dp, wgs, wide) the kernel receives, None where it takes none.
    tracc: EpiStore / EpiStoreLN / the fp16 residual; patch: EpiPatch.
    Restated from the launcher as it stood before csrc/gemm_plan.h: a chain of tests that
    rewrite the code on the way, kept in that shape on purpose."""
    assert shape_ok(M, N, K)
    no_tail, tail_first = bool(variant & NO_TAIL), bool(variant & TAIL_FIRST)
    stagger, staging = bool(variant & STAGGER), bool(variant & ROW_STAGING)
    code = (variant & ~(NO_TAIL | TAIL_FIRST | STAGGER | ROW_STAGING)) % 1000
    if code not in CODES:
        return None
    big = N % 256 == 0 and K >= 128
    tiles256 = _cdiv(M, 256) * (N // 256)
    whole = (_cdiv(M, 256), 0, 0)
    by_size = code == 0
    if by_size and not patch and big and 2 * tiles256 >= ncu:
        code = 259
    if tracc and not patch:
        small_ok = by_size and big and 2 * _cdiv(M, 128) * (N // 256) >= ncu
        if (code in (259, 192, 129, 130) or small_ok) and big and not staging:
            rb, plan = 4, None
            if code == 192:
                rb, plan = 3, (_cdiv(M, 192), 0, 0)
            elif code == 129:
                rb, plan = 2, (_cdiv(M, 128), 0, 0)
            elif code == 130:
                rb, plan = 2, plan_tail(M, N, ncu, 128)
            elif by_size:
                rb, plan = choose_rows(M, N, ncu)
            if rb != 4:
                return ("rows192" if rb == 3 else "rows128", plan)
            if small_ok:
                code = 259
    if code in (192, 129, 130):
        return None
    if code == 259 and not patch and big:
        plan = whole if no_tail else plan_tail(M, N, ncu)
        return ("persistent_staged" if tracc and staging else "persistent", plan)
    if code == 3 and not patch and big:
        return ("persistent_p", None)
    if N % 256 == 0 and code != 128 and (2 * tiles256 >= ncu or code >= 256):
        ntm_dp, wgs, wide = whole if no_tail else plan_tail(M, N, ncu)
        if wgs and tail_first:
            wgs, wide = _cdiv(wgs, 8) * 8, wide | 2
        if stagger and ntm_dp * (N // 256) >= 2 * ncu:
            wide |= 8 << 8
        name = {256: "tile256_s0", 257: "tile256_s1", 260: "tile256_regs"}.get(code, "tile256")
        return (name, (ntm_dp, wgs, wide))
    return ("tile128", None)


def launch_report(M, N, K, ncu, tracc=True, patch=False, variant=0, sk=1):
    """What miclip_gemm_plan reports for this launch: (kernel code, grid, block, gm, ntm_dp,
    wgs, wide), None where the launcher refuses. Split-K comes before the variant."""
    if not shape_ok(M, N, K):
        return None
    if sk > 1:
        return None if K % (sk * 64) else (0, _cdiv(M, 128) * (N // 128), 256, 0, 0, 0, 0)
    choice = launch_choice(M, N, K, ncu, tracc, patch, variant)
    if choice is None:
        return None
    name, plan = choice
    code = variant & ~(NO_TAIL | TAIL_FIRST | STAGGER | ROW_STAGING)
    gm = code // 1000 if code >= 1000 else DEFAULT_GROUP
    if name == "tile128":
        return (1, _cdiv(M, 128) * (N // 128), 256, 0, 0, 0, 0)
    if name == "persistent_p":
        return (6, min(_cdiv(M, 256) * (N // 256), ncu), 512, gm, 0, 0, 0)
    tiles = plan[0] * (N // 256)
    grid = tiles + plan[1] if name.startswith("tile256") else min(max(tiles, plan[1]), ncu)
    return (KERNELS.index(name), grid, 512, gm) + plan


def wide_tail_shape(ncu):
    """A (M, N) at K = 128 whose tail the plan serves with the wide 32 x 128 tasks, the
    smallest found; None if this CU count has none among the candidates."""
    for N in (4096, 2048, 3072, 8192, 1024):
        for r in (256, 224, 192, 160, 128):
            M = 256 * tail_step(N, ncu) + r
            if plan_tail(M, N, ncu)[2] == 1:
                return (M, N)
    return None


# ------------------------------------------------------------------ LayerNorm over gathered rows
def layernorm64(x, rows, stride, gamma, beta, R, normalize, eps=1e-5):
    """Output row r normalises input row rows[r] (or r * stride): float64."""
    idx = rows.long() if rows is not None else torch.arange(R, device=x.device) * stride
    g = x.double()[idx]
    mu = g.mean(-1, keepdim=True)
    var = ((g - mu) ** 2).mean(-1, keepdim=True)
    y = (g - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    if normalize:
        y = y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return y
