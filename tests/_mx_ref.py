"""float64 / exact-integer restatement of the MX-fp8 format as this build uses it (csrc/mx.h,
csrc/gemm_mx.hip, the MX outputs of csrc/norm.hip): the yardstick of
tests/test_gpu_mx_exact.py, checked on the CPU by tests/test_mx_ref.py. Plain torch / numpy /
math; it calls nothing under test, shares no formula with csrc/mx.h or oracle/mx_oracle.py,
and runs on whatever device its arguments live on.

  E4M3 / decode / encode    the 256-entry e4m3fn table built from the format's definition
                            (bias 7, 3 mantissa bits, subnormals m 2^-9, 0x7f / 0xff NaN);
                            RNE encode = nearest table entry, a tie to the even code,
                            magnitudes above 448 saturate
  rule_exponent             E = ceil(log2(amax / 448)) from frexp: amax = m 2^e with m in
                            [1/2, 1) and 448 = 7/8 2^9, so E = e - 9 if m <= 7/8 else e - 8;
                            amax = 0 gives -127; clamped to [-127, 126]
  scale_index / read_plane / write_plane / scale_bytes
                            the tiled plane, from the layout comment of gemm_mx.hip: per
                            (256-row block, 128-k tile) one 1-KiB block
                            [k-block 4][row & 15][row >> 4 & 15], blocks ordered
                            [row block][k tile]
  quantize / dequantize     rows -> (bytes, E) by the rule, and back, float64
  bytes_exact               an MX output that must match bit for bit
  bytes_in_interval         an MX output known to a tolerance
  canary helpers            rows past M and bytes past the plane stay untouched
  gelu_tanh64               GELU's tanh form in float64
  gen_exact                 G1's operands: bytes and exponents with exact fp32 partial sums
  zoo / zoo_sequence        Q's block classes and the order that puts every class into each
                            of the 8 block slots of a 256-k segment

From tests/_gemm_ref.py: layernorm64, gelu64, quick64, act64, e_act, interval_ok, to_T,
emu_store, emu_resid16.
"""
import math

import numpy as np
import torch

import _gemm_ref as G
from _gemm_ref import (F16, F32, act64, e_act, emu_resid16, emu_store, gelu64,  # noqa: F401
                       interval_ok, layernorm64, quick64, to_T)

ACT_NONE, ACT_QUICKGELU, ACT_GELU, ACT_GELU_TANH = 0, 1, 2, 3
E_MIN, E_MAX = -127, 126
TINY = 448.0 * 2.0 ** -126          # below it amax / 448 is an fp32 subnormal
GELU_TANH_TOL = 4.8e-4              # csrc/kernels.h: |tanh form - exact GELU| as the kernel computes it
PLANE_TAIL = 256                    # canary bytes behind a scale plane
CANARY_BYTE = 0xA5


# ------------------------------------------------------------------ e4m3fn
def _build_table():
    t = []
    for code in range(256):
        s, e, m = code >> 7, (code >> 3) & 15, code & 7
        if e == 15 and m == 7:
            v = math.nan
        elif e == 0:
            v = m * 2.0 ** -9                       # subnormal: (m / 8) 2^-6
        else:
            v = (8 + m) * 2.0 ** (e - 10)           # (1 + m / 8) 2^(e - 7)
        t.append(-v if s else v)
    return t


E4M3 = _build_table()                               # python floats, index = code
_MAG = torch.tensor(E4M3[:127], dtype=torch.float64)            # 0 .. 448, ascending with the code
_MID = (_MAG[:-1] + _MAG[1:]) / 2                               # 126 midpoints, exact
_TAB = torch.tensor([0.0 if math.isnan(v) else v for v in E4M3], dtype=torch.float64)


def decode(q):
    """uint8 codes -> float64 (the NaN codes 0x7f / 0xff decode to NaN)."""
    v = _TAB.to(q.device)[q.long()]
    return torch.where((q & 0x7F) == 0x7F, torch.full_like(v, math.nan), v)


def encode(y64):
    """float64 -> uint8 e4m3 code: nearest table entry, ties to the even code, |y| > 448
    saturates to 448; the sign bit of y is kept (so -0 and a negative value that rounds to
    zero give 0x80)."""
    a = y64.abs()
    mid = _MID.to(y64.device)
    above = torch.bucketize(a, mid, right=False)    # midpoints strictly below a
    # bucketize(right=False): index i with mid[i-1] < a <= mid[i]; a tie a == mid[i] gives i
    tie = (above < 126) & (a == mid[above.clamp(max=125)])
    code = above + (tie & (above % 2 == 1)).long()  # at a tie take the even one of i, i + 1
    code = code.clamp(max=126)
    return (code + 128 * torch.signbit(y64).long()).to(torch.uint8)


# ------------------------------------------------------------------ the exponent rule
def rule_exponent(amax64):
    """ceil(log2(amax / 448)) for amax >= 0 (float64 tensor), clamped to [-127, 126]."""
    m, e = torch.frexp(amax64)
    E = torch.where(m <= 0.875, e.long() - 9, e.long() - 8)
    E = torch.where(amax64 == 0, torch.full_like(E, E_MIN), E)
    return E.clamp(E_MIN, E_MAX)


def rule_exponent_rational(amax):
    """The same from exact rationals, one python float at a time (test_mx_ref.py)."""
    from fractions import Fraction
    if amax == 0:
        return E_MIN
    x = Fraction(amax) / 448
    E = 0
    while Fraction(2) ** E < x:
        E += 1
    while Fraction(2) ** (E - 1) >= x:
        E -= 1
    return min(max(E, E_MIN), E_MAX)


# ------------------------------------------------------------------ the tiled scale plane
def scale_bytes(rows, K):
    return (rows + 255) // 256 * (K // 128) * 1024


def scale_index(r, kb, KT):
    """Byte offset of (row r, 32-k block kb): blocks [row block][k tile] of 1 KiB, inside a
    block [k-block 4][row & 15][row >> 4 & 15]. r, kb: integer tensors (broadcast)."""
    block = torch.div(r, 256, rounding_mode="floor") * KT + torch.div(kb, 4, rounding_mode="floor")
    row = r % 256
    inner = (kb % 4) * 256 + (row % 16) * 16 + torch.div(row, 16, rounding_mode="floor")
    return block * 1024 + inner


def _plane_idx(R, K, device):
    r = torch.arange(R, device=device)[:, None]
    kb = torch.arange(K // 32, device=device)[None, :]
    return scale_index(r, kb, K // 128)


def read_plane(plane, R, K):
    """Plane bytes -> E int64 [R, K / 32] of the valid rows."""
    return plane[_plane_idx(R, K, plane.device)].long() - 127


def write_plane(E, K, fill=0, tail=0):
    """E [R, K / 32] -> plane bytes (+ `tail` canary bytes behind it)."""
    R = E.shape[0]
    n = scale_bytes(R, K)
    plane = torch.full((n + tail,), fill, dtype=torch.uint8, device=E.device)
    plane[_plane_idx(R, K, E.device)] = (E + 127).to(torch.uint8)
    if tail:
        plane[n:] = CANARY_BYTE
    return plane


# ------------------------------------------------------------------ quantise / dequantise
def block_amax(y64):
    R, K = y64.shape
    return y64.abs().reshape(R, K // 32, 32).amax(-1)


def pow2(e):
    """2^e as float64 from its bit pattern (|e| <= 1022): exact on every device."""
    return ((e.long() + 1023) << 52).view(torch.float64)


def scaled(y64, E):
    """y / 2^E per block, exact in float64."""
    return y64 * pow2(-E).repeat_interleave(32, 1)


def quantize(y64):
    """[R, K] float64 -> (codes uint8 [R, K], E int64 [R, K / 32]) by the rule."""
    E = rule_exponent(block_amax(y64))
    return encode(scaled(y64, E)), E


def dequantize(q, E):
    return decode(q) * pow2(E).repeat_interleave(32, 1)


# ------------------------------------------------------------------ acceptance
class Verdict:
    """bad_E / bad_q: boolean masks [R, K / 32] / [R, K]; ok iff both are empty."""

    def __init__(self, bad_E, bad_q, E):
        self.bad_E, self.bad_q, self.E = bad_E, bad_q, E
        self.n_bad_E, self.n_bad_q = int(bad_E.sum()), int(bad_q.sum())
        self.ok = self.n_bad_E == 0 and self.n_bad_q == 0

    def __str__(self):
        s = f"wrong exponents {self.n_bad_E} / {self.bad_E.numel()}, wrong bytes {self.n_bad_q} / {self.bad_q.numel()}"
        if self.n_bad_E:
            s += f", first E at {self.bad_E.nonzero()[:4].tolist()}"
        if self.n_bad_q:
            s += f", first byte at {self.bad_q.nonzero()[:4].tolist()}"
        return s


def _written(S, R, K):
    """The written exponents: S is a plane (1-D bytes) or exponents already read (2-D)."""
    return S if S.dim() == 2 else read_plane(S, R, K)


def bytes_exact(q, S, y64, tiny_either=False):
    """q [R, K] codes and plane bytes S must be the rule's exponent and the RNE codes of
    y64 (an exact value per element), bit for bit. tiny_either: a block with
    0 < amax < 448 2^-126 may carry -127 or -126; its bytes must be the RNE codes at the
    exponent written."""
    R, K = y64.shape
    Ew = _written(S, R, K)
    amax = block_amax(y64)
    Er = rule_exponent(amax)
    bad_E = Ew != Er
    if tiny_either:
        tiny = (amax > 0) & (amax < TINY)
        bad_E = bad_E & ~(tiny & ((Ew == -127) | (Ew == -126)))
    Euse = torch.where(bad_E, Er, Ew)
    bad_q = q[:R] != encode(scaled(y64, Euse))
    return Verdict(bad_E, bad_q, Ew)


def bytes_in_interval(q, S, lo64, hi64, tiny_either=False):
    """Each element is known to lie in [lo, hi]. A block passes if (1) its written exponent
    is the rule's for some amax reachable inside the intervals -- the reachable amax are
    [max_i min|v_i|, max_i max|v_i|], and the rule is monotone -- and (2) every byte decodes
    to the RNE value, at the written exponent, of some value in its interval (RNE is
    monotone; -0 equals +0)."""
    R, K = lo64.shape
    Ew = _written(S, R, K)
    straddle = (lo64 <= 0) & (hi64 >= 0)
    amin = torch.where(straddle, torch.zeros_like(lo64), torch.minimum(lo64.abs(), hi64.abs()))
    amx = torch.maximum(lo64.abs(), hi64.abs())
    a_lo, a_hi = block_amax(amin), block_amax(amx)
    E_lo, E_hi = rule_exponent(a_lo), rule_exponent(a_hi)
    bad_E = (Ew < E_lo) | (Ew > E_hi)
    if tiny_either:
        tiny = (a_hi > 0) & (a_lo < TINY)
        bad_E = bad_E & ~(tiny & ((Ew == -127) | (Ew == -126)))
    Euse = torch.where(bad_E, E_hi, Ew)
    d = decode(q[:R])
    dl, dh = decode(encode(scaled(lo64, Euse))), decode(encode(scaled(hi64, Euse)))
    bad_q = ~((dl <= d) & (d <= dh))                # a NaN code is never accepted
    return Verdict(bad_E, bad_q, Ew)


def rows_untouched(buf, M, fill):
    """Rows >= M of a [M + n, N] buffer still hold `fill`."""
    return bool((buf[M:] == fill).all())


def plane_tail_untouched(S, R, K):
    tail = S[scale_bytes(R, K):]
    return tail.numel() == PLANE_TAIL and bool((tail == CANARY_BYTE).all())


# ------------------------------------------------------------------ activations
def gelu_tanh64(v64):
    """0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3)))."""
    return 0.5 * v64 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v64 + 0.044715 * v64 ** 3)))


def act_interval(v64, act):
    """[lo, hi] around the activation of an exact fp32 pre-activation v. act 0 .. 2: act64(v)
    -+ e_act (tests/_gemm_ref.py); act 3 (the tanh form) by the project's documented contract
    gelu64(v) -+ 4.8e-4. A result below the fp32 normal range may be flushed to zero."""
    if act == ACT_GELU_TANH:
        y = gelu64(v64)
        e = torch.full_like(y, GELU_TANH_TOL)
    else:
        y = act64(v64, act)
        e = e_act(v64, y, act)
    lo, hi = y - e, y + e
    flush = y.abs() < G.FP32_MIN_NORMAL
    return torch.where(flush, torch.minimum(lo, torch.zeros_like(lo)), lo), \
        torch.where(flush, torch.maximum(hi, torch.zeros_like(hi)), hi)


# ------------------------------------------------------------------ G1: exact GEMM operands
GROUPS = ("row", "block", "subnormal")


def gen_exact(M, N, K, group, seed, device="cpu"):
    """Operands whose every partial sum is exact in fp32, in any order.
      "row"        elements integers in [-3, 3]; one scale exponent per A row and per W row
                   in [-8, 8]: all products of an output share one exponent
      "block"      the same elements; exponents per (row, k-block) in [-2, 2]: every product
                   is an integer multiple of 2^-4, every partial sum below 2^17
      "subnormal"  "block", but A holds e4m3 subnormals j 2^-9 (j = 1 .. 7) at the k where
                   k % 4 == 1 and W is non-zero only there, so only subnormal codes meet
                   non-zero partners: multiples of 2^-13, partial sums below 2^10
    bias: multiples of 0.25 in [-4, 4], and 1024 at one column of every 32.
    Returns dict(a, w: float64 element values; Ea, Ew: int64 exponents [rows, K / 32];
    bias: fp32 [N])."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)   # noqa: E731
    a, w = ri(-3, 3, M, K).double(), ri(-3, 3, N, K).double()
    if group == "row":
        Ea, Ew = ri(-8, 8, M, 1).expand(M, K // 32), ri(-8, 8, N, 1).expand(N, K // 32)
    else:
        Ea, Ew = ri(-2, 2, M, K // 32), ri(-2, 2, N, K // 32)
    if group == "subnormal":
        sel = (torch.arange(K) % 4 == 1)
        sub = ri(1, 7, M, K).double() * 2.0 ** -9 * (2 * ri(0, 1, M, K).double() - 1)
        a = torch.where(sel[None, :], sub, a)
        w = torch.where(sel[None, :], w, torch.zeros_like(w))
    bias = ri(-16, 16, N).double() * 0.25
    spike = torch.arange(0, N, 32) + ri(0, 31, N // 32)
    bias[spike] = 1024.0
    out = dict(a=a, w=w, Ea=Ea.contiguous(), Ew=Ew.contiguous(), bias=bias.float())
    return {k: v.to(device) for k, v in out.items()}


def operand_values(x, E):
    """Element values times their block scales, float64 (exact)."""
    return x * pow2(E).repeat_interleave(32, 1)


# ------------------------------------------------------------------ Q: the block zoo
def _np_dtype(kind):
    return np.float32 if kind == "fp32" else np.float16


def zoo(kind, seed=0):
    """The block classes of the quantiser test for input type kind ("fp32" / "fp16"):
    (values float64 [Z, 32], every one representable in the type; names [Z])."""
    dt = _np_dtype(kind)
    g = np.random.default_rng(seed)
    blocks, names = [], []

    def add(name, v):
        v = np.asarray(v, dtype=np.float64)
        assert v.shape == (32,) and np.array_equal(v.astype(dt).astype(np.float64), v, equal_nan=False), name
        blocks.append(v)
        names.append(name)

    def body(amax, pos):
        """Random values of the type below amax, amax itself (random sign) at pos."""
        v = (g.uniform(-1, 1, 32) * amax).astype(dt).astype(np.float64)
        v = np.where(np.abs(v) >= amax, 0.0, v)
        v[pos] = amax * g.choice([-1.0, 1.0])
        return v

    # boundary amax: 448 2^k exactly and one ulp either side
    ks = range(-20, 21) if kind == "fp32" else range(-22, 8)
    for k in ks:
        b = dt(448.0) * dt(2.0) ** dt(k)
        for tag, a in (("at", b), ("below", np.nextafter(b, dt(0))), ("above", np.nextafter(b, dt(np.inf)))):
            if np.isfinite(a):
                add(f"boundary {tag} 448*2^{k}", body(float(a), int(g.integers(32))))
    # zero blocks
    add("zeros", np.zeros(32))
    add("negative zeros", -np.zeros(32))
    # a single spike at each position over a tiny non-zero floor
    for p in range(32):
        v = np.full(32, 2.0 ** -12) * g.choice([-1.0, 1.0], 32)
        v[p] = float(dt(100.0 + 11 * p)) * g.choice([-1.0, 1.0])
        add(f"spike at {p}", v)
    # exact RNE ties: every midpoint between adjacent codes (2^-10, which ties to 0, and the
    # odd halves of every step), both signs, at block scales 2^0, 2^-3, 2^4
    mids = ((np.array(E4M3[:126]) + np.array(E4M3[1:127])) / 2)
    mids = np.concatenate([mids, -mids])
    for k in (0, -3, 4):
        for i in range(0, len(mids), 31):
            v = np.zeros(32)
            chunk = mids[i:i + 31]
            v[:len(chunk)] = chunk
            v[31] = 448.0
            add(f"ties 2^{k} #{i // 31}", np.roll(v * 2.0 ** k, int(g.integers(32))))
    # type extremes
    big = float(np.finfo(dt).max)
    add("type max", body(big, 7))
    add("type max negative", -body(big, 30))
    if kind == "fp16":
        sub = g.integers(1, 1024, 32).astype(np.float64) * 2.0 ** -24
        add("fp16 subnormals", sub * g.choice([-1.0, 1.0], 32))
        v = np.zeros(32)
        v[13] = 2.0 ** -24
        add("fp16 smallest subnormal", v)
        add("fp16 subnormal max", body(1023 * 2.0 ** -24, 2))
    else:
        # tiny blocks: 0 < amax < 448 2^-126, elements j 2^-126 (normal fp32 numbers)
        for name, j in (("min normal", 1), ("below 448*2^-127", 223), ("at 448*2^-127", 224),
                        ("above 448*2^-127", 225), ("below 448*2^-126", 447), ("mid", 300)):
            v = g.integers(0, j + 1, 32).astype(np.float64) * g.choice([-1.0, 1.0], 32)
            v[int(g.integers(32))] = j
            add(f"tiny {name}", v * 2.0 ** -126)
    return np.stack(blocks), names


def zoo_sequence(Z, step=37):
    """Order of 8 Z blocks in which block t sits in slot t % 8 of its 256-k segment and every
    class meets every slot exactly once: class(t) = (t // 8 + (t % 8) step) % Z."""
    t = np.arange(8 * Z)
    return (t // 8 + (t % 8) * step) % Z
