"""GPU: edge cases of the attention kernels (csrc/attention.hip) through
miclip_op_attention and miclip_op_attention_q0, against the numpy float64 yardstick of
tests/_attn_ref.py (self-checked on the CPU by tests/test_attn_ref.py).

What is compared with what:
  * every case: the kernel's output against float64 attention on the same rounded
    operands, per element, in the unit u U (u = 2^-11 fp16 / 2^-8 bf16, U[q, d] =
    sum_k p[q, k] |v[k, d]|). The bar is max(4, E_T) u U with E_T the error, in the same
    unit, of the reference model's own dtype-T arithmetic on that input (_attn_ref.bar);
    an element with U = 0 must be exactly 0. Nothing of either reference runs on the GPU.
  * four input families at every N: random N(0, 1.5^2); indicator-V (flat softmax, one
    non-zero V row per head: a dropped, doubled or wrongly masked key moves the output by
    a whole U); one-hot (margin >= 40 log2 units); staircases of +12, -12, +7.5 and +8.5
    log2 units per 32-key tile (a rescale on every tile, none after the first, and the two
    sides of the lazy-rescale threshold 8).
  * B = 2, H = 3; the output has a canary row before and after it, qkv 32 NaN guard rows
    before and after it. Every accept / refuse expectation below is asserted.
  * isolation: the output of (image 1, head 1) bit for bit when every other head's data
    is NaN, or +- the largest finite value; many heads per workgroup (hpw = 2, and 3 where
    a kernel first returns to an LDS buffer) with a short last workgroup: sampled heads
    against float64, and bit for bit on a second launch and with every other head NaN.

Variant -> kernel (kernel_of below restates attn_launch's conditions as ranges of N):
  dh 64  N > 640: refused.  8: attention_x8_kernel, non-causal N = 256..259 only (else
         refused).  0: x8 there; else as 2.  2, 4: attention_pipe_kernel for N <= 288 (4:
         its split form where non-causal and N = 32k + 1..2, k >= 4), the one-head kernel
         above.  1: the one-head attention_kernel<64>: the 16-wave build for more than 12
         query chunks unless N = 32k + 1..3 (non-causal, N >= 64: the extra keys on VALU,
         attend_shift + attend_extra_keys, 12-wave build), else the 12-wave build.
  dh 80  N > 416: refused.  6: attention80p_kernel, non-causal N = 256..259 only.  2:
         attention80s_kernel, non-causal N = 129..288 only.  0: 80p, else 80s, where they
         apply, else as 1.  1: attention_kernel<80>.
  q0     attention_q0_kernel, N <= 768.

Measured on the MI355X: largest kernel ratio |err| / (u U) / largest E_T, over all N and
variants of this file (the bar stays max(4, E_T) per input, it is not derived from these):
                       fp16 dh 64     fp16 dh 80     bf16 dh 64     bf16 dh 80
  random               2.78 / 7.23    2.25 / 7.50    2.63 / 8.23    1.99 / 6.81
  indicator-V          0.99 / 1.88    0.98 / 1.72    0.99 / 1.74    0.99 / 1.74
  one-hot              0 / 0          0 / 0          0 / 0          0 / 0
  stairs +12 +7.5 +8.5 3.78 / 145.7   2.12 / 104.5   3.67 / 167.8   2.59 / 88.9
  stairs -12           1.36 / 2.20    1.26 / 2.47    1.52 / 2.28    1.28 / 3.14
  q0 random            1.24 / 3.50    1.19 / 4.08    1.32 / 2.75    0.94 / 3.23
  q0 indicator-V       0.88 / 1.28    0.88 / 1.28    0.99 / 1.66    0.99 / 1.66
  q0 one-hot           0 / 0          0 / 0          0 / 0          0 / 0
  q0 stairs rising     1.22 / 75.4    1.23 / 73.0    1.20 / 56.2    1.15 / 62.4
  q0 stairs -12        1.22 / 1.58    1.23 / 1.58    1.20 / 2.28    1.15 / 2.10
Per kernel (fp16 / bf16): attention_kernel<64> on 12 waves 3.78 / 3.67 (its extra-key form,
N = 321 and 385, on the rising staircase), on 16 waves 1.69 / 1.60; pipe 1.73 / 1.73, its
split form 1.73 / 1.71; x8 2.41 / 2.35; attention_kernel<80> 1.47 / 1.56, 80s the same bits;
80p 2.25 / 2.59; q0 1.24 / 1.32. No kernel came above 4 u U anywhere, so no case rests on
E_T; the isolation and many-heads cases differ in no bit. Nothing failed: no kernel change.
"""
import ctypes

import numpy as np
import pytest
import torch

import _attn_ref as R

gpu = pytest.mark.gpu
DT = {"fp16": (0, torch.float16), "bf16": (1, torch.bfloat16)}
GUARD = 32              # NaN rows before and after qkv
CANARY = -7.0
B0, H0 = 2, 3
FAMILIES = ("random", "indicator", "one-hot") + tuple(f"stairs{s:+g}" for s in R.STEPS)

N64 = [1, 2, 31, 32, 33, 64, 65, 67, 68, 96, 129, 130, 131, 255, 256, 259, 260, 287, 288, 289,
       321, 324, 385, 388, 513, 609, 640]
N64C = [1, 2, 32, 33, 77, 96, 97, 288, 289, 640]
N80 = [1, 33, 128, 129, 160, 255, 256, 259, 260, 288, 289, 416]
N80C = [1, 77, 129, 416]
SWEEP = ([(64, 0, n) for n in N64] + [(64, 1, n) for n in N64C] +
         [(80, 0, n) for n in N80] + [(80, 1, n) for n in N80C])
VARIANTS = {64: (0, 1, 2, 4, 8), 80: (0, 1, 2, 6)}
NQ0 = [1, 2, 255, 256, 257, 512, 513, 767, 768]
KERNELS = {"plain64/12", "plain64/16", "plain80", "80s", "80p", "pipe", "pipe-split", "x8"}


def kernel_of(dh, N, causal, variant):
    """The kernel attn_launch runs, None where it refuses."""
    if dh == 80:
        if N > 416:
            return None
        p80 = not causal and 256 <= N <= 259
        s80 = not causal and 129 <= N <= 288
        if variant == 6:
            return "80p" if p80 else None
        if variant == 2:
            return "80s" if s80 else None
        if variant == 0 and p80:
            return "80p"
        if variant == 0 and s80:
            return "80s"
        return "plain80"
    if N > 640:
        return None
    x8 = not causal and 256 <= N <= 259
    if variant == 8:
        return "x8" if x8 else None
    if variant == 0 and x8:
        return "x8"
    if variant in (0, 2, 4) and N <= 288:
        split = variant == 4 and not causal and N >= 129 and N % 32 in (1, 2)
        return "pipe-split" if split else "pipe"
    chunks = (N + 31) // 32
    xkeys = not causal and N >= 64 and N % 32 in (1, 2, 3)
    return "plain64/16" if chunks > 12 and not xkeys else "plain64/12"


def test_sweep_reaches_every_kernel_and_boundary():
    """CPU: the table above over the sweep names all eight kernels, and the refusals sit
    at 641 (dh 64) and 417 (dh 80)."""
    seen = {kernel_of(dh, n, c, v) for dh, c, n in SWEEP for v in VARIANTS[dh]}
    assert seen - {None} == KERNELS
    assert kernel_of(64, 640, 0, 0) and all(kernel_of(64, 641, c, v) is None
                                            for c in (0, 1) for v in VARIANTS[64])
    assert kernel_of(80, 416, 0, 0) and all(kernel_of(80, 417, c, v) is None
                                            for c in (0, 1) for v in VARIANTS[80])
    assert [n for n in range(1, 641) if kernel_of(64, n, 0, 8)] == [256, 257, 258, 259]
    assert kernel_of(64, 259, 0, 0) == "x8" and kernel_of(64, 260, 0, 0) == "pipe"
    assert kernel_of(64, 288, 0, 0) == "pipe" and kernel_of(64, 289, 0, 0) == "plain64/12"
    assert kernel_of(64, 385, 0, 1) == "plain64/12" and kernel_of(64, 388, 0, 1) == "plain64/16"
    assert kernel_of(64, 513, 0, 1) == "plain64/12" and kernel_of(64, 640, 1, 1) == "plain64/16"
    assert kernel_of(80, 128, 0, 0) == "plain80" and kernel_of(80, 129, 0, 0) == "80s"
    assert kernel_of(80, 288, 0, 0) == "80s" and kernel_of(80, 289, 0, 0) == "plain80"


# ------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from miclip import _lib
    return _lib.load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(x, T):
    """x [rows, cols] (numpy float64 or a torch tensor, exact in T) on the device between
    2 x GUARD rows of NaN; the returned tensor's rows [GUARD, GUARD + rows) are the data."""
    tdt = DT[T][1]
    x = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
    full = torch.full((x.shape[0] + 2 * GUARD, x.shape[1]), float("nan"), dtype=tdt, device="cuda")
    full[GUARD:GUARD + x.shape[0]] = x.to(device="cuda", dtype=tdt)
    return full


def _launch(lib, full, T, B, N, H, dh, causal, variant, q0=False):
    """(rc, out [rows, H*dh] device tensor of dtype T); the canary rows around the output
    are checked, and after a refusal the output itself must be untouched too."""
    code, tdt = DT[T]
    rows = B if q0 else B * N
    buf = torch.full((rows + 2, H * dh), CANARY, dtype=tdt, device="cuda")
    esz = buf.element_size()
    qp = full.data_ptr() + GUARD * full.shape[1] * esz
    op = buf.data_ptr() + H * dh * esz
    if q0:
        rc = lib.miclip_op_attention_q0(code, qp, op, B, N, H, dh, _stream())
    else:
        rc = lib.miclip_op_attention(code, qp, op, B, N, H, dh, causal, variant, _stream())
    torch.cuda.synchronize()
    assert bool((buf[0] == CANARY).all()) and bool((buf[-1] == CANARY).all()), "canary row written"
    if rc != 0:
        assert bool((buf == CANARY).all()), "a refused launch wrote output"
    return rc, buf[1:-1]


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _one_head_images(x, B, N, H, dh, pairs):
    """The listed (image, head) pairs of a packed torch qkv as len(pairs) one-head images
    [S*N, 3*dh] (numpy float64), the yardstick's input for a subset of heads."""
    xs = x.view(B, N, 3, H, dh)
    sub = torch.stack([xs[b, :, :, h] for b, h in pairs]).double().numpy()    # [S, N, 3, dh]
    return np.ascontiguousarray(sub.reshape(len(pairs) * N, 3 * dh))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(fam, B, N, H, dh, T, causal):
    seed = 1000 * N + 10 * dh + causal
    if fam == "random":
        return R.random(B, N, H, dh, T, seed)
    if fam == "indicator":
        return R.indicator_v(B, N, H, dh, T, seed + 1, causal)[0]
    if fam == "one-hot":
        return R.one_hot(B, N, H, dh, T, seed + 2, causal)[0]
    return R.staircase(B, N, H, dh, T, seed + 3, float(fam[len("stairs"):]))


class Yard:
    """One input with its float64 output, error unit, E_T and per-element bound."""

    def __init__(self, fam, N, dh, T, causal, q0=False):
        u = R.UNIT[T]
        self.qkv = _inputs(fam, B0, N, H0, dh, T, causal)
        out, U = R.attention(self.qkv, B0, N, H0, dh, causal)
        ref_T = R.reference_arithmetic(self.qkv, B0, N, H0, dh, causal, T)
        if q0:      # the CLS rows only
            out, U, ref_T = (a[::N] for a in (out, U, ref_T))
        self.out, self.U, self.u = out, U, u
        self.e_t = R.e_t(out, U, ref_T, u)
        self.const = max(4.0, self.e_t)
        self.bound = R.bar(out, U, ref_T, u)

    def check(self, got):
        """(ratio, within the bar) of a device output."""
        g = _f64(got)
        if not np.isfinite(g).all():
            return float("inf"), False
        return R.ratio(g, self.out, self.U, self.u), R.within(g, self.out, self.bound)


# ------------------------------------------------------------------ a. N sweep x families
@gpu
@pytest.mark.parametrize("T", ["fp16", "bf16"])
@pytest.mark.parametrize("dh,causal,N", SWEEP)
def test_sweep_against_fp64(lib, dh, causal, N, T):
    lines, bad = [], []
    for fam in FAMILIES:
        y = Yard(fam, N, dh, T, causal)
        full = _guarded(y.qkv, T)
        cells = []
        for v in VARIANTS[dh]:
            kern = kernel_of(dh, N, causal, v)
            rc, got = _launch(lib, full, T, B0, N, H0, dh, causal, v)
            if (rc == 0) != (kern is not None):
                bad.append(f"{fam} variant {v}: rc {rc}, expected {kern or 'a refusal'}")
            if rc == 0 and kern is not None:
                r, ok = y.check(got)
                cells.append(f"v{v}:{kern}={r:.2f}")
                if not ok:
                    bad.append(f"{fam} variant {v} ({kern}): {r:.3g} u U over the bar {y.const:.3g}")
            else:
                cells.append(f"v{v}:refused")
        lines.append(f"  {fam} E_T={y.e_t:.2f} bar={y.const:.2f} " + " ".join(cells))
    print(f"ATTN dh={dh} causal={causal} N={N} {T}: |err| / (u U) per variant\n" + "\n".join(lines))
    assert not bad, bad


@gpu
@pytest.mark.parametrize("T", ["fp16", "bf16"])
def test_refusals_are_exact(lib, T):
    """One key past the LDS limit is refused by every variant (640 / 416 run in the sweep),
    and the CLS kernel refuses N = 769; nothing is written."""
    got = []
    for dh, n in ((64, 641), (80, 417)):
        full = _guarded(R.random(1, n, 1, dh, T, n), T)
        for causal in (0, 1):
            for v in VARIANTS[dh] + (3, 9):
                rc, _ = _launch(lib, full, T, 1, n, 1, dh, causal, v)
                got.append((dh, n, causal, v, rc))
    for dh in (64, 80):
        full = _guarded(R.random(1, 769, 1, dh, T, 769), T)
        rc, _ = _launch(lib, full, T, 1, 769, 1, dh, 0, 0, q0=True)
        got.append((dh, 769, 0, "q0", rc))
    print(f"{T}: refused {sum(1 for g in got if g[-1] != 0)} of {len(got)} launches past the limits")
    assert all(g[-1] != 0 for g in got), [g for g in got if g[-1] == 0]


# ------------------------------------------------------------------ b. the CLS-query kernel
@gpu
@pytest.mark.parametrize("T", ["fp16", "bf16"])
@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("N", NQ0)
def test_q0_against_fp64(lib, dh, N, T):
    cells, bad = [], []
    for fam in FAMILIES:
        y = Yard(fam, N, dh, T, 0, q0=True)
        rc, got = _launch(lib, _guarded(y.qkv, T), T, B0, N, H0, dh, 0, 0, q0=True)
        assert rc == 0, lib.miclip_last_error().decode()
        r, ok = y.check(got)
        cells.append(f"{fam} E_T={y.e_t:.2f} bar={y.const:.2f} q0={r:.2f}")
        if not ok:
            bad.append(f"{fam}: {r:.3g} u U over the bar {y.const:.3g}")
    print(f"ATTNQ0 dh={dh} N={N} {T}: |err| / (u U)\n  " + "\n  ".join(cells))
    assert not bad, bad


# ------------------------------------------------------------------ c. isolation
# one ragged N per kernel path: (dh, N, causal, variant, q0)
ISOLATION = [(64, 50, 0, 0, False), (64, 100, 1, 0, False), (64, 257, 0, 0, False),
             (64, 257, 0, 4, False), (64, 321, 0, 0, False), (64, 400, 1, 0, False),
             (80, 130, 0, 0, False), (80, 257, 0, 0, False), (80, 300, 0, 0, False),
             (64, 257, 0, 0, True), (80, 257, 0, 0, True)]


@gpu
@pytest.mark.parametrize("T", ["fp16", "bf16"])
@pytest.mark.parametrize("dh,N,causal,variant,q0", ISOLATION)
def test_head_is_independent_of_its_neighbours(lib, dh, N, causal, variant, q0, T):
    """Pad rows that are not clamped to the head's own last row, or an LDS slot reused
    across heads, would let a neighbour's data in."""
    B, H = 3, 3
    tdt = DT[T][1]
    x = torch.from_numpy(R.random(B, N, H, dh, T, 7 * N + dh)).to(tdt)
    keep = torch.zeros(B * N, 3, H, dh, dtype=torch.bool)
    keep[N:2 * N, :, 1] = True                   # image 1, head 1: its q, k and v
    keep = keep.view(B * N, 3 * H * dh)
    big = torch.finfo(tdt).max
    sign = torch.where(torch.arange(x.numel()).view_as(x) % 3 == 0, -big, big).to(tdt)
    outs = []
    for fill in (None, torch.full_like(x, float("nan")), sign):
        xin = x if fill is None else torch.where(keep, x, fill)
        rc, got = _launch(lib, _guarded(xin, T), T, B, N, H, dh, causal, variant, q0=q0)
        assert rc == 0, lib.miclip_last_error().decode()
        rows = got[1:2] if q0 else got[N:2 * N]
        outs.append(rows[:, dh:2 * dh].clone())
    # the first run is a correct attention (so "identical" is not "identically wrong")
    one = _one_head_images(x, B, N, H, dh, [(1, 1)])
    o64, U = R.attention(one, 1, N, 1, dh, causal)
    ref_T = R.reference_arithmetic(one, 1, N, 1, dh, causal, T)
    if q0:
        o64, U, ref_T = o64[:1], U[:1], ref_T[:1]
    u = R.UNIT[T]
    g64 = _f64(outs[0])
    r = R.ratio(g64, o64, U, u) if np.isfinite(g64).all() else float("inf")
    n_nan = int((_bits(outs[1]) != _bits(outs[0])).sum())
    n_big = int((_bits(outs[2]) != _bits(outs[0])).sum())
    print(f"ISOL dh={dh} N={N} causal={causal} variant={variant} "
          f"{'q0 ' if q0 else ''}{kernel_of(dh, N, causal, variant) if not q0 else 'q0'} {T}: "
          f"(image 1, head 1) {r:.2f} u U; elements differing in bits: NaN neighbours {n_nan}, "
          f"+-max neighbours {n_big}")
    assert np.isfinite(g64).all() and R.within(g64, o64, R.bar(o64, U, ref_T, u))
    assert n_nan == 0 and n_big == 0


# ------------------------------------------------------------------ d. many heads per workgroup
# (dh, N, causal, variant, workgroups per CU the launcher counts on, smallest hpw, the kernel).
# hpw = 2 is the smallest shape with a head boundary inside a workgroup; the two-buffer
# kernels (pipe, and its split form with its two parities of partials) come back to a
# buffer only with the third head, so they also run at hpw = 3. (x8 at hpw = 5 and 80p at
# hpw = 9 are compared bit for bit with hpw = 1 in tests/test_gpu_kernels.py.)
MANY = [(64, 77, 1, 0, 3, 2, "pipe"), (64, 77, 1, 0, 3, 3, "pipe"), (64, 50, 0, 0, 5, 2, "pipe"),
        (64, 50, 0, 0, 5, 3, "pipe"), (64, 257, 0, 0, 2, 2, "x8"), (64, 257, 0, 4, 1, 3, "pipe-split"),
        (80, 257, 0, 0, 1, 2, "80p")]


def _many_shape(per_cu, H, min_hpw):
    """(B, hpw): the smallest B with hpw = ceil(B H / (CUs x per_cu)) >= min_hpw and a short
    last workgroup, from the CU count the launcher reads."""
    slots = torch.cuda.get_device_properties(0).multi_processor_count * per_cu
    B = slots * (min_hpw - 1) // H
    while True:
        B += 1
        hpw = -(-B * H // slots)
        if hpw >= min_hpw and (B * H) % hpw != 0:
            return B, hpw


@gpu
@pytest.mark.parametrize("T", ["fp16", "bf16"])
@pytest.mark.parametrize("dh,N,causal,variant,per_cu,min_hpw,kern", MANY)
def test_many_heads_per_workgroup(lib, dh, N, causal, variant, per_cu, min_hpw, kern, T):
    """The text tower's real shape (1000 prompts x 8 heads at N = 77 is hpw ~ 11) is never
    run by the B = 2 cases: here every workgroup walks hpw >= 2 heads, the last one fewer."""
    H = 5
    tdt = DT[T][1]
    assert kernel_of(dh, N, causal, variant) == kern
    B, hpw = _many_shape(per_cu, H, min_hpw)
    heads = B * H
    grid = -(-heads // hpw)
    short0 = (grid - 1) * hpw                       # first head of the short workgroup
    mid = (grid // 2) * hpw
    sampled = sorted({0, heads - 1, short0 - hpw, short0 - 1, mid + 1, mid + hpw - 1} |
                     set(range(short0, heads)))
    g = torch.Generator().manual_seed(N + dh + causal)
    x = (1.5 * torch.randn(B * N, 3 * H * dh, generator=g)).to(tdt)
    full = _guarded(x, T)
    rc, got = _launch(lib, full, T, B, N, H, dh, causal, variant)
    assert rc == 0, lib.miclip_last_error().decode()
    rc, again = _launch(lib, full, T, B, N, H, dh, causal, variant)
    assert rc == 0, lib.miclip_last_error().decode()
    n_again = int((_bits(again) != _bits(got)).sum())       # every head, run to run
    del again
    pairs = [(bh // H, bh % H) for bh in sampled]
    S = len(pairs)
    sub_qkv = _one_head_images(x, B, N, H, dh, pairs)
    out, U = R.attention(sub_qkv, S, N, 1, dh, causal)
    ref_T = R.reference_arithmetic(sub_qkv, S, N, 1, dh, causal, T)
    u = R.UNIT[T]
    bound, e_t = R.bar(out, U, ref_T, u), R.e_t(out, U, ref_T, u)
    gv = got.view(B, N, H, dh)
    mine = torch.stack([gv[b, :, h] for b, h in pairs])               # [S, N, dh]
    g64 = _f64(mine).reshape(S * N, dh)
    r = R.ratio(g64, out, U, u) if np.isfinite(g64).all() else float("inf")
    # every other head poisoned
    keep = torch.zeros(B, N, 3, H, dh, dtype=torch.bool)
    for b, h in pairs:
        keep[b, :, :, h] = True
    xp = torch.where(keep.view(B * N, 3 * H * dh), x, torch.full_like(x, float("nan")))
    del keep
    rc, got2 = _launch(lib, _guarded(xp, T), T, B, N, H, dh, causal, variant)
    assert rc == 0, lib.miclip_last_error().decode()
    gv2 = got2.view(B, N, H, dh)
    mine2 = torch.stack([gv2[b, :, h] for b, h in pairs])
    n_diff = int((_bits(mine2) != _bits(mine)).sum())
    print(f"MANY dh={dh} N={N} causal={causal} variant={variant} {kern} {T}: B={B} H={H} "
          f"hpw={hpw} grid={grid} (last workgroup {heads - short0} heads), sampled heads "
          f"{sampled}: {r:.2f} u U (E_T {e_t:.2f}, bar {max(4.0, e_t):.2f}); elements differing "
          f"in bits: a second launch {n_again}, with every other head NaN {n_diff}")
    assert hpw >= min_hpw and heads % hpw != 0
    assert np.isfinite(g64).all() and R.within(g64, out, bound)
    assert n_again == 0 and n_diff == 0
