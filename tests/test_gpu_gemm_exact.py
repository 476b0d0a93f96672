"""GPU: the GEMM family (csrc/gemm.hip, csrc/epilogue.h), the patch embedding / class token
and the gathered LayerNorm against tests/_gemm_ref.py (float64, self-checked on the CPU by
tests/test_gemm_ref.py): exact where the arithmetic is exact, a per-element bound elsewhere.

Every case gives its output one canary row behind it, which must stay untouched; store
outputs are pre-filled with NaN, so an element the kernel never wrote cannot match. Shapes
come from the restated launcher plan at the device's own CU count. Every figure is printed
before it is asserted (pytest -s).

C1  integer operands (A, W in [-3, 3], K <= 512, bias a multiple of 0.25 in [-4096, 4096]):
    every partial sum is an exact fp32 integer in any order, v = acc + b is fp32-exact, and
    the RNE to fp16 / bf16 really rounds. Each output element must equal the emulation of
    what the epilogue specifies, bit for bit: store, f32, fp32 residual, fp16 residual
    (IEEE fp16 add), the folded-LN store (statistics chosen so both fmas are exact), patch
    rows + class token. With an activation: C3's interval around act64(v).
    Each case is one (kernel path, M, N, K, group); inside it runs that group's epilogue
    forms in fp16 and bf16 on ONE reference. Group "plain" (bit for bit): store, store with
    bias = NULL, folded-LN store, fp32 residual, fp16 residual, f32, f32 with bias = NULL;
    group "act" (interval): store and folded-LN store x {QuickGELU, GELU}. So every (path,
    epilogue, dtype) the launcher accepts is run and the refused ones (192- / 128-row
    tiles with a non-transposed epilogue) are asserted refused.
    Cases: 128x128 12, one-tile 256x256 72, persistent 72, multi-tile walk 3, row tails
    30 narrow + 5 wide, 192- / 128-row tiles 32 -- 226, each in both groups: 452 -- and
    patch 6, refusals 1: 459. One more case launches nothing: the launcher's own plan
    (miclip_gemm_plan) for the row-tail shapes equals the restated one.
C2  float operands (outlier channels up to 2^10, an all-zero row in A and in W): fp32
    outputs |C - ref64| <= bar S, S = |A||W|^T + |b| (+ |x0| for the residual), bar =
    min(4 x measured, (K + 8) 2^-23); 16-bit outputs interval_ok(ref64 -+ bar S), through
    an activation act64(ref64) -+ (1.13 bar S + e_act). 35 shapes x 2 groups: 70 cases.
    Largest |C - ref64| / S measured on the MI355X over these cases:
      K = 64: 5.39e-7    K = 256: 7.78e-7   (caps 8.58e-6, 3.15e-5; bars 2.16e-6, 3.11e-6)
C3  both activations over every normal fp16 pre-activation with |v| <= 16 and +-0, +-100,
    +-65504 (A = 0, v = bias): the output must be T(act64(v)) unless the reference alone
    says the rounding is ambiguous within e (GELU 2e-5 |y|, QuickGELU (8 + 2.5 |v|) 2^-23
    |y|); there either neighbour passes. One exception: a result whose exact value is
    below the fp32 normal range (|y| < 2^-126) may come out as +-0. 48 cases.
    Outputs that differ from T(act64(v)) on the MI355X, per output row of 36 872 points, the
    same for variants 128 / 258 / 260 / 259, store and folded-LN store, M = 1 and 17:
      QuickGELU fp16 3 (125 points ambiguous)   QuickGELU bf16 1 (167 ambiguous)
      GELU fp16 8 (1 862 ambiguous)             GELU bf16 0 (474 ambiguous)
    All lie in the ambiguous set. Before the fix below GELU bf16 had 61: 8 in the flushed
    band and 53 under it, where the exact value is a bf16 subnormal and -0 was allowed.
D   miclip_op_layernorm_rows (strided and indexed gathers, normalize) against float64:
    fp32 outputs within test_layernorm's 1e-4, 16-bit outputs interval_ok around it. 8 cases.
    Measured: fp32 outputs <= 8.8e-7 from float64.

FOUND AND FIXED (csrc/epilogue.h act_tail): v_exp_f32 and v_rcp_f32 flush a subnormal RESULT to
zero, so both activations returned -0 as soon as their small factor dropped below 2^-126
although its product with v is still a normal fp32 number, which a bf16 output can hold (an
fp16 output rounds it to zero):
  * GELU, v in [-13.140625, -13.0859375] (8 points of the fp16 grid): exact |y| 1.27e-38 ..
    2.59e-38 >= 2^-126 = 1.18e-38. The 8 bf16 GELU cases of the sweep failed on these 8
    points and no other.
  * QuickGELU, v in about (-53.7, -51.3), exact |y| 1.2e-38 .. 6.4e-37: outside the sweep's
    grid but on C1's (multiples of 0.25 from -53.5 to -51.5); 185 of the 261 "act" cases
    of C1 failed on a bf16 pre-activation in one of the two bands, no fp16 one.
The bf16 stores now form that tail as (w h) h with h = 2^(x/2); no other output bit changes.
"""
import ctypes
import functools
import math
import time

import pytest
import torch

import _gemm_ref as G

pytestmark = pytest.mark.gpu

F16, BF16, F32 = G.F16, G.BF16, G.F32
DT = {"fp16": (0, F16), "bf16": (1, BF16)}
CANARY = -7.0
EINVAL = -1
NT, TF, RS = G.NO_TAIL, G.TAIL_FIRST, G.ROW_STAGING

# largest |C - ref64| / S over the C2 cases, fp32 outputs, measured on the MI355X, per K
MEASURED_C2 = {64: 5.39e-7, 256: 7.78e-7}
LN_TOL = 1e-4                     # tests/test_gpu_kernels.py test_layernorm, fp32 out

_T0 = time.time()


def _cap(K):
    """At most K + 2 fp32 roundings or truncations of the accumulation and the bias add
    (+ the two fmas of the folded-LN store or the residual add), each at most 2^-23 of a
    partial sum bounded by S."""
    return (K + 8) * 2.0 ** -23


def _bar(K):
    m = MEASURED_C2[K]
    return _cap(K) if m is None else min(4.0 * m, _cap(K))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from miclip import _lib
    yield _lib.load_library()
    print(f"\ntest_gpu_gemm_exact.py wall time {time.time() - _T0:.1f} s")


@functools.lru_cache(None)
def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g, device="cuda").double()


def _out(M, N, dtype, x0=None):
    """[M + 1, N]: NaN (or x0) in the rows the kernel owns, the canary row behind them."""
    buf = torch.full((M + 1, N), math.nan, device="cuda", dtype=dtype)
    if x0 is not None:
        buf[:M] = x0
    buf[M] = CANARY
    return buf


def _canary_ok(buf, M):
    return bool((buf[M] == CANARY).all())


# ------------------------------------------------------------------ one shape, every epilogue
TRACC = ("store", "ln", "res16")          # transposed-accumulator epilogues (epilogue.h TrAcc)
FORMS = [("store", 0, True), ("store", 1, True), ("store", 2, True), ("store", 0, False),
         ("ln", 0, True), ("ln", 1, True), ("ln", 2, True),
         ("res32", 0, True), ("res16", 0, True), ("f32", 0, True), ("f32", 0, False)]


class Case:
    """Operands and the float64 reference of one (M, N, K), shared by every epilogue form
    and both operand types. exact = C1's integer grid, else C2's float operands."""

    def __init__(self, M, N, K, exact, seed=0):
        g = torch.Generator(device="cuda").manual_seed(1000003 * M + 1009 * N + K + seed)
        self.M, self.N, self.K, self.exact = M, N, K, exact
        if exact:
            self.A64, self.W64 = _ints(g, M, K), _ints(g, N, K)
            self.bias = (_ints(g, N, lo=-16384, hi=16384) * 0.25).float()
            self.mu = _ints(g, M, lo=-4, hi=4).float()
            self.rs = (2.0 ** -_ints(g, M, lo=0, hi=6)).float()
            self.colsum = _ints(g, N, lo=-64, hi=64).float()
            self.c = (_ints(g, N, lo=-16384, hi=16384) * 0.25).float()
            self.x32 = torch.randn(M, N, device="cuda", generator=g) * \
                torch.exp2(torch.randint(-20, 20, (M, 1), device="cuda", generator=g).float())
        else:
            A = torch.randn(M, K, device="cuda", generator=g)
            cols = torch.randperm(K, device="cuda", generator=g)[:3]
            A[:, cols] *= torch.tensor([2.0 ** 10, 2.0 ** 7, 2.0 ** 4], device="cuda")
            A[M // 2] = 0
            W = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
            W[N // 3] = 0
            self.A64, self.W64 = A.double(), W.double()
            self.bias = torch.randn(N, device="cuda", generator=g)
            self.mu = torch.randn(M, device="cuda", generator=g) * 0.5
            self.rs = torch.rand(M, device="cuda", generator=g) + 0.5
            self.colsum = torch.randn(N, device="cuda", generator=g)
            self.c = torch.randn(N, device="cuda", generator=g)
            self.x32 = torch.randn(M, N, device="cuda", generator=g) * 8
        self.stats = torch.stack([self.mu, self.rs], dim=1).contiguous()
        self.x16 = (64 * torch.randn(M, N, device="cuda", generator=g)).to(F16)
        self._ref = {}

    def operands(self, dt):
        """(A, W) in the operand type and their float64 products: acc64, |A||W|^T."""
        if dt not in self._ref:
            T = DT[dt][1]
            A, W = self.A64.to(T), self.W64.to(T)
            if self.exact:
                assert torch.equal(A.double(), self.A64) and torch.equal(W.double(), self.W64)
            self._ref[dt] = (A, W, G.ref64(A, W), G.absdot(A, W))
        return self._ref[dt]


def _launch(lib, case, dt, form, variant):
    """Runs one epilogue form; returns (rc, output buffer)."""
    kind, act, with_bias = form
    code, T = DT[dt]
    A, W, _, _ = case.operands(dt)
    M, N, K = case.M, case.N, case.K
    bias = case.bias if with_bias else None
    if kind == "store":
        out = _out(M, N, T)
        rc = lib.miclip_op_gemm(code, _p(A), _p(W), _p(bias), _p(out), M, N, K, 0, act, variant,
                                _stream())
    elif kind == "ln":
        out = _out(M, N, T)
        rc = lib.miclip_op_gemm_ln(code, _p(A), _p(W), _p(case.c), _p(case.colsum),
                                   _p(case.stats), _p(out), M, N, K, act, variant, _stream())
    elif kind == "res32":
        out = _out(M, N, F32, case.x32)
        rc = lib.miclip_op_gemm(code, _p(A), _p(W), _p(bias), _p(out), M, N, K, 1, 0, variant,
                                _stream())
    elif kind == "res16":
        out = _out(M, N, F16, case.x16)
        rc = lib.miclip_op_gemm(code, _p(A), _p(W), _p(bias), _p(out), M, N, K, 4, 0, variant,
                                _stream())
    else:
        out = _out(M, N, F32)
        rc = lib.miclip_op_gemm(code, _p(A), _p(W), _p(bias), _p(out), M, N, K, 2, 0, variant,
                                _stream())
    return rc, out


def _check_exact(case, dt, form, out):
    """C1: None if every element is what the epilogue specifies, else a message."""
    kind, act, with_bias = form
    T = DT[dt][1]
    M = case.M
    _, _, acc, _ = case.operands(dt)
    got = out[:M]
    if kind == "ln":
        assert G.ln_grid_exact(acc, case.mu, case.rs, case.colsum, case.c)
        v = G.emu_ln_store(acc, case.mu, case.rs, case.colsum, case.c)
    else:
        v = acc + case.bias.double() if with_bias else acc
    assert G.is_fp32_exact(v)
    if kind in ("store", "ln"):
        if act == 0:
            bad = _bits(got) != _bits(G.emu_store(v, T))
        else:
            bad = ~G.act_ok(got, v, act, T)
    elif kind == "res32":
        bad = _bits(got) != _bits(G.emu_resid32(case.x32, v))
    elif kind == "res16":
        bad = _bits(got) != _bits(G.emu_resid16(case.x16, v))
    else:
        bad = _bits(got) != _bits(G.emu_f32(v))
    n = int(bad.sum())
    if n:
        r, c = [int(i) for i in bad.nonzero()[0]]
        return f"{n} wrong elements, first at ({r}, {c}): got {got[r, c].item()!r}, v {v[r, c].item()!r}"
    return None


def _check_bound(case, dt, form, out, ratios):
    """C2: None if every element is within the bar, else a message."""
    kind, act, with_bias = form
    T = DT[dt][1]
    M, K = case.M, case.K
    A, W, acc, absacc = case.operands(dt)
    got = out[:M]
    if kind == "ln":
        v = G.ref64_ln(A, W, case.mu, case.rs, case.colsum, case.c)
        S = G.absdot_ln(A, W, case.mu, case.rs, case.colsum, case.c)
    else:
        v = acc + case.bias.double() if with_bias else acc
        S = absacc + case.bias.double().abs() if with_bias else absacc
    slack = _bar(K) * S
    if kind in ("res32", "f32"):
        if kind == "res32":
            v, S = v + case.x32.double(), S + case.x32.double().abs()
            slack = _bar(K) * S
        err = (got.double() - v).abs()
        ratio = float((err / S.clamp_min(1e-300)).max())
        ratios.append(ratio)
        bad = ~(err <= slack)
    elif kind == "res16":
        lo = (case.x16.double() + G.to_T(v - slack, F16).double()).to(F16).double()
        hi = (case.x16.double() + G.to_T(v + slack, F16).double()).to(F16).double()
        bad = ~((lo <= got.double()) & (got.double() <= hi))
    else:
        bad = ~G.act_ok(got, v, act, T, slack)
    n = int(bad.sum())
    if n:
        r, c = [int(i) for i in bad.nonzero()[0]]
        return (f"{n} elements outside the bar, first at ({r}, {c}): got {got[r, c].item()!r}, "
                f"ref {v[r, c].item()!r}, S {S[r, c].item():.4g}")
    return None


GROUPS = ["plain", "act"]      # forms without / with an activation: separate cases


@pytest.fixture(params=GROUPS)
def group(request):
    return request.param


def _run_forms(lib, M, N, K, variant, exact, group, tracc_only=False):
    case = Case(M, N, K, exact)
    fails, ratios, ran = [], [], 0
    for dt in DT:
        for form in FORMS:
            if (form[1] != 0) != (group == "act"):
                continue
            refused = tracc_only and form[0] not in TRACC
            rc, out = _launch(lib, case, dt, form, variant)
            torch.cuda.synchronize()
            tag = f"{dt} {form[0]} act {form[1]} {'bias' if form[2] else 'no bias'}"
            if refused:
                if rc != EINVAL:
                    fails.append(f"{tag}: expected a refusal, rc {rc}")
                continue
            if rc != 0:
                fails.append(f"{tag}: rc {rc} {lib.miclip_last_error().decode()}")
                continue
            ran += 1
            if not _canary_ok(out, M):
                fails.append(f"{tag}: canary row written")
            msg = _check_exact(case, dt, form, out) if exact else \
                _check_bound(case, dt, form, out, ratios)
            if msg:
                fails.append(f"{tag}: {msg}")
    fig = f", max |C - ref64| / S {max(ratios):.3e} (cap {_cap(K):.3e})" if ratios else ""
    print(f"variant {variant:#x} M {M} N {N} K {K}: {ran} forms run, {len(fails)} failed{fig}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ C1: the kernel paths
def _step(N):
    return G.tail_step(N, _ncu())


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("M", [1, 127, 129])
def test_exact_128x128(lib, M, N, K, group):
    _run_forms(lib, M, N, K, 128, True, group)


@pytest.mark.parametrize("K", [64, 128, 192])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [1, 255, 257])
@pytest.mark.parametrize("variant", [256, 257, 258, 260])
def test_exact_one_tile_256(lib, variant, M, N, K, group):
    _run_forms(lib, M, N, K, variant, True, group)


@pytest.mark.parametrize("K", [64, 128, 192, 320])       # 64: falls back to the one-tile kernel
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [1, 255, 257])
@pytest.mark.parametrize("variant", [259, 259 | RS, 3])
def test_exact_persistent(lib, variant, M, N, K, group):
    _run_forms(lib, M, N, K, variant, True, group)


@pytest.mark.parametrize("variant", [259, 259 | RS, 3])
def test_exact_persistent_walks_several_tiles(lib, variant, group):
    """More tiles than workgroups and a partial last tile-row (264 tiles at 256 CUs)."""
    ncu = _ncu()
    M = 256 * (ncu // 4 + 2) - 100
    assert G._cdiv(M, 256) * 4 > ncu
    _run_forms(lib, M, 1024, 128, variant | NT, True, group)


@pytest.mark.parametrize("r", [1, 16, 17, 37, 256])
@pytest.mark.parametrize("variant", [258, 260, 258 | TF, 259, 0, 130])
def test_exact_row_tail_narrow(lib, variant, r, group):
    ncu, N, K = _ncu(), 1024, 128
    TM = 128 if variant == 130 else 256
    M = TM * _step(N) + r
    plan = G.plan_tail(M, N, ncu, TM)
    assert plan[0] == _step(N) and plan[1] > 0, plan
    print(f"plan {plan}, by-size choice {G.launch_choice(M, N, K, ncu)[0]}")
    _run_forms(lib, M, N, K, variant, True, group, tracc_only=variant == 130)


@pytest.mark.parametrize("variant", [258, 260, 258 | TF, 259, 0])
def test_exact_row_tail_wide(lib, variant, group):
    shape = G.wide_tail_shape(_ncu())
    if shape is None:
        pytest.skip("no candidate shape takes the wide tail tasks at this CU count")
    M, N = shape
    plan = G.plan_tail(M, N, _ncu())
    assert plan[2] == 1 and plan[1] > 0
    print(f"M {M} N {N} plan {plan}")
    _run_forms(lib, M, N, 128, variant, True, group)


def test_row_tail_shapes_reach_the_tail_kernels(lib):
    """The premise of the two tests above, checked instead of assumed: at this device's CU
    count the launcher's own plan (miclip_gemm_plan, ncu = 0) equals the restated one for
    every shape and variant they build, and it runs row-tail tasks of the kind they name.
    No kernel runs."""
    ncu, K = _ncu(), 128
    shapes = [(v, (128 if v == 130 else 256) * _step(1024) + r, 1024, 0)
              for v in (258, 260, 258 | TF, 259, 0, 130) for r in (1, 16, 17, 37, 256)]
    wide = G.wide_tail_shape(ncu)
    if wide is not None:
        shapes += [(v, wide[0], wide[1], 1) for v in (258, 260, 258 | TF, 259, 0)]
    kernels = set()
    for variant, M, N, wide_bit in shapes:
        for epi, tracc in ((0, True), (2, False)):
            out = (ctypes.c_int32 * 8)()
            rc = lib.miclip_gemm_plan(M, N, K, epi, variant, 1, 0, out)
            want = G.launch_report(M, N, K, ncu, tracc, False, variant)
            print(f"variant {variant:#x} M {M} N {N} epi {epi}: rc {rc} plan {list(out)[:7]}")
            if variant == 130 and not tracc:
                assert rc == EINVAL and want is None
                continue
            assert rc == 0 and tuple(out[:7]) == want
            assert out[5] > 0 and out[6] & 1 == wide_bit, "no row tail of the expected kind"
            kernels.add(G.KERNELS[out[0]])
    assert kernels == {"tile256", "tile256_regs", "persistent", "rows128"}


@pytest.mark.parametrize("K", [128, 192])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [1, 191, 193, 383])
@pytest.mark.parametrize("variant", [192, 129])
def test_exact_small_row_tiles(lib, variant, M, N, K, group):
    """192- / 128-row tiles: transposed-accumulator epilogues only, the others refused."""
    _run_forms(lib, M, N, K, variant, True, group, tracc_only=True)


def test_refusals(lib):
    """Shapes and pairs the launcher rejects before it launches anything."""
    buf = torch.zeros(1 << 20, device="cuda")     # every call below is refused before a launch
    p = buf.data_ptr()
    gemm = lambda *a: lib.miclip_op_gemm(0, p, p, p, p, *a, _stream())  # noqa: E731
    assert gemm(16, 100, 64, 0, 0, 0) == EINVAL                 # N % 128
    assert gemm(16, 128, 96, 0, 0, 0) == EINVAL                 # K % 64
    assert gemm(0, 128, 64, 0, 0, 0) == EINVAL                  # M < 1
    assert gemm(16, 256, 128, 0, 0, 7) == EINVAL                # unknown variant
    assert gemm(16, 256, 128, 0, 3, 0) == EINVAL                # unknown activation
    assert gemm(16, 256, 128, 9, 0, 0) == EINVAL                # unknown epilogue
    for variant in (192, 129, 130):
        assert gemm(16, 256, 128, 1, 0, variant) == EINVAL      # fp32 residual: not TrAcc
        assert gemm(16, 256, 128, 2, 0, variant) == EINVAL      # f32
        assert gemm(16, 256, 64, 0, 0, variant) == EINVAL       # one K-tile
        assert gemm(16, 384, 128, 0, 0, variant) == EINVAL      # N % 256
    for epi in (1, 4):
        assert lib.miclip_op_gemm(0, p, p, None, p, 16, 256, 128, epi, 0, 0, _stream()) == EINVAL
    assert lib.miclip_op_gemm_patch(0, p, p, p, p, 10, 256, 128, 3, 0, 0, _stream()) == EINVAL
    assert lib.miclip_op_gemm_patch(0, p, p, p, p, 9, 256, 128, 0, 0, 0, _stream()) == EINVAL
    assert lib.miclip_op_gemm_patch(0, p, p, p, p, 9, 100, 128, 3, 0, 0, _stream()) == EINVAL
    assert lib.miclip_op_gemm_patch(0, p, p, p, p, 9, 256, 128, 3, 0, 7, _stream()) == EINVAL
    assert lib.miclip_op_gemm_patch(0, p, p, None, p, 9, 256, 128, 3, 0, 0, _stream()) == EINVAL
    assert lib.miclip_op_class_token(None, p, p, 1, 2, 256, 0, _stream()) == EINVAL
    assert lib.miclip_op_class_token(p, p, p, 0, 2, 256, 0, _stream()) == EINVAL
    assert lib.miclip_op_layernorm_rows(0, p, None, 0, p, p, p, 1, 1, 256, _stream()) == EINVAL
    assert lib.miclip_op_layernorm_rows(0, p, None, 1, p, p, p, 1, 1, 100, _stream()) == EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------ C1: patch + class token
@pytest.mark.parametrize("npatch", [1, 3, 49])
@pytest.mark.parametrize("variant", [128, 258])
def test_exact_patch_and_class_token(lib, variant, npatch):
    """EpiPatch's row map r -> b (np + 1) + 1 + r % np, the positional row 1 + p and the
    fp16-stream rounding, M = B np straddling a tile edge; then the class rows."""
    N, K = 256, 128
    edge = 128 if variant == 128 else 256
    B = edge // npatch + 1
    M, ntok = B * npatch, npatch + 1
    assert M > edge and M - npatch <= edge
    g = torch.Generator(device="cuda").manual_seed(31 * npatch + variant)
    A64, W64 = _ints(g, M, K), _ints(g, N, K)
    pos = torch.randn(ntok, N, device="cuda", generator=g) * 10
    cls = torch.randn(N, device="cuda", generator=g)
    acc = G.ref64(A64, W64)
    fails = []
    for dt, (code, T) in DT.items():
        A, W = A64.to(T), W64.to(T)
        for resid16, RT in ((0, F32), (1, F16)):
            X = torch.full((B * ntok + 1, N), CANARY, device="cuda", dtype=RT)
            X0 = X.clone()
            rc = lib.miclip_op_gemm_patch(code, _p(A), _p(W), _p(pos), _p(X), M, N, K, npatch,
                                          resid16, variant, _stream())
            assert rc == 0, lib.miclip_last_error().decode()
            torch.cuda.synchronize()
            want = G.emu_patch(acc, pos, npatch, X0)     # class rows and the canary row: -7
            n1 = int((_bits(X) != _bits(want)).sum())
            rc = lib.miclip_op_class_token(_p(cls), _p(pos), _p(X), B, ntok, N, resid16, _stream())
            assert rc == 0, lib.miclip_last_error().decode()
            torch.cuda.synchronize()
            want = G.emu_class_token(cls, pos, ntok, want[:-1])
            n2 = int((_bits(X[:-1]) != _bits(want)).sum())
            ok = bool((X[-1] == CANARY).all())     # every other row is pinned by `want`
            print(f"{dt} stream {RT}: patch {n1} wrong, class token {n2} wrong, canaries {ok}")
            if n1 or n2 or not ok:
                fails.append((dt, RT, n1, n2, ok))
    assert not fails, fails


# ------------------------------------------------------------------ C2: float operands
def _c2_paths():
    ncu = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() \
        else 256
    step = G.tail_step(1024, ncu)
    wide = G.wide_tail_shape(ncu)
    paths = [("128", 128, 129, 384, False)]
    paths += [(str(v), v, 257, 512, False) for v in (256, 257, 258, 260)]
    paths += [("259", 259, 257, 512, False), ("259rs", 259 | RS, 257, 512, False),
              ("3", 3, 257, 512, False),
              ("259walk", 259 | NT, 256 * (ncu // 4 + 2) - 100, 1024, False)]
    paths += [(f"tail{n}", v, 256 * step + 37, 1024, False)
              for n, v in (("258", 258), ("260", 260), ("258tf", 258 | TF), ("259", 259), ("0", 0))]
    paths += [("tail130", 130, 128 * step + 37, 1024, True)]
    if wide:
        paths += [("wide258", 258, wide[0], wide[1], False), ("wide259", 259, wide[0], wide[1], False)]
    paths += [("192", 192, 383, 512, True), ("129", 129, 383, 512, True)]
    return paths


C2_CASES = [pytest.param(v, M, N, K, tr, id=f"{name}-K{K}")
            for name, v, M, N, tr in _c2_paths() for K in (64, 256) if not (tr and K == 64)]


@pytest.mark.parametrize("variant,M,N,K,tracc_only", C2_CASES)
def test_bound_float_operands(lib, variant, M, N, K, tracc_only, group):
    _run_forms(lib, M, N, K, variant, False, group, tracc_only=tracc_only)


# ------------------------------------------------------------------ C3: the activation sweep
@functools.lru_cache(None)
def _grid():
    v = G.fp16_grid()
    pad = (-v.numel()) % 4096
    v = torch.cat([v, torch.zeros(pad, dtype=torch.float64)])
    return v.cuda(), v.numel() - pad


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("kind", ["store", "ln"])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("variant", [128, 258, 260, 259])
def test_activation_over_every_fp16_preactivation(lib, variant, dt, kind, act):
    code, T = DT[dt]
    N, K = 4096, 128
    v_all, n_real = _grid()
    g = torch.Generator(device="cuda").manual_seed(5)
    W = torch.randn(N, K, device="cuda", generator=g).to(T)
    zero_cs = torch.zeros(N, device="cuda")
    bad = differ = ambiguous = nan = 0
    offenders = []
    for M in (1, 17):
        A = torch.zeros(M, K, device="cuda", dtype=T)
        mu = _ints(g, M, lo=-4, hi=4).float()
        rs = (2.0 ** -_ints(g, M, lo=0, hi=6)).float()
        stats = torch.stack([mu, rs], dim=1).contiguous()
        for i in range(0, v_all.numel(), N):
            v = v_all[i:i + N]
            bias = v.float()
            assert torch.equal(bias.double(), v)
            out = _out(M, N, T)
            if kind == "store":
                rc = lib.miclip_op_gemm(code, _p(A), _p(W), _p(bias), _p(out), M, N, K, 0, act,
                                        variant, _stream())
            else:     # colsum = 0: rs (0 - mu 0) + c = c exactly
                rc = lib.miclip_op_gemm_ln(code, _p(A), _p(W), _p(bias), _p(zero_cs), _p(stats),
                                           _p(out), M, N, K, act, variant, _stream())
            assert rc == 0, lib.miclip_last_error().decode()
            torch.cuda.synchronize()
            assert _canary_ok(out, M)
            vv = v.expand(M, N)
            real = (torch.arange(i, i + N, device="cuda") < n_real).expand(M, N)
            got = out[:M]
            nan += int((got.isnan() & real).sum())
            wrong = ~G.act_ok(got, vv, act, T) & real
            bad += int(wrong.sum())
            offenders += vv[wrong].unique().tolist()
            differ += int(((got.double() != G.to_T(G.act64(vv, act), T).double()) & real).sum())
            ambiguous += int((G.ambiguous(vv, act, T) & real).sum())
            if i + N >= n_real:     # the extreme points, what IEEE conversion gives
                ext = {float(x): got[:, j] for j, x in enumerate(v.tolist()) if i + j < n_real}
                if act == 0:
                    assert (ext[65504.0].float() == (65504.0 if T == F16 else 65536.0)).all()
                    assert (ext[-65504.0].float() == (-65504.0 if T == F16 else -65536.0)).all()
                else:
                    assert (ext[-100.0].float() == 0).all() and (ext[100.0].float() == 100).all()
                    assert (ext[-65504.0].float() == 0).all()
    print(f"variant {variant} {dt} {kind} act {act}: {differ} outputs differ from T(act64(v)), "
          f"{ambiguous} points ambiguous, {bad} outside the interval, {nan} NaN")
    if offenders:
        y = G.act64(torch.tensor(offenders, dtype=torch.float64), act)
        print(f"  outside at v in [{min(offenders)}, {max(offenders)}] ({len(set(offenders))} points), "
              f"|act64(v)| in [{float(y.abs().min()):.3e}, {float(y.abs().max()):.3e}]")
    assert nan == 0 and bad == 0
    if act == 0:
        assert differ == 0


# ------------------------------------------------------------------ D: LayerNorm over gathered rows
@pytest.mark.parametrize("gather", ["stride", "index"])
@pytest.mark.parametrize("D", [256, 1536])
@pytest.mark.parametrize("R", [1, 5])
def test_layernorm_rows(lib, R, D, gather):
    g = torch.Generator(device="cuda").manual_seed(R * D)
    rows_in = 13
    x = torch.randn(rows_in, D, device="cuda", generator=g) * 2 + 0.5
    x[2] = 0.75
    x[3] = 0.75                                    # all-equal rows: the output is beta
    gamma = torch.randn(D, device="cuda", generator=g)
    beta = torch.randn(D, device="cuda", generator=g)
    if gather == "stride":
        rows, stride = None, 3                     # rows 0, 3, 6, 9, 12
        flat = [3 * r for r in range(R)]
    else:                                          # a repeated and a descending index
        flat = [7, 2, 2, 9, 0][:R] if R > 1 else [3]
        rows, stride = torch.tensor(flat, device="cuda", dtype=torch.int32), 0
    assert max(flat) < rows_in
    fails = []
    for in16 in (0, 1):
        xin = x.half() if in16 else x
        for normalize in (0, 1):
            ref = G.layernorm64(xin, rows, stride, gamma, beta, R, normalize)
            for r, src in enumerate(flat):
                if src in (2, 3):
                    b64 = beta.double()
                    want = b64 / b64.norm() if normalize else b64
                    assert float((ref[r] - want).abs().max()) <= 1e-12
            for out_f32, dt in ((1, "fp16"), (0, "fp16"), (0, "bf16")):
                code, T = DT[dt]
                OT = F32 if out_f32 else T
                out = _out(R, D, OT)
                flags = out_f32 | (in16 << 1) | (normalize << 2)
                rc = lib.miclip_op_layernorm_rows(code, _p(xin), _p(rows), stride, _p(gamma),
                                                  _p(beta), _p(out), flags, R, D, _stream())
                assert rc == 0, lib.miclip_last_error().decode()
                torch.cuda.synchronize()
                got = out[:R]
                err = float((got.double() - ref).abs().max())
                if out_f32:
                    ok = err <= LN_TOL
                else:
                    ok = bool(G.interval_ok(got, ref - LN_TOL, ref + LN_TOL, T).all())
                print(f"in16 {in16} normalize {normalize} out {OT}: max |err| {err:.3e}")
                if not ok or not _canary_ok(out, R):
                    fails.append((in16, normalize, str(OT), err, _canary_ok(out, R)))
    assert not fails, fails
