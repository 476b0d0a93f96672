"""GPU: the MX-fp8 family -- the quantisers and both 256x256x128 GEMM kernels of
csrc/gemm_mx.hip, csrc/mx.h and the MX outputs of csrc/norm.hip -- against tests/_mx_ref.py
(float64 / exact integers, self-checked on the CPU by tests/test_mx_ref.py, planted faults
included): bit for bit where the arithmetic is exact, every block and every byte inside a
per-element interval elsewhere. No share thresholds.

Data outputs are pre-filled (NaN for fp16, 0xA5 for bytes) and carry a canary row behind
row M - 1; every scale plane is pre-filled with 0xA5 and carries a 256-byte canary tail. Every
figure is printed before it is asserted (pytest -s); the wall time is printed at the end.

Q   miclip_op_quant_mx kinds 0 (fp32), 1 (fp16, 16-B loads, quad blocks), 2 (fp16, 8-lane
    blocks) at (R, K) = (1, 256), (3, 512), (255, 256), (257, 768), (2, 1280): 15 cases. Rows
    are built from the block zoo of _mx_ref.zoo -- amax = 448 2^k exactly and one ulp either
    side (fp32 k = -20 .. 20, fp16 k = -22 .. 7), +0 / -0 blocks, one spike at each of the 32
    positions over a 2^-12 floor, every RNE tie of e4m3 (2^-10 .. the odd halves of every
    step, both signs, at block scales 2^-3, 2^0, 2^4), the type's largest value, fp16
    subnormals, and for fp32 six tiny blocks (0 < amax < 448 2^-126) -- in the order of
    _mx_ref.zoo_sequence, which puts every class into each of the 8 block slots of a 256-k
    segment (small shapes take as many launches as that needs). Exponents and bytes must be
    the reference's bit for bit. Tiny blocks may carry -127 or -126, with the bytes RNE at
    the exponent written.
    Refusals: K = 128, K = 384, R = 0, for each kind: 3 cases.
G1  the GEMM on operands built on the host as bytes and planes (_mx_ref.gen_exact: elements
    integers in [-3, 3], fp32 bias a multiple of 0.25), so that every partial sum is exact in
    fp32 in any order (test_mx_ref.py): group "row" one scale exponent per A row and per W
    row in [-8, 8]; group "block" exponents per (row, k-block) in [-2, 2]; "subnormal" as
    "block" with only e4m3 subnormal codes of A meeting non-zero partners.
    Shapes (1, 256, 128) and (16, 256, 128) (the one-tile kernel only: variants 0 and 1, 2
    refused), (1, 256, 256), (255, 256, 256), (257, 512, 384), (300, 768, 256),
    (513, 256, 640) and the tile walk (1025, 256 ceil((CUs + 3) / 5), 256), variants 0, 1, 2;
    groups row and block at every shape, subnormal at (257, 512, 384) and (300, 768, 256):
    18 cases. Each case runs, per variant, bit for bit: fp16 store (RNE) with bias and with
    bias = NULL, the fp16 residual (IEEE fp16 add on an integer-valued x0), MX out act 0 with
    bias and with bias = NULL; and in the interval form around act64(v) -+ e_act: fp16 store
    act 1, 2, MX out act 1, 2 and act 3 (gelu64(v) -+ 4.8e-4), after checking that every
    32-column block of the reference holds an element with |y| >= 1.
    Launcher refusals (activations an epilogue does not implement, bias = NULL for the
    residual): 1 case.
G2  float operands (blocky as test_gpu_mx._blocky, an all-zero A row and W row, one outlier
    channel of 2^8) quantised on the GPU at (17, 256, 256), (257, 512, 1280), (17, 256, 5120):
    3 cases. max |C - ref64| / S, S = |A_d||W_d|^T + |b|, against float64 on the dequantised
    operands; bar = min(4 x measured, 1e-3). fp16 store and MX out (act 0) in the interval
    form ref64 -+ bar S. Measured on the MI355X: see MEASURED_G2.
L   miclip_op_layernorm_mx, fp32 input (one wave per row, 8-lane blocks) and fp16 input (two
    rows per wave, quad blocks) at (R, D) = (1, 256), (2, 512), (9, 768), (33, 1024),
    (7, 1280), (17, 1536): 12 cases. Row classes N(0.5, 9), constant (y = beta), mean 1000
    with unit spread, one element at 3000 among N(0, 1); gamma of both signs; gamma = beta = 0
    over one 32-column block (scale byte 0, zero bytes). layernorm64 of the input as given
    -+ 1e-4 (LN_TOL), every block and byte.

MEASURED ON THE MI355X (256 CUs; 52 cases, 2.6 s wall for the file)
  Cases run: Q 15 + 3 refusals, G1 18 + 1 launcher refusals, G2 3, L 12. All pass.
  Q   every exponent and byte equal to the reference in all 15 cases (fp32: 192 classes x 8
      slots, fp16: 156 x 8). Tiny blocks: the hardware writes -126 for every one of the six,
      those at and below 448 2^-127 (where the documented rule clamps to -127) included -- fp32
      subnormals are kept, so amax / 448 is a non-zero subnormal and the bit trick gives
      -127 + 1; the bytes are RNE at -126. Harmless (the elements then use half the range),
      accepted as the issue states, and recorded here.
  G1  every case bit for bit on variants 0, 1 and 2, group "block" and "subnormal" included:
      at per-(row, k-block) exponents in [-2, 2] the scaled MFMA sums the 128 products of a
      K-tile, and K-tile after K-tile, exactly -- no deviation to attribute to the adder's
      alignment width, so the spread stays as stated. All interval-form cases (fp16 store
      QuickGELU / GELU, MX out QuickGELU / GELU / tanh form) pass with every 32-column block
      of the reference holding an element with |y| >= 1. Canary rows and plane tails untouched
      everywhere, at K = 128 (one-tile kernel against float64) and on the 260-tile walk over
      256 workgroups as well.
  G2  smallest bar that passes = largest |C - ref64| / S once the fp16 store's own rounding
      cell is taken off, identical on variants 0, 1, 2:
        K = 256: 1.425e-4    K = 1280: 2.546e-4    K = 5120: 2.435e-5
      (with the fp16 rounding left in: 4.78e-4, 6.10e-4, 4.60e-4). Bars min(4 x, 1e-3):
      5.70e-4, 1e-3, 9.74e-5. The all-zero A row and W row give fp16(bias) exactly.
  L   every block and byte of the 12 cases inside layernorm64 -+ 1e-4; constant rows are
      MX(beta) bit for bit, the gamma = beta = 0 block is scale byte 0 over zero bytes.

FOUND AND FIXED (csrc/gemm_mx.hip gemm_mx): the launcher replaced activations it does not
implement instead of refusing them -- epi 0 with act 3 ran the erf GELU, epi 5 with an unknown
act ran none, epi 1 ignored act. It now returns hipErrorInvalidValue outside epi 0 {0, 1, 2},
epi 1 {0}, epi 5 {0, 1, 2, 3}; the model's own calls (capi.hip: (0, none), (1, none),
(5, QuickGELU / GELU / tanh form)) stay inside these sets. No kernel bug was found.
"""
import ctypes
import functools
import math
import time

import numpy as np
import pytest
import torch

import _gemm_ref as G
import _mx_ref as X

pytestmark = pytest.mark.gpu

F16 = torch.float16
CANARY = -7.0
FILL = X.CANARY_BYTE
LN_TOL = 1e-4                     # tests/test_gpu_kernels.py test_layernorm, fp32 out
MX_BOUND = 1e-3                   # tests/test_gpu_mx.py: the project's bound on |err| / sum|a||w|

# smallest bar at which the G2 cases pass (largest |C - ref64| / S net of the fp16 store's
# rounding cell), measured on the MI355X, per K (None: the project bound alone)
MEASURED_G2 = {256: 1.425e-4, 1280: 2.546e-4, 5120: 2.435e-5}

_T0 = time.time()


def _bar(K):
    m = MEASURED_G2[K]
    return MX_BOUND if m is None else min(4.0 * m, MX_BOUND)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from miclip import _lib
    yield _lib.load_library()
    print(f"\ntest_gpu_mx_exact.py wall time {time.time() - _T0:.1f} s")


@functools.lru_cache(None)
def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _check(lib, rc):
    assert rc == 0, lib.miclip_last_error().decode()


def _plane(rows, K, pages=None):
    """A 0xA5-filled plane with its 256-byte canary tail (or `pages` of them)."""
    n = X.scale_bytes(rows, K) + X.PLANE_TAIL
    return torch.full((n,) if pages is None else (pages, n), FILL, dtype=torch.uint8, device="cuda")


# ================================================================== Q: the quantisers
Q_SHAPES = [(1, 256), (3, 512), (255, 256), (257, 768), (2, 1280)]
KINDS = {0: ("fp32", torch.float32), 1: ("fp16", F16), 2: ("fp16", F16)}


@functools.lru_cache(None)
def _zoo(kind):
    blocks, names = X.zoo(kind)
    return torch.from_numpy(blocks), names


@pytest.mark.parametrize("R,K", Q_SHAPES)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_quant_mx_zoo(lib, kind, R, K):
    """Tiny blocks (0 < amax < 448 2^-126): the MI355X writes -126 for all of them, with bytes
    RNE at -126 (module docstring, MEASURED)."""
    tname, dt = KINDS[kind]
    blocks, names = _zoo(tname)
    Z = len(names)
    seq = X.zoo_sequence(Z)
    nblk = R * K // 32
    pages = -(-8 * Z // nblk)
    cls = torch.from_numpy(seq[np.arange(pages * nblk) % (8 * Z)])      # wraps on a multiple of 8
    y = blocks[cls].reshape(pages, R, K)                                # float64, exact in dt
    x = y.to(dt).cuda()
    assert torch.equal(x.double().cpu(), y)
    q = torch.full((pages, R + 1, K), FILL, dtype=torch.uint8, device="cuda")
    S = _plane(R, K, pages)
    for p in range(pages):
        _check(lib, lib.miclip_op_quant_mx(x[p].data_ptr(), kind, R, K, q[p].data_ptr(), S[p].data_ptr(),
                                           _stream()))
    torch.cuda.synchronize()
    rows_ok = bool((q[:, R] == FILL).all())
    tail_ok = bool((S[:, X.scale_bytes(R, K):] == FILL).all())
    E = S[:, X._plane_idx(R, K, "cuda")].long() - 127                   # [pages, R, K / 32]
    v = X.bytes_exact(q[:, :R].reshape(pages * R, K), E.reshape(pages * R, K // 32),
                      y.cuda().reshape(pages * R, K), tiny_either=True)
    cls_d = cls.cuda()
    bad_blk = (v.bad_E | v.bad_q.reshape(pages * R, K // 32, 32).any(-1)).reshape(-1)
    bad_names = sorted({names[c] for c in cls_d[bad_blk].unique().tolist()})
    print(f"\nQ kind {kind} ({R}, {K}): {pages} launches, {pages * nblk} blocks of {Z} classes x 8 slots; {v}; "
          f"canary row {rows_ok}, plane tail {tail_ok}; failing classes {bad_names[:12]}")
    if tname == "fp32":
        amax = X.block_amax(y.cuda().reshape(pages * R, K)).reshape(-1)
        tiny = (amax > 0) & (amax < X.TINY)
        wrote = {}
        for c in cls_d[tiny].unique().tolist():
            wrote[names[c]] = sorted(v.E.reshape(-1)[tiny & (cls_d == c)].unique().tolist())
        print(f"  tiny blocks, exponent written: {wrote}")
    assert rows_ok and tail_ok
    assert v.ok, str(v)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_quant_mx_refusals(lib, kind):
    x = torch.zeros(4, 512, dtype=KINDS[kind][1], device="cuda")
    q = torch.full((4, 512), FILL, dtype=torch.uint8, device="cuda")
    S = _plane(4, 512)
    for R, K in ((4, 128), (4, 384), (0, 256)):
        rc = lib.miclip_op_quant_mx(x.data_ptr(), kind, R, K, q.data_ptr(), S.data_ptr(), _stream())
        print(f"\nQ refusal kind {kind} R {R} K {K}: rc {rc}")
        assert rc != 0
    torch.cuda.synchronize()
    assert bool((q == FILL).all()) and bool((S == FILL).all())


# ================================================================== G1: the GEMM, exact
def _walk_n():
    return 256 * -(-(_ncu() + 3) // 5)


G1_SHAPES = [(1, 256, 128), (16, 256, 128), (1, 256, 256), (255, 256, 256), (257, 512, 384),
             (300, 768, 256), (513, 256, 640), (1025, "walk", 256)]
G1_CASES = [(s, g) for s in G1_SHAPES for g in ("row", "block")] + \
           [((257, 512, 384), "subnormal"), ((300, 768, 256), "subnormal")]
# (epilogue, act, bias?): the first five bit for bit, the rest in the interval form
G1_FORMS = [("store", 0, True), ("store", 0, False), ("res", 0, True), ("mx", 0, True), ("mx", 0, False),
            ("store", 1, True), ("store", 2, True), ("mx", 1, True), ("mx", 2, True), ("mx", 3, True)]
EPI = {"store": 0, "res": 1, "mx": 5}


def _gemm(lib, qa, sa, qw, sw, bias, C, CS, M, N, K, epi, act, variant):
    return lib.miclip_op_gemm_mx_v(qa.data_ptr(), sa.data_ptr(), qw.data_ptr(), sw.data_ptr(), _p(bias),
                                   C.data_ptr(), _p(CS), M, N, K, epi, act, variant, _stream())


def _out16(M, N, x0=None):
    buf = torch.full((M + 1, N), math.nan, device="cuda", dtype=F16)
    if x0 is not None:
        buf[:M] = x0
    buf[M] = CANARY
    return buf


def _out8(M, N):
    return torch.full((M + 1, N), FILL, dtype=torch.uint8, device="cuda"), _plane(M, N)


def _same_bits(a, b):
    return a.view(torch.int16) == b.view(torch.int16)


@pytest.mark.parametrize("shape,group", G1_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gemm_mx_exact(lib, shape, group):
    """On the MI355X all groups are bit for bit, "block" at its stated spread of [-2, 2] per
    (row, k-block) included (module docstring, MEASURED)."""
    M, N, K = shape
    N = _walk_n() if N == "walk" else N
    op = X.gen_exact(M, N, K, group, seed=1000003 * M + 1009 * N + K, device="cuda")
    qa, qw = X.encode(op["a"]), X.encode(op["w"])
    assert torch.equal(X.decode(qa), op["a"]) and torch.equal(X.decode(qw), op["w"])
    sa, sw = X.write_plane(op["Ea"], K), X.write_plane(op["Ew"], K)
    A, W = X.operand_values(op["a"], op["Ea"]), X.operand_values(op["w"], op["Ew"])
    acc = A @ W.t()
    assert torch.equal(acc.float().double(), acc)              # the sums themselves are fp32 numbers
    sab = A.abs() @ W.abs().t()
    bias = op["bias"]
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x0 = torch.randint(-64, 65, (M, N), generator=g, device="cuda").to(F16)
    variants = (0, 1) if K < 256 else (0, 1, 2)
    tiles, ncu = -(-M // 256) * (N // 256), _ncu()
    print(f"\nG1 ({M}, {N}, {K}) {group}: {tiles} tiles on {ncu} CUs, variants {variants}")
    if K < 256:
        C = _out16(M, N)
        assert _gemm(lib, qa, sa, qw, sw, bias, C, None, M, N, K, 0, 0, 2) != 0
    failures = []
    for form, act, with_bias in G1_FORMS:
        b = bias if with_bias else None
        v32 = (acc + bias.double()).float().double() if with_bias else acc     # fp32(acc + bias), exact
        if act != 0:
            y = G.gelu64(v32) if act == 3 else G.act64(v32, act)
            short = int((y.abs().reshape(M, N // 32, 32).amax(-1) < 1).sum())
            print(f"  {form} act {act}: 32-column blocks of the reference without |y| >= 1: {short}")
            assert short == 0
        for variant in variants:
            if form == "mx":
                C, CS = _out8(M, N)
            else:
                C, CS = _out16(M, N, x0 if form == "res" else None), None
            _check(lib, _gemm(lib, qa, sa, qw, sw, b, C, CS, M, N, K, EPI[form], act, variant))
            torch.cuda.synchronize()
            if form == "mx":
                canary = X.rows_untouched(C, M, FILL) and X.plane_tail_untouched(CS, M, N)
                if act == 0:
                    v = X.bytes_exact(C, CS, v32)
                else:
                    v = X.bytes_in_interval(C, CS, *X.act_interval(v32, act))
                nbad, what = v.n_bad_E + v.n_bad_q, str(v)
            else:
                canary = bool((C[M] == CANARY).all())
                if act != 0:
                    bad = ~G.act_ok(C[:M], v32, act, F16)
                elif form == "res":
                    bad = ~_same_bits(C[:M], X.emu_resid16(x0, v32))
                else:
                    bad = ~_same_bits(C[:M], X.emu_store(v32, F16))
                nbad = int(bad.sum())
                what = f"wrong elements {nbad} / {bad.numel()}"
                if nbad:
                    dev = ((C[:M].double() - (v32 + (x0.double() if form == "res" else 0))).abs() / sab.clamp_min(1e-300))
                    what += (f", first at {bad.nonzero()[:4].tolist()}, largest |dev| / |A||W|^T "
                             f"{float(dev[bad].max()):.3e} (2^-10 = {2.0 ** -10:.3e})")
            print(f"  {form:5s} act {act} bias {int(with_bias)} variant {variant}: {what}; canaries {canary}")
            if nbad or not canary:
                failures.append((form, act, with_bias, variant, what, canary))
    assert not failures, failures


def test_gemm_mx_launcher_refusals(lib):
    """gemm_mx refuses an activation its epilogue does not implement (it used to run erf-GELU
    for epi 0 act 3, no activation for an unknown act of epi 5, and to ignore act for epi 1)
    and the residual without a bias; nothing is written."""
    M, N, K = 16, 256, 256
    op = X.gen_exact(M, N, K, "block", seed=1, device="cuda")
    qa, qw = X.encode(op["a"]), X.encode(op["w"])
    sa, sw = X.write_plane(op["Ea"], K), X.write_plane(op["Ew"], K)
    refused = [(0, 3), (0, 4), (0, -1), (1, 1), (1, 2), (1, 3), (1, -1), (5, 4), (5, -1), (5, 100)]
    for epi, act in refused:
        for variant in (0, 1, 2):
            C8, CS = _out8(M, N)
            C16 = _out16(M, N)
            C = C8 if epi == 5 else C16
            rc = _gemm(lib, qa, sa, qw, sw, op["bias"], C, CS if epi == 5 else None, M, N, K, epi, act, variant)
            torch.cuda.synchronize()
            print(f"\nG1 refusal epi {epi} act {act} variant {variant}: rc {rc}")
            assert rc != 0
            assert bool((C8 == FILL).all()) and bool((CS == FILL).all()) and bool(torch.isnan(C16[:M]).all())
    C16 = _out16(M, N)
    assert _gemm(lib, qa, sa, qw, sw, None, C16, None, M, N, K, 1, 0, 0) != 0
    # and what the model calls stays accepted: (0, none), (1, none), (5, QuickGELU / GELU / tanh form)
    for epi, act in ((0, 0), (0, 1), (0, 2), (1, 0), (5, 0), (5, 1), (5, 2), (5, 3)):
        C8, CS = _out8(M, N)
        C16 = _out16(M, N, torch.zeros(M, N, device="cuda", dtype=F16))
        _check(lib, _gemm(lib, qa, sa, qw, sw, op["bias"], C8 if epi == 5 else C16, CS if epi == 5 else None,
                          M, N, K, epi, act, 0))
    torch.cuda.synchronize()


# ================================================================== G2: the GEMM, float operands
def _blocky(R, K, seed):
    """tests/test_gpu_mx.py _blocky: rows whose 32-k blocks span 2^-6 .. 2^6, a zero block, a
    one-spike block and a tiny block."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((R, K)).astype(np.float32)
    x *= np.exp2(g.integers(-6, 7, size=(R, K // 32))).repeat(32, axis=1).astype(np.float32)
    x[0, :32] = 0
    x[min(1, R - 1), 32:64] = 0
    x[min(1, R - 1), 40] = 300.0
    x[R - 1, -32:] *= 1e-30
    return x


def _quant_gpu(lib, x):
    R, K = x.shape
    q = torch.full((R + 1, K), FILL, dtype=torch.uint8, device="cuda")
    S = _plane(R, K)
    _check(lib, lib.miclip_op_quant_mx(x.data_ptr(), 0, R, K, q.data_ptr(), S.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert X.rows_untouched(q, R, FILL) and X.plane_tail_untouched(S, R, K)
    return q, S, X.dequantize(q[:R], X.read_plane(S, R, K))


def _needed_bar(C16, ref, S):
    """Per element the smallest b with fp16(ref - b S) <= C <= fp16(ref + b S): the distance
    from ref to the nearer edge of C's rounding cell, over S. The cell reaches half a spacing
    to each side of C, and the spacing towards zero halves where |C| is a power of two."""
    c = C16.double()
    e = torch.floor(torch.log2(c.abs().clamp_min(2.0 ** -14)))
    up = torch.exp2(e - 10)
    down = torch.where((c.abs() == torch.exp2(e)) & (e > -14), up / 2, up)
    d = ref - c
    outward = (d * torch.sign(c) > 0) | (c == 0)
    return ((d.abs() - torch.where(outward, up, down) / 2).clamp_min(0) / S.clamp_min(1e-300))


@pytest.mark.parametrize("M,N,K", [(17, 256, 256), (257, 512, 1280), (17, 256, 5120)])
def test_gemm_mx_float_operands(lib, M, N, K):
    """Measured on the MI355X: K = 256 1.425e-4, K = 1280 2.546e-4, K = 5120 2.435e-5
    (MEASURED_G2; module docstring)."""
    A = _blocky(M, K, 3 * M + K)
    W = _blocky(N, K, 5 * N + K) * np.float32(2.0 ** -10)       # the outlier products stay inside fp16
    A[:, K // 3] *= np.float32(2.0 ** 8)                       # one outlier channel
    A[M // 2] = 0
    W[N // 3] = 0
    qa, sa, Ad = _quant_gpu(lib, torch.from_numpy(A).cuda())
    qw, sw, Wd = _quant_gpu(lib, torch.from_numpy(W).cuda())
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    ref = G.ref64(Ad, Wd, bias)
    S = G.absdot(Ad, Wd, bias)
    bar = _bar(K)
    failures = []
    for variant in (0, 1, 2):
        C = _out16(M, N)
        _check(lib, _gemm(lib, qa, sa, qw, sw, bias, C, None, M, N, K, 0, 0, variant))
        Q, QS = _out8(M, N)
        _check(lib, _gemm(lib, qa, sa, qw, sw, bias, Q, QS, M, N, K, 5, 0, variant))
        torch.cuda.synchronize()
        c = C[:M].double()
        assert bool(torch.isfinite(c).all())
        meas = float(_needed_bar(C[:M], ref, S).max())
        raw = float(((c - ref).abs() / S.clamp_min(1e-300)).max())
        ok16 = G.interval_ok(C[:M], ref - bar * S, ref + bar * S, F16)
        v = X.bytes_in_interval(Q, QS, ref - bar * S, ref + bar * S)
        canary = bool((C[M] == CANARY).all()) and X.rows_untouched(Q, M, FILL) and \
            X.plane_tail_untouched(QS, M, N)
        zero_rows = bool((C[M // 2] == bias.to(torch.float32).to(F16)).all()) and \
            bool((C[:M, N // 3] == bias[N // 3].to(F16)).all())
        print(f"\nG2 ({M}, {N}, {K}) variant {variant}: max |C - ref64| / S = {meas:.3e} (the smallest bar that passes; raw "
              f"|C - ref64| / S with the fp16 rounding in it {raw:.3e}); bar {bar:.3e}; fp16 outside {int((~ok16).sum())}; MX out {v}; "
              f"canaries {canary}; zero row / column exact {zero_rows}")
        if not (bool(ok16.all()) and v.ok and canary and zero_rows):
            failures.append((variant, meas, int((~ok16).sum()), str(v), canary, zero_rows))
    assert not failures, failures


# ================================================================== L: LayerNorm with MX output
L_SHAPES = [(1, 256), (2, 512), (9, 768), (33, 1024), (7, 1280), (17, 1536)]
L_CLASSES = ("normal", "constant", "mean1000", "spike3000")


def _ln_rows(R, D, first, g):
    x = torch.empty(R, D, dtype=torch.float64)
    kinds = []
    for r in range(R):
        c = L_CLASSES[(first + r) % len(L_CLASSES)]
        kinds.append(c)
        n = torch.randn(D, generator=g, dtype=torch.float64)
        if c == "normal":
            x[r] = 3 * n + 0.5
        elif c == "constant":
            x[r] = 0.5
        elif c == "mean1000":
            x[r] = 1000 + n
        else:
            x[r] = n
            x[r, int(torch.randint(0, D, (1,), generator=g))] = 3000.0
    return x, kinds


@pytest.mark.parametrize("idx", range(len(L_SHAPES)), ids=[f"{r}x{d}" for r, d in L_SHAPES])
@pytest.mark.parametrize("in_f16", [0, 1])
def test_layernorm_mx_every_byte(lib, in_f16, idx):
    R, D = L_SHAPES[idx]
    g = torch.Generator().manual_seed(100 * idx + in_f16)
    x64, kinds = _ln_rows(R, D, idx, g)
    x = x64.to(F16 if in_f16 else torch.float32).cuda()
    gam = 1 + 0.1 * torch.randn(D, generator=g)
    gam = gam * (1 - 2 * (torch.rand(D, generator=g) < 0.25).float())          # negative gamma
    bet = 0.05 * torch.randn(D, generator=g)
    zb = (R + idx) % (D // 32)                                                   # gamma = beta = 0 block
    gam[32 * zb:32 * zb + 32] = 0
    bet[32 * zb:32 * zb + 32] = 0
    gam, bet = gam.cuda(), bet.cuda()
    q = torch.full((R + 1, D), FILL, dtype=torch.uint8, device="cuda")
    S = _plane(R, D)
    _check(lib, lib.miclip_op_layernorm_mx(x.data_ptr(), in_f16, gam.data_ptr(), bet.data_ptr(), q.data_ptr(),
                                           S.data_ptr(), R, D, _stream()))
    torch.cuda.synchronize()
    y = X.layernorm64(x, None, 1, gam, bet, R, False)
    v = X.bytes_in_interval(q, S, y - LN_TOL, y + LN_TOL)
    E = X.read_plane(S, R, D)
    step = X.pow2(E).repeat_interleave(32, 1)
    dev = (X.dequantize(q[:R], E) - y).abs()
    zero_ok = bool((E[:, zb] == -127).all()) and bool((q[:R, 32 * zb:32 * zb + 32] & 0x7F == 0).all())
    const_ok = all(bool((X.bytes_exact(q[r:r + 1], E[r:r + 1], bet.double()[None, :])).ok)
                   for r in range(R) if kinds[r] == "constant")
    canary = X.rows_untouched(q, R, FILL) and X.plane_tail_untouched(S, R, D)
    print(f"\nL in_f16 {in_f16} ({R}, {D}) rows {sorted(set(kinds))}: {v}; largest |deq - y| "
          f"{float(dev.max()):.3e} = {float((dev / step).max()):.3f} of 2^E; zero block {zero_ok}; constant rows "
          f"are MX(beta) {const_ok}; canaries {canary}")
    assert v.ok, str(v)
    assert zero_ok and const_ok and canary
