"""GPU: the ProLIP training kernels (csrc/prolip.hip) at the shapes where their tile,
padding and tail code can go wrong, the semantics the docstrings promise, and
miclip_prolip_adam on its own against torch.optim.Adam. test_gpu_prolip.py covers the
recorded runs at four shapes; this module covers the edges of the same kernels.

Every reference is plain fp64 torch on the CPU. Bar of every numeric comparison:
R.bar(e_ref, P0) = 4 * max(e_ref, 8 * 2^-23 * max|P0|), where e_ref is the distance
of the same CPU reference evaluated in fp32 from its fp64 evaluation (fp32 autograd
against fp64 autograd, fp32 torch.optim.Adam against fp64), never anything the
kernels computed. Adam's m and v take R.bar_on: the same rule with the floor on the
compared quantity. Every comparison prints err / bar before the test asserts.

Inputs: features on the grid k / 32, |k| <= 127, exact in fp32, fp16 and bf16, so the
three feature dtypes must give the same bits. Every float input sits in front of
NaNs and every output in front of a NaN canary: a read past an input that reaches a
result, or a write past an output, shows.

The CPU-side preconditions (the grid's round trips, top-2 logit gaps of at least 1e-3
wherever a count is compared exactly) are asserted before the device is asked for.
"""
import ctypes
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _prolip_ref as R

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SCALE = 100.0
MIN_GAP = 1e-3     # the fp32 logit error is about 1e-5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


class Checks:
    """test_gpu_prolip.Checks with the bar's floor selectable: measures every comparison,
    prints each figure, and fails at the end naming every one over its bar."""

    def __init__(self):
        self.over, self.worst = [], 0.0

    def __call__(self, name, got, want, e_ref, P0=None):
        want = np.asarray(want, dtype=np.float64)
        err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
        b = R.bar(e_ref, P0) if P0 is not None else R.bar_on(e_ref, want)
        ratio = err / b if b > 0 else (0.0 if err == 0 else math.inf)
        self.worst = max(self.worst, ratio)
        line = f"{name}: err {err:.3g}, e_ref {float(e_ref):.3g}, bar {b:.3g}, err/bar {ratio:.3f}"
        print(line)
        if not err <= b:
            self.over.append(line)

    def done(self):
        print(f"worst err/bar {self.worst:.3f}")
        assert not self.over, "over the bar: " + "; ".join(self.over)


# ------------------------------------------------------------------ inputs (CPU)
def _grid_x(n, D, g, pull=None):
    """Features on the grid k / 32, |k| <= 127: exact in fp32, fp16 and bf16."""
    raw = torch.randn(n, D, generator=g)
    if pull is not None:
        raw = raw + pull
    x = (32.0 * raw).round().clamp(-127, 127) / 32.0
    assert x.dtype == F32
    for dt in (F16, BF16):
        assert torch.equal(x.to(dt).float(), x), f"the feature grid does not survive {dt}"
    assert torch.equal(x.double().float(), x)
    return x


def _head(D, E, C, G, g):
    P0 = torch.randn(D, E, generator=g) * D ** -0.5
    P = torch.stack([P0 + 0.02 * torch.randn(D, E, generator=g) for _ in range(G)])
    W = torch.nn.functional.normalize(torch.randn(E, C, generator=g), dim=0)
    return P0, P, W


def _logits64(x, P, W):
    return SCALE * torch.nn.functional.normalize(x.double() @ P.double(), dim=-1) @ W.double()


def _min_gap(L):
    if L.shape[1] < 2:
        return math.inf
    top = L.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def _half_argmax_labels(L64, C, g):
    """About half the rows labelled with their fp64 argmax class, the rest at random:
    the correct count is neither 0 nor n."""
    n = L64.shape[0]
    rnd = torch.randint(0, C, (n,), generator=g)
    return torch.where(torch.rand(n, generator=g) < 0.5, L64.argmax(1), rnd)


def _autograd(x, y, P, W, dtype):
    """(d CE / d(x P), CE, correct count) of cross_entropy(100 normalize(x P) W, y) by
    torch autograd in `dtype`; labels outside [0, C) are not accepted here."""
    Z = (x.to(dtype) @ P.to(dtype)).detach().requires_grad_(True)
    L = SCALE * torch.nn.functional.normalize(Z, dim=-1) @ W.to(dtype)
    ce = torch.nn.functional.cross_entropy(L, y)
    ce.backward()
    return Z.grad.double().numpy(), float(ce.detach()), int((L.argmax(1) == y).sum())


def _references(x, y, P, W):
    """Per configuration: fp64 (dZ, CE, correct) and the fp32 evaluation's distances."""
    out = []
    for k in range(P.shape[0]):
        d64, ce64, ok64 = _autograd(x, y, P[k], W, torch.float64)
        d32, ce32, _ = _autograd(x, y, P[k], W, torch.float32)
        out.append(SimpleNamespace(dZ=d64, ce=ce64, ok=ok64, e_dZ=np.abs(d32 - d64).max(),
                                   e_ce=abs(ce32 - ce64)))
    return out


@functools.lru_cache(maxsize=None)
def _edge_case(n, D, E, C, G):
    """Inputs and CPU references of one edge shape, built once and left unchanged."""
    g = torch.Generator().manual_seed(1000 * n + D + E + C)
    x = _grid_x(n, D, g)
    P0, P, W = _head(D, E, C, G, g)
    L64 = [_logits64(x, P[k], W) for k in range(G)]
    y = _half_argmax_labels(L64[0], C, g)
    gap = min(_min_gap(L) for L in L64)
    assert gap >= MIN_GAP, f"top-2 logit gap {gap:.3g} < {MIN_GAP}: the exact count is not defined"
    return SimpleNamespace(x=x, y=y, P0=P0, P=P, W=W, ref=_references(x, y, P, W))


# ------------------------------------------------------------------ device calls
def _padded(t, dev, pad=64):
    """t on the device with `pad` NaNs (integers: nothing) right behind its last element."""
    t = t.contiguous()
    if not t.is_floating_point():
        return t.to(dev)
    buf = torch.full((t.numel() + pad,), float("nan"), dtype=t.dtype, device=dev)
    buf[:t.numel()] = t.reshape(-1).to(dev)
    return buf[:t.numel()].view(t.shape)


def _guarded(shape, dev, pad, fill=None):
    """(whole NaN buffer, its leading `shape` view): the `pad` elements behind are the canary."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + pad,), float("nan"), device=dev)
    view = buf[:numel].view(shape)
    if fill is not None:
        view.copy_(fill.to(dev))
    return buf, view


def _canary_ok(buf, numel):
    return bool(torch.isnan(buf[numel:]).all())


def _grad_call(x, y, W, P):
    """miclip_prolip_grad through the C ABI on guarded buffers: (dZ [G, n, E], part [G, nt, 2])
    as fp32 numpy arrays; the outputs must be finite and the canaries untouched."""
    from miclip import _lib, prolip
    lib = _lib.load_library()
    dev = torch.device("cuda")
    xd, yd, Wd, Pd = _padded(x, dev), y.to(dev), _padded(W.float(), dev), _padded(P.float(), dev)
    G, n, E = P.shape[0], x.shape[0], P.shape[2]
    nt = (n + 15) // 16
    dbuf, dZ = _guarded((G, n, E), dev, E)        # one more row of dZ
    pbuf, part = _guarded((G, nt, 2), dev, 2)     # one more row tile
    prolip._grad(lib, xd, yd, Wd, Pd, SCALE, dZ, part)
    torch.cuda.synchronize()
    assert _canary_ok(dbuf, dZ.numel()) and _canary_ok(pbuf, part.numel()), "wrote past an output"
    dZ, part = dZ.cpu().numpy(), part.cpu().numpy()
    assert np.isfinite(dZ).all() and np.isfinite(part).all()
    return dZ, part


def _ce_and_count(part, n):
    p = part.astype(np.float64)
    return p[:, :, 0].sum(1) / n, p[:, :, 1].sum(1)


# --------------------------------------------- 1. prolip_grad at edge shapes
EDGE_SHAPES = [           # (n, D, E, C, G)
    (1, 16, 16, 1, 1),         # every minimum; C = 1: CE = 0, dZ = 0, correct = 1, exactly
    (15, 16, 16, 2, 2),        # n below one tile
    (16, 48, 48, 16, 1),       # exact tile, no class padding, E/16 = 3
    (17, 32, 80, 17, 3),       # one row and one class over; E/16 = 5
    (33, 80, 64, 65, 2),       # Cp/16 = 5: the class-tile loop runs twice for wave 0
    (40, 64, 32, 1000, 1),     # Cp = 1008
    (20, 32, 1024, 1024, 1),   # the largest dynamic-LDS launch (131,840 B)
    (1100, 16, 16, 5, 2),      # 69 row tiles
    (8, 1280, 16, 3, 1),       # the largest D
]


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "n{}-D{}-E{}-C{}-G{}".format(*s))
def test_grad_edge_shapes_three_dtypes(shape):
    """dZ and the mean CE against fp64 autograd, the correct count exactly, fp16 / bf16
    features bit-equal to fp32, a configuration inside a G > 1 call bit-equal to a G = 1
    call on it alone.

    Measured on the MI355X, worst err / bar per shape as dZ / CE: n1-C1 0 / 0 (exact),
    n15 0.139 / 0.065, n16-C16 0.145 / 0.147, n17-C17 0.055 / 0.123, n33-C65 0.138 /
    0.059, n40-C1000 0.111 / 0.331, E1024-C1024 0.010 / 0.215, n1100 0.024 / 0.127,
    D1280 0.250 / 0.051; every count and every bitwise comparison holds."""
    n, D, E, C, G = shape
    c = _edge_case(*shape)
    _need_gpu()
    dZ, part = _grad_call(c.x, c.y, c.W, c.P)
    ce, ok = _ce_and_count(part, n)
    _check = Checks()
    for k in range(G):
        r = c.ref[k]
        _check(f"{shape} cfg {k} dZ", dZ[k], r.dZ, r.e_dZ, c.P0)
        _check(f"{shape} cfg {k} CE", ce[k], r.ce, r.e_ce, c.P0)
        assert ok[k] == r.ok, f"cfg {k}: correct count {ok[k]} != fp64's {r.ok}"
    if C == 1:
        assert not dZ.any() and not part[:, :, 0].any() and ok[0] == n
    for dt in (F16, BF16):      # the load widens exactly; nothing else depends on the type
        dZ_t, part_t = _grad_call(c.x.to(dt), c.y, c.W, c.P)
        assert np.array_equal(dZ_t, dZ) and np.array_equal(part_t, part), f"{dt} differs from fp32"
    if G > 1:
        for k in range(G):
            dZ_1, part_1 = _grad_call(c.x, c.y, c.W, c.P[k:k + 1])
            assert np.array_equal(dZ_1[0], dZ[k]) and np.array_equal(part_1[0], part[k]), \
                f"cfg {k} alone differs from cfg {k} of {G}"
    _check.done()


# ------------------------------------------------------------- 2. semantics
@pytest.mark.parametrize("a,b", [(3, 17), (4, 5)])
def test_first_maximum_wins_on_tied_logits(a, b):
    """Two identical columns a < b of W give two equal logits (same instruction sequence,
    same inputs); where the pair is the row maximum the arg-max is a, so rows labelled b
    count as wrong. Reference: fp64 logits with column b overwritten by column a (a BLAS
    need not return equal results for equal columns), torch.argmax = first maximum.
    Exact comparison; nothing to measure."""
    n, D, E, C, tied = 40, 64, 32, 20, 12
    g = torch.Generator().manual_seed(1000 * n + D + E + C + 7 * a + b)
    P0, P, W = _head(D, E, C, 1, g)
    W[:, b] = W[:, a]
    pull = torch.zeros(n, D)
    pull[:tied] = 5.0 * (W[:, a] @ torch.linalg.pinv(P[0]))
    x = _grid_x(n, D, g, pull)
    L64 = _logits64(x, P[0], W)
    L64[:, b] = L64[:, a]
    am = L64.argmax(1)
    assert bool((am[:tied] == a).all()), "the tied pair is not the maximum of the pulled rows"
    others = [k for k in range(C) if k != b]
    assert _min_gap(L64[:, others]) >= MIN_GAP
    y = _half_argmax_labels(L64, C, g)
    y[:tied:2], y[1:tied:2] = a, b
    want = int((am == y).sum())
    assert want <= n - tied // 2
    _need_gpu()
    _, part = _grad_call(x, y, W, P)
    assert _ce_and_count(part, n)[1][0] == want


def test_accuracy_counts_out_of_range_labels_as_wrong():
    """prolip.projector_accuracy with labels C, -1 and 2**40 (beyond int32: narrowed only
    after the range test) among valid ones equals 100 * mean(argmax == label) of the fp64
    logits: those rows are wrong, the rows around them unaffected. Exact comparison."""
    n, D, E, C, G = 37, 48, 32, 7, 2
    g = torch.Generator().manual_seed(1000 * n + D + E + C)
    x = _grid_x(n, D, g)
    P0, P, W = _head(D, E, C, G, g)
    L64 = [_logits64(x, P[k], W) for k in range(G)]
    assert min(_min_gap(L) for L in L64) >= MIN_GAP
    y = _half_argmax_labels(L64[0], C, g)
    for row, bad in ((0, C), (5, -1), (15, 2 ** 40), (16, 2 ** 40 + 3), (17, -2 ** 40), (36, C + 9)):
        y[row] = bad
    want = [100.0 * float((L.argmax(1) == y).double().mean()) for L in L64]
    assert all(0.0 < w < 100.0 for w in want)
    _need_gpu()
    from miclip import prolip
    for dt in (F32, F16, BF16):
        acc = prolip.projector_accuracy(P, x.to(dt), y, W)
        assert acc.shape == (G,) and list(acc) == pytest.approx(want, abs=1e-9), (dt, acc, want)


def test_zero_feature_row_is_clamped_not_nan():
    """An all-zero feature row: |z| = 0 is clamped to 1e-12, f = 0, the logits are 0, its
    CE is log C; everything stays finite, and every other row's dZ (and every other row
    tile's partials) is bit-equal to the same call with a normal row in its place, since
    rows share only n. The zero row is alone in the last row tile, so that tile's CE
    partial is the row's CE. e_ref: the row's CE by fp32 torch against fp64.

    Measured on the MI355X: CE of the zero row err / bar 0.105."""
    n, D, E, C = 33, 64, 32, 20
    g = torch.Generator().manual_seed(1000 * n + D + E + C)
    x_normal = _grid_x(n, D, g)
    P0, P, W = _head(D, E, C, 1, g)
    y = _half_argmax_labels(_logits64(x_normal, P[0], W), C, g)
    x = x_normal.clone()
    x[n - 1] = 0.0

    def row_ce(dtype):
        L = SCALE * torch.nn.functional.normalize(x[n - 1:].to(dtype) @ P[0].to(dtype), dim=-1) @ W.to(dtype)
        return float(torch.nn.functional.cross_entropy(L, y[n - 1:]))
    ce64 = row_ce(torch.float64)
    assert abs(ce64 - math.log(C)) < 1e-12
    _need_gpu()
    dZ, part = _grad_call(x, y, W, P)           # finite, or _grad_call fails
    dZ_n, part_n = _grad_call(x_normal, y, W, P)
    _check = Checks()
    _check("zero row CE", part[0, -1, 0], math.log(C), abs(row_ce(torch.float32) - ce64), P0)
    assert part[0, -1, 1] == float(y[n - 1] == 0)        # all logits equal: arg-max is class 0
    assert np.array_equal(dZ[0, :n - 1], dZ_n[0, :n - 1]) and np.array_equal(part[0, :-1], part_n[0, :-1])
    _check.done()


def test_grad_rerun_is_bit_equal():
    """The same call twice: equal bits in dZ and the partials (five class tiles, a row
    tail, two configurations). Exact comparison."""
    c = _edge_case(33, 80, 64, 65, 2)
    _need_gpu()
    first, again = _grad_call(c.x.half(), c.y, c.W, c.P), _grad_call(c.x.half(), c.y, c.W, c.P)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


# ----------------------------- 3. prolip_adam alone against torch.optim.Adam
ADAM_SHAPES = [        # (n, D, E)
    (1, 16, 16),          # one workgroup, three of its four waves idle
    (17, 48, 80),         # 3 x 5 sixteen-tiles: both halves of the tile guard
    (1100, 32, 16),       # 69 partials per configuration for the fold
    (33, 1280, 16),       # the largest D
]
ADAM_LRS = (1e-2, 1e-3, 3e-4)
ADAM_LAMS = (1.0, 0.0, 0.1)
LR_FACTOR, LAMBDA_DIV = 0.37, 3.0


def _f32(v):
    """The value a C float argument carries."""
    return float(np.float32(v))


def _adam_tiles(D, E):
    return ((D + 31) // 32) * ((E + 31) // 32)      # prolip_adam_tiles


def _torch_adam(x, dZ, P0, P, m, v, lr, lam, eps, step, dtype):
    """One torch.optim.Adam step in `dtype` from the given state: (P, m, v) after it."""
    p = P.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr * _f32(LR_FACTOR), eps=eps)
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.to(dtype).clone(),
                    "exp_avg_sq": v.to(dtype).clone()}
    with torch.no_grad():
        p.grad = x.to(dtype).t() @ dZ.to(dtype) + 2.0 * (lam / LAMBDA_DIV) * (p - P0.to(dtype))
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == step
    return tuple(t.detach().double().numpy() for t in (p, st["exp_avg"], st["exp_avg_sq"]))


@functools.lru_cache(maxsize=None)
def _adam_case(n, D, E, eps, step):
    """State, gradient inputs and the CPU references of one prolip_adam call (G = 3)."""
    G = len(ADAM_LRS)
    g = torch.Generator().manual_seed(1000 * n + D + E + 7 * step + (1 if eps < 1e-6 else 0))
    x = _grid_x(n, D, g)
    P0 = torch.randn(D, E, generator=g) * D ** -0.5
    P = torch.stack([P0 + 0.01 * torch.randn(D, E, generator=g) for _ in range(G)])
    if step == 1:
        m, v = torch.zeros(G, D, E), torch.zeros(G, D, E)
    else:
        m = 1e-3 * torch.randn(G, D, E, generator=g)
        v = (1e-3 * torch.randn(G, D, E, generator=g)) ** 2
    dZ = 0.05 / n * torch.randn(G, n, E, generator=g)
    nt = (n + 15) // 16
    gpart = torch.stack([48.0 * torch.rand(G, nt, generator=g),                  # CE sums of 16 rows
                         torch.randint(0, 17, (G, nt), generator=g).float()], dim=2)
    lrs, lams, eps = [_f32(v_) for v_ in ADAM_LRS], [_f32(v_) for v_ in ADAM_LAMS], _f32(eps)
    r64 = [_torch_adam(x, dZ[k], P0, P[k], m[k], v[k], lrs[k], lams[k], eps, step, torch.float64)
           for k in range(G)]
    r32 = [_torch_adam(x, dZ[k], P0, P[k], m[k], v[k], lrs[k], lams[k], eps, step, torch.float32)
           for k in range(G)]
    diff = P - P0
    mse64 = (diff.double() ** 2).sum((1, 2)).numpy()
    e_mse = np.abs((diff * diff).sum((1, 2)).double().numpy() - mse64).max()
    ce64 = gpart[:, :, 0].double().sum(1).numpy() / n
    e_ce = np.abs((gpart[:, :, 0].sum(1) / n).double().numpy() - ce64).max()
    return SimpleNamespace(x=x, P0=P0, P=P, m=m, v=v, dZ=dZ, gpart=gpart, lrs=lrs, lams=lams, eps=eps,
                           r64=r64, r32=r32, mse64=mse64, e_mse=e_mse, ce64=ce64, e_ce=e_ce,
                           ok=gpart[:, :, 1].double().sum(1).numpy())


def _adam_call(c, xdtype, step):
    """miclip_prolip_adam through the C ABI from c's starting state on guarded buffers:
    (P, m, v, mse_part [G, tiles], history [G, 3]) as numpy arrays."""
    from miclip import _lib
    lib = _lib.load_library()
    dev = torch.device("cuda")
    G, D, E = c.P.shape
    n = c.x.shape[0]
    x, dZ, P0, gpart = (_padded(t, dev) for t in (c.x.to(xdtype), c.dZ, c.P0, c.gpart))
    lr, lam = _padded(torch.tensor(c.lrs), dev), _padded(torch.tensor(c.lams), dev)
    bufs = [_guarded((G, D, E), dev, E, fill) for fill in (c.P, c.m, c.v)]
    bufs += [_guarded((G, _adam_tiles(D, E)), dev, 4), _guarded((G, 3), dev, 3)]
    ptr = [ctypes.c_void_p(view.data_ptr()) for _, view in bufs]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.miclip_prolip_adam(
        p(x), _lib.MICLIP_F32 if xdtype == F32 else _lib.MICLIP_BF16, p(dZ), n, D, E, G, p(P0),
        ptr[0], ptr[1], ptr[2], p(lr), p(lam), LR_FACTOR, LAMBDA_DIV, step, c.eps, p(gpart),
        ptr[3], ptr[4], _lib.stream_handle(dev)), "miclip_prolip_adam")
    torch.cuda.synchronize()
    out = []
    for name, (buf, view) in zip(("P", "m", "v", "mse_part", "history"), bufs):
        assert _canary_ok(buf, view.numel()), f"wrote past {name}"
        out.append(view.cpu().numpy())
        assert np.isfinite(out[-1]).all(), f"{name} not written everywhere"
    return out


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("eps", [1e-4, 1e-8])
@pytest.mark.parametrize("shape", ADAM_SHAPES, ids=lambda s: "n{}-D{}-E{}".format(*s))
def test_adam_alone_matches_torch_adam(shape, eps, step):
    """One miclip_prolip_adam call of three configurations (three lr, three lambda with a
    zero, lr_factor 0.37, lambda_div 3) from a given state (m = v = 0 at step 1, random
    otherwise) against torch.optim.Adam preloaded with that state, fp64 the yardstick and
    fp32 the e_ref; the MSE partials (prolip_adam_tiles(D, E) per configuration) and the
    folded history {sum CE / n, MSE, correct}; bf16 features bit-equal to fp32; a second
    call from the same state bit-equal.

    Measured on the MI355X, worst err / bar over the 24 cases: P 0.665, m 0.217,
    v 0.327, sum of the MSE partials 0.058, history MSE 0.544, history CE 0.250. The
    step moves a weight by 1.1e-4 at the least and, with eps 1e-8 on a small random v,
    by up to 4.9, against bars of 1e-6 .. 9e-5."""
    n, D, E = shape
    c = _adam_case(n, D, E, eps, step)
    _need_gpu()
    P, m, v, mpart, hist = _adam_call(c, F32, step)
    _check = Checks()
    for k in range(P.shape[0]):
        (P64, m64, v64), (P32, m32, v32) = c.r64[k], c.r32[k]
        moved = np.abs(P64 - c.P[k].double().numpy()).max()
        print(f"{shape} eps {eps} step {step} cfg {k}: the step moves P by up to {moved:.3g}")
        _check(f"cfg {k} P", P[k], P64, np.abs(P32 - P64).max(), c.P0)
        _check(f"cfg {k} m", m[k], m64, np.abs(m32 - m64).max())
        _check(f"cfg {k} v", v[k], v64, np.abs(v32 - v64).max())
    assert mpart.shape == (P.shape[0], _adam_tiles(D, E))
    _check("MSE partials", mpart.astype(np.float64).sum(1), c.mse64, c.e_mse, c.P0)
    _check("history MSE", hist[:, 1], c.mse64, c.e_mse, c.P0)
    _check("history CE", hist[:, 0], c.ce64, c.e_ce, c.P0)
    assert np.array_equal(hist[:, 2], c.ok)
    again = _adam_call(c, F32, step)
    bf = _adam_call(c, BF16, step)
    for name, first, second, third in zip(("P", "m", "v", "mse_part", "history"),
                                          (P, m, v, mpart, hist), again, bf):
        assert np.array_equal(first, second), f"{name}: the second call differs"
        assert np.array_equal(first, third), f"{name}: bf16 features differ from fp32"
    _check.done()
