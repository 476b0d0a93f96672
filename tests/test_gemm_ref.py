"""CPU: the GEMM yardstick (tests/_gemm_ref.py) against torch's own CPU arithmetic, the
launcher plan it restates against values worked out by hand from csrc/gemm.hip, and the
conditions the activation sweep of tests/test_gpu_gemm_exact.py rests on. No GPU, no
project kernel."""
import math

import pytest
import torch

import _gemm_ref as G

F16, BF16, F32 = G.F16, G.BF16, G.F32


def _ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _grid_case(seed=0, M=37, N=128, K=192):
    g = torch.Generator().manual_seed(seed)
    A, W = _ints(g, M, K), _ints(g, N, K)
    bias = _ints(g, N, lo=-16384, hi=16384) * 0.25
    return g, A, W, bias


def _bf16_rne_bits(x32):
    b = x32.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return (b - ((b >> 31) << 32)).to(torch.int32).view(F32)


# ------------------------------------------------------------------ emulations
@pytest.mark.parametrize("T", [F16, BF16])
def test_store_and_f32_match_torch_fp32_linear(T):
    g, A, W, bias = _grid_case()
    v = G.ref64(A, W, bias)
    assert G.is_fp32_exact(v) and v.abs().max() <= 9 * 192 + 4096
    lin = torch.nn.functional.linear(A.float(), W.float(), bias.float())   # exact: integers
    assert torch.equal(G.emu_f32(v), lin)
    assert torch.equal(G.emu_store(v, T), lin.to(T))
    # the store really rounds on this grid, and bf16 RNE is the bit formula
    assert (G.emu_store(v, T).double() != v).float().mean() > 0.25
    assert torch.equal(G.emu_store(v, BF16).float(), _bf16_rne_bits(v.float()))
    S = G.absdot(A, W, bias)
    assert (S >= v.abs()).all() and torch.equal(S, A.abs() @ W.abs().t() + bias.abs())


def test_residuals_match_torch_cpu_arithmetic():
    g, A, W, bias = _grid_case(1)
    v = G.ref64(A, W, bias)
    x32 = torch.randn(v.shape, generator=g) * 1000
    assert torch.equal(G.emu_resid32(x32, v), x32 + v.float())
    xh = (64 * torch.randn(v.shape, generator=g)).to(F16)
    th = v.float().to(F16)
    want = xh + th                                    # torch's CPU half add
    got = G.emu_resid16(xh, v)
    assert got.dtype == F16 and torch.equal(got, want)
    assert torch.equal(got, (xh.float() + th.float()).to(F16))    # epilogue.h's fp32 form
    # cancellation, overflow to inf and subnormal sums, on hand-made pairs
    a = torch.tensor([1.0, 65504.0, 6e-8, -1024.0, 0.1], dtype=F16)
    b = torch.tensor([-1.0, 65504.0, 6e-8, 1024.5, 0.2], dtype=torch.float64)
    assert torch.equal(G.emu_resid16(a, b).float().nan_to_num(posinf=7.0),
                       (a + b.to(F16)).float().nan_to_num(posinf=7.0))


@pytest.mark.parametrize("stream", [F32, F16])
@pytest.mark.parametrize("npatch", [1, 3, 49])
def test_patch_and_class_token_rows(stream, npatch):
    g = torch.Generator().manual_seed(npatch)
    B, N = 3, 128
    acc = _ints(g, B * npatch, N, lo=-1000, hi=1000)
    pos = torch.randn(npatch + 1, N, generator=g) * 3
    cls = torch.randn(N, generator=g)
    X0 = torch.full((B * (npatch + 1), N), -7.0).to(stream)
    X = G.emu_patch(acc, pos, npatch, X0)
    want = X0.clone()
    for b in range(B):
        for p in range(npatch):
            want[b * (npatch + 1) + 1 + p] = (acc[b * npatch + p].float() + pos[1 + p]).to(stream)
    assert torch.equal(X, want)
    assert (X[::npatch + 1] == -7.0).all(), "class rows keep the canary"
    rows = G.patch_rows(B * npatch, npatch)
    assert len(set(rows.tolist())) == B * npatch and rows.max() == B * (npatch + 1) - 1
    Y = G.emu_class_token(cls, pos, npatch + 1, X)
    assert torch.equal(Y[::npatch + 1], (cls + pos[0]).to(stream).expand(B, N))
    keep = torch.ones(len(Y), dtype=torch.bool)
    keep[::npatch + 1] = False
    assert torch.equal(Y[keep], X[keep]) and not (Y == -7.0).any()


def test_ln_store_exact_on_the_integer_grid():
    g, A, W, _ = _grid_case(2)
    M, N = A.shape[0], W.shape[0]
    acc = G.ref64(A, W)
    mu = _ints(g, M, lo=-4, hi=4)
    colsum = _ints(g, N, lo=-64, hi=64)
    rs = 2.0 ** -_ints(g, M, lo=0, hi=6)
    c = _ints(g, N, lo=-16384, hi=16384) * 0.25
    assert G.ln_grid_exact(acc, mu, rs, colsum, c)
    z = G.emu_ln_store(acc, mu, rs, colsum, c)
    f = lambda t: t.float()  # noqa: E731
    want = f(rs)[:, None] * (f(acc) - f(mu)[:, None] * f(colsum)[None]) + f(c)[None]   # fp32, exact
    assert torch.equal(z.float(), want) and G.is_fp32_exact(z)
    assert torch.equal(z, G.ref64_ln(A, W, mu, rs, colsum, c))
    # with rounding fmas the emulation still rounds exactly twice
    rs2 = torch.rand(M, generator=g).double() + 0.5
    z2 = G.emu_ln_store(acc, mu, rs2.float(), colsum, c)
    assert G.is_fp32_exact(z2) and not G.ln_grid_exact(acc, mu, rs2.float(), colsum, c)
    r64 = G.ref64_ln(A, W, mu, rs2.float(), colsum, c)
    assert ((z2 - r64).abs() <= 2.0 ** -23 * G.absdot_ln(A, W, mu, rs2.float(), colsum, c)).all()


# ------------------------------------------------------------------ activations, interval
def test_activations_float64():
    v = torch.linspace(-40, 40, 16001, dtype=torch.float64)
    ge = torch.tensor([0.5 * x * math.erfc(-x / math.sqrt(2.0)) for x in v.tolist()],
                      dtype=torch.float64)
    rel = ((G.gelu64(v) - ge).abs() / ge.abs().clamp_min(1e-300)).max().item()
    assert rel <= 1e-13, rel
    qu = torch.tensor([x / (1.0 + math.exp(-1.702 * x)) for x in v.tolist()], dtype=torch.float64)
    rel = ((G.quick64(v) - qu).abs() / qu.abs().clamp_min(1e-300)).max().item()
    assert rel <= 1e-14, rel
    near = torch.linspace(-6, 6, 2001, dtype=torch.float64)
    assert torch.allclose(G.gelu64(near), torch.nn.functional.gelu(near), rtol=0, atol=1e-15)
    assert torch.allclose(G.quick64(near), near * torch.sigmoid(1.702 * near), rtol=0, atol=1e-15)
    # saturation: no NaN anywhere on the line, -0 / v at the ends
    ends = torch.tensor([-65504.0, -8704.0, -100.0, 0.0, 100.0, 8704.0, 65504.0], dtype=torch.float64)
    for act in (G.ACT_QUICKGELU, G.ACT_GELU):
        y = G.act64(ends, act)
        assert not y.isnan().any() and (y[:3].abs() < 1e-30).all() and torch.equal(y[4:], ends[4:])


def test_activations_lipschitz_below_1_13():
    v = torch.linspace(-20, 20, 4_000_001, dtype=torch.float64)
    for act, want in ((G.ACT_GELU, 1.129), (G.ACT_QUICKGELU, 1.100)):
        y = G.act64(v, act)
        slope = ((y[1:] - y[:-1]) / (v[1:] - v[:-1])).abs().max().item()
        print(f"act {act}: max |slope| {slope:.4f}")
        assert abs(slope - want) < 1e-3 and slope < G.ACT_LIPSCHITZ


@pytest.mark.parametrize("T", [F16, BF16, F32])
def test_interval_ok(T):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4096, generator=g).double() * 8
    out = G.to_T(x, T)
    assert G.interval_ok(out, x, x, T).all()
    assert G.interval_ok(out, x - 1e-3, x + 1e-3, T).all()
    up = torch.nextafter(out.float(), torch.full_like(out.float(), math.inf)).to(T) if T == F32 else \
        (out.view(torch.int16) + torch.where(out >= 0, 1, -1).to(torch.int16)).view(T)
    assert not G.interval_ok(up, x, x, T).any(), "the neighbour of T(x) is outside [x, x]"
    nan = torch.full_like(out, math.nan)
    assert not G.interval_ok(nan, x - 1, x + 1, T).any()
    z = torch.zeros(2, dtype=T)
    assert G.interval_ok(-z, z.double(), z.double(), T).all(), "-0 is the rounding of 0 too"
    assert torch.equal(G.to_T(torch.tensor([65504.0, 65520.0]).double(), F16).float(),
                       torch.tensor([65504.0, math.inf]))
    assert G.to_T(torch.tensor([65504.0]).double(), BF16).item() == 65536.0


# ------------------------------------------------------------------ the sweep's grid
def test_fp16_grid():
    v = G.fp16_grid()
    assert v.numel() == 36866 + 6 and v.unique().numel() == 36866 + 5     # +0 == -0
    body = v[:36866]
    assert (body.abs() <= 16).all() and (body.abs() >= 2.0 ** -14).all()
    assert torch.equal(body.to(F16).double(), body)
    assert body.abs().max() == 16 and body.abs().min() == 2.0 ** -14
    assert set(v[36866:].tolist()) == {0.0, 100.0, -100.0, 65504.0, -65504.0}
    assert math.copysign(1.0, v[36867].item()) == -1.0


@pytest.mark.parametrize("act,T,cap,measured", [
    (G.ACT_GELU, F16, 0.06, 0.0505), (G.ACT_GELU, BF16, 0.06, 0.0129),
    (G.ACT_QUICKGELU, F16, 0.01, 0.0034), (G.ACT_QUICKGELU, BF16, 0.01, 0.0045)])
def test_ambiguous_share_of_the_grid(act, T, cap, measured):
    """The sweep accepts either neighbour only where T(y - e) != T(y + e); that must stay
    a small share of the grid or the sweep pins nothing."""
    v = G.fp16_grid()
    share = G.ambiguous(v, act, T).double().mean().item()
    print(f"act {act} {T}: ambiguous share {share:.4%}")
    assert share <= cap
    assert abs(share - measured) < 5e-4
    y = G.act64(v, act)
    assert not y.isnan().any() and G.act_ok(G.to_T(y, T), v, act, T).all()


# ------------------------------------------------------------------ the launcher's plan
def test_plan_tail_table_at_256_cus():
    assert G.plan_tail(16421, 1024, 256) == (64, 48, 0)      # 37 tail rows: 3 x 16 narrow tasks
    assert 16421 - 64 * 256 == 37
    assert G.plan_tail(4352, 4096, 256) == (16, 256, 1)      # 256 tail rows: 8 x 32 wide tasks
    assert 4352 - 16 * 256 == 256
    assert G.plan_tail(300, 256, 256) == (2, 0, 0)           # fewer tile-rows than a round
    assert G.plan_tail(16384 + 257, 1024, 256) == (66, 0, 0)  # more than 256 rows left over
    assert G.plan_tail(16384, 1024, 256) == (64, 0, 0)
    assert G.plan_tail(8224, 1024, 256, 128) == (64, 32, 0)  # 128-row tiles + 32 rows: 2 x 16 tasks
    assert G.tail_step(1024, 256) == 64 and G.tail_step(4096, 256) == 16
    assert G.tail_step(768, 256) == 256 and G.tail_step(1024, 304) == 76
    assert G.wide_tail_shape(256) == (4096 + 256, 4096)


def test_choose_rows_and_launch_choice_at_256_cus():
    assert G.choose_rows(8224, 1024, 256) == (3, (43, 0, 0))         # 260 tiles of 128 > 256, 172 of 192
    assert G.choose_rows(12850, 768, 256) == (3, (67, 0, 0))         # 150 -> 201 tiles of 192
    assert G.choose_rows(4112, 1024, 256) == (2, (33, 0, 0))         # 132 tiles of 128 rows
    assert G.choose_rows(16421, 1024, 256) == (4, (64, 48, 0))
    assert G.launch_choice(16421, 1024, 1024, 256) == ("persistent", (64, 48, 0))
    assert G.launch_choice(16421, 1024, 1024, 256, tracc=False) == ("persistent", (64, 48, 0))
    assert G.launch_choice(16421, 1024, 64, 256) == ("tile256", (64, 48, 0))     # one K-tile
    assert G.launch_choice(12544, 768, 768, 256, patch=True) == ("tile256", (49, 0, 0))
    assert G.launch_choice(12850, 768, 768, 256)[0] == "rows192"
    assert G.launch_choice(12850, 768, 768, 256, tracc=False)[0] == "persistent"
    assert G.launch_choice(4112, 1024, 1024, 256)[0] == "rows128"     # 16 images of ViT-L/14
    assert G.launch_choice(4112, 1024, 1024, 256, tracc=False)[0] == "tile128"
    assert G.launch_choice(77, 512, 512, 256)[0] == "tile128"
    assert G.launch_choice(257, 384, 1024, 256)[0] == "tile128"       # N % 256 != 0
    assert not G.shape_ok(16, 100, 64) and not G.shape_ok(16, 128, 96) and not G.shape_ok(0, 128, 64)
