"""CPU: self-checks of the float64 attention yardstick (tests/_attn_ref.py).

  * attention() equals torch's scaled_dot_product_attention in float64 on the CPU (causal
    and not, head dim 64 and 80); round_to() equals torch's fp32 -> fp16 / bf16 casts;
  * every input family has its stated property (values exact in T, the indicator's closed
    form, the one-hot margin >= 40 log2 units, the staircase's step per 32-key tile);
  * the bar max(4, E_T) u U discriminates: a float64 attention whose P and output are
    rounded to T (and the same with q c2 rounded to T first, as the kernels' shifted
    softmax does) passes it on every family, and the same attention with
      (a) the last key dropped, (b) the last key counted twice, (d) the causal mask off by
      one                               is rejected on the indicator-V family,
      (c) two V rows swapped            is rejected on the random family.
    Measured here (ratios in u U): unmutated <= 1.5 (<= 3.3 with the rounded q c2);
    (a) >= 256, (b) >= 251, (d) an element that must be exactly 0 is not, (c) >= 480;
    E_T 3.6-7.7 on random data, 0.9-1.7 on indicator-V, 6.7-98 on the rising staircases,
    1.6-2.5 on the falling one (so its bar is the derived 4).
"""
import numpy as np
import pytest
import torch

import _attn_ref as R

CASES = [(77, 64, 1), (257, 64, 0), (640, 64, 0), (416, 80, 0)]      # (N, dh, causal)
B, H = 2, 3
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("dh", [64, 80])
@pytest.mark.parametrize("causal", [0, 1])
def test_attention_equals_torch_float64(dh, causal):
    N = 77
    qkv = R.random(B, N, H, dh, "fp16", 3 + dh + causal)
    out, U = R.attention(qkv, B, N, H, dh, causal)
    q, k, v = (torch.from_numpy(np.ascontiguousarray(a)) for a in R.split(qkv, B, N, H, dh))
    mask = torch.full((N, N), float("-inf"), dtype=torch.float64).triu_(1) if causal else None
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    assert ref.dtype == torch.float64
    ref = ref.permute(0, 2, 1, 3).reshape(B * N, H * dh).numpy()
    err = float(np.abs(out - ref).max())
    print(f"dh={dh} causal={causal}: max |attention - torch float64| {err:.3g}")
    assert err <= 1e-13
    # U with V >= 0 is the output itself; and |out| <= U always
    out2, U2 = R.attention(np.abs(qkv), B, N, H, dh, causal)
    assert np.array_equal(out2, U2) and (np.abs(out) <= U * (1 + 1e-15)).all()


@pytest.mark.parametrize("T", ["fp16", "bf16"])
def test_round_to_equals_torch_cast(T):
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 3, 4000),
                        [0.0, 1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]])
    want = torch.from_numpy(x).float().to(TDT[T]).double().numpy()
    assert np.array_equal(R.round_to(x, T), want)
    assert R.is_exact(want, T) and not R.is_exact([1.0 + 2.0 ** -12], T)


def test_pack_split_roundtrip():
    x = np.arange(2 * 5 * 3 * 3 * 4, dtype=np.float64).reshape(2 * 5, 3 * 3 * 4)
    q, k, v = R.split(x, 2, 5, 3, 4)
    assert np.array_equal(R.pack(q, k, v), x)
    # torch's in_proj order: q | k | v, heads inside each
    assert q[1, 2, 3, 1] == x[1 * 5 + 3, 0 * 12 + 2 * 4 + 1]
    assert v[1, 2, 3, 1] == x[1 * 5 + 3, 2 * 12 + 2 * 4 + 1]
    assert np.array_equal(R.merge(q), x[:, :12])


# ------------------------------------------------------------------ the families
@pytest.mark.parametrize("T", ["fp16", "bf16"])
@pytest.mark.parametrize("N,dh,causal", CASES + [(1, 64, 0), (2, 80, 1), (33, 64, 1), (768, 80, 0)])
def test_family_properties(N, dh, causal, T):
    u = R.UNIT[T]
    # random: exact in T, the stated spread
    x = R.random(B, N, H, dh, T, 1)
    assert R.is_exact(x, T) and np.array_equal(x, R.random(B, N, H, dh, T, 1))
    if N >= 64:
        assert abs(x.std() - 1.5) < 0.05
    # indicator-V: exact values, one k* per head from the documented set, the closed form
    x, kstar, want = R.indicator_v(B, N, H, dh, T, 2, causal)
    assert R.is_exact(x, T)
    q, _, v = R.split(x, B, N, H, dh)
    assert (q == 0).all()
    keys = R.indicator_keys(N)
    assert keys[0] == N - 1 and set(keys) <= {0, 31, 32, 32 * ((N - 1) // 32), N - 2, N - 1, 255, 256}
    assert kstar.ravel().tolist() == [keys[i % len(keys)] for i in range(B * H)]
    for b in range(B):
        for h in range(H):
            nz = np.flatnonzero(np.abs(v[b, h]).sum(axis=1))
            assert nz.tolist() == [kstar[b, h]]
            assert np.array_equal(v[b, h, kstar[b, h]], (np.arange(dh) + 1) / 8.0)
    out, U = R.attention(x, B, N, H, dh, causal)
    assert np.abs(out - want).max() <= 1e-15 and np.array_equal(out, U)
    assert ((U == 0) == (want == 0)).all()
    if causal and N > 1:
        assert (U == 0).any()       # the rows before k*: exact zeros are demanded there
    # ... and no expected value is subnormal in T (u U would stop being the rounding unit)
    assert want[want > 0].min() >= 2.0 ** -14
    # one-hot: the winner's margin, the expected rows
    x, t, want = R.one_hot(B, N, H, dh, T, 3, causal)
    assert R.is_exact(x, T)
    assert (t >= 0).all() and (t < N).all() and (not causal or (t <= np.arange(N)).all())
    margin = R.one_hot_margin(x, B, N, H, dh, causal)
    out, _ = R.attention(x, B, N, H, dh, causal)
    print(f"N={N} dh={dh} causal={causal} {T}: one-hot margin {margin:.1f} log2 units")
    assert margin >= 40.0
    assert np.abs(out - want).max() <= 2.0 ** -39 * np.abs(want).max() * N
    # staircase: the step per tile, up to the rounding of K[j, 0] (|K| u each side)
    for step in R.STEPS:
        x = R.staircase(B, N, H, dh, T, 4, step)
        assert R.is_exact(x, T)
        q, k, _ = R.split(x, B, N, H, dh)
        # largest |K|: 158 at N = 640 (dh 64), 214 at the CLS kernel's N = 768 (dh 80)
        assert (q[..., 0] == 8.0).all() and np.abs(k).max() <= (159.0 if N <= 640 else 215.0)
        got = R.staircase_steps(x, B, N, H, dh)
        assert len(got) == (N - 1) // 32
        if len(got):
            tol = 2 * u * abs(step) * ((N - 1) // 32)
            assert np.abs(got - step).max() <= tol, (step, got)
            k0 = k[0, 0, :, 0]
            assert all(len(set(k0[i:i + 32])) == 1 for i in range(0, N, 32))
    # the two steps around the threshold really straddle it on fp16's finer grid
    if T == "fp16" and N > 64:
        lo = R.staircase_steps(R.staircase(B, N, H, dh, T, 4, 7.5), B, N, H, dh)
        hi = R.staircase_steps(R.staircase(B, N, H, dh, T, 4, 8.5), B, N, H, dh)
        assert lo.max() < 8.0 < hi.min()


# ------------------------------------------------------------------ the bar discriminates
def emulated(qkv, N, dh, causal, T, mut=None, prescale=False):
    """A float64 attention whose P (unnormalised, relative to the row max) and output are
    rounded to T; prescale: q c2 rounded to T first, the scores in the base-2 domain.
    mut: "drop" / "dup" (the last key), "swap" (two V rows), "mask" (causal mask off by one)."""
    q, k, v = R.split(qkv, B, N, H, dh)
    vis = R.visible(N, causal)
    if mut == "mask":
        vis = np.tril(np.ones((N, N), dtype=bool), 1)
    w = vis.astype(np.float64)
    if mut == "drop":
        w[:, N - 1] = 0.0
    if mut == "dup":
        w[:, N - 1] *= 2.0
    if mut == "swap":
        v = v.copy()
        v[:, :, [0, N // 2]] = v[:, :, [N // 2, 0]]
    if prescale:
        s = R.round_to(q * (R.LOG2E * dh ** -0.5), T) @ np.swapaxes(k, -1, -2)
    else:
        s = (q @ np.swapaxes(k, -1, -2)) * (R.LOG2E * dh ** -0.5)
    s = np.where(w > 0, s, -np.inf)
    p = np.exp2(s - s.max(axis=-1, keepdims=True))
    P = R.round_to(p, T) * w
    return R.merge(R.round_to((P @ v) / (p * w).sum(axis=-1, keepdims=True), T))


def _families(N, dh, causal, T):
    out = {"random": R.random(B, N, H, dh, T, 11),
           "indicator": R.indicator_v(B, N, H, dh, T, 12, causal)[0],
           "one-hot": R.one_hot(B, N, H, dh, T, 13, causal)[0]}
    for step in R.STEPS:
        out[f"stairs{step:+g}"] = R.staircase(B, N, H, dh, T, 14, step)
    return out


@pytest.mark.parametrize("T", ["fp16", "bf16"])
@pytest.mark.parametrize("N,dh,causal", CASES)
def test_bar_discriminates(N, dh, causal, T):
    u = R.UNIT[T]
    fam = _families(N, dh, causal, T)
    yard = {}
    for name, x in fam.items():
        out, U = R.attention(x, B, N, H, dh, causal)
        ref_T = R.reference_arithmetic(x, B, N, H, dh, causal, T)
        yard[name] = (out, U, R.bar(out, U, ref_T, u), R.e_t(out, U, ref_T, u))
        # the unmutated attention passes, in both forms
        for pre in (False, True):
            got = emulated(x, N, dh, causal, T, None, pre)
            r = R.ratio(got, out, U, u)
            print(f"N={N} dh={dh} causal={causal} {T} {name}: E_T {yard[name][3]:.2f}, "
                  f"unmutated{' (q c2 rounded)' if pre else ''} {r:.2f} u U")
            assert R.within(got, out, yard[name][2]), (name, pre, r)
            assert r <= max(4.0, yard[name][3])
    # the indicator's bar is the derived 4: its reference arithmetic is nearly exact
    assert yard["indicator"][3] <= 4.0

    def rejected(name, mut):
        out, U, bound, _ = yard[name]
        got = emulated(fam[name], N, dh, causal, T, mut)
        r = R.ratio(got, out, U, u)
        print(f"N={N} dh={dh} causal={causal} {T} {name}: mutation {mut} {r:.3g} u U")
        return not R.within(got, out, bound), r

    for mut in ("drop", "dup") + (("mask",) if causal else ()):
        hit, r = rejected("indicator", mut)
        assert hit and r >= 250.0, (mut, r)
    hit, r = rejected("random", "swap")
    assert hit and r >= 90.0, r
