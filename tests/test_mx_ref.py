"""CPU: tests/_mx_ref.py, the float64 yardstick of tests/test_gpu_mx_exact.py, checked against
torch's float8_e4m3fn, exact rationals and oracle/mx_oracle.py -- and every acceptance
function shown to REJECT a planted fault of the kind the GPU test exists to catch."""
import math

import numpy as np
import pytest
import torch

import _mx_ref as X
from oracle import mx_oracle


# ------------------------------------------------------------------ e4m3fn
def test_decode_table_is_torch_float8_e4m3fn():
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    ref = codes.view(torch.float8_e4m3fn).double()
    got = X.decode(codes)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert int(torch.isnan(got).sum()) == 2
    ok = ~torch.isnan(ref)
    assert torch.equal(got[ok], ref[ok])
    assert torch.equal(torch.signbit(got[ok]), torch.signbit(ref[ok]))
    assert X.E4M3[0x7E] == 448.0 and X.E4M3[0x01] == 2.0 ** -9 and X.E4M3[0x08] == 2.0 ** -6


def test_encode_round_trips_and_ties_to_even_at_every_midpoint():
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    assert torch.equal(X.encode(X.decode(codes)), codes)
    mag = torch.tensor(X.E4M3[:127], dtype=torch.float64)
    for sign in (1.0, -1.0):
        for i in range(126):
            lo, hi = float(mag[i]), float(mag[i + 1])
            mid = (lo + hi) / 2
            even = i if i % 2 == 0 else i + 1
            off = 128 if sign < 0 else 0
            y = torch.tensor([mid, math.nextafter(mid, 0.0), math.nextafter(mid, 1e9)],
                                 dtype=torch.float64) * sign
            assert X.encode(y).tolist() == [even + off, i + off, i + 1 + off], (i, sign)
    # 2^-10 ties to zero; above 448 saturates; the sign of zero is kept
    y = torch.tensor([2.0 ** -10, -2.0 ** -10, 1e9, -1e9, 0.0, -0.0, 464.0, 480.0], dtype=torch.float64)
    assert X.encode(y).tolist() == [0, 0x80, 0x7E, 0xFE, 0, 0x80, 0x7E, 0x7E]


def test_encode_agrees_with_torch_cast_on_random_values():
    g = torch.Generator().manual_seed(1)
    y = (torch.randn(200000, generator=g) * torch.exp2(torch.randint(-12, 9, (200000,), generator=g).float()))
    y = y.clamp(-448, 448)
    assert torch.equal(X.encode(y.double()), y.to(torch.float8_e4m3fn).view(torch.uint8))


# ------------------------------------------------------------------ the exponent rule
def test_rule_exponent_on_boundaries_against_rationals():
    vals = []
    for k in list(range(-127, -118)) + list(range(-30, 31)) + [100, 118, 119]:
        b = float(np.ldexp(np.float32(448.0), k))
        for a in (b, float(np.nextafter(np.float32(b), np.float32(0))),
                  float(np.nextafter(np.float32(b), np.float32(np.inf)))):
            if a > 0 and math.isfinite(a):
                vals.append(a)
    vals += [0.0, float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny), 2.0 ** -149, 1.0, 448.0, 449.0]
    got = X.rule_exponent(torch.tensor(vals, dtype=torch.float64)).tolist()
    want = [X.rule_exponent_rational(a) for a in vals]
    assert got == want
    assert X.rule_exponent(torch.tensor([0.0, 448.0, 449.0, 896.0, 896.5, 224.0, 2.0 ** -126, X.TINY / 2,
                                         math.nextafter(X.TINY / 2, 1.0)], dtype=torch.float64)).tolist() == \
        [-127, 0, 1, 1, 2, -1, -127, -127, -126]


def test_rule_exponent_agrees_with_oracle_bit_trick_over_the_normal_range():
    """Where amax / 448 is a normal fp32 number the oracle's (= the kernel's) bit trick is the
    rule: every exponent, 2^16 mantissas spread over the 2^23, the 3 mantissas around 7/8."""
    man = np.concatenate([np.arange(0, 1 << 23, 127, dtype=np.uint32),
                          np.array([0x600000 - 1, 0x600000, 0x600000 + 1, 0x7FFFFF], dtype=np.uint32)])
    for ex in list(range(10, 254, 9)) + [254]:      # amax >= 2^-117: amax / 448 normal
        a = ((np.uint32(ex) << 23) | man).view(np.float32)
        got = X.rule_exponent(torch.from_numpy(a.astype(np.float64))).numpy()
        assert np.array_equal(got, mx_oracle.mx_exponent(a)), ex


# ------------------------------------------------------------------ the scale plane
@pytest.mark.parametrize("R,K", [(1, 128), (600, 1280), (257, 384), (512, 256)])
def test_scale_index_is_a_bijection_onto_the_plane(R, K):
    Rp = (R + 255) // 256 * 256
    idx = X._plane_idx(Rp, K, "cpu").ravel()
    assert idx.numel() == X.scale_bytes(R, K)
    assert torch.equal(idx.sort().values, torch.arange(X.scale_bytes(R, K)))
    # the layout comment: one 1-KiB block per (256-row block, 128-k tile); inside it
    # [k-block 4][row & 15][row >> 4 & 15]
    plane = torch.arange(X.scale_bytes(R, K)).reshape(Rp // 256, K // 128, 4, 16, 16)
    for r, kb in ((0, 0), (R - 1, K // 32 - 1), (R // 2, 1), (min(R - 1, 37), 2)):
        assert int(plane[r // 256, kb // 4, kb % 4, r % 16, (r // 16) % 16]) == \
            int(X.scale_index(torch.tensor(r), torch.tensor(kb), K // 128))
    # and the oracle's restatement of common.h agrees
    r, kb = np.meshgrid(np.arange(R), np.arange(K // 32), indexing="ij")
    assert np.array_equal(mx_oracle.scale_index(r, kb, K // 128), X._plane_idx(R, K, "cpu").numpy())


def test_plane_round_trip_and_tail():
    g = torch.Generator().manual_seed(0)
    E = torch.randint(-127, 127, (300, 12), generator=g)
    S = X.write_plane(E, 384, fill=7, tail=X.PLANE_TAIL)
    assert S.numel() == X.scale_bytes(300, 384) + 256
    assert torch.equal(X.read_plane(S, 300, 384), E)
    assert X.plane_tail_untouched(S, 300, 384)


def test_quantize_agrees_with_oracle_and_round_trips():
    g = np.random.default_rng(0)
    x = (g.standard_normal((37, 256)) * np.exp2(g.integers(-8, 8, (37, 8))).repeat(32, 1)).astype(np.float32)
    x[3, 32:64] = 0
    q, E = X.quantize(torch.from_numpy(x).double())
    q0, E0 = mx_oracle.quantize(x)
    assert np.array_equal(E.numpy(), E0) and np.array_equal(q.numpy(), q0)
    d = X.dequantize(q, E)
    assert np.array_equal(d.numpy(), mx_oracle.dequantize(q0, E0).astype(np.float64))
    assert bool((X.block_amax(torch.from_numpy(x).double()) <= 448 * torch.exp2(E.double())).all())


def test_gelu_tanh64_is_within_the_documented_contract_of_gelu64():
    v = torch.linspace(-12, 12, 200001, dtype=torch.float64)
    d = (X.gelu_tanh64(v) - X.gelu64(v)).abs().max()
    assert 4.0e-4 < float(d) < X.GELU_TANH_TOL
    lo, hi = X.act_interval(v, X.ACT_GELU_TANH)
    assert bool(((lo <= X.gelu_tanh64(v)) & (X.gelu_tanh64(v) <= hi)).all())


# ------------------------------------------------------------------ G1's exactness claim
@pytest.mark.parametrize("group", X.GROUPS)
def test_exact_generators_sum_exactly_in_fp32_in_any_order(group):
    """float32 accumulation of the scaled products in several random orders equals float64,
    and stays inside the stated bounds."""
    M, N, K = 6, 64, 640
    op = X.gen_exact(M, N, K, group, seed=5)
    A, W = X.operand_values(op["a"], op["Ea"]), X.operand_values(op["w"], op["Ew"])
    prod = A[:, None, :] * W[None, :, :]                       # [M, N, K] float64, exact
    ref = prod.sum(-1)
    assert torch.equal(prod.float().double(), prod)
    g = torch.Generator().manual_seed(0)
    for _ in range(5):
        perm = torch.randperm(K, generator=g)
        acc = torch.zeros(M, N, dtype=torch.float32)
        worst = torch.zeros(M, N, dtype=torch.float64)
        for k in perm.tolist():
            acc = acc + prod[..., k].float()
            worst = torch.maximum(worst, acc.double().abs())
        assert torch.equal(acc.double(), ref)
        if group == "block":
            assert float(worst.max()) < 2.0 ** 17 and torch.equal((prod * 16).round(), prod * 16)
        if group == "subnormal":
            assert float(worst.max()) < 2.0 ** 10 and torch.equal((prod * 2 ** 13).round(), prod * 2 ** 13)
    # 4-way split sums (an MFMA's lanes) and tile-wise sums agree too
    parts = prod.reshape(M, N, 4, K // 4).float().sum(-1).sum(-1)
    assert torch.equal(parts.double(), ref)
    # the elements are e4m3 codes and the bias is a multiple of 0.25 with a spike per 32 columns
    assert torch.equal(X.decode(X.encode(op["a"])), op["a"]) and torch.equal(X.decode(X.encode(op["w"])), op["w"])
    assert torch.equal((op["bias"] * 4).round(), op["bias"] * 4)
    assert bool((op["bias"].reshape(-1, 32) == 1024).any(-1).all())
    if group == "subnormal":
        nz = (op["a"] != 0) & (op["w"][:1] != 0)
        assert bool((X.encode(op["a"])[nz] & 0x78 == 0).all())   # only subnormal codes meet a partner


def test_zoo_is_representable_and_sequence_covers_every_slot():
    for kind in ("fp32", "fp16"):
        blocks, names = X.zoo(kind)
        Z = len(names)
        assert blocks.shape == (Z, 32) and Z > 150
        seq = X.zoo_sequence(Z)
        pairs = set(zip(seq.tolist(), (np.arange(8 * Z) % 8).tolist()))
        assert len(pairs) == 8 * Z
        amax = np.abs(blocks).max(-1)
        for k in (-20, 0, 7):
            b = 448.0 * 2.0 ** k
            assert (amax == b).any() and (amax < b).any() and (amax > b).any()
        if kind == "fp32":
            tiny = (amax > 0) & (amax < X.TINY)
            assert tiny.sum() == 6 and (np.abs(blocks[tiny][blocks[tiny] != 0]) >= 2.0 ** -126).all()


# ------------------------------------------------------------------ planted faults
def _mx_case(R=300, K=384, seed=3):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(R, K, generator=g).double() * torch.exp2(
        torch.randint(-6, 7, (R, K // 32), generator=g).double()).repeat_interleave(32, 1)
    y = y.float().double()
    q, E = X.quantize(y)
    buf = torch.full((R + 1, K), X.CANARY_BYTE, dtype=torch.uint8)
    buf[:R] = q
    return y, buf, E, X.write_plane(E, K, fill=X.CANARY_BYTE, tail=X.PLANE_TAIL)


def test_acceptance_passes_the_clean_case():
    y, q, E, S = _mx_case()
    assert X.bytes_exact(q, S, y).ok
    assert X.bytes_in_interval(q, S, y - 1e-4, y + 1e-4).ok
    assert X.rows_untouched(q, 300, X.CANARY_BYTE) and X.plane_tail_untouched(S, 300, 384)


def test_rejects_exponent_off_by_one():
    y, q, E, _ = _mx_case()
    for d in (1, -1):
        E2 = E.clone()
        E2[17, 5] += d
        S = X.write_plane(E2, 384)
        v = X.bytes_exact(q, S, y)
        assert not v.ok and v.n_bad_E == 1 and bool(v.bad_E[17, 5])
        v = X.bytes_in_interval(q, S, y - 1e-4, y + 1e-4)
        assert not v.ok and bool(v.bad_E[17, 5])
        # consistent bytes at the wrong exponent are still a wrong exponent
        q2 = q.clone()
        q2[17, 160:192] = X.encode(X.scaled(y, E2))[17, 160:192]
        assert not X.bytes_exact(q2, S, y).ok and not X.bytes_in_interval(q2, S, y - 1e-4, y + 1e-4).ok


def test_rejects_one_byte_off_by_one_code():
    y, q, E, S = _mx_case()
    big = (X.scaled(y, E).abs() > 1.0).nonzero()    # where one code is far more than 1e-4
    for r, c in big[:: len(big) // 7].tolist():
        for d in (1, -1):
            q2 = q.clone()
            q2[r, c] = int(q2[r, c]) + d
            v = X.bytes_exact(q2, S, y)
            assert not v.ok and v.n_bad_q == 1 and bool(v.bad_q[r, c])
            assert not X.bytes_in_interval(q2, S, y - 1e-4, y + 1e-4).ok


def test_rejects_a_row_written_past_M_and_a_scale_byte_past_the_plane():
    y, q, E, S = _mx_case()
    q2 = q.clone()
    q2[300, 77] = 0
    assert not X.rows_untouched(q2, 300, X.CANARY_BYTE)
    S2 = S.clone()
    S2[X.scale_bytes(300, 384) + 200] = 0
    assert not X.plane_tail_untouched(S2, 300, 384)
    assert not X.plane_tail_untouched(S[:-1], 300, 384)


def _gemm_case(group="block", M=5, N=256, K=384, seed=9):
    op = X.gen_exact(M, N, K, group, seed)
    A, W = X.operand_values(op["a"], op["Ea"]), X.operand_values(op["w"], op["Ew"])
    return op, A, W, A @ W.t() + op["bias"].double()


def _gemm_through_planes(op, SA, SW, M, N, K, drop=None):
    """What a correct kernel computes from bytes and PLANES (so a fault planted in a plane
    propagates), optionally dropping one k element of one output."""
    A = X.dequantize(X.encode(op["a"]), X.read_plane(SA, M, K))
    W = X.dequantize(X.encode(op["w"]), X.read_plane(SW, N, K))
    v = A @ W.t() + op["bias"].double()
    if drop is not None:
        m, n, k = drop
        v[m, n] -= A[m, k] * W[n, k]
    return v


def test_rejects_swapped_scale_bytes_and_a_dropped_k_element():
    M, N, K = 5, 256, 384
    op, A, W, v = _gemm_case(M=M, N=N, K=K)
    SA, SW = X.write_plane(op["Ea"], K), X.write_plane(op["Ew"], K)
    clean = _gemm_through_planes(op, SA, SW, M, N, K)
    assert torch.equal(clean, v)
    x0 = torch.randint(-64, 65, (M, N)).to(torch.float16)

    def accepts(vk):
        """The three exact acceptance forms of G1 on a kernel result vk."""
        q, E = X.quantize(vk.float().double())
        return (torch.equal(X.emu_store(vk, X.F16), X.emu_store(v, X.F16)),
                torch.equal(X.emu_resid16(x0, vk), X.emu_resid16(x0, v)),
                X.bytes_exact(q, X.write_plane(E, N), v.float().double()).ok)

    assert accepts(clean) == (True, True, True)
    # two k-blocks' scale bytes of one A row swapped (pick a row whose two exponents differ)
    r = next(r for r in range(M) if op["Ea"][r, 3] != op["Ea"][r, 7])
    SA2 = SA.clone()
    i, j = (int(X.scale_index(torch.tensor(r), torch.tensor(kb), K // 128)) for kb in (3, 7))
    SA2[i], SA2[j] = SA[j], SA[i]
    assert accepts(_gemm_through_planes(op, SA2, SW, M, N, K)) == (False, False, False)
    # one k element dropped from one output: the bit-for-bit forms see it wherever the output
    # format resolves the lost product p -- fp16: |p| >= the ulp at max(|v|, |v - p|); the MX
    # bytes: |p| >= the block's largest step 32 * 2^E (1/14 .. 1/7 of the block's amax)
    g = torch.Generator().manual_seed(1)
    _, Ev = X.quantize(v.float().double())
    seen16 = seen8 = tried = 0
    for n, k in zip(torch.randint(0, N, (60,), generator=g).tolist(),
                    torch.randint(0, K, (60,), generator=g).tolist()):
        p = abs(float(A[2, k] * W[n, k]))
        if p == 0:
            continue
        tried += 1
        ok16, okres, ok8 = accepts(_gemm_through_planes(op, SA, SW, M, N, K, drop=(2, n, k)))
        top = max(abs(float(v[2, n])), abs(float(v[2, n])) + p)
        if p >= 2.0 ** (math.floor(math.log2(top)) - 10):
            seen16 += 1
            assert not ok16, (n, k, p)
        if p >= 32 * 2.0 ** int(Ev[2, n // 32]):
            seen8 += 1
            assert not ok8, (n, k, p)
    assert tried >= 40 and seen16 >= tried * 3 // 4 and seen8 >= 1, (tried, seen16, seen8)
