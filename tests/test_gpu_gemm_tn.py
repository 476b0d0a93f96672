"""GPU: miclip_op_gemm_tn, G[Nn, K] = sum_m A[m, Nn] X[m, K] (csrc/finetune.hip), fp16 and bf16.

Compared with the float64 product of the rounded operands. Bar: 4 * max(e_ref, 8 * 2^-23 *
max|G|) with e_ref = max|fp32 CPU matmul - fp64|, the convention and factor of
tests/test_gpu_prolip.py. Shapes (M, Nn, K): one row; a row tail inside one 32-row
stage; exactly two stages / slices; one slice + 1 row; two slices - 1 row; column tails of
the 64 x 64 output tile (Nn = 80, K = 16 and 48); 7 images x 257 tokens; a shape whose
slices hold several stages. Two runs are bit-identical, and the workspace past the plan's
bytes and the output's neighbours are left alone.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
SHAPES = [(1, 128, 64), (21, 256, 256), (64, 128, 64), (65, 128, 64), (33, 128, 64),
          (63, 128, 64), (40, 80, 48), (5, 256, 16), (1799, 768, 256), (2049, 256, 256)]
DTYPES = {"fp16": (0, torch.float16), "bf16": (1, torch.bfloat16)}


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    assert torch.cuda.is_available()
    return _lib.load_library()


_REF = {}


def _case(shape, name):
    """Rounded operands and the fp64 / fp32 references, computed once per case."""
    key = (shape, name)
    if key not in _REF:
        M, Nn, K = shape
        g = torch.Generator().manual_seed(1000 + M + Nn + K)
        a = torch.randn(M, Nn, generator=g).to(DTYPES[name][1])
        x = torch.randn(M, K, generator=g).to(DTYPES[name][1])
        g64 = a.double().t() @ x.double()
        e_ref = float((a.float().t() @ x.float() - g64).abs().max())
        _REF[key] = (a, x, g64, e_ref)
    return _REF[key]


def _run(lib, a, x, name):
    from miclip import _lib
    M, Nn = a.shape
    K = x.shape[1]
    ws_bytes = lib.miclip_gemm_tn_ws_bytes(M, Nn, K)
    assert ws_bytes > 0
    pad = 64
    ws = torch.full((ws_bytes // 4 + pad,), float("nan"), device="cuda")
    out = torch.full((Nn * K + 2 * pad,), -7.0, device="cuda")
    ad, xd = a.cuda().contiguous(), x.cuda().contiguous()
    G = out[pad:pad + Nn * K]
    _lib.check(lib.miclip_op_gemm_tn(DTYPES[name][0], ctypes.c_void_p(ad.data_ptr()),
                                     ctypes.c_void_p(xd.data_ptr()),
                                     ctypes.c_void_p(G.data_ptr()), M, Nn, K,
                                     ctypes.c_void_p(ws.data_ptr()),
                                     _lib.stream_handle(torch.device("cuda"))), "miclip_op_gemm_tn")
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[:pad] == -7.0).all()) and bool((o[pad + Nn * K:] == -7.0).all())
    assert bool(torch.isnan(ws[ws_bytes // 4:]).all())
    return o[pad:pad + Nn * K].reshape(Nn, K).clone()


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_tn_against_float64(lib, shape, name):
    a, x, g64, e_ref = _case(shape, name)
    got = _run(lib, a, x, name)
    err = float((got.double() - g64).abs().max())
    bar = 4.0 * max(e_ref, 8.0 * EPS32 * float(g64.abs().max()))
    print(f"gemm_tn {shape} {name}: err {err:.3e} e_ref {e_ref:.3e} bar {bar:.3e}")
    assert np.isfinite(err) and err <= bar
    again = _run(lib, a, x, name)
    assert torch.equal(got, again)
