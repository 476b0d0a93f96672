"""CPU: the fine-tuning entry points of the C ABI (include/miclip.h) are exported and
refuse bad arguments, naming them, before any device access (there is no GPU here: every
call below must return before a launch)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("miclip_gemm_tn_ws_bytes", "miclip_gemm_tn_plan", "miclip_op_gemm_tn", "miclip_ft_adam",
       "miclip_ft_proj_scratch_bytes", "miclip_ft_proj_grad", "miclip_encode_image_trunk",
       "miclip_ft_layout", "miclip_ft_scratch_bytes", "miclip_ft_grad")
FP16, BF16, MXFP8, F32 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j", "8"], check=True)
    return _lib.load_library()


def _p(v=4096):
    """A non-NULL, aligned pointer that is never dereferenced (validation comes first)."""
    return ctypes.c_void_p(v)


def _plan(lib, M, Nn, K):
    s, r = ctypes.c_int32(), ctypes.c_int32()
    assert lib.miclip_gemm_tn_plan(M, Nn, K, ctypes.byref(s), ctypes.byref(r)) == 0
    return s.value, r.value


def _tn(lib, *, dtype=FP16, M=64, Nn=128, K=64, null=None, A=4096):
    a = {n: (None if n == null else _p()) for n in ("A", "X", "G", "workspace")}
    if null != "A":
        a["A"] = _p(A)
    return lib.miclip_op_gemm_tn(dtype, a["A"], a["X"], a["G"], M, Nn, K, a["workspace"], None)


def _adam(lib, *, numel=8, lr=1e-3, step=1, eps=1e-8, null=None):
    a = {n: (None if n == null else _p()) for n in ("params", "grads", "m", "v")}
    return lib.miclip_ft_adam(a["params"], a["grads"], a["m"], a["v"], numel, lr, step, eps, None)


def _grad(lib, *, B=3, W=256, E=64, C=5, dtype=FP16, null=None, scratch=4096):
    names = ("y", "labels", "text_weights", "proj", "dP", "scratch", "stats")
    a = {n: (None if n == null else _p()) for n in names}
    if null != "scratch":
        a["scratch"] = _p(scratch)
    return lib.miclip_ft_proj_grad(a["y"], a["labels"], a["text_weights"], a["proj"], B, W, E, C,
                                   dtype, 100.0, a["dP"], a["scratch"], a["stats"], None)


def test_new_symbols_are_exported_and_abi_stays_9(lib):
    from miclip import _lib
    for s in NEW:
        assert s in _lib.EXPORTS
        assert hasattr(lib, s)
    assert lib.miclip_abi_version() == 10 == _lib.ABI_VERSION


def test_gemm_tn_plan_is_a_function_of_the_shape(lib):
    """Slices of whole 32-row stages; at most 32 of them; about 1024 workgroups."""
    assert _plan(lib, 1, 128, 64) == (1, 32)
    assert _plan(lib, 64, 128, 64) == (2, 32)
    assert _plan(lib, 65, 128, 64) == (3, 32)
    for M, Nn, K in ((1799, 768, 256), (65792, 3072, 1024), (256, 1024, 768), (33, 256, 16)):
        s, r = _plan(lib, M, Nn, K)
        assert 1 <= s <= 32 and r % 32 == 0
        assert (s - 1) * r < M <= s * r               # no empty slice, every row covered
        assert lib.miclip_gemm_tn_ws_bytes(M, Nn, K) == s * Nn * K * 4
    assert _plan(lib, 65792, 3072, 1024)[0] == 2


def test_workspace_and_scratch_bytes_are_zero_outside_the_limits(lib):
    for shape in ((0, 128, 64), (64, 8, 64), (64, 136, 64), (64, 128, 0), (64, 128, 24),
                  (64, 65552, 64)):
        assert lib.miclip_gemm_tn_ws_bytes(*shape) == 0, shape
    assert lib.miclip_ft_proj_scratch_bytes(3, 256, 64, 5) > 0
    assert lib.miclip_ft_proj_scratch_bytes(3, 256, 64, 5) % 256 == 0
    assert lib.miclip_ft_proj_scratch_bytes(300, 1280, 1024, 1024) > \
        lib.miclip_ft_proj_scratch_bytes(3, 1280, 1024, 1024)
    for shape in ((0, 256, 64, 5), (3, 200, 64, 5), (3, 64, 64, 5), (3, 1408, 64, 5),
                  (3, 256, 8, 5), (3, 256, 72, 5), (3, 256, 1040, 5), (3, 256, 64, 0),
                  (3, 256, 64, 1025)):
        assert lib.miclip_ft_proj_scratch_bytes(*shape) == 0, shape


def test_gemm_tn_limits_are_refused_with_the_argument_named(lib):
    for kw, word in (({"M": 0}, b"M:"), ({"M": -5}, b"M:"), ({"Nn": 8}, b"Nn:"),
                     ({"Nn": 136}, b"Nn:"), ({"Nn": 65552}, b"Nn:"), ({"K": 0}, b"K:"),
                     ({"K": 24}, b"K:"), ({"dtype": MXFP8}, b"dtype:"), ({"dtype": F32}, b"dtype:"),
                     ({"A": 4104}, b"aligned")):
        assert _tn(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())
    for name in ("A", "X", "G", "workspace"):
        assert _tn(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()
    s, r = ctypes.c_int32(), ctypes.c_int32()
    assert lib.miclip_gemm_tn_plan(0, 128, 64, ctypes.byref(s), ctypes.byref(r)) == -1
    assert b"M:" in lib.miclip_last_error()


def test_adam_limits_are_refused_with_the_argument_named(lib):
    nan = float("nan")
    for kw, word in (({"numel": 0}, b"numel:"), ({"numel": -1}, b"numel:"), ({"step": 0}, b"step:"),
                     ({"lr": -1e-3}, b"lr:"), ({"lr": nan}, b"lr:"), ({"eps": -1.0}, b"eps:"),
                     ({"eps": nan}, b"eps:")):
        assert _adam(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())
    for name in ("params", "grads", "m", "v"):
        assert _adam(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()


def test_proj_grad_limits_are_refused_with_the_argument_named(lib):
    for kw, word in (({"B": 0}, b"B:"), ({"W": 200}, b"W:"), ({"W": 64}, b"W:"),
                     ({"W": 1408}, b"W:"), ({"E": 8}, b"E:"), ({"E": 72}, b"E:"),
                     ({"E": 1040}, b"E:"), ({"C": 0}, b"C:"), ({"C": 1025}, b"C:"),
                     ({"dtype": MXFP8}, b"compute_dtype:"), ({"dtype": F32}, b"compute_dtype:"),
                     ({"scratch": 4096 + 64}, b"alignment")):
        assert _grad(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())
    for name in ("y", "labels", "text_weights", "proj", "dP", "scratch", "stats"):
        assert _grad(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()


def _ft(lib, *, B=3, N=7, W=256, E=64, C=5, dh=64, act=1, dtype=FP16, x_dtype=FP16, groups=2,
        null=None, scratch=4096):
    names = ("x", "labels", "text_weights", "params", "grads", "scratch", "stats")
    a = {n: (None if n == null else _p()) for n in names}
    if null != "scratch":
        a["scratch"] = _p(scratch)
    return lib.miclip_ft_grad(a["x"], x_dtype, a["labels"], a["text_weights"], a["params"], B, N,
                              W, E, C, dh, act, dtype, 100.0, groups, a["grads"], a["scratch"],
                              a["stats"], None, None)


def test_layout_offsets(lib):
    """The block's 12 tensors, ln_post's 2, proj last; offsets[15] is the total."""
    off = (ctypes.c_int64 * 16)()
    assert lib.miclip_ft_layout(256, 64, off) == 0
    W, E = 256, 64
    sizes = [W, W, 3 * W * W, 3 * W, W * W, W, W, W, 4 * W * W, 4 * W, 4 * W * W, W, W, W, W * E]
    want = [sum(sizes[:i]) for i in range(16)]
    assert list(off) == want and off[15] == 12 * W * W + 15 * W + W * E
    assert lib.miclip_ft_layout(1280, 1024, off) == 0 and off[14] == 12 * 1280 ** 2 + 15 * 1280
    for kw, word in (((200, 64), b"W:"), ((256, 24), b"E:"), ((1408, 64), b"W:"),
                     ((256, 2048), b"E:")):
        assert lib.miclip_ft_layout(*kw, off) == -1
        assert word in lib.miclip_last_error()
    assert lib.miclip_ft_layout(256, 64, None) == -1
    assert lib.miclip_last_error() == b"null argument: offsets"


def test_ft_scratch_bytes_are_zero_outside_the_limits(lib):
    ok = lib.miclip_ft_scratch_bytes(3, 7, 256, 64, 5, 64)
    assert ok > 0 and ok % 256 == 0
    assert lib.miclip_ft_scratch_bytes(2, 5, 640, 128, 20, 80) > 0
    assert lib.miclip_ft_scratch_bytes(6, 7, 256, 64, 5, 64) > ok
    for shape in ((0, 7, 256, 64, 5, 64), (3, 0, 256, 64, 5, 64), (3, 769, 256, 64, 5, 64),
                  (3, 7, 200, 64, 5, 64), (3, 7, 256, 64, 5, 80), (3, 7, 256, 64, 5, 32),
                  (3, 7, 256, 8, 5, 64), (3, 7, 256, 1040, 5, 64), (3, 7, 256, 64, 0, 64),
                  (3, 7, 256, 64, 1025, 64)):
        assert lib.miclip_ft_scratch_bytes(*shape) == 0, shape


def test_ft_grad_limits_are_refused_with_the_argument_named(lib):
    for kw, word in (({"B": 0}, b"B:"), ({"N": 0}, b"N:"), ({"N": 769}, b"N:"),
                     ({"W": 200}, b"W:"), ({"W": 1408}, b"W:"), ({"dh": 32}, b"head_dim:"),
                     ({"dh": 80}, b"W:"), ({"E": 8}, b"E:"), ({"E": 1040}, b"E:"),
                     ({"C": 0}, b"C:"), ({"C": 1025}, b"C:"), ({"groups": 0}, b"groups:"),
                     ({"groups": 3}, b"groups:"), ({"dtype": MXFP8}, b"compute_dtype:"),
                     ({"dtype": F32}, b"compute_dtype:"), ({"x_dtype": BF16}, b"x_dtype:"),
                     ({"act": 3}, b"act:"), ({"act": 0}, b"act:"),
                     ({"scratch": 4096 + 64}, b"scratch:")):
        assert _ft(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())
    for name in ("x", "labels", "text_weights", "params", "grads", "scratch", "stats"):
        assert _ft(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()


def test_trunk_refuses_bad_arguments_by_name(lib):
    for args, word in (((None, _p(), FP16, 1, _p(), None), b"null argument: model"),):
        assert lib.miclip_encode_image_trunk(*args) == -1
        assert lib.miclip_last_error() == word
