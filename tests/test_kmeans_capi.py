"""CPU: the device k-means entry points of the C ABI (include/miclip.h) are exported
and refuse bad arguments, naming them, before any device access (there is no GPU
here: every call below must return before a launch)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("miclip_kmeans_scratch_bytes", "miclip_kmeans_seed", "miclip_kmeans_lloyd")


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j", "8"], check=True)
    return _lib.load_library()


def _p(v=64):
    """A non-NULL pointer that is never dereferenced (validation comes first)."""
    return ctypes.c_void_p(v)


def _seed(lib, *, D=16, Pn=1, k_max=4, null=None):
    names = ["x", "order", "offsets", "prob_class", "prob_k", "prob_off", "u", "scratch", "picks",
             "centres"]
    a = {n: (None if n == null else _p()) for n in names}
    return lib.miclip_kmeans_seed(a["x"], a["order"], a["offsets"], D, a["prob_class"],
                                  a["prob_k"], a["prob_off"], Pn, k_max, a["u"], a["scratch"],
                                  a["picks"], a["centres"], None)


def _lloyd(lib, *, D=16, Pn=1, k_max=4, max_iter=10, null=None):
    names = ["x", "order", "offsets", "prob_class", "prob_k", "prob_off", "tol", "scratch",
             "centres", "labels", "inertia", "n_iter", "strict", "counts"]
    a = {n: (None if n == null else _p()) for n in names}
    return lib.miclip_kmeans_lloyd(a["x"], a["order"], a["offsets"], D, a["prob_class"],
                                   a["prob_k"], a["prob_off"], Pn, k_max, a["tol"], max_iter,
                                   a["scratch"], a["centres"], a["labels"], a["inertia"],
                                   a["n_iter"], a["strict"], a["counts"], None)


def test_new_symbols_are_exported_and_abi_stays_9(lib):
    from miclip import _lib
    for s in NEW:
        assert s in _lib.EXPORTS
        assert hasattr(lib, s)
    assert lib.miclip_abi_version() == 10
    assert lib.miclip_kmeans_scratch_bytes(1000) == 4000
    assert lib.miclip_kmeans_scratch_bytes(0) == 0
    assert lib.miclip_kmeans_scratch_bytes(1 << 31) == 4 << 31


@pytest.mark.parametrize("call", [_seed, _lloyd])
def test_limits_are_refused_with_the_argument_named(lib, call):
    for kw, word in (({"k_max": 1}, b"k_max"), ({"k_max": 17}, b"k_max"), ({"D": 1025}, b"D must"),
                     ({"D": 0}, b"D must"), ({"Pn": 0}, b"Pn"), ({"Pn": 65536}, b"Pn")):
        assert call(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())


def test_max_iter_zero_is_refused(lib):
    assert _lloyd(lib, max_iter=0) == -1
    assert b"max_iter" in lib.miclip_last_error()


def test_null_pointers_are_refused_by_name(lib):
    for name in ("x", "order", "offsets", "prob_class", "prob_k", "prob_off", "u", "scratch",
                 "picks", "centres"):
        assert _seed(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()
    for name in ("x", "order", "offsets", "prob_class", "prob_k", "prob_off", "tol", "scratch",
                 "centres", "labels", "inertia", "n_iter", "counts"):
        assert _lloyd(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()
    # `strict` is optional: a NULL there passes the pointer check (a limit is hit next)
    assert _lloyd(lib, null="strict", k_max=17) == -1
    assert b"k_max" in lib.miclip_last_error()
