"""CPU: the exact t-SNE entry points of the C ABI (include/miclip.h) are exported and
refuse bad arguments, naming them, before any device access (there is no GPU here: every
call below must return before a launch)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("miclip_tsne_scratch_bytes", "miclip_tsne_affinities", "miclip_tsne_run")


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j", "8"], check=True)
    return _lib.load_library()


def _p(v=64):
    """A non-NULL pointer that is never dereferenced (validation comes first)."""
    return ctypes.c_void_p(v)


def _aff(lib, *, N=100, D=16, metric=0, perplexity=30.0, null=None):
    a = {n: (None if n == null else _p()) for n in ("x", "P", "beta", "dist", "scratch")}
    return lib.miclip_tsne_affinities(a["x"], N, D, metric, perplexity, a["P"], a["beta"],
                                      a["dist"], a["scratch"], None)


def _run(lib, *, N=100, n_steps=1, exaggeration=12.0, momentum=0.5, learning_rate=200.0,
         min_gain=0.01, error_every=0, null=None):
    a = {n: (None if n == null else _p())
         for n in ("P", "y", "update", "gains", "scratch", "stats")}
    return lib.miclip_tsne_run(a["P"], N, a["y"], a["update"], a["gains"], n_steps, exaggeration,
                               momentum, learning_rate, min_gain, error_every, a["scratch"],
                               a["stats"], None)


def test_new_symbols_are_exported_and_abi_stays_9(lib):
    from miclip import _lib
    for s in NEW:
        assert s in _lib.EXPORTS
        assert hasattr(lib, s)
    assert lib.miclip_abi_version() == 10


def test_scratch_bytes(lib):
    """64 bytes per row: the forces kernel's 8 floats per row, and the affinities' fp64 row
    sums and fp32 norms; 0 outside the limits on N."""
    assert lib.miclip_tsne_scratch_bytes(4) == 256
    assert lib.miclip_tsne_scratch_bytes(1398) == 1398 * 64
    assert lib.miclip_tsne_scratch_bytes(16384) == 1 << 20
    for n in (3, 0, -1, 16385):
        assert lib.miclip_tsne_scratch_bytes(n) == 0


def test_affinities_limits_are_refused_with_the_argument_named(lib):
    inf, nan = float("inf"), float("nan")
    for kw, word in (({"N": 3}, b"N must"), ({"N": 16385}, b"N must"), ({"D": 0}, b"D must"),
                     ({"D": 4097}, b"D must"), ({"metric": 3}, b"metric"),
                     ({"metric": -1}, b"metric"), ({"perplexity": 0.5}, b"perplexity"),
                     ({"perplexity": 100.0}, b"perplexity"), ({"perplexity": nan}, b"perplexity"),
                     ({"perplexity": inf}, b"perplexity")):
        assert _aff(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())


def test_run_limits_are_refused_with_the_argument_named(lib):
    inf, nan = float("inf"), float("nan")
    for kw, word in (({"N": 3}, b"N must"), ({"N": 16385}, b"N must"), ({"n_steps": 0}, b"n_steps"),
                     ({"error_every": -1}, b"error_every"),
                     ({"learning_rate": 0.0}, b"learning_rate"),
                     ({"learning_rate": -1.0}, b"learning_rate"),
                     ({"learning_rate": inf}, b"learning_rate"),
                     ({"learning_rate": nan}, b"learning_rate"),
                     ({"min_gain": 0.0}, b"min_gain"), ({"min_gain": nan}, b"min_gain"),
                     ({"min_gain": inf}, b"min_gain"), ({"momentum": 1.0}, b"momentum"),
                     ({"momentum": -0.1}, b"momentum"), ({"momentum": nan}, b"momentum"),
                     ({"exaggeration": 0.0}, b"exaggeration"),
                     ({"exaggeration": inf}, b"exaggeration")):
        assert _run(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())


def test_null_pointers_are_refused_by_name(lib):
    for name in ("x", "P", "beta", "scratch"):
        assert _aff(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()
    for name in ("P", "y", "update", "gains", "scratch", "stats"):
        assert _run(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()
    # `dist` is optional: a NULL there passes the pointer check (a limit is hit next)
    assert _aff(lib, null="dist", N=3) == -1
    assert b"N must" in lib.miclip_last_error()


def test_precomputed_ignores_d(lib):
    """With metric 2 x is the [N, N] matrix and D is not looked at: the next limit answers."""
    assert _aff(lib, metric=2, D=0, perplexity=0.5) == -1
    assert b"perplexity" in lib.miclip_last_error()
