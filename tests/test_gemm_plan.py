"""CPU: the GEMM launcher's plan (csrc/gemm_plan.h plan_gemm, seen through miclip_gemm_plan)
against the Python restatement of the launcher it replaced (tests/_gemm_ref.py
launch_choice / launch_report). Every kernel is bit-identical by design, so a launcher that
picks the wrong kernel passes every exact test and only loses speed: this is the test that
sees the choice itself. No GPU: the CU count is an argument."""
import collections
import ctypes
import itertools
import os
import subprocess

import pytest

import _gemm_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

MS = (1, 16, 17, 127, 128, 129, 255, 256, 257, 300, 513, 1028, 2056, 4112, 8224, 12850, 16384,
      16421, 16641, 32896, 65792)
NS = (128, 256, 384, 768, 1024, 1280, 3072, 4096, 5120)
KS = (64, 128, 1024)
NCUS = (256, 304, 64, 1)
# miclip_gemm_plan's epi -> (tracc, patch) of the restatement
EPIS = {"store": (0, True, False), "f32": (2, False, False), "patch": (6, False, True)}
ALL_EPIS = {0: (True, False), 1: (False, False), 2: (False, False), 3: (False, False),
            4: (True, False), 5: (True, False), 6: (False, True)}
NT, TF, ST, RS = G.NO_TAIL, G.TAIL_FIRST, G.STAGGER, G.ROW_STAGING
# every explicit code and flag combination the GPU tests use, each flag on the by-size code,
# a thousands-digit group and an unknown code
VARIANTS = (3, 128, 129, 130, 192, 256, 257, 258, 259, 260, 258 | TF, 259 | RS, 259 | NT,
            2259, 8258 | TF, 0 | NT, 0 | TF, 0 | ST, 0 | RS, 258 | NT, 258 | ST, 260 | TF, 3 | NT,
            192 | RS, 130 | NT, 7, 1000)


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j", "8"], check=True)
    return _lib.load_library()


def _plan(lib, M, N, K, epi, variant, ncu, sk=1):
    out = (ctypes.c_int32 * 8)(*([-9] * 8))
    rc = lib.miclip_gemm_plan(M, N, K, epi, variant, sk, ncu, out)
    if rc != 0:
        assert rc == EINVAL and list(out) == [-9] * 8
        return None
    assert out[7] == 0
    return tuple(out[:7])


def test_plan_equals_the_restated_launcher_by_size(lib):
    """Variant 0 over the whole product; every outcome and tail kind must occur."""
    seen = collections.Counter()
    bad = []
    for M, N, K, ncu, (name, (epi, tracc, patch)) in itertools.product(MS, NS, KS, NCUS,
                                                                       EPIS.items()):
        want = G.launch_report(M, N, K, ncu, tracc, patch)
        got = _plan(lib, M, N, K, epi, 0, ncu)
        if got != want:
            bad.append((M, N, K, ncu, name, got, want))
        kernel, plan = G.launch_choice(M, N, K, ncu, tracc, patch)
        seen[kernel] += 1
        if plan is not None and plan[1] > 0:
            seen[kernel, "wide" if plan[2] else "narrow"] += 1
    print(dict(seen))
    assert not bad, f"{len(bad)} differ, first {bad[:5]}"
    for key in ("tile128", "tile256", "persistent", "rows128", "rows192", ("tile256", "narrow"),
                ("tile256", "wide"), ("persistent", "narrow"), ("persistent", "wide")):
        assert seen[key] > 0, f"the sweep no longer reaches {key}"


def test_plan_equals_the_restated_launcher_for_explicit_variants(lib):
    """Every explicit code and flag at 256 CUs, every epilogue code; refusals both ways."""
    seen = collections.Counter()
    bad = []
    for M, N, K, variant, (epi, (tracc, patch)) in itertools.product(MS, NS, KS, VARIANTS,
                                                                    ALL_EPIS.items()):
        if epi in (1, 3, 5) and M not in (257, 8224, 16421):
            continue          # same classes as 2 / 0: a thinner pass
        want = G.launch_report(M, N, K, 256, tracc, patch, variant)
        got = _plan(lib, M, N, K, epi, variant, 256)
        if got != want:
            bad.append((M, N, K, hex(variant), epi, got, want))
        seen["refused" if want is None else G.KERNELS[want[0]]] += 1
        if want is not None and variant & TF and want[6] & 2:
            seen["tail_first"] += 1
        if want is not None and variant & ST and want[6] >> 8:
            seen["stagger"] += 1
    print(dict(seen))
    assert not bad, f"{len(bad)} differ, first {bad[:5]}"
    for key in G.KERNELS[1:] + ("refused", "tail_first", "stagger"):
        assert seen[key] > 0, f"the sweep no longer reaches {key}"


def test_plan_split_k_and_refused_arguments(lib):
    # split-K is decided before the variant: an unknown code is not looked at
    for M, N, K, sk, variant in ((1, 1024, 4096, 4, 0), (257, 768, 3072, 8, 7), (16, 128, 128, 2, 259),
                                 (16, 1024, 4096, 3, 0), (16, 1024, 64, 2, 0)):
        for epi in (0, 1, 4, 5):
            want = G.launch_report(M, N, K, 256, variant=variant, sk=sk)
            assert _plan(lib, M, N, K, epi, variant, 256, sk) == want, (M, N, K, sk)
    assert G.launch_report(1, 1024, 4096, 256, sk=4) == (0, 8, 256, 0, 0, 0, 0)
    assert G.launch_report(16, 1024, 4096, 256, sk=3) is None        # K % (64 sk)
    # shapes, epilogue codes and CU counts the entry point refuses, with a message
    for args in ((16, 100, 64, 0, 0, 1, 256), (16, 128, 96, 0, 0, 1, 256), (0, 128, 64, 0, 0, 1, 256),
                 (16, 256, 128, 7, 0, 1, 256), (16, 256, 128, -1, 0, 1, 256),
                 (16, 256, 128, 0, 0, 1, -1), (16, 256, 128, 0, 7, 1, 256)):
        assert _plan(lib, *args[:5], args[6], args[5]) is None, args
        assert lib.miclip_last_error()
    assert lib.miclip_gemm_plan(16, 256, 128, 0, 0, 1, 256, None) == EINVAL
    assert b"out" in lib.miclip_last_error()


def test_restated_explicit_variants_by_hand():
    """launch_choice / launch_report at explicit variants, worked out from the launcher."""
    L, R = G.launch_choice, G.launch_report
    assert L(257, 512, 64, 256, variant=259) == ("tile256", (2, 0, 0))      # one K-tile: SCHED 2
    assert L(257, 512, 128, 256, variant=259) == ("persistent", (2, 0, 0))
    assert L(257, 512, 128, 256, variant=259 | RS) == ("persistent_staged", (2, 0, 0))
    assert L(257, 512, 128, 256, tracc=False, variant=259 | RS) == ("persistent", (2, 0, 0))
    assert L(257, 512, 128, 256, patch=True, tracc=False, variant=3) == ("tile128", None)
    assert L(32896, 1024, 128, 256, patch=True, tracc=False, variant=3)[0] == "tile256"
    assert L(257, 512, 128, 256, variant=3) == ("persistent_p", None)
    assert L(257, 384, 128, 256, variant=258) == ("tile128", None)          # N % 256 != 0
    assert L(16421, 1024, 128, 256, variant=258 | TF) == ("tile256", (64, 48, 2))
    assert L(16421, 1024, 128, 256, variant=258 | NT) == ("tile256", (65, 0, 0))
    assert L(16421, 1024, 128, 256, variant=258 | ST) == ("tile256", (64, 48, 0))    # 256 tiles < 2 rounds
    assert L(32896, 4096, 128, 256, variant=258 | ST) == ("tile256", (128, 128, 1 | 8 << 8))
    assert L(16421, 1024, 128, 256, variant=259 | TF) == ("persistent", (64, 48, 0))  # one branch only
    assert L(8224, 1024, 1024, 256, variant=RS) == ("persistent_staged", (33, 0, 0))   # no 192-row tiles
    assert L(4112, 1024, 1024, 256, variant=RS) == ("tile128", None)
    assert L(8224, 1024, 128, 256, variant=130) == ("rows128", (64, 32, 0))
    assert L(8224, 1024, 128, 256, variant=130 | NT) == ("rows128", (64, 32, 0))
    assert L(383, 512, 128, 256, variant=192) == ("rows192", (2, 0, 0))
    assert L(383, 512, 128, 256, variant=192 | RS) is None
    assert L(383, 512, 128, 256, tracc=False, variant=129) is None
    assert L(383, 512, 64, 256, variant=129) is None
    assert L(383, 512, 128, 256, variant=7) is None
    assert R(16421, 1024, 128, 256, variant=2259) == (7, 256, 512, 2, 64, 48, 0)
    assert R(16421, 1024, 128, 256, variant=258 | TF) == (4, 304, 512, 4, 64, 48, 2)
    assert R(16421, 1024, 64, 256) == (4, 304, 512, 4, 64, 48, 0)
    assert R(383, 512, 128, 256, variant=192) == (9, 4, 512, 4, 2, 0, 0)
    assert R(77, 512, 512, 256) == (1, 4, 256, 0, 0, 0, 0)
    assert R(300, 512, 128, 256, variant=3) == (6, 4, 512, 4, 0, 0, 0)
