"""CPU: the Tip-Adapter restatement tests/_tip_ref.py against the recorded reference run
(tests/golden/tip.npz, scripts/make_golden_tip.py) and, where a checkout of the
reference is present, against the reference run live; the host side of miclip/tip.py
(lists, scan, refusals) and the binding of the five C entry points."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _tip_ref as R

REF = os.environ.get("MICLIP_REFERENCE", "/root/reference")
REF_UTILS = os.path.join(REF, "methods", "utils.py")


def _case(golden, tag):
    g = golden("tip")
    m = g["meta"][tag]
    betas, alphas = R.lists(m["scale"], m["step"])
    return g, m, betas, alphas


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_golden(golden, tag):
    g, m, betas, alphas = _case(golden, tag)
    r = R.grid(g[f"{tag}_F"], g[f"{tag}_keys"], g[f"{tag}_key_labels"], g[f"{tag}_W"],
               g[f"{tag}_labels"], betas, alphas)
    n = len(g[f"{tag}_labels"])
    assert r["undecided"].sum() == 0
    np.testing.assert_array_equal(100.0 * r["counts"] / n, g[f"{tag}_acc"])
    np.testing.assert_array_equal(r["counts32"], r["counts"])
    bb, ba, best = R.scan(r["counts"], betas, alphas)
    assert (bb, ba) == tuple(g[f"{tag}_best"])
    assert 100.0 * best / n == g[f"{tag}_acc"].max()


@pytest.mark.skipif(not os.path.isfile(REF_UTILS), reason="no checkout of the reference here")
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_equals_reference_live(golden, tag, capsys):
    spec = importlib.util.spec_from_file_location("reference_methods_utils", REF_UTILS)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g, m, betas, alphas = _case(golden, tag)
    F, K, W = (torch.tensor(g[f"{tag}_{k}"]) for k in ("F", "keys", "W"))
    klab, lab = torch.tensor(g[f"{tag}_key_labels"]), torch.tensor(g[f"{tag}_labels"])
    values = torch.nn.functional.one_hot(klab, m["C"]).float()
    cfg = {"search_hp": True, "search_scale": m["scale"], "search_step": m["step"]}
    seen = []                       # the logits the reference hands to its cls_acc, per pair
    inner = ref.cls_acc

    def recording(output, target, topk=1):
        seen.append(output.clone())
        return inner(output, target, topk)

    ref.cls_acc = recording
    best = ref.search_hp_tip(cfg, K.t().contiguous(), values, F, lab, W)
    r = R.grid(F, K, klab, W, lab, betas, alphas)
    assert tuple(best) == R.scan(r["counts"], betas, alphas)[:2]
    # every pair's logits: the restatement in fp32 equals the reference's own fp32 bit for bit
    assert len(seen) == len(betas) * len(alphas)
    Z32, a32 = R.clip_logits(F, W, torch.float32), R.affinity(F, K, torch.float32)
    for ib, beta in enumerate(betas):
        for ia, alpha in enumerate(alphas):
            got = R.logits(Z32, a32, klab, beta, alpha, torch.float32)
            assert torch.equal(got, seen[ib * len(alphas) + ia]), (ib, ia)
            assert inner(got, lab) == 100.0 * r["counts"][ib, ia] / len(lab)


@pytest.mark.parametrize("scale,step", [([7, 3], [200, 20]), ([1, 1], [1, 1]), ([5.5, 2], [5, 7]),
                                        ([0.1, 12.25], [3, 4]), ([50, 50], [13, 1])])
def test_lists_are_the_reference_expressions(scale, step):
    from miclip import tip
    betas, alphas = tip.beta_alpha_lists({"search_scale": scale, "search_step": step})
    for got, top, n in ((betas, scale[0], step[0]), (alphas, scale[1], step[1])):
        assert len(got) == n and got[0] == 0.1
        assert got == [0.1 + k * (top - 0.1) / n for k in range(n)]   # n points from 0.1, top excluded
    assert (betas, alphas) == R.lists(scale, step)


def test_host_scan(capsys):
    from miclip import tip
    betas, alphas = [0.1, 1.0, 2.0], [0.5, 1.5]
    # strict >: the later equal count does not replace the first maximum (beta-major)
    assert tip.scan_count_grid([[1, 3], [3, 2], [3, 3]], betas, alphas, 4)[:2] == (0.1, 1.5)
    out = capsys.readouterr().out
    assert out.count("New best setting") == 2
    assert "New best setting, beta: 0.10, alpha: 1.50; accuracy: 75.00" in out
    assert "\nAfter searching, the best accuarcy: 75.00.\n" in out
    # alpha runs inside beta
    assert tip.scan_count_grid([[0, 2], [5, 1], [4, 5]], betas, alphas, 5) == (1.0, 0.5, 100.0)
    # an all-zero grid keeps the reference's initial (0, 0) and accuracy 0
    assert tip.scan_count_grid([[0, 0]] * 3, betas, alphas, 7, verbose=False) == (0, 0, 0)
    for counts in ([[1, 3], [3, 2], [3, 3]], [[0, 0]] * 3, [[2, 2], [2, 9], [9, 9]]):
        assert tip.scan_count_grid(counts, betas, alphas, 9, verbose=False)[:2] == \
            R.scan(counts, betas, alphas)[:2]


def _inputs(Nq=6, Nk=4, E=16, C=3):
    g = torch.Generator().manual_seed(0)
    keys = torch.randn(E, Nk, generator=g)
    values = torch.nn.functional.one_hot(torch.arange(Nk) % C, C).half()
    feats = torch.randn(Nq, E, generator=g)
    labels = torch.arange(Nq) % C
    W = torch.randn(E, C, generator=g)
    return keys, values, feats, labels, W


CFG = {"search_hp": True, "search_scale": [7, 3], "search_step": [3, 2]}


def test_value_errors():
    from miclip import tip
    keys, values, feats, labels, W = _inputs()
    with pytest.raises(ValueError, match="search_hp"):
        tip.search_hp_tip(dict(CFG, search_hp=False), keys, values, feats, labels, W)
    bad = values.clone()
    bad[1, 0] = 0.5
    two = values.clone()
    two[2] = 1
    for v in (bad, two, torch.zeros_like(values)):
        with pytest.raises(ValueError, match="one-hot"):
            tip.search_hp_tip(CFG, keys, v, feats, labels, W)
    with pytest.raises(ValueError, match="width"):
        tip.search_hp_tip(CFG, keys, values, feats[:, :8], labels, W)
    with pytest.raises(ValueError, match="clip_weights"):
        tip.search_hp_tip(CFG, keys, values, feats, labels, W[:8])
    with pytest.raises(ValueError, match="width"):     # more value columns than classes
        tip.search_hp_tip(CFG, keys, values, feats, labels, W[:, :2])
    with pytest.raises(ValueError, match="rows"):
        tip.search_hp_tip(CFG, keys, values[:3], feats, labels, W)
    for lab in (labels + 1, labels - 1):
        with pytest.raises(ValueError, match=r"labels must lie in \[0, 3\)"):
            tip.search_hp_tip(CFG, keys, values, feats, lab, W)
    with pytest.raises(ValueError, match="labels"):
        tip.search_hp_tip(CFG, keys, values, feats, labels[:-1], W)
    with pytest.raises(ValueError, match="one-hot"):
        tip.tip_logits(keys, bad, feats, W, 1.0, 1.0)
    # the cache builder: widths, label range
    views = [torch.randn(4, 32), torch.randn(4, 32)]
    proj = torch.randn(32, 16)
    with pytest.raises(ValueError, match="width"):
        tip.cache_model_from_views([v[:, :16] for v in views], labels[:4], proj, 3)
    with pytest.raises(ValueError, match="differs"):
        tip.cache_model_from_views([views[0], views[1].half()], labels[:4], proj, 3)
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 2\)"):
        tip.cache_model_from_views(views, labels[:4], proj, 2)
    with pytest.raises(ValueError, match="no feature views"):
        tip.cache_model_from_views([], labels[:4], proj, 3)


def test_exports_and_symbols():
    import miclip
    from miclip import _lib
    for name in ("build_cache_model", "cache_model_from_views", "search_hp_tip",
                 "tip_accuracy_grid", "tip_logits", "beta_alpha_lists"):
        assert callable(getattr(miclip, name)) and name in miclip.__all__
    names = ("miclip_tip_scratch_bytes", "miclip_tip_keys", "miclip_tip_affinity",
             "miclip_tip_grid", "miclip_tip_logits")
    assert set(names) <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 10
    lib = _lib.load_library()
    for name in names:
        assert getattr(lib, name).argtypes is not None
    assert lib.miclip_abi_version() == 10
    # the scratch query is host-only: positive inside the limits, 0 outside
    assert lib.miclip_tip_scratch_bytes(1, 1, 16, 1, 1, 1) > 0
    assert lib.miclip_tip_scratch_bytes(1 << 24, 65536, 1024, 1024, 1024, 64) > 0
    for bad in ((0, 1, 16, 1, 1, 1), ((1 << 24) + 1, 1, 16, 1, 1, 1), (1, 0, 16, 1, 1, 1),
                (1, 65537, 16, 1, 1, 1), (1, 1, 8, 1, 1, 1), (1, 1, 24, 1, 1, 1),
                (1, 1, 1040, 1, 1, 1), (1, 1, 16, 0, 1, 1), (1, 1, 16, 1025, 1, 1),
                (1, 1, 16, 1, 0, 1), (1, 1, 16, 1, 1025, 1), (1, 1, 16, 1, 1, 0),
                (1, 1, 16, 1, 1, 1025), (1, 1, 16, 1, 1024, 65),
                (-1, 1, 16, 1, 1, 1), (1, -1, 16, 1, 1, 1), (1, 1, -16, 1, 1, 1),
                (1, 1, 16, -1, 1, 1), (1, 1, 16, 1, -1, 1), (1, 1, 16, 1, 1, -1),
                (1, 1, 16, 1, -2, -2), (-(1 << 31), 1, 16, 1, 1, 1)):
        assert lib.miclip_tip_scratch_bytes(*bad) == 0, bad


def test_entries_refuse_every_bad_size_before_any_launch():
    """Each entry returns MICLIP_EINVAL and names the argument for sizes below, above and
    far below its limits (negative values included); the refusal comes before any HIP call,
    so host memory stands in for the device pointers here."""
    import ctypes
    from miclip import _lib
    lib = _lib.load_library()
    raw = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    ok = dict(Nq=2, Nk=3, E=16, C=2, nb=2, na=2)
    F32 = _lib.MICLIP_F32

    def grid(a):
        return lib.miclip_tip_grid(p, p, p, p, p, p, a["Nq"], a["Nk"], a["C"], a["nb"], a["na"], p,
                                   p, None)

    def logits(a):
        return lib.miclip_tip_logits(p, p, p, a["Nq"], a["Nk"], a["C"], 1.0, 1.0, p, p, None)

    def aff(a):
        return lib.miclip_tip_affinity(p, F32, p, a["Nq"], a["Nk"], a["E"], 1.0, p, None)

    def keys(a):
        return lib.miclip_tip_keys(p, F32, a.get("A", 1), a["Nk"], a.get("Wv", 16), a["E"], p, p,
                                   None)

    bad = {"Nq": (0, -1, -(1 << 31), (1 << 24) + 1), "Nk": (0, -1, -65536, 65537),
           "E": (0, -16, 8, 24, 1040), "C": (0, -1, -1024, 1025), "nb": (0, -1, 1025),
           "na": (0, -1, 1025), "A": (0, -1, 1025), "Wv": (0, -16, 8, 40, 65552)}
    for fn, names in ((grid, ("Nq", "Nk", "C", "nb", "na")), (logits, ("Nq", "Nk", "C")),
                      (aff, ("Nq", "Nk", "E")), (keys, ("Nk", "E", "A", "Wv"))):
        for name in names:
            for v in bad[name]:
                rc = fn(dict(ok, **{name: v}))
                msg = lib.miclip_last_error().decode()
                assert rc == -1 and msg.startswith(name + " must"), (fn.__name__, name, v, rc, msg)
    assert grid(dict(ok, nb=1024, na=65)) == -1
    assert lib.miclip_last_error().decode().startswith("nb * na")
    # misaligned operands
    q = ctypes.c_void_p(p.value + 4)
    assert lib.miclip_tip_keys(p, F32, 1, 3, 16, 16, q, p, None) == -1
    assert lib.miclip_tip_keys(p, F32, 1, 3, 16, 16, p, q, None) == -1
    assert lib.miclip_tip_keys(q, F32, 1, 3, 16, 16, p, p, None) == -1
    assert lib.miclip_tip_affinity(q, F32, p, 2, 3, 16, 1.0, p, None) == -1
    assert lib.miclip_tip_grid(p, p, p, p, p, p, 2, 3, 2, 2, 2, p, q, None) == -1
    assert lib.miclip_tip_logits(p, p, p, 2, 3, 2, 1.0, 1.0, p, q, None) == -1
