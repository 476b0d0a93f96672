"""CPU: the ProLIP training module's surface, host logic and argument validation, the
two C entry points' validation (before any device access), and the golden fixture
against the closed-form fp64 restatement that the GPU tests use as their yardstick.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import _prolip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j", "8"], check=True)
    return _lib.load_library()


def test_module_surface_and_state_dict_key():
    from miclip import prolip
    for name in ("VisProjViT", "fit_projector_grid", "fit_projector", "search_hp", "ProLIP",
                 "GridFit", "view_cycle", "schedule_factor"):
        assert hasattr(prolip, name), name
    assert tuple(prolip.LR_LIST) == (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8)
    assert tuple(prolip.LAMBDA_LIST) == (10, 1, 0.1, 0.01, 0.001, 0.0001, 0)
    w = torch.arange(12.0).reshape(4, 3)
    m = prolip.VisProjViT(w.clone())
    assert list(m.state_dict().keys()) == ["vit_proj"]
    assert m.vit_proj.requires_grad
    x = torch.ones(2, 4)
    assert torch.equal(m(x), x @ w)
    assert callable(prolip.ProLIP({"backbone": "ViT-L/14"}))


def test_view_cycle_and_schedule_factor():
    from miclip import prolip
    # the reference's counter starts at 0 and steps before use (methods/ProLIP.py:171-185)
    assert prolip.view_cycle(7, 3) == [1, 2, 0, 1, 2, 0, 1]
    assert prolip.view_cycle(4, 1) == [0, 0, 0, 0]
    assert prolip.view_cycle(5, 2) == [1, 0, 1, 0, 1]
    assert prolip.view_cycle(7, 3) == R.view_cycle(7, 3)
    # CosineAnnealingLR(T_max=12): recorded from torch's scheduler
    sched_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(sched_opt, 12)
    for epoch in range(12):
        want = sched_opt.param_groups[0]["lr"]
        assert prolip.schedule_factor(epoch, 12) == pytest.approx(want, abs=1e-12)
        sched_opt.step()
        sched.step()
    assert prolip.schedule_factor(0, 5) == 1.0
    assert prolip.schedule_factor(3, 12) == pytest.approx(0.5 * (1 + math.cos(math.pi / 4)))


def _args(n=8, D=32, E=16, C=4, V=2, dtype=torch.float16):
    g = torch.Generator().manual_seed(0)
    views = [torch.randn(n, D, generator=g).to(dtype) for _ in range(V)]
    labels = torch.randint(0, C, (n,), generator=g)
    return views, labels, torch.randn(D, E, generator=g), torch.randn(E, C, generator=g)


def test_validation_raises_before_any_device_access():
    """Every one of these must raise ValueError / TypeError from the host checks; on a
    machine without a HIP device a later failure would be a RuntimeError instead."""
    from miclip import prolip
    views, labels, P0, W = _args()
    kw = dict(epochs=2)
    fit = prolip.fit_projector_grid
    with pytest.raises(ValueError, match="no feature views"):
        fit([], labels, P0, W, [1e-3], [0.1], **kw)
    with pytest.raises(ValueError, match="shape"):
        fit([views[0][0]], labels, P0, W, [1e-3], [0.1], **kw)
    with pytest.raises(TypeError, match="dtype"):
        fit([views[0].double()], labels, P0, W, [1e-3], [0.1], **kw)
    with pytest.raises(ValueError, match="width"):
        fit([views[0][:, :16]], labels, P0, W, [1e-3], [0.1], **kw)
    with pytest.raises(ValueError, match="labels shape"):
        fit(views, labels[:-1], P0, W, [1e-3], [0.1], **kw)
    with pytest.raises(TypeError, match="integer labels"):
        fit(views, labels.float(), P0, W, [1e-3], [0.1], **kw)
    bad = labels.clone()
    bad[3] = 4
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 4\)"):
        fit(views, bad, P0, W, [1e-3], [0.1], **kw)
    bad[3] = -1
    with pytest.raises(ValueError, match="labels must lie"):
        fit(views, bad, P0, W, [1e-3], [0.1], **kw)
    with pytest.raises(ValueError, match="differs from views"):
        fit([views[0], views[1][:-1]], labels, P0, W, [1e-3], [0.1], **kw)
    with pytest.raises(ValueError, match="paired"):
        fit(views, labels, P0, W, [1e-3, 1e-4], [0.1], **kw)
    with pytest.raises(ValueError, match="paired"):
        fit(views, labels, P0, W, [], [], **kw)
    with pytest.raises(ValueError, match="epochs"):
        fit(views, labels, P0, W, [1e-3], [0.1], epochs=0)
    with pytest.raises(ValueError, match="text_weights must be"):
        fit(views, labels, P0, W[:-1], [1e-3], [0.1], **kw)
    v40, _, P40, _ = _args(D=40)
    with pytest.raises(ValueError, match="unsupported shapes"):
        fit(v40, labels, P40, W, [1e-3], [0.1], **kw)
    with pytest.raises(ValueError, match="must not be empty"):
        prolip.search_hp(views, labels, P0, W, views[0], labels, epochs=2, lr_list=[])
    with pytest.raises(ValueError, match="width"):
        prolip.search_hp(views, labels, P0, W, views[0][:, :16], labels, epochs=2)
    with pytest.raises(ValueError, match="ViT only"):
        prolip.ProLIP({"backbone": "RN50", "dataset": "cs"})(None, None, None)
    with pytest.raises(ValueError, match="imagenet"):
        prolip.ProLIP({"backbone": "ViT-B/16", "dataset": "imagenet"})(None, None, None)


def test_entry_points_reject_bad_arguments_before_device_access(lib):
    from miclip import _lib
    p = ctypes.c_void_p(1 << 20)   # never dereferenced: validation comes first
    n, D, E, C, G = 8, 32, 16, 4, 2

    def grad(x=p, dt=_lib.MICLIP_FP16, n=n, D=D, E=E, C=C, G=G, dz=p):
        return lib.miclip_prolip_grad(x, dt, p, n, D, E, C, p, p, G, 100.0, dz, p, None)

    def adam(x=p, dt=_lib.MICLIP_FP16, n=n, D=D, E=E, G=G, step=1, div=1.0, hist=p):
        return lib.miclip_prolip_adam(x, dt, p, n, D, E, G, p, p, p, p, p, p, 1.0, div, step, 1e-4,
                                      p, p, hist, None)

    assert grad(x=None) == -1 and b"null" in lib.miclip_last_error()
    assert grad(dz=None) == -1
    assert adam(x=None) == -1
    assert adam(hist=None) == -1
    for kw in (dict(n=0), dict(D=40), dict(D=0), dict(D=1296), dict(E=24), dict(E=1040),
               dict(C=0), dict(C=1025), dict(G=0), dict(dt=_lib.MICLIP_MXFP8), dict(dt=7),
               dict(x=ctypes.c_void_p((1 << 20) + 4))):
        assert grad(**kw) == -1, kw
    for kw in (dict(n=0), dict(D=40), dict(D=1296), dict(E=24), dict(E=1040), dict(G=0),
               dict(step=0), dict(div=0.0), dict(dt=_lib.MICLIP_MXFP8)):
        assert adam(**kw) == -1, kw


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_golden_agrees_with_fp64_restatement(gold, case):
    """The fixture (the reference's fp32 CPU run) and the yardstick (closed-form fp64)
    describe the same computation: their distance e_ref is fp32 rounding accumulated
    over the run, far below what training moved the weights by (5% of max|P - P0|
    here; a wrong formula, schedule, view order or chunk rule is of the order of
    the movement itself)."""
    views, y, P0, W, lrs, lams, T, bs = R.case_inputs(gold, case)
    gp = gold[f"{case}_proj"]
    gp = gp[None] if gp.ndim == 2 else gp
    assert gp.shape[0] == len(lrs)
    for k, (lr, lam) in enumerate(zip(lrs, lams)):
        P, hist = R.restate(views, y, P0, W, lr, lam, T, bs)
        e_ref = np.abs(gp[k] - P).max()
        moved = np.abs(P - P0).max()
        print(f"case {case} cfg {k}: e_ref {e_ref:.3g}, moved {moved:.3g}")
        assert e_ref < 0.05 * moved
        assert hist.shape == (T * (math.ceil(len(y) / bs) if bs else 1), 3)
    if case == "b":
        loss = hist[-1, 0] + lams[0] / math.ceil(len(y) / bs) * hist[-1, 1]
        assert loss == pytest.approx(float(gold["b_loss"]), abs=1e-5)
        tx, ty = gold["a_test_x"].astype(np.float64), gold["a_test_y"]
        f = tx @ P
        lg = (f / np.linalg.norm(f, axis=1, keepdims=True)) @ W.astype(np.float64)
        assert 100.0 * np.mean(lg.argmax(1) == ty) == pytest.approx(float(gold["b_acc"]))


def test_golden_search_table_agrees_with_fp64_restatement(gold):
    views, y, P0, W, lrs, lams, T, _ = R.case_inputs(gold, "s")
    vx, vy = gold["s_val_x"].astype(np.float64), gold["s_val_y"]
    assert gold["s_margin"].min() >= 1e-3
    accs = []
    for lr, lam in zip(lrs, lams):
        P, _ = R.restate(views, y, P0, W, lr, lam, T)
        f = vx @ P
        lg = (f / np.linalg.norm(f, axis=1, keepdims=True)) @ W.astype(np.float64)
        accs.append(100.0 * np.mean(lg.argmax(1) == vy))
    assert np.allclose(np.array(accs).reshape(7, 7), gold["s_acc"])
    best, pick = 0.0, None
    for (lr, lam), a in zip(zip(lrs, lams), accs):
        if a > best:
            best, pick = a, (lr, lam)
    assert pick == (float(gold["s_lr"]), float(gold["s_lam"]))
