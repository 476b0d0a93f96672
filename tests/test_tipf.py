"""CPU: the Tip-Adapter-F yardstick tests/_tipf_ref.py pinned to torch (closed-form dK
against float64 autograd; the AdamW + cosine restatement against torch.optim.AdamW under
CosineAnnealingLR), the seeds of the GPU trajectory test (0 undecided rows in the
restatement alone), and the host checks of miclip.tip's Tip-Adapter-F entry points, which
come before any device is touched."""
import ctypes

import pytest
import torch

import _tip_ref as R
import _tipf_ref as TF

SHAPES = [(33, 17, 16, 3), (257, 130, 48, 20)]      # (b, Nk, E, C)


def _batch(b, Nk, E, C, seed=5):
    d = R.planted(b, Nk, E, C, seed=seed)
    F, K, W = (torch.tensor(d[k], dtype=torch.float64) for k in ("F", "K", "W"))
    return F, K, (100.0 * F) @ W, R._idx(d["labels"]), d["key_labels"]


@pytest.mark.parametrize("shape", SHAPES)
def test_closed_form_gradient_is_autograd(shape):
    F, K, Z, y, klab = _batch(*shape)
    for _, beta, alpha in TF.CONFIGS:
        dK, loss, _ = TF.grad_closed(K, F, Z, y, klab, beta, alpha)
        aK, aloss, _ = TF.grad_autograd(K, F, Z, y, klab, beta, alpha)
        err = TF.rel(dK, aK)
        print(f"{shape} beta {beta} alpha {alpha}: closed-form dK against autograd {err:.3e}")
        assert err <= 1e-12 and abs(float(loss) - float(aloss)) <= 1e-12 * abs(float(aloss))


@pytest.mark.parametrize("shape", SHAPES)
def test_adamw_cosine_restatement_is_torch(shape):
    """6 steps (2 epochs x 3 batches, the last one partial) of both forms in float64."""
    b, Nk, E, C = shape
    d = R.planted(b, Nk, E, C, seed=6)
    views = TF.views_of(d, 2, 6)
    bs = (b + 2) // 3 + 1
    assert (b + bs - 1) // bs == 3 and b % bs
    for lr, beta, alpha in TF.CONFIGS:
        args = (views, d["labels"], d["K"], d["W"], d["key_labels"], lr, beta, alpha)
        a = TF.fit(*args, epochs=2, batch_size=bs, seed=3)
        t = TF.fit(*args, epochs=2, batch_size=bs, seed=3, form="autograd")
        K0 = torch.tensor(d["K"], dtype=torch.float64)
        err = TF.rel(a["keys"][-1] - K0, t["keys"][-1] - K0)
        print(f"{shape} lr {lr}: restated AdamW against torch.optim.AdamW, update error {err:.3e}")
        assert len(a["ce"]) == 6 and err <= 1e-12
        assert TF.rel(a["ce"], t["ce"]) <= 1e-12 and a["correct"] == t["correct"]


@pytest.mark.parametrize("seed", TF.SEEDS)
@pytest.mark.parametrize("idx", range(len(TF.CASES)), ids=TF.IDS)
def test_trajectory_seeds_have_no_undecided_rows(idx, seed):
    """The GPU trajectory test allows the training count to differ from float64 on
    undecided rows only; for its seeds the restatement alone has none at any step, so the
    allowance hides nothing."""
    for shuffle in (True, False):
        for dname in ("fp32", "fp16"):
            c = TF.trajectory_case(idx, seed, shuffle, dname)
            for g, f in enumerate(c["fits"]):
                print(f"{TF.IDS[idx]} seed {seed} shuffle {shuffle} {dname} config {g}: undecided "
                      f"{f['undecided']}, smallest margin {f['min_margin']:.3e}, largest logit "
                      f"error {f['max_err']:.3e}, float32 errors keys {f['err_keys']:.2e} "
                      f"CE {f['err_ce']:.2e}")
                assert sum(f["undecided"]) == 0
                assert f["f32"]["correct"] == f["f64"]["correct"]


def _inputs(n=6, Nk=4, E=16, C=3):
    g = torch.Generator().manual_seed(0)
    keys = torch.randn(E, Nk, generator=g)
    values = torch.nn.functional.one_hot(torch.arange(Nk) % C, C).half()
    feats = torch.randn(n, E, generator=g)
    labels = torch.arange(n) % C
    W = torch.randn(E, C, generator=g)
    return keys, values, W, feats, labels


def test_fit_adapter_grid_refuses_bad_inputs_on_the_host():
    from miclip import tip
    keys, values, W, feats, labels = _inputs()

    def fit(k=keys, v=values, w=W, f=feats, y=labels, lrs=(1e-3,), betas=(1.0,), alphas=(1.0,),
            **kw):
        kw.setdefault("epochs", 1)
        return tip.fit_adapter_grid(k, v, w, f, y, list(lrs), list(betas), list(alphas), **kw)

    with pytest.raises(ValueError, match="common length"):
        fit(lrs=(), betas=(), alphas=())
    with pytest.raises(ValueError, match="common length"):
        fit(betas=(1.0, 2.0))
    with pytest.raises(ValueError, match="at most 64"):
        fit(lrs=[1e-3] * 65, betas=[1.0] * 65, alphas=[1.0] * 65)
    with pytest.raises(ValueError, match="finite"):
        fit(lrs=(float("nan"),))
    with pytest.raises(ValueError, match="finite"):
        fit(betas=(float("inf"),))
    with pytest.raises(TypeError, match="sequence"):
        tip.fit_adapter_grid(keys, values, W, feats, labels, 1e-3, [1.0], [1.0], epochs=1)
    for kw in (dict(epochs=0), dict(epochs=1.5), dict(batch_size=0), dict(batch_size=4097),
               dict(weight_decay=-1.0), dict(eps=-1e-4), dict(eps=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            fit(**kw)
    bad = values.clone()
    bad[1, 0] = 0.5
    with pytest.raises(ValueError, match="one-hot"):
        fit(v=bad)
    with pytest.raises(ValueError, match="one-hot"):
        fit(v=torch.zeros_like(values))
    with pytest.raises(ValueError, match="rows"):
        fit(v=values[:3])
    with pytest.raises(ValueError, match="width"):
        fit(f=feats[:, :8])
    with pytest.raises(ValueError, match="differs"):
        fit(f=[feats, feats[:-1]])
    with pytest.raises(ValueError, match="differs"):
        fit(f=[feats, feats.half()])
    with pytest.raises(ValueError, match="no training views"):
        fit(f=[])
    with pytest.raises(ValueError, match="clip_weights"):
        fit(w=W[:8])
    with pytest.raises(ValueError, match="unsupported shapes"):
        fit(k=torch.randn(24, 4), f=torch.randn(6, 24), w=torch.randn(24, 3))
    for lab in (labels + 1, labels - 1):
        with pytest.raises(ValueError, match=r"train_labels must lie in \[0, 3\)"):
            fit(y=lab)
    with pytest.raises(ValueError, match="train_labels"):
        fit(y=labels[:-1])
    with pytest.raises(TypeError, match="integer"):
        fit(y=labels.float())
    with pytest.raises(ValueError, match="go together"):
        fit(eval_features=feats)
    with pytest.raises(ValueError, match=r"eval_labels must lie in \[0, 3\)"):
        fit(eval_features=feats, eval_labels=labels + 1)
    with pytest.raises(ValueError, match="width"):
        fit(eval_features=feats[:, :8], eval_labels=labels)
    with pytest.raises(ValueError, match="keep_epochs"):
        fit(k=torch.randn(1024, 4096), v=torch.nn.functional.one_hot(torch.arange(4096) % 3, 3),
            w=torch.randn(1024, 3), f=torch.randn(6, 1024), epochs=70, keep_epochs=True)
    with pytest.raises(TypeError, match="one number"):
        tip.fit_adapter(keys, values, W, feats, labels, [1e-3], 1.0, 1.0, epochs=1)
    with pytest.raises(ValueError, match="one-hot"):
        tip.fit_adapter(keys, bad, W, feats, labels, 1e-3, 1.0, 1.0, epochs=1)


def test_tip_adapter_f_refuses_bad_inputs_on_the_host():
    from miclip import tip
    keys, values, W, feats, labels = _inputs()
    tf = {"lr": 1e-3, "train_epoch": 2, "init_beta": 1.0, "init_alpha": 1.17}
    cfg = {"search_hp": True, "search_scale": [7, 3], "search_step": [3, 2], "tip_f": tf}

    def run(c=cfg, v=values, f=feats, y=labels, tfeat=feats, ty=labels):
        return tip.tip_adapter_f(c, keys, v, f, y, tfeat, ty, W)

    with pytest.raises(ValueError, match="tip_f"):
        run(c={k: v for k, v in cfg.items() if k != "tip_f"})
    with pytest.raises(ValueError, match="train_epoch"):
        run(c=dict(cfg, tip_f={k: v for k, v in tf.items() if k != "train_epoch"}))
    with pytest.raises(ValueError, match="unknown"):
        run(c=dict(cfg, tip_f=dict(tf, momentum=0.9)))
    with pytest.raises(ValueError, match="search_hp"):
        run(c=dict(cfg, search_hp=False))
    with pytest.raises(ValueError, match="epochs"):
        run(c=dict(cfg, tip_f=dict(tf, train_epoch=0)))
    with pytest.raises(ValueError, match="test_features"):
        run(tfeat=None)
    bad = values.clone()
    bad[0] = 0
    with pytest.raises(ValueError, match="one-hot"):
        run(v=bad)
    with pytest.raises(ValueError, match=r"train_labels must lie in \[0, 3\)"):
        run(y=labels + 1)
    with pytest.raises(ValueError, match=r"eval_labels must lie in \[0, 3\)"):
        run(ty=labels - 1)
    with pytest.raises(ValueError, match="width"):
        run(tfeat=feats[:, :8])


def test_exports_symbols_and_limits():
    import miclip
    from miclip import _lib
    for name in ("fit_adapter_grid", "fit_adapter", "tip_adapter_f", "AdapterFit"):
        assert callable(getattr(miclip, name)) and name in miclip.__all__
        assert name in miclip.tip.__all__
    names = ("miclip_tipf_scratch_bytes", "miclip_tipf_prepare", "miclip_tipf_step",
             "miclip_tipf_keep_best")
    assert set(names) <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 10
    lib = _lib.load_library()
    for name in names:
        assert getattr(lib, name).argtypes is not None
    assert lib.miclip_abi_version() == 10
    # the scratch query is host-only: positive inside the limits, 0 outside
    assert lib.miclip_tipf_scratch_bytes(1, 1, 16, 1, 1) > 0
    assert lib.miclip_tipf_scratch_bytes(4096, 65536, 1024, 1024, 64) > 0
    # order, offsets, rows, phi, gm, partials, each rounded up to 256 bytes
    assert lib.miclip_tipf_scratch_bytes(256, 4200, 512, 20, 1) == \
        16896 + 256 + 1024 + 256 * 4200 * 4 + 256 * 20 * 4 + 256
    for bad in ((0, 1, 16, 1, 1), (4097, 1, 16, 1, 1), (1, 0, 16, 1, 1), (1, 65537, 16, 1, 1),
                (1, 1, 8, 1, 1), (1, 1, 24, 1, 1), (1, 1, 1040, 1, 1), (1, 1, 16, 0, 1),
                (1, 1, 16, 1025, 1), (1, 1, 16, 1, 0), (1, 1, 16, 1, 65), (-1, 1, 16, 1, 1),
                (1, -1, 16, 1, 1), (1, 1, -16, 1, 1), (1, 1, 16, -1, 1), (1, 1, 16, 1, -1)):
        assert lib.miclip_tipf_scratch_bytes(*bad) == 0, bad


def test_step_refuses_bad_arguments_before_any_launch():
    """miclip_tipf_step and miclip_tipf_keep_best return MICLIP_EINVAL and name the argument;
    the refusal comes before any HIP call, so host memory stands in for device pointers."""
    from miclip import _lib
    lib = _lib.load_library()
    raw = ctypes.create_string_buffer(8192 + 256)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 255) & ~255)
    rows = (ctypes.c_int64 * 4)(0, 1, 2, 1)
    ok = dict(n=3, b=4, Nk=3, E=16, C=2, G=1, lr_factor=1.0, wd=0.01, eps=1e-4, step=1, rows=rows,
              dtype=_lib.MICLIP_F32, F=p, scratch=p)

    def step(**kw):
        a = dict(ok, **kw)
        return lib.miclip_tipf_step(a["F"], a["dtype"], a["n"], a["rows"], a["b"], p, p, p, p, p, p,
                                    p, p, p, a["Nk"], a["E"], a["C"], a["G"], a["lr_factor"],
                                    a["wd"], a["eps"], a["step"], p, None, a["scratch"], None)

    def refused(rc, name):
        msg = lib.miclip_last_error().decode()
        print(f"rc {rc}: {msg}")
        assert rc == -1 and msg.startswith(name), (name, msg)

    for kw, name in ((dict(n=0), "n must"), (dict(n=(1 << 24) + 1), "n must"), (dict(b=0), "b must"),
                     (dict(b=4097), "b must"), (dict(Nk=0), "Nk must"), (dict(Nk=65537), "Nk must"),
                     (dict(E=8), "E must"), (dict(E=24), "E must"), (dict(E=1040), "E must"),
                     (dict(C=0), "C must"), (dict(C=1025), "C must"), (dict(G=0), "G must"),
                     (dict(G=65), "G must"), (dict(step=0), "step must"),
                     (dict(lr_factor=float("nan")), "lr_factor must"),
                     (dict(wd=-0.5), "weight_decay must"), (dict(wd=float("inf")), "weight_decay must"),
                     (dict(eps=-1.0), "eps must"), (dict(eps=float("nan")), "eps must"),
                     (dict(dtype=7), "f_dtype must"), (dict(F=None), "null argument: F"),
                     (dict(rows=None), "null argument: rows_host"),
                     (dict(scratch=ctypes.c_void_p(p.value + 16)), "scratch:"),
                     (dict(F=ctypes.c_void_p(p.value + 4)), "F / keys"),
                     (dict(rows=(ctypes.c_int64 * 4)(0, 1, 3, 1)), "rows_host[2] must"),
                     (dict(rows=(ctypes.c_int64 * 4)(0, -1, 2, 1)), "rows_host[1] must")):
        refused(step(**kw), name)

    def keep(epoch=0, Nk=3, E=16, G=1, counts=p):
        return lib.miclip_tipf_keep_best(counts, epoch, p, p, p, p, Nk, E, G, None)

    refused(keep(epoch=-1), "epoch must")
    refused(keep(Nk=0), "Nk must")
    refused(keep(E=20), "E must")
    refused(keep(G=65), "G must")
    refused(keep(counts=None), "null argument: counts")
    refused(lib.miclip_tipf_prepare(p, 0, 2, p, None), "Nk must")
    refused(lib.miclip_tipf_prepare(p, 3, 1025, p, None), "C must")
    refused(lib.miclip_tipf_prepare(None, 3, 2, p, None), "null argument: key_labels")
