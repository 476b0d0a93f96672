"""GPU: last-group fine-tuning of the image tower (miclip/finetune.py, csrc/finetune.hip),
unlocked_groups 1 (visual.proj) and 2 (the last block and ln_post), fp16 and bf16. The tail's
op-level gradient tests are in tests/test_gpu_finetune_tail.py.

Op level, cases (B, W, E, C): the base case; one row with E = 16 and C = 3 (one 16-column
tile, K tail of the TN GEMM's 64-column tile); 33 rows (a second 32-row stage and slice,
a 16-row tile tail in the head kernel); 5 rows; width 640 / E 128 (the head-dim-80 tower's
shapes); 70 rows at ViT-H-14's width 1280.

  * dP: relative Frobenius error against float64 autograd <= 4 * e_ref, e_ref the error
    of the same step under torch.autocast('cpu') with fp32 masters (the reference's own
    rounding; tests/_ft_ref.py). Measured on the CPU while writing this: e_ref 5.1e-4 ..
    1.6e-3 (fp16) and 4.8e-3 .. 9.5e-3 (bf16); a restatement that rounds y and dZ once,
    as the kernels do, 2.8e-4 .. 3.0e-4 and 2.3e-3 .. 2.4e-3. The factor 4 is the project's.
  * loss: |loss - fp64| <= 4 * max(e_ref(loss), 8 * 2^-23 * |loss|); correct count exact.
  * a zero feature row (|z| clamps at 1e-12) and features collinear with a class (logit 100)
    give finite results; two runs are bit-identical.

Adam: 3 steps on 1, 63 and 64 * 1024 + 1 elements against torch.optim.Adam on the CPU, bar
4 * max(|torch fp32 - fp64 restatement|, 2^-23 * max|p|).

Trajectory: 20 steps on the fixed batch of the base case with lr = 3e-5, chosen on the CPU
so that the float64 loss falls from 11.29 to 2.98 (more than a third) and never reaches
zero. Losses are compared, not parameters (Adam's first steps are sign-like). The autocast
run's per-step deviation from float64 swings between 3e-4 and 1e-2 (fp16) from step to step
as it changes sign, so the bar of every step is 4 x the run's largest per-step deviation.

Model level, seeded 2-layer tower (W 256, resolution 64, patch 32, N = 5, E 64), on the
open_clip surface, groups 1 and 2: the trunk followed by the tail's forward against
oracle/clip_oracle.py at tests/test_gpu_parity.py's 1 - cos bar; trunk rows and features of
B = 3 equal each image run alone, bitwise; after two steps and commit() the frozen
Parameters are bit-unchanged, the unlocked ones changed, and encode_image meets the same bar
against the oracle on the updated state dict; FTOpenCLIP for 2 epochs with val, test,
save_model and cache_embeddings.
"""
import ctypes

import numpy as np
import pytest
import torch

import _ft_ref as R

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3      # tests/test_gpu_parity.py
DTYPES = {"fp16": (0, torch.float16), "bf16": (1, torch.bfloat16)}
CASES = [(3, 256, 64, 5), (1, 256, 16, 3), (33, 256, 64, 20), (5, 256, 64, 5),
         (2, 640, 128, 20), (70, 1280, 256, 40)]
TRAJ_LR = 3e-5


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    assert torch.cuda.is_available()
    return _lib.load_library()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    from miclip import _lib
    return _lib.stream_handle(torch.device("cuda"))


def _proj_grad(lib, y, P, W, labels, name):
    """(sum CE, correct, dP) of miclip_ft_proj_grad; dP sits between canaries."""
    from miclip import _lib
    B, Wd = y.shape
    E, C = P.shape[1], W.shape[1]
    nbytes = lib.miclip_ft_proj_scratch_bytes(B, Wd, E, C)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 256, device="cuda", dtype=torch.uint8)
    scratch[nbytes:] = 0xA5
    pad = 64
    out = torch.full((Wd * E + 2 * pad,), -7.0, device="cuda")
    dP = out[pad:pad + Wd * E]
    stats = torch.full((4,), -7.0, device="cuda")
    yd, Pd, Wd_, ld = (t.cuda().contiguous() for t in (y.float(), P.float(), W.float(),
                                                       labels.long()))
    _lib.check(lib.miclip_ft_proj_grad(_ptr(yd), _ptr(ld), _ptr(Wd_), _ptr(Pd), B, Wd, E, C,
                                       DTYPES[name][0], 100.0, _ptr(dP), _ptr(scratch),
                                       _ptr(stats), _stream()), "miclip_ft_proj_grad")
    torch.cuda.synchronize()
    o, st = out.cpu(), stats.cpu()
    assert bool((o[:pad] == -7.0).all()) and bool((o[pad + Wd * E:] == -7.0).all())
    assert bool((scratch[nbytes:] == 0xA5).all()) and bool((st[2:] == -7.0).all())
    return float(st[0]), float(st[1]), o[pad:pad + Wd * E].reshape(Wd, E).clone()


_REF = {}


def _ref(shape, name):
    key = (shape, name)
    if key not in _REF:
        y, P, W, labels = R.head_case(*shape, seed=3)
        loss64, correct, dP64 = R.autograd_run(y, P, W, labels)
        loss_h, dP_h = R.autocast_run(y, P, W, labels, DTYPES[name][1])
        _REF[key] = (y, P, W, labels, loss64, correct, dP64, abs(loss_h - loss64),
                     R.rel_fro(dP_h, dP64))
    return _REF[key]


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_proj_grad_against_float64_autograd(lib, shape, name):
    y, P, W, labels, loss64, correct, dP64, e_loss, e_dP = _ref(shape, name)
    ce_sum, ok, dP = _proj_grad(lib, y, P, W, labels, name)
    loss = ce_sum / shape[0]
    err = R.rel_fro(dP, dP64)
    loss_bar = 4.0 * max(e_loss, 8.0 * R.EPS32 * abs(loss64))
    print(f"proj_grad {shape} {name}: dP rel {err:.3e} e_ref {e_dP:.3e} ratio {err / e_dP:.2f}; "
          f"loss err {abs(loss - loss64):.3e} bar {loss_bar:.3e}; correct {ok} / {correct}")
    assert np.isfinite(err) and err <= 4.0 * e_dP
    assert abs(loss - loss64) <= loss_bar
    assert ok == correct
    ce2, ok2, dP2 = _proj_grad(lib, y, P, W, labels, name)
    assert ce2 == ce_sum and ok2 == ok and torch.equal(dP, dP2)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_proj_grad_degenerate_rows_are_finite(lib, name):
    y, P, W, labels = R.head_case(4, 256, 64, 5, seed=9)
    y[1] = 0.0                                            # z = 0: the norm clamps at 1e-12
    # row 2: features collinear with class 3 -> logit 100 exactly on that class
    y[2] = torch.linalg.lstsq(P.double().t(), W.double()[:, 3:4]).solution[:, 0].float()
    labels[2] = 3
    ce_sum, ok, dP = _proj_grad(lib, y, P, W, labels, name)
    assert np.isfinite(ce_sum) and bool(torch.isfinite(dP).all())
    logits = R.head_logits(y.double(), P.double(), W.double())
    assert abs(float(logits[2, 3]) - 100.0) < 1e-3
    loss64, correct, dP64 = R.autograd_run(y, P, W, labels)
    assert ok == correct
    assert abs(ce_sum / 4 - loss64) <= 1e-4 * abs(loss64)


@pytest.mark.parametrize("numel", [1, 63, 64 * 1024 + 1])
def test_adam_against_torch(lib, numel):
    from miclip import _lib
    rng = np.random.default_rng(numel)
    p0 = rng.standard_normal(numel).astype(np.float32)
    grads = [(rng.standard_normal(numel) * 10.0 ** -k).astype(np.float32) for k in range(3)]
    lr = 1e-3
    want64 = R.adam_fp64(p0, grads, lr)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=lr)
    p = torch.from_numpy(p0.copy()).cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, g in enumerate(grads, start=1):
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        gd = torch.from_numpy(g).cuda()
        _lib.check(lib.miclip_ft_adam(_ptr(p), _ptr(gd), _ptr(m), _ptr(v), numel, lr, t, 1e-8,
                                      _stream()), "miclip_ft_adam")
        torch.cuda.synchronize()
        e_ref = float(np.abs(pt.detach().numpy().astype(np.float64) - want64[t - 1]).max())
        bar = 4.0 * max(e_ref, R.EPS32 * float(np.abs(want64[t - 1]).max()))
        err = float(np.abs(p.cpu().numpy().astype(np.float64) - want64[t - 1]).max())
        print(f"adam n={numel} step {t}: err {err:.3e} e_ref {e_ref:.3e} bar {bar:.3e}")
        assert err <= bar


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_trajectory_follows_float64(lib, name):
    from miclip import _lib
    shape, steps = CASES[0], 20
    y, P, W, labels = R.head_case(*shape, seed=3)
    want = R.trajectory(y, P, W, labels, TRAJ_LR, steps, torch.float64)
    ref = R.trajectory(y, P, W, labels, TRAJ_LR, steps, DTYPES[name][1])
    assert want[-1] <= want[0] * 2 / 3 and want[-1] > 0.5           # the lr's choice, recorded
    bar = 4.0 * max(abs(a - b) for a, b in zip(ref, want))
    B, Wd, E, C = shape
    nbytes = lib.miclip_ft_proj_scratch_bytes(B, Wd, E, C)
    scratch = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    yd, Wt, ld = y.cuda().contiguous(), W.cuda().contiguous(), labels.long().cuda()
    p = P.float().cuda().contiguous()
    g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    stats = torch.zeros(steps, 2, device="cuda")
    for t in range(steps):
        _lib.check(lib.miclip_ft_proj_grad(_ptr(yd), _ptr(ld), _ptr(Wt), _ptr(p), B, Wd, E, C,
                                           DTYPES[name][0], 100.0, _ptr(g), _ptr(scratch),
                                           _ptr(stats[t]), _stream()), "miclip_ft_proj_grad")
        _lib.check(lib.miclip_ft_adam(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), TRAJ_LR,
                                      t + 1, 1e-8, _stream()), "miclip_ft_adam")
    got = (stats[:, 0].cpu().double() / B).tolist()
    dev = [abs(a - b) for a, b in zip(got, want)]
    print(f"trajectory {name}: first {got[0]:.4f} last {got[-1]:.4f} (fp64 {want[-1]:.4f}); "
          f"max dev {max(dev):.3e} bar {bar:.3e}")
    assert max(dev) <= bar
    assert got[-1] < got[0] * 2 / 3 and all(b < a for a, b in zip(got, got[1:]))


# ---- model level ----
def _tower(name):
    import miclip
    from miclip.configs import CLIPConfig
    from miclip.weights import generate_state_dict
    cfg = CLIPConfig(embed_dim=64, image_resolution=64, vision_layers=2, vision_width=256,
                     vision_patch_size=32, context_length=77, vocab_size=49408,
                     transformer_width=256, transformer_heads=4, transformer_layers=1)
    sd = generate_state_dict(cfg, seed=0)
    model = miclip.CLIP(cfg, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()},
                        device="cuda", compute_dtype=name, surface="open_clip")
    return cfg, sd, model


def _one_minus_cos(a, b):
    c = torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)
    return float((1 - c).max())


def _oracle_features(sd, cfg, imgs):
    from oracle import clip_oracle
    y = torch.as_tensor(clip_oracle.encode_image(sd, cfg, imgs)).double()
    return R.features(y, torch.as_tensor(np.asarray(sd["visual.proj"])).double())


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_trunk_and_tail_forward_match_the_oracle(name):
    from miclip.finetune import LastBlockTrainer
    from miclip.weights import synthetic_images
    cfg, sd, model = _tower(name)
    imgs = synthetic_images(3, 64, seed=5)
    x = torch.from_numpy(imgs).cuda()
    tw = torch.nn.functional.normalize(torch.randn(64, 5, generator=torch.Generator().manual_seed(1)),
                                       dim=0)
    tr = LastBlockTrainer(model, tw, unlocked_groups=2, lr=1e-3, epochs=2)
    want = _oracle_features(sd, cfg, imgs)
    assert _one_minus_cos(tr.features(x).cpu(), want) <= COS_TOL
    # a row of the trunk's output depends on its image alone: bitwise
    full = tr.trunk(x).clone()
    assert full.shape == (3 * 5, 256) and full.dtype == torch.float16
    for b in range(3):
        alone = tr.trunk(x[b:b + 1]).clone()
        assert torch.equal(alone, full[5 * b:5 * b + 5]), b
    f3 = tr.features(x).clone()
    for b in range(3):
        assert torch.equal(tr.features(x[b:b + 1]), f3[b:b + 1]), b


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_trainer_steps_and_commit(name, groups):
    from miclip.finetune import LastBlockTrainer, trainable_names
    from miclip.weights import synthetic_images
    cfg, sd, model = _tower(name)
    imgs = synthetic_images(3, 64, seed=5)
    x = torch.from_numpy(imgs).cuda()
    g = torch.Generator().manual_seed(1)
    tw = torch.nn.functional.normalize(torch.randn(64, 5, generator=g), dim=0)
    labels = torch.tensor([0, 3, 1])
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert _one_minus_cos(model.encode_image(x, normalize=True).cpu(),
                          _oracle_features(sd, cfg, imgs)) <= COS_TOL

    tr = LastBlockTrainer(model, tw, unlocked_groups=groups, lr=1e-3, epochs=2)
    unlocked = set(trainable_names(model, groups))
    assert len(unlocked) == (1 if groups == 1 else 15) and set(tr.names) == unlocked
    losses = []
    for e in range(2):
        tr.set_epoch(e)
        loss_sum, correct = tr.step(x, labels)
        assert loss_sum.is_cuda and correct.is_cuda and loss_sum.dim() == 0
        losses.append(float(loss_sum))
    assert losses[1] < losses[0]
    # nothing reaches the model before commit()
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    tr.commit()
    after = model.state_dict()
    for k in before:
        if k in unlocked:
            assert not torch.equal(before[k], after[k]), k
        else:
            assert torch.equal(before[k], after[k]), k
    sd2 = {k: (after[k].cpu().numpy() if k in unlocked else v) for k, v in sd.items()}
    got = model.encode_image(x, normalize=True, apply_proj=True).cpu()
    assert _one_minus_cos(got, _oracle_features(sd2, cfg, imgs)) <= COS_TOL
    # the first step's loss is that of the untrained model on the oracle's features
    y = torch.as_tensor(__import__("oracle.clip_oracle", fromlist=["x"]).encode_image(sd, cfg, imgs))
    loss64, _, _ = R.autograd_run(y, before["visual.proj"].cpu(), tw, labels)
    assert abs(losses[0] / 3 - loss64) <= 2e-2 * abs(loss64)
    osd = tr.optimizer_state_dict()
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(after[n].cpu())) for n in tr.names],
                           lr=1e-3)
    opt.load_state_dict(osd)
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0
    assert len(opt.state_dict()["state"]) == len(unlocked)
    with pytest.raises(ValueError, match="targets must lie"):
        tr.step(x, torch.tensor([0, 5, 1]))
    with pytest.raises(NotImplementedError):
        LastBlockTrainer(model, tw, unlocked_groups=3, lr=1e-3, epochs=2)
    with pytest.raises(ValueError):
        LastBlockTrainer(model, tw, unlocked_groups=0, lr=1e-3, epochs=2)
    with pytest.raises(NotImplementedError):
        model.lock_image_tower(unlocked_groups=groups)      # the model's own hooks still refuse


def test_mx_models_are_refused():
    from miclip.finetune import LastBlockTrainer

    class _M:
        compute_dtype = "mxfp8"

        def named_parameters(self):
            return iter([("visual.transformer.resblocks.0.ln_1.weight", None),
                         ("visual.proj", None)])
    with pytest.raises(NotImplementedError, match="MX-fp8"):
        LastBlockTrainer(_M(), torch.zeros(64, 5), unlocked_groups=1, lr=1e-3, epochs=1)


@pytest.mark.parametrize("groups", [1, 2])
def test_ftopenclip_end_to_end(tmp_path, capsys, groups):
    from miclip.finetune import FTOpenCLIP
    from miclip.weights import synthetic_images
    cfg_m, sd, model = _tower("fp16")
    g = torch.Generator().manual_seed(2)
    tw = torch.nn.functional.normalize(torch.randn(64, 5, generator=g), dim=0).cuda()

    def loader(seed, n_batches, B):
        out = []
        for b in range(n_batches):
            imgs = torch.from_numpy(synthetic_images(B, 64, seed=seed + b))
            out.append((imgs, torch.randint(0, 5, (B,), generator=g)))
        return out
    train, val, test = loader(10, 2, 4), loader(20, 1, 3), loader(30, 2, 3)
    cfg = {"lr_v": 1e-3, "train_epoch": 2, "root_path": str(tmp_path), "dataset": "cs", "seed": 1,
           "clip_backend": "openclip", "open_clip_model": "ViT-H-14",
           "finetune": {"unlocked_groups": groups, "tune_text": False, "val_interval": 1,
                        "save_model": True, "save_model_dir": "ckpt", "save_optimizer": True,
                        "save_scheduler": True, "cache_embeddings": True,
                        "cache_embeddings_split": "test"}}
    proj0 = model.visual.proj.detach().clone()
    method = FTOpenCLIP(cfg)
    res = method(train, val, test, tw, model, [f"c{i}" for i in range(5)], 0, "cfg", False)
    assert len(res) == 6 and all(isinstance(v, float) for v in res[:5])
    assert isinstance(res[5], np.ndarray) and res[5].shape == (5, 5) and res[5].sum() == 6
    resv = FTOpenCLIP(cfg)(train, val, None, tw, model, [f"c{i}" for i in range(5)], 0, "cfg",
                           True)
    assert len(resv) == 6 and isinstance(resv[0], float) and resv[5] is None
    assert not torch.equal(proj0, model.visual.proj.detach())
    out = capsys.readouterr().out
    for word in ("Trainable params: %d" % (1 if groups == 1 else 15), "Start Training procedure", "Train Epoch: 2 / 2",
                 "Avg Loss:", "[val epoch 1]", "[val epoch 2]", "[test] loss=", "[ckpt] saved ->"):
        assert word in out, word
    ckpts = sorted((tmp_path / "ckpt").glob("ViT-H-14_2_*.pt"))
    assert ckpts and method.checkpoint_path == ckpts[0]
    payload = torch.load(ckpts[0], map_location="cpu", weights_only=False)
    assert set(payload) == {"model_state", "epoch", "timestamp", "cfg", "clip_backend",
                            "open_clip_model", "optimizer_state", "scheduler_state"}
    assert payload["epoch"] == 2 and set(payload["model_state"]) == set(model.state_dict())
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(payload["model_state"][n]))
                            for n in method.trainer.names], lr=1e-3)
    opt.load_state_dict(payload["optimizer_state"])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 2)
    sched.load_state_dict(payload["scheduler_state"])
    assert sched.last_epoch == 2
    cache = tmp_path / "feat_cache_vis" / "ViT-H-14_cs" / "test" / "seed1"
    for f in ("embeddings.pt", "labels.pt", "metadata.csv", "meta.json"):
        assert (cache / f).is_file(), f
