"""GPU: the validation-metrics kernel (csrc/evaluate.hip) and miclip.evaluation.

What is compared with what:
  * logits: bit for bit with miclip_zero_shot(apply_proj = 0) (the head the kernel
    restates); fp16 / bf16 features against the call on the widened fp32 copy;
  * every integer result (predictions, top-3, hit counts, confusion counts, L2
    predictions) exactly against tests/_eval_ref.py (numpy) on the kernel's OWN
    logits, so no fp32-vs-fp64 logit difference can flip one;
  * every floating result against fp64 on the kernel's own logits, with the bars
    below;
  * the whole path against the reference's recorded run, tests/golden/evaluation.npz
    (scripts/make_golden_eval.py), whose rows all have top-k gaps >= 1e-3.

Bars. The issue derives a worst-case absolute cross-entropy error below 1e-4 (a row's
exponent sum has at most 1024 terms rounded at 2^-23 each, the final max + log at
magnitudes <= 128) and asks for 4 x the measured maximum, never above 1e-4. Measured on
the MI355X over the cases of this file (every test prints its figures before it
asserts): row CE 2.05e-6, top-3 probabilities 2.01e-7, batch-mean loss 2.34e-6, L2
`mean` logits 7.3e-7, L2 `logsumexp` logits 3.9e-6.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _eval_ref as R

pytestmark = pytest.mark.gpu

SCALE = 100.0
CE_TOL = 4 * 2.05e-6
PROB_TOL = 4 * 2.01e-7
MEAN_LOSS_TOL = 4 * 2.34e-6
L2_MEAN_TOL = 4 * 7.3e-7
L2_LSE_TOL = 4 * 3.9e-6
assert max(CE_TOL, PROB_TOL, MEAN_LOSS_TOL, L2_MEAN_TOL, L2_LSE_TOL) <= 1e-4

SHAPES = [(1, 16, 3), (15, 64, 17), (17, 512, 20), (33, 768, 1000), (16, 1024, 1024)]
CASES = [f"{b}x{e}x{c}" for b, e, c in SHAPES] + ["ties", "absent"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ------------------------------------------------------------------ inputs (CPU)
@functools.lru_cache(maxsize=None)
def _case(name):
    """(feats [B, E] fp32 on the grid k / 64 -- exact in fp16 and bf16 --, text_weights
    [E, C], labels [B])."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "ties":
        B, E, C = 21, 32, 12
    elif name == "absent":
        B, E, C = 40, 48, 6
    else:
        B, E, C = (int(v) for v in name.split("x"))
    W = torch.nn.functional.normalize(torch.randn(E, C, generator=g), dim=0)
    y = torch.randint(0, C, (B,), generator=g)
    if name == "ties":
        W[:, 1] = W[:, 0]          # bitwise-tied logits in places 1-2 ...
        W[:, 3] = W[:, 2]          # ... and 3-4 for rows built from columns 0 and 2
        y = torch.randint(0, 4, (B,), generator=g)
        raw = 2.0 * W[:, 0][None] + 1.0 * W[:, 2][None] + 0.05 * torch.randn(B, E, generator=g)
        raw[B // 2:] = 1.0 * W[:, 0][None] + 2.0 * W[:, 2][None] + 0.05 * torch.randn(
            B - B // 2, E, generator=g)
    elif name == "absent":
        W[:, 4] = 0.0              # class 4: logit 0 under a positive maximum, never predicted
        y = torch.randint(0, 5, (B,), generator=g)   # class 5 absent from the labels
        y[:3] = 4
        raw = 1.5 * W[:, y.clamp(max=3)].t() + 0.2 * torch.randn(B, E, generator=g)
    else:
        raw = 1.5 * W[:, y].t() + 0.6 * torch.randn(B, E, generator=g)
    f = (64.0 * raw).round().clamp(-255, 255) / 64.0
    if name == "17x512x20":        # planted: logit +100 on class 3 and -100 on class 7
        W[:, 7] = -W[:, 3]
        f[5] = 3.0 * W[:, 3]
        f[6] = 3.0 * W[:, 3]
        y[5], y[6] = 3, 7          # CE ~ 0 and CE ~ 200: exp overflows without the max
    return f.contiguous(), W.contiguous(), y


def _grid_ok(f):
    return all(torch.equal(f.to(dt).float(), f) for dt in (torch.float16, torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _run(name, dtype="fp32", mode=None, reduce="mean", map_name=None, batch=0):
    """One evaluation of a case on the device; everything comes back as numpy."""
    from miclip.evaluation import Evaluator
    f, W, y = _case(name)
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    ctx = None
    if mode is not None:
        m, num_l2 = _map(map_name, W.shape[1])
        ctx = {"l3_to_l2": m, "num_l2": num_l2, "mode": mode, "reduce": reduce, "topk": (1, 3),
               "return_confusion_matrix": True}
    ev = Evaluator(W, scale=SCALE, l2_eval_ctx=ctx, device="cuda")
    n, outs = f.shape[0], []
    for i0 in range(0, n, batch or n):
        i1 = min(i0 + (batch or n), n)
        outs.append(ev.update(f[i0:i1].to(dt), y[i0:i1], rows=True, want_logits=True,
                              want_l2_logits=True))
    res = {k: torch.cat([o[k] for o in outs]).cpu().numpy() for k in outs[0]}
    res["batch_rows"] = [int(o["row_loss"].shape[0]) for o in outs]
    res["counts"] = ev.counts()
    res["tuple"] = ev.compute(return_confusion_matrix=True)
    return res


@functools.lru_cache(maxsize=None)
def _map(map_name, C):
    """(l3_to_l2 tuple, num_l2)."""
    if map_name == "real":
        g = R.load_golden()
        assert C == 20
        return tuple(int(v) for v in g["l3_to_l2"]), int(g["meta"]["num_l2"])
    if map_name == "empty_group":       # group 2 of 5 has no L3 class
        return tuple((0, 1, 3, 4)[c % 4] for c in range(C)), 5
    if map_name == "one":
        return tuple(0 for _ in range(C)), 1
    if map_name == "random37":
        rng = np.random.default_rng(C)
        return tuple(int(v) for v in rng.integers(0, 37, C)), 37
    if map_name == "perm":              # num_l2 = C: the largest LDS footprint
        rng = np.random.default_rng(C + 1)
        return tuple(int(v) for v in rng.permutation(C)), C
    raise KeyError(map_name)


def _zero_shot(f32, W):
    """miclip_zero_shot(apply_proj = 0) on a bare handle whose embed_dim is E (the head
    reads nothing else of the model)."""
    from miclip import _lib
    lib = _lib.load_library()
    E, C = W.shape
    cfg = _lib.MiclipConfig(embed_dim=E, image_resolution=32, vision_layers=1, vision_width=256,
                            vision_patch_size=32, context_length=8, vocab_size=16,
                            transformer_width=256, transformer_heads=4, transformer_layers=0,
                            compute_dtype=_lib.MICLIP_FP16, act=_lib.MICLIP_ACT_QUICKGELU,
                            vision_head_dim=64, options=0)
    h = ctypes.c_void_p()
    _lib.check(lib.miclip_model_create(ctypes.byref(cfg), 0, ctypes.byref(h)), "create")
    try:
        fd, wd = f32.cuda().contiguous(), W.cuda().contiguous()
        logits = torch.empty(fd.shape[0], C, device="cuda")
        _lib.check(lib.miclip_zero_shot(h, fd.data_ptr(), fd.shape[0], 0, wd.data_ptr(), C, SCALE,
                                        logits.data_ptr(), None, 0, _lib.stream_handle()),
                   "miclip_zero_shot")
        return logits.cpu().numpy()
    finally:
        lib.miclip_model_destroy(h)


# ------------------------------------------------------------------ 1. logits, bit for bit
@pytest.mark.parametrize("name", CASES)
def test_logits_bit_exact_with_zero_shot(name):
    f, W, _ = _case(name)
    assert _grid_ok(f) or name == "17x512x20"   # the planted rows are off the grid
    _need_gpu()
    want = _zero_shot(f, W)
    got = _run(name)["logits"]
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for dtype, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        wide = f.to(dt).float()
        want16 = want if torch.equal(wide, f) else _zero_shot(wide, W)
        got16 = _run(name, dtype)["logits"]
        assert np.array_equal(got16.view(np.uint32), want16.view(np.uint32)), dtype


# ------------------------------------------------------------------ 2. integer results
@pytest.mark.parametrize("name", CASES)
def test_integer_results_exact(name):
    _need_gpu()
    _, W, y = _case(name)
    y, C = y.numpy(), W.shape[1]
    r = _run(name)
    z = r["logits"]
    top3 = R.topk(z, 3)
    if name == "ties":      # the precondition: bitwise ties in places 1-2 and 3-4
        s = -np.sort(-z, axis=1)
        assert (s[:, 0] == s[:, 1]).any() and (s[:, 2] == s[:, 3]).any()
        assert ((s[:, 0] == s[:, 1]) & (s[:, 2] == s[:, 3])).any()
    assert np.array_equal(r["top3"], top3)
    assert np.array_equal(r["pred"], top3[:, 0])
    c = r["counts"]
    cm = R.confusion(y, top3[:, 0], C)
    if name == "absent":
        assert cm[5].sum() == 0 and cm[4].sum() > 0 and cm[:, 4].sum() == 0
    assert np.array_equal(c.cm, cm)
    assert (c.rows, c.batches, c.skipped) == (len(y), 1, 0)
    assert c.top1 == R.hits(z, y, 1) and c.top3 == R.hits(z, y, 3)
    t = r["tuple"]
    assert t[1] == c.top1 / len(y) and t[2] == c.top3 / len(y)
    assert abs(t[3] - R.weighted_f1(cm)) <= 1e-12
    assert np.array_equal(t[5], cm) and t[6] is None


# ------------------------------------------------------------------ 3. floating results
@pytest.mark.parametrize("name", CASES)
def test_float_results_against_fp64(name):
    _need_gpu()
    _, _, y = _case(name)
    y = y.numpy()
    r = _run(name)
    z = r["logits"]
    if name == "17x512x20":
        assert abs(z[5, 3] - 100.0) < 1e-3 and abs(z[5, 7] + 100.0) < 1e-3
        with np.errstate(over="ignore"):
            assert not np.isfinite(np.exp(z.astype(np.float32))).all()   # fp32 exp overflows
    ce = R.row_ce(z, y)
    idx, probs = R.top3_probs(z)
    e_ce = float(np.abs(r["row_loss"] - ce).max())
    e_p = float(np.abs(r["top3_prob"] - probs).max())
    e_m = abs(r["tuple"][0] - ce.mean())
    print(f"{name}: row CE err {e_ce:.3g} (bar {CE_TOL:.3g}), top-3 prob err {e_p:.3g} "
          f"(bar {PROB_TOL:.3g}), batch-mean loss err {e_m:.3g} (bar {MEAN_LOSS_TOL:.3g}); "
          f"max CE {ce.max():.4g}")
    assert np.isfinite(r["row_loss"]).all()
    assert e_ce <= CE_TOL and e_p <= PROB_TOL and e_m <= MEAN_LOSS_TOL


# ------------------------------------------------------------------ 4. L2 roll-up
L2_CASES = [("17x512x20", "real"), ("17x512x20", "empty_group"), ("17x512x20", "one"),
            ("15x64x17", "empty_group"), ("33x768x1000", "random37"), ("16x1024x1024", "perm")]


@pytest.mark.parametrize("name,map_name", L2_CASES)
@pytest.mark.parametrize("reduce", ["sum", "mean", "logsumexp"])
def test_l2_rollup_logits_mode(name, map_name, reduce):
    _need_gpu()
    _, W, y = _case(name)
    y, C = y.numpy(), W.shape[1]
    m, num_l2 = _map(map_name, C)
    r = _run(name, mode="logits", reduce=reduce, map_name=map_name)
    z, z2 = r["logits"], r["l2_logits"]
    assert z2.shape == (len(y), num_l2)
    assert np.array_equal(z.view(np.uint32), _run(name)["logits"].view(np.uint32))
    if reduce == "sum":     # bitwise: a torch-CPU fp32 loop in ascending L3 id
        want = torch.zeros(len(y), num_l2)
        zt = torch.from_numpy(z)
        for l3, l2 in enumerate(m):
            want[:, l2] += zt[:, l3]
        assert np.array_equal(z2.view(np.uint32), want.numpy().view(np.uint32))
    else:
        want = R.aggregate(z, m, num_l2, reduce)
        fin = np.isfinite(want)
        assert np.array_equal(np.isneginf(z2), np.isneginf(want))   # empty groups: -inf
        err = float(np.abs(z2[fin] - want[fin]).max())
        bar = L2_MEAN_TOL if reduce == "mean" else L2_LSE_TOL
        print(f"{name}/{map_name}/{reduce}: L2 logits err {err:.3g} (bar {bar:.3g})")
        assert err <= bar
    # integer results on the kernel's own L2 logits
    y2 = np.asarray(m)[y]
    top = R.topk(z2, min(3, num_l2))
    want_top3 = np.full((len(y), 3), -1, dtype=np.int32)
    want_top3[:, :top.shape[1]] = top
    assert np.array_equal(r["l2_top3"], want_top3)
    assert np.array_equal(r["l2_pred"], top[:, 0])
    c = r["counts"]
    assert c.l2_top1 == R.hits(z2, y2, 1) and c.l2_top3 == R.hits(z2, y2, 3)
    cm2 = R.confusion(y2, top[:, 0], num_l2)
    assert np.array_equal(c.cm_l2, cm2)
    l2m = r["tuple"][6]
    assert l2m["top1"] == c.l2_top1 / len(y) and l2m["top3"] == c.l2_top3 / len(y)
    assert abs(l2m["f1"] - R.weighted_f1(cm2)) <= 1e-12 and np.array_equal(l2m["cm"], cm2)


@pytest.mark.parametrize("name,map_name", L2_CASES)
def test_l2_rollup_argmax_mode(name, map_name):
    _need_gpu()
    _, W, y = _case(name)
    y, C = y.numpy(), W.shape[1]
    m, num_l2 = _map(map_name, C)
    r = _run(name, mode="argmax", map_name=map_name)
    pred2, y2 = np.asarray(m)[R.topk(r["logits"], 1)[:, 0]], np.asarray(m)[y]
    assert np.array_equal(r["l2_pred"], pred2)
    assert np.array_equal(r["l2_top3"][:, 0], pred2) and (r["l2_top3"][:, 1:] == -1).all()
    c = r["counts"]
    assert c.l2_top1 == int((pred2 == y2).sum())
    assert np.array_equal(c.cm_l2, R.confusion(y2, pred2, num_l2))
    l2m = r["tuple"][6]
    assert set(l2m) == {"top1", "f1", "mcc", "cm"} and l2m["top1"] == c.l2_top1 / len(y)


def test_aggregate_logits_to_l2_and_accumulator_on_logits():
    """The two reference-named entry points on ready logits (device tensors)."""
    _need_gpu()
    from miclip.evaluation import L2MetricsAccumulator, aggregate_logits_to_l2
    name, map_name = "17x512x20", "real"
    _, W, y = _case(name)
    m, num_l2 = _map(map_name, W.shape[1])
    z = torch.from_numpy(_run(name)["logits"]).cuda()
    for reduce in ("sum", "mean", "logsumexp"):
        got = aggregate_logits_to_l2(z, list(m), num_l2, reduce=reduce)
        assert got.is_cuda and got.shape == (len(y), num_l2)
        want = _run(name, mode="logits", reduce=reduce, map_name=map_name)["l2_logits"]
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        acc = L2MetricsAccumulator(torch.tensor(m), num_l2, reduce=reduce, mode="logits",
                                   return_confusion_matrix=True)
        acc.update(z[:9], y[:9])
        acc.update(z[:0], y[:0])          # the empty batch changes nothing
        acc.update(z[9:], y[9:].cuda())
        got_m = acc.compute()
        want_m = _run(name, mode="logits", reduce=reduce, map_name=map_name)["tuple"][6]
        assert acc.total_seen == len(y)
        assert {k: v for k, v in got_m.items() if k != "cm"} == \
            {k: v for k, v in want_m.items() if k != "cm"}
        assert np.array_equal(got_m["cm"], want_m["cm"])


# ------------------------------------------------------------------ 5. batch split
def test_batch_split_invariance_and_determinism():
    _need_gpu()
    from miclip.evaluation import Evaluator
    g = torch.Generator().manual_seed(50)
    W = torch.nn.functional.normalize(torch.randn(64, 20, generator=g), dim=0)
    y = torch.randint(0, 20, (50,), generator=g)
    f = 1.5 * W[:, y].t() + 0.6 * torch.randn(50, 64, generator=g)
    m, num_l2 = _map("real", 20)
    ctx = {"l3_to_l2": m, "num_l2": num_l2, "mode": "logits", "reduce": "logsumexp"}

    def go(bs):
        ev = Evaluator(W, l2_eval_ctx=ctx, device="cuda")
        outs = [ev.update(f[i:i + bs], y[i:i + bs], rows=True, want_logits=True,
                          want_l2_logits=True) for i in range(0, 50, bs)]
        rows = {k: torch.cat([o[k] for o in outs]).cpu().numpy() for k in outs[0]}
        return rows, ev.counts(), [int(o["row_loss"].shape[0]) for o in outs]

    one, c1, _ = go(50)
    split, c4, sizes = go(16)
    again, c4b, _ = go(16)
    assert sizes == [16, 16, 16, 2]
    for k in one:           # per-row outputs: bit for bit, whatever the batching
        assert np.array_equal(one[k].view(np.uint32), split[k].view(np.uint32)), k
        assert np.array_equal(split[k].view(np.uint32), again[k].view(np.uint32)), k
    for a, b in ((c1, c4), (c4, c4b)):
        assert (a.rows, a.top1, a.top3, a.l2_top1, a.l2_top3, a.skipped) == \
            (b.rows, b.top1, b.top3, b.l2_top1, b.l2_top3, b.skipped)
        assert np.array_equal(a.cm, b.cm) and np.array_equal(a.cm_l2, b.cm_l2)
    assert (c1.batches, c4.batches) == (1, 4)
    assert c4.loss_sum == c4b.loss_sum      # two runs: bitwise the same loss
    # avg_loss = the mean of the per-batch means (PEFT_openclip.py:99, 119), in each case
    ce = one["row_loss"].astype(np.float64)
    for c, sz in ((c1, [50]), (c4, sizes)):
        edges = np.cumsum([0] + sz)
        want = np.mean([ce[a:b].mean() for a, b in zip(edges[:-1], edges[1:])])
        err = abs(c.loss_sum / c.batches - want)
        print(f"batches {sz}: avg_loss err {err:.3g} (bar {MEAN_LOSS_TOL:.3g})")
        assert err <= MEAN_LOSS_TOL


# ------------------------------------------------------------------ 6. the reference's run
class _Stub(torch.nn.Module):
    def encode_image(self, images):
        return images


def _golden_loader(g, with_meta=True):
    f, y = torch.from_numpy(g["feats"]), torch.from_numpy(g["labels"])
    bs, out = g["meta"]["batch"], []
    for i in range(0, len(y), bs):
        md = {k: list(g[f"meta_{k}"][i:i + bs]) for k in ("file_name", "plot_word_label",
                                                          "image_source")}
        out.append((f[i:i + bs], y[i:i + bs], md) if with_meta else (f[i:i + bs], y[i:i + bs]))
    return out


@pytest.mark.parametrize("run", ["argmax_mean", "logits_sum", "logits_mean", "logits_logsumexp"])
def test_run_validation_reproduces_the_reference(run):
    from sklearn.metrics import f1_score, matthews_corrcoef
    g = R.load_golden()
    assert g["meta"]["min_gap"] >= 1e-3 and run in g["meta"]["runs"]
    _need_gpu()
    from miclip.evaluation import ClassificationTracker, Evaluator, run_validation
    mode, reduce = run.split("_")
    tracker = ClassificationTracker()
    W, y = torch.from_numpy(g["text_weights"]), g["labels"]
    l3_to_l2, num_l2 = [int(v) for v in g["l3_to_l2"]], g["meta"]["num_l2"]
    ctx = {"l3_to_l2": l3_to_l2, "num_l2": num_l2, "reduce": reduce, "topk": (1, 3),
           "mode": mode, "return_confusion_matrix": True}
    with_meta = run != "logits_sum"         # both batch forms
    loss, top1, top3, f1, mcc, cm, l2m = run_validation(
        _Stub(), _golden_loader(g, with_meta), W, "cuda", return_confusion_matrix=True,
        cls_track=tracker if with_meta else False, l2_eval_ctx=ctx,
        class_names=list(g["class_names"]))
    ev = Evaluator(W, device="cuda")
    rows = ev.update(torch.from_numpy(g["feats"]), torch.from_numpy(y), rows=True, want_logits=True)
    preds = rows["pred"].cpu().numpy()
    dz = float(np.abs(rows["logits"].cpu().numpy().astype(np.float64) - g["logits"]).max())
    ref = dict(zip(g["meta"]["scalars"], g[f"{run}_scalars"]))
    # the reference's loss is fp32 CE on ITS fp32 logits: both CEs carry the measured CE
    # error, and CE moves by at most 2 max|dz| when the logits move by dz
    bar = 2 * CE_TOL + 2 * dz
    print(f"{run}: loss {loss:.7f} vs {ref['loss']:.7f}, max logit diff {dz:.3g}, bar {bar:.3g}")
    assert abs(loss - ref["loss"]) <= bar
    assert np.array_equal(preds, g["preds"])
    assert np.array_equal(rows["top3"].cpu().numpy(), g["top3"])
    assert abs(top1 - ref["top1"]) <= 1e-12 and abs(top3 - ref["top3"]) <= 1e-12
    assert abs(mcc - ref["mcc"]) <= 1e-12
    assert abs(mcc - matthews_corrcoef(y, preds)) <= 1e-12
    assert abs(f1 - f1_score(y, preds, average="weighted", zero_division=0)) <= 1e-12
    assert np.array_equal(cm, R.confusion(y, preds, W.shape[1]))
    ref2 = dict(zip(g["meta"]["l2_scalars"], g[f"{run}_l2_scalars"]))
    assert abs(l2m["top1"] - ref2["top1"]) <= 1e-12 and abs(l2m["mcc"] - ref2["mcc"]) <= 1e-12
    if mode == "logits":
        assert abs(l2m["top3"] - ref2["top3"]) <= 1e-12
    else:
        assert "top3" not in l2m
    y2 = np.asarray(l3_to_l2)[y]
    cm2 = l2m["cm"]
    assert cm2.sum() == len(y) and np.array_equal(cm2.sum(axis=1), np.bincount(y2, minlength=num_l2))
    yt, yp = R.pairs_from_confusion(cm2)
    assert abs(l2m["f1"] - f1_score(yt, yp, average="weighted", zero_division=0)) <= 1e-12
    # evaluate_features: the same evaluation over the cached features, bit for bit
    from miclip.evaluation import evaluate_features
    tracker2 = ClassificationTracker(list(g["class_names"]))
    md = {k: list(g[f"meta_{k}"]) for k in ("file_name", "plot_word_label", "image_source")}
    again = evaluate_features(torch.from_numpy(g["feats"]), torch.from_numpy(y), W,
                              batch_size=g["meta"]["batch"], return_confusion_matrix=True,
                              cls_track=tracker2, l2_eval_ctx=ctx, metadata=md, device="cuda")
    assert again[:5] == (loss, top1, top3, f1, mcc) and np.array_equal(again[5], cm)
    assert {k: v for k, v in again[6].items() if k != "cm"} == \
        {k: v for k, v in l2m.items() if k != "cm"}
    if not with_meta:
        return
    for a, b in zip(tracker.frames(), tracker2.frames()):
        assert a.equals(b)
    # the ClassificationTracker tables: the reference's columns, row split, labels
    mis, cor = tracker.frames()
    for df, tag in ((mis, "mis"), (cor, "cor")):
        assert list(df.columns) == list(g[f"track_{tag}_columns"])
        assert len(df) == len(g[f"track_{tag}__file_name"])
        for col in df.columns:
            want = g[f"track_{tag}__{col}"]
            if col.startswith("top3_prob_"):
                err = float(np.abs(df[col].to_numpy(dtype=np.float64) - want).max())
                # softmax moves by at most 2 max|dz| (relative) with the logits
                assert err <= 2 * PROB_TOL + 2 * dz, (col, err)
            elif want.dtype.kind in "iu":
                assert np.array_equal(df[col].to_numpy(dtype=np.int64), want), col
            else:
                assert list(df[col].astype(str)) == list(want.astype(str)), col


# ------------------------------------------------------------------ 7. validation errors
def test_validation_errors_raise_before_any_launch():
    _need_gpu()
    from miclip import _lib
    from miclip.evaluation import Evaluator, aggregate_logits_to_l2, run_validation
    g = torch.Generator().manual_seed(7)

    def tw(E, C):
        return torch.randn(E, C, generator=g)
    with pytest.raises(ValueError):
        Evaluator(tw(32, 2), device="cuda")                     # C = 2
    with pytest.raises(ValueError):
        Evaluator(tw(24, 5), device="cuda")                     # E = 24
    with pytest.raises(ValueError):
        Evaluator(tw(1040, 5), device="cuda")                   # E = 1040
    ev = Evaluator(tw(32, 5), device="cuda")
    f = torch.randn(4, 32, generator=g)
    with pytest.raises(ValueError):
        ev.update(f, torch.tensor([0, 1, 5, 2]))                # a label equal to C
    with pytest.raises(TypeError):
        ev.update(f, torch.tensor([0.0, 1.0, 2.0, 3.0]))        # float labels
    with pytest.raises(ValueError):
        Evaluator(tw(32, 5), device="cuda",
                  l2_eval_ctx={"l3_to_l2": [0, 1, 2, 1, 0], "num_l2": 2})   # entry == num_l2
    with pytest.raises(ValueError, match="logits_l3 has 5 classes, but l3_to_l2 has 4 entries."):
        aggregate_logits_to_l2(torch.randn(3, 5, device="cuda"), [0, 1, 1, 0], 2)
    with pytest.raises(ValueError, match="logits_l3 has 5 classes, but l3_to_l2 has 4 entries."):
        Evaluator(tw(32, 5), device="cuda", l2_eval_ctx={"l3_to_l2": [0, 1, 1, 0], "num_l2": 2})
    with pytest.raises(ValueError, match="Expected batch to be"):
        run_validation(_Stub(), [(f, torch.zeros(4, dtype=torch.long), None, None)], tw(32, 5), "cuda")
    assert ev.counts().batches == 0 and ev.counts().rows == 0   # nothing ran
    # the C entry point itself: every limit is MICLIP_EINVAL before any launch
    lib = _lib.load_library()
    fd, wd = torch.zeros(4, 1040, device="cuda"), torch.zeros(1040 * 8, device="cuda")
    yd = torch.zeros(4, dtype=torch.int64, device="cuda")
    loss = torch.full((4,), -7.0, device="cuda")
    state = torch.zeros(int(lib.miclip_eval_state_bytes(5, 2)) // 8, dtype=torch.int64, device="cuda")
    bad_map = (ctypes.c_int32 * 5)(0, 1, 2, 1, 0)
    ok_map = (ctypes.c_int32 * 5)(0, 1, 1, 1, 0)

    def call(E=32, C=5, B=4, m=None, num_l2=1, mode=0):
        return lib.miclip_eval_batch(fd.data_ptr(), _lib.MICLIP_F32, wd.data_ptr(), yd.data_ptr(),
                                     B, E, C, 100.0, m, num_l2, mode, 0, state.data_ptr(), None,
                                     loss.data_ptr(), None, None, None, None, None, None,
                                     _lib.stream_handle())
    for kw in (dict(C=2), dict(E=24), dict(E=1040), dict(E=8), dict(C=1025), dict(B=0),
               dict(m=bad_map, num_l2=2, mode=2), dict(m=ok_map, num_l2=6, mode=2),
               dict(m=ok_map, num_l2=0, mode=2), dict(m=None, num_l2=2, mode=2)):
        assert call(**kw) == -1, kw
    assert lib.miclip_eval_state_bytes(2, 1) == 0 and lib.miclip_eval_state_bytes(5, 6) == 0
    torch.cuda.synchronize()
    assert (loss == -7.0).all() and int(state.abs().sum()) == 0
    assert call(m=ok_map, num_l2=2, mode=2) == 0                # and the good call runs
    torch.cuda.synchronize()
    assert int(state[2]) == 1 and (loss != -7.0).all()
