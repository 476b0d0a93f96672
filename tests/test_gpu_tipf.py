"""GPU: Tip-Adapter-F training of the cache keys (csrc/tip_train.hip, miclip/tip.py) against
the float64 restatement tests/_tipf_ref.py, which test_tipf.py pins to torch.

Floats (the gradient of one step, the key update of a trajectory, the history's mean CE)
are held to a multiple of the float32 restatement's own error against float64 on the same
inputs (the larger of its closed and autograd forms): RATIO = 4, the bar the fine-tuning
tail uses for the same kind of fp32 reorder noise. Measured ratios on the MI355X are in
the docstrings of the tests. Counts may differ from float64 only on undecided rows
(_tip_ref.grid's rule); test_tipf.py asserts that the seeds used here have none, so the
training counts have to equal the float64 counts.

Outputs are written between NaN canaries, the scratch is followed by an 0xA5 guard, and
every figure is printed before it is asserted.
"""
import ctypes

import numpy as np
import pytest
import torch

import _tip_ref as R
import _tipf_ref as TF

pytestmark = pytest.mark.gpu

RATIO = 4.0
PAD = 64
DTYPES = {"fp32": torch.float32, "fp16": torch.float16}
CASE_IDS = range(len(TF.CASES))


def _lib():
    from miclip import _lib
    return _lib, _lib.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dt(t):
    L, _ = _lib()
    return {torch.float32: L.MICLIP_F32, torch.float16: L.MICLIP_FP16}[t.dtype]


class Guarded:
    """A float32 device buffer between two NaN canaries, optionally initialised."""

    def __init__(self, shape, init=None):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + 2 * PAD,), float("nan"), device="cuda")
        self.view = self.buf[PAD:PAD + self.numel].view(shape)
        if init is not None:
            self.view.copy_(torch.as_tensor(init, dtype=torch.float32).expand(shape))

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def numpy(self, name):
        assert bool(torch.isnan(self.buf[:PAD]).all()), f"wrote in front of {name}"
        assert bool(torch.isnan(self.buf[PAD + self.numel:]).all()), f"wrote past {name}"
        out = self.view.cpu().numpy()
        assert np.isfinite(out).all(), f"{name} not written everywhere"
        return out


def _clip_logits(F, W):
    """Z = 100 F W through miclip_tip_affinity, as fit_adapter_grid forms it."""
    L, lib = _lib()
    wt = torch.tensor(np.ascontiguousarray(np.asarray(W).T), dtype=torch.float32).cuda()
    z = torch.empty(F.shape[0], wt.shape[0], device="cuda")
    L.check(lib.miclip_tip_affinity(_p(F), _dt(F), _p(wt), F.shape[0], wt.shape[0], F.shape[1],
                                    100.0, _p(z), L.stream_handle()), "miclip_tip_affinity")
    return z


def dev_step(F, W, labels, key_labels, K0, configs, rows=None, *, lr_factor=1.0, step=1,
             wd=TF.WD, eps=TF.EPS):
    """One miclip_tipf_step from the keys K0 and zero moments; numpy results."""
    L, lib = _lib()
    Fd = F.cuda().contiguous()
    n, E = Fd.shape
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    b, G = len(rows), len(configs)
    K0 = torch.tensor(np.asarray(K0), dtype=torch.float32)
    Nk, C = K0.shape[0], np.asarray(W).shape[1]
    Z = _clip_logits(Fd, W)
    lab = torch.tensor(np.asarray(labels), dtype=torch.int32).cuda()
    klab = torch.tensor(np.asarray(key_labels), dtype=torch.int32).cuda()
    lr, beta, alpha = (torch.tensor([c[i] for c in configs], dtype=torch.float32).cuda()
                       for i in range(3))
    keys = Guarded((G, Nk, E), K0.unsqueeze(0).repeat(G, 1, 1))
    m, v = Guarded((G, Nk, E), 0.0), Guarded((G, Nk, E), 0.0)
    grad, hist = Guarded((G, Nk, E)), Guarded((G, 2))
    nbytes = int(lib.miclip_tipf_scratch_bytes(b, Nk, E, C, G))
    assert nbytes > 0 and nbytes % 256 == 0
    scratch = torch.full((nbytes + 256,), 0xA5, device="cuda", dtype=torch.uint8)
    assert scratch.data_ptr() % 256 == 0
    s = L.stream_handle()
    L.check(lib.miclip_tipf_prepare(_p(klab), Nk, C, _p(scratch), s), "miclip_tipf_prepare")
    L.check(lib.miclip_tipf_step(_p(Fd), _dt(Fd), n, rows.ctypes.data_as(ctypes.c_void_p), b,
                                 _p(lab), _p(Z), _p(klab), keys.ptr, m.ptr, v.ptr, _p(lr),
                                 _p(beta), _p(alpha), Nk, E, C, G, lr_factor, wd, eps, step,
                                 hist.ptr, grad.ptr, _p(scratch), s), "miclip_tipf_step")
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "wrote past the scratch"
    return {"keys": keys.numpy("keys"), "m": m.numpy("m"), "v": v.numpy("v"),
            "grad": grad.numpy("grad"), "history": hist.numpy("history")}


def _api_args(d, views, dname="fp32"):
    """(cache_keys [E, Nk], cache_values, clip_weights, train_views, train_labels) on the
    device, as the Python entry points take them."""
    C = d["W"].shape[1]
    values = torch.nn.functional.one_hot(torch.tensor(d["key_labels"]).long(), C).half().cuda()
    return (torch.tensor(d["K"]).t().contiguous().cuda(), values, torch.tensor(d["W"]).cuda(),
            [torch.as_tensor(x).to(DTYPES[dname]).cuda() for x in views],
            torch.tensor(d["labels"]).cuda())


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("idx", CASE_IDS, ids=TF.IDS)
def test_gradient_of_one_step(idx, G, dname):
    """dK of one step (grad_out) against float64: relative Frobenius error at most RATIO x
    the float32 restatement's own. At C = 1 the gradient is exactly zero on both sides.
    Measured on the MI355X (device error / float32 restatement's error, over G, the
    configurations and both input types): b1-k1 0.01-0.28, b15-k17 0.32-0.89, b17-k65
    0.65-1.05, b33-k130 0.67-1.15; device errors 5e-8 to 8e-7."""
    c = TF.step_case(idx, 1, dname)
    d, configs = c["d"], TF.CONFIGS[:G]
    out = dev_step(c["F"], d["W"], d["labels"], d["key_labels"], d["K"], configs)
    C = TF.CASES[idx][3]
    for g in range(G):
        ref = c["grad64"][g]
        if C == 1:
            print(f"{TF.IDS[idx]} {dname} config {g}: C = 1, largest |dK| {np.abs(out['grad'][g]).max()}")
            assert not ref.any() and not out["grad"][g].any()
            continue
        err, own = TF.rel(out["grad"][g], ref), c["err32"][g]
        print(f"{TF.IDS[idx]} {dname} G={G} config {g}: dK error {err:.3e}, float32 restatement "
              f"{own:.3e}, ratio {err / own if own else float('inf'):.2f} (bar {RATIO})")
        assert np.isfinite(err) and err <= RATIO * own
        # the history of the step: the batch's mean CE and correct count before the update
        l64 = torch.tensor(c["logits64"][g])
        ce = float(torch.nn.functional.cross_entropy(l64, c["y"]))
        assert abs(out["history"][g, 0] - ce) <= 1e-4 * max(1.0, abs(ce))
        assert int(out["history"][g, 1]) == int((l64.argmax(1) == c["y"]).sum())


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("idx", CASE_IDS, ids=TF.IDS)
def test_zero_force_step(idx, dname):
    """beta = 0 (configuration 0) and alpha = 0 (configuration 1): dK, m and v are exactly
    zero and the keys are K (1 - lr_t wd) within 2^-22 |K|: one rounding of the factor, fused
    or not, and one of the product."""
    c = TF.step_case(idx, 1, dname)
    d = c["d"]
    lr, lr_factor = 1e-3, 0.7
    out = dev_step(c["F"], d["W"], d["labels"], d["key_labels"], d["K"],
                   [(lr, 0.0, 1.17), (lr, 5.5, 0.0)], lr_factor=lr_factor, step=3)
    K = d["K"].astype(np.float64)
    want = K * (1 - np.float64(np.float32(lr)) * lr_factor * TF.WD)
    for g in range(2):
        dev = np.abs(out["keys"][g] - want)
        print(f"{TF.IDS[idx]} {dname} config {g}: largest |dK| {np.abs(out['grad'][g]).max()}, "
              f"|m| {np.abs(out['m'][g]).max()}, |v| {np.abs(out['v'][g]).max()}, keys off by "
              f"{(dev / np.maximum(np.abs(K), 1e-300)).max() / 2.0 ** -24:.2f} x 2^-24 |K|")
        assert not out["grad"][g].any() and not out["m"][g].any() and not out["v"][g].any()
        assert (dev <= 2.0 ** -22 * np.abs(K)).all()


def _fit(c, dname, configs, **kw):
    from miclip import tip
    d = c["d"]
    kw.setdefault("epochs", 2)
    kw.setdefault("batch_size", c["b"])
    return tip.fit_adapter_grid(*_api_args(d, [x.float().numpy() for x in c["views"]], dname),
                                [x[0] for x in configs], [x[1] for x in configs],
                                [x[2] for x in configs], weight_decay=TF.WD, eps=TF.EPS, **kw)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffled", "ordered"])
@pytest.mark.parametrize("seed", TF.SEEDS)
@pytest.mark.parametrize("idx", CASE_IDS, ids=TF.IDS)
def test_trajectory(idx, seed, shuffle, dname):
    """2 epochs x 3 steps on two views with a partial last batch, G = 3: the update
    keys - keys0 and the history's mean CE against float64 at most RATIO x the float32
    restatement's own error; the training counts equal the float64 counts except on
    undecided rows (none for these seeds). The update is held per configuration, the mean
    CE as the [steps, G] array the history is: one column of six batches of one row (b = 1)
    is too small a sample, the float32 restatement's error on it falls to 4e-9, a tenth
    of what storing a float32 costs, while the device's 5e-8 to 4e-7 is within an ulp of
    the logits. Measured on the MI355X (device / float32 restatement): update 0.88-1.02
    in all 120 (case, seed, order, type, configuration) entries (the rounding of the fp32
    keys themselves dominates both); CE history b1-k1 0.55-2.09, b15-k17 0.70-1.33,
    b17-k65 0.61-1.01, b33-k130 0.61-1.03, C = 1 exactly 0 on both sides; count
    differences 0 everywhere."""
    c = TF.trajectory_case(idx, seed, shuffle, dname)
    fit = _fit(c, dname, TF.CONFIGS, seed=seed, shuffle=shuffle)
    keys, hist = fit.keys.cpu().numpy(), fit.history.cpu().numpy()
    K0 = c["d"]["K"].astype(np.float64)
    assert hist.shape == (6, 3, 2) and fit.steps_per_epoch == 3
    # the history's mean CE, all [steps, G] of it in one norm
    ec, own = TF.rel(hist[:, :, 0], c["ce64"]), c["err_ce"]
    print(f"{TF.IDS[idx]} seed {seed} {dname}: CE history error {ec:.3e} (float32 {own:.3e}, "
          f"ratio {ec / own if own else 0:.2f}, bar {RATIO})")
    assert np.isfinite(ec) and ec <= RATIO * own
    for g, f in enumerate(c["fits"]):
        ref = f["f64"]
        ek = TF.rel(keys[g].astype(np.float64) - K0, ref["keys"][-1].numpy() - K0)
        eg = TF.rel(hist[:, g, 0], ref["ce"])
        diff = np.abs(hist[:, g, 1].astype(np.int64) - np.array(ref["correct"]))
        print(f"{TF.IDS[idx]} seed {seed} {dname} config {g}: update error {ek:.3e} (float32 "
              f"{f['err_keys']:.3e}, ratio {ek / f['err_keys'] if f['err_keys'] else 0:.2f}), its "
              f"own CE column {eg:.3e} (float32 {f['err_ce']:.3e}), count differences "
              f"{diff.tolist()}, undecided {f['undecided']}")
        assert np.isfinite(ek) and ek <= RATIO * f["err_keys"]
        assert (diff <= np.array(f["undecided"])).all()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) ==
                                                               b.view(torch.int32)).all())


@pytest.mark.parametrize("idx", CASE_IDS, ids=TF.IDS)
def test_independent_and_deterministic(idx):
    """A G = 3 fit equals three G = 1 fits bit for bit, and a second run equals the first."""
    c = TF.trajectory_case(idx, 1, True, "fp32")
    ev = dict(eval_features=c["views"][1].cuda(), eval_labels=torch.tensor(c["d"]["labels"]).cuda(),
              seed=1)
    whole, again = _fit(c, "fp32", TF.CONFIGS, **ev), _fit(c, "fp32", TF.CONFIGS, **ev)
    for name in ("keys", "best_keys", "history"):
        assert _same(getattr(whole, name), getattr(again, name)), name
    assert torch.equal(whole.eval_counts, again.eval_counts)
    for g, cfg in enumerate(TF.CONFIGS):
        one = _fit(c, "fp32", [cfg], **ev)
        assert _same(one.keys[0], whole.keys[g]) and _same(one.best_keys[0], whole.best_keys[g])
        assert _same(one.history[:, 0], whole.history[:, g])
        assert torch.equal(one.eval_counts[:, 0], whole.eval_counts[:, g])
        assert int(one.best_epoch[0]) == int(whole.best_epoch[g])


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("idx", CASE_IDS, ids=TF.IDS)
def test_row_map_is_a_gathered_copy(idx, dname):
    """A step through the row map equals the step on a gathered copy bit for bit, repeated
    rows included."""
    c = TF.trajectory_case(idx, 2, True, dname)
    d, n, b = c["d"], c["n"], c["b"]
    rng = np.random.default_rng(idx)
    rows = rng.integers(0, n, size=b)
    if b > 1:
        rows[-1] = rows[0]                      # a repeated row
    F = c["views"][0]
    a = dev_step(F, d["W"], d["labels"], d["key_labels"], d["K"], TF.CONFIGS, rows, step=2,
                 lr_factor=0.9)
    g = dev_step(F[torch.tensor(rows)], d["W"], d["labels"][rows], d["key_labels"], d["K"],
                 TF.CONFIGS, step=2, lr_factor=0.9)
    for name in ("keys", "m", "v", "grad", "history"):
        assert np.array_equal(a[name].view(np.int32), g[name].view(np.int32)), name


def _first_strict_max(col):
    best, at = 0, -1
    for e, cnt in enumerate(col):
        if cnt > best:
            best, at = cnt, e
    return best, at


@pytest.mark.parametrize("idx", CASE_IDS, ids=TF.IDS)
def test_best_epoch(idx):
    """eval_counts[e, g] is tip_accuracy_grid's count at that epoch's keys and the
    configuration's own pair; best_epoch is the first strict maximum from 0 and best_keys
    that epoch's keys bit for bit."""
    from miclip import tip
    c = TF.trajectory_case(idx, 1, True, "fp32")
    d = c["d"]
    ef, el = c["views"][1].cuda(), torch.tensor(d["labels"]).cuda()
    # large steps, so that the evaluation counts move from epoch to epoch
    configs = [(0.05, 1.0, 1.17), (0.1, 5.5, 1.0), (0.01, 3.0, 3.0)]
    fit = _fit(c, "fp32", configs, epochs=4, eval_features=ef, eval_labels=el, keep_epochs=True)
    keys0, values, W = _api_args(d, [d["F"]])[:3]
    counts = fit.eval_counts.cpu().numpy()
    assert counts.shape == (4, 3) and fit.epoch_keys.shape[:2] == (4, 3)
    assert _same(fit.epoch_keys[-1], fit.keys)
    for g, (_, beta, alpha) in enumerate(configs):
        for e in range(4):
            own = tip.tip_accuracy_grid(fit.epoch_keys[e, g].t(), values, ef, el, W, [beta],
                                        [alpha])[0]
            assert int(own[0, 0]) == counts[e, g], (e, g)
        best, at = _first_strict_max(counts[:, g].tolist())
        print(f"{TF.IDS[idx]} config {g}: evaluation counts {counts[:, g].tolist()} of {len(el)}, "
              f"best {int(fit.best_count[g])} at epoch {int(fit.best_epoch[g])}")
        assert (int(fit.best_count[g]), int(fit.best_epoch[g])) == (best, at)
        assert _same(fit.best_keys[g], fit.epoch_keys[at, g] if at >= 0 else keys0.t().contiguous())


def test_best_epoch_when_nothing_beats_zero():
    """Evaluation labels that no row can match: class 19 owns no key and has zero text
    weights, so its logit is exactly 0, while class 0 (zero text weights, some keys) has
    alpha S > 0 on every row. best_epoch stays -1 and best_keys the initial keys."""
    c = TF.trajectory_case(2, 1, True, "fp32")
    d = dict(c["d"])
    d["W"] = d["W"].copy()
    d["W"][:, [0, 19]] = 0
    assert (d["key_labels"] == 0).any() and not (d["key_labels"] == 19).any()
    ef = c["views"][1].cuda()
    el = torch.full((ef.shape[0],), 19, dtype=torch.int64).cuda()
    fit = _fit(dict(c, d=d), "fp32", TF.CONFIGS, epochs=3, eval_features=ef, eval_labels=el)
    print(f"evaluation counts {fit.eval_counts.cpu().tolist()}")
    assert not fit.eval_counts.any() and not fit.best_count.any()
    assert fit.best_epoch.cpu().tolist() == [-1, -1, -1]
    k0 = torch.tensor(d["K"]).cuda()
    for g in range(3):
        assert _same(fit.best_keys[g], k0) and not _same(fit.keys[g], k0)


CFG = {"search_hp": True, "search_scale": [7, 3], "search_step": [5, 4]}


def test_trained_keys_plug_into_the_search(capsys):
    """search_hp_tip on best_keys as built-in cache keys against the same search through
    the nn.Linear adapter of fit_adapter (the allowance of test_adapter_affinity: the count
    grids may differ on undecided rows only), and tip_adapter_f end to end."""
    from miclip import tip
    c = TF.trajectory_case(3, 1, True, "fp32")
    d = c["d"]
    keys, values, W, views, labels = _api_args(d, [x.numpy() for x in c["views"]])
    ef, el = views[1], labels
    lr, beta, alpha = 0.01, 1.0, 1.17
    adapter = tip.fit_adapter(keys, values, W, views, labels, lr, beta, alpha, epochs=3,
                              batch_size=c["b"], eval_features=ef, eval_labels=el)
    fit = adapter.fit
    assert isinstance(adapter, torch.nn.Linear) and adapter.bias is None
    assert _same(adapter.weight.detach(), fit.best_keys[0])
    best = fit.best_keys[0].t()
    betas, alphas = tip.beta_alpha_lists(CFG)
    own = tip.tip_accuracy_grid(best, values, ef, el, W, betas, alphas)[0].cpu().numpy()
    sup = tip.tip_accuracy_grid(keys, values, ef, el, W, betas, alphas,
                                adapter=adapter)[0].cpu().numpy()
    r = R.grid(ef.cpu().numpy(), fit.best_keys[0].cpu().numpy(), d["key_labels"], d["W"],
               d["labels"], betas, alphas)
    print(f"largest count difference adapter / built-in {np.abs(own - sup).max()}, undecided up "
          f"to {r['undecided'].max()}")
    assert (np.abs(own - sup) <= r["undecided"]).all()
    assert (np.abs(own - r["counts"]) <= r["undecided"]).all()
    pair_own = tip.search_hp_tip(CFG, best, values, ef, el, W)
    pair_sup = tip.search_hp_tip(CFG, keys, values, ef, el, W, adapter=adapter)
    assert pair_own[0] in betas and pair_own[1] in alphas
    if np.array_equal(own, sup):
        assert pair_own == pair_sup
    capsys.readouterr()

    cfg = dict(CFG, tip_f={"lr": lr, "train_epoch": 3, "init_beta": beta, "init_alpha": alpha,
                           "batch_size": c["b"]})
    ad2, bb, ba, fit2 = tip.tip_adapter_f(cfg, keys, values, views, labels, ef, el, W)
    text = capsys.readouterr().out
    print(text)
    assert bb in betas and ba in alphas and (bb, ba) == pair_own
    assert _same(fit2.best_keys, fit.best_keys) and _same(ad2.weight.detach(), fit.best_keys[0])
    assert text.count("Train Epoch:") == 3 and text.count("LR: ") == 3
    assert text.count("test accuracy") == 4 and "After searching" in text
