"""GPU: the Tip-Adapter cache classifier on the device (csrc/tip.hip, miclip/tip.py) against
the float64 restatement tests/_tip_ref.py, which test_tip.py pins to the reference.

Floats (keys, affinity, CLIP logits, Tip logits) follow the rule of test_gpu_tsne.py: the
allowed error is the larger of 8 x the error of the float32 restatement against float64 on
the same inputs and 16 * 2^-24 of the largest magnitude.

Counts: a row is undecided at a (beta, alpha) pair when its float64 top-2 margin is at
most 8 x the float32 restatement's largest logit error at that pair; the device count must
lie within the float64 count +- the number of undecided rows at that pair. Undecided
(row, pair) entries may be at most 1 % of all entries of a case. Measured on the CPU for
the seeds used here (float32 against float64 restatement alone): 0 undecided entries in
every case and every input type (largest share 0 %), so on these inputs the device counts
have to equal the float64 counts.

Outputs are written between NaN / sentinel canaries, the scratch is followed by an 0xA5
guard, and every figure is printed before it is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _tip_ref as R

pytestmark = pytest.mark.gpu

# (Nq, Nk, E, C, nb, na, planted() extras)
SHAPES = [(1, 1, 16, 1, 1, 1, {}),
          (3, 5, 16, 3, 2, 2, {}),
          (65, 43, 48, 5, 7, 3, {}),
          (300, 257, 512, 20, 5, 4, {"empty_class": 19}),     # one class owns no key
          (17, 1030, 768, 20, 3, 3, {}),
          (4, 320, 1024, 20, 200, 20, {}),                    # the full grid on few rows
          (33, 40, 32, 4, 3, 3, {"equal": True}),             # affinity 1, exp(0) = 1
          (20, 64, 64, 6, 4, 2, {"dup": 8}),                  # 8 duplicated keys
          (2, 4200, 16, 7, 2, 2, {}),                         # two staging tiles of sorted keys
          (40, 700, 64, 600, 3, 2, {"noise": 1.0}),           # C > 512: one beta per workgroup
          (30, 40, 16, 20, 30, 3, {"noise": 1.0})]            # 25 betas per workgroup, a tail of 5
IDS = ["q{}-k{}-E{}-C{}-{}x{}".format(*s[:6]) for s in SHAPES]
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SCALE = [7, 30]
PAD = 64
U = 2.0 ** -24
SENTINEL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def case(idx, dname):
    """Inputs (F rounded to the input type) and yardstick values, computed once."""
    Nq, Nk, E, C, nb, na, extra = SHAPES[idx]
    d = R.planted(Nq, Nk, E, C, seed=1000 + idx, **extra)
    F = torch.tensor(d["F"]).to(DTYPES[dname])
    if extra.get("equal"):
        d["K"][0] = F[0].float().numpy()      # the key is the rounded query, bit for bit
    betas, alphas = R.lists(SCALE, [nb, na])
    r = R.grid(F.float(), d["K"], d["key_labels"], d["W"], d["labels"], betas, alphas)
    r.update(d, F=F, betas=betas, alphas=alphas)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def undecided_share(c):
    return float(c["undecided"].sum()) / c["margin"].size


def _tol(ref64, ref32):
    ref64 = np.asarray(ref64, np.float64)
    own = np.abs(np.asarray(ref32, np.float64) - ref64).max()
    return max(8 * own, 16 * U * np.abs(ref64).max())


def _check(name, dev, ref64, ref32):
    err = np.abs(np.asarray(dev, np.float64) - np.asarray(ref64, np.float64)).max()
    tol = _tol(ref64, ref32)
    print(f"{name}: device err {err:.3e}, allowed {tol:.3e} "
          f"(scale {np.abs(np.asarray(ref64)).max():.3e})")
    assert np.isfinite(err) and err <= tol, name
    return err


class Guarded:
    """A device buffer between two canaries: NaN for float32, a sentinel for int32."""

    def __init__(self, shape, dtype=torch.float32):
        self.numel = int(np.prod(shape))
        self.fill = float("nan") if dtype == torch.float32 else SENTINEL
        self.buf = torch.full((self.numel + 2 * PAD,), self.fill, device="cuda", dtype=dtype)
        self.view = self.buf[PAD:PAD + self.numel].view(shape)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def _intact(self, t):
        return bool(torch.isnan(t).all()) if self.buf.dtype == torch.float32 else \
            bool((t == SENTINEL).all())

    def numpy(self, name):
        assert self._intact(self.buf[:PAD]), f"wrote in front of {name}"
        assert self._intact(self.buf[PAD + self.numel:]), f"wrote past {name}"
        out = self.view.cpu().numpy()
        if self.buf.dtype == torch.float32:
            assert np.isfinite(out).all(), f"{name} not written everywhere"
        else:
            assert (out != SENTINEL).all(), f"{name} not written everywhere"
        return out


class Scratch:
    """miclip_tip_scratch_bytes bytes followed by an 0xA5 guard."""

    def __init__(self, *dims):
        _, lib = _lib()
        self.nbytes = int(lib.miclip_tip_scratch_bytes(*dims))
        assert self.nbytes > 0 and self.nbytes % 16 == 0
        self.buf = torch.full((self.nbytes + 256,), 0xA5, device="cuda", dtype=torch.uint8)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def check(self):
        assert bool((self.buf[self.nbytes:] == 0xA5).all()), "wrote past the scratch"


def _lib():
    from miclip import _lib
    return _lib, _lib.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dt(t):
    L, _ = _lib()
    return {torch.float32: L.MICLIP_F32, torch.float16: L.MICLIP_FP16,
            torch.bfloat16: L.MICLIP_BF16}[t.dtype]


def _affinity(F, K, scale=1.0):
    """Device scale * F @ K^T through the C entry, into a guarded buffer."""
    L, lib = _lib()
    Fd, Kd = F.cuda().contiguous(), torch.tensor(np.asarray(K), dtype=torch.float32).cuda()
    out = Guarded((Fd.shape[0], Kd.shape[0]))
    L.check(lib.miclip_tip_affinity(_p(Fd), _dt(Fd), _p(Kd), Fd.shape[0], Kd.shape[0], Fd.shape[1],
                                    scale, out.ptr, L.stream_handle()), "miclip_tip_affinity")
    torch.cuda.synchronize()
    return out


def _grid(c, aff, Z):
    L, lib = _lib()
    Nq, Nk = aff.view.shape
    C, nb, na = Z.view.shape[1], len(c["betas"]), len(c["alphas"])
    klab = torch.tensor(c["key_labels"], dtype=torch.int32).cuda()
    lab = torch.tensor(c["labels"], dtype=torch.int32).cuda()
    betas = torch.tensor(c["betas"], dtype=torch.float32).cuda()
    alphas = torch.tensor(c["alphas"], dtype=torch.float32).cuda()
    counts, scratch = Guarded((nb, na), torch.int32), Scratch(Nq, Nk, 16, C, nb, na)
    L.check(lib.miclip_tip_grid(aff.ptr, _p(klab), Z.ptr, _p(lab), _p(betas), _p(alphas), Nq, Nk,
                                C, nb, na, counts.ptr, scratch.ptr, L.stream_handle()),
            "miclip_tip_grid")
    torch.cuda.synchronize()
    scratch.check()
    return counts.numpy("counts")


def _logits(c, aff, Z, beta, alpha):
    L, lib = _lib()
    Nq, Nk = aff.view.shape
    C = Z.view.shape[1]
    klab = torch.tensor(c["key_labels"], dtype=torch.int32).cuda()
    out, scratch = Guarded((Nq, C)), Scratch(Nq, Nk, 16, C, 1, 1)
    L.check(lib.miclip_tip_logits(aff.ptr, _p(klab), Z.ptr, Nq, Nk, C, beta, alpha, out.ptr,
                                  scratch.ptr, L.stream_handle()), "miclip_tip_logits")
    torch.cuda.synchronize()
    scratch.check()
    return out


def _check_counts(name, dev, c):
    diff = np.abs(dev.astype(np.int64) - c["counts"])
    share = undecided_share(c)
    print(f"{name}: largest count difference {diff.max()}, undecided rows per pair up to "
          f"{c['undecided'].max()}, undecided share {100 * share:.4f} % (cap 1 %)")
    assert share <= 0.01, "the case has too many undecided rows to test anything"
    assert (diff <= c["undecided"]).all(), name


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_grid_and_logits(idx, dname):
    from miclip import tip
    c = case(idx, dname)
    Nq, Nk, E, C, nb, na, _ = SHAPES[idx]
    aff = _affinity(c["F"], c["K"])
    Z = _affinity(c["F"], np.ascontiguousarray(c["W"].T), 100.0)
    a1, z1 = aff.numpy("affinity"), Z.numpy("clip logits")
    _check("affinity", a1, c["aff64"], c["aff32"])
    _check("clip logits", z1, c["Z64"], c["Z32"])
    if SHAPES[idx][6].get("equal"):
        # |F_0|^2: 1 up to the rounding of the unit query to its input type
        print(f"affinity of the key equal to its query: {a1[0, 0]!r} "
              f"(float64 {c['aff64'][0, 0]!r})")
        assert abs(a1[0, 0] - c["aff64"][0, 0]) <= 16 * U and abs(a1[0, 0] - 1.0) < 2e-2
    counts = _grid(c, aff, Z)
    _check_counts("counts", counts, c)

    ib, ia = nb // 2, na // 2
    beta, alpha = c["betas"][ib], c["alphas"][ia]
    lg = _logits(c, aff, Z, beta, alpha)
    l1 = lg.numpy("logits")
    _check("logits", l1, R.logits(c["Z64"], c["aff64"], c["key_labels"], beta, alpha).numpy(),
           R.logits(c["Z32"], c["aff32"], c["key_labels"], beta, alpha, torch.float32).numpy())
    acc = tip.cls_acc(lg.view, torch.tensor(c["labels"]).cuda())
    print(f"cls_acc of the logits at pair ({ib}, {ia}): {acc}, grid count {counts[ib, ia]} / {Nq}")
    assert acc == 100 * float(counts[ib, ia]) / Nq

    # a second run: bit-identical
    aff2 = _affinity(c["F"], c["K"])
    assert np.array_equal(aff2.numpy("affinity"), a1)
    assert np.array_equal(_grid(c, aff2, Z), counts)
    assert np.array_equal(_logits(c, aff2, Z, beta, alpha).numpy("logits"), l1)


KEY_SHAPES = [(1, 16, 16, 1), (5, 32, 16, 2), (43, 48, 48, 3), (257, 768, 512, 2),
              (20, 1280, 1024, 2)]     # (Nk, Wv, E, A); E = 1024 needs more than 64 KiB of LDS


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", KEY_SHAPES, ids=lambda s: "k{}-W{}-E{}-A{}".format(*s))
def test_keys(shape, dname):
    from miclip import tip
    L, lib = _lib()
    Nk, Wv, E, A = shape
    g = torch.Generator().manual_seed(Nk + Wv)
    views = [torch.randn(Nk, Wv, generator=g).to(DTYPES[dname]) for _ in range(A)]
    proj = torch.randn(Wv, E, generator=g) * Wv ** -0.5
    labels = torch.arange(Nk) % 3
    k64 = R.keys([v.float() for v in views], proj).numpy()
    k32 = R.keys([v.float() for v in views], proj, torch.float32).numpy()
    xs = [v.cuda() for v in views]
    ptrs = torch.tensor([x.data_ptr() for x in xs], dtype=torch.int64).cuda()
    Pd = proj.cuda()

    def run():
        out = Guarded((Nk, E))
        L.check(lib.miclip_tip_keys(_p(ptrs), _dt(xs[0]), A, Nk, Wv, E, _p(Pd), out.ptr,
                                    L.stream_handle()), "miclip_tip_keys")
        torch.cuda.synchronize()
        return out.numpy("keys")

    k1 = run()
    _check("keys", k1, k64, k32)
    assert np.array_equal(run(), k1)
    keys, values = tip.cache_model_from_views(views, labels, proj, 4)
    assert tuple(keys.shape) == (E, Nk) and keys.dtype == torch.float32
    assert np.array_equal(keys.t().cpu().numpy(), k1)
    assert values.dtype == torch.float16 and tuple(values.shape) == (Nk, 4)
    assert torch.equal(values.cpu().float(), torch.nn.functional.one_hot(labels, 4).float())


def test_keys_zero_row_is_not_finite():
    """The reference divides the mean by its norm without a floor: documented, not refused."""
    from miclip import tip
    views = [torch.randn(3, 16, generator=torch.Generator().manual_seed(1))]
    views[0][1] = 0
    keys, _ = tip.cache_model_from_views(views, torch.tensor([0, 1, 0]), torch.eye(16), 2)
    k = keys.t().cpu()
    print(f"key of the all-zero row: {k[1][:4].tolist()}")
    assert not torch.isfinite(k[1]).any() and torch.isfinite(k[[0, 2]]).all()


def _api_inputs(c):
    keys = torch.tensor(c["K"]).t().contiguous().cuda()                    # [E, Nk]
    C = c["W"].shape[1]
    values = torch.nn.functional.one_hot(torch.tensor(c["key_labels"]).long(), C).half().cuda()
    return keys, values, c["F"].cuda(), torch.tensor(c["labels"]).cuda(), torch.tensor(c["W"]).cuda()


@pytest.mark.parametrize("idx", [2, 3], ids=[IDS[2], IDS[3]])
def test_search_is_the_host_scan_of_the_device_grid(idx, capsys):
    from miclip import tip
    c = case(idx, "fp16")
    nb, na = SHAPES[idx][4:6]
    cfg = {"search_hp": True, "search_scale": SCALE, "search_step": [nb, na]}
    args = _api_inputs(c)
    counts, betas, alphas = tip.tip_accuracy_grid(*args, *tip.beta_alpha_lists(cfg))
    counts = counts.cpu().numpy()
    _check_counts("api counts", counts, c)
    best = tip.search_hp_tip(cfg, *args)
    out = capsys.readouterr().out
    print(f"search_hp_tip -> {best}; host scan of the device grid -> "
          f"{R.scan(counts, betas, alphas)}")
    assert best == R.scan(counts, betas, alphas)[:2]
    assert "After searching, the best accuarcy: {:.2f}.".format(
        100 * float(counts.max()) / len(c["labels"])) in out
    lg = tip.tip_logits(*args[:3], args[4], *best)
    assert tip.cls_acc(lg, args[3]) == 100 * float(counts.max()) / len(c["labels"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_pair(golden, tag):
    from miclip import tip
    g = golden("tip")
    m = g["meta"][tag]
    betas, alphas = R.lists(m["scale"], m["step"])
    r = R.grid(g[f"{tag}_F"], g[f"{tag}_keys"], g[f"{tag}_key_labels"], g[f"{tag}_W"],
               g[f"{tag}_labels"], betas, alphas)
    n = len(g[f"{tag}_labels"])
    keys = torch.tensor(g[f"{tag}_keys"]).t().contiguous().cuda()
    values = torch.nn.functional.one_hot(torch.tensor(g[f"{tag}_key_labels"]), m["C"]).half().cuda()
    args = (keys, values, torch.tensor(g[f"{tag}_F"]).cuda(), torch.tensor(g[f"{tag}_labels"]).cuda(),
            torch.tensor(g[f"{tag}_W"]).cuda())
    counts = tip.tip_accuracy_grid(*args, betas, alphas)[0].cpu().numpy()
    diff = np.abs(counts - r["counts"])
    print(f"golden {tag}: largest count difference {diff.max()}, undecided {r['undecided'].sum()}")
    assert (diff <= r["undecided"]).all()
    cfg = {"search_hp": True, "search_scale": m["scale"], "search_step": m["step"]}
    best = tip.search_hp_tip(cfg, *args)
    win = r["counts"] == r["counts"].max()
    if r["undecided"][win].sum() == 0 and (r["counts"] + r["undecided"])[~win].max(initial=0) < \
            r["counts"].max():
        print(f"golden {tag}: device pair {best}, reference pair {tuple(g[f'{tag}_best'])}")
        assert best == tuple(g[f"{tag}_best"])
        np.testing.assert_array_equal(100.0 * counts / n, g[f"{tag}_acc"])
    else:
        print(f"golden {tag}: an undecided row touches the winning count; counts compared only")


@functools.lru_cache(maxsize=None)
def few_shot():
    """20 directions, 16 keys each, queries around them, text weights rotated away."""
    d = R.planted(200, 320, 64, 20, seed=77)
    betas, alphas = R.lists(SCALE, [8, 6])
    r = R.grid(d["F"], d["K"], d["key_labels"], d["W"], d["labels"], betas, alphas)
    r.update(d, F=torch.tensor(d["F"]), betas=betas, alphas=alphas)
    return r


def test_planted_few_shot():
    from miclip import tip
    c = few_shot()
    args = _api_inputs(c)
    counts = tip.tip_accuracy_grid(*args, c["betas"], c["alphas"])[0].cpu().numpy()
    _check_counts("few-shot counts", counts, c)
    zs = int((tip.tip_logits(*args[:3], args[4], 1.0, 0.0).argmax(1) == args[3]).sum())
    print(f"few-shot: zero-shot {zs} (float64 {c['zero_shot']}), best Tip {counts.max()} "
          f"(float64 {c['counts'].max()}) of {len(c['labels'])}")
    assert counts.max() >= zs
    assert c["counts"].max() > c["zero_shot"], "the planted data must favour the cache"
    assert abs(int(counts.max()) - int(c["counts"].max())) <= c["undecided"].max()


def test_adapter_affinity():
    """An affinity supplied by a Python adapter (methods/utils.py:76-77) runs through the
    same two entries as the built-in one."""
    from miclip import tip
    c = case(2, "fp32")
    args = _api_inputs(c)
    adapter = torch.nn.Linear(args[0].shape[0], args[0].shape[1], bias=False).cuda()
    with torch.no_grad():
        adapter.weight.copy_(args[0].t())
    own = tip.tip_accuracy_grid(*args, c["betas"], c["alphas"])[0].cpu().numpy()
    sup = tip.tip_accuracy_grid(*args, c["betas"], c["alphas"], adapter=adapter)[0].cpu().numpy()
    print(f"adapter: largest count difference to the built-in affinity {np.abs(own - sup).max()}")
    _check_counts("adapter counts", sup, c)
    assert (np.abs(own - sup) <= c["undecided"]).all()
    lg = tip.tip_logits(*args[:3], args[4], c["betas"][1], c["alphas"][1], adapter=adapter)
    assert tip.cls_acc(lg, args[3]) == 100 * float(sup[1, 1]) / len(c["labels"])


def test_einval_names_the_argument():
    L, lib = _lib()
    buf = torch.zeros(4096, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    s = L.stream_handle()

    def refused(rc, name):
        msg = lib.miclip_last_error().decode()
        print(f"rc {rc}: {msg}")
        assert rc == -1 and msg.startswith(name), (name, msg)

    F32 = L.MICLIP_F32
    ok = dict(Nq=2, Nk=3, E=16, C=2, nb=2, na=2)

    def grid(**kw):
        a = dict(ok, **kw)
        return lib.miclip_tip_grid(p, p, p, p, p, p, a["Nq"], a["Nk"], a["C"], a["nb"], a["na"], p,
                                   p, s)

    def logits(**kw):
        a = dict(ok, **kw)
        return lib.miclip_tip_logits(p, p, p, a["Nq"], a["Nk"], a["C"], 1.0, 1.0, p, p, s)

    def aff(dtype=F32, **kw):
        a = dict(ok, **kw)
        return lib.miclip_tip_affinity(p, dtype, p, a["Nq"], a["Nk"], a["E"], 1.0, p, s)

    def keys(dtype=F32, A=1, Wv=16, **kw):
        a = dict(ok, **kw)
        return lib.miclip_tip_keys(p, dtype, A, a["Nk"], Wv, a["E"], p, p, s)

    for name, values in (("Nq", (0, -1, (1 << 24) + 1)), ("Nk", (0, -1, 65537)),
                         ("C", (0, -1, 1025)), ("nb", (0, -1, 1025)), ("na", (0, -1, 1025))):
        for v in values:
            refused(grid(**{name: v}), name)
    refused(grid(nb=1024, na=65), "nb * na")
    for name, values in (("Nq", (0, -1)), ("Nk", (65537, -1)), ("C", (1025, -1))):
        for v in values:
            refused(logits(**{name: v}), name)
    for name, values in (("Nq", (0, -1, (1 << 24) + 1)), ("Nk", (0, -1, 65537)),
                         ("E", (0, -16, 8, 24, 1040))):
        for v in values:
            refused(aff(**{name: v}), name)
    refused(aff(dtype=2), "f_dtype")
    for name, values in (("Nk", (0, -1, 65537)), ("E", (8, -16, 40, 2048))):
        for v in values:
            refused(keys(**{name: v}), name)
    refused(keys(A=0), "A ")
    refused(keys(A=1025), "A ")
    refused(keys(A=-1), "A ")
    refused(keys(Wv=-16), "Wv")
    refused(keys(Wv=8), "Wv")
    refused(keys(Wv=40), "Wv")
    refused(keys(dtype=7), "view_dtype")
    refused(lib.miclip_tip_grid(p, None, p, p, p, p, 2, 3, 2, 2, 2, p, p, s),
            "null argument: key_labels")
    refused(lib.miclip_tip_logits(p, p, p, 2, 3, 2, 1.0, 1.0, None, p, s), "null argument: logits")
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0     # nothing was launched


def test_build_cache_model_passes_and_files(tmp_path, capsys):
    """build_cache_model over a loader of already-encoded rows (a stub tower that returns
    its input): augment_epoch passes, keys against the restatement, the one-hot values, and
    the load_cache round trip through keys_task{task}.pt / values_task{task}.pt."""
    from miclip import tip

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))
            self.calls = 0

        def encode_image(self, images):
            self.calls += 1
            return images * (1.0 + 0.25 * (self.calls > 2))     # the second pass differs

    g = torch.Generator().manual_seed(5)
    x = torch.randn(21, 32, generator=g)
    y = torch.arange(21) % 4
    loader = [(x[:16], y[:16]), (x[16:], y[16:])]
    proj = torch.randn(32, 16, generator=g)
    cfg = {"load_cache": False, "augment_epoch": 2, "cache_dir": str(tmp_path / "tip"),
           "num_classes": 6}
    model = Stub().cuda()
    keys, values = tip.build_cache_model(cfg, model, loader, 3, proj)
    out = capsys.readouterr().out
    assert "Augment Epoch: 0 / 2" in out and "Augment Epoch: 1 / 2" in out and model.calls == 4
    views = [x, x * 1.25]
    _check("built keys", keys.t().cpu().numpy(), R.keys(views, proj).numpy(),
           R.keys(views, proj, torch.float32).numpy())
    assert tuple(values.shape) == (21, 6) and values.dtype == torch.float16
    assert torch.equal(values.cpu().float(), torch.nn.functional.one_hot(y, 6).float())
    assert (tmp_path / "tip" / "keys_task3.pt").is_file()
    k2, v2 = tip.build_cache_model(dict(cfg, load_cache=True), model, None, 3, proj)
    assert model.calls == 4 and k2.is_cuda
    assert torch.equal(k2, keys) and torch.equal(v2, values) and tuple(k2.shape) == (16, 21)
    # without cfg['num_classes'] the width is F.one_hot's own: the largest label + 1
    _, v3 = tip.build_cache_model(dict(cfg, num_classes=None), model, loader, 4, proj)
    assert tuple(v3.shape) == (21, 4)
