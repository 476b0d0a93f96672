"""GPU: exact t-SNE on the device (csrc/tsne.hip, miclip/embed_vis.py) against the float64
NumPy yardstick tests/_tsne_ref.py, which test_tsne_ref.py pins to scikit-learn.

Tolerance rule, wherever a device value is compared with the float64 yardstick: the
allowed error is the larger of
  * 8 x the error of the yardstick itself evaluated in float32 on the same inputs (the
    factor covers a different, butterfly summation order; it is reference arithmetic,
    never the code under test), and
  * 16 * 2^-24 relative to the largest magnitude in the compared array.
Shapes straddle the 64-lane, 256-thread and multi-workgroup boundaries; outputs land in
NaN-guarded buffers with canaries on both sides. Every figure is printed before it is
asserted.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _tsne_ref as R

pytestmark = pytest.mark.gpu

# (N, D, perplexity, metric, duplicated rows)
SHAPES = [(33, 16, 10.0, "cosine", 0), (64, 32, 5.0, "cosine", 4), (65, 1024, 20.0, "cosine", 0),
          (257, 48, 30.0, "cosine", 8), (300, 64, 30.0, "euclidean", 0),
          (1030, 24, 30.0, "cosine", 0)]
IDS = ["n{}-D{}-{}".format(s[0], s[1], s[3][:3]) for s in SHAPES]
METRIC = {"cosine": 0, "euclidean": 1, "precomputed": 2}
PAD = 64                      # canary floats on each side (keeps 16-byte alignment)
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case(idx):
    """Inputs and yardstick values of SHAPES[idx], computed once and never modified."""
    n, d, perp, metric, dup = SHAPES[idx]
    x = R.planted(n, d, seed=n, dup=dup)
    d64 = R.distances(x, metric)
    d32 = d64.astype(np.float32)
    P64, b64 = R.joint_probabilities(d32, perp)
    P32, b32 = R.joint_probabilities(d32, perp, np.float32)
    c = {"x": x, "d64": d64, "d32": d32, "P64": P64, "b64": b64, "P32": P32, "b32": b32,
         "Pin": P64.astype(np.float32), "y0": R.pca_init(x)}
    for v in c.values():
        v.setflags(write=False)
    return c


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
    """A float32 device buffer between two NaN canaries."""

    def __init__(self, shape, fill=None):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + 2 * PAD,), float("nan"), device="cuda")
        self.view = self.buf[PAD:PAD + self.numel].view(shape)
        if fill is not None:
            self.view.copy_(torch.tensor(np.asarray(fill), dtype=torch.float32))

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def numpy(self, name):
        assert bool(torch.isnan(self.buf[:PAD]).all()), f"wrote in front of {name}"
        assert bool(torch.isnan(self.buf[PAD + self.numel:]).all()), f"wrote past {name}"
        out = self.view.cpu().numpy()
        assert np.isfinite(out).all(), f"{name} not written everywhere"
        return out


def _lib():
    from miclip import _lib
    return _lib, _lib.load_library()


def _scratch(n):
    _, lib = _lib()
    nbytes = lib.miclip_tsne_scratch_bytes(n)
    assert nbytes % 4 == 0
    return Guarded((nbytes // 4,))


def _affinities(x, n, d, metric, perp, want_dist):
    L, lib = _lib()
    xd = torch.tensor(np.asarray(x), dtype=torch.float32).cuda()
    P, beta, scratch = Guarded((n, n)), Guarded((n,)), _scratch(n)
    dist = Guarded((n, n)) if want_dist else None
    L.check(lib.miclip_tsne_affinities(ctypes.c_void_p(xd.data_ptr()), n, d, METRIC[metric],
                                       perp, P.ptr, beta.ptr, dist.ptr if dist else None,
                                       scratch.ptr, L.stream_handle()), "miclip_tsne_affinities")
    torch.cuda.synchronize()
    scratch.view.nan_to_num_()           # the scratch need not be written everywhere
    scratch.numpy("scratch")
    return (P.numpy("P"), beta.numpy("beta"), dist.numpy("dist") if dist else None)


def _run(P, y, update, gains, n_steps, ex, mom, lr, error_every=0, min_gain=0.01):
    L, lib = _lib()
    n = P.shape[0]
    Pd = torch.tensor(np.asarray(P), dtype=torch.float32).cuda()
    yg, ug, gg = Guarded((n, 2), y), Guarded((n, 2), update), Guarded((n, 2), gains)
    stats, scratch = Guarded((4,)), _scratch(n)
    L.check(lib.miclip_tsne_run(ctypes.c_void_p(Pd.data_ptr()), n, yg.ptr, ug.ptr, gg.ptr, n_steps,
                                ex, mom, lr, min_gain, error_every, scratch.ptr, stats.ptr,
                                L.stream_handle()), "miclip_tsne_run")
    torch.cuda.synchronize()
    scratch.view.nan_to_num_()
    scratch.numpy("scratch")
    return yg.numpy("y"), ug.numpy("update"), gg.numpy("gains"), stats.numpy("stats")


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_g1_distances(idx):
    n, d, perp, metric, dup = SHAPES[idx]
    c = case(idx)
    P, beta, dist = _affinities(c["x"], n, d, metric, perp, True)
    bound = (d + 8) * 2.0 ** -23
    assert (np.diag(dist) == 0).all()
    if metric == "cosine":
        dev, ref = np.sqrt(dist.astype(np.float64)), R.cosine_distance(c["x"])
        err = np.abs(dev - ref).max()
        print(f"cosine distance before squaring: err {err:.3e}, allowed {bound:.3e}")
        assert err <= bound
        if dup:
            pair = dev[np.arange(dup), n - dup + np.arange(dup)]
            print(f"duplicated rows: distance {pair.max():.3e}")
            assert pair.max() <= bound
    else:
        sq = (c["x"].astype(np.float64) ** 2).sum(1)
        rel = (np.abs(dist - c["d64"]) / (sq[:, None] + sq[None, :])).max()
        print(f"squared euclidean distance: relative err {rel:.3e}, allowed {bound:.3e}")
        assert rel <= bound
    # without a dist buffer the distances pass through P: the same P, bit for bit
    P2, beta2, _ = _affinities(c["x"], n, d, metric, perp, False)
    assert np.array_equal(P, P2) and np.array_equal(beta, beta2)


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_g2_perplexity_and_joint_p(idx):
    """Metric 2 is fed the float32 distances the yardstick uses: only the search and the
    symmetrisation are under test. The entropy is recomputed on the host in float64 from
    those distances at the device's beta."""
    n, d, perp, metric, dup = SHAPES[idx]
    c = case(idx)
    P, beta, dist = _affinities(c["d32"], n, n, "precomputed", perp, True)
    assert np.array_equal(dist, c["d32"])
    _check("beta", beta, c["b64"], c["b32"])
    _check("P", P, c["P64"], c["P32"])
    assert np.array_equal(P, P.T), "P is not bit-symmetric"
    assert (np.diag(P) == 0).all()
    total = P.astype(np.float64).sum()
    off = P[~np.eye(n, dtype=bool)]
    print(f"sum P - 1 = {total - 1:.3e}, min off-diagonal {off.min():.3e}")
    assert abs(total - 1) <= 1e-6
    assert off.min() >= np.float32(R.EPS)
    p = np.exp(-c["d32"].astype(np.float64) * beta.astype(np.float64)[:, None])
    np.fill_diagonal(p, 0)
    s = p.sum(1)
    H = np.log(s) + beta * (c["d32"] * p).sum(1) / s
    miss = np.abs(H - np.log(perp)) > 2e-5
    print(f"rows off the perplexity by more than 2e-5: {miss.sum()} of {n}, "
          f"worst {np.abs(H - np.log(perp)).max():.3e}")
    assert miss.mean() <= 0.01


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_g3_one_step(idx):
    """update = 0 and gains = 1: gains become 0.8 exactly, update = -lr * 0.8 * g (lr a power
    of two, so g is recovered to two roundings) and y_new = y + update in fp32."""
    n = SHAPES[idx][0]
    c = case(idx)
    lr = 64.0
    for k, (scale, ex) in enumerate(((1e-4, 12.0), (5.0, 1.0), (40.0, 1.0))):
        y = (np.random.default_rng(10 * idx + k).standard_normal((n, 2)) * scale).astype(np.float32)
        kl64, g64, Z64 = R.objective(c["Pin"], y, ex)
        kl32, g32, Z32 = R.objective(c["Pin"], y, ex, np.float32)
        yn, un, gn, st = _run(c["Pin"], y, np.zeros((n, 2)), np.ones((n, 2)), 1, ex, 0.5, lr)
        assert (gn == np.float32(0.8)).all()
        assert np.array_equal(yn, y + un)
        g = un.astype(np.float64) / (-lr) / float(np.float32(0.8))
        _check(f"scale {scale}: gradient", g, g64, g32)
        _check(f"scale {scale}: KL", st[0], kl64, kl32)
        _check(f"scale {scale}: Z", st[2], Z64, Z32)
        n64 = 0.8 * np.sqrt((g64 * g64).sum())
        n32 = np.float32(0.8) * np.sqrt((g32 * g32).sum(dtype=np.float32))
        _check(f"scale {scale}: gradient norm", st[1], n64, n32)
        assert st[3] == 1.0


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_g4_gains_and_momentum(idx):
    n = SHAPES[idx][0]
    c = case(idx)
    rng = np.random.default_rng(100 + idx)
    y = (rng.standard_normal((n, 2)) * 5).astype(np.float32)
    update = (rng.standard_normal((n, 2)) * 0.5).astype(np.float32)
    gains = rng.uniform(0.05, 3.0, (n, 2)).astype(np.float32)
    gains[::7] = np.float32(0.011)          # 0.011 * 0.8 < min_gain: the clip is reached
    lr, mom = 200.0, 0.8
    r64 = R.step(c["Pin"], y, update, gains, 1.0, mom, lr)
    r32 = R.step(c["Pin"], y, update, gains, 1.0, mom, lr, dtype=np.float32)
    keep = np.abs(r64["g"]) >= 1e-5 * np.abs(r64["g"]).max()
    print(f"entries with an undecided sign: {(~keep).mean():.4%}")
    assert (~keep).mean() <= 0.01
    yn, un, gn, st = _run(c["Pin"], y, update, gains, 1, 1.0, mom, lr)
    inc = update.astype(np.float64) * r64["g"] < 0
    rule = np.where(inc, gains + np.float32(0.2),
                    np.maximum(gains * np.float32(0.8), np.float32(0.01))).astype(np.float32)
    assert (gn[::7][~inc[::7] & keep[::7]] == np.float32(0.01)).all()
    assert np.array_equal(gn[keep], rule[keep])
    _check("update", un[keep], r64["update"][keep], r32["update"][keep])
    _check("y", yn[keep], r64["y"][keep], r32["y"][keep])


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
def test_g5_ten_steps(idx):
    n = SHAPES[idx][0]
    c = case(idx)
    lr = R.learning_rate_auto(n)
    ref = {}
    for dt in (np.float64, np.float32):
        y, u, g = c["y0"], np.zeros((n, 2)), np.ones((n, 2))
        for _ in range(10):
            r = R.step(c["Pin"], y, u, g, 12.0, 0.5, lr, dtype=dt, compute_error=False)
            y, u, g = r["y"], r["update"], r["gains"]
        ref[dt] = y
    yn, un, gn, st = _run(c["Pin"], c["y0"], np.zeros((n, 2)), np.ones((n, 2)), 10, 12.0, 0.5, lr)
    _check("y after ten steps", yn, ref[np.float64], ref[np.float32])
    assert st[3] == 10.0
    y4, _, _, st4 = _run(c["Pin"], c["y0"], np.zeros((n, 2)), np.ones((n, 2)), 10, 12.0, 0.5, lr,
                         error_every=4)
    print(f"error_every=4 of 10 steps: stats written after step {st4[3]:.0f}")
    assert st4[3] == 8.0
    assert np.array_equal(y4, yn)


def test_g6_determinism():
    from miclip import embed_vis
    small, big = case(0)["x"], case(3)["x"]
    kw = dict(perplexity=30.0, metric="cosine", init="pca")
    s1 = embed_vis.tsne(small, perplexity=10.0)
    a = embed_vis.tsne(big, **kw)
    b = embed_vis.tsne(big, **kw)
    s2 = embed_vis.tsne(small, perplexity=10.0)
    Pa = embed_vis.affinities(big, perplexity=30.0)[0].cpu().numpy()
    Pb = embed_vis.affinities(big, perplexity=30.0)[0].cpu().numpy()
    print(f"KL {a.kl_divergence!r} / {b.kl_divergence!r}, n_iter {a.n_iter} / {b.n_iter}")
    assert a.coords.dtype == np.float32 and a.coords.shape == (257, 2)
    assert np.isfinite(a.coords).all() and np.isfinite(a.kl_divergence)
    assert np.array_equal(a.coords, b.coords) and a.kl_divergence == b.kl_divergence
    assert a.n_iter == b.n_iter == 999
    assert np.array_equal(Pa, Pb)
    assert np.array_equal(s1.coords, s2.coords) and s1.kl_divergence == s2.kl_divergence


# The largest spread among scikit-learn's exact method and the yardstick's full schedule in
# float64 and in float32, measured on the CPU on the two inputs below (figures in the
# docstring of the test): relative in KL, absolute in trustworthiness.
G7_CASES = [(300, 64, 300, 0), (257, 48, 257, 8)]
G7_SPREAD = {"kl": 0.00742, "trust": 0.00067}


@pytest.mark.parametrize("n,d,seed,dup", G7_CASES, ids=["n300-D64", "n257-D48"])
def test_g7_end_to_end_against_sklearn(n, d, seed, dup):
    """Quality bounds, not point-wise parity: the trajectories are chaotic.

    m and m_t are 3 x the largest spread among scikit-learn exact, the float64 yardstick and
    the float32 yardstick, measured on the CPU on this test's own inputs:
      (300, 64): KL 0.408676 / 0.411607 / 0.408574 (spread 0.742 %), trustworthiness
                 0.964498 / 0.964030 / 0.964688 (spread 0.00066); init 0.9346
      (257, 48): KL 0.304368 / 0.303464 / 0.305029 (spread 0.516 %), trustworthiness
                 0.970262 / 0.970252 / 0.970923 (spread 0.00067); init 0.9427
    so m = 3 * 0.00742 = 0.0223 and m_t = 3 * 0.00067 = 0.0020. scikit-learn's default
    Barnes-Hut gave KL 0.412639 / 0.301766 and trustworthiness 0.9655 / 0.9703.
    """
    from sklearn.manifold import TSNE, trustworthiness

    from miclip import embed_vis
    m, m_t = 3 * G7_SPREAD["kl"], 3 * G7_SPREAD["trust"]
    x = R.planted(n, d, seed=seed, dup=dup)
    y0 = R.pca_init(x)
    kw = dict(n_components=2, perplexity=30.0, metric="cosine", init=y0, random_state=1,
              max_iter=1000)
    sk = TSNE(method="exact", **kw)
    ys = sk.fit_transform(x)
    bh = TSNE(**kw)
    yb = bh.fit_transform(x)
    dev = embed_vis.tsne(x, perplexity=30.0, metric="cosine", init=y0, max_iter=1000)

    def trust(y):
        return trustworthiness(x, y, n_neighbors=10, metric="cosine")
    t_dev, t_sk, t_bh, t_init = trust(dev.coords), trust(ys), trust(yb), trust(y0)
    print(f"KL: device {dev.kl_divergence:.5f}, sklearn exact {sk.kl_divergence_:.5f} "
          f"(allowed x{1 + m:.4f}), Barnes-Hut {bh.kl_divergence_:.5f}")
    print(f"trustworthiness: device {t_dev:.4f}, sklearn exact {t_sk:.4f} (allowed -{m_t:.4f}), "
          f"Barnes-Hut {t_bh:.4f}, init {t_init:.4f}")
    assert dev.n_iter == 999
    assert dev.kl_divergence <= sk.kl_divergence_ * (1 + m)
    assert t_dev >= t_sk - m_t
    assert t_dev >= t_init + 0.02


@functools.lru_cache(maxsize=None)
def _pca_data(n, d):
    rng = np.random.default_rng(n + d)
    basis, _ = np.linalg.qr(rng.standard_normal((d, 8)))
    scale = 0.7 ** np.arange(8)
    x = (rng.standard_normal((n, 8)) * scale) @ basis.T + 1e-3 * rng.standard_normal((n, d))
    return (x + rng.standard_normal(d)).astype(np.float32)


@pytest.mark.parametrize("n,d", [(300, 64), (65, 1024)])
def test_g8_pca(n, d):
    from sklearn.decomposition import PCA

    from miclip import embed_vis
    x = _pca_data(n, d)
    pca = PCA(n_components=8, svd_solver="full")
    ref = pca.fit_transform(x.astype(np.float64))
    own, _ = R.pca(x, 8, np.float32)
    dev, ratio = embed_vis.pca_reduce(x, 8, device="cuda")
    assert dev.dtype == np.float32 and dev.shape == (n, 8)
    for k in range(8):
        def err(a):
            a = a.astype(np.float64)
            return min(np.abs(a - ref[:, k]).max(), np.abs(a + ref[:, k]).max())
        allowed = max(8 * err(own[:, k]), 16 * U * np.abs(ref).max())
        print(f"component {k}: device err {err(dev[:, k]):.3e}, allowed {allowed:.3e}")
        assert err(dev[:, k]) <= allowed
    want = float(pca.explained_variance_ratio_.sum())
    print(f"explained variance ratio sum: device {ratio:.7f}, sklearn {want:.7f}")
    assert abs(ratio - want) <= 1e-4 * want


def test_g9_cache_flow(tmp_path):
    import pandas as pd

    from miclip import embed_vis
    n = 257
    x = case(3)["x"]
    torch.save(torch.tensor(x).half(), tmp_path / "embeddings.pt")
    torch.save(torch.arange(n) % 5, tmp_path / "labels.pt")
    meta = pd.DataFrame({"file_name": [f"{i}.jpg" for i in range(n)],
                         "ground_truth_num_label": np.arange(n) % 5})
    meta.to_csv(tmp_path / "metadata.csv", index=False)
    df = embed_vis.visualize_cache(str(tmp_path))
    coords = np.load(tmp_path / "vis_tsne_coords.npy")
    assert coords.shape == (n, 2) and coords.dtype == np.float32 and np.isfinite(coords).all()
    assert list(df.columns) == ["file_name", "ground_truth_num_label", "x", "y"]
    assert np.array_equal(df["x"].to_numpy(), coords[:, 0])
    with pytest.raises(FileExistsError, match="use --overwrite to replace"):
        embed_vis.visualize_cache(str(tmp_path))
    embed_vis.visualize_cache(str(tmp_path), pca_dim=16, out_prefix="pca16")
    assert np.load(tmp_path / "pca16_tsne_coords.npy").shape == (n, 2)
    meta.iloc[:-1].to_csv(tmp_path / "metadata.csv", index=False)
    with pytest.raises(ValueError, match="Row mismatch: coords_2d has 257 rows, metadata has 256"):
        embed_vis.visualize_cache(str(tmp_path), overwrite=True)


# ---- the large-N paths: more rows per wave (N > 4096) and LDS rows beyond 48 KiB ----
# A NumPy yardstick at this size would take minutes, so the same restatement runs in torch
# on the device (_tsne_ref.t_joint_probabilities / t_objective), in float64 (the reference)
# and in float32 (its own rounding error); test_tsne_ref.py pins it to the NumPy yardstick.
def test_g10_large_n_paths():
    """N = 12 400: four rows per wave in the forces kernel, y in 97 KiB and a row of
    distances in 48.4 KiB of LDS. Affinities from given distances (metric 2), then one step."""
    L, lib = _lib()
    n, perp = 12400, 30.0
    x = torch.from_numpy(R.planted(n, 16, n_clusters=20, seed=7)).cuda().double()
    d32 = torch.clamp(1 - x @ x.t(), 0, 2).fill_diagonal_(0).square_().float()
    del x
    P64, b64 = R.t_joint_probabilities(d32, perp, torch.float64)
    P32, b32 = R.t_joint_probabilities(d32, perp, torch.float32)
    P, beta, scratch = Guarded((n, n)), Guarded((n,)), _scratch(n)
    L.check(lib.miclip_tsne_affinities(ctypes.c_void_p(d32.data_ptr()), n, n, 2, perp, P.ptr,
                                       beta.ptr, None, scratch.ptr, L.stream_handle()),
            "miclip_tsne_affinities")
    torch.cuda.synchronize()
    _check("beta", beta.numpy("beta"), b64.cpu().numpy(), b32.cpu().numpy())
    Pd = P.view
    assert bool(torch.isnan(P.buf[:PAD]).all()) and bool(torch.isnan(P.buf[PAD + P.numel:]).all())
    err = float((Pd.double() - P64).abs().max())
    tol = max(8 * float((P32.double() - P64).abs().max()), 16 * U * float(P64.max()))
    print(f"P: device err {err:.3e}, allowed {tol:.3e}")
    assert err <= tol
    assert bool(torch.equal(Pd, Pd.t())) and bool((Pd.diagonal() == 0).all())
    total = float(Pd.double().sum())
    print(f"sum P - 1 = {total - 1:.3e}")
    assert abs(total - 1) <= 1e-6
    del P32, d32
    Pin = P64.float()
    del P64
    y = torch.from_numpy((np.random.default_rng(3).standard_normal((n, 2)) * 5)
                         .astype(np.float32)).cuda()
    kl64, g64, Z64 = R.t_objective(Pin, y, 1.0, torch.float64)
    kl32, g32, Z32 = R.t_objective(Pin, y, 1.0, torch.float32)
    yg, ug, gg = Guarded((n, 2), y.cpu().numpy()), Guarded((n, 2), np.zeros((n, 2))), \
        Guarded((n, 2), np.ones((n, 2)))
    stats, scratch, lr = Guarded((4,)), _scratch(n), 64.0
    L.check(lib.miclip_tsne_run(ctypes.c_void_p(Pin.data_ptr()), n, yg.ptr, ug.ptr, gg.ptr, 1, 1.0,
                                0.5, lr, 0.01, 0, scratch.ptr, stats.ptr, L.stream_handle()),
            "miclip_tsne_run")
    torch.cuda.synchronize()
    un, st = ug.numpy("update"), stats.numpy("stats")
    assert (gg.numpy("gains") == np.float32(0.8)).all()
    assert np.array_equal(yg.numpy("y"), y.cpu().numpy() + un)
    g = un.astype(np.float64) / (-lr) / float(np.float32(0.8))
    _check("gradient", g, g64.cpu().numpy(), g32.cpu().numpy())
    _check("KL", st[0], float(kl64), float(kl32))
    _check("Z", st[2], float(Z64), float(Z32))
