"""GPU: the trimmed class centroids of csrc/trim.hip (miclip_segment_rank,
miclip_trimmed_centroids) through the raw C ABI, compute_centroids(trim_frac=...) on top
of them, and the `score` subcommand of miclip.clean_testset.

The yardstick is tests/_trim_ref.py (float64; tests/test_trim_ref.py holds it against
hand-made cases). Raw calls put every output in front of canary elements, which must stay
untouched.

Exact checks: ranks against np.lexsort; the kept mask, kept counts and per-round change
counts against the float64 reference on seeds whose smallest float64 cut gap is 1e-4 or
more (asserted; fp32 cosine error is about 1e-6, so no row can cross a cut); the sums on
small-integer rows against the integer sum over the rows the device's own keep marks;
drop == 0 against miclip_class_centroids bit for bit; two calls against each other.

Bars on float data: the per-element error of centroids and similarities against float64
may be at most 4 x the error of the float32 numpy restatement of the same recipe on the
same input (tests/_trim_ref.py with dtype=float32), which allows another equally valid
fp32 summation order. The bar never comes from the device output. Measured on the
MI355X (device error / float32-restatement error, largest over the cases of
test_centroids_and_sims_within_four_times_the_float32_restatement; the test prints them):
centroids 1.043 (D = 768), similarities 1.008 (D = 3); 0 / 0 at D = 1, where both are exact.
"""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import _trim_ref as T

pytestmark = pytest.mark.gpu

CANARY_F, CANARY_I, PAD = -7.0, -7, 8
TILE = 1024          # miclip.outliers._TRIM_TILE, asserted below
EDGE_SIZES = (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _canary(n, dtype):
    fill = CANARY_F if dtype == torch.float32 else (249 if dtype == torch.uint8 else CANARY_I)
    return torch.full((n + PAD,), fill, device="cuda", dtype=dtype)


def _take(t, n):
    a = t.cpu().numpy()
    fill = CANARY_F if a.dtype == np.float32 else (249 if a.dtype == np.uint8 else CANARY_I)
    assert (a[n:] == fill).all(), "canary written"
    return a[:n]


def _untouched(t):
    return _take(t, 0).size == 0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _csr(inv, K):
    inv = np.asarray(inv, np.int64)
    order = np.argsort(inv, kind="stable").astype(np.int32)
    counts = np.bincount(inv, minlength=K)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return order, offsets, counts


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def raw_rank(values, inv, K, N=None):
    """miclip_segment_rank with a canary behind rank_out; returns (rc, ranks or None)."""
    from miclip import _lib
    lib = _lib.load_library()
    order, offsets, _ = _csr(inv, max(K, 1))
    n = len(values)
    rank = _canary(n, torch.int32)
    v, o, f = _dev(values, np.float32), _dev(order, np.int32), _dev(offsets, np.int32)
    rc = lib.miclip_segment_rank(_ptr(v), _ptr(o), _ptr(f), K, n if N is None else N, _ptr(rank),
                                 _lib.stream_handle(v.device))
    torch.cuda.synchronize()
    if rc != 0:
        assert _untouched(rank)
        return rc, None
    return rc, _take(rank, n)


def raw_trim(x, inv, K, drop, rounds, *, eps=1e-12, K_arg=None, N_arg=None):
    """miclip_trimmed_centroids with canaries behind every output; returns (rc, outputs)."""
    from miclip import _lib
    lib = _lib.load_library()
    x = np.ascontiguousarray(x, np.float32)
    N, D = x.shape
    order, offsets, counts = _csr(inv, K)
    r = max(int(rounds), 1)
    bufs = {"sums": _canary(K * D, torch.float32), "centroids": _canary(K * D, torch.float32),
            "keep": _canary(N, torch.uint8), "sims": _canary(N, torch.float32),
            "changed": _canary(r, torch.int32)}
    xd, o, f = _dev(x, np.float32), _dev(order, np.int32), _dev(offsets, np.int32)
    c, d = _dev(inv, np.int32), _dev(drop, np.int32)
    rc = lib.miclip_trimmed_centroids(
        _ptr(xd), _ptr(o), _ptr(f), _ptr(c), _ptr(d), K if K_arg is None else K_arg,
        N if N_arg is None else N_arg, D, int(rounds), float(eps), _ptr(bufs["sums"]),
        _ptr(bufs["centroids"]), _ptr(bufs["keep"]), _ptr(bufs["sims"]), _ptr(bufs["changed"]),
        _lib.stream_handle(xd.device))
    torch.cuda.synchronize()
    if rc != 0:
        assert all(_untouched(b) for b in bufs.values()), "an output was written"
        return rc, None
    out = {"sums": _take(bufs["sums"], K * D).reshape(K, D),
           "centroids": _take(bufs["centroids"], K * D).reshape(K, D),
           "keep": _take(bufs["keep"], N), "sims": _take(bufs["sims"], N),
           "changed": _take(bufs["changed"], r), "counts": counts}
    assert set(np.unique(out["keep"]).tolist()) <= {0, 1}
    return rc, out


# ------------------------------------------------------------------ miclip_segment_rank
def _edge_labels(rng, interleave=True):
    inv = np.repeat(np.arange(len(EDGE_SIZES)), EDGE_SIZES)
    return rng.permutation(inv) if interleave else inv


TIE_VALUES = np.asarray([-3.0, -1.0, -1e-40, -1.4e-45, -0.0, 0.0, 1.4e-45, 1e-40, 0.5, 1.0],
                        np.float32)


def _rank_cases():
    rng = np.random.default_rng(7)
    inv = _edge_labels(rng)
    n = len(inv)
    yield "ties", rng.choice(TIE_VALUES, n), inv, len(EDGE_SIZES)
    yield "all_equal", np.full(n, 0.25, np.float32), inv, len(EDGE_SIZES)
    yield "zeros_of_both_signs", rng.choice(np.asarray([0.0, -0.0], np.float32), n), inv, \
        len(EDGE_SIZES)
    yield "distinct", rng.standard_normal(n).astype(np.float32), inv, len(EDGE_SIZES)
    yield "grouped_order", rng.choice(TIE_VALUES, n), _edge_labels(rng, False), len(EDGE_SIZES)
    yield "one_class", rng.choice(TIE_VALUES, 300), np.zeros(300, np.int64), 1
    yield "one_row", np.asarray([2.0], np.float32), np.zeros(1, np.int64), 1
    yield "singletons", rng.choice(TIE_VALUES, 700), rng.permutation(700), 700
    # empty classes in front, in the middle and behind
    yield "empty_classes", rng.choice(TIE_VALUES, 303), \
        rng.permutation(np.repeat([1, 4], [3, 300])), 7


RANK_CASES = {name: rest for name, *rest in _rank_cases()}


@pytest.mark.parametrize("name", list(RANK_CASES))
def test_segment_rank_is_exactly_lexsort(name):
    from miclip import outliers as O
    assert O._TRIM_TILE == TILE
    values, inv, K = RANK_CASES[name]
    assert (np.abs(TIE_VALUES[[2, 3, 6, 7]]) < np.finfo(np.float32).tiny).all()   # subnormals
    rc, got = raw_rank(values, inv, K)
    assert rc == 0
    want = T.segment_rank(values, inv)
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    for k in np.unique(inv):                      # a permutation of 0 .. n_k - 1 per class
        assert np.array_equal(np.sort(got[inv == k]), np.arange(int((inv == k).sum())))


def test_segment_rank_helper_matches_the_raw_call():
    from miclip import outliers as O
    values, inv, K = RANK_CASES["ties"]
    order, offsets, _ = _csr(inv, K)
    got = O._segment_rank(_dev(values, np.float32), _dev(order, np.int32),
                          _dev(offsets, np.int32), K).cpu().numpy()
    assert np.array_equal(got, T.segment_rank(values, inv))


# ------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def _case(D, seed, f):
    x, lab, planted = T.planted_case(seed, D=D)
    uniq, inv, K = T.layout(lab)
    drop = T.drop_counts(np.bincount(inv, minlength=K), f)
    ref = T.trimmed_centroids(x, inv, K, drop, T.ROUNDS)
    ref32 = T.trimmed_centroids(x, inv, K, drop, T.ROUNDS, dtype=np.float32)
    for r in (ref, ref32):
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return {"x": x, "lab": lab, "uniq": uniq, "inv": inv, "K": K, "drop": drop, "ref": ref,
            "ref32": ref32}


def _meta(lab):
    return pd.DataFrame({"file_name": [f"img_{i:04d}.png" for i in range(len(lab))],
                         "ground_truth_num_label": np.asarray(lab, np.int64),
                         "ground_truth_word_label": [f"class_{int(v)}" for v in lab],
                         "ground_truth_L2_num_label": np.asarray(lab, np.int64) % 2})


@pytest.mark.parametrize("D,seed,f", T.MASK_CASES)
def test_kept_mask_counts_and_changes_equal_the_float64_reference(D, seed, f):
    from miclip.outliers import SingleCentroidScorer
    c = _case(D, seed, f)
    ref = c["ref"]
    if D == 1:      # similarities of exactly +-1: fp32 computes them exactly, ties decide
        assert set(np.abs(ref["sims"]).tolist()) <= {1.0}
    else:
        assert ref["min_gap"] >= T.GAP_MIN, ref["min_gap"]
    scorer = SingleCentroidScorer(torch.from_numpy(c["x"]), torch.from_numpy(c["lab"]),
                                  _meta(c["lab"]))
    res = scorer.compute_centroids(trim_frac=f, trim_rounds=T.ROUNDS)
    print(f"D={D} seed={seed} f={f}: gap {ref['min_gap']:.3e} changed {res.rounds_changed} "
          f"mask mismatches {int((res.kept_mask != ref['keep']).sum())}")
    assert res.kept_mask.dtype == bool and np.array_equal(res.kept_mask, ref["keep"])
    uniq = [int(v) for v in c["uniq"]]
    assert res.kept_counts == {u: int(n) for u, n in zip(uniq, ref["kept_counts"])}
    assert res.rounds_changed == ref["changed"]
    n = np.bincount(c["inv"])
    assert res.class_counts == {u: int(v) for u, v in zip(uniq, n)}      # the full sizes
    assert res.kept_counts == {u: int(v - d) for u, v, d in zip(uniq, n, c["drop"])}
    assert res.trim_frac == f and res.dim == D
    assert scorer.compute_centroids(trim_frac=f, trim_rounds=T.ROUNDS) is res
    assert scorer._centroids is None               # the plain cache is a separate one


ERR_CASES = [(64, 0, 0.1), (64, 4, 0.34), (1, 0, 0.34), (3, 1, 0.34), (65, 2, 0.1),
             (768, 4, 0.34)]


@pytest.mark.parametrize("D,seed,f", ERR_CASES)
def test_centroids_and_sims_within_four_times_the_float32_restatement(D, seed, f):
    c = _case(D, seed, f)
    ref, ref32 = c["ref"], c["ref32"]
    assert np.array_equal(ref32["keep"], ref["keep"])
    rc, out = raw_trim(c["x"], c["inv"], c["K"], c["drop"], T.ROUNDS)
    assert rc == 0
    assert np.array_equal(out["keep"].astype(bool), ref["keep"])
    for name in ("centroids", "sims"):
        err = float(np.abs(out[name].astype(np.float64) - ref[name]).max())
        err32 = float(np.abs(ref32[name].astype(np.float64) - ref[name]).max())
        ratio = err / err32 if err32 > 0 else (0.0 if err == 0 else float("inf"))
        print(f"D={D} seed={seed} f={f} {name}: device {err:.3e} float32 restatement "
              f"{err32:.3e} ratio {ratio:.3f}")
        assert err <= 4.0 * err32, (name, err, err32)


# ------------------------------------------------------------------ exact sums, drop == 0
def _integer_case():
    rng = np.random.default_rng(11)
    sizes = (1, 3, 40, 257, TILE + 6)
    inv = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    x = rng.integers(-8, 9, (len(inv), 70)).astype(np.float32)
    return x, inv, len(sizes), np.asarray(sizes)


def test_sums_are_the_integer_sums_of_the_rows_the_devices_keep_marks():
    x, inv, K, sizes = _integer_case()
    drop = T.drop_counts(sizes, 0.2)
    rc, out = raw_trim(x, inv, K, drop, 2)
    assert rc == 0
    keep = out["keep"].astype(bool)
    assert np.bincount(inv[keep], minlength=K).tolist() == (sizes - drop).tolist()
    want = np.zeros((K, x.shape[1]), np.int64)
    np.add.at(want, inv[keep], x[keep].astype(np.int64))
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(_bits(out["sums"]), _bits(want.astype(np.float32)))
    # and the centroid is those sums over the kept count, normalised (fp32 rounding only)
    m = want / (sizes - drop)[:, None]
    m = m / np.maximum(np.linalg.norm(m, axis=1, keepdims=True), 1e-12)
    assert np.abs(out["centroids"] - m).max() <= 4 * 2.0 ** -23


@pytest.mark.parametrize("kind", ["float", "integer"])
def test_zero_drop_is_bit_identical_to_class_centroids(kind):
    from miclip.outliers import _class_centroids
    if kind == "float":
        c = _case(65, 2, 0.1)
        x, inv, K = c["x"], c["inv"], c["K"]
    else:
        x, inv, K, _ = _integer_case()
    rc, out = raw_trim(x, inv, K, np.zeros(K, np.int32), 3)
    assert rc == 0
    plain, counts = _class_centroids(_dev(x, np.float32), inv, K, 1e-12)
    assert np.array_equal(_bits(out["centroids"]), _bits(plain.cpu().numpy()))
    assert out["keep"].all() and out["changed"].tolist() == [0, 0, 0]
    assert counts.tolist() == out["counts"].tolist()


def test_two_calls_are_bit_identical():
    c = _case(64, 4, 0.34)
    x = c["x"].copy()
    x[c["inv"] == 1] = x[np.flatnonzero(c["inv"] == 1)[0]]      # a class of ties
    a = raw_trim(x, c["inv"], c["K"], c["drop"], T.ROUNDS)[1]
    b = raw_trim(x, c["inv"], c["K"], c["drop"], T.ROUNDS)[1]
    for name in ("sums", "centroids", "sims"):
        assert np.array_equal(_bits(a[name]), _bits(b[name])), name
    assert np.array_equal(a["keep"], b["keep"]) and np.array_equal(a["changed"], b["changed"])
    # the class of identical rows drops its lowest sample indices
    tied = np.flatnonzero(c["inv"] == 1)
    m = int(c["drop"][1])
    assert m > 0 and np.flatnonzero(a["keep"][tied] == 0).tolist() == list(range(m))


# ------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_any_launch():
    from miclip import _lib, outliers as O
    x, inv, K = np.ones((6, 4), np.float32), np.asarray([0, 1, 0, 1, 0, 1]), 2
    drop = np.zeros(K, np.int32)
    for kwargs in ({"rounds": 0}, {"rounds": 9}, {"rounds": 1, "K_arg": 0},
                   {"rounds": 1, "N_arg": 0}):
        rounds = kwargs.pop("rounds")
        rc, out = raw_trim(x, inv, K, drop, rounds, **kwargs)
        assert rc == -1 and out is None, kwargs
        assert _lib.load_library().miclip_last_error()
    assert raw_rank(np.zeros(6, np.float32), inv, 0)[0] == -1
    # one class over the size limit: full-size buffers, so nothing depends on the refusal
    n = O._TRIM_MAX_CLASS_ROWS + 1
    assert raw_rank(np.zeros(n, np.float32), np.zeros(n, np.int64), 1)[0] == -1
    rc, out = raw_trim(np.ones((n, 1), np.float32), np.zeros(n, np.int64), 1,
                       np.zeros(1, np.int32), 1)
    assert rc == -1 and out is None
    assert b"largest supported class" in _lib.load_library().miclip_last_error()
    with pytest.raises(ValueError, match="miclip_trimmed_centroids"):
        O._trimmed_centroids(_dev(x, np.float32), inv, K, drop, 9, 1e-12)


def test_more_rows_than_one_call_takes_are_trimmed_group_by_group():
    """70 000 rows, above the 65 536 of one call, no class above it: the scorer packs the
    classes into two calls, and every class comes out as from a call on its rows alone."""
    from miclip import outliers as O
    rng = np.random.default_rng(13)
    sizes = (40000, 29990, 10)
    lab = rng.permutation(np.repeat(np.asarray([9, 4, 6]), sizes))
    x = rng.standard_normal((len(lab), 4))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    assert len(lab) > O._TRIM_MAX_CLASS_ROWS >= max(sizes)
    assert len(O._trim_groups([29990, 10, 40000], O._TRIM_MAX_CLASS_ROWS)) == 2   # labels 4, 6 | 9
    scorer = O.SingleCentroidScorer(torch.from_numpy(x), torch.from_numpy(lab), _meta(lab))
    res = scorer.compute_centroids(trim_frac=0.25, trim_rounds=2)
    changed = np.zeros(2, np.int64)
    for label, n in zip((9, 4, 6), sizes):
        rows = np.flatnonzero(lab == label)
        drop = T.drop_counts([n], 0.25).astype(np.int32)
        one = O._trimmed_centroids(_dev(x[rows], np.float32), np.zeros(n, np.int64), 1, drop, 2,
                                   1e-12)
        assert np.array_equal(_bits(res.centroids[label].cpu().numpy()),
                              _bits(one["centroids"][0].cpu().numpy())), label
        assert np.array_equal(res.kept_mask[rows], one["keep"].cpu().numpy().astype(bool)), label
        assert res.kept_counts[label] == n - int(drop[0]) and res.class_counts[label] == n
        changed += one["changed"].cpu().numpy()
    assert res.rounds_changed == changed.tolist() and changed[0] == 10000 + 7497 + 2


# ------------------------------------------------------------------ end to end
def _tiny_cache(path):
    """60 unit rows in 3 classes of 20 with one planted row each."""
    x, lab, planted = T.planted_case(5, D=16, sizes=(20, 20, 20), labels=(3, 0, 8))
    assert planted.sum() == 3 and len(x) == 60          # 8 % of 20 is one row per class
    torch.save(torch.from_numpy(x), path / "embeddings.pt")
    torch.save(torch.from_numpy(lab), path / "labels.pt")
    _meta(lab).to_csv(path / "metadata.csv", index=False)
    return x, lab, planted


def test_end_to_end_scorer_and_cli(tmp_path, capsys):
    from miclip import clean_testset, outliers as O
    x, lab, planted = _tiny_cache(tmp_path)
    emb, labels, meta = O.load_cache(O.resolve_cache_paths(tmp_path))
    scorer = O.SingleCentroidScorer(emb, labels, meta)
    res = scorer.compute_centroids(trim_frac=0.1)
    assert res.kept_counts == {0: 18, 3: 18, 8: 18} and res.rounds_changed == [6]
    assert not res.kept_mask[planted].any()
    frame = scorer.score_centroid_distance(centroids=res)
    names = {f"img_{i:04d}.png" for i in np.flatnonzero(planted)}
    top = frame[frame["file_name"].isin(names)]
    assert len(top) == 3 and (top["rank_in_class"] == 1).all()
    assert (frame["class_size"] == 20).all()
    out_csv = tmp_path / "out" / "scores.csv"
    assert clean_testset.main(["score", str(tmp_path), str(out_csv), "--trim-frac", "0.1"]) == 0
    printed = capsys.readouterr().out
    assert "==== Score Completed ====" in printed
    assert str({"cache_dir": str(tmp_path), "output_csv": str(out_csv), "num_samples": 60,
                "method": "single", "num_classes_present": 3, "total_prototypes": 3}) in printed
    got = pd.read_csv(out_csv, float_precision="round_trip")
    assert list(got.columns) == list(frame.columns)
    pd.testing.assert_frame_equal(got.astype(frame.dtypes.to_dict()), frame, check_exact=True)
    # the plain path through the CLI is the plain scorer's frame
    plain_csv = tmp_path / "plain.csv"
    clean_testset.main(["score", str(tmp_path), str(plain_csv)])
    capsys.readouterr()
    plain = O.SingleCentroidScorer(emb, labels, meta).score_centroid_distance()
    got = pd.read_csv(plain_csv, float_precision="round_trip")
    pd.testing.assert_frame_equal(got.astype(plain.dtypes.to_dict()), plain, check_exact=True)
    assert not np.array_equal(plain["sim_to_centroid"].to_numpy(),
                              frame["sim_to_centroid"].to_numpy())
