"""CPU: the float64 restatement of the trimmed class centroids (tests/_trim_ref.py) on
hand-made cases, the host-side argument checks of compute_centroids(trim_frac=...), and
the parser of miclip.clean_testset. Nothing here needs a device.

The last test asserts, for the seeds tests/test_gpu_trim.py uses, the precondition its
exact kept-mask comparison rests on: at every class cut of every round the float64
similarities on the two sides of the cut differ by GAP_MIN = 1e-4 or more, a hundred
times the fp32 cosine error (about 1e-6), so fp32 cannot move a row across a cut.
"""
import numpy as np
import pandas as pd
import pytest
import torch

import _trim_ref as T

GAP_MIN, MASK_CASES, ROUNDS = T.GAP_MIN, T.MASK_CASES, T.ROUNDS


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _run(x, labels, f, rounds=1, dtype=np.float64):
    uniq, inv, K = T.layout(labels)
    drop = T.drop_counts(np.bincount(inv, minlength=K), f)
    return T.trimmed_centroids(x, inv, K, drop, rounds, dtype=dtype), uniq, inv, drop


def test_zero_fraction_is_the_plain_centroid():
    x, lab, _ = T.planted_case(0)
    r, uniq, inv, drop = _run(x, lab, 0.0, rounds=3)
    assert (drop == 0).all() and r["keep"].all() and r["changed"] == [0, 0, 0]
    assert r["min_gap"] is None
    for k in range(len(uniq)):
        m = x[inv == k].astype(np.float64).mean(axis=0)
        np.testing.assert_allclose(r["centroids"][k], m / np.linalg.norm(m), rtol=0, atol=1e-15)
    assert np.array_equal(r["centroids"], r["plain"])


def test_planted_outliers_are_dropped():
    x, lab, planted = T.planted_case(3)
    r, uniq, inv, drop = _run(x, lab, 0.1, rounds=2)
    # 8 % are planted, 10 % are dropped: every planted row of a class that drops any goes
    for k in range(len(uniq)):
        if drop[k] >= int(planted[inv == k].sum()) > 0:
            assert not r["keep"][(inv == k) & planted].any()
    assert r["changed"][0] == int(drop.sum())
    big = [k for k in range(len(uniq)) if drop[k] > 0]
    assert len(big) == 2
    plain_cos = [(r["plain"][k] * _unit(x[(inv == k) & ~planted].astype(np.float64)
                                       .mean(axis=0, keepdims=True))[0]).sum() for k in big]
    trim_cos = [(r["centroids"][k] * _unit(x[(inv == k) & ~planted].astype(np.float64)
                                           .mean(axis=0, keepdims=True))[0]).sum() for k in big]
    assert all(t > p for t, p in zip(trim_cos, plain_cos))   # closer to the clean mean


def test_identical_class_drops_its_lowest_sample_indices():
    row = _unit(np.arange(1.0, 9.0)[None])[0]
    other = _unit(np.arange(8.0, 0.0, -1.0)[None])[0]
    lab = np.asarray([4, 9, 4, 4, 9, 4, 4, 4, 9, 4, 4, 4, 4])        # ten 4s, three 9s
    x = np.where((lab == 4)[:, None], row, other)
    r, uniq, inv, drop = _run(x, lab, 0.3, rounds=2)
    assert drop.tolist() == [3, 0]
    fours = np.flatnonzero(lab == 4)
    assert np.flatnonzero(~r["keep"]).tolist() == fours[:3].tolist()
    assert r["changed"] == [3, 0] and r["min_gap"] == 0.0
    assert T.segment_rank(np.zeros(13), inv)[fours].tolist() == list(range(10))


def test_negative_zero_ties_with_zero():
    v = np.asarray([0.0, -0.0, -0.0, 0.0, -1.0], np.float32)
    assert T.segment_rank(v, np.zeros(5, np.int64)).tolist() == [1, 2, 3, 4, 0]


@pytest.mark.parametrize("f", [0.0, 0.1, 0.25, 0.34, 0.499])
def test_kept_counts(f):
    x, lab, _ = T.planted_case(1)
    r, uniq, inv, drop = _run(x, lab, f, rounds=3)
    n = np.bincount(inv)
    assert drop.tolist() == [int(np.floor(f * v)) for v in n]
    assert r["kept_counts"].tolist() == (n - drop).tolist()
    assert np.bincount(inv[r["keep"]], minlength=len(uniq)).tolist() == (n - drop).tolist()
    assert (r["kept_counts"] >= 1).all()


def test_labels_may_be_sparse_and_interleaved():
    x, lab, _ = T.planted_case(2)
    a, _, inv, _ = _run(x, lab, 0.2, rounds=2)
    # the same rows grouped by class with contiguous labels 0..K-1: the same answer per row
    order = np.argsort(inv, kind="stable")
    b, _, inv_b, _ = _run(x[order], inv[order], 0.2, rounds=2)
    assert np.array_equal(a["keep"][order], b["keep"])
    np.testing.assert_allclose(a["centroids"], b["centroids"], rtol=0, atol=1e-15)
    assert a["changed"] == b["changed"]


def _scorer(n=12, d=4):
    from miclip.outliers import SingleCentroidScorer
    x = torch.from_numpy(_unit(np.random.default_rng(0).standard_normal((n, d))).astype(np.float32))
    lab = torch.arange(n) % 3
    meta = pd.DataFrame({"file_name": [f"f{i}.png" for i in range(n)],
                         "ground_truth_num_label": lab.numpy()})
    return SingleCentroidScorer(x, lab, meta, device="cpu")     # no kernel may run on it


@pytest.mark.parametrize("kwargs", [
    {"trim_frac": 0.5}, {"trim_frac": -0.01}, {"trim_frac": True}, {"trim_frac": "0.1"},
    {"trim_frac": float("nan")}, {"trim_frac": float("inf")}, {"trim_frac": 1},
    {"trim_frac": 0.1, "trim_rounds": 0}, {"trim_frac": 0.1, "trim_rounds": 9},
    {"trim_frac": 0.1, "trim_rounds": 2.0}, {"trim_frac": 0.1, "trim_rounds": True},
    {"trim_frac": 0.1, "trim_rounds": None}])
def test_compute_centroids_refuses_bad_trim_arguments_on_the_host(kwargs, monkeypatch):
    from miclip import outliers

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    for name in ("_row_norms", "_class_layout", "_trimmed_centroids"):
        monkeypatch.setattr(outliers, name, no_device)
    with pytest.raises(ValueError, match="trim_frac|trim_rounds"):
        _scorer().compute_centroids(**kwargs)


def test_trimmed_results_are_cached_per_setting_apart_from_the_plain_one(monkeypatch):
    from miclip import outliers
    calls = []

    def fake(x, inv, K, drop, rounds, eps):
        calls.append((drop.tolist(), rounds))
        return {"centroids": torch.zeros(K, x.shape[1]), "keep": torch.ones(len(inv), dtype=torch.uint8),
                "changed": torch.zeros(rounds, dtype=torch.int32),
                "counts": np.bincount(inv, minlength=K)}
    monkeypatch.setattr(outliers, "_trimmed_centroids", fake)
    monkeypatch.setattr(outliers, "_row_norms",
                        lambda x, *a, **k: (torch.ones(x.shape[0]), None))
    s = _scorer()
    a = s.compute_centroids(trim_frac=0.25)
    assert s.compute_centroids(trim_frac=0.25, trim_rounds=1) is a
    b = s.compute_centroids(trim_frac=0.25, trim_rounds=2)
    c = s.compute_centroids(trim_frac=0.0)
    assert calls == [([1, 1, 1], 1), ([1, 1, 1], 2), ([0, 0, 0], 1)]
    assert b is not a and c is not a and s._centroids is None
    assert a.trim_frac == 0.25 and a.class_counts == {0: 4, 1: 4, 2: 4}
    assert a.kept_counts == {0: 4, 1: 4, 2: 4} and a.rounds_changed == [0]
    assert a.kept_mask.dtype == bool and a.kept_mask.shape == (12,)
    from miclip.outliers import CentroidResult
    plain = CentroidResult(centroids={}, class_counts={}, dim=4)
    assert (plain.trim_frac, plain.kept_counts, plain.kept_mask, plain.rounds_changed) == (None,) * 4


def test_cli_flags_defaults_and_refusals(capsys):
    from miclip import clean_testset as C
    a = C.parse_args(["score", "cache", "out.csv"])
    assert (a.method, a.k_mode, a.k_fixed, a.k_max, a.min_samples_per_proto, a.random_state,
            a.n_init, a.max_iter) == ("single", "heuristic", 2, 4, 15, 0, 10, 100)
    assert (a.trim_frac, a.trim_rounds, a.kmeans) == (None, 1, "sklearn")
    assert str(a.cache_dir) == "cache" and str(a.output) == "out.csv"
    a = C.parse_args(
        ["score", "c", "o", "--method", "multi", "--k-mode", "fixed", "--k-fixed", "3", "--k-max",
         "5", "--min-samples-per-proto", "7", "--random-state", "9", "--n-init", "2",
         "--max-iter", "11", "--kmeans", "device"])
    assert (a.method, a.k_mode, a.k_fixed, a.k_max, a.min_samples_per_proto, a.random_state,
            a.n_init, a.max_iter, a.kmeans, a.trim_frac, a.trim_rounds) == (
        "multi", "fixed", 3, 5, 7, 9, 2, 11, "device", None, 1)
    a = C.parse_args(["score", "c", "o", "--trim-frac", "0.2", "--trim-rounds", "3"])
    assert (a.method, a.trim_frac, a.trim_rounds, a.kmeans) == ("single", 0.2, 3, "sklearn")
    assert C.parse_args(["score", "c", "o", "--method", "multi"]).kmeans == "sklearn"
    with pytest.raises(NotImplementedError, match="`select` is not implemented yet"):
        C.main(["select", "scores.csv", "rule.json", "out.csv"])
    with pytest.raises(NotImplementedError, match="`materialize` is not implemented yet"):
        C.main(["materialize", "imgs", "index.csv", "keep.csv", "out", "--invert", "--no-symlink"])
    for bad in (["score", "c", "o", "--method", "both"], ["score", "c"], [],
                ["score", "c", "o", "--method", "multi", "--kmeans", "host"],
                # a flag the chosen method would ignore is refused, not dropped
                ["score", "c", "o", "--method", "multi", "--trim-frac", "0.1"],
                ["score", "c", "o", "--method", "multi", "--trim-rounds", "2"],
                ["score", "c", "o", "--kmeans", "device"],
                ["score", "c", "o", "--kmeans", "sklearn"],
                ["score", "c", "o", "--trim-rounds", "2"]):
        with pytest.raises(SystemExit):
            C.main(bad)
    err = capsys.readouterr().err
    assert "--method single only" in err and "--method multi only" in err
    assert "--trim-rounds needs --trim-frac" in err


def test_cli_score_reports_a_missing_cache_before_any_device_work(tmp_path):
    from miclip import clean_testset as C
    with pytest.raises(FileNotFoundError, match="Missing cache file"):
        C.main(["score", str(tmp_path), str(tmp_path / "out.csv"), "--trim-frac", "0.1"])


@pytest.mark.parametrize("D,seed,f", MASK_CASES)
def test_gap_precondition_of_the_gpu_mask_test(D, seed, f):
    x, lab, _ = T.planted_case(seed, D=D)
    r, _, _, _ = _run(x, lab, f, rounds=ROUNDS)
    r32, _, _, _ = _run(x, lab, f, rounds=ROUNDS, dtype=np.float32)
    if D == 1:
        assert set(np.abs(r["sims"]).tolist()) <= {1.0} and np.array_equal(r32["sims"], r["sims"])
    else:
        assert r["min_gap"] >= GAP_MIN, r["min_gap"]
    assert np.array_equal(r32["keep"], r["keep"]) and r32["changed"] == r["changed"]
    if D == 64 and f == 0.1:
        assert r["changed"] == [29, 0, 0, 0] and 1.75e-3 <= r["min_gap"] <= 4.15e-3
    if D == 64 and f == 0.34:
        assert r["changed"] == {0: [101, 4, 0, 0], 1: [101, 2, 0, 0], 4: [101, 4, 2, 0]}[seed]


# ------------------------------------------------------------------ C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    import os
    import subprocess
    from miclip import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        subprocess.run(["make", "-C", root, "-j", "8"], check=True)
    return _lib.load_library()


def _p():
    """A non-NULL pointer that is never dereferenced (validation comes first)."""
    import ctypes
    return ctypes.c_void_p(64)


def _trim_call(lib, *, K=2, N=6, D=4, rounds=1, null=None):
    names = ["x", "order", "offsets", "cls", "drop", "sums", "centroids", "keep", "sims", "changed"]
    a = {n: (None if n == null else _p()) for n in names}
    return lib.miclip_trimmed_centroids(a["x"], a["order"], a["offsets"], a["cls"], a["drop"], K, N,
                                        D, rounds, 1e-12, a["sums"], a["centroids"], a["keep"],
                                        a["sims"], a["changed"], None)


def _rank_call(lib, *, K=2, N=6, null=None):
    names = ["values", "order", "offsets", "rank_out"]
    a = {n: (None if n == null else _p()) for n in names}
    return lib.miclip_segment_rank(a["values"], a["order"], a["offsets"], K, N, a["rank_out"], None)


def test_entry_points_are_exported_and_refuse_bad_arguments_before_any_launch(lib):
    from miclip import _lib, outliers
    for s in ("miclip_segment_rank", "miclip_trimmed_centroids"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    assert lib.miclip_abi_version() == 10 == _lib.ABI_VERSION
    over = outliers._TRIM_MAX_CLASS_ROWS + 1
    for kw, word in (({"rounds": 0}, b"rounds"), ({"rounds": 9}, b"rounds"), ({"K": 0}, b"K must"),
                     ({"K": 65536}, b"K must"), ({"N": 0}, b"N must"), ({"D": 0}, b"D must"),
                     ({"N": over}, b"largest supported class"), ({"null": "drop"}, b"drop"),
                     ({"null": "keep"}, b"keep"), ({"null": "changed"}, b"changed")):
        assert _trim_call(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())
    for kw, word in (({"K": 0}, b"K must"), ({"N": 0}, b"N must"),
                     ({"N": over}, b"largest supported class"), ({"null": "values"}, b"values"),
                     ({"null": "rank_out"}, b"rank_out")):
        assert _rank_call(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())
    assert outliers._TRIM_MAX_ROUNDS == 8 and outliers._TRIM_TILE == 1024


def test_a_cache_larger_than_one_call_goes_through_class_groups(monkeypatch):
    """More rows than one call takes: classes are packed into groups, each group is one
    call on its own rows, and the pieces are those of one call over everything."""
    from miclip import outliers
    assert outliers._trim_groups([5, 1, 4, 6, 2, 9], 10) == [[0, 1, 2], [3, 4], [5]]
    assert outliers._trim_groups([3, 3], 10) == [[0, 1]]
    assert outliers._trim_groups([10, 10], 10) == [[0], [1]]
    x, lab, _ = T.planted_case(3, D=8)
    _, inv, K = T.layout(lab)
    drop = T.drop_counts(np.bincount(inv), 0.2).astype(np.int32)
    calls = []

    def fake(x, inv, K, drop, rounds, eps):
        calls.append((x.shape[0], K))
        r = T.trimmed_centroids(x.numpy(), inv, K, drop, rounds, eps)
        return {"centroids": torch.from_numpy(r["centroids"].astype(np.float32)),
                "keep": torch.from_numpy(r["keep"].astype(np.uint8)),
                "changed": torch.tensor(r["changed"], dtype=torch.int32),
                "counts": np.bincount(inv, minlength=K)}
    monkeypatch.setattr(outliers, "_trimmed_centroids", fake)
    whole = outliers._trimmed_centroids_grouped(torch.from_numpy(x), inv, K, drop, 3, 1e-12)
    assert calls == [(len(x), K)]
    parts = outliers._trimmed_centroids_grouped(torch.from_numpy(x), inv, K, drop, 3, 1e-12,
                                                limit=260)
    sizes = np.bincount(inv).tolist()                    # [3, 257, 1, 40] for labels 2, 5, 7, 11
    assert calls[1:] == [(sizes[0] + sizes[1], 2), (sizes[2] + sizes[3], 2)]
    for name in ("centroids", "keep", "changed"):
        assert torch.equal(whole[name], parts[name]), name
    assert parts["counts"].tolist() == sizes


def test_a_class_over_the_limit_is_refused_by_name_on_the_host(monkeypatch):
    from miclip import outliers
    monkeypatch.setattr(outliers, "_TRIM_MAX_CLASS_ROWS", 3)
    with pytest.raises(ValueError, match="class 0 has 4"):
        _scorer().compute_centroids(trim_frac=0.1)
