"""CPU: miclip.evaluation's surface and host logic -- F1 and MCC from confusion counts
against sklearn, the L2MetricsAccumulator mode / topk rules, the ClassificationTracker
tables, the C entry points' validation (before any device access), the golden fixture
against the fp64 restatement -- and that nothing computes without a device.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j", "8"], check=True)
    return _lib.load_library()


def test_import_and_surface_without_a_device():
    import miclip
    from miclip import evaluation as ev
    for name in ("run_validation", "evaluate_features", "Evaluator", "L2MetricsAccumulator",
                 "aggregate_logits_to_l2", "map_l3_targets_to_l2", "ClassificationTracker",
                 "weighted_f1", "mcc_from_confusion"):
        assert hasattr(ev, name), name
    assert miclip.run_validation is ev.run_validation
    assert miclip.evaluate_features is ev.evaluate_features
    assert "W&B" in ev.__doc__ and "draw_cm" in ev.__doc__       # out of scope, said so
    t = torch.tensor([0, 3, 1])
    assert ev.map_l3_targets_to_l2(t, [5, 6, 7, 8]).tolist() == [5, 8, 6]
    assert ev.map_l3_targets_to_l2(t, torch.tensor([5, 6, 7, 8])).tolist() == [5, 8, 6]


CMS = {
    "mixed": [[5, 1, 0], [2, 3, 1], [0, 0, 4]],
    "all_one_class": [[0, 0, 0], [0, 7, 0], [0, 0, 0]],               # MCC 0
    "one_predicted": [[0, 3, 0], [0, 4, 0], [0, 2, 0]],               # MCC 0
    "absent_and_never_predicted": [[3, 0, 1, 0], [0, 0, 0, 0], [2, 0, 2, 0], [1, 0, 1, 0]],
    "perfect": [[2, 0], [0, 5]],
    "all_wrong": [[0, 4], [3, 0]],
}


@pytest.mark.parametrize("name", sorted(CMS))
def test_f1_and_mcc_from_confusion_against_sklearn(name):
    from sklearn.metrics import f1_score, matthews_corrcoef
    from miclip.evaluation import mcc_from_confusion, weighted_f1
    cm = np.array(CMS[name])
    yt, yp = R.pairs_from_confusion(cm)
    assert np.array_equal(R.confusion(yt, yp, cm.shape[0]), cm)
    assert abs(weighted_f1(cm) - f1_score(yt, yp, average="weighted", zero_division=0)) <= 1e-12
    assert abs(weighted_f1(cm) - R.weighted_f1(cm)) <= 1e-12
    assert abs(mcc_from_confusion(cm) - matthews_corrcoef(yt, yp)) <= 1e-12
    if name in ("all_one_class", "one_predicted"):
        assert mcc_from_confusion(cm) == 0.0
    assert weighted_f1(np.zeros((3, 3))) == 0.0 and mcc_from_confusion(np.zeros((3, 3))) == 0.0


def test_l2_accumulator_mode_and_topk_rules():
    from miclip.evaluation import L2MetricsAccumulator
    a = L2MetricsAccumulator([0, 0, 1], 2, topk=(1, 3), mode="argmax")
    assert a.topk == (1,) and a.mode == "argmax" and a.reduce == "mean" and a.total_seen == 0
    b = L2MetricsAccumulator([0, 0, 1], 2, reduce="sum", topk=[1, 3], mode="logits",
                             return_confusion_matrix=True)
    assert b.topk == (1, 3) and b.num_l2 == 2 and b.return_confusion_matrix
    with pytest.raises(ValueError, match="Unsupported mode='softmax'. Expected 'argmax' or 'logits'."):
        L2MetricsAccumulator([0, 0, 1], 2, mode="softmax")


def test_classification_tracker_tables(tmp_path, capsys):
    from miclip.evaluation import TRACK_COLUMNS, ClassificationTracker
    t = ClassificationTracker(class_names=["heath", "bog", "fen"])
    meta = {"file_name": ["a.jpg", "b.jpg", "c.jpg"], "plot_word_label": ["bog", "fen", "heath"],
            "image_source": ["survey", "citizen", "survey"]}
    t.track_classification(torch.tensor([1, 0, 0]), torch.tensor([1, 2, 0]),
                           torch.tensor([[1, 0, 2], [0, 2, 1], [0, 1, 2]]),
                           torch.tensor([[.7, .2, .1], [.5, .3, .2], [.6, .3, .1]]), meta)
    mis, cor = t.frames()
    want = ["file_name", "ground_truth_num_label", "ground_truth_word_label", "predicted_label",
            "predicted_word_label", "dataset", "top3_label_1", "top3_prob_1", "top3_label_2",
            "top3_prob_2", "top3_label_3", "top3_prob_3"]            # evaluation.py:317-329
    assert list(TRACK_COLUMNS) == want
    assert list(mis.columns) == want and list(cor.columns) == want
    assert list(mis["file_name"]) == ["b.jpg"] and list(cor["file_name"]) == ["a.jpg", "c.jpg"]
    assert list(mis["predicted_word_label"]) == ["heath"] and list(mis["dataset"]) == ["citizen"]
    assert list(cor["top3_label_2"]) == [0, 1] and cor["top3_prob_1"].tolist() == \
        pytest.approx([.7, .6])
    assert t.misclassified[0]["top3_predictions"][2] == {"label": 1, "probability": pytest.approx(.2)}
    t.save_classification(tmp_path)
    assert sorted(os.listdir(tmp_path)) == ["correct.csv", "misclassified.csv"]
    assert open(tmp_path / "misclassified.csv").readline().strip().split(",") == want
    empty = ClassificationTracker()
    assert list(empty.frames()[0].columns) == want and len(empty.frames()[1]) == 0
    capsys.readouterr()
    empty.save_classification()
    assert capsys.readouterr().out.splitlines() == ["No misclassified samples",
                                                    "No correctly classified samples"]


def test_entry_points_validate_before_any_device_access(lib):
    """MICLIP_EINVAL for every limit of the issue, with null device pointers never read."""
    from miclip import _lib
    assert lib.miclip_eval_state_bytes(20, 8) == 8 * (8 + 20 * 20 + 8 * 8)
    assert lib.miclip_eval_state_bytes(1024, 1024) == 8 * (8 + 2 * 1024 * 1024)
    for C, L in ((2, 1), (1025, 1), (5, 0), (5, 6)):
        assert lib.miclip_eval_state_bytes(C, L) == 0
    assert lib.miclip_eval_reset(None, 5, 2, None) == -1
    assert lib.miclip_eval_reset(ctypes.c_void_p(4096), 2, 1, None) == -1
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected first
    ok_map, bad_map = (ctypes.c_int32 * 5)(0, 1, 1, 1, 0), (ctypes.c_int32 * 5)(0, 1, 2, 1, 0)

    def call(E=32, C=5, B=4, m=None, num_l2=1, mode=0, flags=0, dtype=_lib.MICLIP_F32, f=p):
        return lib.miclip_eval_batch(f, dtype, p, p, B, E, C, 100.0, m, num_l2, mode, flags, p, None,
                                     p, None, None, None, None, None, None, None)
    for kw in (dict(C=2), dict(C=1025), dict(E=24), dict(E=1040), dict(E=0), dict(B=0),
               dict(m=bad_map, num_l2=2, mode=_lib.MICLIP_EVAL_L2_SUM),
               dict(m=ok_map, num_l2=6, mode=_lib.MICLIP_EVAL_L2_MEAN),
               dict(m=ok_map, num_l2=0, mode=_lib.MICLIP_EVAL_L2_ARGMAX),
               dict(m=None, num_l2=2, mode=_lib.MICLIP_EVAL_L2_ARGMAX),
               dict(m=ok_map, num_l2=2, mode=_lib.MICLIP_EVAL_L2_NONE),
               dict(m=ok_map, num_l2=2, mode=5), dict(flags=2), dict(dtype=7),
               dict(f=ctypes.c_void_p(4100)), dict(f=None),
               dict(flags=_lib.MICLIP_EVAL_LOGITS_IN)):       # logits-in without logits
        assert call(**kw) == -1, kw
    assert lib.miclip_last_error()


def test_golden_fixture_against_the_fp64_restatement():
    """The recorded reference run and tests/_eval_ref.py agree (the yardstick is sound)."""
    g = R.load_golden()
    meta = g["meta"]
    assert (meta["n"], meta["E"], meta["C"], meta["batch"]) == (53, 64, 20, 16)
    assert meta["min_gap"] >= 1e-3 and "stand_in" in meta and len(g["l3_to_l2"]) == 20
    z, y = g["logits"].astype(np.float64), g["labels"]
    f = g["feats"].astype(np.float64)
    z64 = 100.0 * (f / np.linalg.norm(f, axis=1, keepdims=True)) @ g["text_weights"].astype(np.float64)
    assert np.abs(z - z64).max() < 1e-4
    assert np.array_equal(R.topk(z64, 3), g["top3"]) and np.array_equal(g["preds"], g["top3"][:, 0])
    m, num_l2 = [int(v) for v in g["l3_to_l2"]], meta["num_l2"]
    edges = list(range(0, 53, 16)) + [53]
    ce = R.row_ce(z64, y)
    loss = np.mean([ce[a:b].mean() for a, b in zip(edges[:-1], edges[1:])])
    for run in meta["runs"]:
        s = dict(zip(meta["scalars"], g[f"{run}_scalars"]))
        assert abs(s["loss"] - loss) < 1e-4
        assert s["top1"] == pytest.approx(R.hits(z64, y, 1) / 53, abs=1e-12)
        assert s["top3"] == pytest.approx(R.hits(z64, y, 3) / 53, abs=1e-12)
        cm = R.confusion(y, g["preds"], 20)
        assert np.array_equal(g[f"{run}_cm_stand_in"], cm)
        assert s["f1_stand_in"] == pytest.approx(R.weighted_f1(cm), abs=1e-6)
        mode, reduce = run.split("_")
        s2 = dict(zip(meta["l2_scalars"], g[f"{run}_l2_scalars"]))
        y2 = np.asarray(m)[y]
        if mode == "argmax":
            assert s2["top1"] == pytest.approx(float((np.asarray(m)[g["preds"]] == y2).mean()), abs=1e-12)
            assert np.isnan(s2["top3"])
        else:
            z2 = R.aggregate(z64, m, num_l2, reduce)
            assert np.abs(z2 - g[f"agg_{reduce}"]).max() < 1e-3
            assert s2["top1"] == pytest.approx(R.hits(z2, y2, 1) / 53, abs=1e-12)
            assert s2["top3"] == pytest.approx(R.hits(z2, y2, 3) / 53, abs=1e-12)
    assert len(g["track_mis__file_name"]) + len(g["track_cor__file_name"]) == 53


def test_every_call_raises_without_a_device(monkeypatch):
    from miclip import evaluation as ev
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    W, f, y = torch.randn(32, 5), torch.randn(4, 32), torch.tensor([0, 1, 2, 3])
    z = torch.randn(4, 5)

    class Stub(torch.nn.Module):
        def encode_image(self, x):
            return x
    acc = ev.L2MetricsAccumulator([0, 0, 1, 1, 1], 2, mode="logits")
    calls = [
        lambda: ev.Evaluator(W),
        lambda: ev.Evaluator(W, device="cpu"),
        lambda: ev.evaluate_features(f, y, W),
        lambda: ev.evaluate_features(f, y, W, batch_size=2, cls_track=True),
        lambda: ev.run_validation(Stub(), [(f, y)], W),
        lambda: ev.run_validation(Stub(), [(f, y)], W, "cpu"),
        lambda: ev.aggregate_logits_to_l2(z, [0, 0, 1, 1, 1], 2),
        lambda: acc.update(z, y),
        lambda: acc.compute(),
        lambda: ev.ClassificationTracker().top3_metrics(z, y),
    ]
    for i, fn in enumerate(calls):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
