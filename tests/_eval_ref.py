"""fp64 numpy restatement of the validation metrics, CPU only: the yardstick of
tests/test_gpu_evaluation.py and tests/test_evaluation.py. It touches nothing under
test. Line numbers are the reference's (methods/PEFT_openclip.py `_run_validation`,
aihab_utils/evaluation.py, methods/utils.py).
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluation.npz")


def load_golden():
    z = np.load(GOLDEN)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d["meta"]).decode())
    return d


def topk(z, k):
    """Indices of the k largest per row, value descending, the lower index first
    among equals (torch.topk(sorted=True) for distinct values; utils.py:16-21): a
    stable argsort of the negated values."""
    z = np.asarray(z)
    return np.argsort(-z, axis=1, kind="stable")[:, :k]


def row_ce(z, y):
    """CrossEntropyLoss per row in fp64 (PEFT_openclip.py:62, 93): logsumexp(z) - z[y]."""
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
    return lse - z[np.arange(len(y)), np.asarray(y)]


def softmax(z):
    """F.softmax(dim=1) in fp64 (evaluation.py:265)."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def top3_probs(z):
    """(top-3 indices, their softmax probabilities), evaluation.py:261-268."""
    idx = topk(z, 3)
    return idx, np.take_along_axis(softmax(z), idx, axis=1)


def confusion(y, pred, k):
    """Counts [k, k], rows = true labels, columns = predictions."""
    cm = np.zeros((k, k), dtype=np.int64)
    np.add.at(cm, (np.asarray(y), np.asarray(pred)), 1)
    return cm


def hits(z, y, k):
    """Rows whose label is among the top k (cls_acc, utils.py:16-21; evaluation.py:206-214)."""
    k = min(k, np.asarray(z).shape[1])
    return int((topk(z, k) == np.asarray(y)[:, None]).any(axis=1).sum())


def aggregate(z, l3_to_l2, num_l2, reduce):
    """aggregate_logits_to_l2 (evaluation.py:92-142) in fp64, ascending L3 id."""
    z = np.asarray(z, dtype=np.float64)
    if reduce == "logsumexp":
        out = np.full((z.shape[0], num_l2), -np.inf)
        for l3, l2 in enumerate(l3_to_l2):
            out[:, l2] = np.logaddexp(out[:, l2], z[:, l3])
        return out
    out, counts = np.zeros((z.shape[0], num_l2)), np.zeros(num_l2)
    for l3, l2 in enumerate(l3_to_l2):
        out[:, l2] += z[:, l3]
        counts[l2] += 1
    return out / np.maximum(counts, 1) if reduce == "mean" else out


def weighted_f1(cm):
    """torcheval MulticlassF1Score(average="weighted") from counts: sum_c support_c / N *
    2 TP_c / (pred_c + support_c), 0 / 0 = 0 (PEFT_openclip.py:65, 122)."""
    cm = np.asarray(cm, dtype=np.float64)
    total = 0.0
    for c in range(cm.shape[0]):
        den = cm[:, c].sum() + cm[c].sum()
        if den > 0:
            total += cm[c].sum() * 2.0 * cm[c, c] / den
    return total / cm.sum()


def pairs_from_confusion(cm):
    """(y_true, y_pred) lists that have the confusion counts cm."""
    cm = np.asarray(cm)
    yt, yp = [], []
    for t in range(cm.shape[0]):
        for p in range(cm.shape[1]):
            yt += [t] * int(cm[t, p])
            yp += [p] * int(cm[t, p])
    return np.array(yt, dtype=np.int64), np.array(yp, dtype=np.int64)
