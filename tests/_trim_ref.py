"""Float64 numpy restatement of the trimmed class centroids (DESIGN "Trimmed class
centroids"), the yardstick of tests/test_gpu_trim.py. tests/test_trim_ref.py holds it
against hand-made cases.

Definition. x [N, D] are the rows as the scorer sees them (unit rows, fp32 values), inv
[N] the class index of each row, drop[k] = floor(trim_frac * n_k) an integer per class.
    c_0 = normalize(sum of the class's rows in ascending sample order / n_k)
    round t = 1..T:
        s_i       = x_i . c_{t-1}[inv[i]]
        r_i       = 0-based rank of i among ALL rows of its class by the key
                    (s ascending, sample index ascending)
        keep_t[i] = r_i >= drop[class]
        c_t       = normalize(sum of the kept rows in ascending sample order / kept count)
        changed[t-1] = #{i : keep_t[i] != keep_{t-1}[i]},  keep_0 = all ones
normalize(v) = v / max(|v|, eps). `dtype` chooses the arithmetic: float64 is the
reference, float32 the "same recipe in the device's precision" whose own error against
float64 sets the tests' bars.
"""
import math

import numpy as np


def drop_counts(counts, trim_frac):
    """drop[k] = floor(trim_frac * n_k) in Python float64."""
    return np.asarray([int(math.floor(float(trim_frac) * int(n))) for n in counts], np.int64)


def segment_rank(values, inv):
    """rank[i] = #{j in class of i : (values[j], j) < (values[i], i)}; -0 and +0 tie."""
    values = np.asarray(values)
    inv = np.asarray(inv)
    rank = np.zeros(len(values), np.int64)
    for k in np.unique(inv):
        idx = np.flatnonzero(inv == k)
        v = values[idx] + 0.0                      # -0 + 0 = +0: the two zeros compare equal
        rank[idx[np.lexsort((idx, v))]] = np.arange(len(idx))
    return rank


def _normalize(v, eps):
    n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return v / np.maximum(n, v.dtype.type(eps))


def class_sums(x, inv, K, keep):
    sums = np.zeros((K, x.shape[1]), x.dtype)
    kept = np.zeros(K, np.int64)
    for k in range(K):
        sel = (inv == k) & keep
        kept[k] = int(sel.sum())
        if kept[k]:
            sums[k] = x[sel].sum(axis=0)
    return sums, kept


def trimmed_centroids(x, inv, K, drop, rounds, eps=1e-12, dtype=np.float64):
    """Returns {"centroids" [K, D] = c_T, "plain" = c_0, "sums" [K, D], "keep" bool [N],
    "sims" [N] (round T, against c_{T-1}), "changed" [T], "kept_counts" [K],
    "min_gap": the smallest s_(m+1) - s_(m) over every class cut (0 < drop < n_k) of
    every round, None when nothing is cut}."""
    x = np.asarray(x).astype(dtype)
    inv = np.asarray(inv, np.int64)
    drop = np.asarray(drop, np.int64)
    N = x.shape[0]
    keep = np.ones(N, bool)
    sums, kept = class_sums(x, inv, K, keep)
    cent = plain = _normalize(sums / np.maximum(kept, 1)[:, None].astype(dtype), eps)
    changed, gaps, sims = [], [], None
    for _ in range(int(rounds)):
        sims = (x * cent[inv]).sum(axis=1)
        new = np.ones(N, bool)
        for k in range(K):
            idx = np.flatnonzero(inv == k)
            m = int(min(max(drop[k], 0), max(len(idx) - 1, 0)))
            o = idx[np.lexsort((idx, sims[idx] + 0.0))]
            new[o[:m]] = False
            if 0 < m < len(idx):
                gaps.append(float(sims[o[m]] - sims[o[m - 1]]))
        changed.append(int((new != keep).sum()))
        keep = new
        sums, kept = class_sums(x, inv, K, keep)
        cent = _normalize(sums / np.maximum(kept, 1)[:, None].astype(dtype), eps)
    return {"centroids": cent, "plain": plain, "sums": sums, "keep": keep, "sims": sims,
            "changed": changed, "kept_counts": kept, "min_gap": min(gaps) if gaps else None}


# ------------------------------------------------------------------ the shared generator
SIZES, LABELS, DIM = (1, 3, 40, 257), (7, 2, 11, 5), 64
GAP_MIN = 1e-4      # smallest float64 cut gap the exact kept-mask test accepts
ROUNDS = 4
# (D, seed, trim_frac) of the exact kept-mask test; D = 1 has similarities of exactly
# +-1 (every product is exact in fp32), so there the tie rule alone decides
MASK_CASES = ([(64, s, 0.1) for s in range(5)] + [(64, s, 0.34) for s in (0, 1, 4)] +
              [(D, s, f) for D, s in ((1, 0), (3, 0), (3, 1), (65, 1), (65, 2), (768, 4))
               for f in (0.1, 0.34)])


def planted_case(seed, D=DIM, sizes=SIZES, labels=LABELS, unit=True):
    """Rows = class direction + 0.6 N(0,1); the first 8 % of each class replaced by
    -direction + 2 N(0,1) (the planted outliers); rows permuted with default_rng(seed) and
    stored as fp32 (unit: scaled to unit length in float64 first, so the scorer takes
    them as they are). Returns (x fp32 [N, D], labels int64 [N], planted bool [N])."""
    r = np.random.default_rng(seed)
    K = len(sizes)
    lab = np.repeat(np.asarray(labels, np.int64), sizes)
    dirs = r.standard_normal((K, D))
    x = np.concatenate([dirs[i] + 0.6 * r.standard_normal((n, D)) for i, n in enumerate(sizes)])
    planted = np.zeros(len(x), bool)
    for i, (lo, n) in enumerate(zip(np.cumsum([0] + list(sizes[:-1])), sizes)):
        m = int(0.08 * n)
        x[lo:lo + m] = -dirs[i] + 2.0 * r.standard_normal((m, D))
        planted[lo:lo + m] = True
    p = r.permutation(len(x))
    x, lab, planted = x[p], lab[p], planted[p]
    if unit:
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), lab, planted


def layout(labels):
    """(uniq, inv int64 [N], K) as SingleCentroidScorer._classes builds them."""
    uniq, inv = np.unique(np.asarray(labels), return_inverse=True)
    return uniq, inv.astype(np.int64), len(uniq)
