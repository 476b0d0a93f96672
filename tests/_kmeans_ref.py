"""float64 numpy yardstick of the device k-means (csrc/kmeans.hip): the k-means++
seeding rules of miclip_kmeans_seed and scikit-learn's Lloyd loop as
miclip_kmeans_lloyd restates it. tests/test_kmeans_ref.py holds the Lloyd part
against scikit-learn itself; the GPU tests compare the kernels with this file.

Lloyd rules (sklearn.cluster._kmeans._kmeans_single_lloyd, dense, unit weights):
  E-step   argmin_j |x - c_j|^2, lowest index on a tie;
  M-step   cluster means;
  empty    in ascending cluster order an empty cluster takes the row farthest from
           its own (old) centre, the next one the next farthest, lowest row among
           equals; the row leaves its old cluster's sum and count;
  stop     labels equal the previous iteration's (strict), else
           sum |c_new - c_old|^2 <= tol; after a non-strict exit one more E-step;
  inertia  sum |x - c_label|^2.
"""
from dataclasses import dataclass

import numpy as np

SLOTS = 16


def planted(n, D, k, seed, noise=0.15):
    """n unit-norm fp32 rows in k tight modes: noise / sqrt(D) Gaussian around k
    random unit directions, modes dealt round-robin then shuffled. Returns (X, mode)."""
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((k, D))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    mode = rng.permutation(np.arange(n) % k)
    x = dirs[mode] + rng.standard_normal((n, D)) * (noise / np.sqrt(D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), mode


def tol_of(x, rel=1e-4):
    """scikit-learn's scaled tolerance: rel * mean over columns of the column variance."""
    return float(rel * np.mean(np.var(np.asarray(x, np.float64), axis=0)))


def sqdist(x, c):
    """[n, k] squared distances from direct differences, float64."""
    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    for j in range(c.shape[0]):
        out[:, j] = ((x - c[j]) ** 2).sum(axis=1)
    return out


def assign(x, c):
    """(labels, own d^2, gap = second-nearest minus nearest d^2, second label)."""
    d2 = sqdist(x, c)
    lab = np.argmin(d2, axis=1)            # first minimum
    rows = np.arange(d2.shape[0])
    own = d2[rows, lab]
    rest = d2.copy()
    rest[rows, lab] = np.inf
    second = np.argmin(rest, axis=1)
    return lab, own, rest[rows, second] - own, second


@dataclass
class Fit:
    centres: np.ndarray
    labels: np.ndarray
    inertia: float
    n_iter: int
    strict: bool
    min_gap: float
    relocated: int


def lloyd(x, c0, max_iter, tol):
    x = np.asarray(x, np.float64)
    c = np.array(c0, np.float64)
    n, k = x.shape[0], c.shape[0]
    old = np.full(n, -1)
    strict, min_gap, n_iter, relocated = False, np.inf, 0, 0
    lab = old
    for it in range(int(max_iter)):
        lab, own, gap, _ = assign(x, c)
        min_gap = min(min_gap, float(gap.min()))
        sums = np.zeros_like(c)
        for j in range(k):
            sums[j] = x[lab == j].sum(axis=0)
        cnt = np.bincount(lab, minlength=k).astype(np.int64)
        empty = np.flatnonzero(cnt == 0)
        if empty.size:
            far = np.lexsort((np.arange(n), -own))     # largest distance first, lowest row on ties
            for t, j in enumerate(empty):
                r = far[t]
                sums[lab[r]] -= x[r]
                sums[j] = x[r]
                cnt[j] = 1
                cnt[lab[r]] -= 1
                relocated += 1
        new = sums / cnt[:, None]
        shift = float(((new - c) ** 2).sum())
        c = new
        n_iter = it + 1
        if np.array_equal(lab, old):
            strict = True
            break
        if shift <= tol:
            break
        old = lab
    if not strict:
        lab, _, gap, _ = assign(x, c)
        min_gap = min(min_gap, float(gap.min()))
    inertia = float(((x - c[lab]) ** 2).sum())
    return Fit(c, lab, inertia, n_iter, strict, min_gap, relocated)


def first_pick(u0, n):
    """Pick 0: min(floor(u0 * n), n - 1), the product taken in fp32 as the kernel does."""
    return int(min(max(np.floor(np.float32(u0) * np.float32(n)), 0), n - 1))


def seed_mind(x, chosen):
    """mind[j] = min over the chosen rows of |x_j - x_c|^2, float64."""
    x = np.asarray(x, np.float64)
    return sqdist(x, x[list(chosen)]).min(axis=1)


def seed(x, k, u):
    """k-means++ picks by the rules of miclip_kmeans_seed, float64 sums."""
    n = x.shape[0]
    picks = [first_pick(u[0], n)]
    for t in range(1, k):
        mind = seed_mind(x, picks)
        total = mind.sum()
        if total == 0:
            picks.append(min(set(range(n)) - set(picks)))
            continue
        cum = np.cumsum(mind)
        hit = np.flatnonzero(cum > np.float64(u[t]) * total)
        picks.append(int(hit[0]) if hit.size else int(np.flatnonzero(mind > 0)[-1]))
    return picks
