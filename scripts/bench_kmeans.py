#!/usr/bin/env python3
"""Time MultiPrototypeScorer.compute_prototypes: the device k-means backend
(csrc/kmeans.hip, two launches for every class and restart) against the
scikit-learn backend (one host fit per class), in the same process, the two
alternating round by round, each round under its own time limit.

    python scripts/bench_kmeans.py [--rounds 3] [--classes 20] [--rows 3000] [--out FILE]

Workload: `classes` classes of `rows` unit-norm rows each, D = 768, six loose modes
per class, heuristic k (with the default k_max = 4 that is k = 4), n_init = 10.
Times are host clock around one compute_prototypes call that ends in a device
synchronise, after one untimed warm-up of the device path; the best round counts.
A second record times the Lloyd launch alone at n_c = `rows` for a fixed number
of iterations (tol < 0, so only unchanged labels could stop it early) and reports
the time per iteration actually run. One JSON line per record. Not part of bench.py.
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))


class RoundTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise RoundTimeout()


def make_cache(classes, rows, D, seed, noise=0.9, modes=6):
    rng = np.random.default_rng(seed)
    xs, labs = [], []
    for c in range(classes):
        dirs = rng.standard_normal((modes, D))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        x = dirs[rng.integers(0, modes, rows)] + rng.standard_normal((rows, D)) * (noise / D ** 0.5)
        xs.append(x / np.linalg.norm(x, axis=1, keepdims=True))
        labs.append(np.full(rows, c))
    perm = rng.permutation(classes * rows)
    x = np.concatenate(xs)[perm].astype(np.float32)
    lab = np.concatenate(labs)[perm]
    meta = pd.DataFrame({"file_name": [f"f{i:06d}" for i in range(len(x))],
                         "ground_truth_num_label": lab})
    return torch.from_numpy(x), torch.from_numpy(lab), meta


def timed(scorer, backend, limit_s):
    """Seconds of one compute_prototypes(kmeans=backend), None when over the limit."""
    scorer._prototypes = None
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(int(limit_s))
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = scorer.compute_prototypes(kmeans=backend)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    except RoundTimeout:
        return None, None
    finally:
        signal.alarm(0)


def lloyd_per_iteration(rows, D, k, iters, dev):
    """One class of `rows` unstructured rows, one problem: Lloyd launch at max_iter = 1 and
    at max_iter = 1 + iters with tol < 0; (t_long - t_short) / (iterations run - 1)."""
    from miclip import outliers as O
    rng = np.random.default_rng(5)
    x = rng.standard_normal((rows, D))
    x = torch.from_numpy((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)).to(dev)
    inv = np.zeros(rows, np.int64)
    _, counts, layout = O._class_layout(x, inv, 1, 1e-12)
    table = O._kmeans_table(counts, [0], [k], 1, dev)
    u = torch.from_numpy(np.random.default_rng(6).random((1, 16), dtype=np.float32)).to(dev)
    tol = torch.full((1,), -1.0, device=dev)
    _, c0 = O._kmeans_seed(x, layout, table, u)
    out = {}
    for name, mi in (("short", 1), ("long", 1 + iters)):
        best = None
        for _ in range(4):       # the first pass is the warm-up
            cen = c0.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = O._kmeans_lloyd(x, layout, table, tol, mi, cen)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out[name] = (best, int(fit["n_iter"][0]))
    (ts, ns), (tl, nl) = out["short"], out["long"]
    return {"workload": "lloyd_per_iteration", "rows": rows, "D": D, "k": k,
            "launch_1_iter_s": round(ts, 6), "launch_long_s": round(tl, 6), "iters_long": nl,
            "us_per_iteration": round((tl - ts) / max(nl - ns, 1) * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds per timed call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from miclip.outliers import MultiPrototypeScorer
    assert torch.cuda.is_available(), "needs a HIP device"
    x, lab, meta = make_cache(a.classes, a.rows, a.dim, seed=1)
    sc = MultiPrototypeScorer(x, lab, meta)
    sc._get_normalized_embeddings()
    timed(sc, "device", a.limit)                      # warm-up (library load, allocator)
    dev_s, skl_s, res = [], [], {}
    for _ in range(a.rounds):
        for backend, acc in (("device", dev_s), ("sklearn", skl_s)):
            t, r = timed(sc, backend, a.limit)
            acc.append(None if t is None else round(t, 5))
            if r is not None:
                res[backend] = r
    fit = sc._kmeans_fit if "device" in res else None
    rec = {"workload": "compute_prototypes", "classes": a.classes, "rows": a.rows, "D": a.dim,
           "n_init": 10, "max_iter": 100, "rounds": a.rounds, "limit_s": a.limit,
           "k": sorted(set(res["device"].k_per_class.values())) if "device" in res else None,
           "device_s": dev_s, "sklearn_s": skl_s,
           "device": torch.cuda.get_device_name(0)}
    good_d = [t for t in dev_s if t is not None]
    good_s = [t for t in skl_s if t is not None]
    if good_d:
        rec["device_best_s"] = min(good_d)
    if good_s:
        rec["sklearn_best_s"] = min(good_s)
    if good_d and good_s:
        rec["sklearn_over_device"] = round(min(good_s) / min(good_d), 2)
    if fit is not None:
        n_it = fit["n_iter"].cpu().numpy()
        rec["problems"] = int(n_it.size)
        rec["n_iter_mean"] = round(float(n_it.mean()), 2)
        rec["n_iter_max"] = int(n_it.max())
    lines = [rec, lloyd_per_iteration(a.rows, a.dim, 4, 20, sc.device)]
    text = "\n".join(json.dumps(r) for r in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
