#!/usr/bin/env python3
"""Time miclip.embed_vis.tsne (exact t-SNE on the device, csrc/tsne.hip) against
sklearn.manifold.TSNE with the reference's arguments (feat_vis.py:150-157: perplexity 30,
cosine, PCA init, random_state 1; scikit-learn's default Barnes-Hut method) on the host's
threads, in the same process, alternating round by round.

    python scripts/bench_tsne.py [--rounds 3] [--sizes 1398,4200] [--dim 768] [--out FILE]

Workload: N unit-norm rows around 20 planted directions, D = 768, 1 000 iterations. Times
are host clock around one call (the device call ends in its last read-back), after one
untimed device warm-up; the best round counts. A second record per size times
miclip_tsne_run alone: one long call against a short one, (t_long - t_short) / (steps
difference), and the affinities call. One JSON line per record. Not part of bench.py.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))


def make_rows(n, d, seed, modes=20, noise=0.9):
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((modes, d))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    x = dirs[rng.integers(0, modes, n)] + rng.standard_normal((n, d)) * (noise / d ** 0.5)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def fit_record(x, rounds):
    from sklearn.manifold import TSNE, trustworthiness

    from miclip import embed_vis
    n, d = x.shape
    embed_vis.tsne(x, max_iter=250)                      # warm-up (library load, allocator)
    dev_s, skl_s, dev, skl = [], [], None, None
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = embed_vis.tsne(x, perplexity=30.0, metric="cosine", init="pca", seed=1)
        torch.cuda.synchronize()
        dev_s.append(round(time.perf_counter() - t0, 4))
        t0 = time.perf_counter()
        skl = TSNE(n_components=2, perplexity=30.0, metric="cosine", init="pca", random_state=1)
        ys = skl.fit_transform(x)
        skl_s.append(round(time.perf_counter() - t0, 4))
    sub = np.random.default_rng(0).permutation(n)[:min(n, 1500)]

    def trust(y):
        return round(float(trustworthiness(x[sub], y[sub], n_neighbors=10, metric="cosine")), 4)
    return {"workload": "tsne_fit", "N": n, "D": d, "perplexity": 30.0, "metric": "cosine",
            "max_iter": 1000, "rounds": rounds, "threads": torch.get_num_threads(),
            "device_s": dev_s, "sklearn_barnes_hut_s": skl_s,
            "device_best_s": min(dev_s), "sklearn_best_s": min(skl_s),
            "sklearn_over_device": round(min(skl_s) / min(dev_s), 2),
            "device_kl": round(dev.kl_divergence, 5), "sklearn_kl": round(float(skl.kl_divergence_), 5),
            "device_n_iter": dev.n_iter, "sklearn_n_iter": int(skl.n_iter_),
            "device_trustworthiness": trust(dev.coords), "sklearn_trustworthiness": trust(ys),
            "device": torch.cuda.get_device_name(0)}


def kernel_record(x, short=100, long=1100):
    from miclip import _lib, embed_vis
    lib = _lib.load_library()
    n, d = x.shape
    dev = torch.device("cuda")
    xd = torch.from_numpy(x).to(dev)
    best_aff = None
    for _ in range(4):                                   # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P, _, _ = embed_vis.affinities(xd, perplexity=30.0, metric="cosine")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best_aff = dt if best_aff is None else min(best_aff, dt)
    y0 = torch.from_numpy(embed_vis.random_init(n, 1)).to(dev)
    scratch = torch.empty(int(lib.miclip_tsne_scratch_bytes(n)), device=dev, dtype=torch.uint8)
    stats = torch.zeros(4, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {}
    for name, steps in (("short", short), ("long", long)):
        best = None
        for _ in range(4):
            y, u, g = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(lib.miclip_tsne_run(p(P), n, p(y), p(u), p(g), steps, 1.0, 0.8, 200.0,
                                           0.01, 0, p(scratch), p(stats),
                                           _lib.stream_handle(dev)), "miclip_tsne_run")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out[name] = best
    return {"workload": "tsne_kernels", "N": n, "D": d, "affinities_s": round(best_aff, 6),
            "run_short_steps": short, "run_short_s": round(out["short"], 6),
            "run_long_steps": long, "run_long_s": round(out["long"], 6),
            "us_per_iteration": round((out["long"] - out["short"]) / (long - short) * 1e6, 2),
            "p_bytes": n * n * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="1398,4200")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = []
    for n in (int(s) for s in a.sizes.split(",")):
        x = make_rows(n, a.dim, seed=n)
        lines.append(fit_record(x, a.rounds))
        lines.append(kernel_record(x))
        print(json.dumps(lines[-2]))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
