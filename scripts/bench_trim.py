#!/usr/bin/env python3
"""Time the trimmed class centroids (csrc/trim.hip, miclip_trimmed_centroids) against a
torch restatement on the same GPU (per-class argsort and index_add_) and against the
float64 numpy reference of tests/_trim_ref.py on the host.

    python scripts/bench_trim.py [--iters 50] [--warmup 5] [--out FILE]

Shapes: 1 398 and 4 200 unit rows x 768 in 20 classes of uneven size, trim_frac = 0.1,
1 and 4 rounds; one more record puts all 4 200 rows into one class (the rank kernel's
largest n^2). Device times are device events around `iters` back-to-back calls on
pre-uploaded inputs after `warmup` untimed ones, the median of 5 such windows, per
call; the numpy time is a host clock, best of 3. Each record also reports whether the
three kept masks agree, and the per-piece device times of one C call taken the same
way: the plain centroid (miclip_class_centroids), the rank kernel alone
(miclip_segment_rank), and the cost of one more round ((t_4 - t_1) / 3). One JSON line
per record, by default into profiles/outliers/bench_trim.jsonl. With --profile the
script only runs `iters` calls of the first 4-round shape, for a kernel trace taken
around it. Not part of bench.py.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_rows(n, D, classes, seed):
    """Unit rows around `classes` directions, class sizes uneven, 8 % per class pointing away."""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.full(classes, 4.0))
    inv = np.sort(rng.choice(classes, n, p=w))
    inv[:classes] = np.arange(classes)              # no empty class
    inv = np.sort(inv)
    dirs = rng.standard_normal((classes, D))
    x = dirs[inv] + 0.6 * rng.standard_normal((n, D))
    for k in range(classes):
        idx = np.flatnonzero(inv == k)
        m = int(0.08 * len(idx))
        x[idx[:m]] = -dirs[k] + 2.0 * rng.standard_normal((m, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    p = rng.permutation(n)
    return x[p].astype(np.float32), inv[p].astype(np.int64)


def event_time(fn, iters, warmup, windows=5):
    """Median over `windows` of (device time of `iters` calls) / iters, in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


class Problem:
    def __init__(self, x, inv, K, f, dev):
        from miclip import _lib
        self.lib, self._lib = _lib.load_library(), _lib
        self.N, self.D, self.K, self.dev = x.shape[0], x.shape[1], K, dev
        self.x_h, self.inv_h = x, inv
        counts = np.bincount(inv, minlength=K)
        self.drop_h = np.asarray([int(np.floor(f * int(c))) for c in counts], np.int32)
        order = np.argsort(inv, kind="stable").astype(np.int32)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(dev)   # noqa: E731
        self.x, self.order, self.offsets = up(x, np.float32), up(order, np.int32), up(offsets, np.int32)
        self.cls, self.drop = up(inv, np.int32), up(self.drop_h, np.int32)
        self.inv_l = self.cls.long()
        self.sums = torch.empty(K, self.D, device=dev)
        self.cent = torch.empty(K, self.D, device=dev)
        self.keep = torch.empty(self.N, device=dev, dtype=torch.uint8)
        self.sims = torch.empty(self.N, device=dev)
        self.changed = torch.empty(8, device=dev, dtype=torch.int32)
        self.rank = torch.empty(self.N, device=dev, dtype=torch.int32)
        self.class_idx = [torch.from_numpy(np.flatnonzero(inv == k)).to(dev) for k in range(K)]
        self.counts_f = up(np.maximum(counts - self.drop_h, 1), np.float32)
        self.counts0_f = up(np.maximum(counts, 1), np.float32)

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr())

    def device(self, rounds):
        p, s = self._p, self._lib.stream_handle(self.dev)
        self._lib.check(self.lib.miclip_trimmed_centroids(
            p(self.x), p(self.order), p(self.offsets), p(self.cls), p(self.drop), self.K, self.N,
            self.D, rounds, 1e-12, p(self.sums), p(self.cent), p(self.keep), p(self.sims),
            p(self.changed), s), "miclip_trimmed_centroids")

    def plain(self):
        p, s = self._p, self._lib.stream_handle(self.dev)
        self._lib.check(self.lib.miclip_class_centroids(
            p(self.x), p(self.order), p(self.offsets), self.K, self.D, 1e-12, p(self.sums),
            p(self.cent), s), "miclip_class_centroids")

    def rank_only(self):
        p, s = self._p, self._lib.stream_handle(self.dev)
        self._lib.check(self.lib.miclip_segment_rank(
            p(self.sims), p(self.order), p(self.offsets), self.K, self.N, p(self.rank), s),
            "miclip_segment_rank")

    def torch_restatement(self, rounds):
        """The same recipe in torch ops on the device: index_add_ sums, a stable argsort per
        class (a stable ascending sort of rows in sample order is the (s, index) key)."""
        F = torch.nn.functional
        sums = torch.zeros(self.K, self.D, device=self.dev).index_add_(0, self.inv_l, self.x)
        cent = F.normalize(sums / self.counts0_f[:, None], dim=1, eps=1e-12)
        keep = None
        for _ in range(rounds):
            s = (self.x * cent.index_select(0, self.inv_l)).sum(dim=1)
            keep = torch.ones(self.N, device=self.dev, dtype=torch.bool)
            for k, idx in enumerate(self.class_idx):
                m = int(self.drop_h[k])
                if m:
                    o = torch.argsort(s.index_select(0, idx), stable=True)
                    keep[idx.index_select(0, o[:m])] = False
            rows = keep.nonzero().flatten()
            sums = torch.zeros(self.K, self.D, device=self.dev).index_add_(
                0, self.inv_l.index_select(0, rows), self.x.index_select(0, rows))
            cent = F.normalize(sums / self.counts_f[:, None], dim=1, eps=1e-12)
        return cent, keep


def record(name, n, D, K, f, rounds_list, a, dev, seed):
    import _trim_ref as T
    x, inv = make_rows(n, D, K, seed)
    pr = Problem(x, inv, K, f, dev)
    recs = []
    t_dev = {}
    for rounds in rounds_list:
        t_dev[rounds] = event_time(lambda: pr.device(rounds), a.iters, a.warmup)
        t_torch = event_time(lambda: pr.torch_restatement(rounds), max(a.iters // 10, 3), 2)
        pr.device(rounds)
        keep_d = pr.keep.cpu().numpy().astype(bool)
        cent_d = pr.cent.cpu().numpy()
        cent_t, keep_t = pr.torch_restatement(rounds)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            ref = T.trimmed_centroids(x, inv, K, pr.drop_h, rounds)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        recs.append({
            "workload": name, "rows": n, "D": D, "classes": K, "largest_class": int(np.bincount(inv).max()),
            "trim_frac": f, "rounds": rounds, "iters": a.iters, "warmup": a.warmup,
            "device_us": round(t_dev[rounds][0], 2), "device_us_min_max": [round(v, 2) for v in t_dev[rounds][1:]],
            "torch_us": round(t_torch[0], 2), "torch_us_min_max": [round(v, 2) for v in t_torch[1:]],
            "numpy_f64_us": round(best * 1e6, 1),
            "torch_over_device": round(t_torch[0] / t_dev[rounds][0], 2),
            "numpy_over_device": round(best * 1e6 / t_dev[rounds][0], 2),
            "mask_equal_numpy": bool(np.array_equal(keep_d, ref["keep"])),
            "mask_equal_torch": bool(np.array_equal(keep_d, keep_t.cpu().numpy())),
            "centroid_max_err_vs_f64": float(np.abs(cent_d - ref["centroids"]).max()),
            "torch_centroid_max_err_vs_f64": float(np.abs(cent_t.cpu().numpy() - ref["centroids"]).max()),
            "min_gap_f64": ref["min_gap"], "changed": ref["changed"],
            "device": torch.cuda.get_device_name(0)})
    pieces = {"plain_centroids_us": round(event_time(pr.plain, a.iters, a.warmup)[0], 2),
              "segment_rank_us": round(event_time(pr.rank_only, a.iters, a.warmup)[0], 2)}
    if len(rounds_list) > 1:
        lo, hi = min(rounds_list), max(rounds_list)
        pieces["per_extra_round_us"] = round((t_dev[hi][0] - t_dev[lo][0]) / (hi - lo), 2)
    for r in recs:
        r.update(pieces)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outliers", "bench_trim.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda", 0)
    if a.profile:
        x, inv = make_rows(4200, 768, 20, 2)
        pr = Problem(x, inv, 20, 0.1, dev)
        for _ in range(a.iters):
            pr.device(4)
        torch.cuda.synchronize()
        return
    lines = []
    lines += record("trimmed_centroids", 1398, 768, 20, 0.1, (1, 4), a, dev, seed=1)
    lines += record("trimmed_centroids", 4200, 768, 20, 0.1, (1, 4), a, dev, seed=2)
    lines += record("trimmed_centroids_one_class", 4200, 768, 1, 0.1, (1, 4), a, dev, seed=3)
    text = "\n".join(json.dumps(r) for r in lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
