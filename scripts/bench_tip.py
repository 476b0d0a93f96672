#!/usr/bin/env python3
"""Time one miclip.tip.search_hp_tip (the fused (beta, alpha) grid of csrc/tip.hip) against
the reference's loop (methods/utils.py:74-90 with cls_acc, :16-21) restated in torch on the
same device, in the same process, the two alternating round by round.

    python scripts/bench_tip.py [--rounds 5] [--out profiles/tip/bench_tip.jsonl]

Workload: Nq = 1 398 unit query rows around 20 planted directions, Nk in {320, 4 200} keys,
E in {512, 768}, C = 20, search_scale [7, 3] and search_step [200, 20] (the reference's
YAML names neither key; these are the values used here): 4 000 pairs. Features, keys and
values are fp16 in the torch loop, as the reference's fp16 model produces them; the device
path reads the same fp16 features and fp32 keys. Times are host clock around the whole
call, read-back included (the torch loop synchronises once per pair, the device path once
per search plus its host checks), after five untimed device calls and 200 untimed pairs of
the loop; the best round counts, and every round is recorded. The
per-kernel split of the device path is taken with device events around each C call, best
of 5. One JSON line per setting. Not part of bench.py.
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))

CFG = {"search_hp": True, "search_scale": [7, 3], "search_step": [200, 20]}


def make_data(Nq, Nk, E, C, seed):
    g = torch.Generator().manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(C, E, generator=g), dim=1)

    def around(lab, amount):
        x = dirs[lab] + amount * E ** -0.5 * torch.randn(len(lab), E, generator=g)
        return torch.nn.functional.normalize(x, dim=1)

    klab, qlab = torch.arange(Nk) % C, torch.randint(0, C, (Nq,), generator=g)
    return (around(qlab, 2.5).half(), around(klab, 2.5), around(torch.arange(C), 3.5).t().contiguous(),
            klab, qlab)


def torch_loop(beta_list, alpha_list, cache_keys, cache_values, features, labels, clip_weights):
    """The reference's search restated in torch: every pair recomputes the affinity, the
    cache term, the CLIP logits and the accuracy, and reads the hit count back on the host
    (the reference's cls_acc synchronises once per pair too); strict > keeps the first best."""
    n = labels.shape[0]
    best_acc, best_beta, best_alpha = 0, 0, 0
    for beta in beta_list:
        for alpha in alpha_list:
            aff = features @ cache_keys
            cache_term = torch.exp(-(beta - beta * aff)) @ cache_values
            zero_shot = 100.0 * features @ clip_weights
            logits = zero_shot + alpha * cache_term
            hits = logits.topk(1, dim=1).indices[:, 0].eq(labels).sum()
            acc = 100 * float(hits.cpu()) / n
            if acc > best_acc:
                best_acc, best_beta, best_alpha = acc, beta, alpha
    return best_beta, best_alpha, best_acc


def kernel_split(tip, keys, values, F, labels, W, betas, alphas, reps=5):
    """Best-of-reps device-event time of each C call of the device path, in microseconds."""
    from miclip import _lib
    lib = _lib.load_library()
    dev = F.device
    Nq, E = F.shape
    Nk, C, nb, na = keys.shape[1], W.shape[1], len(betas), len(alphas)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    K = keys.float().t().contiguous()
    Wt = W.float().t().contiguous()
    aff = torch.empty(Nq, Nk, device=dev)
    Z = torch.empty(Nq, C, device=dev)
    klab = values.float().argmax(1).int()
    lab = labels.int()
    b = torch.tensor(betas, dtype=torch.float32, device=dev)
    a = torch.tensor(alphas, dtype=torch.float32, device=dev)
    counts = torch.empty(nb, na, device=dev, dtype=torch.int32)
    logits = torch.empty(Nq, C, device=dev)
    scratch = torch.empty(int(lib.miclip_tip_scratch_bytes(Nq, Nk, E, C, nb, na)), device=dev,
                          dtype=torch.uint8)
    s = _lib.stream_handle(dev)
    dt = tip._DTYPES[F.dtype]
    calls = {
        "affinity_us": lambda: lib.miclip_tip_affinity(p(F), dt, p(K), Nq, Nk, E, 1.0, p(aff), s),
        "clip_logits_us": lambda: lib.miclip_tip_affinity(p(F), dt, p(Wt), Nq, C, E, 100.0, p(Z), s),
        "grid_us": lambda: lib.miclip_tip_grid(p(aff), p(klab), p(Z), p(lab), p(b), p(a), Nq, Nk, C,
                                               nb, na, p(counts), p(scratch), s),
        "logits_us": lambda: lib.miclip_tip_logits(p(aff), p(klab), p(Z), Nq, Nk, C, betas[1],
                                                   alphas[1], p(logits), p(scratch), s),
    }
    out = {}
    for name, fn in calls.items():
        best = None
        for _ in range(reps + 1):                      # the first pass is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(fn(), name)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1) * 1e3
            best = t if best is None else min(best, t)
        out[name] = round(best, 1)
    return out


def record(Nq, Nk, E, C, rounds):
    from miclip import tip
    dev = torch.device("cuda")
    F, K, W, klab, qlab = make_data(Nq, Nk, E, C, seed=Nk + E)
    F, qlab = F.to(dev), qlab.to(dev)
    keys32 = K.t().contiguous().to(dev)                                     # [E, Nk]
    values = torch.nn.functional.one_hot(klab, C).half().to(dev)
    W32 = W.to(dev)
    keys16, W16 = keys32.half(), W32.half()
    betas, alphas = tip.beta_alpha_lists(CFG)

    def device_call():
        with contextlib.redirect_stdout(io.StringIO()):
            return tip.search_hp_tip(CFG, keys32, values, F, qlab, W32)

    def torch_call():
        return torch_loop(betas, alphas, keys16, values, F, qlab, W16)

    for _ in range(5):                                  # untimed: the device time settles
        device_call()
    torch_loop(betas[:10], alphas, keys16, values, F, qlab, W16)           # warm-up of every op
    dev_s, ref_s, got, want = [], [], None, None
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = device_call()
        torch.cuda.synchronize()
        dev_s.append(round(time.perf_counter() - t0, 6))
        t0 = time.perf_counter()
        want = torch_call()
        torch.cuda.synchronize()
        ref_s.append(round(time.perf_counter() - t0, 6))
    counts = tip.tip_accuracy_grid(keys32, values, F, qlab, W32, betas, alphas)[0].cpu()
    rec = {"workload": "search_hp_tip", "Nq": Nq, "Nk": Nk, "E": E, "C": C,
           "search_scale": CFG["search_scale"], "search_step": CFG["search_step"],
           "pairs": len(betas) * len(alphas), "rounds": rounds,
           "device_s": dev_s, "torch_loop_s": ref_s, "device_best_s": min(dev_s),
           "torch_loop_best_s": min(ref_s),
           "torch_loop_over_device": round(min(ref_s) / min(dev_s), 2),
           "device_pair": list(got), "torch_fp16_pair": list(want[:2]),
           "device_best_acc": round(100.0 * int(counts.max()) / Nq, 4),
           "torch_fp16_best_acc": round(want[2], 4),
           "device": torch.cuda.get_device_name(0)}
    rec.update(kernel_split(tip, keys32, values, F, qlab, W32, betas, alphas))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tip", "bench_tip.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = []
    for Nk in (320, 4200):
        for E in (512, 768):
            lines.append(record(1398, Nk, E, 20, a.rounds))
            print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
