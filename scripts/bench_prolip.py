#!/usr/bin/env python3
"""Time ProLIP projector training: the fused HIP path (miclip.prolip) against a plain
torch-on-GPU loop that restates the reference (methods/ProLIP.py), on the same
device, in the same process, the two alternating round by round.

    python scripts/bench_prolip.py [--rounds 3] [--search-epochs 300] [--out FILE]

Workloads (seeded synthetic features with class structure, fp16 cache):
  search   the 49-configuration (lr, lambda) search, 300 epochs, D 768, E 512, C 20,
           n 320, 3 views. torch: search_init_hp's loop (:302-361), 49 runs one after
           another. fused: one fit_projector_grid call (3 kernels per step for all 49).
  chunked  one fit with feat_batch_size 64, n 4096, 5 epochs (320 steps). torch:
           forward's chunked loop (:191-226) with its two .item() and cls_acc per step.
Times are host clock around work that ends in a device synchronise, after one
untimed warm-up of each path; one JSON line per workload. The torch loop gets the
features already widened to fp32 on the device (not charged to it). Not part of
bench.py.
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))


def make(n, D, E, C, V, seed, dev):
    g = torch.Generator().manual_seed(seed)
    P0 = torch.randn(D, E, generator=g) * D ** -0.5
    W = F.normalize(torch.randn(E, C, generator=g), dim=0)
    y = torch.randint(0, C, (n,), generator=g)
    pinv = torch.linalg.pinv(P0)
    views = [((W[:, y].t() + 0.35 * torch.randn(n, E, generator=g)) @ pinv
              + 0.05 * torch.randn(n, D, generator=g)).half().to(dev) for _ in range(V)]
    return views, y.to(dev), P0.to(dev), W.to(dev)


def torch_run(views32, y, P0, W, lr, lam, epochs, bs=0, log=False):
    """The reference's loop on the GPU with autograd, Adam(eps=1e-4), CosineAnnealingLR."""
    proj = torch.nn.Parameter(P0.clone())
    opt = torch.optim.Adam([proj], lr=lr, eps=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs)
    mse = torch.nn.MSELoss(reduction="sum")
    n, cnt = views32[0].shape[0], 0
    chunks = [(i, min(i + bs, n)) for i in range(0, n, bs)] if bs else [(0, n)]
    lam_eff = lam / len(chunks)
    for _ in range(epochs):
        cnt = 0 if (cnt + 1) % len(views32) == 0 else cnt + 1
        for i0, i1 in chunks:
            x, t = views32[cnt][i0:i1], y[i0:i1]
            logits = 100.0 * F.normalize(x @ proj, dim=-1) @ W
            loss1, loss2 = F.cross_entropy(logits, t), mse(P0.view(-1), proj.view(-1))
            loss = loss1 + lam_eff * loss2
            if log:   # forward's bookkeeping: cls_acc and two .item() per step
                float((logits.topk(1, 1, True, True)[1].t().eq(t.view(1, -1))).float().sum().cpu())
                loss1.item(), loss2.item()
            opt.zero_grad()
            loss.backward()
            opt.step()
        sched.step()
    return proj.detach()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--search-epochs", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_prolip.py needs a HIP device (no CPU fallback)")
    from miclip import prolip
    dev = torch.device("cuda")
    lines = []

    def report(name, shape, fused_s, torch_s, diff, steps, launches, extra=None):
        rec = {"workload": name, **shape, "rounds": len(fused_s), "steps": steps,
               "fused_s": [round(t, 5) for t in fused_s], "torch_s": [round(t, 5) for t in torch_s],
               "fused_best_s": round(min(fused_s), 5), "torch_best_s": round(min(torch_s), 5),
               "torch_over_fused": round(min(torch_s) / min(fused_s), 2),
               "fused_us_per_step": round(1e6 * min(fused_s) / steps, 2),
               "fused_kernels_per_step": launches, "max_abs_diff_proj": float(diff),
               "device": torch.cuda.get_device_name(0)}
        rec.update(extra or {})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # ---- search
    T = args.search_epochs
    shape = dict(D=768, E=512, C=20, n=320, views=3, G=49, epochs=T)
    views, y, P0, W = make(320, 768, 512, 20, 3, 1, dev)
    views32 = [v.float() for v in views]
    pairs = [(lr, lam) for lr in prolip.LR_LIST for lam in prolip.LAMBDA_LIST]
    lrs, lams = [p[0] for p in pairs], [p[1] for p in pairs]

    def fused_search(epochs=T):
        return prolip.fit_projector_grid(views, y, P0, W, lrs, lams, epochs=epochs).proj

    def torch_search(epochs=T):
        return torch.stack([torch_run(views32, y, P0, W, lr, lam, epochs) for lr, lam in pairs])

    fused_search(3), torch_search(2)            # warm-up: code objects, allocator, autograd
    fs, ts = [], []
    for _ in range(args.rounds):
        t, pf = timed(fused_search)
        fs.append(t)
        t, pt = timed(torch_search)
        ts.append(t)
    # fused vs torch per lr (max over the 7 lambdas and all weights): two fp32 runs of the
    # same 300 steps; they drift apart where lr / eps is large (eps = 1e-4)
    by_lr = (pf - pt).abs().flatten(1).max(dim=1).values.view(7, 7).max(dim=1).values
    report("search", shape, fs, ts, (pf - pt).abs().max(), T, 3,
           {"max_abs_diff_proj_by_lr": {f"{lr:g}": float(d) for lr, d in zip(prolip.LR_LIST, by_lr)}})

    # ---- chunked fit
    shape = dict(D=768, E=512, C=20, n=4096, views=3, G=1, epochs=5, feat_batch_size=64)
    views, y, P0, W = make(4096, 768, 512, 20, 3, 2, dev)
    views32 = [v.float() for v in views]

    def fused_fit():
        return prolip.fit_projector_grid(views, y, P0, W, [1e-4], [0.1], epochs=5,
                                         feat_batch_size=64).proj[0]

    def torch_fit():
        return torch_run(views32, y, P0, W, 1e-4, 0.1, 5, bs=64, log=True)

    fused_fit(), torch_fit()
    fs, ts = [], []
    for _ in range(max(args.rounds, 5)):
        t, pf = timed(fused_fit)
        fs.append(t)
        t, pt = timed(torch_fit)
        ts.append(t)
    report("chunked", shape, fs, ts, (pf - pt).abs().max(), 5 * math.ceil(4096 / 64), 3)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
