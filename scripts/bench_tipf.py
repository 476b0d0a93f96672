#!/usr/bin/env python3
"""Time one Tip-Adapter-F fit (miclip.tip.fit_adapter_grid, the kernels of
csrc/tip_train.hip) against the same recipe in torch fp32 autograd on the same device, in
the same process, the two alternating round by round.

    python scripts/bench_tipf.py [--rounds 5] [--out profiles/tip/bench_tipf.jsonl]

Workload: 20 epochs over n = 4 200 cached unit rows around 20 planted directions (fp16, two
views), batches of 256 (17 steps per epoch, the last one partial), (Nk, E) in {(320, 512),
(320, 768), (4 200, 512), (4 200, 768)}, C = 20, at G = 1 and G = 8 configurations, with
the per-epoch evaluation on 1 398 rows and the best epoch kept. The torch side is the
published loop's shape: per configuration an nn.Linear(E, Nk, bias=False) adapter, AdamW
(eps 1e-4) under CosineAnnealingLR, the loss and the batch's hit count read back every
step, an evaluation after every epoch and a clone of the best weight; its G configurations
run one after the other. Times are host clock around the whole fit with a synchronisation
at the end (the device path reads nothing back before it), after one untimed round of
each; the best round counts and every round is recorded. The split of the device path is
taken with device events around each C call (one step = the staging, forward, loss and
AdamW launches), best of 5. One JSON line per setting. Nothing gates on these numbers.
Not part of bench.py.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))

N, NQ, C, BATCH, EPOCHS = 4200, 1398, 20, 256, 20
GRID = [(1e-3, 1.0, 1.17), (1e-3, 5.5, 1.0), (3e-3, 1.0, 3.0), (3e-4, 3.0, 1.17),
        (1e-3, 2.0, 2.0), (2e-3, 5.5, 3.0), (5e-4, 1.0, 1.0), (1e-3, 4.0, 1.5)]


def make_data(Nk, E, seed):
    g = torch.Generator().manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(C, E, generator=g), dim=1)

    def around(lab, amount):
        x = dirs[lab] + amount * E ** -0.5 * torch.randn(len(lab), E, generator=g)
        return torch.nn.functional.normalize(x, dim=1)

    klab = torch.arange(Nk) % C
    tlab, qlab = torch.randint(0, C, (N,), generator=g), torch.randint(0, C, (NQ,), generator=g)
    views = [around(tlab, 2.5).half(), around(tlab, 2.5).half()]
    return (views, tlab, around(qlab, 2.5).half(), qlab, around(klab, 2.5),
            around(torch.arange(C), 3.5).t().contiguous(), klab)


def torch_fit(keys, values, W, views, labels, ef, el, configs, seed=0):
    """The recipe in torch fp32 autograd, one configuration after the other."""
    from miclip.finetune import cache_order, cache_view
    views = [v.float() for v in views]
    ef = ef.float()
    vals = values.float()
    n = views[0].shape[0]
    spe = (n + BATCH - 1) // BATCH
    out = []
    for lr, beta, alpha in configs:
        adapter = torch.nn.Linear(keys.shape[0], keys.shape[1], bias=False).to(keys.device)
        with torch.no_grad():
            adapter.weight.copy_(keys.t())
        opt = torch.optim.AdamW(adapter.parameters(), lr=lr, eps=1e-4)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, EPOCHS * spe)
        best_acc, best = 0.0, adapter.weight.detach().clone()
        for e in range(EPOCHS):
            f = views[cache_view(e, len(views))]
            order = cache_order(n, seed, e).to(keys.device)
            correct, losses = 0, []
            for s in range(spe):
                rows = order[s * BATCH:(s + 1) * BATCH]
                x, y = f[rows], labels[rows]
                logits = 100.0 * x @ W + alpha * (torch.exp(-(beta - beta * adapter(x))) @ vals)
                loss = torch.nn.functional.cross_entropy(logits, y)
                correct += int((logits.argmax(1) == y).sum().item())
                losses.append(loss.item())
                opt.zero_grad()
                loss.backward()
                opt.step()
                sched.step()
            with torch.no_grad():
                logits = 100.0 * ef @ W + alpha * (torch.exp(-(beta - beta * adapter(ef))) @ vals)
                acc = int((logits.argmax(1) == el).sum().item())
            if acc > best_acc:
                best_acc, best = acc, adapter.weight.detach().clone()
        out.append((best_acc, best))
    return out


def call_split(data, Nk, E, G, reps=5):
    """Best-of-reps device-event time of each C call of the device path, in microseconds."""
    from miclip import _lib, tip
    views, tlab, ef, el, K, W, klab = data
    lib = _lib.load_library()
    dev = views[0].device
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    F, dt = views[0], tip._DTYPES[views[0].dtype]
    Wt = W.float().t().contiguous()
    Z, ez = torch.empty(N, C, device=dev), torch.empty(NQ, C, device=dev)
    keys = K.unsqueeze(0).repeat(G, 1, 1).contiguous()
    m, v, best = torch.zeros_like(keys), torch.zeros_like(keys), keys.clone()
    lr, beta, alpha = (torch.tensor([c[i] for c in GRID[:G]], dtype=torch.float32, device=dev)
                       for i in range(3))
    lab, kl, elab = tlab.int(), klab.int().to(dev), el.int()
    hist = torch.zeros(G, 2, device=dev)
    counts = torch.zeros(1, G, device=dev, dtype=torch.int32)
    bc, be = torch.zeros(G, device=dev, dtype=torch.int32), torch.zeros(G, device=dev, dtype=torch.int32)
    aff = torch.empty(NQ, Nk, device=dev)
    scratch = torch.empty(int(lib.miclip_tipf_scratch_bytes(BATCH, Nk, E, C, G)), device=dev,
                          dtype=torch.uint8)
    tscr = torch.empty(int(lib.miclip_tip_scratch_bytes(NQ, Nk, E, C, 1, 1)), device=dev,
                       dtype=torch.uint8)
    rows = torch.randperm(N)[:BATCH].contiguous()
    s = _lib.stream_handle(dev)
    _lib.check(lib.miclip_tip_affinity(p(F), dt, p(Wt), N, C, E, 100.0, p(Z), s), "Z")
    _lib.check(lib.miclip_tip_affinity(p(ef), dt, p(Wt), NQ, C, E, 100.0, p(ez), s), "Z")
    _lib.check(lib.miclip_tipf_prepare(p(kl), Nk, C, p(scratch), s), "prepare")
    calls = {
        "step_us": lambda: lib.miclip_tipf_step(
            p(F), dt, N, ctypes.c_void_p(rows.data_ptr()), BATCH, p(lab), p(Z), p(kl), p(keys),
            p(m), p(v), p(lr), p(beta), p(alpha), Nk, E, C, G, 1.0, 0.01, 1e-4, 1, p(hist), None,
            p(scratch), s),
        "eval_affinity_us": lambda: lib.miclip_tip_affinity(p(ef), dt, p(keys[0]), NQ, Nk, E, 1.0,
                                                            p(aff), s),
        "eval_grid_us": lambda: lib.miclip_tip_grid(p(aff), p(kl), p(ez), p(elab), p(beta), p(alpha),
                                                    NQ, Nk, C, 1, 1, p(counts), p(tscr), s),
        "keep_best_us": lambda: lib.miclip_tipf_keep_best(p(counts), 0, p(keys), p(best), p(bc),
                                                          p(be), Nk, E, G, s),
    }
    out = {}
    for name, fn in calls.items():
        best_t = None
        for _ in range(reps + 1):                      # the first pass is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(fn(), name)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1) * 1e3
            best_t = t if best_t is None else min(best_t, t)
        out[name] = round(best_t, 1)
    return out


def record(Nk, E, G, rounds):
    from miclip import tip
    dev = torch.device("cuda")
    views, tlab, ef, el, K, W, klab = make_data(Nk, E, seed=Nk + E)
    views, tlab, ef, el = [v.to(dev) for v in views], tlab.to(dev), ef.to(dev), el.to(dev)
    K, W = K.to(dev), W.to(dev)
    keys = K.t().contiguous()                                               # [E, Nk]
    values = torch.nn.functional.one_hot(klab, C).half().to(dev)
    cfgs = GRID[:G]

    def device_call():
        return tip.fit_adapter_grid(keys, values, W, views, tlab, [c[0] for c in cfgs],
                                    [c[1] for c in cfgs], [c[2] for c in cfgs], epochs=EPOCHS,
                                    batch_size=BATCH, eval_features=ef, eval_labels=el)

    def torch_call():
        return torch_fit(keys, values, W, views, tlab, ef, el, cfgs)

    dev_s, ref_s, fit, ref = [], [], None, None
    for r in range(rounds + 1):                         # round 0 is the untimed warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = device_call()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ref = torch_call()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r:
            dev_s.append(round(t1 - t0, 6))
            ref_s.append(round(t2 - t1, 6))
    steps = EPOCHS * fit.steps_per_epoch
    rec = {"workload": "fit_adapter_grid", "n": N, "Nq": NQ, "Nk": Nk, "E": E, "C": C, "G": G,
           "batch": BATCH, "epochs": EPOCHS, "steps": steps, "rounds": rounds,
           "device_s": dev_s, "torch_autograd_s": ref_s, "device_best_s": min(dev_s),
           "torch_autograd_best_s": min(ref_s),
           "torch_over_device": round(min(ref_s) / min(dev_s), 2),
           "device_us_per_step": round(1e6 * min(dev_s) / steps, 1),
           "device_best_counts": fit.best_count.cpu().tolist(),
           "torch_best_counts": [r[0] for r in ref],
           "device": torch.cuda.get_device_name(0)}
    rec.update(call_split((views, tlab, ef, el, K, W, klab), Nk, E, G))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tip", "bench_tipf.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = []
    for Nk, E in ((320, 512), (320, 768), (4200, 512), (4200, 768)):
        for G in (1, 8):
            lines.append(record(Nk, E, G, a.rounds))
            print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
