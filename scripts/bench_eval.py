#!/usr/bin/env python3
"""Time the fused validation metrics (miclip.evaluation.evaluate_features, one
miclip_eval_batch call per batch) against the composition that was available before
it: miclip_zero_shot(k = 3) per batch plus the torch ops of `_run_validation`
(methods/PEFT_openclip.py:89-117) and of `L2MetricsAccumulator.update` in mode
"logits" / reduce "mean", with their `.item()` and `.cpu()` calls -- on the same
device, in the same process, the two alternating round by round.

    python scripts/bench_eval.py [--rounds 3] [--out profiles/eval/bench_eval.jsonl]

Workloads: N = 65,536 cached features (fp32, on the device), E = 768, batches of 256,
with an L3 -> L2 map; C = 20 (8 groups) and C = 1000 (37 groups). The baseline's L2
aggregation is one index_add_ per batch (the reference loops over the C classes in
Python, which at C = 1000 would be 2,000 launches per batch: not charged to it).
Times are host clock around work that ends in a device synchronise, after one untimed
warm-up of each path; a timed window is `inner` whole evaluations (times are per
evaluation), best of `rounds`. One JSON line per workload. Not part of
bench.py.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))


def make(n, E, C, num_l2, seed, dev):
    g = torch.Generator().manual_seed(seed)
    W = F.normalize(torch.randn(E, C, generator=g), dim=0)
    y = torch.randint(0, C, (n,), generator=g)
    f = (W[:, y].t() + 0.15 * torch.randn(n, E, generator=g)).contiguous()
    m = torch.randint(0, num_l2, (C,), generator=g)
    return f.to(dev), y.to(dev), W.to(dev), m


class ZeroShot:
    """miclip_zero_shot(apply_proj = 0) on a bare handle of embed_dim E."""

    def __init__(self, E):
        from miclip import _lib
        self._lib, self.lib = _lib, _lib.load_library()
        cfg = _lib.MiclipConfig(embed_dim=E, image_resolution=32, vision_layers=1,
                                vision_width=256, vision_patch_size=32, context_length=8,
                                vocab_size=16, transformer_width=256, transformer_heads=4,
                                transformer_layers=0, compute_dtype=_lib.MICLIP_FP16,
                                act=_lib.MICLIP_ACT_QUICKGELU, vision_head_dim=64, options=0)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.miclip_model_create(ctypes.byref(cfg), 0, ctypes.byref(self.h)), "create")

    def __call__(self, f, W, k):
        assert f.is_contiguous() and W.is_contiguous()
        B, C = f.shape[0], W.shape[1]
        logits = torch.empty(B, C, device=f.device)
        top = torch.empty(B, k, device=f.device, dtype=torch.int32)
        self._lib.check(self.lib.miclip_zero_shot(self.h, f.data_ptr(), B, 0, W.data_ptr(), C, 100.0,
                                                  logits.data_ptr(), top.data_ptr(), k,
                                                  self._lib.stream_handle(f.device)), "zero_shot")
        return logits, top.long()

    def close(self):
        self.lib.miclip_model_destroy(self.h)


def baseline(zs, f, y, W, m, num_l2, bs):
    """The reference's loop body with the head kernel that existed before."""
    from miclip.evaluation import mcc_from_confusion, weighted_f1
    C, dev = W.shape[1], f.device
    m_d = m.to(dev)
    counts = torch.bincount(m_d, minlength=num_l2).clamp_min(1).float()
    cm = torch.zeros(C * C, dtype=torch.long, device=dev)
    cm2 = torch.zeros(num_l2 * num_l2, dtype=torch.long, device=dev)
    total_loss, top1, top3, seen, batches, l2_1, l2_3 = 0.0, 0, 0, 0, 0, 0, 0
    y_true, y_pred, y2_true, y2_pred = [], [], [], []
    for i in range(0, f.shape[0], bs):
        x, t = f[i:i + bs], y[i:i + bs]
        logits, top = zs(x, W, 3)
        loss = F.cross_entropy(logits, t)
        total_loss += loss.item()                                          # :99
        top1 += int((top[:, :1] == t[:, None]).sum().cpu().numpy())        # cls_acc, utils.py:19
        top3 += int((top == t[:, None]).sum().cpu().numpy())
        preds = top[:, 0]
        seen += len(t)
        batches += 1
        y_true.append(t.cpu())                                             # :107-108
        y_pred.append(preds.cpu())
        cm += torch.bincount(t * C + preds, minlength=C * C)               # the F1 / CM updates
        t2 = m_d[t]                                                        # evaluation.py:190
        l2 = torch.zeros(len(t), num_l2, device=dev).index_add_(1, m_d, logits) / counts
        tk = l2.topk(min(3, num_l2), dim=1).indices
        correct = tk.eq(t2.view(-1, 1))
        l2_1 += int(correct[:, :1].any(dim=1).sum().item())                # :213
        l2_3 += int(correct.any(dim=1).sum().item())
        p2 = l2.argmax(dim=1)
        y2_true.append(t2.cpu())
        y2_pred.append(p2.cpu())
        cm2 += torch.bincount(t2 * num_l2 + p2, minlength=num_l2 * num_l2)
    cmh, cm2h = cm.view(C, C).cpu().numpy(), cm2.view(num_l2, num_l2).cpu().numpy()
    return (total_loss / batches, top1 / seen, top3 / seen, weighted_f1(cmh), mcc_from_confusion(cmh),
            cmh, {"top1": l2_1 / seen, "top3": l2_3 / seen, "f1": weighted_f1(cm2h),
                  "mcc": mcc_from_confusion(cm2h), "cm": cm2h})


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=8, help="evaluations per timed window")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "bench_eval.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs a HIP device")
    from miclip.evaluation import evaluate_features
    dev = torch.device("cuda", 0)
    lines = []
    for C, num_l2 in ((20, 8), (1000, 37)):
        E = 768
        f, y, W, m = make(args.n, E, C, num_l2, 5, dev)
        ctx = {"l3_to_l2": m.tolist(), "num_l2": num_l2, "mode": "logits", "reduce": "mean",
               "topk": (1, 3), "return_confusion_matrix": True}
        zs = ZeroShot(E)

        def fused():
            for _ in range(args.inner):
                out = evaluate_features(f, y, W, batch_size=args.batch, l2_eval_ctx=ctx,
                                        return_confusion_matrix=True)
            return out

        def torch_path():
            for _ in range(args.inner):
                out = baseline(zs, f, y, W, m, num_l2, args.batch)
            return out
        timed(fused), timed(torch_path)                       # warm-up, untimed
        t_f, t_t = [], []
        for _ in range(args.rounds):                          # interleaved
            dt, a = timed(fused)
            t_f.append(dt)
            dt, b = timed(torch_path)
            t_t.append(dt)
        zs.close()
        same = (a[1] == b[1] and a[2] == b[2] and np.array_equal(a[5], b[5])
                and a[6]["top1"] == b[6]["top1"] and np.array_equal(a[6]["cm"], b[6]["cm"]))
        t_f, t_t = [v / args.inner for v in t_f], [v / args.inner for v in t_t]
        batches = -(-args.n // args.batch)
        lines.append({
            "workload": f"evaluate_features C={C}", "N": args.n, "E": E, "C": C, "num_l2": num_l2,
            "batch": args.batch, "batches": batches, "rounds": args.rounds, "evaluations_per_window": args.inner,
            "fused_s": [round(v, 5) for v in t_f], "baseline_s": [round(v, 5) for v in t_t],
            "fused_best_s": round(min(t_f), 5), "baseline_best_s": round(min(t_t), 5),
            "baseline_over_fused": round(min(t_t) / min(t_f), 3),
            "fused_us_per_batch": round(1e6 * min(t_f) / batches, 2),
            "baseline_us_per_batch": round(1e6 * min(t_t) / batches, 2),
            "integer_results_equal": bool(same), "loss_fused": a[0], "loss_baseline": b[0],
            "device": torch.cuda.get_device_name(0)})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
