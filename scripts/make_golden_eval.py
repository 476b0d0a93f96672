#!/usr/bin/env python3
"""Regenerate tests/golden/evaluation.npz from a checkout of the reference project.

    python scripts/make_golden_eval.py /path/to/reference [--out tests/golden/evaluation.npz]

Runs the reference's own `_run_validation` (methods/PEFT_openclip.py:50-136),
`L2MetricsAccumulator` and `aggregate_logits_to_l2` (aihab_utils/evaluation.py) on
the CPU in fp32 and records inputs and results. The stub model's `encode_image`
returns its input, so "images" are features. `wandb`, `seaborn` and `torcheval` are
not dependencies of this project: stand-in modules are installed in this process only. The
stand-in F1 and confusion matrix are NOT the reference's results (the file's
metadata says so; the tests check F1 against sklearn); loss, top-1, top-3, MCC, the
L2 top-k / MCC, the aggregated logits, the ClassificationTracker tables and the
20-entry map of `build_l3_to_l2_map()` are the reference's own. Developer tool: no
test and no GPU job runs it.

Case: 53 rows in batches of 16 with metadata, E = 64, C = 20, the real L3 -> L2 map;
L2 modes argmax and logits x {sum, mean, logsumexp}. The seed is advanced until, in
every row, the gaps between the 1st / 2nd and the 3rd / 4th L3 logits, and the same
gaps in every reduce's L2 logits, are >= 1e-3, so the reference's fp32 summation
order cannot flip an integer result; the smallest gap is recorded.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

N, E, C, BATCH = 53, 64, 20, 16
MIN_GAP = 1e-3


class StubModel(nn.Module):
    def encode_image(self, images):
        return images


def install_stand_ins(tables):
    """wandb (log / Table / Image), seaborn and torcheval.metrics for this process."""
    wandb = types.ModuleType("wandb")

    class Table:
        def __init__(self, dataframe=None, **kw):
            self.dataframe = dataframe

    def log(d, *a, **k):
        for key, v in d.items():
            if isinstance(v, Table):
                tables[key] = v.dataframe
    wandb.Table, wandb.log, wandb.Image = Table, log, lambda *a, **k: None
    wandb.init = wandb.finish = lambda *a, **k: None
    wandb.config, wandb.run = {}, None
    sys.modules["wandb"] = wandb
    sys.modules["seaborn"] = types.ModuleType("seaborn")

    class _Pairs:
        def __init__(self, num_classes, average=None):
            self.k, self.t, self.p = int(num_classes), [], []

        def update(self, preds, targets):
            self.p.append(preds.detach().cpu().long())
            self.t.append(targets.detach().cpu().long())

        def cm(self):
            cm = torch.zeros(self.k, self.k, dtype=torch.long)
            if self.t:
                cm.index_put_((torch.cat(self.t), torch.cat(self.p)), torch.tensor(1), accumulate=True)
            return cm

    class MulticlassConfusionMatrix(_Pairs):
        def compute(self):
            return self.cm()

    class MulticlassF1Score(_Pairs):
        def compute(self):
            cm = self.cm().double()
            tp, sup, pred = cm.diag(), cm.sum(1), cm.sum(0)
            den = pred + sup
            f1 = torch.where(den > 0, 2 * tp / den.clamp_min(1), torch.zeros_like(den))
            return (f1 * sup).sum() / sup.sum().clamp_min(1)

    te, tem = types.ModuleType("torcheval"), types.ModuleType("torcheval.metrics")
    tem.MulticlassF1Score, tem.MulticlassConfusionMatrix = MulticlassF1Score, MulticlassConfusionMatrix
    te.metrics = tem
    sys.modules["torcheval"], sys.modules["torcheval.metrics"] = te, tem


def make_data(seed):
    g = torch.Generator().manual_seed(seed)
    W = F.normalize(torch.randn(E, C, generator=g), dim=0)
    y = torch.randint(0, C, (N,), generator=g)
    f = 1.7 * (W[:, y].t() + 0.42 * torch.randn(N, E, generator=g))
    return f.contiguous(), y, W.contiguous()


def gaps(lg):
    """Smallest 1st-2nd and 3rd-4th gap over the rows (3rd-4th only with >= 4 columns)."""
    k = min(4, lg.shape[1])
    v = lg.topk(k, dim=1).values
    out = float((v[:, 0] - v[:, 1]).min())
    if k == 4:
        out = min(out, float((v[:, 2] - v[:, 3]).min()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tests", "golden", "evaluation.npz"))
    args = ap.parse_args()
    tables = {}
    install_stand_ins(tables)
    sys.path.insert(0, os.path.abspath(args.reference))
    from aihab_utils.evaluation import aggregate_logits_to_l2
    from data import REASSIGN_LABEL_NAME_L3, build_l3_to_l2_map
    from methods.PEFT_openclip import _run_validation
    torch.set_num_threads(1)
    l3_to_l2, l2_names = build_l3_to_l2_map()
    num_l2 = len(l2_names)
    assert len(l3_to_l2) == C
    class_names = [REASSIGN_LABEL_NAME_L3[i] for i in range(C)]

    for seed in range(300, 400):
        f, y, W = make_data(seed)
        lg = 100.0 * F.normalize(f, dim=-1) @ W
        agg = {r: aggregate_logits_to_l2(lg, l3_to_l2, num_l2, reduce=r)
               for r in ("sum", "mean", "logsumexp")}
        margin = min([gaps(lg)] + [gaps(v) for v in agg.values()])
        acc = float((lg.argmax(1) == y).float().mean())
        if margin >= MIN_GAP and 0.5 < acc < 0.95:
            break
    assert margin >= MIN_GAP, "no seed with every gap >= 1e-3"

    meta_all = {"file_name": [f"plot_{i:03d}.jpg" for i in range(N)],
                "plot_word_label": [class_names[int(v)] for v in y],
                "image_source": [("survey", "citizen")[i % 2] for i in range(N)]}
    loader = [(f[i:i + BATCH], y[i:i + BATCH], {k: v[i:i + BATCH] for k, v in meta_all.items()})
              for i in range(0, N, BATCH)]
    out = {"feats": f, "labels": y, "text_weights": W, "l3_to_l2": np.array(l3_to_l2, np.int64),
           "logits": lg, "class_names": np.array(class_names), "l2_names": np.array(l2_names),
           **{f"meta_{k}": np.array(v) for k, v in meta_all.items()},
           **{f"agg_{r}": v for r, v in agg.items()}}
    runs = [("argmax", "mean"), ("logits", "sum"), ("logits", "mean"), ("logits", "logsumexp")]
    for mode, reduce in runs:
        tables.clear()
        ctx = {"l3_to_l2": l3_to_l2, "num_l2": num_l2, "reduce": reduce, "topk": (1, 3),
               "mode": mode, "return_confusion_matrix": True}
        with contextlib.redirect_stdout(io.StringIO()):
            loss, top1, top3, f1, mcc, cm, l2m = _run_validation(
                StubModel(), loader, W, "cpu", return_confusion_matrix=True, cls_track=True,
                l2_eval_ctx=ctx)
        tag = f"{mode}_{reduce}"
        out[f"{tag}_scalars"] = np.array([loss, top1, top3, f1, mcc], np.float64)
        out[f"{tag}_cm_stand_in"] = np.asarray(cm)
        out[f"{tag}_l2_scalars"] = np.array([l2m["top1"], l2m.get("top3", np.nan), l2m["f1"],
                                             l2m["mcc"]], np.float64)
        out[f"{tag}_l2_cm_stand_in"] = np.asarray(l2m["cm"])
    # the tracker tables are the same in every run (they do not depend on the L2 context)
    for key, name in (("Misclassifications", "mis"), ("Corclassifications", "cor")):
        df = tables[key]
        out[f"track_{name}_columns"] = np.array(list(df.columns))
        for col in df.columns:
            out[f"track_{name}__{col}"] = df[col].to_numpy()
    out["preds"] = lg.argmax(1)
    out["top3"] = lg.topk(3, dim=1).indices
    meta = {"n": N, "E": E, "C": C, "batch": BATCH, "num_l2": num_l2, "seed": seed,
            "min_gap": margin, "runs": [f"{m}_{r}" for m, r in runs],
            "scalars": ["loss", "top1", "top3", "f1_stand_in", "mcc"],
            "l2_scalars": ["top1", "top3", "f1_stand_in", "mcc"],
            "stand_in": "f1 and the confusion matrices come from this script's stand-in for "
                        "torcheval, not from the reference; everything else is the reference's"}
    arrays = {k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    arrays = {k: (v.astype(str) if v.dtype == object else v) for k, v in arrays.items()}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes); seed {seed}, min gap "
          f"{margin:.4g}, top1 {top1:.4f}, loss {loss:.6f}")


if __name__ == "__main__":
    main()
