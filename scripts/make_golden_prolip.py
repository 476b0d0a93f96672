#!/usr/bin/env python3
"""Regenerate tests/golden/prolip.npz from a checkout of the reference project.

    python scripts/make_golden_prolip.py /path/to/reference [--out tests/golden/prolip.npz]

Runs the reference's own `methods/ProLIP.py` (`ProLIP.search_init_hp` and
`ProLIP.forward`) on the CPU in fp32 and records inputs and results. The
reference moves tensors with `.cuda()`; inside this process only,
`torch.Tensor.cuda` and `nn.Module.cuda` are made to return `self`. `forward`
gets a stub model whose `encode_image` returns its input (so "images" are
pre-projection features) and a temporary cache directory laid out as the
reference expects. Developer tool: no test and no GPU job runs it.

Cases (see tests/test_gpu_prolip.py):
  A  "full"     41 raw rows, 37 after the label filter; D 48, E 32, C 5, V 3,
                T 12; 3 x 3 (lr, lambda) grid through search_init_hp
  B  "chunked"  case A's data, feat_batch_size 16, T 7, through forward with a
                23-row test split
  C  "wide"     N 40, D 80, E 48, C 20, V 1, T 6, two planted rows whose logit
                is 100 at step 0 (exp overflows fp32 without the max subtraction)
  S  "search"   case A's shapes, 23-row validation split, the 7 x 7 grid through
                forward with search_lr; per configuration the validation
                accuracy and the smallest top-2 logit margin are recorded, and
                the seed is advanced until every margin is >= 1e-3
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class StubModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1))

    def encode_image(self, images):
        return images


def make_data(seed, n_raw, n_keep, D, E, C, V, n_eval, half=True):
    """Features with class structure: x = (W[:, y] + noise) @ pinv(P0) + noise."""
    g = torch.Generator().manual_seed(seed)
    P0 = torch.randn(D, E, generator=g) * D ** -0.5
    W = F.normalize(torch.randn(E, C, generator=g), dim=0)
    pinv = torch.linalg.pinv(P0.double()).float()            # [E, D]
    labels = torch.randint(0, C, (n_raw,), generator=g)
    drop = torch.randperm(n_raw, generator=g)[: n_raw - n_keep]
    labels[drop] = C + torch.randint(0, 2, (len(drop),), generator=g)   # filtered out by labels < C

    def feats(y, noise):
        yy = y.clamp(max=C - 1)
        z = W[:, yy].t() + noise * torch.randn(len(y), E, generator=g)
        x = z @ pinv + 0.05 * torch.randn(len(y), D, generator=g)
        return x.half().float() if half else x

    views = [feats(labels, 0.35) for _ in range(V)]
    ev_y = torch.randint(0, C, (n_eval,), generator=g)
    ev_x = feats(ev_y, 0.45)
    return P0, W, labels, views, ev_x, ev_y


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def base_cfg(root, V, T, **kw):
    cfg = {"backbone": "ViT-B/16", "dataset": "cs", "root_path": root, "aug_views": V,
           "train_epoch": T, "search_lr": False, "lr_v": 1e-3, "lambda_v": 0.1,
           "lambda_funct_1_N": False, "lambda_funct_1_N2": False, "feat_batch_size": 0,
           "save_checkpoints": False}
    cfg.update(kw)
    return cfg


def search_one(ProLIP, cfg, lr, lam, P0, W, views, labels):
    m = ProLIP(cfg)
    proj = quiet(m.search_init_hp, nn.MSELoss(reduction="sum"), cfg, lr, lam, StubModel(),
                 {"visual.proj": P0.clone()}, W, views, labels)
    return proj.vit_proj.detach().clone()


def run_forward(ProLIP, cfg, P0, W, raw_views, raw_labels, val, test, C, shots=4, task=1):
    """ProLIP.forward in a temporary working directory; returns (loss, acc, trained
    projector, the results_lr line or None)."""
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        cfg = dict(cfg, root_path=tmp)
        d = os.path.join(tmp, "features_ViTB16_cs", f"{shots}_shot", f"seed{task}")
        os.makedirs(d)
        torch.save(raw_labels, os.path.join(d, "label.pth"))
        for v, x in enumerate(raw_views):
            torch.save(x, os.path.join(d, f"f{v}.pth"))
        sd = {"visual.proj": P0.clone()}
        os.chdir(tmp)
        try:
            loss, acc = quiet(
                ProLIP(cfg), train_loader=None, val_loader=[val] if val else None,
                test_loader=[test], test_loader_v2=None, test_loader_sketch=None,
                test_loader_a=None, test_loader_r=None, text_weights=W, text_weights_a=None,
                text_weights_r=None, text_weights_before=None, model=StubModel(), state_dict=sd,
                classnames=[f"c{i}" for i in range(C)], task=task, shots=shots, config_file="golden",
                test_config_path="golden.yaml")
            line = None
            p = os.path.join("results_lr", "golden", f"cs{shots}_shot_lr.txt")
            if os.path.isfile(p):
                line = open(p).read().strip()
        finally:
            os.chdir(cwd)
    # the reference trains state_dict["visual.proj"] in place (nn.Parameter shares storage)
    return float(loss.detach()), float(acc), sd["visual.proj"].detach().clone(), line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tests", "golden", "prolip.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self
    from methods.ProLIP import ProLIP
    torch.set_num_threads(1)
    out, meta = {}, {}
    lr_list = [1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8]
    lambda_list = [10, 1, 0.1, 0.01, 0.001, 0.0001, 0]

    # ---- A and B share data
    D, E, C, V = 48, 32, 5, 3
    P0, W, raw_y, raw_views, test_x, test_y = make_data(11, 41, 37, D, E, C, V, 23)
    keep = torch.where(raw_y < C)[0]
    assert len(keep) == 37
    y, views = raw_y[keep], [x[keep] for x in raw_views]
    a_lrs = [lr for lr in (1e-2, 1e-3, 1e-5) for _ in range(3)]
    a_lams = [lam for _ in range(3) for lam in (10, 0.1, 0)]
    cfg = base_cfg("", V, 12)
    out.update(a_P0=P0, a_W=W, a_raw_labels=raw_y, a_raw_views=torch.stack(raw_views).half(),
               a_test_x=test_x.half(), a_test_y=test_y, a_lrs=np.array(a_lrs), a_lams=np.array(a_lams),
               a_proj=torch.stack([search_one(ProLIP, cfg, lr, lam, P0, W, views, y)
                                   for lr, lam in zip(a_lrs, a_lams)]))
    meta["a"] = {"epochs": 12}
    cfg = base_cfg("", V, 7, feat_batch_size=16, lr_v=1e-3, lambda_v=0.1)
    loss, acc, proj, _ = run_forward(ProLIP, cfg, P0, W, raw_views, raw_y, None, (test_x, test_y), C)
    out.update(b_proj=proj, b_loss=np.float64(loss), b_acc=np.float64(acc))
    meta["b"] = {"epochs": 7, "feat_batch_size": 16, "lr": 1e-3, "lam": 0.1, "shots": 4, "task": 1}

    # ---- C: wide, saturated
    D, E, C = 80, 48, 20
    P0, W, y, views, _, _ = make_data(23, 40, 40, D, E, C, 1, 1, half=False)
    pinv = torch.linalg.pinv(P0.double())
    x = views[0]
    c0, c1 = 3, 17
    plant = (4.0 * (W[:, c0].double() @ pinv)).float()
    x[5], y[5] = plant, c0          # logit 100 on its own class
    x[6], y[6] = plant, c1          # logit 100 on another class
    with torch.no_grad():
        lg = 100.0 * F.normalize(x @ P0, dim=-1) @ W
    assert abs(float(lg[5, c0]) - 100.0) < 1e-3 and not torch.isfinite(lg.exp()).all()
    cfg = base_cfg("", 1, 6)
    c_lrs, c_lams = [1e-3, 1e-2], [0.1, 1.0]
    out.update(c_P0=P0, c_W=W, c_labels=y, c_x=x, c_lrs=np.array(c_lrs), c_lams=np.array(c_lams),
               c_proj=torch.stack([search_one(ProLIP, cfg, lr, lam, P0, W, [x], y)
                                   for lr, lam in zip(c_lrs, c_lams)]))
    meta["c"] = {"epochs": 6}

    # ---- S: the full search; advance the seed until every margin is >= 1e-3
    D, E, C, V = 48, 32, 5, 3
    for seed in range(100, 200):
        P0, W, raw_y, raw_views, val_x, val_y = make_data(seed, 41, 37, D, E, C, V, 23)
        keep = torch.where(raw_y < C)[0]
        y, views = raw_y[keep], [x[keep] for x in raw_views]
        cfg = base_cfg("", V, 12)
        accs, margins = [], []
        for lr in lr_list:
            for lam in lambda_list:
                P = search_one(ProLIP, cfg, lr, lam, P0, W, views, y)
                with torch.no_grad():
                    lg = 100.0 * F.normalize(val_x @ P, dim=-1) @ W
                top2 = lg.topk(2, dim=1).values
                margins.append(float((top2[:, 0] - top2[:, 1]).min()))
                accs.append(100.0 * float((lg.argmax(1) == val_y).float().sum()) / len(val_y))
        if min(margins) >= 1e-3 and len(set(accs)) > 2:
            break
    assert min(margins) >= 1e-3, "no seed with every top-2 margin >= 1e-3"
    cfg = base_cfg("", V, 12, search_lr=True)
    loss, acc, proj, line = run_forward(ProLIP, cfg, P0, W, raw_views, raw_y, (val_x, val_y),
                                        (val_x, val_y), C)
    lr_s, lam_s = (float(t) for t in line.split(","))
    out.update(s_P0=P0, s_W=W, s_raw_labels=raw_y, s_raw_views=torch.stack(raw_views).half(),
               s_val_x=val_x.half(), s_val_y=val_y, s_acc=np.array(accs).reshape(7, 7),
               s_margin=np.array(margins).reshape(7, 7), s_lr=np.float64(lr_s),
               s_lam=np.float64(lam_s), s_proj=proj, s_loss=np.float64(loss),
               s_acc_test=np.float64(acc))
    meta["s"] = {"epochs": 12, "seed": seed, "shots": 4, "task": 1}

    arrays = {k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes); S seed {seed}, chosen "
          f"lr {lr_s} lambda {lam_s}, min margin {min(margins):.4g}, "
          f"accs {sorted(set(accs))}; B loss {out['b_loss']} acc {out['b_acc']}")


if __name__ == "__main__":
    main()
