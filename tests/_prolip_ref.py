"""Closed-form fp64 restatement of a ProLIP training run (methods/ProLIP.py:165-259)
and the error bar the ProLIP tests share. CPU only; nothing here touches the code
under test.

One step, for features X [n, D], labels y, projector P, start P0, text weights W:
    Z = X P;  nrm = max(|z|, 1e-12);  f = Z / nrm;  L = scale * f W
    CE = mean(logsumexp(L) - L[y]);  Gm = (softmax(L) - onehot(y)) / n
    dF = scale * Gm W^T;  dZ = (dF - f (f . dF)) / nrm
    dP = X^T dZ + 2 lambda (P - P0)
    Adam(beta 0.9 / 0.999, eps, bias correction by the step counter) with
    lr * 0.5 (1 + cos(pi epoch / T))
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prolip.npz")
EPS32 = 2.0 ** -23


def load_golden():
    import json
    z = np.load(GOLDEN)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d["meta"]).decode())
    return d


def view_cycle(epochs, V):
    out, cnt = [], 0
    for _ in range(epochs):
        cnt = 0 if (cnt + 1) % V == 0 else cnt + 1
        out.append(cnt)
    return out


def step_terms(X, y, P, W, scale=100.0):
    """(CE, correct count, dZ) of one forward / backward in X's dtype (closed form)."""
    n = X.shape[0]
    Z = X @ P
    nrm = Z.norm(dim=1, keepdim=True).clamp_min(1e-12)
    f = Z / nrm
    L = scale * (f @ W)
    lse = torch.logsumexp(L, dim=1)
    ce = (lse - L[torch.arange(n), y]).mean()
    Gm = torch.softmax(L, dim=1)
    Gm[torch.arange(n), y] -= 1.0
    Gm = Gm / n
    dF = scale * (Gm @ W.t())
    dZ = (dF - f * (f * dF).sum(dim=1, keepdim=True)) / nrm
    return ce, int((L.argmax(dim=1) == y).sum()), dZ


def restate(views, y, P0, W, lr, lam, epochs, feat_batch_size=0, scale=100.0, eps=1e-4,
            dtype=np.float64):
    """Run of one configuration in `dtype` (fp64: the yardstick; fp32: a second fp32
    evaluation for the history's error bar): (P [D, E], history [steps, 3] = {CE, MSE,
    correct})."""
    views = [torch.as_tensor(np.asarray(v).astype(dtype)) for v in views]
    y = torch.as_tensor(np.asarray(y)).long()
    P0 = torch.as_tensor(np.asarray(P0).astype(dtype))
    W = torch.as_tensor(np.asarray(W).astype(dtype))
    n = views[0].shape[0]
    bs = int(feat_batch_size)
    chunks = [(i, min(i + bs, n)) for i in range(0, n, bs)] if bs > 0 else [(0, n)]
    lam_eff = float(lam) / len(chunks)
    P, m, v = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0)
    hist, t = [], 0
    for epoch, vi in enumerate(view_cycle(epochs, len(views))):
        lr_t = float(lr) * 0.5 * (1.0 + math.cos(math.pi * epoch / epochs))
        for i0, i1 in chunks:
            X = views[vi][i0:i1]
            ce, ok, dZ = step_terms(X, y[i0:i1], P, W, scale)
            diff = P - P0
            hist.append([float(ce), float((diff * diff).sum()), float(ok)])
            g = X.t() @ dZ + 2.0 * lam_eff * diff
            t += 1
            m = 0.9 * m + 0.1 * g
            v = 0.999 * v + 0.001 * g * g
            denom = v.sqrt() / math.sqrt(1.0 - 0.999 ** t) + eps
            P = P - (lr_t / (1.0 - 0.9 ** t)) * (m / denom)
    return P.double().numpy(), np.array(hist)


def bar(e_ref, P0):
    """4 * max(the reference's own fp32 error, 8 ulp of the largest start weight)."""
    return 4.0 * max(float(e_ref), 8.0 * EPS32 * float(np.abs(np.asarray(P0)).max()))


def bar_on(e_ref, want):
    """bar() with the 8 ulp floor taken on the compared quantity itself, for values
    whose scale has nothing to do with the weights' (Adam's m and v: v is about 1e-6,
    where 8 ulp of max|P0| would be about 6e-7 and allow an error as large as v)."""
    return 4.0 * max(float(e_ref), 8.0 * EPS32 * float(np.abs(np.asarray(want)).max()))


def case_inputs(gold, case):
    """(views [V][n, D] float32 arrays, labels [n], P0, W, lrs, lams, epochs, feat_batch_size)
    of golden case 'a' / 'b' / 'c' / 's' after the label filter."""
    meta = gold["meta"][case]
    src = "a" if case == "b" else case
    P0, W = gold[f"{src}_P0"], gold[f"{src}_W"]
    C = W.shape[1]
    if src == "c":
        views, y = [gold["c_x"]], gold["c_labels"]
    else:
        raw_y = gold[f"{src}_raw_labels"]
        keep = np.flatnonzero(raw_y < C)
        y = raw_y[keep]
        views = [v[keep] for v in gold[f"{src}_raw_views"]]
    if case == "b":
        lrs, lams = [meta["lr"]], [meta["lam"]]
    elif case == "s":
        lrs = [lr for lr in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8) for _ in range(7)]
        lams = [lam for _ in range(7) for lam in (10, 1, 0.1, 0.01, 0.001, 0.0001, 0)]
    else:
        lrs, lams = list(gold[f"{src}_lrs"]), list(gold[f"{src}_lams"])
    return views, y, P0, W, lrs, lams, meta["epochs"], meta.get("feat_batch_size", 0)
