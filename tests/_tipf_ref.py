"""Torch restatement of the Tip-Adapter-F recipe, written from its formulas (the yardstick
of tests/test_tipf.py and tests/test_gpu_tipf.py). `dtype=torch.float64` is the yardstick;
`dtype=torch.float32` evaluates the same restatement in float32, the reference
arithmetic's own error. Data come from _tip_ref.planted.

  A      = F_b K^T                           [b, Nk]
  phi    = exp(-(beta - beta * A))
  S[r,c] = sum over the keys k of class c of phi[r, k]
  logits = Z_b + alpha * S,  Z = 100 * F W
  loss   = mean cross-entropy(logits, y_b)
  g      = (softmax(logits) - onehot(y_b)) / b
  dA     = alpha * beta * phi * g[:, cls(k)]
  dK     = dA^T F_b                           [Nk, E]

AdamW at 1-based step t of T, betas 0.9 / 0.999:
  lr_t = lr * 0.5 * (1 + cos(pi (t - 1) / T))
  K <- K * (1 - lr_t * wd);  m <- 0.9 m + 0.1 dK;  v <- 0.999 v + 0.001 dK^2
  K <- K - (lr_t / (1 - 0.9^t)) * m / (sqrt(v) / sqrt(1 - 0.999^t) + eps)

Two forms: `closed` (the formulas above) and `autograd` (torch autograd through the forward,
torch.optim.AdamW and CosineAnnealingLR); test_tipf.py pins one to the other in float64.
The float32 restatement's own error is the largest over its forms: closed, autograd, and
closed with Z taken as 100 (F W) instead of (100 F) W (clip_logits).
Epoch e trains on view e % V in the order finetune.cache_order(n, seed, e, shuffle).
"""
import functools
import math

import numpy as np
import torch

import _tip_ref as R

# (b, Nk, E, C, planted() extras): the smallest shapes at which the tiling can go wrong
CASES = [(1, 1, 16, 2, {}),
         (15, 17, 16, 3, {}),
         (17, 65, 48, 20, {"empty_class": 19}),     # one empty class; planted() interleaves
         (33, 130, 64, 20, {}),
         (64, 65, 32, 1, {})]
IDS = ["b{}-k{}-E{}-C{}".format(*c[:4]) for c in CASES]
# G = 1 uses the first configuration, G = 3 all of them: (lr, beta, alpha)
CONFIGS = [(1e-3, 1.0, 1.17), (3e-3, 5.5, 1.0), (2e-4, 3.0, 3.0)]
SEEDS = (1, 2)
WD, EPS = 0.01, 1e-4


def _t(x, dtype):
    return x.to(dtype) if isinstance(x, torch.Tensor) else torch.tensor(np.asarray(x)).to(dtype)


def _one_hot(key_labels, C, dtype):
    kl = R._idx(key_labels)
    oh = torch.zeros(len(kl), C, dtype=dtype)
    oh[torch.arange(len(kl)), kl] = 1
    return oh


def lr_factor(t, T):
    return 0.5 * (1.0 + math.cos(math.pi * (t - 1) / T))


def clip_logits(F, W, z_form="scaled_rows"):
    """Z = 100 F W. The formula does not say where the factor goes; in float64 that is
    immaterial, in float32 (100 F) W ("scaled_rows", _tip_ref.clip_logits' form) and
    100 (F W) ("scaled_product") round differently, and both are the float32 restatement."""
    return (100.0 * F) @ W if z_form == "scaled_rows" else 100.0 * (F @ W)


def forward(K, Fb, Zb, key_labels, beta, alpha):
    """(logits [b, C], phi [b, Nk]) in the dtype of K."""
    C = Zb.shape[1]
    phi = (-(beta - beta * (Fb @ K.t()))).exp()
    return Zb + alpha * (phi @ _one_hot(key_labels, C, K.dtype)), phi


def grad_closed(K, Fb, Zb, yb, key_labels, beta, alpha):
    """(dK, loss, logits) by the closed form."""
    logits, phi = forward(K, Fb, Zb, key_labels, beta, alpha)
    b, C = logits.shape
    g = torch.softmax(logits, dim=1)
    g[torch.arange(b), yb] -= 1
    g = g / b
    dA = alpha * beta * phi * g[:, R._idx(key_labels)]
    loss = torch.nn.functional.cross_entropy(logits, yb)
    return dA.t() @ Fb, loss, logits


def grad_autograd(K, Fb, Zb, yb, key_labels, beta, alpha):
    """(dK, loss, logits) by autograd."""
    Kp = K.clone().requires_grad_(True)
    logits, _ = forward(Kp, Fb, Zb, key_labels, beta, alpha)
    loss = torch.nn.functional.cross_entropy(logits, yb)
    (dK,) = torch.autograd.grad(loss, Kp)
    return dK, loss.detach(), logits.detach()


def adamw_closed(K, m, v, dK, lr, t, T, wd=WD, eps=EPS):
    """One step of the restated AdamW under the cosine schedule; returns (K, m, v)."""
    lr_t = lr * lr_factor(t, T)
    K = K * (1 - lr_t * wd)
    m = 0.9 * m + 0.1 * dK
    v = 0.999 * v + 0.001 * dK * dK
    K = K - (lr_t / (1 - 0.9 ** t)) * m / (v.sqrt() / math.sqrt(1 - 0.999 ** t) + eps)
    return K, m, v


def views_of(d, V, seed):
    """V training views of planted data d: view 0 is d["F"], the others are unit rows a small
    step away from it (float32 numpy, as planted's arrays)."""
    g = torch.Generator().manual_seed(7700 + seed)
    F = torch.tensor(d["F"], dtype=torch.float64)
    out = [d["F"]]
    for _ in range(1, V):
        x = F + 0.3 * F.shape[1] ** -0.5 * torch.randn(F.shape, generator=g, dtype=torch.float64)
        out.append(torch.nn.functional.normalize(x, dim=1).float().numpy())
    return out


def fit(views, labels, K0, W, key_labels, lr, beta, alpha, *, epochs, batch_size, seed=0,
        shuffle=True, wd=WD, eps=EPS, dtype=torch.float64, form="closed", z_form="scaled_rows"):
    """The whole loop for one configuration. Returns a dict:
      keys [epochs, Nk, E]   the keys after every epoch
      ce [steps], correct [steps]   mean CE and correct rows of every batch before its update
      logits                 list of [b_t, C] per step
      rows                   list of the row indices per step"""
    from miclip.finetune import cache_order, cache_view
    Fs = [_t(x, dtype) for x in views]
    Wt = _t(W, dtype)
    Zs = [clip_logits(f, Wt, z_form) for f in Fs]
    y = R._idx(labels)
    n = Fs[0].shape[0]
    spe = (n + batch_size - 1) // batch_size
    T = epochs * spe
    K = _t(K0, dtype).clone()
    m, v = torch.zeros_like(K), torch.zeros_like(K)
    if form == "autograd":
        Kp = K.clone().requires_grad_(True)
        opt = torch.optim.AdamW([Kp], lr=lr, eps=eps, weight_decay=wd)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T)
    out = {"keys": [], "ce": [], "correct": [], "logits": [], "rows": []}
    t = 0
    for e in range(epochs):
        vi = cache_view(e, len(Fs))
        order = cache_order(n, seed, e, shuffle)
        for s in range(spe):
            rows = order[s * batch_size:(s + 1) * batch_size]
            t += 1
            Fb, Zb, yb = Fs[vi][rows], Zs[vi][rows], y[rows]
            if form == "autograd":
                logits, _ = forward(Kp, Fb, Zb, key_labels, beta, alpha)
                loss = torch.nn.functional.cross_entropy(logits, yb)
                opt.zero_grad()
                loss.backward()
                opt.step()
                sched.step()
                logits, loss = logits.detach(), loss.detach()
            else:
                dK, loss, logits = grad_closed(K, Fb, Zb, yb, key_labels, beta, alpha)
                K, m, v = adamw_closed(K, m, v, dK, lr, t, T, wd, eps)
            out["ce"].append(float(loss))
            out["correct"].append(int((logits.argmax(1) == yb).sum()))
            out["logits"].append(logits)
            out["rows"].append(rows)
        out["keys"].append((Kp.detach() if form == "autograd" else K).clone())
    out["keys"] = torch.stack(out["keys"])
    return out


def undecided(l64, l32):
    """Rows of one batch whose float64 top-2 margin is at most 8 x the largest
    |float32 - float64| logit difference (_tip_ref.grid's rule); (count, smallest margin,
    error)."""
    err = float((l32.double() - l64).abs().max())
    if l64.shape[1] < 2:
        return 0, float("inf"), err
    top = l64.topk(2, dim=1).values
    margin = top[:, 0] - top[:, 1]
    return int((margin <= 8 * err).sum()), float(margin.min()), err


def rel(a, ref):
    """Relative Frobenius error of a against ref (0 / 0 = 0)."""
    a, ref = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(ref)).double()
    den = float(ref.norm())
    num = float((a - ref).norm())
    return 0.0 if num == 0 else num / den if den > 0 else float("inf")


@functools.lru_cache(maxsize=None)
def step_case(idx, seed, dname="fp32"):
    """One batch of case idx (n = b) with F rounded to the input type, and the float64 /
    float32 gradients of every configuration at the initial keys, computed once."""
    b, Nk, E, C, extra = CASES[idx]
    d = R.planted(b, Nk, E, C, seed=seed, **extra)
    Fr = torch.tensor(d["F"]).to({"fp32": torch.float32, "fp16": torch.float16}[dname])
    y = R._idx(d["labels"])
    res = {"d": d, "F": Fr, "y": y, "grad64": [], "err32": [], "logits64": []}
    for lr, beta, alpha in CONFIGS:
        per = {}
        for dt in (torch.float64, torch.float32):
            F, K, W = Fr.to(dt), _t(d["K"], dt), _t(d["W"], dt)
            Z = clip_logits(F, W)
            per[dt] = [grad_closed(K, F, Z, y, d["key_labels"], beta, alpha),
                       grad_autograd(K, F, Z, y, d["key_labels"], beta, alpha),
                       grad_closed(K, F, clip_logits(F, W, "scaled_product"), y, d["key_labels"],
                                   beta, alpha)]
        g64 = per[torch.float64][0][0]
        res["grad64"].append(g64.numpy())
        res["logits64"].append(per[torch.float64][0][2].numpy())
        # the float32 restatement's own error: the largest of its forms (closed, autograd,
        # closed with the other placement of the factor 100)
        res["err32"].append(max(rel(r[0], g64) for r in per[torch.float32]))
    return res


@functools.lru_cache(maxsize=None)
def trajectory_case(idx, seed, shuffle, dname="fp32"):
    """2 epochs x 3 steps (batch b, n = 2 b + max(1, b // 2): a partial last batch where b
    allows one) on two views, every configuration, float64 and both float32 forms."""
    b, Nk, E, C, extra = CASES[idx]
    n = 2 * b + max(1, b // 2)
    d = R.planted(n, Nk, E, C, seed=seed, **extra)
    tdt = {"fp32": torch.float32, "fp16": torch.float16}[dname]
    views = [torch.tensor(x).to(tdt) for x in views_of(d, 2, seed)]
    res = {"d": d, "views": views, "n": n, "b": b, "fits": []}
    for lr, beta, alpha in CONFIGS:
        kw = dict(epochs=2, batch_size=b, seed=seed, shuffle=shuffle)
        args = ([x.float() for x in views], d["labels"], d["K"], d["W"], d["key_labels"], lr, beta,
                alpha)
        f64 = fit(*args, dtype=torch.float64, **kw)
        f32 = fit(*args, dtype=torch.float32, **kw)
        # the float32 restatement's own error: the largest of its forms (closed, autograd,
        # closed with the other placement of the factor 100)
        all32 = [f32, fit(*args, dtype=torch.float32, form="autograd", **kw),
                 fit(*args, dtype=torch.float32, z_form="scaled_product", **kw)]
        K0 = torch.tensor(d["K"], dtype=torch.float64)
        und = [undecided(l64, l32) for l64, l32 in zip(f64["logits"], f32["logits"])]
        res["fits"].append({
            "f64": f64, "f32": f32, "all32": all32,
            "err_keys": max(rel(r["keys"][-1].double() - K0, f64["keys"][-1] - K0) for r in all32),
            "err_ce": max(rel(r["ce"], f64["ce"]) for r in all32),
            "undecided": [u[0] for u in und],
            "min_margin": min(u[1] for u in und), "max_err": max(u[2] for u in und)})
    # the history's mean CE is one [steps, G] array: its float64 value and the float32
    # restatement's error on all of it, again the largest over the three forms
    res["ce64"] = np.array([f["f64"]["ce"] for f in res["fits"]]).T
    res["err_ce"] = max(rel(np.array([f["all32"][k]["ce"] for f in res["fits"]]).T, res["ce64"])
                        for k in range(3))
    return res
