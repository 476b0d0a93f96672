"""Float64 torch restatement of the Tip-Adapter cache classifier, written from its formulas
(the yardstick of tests/test_tip.py and tests/test_gpu_tip.py; `dtype=torch.float32`
evaluates the same restatement in float32, the reference arithmetic's own error).

  keys      f_v = x_v @ proj / max(|x_v @ proj|, 1e-12) per view; m = mean over the views;
            keys = m / |m| (a plain division)
  affinity  Aff = F @ keys^T
  Z         100 * F @ W
  s_c(beta) sum over the keys k of class c of exp(-(beta - beta * Aff_k))
  logits    Z + alpha * s(beta); the prediction is the first argmax
  search    beta-major scan of the correct counts from 0, replaced on a strictly
            greater count only
"""
import numpy as np
import torch


def lists(scale, step):
    betas = [i * (scale[0] - 0.1) / step[0] + 0.1 for i in range(step[0])]
    alphas = [i * (scale[1] - 0.1) / step[1] + 0.1 for i in range(step[1])]
    return betas, alphas


def _t(x, dtype):
    return x.to(dtype) if isinstance(x, torch.Tensor) else torch.tensor(np.array(x)).to(dtype)


def _idx(x):
    return x.long() if isinstance(x, torch.Tensor) else torch.tensor(np.array(x)).long()


def keys(views, proj, dtype=torch.float64):
    """[Nk, E] from the views [A][Nk, Wv] and proj [Wv, E]."""
    P = _t(proj, dtype)
    total = None
    for x in views:
        z = _t(x, dtype) @ P
        f = z / z.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        total = f if total is None else total + f
    m = total / len(views)
    return m / m.norm(dim=-1, keepdim=True)


def affinity(F, K, dtype=torch.float64):
    return _t(F, dtype) @ _t(K, dtype).t()


def clip_logits(F, W, dtype=torch.float64):
    return (100.0 * _t(F, dtype)) @ _t(W, dtype)


def class_sums(aff, key_labels, C, beta, dtype=torch.float64):
    one_hot = torch.zeros(len(key_labels), C, dtype=dtype)
    one_hot[torch.arange(len(key_labels)), _idx(key_labels)] = 1
    return (-(beta - beta * _t(aff, dtype))).exp() @ one_hot


def logits(Z, aff, key_labels, beta, alpha, dtype=torch.float64):
    Z = _t(Z, dtype)
    return Z + class_sums(aff, key_labels, Z.shape[1], beta, dtype) * alpha


def scan(counts, betas, alphas):
    """(best_beta, best_alpha, best_count) of the beta-major strict-> scan from 0."""
    best, bb, ba = 0, 0, 0
    for ib, beta in enumerate(betas):
        for ia, alpha in enumerate(alphas):
            if int(counts[ib][ia]) > best:
                best, bb, ba = int(counts[ib][ia]), beta, alpha
    return bb, ba, best


def grid(F, K, key_labels, W, labels, betas, alphas, aff=None):
    """The whole grid in float64 and float32 on the same inputs (aff: a supplied affinity
    instead of F @ K^T). Returns a dict of numpy arrays:
      aff64 / aff32, Z64 / Z32          the shared operands
      counts [nb, na]                   float64 correct counts
      counts32 [nb, na]                 the float32 restatement's
      margin [nb, na, Nq]               float64 top-2 logit margin of every row (inf for C = 1)
      err [nb, na]                      largest |float32 logit - float64 logit| at the pair
      undecided [nb, na]                rows with margin <= 8 * err at the pair
      zero_shot                         float64 correct count of Z alone"""
    lab = _idx(labels)
    out = {}
    per = {}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        a = affinity(F, K, dt) if aff is None else _t(aff, dt)
        Z = clip_logits(F, W, dt)
        C = Z.shape[1]
        L = torch.empty(len(betas), len(alphas), Z.shape[0], C, dtype=dt)
        for ib, beta in enumerate(betas):
            S = class_sums(a, key_labels, C, beta, dt)
            for ia, alpha in enumerate(alphas):
                L[ib, ia] = Z + S * alpha
        per[name] = L
        out["aff" + name], out["Z" + name] = a.numpy(), Z.numpy()
    L64, L32 = per["64"], per["32"].double()
    out["counts"] = (L64.argmax(-1) == lab).sum(-1).numpy()
    out["counts32"] = (per["32"].argmax(-1) == lab).sum(-1).numpy()
    if L64.shape[-1] > 1:
        top = L64.topk(2, dim=-1).values
        out["margin"] = (top[..., 0] - top[..., 1]).numpy()
    else:
        out["margin"] = np.full(L64.shape[:-1], np.inf)
    out["err"] = (L32 - L64).abs().amax(dim=(-1, -2)).numpy()
    out["undecided"] = (out["margin"] <= 8 * out["err"][..., None]).sum(-1)
    out["zero_shot"] = int((torch.tensor(out["Z64"]).argmax(-1) == lab).sum())
    return out


def planted(Nq, Nk, E, C, seed, noise=2.5, rotate=3.5, empty_class=None, equal=False, dup=0):
    """Few-shot data around C planted directions: unit keys (class k % C, or skipping
    `empty_class`), unit queries around the directions, text weights [E, C] that are the
    directions deliberately rotated by `rotate`. equal: key 0 is query 0 exactly;
    dup: keys 1 .. dup repeat key 0. float32 numpy arrays; labels int64."""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(C, E, generator=g, dtype=torch.float64), dim=1)
    owners = [c for c in range(C) if c != empty_class] or [0]
    klab = torch.tensor([owners[k % len(owners)] for k in range(Nk)])
    qlab = torch.randint(0, C, (Nq,), generator=g)
    if empty_class is not None and C > 1:
        qlab[qlab == empty_class] = owners[0]

    def around(lab, amount):
        x = dirs[lab] + amount * E ** -0.5 * torch.randn(len(lab), E, generator=g, dtype=torch.float64)
        return torch.nn.functional.normalize(x, dim=1)

    K, F = around(klab, noise), around(qlab, noise)
    W = around(torch.arange(C), rotate).t().contiguous()
    K, F, W = K.float(), F.float(), W.float()
    if equal:
        K[0], klab[0] = F[0], qlab[0]
    for d in range(1, min(dup, Nk - 1) + 1):
        K[d], klab[d] = K[0], klab[0]
    return {"F": F.numpy(), "K": K.numpy(), "W": W.numpy(), "key_labels": klab.numpy(),
            "labels": qlab.numpy()}
