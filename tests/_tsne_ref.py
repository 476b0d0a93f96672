"""NumPy restatement of exact t-SNE as scikit-learn 1.7 computes it -- the yardstick of
the device kernels (csrc/tsne.hip). Every function takes `dtype`: float64 is the
reference, float32 is the same arithmetic at the device's storage precision and gives
the reference's own rounding error (the tolerance rule of test_gpu_tsne.py).

Restated from sklearn/manifold/_t_sne.py (_joint_probabilities, _kl_divergence,
_gradient_descent, TSNE._fit, TSNE._tsne) and _utils._binary_search_perplexity; the
objective is in the separable form the device uses,
    g_i = 4 (exaggeration * sum_j p w (y_i - y_j) - sum_j w^2 (y_i - y_j) / Z),
    KL  = sum pe log max(pe, eps) - sum pe log w + log Z * sum pe,   pe = exaggeration * p,
which is scikit-learn's with Q = w / Z left unfloored (test_tsne_ref.py pins the two).
"""
import numpy as np
import torch

EPS = float(np.finfo(np.double).eps)
EXPLORATION_ITERS = 250
N_ITER_CHECK = 50


def planted(n, d, n_clusters=5, seed=0, dup=0, spread=0.35):
    """Unit-norm rows around `n_clusters` planted directions; the last `dup` rows repeat
    the first `dup`. float32."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d))
    lab = np.arange(n) % n_clusters
    x = centres[lab] + spread * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = x.astype(np.float32)
    if dup:
        x[n - dup:] = x[:dup]
    return x


def cosine_distance(x, dtype=np.float64):
    """sklearn.metrics.pairwise.cosine_distances: clip(1 - x^ x^T, 0, 2), zero diagonal."""
    x = np.asarray(x, dtype)
    nrm = np.sqrt((x * x).sum(1))
    nrm[nrm == 0] = 1
    xn = x / nrm[:, None]
    d = 1 - xn @ xn.T
    np.clip(d, 0, 2, out=d)
    np.fill_diagonal(d, 0)
    return d


def distances(x, metric, dtype=np.float64):
    """What TSNE._fit feeds the perplexity search (method exact)."""
    if metric == "cosine":
        d = cosine_distance(x, dtype)
        return d * d                      # _t_sne.py: every non-euclidean metric is squared
    if metric == "euclidean":
        x = np.asarray(x, dtype)
        sq = (x * x).sum(1)
        d = sq[:, None] + sq[None, :] - 2 * (x @ x.T)
        np.maximum(d, 0, out=d)
        np.fill_diagonal(d, 0)
        return d
    if metric == "precomputed":
        d = np.asarray(x, dtype)
        return d * d
    raise ValueError(metric)


def binary_search_perplexity(d, perplexity, dtype=np.float64):
    """_utils._binary_search_perplexity over all rows at once -> (conditional P, beta).
    beta is the value the returned row was evaluated at."""
    d = np.asarray(d, dtype)
    n = d.shape[0]
    target = dtype(np.log(perplexity))
    beta = np.ones(n, dtype)
    bmin = np.full(n, -np.inf, dtype)
    bmax = np.full(n, np.inf, dtype)
    active = np.ones(n, bool)
    P = np.zeros((n, n), dtype)
    for step in range(100):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        p = np.exp(-d[idx] * beta[idx, None])
        p[np.arange(idx.size), idx] = 0
        s = p.sum(1)
        s[s == 0] = dtype(1e-8)
        H = np.log(s) + beta[idx] * ((d[idx] * p).sum(1) / s)
        P[idx] = p / s[:, None]
        diff = H - target
        done = np.abs(diff) <= dtype(1e-5)
        active[idx[done]] = False
        if step == 99:
            break
        up = idx[~done & (diff > 0)]
        dn = idx[~done & ~(diff > 0)]
        bmin[up] = beta[up]
        beta[up] = np.where(np.isinf(bmax[up]), beta[up] * 2, (beta[up] + bmax[up]) / 2)
        bmax[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(bmin[dn]), beta[dn] / 2, (beta[dn] + bmin[dn]) / 2)
    return P, beta


def joint_probabilities(d, perplexity, dtype=np.float64):
    """_joint_probabilities as a dense [N, N] matrix with a zero diagonal -> (P, beta)."""
    C, beta = binary_search_perplexity(d, perplexity, dtype)
    P = C + C.T
    s = max(P.sum(dtype=dtype), dtype(EPS))
    P = np.maximum(P / s, dtype(EPS))
    np.fill_diagonal(P, 0)
    return P, beta


def row_entropy(P_joint):
    """Conditional entropy of each row of a joint P (float64), for the perplexity check."""
    P = np.asarray(P_joint, np.float64)
    c = P / P.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(c > 0, c * np.log(c), 0.0)
    return -t.sum(1)


def objective(P, y, exaggeration=1.0, dtype=np.float64, compute_error=True):
    """-> (KL, grad [N, 2], Z) in the separable form of the module docstring."""
    P = np.asarray(P, dtype)
    y = np.asarray(y, dtype)
    ex = dtype(exaggeration)
    diff = y[:, None, :] - y[None, :, :]
    w = 1 / (1 + (diff * diff).sum(-1))
    np.fill_diagonal(w, 0)
    Z = w.sum(1).sum()
    attr = ((P * w)[:, :, None] * diff).sum(1)
    rep = ((w * w)[:, :, None] * diff).sum(1)
    g = 4 * (ex * attr - rep / Z)
    kl = dtype(np.nan)
    if compute_error:
        pe = P * ex
        np.fill_diagonal(w, 1)
        a = (pe * np.log(np.maximum(pe, dtype(EPS)))).sum()
        b = (pe * np.log(w)).sum()
        kl = a - b + np.log(Z) * pe.sum()
    return kl, g.astype(dtype), Z


def step(P, y, update, gains, exaggeration, momentum, lr, min_gain=0.01, dtype=np.float64,
         compute_error=True):
    """One iteration of _gradient_descent -> dict(y, update, gains, kl, grad_norm, Z, g);
    g is the gradient before the gains multiply, grad_norm is taken after it."""
    y = np.asarray(y, dtype)
    update = np.asarray(update, dtype)
    gains = np.asarray(gains, dtype).copy()
    kl, g, Z = objective(P, y, exaggeration, dtype, compute_error)
    inc = update * g < 0
    gains[inc] += dtype(0.2)
    gains[~inc] *= dtype(0.8)
    np.clip(gains, dtype(min_gain), np.inf, out=gains)
    gg = g * gains
    update = dtype(momentum) * update - dtype(lr) * gg
    return {"y": y + update, "update": update, "gains": gains, "kl": kl,
            "grad_norm": np.sqrt((gg * gg).sum()), "Z": Z, "g": g}


def _descent(P, y, update, gains, it, max_iter, exaggeration, momentum, lr, patience,
             min_grad_norm, dtype):
    best, best_it, kl, i = np.inf, it, np.nan, it
    for i in range(it, max_iter):
        check = (i + 1) % N_ITER_CHECK == 0
        r = step(P, y, update, gains, exaggeration, momentum, lr, 0.01, dtype,
                 compute_error=check or i == max_iter - 1)
        y, update, gains = r["y"], r["update"], r["gains"]
        if check or i == max_iter - 1:
            kl = float(r["kl"])
        if check:
            if kl < best:
                best, best_it = kl, i
            elif i - best_it > patience:
                break
            if r["grad_norm"] <= min_grad_norm:
                break
    return y, kl, i


def learning_rate_auto(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4, 50)


def run_schedule(P, y0, max_iter=1000, early_exaggeration=12.0, lr=None,
                 n_iter_without_progress=300, min_grad_norm=1e-7, dtype=np.float64):
    """TSNE._tsne: 250 iterations at early exaggeration and momentum 0.5, then momentum
    0.8 up to max_iter -> (y, KL of the last iteration run, n_iter)."""
    n = P.shape[0]
    lr = learning_rate_auto(n, early_exaggeration) if lr is None else lr
    y = np.asarray(y0, dtype)
    z, o = np.zeros_like(y), np.ones_like(y)
    y, kl, it = _descent(P, y, z, o, 0, EXPLORATION_ITERS, early_exaggeration, 0.5, lr,
                         EXPLORATION_ITERS, min_grad_norm, dtype)
    if it < EXPLORATION_ITERS or max_iter - EXPLORATION_ITERS > 0:
        y, kl, it = _descent(P, y, np.zeros_like(y), np.ones_like(y), it + 1, max_iter, 1.0,
                             0.8, lr, n_iter_without_progress, min_grad_norm, dtype)
    return y, kl, it


def pca_init(x, dtype=np.float64):
    """Top-2 exact PCA scaled as TSNE._fit does: y / std(y[:, 0]) * 1e-4; each component's
    largest-magnitude loading is positive."""
    comps, _ = pca(x, 2, dtype)
    return (comps / np.std(comps[:, 0]) * 1e-4).astype(np.float32)


def pca(x, k, dtype=np.float64):
    """Covariance eigendecomposition -> (scores [N, k], explained-variance-ratio sum)."""
    x = np.asarray(x, dtype)
    xc = x - x.mean(0)
    cov = (xc.T @ xc) / dtype(max(x.shape[0] - 1, 1))
    val, vec = np.linalg.eigh(cov.astype(np.float64))
    order = np.argsort(val)[::-1][:k]
    vec = vec[:, order]
    sign = np.sign(vec[np.abs(vec).argmax(0), np.arange(vec.shape[1])])
    sign[sign == 0] = 1
    vec = (vec * sign).astype(dtype)
    return xc @ vec, float(val[order].sum() / val.sum())


# ---- the same restatement in torch, for sizes at which NumPy on the host takes minutes ----
def t_joint_probabilities(d, perplexity, dtype):
    d = d.to(dtype)
    n = d.shape[0]
    eye = torch.eye(n, dtype=torch.bool, device=d.device)
    target = torch.log(torch.tensor(perplexity, dtype=dtype, device=d.device))
    beta = torch.ones(n, dtype=dtype, device=d.device)
    bmin, bmax = torch.full_like(beta, -np.inf), torch.full_like(beta, np.inf)
    active = torch.ones(n, dtype=torch.bool, device=d.device)
    C = torch.zeros_like(d)
    for step in range(100):
        if not bool(active.any()):
            break
        p = torch.exp(-d * beta[:, None]).masked_fill_(eye, 0)
        s = p.sum(1)
        s = torch.where(s == 0, torch.full_like(s, 1e-8), s)
        H = torch.log(s) + beta * ((d * p).sum(1) / s)
        C = torch.where(active[:, None], p / s[:, None], C)
        diff = H - target
        done = diff.abs() <= 1e-5
        active = active & ~done
        if step == 99:
            break
        up, dn = active & (diff > 0), active & ~(diff > 0)
        bmin = torch.where(up, beta, bmin)
        bmax = torch.where(dn, beta, bmax)
        beta = torch.where(up, torch.where(torch.isinf(bmax), beta * 2, (beta + bmax) / 2), beta)
        beta = torch.where(dn, torch.where(torch.isinf(bmin), beta / 2, (beta + bmin) / 2), beta)
    P = C + C.t()
    P = torch.clamp(P / torch.clamp(P.sum(), min=EPS), min=EPS).masked_fill_(eye, 0)
    return P, beta


def t_objective(P, y, exaggeration, dtype):
    P, y = P.to(dtype), y.to(dtype)
    n = P.shape[0]
    eye = torch.eye(n, dtype=torch.bool, device=P.device)
    dx, dy = y[:, None, 0] - y[None, :, 0], y[:, None, 1] - y[None, :, 1]
    w1 = 1 / (1 + dx * dx + dy * dy)
    w = w1.masked_fill(eye, 0)
    Z = w.sum(1).sum()
    pw, ww = P * w, w * w
    attr = torch.stack(((pw * dx).sum(1), (pw * dy).sum(1)), 1)
    rep = torch.stack(((ww * dx).sum(1), (ww * dy).sum(1)), 1)
    g = 4 * (exaggeration * attr - rep / Z)
    pe = P * exaggeration
    kl = ((pe * torch.log(torch.clamp(pe, min=EPS))).sum() - (pe * torch.log(w1)).sum()
          + torch.log(Z) * pe.sum())
    return kl, g, Z
