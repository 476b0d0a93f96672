"""Embedding-cache visualiser: the device counterpart of feat_cache_vis/feat_vis.py.

    python -m miclip.embed_vis --cache_dir CACHE --tsne [--pca_dim 50] [--out_prefix vis]

loads embeddings.pt / metadata.csv / labels.pt as cache_openclip_embeddings wrote them,
optionally pre-reduces with PCA, embeds in 2-D with exact t-SNE on the device and saves
<prefix>_tsne_coords.npy.

  * t-SNE  (feat_vis.py:150-157, sklearn.manifold.TSNE)   miclip_tsne_affinities /
                                                          miclip_tsne_run
  * PCA    (feat_vis.py:124-137, sklearn PCA)             torch covariance on the device,
                                                          float64 eigh on the host

The t-SNE is scikit-learn 1.7's, rule for rule, in its exact form: dense P and all-pairs
repulsion where scikit-learn's default approximates with Barnes-Hut. The trajectories of
the two differ (the iteration is chaotic); the quality (KL, trustworthiness) is the
same. What stays out: UMAP (umap-learn is not available, so its parity can not be
pinned) and the plotly HTML page.
"""
import argparse
import collections
import ctypes
from pathlib import Path

import numpy as np
import torch

from . import _lib

__all__ = ["TsneResult", "load_cache", "pca_reduce", "affinities", "tsne", "visualize_cache",
           "build_argparser", "main"]

TsneResult = collections.namedtuple("TsneResult", "coords kl_divergence n_iter learning_rate")

METRICS = {"cosine": 0, "euclidean": 1, "precomputed": 2}
N_MIN, N_MAX, D_MAX = 4, 16384, 4096
_EXPLORATION_ITERS = 250      # _t_sne.py _EXPLORATION_MAX_ITER
_N_ITER_CHECK = 50            # _t_sne.py _N_ITER_CHECK
_MIN_GAIN = 0.01


def load_cache(cache_dir):
    """feat_vis.py:93-108 -> (embeddings, metadata DataFrame, labels or None)."""
    import pandas as pd
    cache_root = Path(cache_dir)
    emb_path = cache_root / "embeddings.pt"
    meta_path = cache_root / "metadata.csv"
    lab_path = cache_root / "labels.pt"
    if not emb_path.is_file():
        raise FileNotFoundError(f"Missing embeddings file: {emb_path}")
    if not meta_path.is_file():
        raise FileNotFoundError(f"Missing metadata file: {meta_path}")
    embeddings = torch.load(emb_path, map_location="cpu", weights_only=True)
    metadata = pd.read_csv(meta_path)
    labels = (torch.load(lab_path, map_location="cpu", weights_only=True)
              if lab_path.is_file() else None)
    return embeddings, metadata, labels


def _as_f32(features, device):
    """[N, D] float32 contiguous tensor on `device` from numpy / torch, fp16 / bf16 / fp32."""
    if isinstance(features, np.ndarray):
        arr = np.ascontiguousarray(features)
        t = torch.from_numpy(arr if arr.flags.writeable else arr.copy())
    else:
        t = features.detach()
    if t.dim() != 2:
        raise ValueError(f"features must be [N, D], got shape {tuple(t.shape)}")
    if not t.is_floating_point():
        raise ValueError(f"features must be floating point, got {t.dtype}")
    return t.to(device=device, dtype=torch.float32).contiguous()


def _device(device):
    return torch.device("cuda" if device is None else device)


def pca_reduce(features, k, *, device=None):
    """The PCA pre-reduction of feat_vis.py:124-137 -> (reduced [N, k] float32 numpy,
    explained-variance-ratio sum). Centring, the D x D covariance and the projection run
    on the device in fp32, the eigendecomposition on the host in float64; each
    component's largest-magnitude loading is positive. k >= D skips the reduction with
    the reference's warning and returns (features as float32, None)."""
    k = int(k)
    if k <= 0:
        raise ValueError("pca_dim must be a positive integer.")
    x = _as_f32(features, _device(device))
    if k >= x.shape[1]:
        print(f"[warn] pca_dim={k} >= embedding_dim={x.shape[1]}; skipping PCA.")
        return x.cpu().numpy(), None
    xc = x - x.mean(0, keepdim=True)
    cov = (xc.t() @ xc) / max(x.shape[0] - 1, 1)
    val, vec = np.linalg.eigh(cov.cpu().numpy().astype(np.float64))
    order = np.argsort(val)[::-1][:k]
    vec = vec[:, order]
    sign = np.sign(vec[np.abs(vec).argmax(0), np.arange(k)])
    sign[sign == 0] = 1
    comps = torch.from_numpy((vec * sign).astype(np.float32)).to(x.device)
    return (xc @ comps).cpu().numpy(), float(val[order].sum() / val.sum())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _scratch(n, dev):
    lib = _lib.load_library()
    return torch.empty(int(lib.miclip_tsne_scratch_bytes(n)), device=dev, dtype=torch.uint8)


def affinities(features, *, perplexity=30.0, metric="cosine", device=None, keep_dist=False):
    """The joint probabilities of TSNE._fit on the device -> (P [N, N], beta [N], dist
    [N, N] or None) as float32 device tensors. P is bit-symmetric with a zero diagonal;
    dist is what the perplexity search was fed (squared, as scikit-learn feeds it)."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    dev = _device(device)
    x = _as_f32(features, dev)
    n, d = x.shape
    if metric == "precomputed":
        if n != d:
            raise ValueError(f"a precomputed distance matrix must be square, got {tuple(x.shape)}")
        if bool((x < 0).any()):
            raise ValueError("precomputed distances must be non-negative")
        x = x * x                     # _t_sne.py squares every non-euclidean metric
    lib = _lib.load_library()
    P = torch.empty(n, n, device=dev, dtype=torch.float32)
    beta = torch.empty(n, device=dev, dtype=torch.float32)
    dist = torch.empty(n, n, device=dev, dtype=torch.float32) if keep_dist else None
    scratch = _scratch(n, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.miclip_tsne_affinities(_ptr(x), n, d, METRICS[metric], float(perplexity),
                                              _ptr(P), _ptr(beta), _ptr(dist), _ptr(scratch),
                                              _lib.stream_handle(dev)), "miclip_tsne_affinities")
    return P, beta, dist


def random_init(n, seed):
    """TSNE._fit's init="random": 1e-4 * RandomState(seed).standard_normal((n, 2)), float32."""
    return 1e-4 * np.random.RandomState(seed).standard_normal(size=(n, 2)).astype(np.float32)


def _initial_embedding(features, init, metric, seed, dev):
    n = features.shape[0]
    if isinstance(init, str):
        if init == "random":
            return random_init(n, seed)
        if init == "pca":
            if metric == "precomputed":
                raise ValueError('The parameter init="pca" cannot be used with '
                                 'metric="precomputed".')
            if features.shape[1] < 3:
                raise ValueError('init="pca" needs more than 2 feature dimensions')
            y, _ = pca_reduce(features, 2, device=dev)
            return (y / np.std(y[:, 0]) * 1e-4).astype(np.float32)
        raise ValueError("'init' must be 'pca', 'random', or an [N, 2] array")
    y = np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init,
                   dtype=np.float32)
    if y.shape != (n, 2):
        raise ValueError(f"init must have shape ({n}, 2), got {y.shape}")
    if not np.isfinite(y).all():
        raise ValueError("init contains NaN or infinity")
    return y


def tsne(features, *, perplexity=30.0, metric="cosine", init="pca", seed=1, max_iter=1000,
         early_exaggeration=12.0, learning_rate="auto", n_iter_without_progress=300,
         min_grad_norm=1e-7, device=None):
    """sklearn.manifold.TSNE(n_components=2, ...).fit_transform in its exact form on the
    device -> TsneResult(coords float32 [N, 2], kl_divergence, n_iter, learning_rate).

    scikit-learn's schedule (TSNE._tsne): learning_rate "auto" = max(N / early_exaggeration
    / 4, 50); 250 iterations at the early exaggeration and momentum 0.5 (patience 250),
    then momentum 0.8 up to max_iter; every 50 iterations one read-back of four floats for
    the convergence rules of _gradient_descent. kl_divergence is the error of the last
    iteration run. features: [N, D] (or [N, N] distances for metric="precomputed", squared
    first as scikit-learn does), numpy or torch, on any device, fp16 / bf16 / fp32."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    dev = _device(device)
    x = _as_f32(features, dev)
    n, d = x.shape
    if not N_MIN <= n <= N_MAX:
        raise ValueError(f"N must be in {N_MIN}..{N_MAX}, got {n}")
    if metric != "precomputed" and not 1 <= d <= D_MAX:
        raise ValueError(f"D must be in 1..{D_MAX}, got {d}")
    if not 1 <= perplexity < n:
        raise ValueError(f"perplexity must be in [1, N), got {perplexity} for N = {n}")
    if max_iter < _EXPLORATION_ITERS:
        raise ValueError(f"max_iter must be >= {_EXPLORATION_ITERS}, got {max_iter}")
    if not bool(torch.isfinite(x).all()):
        raise ValueError("features contain NaN or infinity")
    lr = max(n / early_exaggeration / 4, 50) if learning_rate == "auto" else float(learning_rate)
    y0 = _initial_embedding(x, init, metric, seed, dev)

    lib = _lib.load_library()
    P, _, _ = affinities(x, perplexity=perplexity, metric=metric, device=dev)
    y = torch.tensor(y0, dtype=torch.float32, device=dev)
    scratch = _scratch(n, dev)
    stats = torch.zeros(4, device=dev, dtype=torch.float32)
    stream = _lib.stream_handle(dev)

    def descent(it, end, exaggeration, momentum, patience):
        """_gradient_descent from iteration `it`: -> (error, last iteration index)."""
        update = torch.zeros_like(y)
        gains = torch.ones_like(y)
        best, best_it, kl, last = np.inf, it, float("nan"), it
        while it < end:
            nxt = min((it // _N_ITER_CHECK + 1) * _N_ITER_CHECK, end)
            with torch.cuda.device(dev):
                _lib.check(lib.miclip_tsne_run(_ptr(P), n, _ptr(y), _ptr(update), _ptr(gains),
                                               nxt - it, float(exaggeration), float(momentum),
                                               float(lr), _MIN_GAIN, 0, _ptr(scratch),
                                               _ptr(stats), stream), "miclip_tsne_run")
            kl, grad_norm = (float(v) for v in stats.cpu()[:2])
            last = nxt - 1
            if nxt % _N_ITER_CHECK == 0:
                if kl < best:
                    best, best_it = kl, last
                elif last - best_it > patience:
                    break
                if grad_norm <= min_grad_norm:
                    break
            it = nxt
        return kl, last

    kl, it = descent(0, _EXPLORATION_ITERS, early_exaggeration, 0.5, _EXPLORATION_ITERS)
    if it < _EXPLORATION_ITERS or max_iter - _EXPLORATION_ITERS > 0:
        kl, it = descent(it + 1, max_iter, 1.0, 0.8, n_iter_without_progress)
    return TsneResult(y.cpu().numpy(), kl, it, lr)


def visualize_cache(cache_dir, *, pca_dim=None, out_prefix="vis", overwrite=False, seed=1,
                    device=None, **tsne_kw):
    """main() of feat_vis.py:111-181 with --tsne: load the cache, optionally pre-reduce
    with PCA, embed, save <out_prefix>_tsne_coords.npy in the cache folder, and return
    metadata with the columns x and y."""
    embeddings, metadata, labels = load_cache(cache_dir)
    print({"embeddings.shape": tuple(embeddings.shape), "metadata.rows": int(len(metadata)),
           "labels.shape": tuple(labels.shape) if labels is not None else None})
    coords_path = Path(cache_dir) / f"{out_prefix}_tsne_coords.npy"
    if coords_path.exists() and not overwrite:
        raise FileExistsError(f"Output exists: {coords_path} (use --overwrite to replace)")
    features = embeddings
    if pca_dim is not None:
        features, ratio = pca_reduce(embeddings, int(pca_dim), device=device)
        if ratio is not None:
            print({"pca_dim": int(pca_dim), "pca_explained_variance_ratio_sum": ratio,
                   "features.shape": tuple(features.shape)})
    result = tsne(features, seed=seed, device=device, **tsne_kw)
    coords_2d = np.asarray(result.coords)
    print({"reducer": "tsne", "coords_2d.shape": tuple(coords_2d.shape),
           "kl_divergence": result.kl_divergence, "n_iter": result.n_iter})
    coords_path.parent.mkdir(parents=True, exist_ok=True)
    np.save(coords_path, coords_2d)
    print(f"[save] coords -> {coords_path}")
    if coords_2d.shape[0] != len(metadata):
        raise ValueError(f"Row mismatch: coords_2d has {coords_2d.shape[0]} rows, "
                         f"metadata has {len(metadata)} rows.")
    df_plot = metadata.copy()
    df_plot["x"] = coords_2d[:, 0]
    df_plot["y"] = coords_2d[:, 1]
    return df_plot


def build_argparser() -> argparse.ArgumentParser:
    """The flags of feat_vis.py:32-90."""
    parser = argparse.ArgumentParser(description="Visualize cached image embeddings in 2D.")
    parser.add_argument("--cache_dir", type=str, required=True,
                        help="Path to cache folder containing embeddings.pt and metadata.csv.")
    reducer = parser.add_mutually_exclusive_group(required=True)
    reducer.add_argument("--umap", action="store_true", help="UMAP (not available here).")
    reducer.add_argument("--tsne", action="store_true", help="Use t-SNE for 2D reduction.")
    parser.add_argument("--pca_dim", type=int, default=None,
                        help="Optional PCA pre-reduction dimension.")
    parser.add_argument("--out_prefix", type=str, default="vis",
                        help="Output prefix for the coords file.")
    parser.add_argument("--overwrite", action="store_true",
                        help="Overwrite existing outputs if present.")
    parser.add_argument("--color_by", type=str, default="ground_truth_word_label",
                        help="Accepted and ignored: no plot is written.")
    parser.add_argument("--hover", type=str,
                        default="file_name,ground_truth_word_label,ground_truth_num_label",
                        help="Accepted and ignored: no plot is written.")
    parser.add_argument("--umap_neighbors", type=int, default=30, help="UMAP n_neighbors.")
    parser.add_argument("--umap_min_dist", type=float, default=0.1, help="UMAP min_dist.")
    parser.add_argument("--umap_metric", type=str, default="euclidean", help="UMAP metric.")
    parser.add_argument("--tsne_perplexity", type=float, default=30.0, help="t-SNE perplexity.")
    parser.add_argument("--tsne_metric", type=str, default="cosine", help="t-SNE metric.")
    parser.add_argument("--tsne_init", type=str, default="pca", help="t-SNE init method.")
    parser.add_argument("--seed", type=int, default=1, help="Random seed.")
    return parser


def main(argv=None):
    args = build_argparser().parse_args(argv)
    if args.umap:
        raise NotImplementedError(
            "--umap is not built: umap-learn is not available, so a device UMAP could not be "
            "pinned against the reference's; use --tsne")
    print("[note] --color_by and --hover are accepted and ignored: the plotly page is out of "
          "scope, only the coordinates are written")
    return visualize_cache(args.cache_dir, pca_dim=args.pca_dim, out_prefix=args.out_prefix,
                           overwrite=args.overwrite, seed=int(args.seed),
                           perplexity=float(args.tsne_perplexity), metric=str(args.tsne_metric),
                           init=str(args.tsne_init))


if __name__ == "__main__":
    main()
