"""Outlier scoring of the embeddings cache on the GPU.

Counterpart of tools/outlier_cleaning.py (same names, arguments, outputs and
errors): `CachePaths`, `CentroidResult`, `MultiPrototypeResult`,
`resolve_cache_paths`, `load_cache`, `SingleCentroidScorer`,
`MultiPrototypeScorer`. The arithmetic on the embeddings runs in the HIP
kernels of csrc/scoring.hip through the C ABI:

  * row norms / re-normalisation      miclip_row_norms        (:229-247)
  * class centroids                   miclip_class_centroids  (:250-291)
  * trimmed class centroids           miclip_trimmed_centroids (:250-257, the
    (compute_centroids(trim_frac=))   reserved "trimmed-centroid support")
  * cosine to own centroid            miclip_proto_scores     (:293-383)
  * nearest own-class prototype and
    best other-class prototype        miclip_proto_scores     (:557-760)
  * k-means fit of the prototypes     miclip_kmeans_seed /
    (compute_prototypes(kmeans=       miclip_kmeans_lloyd     (:511-541)
    "device"))

What stays on the host, as in the reference: label bookkeeping
(torch.unique) and the pandas ranking / quantile / sort post-processing. The
k-means fit of compute_prototypes has two backends: kmeans="sklearn" (the
default) is the reference's scikit-learn KMeans with its parameters (:488-498),
one host fit per class; kmeans="device" runs every (class, restart) pair as one
problem of a single seeding launch and a single Lloyd launch (csrc/kmeans.hip),
with no host round trip and without scikit-learn, which only the "sklearn"
backend imports. The two backends draw different seeds, so on unstructured data
they may settle in different, equally valid local optima. Embeddings live on
the HIP device; there is no CPU fallback.
"""
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import ctypes
import math
import numbers

import numpy as np
import pandas as pd
import torch

from . import _lib


@dataclass
class CachePaths:
    cache_dir: Path
    embeddings: Path
    labels: Path
    metadata: Path
    meta_json: Optional[Path] = None


@dataclass
class CentroidResult:
    centroids: Dict[int, torch.Tensor]
    class_counts: Dict[int, int]
    dim: int
    # set by compute_centroids(trim_frac=...) only; class_counts stays the full class size
    trim_frac: Optional[float] = None
    kept_counts: Optional[Dict[int, int]] = None
    kept_mask: Optional[np.ndarray] = None          # bool [N] on the host, sample order
    rounds_changed: Optional[List[int]] = None      # flags flipped in each trimming round


@dataclass
class MultiPrototypeResult:
    prototypes: Dict[int, torch.Tensor]
    class_counts: Dict[int, int]
    prototype_counts: Dict[int, List[int]]
    k_per_class: Dict[int, int]
    dim: int


def resolve_cache_paths(cache_dir: Path) -> CachePaths:
    """embeddings.pt / labels.pt / metadata.csv / meta.json under cache_dir
    (the layout cache_openclip_embeddings writes)."""
    cache_dir = Path(cache_dir)
    return CachePaths(cache_dir=cache_dir, embeddings=cache_dir / "embeddings.pt",
                      labels=cache_dir / "labels.pt", metadata=cache_dir / "metadata.csv",
                      meta_json=cache_dir / "meta.json")


def _load_tensor_cpu(path: Path) -> torch.Tensor:
    """A cache file holds one tensor (loaded with weights_only=True)."""
    obj = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(obj, torch.Tensor):
        return obj
    raise TypeError(f"Expected tensor at '{path}', got {type(obj).__name__}.")


def _validate_embeddings_labels(embeddings, labels, *, allow_empty=False):
    """Shape / dtype / row-count checks on an (embeddings [N, D], labels [N]) pair.

    Returns (embeddings, labels as int64 [N], N, D). The error types and texts
    are the reference's (tools/outlier_cleaning.py), since callers match on them.
    A [N, 1] label column is accepted as [N]."""
    if labels.ndim == 2 and labels.shape[-1] == 1:
        labels = labels[:, 0]
    checks = (
        (embeddings.ndim == 2, ValueError,
         lambda: f"Expected embeddings shape [N, D], got {tuple(embeddings.shape)}."),
        (labels.ndim == 1, ValueError,
         lambda: f"Expected labels shape [N], got {tuple(labels.shape)}."),
        (embeddings.is_floating_point(), TypeError,
         lambda: f"Expected floating embeddings, got dtype={embeddings.dtype}."),
    )
    for ok, exc, msg in checks:
        if not ok:
            raise exc(msg())
    n, d = (int(v) for v in embeddings.shape)
    if labels.shape[0] != n:
        raise ValueError(f"Row mismatch between embeddings and labels: {n} vs {int(labels.shape[0])}.")
    if n == 0 and not allow_empty:
        raise ValueError("Empty inputs: no samples available.")
    return embeddings, labels.long(), n, d


def load_cache(paths: CachePaths) -> Tuple[torch.Tensor, torch.Tensor, pd.DataFrame]:
    """(embeddings, labels, metadata) of a cache directory, rows cross-checked:
    the three files exist, embeddings / labels are a consistent pair, metadata.csv
    has one row per sample with file_name and ground_truth_num_label, and its labels
    equal labels.pt row for row (the first disagreeing row is reported)."""
    files = (paths.embeddings, paths.labels, paths.metadata)
    absent = [str(f) for f in files if not Path(f).is_file()]
    if absent:
        raise FileNotFoundError("Missing cache file(s): " + ", ".join(absent))
    embeddings, labels, n, _ = _validate_embeddings_labels(_load_tensor_cpu(paths.embeddings),
                                                           _load_tensor_cpu(paths.labels))
    metadata = pd.read_csv(paths.metadata)
    if len(metadata) != n:
        raise ValueError(f"Row mismatch between embeddings and metadata: {n} vs {len(metadata)}.")
    need = sorted({"file_name", "ground_truth_num_label"}.difference(metadata.columns))
    if need:
        raise ValueError(f"metadata.csv is missing required column(s): {', '.join(need)}")
    csv_labels = metadata["ground_truth_num_label"].astype(int).to_numpy()
    diff = np.flatnonzero(csv_labels != labels.numpy())
    if diff.size:
        i = int(diff[0])
        raise ValueError(f"Label mismatch between labels.pt and metadata.csv at row {i}: "
                         f"labels.pt={int(labels[i])}, metadata.csv={int(csv_labels[i])}.")
    return embeddings, labels, metadata


# ------------------------------------------------------------------ device ops
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return _lib.stream_handle(dev)


def _row_norms(x: torch.Tensor, eps: float = 1e-12, normalize: bool = False):
    lib = _lib.load_library()
    norms = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    out = torch.empty_like(x) if normalize else None
    with torch.cuda.device(x.device):
        _lib.check(lib.miclip_row_norms(_ptr(x), x.shape[0], x.shape[1], _ptr(norms), float(eps),
                                        _ptr(out), _stream(x.device)), "miclip_row_norms")
    return norms, out


def _class_centroids(x: torch.Tensor, inv: np.ndarray, K: int, eps: float):
    """normalize(per-class mean) with the rows of each class summed in sample order."""
    cent, counts, _ = _class_layout(x, inv, K, eps)
    return cent, counts


def _csr_layout(inv: np.ndarray, K: int, dev):
    """The class layout every per-class kernel walks: (order, offsets) as device int32
    and the host counts [K]. Class k's rows are order[offsets[k] .. offsets[k + 1]), in
    ascending sample order (a stable sort of the class indices)."""
    order = np.argsort(inv, kind="stable").astype(np.int32)
    counts = np.bincount(inv, minlength=K)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return torch.from_numpy(order).to(dev), torch.from_numpy(offsets).to(dev), counts


def _class_layout(x: torch.Tensor, inv: np.ndarray, K: int, eps: float):
    """_class_centroids plus the device class layout it was computed on:
    (centroids, counts, {"order", "offsets" (device int32), "sums" [K, D]})."""
    lib = _lib.load_library()
    dev = x.device
    order_d, off_d, counts = _csr_layout(inv, K, dev)
    D = x.shape[1]
    sums = torch.empty(K, D, device=dev, dtype=torch.float32)
    cent = torch.empty(K, D, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.miclip_class_centroids(_ptr(x), _ptr(order_d), _ptr(off_d), K, D,
                                              float(eps), _ptr(sums), _ptr(cent), _stream(dev)),
                   "miclip_class_centroids")
    return cent, counts, {"order": order_d, "offsets": off_d, "sums": sums}


_TRIM_TILE, _TRIM_MAX_CLASS_ROWS, _TRIM_MAX_ROUNDS = 1024, 65536, 8   # limits of csrc/trim.hip


def _segment_rank(values: torch.Tensor, order_d: torch.Tensor, off_d: torch.Tensor, K: int):
    """miclip_segment_rank: 0-based rank of every row inside its class by the key
    (value ascending, sample index ascending); int32 [N] in sample order."""
    lib = _lib.load_library()
    N, dev = values.shape[0], values.device
    rank = torch.empty(N, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        _lib.check(lib.miclip_segment_rank(_ptr(values), _ptr(order_d), _ptr(off_d), K, N,
                                           _ptr(rank), _stream(dev)), "miclip_segment_rank")
    return rank


def _trim_drop(counts, trim_frac: float) -> np.ndarray:
    """drop[k] = floor(trim_frac * n_k), in Python float64 on the host."""
    return np.asarray([int(math.floor(float(trim_frac) * int(n))) for n in counts], np.int32)


def _trimmed_centroids(x: torch.Tensor, inv: np.ndarray, K: int, drop: np.ndarray, rounds: int,
                       eps: float):
    """miclip_trimmed_centroids on the class layout of `inv`: every round on the
    device in one call. Returns device tensors {"centroids", "sums" [K, D], "keep"
    uint8 [N], "sims" [N], "changed" int32 [rounds]} and the host "counts" [K]."""
    lib = _lib.load_library()
    N, D = x.shape
    dev = x.device
    order_d, off_d, counts = _csr_layout(inv, K, dev)
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)   # noqa: E731
    cls_d, drop_d = as_dev(inv), as_dev(drop)
    out = {"sums": torch.empty(K, D, device=dev, dtype=torch.float32),
           "centroids": torch.empty(K, D, device=dev, dtype=torch.float32),
           "keep": torch.empty(N, device=dev, dtype=torch.uint8),
           "sims": torch.empty(N, device=dev, dtype=torch.float32),
           "changed": torch.empty(int(rounds), device=dev, dtype=torch.int32)}
    with torch.cuda.device(dev):
        _lib.check(lib.miclip_trimmed_centroids(
            _ptr(x), _ptr(order_d), _ptr(off_d), _ptr(cls_d), _ptr(drop_d), K, N, D, int(rounds),
            float(eps), _ptr(out["sums"]), _ptr(out["centroids"]), _ptr(out["keep"]),
            _ptr(out["sims"]), _ptr(out["changed"]), _stream(dev)), "miclip_trimmed_centroids")
    out["counts"] = counts
    return out


def _trim_groups(counts, limit: int) -> List[List[int]]:
    """Consecutive classes packed into groups of at most `limit` rows each (a class is
    never split; the caller has checked that none is larger than `limit`)."""
    groups, rows = [[]], 0
    for k, n in enumerate(counts):
        if groups[-1] and rows + int(n) > limit:
            groups.append([])
            rows = 0
        groups[-1].append(k)
        rows += int(n)
    return groups


def _trimmed_centroids_grouped(x: torch.Tensor, inv: np.ndarray, K: int, drop: np.ndarray,
                               rounds: int, eps: float, limit: int = _TRIM_MAX_CLASS_ROWS):
    """_trimmed_centroids for any number of rows. One call takes at most `limit` rows, and
    trimming a class touches that class's rows only, so a larger cache goes through one
    call per group of _trim_groups, each on a gathered copy of its rows (ascending sample
    order, so every sum keeps its order: the results are those of a single call, bit for
    bit). Returns {"centroids" [K, D], "keep" uint8 [N], "changed" int32 [rounds]} on the
    device and the host "counts"; nothing is read back."""
    counts = np.bincount(inv, minlength=K)
    groups = _trim_groups(counts, limit)
    if len(groups) == 1:
        return _trimmed_centroids(x, inv, K, drop, rounds, eps)
    dev = x.device
    cent = torch.empty(K, x.shape[1], device=dev, dtype=torch.float32)
    keep = torch.empty(x.shape[0], device=dev, dtype=torch.uint8)
    changed = torch.zeros(int(rounds), device=dev, dtype=torch.int32)
    first = np.cumsum([0] + [len(g) for g in groups])
    group_of = np.repeat(np.arange(len(groups)), [len(g) for g in groups])
    for gi, g in enumerate(groups):
        rows = np.flatnonzero(group_of[inv] == gi)            # ascending sample order
        rows_d = torch.from_numpy(rows).to(dev)
        out = _trimmed_centroids(x.index_select(0, rows_d).contiguous(), inv[rows] - first[gi],
                                 len(g), drop[g[0]:g[-1] + 1], rounds, eps)
        cent[g[0]:g[-1] + 1] = out["centroids"]
        keep[rows_d] = out["keep"]
        changed += out["changed"]
    return {"centroids": cent, "keep": keep, "changed": changed, "counts": counts}


def _proto_scores(x, protos, owner, cls, inv_nx=None, inv_np=None):
    lib = _lib.load_library()
    N, D = x.shape
    P = protos.shape[0]
    dev = x.device
    own = torch.empty(N, device=dev, dtype=torch.float32)
    arg = torch.empty(N, device=dev, dtype=torch.int32)
    oth = torch.empty(N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.miclip_proto_scores(_ptr(x), _ptr(protos), _ptr(owner), _ptr(cls),
                                           _ptr(inv_nx), _ptr(inv_np), N, P, D, _ptr(own),
                                           _ptr(arg), _ptr(oth), _stream(dev)),
                   "miclip_proto_scores")
    return own, arg, oth


_KMEANS_MAX_K, _KMEANS_MAX_D, _KMEANS_SLOTS = 16, 1024, 16   # limits of csrc/kmeans.hip


def _kmeans_table(counts, classes, ks, n_init, dev):
    """Problem table of miclip_kmeans_*: n_init consecutive problems per class of
    `classes` (indices into the class layout) with ks[i] clusters; a problem's rows
    of the per-row buffers start at "off"."""
    prob_class = np.repeat(np.asarray(classes, np.int64), n_init)
    prob_k = np.repeat(np.asarray(ks, np.int64), n_init)
    rows = np.asarray(counts, np.int64)[prob_class]
    total = int(rows.sum())
    if total >= 2 ** 31:
        raise ValueError(f"k-means problem table too large: {total} rows over all restarts.")
    prob_off = np.concatenate([[0], np.cumsum(rows)[:-1]])
    as_dev = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)   # noqa: E731
    return {"cls": as_dev(prob_class), "k": as_dev(prob_k), "off": as_dev(prob_off),
            "Pn": int(prob_class.size), "k_max": int(prob_k.max()), "total": total}


def _kmeans_seed(x, layout, table, u, scratch=None):
    """miclip_kmeans_seed: (picks [Pn, 16] int32, centres [Pn, 16, D]) from uniforms u [Pn, 16]."""
    lib = _lib.load_library()
    dev, D, Pn = x.device, x.shape[1], table["Pn"]
    if scratch is None:
        scratch = torch.empty(table["total"], device=dev, dtype=torch.float32)
    picks = torch.empty(Pn, _KMEANS_SLOTS, device=dev, dtype=torch.int32)
    centres = torch.zeros(Pn, _KMEANS_SLOTS, D, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.miclip_kmeans_seed(_ptr(x), _ptr(layout["order"]), _ptr(layout["offsets"]),
                                          D, _ptr(table["cls"]), _ptr(table["k"]),
                                          _ptr(table["off"]), Pn, table["k_max"], _ptr(u),
                                          _ptr(scratch), _ptr(picks), _ptr(centres), _stream(dev)),
                   "miclip_kmeans_seed")
    return picks, centres


def _kmeans_lloyd(x, layout, table, tol, max_iter, centres, scratch=None):
    """miclip_kmeans_lloyd from `centres` [Pn, 16, D], which is updated in place."""
    lib = _lib.load_library()
    dev, D, Pn = x.device, x.shape[1], table["Pn"]
    if scratch is None:
        scratch = torch.empty(table["total"], device=dev, dtype=torch.float32)
    out = {"centres": centres,
           "labels": torch.empty(table["total"], device=dev, dtype=torch.int32),
           "inertia": torch.empty(Pn, device=dev, dtype=torch.float32),
           "n_iter": torch.empty(Pn, device=dev, dtype=torch.int32),
           "strict": torch.empty(Pn, device=dev, dtype=torch.int32),
           "counts": torch.empty(Pn, _KMEANS_SLOTS, device=dev, dtype=torch.int32)}
    with torch.cuda.device(dev):
        _lib.check(lib.miclip_kmeans_lloyd(_ptr(x), _ptr(layout["order"]), _ptr(layout["offsets"]),
                                           D, _ptr(table["cls"]), _ptr(table["k"]),
                                           _ptr(table["off"]), Pn, table["k_max"], _ptr(tol),
                                           int(max_iter), _ptr(scratch), _ptr(centres),
                                           _ptr(out["labels"]), _ptr(out["inertia"]),
                                           _ptr(out["n_iter"]), _ptr(out["strict"]),
                                           _ptr(out["counts"]), _stream(dev)),
                   "miclip_kmeans_lloyd")
    return out


def _kmeans_class_tol(x, layout, counts, rel=1e-4):
    """scikit-learn's scaled tolerance per class, on the device: rel * mean over the
    columns of the column variance = rel * (sum |x|^2 / n - |sum x / n|^2) / D, from the
    class sums of miclip_class_centroids and the row norms (fp64, class order)."""
    norms, _ = _row_norms(x)
    off = layout["offsets"].long()
    sq = norms.double().square().index_select(0, layout["order"].long())
    run = torch.cat([sq.new_zeros(1), sq.cumsum(0)])
    n = torch.from_numpy(np.maximum(np.asarray(counts, np.float64), 1.0)).to(x.device)
    ssq = run.index_select(0, off[1:]) - run.index_select(0, off[:-1])
    mean_sq = (layout["sums"].double() / n[:, None]).square().sum(dim=1)
    return (rel * (ssq / n - mean_sq) / x.shape[1]).clamp_min(0.0).float()


def _kmeans_fit_device(x, layout, counts, classes, ks, n_init, max_iter, random_state):
    """n_init k-means++ / Lloyd fits of every class of `classes`, in two launches. Returns
    the Lloyd outputs with "inertia" / "n_iter" shaped [len(classes), n_init] next to the
    flat per-problem "centres" [Pn, 16, D], "labels", "counts", and the "table"."""
    dev = x.device
    table = _kmeans_table(counts, classes, ks, n_init, dev)
    u = np.random.default_rng(random_state).random((table["Pn"], _KMEANS_SLOTS), dtype=np.float32)
    tol = _kmeans_class_tol(x, layout, counts).index_select(0, table["cls"].long()).contiguous()
    scratch = torch.empty(table["total"], device=dev, dtype=torch.float32)
    picks, centres = _kmeans_seed(x, layout, table, torch.from_numpy(u).to(dev), scratch)
    fit = _kmeans_lloyd(x, layout, table, tol, max_iter, centres, scratch)
    fit["inertia"] = fit["inertia"].view(len(classes), n_init)
    fit["n_iter"] = fit["n_iter"].view(len(classes), n_init)
    fit.update(picks=picks, table=table, tol=tol)
    return fit


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("miclip outlier scoring needs a HIP device (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


# ------------------------------------------------------------------ scorers
class SingleCentroidScorer:
    """Single-centroid scorer (tools/outlier_cleaning.py:178-383) on the GPU."""

    def __init__(self, embeddings: torch.Tensor, labels: torch.Tensor, metadata: pd.DataFrame,
                 *, normalize_tol: float = 1e-3, eps: float = 1e-12, device=None):
        embeddings, labels, num_samples, dim = _validate_embeddings_labels(
            embeddings, labels, allow_empty=False)
        if not isinstance(metadata, pd.DataFrame):
            raise TypeError(f"Expected metadata to be pandas DataFrame, got {type(metadata).__name__}.")
        if int(len(metadata)) != num_samples:
            raise ValueError("Row mismatch between embeddings and metadata: "
                             f"{num_samples} vs {int(len(metadata))}.")
        self.device = _device(device)
        self.embeddings = embeddings.detach().to(self.device, torch.float32).contiguous()
        self.labels = labels.detach().cpu()
        self.metadata = metadata.copy().reset_index(drop=True)
        self.num_samples = num_samples
        self.dim = dim
        self.normalize_tol = float(normalize_tol)
        self.eps = float(eps)
        self._centroids: Optional[CentroidResult] = None
        self._trimmed_centroids: Dict[Tuple[float, int], CentroidResult] = {}
        self._normalized_embeddings: Optional[torch.Tensor] = None
        if "ground_truth_num_label" in self.metadata.columns:
            meta_labels = torch.tensor(
                self.metadata["ground_truth_num_label"].astype(int).to_numpy(), dtype=torch.long)
            bad = torch.nonzero(meta_labels != self.labels, as_tuple=False).flatten()
            if int(bad.numel()) > 0:
                i = int(bad[0].item())
                raise ValueError("Label mismatch between labels tensor and metadata at row "
                                 f"{i}: labels={int(self.labels[i])}, metadata={int(meta_labels[i])}.")

    def _classes(self):
        uniq, inv = torch.unique(self.labels, sorted=True, return_inverse=True)
        return uniq, inv.numpy().astype(np.int64)

    def _get_normalized_embeddings(self) -> torch.Tensor:
        """Unit-norm rows on the device, computed once: the row norms come from the
        HIP kernel; rows are re-normalised (same kernel) only when some norm is off
        by more than normalize_tol; NaN / Inf norms are an error."""
        if self._normalized_embeddings is None:
            norms, _ = _row_norms(self.embeddings)
            if not torch.isfinite(norms).all().item():
                raise ValueError("Non-finite embedding norms found (NaN/Inf).")
            worst = (norms - 1.0).abs().max().item()
            emb = self.embeddings
            if worst > self.normalize_tol:
                print(f"[warn] Unnormalized embeddings detected (max |norm-1|={worst:.3e}); normalizing.")
                emb = _row_norms(self.embeddings, self.eps, normalize=True)[1]
            self._normalized_embeddings = emb
        return self._normalized_embeddings

    def compute_centroids(self, *, trim_frac: Optional[float] = None,
                          trim_rounds: int = 1) -> CentroidResult:
        """Per-class normalised centroids. With trim_frac = f in [0, 0.5) the centroid
        is trimmed (DESIGN "Trimmed class centroids"): trim_rounds times over, the
        floor(f * n_k) rows of each class least similar to the current centroid (ties:
        the lower sample index first) are left out and the centroid is re-formed from
        the rest, all on the device (miclip_trimmed_centroids). The result also names
        the kept rows; class_counts stays the full class size."""
        if trim_frac is not None:
            return self._compute_trimmed_centroids(trim_frac, trim_rounds)
        if self._centroids is not None:
            return self._centroids
        emb = self._get_normalized_embeddings()
        uniq, inv = self._classes()
        K = int(uniq.numel())
        if K == 0:
            raise ValueError("No labels present to compute centroids.")
        cent, counts = _class_centroids(emb, inv, K, self.eps)
        self._centroids = CentroidResult(
            centroids={int(uniq[i]): cent[i] for i in range(K)},
            class_counts={int(uniq[i]): int(counts[i]) for i in range(K)}, dim=self.dim)
        return self._centroids

    def _compute_trimmed_centroids(self, trim_frac, trim_rounds) -> CentroidResult:
        if isinstance(trim_frac, bool) or not isinstance(trim_frac, numbers.Real) or \
                not 0.0 <= float(trim_frac) < 0.5:
            raise ValueError(f"trim_frac must be a real number with 0 <= trim_frac < 0.5, "
                             f"got {trim_frac!r}.")
        if isinstance(trim_rounds, bool) or not isinstance(trim_rounds, numbers.Integral) or \
                not 1 <= int(trim_rounds) <= _TRIM_MAX_ROUNDS:
            raise ValueError(f"trim_rounds must be an int in [1, {_TRIM_MAX_ROUNDS}], "
                             f"got {trim_rounds!r}.")
        key = (float(trim_frac), int(trim_rounds))
        if key in self._trimmed_centroids:
            return self._trimmed_centroids[key]
        uniq, inv = self._classes()
        K = int(uniq.numel())
        if K == 0:
            raise ValueError("No labels present to compute centroids.")
        sizes = np.bincount(inv, minlength=K)
        if int(sizes.max()) > _TRIM_MAX_CLASS_ROWS:
            big = int(np.argmax(sizes))
            raise ValueError(f"trim_frac supports classes of at most {_TRIM_MAX_CLASS_ROWS} "
                             f"rows, class {int(uniq[big])} has {int(sizes[big])}.")
        emb = self._get_normalized_embeddings()
        drop = _trim_drop(sizes, key[0])
        out = _trimmed_centroids_grouped(emb, inv, K, drop, key[1], self.eps)
        # the one copy to the host: the keep flags and the per-round change counts
        host = torch.cat([out["keep"].to(torch.int32), out["changed"]]).cpu().numpy()
        kept_mask = host[:self.num_samples].astype(bool)
        kept = np.bincount(inv[kept_mask], minlength=K)
        cent, counts = out["centroids"], out["counts"]
        res = CentroidResult(
            centroids={int(uniq[i]): cent[i] for i in range(K)},
            class_counts={int(uniq[i]): int(counts[i]) for i in range(K)}, dim=self.dim,
            trim_frac=key[0], kept_counts={int(uniq[i]): int(kept[i]) for i in range(K)},
            kept_mask=kept_mask, rounds_changed=[int(v) for v in host[self.num_samples:]])
        self._trimmed_centroids[key] = res
        return res

    def _frame(self):
        scores = self.metadata.copy().reset_index(drop=True)
        scores["ground_truth_num_label"] = self.labels.numpy().astype(int)
        if "ground_truth_word_label" not in scores.columns:
            scores["ground_truth_word_label"] = ""
        if "ground_truth_L2_num_label" not in scores.columns:
            scores["ground_truth_L2_num_label"] = -1
        if "file_name" not in scores.columns:
            scores["file_name"] = ""
        return scores

    @staticmethod
    def _class_ranks(scores, sim_col, counts):
        scores["class_size"] = scores["ground_truth_num_label"].map(counts).astype(int)
        scores["rank_in_class"] = (scores.groupby("ground_truth_num_label")["outlier_score"]
                                   .rank(method="first", ascending=False).astype(int))
        scores["pct_rank_in_class"] = scores["rank_in_class"] / scores["class_size"]
        p05 = scores.groupby("ground_truth_num_label")[sim_col].transform(
            lambda col: col.quantile(0.05))
        scores["is_bottom_5pct"] = scores[sim_col] <= p05

    def score_centroid_distance(self, *, centroids: Optional[CentroidResult] = None) -> pd.DataFrame:
        res = centroids if centroids is not None else (
            self._centroids if self._centroids is not None else self.compute_centroids())
        if int(res.dim) != self.dim:
            raise ValueError(f"Centroid dim mismatch: expected {self.dim}, got {int(res.dim)}.")
        emb = self.embeddings
        if not bool(torch.isfinite(emb).all()):
            raise ValueError("Non-finite embeddings found (NaN/Inf).")
        uniq, inv = self._classes()
        missing = [int(v) for v in uniq if int(v) not in res.centroids]
        if missing:
            raise ValueError("Missing centroid(s) for label(s): " + ", ".join(str(v) for v in sorted(missing)))
        rows = torch.stack([res.centroids[int(v)].reshape(-1) for v in uniq]).to(
            self.device, torch.float32).contiguous()
        if not bool(torch.isfinite(rows).all()):
            raise ValueError("Non-finite centroid values found (NaN/Inf).")
        K = rows.shape[0]
        # cosine_similarity(emb, centroid[inv]): x/max(|x|,eps) . c/max(|c|,eps)
        nx, _ = _row_norms(emb)
        nc, _ = _row_norms(rows)
        inv_nx = 1.0 / nx.clamp_min(self.eps)
        inv_nc = 1.0 / nc.clamp_min(self.eps)
        owner = torch.arange(K, device=self.device, dtype=torch.int32)
        cls = torch.from_numpy(inv.astype(np.int32)).to(self.device)
        sim, _, _ = _proto_scores(emb, rows, owner, cls, inv_nx, inv_nc)
        sim = sim.cpu().numpy()
        scores = self._frame()
        scores["sim_to_centroid"] = sim
        scores["outlier_score"] = 1.0 - sim
        self._class_ranks(scores, "sim_to_centroid", res.class_counts)
        cols = ["file_name", "ground_truth_num_label", "ground_truth_word_label",
                "ground_truth_L2_num_label", "sim_to_centroid", "outlier_score", "class_size",
                "rank_in_class", "pct_rank_in_class", "is_bottom_5pct"]
        return scores[cols].sort_values(by=["outlier_score", "ground_truth_num_label", "file_name"],
                                        ascending=[False, True, True]).reset_index(drop=True)


class MultiPrototypeScorer(SingleCentroidScorer):
    """Multi-prototype scorer (tools/outlier_cleaning.py:386-760) on the GPU."""

    def __init__(self, embeddings, labels, metadata, *, normalize_tol: float = 1e-3,
                 eps: float = 1e-12, device=None):
        super().__init__(embeddings, labels, metadata, normalize_tol=normalize_tol, eps=eps,
                         device=device)
        self._prototypes: Optional[MultiPrototypeResult] = None
        self._prototype_config = None
        self._kmeans_fit = None   # device backend: the last fit's per-restart outputs

    def compute_prototypes(self, *, k_mode: str = "heuristic", k_fixed: int = 2, k_max: int = 4,
                           min_samples_per_proto: int = 15, random_state: int = 0,
                           n_init: int = 10, max_iter: int = 100,
                           kmeans: str = "sklearn") -> MultiPrototypeResult:
        """Per-class prototypes. kmeans="sklearn" fits each class on the host with
        scikit-learn (the reference's path); kmeans="device" fits every class and
        restart in two launches of csrc/kmeans.hip (k-means++ seeds drawn from
        numpy.random.default_rng(random_state), the restart with the lowest inertia
        wins, the first one among equals) and needs k <= 16 and D <= 1024."""
        if k_mode not in {"heuristic", "fixed"}:
            raise ValueError(f"Unsupported k_mode '{k_mode}'. Expected one of: heuristic, fixed.")
        if kmeans not in {"sklearn", "device"}:
            raise ValueError(f"Unsupported kmeans '{kmeans}'. Expected one of: sklearn, device.")
        for name, v in (("k_fixed", k_fixed), ("k_max", k_max),
                        ("min_samples_per_proto", min_samples_per_proto), ("n_init", n_init),
                        ("max_iter", max_iter)):
            if int(v) < 1:
                raise ValueError(f"{name} must be >= 1, got {v}.")
        config = (str(k_mode), int(k_fixed), int(k_max), int(min_samples_per_proto),
                  int(random_state), int(n_init), int(max_iter), str(kmeans))
        if self._prototypes is not None and self._prototype_config == config:
            return self._prototypes
        if kmeans == "sklearn":
            try:
                from sklearn.cluster import KMeans
            except ImportError as exc:
                raise ImportError("scikit-learn is required for multi-prototype scoring with "
                                  "kmeans='sklearn'. Install it, or use kmeans='device'.") from exc
        emb = self._get_normalized_embeddings()
        uniq, inv = self._classes()
        if int(uniq.numel()) == 0:
            raise ValueError("No labels present to compute prototypes.")
        K = int(uniq.numel())
        means, counts, layout = _class_layout(emb, inv, K, self.eps)   # the k = 1 prototypes
        if kmeans == "device":
            return self._compute_prototypes_device(emb, uniq, inv, means, counts, layout, config)
        prototypes, class_counts, prototype_counts, k_per_class = {}, {}, {}, {}
        for ci in range(K):
            label_id = int(uniq[ci])
            n_c = int(counts[ci])
            class_counts[label_id] = n_c
            k_c = self._class_k(n_c, config)
            if k_c == 1:
                center = means[ci:ci + 1]
                if not bool(torch.isfinite(center).all()):
                    raise ValueError(f"Non-finite prototype found for class {label_id} (k=1).")
                prototypes[label_id] = center
                prototype_counts[label_id] = [n_c]
                k_per_class[label_id] = 1
                continue
            idx = torch.from_numpy(np.nonzero(inv == ci)[0]).to(self.device)
            x_c = emb.index_select(0, idx).contiguous()
            km = KMeans(n_clusters=k_c, random_state=int(random_state), n_init=int(n_init),
                        max_iter=int(max_iter))
            km.fit(x_c.cpu().numpy())
            centers = torch.from_numpy(km.cluster_centers_.astype(np.float32)).to(self.device)
            _, centers = _row_norms(centers.contiguous(), self.eps, normalize=True)
            if not bool(torch.isfinite(centers).all()):
                raise ValueError(f"Non-finite prototype centers found for class {label_id}.")
            # re-assign by cosine (x_c @ centers^T, argmax) for the prototype counts
            zeros = torch.zeros(k_c, device=self.device, dtype=torch.int32)
            zc = torch.zeros(x_c.shape[0], device=self.device, dtype=torch.int32)
            _, arg, _ = _proto_scores(x_c, centers, zeros, zc)
            cnt = np.bincount(arg.cpu().numpy(), minlength=k_c)
            prototypes[label_id] = centers
            prototype_counts[label_id] = [int(v) for v in cnt]
            k_per_class[label_id] = k_c
        self._prototypes = MultiPrototypeResult(prototypes=prototypes, class_counts=class_counts,
                                                prototype_counts=prototype_counts,
                                                k_per_class=k_per_class, dim=self.dim)
        self._prototype_config = config
        return self._prototypes

    @staticmethod
    def _class_k(n_c: int, config) -> int:
        """Prototypes of a class of n_c rows (tools/outlier_cleaning.py:470-486)."""
        k_mode, k_fixed, k_max, min_samples_per_proto = config[:4]
        if k_mode == "heuristic":
            base_k = 1 if n_c < 20 else 3 if n_c < 100 else 4 if n_c < 200 else \
                5 if n_c < 300 else 6
        else:
            base_k = int(k_fixed)
        base_k = min(base_k, int(k_max))
        return max(1, int(min(base_k, n_c, max(1, n_c // int(min_samples_per_proto)))))

    def _compute_prototypes_device(self, emb, uniq, inv, means, counts, layout, config):
        """compute_prototypes(kmeans="device"): every class with k > 1, times n_init
        restarts, is one problem of one miclip_kmeans_seed and one miclip_kmeans_lloyd
        launch. Nothing is read back before the result is assembled: the winning
        restart is gathered on the device (torch.argmin: the first minimum), the
        prototype counts come from one miclip_proto_scores call over all rows, and a
        single copy at the end fetches those counts and the finiteness flags."""
        random_state, n_init, max_iter = config[4:7]
        dev, D, K = self.device, self.dim, int(uniq.numel())
        ks = [self._class_k(int(counts[ci]), config) for ci in range(K)]
        if max(ks) > _KMEANS_MAX_K:
            raise ValueError(f"kmeans='device' supports at most {_KMEANS_MAX_K} prototypes per "
                             f"class, got {max(ks)}.")
        if D > _KMEANS_MAX_D and max(ks) > 1:
            raise ValueError(f"kmeans='device' supports embedding dims up to {_KMEANS_MAX_D}, "
                             f"got {D}.")
        multi = [ci for ci in range(K) if ks[ci] > 1]
        blocks = [means[ci:ci + 1] for ci in range(K)]
        self._kmeans_fit = None
        if multi:
            fit = _kmeans_fit_device(emb, layout, counts, multi, [ks[ci] for ci in multi],
                                     int(n_init), int(max_iter), int(random_state))
            best = fit["inertia"].argmin(dim=1)                                   # [len(multi)]
            chosen = torch.arange(len(multi), device=dev) * int(n_init) + best
            centres = fit["centres"].index_select(0, chosen)                      # [m, 16, D]
            rows = torch.cat([centres[i, :ks[ci]] for i, ci in enumerate(multi)]).contiguous()
            _, rows = _row_norms(rows, self.eps, normalize=True)
            at = 0
            for ci in multi:
                blocks[ci] = rows[at:at + ks[ci]]
                at += ks[ci]
            fit["chosen"] = best
            fit["classes"] = [int(uniq[ci]) for ci in multi]
            self._kmeans_fit = fit
        protos = torch.cat(blocks).contiguous()
        first = np.concatenate([[0], np.cumsum(ks)])
        owner = torch.from_numpy(np.repeat(np.arange(K), ks).astype(np.int32)).to(dev)
        cls = torch.from_numpy(inv.astype(np.int32)).to(dev)
        # re-assign by cosine (rows and prototypes are unit vectors) for the prototype counts
        _, arg, _ = _proto_scores(emb, protos, owner, cls)
        sizes = torch.zeros(protos.shape[0], device=dev, dtype=torch.int64)
        sizes.scatter_add_(0, arg.long(), torch.ones_like(arg, dtype=torch.int64))
        finite = torch.isfinite(protos).all(dim=1)
        host = torch.cat([sizes, finite.long()]).cpu().numpy()      # the one copy to the host
        sizes_h, finite_h = host[:protos.shape[0]], host[protos.shape[0]:]
        prototypes, class_counts, prototype_counts, k_per_class = {}, {}, {}, {}
        for ci in range(K):
            label_id = int(uniq[ci])
            lo, hi = int(first[ci]), int(first[ci + 1])
            if not finite_h[lo:hi].all():
                raise ValueError(f"Non-finite prototype found for class {label_id} (k=1)."
                                 if ks[ci] == 1 else
                                 f"Non-finite prototype centers found for class {label_id}.")
            prototypes[label_id] = blocks[ci]
            class_counts[label_id] = int(counts[ci])
            prototype_counts[label_id] = ([int(counts[ci])] if ks[ci] == 1 else
                                          [int(v) for v in sizes_h[lo:hi]])
            k_per_class[label_id] = ks[ci]
        self._prototypes = MultiPrototypeResult(prototypes=prototypes, class_counts=class_counts,
                                                prototype_counts=prototype_counts,
                                                k_per_class=k_per_class, dim=self.dim)
        self._prototype_config = config
        return self._prototypes

    def score_prototype_distance(self, *, prototypes: Optional[MultiPrototypeResult] = None) -> pd.DataFrame:
        res = prototypes if prototypes is not None else (
            self._prototypes if self._prototypes is not None else self.compute_prototypes())
        if int(res.dim) != self.dim:
            raise ValueError(f"Prototype dim mismatch: expected {self.dim}, got {int(res.dim)}.")
        emb = self._get_normalized_embeddings()
        uniq, inv = self._classes()
        missing = [int(v) for v in uniq if int(v) not in res.prototypes]
        if missing:
            raise ValueError("Missing prototype(s) for label(s): " + ", ".join(str(v) for v in sorted(missing)))
        # all prototypes in sorted label order (the reference's all_prototypes)
        blocks, owners, first, sizes = [], [], {}, []
        label_to_ci = {int(v): i for i, v in enumerate(uniq)}
        for label_id in sorted(res.prototypes.keys()):
            block = res.prototypes[label_id]
            block = (block.unsqueeze(0) if block.ndim == 1 else block).to(self.device, torch.float32)
            if int(block.shape[1]) != self.dim:
                raise ValueError(f"Prototype dim mismatch in class {label_id}: "
                                 f"expected {self.dim}, got {int(block.shape[1])}.")
            if not bool(torch.isfinite(block).all()):
                raise ValueError(f"Non-finite prototype values found for class {label_id}.")
            counts_c = res.prototype_counts[label_id]
            if len(counts_c) != int(block.shape[0]):
                raise ValueError(f"prototype_counts length mismatch for class {label_id}: "
                                 f"{len(counts_c)} vs {int(block.shape[0])}.")
            first[label_id] = sum(b.shape[0] for b in blocks)
            blocks.append(block)
            owners += [label_to_ci.get(label_id, -1)] * int(block.shape[0])
            sizes += list(counts_c)
        protos = torch.cat(blocks).contiguous()
        owner = torch.tensor(owners, device=self.device, dtype=torch.int32)
        cls = torch.from_numpy(inv.astype(np.int32)).to(self.device)
        own, arg, oth = _proto_scores(emb, protos, owner, cls)
        own, arg, oth = own.cpu().numpy(), arg.cpu().numpy(), oth.cpu().numpy()
        lab = self.labels.numpy().astype(int)
        first_of = np.asarray([first[int(v)] for v in lab])
        proto_id = arg - first_of
        n_in_class = np.asarray([res.prototypes[int(v)].reshape(-1, self.dim).shape[0] for v in lab])
        proto_size = np.asarray(sizes)[arg]
        if int(uniq.numel()) <= 1:
            oth = np.full_like(own, np.nan)
            margin = np.full_like(own, np.nan)
        else:
            oth = np.where(np.isinf(oth), np.nan, oth).astype(np.float32)
            margin = own - oth
        scores = self._frame()
        scores["method"] = "multi_prototype"
        scores["sim_to_prototype"] = own
        scores["sim_to_centroid"] = scores["sim_to_prototype"]
        scores["outlier_score"] = 1.0 - own
        scores["prototype_id"] = proto_id.astype(int)
        scores["num_prototypes_in_class"] = n_in_class.astype(int)
        scores["prototype_size"] = proto_size.astype(int)
        self._class_ranks(scores, "sim_to_prototype", res.class_counts)
        scores["rank_in_prototype"] = (scores.groupby(["ground_truth_num_label", "prototype_id"])
                                       ["outlier_score"].rank(method="first", ascending=False)
                                       .astype(int))
        scores["pct_rank_in_prototype"] = scores["rank_in_prototype"] / scores["prototype_size"]
        scores["sim_to_other_class_best"] = oth
        scores["margin_to_other_class"] = margin
        cols = ["file_name", "ground_truth_num_label", "ground_truth_word_label",
                "ground_truth_L2_num_label", "sim_to_centroid", "outlier_score", "class_size",
                "rank_in_class", "pct_rank_in_class", "is_bottom_5pct", "method",
                "sim_to_prototype", "prototype_id", "num_prototypes_in_class", "prototype_size",
                "rank_in_prototype", "pct_rank_in_prototype", "sim_to_other_class_best",
                "margin_to_other_class"]
        return scores[cols].sort_values(by=["outlier_score", "ground_truth_num_label", "file_name"],
                                        ascending=[False, True, True]).reset_index(drop=True)
