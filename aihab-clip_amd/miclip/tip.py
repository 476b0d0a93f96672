"""Tip-Adapter's training-free cache classifier and its (beta, alpha) search, on the GPU.

Counterpart of the Tip-Adapter helpers of methods/utils.py (same names and argument
order): `build_cache_model` (:23-62) and `search_hp_tip` (:64-94). The reference runs,
for every (beta, alpha) pair, two matmuls, an exp over [Nq, Nk], a matmul against the
one-hot values, a topk and a `.cpu()` synchronisation (cls_acc, :16-21). All pairs share
one affinity matrix and one set of CLIP logits, so here the grid is one evaluation in
the HIP kernels of csrc/tip.hip through the C ABI:

  * cache keys from the cached views            miclip_tip_keys      (:37-48)
  * affinity = features @ cache_keys, and
    clip_logits = 100 * features @ clip_weights miclip_tip_affinity  (:79, :82)
  * correct counts of every (beta, alpha) pair  miclip_tip_grid      (:74-90, :16-21)
  * the logits of one pair                      miclip_tip_logits    (:81-83)

The one-hot check of cache_values and the range check of the labels run on the host
before any launch (one copy of each); after them a search reads the device once, the
[nb, na] count grid, and the choice of the best pair runs on the host over integers,
beta-major with a strict `>`, as the reference's loop does.

Deliberate departures from the reference:
  * cfg['load_cache'] True loads keys_task{task}.pt / values_task{task}.pt from
    cfg['cache_dir'] and False saves them (the reference's load branch reads an
    undefined variable and its saves are commented out);
  * cfg['search_hp'] False raises ValueError naming the key (the reference returns an
    unbound local);
  * the number of classes is clip_weights.shape[1], not F.one_hot's maximum label:
    cache_values narrower than that are accepted (the missing classes own no key and
    contribute 0), wider ones raise ValueError; build_cache_model takes the width from
    cfg['num_classes'] when that key is present;
  * cache_values is the reference's fp16 one-hot matrix; anything that is not one-hot
    raises ValueError (the kernels sum per class instead of multiplying by it);
  * tqdm's progress bar is not reproduced; the print lines are.
An all-zero mean row yields a non-finite key, as in the reference (:48 divides by the
norm without a floor). There is no CPU fallback.

Tip-Adapter-F, the fine-tuned variant that `adapter=` is the hook of, trains the keys on
cached joint-space features in the kernels of csrc/tip_train.hip (fit_adapter_grid,
fit_adapter, tip_adapter_f at the end of this file): AdamW under a cosine schedule, a
grid of (lr, beta, alpha) configurations per launch, the best epoch kept by a device
kernel, no host wait until the result is read. The recipe is stated in
fit_adapter_grid's docstring and in include/miclip.h; the reference checkout does not
contain that loop.
"""
import ctypes
import dataclasses
import math
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from .feature_cache import _model_device, _view_sampler, compute_image_features

_DTYPES = {torch.float32: _lib.MICLIP_F32, torch.float16: _lib.MICLIP_FP16,
           torch.bfloat16: _lib.MICLIP_BF16}

__all__ = ["build_cache_model", "cache_model_from_views", "search_hp_tip", "tip_accuracy_grid",
           "tip_logits", "beta_alpha_lists", "scan_count_grid", "cls_acc", "AdapterFit",
           "fit_adapter_grid", "fit_adapter", "tip_adapter_f", "cosine_lr_factor"]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def cls_acc(output, target, topk=1):
    """Top-k accuracy in percent, the counterpart of methods/utils.py:16-21: the share of
    rows whose label is among the k largest logits (one host read)."""
    hits = (output.topk(topk, dim=1).indices == target.view(-1, 1)).any(dim=1)
    return 100 * float(hits.sum().item()) / target.shape[0]


def beta_alpha_lists(cfg) -> Tuple[List[float], List[float]]:
    """The reference's grids (methods/utils.py:68-69), in Python floats as there."""
    scale, step = cfg['search_scale'], cfg['search_step']
    beta_list = [i * (scale[0] - 0.1) / step[0] + 0.1 for i in range(step[0])]
    alpha_list = [i * (scale[1] - 0.1) / step[1] + 0.1 for i in range(step[1])]
    return beta_list, alpha_list


def scan_count_grid(counts, beta_list: Sequence[float], alpha_list: Sequence[float], n: int,
                    verbose: bool = True):
    """The reference's scan (methods/utils.py:71-92) over the counts [nb, na] of correct
    rows out of n: beta-major, from best_acc = 0, a pair replaces the best only on a
    strictly greater count. Returns (best_beta, best_alpha, best_acc in percent)."""
    best_cnt, best_acc = 0, 0
    best_beta, best_alpha = 0, 0
    for ib, beta in enumerate(beta_list):
        for ia, alpha in enumerate(alpha_list):
            cnt = int(counts[ib][ia])
            if cnt > best_cnt:
                best_cnt, best_acc = cnt, 100 * float(cnt) / n
                if verbose:
                    print("New best setting, beta: {:.2f}, alpha: {:.2f}; accuracy: {:.2f}".format(
                        beta, alpha, best_acc))
                best_beta, best_alpha = beta, alpha
    if verbose:
        print("\nAfter searching, the best accuarcy: {:.2f}.\n".format(best_acc))
    return best_beta, best_alpha, best_acc


def _check_labels(name, labels, n, C):
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError(f"Expected {name} shape [{n}], got {tuple(getattr(labels, 'shape', ()))}.")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError(f"Expected integer {name}, got dtype={labels.dtype}.")
    lab = labels.detach().to("cpu", torch.int64)
    if int(lab.min()) < 0 or int(lab.max()) >= C:
        raise ValueError(f"{name} must lie in [0, {C}); got [{int(lab.min())}, {int(lab.max())}].")
    return lab.to(torch.int32)


def _key_labels(cache_values, Nk, C):
    """int32 class of every key from the one-hot cache_values [Nk, <= C] (host check)."""
    if not isinstance(cache_values, torch.Tensor) or cache_values.ndim != 2:
        raise ValueError("Expected cache_values as a one-hot [Nk, C] tensor.")
    if cache_values.shape[0] != Nk:
        raise ValueError(f"cache_values has {cache_values.shape[0]} rows, cache_keys has {Nk} keys.")
    if not 1 <= cache_values.shape[1] <= C:
        raise ValueError(f"cache_values has width {cache_values.shape[1]}, clip_weights has "
                         f"{C} classes.")
    v = cache_values.detach().to("cpu", torch.float32)
    one_hot = ((v == 0) | (v == 1)).all() and bool((v.sum(dim=1) == 1).all())
    if not one_hot:
        raise ValueError("cache_values must be one-hot (one 1 per row, 0 elsewhere).")
    return v.argmax(dim=1).to(torch.int32)


def _check_inputs(cache_keys, cache_values, features, clip_weights):
    for name, t in (("cache_keys", cache_keys), ("features", features),
                    ("clip_weights", clip_weights)):
        if not isinstance(t, torch.Tensor) or t.ndim != 2 or not t.is_floating_point():
            raise ValueError(f"Expected {name} as a floating [rows, cols] tensor.")
    E, Nk = (int(s) for s in cache_keys.shape)
    Nq, C = int(features.shape[0]), int(clip_weights.shape[1])
    if features.shape[1] != E:
        raise ValueError(f"features has width {features.shape[1]}, cache_keys [E, Nk] has E = {E}.")
    if clip_weights.shape[0] != E:
        raise ValueError(f"clip_weights must be [{E}, C], got {tuple(clip_weights.shape)}.")
    if E % 16 or not (16 <= E <= 1024 and 1 <= C <= 1024 and 1 <= Nk <= 65536
                      and 1 <= Nq <= 1 << 24):
        raise ValueError(f"unsupported shapes Nq={Nq}, Nk={Nk}, E={E}, C={C}: need E % 16 == 0 in "
                         f"[16, 1024], C in [1, 1024], Nk in [1, 65536], Nq in [1, 2^24].")
    return Nq, Nk, E, C, _key_labels(cache_values, Nk, C)


def _device_of(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("miclip Tip-Adapter needs a HIP device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _feature_operand(x, dev):
    x = x.detach().to(dev)
    return (x if x.dtype in _DTYPES else x.float()).contiguous()


class _Prepared:
    """Device operands shared by the grid and the logits: affinity [Nq, Nk], clip logits
    [Nq, C], key labels and the scratch."""

    def __init__(self, checked, cache_keys, features, clip_weights, adapter, nb=1, na=1):
        Nq, Nk, E, C, key_lab = checked          # _check_inputs' result: the one host check
        self.shape = (Nq, Nk, E, C)
        self.dev = dev = _device_of(features, cache_keys, clip_weights)
        self.lib = lib = _lib.load_library()
        nbytes = lib.miclip_tip_scratch_bytes(Nq, Nk, E, C, nb, na)
        if nbytes <= 0:
            raise ValueError(f"unsupported grid nb={nb}, na={na}: need 1 <= nb, na <= 1024 and "
                             f"nb * na <= 65536.")
        f = _feature_operand(features, dev)
        with torch.cuda.device(dev):
            stream = _lib.stream_handle(dev)
            wt = clip_weights.detach().to(dev, torch.float32).t().contiguous()      # [C, E]
            self.clip_logits = torch.empty(Nq, C, device=dev, dtype=torch.float32)
            _lib.check(lib.miclip_tip_affinity(_ptr(f), _DTYPES[f.dtype], _ptr(wt), Nq, C, E, 100.0,
                                               _ptr(self.clip_logits), stream),
                       "miclip_tip_affinity")
            if adapter:
                aff = adapter(features)                                   # methods/utils.py:76-77
                if tuple(aff.shape) != (Nq, Nk):
                    raise ValueError(f"adapter(features) must be [{Nq}, {Nk}], got "
                                     f"{tuple(aff.shape)}.")
                self.affinity = aff.detach().to(dev, torch.float32).contiguous()
            else:
                keys = cache_keys.detach().to(dev, torch.float32).t().contiguous()   # [Nk, E]
                self.affinity = torch.empty(Nq, Nk, device=dev, dtype=torch.float32)
                _lib.check(lib.miclip_tip_affinity(_ptr(f), _DTYPES[f.dtype], _ptr(keys), Nq, Nk,
                                                   E, 1.0, _ptr(self.affinity), stream),
                           "miclip_tip_affinity")
            self.key_labels = key_lab.to(dev)
            self.scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)


def tip_accuracy_grid(cache_keys, cache_values, features, labels, clip_weights,
                      beta_list: Sequence[float], alpha_list: Sequence[float], adapter=None):
    """Correct-row counts of every (beta, alpha) pair in one device pass.

    cache_keys [E, Nk], cache_values one-hot [Nk, C], features [Nq, E] (fp32 / fp16 /
    bf16), labels [Nq] in [0, C), clip_weights [E, C]; adapter(features) replaces
    features @ cache_keys when given. Returns (counts [nb, na] int32 on the device,
    beta_list, alpha_list). The host checks come first: cache_values (one-hot) and labels
    (range) are each copied to the host once, which waits for the device when they live
    there; after that nothing synchronises until the counts are read."""
    beta_list, alpha_list = [float(b) for b in beta_list], [float(a) for a in alpha_list]
    nb, na = len(beta_list), len(alpha_list)
    if nb < 1 or na < 1:
        raise ValueError("beta_list and alpha_list must not be empty.")
    checked = _check_inputs(cache_keys, cache_values, features, clip_weights)
    Nq, C = checked[0], checked[3]
    lab = _check_labels("labels", labels, Nq, C)
    if nb > 1024 or na > 1024 or nb * na > 65536:
        raise ValueError(f"unsupported grid nb={nb}, na={na}: need nb, na <= 1024 and "
                         f"nb * na <= 65536.")
    p = _Prepared(checked, cache_keys, features, clip_weights, adapter, nb, na)
    Nq, Nk, _, C = p.shape
    with torch.cuda.device(p.dev):
        betas = torch.tensor(beta_list, dtype=torch.float32).to(p.dev)
        alphas = torch.tensor(alpha_list, dtype=torch.float32).to(p.dev)
        counts = torch.empty(nb, na, device=p.dev, dtype=torch.int32)
        lab = lab.to(p.dev)
        _lib.check(p.lib.miclip_tip_grid(_ptr(p.affinity), _ptr(p.key_labels), _ptr(p.clip_logits),
                                         _ptr(lab), _ptr(betas), _ptr(alphas), Nq, Nk, C, nb, na,
                                         _ptr(counts), _ptr(p.scratch), _lib.stream_handle(p.dev)),
                   "miclip_tip_grid")
    return counts, beta_list, alpha_list


def tip_logits(cache_keys, cache_values, features, clip_weights, beta: float, alpha: float,
               adapter=None):
    """clip_logits + alpha * exp(-(beta - beta * affinity)) @ cache_values, [Nq, C] fp32 on
    the device (methods/utils.py:81-83): what the chosen pair classifies with."""
    p = _Prepared(_check_inputs(cache_keys, cache_values, features, clip_weights), cache_keys,
                  features, clip_weights, adapter)
    Nq, Nk, _, C = p.shape
    with torch.cuda.device(p.dev):
        out = torch.empty(Nq, C, device=p.dev, dtype=torch.float32)
        _lib.check(p.lib.miclip_tip_logits(_ptr(p.affinity), _ptr(p.key_labels),
                                           _ptr(p.clip_logits), Nq, Nk, C, float(beta),
                                           float(alpha), _ptr(out), _ptr(p.scratch),
                                           _lib.stream_handle(p.dev)), "miclip_tip_logits")
    return out


def search_hp_tip(cfg, cache_keys, cache_values, features, labels, clip_weights, adapter=None):
    """(best_beta, best_alpha) of the reference's grid search (methods/utils.py:64-94)."""
    if cfg['search_hp'] != True:   # noqa: E712 -- the reference's own comparison
        raise ValueError("cfg['search_hp'] is not True: search_hp_tip has nothing to return "
                         "(the reference reads an unbound local here).")
    beta_list, alpha_list = beta_alpha_lists(cfg)
    counts, _, _ = tip_accuracy_grid(cache_keys, cache_values, features, labels, clip_weights,
                                     beta_list, alpha_list, adapter)
    best_beta, best_alpha, _ = scan_count_grid(counts.cpu().tolist(), beta_list, alpha_list,
                                               int(features.shape[0]))
    return best_beta, best_alpha


def _proj_matrix(proj):
    w = proj.vit_proj if hasattr(proj, "vit_proj") else proj
    if not isinstance(w, torch.Tensor) or w.ndim != 2 or not w.is_floating_point():
        raise ValueError("Expected proj as VisProjViT or a floating [Wv, E] tensor.")
    return w


def cache_model_from_views(views: Sequence[torch.Tensor], labels: torch.Tensor, proj,
                           num_classes: int):
    """(cache_keys [E, Nk] fp32, cache_values [Nk, num_classes] fp16 one-hot) from the
    cached pre-projection views f{v} ([Nk, Wv] each) without running the tower:
    methods/utils.py:38-50 with the encode replaced by the cache."""
    views = list(views) if views is not None else []
    if not views:
        raise ValueError("Empty inputs: no feature views.")
    w = _proj_matrix(proj)
    Wv, E = (int(s) for s in w.shape)
    for k, x in enumerate(views):
        if not isinstance(x, torch.Tensor) or x.ndim != 2 or not x.is_floating_point():
            raise ValueError(f"Expected views[{k}] as a floating [Nk, Wv] tensor.")
        if x.shape[1] != Wv:
            raise ValueError(f"views[{k}] has width {x.shape[1]}, the projector expects {Wv}.")
        if x.shape != views[0].shape or x.dtype != views[0].dtype:
            raise ValueError(f"views[{k}] differs from views[0] in shape or dtype.")
    Nk, A = int(views[0].shape[0]), len(views)
    num_classes = int(num_classes)
    if Wv % 16 or E % 16 or not (16 <= E <= 1024 and 1 <= Nk <= 65536 and 1 <= A <= 1024
                                 and 1 <= num_classes <= 1024):
        raise ValueError(f"unsupported shapes Nk={Nk}, Wv={Wv}, E={E}, A={A}, "
                         f"num_classes={num_classes}.")
    lab = _check_labels("labels", labels, Nk, num_classes)
    dev = _device_of(*views, w)
    lib = _lib.load_library()
    xs = [_feature_operand(x, dev) for x in views]
    with torch.cuda.device(dev):
        P = w.detach().to(dev, torch.float32).contiguous()
        ptrs = torch.tensor([x.data_ptr() for x in xs], dtype=torch.int64).to(dev)
        keys = torch.empty(Nk, E, device=dev, dtype=torch.float32)
        _lib.check(lib.miclip_tip_keys(_ptr(ptrs), _DTYPES[xs[0].dtype], A, Nk, Wv, E, _ptr(P),
                                       _ptr(keys), _lib.stream_handle(dev)), "miclip_tip_keys")
        # the launch above reads xs and ptrs stream-ordered; keep them until it is queued
        values = F.one_hot(lab.to(dev, torch.int64), num_classes).half()
    return keys.permute(1, 0), values


@torch.no_grad()
def build_cache_model(cfg, clip_model, train_loader_cache, task, proj):
    """The cache model of methods/utils.py:23-62: cfg['augment_epoch'] passes of the tower
    over the loader (raw uint8 batches through the view sampler of pass a, as
    cache_preprojection_features does), then the keys and the one-hot values."""
    cache_dir = Path(cfg['cache_dir'])
    if cfg['load_cache'] == False:   # noqa: E712 -- the reference's own comparison
        views, labels = [], None
        for augment_idx in range(cfg['augment_epoch']):
            print('Augment Epoch: {:} / {:}'.format(augment_idx, cfg['augment_epoch']))
            x, y = compute_image_features(clip_model, train_loader_cache,
                                          augment=_view_sampler(cfg, clip_model, augment_idx))
            views.append(x)
            if augment_idx == 0:
                labels = y
        if not views:
            raise ValueError("cfg['augment_epoch'] must be >= 1.")
        num_classes = cfg.get('num_classes') if hasattr(cfg, 'get') else None
        if num_classes is None:
            num_classes = int(labels.max()) + 1          # F.one_hot's own rule (:50)
        cache_keys, cache_values = cache_model_from_views(views, labels, proj, num_classes)
        cache_dir.mkdir(parents=True, exist_ok=True)
        torch.save(cache_keys, cache_dir / f'keys_task{task}.pt')
        torch.save(cache_values, cache_dir / f'values_task{task}.pt')
    else:
        dev = _model_device(clip_model)
        cache_keys = torch.load(cache_dir / f'keys_task{task}.pt', map_location=dev,
                                weights_only=True)
        cache_values = torch.load(cache_dir / f'values_task{task}.pt', map_location=dev,
                                  weights_only=True)
    return cache_keys, cache_values


# ---- Tip-Adapter-F: the cache keys trained on cached features (csrc/tip_train.hip) ----

_KEEP_EPOCHS_MAX_BYTES = 1 << 30   # keep_epochs is a test and debug aid


@dataclasses.dataclass
class AdapterFit:
    """Result of fit_adapter_grid, all tensors on the device:
    keys [G, Nk, E] after the last step; best_keys [G, Nk, E], best_epoch [G] and
    best_count [G] (int32) of the first epoch whose evaluation count is strictly greater
    than every earlier one, from 0 (the initial keys, -1 and 0 when none is); history
    [steps, G, 2] = {mean CE, correct rows} of every training batch before its update;
    eval_counts [epochs, G] int32 (None without evaluation rows); epoch_keys
    [epochs, G, Nk, E] with keep_epochs, else None; lrs / betas / alphas as given;
    steps_per_epoch and n for reading the history."""
    keys: torch.Tensor
    best_keys: torch.Tensor
    best_epoch: torch.Tensor
    best_count: torch.Tensor
    history: torch.Tensor
    eval_counts: Optional[torch.Tensor]
    epoch_keys: Optional[torch.Tensor]
    lrs: List[float]
    betas: List[float]
    alphas: List[float]
    steps_per_epoch: int
    n: int


def _finite_list(name, xs):
    try:
        out = [float(x) for x in xs]
    except TypeError:
        raise TypeError(f"Expected {name} as a sequence of numbers.") from None
    if not all(math.isfinite(x) for x in out):
        raise ValueError(f"{name} must be finite, got {out}.")
    return out


def _check_views(train_views, E):
    views = [train_views] if isinstance(train_views, torch.Tensor) else \
        (list(train_views) if train_views is not None else [])
    if not views:
        raise ValueError("Empty inputs: no training views.")
    for k, x in enumerate(views):
        if not isinstance(x, torch.Tensor) or x.ndim != 2 or not x.is_floating_point():
            raise ValueError(f"Expected train_views[{k}] as a floating [n, E] tensor.")
        if x.shape[1] != E:
            raise ValueError(f"train_views[{k}] has width {x.shape[1]}, cache_keys [E, Nk] has "
                             f"E = {E}.")
        if x.shape != views[0].shape or x.dtype != views[0].dtype:
            raise ValueError(f"train_views[{k}] differs from train_views[0] in shape or dtype.")
    return views


def cosine_lr_factor(t: int, T: int) -> float:
    """CosineAnnealingLR(T)'s factor at 1-based step t: 0.5 (1 + cos(pi (t - 1) / T))."""
    return 0.5 * (1.0 + math.cos(math.pi * (t - 1) / T))


def fit_adapter_grid(cache_keys, cache_values, clip_weights, train_views, train_labels,
                     lrs: Sequence[float], betas: Sequence[float], alphas: Sequence[float], *,
                     epochs: int, batch_size: int = 256, weight_decay: float = 0.01,
                     eps: float = 1e-4, seed: int = 0, shuffle: bool = True, eval_features=None,
                     eval_labels=None, keep_epochs: bool = False) -> AdapterFit:
    """Tip-Adapter-F training of the cache keys for G = len(lrs) configurations
    (lrs[g], betas[g], alphas[g]) at once, on cached joint-space features.

    cache_keys [E, Nk], cache_values one-hot [Nk, <= C], clip_weights [E, C] as for
    search_hp_tip; train_views: one [n, E] tensor or a list of V of them (fp32 / fp16 /
    bf16), train_labels [n] in [0, C). Epoch e trains on view e % V in the order
    finetune.cache_order(n, seed, e, shuffle), in batches of batch_size rows (the last one
    partial and averaged over its own rows); the cosine schedule advances once per step
    over T = epochs * steps per epoch; AdamW with betas 0.9 / 0.999.

    With eval_features [Nq, E] and eval_labels [Nq], every configuration is evaluated
    after every epoch at its own (beta, alpha) with the kernels of tip_accuracy_grid, and
    the keys of the first epoch that beats every earlier count (from 0) are kept: a device
    kernel takes that decision. Without them best_keys is keys and best_epoch is
    epochs - 1. The host checks come first (cache_values and the labels are copied to the
    host once); after them nothing waits for the device. keep_epochs keeps every epoch's
    keys (refused above 1 GiB)."""
    lrs, betas, alphas = (_finite_list(nm, xs) for nm, xs in
                          (("lrs", lrs), ("betas", betas), ("alphas", alphas)))
    G = len(lrs)
    if G < 1 or len(betas) != G or len(alphas) != G:
        raise ValueError(f"lrs, betas and alphas must have one common length >= 1, got "
                         f"{len(lrs)}, {len(betas)}, {len(alphas)}.")
    if G > 64:
        raise ValueError(f"at most 64 configurations per fit, got {G}.")
    for name, val, lo in (("epochs", epochs, 1), ("batch_size", batch_size, 1)):
        if isinstance(val, bool) or not isinstance(val, int) or val < lo:
            raise ValueError(f"{name} must be an integer >= {lo}, got {val!r}.")
    if batch_size > 4096:
        raise ValueError(f"batch_size must be at most 4096, got {batch_size}.")
    weight_decay, eps = float(weight_decay), float(eps)
    if not (math.isfinite(weight_decay) and weight_decay >= 0):
        raise ValueError(f"weight_decay must be finite and >= 0, got {weight_decay}.")
    if not (math.isfinite(eps) and eps >= 0):
        raise ValueError(f"eps must be finite and >= 0, got {eps}.")
    if not isinstance(cache_keys, torch.Tensor) or cache_keys.ndim != 2:
        raise ValueError("Expected cache_keys as a floating [rows, cols] tensor.")
    views = _check_views(train_views, int(cache_keys.shape[0]))
    n, Nk, E, C, key_lab = _check_inputs(cache_keys, cache_values, views[0], clip_weights)
    lab = _check_labels("train_labels", train_labels, n, C)
    if (eval_features is None) != (eval_labels is None):
        raise ValueError("eval_features and eval_labels go together.")
    evaluate = eval_features is not None
    if evaluate:
        Nq = _check_inputs(cache_keys, cache_values, eval_features, clip_weights)[0]
        elab = _check_labels("eval_labels", eval_labels, Nq, C)
    if keep_epochs and epochs * G * Nk * E * 4 > _KEEP_EPOCHS_MAX_BYTES:
        raise ValueError(f"keep_epochs would hold {epochs * G * Nk * E * 4} bytes, more than "
                         f"{_KEEP_EPOCHS_MAX_BYTES}.")
    from .finetune import cache_order, cache_view

    bmax = min(batch_size, n)
    steps_per_epoch = (n + batch_size - 1) // batch_size
    T = epochs * steps_per_epoch
    dev = _device_of(*views, cache_keys, clip_weights)
    lib = _lib.load_library()
    nbytes = lib.miclip_tipf_scratch_bytes(bmax, Nk, E, C, G)
    if nbytes <= 0:
        raise ValueError(f"unsupported shapes b={bmax}, Nk={Nk}, E={E}, C={C}, G={G}.")
    fs = [_feature_operand(x, dev) for x in views]
    with torch.cuda.device(dev):
        stream = _lib.stream_handle(dev)
        f32 = dict(device=dev, dtype=torch.float32)
        wt = clip_weights.detach().to(dev, torch.float32).t().contiguous()          # [C, E]

        def clip_logits(f):
            z = torch.empty(f.shape[0], C, **f32)
            _lib.check(lib.miclip_tip_affinity(_ptr(f), _DTYPES[f.dtype], _ptr(wt), f.shape[0], C,
                                               E, 100.0, _ptr(z), stream), "miclip_tip_affinity")
            return z

        zs = [clip_logits(f) for f in fs]            # independent of the keys: once per view
        k0 = cache_keys.detach().to(dev, torch.float32).t().contiguous()            # [Nk, E]
        keys = k0.unsqueeze(0).repeat(G, 1, 1).contiguous()
        m, v = torch.zeros_like(keys), torch.zeros_like(keys)
        lr_d, beta_d, alpha_d = (torch.tensor(x, dtype=torch.float32).to(dev)
                                 for x in (lrs, betas, alphas))
        lab_d, key_lab_d = lab.to(dev), key_lab.to(dev)
        history = torch.zeros(T, G, 2, **f32)
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        _lib.check(lib.miclip_tipf_prepare(_ptr(key_lab_d), Nk, C, _ptr(scratch), stream),
                   "miclip_tipf_prepare")
        best_keys = eval_counts = epoch_keys = None
        if evaluate:
            ef = _feature_operand(eval_features, dev)
            ez, elab_d = clip_logits(ef), elab.to(dev)
            aff = torch.empty(Nq, Nk, **f32)
            tip_scratch = torch.empty(lib.miclip_tip_scratch_bytes(Nq, Nk, E, C, 1, 1), device=dev,
                                      dtype=torch.uint8)
            eval_counts = torch.zeros(epochs, G, device=dev, dtype=torch.int32)
            best_keys = keys.clone()
            best_count = torch.zeros(G, device=dev, dtype=torch.int32)
            best_epoch = torch.full((G,), -1, device=dev, dtype=torch.int32)
        if keep_epochs:
            epoch_keys = torch.empty(epochs, G, Nk, E, **f32)

        t = 0
        for e in range(epochs):
            vi = cache_view(e, len(fs))
            order = cache_order(n, seed, e, shuffle)
            for s in range(steps_per_epoch):
                rows = order[s * batch_size:(s + 1) * batch_size].contiguous()
                t += 1
                _lib.check(lib.miclip_tipf_step(
                    _ptr(fs[vi]), _DTYPES[fs[vi].dtype], n, ctypes.c_void_p(rows.data_ptr()),
                    int(rows.shape[0]), _ptr(lab_d), _ptr(zs[vi]), _ptr(key_lab_d), _ptr(keys),
                    _ptr(m), _ptr(v), _ptr(lr_d), _ptr(beta_d), _ptr(alpha_d), Nk, E, C, G,
                    cosine_lr_factor(t, T), weight_decay, eps, t, _ptr(history[t - 1]), None,
                    _ptr(scratch), stream), "miclip_tipf_step")
            if evaluate:
                for g in range(G):
                    _lib.check(lib.miclip_tip_affinity(_ptr(ef), _DTYPES[ef.dtype], _ptr(keys[g]),
                                                       Nq, Nk, E, 1.0, _ptr(aff), stream),
                               "miclip_tip_affinity")
                    _lib.check(lib.miclip_tip_grid(
                        _ptr(aff), _ptr(key_lab_d), _ptr(ez), _ptr(elab_d), _ptr(beta_d[g:]),
                        _ptr(alpha_d[g:]), Nq, Nk, C, 1, 1, _ptr(eval_counts[e, g:]),
                        _ptr(tip_scratch), stream), "miclip_tip_grid")
                _lib.check(lib.miclip_tipf_keep_best(_ptr(eval_counts), e, _ptr(keys),
                                                     _ptr(best_keys), _ptr(best_count),
                                                     _ptr(best_epoch), Nk, E, G, stream),
                           "miclip_tipf_keep_best")
            if keep_epochs:
                epoch_keys[e].copy_(keys)
        if not evaluate:
            best_keys = keys
            best_count = torch.zeros(G, device=dev, dtype=torch.int32)
            best_epoch = torch.full((G,), epochs - 1, device=dev, dtype=torch.int32)
    return AdapterFit(keys=keys, best_keys=best_keys, best_epoch=best_epoch, best_count=best_count,
                      history=history, eval_counts=eval_counts, epoch_keys=epoch_keys, lrs=lrs,
                      betas=betas, alphas=alphas, steps_per_epoch=steps_per_epoch, n=n)


def _linear_from_keys(best_keys, fit):
    Nk, E = (int(s) for s in best_keys.shape)
    adapter = torch.nn.Linear(E, Nk, bias=False).to(best_keys.device, torch.float32)
    with torch.no_grad():
        adapter.weight.copy_(best_keys)
    adapter.fit = fit
    return adapter


def fit_adapter(cache_keys, cache_values, clip_weights, train_views, train_labels, lr: float,
                beta: float, alpha: float, **kwargs):
    """fit_adapter_grid for one configuration, as the recipe's adapter: an
    nn.Linear(E, Nk, bias=False) on the device whose weight is the best keys, with the
    AdapterFit attached as `.fit`. It can be passed as the `adapter=` of search_hp_tip,
    tip_accuracy_grid and tip_logits. Because it has no bias, adapter(f) = f best_keys^T is
    the built-in affinity with cache_keys = best_keys.t(): the search after training needs
    no Python adapter, and tip_adapter_f runs it that way."""
    for name, x in (("lr", lr), ("beta", beta), ("alpha", alpha)):
        if isinstance(x, (list, tuple, torch.Tensor)):
            raise TypeError(f"Expected {name} as one number; fit_adapter_grid takes lists.")
    fit = fit_adapter_grid(cache_keys, cache_values, clip_weights, train_views, train_labels,
                           [lr], [beta], [alpha], **kwargs)
    return _linear_from_keys(fit.best_keys[0], fit)


def tip_adapter_f(cfg, cache_keys, cache_values, train_views, train_labels, test_features,
                  test_labels, clip_weights):
    """The whole Tip-Adapter-F recipe on cached features: train the keys with
    cfg['tip_f'] = {lr, train_epoch, init_beta, init_alpha[, batch_size, weight_decay, eps,
    seed]}, keep the best epoch on (test_features, test_labels), then search (beta, alpha)
    with search_hp_tip on the best keys (as built-in cache keys: the adapter has no bias).
    Prints the recipe's per-epoch lines from the history, read once at the end. Returns
    (adapter, best_beta, best_alpha, fit)."""
    tf = cfg.get('tip_f') if hasattr(cfg, 'get') else None
    if not hasattr(tf, 'get'):
        raise ValueError("cfg['tip_f'] must be a mapping with lr, train_epoch, init_beta and "
                         "init_alpha.")
    missing = [k for k in ('lr', 'train_epoch', 'init_beta', 'init_alpha') if k not in tf]
    if missing:
        raise ValueError(f"cfg['tip_f'] lacks {missing}.")
    unknown = sorted(set(tf) - {'lr', 'train_epoch', 'init_beta', 'init_alpha', 'batch_size',
                                'weight_decay', 'eps', 'seed'})
    if unknown:
        raise ValueError(f"cfg['tip_f'] has unknown keys {unknown}.")
    if cfg['search_hp'] != True:   # noqa: E712 -- search_hp_tip's own comparison
        raise ValueError("cfg['search_hp'] is not True: tip_adapter_f ends with search_hp_tip.")
    beta_alpha_lists(cfg)
    if test_features is None or test_labels is None:
        raise ValueError("tip_adapter_f needs test_features and test_labels.")
    lr, epochs = float(tf['lr']), tf['train_epoch']
    fit = fit_adapter_grid(cache_keys, cache_values, clip_weights, train_views, train_labels,
                           [lr], [tf['init_beta']], [tf['init_alpha']], epochs=epochs,
                           batch_size=tf.get('batch_size', 256),
                           weight_decay=tf.get('weight_decay', 0.01), eps=tf.get('eps', 1e-4),
                           seed=tf.get('seed', 0), eval_features=test_features,
                           eval_labels=test_labels)
    spe, T, Nq = fit.steps_per_epoch, epochs * fit.steps_per_epoch, int(test_features.shape[0])
    hist = fit.history[:, 0].cpu().view(epochs, spe, 2)             # the one host read
    counts, best_epoch = fit.eval_counts[:, 0].cpu().tolist(), int(fit.best_epoch[0])
    for e in range(epochs):
        print('Train Epoch: {:} / {:}'.format(e, epochs))
        correct = int(hist[e, :, 1].sum())
        print('LR: {:.6f}, Acc: {:.4f} ({:}/{:}), Loss: {:.4f}'.format(
            lr * cosine_lr_factor((e + 1) * spe + 1, T), correct / fit.n, correct, fit.n,
            float(hist[e, :, 0].mean())))
        print("**** Tip-Adapter-F's test accuracy: {:.2f}. ****\n".format(100 * counts[e] / Nq))
    best = 100 * int(fit.best_count[0]) / Nq
    print(f"**** After fine-tuning, Tip-Adapter-F's best test accuracy: {best:.2f}, at epoch: "
          f"{best_epoch}. ****\n")
    best_beta, best_alpha = search_hp_tip(cfg, fit.best_keys[0].t(), cache_values, test_features,
                                          test_labels, clip_weights)
    return _linear_from_keys(fit.best_keys[0], fit), best_beta, best_alpha, fit
