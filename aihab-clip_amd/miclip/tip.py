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
"""
import ctypes
from pathlib import Path
from typing import List, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from .feature_cache import _model_device, _view_sampler, compute_image_features

_DTYPES = {torch.float32: _lib.MICLIP_F32, torch.float16: _lib.MICLIP_FP16,
           torch.bfloat16: _lib.MICLIP_BF16}

__all__ = ["build_cache_model", "cache_model_from_views", "search_hp_tip", "tip_accuracy_grid",
           "tip_logits", "beta_alpha_lists", "scan_count_grid", "cls_acc"]


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
