"""ProLIP projector training on the pre-projection feature cache, on the GPU.

Counterpart of methods/ProLIP.py (same names, keyword signature, files and
return values): `VisProjViT` (:31-41), `ProLIP(cfg)(...)` (:44-299) and the
hyper-parameter search of `search_init_hp` (:302-361) as `search_hp`. The
arithmetic of a training step runs in the HIP kernels of csrc/prolip.hip through
the C ABI, for a whole grid of (lr, lambda) configurations at once:

  * forward, cross-entropy, accuracy and the
    backward down to d loss / d(x @ proj)       miclip_prolip_grad  (:232-248)
  * projector gradient + MSE pull + Adam step   miclip_prolip_adam  (:243-256)

so one step of all G configurations is two calls, where the reference runs
G separate torch loops of about 30 launches and two `.item()` synchronisations
each. Nothing here uses torch autograd; nothing synchronises with the device
until the history is read. Master weights and optimiser state are fp32 whatever
the cache dtype (fp16 by default, widened exactly in the kernels' loads).

What stays on the host, as in the reference: the view counter, the cosine
schedule factor, the choice of the best pair and the file bookkeeping.

Deliberate departures of `ProLIP` from the reference:
  * any ViT backbone is accepted (the reference names ViT-B/16 and ViT-B/32 only);
  * RN50 / RN101 and dataset == 'imagenet' raise ValueError: the towers here are
    ViT only, and the ImageNet variants need test sets this library does not ship;
  * state_dict["visual.proj"] is not mutated (the reference trains it in place
    through nn.Parameter(vit_proj), :161); the trained projector is the returned
    module's / checkpoint's `vit_proj`.
There is no CPU fallback.
"""
import ctypes
import math
from dataclasses import dataclass
from pathlib import Path
from typing import List, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .feature_cache import _feature_cache_dir, compute_image_features

LR_LIST = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8)          # methods/ProLIP.py:119
LAMBDA_LIST = (10, 1, 0.1, 0.01, 0.001, 0.0001, 0)            # :120

_X_DTYPES = {torch.float32: _lib.MICLIP_F32, torch.float16: _lib.MICLIP_FP16,
             torch.bfloat16: _lib.MICLIP_BF16}


class VisProjViT(nn.Module):
    """x @ vit_proj with a trainable vit_proj (methods/ProLIP.py:31-41); the
    state-dict key is the reference's, so `save_checkpoints` files interchange."""

    def __init__(self, vit_proj):
        super().__init__()
        self.vit_proj = nn.Parameter(vit_proj)
        self.vit_proj.requires_grad = True

    def forward(self, x_before_proj):
        return x_before_proj @ self.vit_proj


@dataclass
class GridFit:
    """Result of fit_projector_grid: proj [G, D, E] fp32 on the device; history
    [steps, G, 3] fp32 on the device = {loss1 (mean CE), loss2 (sum((P - P0)^2)),
    correct count} of every step, taken before that step's update."""
    proj: torch.Tensor
    history: torch.Tensor
    lrs: List[float]
    lams: List[float]
    lambda_div: float = 1.0

    def total_loss(self, step: int = -1) -> np.ndarray:
        """loss1 + (lambda / chunks) * loss2 of one step, per configuration (:216, :246)."""
        h = self.history[step].double().cpu().numpy()
        return h[:, 0] + np.asarray(self.lams, dtype=np.float64) / self.lambda_div * h[:, 1]


def view_cycle(epochs: int, views: int) -> List[int]:
    """The view each epoch trains on: the reference's counter (:171, :181-185),
    which starts at 0 and steps before use, so epoch 0 uses view 1 when views > 1."""
    out, cnt = [], 0
    for _ in range(int(epochs)):
        cnt = 0 if (cnt + 1) % views == 0 else cnt + 1
        out.append(cnt)
    return out


def schedule_factor(epoch: int, epochs: int) -> float:
    """CosineAnnealingLR(T_max=epochs, eta_min=0) in closed form: lr(epoch) / lr(0)."""
    return 0.5 * (1.0 + math.cos(math.pi * epoch / epochs))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("miclip ProLIP training needs a HIP device (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _check_features(name, x, labels, D, C, check_range=True):
    if not isinstance(x, torch.Tensor) or x.ndim != 2:
        raise ValueError(f"Expected {name} shape [n, D], got {tuple(getattr(x, 'shape', ()))}.")
    if x.dtype not in _X_DTYPES:
        raise TypeError(f"Expected {name} dtype float32, float16 or bfloat16, got {x.dtype}.")
    if x.shape[1] != D:
        raise ValueError(f"{name} has width {x.shape[1]}, the projector expects {D}.")
    if x.shape[0] < 1:
        raise ValueError(f"Empty inputs: {name} has no rows.")
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.shape[0] != x.shape[0]:
        raise ValueError(f"Expected labels shape [{x.shape[0]}], got "
                         f"{tuple(getattr(labels, 'shape', ()))}.")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError(f"Expected integer labels, got dtype={labels.dtype}.")
    lab = labels.detach().to("cpu", torch.int64)
    if check_range and (int(lab.min()) < 0 or int(lab.max()) >= C):
        raise ValueError(f"labels must lie in [0, {C}); got [{int(lab.min())}, {int(lab.max())}].")
    return lab


def _check_head(vit_proj, text_weights):
    for name, t in (("vit_proj", vit_proj), ("text_weights", text_weights)):
        if not isinstance(t, torch.Tensor) or t.ndim != 2 or not t.is_floating_point():
            raise ValueError(f"Expected {name} as a floating [rows, cols] tensor.")
    D, E = (int(s) for s in vit_proj.shape)
    C = int(text_weights.shape[1])
    if text_weights.shape[0] != E:
        raise ValueError(f"text_weights must be [{E}, C], got {tuple(text_weights.shape)}.")
    if D % 16 or E % 16 or not (16 <= D <= 1280 and 16 <= E <= 1024 and 1 <= C <= 1024):
        raise ValueError(f"unsupported shapes D={D}, E={E}, C={C}: need D % 16 == 0 in [16, 1280], "
                         f"E % 16 == 0 in [16, 1024], C in [1, 1024].")
    return D, E, C


def _grad(lib, x, labels, W, P, scale, dZ, gpart):
    n, D = x.shape
    G, _, E = P.shape
    _lib.check(lib.miclip_prolip_grad(_ptr(x), _X_DTYPES[x.dtype], _ptr(labels), n, D, E,
                                      W.shape[1], _ptr(W), _ptr(P), G, float(scale), _ptr(dZ),
                                      _ptr(gpart), _lib.stream_handle(x.device)),
               "miclip_prolip_grad")


def fit_projector_grid(views: Sequence[torch.Tensor], labels: torch.Tensor, vit_proj: torch.Tensor,
                       text_weights: torch.Tensor, lrs: Sequence[float], lams: Sequence[float], *,
                       epochs: int, feat_batch_size: int = 0, scale: float = 100.0,
                       eps: float = 1e-4, device=None) -> GridFit:
    """Train G = len(lrs) projectors from vit_proj, configuration g with (lrs[g], lams[g]).

    views: the cached pre-projection features f{v} ([n, D] each, fp32 / fp16 /
    bf16), labels [n] in [0, C). One epoch is one full-batch Adam step on the
    view `view_cycle` names, or with feat_batch_size > 0 one step per chunk of
    rows in row order (CE averaged over the chunk, lambda / ceil(n /
    feat_batch_size), step counter running across chunks); the cosine schedule
    advances once per epoch (methods/ProLIP.py:165-259)."""
    views = list(views) if views is not None else []
    if not views:
        raise ValueError("Empty inputs: no feature views.")
    D, E, C = _check_head(vit_proj, text_weights)
    lab = None
    for k, x in enumerate(views):
        lab = _check_features(f"views[{k}]", x, labels, D, C) if k == 0 else lab
        if k and (x.shape != views[0].shape or x.dtype != views[0].dtype or x.ndim != 2):
            raise ValueError(f"views[{k}] differs from views[0] in shape or dtype.")
    lrs, lams = [float(v) for v in lrs], [float(v) for v in lams]
    G = len(lrs)
    if G < 1 or len(lams) != G:
        raise ValueError(f"lrs and lams must be paired lists of length >= 1, got {G} and {len(lams)}.")
    epochs, bs = int(epochs), int(feat_batch_size or 0)
    if epochs < 1 or bs < 0:
        raise ValueError("epochs must be >= 1 and feat_batch_size >= 0.")
    if not (eps >= 0.0) or any(not math.isfinite(v) for v in lrs + lams):
        raise ValueError("lrs, lams must be finite and eps >= 0.")
    n = int(views[0].shape[0])
    chunks = [(i0, min(i0 + bs, n)) for i0 in range(0, n, bs)] if bs > 0 else [(0, n)]
    lam_div = float(max(len(chunks), 1))

    dev = _device(device)
    lib = _lib.load_library()
    xs = [x.detach().to(dev).contiguous() for x in views]
    y = lab.to(dev)
    W = text_weights.detach().to(dev, torch.float32).contiguous()
    P0 = vit_proj.detach().to(dev, torch.float32).contiguous()
    P = P0.unsqueeze(0).repeat(G, 1, 1).contiguous()
    m, v = torch.zeros_like(P), torch.zeros_like(P)
    lr_d = torch.tensor(lrs, dtype=torch.float32).to(dev)
    lam_d = torch.tensor(lams, dtype=torch.float32).to(dev)
    nmax = max(i1 - i0 for i0, i1 in chunks)
    dZ = torch.empty(G, nmax, E, device=dev, dtype=torch.float32)
    gpart = torch.empty(G, (nmax + 15) // 16, 2, device=dev, dtype=torch.float32)
    mpart = torch.empty(G, ((D + 31) // 32) * ((E + 31) // 32), device=dev, dtype=torch.float32)
    hist = torch.empty(epochs * len(chunks), G, 3, device=dev, dtype=torch.float32)
    xdt = _X_DTYPES[xs[0].dtype]
    step = 0
    with torch.cuda.device(dev):
        stream = _lib.stream_handle(dev)
        for epoch, vi in enumerate(view_cycle(epochs, len(xs))):
            factor = schedule_factor(epoch, epochs)
            for i0, i1 in chunks:
                xc, yc = xs[vi][i0:i1], y[i0:i1]
                _grad(lib, xc, yc, W, P, scale, dZ, gpart)
                _lib.check(lib.miclip_prolip_adam(
                    _ptr(xc), xdt, _ptr(dZ), i1 - i0, D, E, G, _ptr(P0), _ptr(P), _ptr(m), _ptr(v),
                    _ptr(lr_d), _ptr(lam_d), factor, lam_div, step + 1, float(eps), _ptr(gpart),
                    _ptr(mpart), _ptr(hist[step]), stream), "miclip_prolip_adam")
                step += 1
    return GridFit(proj=P, history=hist, lrs=lrs, lams=lams, lambda_div=lam_div)


def fit_projector(views, labels, vit_proj, text_weights, lr: float, lam: float, *, epochs: int,
                  feat_batch_size: int = 0, scale: float = 100.0, eps: float = 1e-4,
                  device=None) -> VisProjViT:
    """fit_projector_grid for one (lr, lambda); returns the trained VisProjViT.
    Its `history` / `fit` attributes carry the per-step record."""
    fit = fit_projector_grid(views, labels, vit_proj, text_weights, [lr], [lam], epochs=epochs,
                             feat_batch_size=feat_batch_size, scale=scale, eps=eps, device=device)
    proj = VisProjViT(fit.proj[0].clone())
    proj.fit = fit
    proj.history = fit.history[:, 0]
    return proj


def projector_accuracy(projs: torch.Tensor, feats: torch.Tensor, labels: torch.Tensor,
                       text_weights: torch.Tensor, *, scale: float = 100.0, device=None):
    """Top-1 accuracy (%) of scale * normalize(feats @ projs[g]) @ text_weights for
    every projector of projs [G, D, E] (methods/ProLIP.py:125-130, :288-293), in
    one miclip_prolip_grad launch (its correct-count partials; first maximum wins)."""
    if not isinstance(projs, torch.Tensor) or projs.ndim != 3:
        raise ValueError("Expected projs shape [G, D, E].")
    D, E, C = _check_head(projs[0], text_weights)
    lab = _check_features("feats", feats, labels, D, C, check_range=False)   # others never match
    dev = _device(device if device is not None else (projs.device if projs.is_cuda else None))
    lib = _lib.load_library()
    x = feats.detach().to(dev).contiguous()
    P = projs.detach().to(dev, torch.float32).contiguous()
    W = text_weights.detach().to(dev, torch.float32).contiguous()
    n, G = x.shape[0], P.shape[0]
    dZ = torch.empty(G, n, E, device=dev, dtype=torch.float32)
    gpart = torch.empty(G, (n + 15) // 16, 2, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _grad(lib, x, lab.to(dev), W, P, scale, dZ, gpart)
    correct = gpart[:, :, 1].double().sum(dim=1).cpu().numpy()
    return 100.0 * correct / n


def search_hp(views, labels, vit_proj, text_weights, val_feats, val_labels, *, epochs: int,
              lr_list: Sequence[float] = LR_LIST, lambda_list: Sequence[float] = LAMBDA_LIST,
              scale: float = 100.0, eps: float = 1e-4, device=None):
    """The (lr, lambda) search of methods/ProLIP.py:116-137 with every pair trained
    in one batched fit. Returns (lr, lam, acc, table): table [len(lr_list),
    len(lambda_list)] of validation accuracies (%); the winner is the first pair,
    lr-major, whose accuracy is strictly greater than every earlier one (starting
    from 0.0; if every accuracy is 0 the first pair is returned)."""
    lr_list, lambda_list = list(lr_list), list(lambda_list)
    if not lr_list or not lambda_list:
        raise ValueError("lr_list and lambda_list must not be empty.")
    D, E, C = _check_head(vit_proj, text_weights)
    _check_features("val_feats", val_feats, val_labels, D, C, check_range=False)
    pairs = [(lr, lam) for lr in lr_list for lam in lambda_list]
    fit = fit_projector_grid(views, labels, vit_proj, text_weights, [p[0] for p in pairs],
                             [p[1] for p in pairs], epochs=epochs, scale=scale, eps=eps,
                             device=device)
    acc = projector_accuracy(fit.proj, val_feats, val_labels, text_weights, scale=scale,
                             device=fit.proj.device)
    best_acc, best = 0.0, pairs[0]
    for pair, a in zip(pairs, acc):
        if a > best_acc:
            best_acc, best = float(a), pair
    return best[0], best[1], best_acc, acc.reshape(len(lr_list), len(lambda_list))


class ProLIP:
    """`ProLIP(cfg)(train_loader=..., ..., model=, state_dict=, classnames=, task=,
    shots=, config_file=, test_config_path=)` as main.py calls it
    (methods/ProLIP.py:44-299). Reads the cache cache_preprojection_features wrote
    (feature_cache._feature_cache_dir), trains on the GPU and returns (loss,
    acc_test): the last step's total loss and the test accuracy in percent."""

    def __init__(self, args):
        self.cfg = args

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def forward(self, train_loader, val_loader, test_loader, test_loader_v2=None,
                test_loader_sketch=None, test_loader_a=None, test_loader_r=None,
                text_weights=None, text_weights_a=None, text_weights_r=None,
                text_weights_before=None, model=None, state_dict=None, classnames=None,
                task: int = 1, shots: int = 0, config_file: str = "", test_config_path: str = ""):
        cfg = self.cfg
        backbone = str(cfg.get("backbone", ""))
        if backbone in ("RN50", "RN101"):
            raise ValueError(f"backbone {backbone}: miclip's towers are ViT only")
        if cfg.get("dataset") == "imagenet":
            raise ValueError("dataset 'imagenet' (the five-test-set variant) is not supported")
        if state_dict is None or "visual.proj" not in state_dict:
            raise ValueError('state_dict["visual.proj"] is required')
        if text_weights is None or classnames is None or model is None:
            raise ValueError("text_weights, classnames and model are required")
        aug_views, epochs = int(cfg["aug_views"]), int(cfg["train_epoch"])
        if aug_views < 1:
            raise ValueError("Empty inputs: aug_views must be >= 1.")
        vit_proj = state_dict["visual.proj"].detach().float().clone()   # never trained in place
        n_cls = len(classnames)

        cache_dir = _feature_cache_dir(cfg)
        train_labels = torch.load(cache_dir / "label.pth", map_location="cpu", weights_only=True)
        keep = torch.where(train_labels < n_cls)[0]
        train_labels = train_labels[keep]
        views = [torch.load(cache_dir / f"f{v}.pth", map_location="cpu", weights_only=True)[keep]
                 for v in range(aug_views)]
        dev = None
        try:
            p = next(iter(model.parameters()))
            dev = p.device if p.is_cuda else None
        except (StopIteration, AttributeError, TypeError):
            pass

        if cfg.get("search_lr"):
            val_x, val_y = compute_image_features(model, val_loader)
            lr_v, lambda_v, _, _ = search_hp(views, train_labels, vit_proj, text_weights, val_x,
                                             val_y, epochs=epochs, device=dev)
        else:
            lr_v = cfg["lr_v"]
            if cfg.get("lambda_funct_1_N"):
                lambda_v = 1 / shots
            elif cfg.get("lambda_funct_1_N2"):
                lambda_v = 1 / shots ** 2
            else:
                lambda_v = cfg["lambda_v"]
        print(f"Search completed ===> lr: {lr_v}, lambda: {lambda_v}")
        if cfg.get("search_lr"):
            path = Path("results_lr") / config_file / f"{cfg['dataset']}{shots}_shot_lr.txt"
            path.parent.mkdir(parents=True, exist_ok=True)
            with path.open("a", encoding="utf-8") as fh:
                fh.write(f"{lr_v}, {lambda_v}\n")

        proj = fit_projector(views, train_labels, vit_proj, text_weights, lr_v, lambda_v,
                             epochs=epochs, feat_batch_size=int(cfg.get("feat_batch_size", 0) or 0),
                             device=dev)
        self.proj = proj
        if cfg.get("save_checkpoints") is True:
            path = (Path("trained_models") / config_file / cfg["dataset"] / f"{shots}_shot"
                    / f"{cfg['dataset']}_seed{task}.pth")
            path.parent.mkdir(parents=True, exist_ok=True)
            torch.save(proj.state_dict(), path)

        test_x, test_y = compute_image_features(model, test_loader)
        with torch.no_grad():
            if hasattr(model, "zero_shot"):   # the encode path's head (miclip_zero_shot)
                _, top = model.zero_shot(proj(test_x.float().to(proj.vit_proj.device)), text_weights,
                                         100.0, k=1, apply_proj=False)
                acc_test = 100.0 * float(np.mean(top[:, 0].cpu().numpy() == test_y.cpu().numpy()))
            else:                             # a model without a miclip handle
                acc_test = float(projector_accuracy(proj.vit_proj.detach()[None], test_x, test_y,
                                                    text_weights)[0])
        loss = float(proj.fit.total_loss(-1)[0])
        return loss, acc_test
