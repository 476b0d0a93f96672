"""Fine-tuning of the image tower's tail on the HIP device (methods/PEFT_openclip.py:139-384).

The reference's default method, `FTOpenCLIP`, unlocks the last groups of the image
tower with open_clip's `lock_image_tower(unlocked_groups=...)` (:196-197), trains them
under autocast with Adam and CosineAnnealingLR (:231-279), validates (:281-313),
tests (:315-346), saves a checkpoint (:350-363) and caches embeddings (:365-379).

Groups are counted from the back as open_clip's `VisionTransformer.lock` does:

  * group 1: `visual.proj`
  * group 2: `visual.transformer.resblocks.{L-1}.*` and `visual.ln_post.*`

open_clip itself is not available here and the reference pins no version of it, so
this grouping is the contract (parity unpinned, as for the rest of the open_clip
surface, openclip.py).

`unlocked_groups` 1 and 2 are built; 3 and more (a gradient through a full block),
0 (an empty parameter list) and `tune_text` raise as the table in DESIGN says.
`CLIP.lock_image_tower` / `lock_text_tower` are never called. With every earlier
block frozen the input x of the last block carries no gradient, so a training step is
the frozen trunk (`miclip_encode_image_trunk`), then `miclip_ft_grad` -- the last block
on the CLS query, ln_post, proj, the loss, and a backward that is CLS-row work plus one
contraction dQKV^T . xhat over the token rows on the transposing-read MFMA GEMM of
csrc/finetune.hip -- then `miclip_ft_adam`.

Numerics: master parameters, gradients and the Adam state are fp32; GEMM operands are
rounded once (RNE) to the model's compute dtype, gradient operands under a power-of-two
scale undone in fp32; LayerNorm statistics, softmax, activation derivatives, normalise
and loss are fp32. No float atomics: a step is bit-identical run to run.

The trunk is a function of the images alone and its weights never change, so with
`finetune.trunk_cache_views` = V >= 1 it is run once per view before epoch 0 (`TrunkCache`,
`LastBlockTrainer.fill_view`; what ProLIP's `aug_views` passes of
`cache_preprojection_features` are to the projector) and every epoch trains on the cached
residual stream through `miclip_ft_grad_rows`, which reads the cache through a row map
instead of a gathered copy (`LastBlockTrainer.step_rows`).
"""
import ctypes
import math
from datetime import datetime
from pathlib import Path
from typing import List, Optional

import torch

from . import _lib
from .evaluation import run_validation
from .feature_cache import (_canonical_backbone_name, _model_device, _view_sampler,
                            cache_openclip_embeddings, is_raw_batch, prepare_images, raw_sizes)

ADAM_EPS = 1e-8          # torch.optim.Adam's default, which the reference keeps (:233)
LOGIT_SCALE = 100.0      # :262, logit_scale is ignored by the reference
_BLOCK_TENSORS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias",
                  "attn.out_proj.weight", "attn.out_proj.bias", "ln_2.weight", "ln_2.bias",
                  "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
_COMPUTE = {"fp16": _lib.MICLIP_FP16, "float16": _lib.MICLIP_FP16,
            "bf16": _lib.MICLIP_BF16, "bfloat16": _lib.MICLIP_BF16}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def cosine_factor(epoch: int, epochs: int) -> float:
    """CosineAnnealingLR(T_max=epochs, eta_min=0) in closed form: lr(epoch) / lr(0) (:234)."""
    return 0.5 * (1.0 + math.cos(math.pi * epoch / epochs))


def _vision_layers(model) -> int:
    cfg = getattr(model, "config", None)
    if cfg is not None and hasattr(cfg, "vision_layers"):
        return int(cfg.vision_layers)
    idx = [int(n.split(".")[3]) for n, _ in model.named_parameters()
           if n.startswith("visual.transformer.resblocks.")]
    if not idx:
        raise ValueError("model has no visual.transformer.resblocks.* parameters")
    return max(idx) + 1


def trainable_names(model, unlocked_groups: int, tune_text: bool = False) -> List[str]:
    """State-dict names that `lock_image_tower(unlocked_groups=...)` leaves trainable,
    in `named_parameters` order (the order torch.optim.Adam numbers them in)."""
    if tune_text:
        raise NotImplementedError("tune_text=True: training the text tower is not supported "
                                  "(the image tower's last groups only)")
    g = int(unlocked_groups)
    if g <= 0:
        raise ValueError("optimizer got an empty parameter list")   # torch.optim.Adam([])
    L = _vision_layers(model)
    if g >= 3:
        first = f"visual.transformer.resblocks.{L - 2}" if L >= 2 else "visual.ln_pre"
        raise NotImplementedError(
            f"unlocked_groups={g}: group 3 ({first}.*) would need a gradient through a full "
            f"transformer block; groups 1 (visual.proj) and 2 (the last block and ln_post) "
            f"are the scope")
    want = {"visual.proj"}
    if g == 2:
        want |= {f"visual.transformer.resblocks.{L - 1}.{t}" for t in _BLOCK_TENSORS}
        want |= {"visual.ln_post.weight", "visual.ln_post.bias"}
    names = [n for n, _ in model.named_parameters() if n in want]
    missing = want - set(names)
    if missing:
        raise ValueError(f"model lacks the parameters {sorted(missing)}")
    return names


def cache_order(n: int, seed: int, epoch: int, shuffle: bool = True) -> torch.Tensor:
    """Order (int64 [n], host) in which an epoch visits the n cached images: a
    `torch.randperm` under a CPU generator seeded from (seed, epoch), whatever the batch
    size; ascending when `shuffle` is off."""
    n = int(n)
    if not shuffle:
        return torch.arange(n, dtype=torch.int64)
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 1000003 + int(epoch)) % (1 << 63))
    return torch.randperm(n, generator=g, dtype=torch.int64)


def cache_view(epoch: int, views: int) -> int:
    """The cached view that epoch `epoch` trains on: views are taken in turn."""
    return int(epoch) % int(views)


def trunk_cache_config(cfg):
    """(views, shuffle, max_bytes) from cfg["finetune"]: `trunk_cache_views` (0 or absent:
    no cache), `trunk_cache_shuffle` (True) and `trunk_cache_max_bytes` (None: half of the
    free device memory when the method starts)."""
    ft = (cfg.get("finetune") if hasattr(cfg, "get") else None) or {}
    views = ft.get("trunk_cache_views", 0)
    views = 0 if views is None else views
    if isinstance(views, bool) or not isinstance(views, int):
        raise ValueError(f"finetune.trunk_cache_views must be an integer >= 0, got {views!r}")
    if views < 0:
        raise ValueError(f"finetune.trunk_cache_views must be >= 0, got {views}")
    budget = ft.get("trunk_cache_max_bytes", None)
    if budget is not None:
        if isinstance(budget, bool) or not isinstance(budget, int) or budget < 0:
            raise ValueError(f"finetune.trunk_cache_max_bytes must be an integer >= 0, got "
                             f"{budget!r}")
    return views, bool(ft.get("trunk_cache_shuffle", True)), budget


class TrunkCache:
    """The frozen trunk's output for whole passes over a loader. Per view: x [n * N, W] on
    the device in the handle's stream type (image i's token block is rows i * N .. i * N + N),
    the targets [n] as int64 on the host (`targets_host`) and on the device (`targets`), and
    n. `max_bytes` (None: no limit) bounds the bytes of x over all views; `batch_size` is the
    size of the first batch that was cached."""

    def __init__(self, max_bytes: Optional[int] = None):
        self.max_bytes = None if max_bytes is None else int(max_bytes)
        self.x, self.targets, self.targets_host, self.n = [], [], [], []
        self.batch_size = None

    @property
    def views(self) -> int:
        return len(self.x)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.x)


class LastBlockTrainer:
    """Adam on the unlocked tail of `model`'s image tower against fixed `text_weights`
    [E, C]: what :231-234 and the batch loop :247-274 do for one model.

    step(images, targets) runs the frozen trunk (`miclip_encode_image_trunk`), the tail's
    forward and backward (`miclip_ft_grad`) and the optimiser (`miclip_ft_adam`), and
    returns device tensors (sum of the rows' cross-entropy, correct count) without a host
    synchronisation beyond the range check of host-side labels; set_epoch(e) moves the
    cosine schedule; commit() writes the master parameters into the model, after which
    `encode_image`, `run_validation` and the caches see the tuned model.

    fill_view(cache, loader) runs the trunk once over a loader into a `TrunkCache`;
    step_rows(cache, view, rows) is step() on cached images, without the trunk
    (`miclip_ft_grad_rows` reads the cache through the row map), bit-identical to step() on
    the same images.
    """

    def __init__(self, model, text_weights, *, unlocked_groups: int = 1, lr: float,
                 epochs: int, tune_text: bool = False):
        self.names = trainable_names(model, unlocked_groups, tune_text)
        if getattr(model, "compute_dtype", None) not in _COMPUTE:
            raise NotImplementedError(
                f"compute dtype {getattr(model, 'compute_dtype', None)!r}: fine-tuning runs on "
                f"fp16 and bf16 models (MX-fp8 operands have no backward)")
        if int(epochs) < 1:
            raise ValueError("epochs must be >= 1")
        if not float(lr) >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        self.model = model
        self.unlocked_groups = int(unlocked_groups)
        self.lr0, self.epochs, self.epoch, self.steps = float(lr), int(epochs), 0, 0
        self.dtype = _COMPUTE[model.compute_dtype]
        self.device = model.device
        self.lib = _lib.load_library()
        cfg = model.config
        self.W, self.E = (int(s) for s in model.visual.proj.shape)
        self.N, self.dh = int(cfg.n_tokens), int(cfg.vision_head_width)
        self.act = _lib.MICLIP_ACT_GELU if cfg.act == "erf" else _lib.MICLIP_ACT_QUICKGELU
        self.x_dtype = torch.float16 if model.numerics()["resid16"] else torch.float32
        tw = text_weights.detach().to(self.device, torch.float32).contiguous()
        if tw.ndim != 2 or tw.shape[0] != self.E:
            raise ValueError(f"text_weights must be [{self.E}, C], got {tuple(tw.shape)}")
        self.text_weights, self.C = tw, int(tw.shape[1])
        if self.lib.miclip_ft_scratch_bytes(1, self.N, self.W, self.E, self.C, self.dh) <= 0:
            raise ValueError(
                f"unsupported shapes N={self.N}, W={self.W}, E={self.E}, C={self.C}, head_dim="
                f"{self.dh}: need N <= 768, W % 128 == 0 in [128, 1280], E % 16 == 0 in "
                f"[16, 1024], C in [1, 1024], head_dim 64 or 80")
        # flat fp32 master block of the tail (miclip_ft_layout), its gradient and Adam state
        pre = f"visual.transformer.resblocks.{int(cfg.vision_layers) - 1}."
        self.tensors = [pre + t for t in _BLOCK_TENSORS] + ["visual.ln_post.weight",
                                                            "visual.ln_post.bias", "visual.proj"]
        off = (ctypes.c_int64 * 16)()
        _lib.check(self.lib.miclip_ft_layout(self.W, self.E, off), "miclip_ft_layout")
        self.offsets = list(off)
        sd = model.state_dict()
        self.params = torch.cat([sd[n].detach().to(self.device, torch.float32).reshape(-1)
                                 for n in self.tensors]).contiguous()
        if self.params.numel() != self.offsets[15]:
            raise ValueError("the model's tail does not have the layout's shapes")
        self.shapes = {n: tuple(sd[n].shape) for n in self.tensors}
        self.grads = torch.zeros_like(self.params)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        # the trained span of the block: everything (groups 2) or proj's slice (groups 1)
        self._lo = 0 if self.unlocked_groups == 2 else self.offsets[14]
        self._scratch = None
        self._x = None

    @property
    def lr(self) -> float:
        return self.lr0 * cosine_factor(self.epoch, self.epochs)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def _slice(self, flat, name):
        i = self.tensors.index(name)
        return flat[self.offsets[i]:self.offsets[i + 1]].view(self.shapes[name])

    def _buffers(self, B):
        need = self.lib.miclip_ft_scratch_bytes(B, self.N, self.W, self.E, self.C, self.dh)
        if need <= 0:
            raise ValueError(f"unsupported batch size {B}")
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, device=self.device, dtype=torch.uint8)
        if self._x is None or self._x.shape[0] != B * self.N:
            self._x = torch.empty(B * self.N, self.W, device=self.device, dtype=self.x_dtype)
        return self._scratch, self._x

    def _labels(self, targets, B):
        if not isinstance(targets, torch.Tensor) or targets.ndim != 1 or targets.shape[0] != B:
            raise ValueError(f"Expected targets shape [{B}], got "
                             f"{tuple(getattr(targets, 'shape', ()))}.")
        if targets.dtype.is_floating_point or targets.dtype == torch.bool:
            raise TypeError(f"Expected integer targets, got dtype={targets.dtype}.")
        lab = targets.detach().to("cpu", torch.int64)
        if int(lab.min()) < 0 or int(lab.max()) >= self.C:
            raise ValueError(f"targets must lie in [0, {self.C}); got "
                             f"[{int(lab.min())}, {int(lab.max())}].")
        return targets.detach().to(self.device, torch.int64).contiguous()

    @torch.no_grad()
    def trunk(self, images):
        """Residual stream [B * N, W] entering the last block (the handle's stream type)."""
        h = self.model._require()
        R = self.model.config.image_resolution
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, R, R):
            raise ValueError(f"expected images [B, 3, {R}, {R}], got {tuple(images.shape)}")
        B = int(images.shape[0])
        if B < 1:
            raise ValueError("Empty inputs: the batch has no images.")
        in_dt = {torch.float16: _lib.MICLIP_FP16, torch.bfloat16: _lib.MICLIP_BF16}.get(
            images.dtype, _lib.MICLIP_F32)
        img = images.to(device=self.device, dtype=images.dtype if in_dt != _lib.MICLIP_F32
                        else torch.float32).contiguous()
        _, x = self._buffers(B)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.miclip_encode_image_trunk(
                h.ptr, _ptr(img), in_dt, B, _ptr(x), _lib.stream_handle(self.device)),
                "miclip_encode_image_trunk")
        return x

    @torch.no_grad()
    def grad(self, x, targets, feats=None):
        """Loss statistics and the gradients (into self.grads) for the residual stream x
        [B * N, W]; no optimiser step. feats (optional, [B, W] fp32) receives ln_post of
        the CLS rows under the master parameters."""
        B = int(x.shape[0]) // self.N
        labels = self._labels(targets, B)
        scratch, _ = self._buffers(B)
        stats = torch.empty(2, device=self.device, dtype=torch.float32)
        xdt = _lib.MICLIP_FP16 if x.dtype == torch.float16 else _lib.MICLIP_F32
        with torch.cuda.device(self.device):
            _lib.check(self.lib.miclip_ft_grad(
                _ptr(x), xdt, _ptr(labels), _ptr(self.text_weights), _ptr(self.params), B, self.N,
                self.W, self.E, self.C, self.dh, self.act, self.dtype, LOGIT_SCALE,
                self.unlocked_groups, _ptr(self.grads), _ptr(scratch), _ptr(stats),
                _ptr(feats) if feats is not None else None, _lib.stream_handle(self.device)),
                "miclip_ft_grad")
        return stats

    def adam(self):
        self.steps += 1
        n = self.params.numel() - self._lo
        with torch.cuda.device(self.device):
            _lib.check(self.lib.miclip_ft_adam(
                _ptr(self.params[self._lo:]), _ptr(self.grads[self._lo:]), _ptr(self.m[self._lo:]),
                _ptr(self.v[self._lo:]), n, float(self.lr), self.steps, ADAM_EPS,
                _lib.stream_handle(self.device)), "miclip_ft_adam")

    @torch.no_grad()
    def step(self, images, targets):
        x = self.trunk(images)
        stats = self.grad(x, targets)
        self.adam()
        return stats[0], stats[1]

    @torch.no_grad()
    def fill_view(self, cache: TrunkCache, loader, augment=None) -> int:
        """One pass of `trunk` over `loader`, appended to `cache` as a view; returns the
        view's index. Raw uint8 batches go through `prepare_images` with the parameters of
        `augment(sizes, first_row)` (as `compute_image_features`); transformed tensors are
        stored as the loader yields them. Raises ValueError, leaving the cache as it was,
        once the cached bytes would pass `cache.max_bytes`. While a view is filled its
        batches and their concatenation exist side by side."""
        parts, labels, row, held = [], [], 0, cache.nbytes
        for images, targets in loader:
            params = None
            if augment is not None and is_raw_batch(images):
                params = augment(raw_sizes(images), row)
            img = prepare_images(self.model, images, self.device, params)
            B = int(img.shape[0])
            lab = self._labels(targets, B)
            held += B * self.N * self.W * (torch.finfo(self.x_dtype).bits // 8)
            if cache.max_bytes is not None and held > cache.max_bytes:
                raise ValueError(
                    f"trunk cache: view {cache.views} needs {held} bytes after {row + B} images, "
                    f"over the budget of {cache.max_bytes} bytes (finetune.trunk_cache_max_bytes)")
            parts.append(self.trunk(img).clone())
            labels.append(lab)
            row += B
        if not parts:
            raise ValueError("Empty inputs: the loader yielded no batch.")
        if cache.batch_size is None:
            cache.batch_size = int(labels[0].numel())
        lab = torch.cat(labels)
        cache.x.append(torch.cat(parts) if len(parts) > 1 else parts[0])
        cache.targets.append(lab)
        cache.targets_host.append(lab.cpu())
        cache.n.append(row)
        return cache.views - 1

    @torch.no_grad()
    def grad_rows(self, cache: TrunkCache, view: int, rows, labels=None, feats=None):
        """`grad` for the cached images `rows` (host indices into view `view`, repeats
        allowed), read in place through `miclip_ft_grad_rows`. `labels` (optional, device
        int64 [B]) spares the gather of the view's targets."""
        idx = torch.as_tensor(rows, dtype=torch.int64, device="cpu").reshape(-1).contiguous()
        B, n, x = int(idx.numel()), cache.n[view], cache.x[view]
        if B < 1:
            raise ValueError("Empty inputs: rows has no index.")
        if int(idx.min()) < 0 or int(idx.max()) >= n:
            raise ValueError(f"rows must lie in [0, {n}); got [{int(idx.min())}, {int(idx.max())}].")
        if labels is None:
            labels = cache.targets[view][idx.to(self.device)]
        need = self.lib.miclip_ft_rows_scratch_bytes(B, self.N, self.W, self.E, self.C, self.dh)
        if need <= 0:
            raise ValueError(f"unsupported batch size {B}")
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, device=self.device, dtype=torch.uint8)
        stats = torch.empty(2, device=self.device, dtype=torch.float32)
        xdt = _lib.MICLIP_FP16 if x.dtype == torch.float16 else _lib.MICLIP_F32
        with torch.cuda.device(self.device):
            _lib.check(self.lib.miclip_ft_grad_rows(
                _ptr(x), xdt, n, ctypes.cast(idx.data_ptr(), ctypes.POINTER(ctypes.c_int64)),
                _ptr(labels), _ptr(self.text_weights), _ptr(self.params), B, self.N, self.W,
                self.E, self.C, self.dh, self.act, self.dtype, LOGIT_SCALE, self.unlocked_groups,
                _ptr(self.grads), _ptr(self._scratch), _ptr(stats),
                _ptr(feats) if feats is not None else None, _lib.stream_handle(self.device)),
                "miclip_ft_grad_rows")
        return stats

    @torch.no_grad()
    def step_rows(self, cache: TrunkCache, view: int, rows, labels=None):
        """`step` on the cached images `rows` of view `view`: no trunk."""
        stats = self.grad_rows(cache, view, rows, labels)
        self.adam()
        return stats[0], stats[1]

    @torch.no_grad()
    def features(self, images, normalize=True):
        """Embeddings [B, E] of `images` under the master parameters (before commit())."""
        x = self.trunk(images)
        B = int(images.shape[0])
        y = torch.empty(B, self.W, device=self.device, dtype=torch.float32)
        self.grad(x, torch.zeros(B, dtype=torch.int64), feats=y)   # self.grads is per step
        f = y @ self._slice(self.params, "visual.proj")
        return torch.nn.functional.normalize(f, dim=-1) if normalize else f

    @torch.no_grad()
    def commit(self) -> None:
        params = dict(self.model.named_parameters())
        for n in self.names:
            params[n].data.copy_(self._slice(self.params, n))
        self.model.refresh_weights()

    def optimizer_state_dict(self) -> dict:
        """torch.optim.Adam's state_dict over the trainable parameters in
        `named_parameters` order, as `optimizer.state_dict()` at :55 of
        aihab_utils/checkpointing.py would hold it."""
        opt = torch.optim.Adam([torch.nn.Parameter(self._slice(self.params, n).clone())
                                for n in self.names], lr=self.lr0)
        sd = opt.state_dict()
        group = sd["param_groups"][0]
        group["initial_lr"] = self.lr0        # CosineAnnealingLR's mark on the group
        group["lr"] = self.lr
        if self.steps:
            sd["state"] = {i: {"step": torch.tensor(float(self.steps)),
                               "exp_avg": self._slice(self.m, n).clone(),
                               "exp_avg_sq": self._slice(self.v, n).clone()}
                           for i, n in enumerate(self.names)}
        return sd

    def scheduler_state_dict(self) -> dict:
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=self.lr0)
        sd = torch.optim.lr_scheduler.CosineAnnealingLR(opt, self.epochs).state_dict()
        sd["last_epoch"] = self.epoch
        sd["_step_count"] = self.epoch + 1
        sd["_last_lr"] = [self.lr]
        return sd


def checkpoint_path(cfg, epoch: int, timestamp: str) -> Path:
    """File name of aihab_utils/checkpointing.py:17-30."""
    ft = cfg.get("finetune", {}) or {}
    out = Path(ft.get("save_model_dir", "model_ckpt"))
    if not out.is_absolute():
        out = Path(cfg.get("root_path", "./")) / out
    name = _canonical_backbone_name(str(cfg.get("open_clip_model", cfg.get("backbone", "openclip"))))
    return out / f"{name}_{int(epoch)}_{timestamp}.pt".replace("/", "_")


def save_checkpoint(cfg, model, trainer: Optional[LastBlockTrainer], epoch: int) -> Path:
    """Payload keys of aihab_utils/checkpointing.py:46-57."""
    ft = cfg.get("finetune", {}) or {}
    ts = datetime.now().strftime("%Y%m%d_%H")
    path = checkpoint_path(cfg, epoch, ts)
    path.parent.mkdir(parents=True, exist_ok=True)
    payload = {"model_state": model.state_dict(), "epoch": int(epoch), "timestamp": ts, "cfg": cfg,
               "clip_backend": cfg.get("clip_backend", "openclip"),
               "open_clip_model": cfg.get("open_clip_model", None)}
    if bool(ft.get("save_optimizer", True)) and trainer is not None:
        payload["optimizer_state"] = trainer.optimizer_state_dict()
    if bool(ft.get("save_scheduler", True)) and trainer is not None:
        payload["scheduler_state"] = trainer.scheduler_state_dict()
    torch.save(payload, path)
    return path


def _l2_context(cfg, ft_cfg, text_weights, device):
    """l2_eval_ctx of :166-193. The reference takes the L3 -> L2 map from its data
    package; here it comes with the config (`l3_to_l2`, `l2_names`)."""
    if not bool(ft_cfg.get("eval_l2", False)):
        return None
    subset = cfg.get("subset_l3", []) or []
    if isinstance(subset, (str, int)):
        subset = [subset]
    if len(subset) > 0:
        print("[warn] L2 eval disabled because subset_l3 is set.")
        return None
    l3_to_l2, l2_names = cfg.get("l3_to_l2"), cfg.get("l2_names")
    if l3_to_l2 is None or l2_names is None or len(l3_to_l2) != int(text_weights.shape[1]):
        print("[warn] L2 eval disabled due to L3 mapping size mismatch.")
        return None
    mode = str(ft_cfg.get("l2_eval_mode", "argmax")).lower()
    return {"l3_to_l2": torch.tensor(list(l3_to_l2), device=device, dtype=torch.long),
            "num_l2": len(l2_names), "l2_names": list(l2_names), "reduce": "mean",
            "topk": (1,) if mode == "argmax" else (1, 3), "mode": mode,
            "return_confusion_matrix": False}


def validate_config(cfg, model):
    """The settings FTOpenCLIP reads, checked before any device work:
    (unlocked_groups, tune_text, lr, epochs, val_interval)."""
    if "finetune" not in cfg:
        raise KeyError("finetune")
    ft = cfg["finetune"] or {}
    groups = int(ft.get("unlocked_groups", 1))
    tune_text = bool(ft.get("tune_text", False))
    trainable_names(model, groups, tune_text)
    lr, epochs = float(cfg["lr_v"]), int(cfg["train_epoch"])
    if epochs < 1:
        raise ValueError("train_epoch must be >= 1")
    return groups, tune_text, lr, epochs, int(ft.get("val_interval", 0))


class FTOpenCLIP:
    """`FTOpenCLIP(cfg)(train_loader, val_loader, test_loader, text_weights, model,
    classnames, shots, config_file, return_valid, prompt_tokens=None,
    num_templates=None)` as the reference calls it (:139-384): the same config keys,
    prints and return tuple, with the training step on the device and one host read
    per epoch."""

    def __init__(self, args):
        self.cfg = args

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def forward(self, train_loader, val_loader, test_loader, text_weights, model, classnames,
                shots, config_file, return_valid, prompt_tokens=None, num_templates=None):
        cfg = self.cfg
        groups, tune_text, lr, epochs, val_interval = validate_config(cfg, model)
        views, shuffle, budget = trunk_cache_config(cfg)
        ft_cfg = cfg["finetune"] or {}
        if getattr(model, "surface", None) != "open_clip":
            raise ValueError("FTOpenCLIP needs a model on the open_clip surface (encode_image "
                             "returns the projected embedding that validation scores)")
        device = _model_device(model)
        l2_ctx = _l2_context(cfg, ft_cfg, text_weights, device)

        names = trainable_names(model, groups)
        total = sum(1 for _ in model.named_parameters())
        print(f"Trainable params: {len(names)} ({len(names) / total:.1%})")
        print(f"Frozen params   : {total - len(names)}")
        tops = {}
        for n in names:
            tops.setdefault(n.split(".")[1] if "." in n else n, []).append(n)
        for g, ns in tops.items():
            print(f"  {g}: {len(ns)} params")
        print("Trainable (sample):", names[:10])
        vis = [n for n in names if n.startswith("visual")]
        print(f"Trainable vision params : {len(vis)}")
        print("Trainable vision (sample):", vis[:10])
        print("Trainable text params : 0")
        print("Trainable text (sample)  :", [])

        trainer = LastBlockTrainer(model, text_weights, unlocked_groups=groups, lr=lr, epochs=epochs)
        self.trainer = trainer
        cache = None
        if views:   # the frozen trunk, once per view (ProLIP's aug_views passes)
            if budget is None:
                budget = torch.cuda.mem_get_info(device)[0] // 2
            cache = TrunkCache(budget)
            for v in range(views):
                trainer.fill_view(cache, train_loader, _view_sampler(cfg, model, v))
        self.trunk_cache = cache
        seed = int(cfg.get("seed", 1) or 1)
        val = (None,) * 6
        print("\nStart Training procedure")
        for e in range(epochs):
            print("Train Epoch: {:} / {:}".format(e + 1, epochs))
            trainer.set_epoch(e)
            acc = torch.zeros(2, device=device, dtype=torch.float32)   # sum of batch-mean CE, correct
            seen = batches = 0
            if cache is None:
                for images, targets in train_loader:
                    x = prepare_images(model, images, device)
                    loss_sum, correct = trainer.step(x, targets)
                    acc[0] += loss_sum / x.shape[0]
                    acc[1] += correct
                    seen += int(x.shape[0])
                    batches += 1
            else:
                view = cache_view(e, views)
                order = cache_order(cache.n[view], seed, e, shuffle)
                labels = cache.targets[view][order.to(device)]    # the epoch's one upload
                for lo in range(0, cache.n[view], cache.batch_size):
                    rows = order[lo:lo + cache.batch_size]
                    B = int(rows.numel())
                    loss_sum, correct = trainer.step_rows(cache, view, rows, labels[lo:lo + B])
                    acc[0] += loss_sum / B
                    acc[1] += correct
                    seen += B
                    batches += 1
            run_loss, hits = acc.tolist()                              # the epoch's one host read
            print("Acc: {:.4f} ({:}/{:}), Avg Loss: {:.4f}, LR: {:.2e}".format(
                hits / max(seen, 1), hits, seen, run_loss / max(batches, 1), trainer.lr))
            trainer.set_epoch(e + 1)

            if (val_interval and (e + 1) % val_interval == 0) or e + 1 == epochs:
                if val_loader is not None:
                    trainer.commit()
                    r = run_validation(model, val_loader, text_weights, device,
                                       return_confusion_matrix=False, l2_eval_ctx=l2_ctx)
                    val = r[:6]
                    print(f"[val epoch {e + 1}] loss={r[0]:.4f}, top1_acc={r[1]:.4f}, "
                          f"top3_acc={r[2]:.4f}, f1={r[3]:.4f}, mcc={r[4]:.4f}")
                    if r[6] is not None:
                        print(_l2_line(f"[val epoch {e + 1} L2]", r[6]))
                else:
                    print(f"[val epoch {e + 1}] skipped (val_loader=None)")
        trainer.commit()

        test = (None,) * 6
        if test_loader is not None:
            r = run_validation(model, test_loader, text_weights, device,
                               return_confusion_matrix=True, cls_track=True, l2_eval_ctx=l2_ctx,
                               class_names=classnames)
            test = r[:6]
            print(f"[test] loss={r[0]:.4f}, top1_acc={r[1]:.4f}, top3_acc={r[2]:.4f}, "
                  f"f1={r[3]:.4f}, mcc={r[4]:.4f}")
            if r[6] is not None:
                print(_l2_line("[test L2]", r[6]))
        else:
            print("[test] skipped (test_loader=None)")

        saved = None
        if bool(ft_cfg.get("save_model", False)):
            try:
                saved = save_checkpoint(cfg, model, trainer, int(cfg.get("train_epoch", 0)))
                print(f"[ckpt] saved -> {saved}")
            except Exception as exc:   # the reference reports and goes on (:362-363)
                print(f"[ckpt] save failed: {exc}")
        self.checkpoint_path = saved

        if bool(ft_cfg.get("cache_embeddings", False)):
            split = str(ft_cfg.get("cache_embeddings_split", "test")).lower()
            loader = {"train": train_loader, "val": val_loader, "test": test_loader}.get(
                split, test_loader)
            if loader is None:
                print(f"[warn] cache_embeddings requested but loader for split '{split}' is None.")
            else:
                cache_openclip_embeddings(cfg=cfg, model=model, loader=loader, split=split,
                                          checkpoint_path=saved)
        return val if return_valid else test


def _l2_line(tag, m):
    msg = f"{tag} top1={m['top1']:.4f}, "
    if "top3" in m:
        msg += f"top3={m['top3']:.4f}, "
    return msg + f"f1={m['f1']:.4f}, mcc={m['mcc']:.4f}"
