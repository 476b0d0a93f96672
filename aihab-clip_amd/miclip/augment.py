"""Training augmentations of the reference's CLIP transform.

Counterpart of data/clip_transforms.py:26-56 `build_clip_transforms` and
data/data_utils.py:9-31 `BottomSquareCrop`, which are torchvision.transforms.v2
on PIL images:

  train geometry (one of)  bottom_crop   BottomSquareCrop(R)
                           random_crop   RandomResizedCrop(R, scale=(0.5, 1), ratio=(3/4, 4/3),
                                         BICUBIC) = crop(i, j, h, w) then resize((R, R))
                           neither       Resize(R) of the short side + CenterCrop(R)
  then                     flip          RandomHorizontalFlip(0.5)
                           rotation      RandomRotation(30): Image.rotate(angle, NEAREST,
                                         expand=False, center=None, fillcolor=0)
  last, both modes         ToTensor + Normalize(CLIP_MEAN, CLIP_STD)

The random parameters are drawn here on the host (`sample_params`); the device
kernels behind `CLIP.preprocess_images(..., augment=params)` and the host
function `apply_params` are deterministic functions of them with bit-equal
outputs. A parameter set depends only on (seed, view, index of the image in
the pass), never on the batch size or the order of calls.

The distributions follow torchvision's published `RandomResizedCrop.get_params`,
`RandomHorizontalFlip` and `RandomRotation.get_params`. torchvision is not a
dependency of this package, so agreement with torchvision's own random stream
(torch's global generator) is not pinned: equal seeds give different, equally
distributed views.
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .weights import CLIP_MEAN, CLIP_STD

# miclip_aug_desc.mode (include/miclip.h MICLIP_AUG_*)
RESIZE_CENTER = 0
STRETCH = 1
CROP = 2

SCALE = (0.5, 1.0)
RATIO = (3.0 / 4.0, 4.0 / 3.0)
DEGREES = 30.0
CROP_ERROR = "Crop size must be smaller than the image dimensions."


@dataclass(frozen=True)
class AugParams:
    """One image's augmentation: geometry `mode` with its box (STRETCH, CROP),
    horizontal flip after the resize, rotation angle in degrees (None: none)."""
    mode: int = RESIZE_CENTER
    top: int = 0
    left: int = 0
    height: int = 0
    width: int = 0
    flip: bool = False
    angle: Optional[float] = None


# ------------------------------------------------------------------ rotation --
def _fix(v: float) -> int:
    """Geometry.c FIX: 16.16 fixed point, round half up."""
    return math.floor(v * 65536.0 + 0.5)


def rotation_affine(angle: float, w: int, h: int) -> Tuple[int, ...]:
    """(a0 .. a5), the 16.16 output -> source map of `Image.rotate(angle)` on a w x h image.

    PIL/Image.py `rotate` (NEAREST, expand=False, center=None): angle %= 360, the
    matrix of -radians(angle) with cos and sin rounded to 15 decimals about the
    centre (w/2, h/2); libImaging/Geometry.c `affine_fixed` then folds the
    half-pixel in (a2 = FIX(m2 + m0/2 + m1/2), a5 = FIX(m5 + m3/2 + m4/2)).
    For 0 / 180 (and 90 / 270 on a square image) Pillow copies or transposes;
    those are returned as the exact integer maps, so a consumer has one rule:
        xin = (a2 + y*a1 + x*a0) >> 16,  yin = (a5 + y*a4 + x*a3) >> 16
    in wrapping 32-bit arithmetic, fill 0 outside the image.
    """
    one, half = 65536, 32768
    angle = angle % 360.0
    rad = -math.radians(angle)
    c, s = round(math.cos(rad), 15), round(math.sin(rad), 15)
    if angle == 0 or (s == 0.0 and c > 0):
        return (one, 0, half, 0, one, half)
    if angle == 180 or (s == 0.0 and c < 0):
        return (-one, 0, (w - 1) * one + half, 0, -one, (h - 1) * one + half)
    if angle == 90 and w == h:      # ROTATE_90: out(x, y) = in(w-1-y, x)
        return (0, -one, (w - 1) * one + half, one, 0, half)
    if angle == 270 and w == h:     # ROTATE_270: out(x, y) = in(y, h-1-x)
        return (0, one, half, -one, 0, (h - 1) * one + half)
    m = [c, s, 0.0, -s, c, 0.0]
    cx, cy = w / 2, h / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def rotate_nearest(img: np.ndarray, affine: Sequence[int]) -> np.ndarray:
    """numpy statement of the rule in `rotation_affine` on an HxW[xC] array
    (what the device rotation kernel computes)."""
    h, w = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (int(v) for v in affine)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xin = _wrap32(a2 + y * a1 + x * a0) >> 16
    yin = _wrap32(a5 + y * a4 + x * a3) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


# ------------------------------------------------------------------- sampler --
# uniforms reserved per image, in this order: flip, angle, 10 x (area, aspect) of
# RandomResizedCrop's attempts, i, j; 8 Philox4x64 counter steps
_DRAWS = 32


def _uniforms(seed: int, view: int, start: int, n: int) -> np.ndarray:
    """[n, _DRAWS] doubles in [0, 1): row k is a function of (seed, view, start + k)
    alone -- Philox keyed by (seed, view), its counter set to the image's index."""
    mask = (1 << 64) - 1
    bg = np.random.Philox(key=np.array([int(seed) & mask, int(view) & mask], dtype=np.uint64))
    bg.advance(int(start) * (_DRAWS // 4))
    return np.random.Generator(bg).random((n, _DRAWS))


def _random_resized_crops(u: np.ndarray, H: np.ndarray, W: np.ndarray):
    """torchvision RandomResizedCrop.get_params for every row -> lists (i, j, h, w)."""
    area = (H * W).astype(np.float64)[:, None]
    lo, hi = math.log(RATIO[0]), math.log(RATIO[1])
    target = area * (SCALE[0] + (SCALE[1] - SCALE[0]) * u[:, 2:22:2])
    aspect = np.exp(lo + (hi - lo) * u[:, 3:22:2])
    w = np.rint(np.sqrt(target * aspect)).astype(np.int64)      # round half to even, as Python
    h = np.rint(np.sqrt(target / aspect)).astype(np.int64)
    ok = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
    first = ok.argmax(axis=1)
    rows = np.arange(len(H))
    w, h, hit = w[rows, first], h[rows, first], ok.any(axis=1)
    # randint(0, H - h + 1), randint(0, W - w + 1)
    i = np.minimum((u[:, 22] * (H - h + 1)).astype(np.int64), H - h)
    j = np.minimum((u[:, 23] * (W - w + 1)).astype(np.int64), W - w)
    out = []
    for k in range(len(H)):
        if hit[k]:
            out.append((int(i[k]), int(j[k]), int(h[k]), int(w[k])))
        else:
            out.append(_central_crop(int(H[k]), int(W[k])))
    return out


def _central_crop(H: int, W: int) -> Tuple[int, int, int, int]:
    """get_params' fallback after 10 rejected attempts: the aspect clamped to RATIO."""
    in_ratio = float(W) / float(H)
    if in_ratio < min(RATIO):
        w = W
        h = int(round(w / min(RATIO)))
    elif in_ratio > max(RATIO):
        h = H
        w = int(round(h * max(RATIO)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def bottom_square_crop(H: int, W: int, R: int) -> Tuple[int, int]:
    """BottomSquareCrop(R) anchor (top, left) (data/data_utils.py:24-30)."""
    if R > W or R > H:
        raise ValueError(CROP_ERROR)
    return H - R, (W - R) // 2


def sample_params(sizes: Sequence[Tuple[int, int]], augmentations: Optional[Dict],
                  resolution: int, seed: int = 1, view: int = 0, start: int = 0
                  ) -> List[AugParams]:
    """Train-transform parameters of images `start`, `start + 1`, ... of pass `view`.

    sizes: (H, W) of each image; augmentations: the reference's switches
    (`bottom_crop`, `random_crop`, `flip`, `rotation`). Image k's parameters
    are a function of (seed, view, start + k) and its size alone, so any split
    of a pass into batches, in any order, gives the same parameters. The flip
    and angle variates have their own places in the image's stream, so they
    depend neither on the image size nor on which switches are on.
    """
    aug = augmentations or {}
    n, R = len(sizes), int(resolution)
    if n == 0:
        return []
    u = _uniforms(seed, view, start, n)
    H = np.array([int(s[0]) for s in sizes], dtype=np.int64)
    W = np.array([int(s[1]) for s in sizes], dtype=np.int64)
    if H.min() < 1 or W.min() < 1:
        raise ValueError("image sizes must be positive")
    mode, boxes = RESIZE_CENTER, [(0, 0, 0, 0)] * n
    if aug.get("bottom_crop", False):
        mode = CROP
        boxes = [bottom_square_crop(int(h), int(w), R) + (R, R) for h, w in zip(H, W)]
    elif aug.get("random_crop", False):
        mode, boxes = STRETCH, _random_resized_crops(u, H, W)
    flips = (u[:, 0] < 0.5).tolist() if aug.get("flip", False) else [False] * n
    angles = (-DEGREES + 2 * DEGREES * u[:, 1]).tolist() if aug.get("rotation", False) \
        else [None] * n
    return [AugParams(mode, *boxes[k], flip=flips[k], angle=angles[k]) for k in range(n)]


# ---------------------------------------------------------------- host apply --
def _normalize(u8: np.ndarray) -> torch.Tensor:
    a = np.asarray(u8, dtype=np.float32) / 255.0                             # ToTensor
    a = (a - np.asarray(CLIP_MEAN, np.float32)) / np.asarray(CLIP_STD, np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def apply_params(image, p: AugParams, resolution: int, uint8: bool = False):
    """The train transform with given parameters on one PIL image (or HxW[xC] uint8
    array), on the host with Pillow: float32 [3, R, R], or with uint8=True the
    RGB pixels uint8 [R, R, 3]. Bit-equal to `CLIP.preprocess_images(augment=[p])`."""
    from PIL import Image
    R = int(resolution)
    if isinstance(image, np.ndarray):
        image = Image.fromarray(image[:, :, 0] if image.ndim == 3 and image.shape[2] == 1
                                else image)
    if p.mode == RESIZE_CENTER:
        w, h = image.size
        if w <= h:
            nw, nh = R, int(R * h / w)
        else:
            nw, nh = int(R * w / h), R
        image = image.resize((nw, nh), Image.BICUBIC)
        left, top = int(round((nw - R) / 2.0)), int(round((nh - R) / 2.0))
        image = image.crop((left, top, left + R, top + R))
    elif p.mode in (STRETCH, CROP):
        w, h = image.size
        if p.mode == CROP and (R > w or R > h):
            raise ValueError(CROP_ERROR)
        if (p.top < 0 or p.left < 0 or p.height < 1 or p.width < 1 or p.top + p.height > h
                or p.left + p.width > w or (p.mode == CROP and (p.height, p.width) != (R, R))):
            raise ValueError(f"box {(p.top, p.left, p.height, p.width)} does not fit the "
                             f"{h}x{w} image")
        image = image.crop((p.left, p.top, p.left + p.width, p.top + p.height))
        if p.mode == STRETCH:
            image = image.resize((R, R), Image.BICUBIC)
    else:
        raise ValueError(f"unknown augmentation mode {p.mode}")
    if p.flip:
        image = image.transpose(Image.FLIP_LEFT_RIGHT)
    if p.angle is not None:
        image = image.rotate(p.angle, Image.NEAREST, expand=False, center=None, fillcolor=0)
    u8 = np.asarray(image.convert("RGB"))
    return u8 if uint8 else _normalize(u8)


class ClipTransform:
    """Host callable returned by `build_clip_transforms`: PIL image -> float32 [3, R, R]."""

    def __init__(self, augmentations: Optional[Dict], is_train: bool, resolution: int,
                 seed: Optional[int] = None):
        self.augmentations = dict(augmentations or {}) if is_train else {}
        self.is_train = bool(is_train)
        self.resolution = int(resolution)
        self.seed = int(np.random.SeedSequence(seed).generate_state(1)[0])
        self._count = 0

    def params(self, image) -> AugParams:
        """Draws the next image's parameters (one generator state per call)."""
        w, h = image.size
        p = sample_params([(h, w)], self.augmentations, self.resolution, self.seed, 0,
                          self._count)[0]
        self._count += 1
        return p

    def apply(self, image, p: AugParams) -> torch.Tensor:
        return apply_params(image, p, self.resolution)

    def __call__(self, image) -> torch.Tensor:
        from PIL import Image
        if isinstance(image, np.ndarray):
            image = Image.fromarray(image)
        return self.apply(image, self.params(image))

    def __repr__(self):
        return (f"ClipTransform(train={self.is_train}, {self.augmentations}, "
                f"resolution={self.resolution})")


def build_clip_transforms(preproc: Optional[Dict], is_train: bool, resolution: int = 224,
                          seed: Optional[int] = None) -> ClipTransform:
    """Drop-in for data/clip_transforms.py:26-56 on Pillow alone (no torchvision).

    `preproc` is the reference's `data.preprocessing` mapping; its
    `augmentations` switches apply to the train split only. `seed` (not in the
    reference, which uses torch's global generator) fixes the stream of views."""
    aug = preproc.get("augmentations", {}) if preproc else {}
    return ClipTransform(aug, is_train, resolution, seed)
