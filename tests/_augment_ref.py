"""Yardstick of the train-transform tests: Pillow, called the way torchvision.transforms.v2
calls it on a PIL image (data/clip_transforms.py:36-56 with given parameters):

    crop (F.crop -> Image.crop) -> resize (Image.resize((R, R), BICUBIC)) ->
    transpose(FLIP_LEFT_RIGHT) -> rotate(angle, NEAREST, expand=False, center=None,
    fillcolor=0) -> convert("RGB") -> x / 255 -> Normalize(CLIP_MEAN, CLIP_STD)

Parameters are plain values (no miclip types), so nothing of the code under test
runs here; the test geometry (neither crop) is oracle.pil_resample's.
"""
import numpy as np
from PIL import Image

from oracle import pil_resample as P

RESIZE_CENTER, STRETCH, CROP = 0, 1, 2


def to_pil(img):
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    return Image.fromarray(img)


def image(rng, h, w, c=3, smooth=False):
    if smooth:
        y, x = np.mgrid[0:h, 0:w]
        base = 127 + 60 * np.sin(x / 17.0)[..., None] * np.cos(y / 23.0)[..., None]
        return np.clip(base + rng.normal(0, 20, (h, w, c)), 0, 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def transform_u8(img, R, mode=RESIZE_CENTER, box=None, flip=False, angle=None):
    """uint8 [R, R, 3] of one HxWxC uint8 image; box = (top, left, height, width)."""
    if mode == RESIZE_CENTER:
        im = to_pil(P.crop_u8(np.asarray(img), R, resize=P.pil_resize))
    else:
        top, left, h, w = box
        im = to_pil(img).crop((left, top, left + w, top + h))
        if mode == STRETCH:
            im = im.resize((R, R), Image.BICUBIC)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if angle is not None:
        im = im.rotate(angle, Image.NEAREST, expand=False, center=None, fillcolor=0)
    return np.asarray(im.convert("RGB"))


def transform(img, R, **kw):
    """float32 [3, R, R]: transform_u8 + ToTensor + Normalize."""
    return P.normalize(transform_u8(img, R, **kw))
