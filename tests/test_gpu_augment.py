"""GPU: the train transform on the device (miclip_preprocess_aug).

`CLIP.preprocess_images(..., augment=params)` against Pillow called the way
torchvision calls it (tests/_augment_ref.py): crop -> resize -> flip -> rotate ->
RGB -> ToTensor -> Normalize. Bar: bit equality of the uint8 pixels and of the
float32 tensor, everywhere.
"""
import dataclasses

import numpy as np
import pytest
import torch

import _augment_ref as ref
from miclip import augment as A

pytestmark = pytest.mark.gpu

ANGLES = [0.0, 30.0, -30.0, 17.3, 1e-9, 90.0, 180.0, 270.0]
_MODELS = {}


def _tiny_model(n):
    import miclip
    from miclip.configs import CLIPConfig
    from miclip.weights import generate_state_dict
    if n not in _MODELS:
        cfg = CLIPConfig(embed_dim=64, image_resolution=n, vision_layers=1, vision_width=256,
                         vision_patch_size=n // 7, context_length=77, vocab_size=49408,
                         transformer_width=256, transformer_heads=4, transformer_layers=1)
        sd = {k: torch.from_numpy(v) for k, v in generate_state_dict(cfg, seed=0).items()}
        _MODELS[n] = miclip.CLIP(cfg, sd, device="cuda")
    return _MODELS[n]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    yield
    _MODELS.clear()


def _want(img, R, p, uint8):
    f = ref.transform_u8 if uint8 else ref.transform
    return f(img, R, mode=p.mode, box=(p.top, p.left, p.height, p.width), flip=p.flip,
             angle=p.angle)


def _check(m, imgs, params):
    """uint8 and float32 device outputs of the batch == Pillow, image by image."""
    R = m.config.image_resolution
    u8 = m.preprocess_images(imgs, uint8=True, augment=params).cpu().numpy()
    f32 = m.preprocess_images(imgs, augment=params).cpu().numpy()
    assert u8.shape == (len(imgs), R, R, 3) and u8.dtype == np.uint8
    assert f32.shape == (len(imgs), 3, R, R) and f32.dtype == np.float32
    for i, (img, p) in enumerate(zip(imgs, params)):
        want = _want(img, R, p, True)
        bad = np.argwhere(u8[i] != want)
        assert bad.size == 0, (i, img.shape, p, bad[:5], u8[i][tuple(bad[0])], want[tuple(bad[0])])
        assert np.array_equal(f32[i], _want(img, R, p, False)), (i, img.shape, p)
    return u8, f32


def _stretch(top, left, h, w, **kw):
    return A.AugParams(A.STRETCH, top, left, h, w, **kw)


# ------------------------------------------------------------------- STRETCH --
@pytest.mark.parametrize("R", [28, 224])
def test_stretch_boxes_bit_exact(R):
    rng = np.random.default_rng(R)
    s = R / 224
    cases = [      # (H, W, C), box (top, left, h, w) at R = 224; scaled for R = 28
        ((300, 400, 3), (20, 30, 150, 260)),      # up in y, down in x
        ((300, 400, 3), (11, 7, 260, 150)),       # down in y, up in x
        ((439, 585, 3), (0, 0, 310, 413)),        # box at (0, 0)
        ((439, 585, 3), (439 - 333, 585 - 444, 333, 444)),   # ends at the last pixel
        ((439, 585, 3), (0, 0, 439, 585)),        # the whole image
        ((333, 517, 1), (100, 17, 199, 265)),     # 'L' image
        ((333, 517, 1), (333 - 224, 517 - 225, 224, 225)),   # identity in y, last pixel
        ((64, 64, 3), (3, 5, 1, 1)),              # one pixel
        ((64, 64, 3), (60, 59, 3, 5)),
        ((1080, 1920, 3), (0, 0, 1080, 1440)),    # 6.4x down (R = 224)
    ]
    imgs, params = [], []
    for (H, W, C), (t, l, h, w) in cases:
        H, W = max(int(H * s), 8), max(int(W * s), 8)
        h, w = max(int(h * s), 1), max(int(w * s), 1)
        t, l = min(int(t * s), H - h), min(int(l * s), W - w)
        imgs.append(ref.image(rng, H, W, C, smooth=len(imgs) % 2 == 1))
        params.append(_stretch(t, l, h, w))
    _check(_tiny_model(R), imgs, params)


@pytest.mark.parametrize("B", [1, 40])
def test_stretch_ragged_batches(B):
    rng = np.random.default_rng(B)
    sizes = [(int(h), int(w)) for h, w in rng.integers(120, 640, (B, 2))]
    imgs = [ref.image(rng, h, w, 1 if i % 7 == 3 else 3, smooth=True)
            for i, (h, w) in enumerate(sizes)]
    params = A.sample_params(sizes, {"random_crop": True}, 224, seed=B)
    assert all(p.mode == A.STRETCH for p in params)
    _check(_tiny_model(224), imgs, params)


def test_everything_at_336():
    rng = np.random.default_rng(336)
    sizes = [(439, 585), (600, 500), (336, 336), (1000, 1400), (200, 150), (439, 585)]
    imgs = [ref.image(rng, h, w, 3, smooth=True) for h, w in sizes]
    params = A.sample_params(sizes, {"random_crop": True, "flip": True, "rotation": True}, 336,
                             seed=3)
    params[2] = A.AugParams(A.CROP, 0, 0, 336, 336, flip=True, angle=-7.5)
    params[5] = A.AugParams(flip=True)
    _check(_tiny_model(336), imgs, params)


# ---------------------------------------------------------------------- CROP --
@pytest.mark.parametrize("R", [28, 224])
def test_crop_equals_slicing(R):
    rng = np.random.default_rng(R + 1)
    sizes = [(R, R, 3), (R + 1, R + 7, 3), (2 * R + 3, 3 * R, 1), (439, 585, 3)]
    imgs = [ref.image(rng, h, w, c) for h, w, c in sizes]
    params = A.sample_params([s[:2] for s in sizes], {"bottom_crop": True}, R)
    params[3] = A.AugParams(A.CROP, 5, 9, R, R)                 # any R x R box
    m = _tiny_model(R)
    u8 = m.preprocess_images(imgs, uint8=True, augment=params).cpu().numpy()
    for i, (img, p) in enumerate(zip(imgs, params)):
        if i < 3:
            assert (p.top, p.left) == (img.shape[0] - R, (img.shape[1] - R) // 2)
        cut = img[p.top:p.top + R, p.left:p.left + R]
        assert np.array_equal(u8[i], np.repeat(cut, 3, axis=2) if cut.shape[2] == 1 else cut), i
    _check(m, imgs, params)


# ------------------------------------------------------------- RESIZE_CENTER --
def test_resize_center_equals_the_test_transform():
    rng = np.random.default_rng(5)
    sizes = [(480, 640, 3), (300, 224, 3), (224, 224, 3), (100, 150, 3), (333, 517, 1),
             (7, 9, 3), (1080, 1920, 3)]
    imgs = [ref.image(rng, h, w, c, smooth=True) for h, w, c in sizes]
    m = _tiny_model(224)
    none = [A.AugParams()] * len(imgs)
    assert torch.equal(m.preprocess_images(imgs, augment=none), m.preprocess_images(imgs))
    assert torch.equal(m.preprocess_images(imgs, uint8=True, augment=none),
                       m.preprocess_images(imgs, uint8=True))
    batch = torch.from_numpy(np.stack([imgs[0]] * 3)).cuda()      # [B,H,W,C] device tensor
    assert torch.equal(m.preprocess_images(batch, augment=none[:3]), m.preprocess_images(batch))


# ---------------------------------------------------------------------- flip --
@pytest.mark.parametrize("R", [28, 224])
def test_flip_with_each_geometry(R):
    rng = np.random.default_rng(R + 2)
    H, W = 2 * R + 5, 3 * R + 1
    imgs = [ref.image(rng, H, W, c, smooth=True) for c in (3, 3, 3, 1, 3, 3)]
    params = [A.AugParams(flip=True),
              _stretch(3, 10, R + 9, 2 * R + 3, flip=True),
              A.AugParams(A.CROP, H - R, 4, R, R, flip=True),
              _stretch(0, 0, H, W, flip=True),
              _stretch(3, 10, R + 9, 2 * R + 3, flip=False),
              _stretch(1, 2, R - 5, R - 3, flip=True, angle=12.0)]
    u8, _ = _check(_tiny_model(R), imgs, params)
    assert not np.array_equal(u8[1], u8[1][:, ::-1])


# ------------------------------------------------------------------ rotation --
@pytest.mark.parametrize("R", [28, 224])
def test_rotation_angles(R):
    rng = np.random.default_rng(R + 3)
    H, W = 2 * R + 5, 3 * R + 1
    geos = [dict(), dict(mode=A.STRETCH, top=3, left=10, height=R + 9, width=2 * R + 3),
            dict(mode=A.CROP, top=H - R, left=4, height=R, width=R)]
    imgs, params = [], []
    for k, angle in enumerate(ANGLES + [-17.3, 29.999, -1e-9]):
        imgs.append(ref.image(rng, H, W, 1 if k == 4 else 3))
        params.append(A.AugParams(angle=angle, flip=k % 3 == 1, **geos[k % 3]))
    _check(_tiny_model(R), imgs, params)


def test_rotation_mixed_batch_and_independence():
    rng = np.random.default_rng(9)
    R = 224
    sizes = [(439, 585), (300, 260), (250, 333), (439, 585), (600, 800), (224, 224)]
    imgs = [ref.image(rng, h, w, 3, smooth=True) for h, w in sizes]
    params = A.sample_params(sizes, {"random_crop": True, "flip": True, "rotation": True}, R,
                             seed=11)
    for i in (1, 4):                                  # unrotated images among rotated ones
        params[i] = dataclasses.replace(params[i], angle=None)
    m = _tiny_model(R)
    u8, f32 = _check(m, imgs, params)
    order = [3, 0, 5]                                 # other neighbours, other tap maxima
    sub = m.preprocess_images([imgs[i] for i in order], augment=[params[i] for i in order])
    for k, i in enumerate(order):
        assert np.array_equal(sub[k].cpu().numpy(), f32[i])
    for i in (1, 2):                                  # alone: single pass (1), two passes (2)
        one = m.preprocess_images([imgs[i]], uint8=True, augment=[params[i]]).cpu().numpy()[0]
        assert np.array_equal(one, u8[i])


# ------------------------------------------------------- out-of-bounds writes --
@pytest.mark.parametrize("uint8", [False, True])
def test_guard_regions_stay_untouched(uint8):
    rng = np.random.default_rng(13)
    R, B, G = 28, 5, 4096
    sizes = [(61, 83), (40, 40), (90, 57), (28, 28), (33, 29)]
    imgs = [ref.image(rng, h, w, 3) for h, w in sizes]
    m = _tiny_model(R)
    dt, fill = (torch.uint8, 0xA5) if uint8 else (torch.float32, -12345.0)
    n = B * 3 * R * R
    for aug in ({"random_crop": True, "flip": True}, {"random_crop": True, "rotation": True}):
        params = A.sample_params(sizes, aug, R, seed=2)
        big = torch.full((G + n + G,), fill, dtype=dt, device="cuda")
        out = big[G:G + n].view((B, R, R, 3) if uint8 else (B, 3, R, R))
        got = m.preprocess_images(imgs, uint8=uint8, out=out, augment=params)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert bool((big[:G] == fill).all()) and bool((big[G + n:] == fill).all())
        for i, (img, p) in enumerate(zip(imgs, params)):
            assert np.array_equal(out[i].cpu().numpy(), _want(img, R, p, uint8))


# -------------------------------------------------------------------- errors --
def test_errors():
    m = _tiny_model(224)
    img = np.zeros((300, 400, 3), np.uint8)
    for box in [(0, 0, 301, 400), (1, 0, 300, 400), (0, 1, 300, 400), (-1, 0, 10, 10),
                (0, 0, 0, 10), (0, 2 ** 31 - 1, 10, 10)]:
        with pytest.raises(ValueError, match="leaves the"):
            m.preprocess_images([img], augment=[_stretch(*box)])
        with pytest.raises(ValueError):
            m.preprocess_images([img], augment=[A.AugParams(A.CROP, *box)])
    with pytest.raises(ValueError, match="not 224x224"):
        m.preprocess_images([img], augment=[A.AugParams(A.CROP, 0, 0, 224, 225)])
    with pytest.raises(ValueError, match="unknown mode"):
        m.preprocess_images([img], augment=[A.AugParams(3)])
    small = np.zeros((200, 300, 3), np.uint8)
    text = "Crop size must be smaller than the image dimensions."
    with pytest.raises(ValueError, match=text):                 # BottomSquareCrop's own error
        m.preprocess_images([small], augment=[A.AugParams(A.CROP, 0, 38, 224, 224)])
    with pytest.raises(ValueError, match=text):
        A.sample_params([(200, 300)], {"bottom_crop": True}, 224)
    big = np.zeros((4000, 4000, 1), np.uint8)                   # 4000 -> 224: 73 taps
    with pytest.raises(ValueError, match="taps"):
        m.preprocess_images([big], augment=[_stretch(0, 0, 4000, 4000)])
    with pytest.raises(ValueError, match="taps"):
        m.preprocess_images([big], augment=[_stretch(0, 0, 4000, 300)])
    with pytest.raises(ValueError, match="taps"):
        m.preprocess_images([big], augment=[A.AugParams()])
    with pytest.raises(ValueError, match="entries"):
        m.preprocess_images([img, img], augment=[A.AugParams()])
    assert m.preprocess_images([], augment=[]).shape == (0, 3, 224, 224)
    # the handle still works after the refusals
    ok = m.preprocess_images([big], uint8=True, augment=[_stretch(0, 0, 2000, 2000)])
    assert int(ok.max()) == 0


# -------------------------------------------------------------------- driver --
def _loader(imgs, labels, bs):
    return [(imgs[s:s + bs], torch.from_numpy(labels[s:s + bs])) for s in range(0, len(imgs), bs)]


def test_cache_driver_writes_augmented_views(tmp_path):
    from miclip.feature_cache import cache_preprojection_features
    rng = np.random.default_rng(21)
    R, n = 28, 21
    sizes = [(int(h), int(w)) for h, w in rng.integers(40, 120, (n, 2))]
    imgs = [ref.image(rng, h, w, 3, smooth=True) for h, w in sizes]
    labels = np.arange(n, dtype=np.int64) % 4
    aug = {"bottom_crop": False, "random_crop": True, "flip": False, "rotation": True}
    cfg = {"root_path": str(tmp_path), "dataset": "cs", "seed": 7, "shots": 4,
           "backbone": "tiny", "aug_views": 3, "cache_dtype": "fp32",
           "data": {"batch_size": 16, "preprocessing": {"resize": 439, "resolution": R,
                                                        "augmentations": aug}}}
    m = _tiny_model(R)
    d = cache_preprojection_features(cfg, {"clip_model": m}, _loader(imgs, labels, 16),
                                     {"train_size": n})
    views = [torch.load(d / f"f{v}.pth", weights_only=True) for v in range(3)]
    assert torch.equal(torch.load(d / "label.pth", weights_only=True), torch.from_numpy(labels))
    for a in range(3):
        assert views[a].shape == (n, 256) and views[a].dtype == torch.float32
        for b in range(a):
            assert not torch.equal(views[a], views[b])
    # each view = encode_image of the host transform with the same parameters, bitwise
    pix16 = []
    for v in range(3):
        params = A.sample_params(sizes, aug, R, seed=7, view=v)
        host = torch.stack([A.apply_params(im, p, R) for im, p in zip(imgs, params)]).cuda()
        pix16.append(host)
        feats = torch.cat([m.encode_image(host[s:s + 16]) for s in range(0, n, 16)]).cpu()
        assert torch.equal(views[v], feats), v
    # a rerun with the same seed reproduces the files; another seed does not
    d2 = cache_preprojection_features(dict(cfg, root_path=str(tmp_path / "again")),
                                      {"clip_model": m}, _loader(imgs, labels, 16), None)
    for v in range(3):
        assert torch.equal(torch.load(d2 / f"f{v}.pth", weights_only=True), views[v])
    d3 = cache_preprojection_features(dict(cfg, seed=8, aug_views=1), {"clip_model": m},
                                      _loader(imgs, labels, 16), None)
    assert not torch.equal(torch.load(d3 / "f0.pth", weights_only=True), views[0])
    # the preprocessed pixels do not depend on the batch size
    from miclip.feature_cache import _view_sampler, prepare_images
    for v in (0, 2):
        sampler = _view_sampler(cfg, m, v)
        for bs in (16, 5):
            pix = torch.cat([prepare_images(m, imgs[s:s + bs], m.device,
                                            sampler(sizes[s:s + bs], s))
                             for s in range(0, n, bs)])
            assert torch.equal(pix, pix16[v]), (v, bs)
    # without data.preprocessing the views are what the loader yields (today's behaviour)
    plain = {k: v for k, v in cfg.items() if k != "data"}
    d4 = cache_preprojection_features(dict(plain, root_path=str(tmp_path / "plain"), aug_views=2),
                                      {"clip_model": m}, _loader(imgs, labels, 16), None)
    assert torch.equal(torch.load(d4 / "f0.pth", weights_only=True),
                       torch.load(d4 / "f1.pth", weights_only=True))
