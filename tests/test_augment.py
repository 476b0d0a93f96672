"""CPU: the host side of the train augmentations (miclip/augment.py).

Pillow (tests/_augment_ref.py) is the yardstick; the bar is bit equality.
"""
import math

import numpy as np
import pytest

import _augment_ref as ref
from miclip import augment as A

ANGLES = [0.0, 30.0, -30.0, 17.3, 1e-9, 90.0, 180.0, 270.0]


# ---------------------------------------------------------------- rotation rule
@pytest.mark.parametrize("R", [7, 28, 224, 336])
def test_rotation_rule_matches_pillow(R):
    rng = np.random.default_rng(R)
    img = ref.image(rng, R, R)
    for angle in ANGLES:
        want = np.asarray(ref.to_pil(img).rotate(angle, 0, expand=False, center=None,
                                                 fillcolor=0))
        got = A.rotate_nearest(img, A.rotation_affine(angle, R, R))
        assert np.array_equal(got, want), (R, angle)


def test_rotation_rule_non_square_and_grey():
    rng = np.random.default_rng(2)
    img = ref.image(rng, 5, 9, 1)[:, :, 0]
    for angle in ANGLES + [-17.3, 123.4]:
        want = np.asarray(ref.to_pil(img).rotate(angle, 0, fillcolor=0))
        assert np.array_equal(A.rotate_nearest(img, A.rotation_affine(angle, 9, 5)), want), angle


def test_right_angles_are_exact_integer_maps():
    one = 65536
    assert A.rotation_affine(0.0, 8, 8) == (one, 0, one // 2, 0, one, one // 2)
    assert A.rotation_affine(360.0, 8, 8) == A.rotation_affine(0.0, 8, 8)
    assert A.rotation_affine(-90.0, 8, 8) == A.rotation_affine(270.0, 8, 8)
    for angle in (90.0, 180.0, 270.0):
        assert all(v % (one // 2) == 0 for v in A.rotation_affine(angle, 8, 8))


# ---------------------------------------------------------------------- sampler
AUG = {"random_crop": True, "flip": True, "rotation": True}


def test_sampler_independent_of_batch_split():
    rng = np.random.default_rng(0)
    sizes = [(int(h), int(w)) for h, w in rng.integers(40, 700, (23, 2))]
    whole = A.sample_params(sizes, AUG, 224, seed=5, view=2, start=0)
    for bs in (1, 5, 16):
        parts = []
        for s in reversed(range(0, len(sizes), bs)):          # any order of calls
            parts = A.sample_params(sizes[s:s + bs], AUG, 224, seed=5, view=2, start=s) + parts
        assert parts == whole
    assert whole == A.sample_params(sizes, AUG, 224, seed=5, view=2)


def test_sampler_differs_across_views_and_seeds():
    sizes = [(439, 585)] * 16
    a = A.sample_params(sizes, AUG, 224, seed=1, view=0)
    assert a != A.sample_params(sizes, AUG, 224, seed=1, view=1)
    assert a != A.sample_params(sizes, AUG, 224, seed=2, view=0)
    assert len({(p.top, p.left, p.height, p.width) for p in a}) > 1
    assert len({p.angle for p in a}) == len(a)


def test_sampler_ranges():
    H, W = 439, 585
    ps = A.sample_params([(H, W)] * 2000, AUG, 224, seed=3, view=0)
    flips = 0
    for p in ps:
        assert p.mode == A.STRETCH
        assert 0 <= p.top and p.top + p.height <= H and 0 <= p.left and p.left + p.width <= W
        assert p.height >= 1 and p.width >= 1
        # w = round(sqrt(A r)), h = round(sqrt(A / r)): each within 0.5 of the real value
        lo_a = (p.width - 0.5) * (p.height - 0.5)
        hi_a = (p.width + 0.5) * (p.height + 0.5)
        assert hi_a >= 0.5 * H * W and lo_a <= 1.0 * H * W
        assert (p.width + 0.5) / (p.height - 0.5) >= 3 / 4
        assert (p.width - 0.5) / (p.height + 0.5) <= 4 / 3
        assert -30.0 <= p.angle <= 30.0
        flips += p.flip
    assert 850 < flips < 1150                      # p = 0.5, n = 2000: 6.7 sigma
    angles = np.array([p.angle for p in ps])
    assert angles.min() < -25 and angles.max() > 25 and abs(angles.mean()) < 2.0
    areas = np.array([p.height * p.width for p in ps]) / (H * W)
    assert areas.min() < 0.55 and areas.max() > 0.95


def test_sampler_switches():
    sizes = [(300, 400)] * 8
    for p in A.sample_params(sizes, {}, 224):
        assert p == A.AugParams()
    for p in A.sample_params(sizes, {"bottom_crop": True, "random_crop": True}, 224):
        assert (p.mode, p.top, p.left, p.height, p.width) == (A.CROP, 76, 88, 224, 224)
        assert not p.flip and p.angle is None
    # the flip and the angle of a row do not depend on the geometry switch or the size
    a = A.sample_params(sizes, AUG, 224, seed=9)
    b = A.sample_params([(50, 60)] * 8, {"flip": True, "rotation": True}, 224, seed=9)
    assert [(p.flip, p.angle) for p in a] == [(p.flip, p.angle) for p in b]
    with pytest.raises(ValueError, match="Crop size must be smaller than the image dimensions."):
        A.sample_params([(300, 200)], {"bottom_crop": True}, 224)


def test_sampler_fallback_when_every_attempt_fails():
    # 10 x 400: any accepted h would be >= sqrt(2000 / (4/3)) = 38.7 > 10
    for view in range(5):
        p = A.sample_params([(10, 400)], {"random_crop": True}, 224, seed=1, view=view)[0]
        assert (p.height, p.width, p.top, p.left) == (10, 13, 0, (400 - 13) // 2)
    p = A.sample_params([(400, 10)], {"random_crop": True}, 224)[0]
    assert (p.height, p.width, p.top, p.left) == (13, 10, (400 - 13) // 2, 0)


# --------------------------------------------------------------- host transform
@pytest.mark.parametrize("R", [28, 224])
@pytest.mark.parametrize("aug", [
    {"random_crop": True, "rotation": True},
    {"random_crop": True, "flip": True},
    {"bottom_crop": True, "flip": True, "rotation": True},
    {"flip": True, "rotation": True},
])
def test_host_transform_matches_yardstick(R, aug):
    rng = np.random.default_rng(R)
    tf = A.build_clip_transforms({"resolution": R, "augmentations": aug}, True, R, seed=4)
    for k, (h, w, c) in enumerate([(439, 585, 3), (300, 260, 3), (333, 517, 1), (250, 250, 3)]):
        img = ref.image(rng, h, w, c, smooth=True)
        pil = ref.to_pil(img)
        p = tf.params(pil)
        want = ref.transform(img, R, mode=p.mode, box=(p.top, p.left, p.height, p.width),
                             flip=p.flip, angle=p.angle)
        got = tf.apply(pil, p).numpy()
        assert got.dtype == np.float32 and got.shape == (3, R, R)
        assert np.array_equal(got, want), (h, w, c, p)
        assert np.array_equal(A.apply_params(img, p, R, uint8=True),
                              ref.transform_u8(img, R, mode=p.mode,
                                               box=(p.top, p.left, p.height, p.width),
                                               flip=p.flip, angle=p.angle))


def test_host_transform_is_seeded_and_varies():
    img = ref.to_pil(ref.image(np.random.default_rng(1), 120, 160))
    pre = {"augmentations": AUG}
    a = [A.build_clip_transforms(pre, True, 28, seed=7)(img) for _ in range(2)]
    tf = A.build_clip_transforms(pre, True, 28, seed=7)
    b = [tf(img), tf(img)]
    assert np.array_equal(a[0], a[1]) and np.array_equal(a[0], b[0])
    assert not np.array_equal(b[0], b[1])


def test_test_split_equals_transform():
    import miclip
    from miclip.preprocess import Transform
    assert miclip.build_clip_transforms is A.build_clip_transforms
    rng = np.random.default_rng(6)
    pre = {"resolution": 224, "augmentations": {"random_crop": True, "rotation": True,
                                                "flip": True}}
    tf = A.build_clip_transforms(pre, False, 224)
    for h, w, c in [(439, 585, 3), (301, 224, 3), (333, 517, 1)]:
        pil = ref.to_pil(ref.image(rng, h, w, c, smooth=True))
        assert np.array_equal(tf(pil).numpy(), Transform(224)(pil).numpy())
    # no switches on the train split: the same geometry
    tf = A.build_clip_transforms(None, True, 224)
    assert np.array_equal(tf(pil).numpy(), Transform(224)(pil).numpy())


def test_bottom_crop_error_text():
    tf = A.build_clip_transforms({"augmentations": {"bottom_crop": True}}, True, 224)
    with pytest.raises(ValueError, match="Crop size must be smaller than the image dimensions."):
        tf(ref.to_pil(ref.image(np.random.default_rng(0), 200, 300)))
    assert math.isclose(A.RATIO[0] * A.RATIO[1], 1.0)
