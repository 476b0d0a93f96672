#!/usr/bin/env python3
"""Cost of the on-device train transform (csrc/preprocess.hip, miclip_preprocess_aug)
next to the test transform, the host Pillow path and the encoder it feeds.

    python scripts/bench_augment.py [--rounds 5] [--iters 20] [--out FILE]

Workload: `--batch` (256) decoded uint8 RGB images of 439 x 585 (the reference's
`resize: 439` of a 4:3 frame) already in device memory -> float32 [B, 3, 224, 224].
In one process, the variants alternating round by round:

  center        preprocess_images(frames)                       (the test transform)
  random_crop   augment = RandomResizedCrop boxes               (tables + stretch resample)
  crop_rotate   augment = boxes + RandomRotation(30)            (+ uint8 scratch + gather)

each timed with device events around `--iters` calls on torch's current stream
(the parameters are drawn before the window; drawing them is timed apart, per
image, on the host), after an untimed warm-up of every variant. The best round
counts; all rounds are recorded. Then

  host_pillow   augment.apply_params on one thread (the reference's num_workers: 0),
                `--cpu-images` images, random_crop + rotation
  cache_loop    compute_image_features(to_cpu=True, fp16) of ViT-B/32 over
                `--loop-batches` such batches, without and with the augmentation
                (host clock around the loop, which ends in a device synchronise),
                alternating

One JSON line per record. Not part of bench.py.
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "aihab-clip_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

AUGS = {"center": None,
        "random_crop": {"random_crop": True},
        "crop_rotate": {"random_crop": True, "rotation": True}}


def frames_u8(B, H, W, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy = torch.linspace(0, 6.28, H, device="cuda").view(1, H, 1, 1)
    xx = torch.linspace(0, 6.28, W, device="cuda").view(1, 1, W, 1)
    ph = torch.rand(B, 1, 1, 3, device="cuda", generator=g) * 6.28
    return (127 + 60 * torch.sin(xx * 3 + ph) * torch.cos(yy * 2 + ph)
            + torch.randn(B, H, W, 3, device="cuda", generator=g) * 20).clamp_(0, 255).to(torch.uint8)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--height", type=int, default=439)
    ap.add_argument("--width", type=int, default=585)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-images", type=int, default=64)
    ap.add_argument("--loop-batches", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"

    import miclip
    from miclip import augment as A
    from miclip.feature_cache import compute_image_features
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", miclip.SeededWeightsWarning)
        _, model, _ = miclip.load("ViT-B/32", device="cuda")
    R, B, H, W = model.config.image_resolution, a.batch, a.height, a.width
    frames = frames_u8(B, H, W)
    sizes = [(H, W)] * B
    out = torch.empty(B, 3, R, R, device="cuda")
    dev_name = torch.cuda.get_device_name(0)
    common = {"batch": B, "image": f"{H}x{W}x3", "resolution": R, "device": dev_name}
    lines = []

    # --- the three device calls, alternating ---
    t0 = time.perf_counter()
    params = {k: None if aug is None else A.sample_params(sizes, aug, R, seed=1, view=0)
              for k, aug in AUGS.items()}
    sample_us = (time.perf_counter() - t0) / (2 * B) * 1e6
    calls = {k: (lambda p=p: model.preprocess_images(frames, out=out, augment=p))
             for k, p in params.items()}
    for fn in calls.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            ms[k].append(round(event_ms(fn, a.iters), 4))
    best = {k: min(v) for k, v in ms.items()}
    rec = dict(common, workload="preprocess_calls", rounds=a.rounds, iters=a.iters,
               ms_per_batch=ms, sample_params_us_per_image=round(sample_us, 2))
    for k, v in best.items():
        rec[f"{k}_us_per_image"] = round(v / B * 1e3, 3)
    rec["random_crop_over_center"] = round(best["random_crop"] / best["center"], 2)
    rec["crop_rotate_over_center"] = round(best["crop_rotate"] / best["center"], 2)
    lines.append(rec)
    print(json.dumps(rec), flush=True)

    # --- the host path, one thread ---
    torch.set_num_threads(1)
    host = frames[: a.cpu_images].cpu().numpy()
    ps = params["crop_rotate"][: a.cpu_images]
    same = np.array_equal(A.apply_params(host[0], ps[0], R).numpy(),
                          model.preprocess_images(frames[:1], augment=ps[:1])[0].cpu().numpy())
    t0 = time.perf_counter()
    for im, p in zip(host, ps):
        A.apply_params(im, p, R)
    dt = time.perf_counter() - t0
    rec = dict(common, workload="host_pillow", images=len(ps), threads=1,
               augmentations=AUGS["crop_rotate"], us_per_image=round(dt / len(ps) * 1e6, 1),
               images_per_s=round(len(ps) / dt, 1), device_output_bit_identical=bool(same))
    lines.append(rec)
    print(json.dumps(rec), flush=True)

    # --- the ViT-B/32 cache loop, alternating ---
    labels = torch.zeros(B, dtype=torch.int64)
    loader = [(frames, labels)] * a.loop_batches

    def loop(aug):
        sampler = None
        if aug is not None:
            def sampler(s, row):
                return A.sample_params(s, aug, R, 1, 0, row)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        compute_image_features(model, loader, to_cpu=True, out_dtype=torch.float16,
                               augment=sampler)
        torch.cuda.synchronize()
        return B * a.loop_batches / (time.perf_counter() - t0)

    loop(None)
    loop(AUGS["crop_rotate"])
    rate = {"plain": [], "augmented": []}
    for _ in range(a.rounds):
        rate["plain"].append(round(loop(None), 1))
        rate["augmented"].append(round(loop(AUGS["crop_rotate"]), 1))
    rec = dict(common, workload="cache_loop", model="ViT-B/32", batches=a.loop_batches,
               rounds=a.rounds, augmentations=AUGS["crop_rotate"], images_per_s=rate,
               plain_best=max(rate["plain"]), augmented_best=max(rate["augmented"]))
    rec["augmented_over_plain"] = round(rec["augmented_best"] / rec["plain_best"], 3)
    lines.append(rec)
    print(json.dumps(rec), flush=True)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
