#!/usr/bin/env python3
"""Time last-block fine-tuning from the trunk cache (miclip.finetune.TrunkCache) on one device.

    python scripts/bench_finetune_cache.py [--rounds 3] [--steps 5] [--model ViT-L/14]
                                           [--batch 256] [--batches 4] [--out FILE]

One config (fp16, seeded weights and images), in one process, bench_finetune.py's protocol:
  step     ms of the uncached group-2 training step (trunk + miclip_ft_grad + miclip_ft_adam,
           `LastBlockTrainer.step`: the code path without the cache) and of the cached step
           (`step_rows`: miclip_ft_grad_rows + miclip_ft_adam on a shuffled batch of the
           cache), alternating round by round; the ratio uncached / cached.
  fill     ms of `fill_view` over `batches` batches (one view), and the cached bytes.
Times are device events around work that ends in a synchronise, after one untimed warm-up of
every path; medians over the rounds; one JSON line per record. Not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_finetune import timed  # noqa: E402


def bench(name, B, batches, rounds, steps):
    import miclip
    from miclip.finetune import LastBlockTrainer, TrunkCache, cache_order
    from miclip.weights import synthetic_images
    _, model, _ = miclip.load(name, device="cuda", compute_dtype="fp16")
    cfg = model.config
    g = torch.Generator().manual_seed(0)
    C = 20
    tw = F.normalize(torch.randn(cfg.embed_dim, C, generator=g), dim=0).cuda()
    loader = [(torch.from_numpy(synthetic_images(B, cfg.image_resolution, seed=3 + b)).cuda().half(),
               torch.randint(0, C, (B,), generator=g)) for b in range(batches)]
    imgs, labels = loader[0][0], loader[0][1].cuda()
    tr = LastBlockTrainer(model, tw, unlocked_groups=2, lr=1e-5, epochs=10)

    fill = lambda: tr.fill_view(TrunkCache(), loader)
    fill()
    torch.cuda.synchronize()
    fill_ms = [timed(fill, 1) for _ in range(rounds)]
    cache = TrunkCache()
    tr.fill_view(cache, loader)
    n = cache.n[0]

    check = tr._labels
    tr._labels = lambda t, b: labels              # no host range check inside the timed loop
    order = cache_order(n, 1, 0)
    lab = cache.targets[0][order.cuda()]
    turn = [0]

    def cached():
        lo = (turn[0] % batches) * B
        turn[0] += 1
        tr.step_rows(cache, 0, order[lo:lo + B], lab[lo:lo + B])
    plain = lambda: tr.step(imgs, labels)
    plain(); cached()
    torch.cuda.synchronize()
    p_ms, c_ms = [], []
    for _ in range(rounds):
        p_ms.append(timed(plain, steps))
        c_ms.append(timed(cached, steps))
    tr._labels = check
    rec = {"record": "trunk_cache", "model": name, "batch": B, "dtype": "fp16", "groups": 2,
           "cached_images": n, "views": 1, "cached_bytes": cache.nbytes,
           "bytes_per_image": cache.nbytes // n, "fill_ms_per_view": statistics.median(fill_ms),
           "fill_ms_all": fill_ms, "uncached_step_ms": statistics.median(p_ms),
           "cached_step_ms": statistics.median(c_ms), "uncached_step_ms_all": p_ms,
           "cached_step_ms_all": c_ms}
    rec["uncached_over_cached"] = rec["uncached_step_ms"] / rec["cached_step_ms"]
    rec["fill_over_uncached_epoch"] = rec["fill_ms_per_view"] / (batches * rec["uncached_step_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--model", default="ViT-L/14")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune",
                                                  "bench_finetune_cache.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune_cache needs a HIP device (no CPU fallback)")
    props = torch.cuda.get_device_properties(0)
    head = {"record": "device", "name": props.name, "rounds": a.rounds, "steps": a.steps}
    lines = [json.dumps(head)]
    print(lines[-1], flush=True)
    lines.append(json.dumps(bench(a.model, a.batch, a.batches, a.rounds, a.steps)))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
