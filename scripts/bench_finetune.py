#!/usr/bin/env python3
"""Time last-block fine-tuning (miclip.finetune) on one device.

    python scripts/bench_finetune.py [--rounds 3] [--steps 5] [--configs ...] [--out FILE]

Per config (model, batch; fp16, seeded weights and images), in one process:
  step     images/s of a group-2 training step (trunk + miclip_ft_grad + miclip_ft_adam)
           and of `encode_image` on the same batch, alternating round by round; the
           ratio step / encode. encode_image is the unchanged yardstick.
  parts    hipEvent times of one step's parts: trunk, tail (forward + backward), adam.
  torch    the same step written as the reference runs it: oracle/clip_oracle.py's
           residual_block + ln_post on the device under torch.autocast with autograd
           through the last block and torch.optim.Adam, on the same trunk output.
And once: TFLOP/s of miclip_op_gemm_tn at (65792, 2048, 1024) beside miclip_op_gemm at the
same FLOP count (M 65792, N 2048, K 1024).
Times are device events around work that ends in a synchronise, after one untimed warm-up
of every path; medians over the rounds; one JSON line per record. Not part of bench.py.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aihab-clip_amd"))
sys.path.insert(0, ROOT)

CONFIGS = {"ViT-L/14": 256, "ViT-B/32": 256, "ViT-H-14": 128}


def timed(fn, reps):
    """Median-free helper: milliseconds of `reps` calls of fn between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def torch_step_factory(model, trainer, tw, labels):
    """The reference-style step on the trunk output: autograd through the last block."""
    from oracle import clip_oracle
    cfg = model.config
    pre = f"visual.transformer.resblocks.{cfg.vision_layers - 1}."
    sd = {n: torch.nn.Parameter(p.detach().clone()) for n, p in model.named_parameters()
          if n in trainer.tensors}
    opt = torch.optim.Adam(list(sd.values()), lr=1e-5)
    N, W = trainer.N, trainer.W

    def step(x):
        xs = x.view(-1, N, W).float().permute(1, 0, 2)
        with torch.autocast("cuda", dtype=torch.float16):
            h = clip_oracle.residual_block(xs, sd, pre, cfg.vision_heads, act=cfg.act)
            y = clip_oracle.layer_norm(h[0], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"])
            f = F.normalize(y @ sd["visual.proj"], dim=-1)
            loss = F.cross_entropy(100.0 * f @ tw, labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def bench_model(name, B, rounds, steps):
    import miclip
    from miclip.finetune import LastBlockTrainer
    from miclip.weights import synthetic_images
    _, model, _ = miclip.load(name, device="cuda", compute_dtype="fp16")
    cfg = model.config
    imgs = torch.from_numpy(synthetic_images(B, cfg.image_resolution, seed=3)).cuda().half()
    g = torch.Generator().manual_seed(0)
    C = 20
    tw = F.normalize(torch.randn(cfg.embed_dim, C, generator=g), dim=0).cuda()
    labels = torch.randint(0, C, (B,), generator=g).cuda()
    tr = LastBlockTrainer(model, tw, unlocked_groups=2, lr=1e-5, epochs=10)
    labels_dev = labels.to(torch.int64)
    tr._labels = lambda t, b: labels_dev          # no host range check inside the timed loop
    out = torch.empty(B, model.image_dim, device="cuda")
    enc = lambda: model.encode_image(imgs, out=out)
    step = lambda: tr.step(imgs, labels)
    enc(); step()
    torch.cuda.synchronize()
    e_ms, s_ms = [], []
    for _ in range(rounds):
        e_ms.append(timed(enc, steps))
        s_ms.append(timed(step, steps))
    x = tr.trunk(imgs)
    parts = {"trunk": lambda: tr.trunk(imgs), "tail": lambda: tr.grad(x, labels), "adam": tr.adam}
    part_ms = {k: statistics.median(timed(f, steps) for _ in range(rounds)) for k, f in parts.items()}
    rec = {"record": "step", "model": name, "batch": B, "dtype": "fp16", "groups": 2,
           "encode_ms": statistics.median(e_ms), "step_ms": statistics.median(s_ms),
           "encode_ms_all": e_ms, "step_ms_all": s_ms, "parts_ms": part_ms}
    rec["encode_img_s"] = B / rec["encode_ms"] * 1e3
    rec["step_img_s"] = B / rec["step_ms"] * 1e3
    rec["step_over_encode"] = rec["step_ms"] / rec["encode_ms"]
    try:
        tstep = torch_step_factory(model, tr, tw, labels)
        tstep(x)
        torch.cuda.synchronize()
        t_ms = [timed(lambda: tstep(x), steps) for _ in range(rounds)]
        rec["torch_tail_ms"] = statistics.median(t_ms)
        rec["torch_tail_over_tail"] = rec["torch_tail_ms"] / (part_ms["tail"] + part_ms["adam"])
    except Exception as exc:                       # the baseline is optional; say why it is absent
        rec["torch_tail_error"] = f"{type(exc).__name__}: {exc}"[:200]
    del tr, model
    torch.cuda.empty_cache()
    return rec


def bench_gemm(rounds, reps):
    from miclip import _lib
    lib = _lib.load_library()
    M, Nn, K = 65792, 2048, 1024
    g = torch.Generator().manual_seed(1)
    A = torch.randn(M, Nn, generator=g).half().cuda()
    X = torch.randn(M, K, generator=g).half().cuda()
    G = torch.empty(Nn, K, device="cuda")
    ws = torch.empty(lib.miclip_gemm_tn_ws_bytes(M, Nn, K), device="cuda", dtype=torch.uint8)
    st = _lib.stream_handle(torch.device("cuda"))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    tn = lambda: _lib.check(lib.miclip_op_gemm_tn(0, p(A), p(X), p(G), M, Nn, K, p(ws), st))
    # NT GEMM of the same FLOP count: C [M, 2048] = A2 [M, 1024] . W2 [2048, 1024]^T
    Wn = torch.randn(Nn, K, generator=g).half().cuda()
    Cn = torch.empty(M, Nn, device="cuda", dtype=torch.float16)
    nt = lambda: _lib.check(lib.miclip_op_gemm(0, p(X), p(Wn), None, p(Cn), M, Nn, K, 0, 0, 0, st))
    tn(); nt()
    torch.cuda.synchronize()
    flop = 2.0 * M * Nn * K
    tn_ms = [timed(tn, reps) for _ in range(rounds)]
    nt_ms = [timed(nt, reps) for _ in range(rounds)]
    return {"record": "gemm_tn", "shape": [M, Nn, K], "dtype": "fp16",
            "tn_ms": statistics.median(tn_ms), "nt_ms": statistics.median(nt_ms),
            "tn_tflops": flop / statistics.median(tn_ms) / 1e9,
            "nt_tflops": flop / statistics.median(nt_ms) / 1e9, "tn_ms_all": tn_ms,
            "nt_ms_all": nt_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune",
                                                  "bench_finetune.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune needs a HIP device (no CPU fallback)")
    props = torch.cuda.get_device_properties(0)
    head = {"record": "device", "name": props.name, "clock_mhz": getattr(props, "clock_rate", 0) / 1e3,
            "rounds": a.rounds, "steps": a.steps}
    lines = [json.dumps(head)]
    print(lines[-1], flush=True)
    lines.append(json.dumps(bench_gemm(a.rounds, 5)))
    print(lines[-1], flush=True)
    for name in a.configs:
        lines.append(json.dumps(bench_model(name, CONFIGS[name], a.rounds, a.steps)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
