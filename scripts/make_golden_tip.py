#!/usr/bin/env python3
"""Regenerate tests/golden/tip.npz from a checkout of the reference project.

    python scripts/make_golden_tip.py /path/to/reference [--out tests/golden/tip.npz]

Imports the reference's `methods/utils.py` by path and runs its own `search_hp_tip` on
the CPU in fp32 (it has no `.cuda()` call) on two small cases. Recorded: the inputs, the
returned (best_beta, best_alpha) and the accuracy of every pair, taken from the
reference's own `cls_acc` calls (the module attribute is wrapped by a recorder; its
arithmetic is untouched). `build_cache_model` calls `.cuda()` and is not run: the keys
are inputs here. The seed of a case is advanced until every top-2 logit margin of the
grid is >= 1e-3, so float64 and fp32 agree on every prediction. The file is written with
fixed zip timestamps: running the script twice gives the same bytes. Developer tool: no
test and no GPU job runs it.

Cases:
  a  Nq 40, Nk 30, E 32, C 5,  search_scale [7, 3],   search_step [6, 4]
  b  Nq 64, Nk 48, E 48, C 8,  search_scale [5.5, 2], search_step [5, 5]; class 7 owns no
     key (the one-hot width is still 8)
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

CASES = {"a": dict(Nq=40, Nk=30, E=32, C=5, scale=[7, 3], step=[6, 4], empty=None),
         "b": dict(Nq=64, Nk=48, E=48, C=8, scale=[5.5, 2], step=[5, 5], empty=7)}


def make_data(seed, Nq, Nk, E, C, empty):
    """Unit keys and queries around C random directions, text weights off the directions."""
    g = torch.Generator().manual_seed(seed)
    dirs = F.normalize(torch.randn(C, E, generator=g), dim=1)
    owners = [c for c in range(C) if c != empty]
    klab = torch.tensor([owners[k % len(owners)] for k in range(Nk)])
    qlab = torch.randint(0, C, (Nq,), generator=g)

    def around(lab, amount):
        return F.normalize(dirs[lab] + amount * E ** -0.5 * torch.randn(len(lab), E, generator=g),
                           dim=1)

    return around(qlab, 1.0), around(klab, 1.0), around(torch.arange(C), 0.9).t().contiguous(), \
        klab, qlab


def write_npz(path, arrays):
    """np.savez's layout with a fixed timestamp and no compression."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tests", "golden", "tip.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        "reference_methods_utils", os.path.join(args.reference, "methods", "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.set_num_threads(1)

    accs = []
    inner = ref.cls_acc

    def recording_cls_acc(output, target, topk=1):
        acc = inner(output, target, topk)
        accs.append(acc)
        return acc

    ref.cls_acc = recording_cls_acc
    out, meta = {}, {}
    for tag, c in CASES.items():
        for seed in range(100, 200):
            Fq, K, W, klab, qlab = make_data(seed, c["Nq"], c["Nk"], c["E"], c["C"], c["empty"])
            values = F.one_hot(klab, c["C"]).half()
            cfg = {"search_hp": True, "search_scale": c["scale"], "search_step": c["step"]}
            betas = [i * (c["scale"][0] - 0.1) / c["step"][0] + 0.1 for i in range(c["step"][0])]
            alphas = [i * (c["scale"][1] - 0.1) / c["step"][1] + 0.1 for i in range(c["step"][1])]
            margin = np.inf
            aff, zero_shot = Fq.double() @ K.double().t(), 100.0 * Fq.double() @ W.double()
            for beta in betas:
                sums = torch.exp(beta * (aff - 1.0)) @ values.double()
                for alpha in alphas:
                    top = (zero_shot + alpha * sums).topk(2, dim=1).values
                    margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
            if margin < 1e-3:
                continue
            del accs[:]
            with contextlib.redirect_stdout(io.StringIO()):
                # cache_values in fp32: the reference's half() values cannot meet fp32
                # features in a CPU matmul; one-hot entries are exact in either type
                best = ref.search_hp_tip(cfg, K.t().contiguous(), values.float(), Fq, qlab, W)
            grid = np.array(accs, dtype=np.float64).reshape(len(betas), len(alphas))
            if len(set(accs)) > 2:
                break
        else:
            raise SystemExit(f"case {tag}: no seed with every margin >= 1e-3")
        out.update({f"{tag}_F": Fq.numpy(), f"{tag}_keys": K.numpy(), f"{tag}_W": W.numpy(),
                    f"{tag}_key_labels": klab.numpy(), f"{tag}_labels": qlab.numpy(),
                    f"{tag}_acc": grid, f"{tag}_best": np.array(best, dtype=np.float64)})
        meta[tag] = {"seed": seed, "scale": c["scale"], "step": c["step"], "C": c["C"],
                     "min_margin": margin}
        print(f"case {tag}: seed {seed}, best {best}, min margin {margin:.4g}, "
              f"accs {sorted(set(accs))}")
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    write_npz(args.out, out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
