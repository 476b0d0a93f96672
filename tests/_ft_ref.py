"""Torch (CPU) restatement of what miclip/finetune.py trains: the head of the image
tower behind the frozen trunk, for unlocked_groups = 1 (visual.proj).

    z = y @ P,  f = z / max(|z|, 1e-12),  logits = 100 f @ W,  loss = mean CE

The dtype is a parameter: float64 is the yardstick. `autocast_run` evaluates the same
step the way the reference does (fp32 masters under torch.autocast, no GradScaler) and
gives the reference's own error e_ref. The model-level reference is
oracle/clip_oracle.py's encode_image followed by `features`.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23
SCALE = 100.0


def features(y, P):
    return F.normalize(y @ P, dim=-1)


def head_logits(y, P, W):
    return SCALE * features(y, P) @ W


def autograd_run(y, P, W, labels, dtype=torch.float64):
    """(mean CE, correct count, dP) by autograd in `dtype`."""
    y, W = torch.as_tensor(y).to(dtype), torch.as_tensor(W).to(dtype)
    P = torch.as_tensor(P).to(dtype).clone().requires_grad_(True)
    labels = torch.as_tensor(labels).long()
    logits = head_logits(y, P, W)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    correct = int((logits.argmax(dim=1) == labels).sum())
    return float(loss.detach()), correct, P.grad.detach().clone()


def autocast_run(y, P, W, labels, half):
    """The same step with fp32 masters under torch.autocast('cpu', dtype=half):
    (mean CE, dP as fp32), the reference's own rounding."""
    y, W = torch.as_tensor(y).float(), torch.as_tensor(W).float()
    P = torch.as_tensor(P).float().clone().requires_grad_(True)
    labels = torch.as_tensor(labels).long()
    with torch.autocast("cpu", dtype=half):
        loss = F.cross_entropy(head_logits(y, P, W), labels)
    loss.backward()
    return float(loss.detach()), P.grad.detach().float().clone()


def closed_form(y, P, W, labels):
    """dZ = d(mean CE)/d(y @ P) and dP = y^T dZ written out (the identities the
    kernels use), in the inputs' dtype."""
    n = y.shape[0]
    z = y @ P
    nrm = z.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    f = z / nrm
    logits = SCALE * f @ W
    gm = torch.softmax(logits, dim=-1)
    gm[torch.arange(n), labels] -= 1.0
    gm = gm / n
    dF = SCALE * gm @ W.t()
    dZ = (dF - f * (f * dF).sum(-1, keepdim=True)) / nrm
    return dZ, y.t() @ dZ


def rel_fro(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def cosine_factor(epoch, epochs):
    return 0.5 * (1.0 + math.cos(math.pi * epoch / epochs))


def adam_fp64(p, grads, lr, eps=1e-8):
    """torch.optim.Adam's rule in float64 over a list of per-step gradients: the
    parameter after each step."""
    p = np.asarray(p, dtype=np.float64).copy()
    m, v, out = np.zeros_like(p), np.zeros_like(p), []
    for t, g in enumerate(grads, start=1):
        g = np.asarray(g, dtype=np.float64)
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        denom = np.sqrt(v) / math.sqrt(1 - 0.999 ** t) + eps
        p = p - (lr / (1 - 0.9 ** t)) * (m / denom)
        out.append(p.copy())
    return out


def head_case(B, W, E, C, seed):
    """Seeded inputs of one op-level case: y [B, W] (ln_post-like rows), P [W, E],
    text weights [E, C] with unit columns, labels [B]."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, W, generator=g)
    P = torch.randn(W, E, generator=g) * W ** -0.5
    Wt = F.normalize(torch.randn(E, C, generator=g), dim=0)
    labels = torch.randint(0, C, (B,), generator=g)
    return y, P, Wt, labels


def trajectory(y, P, W, labels, lr, steps, mode):
    """Per-step mean CE (before each update) of `steps` Adam steps on one fixed batch.
    mode: torch.float64 (yardstick) or torch.float16 / bfloat16 (fp32 masters under
    autocast, the reference's run)."""
    half = mode if mode in (torch.float16, torch.bfloat16) else None
    dt = torch.float32 if half else mode
    y, W = y.to(dt), W.to(dt)
    p = P.to(dt).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        if half:
            with torch.autocast("cpu", dtype=half):
                loss = F.cross_entropy(head_logits(y, p, W), labels)
        else:
            loss = F.cross_entropy(head_logits(y, p, W), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


# ---- group 2: the last block on the CLS query, ln_post, proj ----
TAIL_NAMES = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias",
              "attn.out_proj.weight", "attn.out_proj.bias", "ln_2.weight", "ln_2.bias",
              "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias",
              "ln_post.weight", "ln_post.bias", "proj")


def _act(name):
    return F.gelu if name == "erf" else (lambda t: t * torch.sigmoid(1.702 * t))


def tail_features(x, p, heads, act):
    """ln_post of the CLS row of the last block (clip/model.py:183-186, 226-229) for the
    residual stream x [B, N, W] and the 15 tensors p (TAIL_NAMES order): only the CLS query
    is attended, everything after the attention runs on [B, W]."""
    B, N, W = x.shape
    dh = W // heads
    h = F.layer_norm(x, (W,), p[0], p[1], 1e-5)
    qkv = F.linear(h, p[2], p[3])
    q, k, v = qkv.split(W, dim=-1)
    q = q[:, :1].reshape(B, 1, heads, dh).transpose(1, 2)
    k = k.reshape(B, N, heads, dh).transpose(1, 2)
    v = v.reshape(B, N, heads, dh).transpose(1, 2)
    att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    o = (att @ v).transpose(1, 2).reshape(B, W)
    x1 = x[:, 0] + F.linear(o, p[4], p[5])
    h2 = F.layer_norm(x1, (W,), p[6], p[7], 1e-5)
    x2 = x1 + F.linear(_act(act)(F.linear(h2, p[8], p[9])), p[10], p[11])
    return F.layer_norm(x2, (W,), p[12], p[13], 1e-5)


def tail_case(B, N, W, E, C, seed):
    """Seeded x [B, N, W] (values exact in fp16), the 15 parameter tensors, text weights
    [E, C] with unit columns, labels [B]."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(B, N, W).half().float()
    ln = lambda: [1.0 + 0.1 * rn(W), 0.1 * rn(W)]
    lin = lambda o, i: [rn(o, i) * i ** -0.5, 0.02 * rn(o)]
    p = ln() + lin(3 * W, W) + lin(W, W) + ln() + lin(4 * W, W) + lin(W, 4 * W) + ln() + \
        [rn(W, E) * W ** -0.5]
    Wt = F.normalize(rn(E, C), dim=0)
    labels = torch.randint(0, C, (B,), generator=g)
    return x, p, Wt, labels


def tail_run(x, p, Wt, labels, heads, act, mode):
    """(mean CE, correct count, [15 gradients], y) by autograd: mode torch.float64 is the
    yardstick, torch.float16 / bfloat16 run fp32 masters under autocast (the reference)."""
    half = mode if mode in (torch.float16, torch.bfloat16) else None
    dt = torch.float32 if half else mode
    x, Wt = x.to(dt), Wt.to(dt)
    ps = [t.to(dt).clone().requires_grad_(True) for t in p]

    def fwd():
        y = tail_features(x, ps, heads, act)
        return y, head_logits(y, ps[14], Wt)
    if half:
        with torch.autocast("cpu", dtype=half):
            y, logits = fwd()
            loss = F.cross_entropy(logits, labels)
    else:
        y, logits = fwd()
        loss = F.cross_entropy(logits, labels)
    loss.backward()
    correct = int((logits.argmax(dim=1) == labels).sum())
    return float(loss.detach()), correct, [t.grad.detach().float() if half else t.grad.detach()
                                           for t in ps], y.detach()


def tail_loss_cast_at_gemm(x, p, Wt, labels, heads, act, half):
    """Mean CE of the tail evaluated in float64 with every GEMM / attention operand
    rounded once to `half` (activations and weights) and nothing else rounded: the
    explicit cast-at-GEMM restatement, an evaluation that rounds in other places than
    autocast does. The head (proj, normalise, logits) stays unrounded."""
    r = lambda t: t.to(half).double()
    x = x.double()
    p = [t.double() for t in p]
    B, N, W = x.shape
    dh = W // heads
    h = r(F.layer_norm(x, (W,), p[0], p[1], 1e-5))
    qkv = r(F.linear(h, r(p[2]), p[3]))
    q, k, v = qkv.split(W, dim=-1)
    q = q[:, :1].reshape(B, 1, heads, dh).transpose(1, 2)
    k = k.reshape(B, N, heads, dh).transpose(1, 2)
    v = v.reshape(B, N, heads, dh).transpose(1, 2)
    att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    o = r((att @ v).transpose(1, 2).reshape(B, W))
    x1 = x[:, 0] + F.linear(o, r(p[4]), p[5])
    h2 = r(F.layer_norm(x1, (W,), p[6], p[7], 1e-5))
    a = r(_act(act)(F.linear(h2, r(p[8]), p[9])))
    x2 = x1 + F.linear(a, r(p[10]), p[11])
    y = F.layer_norm(x2, (W,), p[12], p[13], 1e-5)
    return float(F.cross_entropy(head_logits(y, p[14], Wt.double()), labels))


def tail_trajectory(x, p, Wt, labels, heads, act, lr, steps, mode):
    """Per-step mean CE (before each update) of `steps` Adam steps over all 15 tensors on
    one fixed batch; mode as in tail_run."""
    half = mode if mode in (torch.float16, torch.bfloat16) else None
    dt = torch.float32 if half else mode
    x, Wt = x.to(dt), Wt.to(dt)
    ps = [t.to(dt).clone().requires_grad_(True) for t in p]
    opt = torch.optim.Adam(ps, lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        if half:
            with torch.autocast("cpu", dtype=half):
                loss = F.cross_entropy(head_logits(tail_features(x, ps, heads, act), ps[14], Wt),
                                       labels)
        else:
            loss = F.cross_entropy(head_logits(tail_features(x, ps, heads, act), ps[14], Wt),
                                   labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses
