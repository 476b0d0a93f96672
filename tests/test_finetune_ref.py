"""CPU: the mathematics and the host-side contract of miclip/finetune.py.

  * the restated head equals oracle/clip_oracle.py's encode_image -> @ proj -> normalise;
  * the closed-form dZ / dP identities equal fp64 autograd (relative 1e-12);
  * trainable_names for groups 1 and 2, and the errors for 0, 3 and tune_text;
  * the cosine factor against torch's CosineAnnealingLR;
  * FTOpenCLIP's config validation against a stub model (no device).
"""
import math

import numpy as np
import pytest
import torch

import _ft_ref as R


class _Stub(torch.nn.Module):
    """Parameter names of a 3-layer image tower plus a text block, no device."""
    compute_dtype = "fp16"
    surface = "open_clip"

    def __init__(self, layers=3):
        super().__init__()
        from miclip.finetune import _BLOCK_TENSORS
        names = ["visual.class_embedding", "visual.conv1.weight", "visual.ln_pre.weight",
                 "visual.ln_pre.bias"]
        for l in range(layers):
            names += [f"visual.transformer.resblocks.{l}.{t}" for t in _BLOCK_TENSORS]
        names += ["visual.ln_post.weight", "visual.ln_post.bias", "visual.proj",
                  "transformer.resblocks.0.ln_1.weight", "text_projection", "logit_scale"]
        self._names = names
        self._p = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(1)) for _ in names])

    def named_parameters(self, *a, **k):
        return iter(zip(self._names, self._p))


def test_head_matches_the_oracle_on_the_cls_row():
    from miclip.configs import CLIPConfig
    from miclip.weights import generate_state_dict, synthetic_images
    from oracle import clip_oracle
    cfg = CLIPConfig(embed_dim=64, image_resolution=64, vision_layers=2, vision_width=256,
                     vision_patch_size=32, context_length=77, vocab_size=49408,
                     transformer_width=256, transformer_heads=4, transformer_layers=1)
    sd = generate_state_dict(cfg, seed=0)
    imgs = synthetic_images(3, 64, seed=5)
    y = torch.as_tensor(clip_oracle.encode_image(sd, cfg, imgs)).double()
    P = torch.as_tensor(sd["visual.proj"]).double()
    f = R.features(y, P)
    want = (y @ P) / (y @ P).norm(dim=-1, keepdim=True)
    assert y.shape == (3, 256) and f.shape == (3, 64)
    assert float((f - want).abs().max()) <= 1e-15
    assert float((f.norm(dim=-1) - 1).abs().max()) <= 1e-14


@pytest.mark.parametrize("shape", [(3, 256, 64, 5), (1, 256, 16, 3), (33, 256, 64, 20),
                                   (2, 640, 128, 20)])
def test_closed_form_equals_fp64_autograd(shape):
    y, P, W, labels = R.head_case(*shape, seed=3)
    y, P, W = y.double(), P.double(), W.double()
    _, _, dP = R.autograd_run(y, P, W, labels)
    dZ, dP_cf = R.closed_form(y, P, W, labels)
    assert R.rel_fro(dP_cf, dP) <= 1e-12
    # dZ is orthogonal to f row by row (the normalise's null direction)
    f = R.features(y, P)
    assert float(((dZ * f).sum(-1)).abs().max()) <= 1e-12 * float(dZ.abs().max() + 1)


def test_trainable_names_groups():
    from miclip.finetune import _BLOCK_TENSORS, trainable_names
    m = _Stub(3)
    assert trainable_names(m, 1) == ["visual.proj"]
    g2 = trainable_names(m, 2)
    assert g2 == [f"visual.transformer.resblocks.2.{t}" for t in _BLOCK_TENSORS] + \
        ["visual.ln_post.weight", "visual.ln_post.bias", "visual.proj"]
    assert len(g2) == 15 and not any(".resblocks.1." in n for n in g2)


def test_trainable_names_errors():
    from miclip.finetune import trainable_names
    m = _Stub(3)
    with pytest.raises(ValueError, match="empty parameter list"):
        trainable_names(m, 0)
    with pytest.raises(NotImplementedError, match=r"resblocks\.1"):
        trainable_names(m, 3)
    with pytest.raises(NotImplementedError, match="tune_text"):
        trainable_names(m, 1, tune_text=True)
    # the message torch itself gives
    with pytest.raises(ValueError, match="empty parameter list"):
        torch.optim.Adam([])


def test_cosine_factor_is_cosine_annealing():
    from miclip.finetune import cosine_factor
    T, lr0 = 7, 3e-4
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T)
    for e in range(T + 1):
        assert cosine_factor(e, T) == R.cosine_factor(e, T)
        assert math.isclose(opt.param_groups[0]["lr"], lr0 * cosine_factor(e, T),
                            rel_tol=1e-12, abs_tol=1e-20)
        opt.step()
        sched.step()
    assert cosine_factor(0, T) == 1.0 and abs(cosine_factor(T, T)) < 1e-16


def test_config_validation_on_a_stub_model():
    from miclip.finetune import FTOpenCLIP, validate_config
    m = _Stub(3)
    ok = {"lr_v": 1e-4, "train_epoch": 2, "finetune": {"unlocked_groups": 1, "val_interval": 1}}
    assert validate_config(ok, m) == (1, False, 1e-4, 2, 1)
    assert validate_config({"lr_v": 1e-4, "train_epoch": 1, "finetune": {}}, m)[0] == 1
    with pytest.raises(KeyError):
        validate_config({"lr_v": 1e-4, "train_epoch": 2}, m)
    with pytest.raises(KeyError):
        validate_config({"train_epoch": 2, "finetune": {}}, m)
    bad = lambda **ft: {"lr_v": 1e-4, "train_epoch": 2, "finetune": ft}
    with pytest.raises(ValueError):
        validate_config(bad(unlocked_groups=0), m)
    with pytest.raises(NotImplementedError):
        validate_config(bad(unlocked_groups=3), m)
    assert validate_config(bad(unlocked_groups=2), m)[0] == 2
    with pytest.raises(NotImplementedError):
        validate_config(bad(tune_text=True), m)
    with pytest.raises(ValueError):
        validate_config({"lr_v": 1e-4, "train_epoch": 0, "finetune": {}}, m)
    # the method object refuses the same settings before it touches a device
    with pytest.raises(NotImplementedError):
        FTOpenCLIP(bad(tune_text=True))(None, None, None, torch.zeros(64, 5), m, ["a"] * 5, 0,
                                        "cfg", False)


def test_adam_restatement_matches_torch_in_float64():
    rng = np.random.default_rng(0)
    p0 = rng.standard_normal(63)
    grads = [rng.standard_normal(63) * 10.0 ** -k for k in range(3)]
    want = R.adam_fp64(p0, grads, lr=1e-2)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=1e-2)
    for g, w in zip(grads, want):
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        assert np.abs(p.detach().numpy() - w).max() <= 1e-14


@pytest.mark.parametrize("act,heads", [("quick", 4), ("erf", 2)])
def test_tail_restatement_equals_the_oracle_block(act, heads):
    """tail_features == ln_post(residual_block(x)[CLS]) of oracle/clip_oracle.py."""
    from oracle import clip_oracle
    B, N, W = 3, 7, 256
    x, p, _, _ = R.tail_case(B, N, W, 64, 5, seed=11)
    pre = "visual.transformer.resblocks.1."
    sd = {pre + n: t for n, t in zip(R.TAIL_NAMES[:12], p[:12])}
    full = clip_oracle.residual_block(x.permute(1, 0, 2), sd, pre, heads, act=act)  # LND
    want = clip_oracle.layer_norm(full.permute(1, 0, 2)[:, 0, :], p[12], p[13])
    got = R.tail_features(x, p, heads, act)
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())
    want64 = R.tail_features(x.double(), [t.double() for t in p], heads, act)
    assert float((got.double() - want64).abs().max()) <= 2e-5 * float(want64.abs().max())


def test_tail_closed_forms_equal_fp64_autograd():
    """dW_in = G * gamma + db (x) beta, d b_in = db, dgamma1 = sum_n W_in G, dbeta1 = sum_n
    W_in db with G = dQKV^T xhat over all rows, and the CLS-query attention backward."""
    B, N, W, heads = 2, 5, 256, 4
    dh = W // heads
    x, p, Wt, labels = R.tail_case(B, N, W, 64, 5, seed=12)
    x, Wt = x.double(), Wt.double()
    p = [t.double() for t in p]
    _, _, grads, _ = R.tail_run(x, p, Wt, labels, heads, "quick", torch.float64)
    # dQKV by autograd with qkv as the leaf
    xhat = torch.nn.functional.layer_norm(x, (W,))
    h = xhat * p[0] + p[1]
    qkv = torch.nn.functional.linear(h, p[2], p[3]).detach().requires_grad_(True)
    q, k, v = qkv.split(W, dim=-1)
    qh = q[:, :1].reshape(B, 1, heads, dh).transpose(1, 2)
    kh = k.reshape(B, N, heads, dh).transpose(1, 2)
    vh = v.reshape(B, N, heads, dh).transpose(1, 2)
    att = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    o = (att @ vh).transpose(1, 2).reshape(B, W)
    x1 = x[:, 0] + torch.nn.functional.linear(o, p[4], p[5])
    h2 = torch.nn.functional.layer_norm(x1, (W,), p[6], p[7], 1e-5)
    u = torch.nn.functional.linear(h2, p[8], p[9])
    x2 = x1 + torch.nn.functional.linear(u * torch.sigmoid(1.702 * u), p[10], p[11])
    y = torch.nn.functional.layer_norm(x2, (W,), p[12], p[13], 1e-5)
    loss = torch.nn.functional.cross_entropy(R.head_logits(y, p[14], Wt), labels)
    o.retain_grad()
    loss.backward()
    dqkv = qkv.grad.reshape(B * N, 3 * W)
    assert float(dqkv.reshape(B, N, 3 * W)[:, 1:, :W].abs().max()) == 0.0   # dQ: CLS rows only
    G = dqkv.t() @ xhat.reshape(B * N, W)
    db = dqkv.sum(0)
    rel = lambda a, b: R.rel_fro(a, b)
    assert rel(G * p[0][None, :] + db[:, None] * p[1][None, :], grads[2]) <= 1e-12
    assert rel(db, grads[3]) <= 1e-12
    assert rel((p[2] * G).sum(0), grads[0]) <= 1e-12
    assert rel((p[2] * db[:, None]).sum(0), grads[1]) <= 1e-12
    # attention backward per (image, head)
    dO = o.grad.reshape(B, heads, dh)
    pr = att[:, :, 0, :].detach()                                   # [B, H, N]
    dP = torch.einsum("bhd,bhnd->bhn", dO, vh.detach())
    dS = pr * (dP - (pr * dP).sum(-1, keepdim=True))
    dV = pr[..., None] * dO[:, :, None, :]
    dK = dS[..., None] * qh.detach() / math.sqrt(dh)
    dq = torch.einsum("bhn,bhnd->bhd", dS, kh.detach()) / math.sqrt(dh)
    pack = lambda t: t.transpose(1, 2).reshape(B, N, W)
    g3 = qkv.grad
    assert rel(pack(dK), g3[:, :, W:2 * W]) <= 1e-12
    assert rel(pack(dV), g3[:, :, 2 * W:]) <= 1e-12
    assert rel(dq.reshape(B, W), g3[:, 0, :W]) <= 1e-12
