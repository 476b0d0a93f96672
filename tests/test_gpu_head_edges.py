"""GPU: edge cases of the head, top-k and text embed / EOT kernels (csrc/embed.hip:
head_proj_kernel, head_logits_kernel, topk_rows_kernel, token_embed_kernel, eot_kernel).

What is compared with what (the yardstick is tests/_head_ref.py, numpy float64):
  * logits of miclip_zero_shot against float64 on the same fp32 inputs, at every k-chunk
    count the wave split treats differently (nk = E / 16 = 1, 2, 3, 5, 17, 64) and at
    ragged row / class tiles; an all-zero feature row gives exact zeros;
  * a row's logits bit for bit whatever batch it runs in, and run to run;
  * the projection path (visual.proj loaded on the handle) against float64, across the
    regrow of the handle's scratch;
  * top-k exactly against a lexsort of the kernel's OWN logits (so no fp32-vs-fp64
    difference can flip a pick): planted bitwise ties, +-inf, NaN; torch.topk's order
    (NaN first, the lower index first among equals);
  * encode_text of a model with no text block (token_embed -> ln_final on the EOT rows
    -> text_projection) against its closed form, with repeated maxima placed on either
    side of the 64-lane boundary and on two passes of one lane.
Every caller-owned output has one canary row behind it, which must stay untouched.

Bars: 4 x the largest error measured on the MI355X over the cases of this file (every
test prints its figure before it asserts), never above the worst-case bound next to it.
  logits (apply_proj = 0), per E, cap scale * (E + 8) * 2^-24:
    E = 16: 1.55e-5   E = 32: 1.22e-5   E = 48: 1.43e-5   (caps 1.43e-4, 2.38e-4, 3.34e-4)
    E = 80: 1.64e-5   E = 272: 1.66e-5   E = 1024: 3.11e-5  (caps 5.25e-4, 1.67e-3, 6.15e-3)
  logits (apply_proj = 1), cap scale * (Din + E + 8) * 2^-24 >= 1.67e-3: 2.19e-5
  x_proj = x_before @ text_projection, relative to max |row| * max |column| (the unit of
    the bound, by Cauchy-Schwarz), cap (256 + 8) * 2^-24 = 1.57e-5: 3.87e-8
  x_before (ln_final): the fp32 LayerNorm bar of test_layernorm, 1e-4 (measured 4.1e-7
    on the fp16 stream, 5.8e-7 on the fp32 stream; a wrong position differs by > 1e-2).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _head_ref as R

gpu = pytest.mark.gpu
SCALE = 100.0
CANARY_F, CANARY_I = -7.0, -7

# largest |logit - fp64| measured on the MI355X over LOGIT_CASES and the zero-row cases, per E
MEASURED_LOGITS = {16: 1.55e-5, 32: 1.22e-5, 48: 1.43e-5, 80: 1.64e-5, 272: 1.66e-5, 1024: 3.11e-5}
MEASURED_PROJ = 2.19e-5         # over PROJ_CASES, both calls
MEASURED_XPROJ = 3.87e-8         # relative, over TEXT_CASES
LN_TOL = 1e-4                   # tests/test_gpu_kernels.py test_layernorm, fp32 out


def _bar(measured, cap):
    """4 x measured, never above the derived cap."""
    return min(4.0 * measured, cap)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ------------------------------------------------------------------ CPU: the yardstick itself
def test_reference_topk_matches_torch():
    R.selfcheck_topk()


def test_reference_text_eot_matches_torch():
    R.selfcheck_text()


def test_reference_head_and_scoring_match_torch():
    R.selfcheck_head_and_scoring()


# ------------------------------------------------------------------ a bare handle
class Head:
    """miclip_zero_shot on a bare handle whose embed_dim is E (with apply_proj = 0 the
    head reads nothing else of the model); `proj` [vision_width, E] is loaded as
    visual.proj for apply_proj = 1. The caller owns logits and topk: both get one canary
    row, checked after every call."""

    def __init__(self, E, vision_width=256, proj=None):
        from miclip import _lib
        self._lib, self.lib = _lib, _lib.load_library()
        cfg = _lib.MiclipConfig(embed_dim=E, image_resolution=32, vision_layers=1,
                                vision_width=vision_width, vision_patch_size=32,
                                context_length=8, vocab_size=16, transformer_width=256,
                                transformer_heads=4, transformer_layers=0,
                                compute_dtype=_lib.MICLIP_FP16, act=_lib.MICLIP_ACT_QUICKGELU,
                                vision_head_dim=64, options=0)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.miclip_model_create(ctypes.byref(cfg), 0, ctypes.byref(self.h)), "create")
        if proj is not None:
            a = np.ascontiguousarray(proj, dtype=np.float32)
            t = (_lib.MiclipTensor * 1)()
            t[0].name, t[0].data, t[0].numel = b"visual.proj", a.ctypes.data, a.size
            _lib.check(self.lib.miclip_model_load_weights(self.h, t, 1), "load visual.proj")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.miclip_model_destroy(self.h)

    def run(self, f, tw, k=0, apply_proj=0):
        """(logits [B, C] numpy, topk [B, k] numpy or None)."""
        fd = torch.as_tensor(f, dtype=torch.float32).cuda().contiguous()
        wd = torch.as_tensor(tw, dtype=torch.float32).cuda().contiguous()
        B, C = fd.shape[0], wd.shape[1]
        logits = torch.full((B + 1, C), CANARY_F, device="cuda")
        top = torch.full((B + 1, max(k, 1)), CANARY_I, device="cuda", dtype=torch.int32)
        self._lib.check(self.lib.miclip_zero_shot(
            self.h, fd.data_ptr(), B, apply_proj, wd.data_ptr(), C, SCALE, logits.data_ptr(),
            top.data_ptr() if k else None, k, self._lib.stream_handle()), "miclip_zero_shot")
        z, t = logits.cpu().numpy(), top.cpu().numpy()
        assert (z[B] == CANARY_F).all() and (t[B] == CANARY_I).all(), "canary row written"
        return z[:B], (t[:B] if k else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _head_inputs(B, E, C, seed):
    """(f [B, E], tw [E, C] unit-norm columns): f = 1.5 tw[:, y].T + noise with
    |noise| ~ 1.1, so the label's logit is 100 cos ~ 60 .. 90."""
    g = torch.Generator().manual_seed(seed)
    tw = torch.nn.functional.normalize(torch.randn(E, C, generator=g), dim=0)
    y = torch.randint(0, C, (B,), generator=g)
    f = 1.5 * tw[:, y].t() + (1.1 / E ** 0.5) * torch.randn(B, E, generator=g)
    return f.contiguous().numpy(), tw.contiguous().numpy(), y.numpy()


# ------------------------------------------------------------------ a. logits against fp64
# every E of {16, 32, 48, 80, 272, 1024}, B of {1, 15, 16, 17, 33}, C of {1, 15, 17, 65}
LOGIT_CASES = [(1, 16, 1), (17, 16, 65), (15, 32, 17), (33, 32, 15), (16, 48, 15), (17, 48, 1),
               (33, 80, 17), (1, 80, 65), (15, 272, 65), (16, 272, 17), (17, 1024, 15),
               (33, 1024, 65)]


@gpu
@pytest.mark.parametrize("B,E,C", LOGIT_CASES)
def test_logits_against_fp64(B, E, C):
    f, tw, y = _head_inputs(B, E, C, 1000 * B + 10 * E + C)
    want = R.logits(f, tw, SCALE)
    top = want[np.arange(B), y]
    assert 55.0 <= top.min() and top.max() <= 95.0, (top.min(), top.max())
    cap = R.logits_cap(SCALE, E)
    bar = _bar(MEASURED_LOGITS[E], cap)
    _need_gpu()
    with Head(E) as h:
        z, _ = h.run(f, tw)
    err = float(np.abs(z.astype(np.float64) - want).max())
    print(f"B={B} E={E} C={C}: max |logit - fp64| {err:.3g} (bar {bar:.3g}, cap {cap:.3g}), "
          f"label logits {top.min():.1f} .. {top.max():.1f}")
    assert bar <= cap and err <= bar


@gpu
@pytest.mark.parametrize("B,E,C,row", [(17, 48, 15, 16), (1, 16, 1, 0), (33, 80, 17, 5)])
def test_zero_feature_row_gives_zero_logits(B, E, C, row):
    """|f| = 0 takes the eps branch: 0 / 1e-12 = 0 exactly, never NaN."""
    _need_gpu()
    f, tw, _ = _head_inputs(B, E, C, 77 + B)
    f[row] = 0.0
    with Head(E) as h:
        z, _ = h.run(f, tw)
    keep = np.arange(B) != row
    err = float(np.abs(z[keep] - R.logits(f, tw, SCALE)[keep]).max()) if B > 1 else 0.0
    bar = _bar(MEASURED_LOGITS[E], R.logits_cap(SCALE, E))
    print(f"B={B} E={E} C={C}: zero row {row} -> max |logit| {np.abs(z[row]).max():.3g}; "
          f"the other rows: max |logit - fp64| {err:.3g} (bar {bar:.3g})")
    assert np.isfinite(z).all() and (z[row] == 0.0).all()
    assert err <= bar       # the other rows are untouched by it


# ------------------------------------------------------------------ b. batch invariance
@gpu
def test_logits_batch_invariant_and_deterministic():
    _need_gpu()
    B, E, C = 33, 80, 17
    f, tw, _ = _head_inputs(B, E, C, 5)
    with Head(E) as h:
        full, _ = h.run(f, tw)
        again, _ = h.run(f, tw)
        tail, _ = h.run(f[16:33], tw)
        rows = np.concatenate([h.run(f[r:r + 1], tw)[0] for r in range(B)])
    n_one = int((_bits(rows) != _bits(full)).sum())
    n_tail = int((_bits(tail) != _bits(full[16:33])).sum())
    n_again = int((_bits(again) != _bits(full)).sum())
    print(f"logits differing in bits: B=1 calls {n_one}, rows [16:33] {n_tail}, repeat {n_again}")
    assert n_one == 0 and n_tail == 0 and n_again == 0


# ------------------------------------------------------------------ c. projection path
PROJ_CASES = [(256, 16, 1), (256, 48, 17), (512, 16, 17), (512, 48, 1)]


@functools.lru_cache(maxsize=None)
def _visual_proj(Wv, E):
    """visual.proj [Wv, E] of the seeded tiny model (tests/test_preprocess.py _tiny_model)."""
    from miclip.configs import CLIPConfig
    from miclip.weights import generate_state_dict
    cfg = CLIPConfig(embed_dim=E, image_resolution=32, vision_layers=1, vision_width=Wv,
                     vision_patch_size=32, context_length=8, vocab_size=16,
                     transformer_width=256, transformer_heads=4, transformer_layers=1)
    return generate_state_dict(cfg, seed=0, towers=("visual",))["visual.proj"]


def _proj_inputs(B, Wv, E, C, seed):
    """x = (1.5 tw[:, y].T + noise) @ proj^T: proj^T proj ~ I (std Wv^-1/2, Wv >> E), so
    x @ proj lands near the features of _head_inputs."""
    g, tw, _ = _head_inputs(B, E, C, seed)
    return (g @ _visual_proj(Wv, E).T).astype(np.float32), tw


@gpu
@pytest.mark.parametrize("Wv,E,B", PROJ_CASES)
def test_projection_path_against_fp64_across_scratch_regrow(Wv, E, B):
    _need_gpu()
    C = 17
    proj = _visual_proj(Wv, E)
    x, tw = _proj_inputs(300, Wv, E, C, Wv + E)
    cap = R.logits_cap(SCALE, E, Wv)
    bar = _bar(MEASURED_PROJ, cap)
    with Head(E, Wv, proj) as h:
        first, _ = h.run(x[:B], tw, apply_proj=1)       # scratch: 256 rows
        big, _ = h.run(x, tw, apply_proj=1)             # 300 rows: the scratch regrows
        back, _ = h.run(x[:B], tw, apply_proj=1)
    want = R.logits(x, tw, SCALE, proj)
    e1 = float(np.abs(first - want[:B]).max())
    e2 = float(np.abs(big - want).max())
    print(f"Wv={Wv} E={E} B={B}: max |logit - fp64| {e1:.3g}, after the regrow (B=300) {e2:.3g} "
          f"(bar {bar:.3g}, cap {cap:.3g}); max |logit| {np.abs(want).max():.1f}")
    assert np.abs(want).max() >= 40.0
    assert bar <= cap and e1 <= bar and e2 <= bar
    assert np.array_equal(_bits(first), _bits(big[:B])) and np.array_equal(_bits(first), _bits(back))


@gpu
def test_projection_needs_visual_proj():
    _need_gpu()
    f, tw, _ = _head_inputs(2, 256, 3, 1)
    with Head(16) as h:
        with pytest.raises(Exception, match="visual.proj not loaded"):
            h.run(f, tw[:16], apply_proj=1)


# ------------------------------------------------------------------ d. top-k, exact
TOPK_E = 32


def _ks(C):
    return sorted({1, min(3, C), C})


def _pos_inputs(B, C, seed, planted=()):
    """All-positive f and tw (so a +-inf column gives +-inf logits, never NaN); row b
    leans on column planted[b % len(planted)], which makes the planted columns the top."""
    g = torch.Generator().manual_seed(seed)
    tw = torch.nn.functional.normalize(torch.rand(TOPK_E, C, generator=g) + 0.05, dim=0)
    cols = [planted[b % len(planted)] if planted else b % C for b in range(B)]
    f = 1.5 * tw[:, cols].t() + 0.1 * torch.rand(B, TOPK_E, generator=g)
    return f.contiguous().numpy(), tw.contiguous().numpy()


def _check_topk(h, f, tw, tag):
    C = tw.shape[1]
    out = None
    for k in _ks(C):
        z, t = h.run(f, tw, k=k)
        if out is None:
            out = z
        assert np.array_equal(_bits(z), _bits(out))      # the logits do not depend on k
        want = R.topk(z, k)
        ok_range = bool(((t >= 0) & (t < C)).all())
        distinct = all(len(set(row)) == k for row in t.tolist())
        print(f"{tag} C={C} k={k}: in range {ok_range}, distinct {distinct}, "
              f"rows differing from the lexsort {int((t != want).any(axis=1).sum())} of {len(t)}")
        assert ok_range and distinct
        assert np.array_equal(t, want), (tag, k, t[:4], want[:4])
    return out


@gpu
@pytest.mark.parametrize("C", [1, 15, 64, 65, 130])
def test_topk_planted_ties(C):
    """Duplicated tw columns give bit-equal logits: neighbours (c, c + 1), one lane on two
    passes (c, c + 64), first and last (0, C - 1). The lower index must come first."""
    _need_gpu()
    pairs = [(a, b) for a, b in ((3, 4), (5, 5 + 64), (0, C - 1)) if a < b < C]
    planted = sorted({c for p in pairs for c in p})
    f, tw = _pos_inputs(7, C, C, planted)
    for a, b in pairs:
        tw[:, b] = tw[:, a]
    with Head(TOPK_E) as h:
        z = _check_topk(h, f, tw, "ties")
        for a, b in pairs:      # the precondition: the planted logits are bit-equal
            assert np.array_equal(_bits(z[:, a]), _bits(z[:, b])), (a, b)
        # every column equal: every logit of a row ties, k = C must return 0 .. C-1
        tw[:] = tw[:, :1]
        z = _check_topk(h, f, tw, "all equal")
        assert (_bits(z) == _bits(z[:, :1])).all()
        _, t = h.run(f, tw, k=C)
        assert (t == np.arange(C)[None]).all()


@gpu
@pytest.mark.parametrize("C", [15, 64, 65, 130])
def test_topk_infinite_logits(C):
    _need_gpu()
    f, tw = _pos_inputs(5, C, 100 + C)
    hi, lo, lo2 = C - 1, 2, C // 2
    tw[:, hi], tw[:, lo], tw[:, lo2] = np.inf, -np.inf, -np.inf
    with Head(TOPK_E) as h:
        z = _check_topk(h, f, tw, "inf")
        assert (z[:, hi] == np.inf).all() and (z[:, lo] == -np.inf).all()
        assert np.isfinite(np.delete(z, [hi, lo, lo2], axis=1)).all()
        _, t = h.run(f, tw, k=C)
        assert (t[:, 0] == hi).all() and (t[:, -2] == lo).all() and (t[:, -1] == lo2).all()


@gpu
@pytest.mark.parametrize("C", [1, 15, 64, 65, 130])
def test_topk_nan_logits(C):
    """torch.topk's contract: NaN ranks above every number, the lower index first among
    NaNs; the k indices of a row are distinct and in [0, C) even where fewer than k
    logits are numbers (k = C here, and the all-NaN tw)."""
    _need_gpu()
    f, tw = _pos_inputs(5, C, 200 + C)
    nan_cols = sorted({c for c in (C - 1, 1, 1 + 64, 7) if 0 <= c < C})
    tw[:, nan_cols] = np.nan
    if C > 20:
        tw[:, 20] = np.inf
    with Head(TOPK_E) as h:
        z = _check_topk(h, f, tw, "nan")
        assert np.isnan(z[:, nan_cols]).all() and np.isnan(z).sum() == 5 * len(nan_cols)
        _, t = h.run(f, tw, k=C)
        assert (t[:, :len(nan_cols)] == np.asarray(nan_cols)[None]).all()
        tw[:] = np.nan
        z = _check_topk(h, f, tw, "all nan")
        assert np.isnan(z).all()


# ------------------------------------------------------------------ e. text embed and EOT
VOCAB, WT = 64, 256
# (context_length, embed_dim, resid_f32): every length and every embed_dim, both streams
TEXT_CASES = [(1, 1, False), (1, 15, True), (8, 15, False), (8, 17, True), (64, 17, False),
              (64, 40, True), (65, 40, False), (65, 1, True), (77, 1, False), (77, 15, True),
              (130, 17, False), (130, 40, True)]


def _placements(L):
    """Positions of the prompt's maximum id; the expected EOT is the first of them."""
    cand = [[0], [L - 1], [63, 64], [64, 65], [5, 70], list(range(L))]
    return [p for p in cand if max(p) < L]


def _prompts(L, placements, seed):
    rng = np.random.default_rng(seed)
    tok = rng.integers(0, VOCAB - 10, (len(placements), L)).astype(np.int64)
    for i, pl in enumerate(placements):
        tok[i, pl] = VOCAB - 1 if i % 2 == 0 else VOCAB - 5
    return tok


def _text_model(L, E, resid_f32):
    import miclip
    from miclip.configs import CLIPConfig
    from miclip.weights import generate_state_dict
    shape = dict(embed_dim=E, image_resolution=32, vision_layers=1, vision_width=256,
                 vision_patch_size=32, context_length=L, vocab_size=VOCAB, transformer_width=WT,
                 transformer_heads=4)
    # the generator draws every tensor from its own stream and needs >= 1 text block:
    # the 0-block model is the 1-block one without the block's tensors
    sd = generate_state_dict(CLIPConfig(transformer_layers=1, **shape), seed=0)
    sd = {k: v for k, v in sd.items() if not k.startswith("transformer.resblocks.")}
    cfg = CLIPConfig(transformer_layers=0, **shape)
    model = miclip.CLIP(cfg, {k: torch.from_numpy(v) for k, v in sd.items()}, device="cuda",
                        options={"resid_f32": True} if resid_f32 else None)
    return model, sd


def _encode_text(model, tok):
    """miclip_encode_text into caller-owned buffers with one canary row each."""
    from miclip import _lib
    h = model._handle
    P = tok.shape[0]
    td = torch.from_numpy(tok).cuda()
    xb = torch.full((P + 1, WT), CANARY_F, device="cuda")
    xp = torch.full((P + 1, model.config.embed_dim), CANARY_F, device="cuda")
    _lib.check(h.lib.miclip_encode_text(h.ptr, td.data_ptr(), P, xb.data_ptr(), xp.data_ptr(),
                                        _lib.stream_handle()), "miclip_encode_text")
    xb, xp = xb.cpu().numpy(), xp.cpu().numpy()
    assert (xb[P] == CANARY_F).all() and (xp[P] == CANARY_F).all(), "canary row written"
    return xb[:P], xp[:P]


@gpu
@pytest.mark.parametrize("L,E,resid_f32", TEXT_CASES)
def test_text_embed_eot_closed_form(L, E, resid_f32):
    """Route: the Python CLIP wrapper accepts transformer_layers = 0, so encode_text is
    token_embed -> ln_final on the EOT rows -> text_projection, with a closed form."""
    _need_gpu()
    from miclip import _lib
    model, sd = _text_model(L, E, resid_f32)
    flags = model._handle.lib.miclip_model_flags(model._handle.ptr)
    resid16 = bool(flags & _lib.MICLIP_MODEL_RESID16)
    assert resid16 == (not resid_f32)
    places = _placements(L)
    tok = _prompts(L, places, 31 * L + E)
    batches = [tok, np.concatenate([tok, tok])[1:4], tok[-1:], tok[:1]]   # P = all, 3, 1, 1
    proj = sd["text_projection"].astype(np.float64)
    cap = (WT + 8) * R.U24
    bar = _bar(MEASURED_XPROJ, cap)
    worst_b = worst_p = 0.0
    for t in batches:
        want, eot = R.text_eot_features(t, sd["token_embedding.weight"], sd["positional_embedding"],
                                        sd["ln_final.weight"], sd["ln_final.bias"], resid16)
        xb, xp = _encode_text(model, t)
        # a wrong position moves x_before by O(1): the rows of two positions differ
        e_b = float(np.abs(xb - want).max())
        ref_p = xb.astype(np.float64) @ proj
        # sum_d |x_d w_de| <= |x| |w_e| (Cauchy-Schwarz): the unit of the bound
        unit = np.sqrt((xb.astype(np.float64) ** 2).sum(axis=1)).max() * \
            np.sqrt((proj ** 2).sum(axis=0)).max()
        e_p = float(np.abs(xp - ref_p).max() / unit)
        worst_b, worst_p = max(worst_b, e_b), max(worst_p, e_p)
        print(f"L={L} E={E} resid16={resid16} P={len(t)} EOT {eot.tolist()}: x_before err {e_b:.3g} "
              f"(bar {LN_TOL:.3g}), x_proj rel err {e_p:.3g} (bar {bar:.3g}, cap {cap:.3g})")
        assert e_b <= LN_TOL
        assert bar <= cap and e_p <= bar
    # the expected positions: the first of each placement
    _, eot = R.text_eot_features(tok, sd["token_embedding.weight"], sd["positional_embedding"],
                                 sd["ln_final.weight"], sd["ln_final.bias"], resid16)
    assert eot.tolist() == [p[0] for p in places]
    if L > 1:   # the precondition of "a wrong position differs by O(1)"
        a = R.layernorm(sd["token_embedding.weight"][VOCAB - 1] + sd["positional_embedding"][0],
                        sd["ln_final.weight"], sd["ln_final.bias"])
        b = R.layernorm(sd["token_embedding.weight"][VOCAB - 1] + sd["positional_embedding"][L - 1],
                        sd["ln_final.weight"], sd["ln_final.bias"])
        assert np.abs(a - b).max() >= 100 * LN_TOL
