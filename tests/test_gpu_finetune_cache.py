"""GPU: last-block fine-tuning from a cached frozen trunk (miclip_ft_grad_rows,
miclip/finetune.py's TrunkCache / fill_view / step_rows and FTOpenCLIP's trunk_cache_* keys).

Everything here is an equality: the row-mapped entry reads the cache in place and must give,
bit for bit, what miclip_ft_grad gives on a contiguous copy of the same token blocks, so there
is no tolerance anywhere in this file.

Op level (tests/_ft_ref.tail_case, seed 21, the x of all cached images; the batch's labels are
those of the images picked), fp16 and bf16 compute:
  * 7 cached images, rows [5, 0, 5], N 7, W 256: an image twice; fp16 and fp32 stream;
    groups 1 (a sentinel survives outside proj's slice) and 2;
  * 4 cached images, rows [3, 1], N 257: rows cross a 256-row tile and several TN-GEMM slices;
  * 3 cached images, rows [2], N 5, W 640, head dim 80, erf;
  * 2 cached images, rows [0, 1]: the identity map against the plain entry on the whole cache.
The scratch ends in a canary, the cache is unchanged afterwards, a second call is identical.

Trainer level, the tiny tower of tests/test_gpu_finetune.py (N 5, W 256, 2 layers, E 64): two
views of 7 images in batches 3 / 3 / 1, 3 epochs, shuffled; step_rows on the cache equals a
replay of step() on the images in the same order (params, m, v, every step's statistics). This
rests on a trunk row depending on its image alone
(test_gpu_finetune.py::test_trunk_and_tail_forward_match_the_oracle).

FTOpenCLIP: trunk_cache_views 2 over 3 epochs commits the replay's state dict with 2 x batches
trunk calls; trunk_cache_views 0 is the run without the key; a budget one byte short raises
before any step.
"""
import ctypes

import numpy as np
import pytest
import torch

import _ft_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": 0, "bf16": 1}
ACTS = {"quick": 1, "erf": 2}
X_FP16, X_F32 = 0, 3
SENTINEL = -3.0
# (cached images, rows, N, W, dh, E, C, act)
BASE = (7, (5, 0, 5), 7, 256, 64, 64, 5, "quick")
TILE = (4, (3, 1), 257, 256, 64, 64, 20, "quick")
DH80 = (3, (2,), 5, 640, 80, 128, 20, "erf")
IDENT = (2, (0, 1), 7, 256, 64, 64, 5, "quick")


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    assert torch.cuda.is_available()
    return _lib.load_library()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


_CASE = {}


def _case(case):
    """Device inputs of a case, made once: the cache in both stream types, the flat
    parameter block, the text weights and every cached image's label."""
    if case not in _CASE:
        n, _, N, W, dh, E, C, act = case
        x, p, Wt, labels = R.tail_case(n, N, W, E, C, seed=21)
        _CASE[case] = {X_FP16: x.half().cuda().reshape(n * N, W).contiguous(),
                       X_F32: x.float().cuda().reshape(n * N, W).contiguous(),
                       "flat": torch.cat([t.reshape(-1).float() for t in p]).cuda(),
                       "Wt": Wt.float().cuda().contiguous(), "labels": labels.long().cuda()}
    return _CASE[case]


def _grad(lib, x, x_dtype, rows, cached, labels, d, case, name, groups):
    """(grads with their padding, stats, feats) of miclip_ft_grad (rows None: x is the batch)
    or miclip_ft_grad_rows (x is the cache of `cached` images)."""
    from miclip import _lib
    _, _, N, W, dh, E, C, act = case
    B = int(labels.numel())
    off = (ctypes.c_int64 * 16)()
    assert lib.miclip_ft_layout(W, E, off) == 0 and d["flat"].numel() == off[15]
    size = lib.miclip_ft_scratch_bytes if rows is None else lib.miclip_ft_rows_scratch_bytes
    nbytes = size(B, N, W, E, C, dh)
    assert nbytes > 0
    scratch = torch.empty(nbytes + 256, device="cuda", dtype=torch.uint8)
    scratch[nbytes:] = 0xA5
    grads = torch.full((off[15] + 64,), SENTINEL, device="cuda")
    stats = torch.full((4,), -7.0, device="cuda")
    y = torch.full((B * W + 64,), -7.0, device="cuda")
    st = _lib.stream_handle(torch.device("cuda"))
    tail = (_ptr(labels), _ptr(d["Wt"]), _ptr(d["flat"]), B, N, W, E, C, dh, ACTS[act],
            DTYPES[name], 100.0, groups, _ptr(grads), _ptr(scratch), _ptr(stats), _ptr(y), st)
    if rows is None:
        _lib.check(lib.miclip_ft_grad(_ptr(x), x_dtype, *tail), "miclip_ft_grad")
    else:
        host = (ctypes.c_int64 * B)(*rows)
        _lib.check(lib.miclip_ft_grad_rows(_ptr(x), x_dtype, cached, host, *tail),
                   "miclip_ft_grad_rows")
        for i in range(B):      # the array is the caller's again on return
            host[i] = -1
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all())
    g, s, yc = grads.cpu(), stats.cpu(), y.cpu()
    assert bool((s[2:] == -7.0).all()) and bool((yc[B * W:] == -7.0).all())
    assert bool((g[off[15]:] == SENTINEL).all())
    if groups == 1:
        assert bool((g[:off[14]] == SENTINEL).all())
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(s[:2]).all())
    return g, s[:2].clone(), yc[:B * W].clone()


def _check_rows_equal_a_contiguous_copy(lib, case, name, x_dtype, groups):
    n, rows, N, W = case[:4]
    d = _case(case)
    cache = d[x_dtype]
    before = cache.clone()
    idx = torch.tensor(rows, device="cuda")
    labels = d["labels"][idx].contiguous()
    batch = cache.reshape(n, N, W)[idx].reshape(len(rows) * N, W).contiguous()
    want = _grad(lib, batch, x_dtype, None, n, labels, d, case, name, groups)
    got = _grad(lib, cache, x_dtype, rows, n, labels, d, case, name, groups)
    for a, b, what in zip(got, want, ("grads", "stats", "feats")):
        assert torch.equal(a, b), what
    assert torch.equal(cache, before)
    again = _grad(lib, cache, x_dtype, rows, n, labels, d, case, name, groups)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    return got


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("x_dtype", [X_FP16, X_F32], ids=["x16", "x32"])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_a_repeated_image_in_both_stream_types_and_groups(lib, name, x_dtype, groups):
    _check_rows_equal_a_contiguous_copy(lib, BASE, name, x_dtype, groups)


@pytest.mark.parametrize("case", [TILE, DH80], ids=["n257", "dh80"])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_rows_across_tiles_and_head_dim_80(lib, name, case):
    _check_rows_equal_a_contiguous_copy(lib, case, name, X_FP16, 2)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_identity_map_is_the_plain_entry_on_the_whole_cache(lib, name):
    n, rows = IDENT[:2]
    d = _case(IDENT)
    want = _grad(lib, d[X_FP16], X_FP16, None, n, d["labels"], d, IDENT, name, 2)
    got = _grad(lib, d[X_FP16], X_FP16, rows, n, d["labels"], d, IDENT, name, 2)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_a_bad_index_is_refused_before_any_launch(lib):
    d = _case(BASE)
    labels = d["labels"][:3].contiguous()
    for rows in ((5, 7, 0), (5, -1, 0)):
        with pytest.raises(ValueError, match="rows"):
            _grad(lib, d[X_FP16], X_FP16, rows, 7, labels, d, BASE, "fp16", 2)
    torch.cuda.synchronize()


# ---- trainer level ----
def _tower(name):
    import miclip
    from miclip.configs import CLIPConfig
    from miclip.weights import generate_state_dict
    cfg = CLIPConfig(embed_dim=64, image_resolution=64, vision_layers=2, vision_width=256,
                     vision_patch_size=32, context_length=77, vocab_size=49408,
                     transformer_width=256, transformer_heads=4, transformer_layers=1)
    sd = generate_state_dict(cfg, seed=0)
    return miclip.CLIP(cfg, {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()},
                       device="cuda", compute_dtype=name, surface="open_clip")


def _text_weights(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(64, 5, generator=g), dim=0)


def _batches(imgs, labels, B):
    return [(imgs[i:i + B], labels[i:i + B]) for i in range(0, imgs.shape[0], B)]


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_cached_epochs_equal_a_replay_through_step(name, groups):
    from miclip.finetune import LastBlockTrainer, TrunkCache, cache_order, cache_view
    from miclip.weights import synthetic_images
    model = _tower(name)
    tw = _text_weights(1)
    views = [torch.from_numpy(synthetic_images(7, 64, seed=s)) for s in (5, 6)]
    labels = torch.randint(0, 5, (7,), generator=torch.Generator().manual_seed(3))
    epochs, seed, B = 3, 4, 3

    cached = LastBlockTrainer(model, tw, unlocked_groups=groups, lr=1e-3, epochs=epochs)
    cache = TrunkCache()
    for v, imgs in enumerate(views):
        assert cached.fill_view(cache, _batches(imgs, labels, B)) == v
    assert cache.views == 2 and cache.n == [7, 7] and cache.batch_size == 3
    assert cache.nbytes == 2 * 7 * 5 * 256 * 2
    for v in range(2):
        assert cache.x[v].shape == (7 * 5, 256) and cache.x[v].dtype == torch.float16
        assert cache.x[v].is_cuda and cache.targets[v].is_cuda
        assert cache.targets[v].dtype == torch.int64 == cache.targets_host[v].dtype
        assert torch.equal(cache.targets_host[v], labels) and not cache.targets_host[v].is_cuda
    assert not torch.equal(cache.x[0], cache.x[1])
    kept = [x.clone() for x in cache.x]

    replay = LastBlockTrainer(model, tw, unlocked_groups=groups, lr=1e-3, epochs=epochs)
    got, want = [], []
    for e in range(epochs):
        cached.set_epoch(e)
        replay.set_epoch(e)
        view, order = cache_view(e, 2), cache_order(7, seed, e)
        for lo in range(0, 7, B):
            rows = order[lo:lo + B]
            got.append(torch.stack(cached.step_rows(cache, view, rows)))
            want.append(torch.stack(replay.step(views[view][rows].cuda(), labels[rows])))
    assert len(got) == 9 and cached.steps == replay.steps == 9
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    for a, b, what in ((cached.params, replay.params, "params"), (cached.m, replay.m, "m"),
                       (cached.v, replay.v, "v")):
        assert torch.equal(a, b), what
    assert all(torch.equal(a, b) for a, b in zip(cache.x, kept))
    with pytest.raises(ValueError, match="rows must lie"):
        cached.step_rows(cache, 0, [0, 7])
    assert cached.steps == 9


# ---- FTOpenCLIP ----
def _loaders():
    from miclip.weights import synthetic_images
    g = torch.Generator().manual_seed(2)

    def loader(seed, n_batches, B):
        return [(torch.from_numpy(synthetic_images(B, 64, seed=seed + b)),
                 torch.randint(0, 5, (B,), generator=g)) for b in range(n_batches)]
    return loader(10, 2, 4), loader(20, 1, 3), loader(30, 2, 3)


def _cfg(tmp_path, groups, epochs, **keys):
    return {"lr_v": 1e-3, "train_epoch": epochs, "root_path": str(tmp_path), "dataset": "cs",
            "seed": 1, "clip_backend": "openclip", "open_clip_model": "ViT-H-14",
            "finetune": dict({"unlocked_groups": groups, "tune_text": False, "val_interval": 1},
                             **keys)}


@pytest.mark.parametrize("groups", [1, 2])
def test_ftopenclip_trains_from_the_cache(tmp_path, capsys, monkeypatch, groups):
    from miclip.finetune import FTOpenCLIP, LastBlockTrainer, cache_order
    train, val, test = _loaders()
    tw = _text_weights(2).cuda()
    names = [f"c{i}" for i in range(5)]
    calls = []
    trunk = LastBlockTrainer.trunk
    monkeypatch.setattr(LastBlockTrainer, "trunk",
                        lambda self, images: calls.append(1) or trunk(self, images))
    model = _tower("fp16")
    method = FTOpenCLIP(_cfg(tmp_path, groups, 3, trunk_cache_views=2))
    res = method(train, val, test, tw, model, names, 0, "cfg", False)
    assert len(calls) == 2 * len(train)
    assert len(res) == 6 and all(isinstance(v, float) for v in res[:5])
    assert isinstance(res[5], np.ndarray) and res[5].shape == (5, 5) and res[5].sum() == 6
    out = capsys.readouterr().out
    for word in ("Trainable params: %d" % (1 if groups == 1 else 15), "Start Training procedure",
                 "Train Epoch: 3 / 3", "Avg Loss:", "[val epoch 1]", "[val epoch 3]",
                 "[test] loss="):
        assert word in out, word
    assert out.count("/8), Avg Loss:") == 3          # every epoch saw the 8 cached images
    assert method.trunk_cache.views == 2 and method.trunk_cache.n == [8, 8]

    monkeypatch.setattr(LastBlockTrainer, "trunk", trunk)
    other = _tower("fp16")
    imgs = torch.cat([b[0] for b in train])
    labels = torch.cat([b[1] for b in train])
    tr = LastBlockTrainer(other, tw, unlocked_groups=groups, lr=1e-3, epochs=3)
    for e in range(3):
        tr.set_epoch(e)
        order = cache_order(8, 1, e)
        for lo in range(0, 8, 4):
            rows = order[lo:lo + 4]
            tr.step(imgs[rows].cuda(), labels[rows])
    tr.commit()
    a, b = model.state_dict(), other.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_zero_views_is_the_run_without_the_key(tmp_path, capsys):
    from miclip.finetune import FTOpenCLIP
    train, val, test = _loaders()
    tw = _text_weights(2).cuda()
    names = [f"c{i}" for i in range(5)]
    runs = []
    for keys in ({}, {"trunk_cache_views": 0}):
        model = _tower("fp16")
        method = FTOpenCLIP(_cfg(tmp_path, 2, 2, **keys))
        res = method(train, val, test, tw, model, names, 0, "cfg", False)
        assert method.trunk_cache is None
        runs.append((res, {k: v.detach().clone() for k, v in model.state_dict().items()},
                     capsys.readouterr().out))
    (ra, sa, oa), (rb, sb, ob) = runs
    assert ra[:5] == rb[:5] and np.array_equal(ra[5], rb[5])
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert oa == ob


def test_a_budget_one_byte_short_raises_before_any_step(tmp_path):
    from miclip.finetune import FTOpenCLIP
    train, val, test = _loaders()
    tw = _text_weights(2).cuda()
    model = _tower("fp16")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    view_bytes = 8 * 5 * 256 * 2
    method = FTOpenCLIP(_cfg(tmp_path, 2, 2, trunk_cache_views=1,
                             trunk_cache_max_bytes=view_bytes - 1))
    with pytest.raises(ValueError, match=rf"{view_bytes} bytes.*budget of {view_bytes - 1} bytes"):
        method(train, val, test, tw, model, [f"c{i}" for i in range(5)], 0, "cfg", False)
    assert method.trainer.steps == 0
    assert all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    # the exact size fits
    FTOpenCLIP(_cfg(tmp_path, 2, 1, trunk_cache_views=1, trunk_cache_max_bytes=view_bytes))(
        train, None, None, tw, model, [f"c{i}" for i in range(5)], 0, "cfg", False)
