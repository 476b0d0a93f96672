"""CPU: the trunk cache of last-block fine-tuning -- the C-ABI entry points
miclip_ft_rows_scratch_bytes / miclip_ft_grad_rows refuse bad arguments, naming them, before
any device access (there is no GPU here: every call below must return before a launch), and
the host-side schedule and config parsing of miclip/finetune.py."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP16, BF16, MXFP8, F32 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from miclip import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j", "8"], check=True)
    return _lib.load_library()


def _p(v=4096):
    """A non-NULL, aligned pointer that is never dereferenced (validation comes first)."""
    return ctypes.c_void_p(v)


def _rows(lib, *, rows=(5, 0, 5), cache_images=7, B=None, N=7, W=256, E=64, C=5, dh=64, act=1,
          dtype=FP16, x_dtype=FP16, groups=2, null=None, scratch=4096):
    names = ("x_cache", "labels", "text_weights", "params", "grads", "scratch", "stats")
    a = {n: (None if n == null else _p()) for n in names}
    if null != "scratch":
        a["scratch"] = _p(scratch)
    r = None if null == "rows" else (ctypes.c_int64 * len(rows))(*rows)
    B = len(rows) if B is None else B
    return lib.miclip_ft_grad_rows(a["x_cache"], x_dtype, cache_images, r, a["labels"],
                                   a["text_weights"], a["params"], B, N, W, E, C, dh, act, dtype,
                                   100.0, groups, a["grads"], a["scratch"], a["stats"], None, None)


def test_symbols_are_exported_and_abi_stays_9(lib):
    from miclip import _lib
    for s in ("miclip_ft_rows_scratch_bytes", "miclip_ft_grad_rows"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    assert lib.miclip_abi_version() == 10 == _lib.ABI_VERSION


def test_rows_scratch_is_the_plain_scratch_plus_the_index_area(lib):
    for shape in ((3, 7, 256, 64, 5, 64), (2, 5, 640, 128, 20, 80), (256, 257, 1024, 768, 20, 64),
                  (1, 1, 128, 16, 1, 64)):
        plain, rows = lib.miclip_ft_scratch_bytes(*shape), lib.miclip_ft_rows_scratch_bytes(*shape)
        assert plain > 0 and rows >= plain + 8 * shape[0] and rows % 256 == 0, shape
    for shape in ((0, 7, 256, 64, 5, 64), (3, 0, 256, 64, 5, 64), (3, 769, 256, 64, 5, 64),
                  (3, 7, 200, 64, 5, 64), (3, 7, 256, 64, 5, 80), (3, 7, 256, 64, 5, 32),
                  (3, 7, 256, 8, 5, 64), (3, 7, 256, 64, 0, 64), (3, 7, 256, 64, 1025, 64)):
        assert lib.miclip_ft_rows_scratch_bytes(*shape) == 0, shape


def test_grad_rows_refuses_bad_arguments_by_name(lib):
    for kw, word in (({"rows": (5, -1, 5)}, b"rows:"), ({"rows": (5, 0, 7)}, b"rows:"),
                     ({"rows": (7,)}, b"rows:"), ({"cache_images": 0}, b"cache_images:"),
                     ({"cache_images": -3}, b"cache_images:"),
                     ({"rows": (0,), "cache_images": 1 << 40}, b"cache_images:"),
                     ({"groups": 3}, b"groups:"), ({"groups": 0}, b"groups:"),
                     ({"dh": 32}, b"head_dim:"), ({"dh": 80}, b"W:"), ({"rows": ()}, b"B:"),
                     ({"N": 0}, b"N:"), ({"N": 769}, b"N:"), ({"W": 200}, b"W:"),
                     ({"E": 8}, b"E:"), ({"C": 0}, b"C:"), ({"dtype": MXFP8}, b"compute_dtype:"),
                     ({"x_dtype": BF16}, b"x_dtype:"), ({"act": 3}, b"act:"),
                     ({"scratch": 4096 + 64}, b"scratch:")):
        assert _rows(lib, **kw) == -1, kw
        assert word in lib.miclip_last_error(), (kw, lib.miclip_last_error())
    for name in ("x_cache", "rows", "labels", "text_weights", "params", "grads", "scratch", "stats"):
        assert _rows(lib, null=name) == -1
        assert lib.miclip_last_error() == b"null argument: " + name.encode()
    # the message of a bad index names the position, the value and the bound
    assert _rows(lib, rows=(5, 0, 7)) == -1
    msg = lib.miclip_last_error()
    assert b"rows[2]" in msg and b"7" in msg


def test_cache_order():
    from miclip.finetune import cache_order
    for n in (1, 7, 64):
        o = cache_order(n, 3, 0)
        assert o.dtype == torch.int64 and o.device.type == "cpu"
        assert sorted(o.tolist()) == list(range(n))
        assert torch.equal(o, cache_order(n, 3, 0))
        assert cache_order(n, 3, 5, shuffle=False).tolist() == list(range(n))
    assert not torch.equal(cache_order(7, 3, 0), cache_order(7, 3, 1))
    assert not torch.equal(cache_order(7, 3, 0), cache_order(7, 4, 0))
    # the state of the global generator plays no part
    torch.manual_seed(0)
    a = cache_order(7, 1, 2)
    torch.manual_seed(123)
    torch.randperm(5)
    assert torch.equal(a, cache_order(7, 1, 2))


def test_view_schedule_is_the_epoch_modulo_the_views():
    from miclip.finetune import cache_view
    assert [cache_view(e, 3) for e in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    assert [cache_view(e, 1) for e in range(3)] == [0, 0, 0]
    assert [cache_view(e, 2) for e in range(3)] == [0, 1, 0]


def test_key_parser_defaults_and_errors():
    from miclip.finetune import trunk_cache_config
    assert trunk_cache_config({"finetune": {}}) == (0, True, None)
    assert trunk_cache_config({"finetune": None}) == (0, True, None)
    assert trunk_cache_config({}) == (0, True, None)
    assert trunk_cache_config({"finetune": {"trunk_cache_views": None}}) == (0, True, None)
    assert trunk_cache_config({"finetune": {"trunk_cache_views": 3, "trunk_cache_shuffle": False,
                                            "trunk_cache_max_bytes": 1 << 30}}) == \
        (3, False, 1 << 30)
    for bad in (-1, 1.5, 2.0, "2", True):
        with pytest.raises(ValueError, match="trunk_cache_views"):
            trunk_cache_config({"finetune": {"trunk_cache_views": bad}})
    for bad in (-1, 0.5, "1G"):
        with pytest.raises(ValueError, match="trunk_cache_max_bytes"):
            trunk_cache_config({"finetune": {"trunk_cache_views": 1, "trunk_cache_max_bytes": bad}})


def test_validate_config_keeps_its_tuple_with_the_new_keys():
    from miclip.finetune import validate_config

    class _M:
        def named_parameters(self):
            return iter([("visual.transformer.resblocks.0.ln_1.weight", None),
                         ("visual.proj", None)])
    cfg = {"lr_v": 1e-3, "train_epoch": 4,
           "finetune": {"unlocked_groups": 1, "val_interval": 2, "trunk_cache_views": 2,
                        "trunk_cache_shuffle": False, "trunk_cache_max_bytes": 1 << 20}}
    assert validate_config(cfg, _M()) == (1, False, 1e-3, 4, 2)


def test_empty_cache_reports_no_views():
    from miclip.finetune import TrunkCache
    c = TrunkCache(100)
    assert c.views == 0 and c.nbytes == 0 and c.max_bytes == 100 and c.batch_size is None
