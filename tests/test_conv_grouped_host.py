"""CPU: host side of the native grouped 3x3 kernel (csrc/conv_grouped.inc) -- weight packer against its index-by-index
statement and the documented layout, the plan query's answers, argument checks of the entry point, and the C-ABI export
list."""
import ctypes
import os
import re

import pytest
import torch

from bts_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c,groups", [(64, 4), (64, 8), (64, 16), (128, 16), (128, 32), (192, 12)])
def test_packer_matches_its_statement_and_the_documented_layout(c, groups):
    """Integer weights: packer and statement agree bit for bit, and float ((s*9 + tap)*16 + k)*64 + lane holds the weight
    from input channel 64 s + 16 (lane >> 4) + k to output channel 64 s + lane (include/bts_hip.h), exactly 0 across groups."""
    cg = c // groups
    g = torch.Generator().manual_seed(c + groups)
    w = torch.randint(1, 9, (c, cg, 3, 3), generator=g).float()           # no zero weight: a 0 in the pack is structural
    u, ref = ops.pack_grouped_native(w, groups), ops.pack_grouped_native_reference(w, groups)
    assert u.dtype == torch.float32 and u.numel() == 144 * c and u.is_contiguous()
    assert torch.equal(u, ref)
    for flat in torch.randint(0, u.numel(), (400,), generator=g).tolist() + [0, u.numel() - 1]:
        lane = flat % 64; r = flat // 64
        k = r % 16; r //= 16
        tap = r % 9; s = r // 9
        n, ci = 64 * s + lane, 64 * s + 16 * (lane >> 4) + k
        want = float(w[n, ci % cg, tap // 3, tap % 3]) if ci // cg == n // cg else 0.0
        assert float(u[flat]) == want, (flat, s, tap, k, lane)
    assert (s, tap, k, lane) == (c // 64 - 1, 8, 15, 63)
    assert int((u == 0).sum()) == 144 * c - 9 * c * cg                    # cross-group entries, and only they, are zero


def test_packer_rejects_other_shapes():
    for shape, groups in (((96, 8, 3, 3), 12), ((64, 2, 3, 3), 32), ((64, 32, 3, 3), 2), ((128, 64, 3, 3), 2), ((64, 8, 1, 1), 8),
                          ((64, 8, 3, 3), 4), ((64, 8, 5, 5), 8)):
        with pytest.raises(_lib.BtsHipError, match="pack_grouped_native"):
            ops.pack_grouped_native(torch.zeros(shape), groups)


# every stride-1 grouped layer with <= 16 channels per group: (layer, channels, channels per group), input map = image >> (layer + 1)
LAYERS = {"resnext101_32x8d": ((1, 256, 8), (2, 512, 16)), "resnext50_32x4d": ((1, 128, 4), (2, 256, 8), (3, 512, 16))}


def test_plan_query_eligibility():
    """Every class scripts/grouped_conv_bench.py measured at fill_frames 16 beat the bundle launch by more than the spread
    (DESIGN 3d), so every one is eligible there."""
    for (H, W) in ((416, 544), (352, 1216)):
        for layers in LAYERS.values():
            for li, c, cg in layers:
                h, w = H >> (li + 1), W >> (li + 1)
                p = ops.conv_grouped_plan(h, w, c, c // cg, precision="fp32", fill_frames=16)
                assert p.eligible and (p.bm, p.bn) == (128, 64), (H, W, li, p)
                assert p.workgroups == ((h + 7) // 8) * ((w + 15) // 16) * (c // 64)
                assert not ops.conv_grouped_plan(h, w, c, c // cg, precision="bf16x3", fill_frames=16).eligible
                assert not ops.conv_grouped_plan(h, w, c, c // cg, precision="bf16", fill_frames=16).eligible
    none = (0, 0, 0)
    assert tuple(ops.conv_grouped_plan(26, 34, 1024, 32, precision=0, fill_frames=16)) == none       # 32 channels per group
    assert tuple(ops.conv_grouped_plan(13, 17, 2048, 32, precision=0, fill_frames=16)) == none       # 64 channels per group
    assert tuple(ops.conv_grouped_plan(52, 68, 96, 12, precision=0, fill_frames=16)) == none         # not whole 64-channel slabs
    assert tuple(ops.conv_grouped_plan(16, 24, 256, 32, precision=0, fill_frames=16)) == none        # tiny map: 16 x 16 pairs < 1024
    assert tuple(ops.conv_grouped_plan(9, 17, 256, 32, precision=0, fill_frames=4096)) == none       # under-filled grid (0.30)
    assert tuple(ops.conv_grouped_plan(104, 136, 256, 32, precision=0, fill_frames=2)) == none       # 2 x 468 pairs < 1024
    assert ops.conv_grouped_plan(104, 136, 256, 32, precision=0, fill_frames=3).eligible
    with ops.launch_config(fill_frames=16, precision="fp32"):
        assert ops.conv_grouped_plan(52, 68, 512, 32).eligible
    with ops.launch_config(fill_frames=16, precision="bf16"):
        assert not ops.conv_grouped_plan(52, 68, 512, 32).eligible
    # no B argument exists: the answer is a function of per-frame geometry and the declaration
    import inspect
    assert list(inspect.signature(ops.conv_grouped_plan).parameters) == ["h", "w", "c", "groups", "precision", "fill_frames"]
    assert "int B" not in re.search(r"int bts_conv_grouped_plan\(([^)]*)\)", open(os.path.join(ROOT, "include", "bts_hip.h")).read()).group(1)
    with pytest.raises(_lib.BtsHipError, match="conv_grouped_plan"):
        ops.conv_grouped_plan(52, 68, 512, 32, precision=0, fill_frames=5000)
    with pytest.raises(_lib.BtsHipError, match="conv_grouped_plan"):
        ops.conv_grouped_plan(52, 68, 512, 32, precision=0, fill_frames=-1)
    with pytest.raises(_lib.BtsHipError, match="conv_grouped_plan"):
        ops.conv_grouped_plan(52, 68, 512, 32, precision="fp16")
    bm, bn, wgs = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_long(0)
    q = _lib.load_real().bts_conv_grouped_plan
    assert q(52, 68, 512, 32, 0, 4097, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(wgs)) != 0
    assert q(52, 68, 512, 32, 0, 16, None, ctypes.byref(bn), ctypes.byref(wgs)) != 0


def test_entry_point_rejects_bad_arguments_on_the_host():
    """The launch entry point validates before it touches the GPU."""
    lib = _lib.load_real()
    f = lib.bts_conv_grouped_fwd_f32
    a = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails its checks first
    INVALID, UNSUPPORTED = f(None, 64, 1, 4, 4, 64, 4, a, a, a, 0, a, 64, None), f(a, 96, 1, 4, 4, 96, 12, a, a, a, 0, a, 96, None)
    assert INVALID != 0 and UNSUPPORTED != 0 and INVALID != UNSUPPORTED                       # null x; c % 64 != 0
    assert b"not built" in lib.bts_hip_error_string(UNSUPPORTED)
    assert f(a, 64, 1, 4, 4, 64, 4, None, a, a, 0, a, 64, None) == INVALID                    # null w_packed
    assert f(a, 64, 1, 4, 4, 64, 4, a, a, a, 0, None, 64, None) == INVALID                    # null y
    assert f(a, 64, 1, 4, 4, 64, 4, a, a, None, 0, a, 64, None) == INVALID                    # half an e1 pair
    assert f(a, 64, 1, 4, 4, 64, 4, a, None, a, 0, a, 64, None) == INVALID
    assert f(a, 32, 1, 4, 4, 64, 4, a, a, a, 0, a, 64, None) == INVALID                       # x stride < c
    assert f(a, 66, 1, 4, 4, 64, 4, a, a, a, 0, a, 64, None) == INVALID                       # x stride not a multiple of 4
    assert f(a, 64, 1, 4, 4, 64, 4, a, a, a, 0, a, 32, None) == INVALID                       # y stride < c
    assert f(a, 64, 1, 4, 4, 64, 4, a, a, a, 0, a, 70, None) == INVALID                       # y stride not a multiple of 4
    assert f(ctypes.c_void_p(4100), 64, 1, 4, 4, 64, 4, a, a, a, 0, a, 64, None) == INVALID   # x not 16-byte aligned
    assert f(a, 64, 1, 4, 4, 64, 5, a, a, a, 0, a, 64, None) == INVALID                       # c % groups
    assert f(a, 64, 1, 4, 4, 64, 0, a, a, a, 0, a, 64, None) == INVALID                       # no groups
    assert f(a, 64, 1, 4, 4, 64, 4, a, a, a, 3, a, 64, None) == INVALID                       # sigmoid is not built
    assert f(a, 64, 0, 4, 4, 64, 4, a, a, a, 0, a, 64, None) == INVALID                       # B 0
    assert f(a, 64, 1, 4, 4, 64, 2, a, a, a, 0, a, 64, None) == UNSUPPORTED                   # 32 channels per group
    assert f(a, 64, 1, 4, 4, 64, 32, a, a, a, 0, a, 64, None) == UNSUPPORTED                  # 2 channels per group
    assert f(a, 64, 32768, 512, 512, 64, 4, a, a, a, 0, a, 64, None) == UNSUPPORTED           # 2^33 pixels: past the 32-bit counters


def test_forward_wrapper_rejects_views_that_do_not_fit():
    """ops.conv_grouped_forward refuses CPU tensors like every hot-path wrapper (no fallback)."""
    w = ops.pack_grouped_native(torch.zeros(64, 16, 3, 3), 4)
    with pytest.raises(_lib.BtsHipError):
        ops.conv_grouped_forward(torch.zeros(16, 64), 1, 4, 4, w, 64, 4)


def test_exports_and_abi_version_unchanged():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    for name in ("bts_conv_grouped_fwd_f32", "bts_conv_grouped_plan"):          # prototypes: test_host_logic's table-driven test
        assert name in _lib.ABI and re.search(r"\b%s\s*\(" % name, hdr)
    assert _lib.ABI["bts_conv_grouped_fwd_f32"].role == _lib.LAUNCH and _lib.ABI["bts_conv_grouped_plan"].role == _lib.QUERY
    assert len(_lib.ABI["bts_conv_grouped_fwd_f32"].argtypes) == 14 and len(_lib.ABI["bts_conv_grouped_plan"].argtypes) == 9
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr
    from bts_amd import conv_plan, plan
    assert "bts_conv_grouped_fwd_f32" not in plan._KINDS and "bts_conv_grouped_plan" not in plan._KINDS
    assert _lib.ABI["bts_conv_grouped_fwd_f32"].plan is None
    assert [conv_plan.grouped_kernel_name(cg) for cg in (4, 8, 16)] == ["conv_grouped_kernel<%d>" % cg for cg in (4, 8, 16)]


def test_model_attribute_defaults_to_bundles():
    from bts_amd import bts as M
    from bts_amd.encoder_hip import ResNetHip
    from parity_util import Params
    m = M.BtsModel(Params("resnext50_bts", 512, 10.0, "nyu"))
    assert m.grouped_conv == "bundles"
    plan = ResNetHip(m.encoder.base_model)
    assert plan.grouped_conv == "bundles" and ResNetHip.GROUPED_MODES == ("bundles", "auto", "native")
