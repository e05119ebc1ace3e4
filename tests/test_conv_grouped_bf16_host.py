"""CPU: host side of the bf16 grouped 3x3 kernel (csrc/conv_grouped_bf16.inc) -- the C-ABI exports, the weight packer against
its index-by-index statement and the documented layout, the plan query's answers, argument checks of the entry point and the
``grouped_conv_bf16`` attribute."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from bts_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = (0, 0, 0)


def test_exports_and_abi_version_unchanged():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    lib = _lib.load_real()
    for name in ("bts_conv_grouped_bf16_fwd_f32", "bts_conv_grouped_bf16_plan"):
        assert name in _lib.ABI and re.search(r"\bint %s\s*\(" % name, hdr) and hasattr(lib, name)
    launch, query = _lib.ABI["bts_conv_grouped_bf16_fwd_f32"], _lib.ABI["bts_conv_grouped_bf16_plan"]
    assert launch.role == _lib.LAUNCH and query.role == _lib.QUERY
    assert launch.argtypes == _lib.ABI["bts_conv_grouped_fwd_f32"].argtypes and query.argtypes == _lib.ABI["bts_conv_grouped_plan"].argtypes
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr and lib.bts_hip_abi_version() == 17
    from bts_amd import conv_plan, plan
    assert launch.plan is None and "bts_conv_grouped_bf16_fwd_f32" not in plan._KINDS
    names = [conv_plan.grouped_bf16_kernel_name(cg) for cg in (4, 8, 16)]
    assert names == ["conv_grouped_bf16_kernel<%d>" % cg for cg in (4, 8, 16)]
    assert not any(n.startswith("conv_grouped_kernel") for n in names)         # existing tests count fp32 launches by that prefix


@pytest.mark.parametrize("c,groups", [(64, 4), (64, 8), (64, 16), (128, 16), (128, 32), (192, 12)])
def test_packer_matches_its_statement_and_the_documented_layout(c, groups):
    """Random weights: packer and statement agree bit for bit; bf16 index (((s*9 + tap)*4 + b)*64 + lane)*4 + j holds the
    weight from input channel 64 s + 16 b + 4 (lane >> 4) + j to output channel 64 s + 16 b + (lane & 15), rounded as
    Tensor.to(torch.bfloat16) rounds it, exactly 0 across groups."""
    cg = c // groups
    g = torch.Generator().manual_seed(c + groups)
    w = torch.randn((c, cg, 3, 3), generator=g) + 3.0                         # |w| > 0 after rounding: a 0 in the pack is structural
    w[0, 0, 0, :2] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])     # ties: to even, 1.0 and 1 + 2^-6
    assert bool((w.to(torch.bfloat16) != 0).all())
    u, ref = ops.pack_grouped_native_bf16(w, groups), ops.pack_grouped_native_bf16_reference(w, groups)
    assert u.dtype == torch.bfloat16 and u.numel() == 144 * c and u.is_contiguous() and u.dim() == 1
    assert torch.equal(u.view(torch.int16), ref.view(torch.int16))
    wb = w.to(torch.bfloat16)
    assert float(wb[0, 0, 0, 0]) == 1.0 and float(wb[0, 0, 0, 1]) == 1.0 + 2.0 ** -6
    for flat in torch.randint(0, u.numel(), (400,), generator=g).tolist() + [0, u.numel() - 1]:
        j = flat % 4; r = flat // 4
        lane = r % 64; r //= 64
        b = r % 4; r //= 4
        tap = r % 9; s = r // 9
        n, ci = 64 * s + 16 * b + (lane & 15), 64 * s + 16 * b + 4 * (lane >> 4) + j
        want = float(wb[n, ci % cg, tap // 3, tap % 3]) if ci // cg == n // cg else 0.0
        assert float(u[flat]) == want, (flat, s, tap, b, lane, j)
    assert (s, tap, b, lane, j) == (c // 64 - 1, 8, 3, 63, 3)
    assert int((u == 0).sum()) == 144 * c - 9 * c * cg                        # cross-group entries, and only they, are zero
    # the fp32 pack of the rounded weight holds the same values, in its own order
    assert sorted(u.float().tolist()) == sorted(ops.pack_grouped_native(wb.float(), groups).tolist())


def test_packer_rejects_other_shapes():
    for shape, groups in (((96, 8, 3, 3), 12), ((64, 2, 3, 3), 32), ((64, 32, 3, 3), 2), ((128, 64, 3, 3), 2), ((64, 8, 1, 1), 8),
                          ((64, 8, 3, 3), 4), ((64, 8, 5, 5), 8)):
        with pytest.raises(_lib.BtsHipError, match="pack_grouped_native"):
            ops.pack_grouped_native_bf16(torch.zeros(shape), groups)
        with pytest.raises(_lib.BtsHipError, match="pack_grouped_native"):
            ops.pack_grouped_native_bf16_reference(torch.zeros(shape), groups)


def test_plan_query_refusals():
    """Precision 0 and 1, 32 / 64 channels per group, c % 64 != 0, non-positive sizes and the shapes the launch refuses are
    never eligible, whatever the declaration; the answer has no batch argument."""
    for prec in ("fp32", "bf16x3", 0, 1):
        for ff in (1, 16, 4096):
            for (h, w, c, groups) in ((104, 136, 256, 32), (52, 68, 512, 32), (104, 136, 128, 32)):
                assert tuple(ops.conv_grouped_bf16_plan(h, w, c, groups, precision=prec, fill_frames=ff)) == NONE
    for ff in (1, 16, 4096):
        assert tuple(ops.conv_grouped_bf16_plan(26, 34, 1024, 32, precision="bf16", fill_frames=ff)) == NONE     # 32 per group
        assert tuple(ops.conv_grouped_bf16_plan(13, 17, 2048, 32, precision="bf16", fill_frames=ff)) == NONE     # 64 per group
        assert tuple(ops.conv_grouped_bf16_plan(52, 68, 96, 12, precision="bf16", fill_frames=ff)) == NONE       # c % 64
        assert tuple(ops.conv_grouped_bf16_plan(52, 68, 64, 32, precision="bf16", fill_frames=ff)) == NONE       # 2 per group
        assert tuple(ops.conv_grouped_bf16_plan(52, 68, 256, 7, precision="bf16", fill_frames=ff)) == NONE       # c % groups
        assert tuple(ops.conv_grouped_bf16_plan(0, 68, 256, 32, precision="bf16", fill_frames=ff)) == NONE
        assert tuple(ops.conv_grouped_bf16_plan(52, -3, 256, 32, precision="bf16", fill_frames=ff)) == NONE
        assert tuple(ops.conv_grouped_bf16_plan(52, 68, 0, 32, precision="bf16", fill_frames=ff)) == NONE
        assert tuple(ops.conv_grouped_bf16_plan(52, 68, 256, 0, precision="bf16", fill_frames=ff)) == NONE
    with ops.launch_config(fill_frames=16, precision="fp32"):
        assert not ops.conv_grouped_bf16_plan(52, 68, 512, 32).eligible
    assert list(inspect.signature(ops.conv_grouped_bf16_plan).parameters) == ["h", "w", "c", "groups", "precision", "fill_frames"]
    proto = re.search(r"int bts_conv_grouped_bf16_plan\(([^)]*)\)", open(os.path.join(ROOT, "include", "bts_hip.h")).read()).group(1)
    assert "int B" not in proto
    for bad in (dict(fill_frames=5000), dict(fill_frames=-1), dict(precision="fp16")):
        with pytest.raises(_lib.BtsHipError, match="conv_grouped_bf16_plan"):
            ops.conv_grouped_bf16_plan(52, 68, 512, 32, **{**dict(precision=2, fill_frames=16), **bad})
    bm, bn, wgs = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_long(0)
    q = _lib.load_real().bts_conv_grouped_bf16_plan
    assert q(52, 68, 512, 32, 2, 4097, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(wgs)) != 0
    assert q(52, 68, 512, 32, 2, 16, None, ctypes.byref(bn), ctypes.byref(wgs)) != 0


@pytest.mark.parametrize("h,w,c,groups", [(104, 136, 256, 32), (52, 68, 512, 32), (104, 136, 128, 32), (26, 34, 512, 32),
                                          (88, 304, 256, 32), (9, 17, 256, 32)])
def test_plan_query_is_monotone_in_fill_frames(h, w, c, groups):
    """A larger declared launch never turns an eligible layer away: over fill_frames = 1 .. 4096 the answer switches at most
    once, from refused to accepted; an accepted layer reports the 8 x 16-pixel tile, the 64-channel slab and its (tile, slab)
    pairs per frame."""
    answers = [ops.conv_grouped_bf16_plan(h, w, c, groups, precision="bf16", fill_frames=ff) for ff in range(1, 4097)]
    flags = [p.eligible for p in answers]
    assert flags == sorted(flags), "eligibility is not monotone in fill_frames"
    for p in answers:
        if p.eligible:
            assert (p.bm, p.bn, p.workgroups) == (128, 64, ((h + 7) // 8) * ((w + 15) // 16) * (c // 64))
        else:
            assert tuple(p) == NONE
    if any(flags):          # around the threshold: the last refused and the first accepted declaration are neighbours
        first = flags.index(True)
        assert all(flags[first:]) and not any(flags[:first])


def test_entry_point_rejects_bad_arguments_on_the_host():
    """The launch entry point validates before it touches the GPU: the alignment and shape rules of the fp32 entry point."""
    lib = _lib.load_real()
    f = lib.bts_conv_grouped_bf16_fwd_f32
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
    assert f(a, 64, 1, 4, 4, 64, 4, ctypes.c_void_p(4104), a, a, 0, a, 64, None) == INVALID   # weights not 16-byte aligned
    assert f(a, 64, 1, 4, 4, 64, 5, a, a, a, 0, a, 64, None) == INVALID                       # c % groups
    assert f(a, 64, 1, 4, 4, 64, 0, a, a, a, 0, a, 64, None) == INVALID                       # no groups
    assert f(a, 64, 1, 4, 4, 64, 4, a, a, a, 3, a, 64, None) == INVALID                       # sigmoid is not built
    assert f(a, 64, 0, 4, 4, 64, 4, a, a, a, 0, a, 64, None) == INVALID                       # B 0
    assert f(a, 64, 1, 4, 4, 64, 2, a, a, a, 0, a, 64, None) == UNSUPPORTED                   # 32 channels per group
    assert f(a, 64, 1, 4, 4, 64, 32, a, a, a, 0, a, 64, None) == UNSUPPORTED                  # 2 channels per group
    assert f(a, 64, 32768, 512, 512, 64, 4, a, a, a, 0, a, 64, None) == UNSUPPORTED           # 2^33 pixels: past the 32-bit counters


def test_forward_wrapper_rejects_what_does_not_fit():
    """ops.conv_grouped_bf16_forward refuses CPU tensors like every hot-path wrapper (no fallback)."""
    w = ops.pack_grouped_native_bf16(torch.zeros(64, 16, 3, 3), 4)
    with pytest.raises(_lib.BtsHipError):
        ops.conv_grouped_bf16_forward(torch.zeros(16, 64), 1, 4, 4, w, 64, 4)


def test_model_attribute():
    from bts_amd import bts as M
    from bts_amd.encoder_hip import ResNetHip
    from parity_util import Params
    m = M.BtsModel(Params("resnext50_bts", 512, 10.0, "nyu"))
    assert m.grouped_conv_bf16 == "bundles" and m.grouped_conv == "bundles"
    for mode in ("auto", "native", "bundles"):
        m.grouped_conv_bf16 = mode
        assert m.grouped_conv_bf16 == mode and m.grouped_conv == "bundles"
    for bad in ("sometimes", "", None, True, 1, "Native"):
        with pytest.raises(_lib.BtsHipError, match="grouped_conv_bf16"):
            m.grouped_conv_bf16 = bad
        assert m.grouped_conv_bf16 == "bundles"
    m.grouped_conv = "native"
    assert m.grouped_conv_bf16 == "bundles"
    plan = ResNetHip(m.encoder.base_model)
    assert plan.grouped_conv_bf16 == "bundles" and plan.grouped_conv == "bundles"
