"""CPU: host side of the fused Winograd conv1 kernel (csrc/conv_wino_tail.inc) -- weight packer against its fp64 statement
and the documented layout, the fp64 identity of the formulation, the plan query's answers, argument checks of the entry
point, and the C-ABI export list."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from bts_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


@pytest.mark.parametrize("n_tail", [0, 1, 4])
def test_packer_matches_its_fp64_statement_and_the_documented_layout(n_tail):
    """Integer weights (U in quarters, exact): packer and fp64 statement agree bit for bit, and an element sits where
    include/bts_hip.h says: ((((xi*2 + cb)*2 + half)*64 + lane)*4 + q holds U[xi][16 cb + (lane & 15)][16 half + 4 (lane >> 4) + q];
    (cb*9 + tap)*64 + lane holds w_tail[16 cb + (lane & 15)][tap][lane >> 4], zero for absent slots."""
    g = torch.Generator().manual_seed(11 + n_tail)
    w = torch.randint(-5, 6, (32, 32 + n_tail, 3, 3), generator=g).float()
    (u, t), (ur, tr) = ops.pack_conv_tail_wino(w, n_tail), ops.pack_conv_tail_wino_reference(w, n_tail)
    assert u.dtype == torch.float32 and u.numel() == 16 * 32 * 32 and t.numel() == 2 * 9 * 64
    assert torch.equal(u, ur) and torch.equal(t, tr)
    for flat in torch.randint(0, u.numel(), (300,), generator=g).tolist() + [0, u.numel() - 1]:
        q = flat % 4; r = flat // 4
        lane = r % 64; r //= 64
        half = r % 2; r //= 2
        cb = r % 2; xi = r // 2
        n, c = 16 * cb + (lane & 15), 16 * half + 4 * (lane >> 4) + q
        want = (G @ w[n, c].double() @ G.t())[xi // 4, xi % 4]
        assert float(u[flat]) == float(want), (flat, xi, cb, half, lane, q)
    assert xi == 15
    for flat in range(t.numel()):
        lane = flat % 64; tap = (flat // 64) % 9; cb = flat // 576
        j = lane >> 4
        want = float(w[16 * cb + (lane & 15), 32 + j, tap // 3, tap % 3]) if j < n_tail else 0.0
        assert float(t[flat]) == want, (flat, cb, tap, lane)


def test_packer_float_weights_are_the_fp64_value_rounded_once():
    w = torch.randn((32, 36, 3, 3), generator=torch.Generator().manual_seed(3))
    u, _ = ops.pack_conv_tail_wino(w, 4)
    ur, _ = ops.pack_conv_tail_wino_reference(w, 4)
    # both round one fp64 value; the two fp64 evaluations differ by fp64 rounding only, so at most a last-bit tie flips
    assert float((u - ur).abs().max()) <= 2.0 ** -23 * float(w.abs().max()) * 2.25


def test_packer_rejects_other_shapes():
    for shape, n_tail in (((32, 20, 3, 3), 4), ((16, 36, 3, 3), 4), ((32, 68, 3, 3), 4), ((32, 37, 3, 3), 5), ((32, 36, 1, 1), 4)):
        with pytest.raises(_lib.BtsHipError):
            ops.pack_conv_tail_wino(torch.zeros(shape), n_tail)


@pytest.mark.parametrize("B,h,w,n_tail", [(1, 3, 5, 4), (1, 4, 32, 4), (2, 7, 33, 4), (1, 8, 64, 1), (1, 6, 40, 0), (1, 1, 1, 2), (1, 2, 1, 4)])
def test_formulation_identity_fp64(B, h, w, n_tail):
    """The window-by-window statement (main channels F(2x2,3x3), tail direct) equals F.conv2d in fp64, odd and even maps."""
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn((B, 8, h, w), generator=g, dtype=torch.float64)
    planes = torch.randn((B, n_tail, h, w), generator=g, dtype=torch.float64)
    wt = torch.randn((6, 8 + n_tail, 3, 3), generator=g, dtype=torch.float64)
    ref = F.conv2d(torch.cat([x, planes], 1), wt, padding=1)
    got = ops.conv_tail_wino_reference(x, planes, wt)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_plan_query_eligibility():
    for (h, w) in ((352, 1216), (416, 544)):                     # KITTI and NYU at the declaration bench.py makes
        p = ops.conv_tail_wino_plan(h, w, 32, 32, 4, precision="fp32", fill_frames=16)
        assert p.eligible and (p.bm, p.bn) == (32, 32), (h, w, p)
        assert p.workgroups == ((h + 3) // 4) * ((w + 31) // 32)
        assert not ops.conv_tail_wino_plan(h, w, 32, 32, 4, precision="bf16x3", fill_frames=16).eligible
        assert not ops.conv_tail_wino_plan(h, w, 32, 32, 4, precision="bf16", fill_frames=16).eligible
        assert not ops.conv_tail_wino_plan(h, w, 16, 16, 4, precision="fp32", fill_frames=16).eligible      # bts_size 256
        assert not ops.conv_tail_wino_plan(h, w, 64, 32, 4, precision="fp32", fill_frames=16).eligible
        assert not ops.conv_tail_wino_plan(h, w, 32, 64, 4, precision="fp32", fill_frames=16).eligible
        assert not ops.conv_tail_wino_plan(h, w, 32, 32, 5, precision="fp32", fill_frames=16).eligible
    assert ops.conv_tail_wino_plan(352, 1216, 32, 32, 4, precision=0, fill_frames=1).workgroups == 3344          # one KITTI frame fills the chip
    none = (0, 0, 0)
    assert tuple(ops.conv_tail_wino_plan(64, 96, 32, 32, 4, precision=0, fill_frames=8)) == none      # 48 workgroups per frame
    assert tuple(ops.conv_tail_wino_plan(352, 40, 32, 32, 4, precision=0, fill_frames=4096)) == none  # under-filled grid (0.625)
    with ops.launch_config(fill_frames=16, precision="fp32"):
        assert ops.conv_tail_wino_plan(352, 1216, 32, 32).eligible
    with ops.launch_config(fill_frames=16, precision="bf16"):
        assert not ops.conv_tail_wino_plan(352, 1216, 32, 32).eligible
    with pytest.raises(_lib.BtsHipError):
        ops.conv_tail_wino_plan(352, 1216, 32, 32, 4, precision=0, fill_frames=5000)


def test_entry_point_rejects_bad_arguments_on_the_host():
    """The launch entry point validates before it touches the GPU."""
    f = _lib.load_real().bts_conv_tail_wino_fwd_f32
    a = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails its checks first
    assert f(None, 32, 1, 4, 4, 32, a, a, a, a, a, a, 4, 32, 0, a, None) != 0        # null x
    assert f(a, 32, 1, 4, 4, 32, None, a, a, a, a, a, 4, 32, 0, a, None) != 0        # null u
    assert f(a, 32, 1, 4, 4, 32, a, None, a, a, a, a, 4, 32, 0, a, None) != 0        # null w_tail
    assert f(a, 32, 1, 4, 4, 32, a, a, a, a, a, a, 4, 32, 0, None, None) != 0        # null y
    assert f(a, 32, 1, 4, 4, 32, a, a, a, a, None, a, 4, 32, 0, a, None) != 0        # a declared plane is null
    assert f(a, 16, 1, 4, 4, 32, a, a, a, a, a, a, 4, 32, 0, a, None) != 0           # x stride < 32
    assert f(a, 34, 1, 4, 4, 32, a, a, a, a, a, a, 4, 32, 0, a, None) != 0           # x stride not a multiple of 4
    assert f(a, 32, 1, 4, 4, 32, a, a, a, a, a, a, 5, 32, 0, a, None) != 0           # n_tail 5
    assert f(a, 32, 1, 4, 4, 32, a, a, a, a, a, a, 4, 32, 3, a, None) != 0           # sigmoid is not built
    assert f(a, 16, 1, 4, 4, 16, a, a, a, a, a, a, 4, 16, 0, a, None) != 0           # bts_size 256's conv1
    assert f(a, 64, 1, 4, 4, 64, a, a, a, a, a, a, 4, 32, 0, a, None) != 0           # c_main 64


def test_exports_and_abi_version_unchanged():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    for name in ("bts_conv_tail_wino_fwd_f32", "bts_conv_tail_wino_plan"):      # prototypes: test_host_logic's table-driven test
        assert name in _lib.ABI and re.search(r"\b%s\s*\(" % name, hdr)
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr
    assert "BTS_OP_CONV_TAIL_WINO = 14" in hdr
    from bts_amd import plan
    assert plan._KINDS["bts_conv_tail_wino_fwd_f32"] == (14, "conv_tail_wino")
