"""CPU: host side of the shared-patch F(2x2,2x2) upconv -- weight packer against its fp64 statement, the fp64 identity of
the formulation, the plan query's eligibility answers, and the C-ABI export list."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from bts_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cout,cin", [(32, 32), (64, 96), (128, 64)])
def test_packer_matches_its_fp64_statement_and_the_documented_layout(cout, cin):
    """Integer weights: the fp32 packer and the fp64 reference statement must agree bit for bit; and an element sits where
    include/bts_hip.h says: ((((((xi*nchunks + chunk)*(c_out/32) + ct)*4 + cls)*4 + g)*64 + lh*32 + li)*4 + q holds
    U_cls[xi][n = 32 ct + li][k = 32 chunk + 8 g + 4 lh + q]."""
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randint(-5, 6, (cout, cin, 3, 3), generator=g).float()
    u, ref = ops.pack_upconv_up9(w), ops.pack_upconv_up9_reference(w)
    assert u.dtype == torch.float32 and u.numel() == 36 * cin * cout
    assert torch.equal(u, ref)
    # the layout, from the definition: U_cls = G g_cls G^T with g_cls the pre-summed 2x2 filter of pack_upconv_subpixel
    sub, _, c_in_ld = ops.pack_upconv_subpixel(w)                       # [4][cout_pad][(ty*2+tx)*c_in_ld + c]
    G = torch.tensor([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=torch.float64)
    nchunks, n_ct = cin // 32, cout // 32
    idx = torch.randint(0, u.numel(), (300,), generator=g).tolist() + [0, u.numel() - 1]
    for flat in idx:
        q = flat % 4; r = flat // 4
        li = r % 32; r //= 32
        lh = r % 2; r //= 2
        gi = r % 4; r //= 4
        cls = r % 4; r //= 4
        ct = r % n_ct; r //= n_ct
        chunk = r % nchunks; xi = r // nchunks
        n, k = 32 * ct + li, 32 * chunk + 8 * gi + 4 * lh + q
        g2 = sub[cls, n, :4 * c_in_ld].view(4, c_in_ld)[:, k].view(2, 2).double()
        want = (G @ g2 @ G.t())[xi // 3, xi % 3]
        assert float(u[flat]) == float(want), (flat, xi, chunk, ct, cls, gi, lh, li, q)
    assert xi == 8                                                       # the last element is transform position 8


def test_packer_float_weights_round_like_the_statement():
    """Random float weights: the fp32 sums of at most nine weights stay within a few ulp of the fp64 statement."""
    w = torch.randn((32, 64, 3, 3), generator=torch.Generator().manual_seed(3))
    u, ref = ops.pack_upconv_up9(w), ops.pack_upconv_up9_reference(w)
    assert float((u - ref).abs().max()) <= 8 * 2.0 ** -24 * float(w.abs().max()) * 9


def test_packer_rejects_partial_chunks():
    with pytest.raises(_lib.BtsHipError):
        ops.pack_upconv_up9(torch.zeros(32, 48, 3, 3))
    with pytest.raises(_lib.BtsHipError):
        ops.pack_upconv_up9(torch.zeros(48, 32, 3, 3))


@pytest.mark.parametrize("B,h,w", [(1, 3, 5), (1, 8, 16), (2, 7, 15), (1, 9, 33), (1, 16, 32), (1, 1, 1), (1, 2, 1)])
def test_formulation_identity_fp64(B, h, w):
    """The window-by-window F(2x2,2x2) statement equals conv3x3(nearest2x(x)) in fp64, odd and even maps alike, and
    covers every output pixel exactly once (upconv_up9_reference raises otherwise)."""
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn((B, 8, h, w), generator=g, dtype=torch.float64)
    wt = torch.randn((6, 8, 3, 3), generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    got = ops.upconv_up9_reference(x, wt)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_plan_query_eligibility():
    # the KITTI decoder's upconv3 / 2 / 1 (352x1216) at the declaration bench.py makes
    for (h, w, cin, cout) in ((44, 152, 128, 128), (88, 304, 128, 64), (176, 608, 64, 32)):
        p = ops.upconv_up9_plan(h, w, cin, cout, precision="fp32", fill_frames=16)
        assert p.eligible and (p.bm, p.bn) == (32, 32), (h, w, p)
        assert p.workgroups == ((h // 2 + 1 + 3) // 4) * ((w // 2 + 1 + 7) // 8) * (cout // 32)
        # single-frame declarations keep the sub-pixel halo kernel (and its bits) on every one of them
        assert not ops.upconv_up9_plan(h, w, cin, cout, precision="fp32", fill_frames=1).eligible
        assert not ops.upconv_up9_plan(h, w, cin, cout, precision="fp32", fill_frames=2).eligible
        # non-fp32 arithmetic
        assert not ops.upconv_up9_plan(h, w, cin, cout, precision="bf16x3", fill_frames=16).eligible
        assert not ops.upconv_up9_plan(h, w, cin, cout, precision="bf16", fill_frames=16).eligible
    none = (0, 0, 0)
    assert tuple(ops.upconv_up9_plan(8, 16, 128, 128, precision=0, fill_frames=16)) == none       # small: 4 workgroups per frame
    assert tuple(ops.upconv_up9_plan(11, 38, 128, 128, precision=0, fill_frames=4096)) == none    # under-filled grid (0.625), upconv5's map
    assert tuple(ops.upconv_up9_plan(44, 152, 100, 128, precision=0, fill_frames=16)) == none     # c_in is not whole chunks
    assert tuple(ops.upconv_up9_plan(44, 152, 128, 48, precision=0, fill_frames=16)) == none      # c_out is not whole tiles
    # the default comes from the launch_config in force
    with ops.launch_config(fill_frames=16, precision="fp32"):
        assert ops.upconv_up9_plan(44, 152, 128, 128).eligible
    with ops.launch_config(fill_frames=16, precision="bf16x3"):
        assert not ops.upconv_up9_plan(44, 152, 128, 128).eligible
    with pytest.raises(_lib.BtsHipError):
        ops.upconv_up9_plan(44, 152, 128, 128, precision=0, fill_frames=5000)


def test_entry_point_rejects_bad_arguments_on_the_host():
    """The launch entry point validates before it touches the GPU: null pointers, partial chunks, short strides."""
    lib = _lib.load_real()
    INVALID, UNSUPPORTED = lib.bts_upconv_up9_fwd_f32(None, 32, 1, 4, 4, 32, None, 32, None, None, 0, None, 32, None), None
    assert INVALID != 0
    a = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails its checks first
    UNSUPPORTED = lib.bts_upconv_up9_fwd_f32(a, 48, 1, 4, 4, 48, a, 32, None, None, 0, a, 32, None)
    assert UNSUPPORTED != 0
    assert lib.bts_upconv_up9_fwd_f32(a, 16, 1, 4, 4, 32, a, 32, None, None, 0, a, 32, None) != 0      # x stride < c_in
    assert lib.bts_upconv_up9_fwd_f32(a, 32, 1, 4, 4, 32, a, 32, None, None, 0, a, 16, None) != 0      # y stride < c_out
    assert lib.bts_upconv_up9_fwd_f32(a, 32, 1, 4, 4, 32, a, 32, a, None, 0, a, 32, None) != 0         # half an e2 pair
    assert lib.bts_upconv_up9_fwd_f32(a, 32, 1, 4, 4, 32, a, 32, None, None, 3, a, 32, None) != 0      # sigmoid is not built


def test_exports_and_abi_version_unchanged():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    for name in ("bts_upconv_up9_fwd_f32", "bts_upconv_up9_plan"):              # prototypes: test_host_logic's table-driven test
        assert name in _lib.ABI and re.search(r"\b%s\s*\(" % name, hdr)
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr
    assert "BTS_OP_UPCONV_UP9 = 12" in hdr
    from bts_amd import plan
    assert plan._KINDS["bts_upconv_up9_fwd_f32"] == (12, "upconv_up9")
