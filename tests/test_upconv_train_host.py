"""CPU: host side of the sub-pixel upconv training path -- the fp64 statement of its three passes against torch
autograd, the entry points' argument checks, the weight-gradient plan query over tests/upconv_train_cases.py, and the
C-ABI export list."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import upconv_train_cases as uc
from bts_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B,cin,cout,h,w", [(2, 5, 3, 4, 6), (3, 8, 40, 5, 7), (1, 4, 12, 1, 1), (2, 12, 36, 3, 9)])
def test_reference_statement_equals_autograd_fp64(B, cin, cout, h, w):
    """Forward, input gradient and weight gradient of the sub-pixel statement == autograd of
    conv2d(interpolate(x, 2, 'nearest'), w, padding=1) in fp64: odd maps, B > 1, c_out not a multiple of 32."""
    g = torch.Generator().manual_seed(1000 * h + w)
    x = torch.randn((B, cin, h, w), generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((B, cout, 2 * h, 2 * w), generator=g, dtype=torch.float64)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    y.backward(dy)
    ry, rdx, rdw = ops.upconv_subpixel_grads_reference(x, wt, dy)
    for got, ref, what in ((ry, y.detach(), "forward"), (rdx, x.grad, "input gradient"), (rdw, wt.grad, "weight gradient")):
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), what


def test_dgrad_pack_statement_holds_the_documented_elements():
    """[c][(4r+s)*c_out + n] = K[r,s][c][n] with K[3-py-2ty, 3-px-2tx] = g_(py,px)[ty,tx]^T; (py,ty) -> r is a bijection."""
    assert sorted(3 - py - 2 * ty for py in (0, 1) for ty in (0, 1)) == [0, 1, 2, 3]
    g = torch.Generator().manual_seed(5)
    w = torch.randint(-5, 6, (8, 12, 3, 3), generator=g).float()
    pack = ops.pack_upconv_dgrad_reference(w)
    assert tuple(pack.shape) == ops.upconv_train_pack_shapes(8, 12)[1] == (32, 128)
    S = {p: torch.tensor(ops._SUBPIX_S[p]) for p in (0, 1)}
    seen = 0
    for py in (0, 1):
        for px in (0, 1):
            gc = torch.einsum("ta,ncab,ub->nctu", S[py], w, S[px])
            for ty in (0, 1):
                for tx in (0, 1):
                    rs = 4 * (3 - py - 2 * ty) + (3 - px - 2 * tx)
                    assert torch.equal(pack[:12, rs * 8:(rs + 1) * 8], gc[:, :, ty, tx].t())
                    seen += 1
    assert seen == 16 and float(pack[12:].abs().max()) == 0.0
    # and the convolution it drives: a 4x4 / stride-2 / padding-1 convolution over dy is the input gradient
    dy = torch.randn((2, 8, 6, 10), generator=g, dtype=torch.float64)
    K = pack[:12, :128].double().view(12, 4, 4, 8).permute(0, 3, 1, 2)          # [c_in][c_out][r][s]
    _, rdx, _ = ops.upconv_subpixel_grads_reference(torch.zeros(2, 12, 3, 5), w, dy)
    assert float((F.conv2d(dy, K, stride=2, padding=1) - rdx).abs().max()) <= 1e-12 * float(rdx.abs().max())


def test_entry_points_reject_bad_arguments_on_the_host():
    """Every new entry point validates before it touches the GPU (every call below fails its checks first)."""
    lib = _lib.load_real()
    a, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    dg, wg = lib.bts_upconv_dgrad_f32, lib.bts_upconv_wgrad_f32
    # dgrad(dy, dy_stride, B, h, w, c_out, w_dgrad, c_in, dx, dx_stride, precision, fill, ws, ws_floats, stream)
    assert dg(None, 32, 1, 4, 4, 32, a, 32, a, 32, 0, 0, None, 0, None) != 0          # null dy
    assert dg(a, 32, 1, 4, 4, 32, None, 32, a, 32, 0, 0, None, 0, None) != 0          # null weights
    assert dg(a, 32, 1, 4, 4, 32, a, 32, None, 32, 0, 0, None, 0, None) != 0          # null dx
    assert dg(a, 32, 1, 4, 4, 30, a, 32, a, 32, 0, 0, None, 0, None) != 0             # c_out % 4
    assert dg(a, 32, 1, 4, 4, 32, a, 30, a, 32, 0, 0, None, 0, None) != 0             # c_in % 4
    assert dg(a, 16, 1, 4, 4, 32, a, 32, a, 32, 0, 0, None, 0, None) != 0             # dy stride < c_out
    assert dg(a, 32, 1, 4, 4, 32, a, 32, a, 16, 0, 0, None, 0, None) != 0             # dx stride < c_in
    assert dg(odd, 32, 1, 4, 4, 32, a, 32, a, 32, 0, 0, None, 0, None) != 0           # misaligned dy
    assert dg(a, 32, 1, 4, 4, 32, a, 32, a, 32, 0, 0, a, 0, None) != 0                # a workspace of 0 floats
    assert dg(a, 32, 1, 4, 4, 32, a, 32, a, 32, 0, 0, odd, 1 << 20, None) != 0        # misaligned workspace
    assert dg(a, 32, 0, 4, 4, 32, a, 32, a, 32, 0, 0, None, 0, None) != 0             # B = 0
    assert dg(a, 32, 1, 4, 4, 32, a, 32, a, 32, 7, 0, None, 0, None) != 0             # precision out of range
    # wgrad(x, x_stride, B, h, w, c_in, dy, dy_stride, c_out, dw, ws, ws_floats, stream)
    need = 16 * 32 * 32
    assert wg(None, 32, 1, 4, 4, 32, a, 32, 32, a, a, need, None) != 0                # null x
    assert wg(a, 32, 1, 4, 4, 32, None, 32, 32, a, a, need, None) != 0                # null dy
    assert wg(a, 32, 1, 4, 4, 32, a, 32, 32, None, a, need, None) != 0                # null dw
    assert wg(a, 32, 1, 4, 4, 32, a, 32, 32, a, None, need, None) != 0                # the workspace is mandatory
    assert wg(a, 32, 1, 4, 4, 32, a, 32, 32, a, a, need - 1, None) != 0               # short workspace
    assert wg(a, 32, 1, 4, 4, 30, a, 32, 32, a, a, need, None) != 0                   # c_in % 4
    assert wg(a, 32, 1, 4, 4, 32, a, 32, 30, a, a, need, None) != 0                   # c_out % 4
    assert wg(a, 16, 1, 4, 4, 32, a, 32, 32, a, a, need, None) != 0                   # x stride < c_in
    assert wg(a, 32, 1, 4, 4, 32, a, 16, 32, a, a, need, None) != 0                   # dy stride < c_out
    assert wg(a, 32, 1, 4, 4, 32, a, 32, 32, a, odd, need, None) != 0                 # misaligned workspace
    assert wg(a, 32, 1, 4, 4, 32, odd, 32, 32, a, a, need, None) != 0                 # misaligned dy
    # the plan queries reject what the launches reject
    i, l = ctypes.c_int(0), ctypes.c_long(0)
    assert lib.bts_upconv_wgrad_plan_f32(1, 4, 4, 32, 32, need - 1, i, i, l, l) != 0
    assert lib.bts_upconv_wgrad_plan_f32(1, 4, 4, 30, 32, need, i, i, l, l) != 0
    assert lib.bts_upconv_wgrad_plan_f32(1, 4, 4, 32, 32, need, None, None, None, None) == 0      # outputs are optional
    assert lib.bts_upconv_dgrad_plan(1, 4, 4, 30, 32, 0, 0, 0, i, i, i) != 0
    assert lib.bts_upconv_dgrad_plan(1, 4, 4, 32, 32, 0, 0, 0, None, i, i) != 0
    # pack: null table, no entries, no blocks
    assert lib.bts_upconv_train_pack_f32(None, 1, 1, None) != 0
    assert lib.bts_upconv_train_pack_f32(a, 0, 1, None) != 0
    assert lib.bts_upconv_train_pack_f32(a, 1, 0, None) != 0
    assert lib.bts_upconv_train_pack_blocks(32, 32, 32, 32) == 2                 # 5 * 1024 floats, 4096 per block
    # the Python wrappers refuse CPU tensors (no fallback)
    with pytest.raises(_lib.BtsHipError):
        ops.upconv_wgrad(torch.zeros(16, 32), 1, 4, 4, 32, torch.zeros(64, 32), 32, torch.zeros(need))
    with pytest.raises(_lib.BtsHipError):
        ops.upconv_dgrad(torch.zeros(64, 32), 1, 4, 4, torch.zeros(32, 512), 32, 32, torch.zeros(16, 32))


def test_conv_fwd_still_refuses_even_kernel_sizes():
    """The 4x4 gather is reached from bts_upconv_dgrad_f32 only: bts_conv_plan_f32's accept set stays odd ksize."""
    from bts_amd import conv_plan
    d = conv_plan.geometry_desc(1, 8, 10, 32, 32, 4, stride=2, pad=1, fake_pointers=True)
    assert conv_plan.query(d).rc != 0
    bm, bn, kind, splitk = ops.upconv_dgrad_plan(1, 4, 5, 32, 32)
    assert kind == conv_plan.Family.ROW and bm in (64, 128) and bn == 32 and not splitk


def test_dgrad_plan_confirms_the_split_k_case():
    B, h, w, cin, cout = uc.DGRAD_CASES[-1]
    assert ops.upconv_dgrad_plan(B, h, w, cout, cin, uc.DGRAD_SPLITK_WS)[3]
    assert not ops.upconv_dgrad_plan(B, h, w, cout, cin, 0)[3]                    # no workspace, no split


@pytest.mark.parametrize("c", uc.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_plan_of_every_case(c):
    bm, bn, split, pps = uc.plan_of(c)
    M = c.B * c.h * c.w
    assert (bm, bn) == c.tile and (split > 1) == c.split, (c.name, bm, bn, split)
    assert pps % 32 == 0 and (split - 1) * pps < M <= split * pps
    assert split * 16 * c.c_out * c.c_in <= c.ws_floats                           # what the launch writes fits


def test_wgrad_case_table_reaches_every_tile_split_and_unsplit():
    reached = {(uc.plan_of(c)[:2], uc.plan_of(c)[2] > 1) for c in uc.WGRAD_CASES}
    for tile in ((128, 128), (64, 128), (32, 128), (64, 64)):
        for split in (False, True):
            assert (tile, split) in reached, "no case runs the %dx%d tile %s" % (tile + ("split" if split else "unsplit",))
    assert {uc.BY_NAME[n].tile for n in uc.WGRAD_FLOAT_CASES} == {(128, 128), (64, 128), (32, 128), (64, 64)}


def test_exports_bindings_and_abi_version():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    names = ("bts_upconv_dgrad_f32", "bts_upconv_dgrad_plan", "bts_upconv_wgrad_f32", "bts_upconv_wgrad_plan_f32",
             "bts_upconv_train_pack_blocks", "bts_upconv_train_pack_f32")
    lib = _lib.load_real()
    for name in names:                        # the prototypes themselves: test_host_logic's table-driven test
        assert name in _lib.ABI and re.search(r"\b%s\s*\(" % name, hdr), name
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr and lib.bts_hip_abi_version() == 17
    # host-only queries pass through a plan recording untouched; the launches are foreign to a recorded forward
    from bts_amd import plan
    rec = plan._Recorder()
    proxy = plan._Proxy(lib, rec)
    for name in ("bts_upconv_dgrad_plan", "bts_upconv_wgrad_plan_f32", "bts_upconv_train_pack_blocks"):
        assert _lib.ABI[name].role == _lib.QUERY and name not in plan._KINDS
        assert getattr(proxy, name) is getattr(lib, name), name
    for name in ("bts_upconv_dgrad_f32", "bts_upconv_wgrad_f32", "bts_upconv_train_pack_f32"):
        assert _lib.ABI[name].role == _lib.LAUNCH and name not in plan._KINDS
        assert getattr(proxy, name) is not getattr(lib, name), name
    assert rec.calls == [] and rec.foreign == []


def test_switch_defaults_off():
    from bts_amd import bts as M
    from bts_amd import synth
    from parity_util import CONFIGS, Params
    enc, md, ds, _, _ = CONFIGS["K"]
    dec = M.bts(Params(enc, 512, md, ds), synth.ENCODER_CHANNELS[enc], 512)
    assert dec.subpixel_upconv_train is False
    assert isinstance(M.BtsModel.subpixel_upconv_train, property)
