"""CPU: host side of the native grouped 3x3 training path (csrc/conv_grouped_wgrad.inc, pack.hip gmode 3 / 4) -- the two
per-step packed layouts against their index-by-index statement, the weight-gradient plan query, argument checks of the
entry point, the C-ABI export list and the model switch."""
import ctypes
import os
import re

import pytest
import torch

from bts_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c,groups", [(64, 4), (64, 8), (64, 16), (128, 32), (192, 12)])
def test_train_pack_layouts_match_the_forward_layout(c, groups):
    """The forward pack is the inference layout of w; the input-gradient pack is the inference layout of the flipped,
    group-transposed weight w_t[cg g + i][o][8 - tap] = w[cg g + o][i][tap], built here entry by entry."""
    cg = c // groups
    g = torch.Generator().manual_seed(3 * c + groups)
    w = torch.randint(1, 99, (c, cg, 3, 3), generator=g).float()          # no zero weight: a 0 in the pack is structural
    fwd = ops.pack_grouped_train_reference(w, groups, dgrad=False)
    assert torch.equal(fwd, ops.pack_grouped_native_reference(w, groups))
    w_t = torch.empty_like(w)
    for grp in range(groups):
        for o in range(cg):
            for i in range(cg):
                w_t[cg * grp + i, o] = w[cg * grp + o, i].flatten().flip(0).view(3, 3)
    assert torch.equal(ops.grouped_dgrad_weight(w, groups), w_t)
    dg = ops.pack_grouped_train_reference(w, groups, dgrad=True)
    assert torch.equal(dg, ops.pack_grouped_native_reference(w_t, groups))
    assert int((dg == 0).sum()) == 144 * c - 9 * c * cg                   # cross-group entries, and only they, are zero
    assert not torch.equal(dg, fwd)


def test_train_pack_rows_are_one_table_row_per_weight():
    """WeightPacker describes a native pack as ONE row of the bts_pack_weights_f32 table (gmode 3 / 4, 144 c floats) and
    leaves the rows of the bundle modes as they were."""
    from bts_amd.train import WeightPacker as P
    w = torch.zeros(256, 8, 3, 3)
    for mode, gmode in ((P.FWD_NATIVE, 3), (P.DGRAD_NATIVE, 4)):
        rows, shape = P._rows(w, 0, mode, 32)
        assert shape == (144 * 256,) and len(rows) == 1
        so, do, _, _, k, _, rows_pad, k_pad, _, _, _, cg, gm = rows[0]
        assert (so, do, k, rows_pad * k_pad, cg, gm) == (0, 0, 3, 144 * 256, 8, gmode)
    rows, shape = P._rows(w, 32, P.FWD, 32)
    assert shape == (8, 32, 288) and [r[12] for r in rows] == [1] * 8
    rows, shape = P._rows(w, 32, P.DGRAD, 32)
    assert [r[12] for r in rows] == [2] * 8
    for bad, groups in ((torch.zeros(256, 32, 3, 3), 8), (torch.zeros(96, 8, 3, 3), 12), (torch.zeros(64, 8, 1, 1), 8)):
        with pytest.raises(_lib.BtsHipError, match="native pack"):
            P._rows(bad, 0, P.FWD_NATIVE, groups)


def test_native_layer_rule_is_a_shape_rule():
    from bts_amd import train
    f = train._grouped_native_layer
    assert f(True, 256, 32, 3, 1, 1, 1) and f(True, 128, 32, 3, 1, 1, 1) and f(True, 512, 32, 3, 1, 1, 1)
    assert not f(False, 256, 32, 3, 1, 1, 1)
    assert not f(True, 256, 32, 3, 2, 1, 1)               # stride 2
    assert not f(True, 1024, 32, 3, 1, 1, 1)              # 32 channels per group
    assert not f(True, 2048, 32, 3, 1, 1, 1)              # 64
    assert not f(True, 256, 32, 3, 1, 2, 2)               # dilated
    assert not f(True, 256, 32, 1, 1, 0, 1)
    with ops.launch_config(precision="bf16x3"):
        assert not f(True, 256, 32, 3, 1, 1, 1)


def test_wgrad_plan_query():
    """Deterministic in its arguments, unsplit without workspace, never more workspace than given, the documented rule."""
    q = ops.conv_grouped_wgrad_plan
    per = 144 * 256
    assert q(3, 35, 250, 256, 16, 48 << 20) == q(3, 35, 250, 256, 16, 48 << 20) == (120, 120 * per)   # 240 tiles, 128 wanted, 2 each
    assert q(3, 35, 250, 256, 16, 0) == (1, 0)
    assert q(3, 35, 250, 256, 16, 2 * per - 1) == (1, 0)                   # room for fewer than two partials
    assert q(3, 35, 250, 256, 16, 2 * per) == (2, 2 * per)
    for ws in (0, 1, per, 3 * per + 5, 50 * per, 119 * per, 1 << 40):
        s, used = q(3, 35, 250, 256, 16, ws)
        assert 1 <= s <= 120 and used <= ws and used == (s * per if s > 1 else 0)
    assert q(1, 1, 1, 64, 16, 48 << 20) == (1, 0)                          # one tile
    assert q(4, 88, 176, 256, 32, 48 << 20) == (121, 121 * per)            # 484 tiles in 128 wanted -> 4 each -> 121
    assert q(4, 22, 44, 1024, 64, 48 << 20) == (18, 18 * 144 * 1024)       # 36 tiles, 32 wanted -> 2 each
    for shape in ((2, 8, 8, 96, 12), (2, 8, 8, 64, 2), (2, 8, 8, 64, 32), (2, 8, 8, 2048, 32)):
        with pytest.raises(_lib.BtsHipError, match="not built"):
            q(*shape, 1 << 20)
    lib = _lib.load_real()
    s, used = ctypes.c_int(0), ctypes.c_long(0)
    assert lib.bts_conv_grouped_wgrad_plan(2, 8, 8, 64, 4, 0, None, ctypes.byref(used)) != 0
    assert lib.bts_conv_grouped_wgrad_plan(2, 8, 8, 64, 4, -1, ctypes.byref(s), ctypes.byref(used)) != 0
    assert lib.bts_conv_grouped_wgrad_plan(32768, 512, 512, 64, 4, 0, ctypes.byref(s), ctypes.byref(used)) != 0   # 2^33 pixels


def test_wgrad_entry_point_rejects_bad_arguments_on_the_host():
    """The launch entry point validates before it touches the GPU."""
    lib = _lib.load_real()
    f = lib.bts_conv_grouped_wgrad_f32
    a = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails its checks first
    INVALID, UNSUPPORTED = f(None, 64, a, 64, 1, 4, 4, 64, 4, a, None, 0, None), f(a, 96, a, 96, 1, 4, 4, 96, 12, a, None, 0, None)
    assert INVALID != 0 and UNSUPPORTED != 0 and INVALID != UNSUPPORTED                       # null x; c % 64 != 0
    assert f(a, 64, None, 64, 1, 4, 4, 64, 4, a, None, 0, None) == INVALID                    # null dy
    assert f(a, 64, a, 64, 1, 4, 4, 64, 4, None, None, 0, None) == INVALID                    # null dw
    assert f(a, 32, a, 64, 1, 4, 4, 64, 4, a, None, 0, None) == INVALID                       # x stride < c
    assert f(a, 64, a, 66, 1, 4, 4, 64, 4, a, None, 0, None) == INVALID                       # dy stride not a multiple of 4
    assert f(ctypes.c_void_p(4100), 64, a, 64, 1, 4, 4, 64, 4, a, None, 0, None) == INVALID   # x not 16-byte aligned
    assert f(a, 64, a, 64, 1, 4, 4, 64, 4, a, ctypes.c_void_p(4100), 1 << 20, None) == INVALID   # ws not 16-byte aligned
    assert f(a, 64, a, 64, 1, 4, 4, 64, 4, a, a, -1, None) == INVALID
    assert f(a, 64, a, 64, 0, 4, 4, 64, 4, a, None, 0, None) == INVALID                       # B 0
    assert f(a, 64, a, 64, 1, 4, 4, 64, 5, a, None, 0, None) == INVALID                       # c % groups
    assert f(a, 64, a, 64, 1, 4, 4, 64, 2, a, None, 0, None) == UNSUPPORTED                   # 32 channels per group
    assert f(a, 64, a, 64, 32768, 512, 512, 64, 4, a, None, 0, None) == UNSUPPORTED           # 2^33 pixels
    with pytest.raises(_lib.BtsHipError):                                                     # no CPU fallback
        ops.conv_grouped_wgrad(torch.zeros(16, 64), 1, 4, 4, torch.zeros(16, 64), 64, 4)


def test_exports_and_abi_version_unchanged():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    lib = _lib.load_real()
    for name in ("bts_conv_grouped_wgrad_f32", "bts_conv_grouped_wgrad_plan"):
        assert name in _lib.ABI and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name)
    assert _lib.ABI["bts_conv_grouped_wgrad_f32"].role == _lib.LAUNCH and _lib.ABI["bts_conv_grouped_wgrad_plan"].role == _lib.QUERY
    assert len(_lib.ABI["bts_conv_grouped_wgrad_f32"].argtypes) == 13 and len(_lib.ABI["bts_conv_grouped_wgrad_plan"].argtypes) == 8
    assert _lib.ABI["bts_conv_grouped_wgrad_f32"].plan is None
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr and lib.bts_hip_abi_version() == 17
    from bts_amd import conv_plan
    assert [conv_plan.grouped_wgrad_kernel_name(cg) for cg in (4, 8, 16)] == ["conv_grouped_wgrad_kernel<%d>" % cg for cg in (4, 8, 16)]


def test_model_attribute_defaults_to_bundles():
    import inspect
    from bts_amd import bts as M, train
    from parity_util import Params
    m = M.BtsModel(Params("resnext50_bts", 512, 10.0, "nyu"))
    assert m.grouped_conv_train is False and m.encoder.grouped_conv_train is False and m.grouped_conv == "bundles"
    m.grouped_conv_train = True
    assert m.encoder.grouped_conv_train is True and m.grouped_conv == "bundles"
    assert inspect.signature(train.conv2d).parameters["grouped_native"].default is False
