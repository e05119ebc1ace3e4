"""CPU: host side of the planar-tail convolution with bf16 main operands (bts_conv_tail_bf16_fwd_f32) -- the C-ABI export
list and prototypes, every validation error of the entry point, the plan query's answers, and the weight packer against a
torch statement."""
import ctypes
import os
import re

import pytest
import torch

from bts_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("bts_conv_tail_bf16_fwd_f32", "bts_conv_tail_bf16_plan")


def _header():
    return open(os.path.join(ROOT, "include", "bts_hip.h")).read()


def test_exports_prototypes_and_abi_version_unchanged():
    """(The prototypes themselves: test_host_logic.test_abi_table_matches_every_header_prototype.)"""
    hdr = _header()
    lib = _lib.load_real()
    for name in NAMES:
        assert name in _lib.ABI and re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr
    assert lib.bts_hip_abi_version() == 17
    assert "BTS_OP_CONV_TAIL_BF16 = 13" in hdr
    from bts_amd import plan
    assert plan._KINDS["bts_conv_tail_bf16_fwd_f32"] == (13, "conv_tail_bf16")
    # the plan query is a pure host query: a recording hands out the real function, not a recorder
    rec = plan._Recorder()
    proxy = plan._Proxy(lib, rec)
    assert proxy.bts_conv_tail_bf16_plan is lib.bts_conv_tail_bf16_plan
    bn, wgs = ctypes.c_int(0), ctypes.c_long(0)
    assert proxy.bts_conv_tail_bf16_plan(88, 304, 224, 128, 1, 16, ctypes.byref(bn), ctypes.byref(wgs)) == 0
    assert rec.calls == [] and rec.foreign == []


def _call(**kw):
    """The entry point with fake pointers (never dereferenced: every call fails a check first) and one field changed."""
    a = ctypes.c_void_p(4096)
    args = dict(x=a, x_pix_stride=64, B=1, h=8, w=32, c_main=64, w_main=a, w_tail=a, tail=a, n_tail=1, c_out=64, c_out_pad=64,
                e2_scale=None, e2_shift=None, act=2, y=a, y_pix_stride=64)
    args.update(kw)
    order = ("x", "x_pix_stride", "B", "h", "w", "c_main", "w_main", "w_tail", "tail", "n_tail", "c_out", "c_out_pad", "e2_scale",
             "e2_shift", "act", "y", "y_pix_stride")
    return _lib.load_real().bts_conv_tail_bf16_fwd_f32(*[args[k] for k in order], None)


@pytest.mark.parametrize("kw,code", [
    (dict(x=None), INVALID), (dict(w_main=None), INVALID), (dict(w_tail=None), INVALID), (dict(tail=None), INVALID),
    (dict(y=None), INVALID),
    (dict(B=0), INVALID), (dict(h=0), INVALID), (dict(c_out=0), INVALID),
    (dict(c_main=48, x_pix_stride=48), UNSUPPORTED),                   # no whole 32-channel chunks
    (dict(c_out_pad=48), INVALID), (dict(c_out_pad=32), INVALID),      # not a multiple of 32; smaller than c_out
    (dict(x_pix_stride=32), INVALID),                                  # x stride < c_main
    (dict(x_pix_stride=66), INVALID),                                  # x stride no multiple of 4
    (dict(y_pix_stride=32), INVALID),                                  # y stride < c_out
    (dict(w_main=ctypes.c_void_p(4096 + 8)), INVALID),                 # w_main not 16-byte aligned
    (dict(x=ctypes.c_void_p(4096 + 4)), INVALID),
    (dict(tail=ctypes.c_void_p(4096 + 2)), INVALID),                   # plane not 4-byte aligned
    (dict(n_tail=2), UNSUPPORTED), (dict(n_tail=4), UNSUPPORTED), (dict(n_tail=0), INVALID), (dict(n_tail=5), INVALID),
    (dict(act=3), INVALID), (dict(act=-1), INVALID),                   # sigmoid is not built
    (dict(e2_scale=ctypes.c_void_p(4096)), INVALID), (dict(e2_shift=ctypes.c_void_p(4096)), INVALID),      # half an e2 pair
])
def test_entry_point_rejects_bad_arguments_on_the_host(kw, code):
    assert _call(**kw) == code, kw


def test_a_plane_at_a_4_byte_offset_is_accepted_by_the_alignment_check():
    """4-byte alignment is all the plane needs: a 4-byte offset passes that check (the call then fails a later one)."""
    assert _call(tail=ctypes.c_void_p(4096 + 4), act=3) == INVALID
    assert _call(tail=ctypes.c_void_p(4096 + 4), n_tail=2) == UNSUPPORTED


LAYERS = [   # (h, w, c_main, c_out): conv3 / conv2 of DenseNet161 at 352x1216 and of ResNeXt101 at 416x544
    (88, 304, 224, 128), (176, 608, 160, 64), (104, 136, 384, 128), (208, 272, 128, 64),
]


def test_plan_query():
    for h, w, c_main, c_out in LAYERS:
        p = ops.conv_tail_bf16_plan(h, w, c_main, c_out, 1, fill_frames=16)
        bn = 128 if c_out >= 128 else 64
        assert p.eligible and p.bn == bn, (h, w, c_main, c_out, tuple(p))
        assert p.workgroups == 16 * ((h + 3) // 4) * ((w + 31) // 32) * ((c_out + bn - 1) // bn)
        none = (0, 0)
        assert tuple(ops.conv_tail_bf16_plan(h, w, 48, c_out, 1, fill_frames=16)) == none            # c_main: no whole chunks
        assert tuple(ops.conv_tail_bf16_plan(h, w, c_main, c_out, 2, fill_frames=16)) == none        # two planes are not built
        assert tuple(ops.conv_tail_bf16_plan(h, w, c_main, 32, 1, fill_frames=16)) == none           # narrower than a tile
    assert tuple(ops.conv_tail_bf16_plan(22, 76, 224, 128, 1, fill_frames=16)) == (0, 0)            # 4x32 grid 0.72 real pixels
    assert ops.conv_tail_bf16_plan(16, 32, 64, 64, 1, fill_frames=16).eligible                       # full tiles, small map
    # the default comes from the launch_config in force
    with ops.launch_config(fill_frames=16, precision="bf16"):
        assert tuple(ops.conv_tail_bf16_plan(88, 304, 224, 128)) == tuple(ops.conv_tail_bf16_plan(88, 304, 224, 128, 1, fill_frames=16))
    with pytest.raises(_lib.BtsHipError):
        ops.conv_tail_bf16_plan(88, 304, 224, 128, 1, fill_frames=5000)


def test_plan_answer_does_not_depend_on_the_batch():
    """The query takes no batch at all; and what a model asks inside its own scope with fill_frames pinned is the same
    answer whatever batch it was called with (ops.model_launch_config)."""
    class M:
        fill_frames, conv_precision = 16, "bf16"
    for h, w, c_main, c_out in LAYERS:
        answers = set()
        for batch in (1, 2, 3, 8, 16, 64):
            with ops.model_launch_config(M, batch):
                answers.add(tuple(ops.conv_tail_bf16_plan(h, w, c_main, c_out)))
        assert len(answers) == 1 and answers.pop()[0] > 0


@pytest.mark.parametrize("cout,c_main", [(64, 32), (96, 64), (40, 96), (128, 224)])
def test_packer_against_a_torch_statement(cout, c_main):
    g = torch.Generator().manual_seed(cout * 7 + c_main)
    w = torch.randn((cout, c_main + 1, 3, 3), generator=g) * 0.37
    w_main, w_tail = ops.pack_conv_tail_bf16(w, 1)
    cout_pad = (cout + 31) // 32 * 32
    assert w_main.dtype == torch.bfloat16 and tuple(w_main.shape) == (cout_pad, 9 * c_main) and w_main.is_contiguous()
    assert w_tail.dtype == torch.float32 and tuple(w_tail.shape) == (cout_pad, 9, 4) and w_tail.is_contiguous()
    rounded = w[:, :c_main].to(torch.bfloat16)                                  # [cout, c, ky, kx], round to nearest even
    assert not torch.equal(rounded.float(), w[:, :c_main])                      # the rounding is a real one
    for tap in range(9):
        want = rounded[:, :, tap // 3, tap % 3]                                 # k = tap * c_main + c
        assert torch.equal(w_main[:cout, tap * c_main:(tap + 1) * c_main].view(torch.int16), want.contiguous().view(torch.int16)), tap
        assert torch.equal(w_tail[:cout, tap, 0].view(torch.int32), w[:, c_main, tap // 3, tap % 3].contiguous().view(torch.int32)), tap
    assert int((w_main[cout:].view(torch.int16) != 0).sum()) == 0               # pad rows
    assert int((w_tail[cout:].view(torch.int32) != 0).sum()) == 0
    assert int((w_tail[:, :, 1:].view(torch.int32) != 0).sum()) == 0            # unused plane slots


def test_packer_rejects_what_the_kernel_does_not_take():
    with pytest.raises(_lib.BtsHipError):
        ops.pack_conv_tail_bf16(torch.zeros(64, 49, 3, 3), 1)                   # 48 main channels
    with pytest.raises(_lib.BtsHipError):
        ops.pack_conv_tail_bf16(torch.zeros(64, 33, 1, 1), 1)
    with pytest.raises(_lib.BtsHipError):
        ops.pack_conv_tail_bf16(torch.zeros(64, 33, 3, 3), 0)


def test_model_switch_defaults_off_and_reaches_the_decoder():
    from types import SimpleNamespace
    from parity_util import Params
    from bts_amd import synth
    from bts_amd.bts import BtsModel, bts
    dec = bts(Params("densenet161_bts", 512, 80.0, "kitti"), synth.ENCODER_CHANNELS["densenet161_bts"], 512)
    assert dec.bf16_tail_convs is False
    m = SimpleNamespace(decoder=dec)                         # the property only reaches for the model's decoder
    assert isinstance(BtsModel.bf16_tail_convs, property) and BtsModel.bf16_tail_convs.fget(m) is False
    BtsModel.bf16_tail_convs.fset(m, 1)
    assert dec.bf16_tail_convs is True and BtsModel.bf16_tail_convs.fget(m) is True
    # the packs exist for both layers of this channel plan (224 and 160 main channels) and hold the documented shapes
    packs = dec.packed_tail_bf16()
    assert sorted(packs) == ["conv2", "conv3"]
    assert tuple(packs["conv3"][0].shape) == (128, 9 * 224) and tuple(packs["conv2"][0].shape) == (64, 9 * 160)
    assert dec.packed_tail_bf16() is packs                   # cached until the weights change
    with torch.no_grad():
        dec.conv3[0].weight.add_(1.0)
    assert dec.packed_tail_bf16() is not packs
