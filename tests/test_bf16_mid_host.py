"""CPU: host side of the bf16-resident bottleneck intermediate (``BtsModel.bf16_mid_storage``) -- the three new
C-ABI symbols (bts_conv1x1_bf16_fwd_bf16, bts_conv3x3_bf16in_fwd_f32, bts_conv3x3_bf16in_plan), their argument checks (made
before any GPU work, so never-dereferenced pointers do), the consumer query against bts_conv_plan_f32's own answer, and the
model attribute's validation."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from bts_amd import _lib, conv_plan, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROD, CONS, PLAN = "bts_conv1x1_bf16_fwd_bf16", "bts_conv3x3_bf16in_fwd_f32", "bts_conv3x3_bf16in_plan"


def test_exports_and_abi_version_unchanged():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    lib = _lib.load_real()
    from bts_amd import plan
    for name in (PROD, CONS, PLAN):
        assert name in _lib.ABI and re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert _lib.ABI[name].plan is None and name not in plan._KINDS, name      # a foreign launch to the plan recorder
    assert _lib.ABI[PROD].role == _lib.LAUNCH and _lib.ABI[CONS].role == _lib.LAUNCH and _lib.ABI[PLAN].role == _lib.QUERY
    # the producer has the fp32 entry point's prototype (y a void pointer), the consumer 15 arguments and the stream
    assert _lib.ABI[PROD].argtypes == _lib.ABI["bts_conv1x1_bf16_fwd_f32"].argtypes
    assert len(_lib.ABI[CONS].argtypes) == 16 and len(_lib.ABI[PLAN].argtypes) == 7
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr and lib.bts_hip_abi_version() == 17
    assert conv_plan.wide_1x1_bf16_kernel_name(192, True) == "conv1x1_bf16_ybf16_kernel<192>"
    assert conv_plan.wide_1x1_bf16_kernel_name(192) == "conv1x1_bf16_kernel<192>"
    assert conv_plan.bf16in_3x3_kernel_name(64) == "conv3x3_bf16in_kernel<64>"
    assert [conv_plan.bf16in_3x3_tile(c) for c in (32, 48, 64, 96, 128, 192, 256)] == [64, 64, 64, 64, 128, 64, 128]


A = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails its checks first


def P(v):
    return ctypes.c_void_p(v)


# ------------------------------------------------------------------------------------------------------------ the producer
PGOOD = dict(x=A, xs=96, npix=300, c_in=48, w=A, k_pad=64, c_out=192, c_out_pad=192, ps=A, pb=A, pre_relu=1, es=A, eb=A, act=1,
             y=A, ys=192)


def _prod(entry=PROD, **kw):
    a = dict(PGOOD, **kw)
    return getattr(_lib.load_real(), entry)(a["x"], a["xs"], a["npix"], a["c_in"], a["w"], a["k_pad"], a["c_out"], a["c_out_pad"],
                                            a["ps"], a["pb"], a["pre_relu"], a["es"], a["eb"], a["act"], a["y"], a["ys"], None)


INVALID, UNSUPPORTED = _prod(x=None), _prod(c_out=128, c_out_pad=128, ys=128)


def test_the_two_codes_are_the_fp32_entry_points():
    assert INVALID != 0 and UNSUPPORTED != 0 and INVALID != UNSUPPORTED
    assert _prod("bts_conv1x1_bf16_fwd_f32", x=None) == INVALID
    assert _prod("bts_conv1x1_bf16_fwd_f32", c_out=128, c_out_pad=128, ys=128) == UNSUPPORTED


PRODUCER_REJECTS = [
    (dict(x=None), "I"), (dict(w=None), "I"), (dict(y=None), "I"),                                 # null operands
    (dict(ps=None), "I"), (dict(pb=None), "I"), (dict(es=None), "I"), (dict(eb=None), "I"),        # half a pair
    (dict(xs=32), "I"), (dict(ys=128), "I"),                                                       # strides < c_in / < c_out
    (dict(xs=98), "I"), (dict(ys=194), "I"),                                                       # strides not multiples of 4
    (dict(x=P(4100)), "I"), (dict(w=P(4104)), "I"), (dict(ps=P(4097)), "I"),                       # x / w / a vector misaligned
    (dict(act=3), "I"), (dict(act=-1), "I"), (dict(npix=0), "I"), (dict(npix=-5), "I"),
    (dict(c_out_pad=160), "I"),
    (dict(c_out=128, c_out_pad=128, ys=128), "U"), (dict(c_out=256, c_out_pad=256, ys=256), "U"),  # c_out % 192
    (dict(c_in=40), "U"), (dict(c_in=8, k_pad=32), "U"),                                           # c_in % 16
    (dict(k_pad=48), "U"), (dict(k_pad=32), "U"),                                                  # k_pad % 32, k_pad < c_in
    (dict(xs=1 << 26), "U"), (dict(ys=1 << 26), "U"),                                              # the 2^26 stride limit
    (dict(c_out=192 * 30000, c_out_pad=192 * 30000, ys=192 * 30000, k_pad=1024), "U"),             # plane past 2^32 elements
    (dict(c_in=32768, xs=32768, k_pad=32768), "U"),                                                # vectors do not fit LDS
    (dict(npix=1 << 40), "U"),                                                                     # more tiles than a grid holds
]


@pytest.mark.parametrize("kw,code", PRODUCER_REJECTS)
def test_producer_applies_every_check_of_the_fp32_entry_point(kw, code):
    want = {"I": INVALID, "U": UNSUPPORTED}[code]
    assert _prod(**kw) == want, kw
    assert _prod("bts_conv1x1_bf16_fwd_f32", **kw) == want, kw                 # the same fault, the same code, in both


@pytest.mark.parametrize("addr", [4098, 4100])
def test_producer_wants_an_8_byte_aligned_bf16_base(addr):
    assert _prod(y=P(addr)) == INVALID
    assert _prod(y=P(4104), npix=1 << 40) == UNSUPPORTED                       # 8-byte aligned passes on to the later checks


# ------------------------------------------------------------------------------------------------------------ the consumer
CGOOD = dict(x=A, xs=192, B=2, h=8, w=64, c_in=192, wt=A, k_pad=1728, c_out=48, c_out_pad=64, es=A, eb=A, act=1, y=A, ys=48)


def _cons(**kw):
    a = dict(CGOOD, **kw)
    return _lib.load_real().bts_conv3x3_bf16in_fwd_f32(a["x"], a["xs"], a["B"], a["h"], a["w"], a["c_in"], a["wt"], a["k_pad"],
                                                        a["c_out"], a["c_out_pad"], a["es"], a["eb"], a["act"], a["y"], a["ys"], None)


@pytest.mark.parametrize("kw,code", [
    (dict(x=None), "I"), (dict(wt=None), "I"), (dict(y=None), "I"),                                # null operands
    (dict(es=None), "I"), (dict(eb=None), "I"),                                                    # half a pair
    (dict(x=P(4100)), "I"), (dict(x=P(4098)), "I"),                                                # x not 8-byte aligned
    (dict(wt=P(4104)), "I"), (dict(y=P(4098)), "I"), (dict(es=P(4097)), "I"),                      # w / y / a vector misaligned
    (dict(xs=194), "I"), (dict(xs=198), "I"),                                                      # stride not a multiple of 4
    (dict(xs=160), "I"), (dict(ys=44), "I"),                                                       # strides < c_in / < c_out
    (dict(act=3), "I"), (dict(act=-1), "I"), (dict(B=0), "I"), (dict(h=0), "I"), (dict(w=-1), "I"),
    (dict(c_out_pad=48), "I"), (dict(c_out_pad=32), "I"),                                          # pad % 32, pad < c_out
    (dict(c_in=48, xs=48, k_pad=432), "U"), (dict(c_in=16, xs=16, k_pad=160), "U"),                # c_in % 32
    (dict(k_pad=1732), "U"), (dict(k_pad=1696), "U"),                                              # k_pad % 8, k_pad < 9 c_in
    (dict(B=4096, h=1024, w=1024, xs=192), "U"),                                                   # B h w xs >= 2^32 (and B h w >= 2^31)
    (dict(B=32, h=1024, w=1024, xs=192), "U"),                                                     # B h w xs >= 2^32 alone
    (dict(c_out=3 << 20, c_out_pad=3 << 20, ys=3 << 20), "U"),                                     # c_out_pad k_pad >= 2^32
    (dict(ys=1 << 26), "U"),                                                                       # 64 ys >= 2^32
])
def test_consumer_rejects_bad_arguments_on_the_host(kw, code):
    assert _cons(**kw) == {"I": INVALID, "U": UNSUPPORTED}[code], kw


def test_consumer_absent_e1_passes_the_pair_check():
    assert _cons(es=None, eb=None, act=3) == INVALID
    assert _cons(es=None, eb=None, c_in=48, xs=48, k_pad=432) == UNSUPPORTED
    assert _cons(x=P(4104), es=None, eb=None, k_pad=1732) == UNSUPPORTED       # an 8-byte aligned prefix view is fine


# ------------------------------------------------------------------------------------------------------------ the query
HALO_BF16 = int(conv_plan.Family.HALO_BF16)
DUMMY = 1 << 20


def _dispatch_kind(h, w, c_in, c_out, ff, workspace):
    """bts_conv_plan_f32's own answer for the growth-convolution form of the layer at precision 2: no prologue, no residual,
    no y2, stride 1, dilation 1, NHWC, pre-rounded weights supplied; with or without a split-K workspace lent."""
    d = _lib.ConvDesc()
    d.x = d.w = d.y = d.w_split = DUMMY
    d.x_pix_stride, d.c_in_ld, d.k_pad = c_in, c_in, conv_plan.round_up(9 * c_in, 32)
    d.B, d.h_in, d.w_in, d.up, d.ksize, d.dil, d.stride, d.pad = 1, h, w, 1, 3, 1, 1, 1
    d.c_out, d.c_out_pad, d.y_pix_stride = c_out, conv_plan.round_up(c_out, 32), conv_plan.round_up(c_out, 4)
    d.precision, d.fill_frames = 2, ff
    if workspace:
        d.splitk_ws, d.splitk_ws_floats = DUMMY, 1 << 40
    bm, bn, kind = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.load_real().bts_conv_plan_f32(ctypes.byref(d), ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(kind))
    return (kind.value if rc == 0 else -1), bn.value


# DenseNet161's four blocks at 352x1216 and 352x704 (192 -> 48), and maps / widths around every condition of the dispatch
MAPS = [(88, 304), (44, 152), (22, 76), (11, 38), (88, 176), (44, 88), (22, 44), (11, 22),
        (4, 32), (8, 64), (16, 32), (5, 31), (9, 33), (12, 40), (3, 100), (64, 96), (1, 1), (26, 34)]
WIDTHS = [(192, 48), (192, 64), (192, 128), (64, 32), (32, 96), (128, 256), (48, 48), (100, 48), (2048, 128)]


@pytest.mark.parametrize("ff", [1, 2, 4, 8, 16, 64, 4096])
def test_query_is_the_dispatchs_halo_bf16_answer(ff):
    taken = 0
    for h, w in MAPS:
        for c_in, c_out in WIDTHS:
            p = ops.conv3x3_bf16in_plan(h, w, c_in, c_out, fill_frames=ff)
            kind_ws, bn_ws = _dispatch_kind(h, w, c_in, c_out, ff, True) if c_in % 4 == 0 else (-1, 0)
            kind_no, _ = _dispatch_kind(h, w, c_in, c_out, ff, False) if c_in % 4 == 0 else (-1, 0)
            assert p.eligible == (kind_ws == HALO_BF16), (h, w, c_in, c_out, ff, tuple(p), kind_ws)
            if p.eligible:                      # ... and the caller that lends no workspace gets the same kernel
                taken += 1
                assert kind_no == HALO_BF16 and c_in % 32 == 0
                tiles = ((h + 3) // 4) * ((w + 31) // 32)
                assert tuple(p) == (bn_ws, ff * tiles * ((c_out + bn_ws - 1) // bn_ws)), (h, w, c_in, c_out, ff, tuple(p))
                assert bn_ws == conv_plan.bf16in_3x3_tile(c_out)
            else:
                assert tuple(p) == (0, 0)
    assert taken > 0


def test_query_on_densenet161():
    """fill_frames 16: blocks 1-2 at 352x1216 and at 352x704 run the growth convolution on the bf16 halo tile; the deeper
    maps tile too raggedly (4x32 tiles under 0.80 real pixels: 22x76 is 0.73)."""
    got = {(h, w): ops.conv3x3_bf16in_plan(h, w, 192, 48, fill_frames=16).eligible for h, w in MAPS[:8]}
    assert got == {(88, 304): True, (44, 152): True, (22, 76): False, (11, 38): False,
                   (88, 176): True, (44, 88): True, (22, 44): False, (11, 22): False}, got
    assert tuple(ops.conv3x3_bf16in_plan(88, 304, 192, 48, fill_frames=16)) == (64, 16 * 22 * 10)
    with ops.launch_config(fill_frames=16, precision="bf16"):
        assert tuple(ops.conv3x3_bf16in_plan(88, 304, 192, 48)) == tuple(ops.conv3x3_bf16in_plan(88, 304, 192, 48, fill_frames=16))


def test_query_argument_checks_and_no_batch_parameter():
    assert list(inspect.signature(ops.conv3x3_bf16in_plan).parameters) == ["h", "w", "c_in", "c_out", "fill_frames"]
    lib = _lib.load_real()
    bn, wgs = ctypes.c_int(7), ctypes.c_long(7)
    assert lib.bts_conv3x3_bf16in_plan(88, 304, 192, 48, -1, ctypes.byref(bn), ctypes.byref(wgs)) == INVALID
    assert lib.bts_conv3x3_bf16in_plan(88, 304, 192, 48, 4097, ctypes.byref(bn), ctypes.byref(wgs)) == INVALID
    assert lib.bts_conv3x3_bf16in_plan(88, 304, 192, 48, 16, None, ctypes.byref(wgs)) == INVALID
    assert lib.bts_conv3x3_bf16in_plan(88, 304, 192, 48, 16, ctypes.byref(bn), None) == INVALID
    for bad in ((0, 304, 192, 48), (88, -1, 192, 48), (88, 304, 0, 48), (88, 304, 192, 0), (88, 304, 200, 48)):
        assert lib.bts_conv3x3_bf16in_plan(*bad, 16, ctypes.byref(bn), ctypes.byref(wgs)) == 0 and (bn.value, wgs.value) == (0, 0), bad
    with pytest.raises(_lib.BtsHipError):
        ops.conv3x3_bf16in_plan(88, 304, 192, 48, fill_frames=5000)


# ------------------------------------------------------------------------------------------------------------ wrappers, model
def test_wrappers_refuse_cpu_tensors_and_wrong_types():
    w1 = torch.zeros((1, 192, 64), dtype=torch.int16)
    with pytest.raises(_lib.BtsHipError):
        ops.conv1x1_bf16_forward(torch.zeros(40, 48), 40, 48, w1, 192, torch.zeros((40, 192), dtype=torch.bfloat16))
    w3 = torch.zeros((1, 64, 9 * 32), dtype=torch.int16)
    with pytest.raises(_lib.BtsHipError):
        ops.conv3x3_bf16in_forward(torch.zeros((128, 32), dtype=torch.bfloat16), 1, 4, 32, 32, w3, 48, torch.zeros(128, 48))
    with pytest.raises(_lib.BtsHipError):
        ops.conv3x3_bf16in_forward(torch.zeros((128, 32)), 1, 4, 32, 32, w3, 48, torch.zeros(128, 48))


@pytest.mark.parametrize("bad", [1, 0, "all", None, "True", 1.0])
def test_model_switch_is_a_bool(bad):
    from bts_amd import bts as M
    from parity_util import Params
    m = M.BtsModel(Params("densenet121_bts", 64, 80.0, "kitti"))
    assert m.bf16_mid_storage is False
    with pytest.raises(_lib.BtsHipError, match="bf16_mid_storage"):
        m.bf16_mid_storage = bad
    assert m.bf16_mid_storage is False
    m.bf16_mid_storage = True
    assert m.bf16_mid_storage is True
    m.bf16_mid_storage = False


def test_graphed_model_keys_on_the_switch_and_the_encoder_plan_has_it():
    import bts_amd.graph as G
    from bts_amd.encoder_hip import DenseNetHip
    assert "bf16_mid_storage" in inspect.getsource(G.GraphedModel.forward)
    assert "bf16_mid_storage" in inspect.getsource(DenseNetHip.run)
