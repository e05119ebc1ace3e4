"""CPU: host side of the wide bf16 1x1 tile at 128 / 192 / 256 channels per workgroup (bts_conv1x1_bf16_wide_fwd_f32 /
bts_conv1x1_bf16_wide_plan, csrc/conv_1x1_bf16.inc) -- the C-ABI export list, the argument checks of the entry point (made
before any GPU work, so never-dereferenced pointers do), the plan query's answers, the wrapper's refusals and the model
switch's third value."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from bts_amd import _lib, conv_plan, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, PLAN = "bts_conv1x1_bf16_wide_fwd_f32", "bts_conv1x1_bf16_wide_plan"
OLD_FWD, OLD_PLAN = "bts_conv1x1_bf16_fwd_f32", "bts_conv1x1_bf16_plan"


def test_exports_and_abi_version_unchanged():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    for name in (FWD, PLAN):
        assert name in _lib.ABI and re.search(r"\b%s\s*\(" % name, hdr)
    assert _lib.ABI[FWD].role == _lib.LAUNCH and _lib.ABI[PLAN].role == _lib.QUERY
    assert _lib.ABI[FWD].plan is None and _lib.ABI[PLAN].plan is None
    assert len(_lib.ABI[FWD].argtypes) == 22 and len(_lib.ABI[PLAN].argtypes) == 9
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr
    from bts_amd import plan
    assert FWD not in plan._KINDS and PLAN not in plan._KINDS           # a foreign launch to the plan recorder
    assert conv_plan.wide_1x1_bf16_kernel_name(128) == "conv1x1_bf16_kernel<128>"
    assert conv_plan.wide_1x1_bf16_kernel_name(256) == "conv1x1_bf16_kernel<256>"
    lib = _lib.load_real()
    assert lib.bts_hip_abi_version() == 17 and hasattr(lib, FWD) and hasattr(lib, PLAN)


A = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails its checks first
GOOD = dict(x=A, xs=96, npix=300, c_in=48, w=A, k_pad=64, c_out=256, c_out_pad=256, ps=A, pb=A, pre_relu=1, es=A, eb=A, res=A, rs=320,
            act=1, y=A, ys=256, y2=A, y2s=512, bn=0)


def _call(**kw):
    a = dict(GOOD, **kw)
    return _lib.load_real().bts_conv1x1_bf16_wide_fwd_f32(
        a["x"], a["xs"], a["npix"], a["c_in"], a["w"], a["k_pad"], a["c_out"], a["c_out_pad"], a["ps"], a["pb"], a["pre_relu"], a["es"],
        a["eb"], a["res"], a["rs"], a["act"], a["y"], a["ys"], a["y2"], a["y2s"], a["bn"], None)


def _old(c_out):
    return _lib.load_real().bts_conv1x1_bf16_fwd_f32(A, 96, 300, 48, A, 64, c_out, c_out, A, A, 1, A, A, 1, A, c_out, None)


INVALID, UNSUPPORTED = _old(0), _old(128)        # the old entry point's two codes


def test_the_two_codes_are_the_siblings():
    assert INVALID != 0 and UNSUPPORTED != 0 and INVALID != UNSUPPORTED
    assert _call(x=None) == INVALID and _call(c_out=64, c_out_pad=64) == UNSUPPORTED
    assert b"not built" in _lib.load_real().bts_hip_error_string(UNSUPPORTED)


def test_old_entry_point_and_query_still_refuse_the_other_widths():
    assert _old(128) == UNSUPPORTED and _old(256) == UNSUPPORTED
    for c_out in (128, 256):
        assert tuple(ops.conv1x1_bf16_plan(88, 304, 96, c_out, fill_frames=16)) == (0, 0, 0)
        assert tuple(ops.conv1x1_bf16_plan(88, 304, 96, c_out, fill_frames=4096)) == (0, 0, 0)


W = dict(c_out=192 * 30000, c_out_pad=192 * 30000, ys=192 * 30000, rs=192 * 30000, y2s=192 * 30000, k_pad=1024)


@pytest.mark.parametrize("kw,code", [
    # everything the old entry point's table rejects, with the same code
    (dict(x=None), "I"), (dict(w=None), "I"), (dict(y=None), "I"),                                 # null operands
    (dict(ps=None), "I"), (dict(pb=None), "I"), (dict(es=None), "I"), (dict(eb=None), "I"),        # half a pair
    (dict(xs=32), "I"), (dict(ys=128), "I"),                                                       # strides < c_in / < c_out
    (dict(xs=98), "I"), (dict(ys=258), "I"),                                                       # strides not multiples of 4
    (dict(x=ctypes.c_void_p(4100)), "I"), (dict(w=ctypes.c_void_p(4104)), "I"),                    # x / w not 16-byte aligned
    (dict(y=ctypes.c_void_p(4098)), "I"), (dict(ps=ctypes.c_void_p(4097)), "I"),                   # y / a vector not 4-byte aligned
    (dict(act=3), "I"), (dict(act=-1), "I"), (dict(npix=0), "I"), (dict(npix=-5), "I"),
    (dict(c_out_pad=160), "I"),                                                                    # pad below c_out
    (dict(c_in=40), "U"), (dict(c_in=8, k_pad=32), "U"),                                           # c_in % 16
    (dict(k_pad=48), "U"), (dict(k_pad=80), "U"),                                                  # k_pad % 32
    (dict(k_pad=32), "U"),                                                                         # k_pad < c_in
    (dict(xs=1 << 26), "U"), (dict(ys=1 << 27), "U"),                                              # past the 32-bit in-tile offsets
    (W, "U"),                                                                                      # plane past 2^32 elements
    (dict(c_in=32768, xs=32768, k_pad=32768), "U"),                                                # vectors do not fit LDS
    (dict(npix=1 << 40), "U"),                                                                     # more tiles than a grid holds
    # res / y2: the same view checks
    (dict(rs=252), "I"), (dict(y2s=128), "I"),                                                     # stride below c_out
    (dict(rs=322), "I"), (dict(y2s=258), "I"),                                                     # stride not a multiple of 4
    (dict(res=ctypes.c_void_p(4098)), "I"), (dict(y2=ctypes.c_void_p(4097)), "I"),                 # misaligned
    (dict(rs=1 << 26), "U"), (dict(y2s=1 << 26), "U"),
    # bn
    (dict(bn=64), "I"), (dict(bn=1), "I"), (dict(bn=-128), "I"), (dict(bn=512), "I"),              # not one of 0 / 128 / 192 / 256
    (dict(bn=192), "U"), (dict(bn=256, c_out=384, c_out_pad=384, ys=384, rs=384, y2s=384), "U"),   # does not divide c_out
    (dict(bn=256, c_out=128, c_out_pad=128), "U"),
    (dict(c_out=64, c_out_pad=64), "U"), (dict(c_out=96, c_out_pad=96), "U"),                      # no whole 128-channel tile
    (dict(c_out=64, c_out_pad=64, bn=128), "U"),
])
def test_entry_point_rejects_bad_arguments_on_the_host(kw, code):
    assert _call(**kw) == {"I": INVALID, "U": UNSUPPORTED}[code], kw


def test_absent_operands_pass_their_checks():
    """Both vectors of a pair absent, and a stride given for a null res / y2, are fine: such a call fails a LATER check."""
    assert _call(ps=None, pb=None, es=None, eb=None, act=3) == INVALID
    assert _call(ps=None, pb=None, es=None, eb=None, c_in=40) == UNSUPPORTED
    assert _call(res=None, rs=3, y2=None, y2s=-7, c_in=40) == UNSUPPORTED          # not INVALID: the strides are ignored
    assert _call(res=None, rs=1 << 30, y2=None, y2s=1 << 30, bn=192) == UNSUPPORTED


# (encoder, stage, form): (h, w, c_in, c_out, has_res) of the layer classes of ResNeXt-101 and ResNet-50 at 416x544 and DenseNet121
# at 352x1216 -- the classes scripts/conv1x1_bf16_wide_bench.py measures.
R = (104, 136), (52, 68), (26, 34), (13, 17)
D = (88, 304), (44, 152), (22, 76), (11, 38)
CLASSES = {
    ("resnext101", "l1", "conv1 first"): R[0] + (64, 256, 0), ("resnext101", "l1", "conv1"): R[0] + (256, 256, 0),
    ("resnext101", "l1", "down"): R[0] + (64, 256, 0), ("resnext101", "l1", "conv3"): R[0] + (256, 256, 1),
    ("resnext101", "l2", "conv1 first"): R[0] + (256, 512, 0), ("resnext101", "l2", "conv1"): R[1] + (512, 512, 0),
    ("resnext101", "l2", "conv3"): R[1] + (512, 512, 1),
    ("resnext101", "l3", "conv1 first"): R[1] + (512, 1024, 0), ("resnext101", "l3", "conv1"): R[2] + (1024, 1024, 0),
    ("resnext101", "l3", "conv3"): R[2] + (1024, 1024, 1),
    ("resnext101", "l4", "conv1 first"): R[2] + (1024, 2048, 0), ("resnext101", "l4", "conv1"): R[3] + (2048, 2048, 0),
    ("resnext101", "l4", "conv3"): R[3] + (2048, 2048, 1),
    ("resnet50", "l1", "down"): R[0] + (64, 256, 0), ("resnet50", "l1", "conv3"): R[0] + (64, 256, 1),
    ("resnet50", "l2", "conv1 first"): R[0] + (256, 128, 0), ("resnet50", "l2", "conv1"): R[1] + (512, 128, 0),
    ("resnet50", "l2", "conv3"): R[1] + (128, 512, 1),
    ("resnet50", "l3", "conv1 first"): R[1] + (512, 256, 0), ("resnet50", "l3", "conv1"): R[2] + (1024, 256, 0),
    ("resnet50", "l3", "conv3"): R[2] + (256, 1024, 1),
    ("resnet50", "l4", "conv1 first"): R[2] + (1024, 512, 0), ("resnet50", "l4", "conv1"): R[3] + (2048, 512, 0),
    ("resnet50", "l4", "conv3"): R[3] + (512, 2048, 1),
    ("densenet121", "b1", "first"): D[0] + (64, 128, 0), ("densenet121", "b1", "last"): D[0] + (224, 128, 0),
    ("densenet121", "b2", "first"): D[1] + (128, 128, 0), ("densenet121", "b2", "last"): D[1] + (480, 128, 0),
    ("densenet121", "b3", "first"): D[2] + (256, 128, 0), ("densenet121", "b3", "last"): D[2] + (992, 128, 0),
    ("densenet121", "b4", "first"): D[3] + (512, 128, 0), ("densenet121", "b4", "last"): D[3] + (992, 128, 0),
}
# What profiles/conv1x1_bf16_wide_bench.txt decided at fill_frames 16: the classes that beat today's path by more
# than the run-to-run spread as a B = 16 launch and do not lose as the B = 4 sub-batch launch, and the tile of each.
# Every accepted class runs the 128-wide tile: 256 lost to it on some class of every width.  Left out: the classes of 848 / 896
# declared workgroups, marginal at B = 4 (ResNet-50 l3 "conv1 first" and "conv3", DenseNet121 b2), and DenseNet121 b3 / b4 "first"
# (224 / 64 declared workgroups: they won in isolation, but the same blocks lose at K 992).
ACCEPTED_AT_16 = {k: 128 for k in (
    ("resnext101", "l1", "conv1 first"), ("resnext101", "l1", "conv1"), ("resnext101", "l1", "down"), ("resnext101", "l1", "conv3"),
    ("resnext101", "l2", "conv1 first"), ("resnext101", "l2", "conv1"), ("resnext101", "l2", "conv3"),
    ("resnext101", "l3", "conv1 first"),
    ("resnet50", "l1", "down"), ("resnet50", "l1", "conv3"), ("resnet50", "l2", "conv1 first"), ("resnet50", "l2", "conv3"),
    ("densenet121", "b1", "first"), ("densenet121", "b1", "last"),
)}


def test_plan_query_has_no_batch_parameter():
    assert list(inspect.signature(ops.conv1x1_bf16_wide_plan).parameters) == ["h", "w", "c_in", "c_out", "has_res", "fill_frames"]
    assert len(_lib.ABI[PLAN].argtypes) == 9              # h, w, c_in, c_out, has_res, fill_frames, *bm, *bn, *workgroups


def test_plan_query_answers_what_the_bench_decided():
    for key, (h, w, c_in, c_out, has_res) in CLASSES.items():
        p = tuple(ops.conv1x1_bf16_wide_plan(h, w, c_in, c_out, has_res=bool(has_res), fill_frames=16))
        if key in ACCEPTED_AT_16:
            bn = ACCEPTED_AT_16[key]
            assert p == (128, bn, (h * w + 127) // 128 * (c_out // bn)), (key, p)
            assert bn == conv_plan.wide_1x1_bf16_tile(c_out), key        # the tile KernelTrace names for bn = 0
        else:
            assert p == (0, 0, 0), (key, p)
        assert tuple(ops.conv1x1_bf16_wide_plan(h, w, c_in + 8, c_out, fill_frames=16)) == (0, 0, 0)   # no whole 16-k MFMA blocks
        assert tuple(ops.conv1x1_bf16_wide_plan(h, w, c_in, 64, fill_frames=16)) == (0, 0, 0)          # no whole N tile
        assert tuple(ops.conv1x1_bf16_wide_plan(h, w, c_in, 96, fill_frames=16)) == (0, 0, 0)


def test_plan_query_edges():
    # c_out % 192 == 0: the tile and the threshold of the first kernel (DenseNet161's bottlenecks)
    assert tuple(ops.conv1x1_bf16_wide_plan(88, 304, 96, 192, fill_frames=16)) == tuple(ops.conv1x1_bf16_plan(88, 304, 96, 192, fill_frames=16))
    assert tuple(ops.conv1x1_bf16_wide_plan(22, 76, 384, 192, fill_frames=16)) == (0, 0, 0)
    assert tuple(ops.conv1x1_bf16_wide_plan(88, 304, 96, 384, fill_frames=16)) == (128, 192, 2 * 209)
    # workgroups per frame = ceil(h w / 128) * c_out / bn, wherever a class is accepted
    for c_out in (128, 256, 512, 1024, 2048):
        p = ops.conv1x1_bf16_wide_plan(100, 100, 64, c_out, fill_frames=4096)
        if p.eligible:
            assert p.bm == 128 and p.bn in (128, 256) and p.workgroups == 79 * (c_out // p.bn), tuple(p)
    assert tuple(ops.conv1x1_bf16_wide_plan(0, 100, 64, 256, fill_frames=16)) == (0, 0, 0)
    # the default comes from the launch_config in force
    with ops.launch_config(fill_frames=16, precision="bf16"):
        for h, w, c_in, c_out, has_res in CLASSES.values():
            assert (tuple(ops.conv1x1_bf16_wide_plan(h, w, c_in, c_out, bool(has_res)))
                    == tuple(ops.conv1x1_bf16_wide_plan(h, w, c_in, c_out, bool(has_res), fill_frames=16)))
    with pytest.raises(_lib.BtsHipError):
        ops.conv1x1_bf16_wide_plan(88, 304, 96, 256, fill_frames=5000)
    bm, bn, wgs = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_long(7)
    lib = _lib.load_real()
    ref = ctypes.byref
    assert lib.bts_conv1x1_bf16_wide_plan(88, 304, 96, 256, 0, -1, ref(bm), ref(bn), ref(wgs)) == INVALID
    assert lib.bts_conv1x1_bf16_wide_plan(88, 304, 96, 256, 0, 4097, ref(bm), ref(bn), ref(wgs)) == INVALID
    assert lib.bts_conv1x1_bf16_wide_plan(88, 304, 96, 256, 0, 16, None, ref(bn), ref(wgs)) == INVALID
    assert lib.bts_conv1x1_bf16_wide_plan(88, 304, 96, 256, 0, 16, ref(bm), None, ref(wgs)) == INVALID
    assert lib.bts_conv1x1_bf16_wide_plan(88, 304, 96, 256, 0, 16, ref(bm), ref(bn), None) == INVALID


def test_plan_answer_does_not_depend_on_the_batch():
    class M:
        fill_frames, conv_precision = 16, "bf16"
    for h, w, c_in, c_out, has_res in CLASSES.values():
        answers = set()
        for batch in (1, 2, 3, 8, 16, 64):
            with ops.model_launch_config(M, batch):
                answers.add(tuple(ops.conv1x1_bf16_wide_plan(h, w, c_in, c_out, bool(has_res))))
        assert len(answers) == 1


def test_forward_wrapper_refuses_cpu_tensors_and_shapes_the_kernel_does_not_take():
    x, y = torch.zeros(40, 48), torch.zeros(40, 256)
    w = torch.zeros((1, 256, 64), dtype=torch.int16)
    with pytest.raises(_lib.BtsHipError):
        ops.conv1x1_bf16_wide_forward(x, 40, 48, w, 256, y)                                       # CPU tensors


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the wrapper's own argument checks run, and every call below fails one of them
    before anything is launched."""
    @staticmethod
    def make(t):
        return t.as_subclass(_FakeCuda)

    @property
    def is_cuda(self):
        return True


def test_forward_wrapper_argument_checks():
    f = _FakeCuda.make
    x, y = f(torch.zeros(40, 64)), f(torch.zeros(40, 256))
    w = f(torch.zeros((1, 256, 64), dtype=torch.int16))
    bad = [
        dict(w_plane=f(torch.zeros((1, 256, 64)))),                               # fp32 weight plane
        dict(act=ops.ACT_SIGMOID),
        dict(c_out=64, y2d=f(torch.zeros(40, 64))),                               # c_out 64
        dict(npix=41),                                                            # views that do not fit
        dict(c_in=80),
        dict(y2d=f(torch.zeros(40, 128))),
        dict(bn=64), dict(bn=192),
        dict(res2d=f(torch.zeros(40, 128))), dict(y2_2d=f(torch.zeros(39, 256))),
    ]
    for kw in bad:
        a = dict(x2d=x, npix=40, c_in=64, w_plane=w, c_out=256, y2d=y)
        a.update(kw)
        with pytest.raises(_lib.BtsHipError):
            ops.conv1x1_bf16_wide_forward(**a)


def test_model_switch_accepts_three_values_only():
    from bts_amd import bts as M
    from parity_util import Params
    m = M.BtsModel(Params("resnet50_bts", 512, 10.0, "nyu"))
    assert m.bf16_wide_1x1 is False
    for v in (True, "all", False):
        m.bf16_wide_1x1 = v
        assert m.bf16_wide_1x1 == v and type(m.bf16_wide_1x1) is type(v)
    for v in ("some", "ALL", 2, None, "true"):
        with pytest.raises(_lib.BtsHipError):
            m.bf16_wide_1x1 = v
    assert m.bf16_wide_1x1 is False
