"""CPU: host side of the wide bf16 1x1 kernel (csrc/conv_1x1_bf16.inc) -- the C-ABI export list, the argument checks of the
entry point (made before any GPU work, so never-dereferenced pointers do), the plan query's answers, and the wrapper's
refusal of CPU tensors."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from bts_amd import _lib, conv_plan, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, PLAN = "bts_conv1x1_bf16_fwd_f32", "bts_conv1x1_bf16_plan"


def test_exports_and_abi_version_unchanged():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    for name in (FWD, PLAN):
        assert name in _lib.ABI and re.search(r"\b%s\s*\(" % name, hdr)
    assert _lib.ABI[FWD].role == _lib.LAUNCH and _lib.ABI[PLAN].role == _lib.QUERY
    assert _lib.ABI[FWD].plan is None and _lib.ABI[PLAN].plan is None
    assert len(_lib.ABI[FWD].argtypes) == 17 and len(_lib.ABI[PLAN].argtypes) == 8
    assert _lib.ABI_VERSION == 17 and "#define BTS_HIP_ABI_VERSION 17" in hdr
    from bts_amd import plan
    assert FWD not in plan._KINDS and PLAN not in plan._KINDS           # a foreign launch to the plan recorder
    assert conv_plan.wide_1x1_bf16_kernel_name(192) == "conv1x1_bf16_kernel<192>"
    lib = _lib.load_real()
    assert lib.bts_hip_abi_version() == 17 and hasattr(lib, FWD) and hasattr(lib, PLAN)


A = ctypes.c_void_p(4096)                       # never dereferenced: every call below fails its checks first
GOOD = dict(x=A, xs=96, npix=300, c_in=48, w=A, k_pad=64, c_out=192, c_out_pad=192, ps=A, pb=A, pre_relu=1, es=A, eb=A, act=1,
            y=A, ys=192)


def _call(**kw):
    a = dict(GOOD, **kw)
    return _lib.load_real().bts_conv1x1_bf16_fwd_f32(a["x"], a["xs"], a["npix"], a["c_in"], a["w"], a["k_pad"], a["c_out"], a["c_out_pad"],
                                                      a["ps"], a["pb"], a["pre_relu"], a["es"], a["eb"], a["act"], a["y"], a["ys"], None)


INVALID, UNSUPPORTED = _call(x=None), _call(c_out=128, c_out_pad=128, ys=128)


def test_the_two_codes_are_the_librarys_own():
    lib = _lib.load_real()
    assert INVALID != 0 and UNSUPPORTED != 0 and INVALID != UNSUPPORTED
    assert b"not built" in lib.bts_hip_error_string(UNSUPPORTED)
    # the sibling entry points return the same two codes for the same faults
    assert lib.bts_conv_grouped_fwd_f32(None, 64, 1, 4, 4, 64, 4, A, A, A, 0, A, 64, None) == INVALID
    assert lib.bts_conv_grouped_fwd_f32(A, 96, 1, 4, 4, 96, 12, A, A, A, 0, A, 96, None) == UNSUPPORTED


@pytest.mark.parametrize("kw,code", [
    (dict(x=None), "I"), (dict(w=None), "I"), (dict(y=None), "I"),                                 # null operands
    (dict(ps=None), "I"), (dict(pb=None), "I"), (dict(es=None), "I"), (dict(eb=None), "I"),        # half a pair
    (dict(xs=32), "I"), (dict(ys=128), "I"),                                                       # strides < c_in / < c_out
    (dict(xs=98), "I"), (dict(ys=194), "I"),                                                       # strides not multiples of 4
    (dict(x=ctypes.c_void_p(4100)), "I"), (dict(w=ctypes.c_void_p(4104)), "I"),                    # x / w not 16-byte aligned
    (dict(y=ctypes.c_void_p(4098)), "I"), (dict(ps=ctypes.c_void_p(4097)), "I"),                   # y / a vector not 4-byte aligned
    (dict(act=3), "I"), (dict(act=-1), "I"), (dict(npix=0), "I"), (dict(npix=-5), "I"),
    (dict(c_out_pad=160), "I"),                                                                    # pad below c_out
    (dict(c_out=128, c_out_pad=128, ys=128), "U"), (dict(c_out=256, c_out_pad=256, ys=256), "U"),  # c_out % 192
    (dict(c_in=40), "U"), (dict(c_in=8, k_pad=32), "U"),                                           # c_in % 16
    (dict(k_pad=48), "U"), (dict(k_pad=80), "U"),                                                  # k_pad % 32
    (dict(k_pad=32), "U"),                                                                         # k_pad < c_in
    (dict(xs=1 << 26), "U"), (dict(ys=1 << 27), "U"),                                              # past the 32-bit in-tile offsets
    (dict(c_out=192 * 30000, c_out_pad=192 * 30000, ys=192 * 30000, k_pad=1024), "U"),             # plane past 2^32 elements
    (dict(c_in=32768, xs=32768, k_pad=32768), "U"),                                                # vectors do not fit LDS
    (dict(npix=1 << 40), "U"),                                                                     # more tiles than a grid holds
])
def test_entry_point_rejects_bad_arguments_on_the_host(kw, code):
    assert _call(**kw) == {"I": INVALID, "U": UNSUPPORTED}[code], kw


def test_absent_affines_pass_the_pair_checks():
    """Both vectors of a pair absent is fine: such a call fails a LATER check."""
    assert _call(ps=None, pb=None, es=None, eb=None, act=3) == INVALID
    assert _call(ps=None, pb=None, es=None, eb=None, c_in=40) == UNSUPPORTED


# DenseNet161 at 352x1216: (h, w, c_in of the first / a middle / the last bottleneck) of blocks 1..4; c_out 192
BLOCKS = {1: (88, 304, (96, 240, 336)), 2: (44, 152, (192, 480, 720)), 3: (22, 76, (384, 1248, 2064)), 4: (11, 38, (1056, 1632, 2160))}
# What profiles/conv1x1_bf16_bench.txt decided: at fill_frames 16 blocks 1 and 2 beat today's path by more than
# the run-to-run spread as a B = 16 launch and do not lose as the B = 4 sub-batch launch; block 3 loses at B = 4, block 4 always
ACCEPTED_AT_16 = (1, 2)


def test_plan_query_has_no_batch_parameter():
    assert list(inspect.signature(ops.conv1x1_bf16_plan).parameters) == ["h", "w", "c_in", "c_out", "fill_frames"]
    assert len(_lib.ABI[PLAN].argtypes) == 8              # h, w, c_in, c_out, fill_frames, *bm, *bn, *workgroups


def test_plan_query():
    none = (0, 0, 0)
    for blk, (h, w, cins) in BLOCKS.items():
        for c_in in cins:
            p = ops.conv1x1_bf16_plan(h, w, c_in, 192, fill_frames=16)
            if blk in ACCEPTED_AT_16:
                assert tuple(p) == (128, 192, (h * w + 127) // 128), (blk, c_in, tuple(p))
            else:
                assert tuple(p) == none, (blk, c_in, tuple(p))
            assert tuple(ops.conv1x1_bf16_plan(h, w, c_in, 128, fill_frames=16)) == none      # DenseNet121 / ASPP width
            assert tuple(ops.conv1x1_bf16_plan(h, w, c_in, 256, fill_frames=16)) == none      # ResNe(X)t width
            assert tuple(ops.conv1x1_bf16_plan(h, w, c_in + 8, 192, fill_frames=16)) == none  # no whole 16-k MFMA blocks
    # two N tiles: workgroups count both
    assert tuple(ops.conv1x1_bf16_plan(88, 304, 96, 384, fill_frames=16)) == (128, 192, 2 * 209)
    # a declared launch below the threshold (csrc/conv_1x1_bf16.inc: kC1bMinWgs = 512 workgroups), and just above it
    assert tuple(ops.conv1x1_bf16_plan(8, 12, 96, 192, fill_frames=1)) == none
    assert tuple(ops.conv1x1_bf16_plan(11, 38, 1056, 192, fill_frames=2)) == none
    assert tuple(ops.conv1x1_bf16_plan(88, 304, 96, 192, fill_frames=2)) == none                 # 418
    assert tuple(ops.conv1x1_bf16_plan(88, 304, 96, 192, fill_frames=3)) == (128, 192, 209)      # 627
    assert tuple(ops.conv1x1_bf16_plan(44, 152, 192, 192, fill_frames=8)) == none                # 424
    assert tuple(ops.conv1x1_bf16_plan(2, 3, 96, 192, fill_frames=4096)) == (128, 192, 1)        # what the GPU tests pin
    # the default comes from the launch_config in force
    with ops.launch_config(fill_frames=16, precision="bf16"):
        assert tuple(ops.conv1x1_bf16_plan(88, 304, 96, 192)) == tuple(ops.conv1x1_bf16_plan(88, 304, 96, 192, fill_frames=16))
    with pytest.raises(_lib.BtsHipError):
        ops.conv1x1_bf16_plan(88, 304, 96, 192, fill_frames=5000)
    bm, bn, wgs = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_long(7)
    lib = _lib.load_real()
    assert lib.bts_conv1x1_bf16_plan(88, 304, 96, 192, -1, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(wgs)) == INVALID
    assert lib.bts_conv1x1_bf16_plan(88, 304, 96, 192, 4097, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(wgs)) == INVALID
    assert lib.bts_conv1x1_bf16_plan(88, 304, 96, 192, 16, None, ctypes.byref(bn), ctypes.byref(wgs)) == INVALID


def test_plan_answer_does_not_depend_on_the_batch():
    """What a model asks inside its own scope with fill_frames pinned is the same answer whatever batch it was called with."""
    class M:
        fill_frames, conv_precision = 16, "bf16"
    for blk, (h, w, cins) in BLOCKS.items():
        answers = set()
        for batch in (1, 2, 3, 8, 16, 64):
            with ops.model_launch_config(M, batch):
                answers.add(tuple(ops.conv1x1_bf16_plan(h, w, cins[1], 192)))
        assert len(answers) == 1


def test_forward_wrapper_refuses_cpu_tensors_and_shapes_the_kernel_does_not_take():
    x, y = torch.zeros(40, 48), torch.zeros(40, 192)
    w = torch.zeros((1, 192, 64), dtype=torch.int16)
    with pytest.raises(_lib.BtsHipError):
        ops.conv1x1_bf16_forward(x, 40, 48, w, 192, y)
