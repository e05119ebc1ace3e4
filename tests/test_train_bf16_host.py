"""CPU: host side of train_precision "bf16" -- the model switch, the three new C entry points (header, ABI table, roles,
no plan kind, ABI version unchanged), the bf16 plan query against the fp32 one on every case of tests/wgrad_cases.py, and
the argument checks of the wrappers.  No GPU: plan queries are host arithmetic."""
import ctypes
import os
import re

import pytest
import torch

import wgrad_cases as wc
from bts_amd import _lib, ops, train
from bts_amd._lib import BtsHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bts_conv_wgrad_bf16_f32", "bts_conv_wgrad_bf16_plan_f32", "bts_conv_wgrad_batch_bf16_f32")


class Params:
    def __init__(self, enc, bts_size, max_depth, dataset):
        self.encoder, self.bts_size, self.max_depth, self.dataset = enc, bts_size, max_depth, dataset


def test_train_precision_defaults_to_fp32_and_validates_its_value():
    from bts_amd import bts as M
    m = M.BtsModel(Params("densenet121_bts", 512, 80.0, "kitti"))
    assert m.train_precision == m.encoder.train_precision == m.decoder.train_precision == "fp32"
    assert m.conv_precision == "fp32"
    m.train_precision = "bf16"
    assert m.train_precision == m.encoder.train_precision == m.decoder.train_precision == "bf16"
    assert m.conv_precision == "fp32"                          # a switch of its own
    for bad in ("bf16x3", "fp16", "", 2, None, True):
        with pytest.raises(BtsHipError, match="train_precision"):
            m.train_precision = bad
        assert m.train_precision == "bf16"
    m.train_precision = "fp32"
    assert m.encoder.train_precision == m.decoder.train_precision == "fp32"


def test_precision_scope_is_thread_local_grad_only_and_refuses_other_launch_precisions():
    import threading
    assert train.current_train_precision() == 0
    with pytest.raises(BtsHipError, match="train_precision"):
        train.precision_scope("bf16x3")
    if ops._ENV_PRECISION:                                     # $BTS_CONV_PRECISION=1 keeps its precedence: the scope reads fp32
        with train.precision_scope("bf16"):
            assert train.current_train_precision() == 0
        return
    with train.precision_scope("bf16"):
        assert train.current_train_precision() == 2
        seen = []
        t = threading.Thread(target=lambda: seen.append(train.current_train_precision()))
        t.start()
        t.join()
        assert seen == [0]                                     # what autograd's backward thread would see: nothing
        with train.precision_scope("fp32"):
            assert train.current_train_precision() == 0
        assert train.current_train_precision() == 2
    assert train.current_train_precision() == 0
    with torch.no_grad(), train.precision_scope("bf16"):       # read only by a grad-enabled forward
        assert train.current_train_precision() == 0
    for pr in ("bf16x3", "bf16"):
        with ops.launch_config(precision=pr):
            with pytest.raises(BtsHipError, match="conv_precision 'fp32'"):
                with train.precision_scope("bf16"):
                    pass
            with train.precision_scope("fp32"):
                assert train.current_train_precision() == 0
    assert train.current_train_precision() == 0


def test_refuse_bf16_is_unchanged():
    with ops.launch_config(precision="bf16"):
        if not ops._ENV_PRECISION:
            with pytest.raises(BtsHipError, match="inference"):
                train.refuse_bf16("somewhere")
    with train.precision_scope("bf16"):
        train.refuse_bf16("somewhere")                         # the new switch is not the inference mode


def test_new_entry_points_are_launches_and_a_query_without_a_plan_kind():
    from bts_amd import plan
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    lib = _lib.load_real()
    for name in NEW:
        assert name in _lib.ABI and name in _lib.SYMBOLS
        assert re.search(r"\bint\s+%s\(" % name, hdr), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert _lib.ABI[name].plan is None and name not in plan._KINDS
        assert getattr(lib, name).restype is ctypes.c_int
    assert _lib.ABI["bts_conv_wgrad_bf16_f32"].role == _lib.LAUNCH
    assert _lib.ABI["bts_conv_wgrad_batch_bf16_f32"].role == _lib.LAUNCH
    assert _lib.ABI["bts_conv_wgrad_bf16_plan_f32"].role == _lib.QUERY
    # same prototypes as their fp32 twins
    assert _lib.ABI["bts_conv_wgrad_bf16_f32"].argtypes == _lib.ABI["bts_conv_wgrad_f32"].argtypes
    assert _lib.ABI["bts_conv_wgrad_bf16_plan_f32"].argtypes == _lib.ABI["bts_conv_wgrad_plan_f32"].argtypes
    assert _lib.ABI["bts_conv_wgrad_batch_bf16_f32"].argtypes == _lib.ABI["bts_conv_wgrad_batch_f32"].argtypes


def test_abi_version_and_plan_kinds_are_unchanged():
    from bts_amd import plan
    assert _lib.ABI_VERSION == 17 and _lib.load_real().bts_hip_abi_version() == 17
    assert "#define BTS_HIP_ABI_VERSION 17" in " ".join(open(os.path.join(ROOT, "include", "bts_hip.h")).read().split())
    assert sorted(k for k, _ in plan._KINDS.values()) == list(range(1, 15))
    assert ctypes.sizeof(_lib.ConvWgradDesc) == 136 and ctypes.sizeof(_lib.ConvWgradBatchItem) == 32      # no struct changed


def _desc(c, ws=True):
    nb = max(c.n_bundles, 1)
    d = ops._wgrad_desc(c.B, c.h, c.w, c.c_in, c.c_out, c.ksize, c.dil, c.stride, c.pad, c.up, c.n_bundles,
                        nb * c.c_in + c.x_extra, nb * c.c_out + c.dy_extra)
    d.x = d.dy = d.dw = ops._PLAN_DUMMY_PTR
    if c.pre:
        d.pre_scale = d.pre_shift = ops._PLAN_DUMMY_PTR
        d.pre_relu = int(c.pre_relu)
    if ws and c.ws_floats is not None:
        d.ws, d.ws_floats = ops._PLAN_DUMMY_PTR, c.ws_floats
    return d


def _query(name, d):
    bm, bn, split, pps = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_long(0), ctypes.c_long(0)
    rc = getattr(_lib.load_real(), name)(ctypes.byref(d), ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(split), ctypes.byref(pps))
    return rc, (bm.value, bn.value, split.value, pps.value)


@pytest.mark.parametrize("c", wc.CASES + [c for _, c in wc.PATH_CASES], ids=lambda c: c.name)
def test_bf16_plan_is_the_fp32_plan_or_unsupported(c):
    for ws in (True, False):
        d = _desc(c, ws)
        rc32, want = _query("bts_conv_wgrad_plan_f32", d)
        rc, got = _query("bts_conv_wgrad_bf16_plan_f32", d)
        assert rc32 == 0
        assert rc in (0, ops.BTS_ERR_UNSUPPORTED), (c.name, rc)
        if rc == 0:
            assert got == want, (c.name, got, want)
            assert want[3] % 32 == 0                           # whole K-steps: whole pixel pairs
        nb = max(c.n_bundles, 1)
        py = ops.conv_wgrad_plan(c.B, c.h, c.w, c.c_in, c.c_out, c.ksize, dil=c.dil, stride=c.stride, pad=c.pad, up=c.up,
                                 ws_floats=c.ws_floats if ws else None, n_bundles=c.n_bundles, pre=c.pre, pre_relu=c.pre_relu,
                                 x_pix_stride=nb * c.c_in + c.x_extra, dy_pix_stride=nb * c.c_out + c.dy_extra, precision="bf16")
        assert py == (want if rc == 0 else None)


def test_bf16_plan_accepts_null_outputs_like_the_fp32_query():
    d = _desc(wc.BY_NAME["t64_s7"])
    assert _lib.load_real().bts_conv_wgrad_bf16_plan_f32(ctypes.byref(d), None, None, None, None) in (0, ops.BTS_ERR_UNSUPPORTED)


BAD = [
    ("null x", lambda d: setattr(d, "x", None)),
    ("null dy", lambda d: setattr(d, "dy", None)),
    ("null dw", lambda d: setattr(d, "dw", None)),
    ("B 0", lambda d: setattr(d, "B", 0)),
    ("c_in % 4", lambda d: setattr(d, "c_in", d.c_in + 2)),
    ("c_out % 4", lambda d: setattr(d, "c_out", d.c_out + 1)),
    ("up 3", lambda d: setattr(d, "up", 3)),
    ("ksize 2", lambda d: setattr(d, "ksize", 2)),
    ("ksize 9", lambda d: setattr(d, "ksize", 9)),
    ("dil 0", lambda d: setattr(d, "dil", 0)),
    ("pad -1", lambda d: setattr(d, "pad", -1)),
    ("x stride", lambda d: setattr(d, "x_pix_stride", d.c_in - 4)),
    ("dy stride % 4", lambda d: setattr(d, "dy_pix_stride", d.dy_pix_stride + 1)),
    ("x misaligned", lambda d: setattr(d, "x", ops._PLAN_DUMMY_PTR + 4)),
    ("dw misaligned", lambda d: setattr(d, "dw", ops._PLAN_DUMMY_PTR + 8)),
    ("ws misaligned", lambda d: setattr(d, "ws", ops._PLAN_DUMMY_PTR + 4)),
    ("pre_scale without shift", lambda d: setattr(d, "pre_scale", ops._PLAN_DUMMY_PTR)),
    ("bundles too many", lambda d: setattr(d, "n_bundles", 70000)),
    ("output 0 high", lambda d: (setattr(d, "h_in", 1), setattr(d, "ksize", 7), setattr(d, "pad", 0))),
    ("2^32 pixels", lambda d: (setattr(d, "B", 70000), setattr(d, "h_in", 300), setattr(d, "w_in", 300))),
]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_bf16_plan_rejects_what_the_fp32_query_rejects(what, spoil):
    """Same code for a descriptor both refuse -- and no launch is attempted for it: the bf16 launch runs the same
    prepare step before it touches the GPU (checked through the launch entry with a null stream on a bad descriptor)."""
    d = _desc(wc.BY_NAME["t64_s7"])
    spoil(d)
    rc32, _ = _query("bts_conv_wgrad_plan_f32", d)
    rc, _ = _query("bts_conv_wgrad_bf16_plan_f32", d)
    assert rc32 != 0, what
    assert rc == rc32, (what, rc, rc32)
    assert _lib.load_real().bts_conv_wgrad_bf16_f32(ctypes.byref(d), None) == rc32, what
    assert _lib.load_real().bts_conv_wgrad_bf16_plan_f32(None, None, None, None, None) == _lib.load_real().bts_conv_wgrad_plan_f32(None, None, None, None, None) != 0


def test_batch_bf16_launch_checks_its_table_like_the_fp32_launch():
    lib = _lib.load_real()
    n = 1
    table = ctypes.create_string_buffer(int(lib.bts_conv_wgrad_batch_table_bytes(n)))       # zeros: no magic
    bp = (ctypes.c_void_p * 1)(ops._PLAN_DUMMY_PTR)
    for name in ("bts_conv_wgrad_batch_f32", "bts_conv_wgrad_batch_bf16_f32"):
        assert getattr(lib, name)(table, ops._PLAN_DUMMY_PTR, n, bp, 1, None, None) == -1, name
        assert getattr(lib, name)(None, ops._PLAN_DUMMY_PTR, n, bp, 1, None, None) == -1, name
    descs = [_desc(wc.BY_NAME["t64_s7"], ws=False)]
    plan, table = ops.conv_wgrad_batch_plan_descs(descs, [(ops._PLAN_DUMMY_PTR, 1 << 60)], 1 << 20, with_table=True)
    assert plan[0][2] > 1
    for name in ("bts_conv_wgrad_batch_f32", "bts_conv_wgrad_batch_bf16_f32"):
        assert getattr(lib, name)(table, ops._PLAN_DUMMY_PTR, 2, bp, 1, None, None) == -1, name      # n mismatch
        assert getattr(lib, name)(table, None, 1, bp, 1, None, None) == -1, name                     # no device table
        assert getattr(lib, name)(table, ops._PLAN_DUMMY_PTR, 1, bp, 1, None, None) == -1, name      # split > 1 needs ws


def test_wrapper_precision_names():
    assert ops.wgrad_precision(None) == ops.wgrad_precision("fp32") == ops.wgrad_precision(0) == 0
    assert ops.wgrad_precision("bf16") == ops.wgrad_precision(2) == 2
    for bad in ("bf16x3", 1, "half", [2]):
        with pytest.raises(BtsHipError, match="precision"):
            ops.wgrad_precision(bad)
    with pytest.raises(BtsHipError, match="precision"):
        ops.conv_wgrad_plan(1, 8, 8, 16, 16, 3, precision="bf16x3")
