"""ctypes binding of libbts_hip.so (C ABI declared in include/bts_hip.h).

The product path has NO fallback: if the library is missing or a symbol is absent this
module raises at import/first use, and every op raises on non-CUDA tensors.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Any, Dict, NamedTuple, Optional, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbts_hip.so")

ABI_VERSION = 17


class ConvDesc(C.Structure):
    """struct bts_conv_desc (include/bts_hip.h) -- field order and types must match."""
    _fields_ = [
        ("x", C.c_void_p), ("x_pix_stride", C.c_long), ("c_in_ld", C.c_int), ("k_pad", C.c_int),
        ("B", C.c_int), ("h_in", C.c_int), ("w_in", C.c_int), ("up", C.c_int),
        ("ksize", C.c_int), ("dil", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
        ("w", C.c_void_p), ("c_out", C.c_int), ("c_out_pad", C.c_int),
        ("pre_scale", C.c_void_p), ("pre_shift", C.c_void_p), ("pre_relu", C.c_int),
        ("e1_scale", C.c_void_p), ("e1_shift", C.c_void_p), ("act", C.c_int),
        ("e2_scale", C.c_void_p), ("e2_shift", C.c_void_p),
        ("y", C.c_void_p), ("y_pix_stride", C.c_long), ("y_nchw", C.c_int),
        ("subpixel", C.c_int), ("y2", C.c_void_p), ("y2_pix_stride", C.c_long),
        ("splitk_ws", C.c_void_p), ("splitk_ws_floats", C.c_long),
        ("res", C.c_void_p), ("res_pix_stride", C.c_long), ("n_bundles", C.c_int), ("precision", C.c_int),
        ("tail_planes", C.c_void_p * 4), ("n_tail", C.c_int), ("fill_frames", C.c_int), ("w_split", C.c_void_p), ("w_wino", C.c_void_p),
    ]


class ConvWgradDesc(C.Structure):
    """struct bts_conv_wgrad_desc (include/bts_hip.h)."""
    _fields_ = [
        ("x", C.c_void_p), ("x_pix_stride", C.c_long), ("c_in", C.c_int),
        ("dy", C.c_void_p), ("dy_pix_stride", C.c_long), ("c_out", C.c_int),
        ("B", C.c_int), ("h_in", C.c_int), ("w_in", C.c_int),
        ("up", C.c_int), ("ksize", C.c_int), ("dil", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
        ("dw", C.c_void_p), ("ws", C.c_void_p), ("ws_floats", C.c_long), ("n_bundles", C.c_int),
        ("pre_scale", C.c_void_p), ("pre_shift", C.c_void_p), ("pre_relu", C.c_int),
    ]


class ConvWgradBatchItem(C.Structure):
    """struct bts_conv_wgrad_batch_item (include/bts_hip.h)."""
    _fields_ = [("bm", C.c_int), ("bn", C.c_int), ("split", C.c_long), ("pix_per_split", C.c_long), ("ws_offset", C.c_long)]


class AdamwPack(C.Structure):
    """struct bts_adamw_pack (include/bts_hip.h)."""
    _fields_ = [("dst", C.c_void_p), ("k_pad", C.c_long), ("c_in_ld", C.c_int), ("mode", C.c_int)]


class AdamwItem(C.Structure):
    """struct bts_adamw_item (include/bts_hip.h)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("numel", C.c_long),
                ("hyper", C.c_int), ("c_out", C.c_int), ("c_in", C.c_int), ("ksize", C.c_int),
                ("n_packs", C.c_int), ("reserved", C.c_int), ("packs", AdamwPack * 2)]


class AdamwHyper(C.Structure):
    """struct bts_adamw_hyper (include/bts_hip.h)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("step", C.c_double)]


class AdamwPlanItem(C.Structure):
    """struct bts_adamw_plan_item (include/bts_hip.h)."""
    _fields_ = [("kind", C.c_int), ("reserved", C.c_int), ("first_block", C.c_long), ("n_blocks", C.c_long)]


QUERY, LAUNCH = "query", "launch"


class Entry(NamedTuple):
    """One C entry point (include/bts_hip.h).  ``role``: QUERY = host arithmetic only, enqueues nothing; LAUNCH = enqueues
    work on the stream passed as its last argument.  ``plan``: (BTS_OP_* kind, member of the bts_op union) when
    bts_plan_run can replay it -- plan.hip and the header spell the same numbers."""
    restype: Any
    argtypes: tuple
    role: str
    plan: Optional[Tuple[int, str]] = None


def _query(restype, *argtypes):
    return Entry(restype, argtypes, QUERY)


def _launch(*argtypes, plan=None):
    return Entry(C.c_int, argtypes, LAUNCH, plan)


_vp, _i, _l64, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
_pi, _pl, _pvp = C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_void_p)
_conv, _wgrad = C.POINTER(ConvDesc), C.POINTER(ConvWgradDesc)

# The whole C ABI, one row per entry point: a new one costs one row here (plus its header prototype, its C function, its
# plan.hip case when replayable, and its wrapper).  Argument order = the C prototypes.
ABI: Dict[str, Entry] = {
    "bts_hip_abi_version": _query(_i),
    "bts_hip_error_string": _query(C.c_char_p, _i),
    "bts_lpg_fwd_f32": _launch(_vp, _i, _i, _i, _i, _vp, _vp, _vp, plan=(10, "lpg")),
    "bts_lpg_bwd_f32": _launch(_vp, _vp, _i, _i, _i, _i, _vp, _vp),
    "bts_lpg_fused_fwd_f32": _launch(_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _l64, _vp, _vp, plan=(4, "lpg_fused")),
    "bts_reduc_fwd_f32": _launch(_vp, _l64, _l64, _i, _i, _vp, _l64, _f, _i, _i, _vp, _vp, plan=(2, "reduc")),
    "bts_reduc_lpg_fwd_f32": _launch(_vp, _l64, _i, _i, _i, _i, _i, _vp, _l64, _f, _i, _vp, _vp, _vp, _vp, _vp, plan=(3, "reduc_lpg")),
    "bts_reduc_bwd_f32": _launch(_vp, _l64, _i, _i, _i, _i, _i, _vp, _l64, _vp, _l64, _f, _i, _vp, _vp, _l64, _vp, _vp, _vp),
    "bts_reduc_bwd_max_waves": _query(_l64, _i, _i, _i),
    "bts_conv_fwd_f32": _launch(_conv, _vp, plan=(1, "conv")),
    "bts_upconv_combine_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _vp, _i, _vp, _l64, _vp, plan=(11, "upconv_combine")),
    "bts_upconv_up9_fwd_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _l64, _vp, plan=(12, "upconv_up9")),
    "bts_upconv_up9_plan": _query(_i, _i, _i, _i, _i, _i, _i, _pi, _pi, _pl),
    "bts_conv_tail_bf16_fwd_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _l64, _vp,
                                          plan=(13, "conv_tail_bf16")),
    "bts_conv_tail_bf16_plan": _query(_i, _i, _i, _i, _i, _i, _i, _pi, _pl),
    "bts_conv_tail_wino_fwd_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp,
                                          plan=(14, "conv_tail_wino")),
    "bts_conv_tail_wino_plan": _query(_i, _i, _i, _i, _i, _i, _i, _i, _pi, _pi, _pl),
    # opt-in and not replayable by bts_plan_run: no plan kind (a recording reports it as a foreign launch)
    "bts_conv_grouped_fwd_f32": _launch(_vp, _l64, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _l64, _vp),
    "bts_conv_grouped_plan": _query(_i, _i, _i, _i, _i, _i, _i, _pi, _pi, _pl),
    "bts_conv_grouped_bf16_fwd_f32": _launch(_vp, _l64, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _l64, _vp),
    "bts_conv_grouped_bf16_plan": _query(_i, _i, _i, _i, _i, _i, _i, _pi, _pi, _pl),
    "bts_conv_grouped_wgrad_f32": _launch(_vp, _l64, _vp, _l64, _i, _i, _i, _i, _i, _vp, _vp, _l64, _vp),
    "bts_conv_grouped_wgrad_plan": _query(_i, _i, _i, _i, _i, _i, _l64, _pi, _pl),
    "bts_conv1x1_bf16_fwd_f32": _launch(_vp, _l64, _l64, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _l64, _vp),
    "bts_conv1x1_bf16_plan": _query(_i, _i, _i, _i, _i, _i, _pi, _pi, _pl),
    # the bf16-resident bottleneck intermediate (BtsModel.bf16_mid_storage): producer, consumer, the consumer's query
    "bts_conv1x1_bf16_fwd_bf16": _launch(_vp, _l64, _l64, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _l64, _vp),
    "bts_conv3x3_bf16in_fwd_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _l64, _vp),
    "bts_conv3x3_bf16in_plan": _query(_i, _i, _i, _i, _i, _i, _pi, _pl),
    "bts_conv1x1_bf16_wide_fwd_f32": _launch(_vp, _l64, _l64, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _l64, _i, _vp, _l64,
                                             _vp, _l64, _i, _vp),
    "bts_conv1x1_bf16_wide_plan": _query(_i, _i, _i, _i, _i, _i, _i, _pi, _pi, _pl),
    "bts_conv_plan_f32": _query(_i, _conv, _pi, _pi, _pi),
    "bts_conv_plan_ksteps_f32": _query(_i, _conv, _pl, _pl),
    "bts_conv_wgrad_f32": _launch(_wgrad, _vp),
    "bts_conv_wgrad_plan_f32": _query(_i, _wgrad, _pi, _pi, _pl, _pl),
    "bts_conv_wgrad_batch_table_bytes": _query(_l64, _i),
    "bts_conv_wgrad_batch_plan_f32": _query(_i, _wgrad, _i, _pvp, _pl, _i, _l64, _vp, C.POINTER(ConvWgradBatchItem)),
    "bts_conv_wgrad_batch_f32": _launch(_vp, _vp, _i, _pvp, _i, _vp, _vp),
    # bf16 operands, fp32 accumulation (train_precision "bf16"): the fp32 descriptor, planner and batch table
    "bts_conv_wgrad_bf16_f32": _launch(_wgrad, _vp),
    "bts_conv_wgrad_bf16_plan_f32": _query(_i, _wgrad, _pi, _pi, _pl, _pl),
    "bts_conv_wgrad_batch_bf16_f32": _launch(_vp, _vp, _i, _pvp, _i, _vp, _vp),
    "bts_upconv_dgrad_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _i, _vp, _l64, _i, _i, _vp, _l64, _vp),
    "bts_upconv_dgrad_plan": _query(_i, _i, _i, _i, _i, _i, _i, _i, _l64, _pi, _pi, _pi),
    "bts_upconv_wgrad_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _l64, _i, _vp, _vp, _l64, _vp),
    "bts_upconv_wgrad_plan_f32": _query(_i, _i, _i, _i, _i, _i, _l64, _pi, _pi, _pl, _pl),
    "bts_upconv_train_pack_blocks": _query(_l64, _l64, _l64, _l64, _l64),
    "bts_upconv_train_pack_f32": _launch(_vp, _i, _l64, _vp),
    "bts_pack_weights_blocks": _query(_l64, _l64, _l64),
    "bts_pack_weights_f32": _launch(_vp, _i, _l64, _vp),
    "bts_pack_wino_floats": _query(_l64, _i, _i, _i, _i),
    "bts_pack_wino_f32": _launch(_vp, _i, _l64, _i, _i, _i, _vp, _vp),
    "bts_bn_train_ws_floats": _query(_l64, _l64, _i),
    "bts_bn_train_stats_f32": _launch(_vp, _l64, _l64, _i, _vp, _vp, _f, _f, _vp, _vp, _vp, _l64, _vp, _vp, _vp, _vp, _vp),
    "bts_bn_apply_nhwc_f32": _launch(_vp, _l64, _l64, _i, _vp, _vp, _i, _vp, _l64, _vp),
    "bts_bn_train_bwd_f32": _launch(_vp, _l64, _vp, _l64, _l64, _i, _vp, _vp, _vp, _vp, _i, _vp, _l64, _vp, _vp, _vp, _l64, _vp),
    "bts_bn_frozen_vectors_f32": _launch(_vp, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp),
    "bts_bn_frozen_bwd_f32": _launch(_vp, _l64, _vp, _l64, _l64, _i, _vp, _vp, _vp, _vp, _i, _vp, _l64, _vp, _vp, _vp, _l64, _i, _vp),
    "bts_nchw_to_nhwc_f32": _launch(_vp, _i, _i, _l64, _vp, _l64, _i, _vp, plan=(5, "nchw_to_nhwc")),
    "bts_nhwc_to_nchw_f32": _launch(_vp, _l64, _i, _i, _l64, _vp, _vp, plan=(6, "nhwc_to_nchw")),
    "bts_pack_planes_f32": _launch(_vp, _vp, _vp, _vp, _i, _l64, _vp, _l64, _vp),
    "bts_maxpool3x3s2_nhwc_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _l64, _vp, _l64, _vp, plan=(7, "maxpool")),
    "bts_bn_relu_avgpool2_nhwc_f32": _launch(_vp, _l64, _i, _i, _i, _i, _vp, _vp, _vp, _l64, _vp, plan=(8, "avgpool")),
    "bts_get_depth_f32": _launch(_vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, plan=(9, "get_depth")),
    "bts_eval_ws_doubles": _query(_l64, _i, _i, _i),
    "bts_eval_depth_metrics_f32": _launch(_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _f, _f, _i, _i, _i, _i, _vp, _l64, _vp, _vp, _vp),
    "bts_depth_loss_ws_doubles": _query(_l64, _l64),
    "bts_depth_loss_fwd_f32": _launch(_vp, _vp, _vp, _f, _l64, _i, _f, _vp, _l64, _vp, _vp, _vp),
    "bts_depth_loss_bwd_f32": _launch(_vp, _vp, _vp, _f, _l64, _i, _f, _vp, _vp, _vp, _vp),
    "bts_adamw_table_bytes": _query(_l64, _i),
    "bts_adamw_flat_span": _query(_l64),
    "bts_adamw_plan_f32": _query(_i, _vp, _i, _vp, _pl, _vp),
    "bts_adamw_step_f32": _launch(_vp, _i, _l64, _vp, _i, _vp, _vp),
    # replays a recorded forward; bts_amd/plan.py refines these pointer types once it has built bts_op / bts_plan_patch
    "bts_plan_run": _launch(_vp, _i, _vp, _i, _pvp, _i, _vp),
}
SYMBOLS = tuple(ABI)


class BtsHipError(RuntimeError):
    pass


def source_hash() -> str:
    """sha256 (first 16 hex digits) over the kernel sources the library is built from (csrc/*.hip, common.h,
    include/bts_hip.h): stamps profiles so that a counter value measured on older kernels is never quoted for newer ones."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h"))
                   + glob.glob(os.path.join(_HERE, "csrc", "*.inc")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "bts_hip.h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


_lib = None
_tls = threading.local()


class recording:
    """While active (this thread only), load() hands out `proxy` instead of the library: bts_amd/plan.py records the
    calls a forward makes through it."""

    def __init__(self, proxy):
        self.proxy = proxy

    def __enter__(self):
        self.prev = getattr(_tls, "proxy", None)
        _tls.proxy = self.proxy
        return self.proxy

    def __exit__(self, *exc):
        _tls.proxy = self.prev
        return False


def is_recording() -> bool:
    return getattr(_tls, "proxy", None) is not None


def load():
    """The loaded library (or the recording proxy standing in for it, see `recording`)."""
    proxy = getattr(_tls, "proxy", None)
    return proxy if proxy is not None else load_real()


def load_real():
    """Load the library once; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BtsHipError(
            "bts_amd: %s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C bts_amd/csrc`; there is no CPU/PyTorch fallback for the hot path" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, e in ABI.items():
        if not hasattr(lib, name):
            raise BtsHipError("bts_amd: symbol %s missing from %s" % (name, LIB_PATH))
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = e.restype, list(e.argtypes)
    if lib.bts_hip_abi_version() != ABI_VERSION:
        raise BtsHipError("bts_amd: ABI version mismatch (%d != %d)" % (lib.bts_hip_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


TORCH_LIB_PATH = os.path.join(_HERE, "libbts_torch.so")
_torch_ops = None


def load_torch_ops():
    """``torch.ops.bts_hip``: the TORCH_LIBRARY operator shell over the C ABI (csrc/torch_ops.cpp -> libbts_torch.so:
    TORCH_CHECK validation, device guard, current stream).  Loaded once; raises loudly if it is not built."""
    global _torch_ops
    if _torch_ops is not None:
        return _torch_ops
    import torch
    load_real()                                    # the C ABI library first: libbts_torch.so links against it
    if not os.path.exists(TORCH_LIB_PATH):
        raise BtsHipError("bts_amd: %s not found -- build it with `make -C bts_amd/csrc` (or BTS_BINDING=ctypes to bind the "
                          "C ABI directly)" % TORCH_LIB_PATH)
    torch.ops.load_library(TORCH_LIB_PATH)
    _torch_ops = torch.ops.bts_hip
    return _torch_ops


def check(code: int, what: str):
    if code != 0:
        msg = load().bts_hip_error_string(code)
        raise BtsHipError("%s failed: %s (code %d)" % (what, msg.decode() if msg else "?", code))
