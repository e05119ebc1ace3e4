"""Host-side wrappers over the C ABI (include/bts_hip.h): argument validation, weight packing,
stream plumbing.  torch is used only for device memory and the current stream.

Every function requires CUDA(ROCm) fp32 tensors and raises otherwise -- no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib, conv_plan
from ._lib import BtsHipError, ConvDesc, ConvWgradBatchItem, ConvWgradDesc
from .conv_plan import conv_out_hw, round_up

ACT_NONE, ACT_RELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3


class KernelTrace:
    """Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg).
    Each record: (kernel, tag, algorithmic flops, algorithmic bytes, start event, end event, executed flops).
    Algorithmic = the reference formulation's op count; executed = what the kernel's own formulation issues
    (they differ for the sub-pixel upconv, which needs 4 taps where the reference spends 9)."""

    def __init__(self):
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kern, tag, flops, nbytes, s, e, xflops in self.records:
            d = out.setdefault(kern, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0, xflops=0.0, tags={}))
            ms = s.elapsed_time(e)
            d["launches"] += 1
            d["ms"] += ms
            d["flops"] += flops
            d["bytes"] += nbytes
            d["xflops"] += xflops
            t = d["tags"].setdefault(tag, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0, xflops=0.0))
            t["launches"] += 1
            t["ms"] += ms
            t["flops"] += flops
            t["bytes"] += nbytes
            t["xflops"] += xflops
        return out


_trace: Optional[KernelTrace] = None


def set_trace(t: Optional[KernelTrace]):
    global _trace
    _trace = t


def _launch(kern: str, tag: str, flops: float, nbytes: float, fn, xflops: Optional[float] = None):
    if _trace is None:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = fn()
    e.record()
    _trace.records.append((kern, tag, flops, nbytes, s, e, flops if xflops is None else xflops))
    return rc


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _need(t: torch.Tensor, name: str):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise BtsHipError("bts_amd.%s: expected a CUDA/ROCm tensor (the hot path has no CPU fallback)" % name)
    if t.dtype != torch.float32:
        raise BtsHipError("bts_amd.%s: expected float32, got %s" % (name, t.dtype))


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _rows2d(t: torch.Tensor, name: str) -> Tuple[int, int]:
    """A [npix, C] NHWC view: unit channel stride, arbitrary (>= C) pixel stride."""
    _need(t, name)
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise BtsHipError("bts_amd.%s: expected a [npix, C] view with unit channel stride" % name)
    return t.stride(0), t.shape[1]


def _rows2d_bf16(t: torch.Tensor, name: str) -> Tuple[int, int]:
    """A [npix, C] view of a BFLOAT16 NHWC buffer (a bf16-resident activation): unit channel stride, a pixel stride that is
    a multiple of 4 elements, an 8-byte aligned base -- what the kernels that move four channels per lane need."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise BtsHipError("bts_amd.%s: expected a CUDA/ROCm tensor (the hot path has no CPU fallback)" % name)
    if t.dtype != torch.bfloat16:
        raise BtsHipError("bts_amd.%s: expected bfloat16, got %s" % (name, t.dtype))
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise BtsHipError("bts_amd.%s: expected a [npix, C] view with unit channel stride" % name)
    if t.stride(0) % 4 or t.data_ptr() % 8:
        raise BtsHipError("bts_amd.%s: bf16 rows must be 8-byte aligned (pixel stride %d, a multiple of 4 elements)" % (name, t.stride(0)))
    return t.stride(0), t.shape[1]


def _rows2d_c(t: torch.Tensor, C: int, npix: int, name: str) -> int:
    """The pixel stride of a _rows2d view that a kernel walks as ``npix`` rows of ``C`` channels, 16 bytes per lane:
    C a positive multiple of 4 within the view's width, exactly npix rows, 16-byte aligned rows."""
    stride, width = _rows2d(t, name)
    if C <= 0 or C % 4 or C > width:
        raise BtsHipError("bts_amd.%s: C must be a positive multiple of 4 within the view (%d/%d)" % (name, C, width))
    if t.shape[0] != npix:
        raise BtsHipError("bts_amd.%s: view has %d rows, expected %d" % (name, t.shape[0], npix))
    if stride % 4 or t.data_ptr() % 16:
        raise BtsHipError("bts_amd.%s: rows must be 16-byte aligned (pixel stride %d, a multiple of 4 floats)" % (name, stride))
    return stride


def _channel_vec(v: Optional[torch.Tensor], C: int, name: str, what: str, aligned: bool = True):
    """A per-channel fp32 vector a kernel reads (or writes) C elements of: contiguous, at least C long, and -- for the
    kernels that take it 16 bytes per lane -- 16-byte aligned."""
    _need(v, name)
    if v.dim() != 1 or v.numel() < C or (v.numel() > 1 and v.stride(0) != 1):
        raise BtsHipError("bts_amd.%s: %s must be a contiguous vector of at least %d elements, got %s"
                          % (name, what, C, tuple(v.shape)))
    if aligned and v.data_ptr() % 16:
        raise BtsHipError("bts_amd.%s: %s must be 16-byte aligned" % (name, what))
    return v


def _enqueue(entry: str, anchor: torch.Tensor, args: Sequence = (), trace=None, run=None):
    """Enqueue the C entry point ``entry`` on ``anchor``'s device and current stream, and check its return code.
    ``args``: the prototype's arguments without the stream.  ``run``: a ready closure to call instead (the
    torch-operator bindings).  ``trace`` = (kernel, tag, flops, bytes, executed flops or None): what a KernelTrace
    records for the launch; without an active trace the call is made directly."""
    with torch.cuda.device(anchor.device):
        if _trace is None or trace is None:
            rc = run() if run is not None else getattr(_lib.load(), entry)(*args, _stream(anchor))
        else:
            if run is None:
                fn, stream = getattr(_lib.load(), entry), _stream(anchor)
                run = lambda: fn(*args, stream)
            rc = _launch(trace[0], trace[1], trace[2], trace[3], run, xflops=trace[4])
    _lib.check(rc, entry)


def _check_act3(act: int, who: str):
    if act not in (ACT_NONE, ACT_RELU, ACT_ELU):
        raise BtsHipError("%s: act must be none, ReLU or ELU" % who)


def _e2_vectors(e2, n: int, who: str, what: str = "e2"):
    """The (scale, shift) pair of an e2 (or ``what``) affine over ``n`` channels, checked; (None, None) when absent."""
    if e2 is None:
        return None, None
    es, eb = e2
    _need(es, who)
    _need(eb, who)
    if es.numel() < n or eb.numel() < n:
        raise BtsHipError("%s: %s vectors need %d elements" % (who, what, n))
    return es, eb


def _dense_planes(planes, npix: int, who: str, at_most: int = 4) -> list:
    """One-channel maps given as separate tensors (a planar tail, pack_planes' sources): at most ``at_most`` contiguous
    fp32 maps of ``npix`` floats each."""
    planes = list(planes) if planes else []
    if len(planes) > at_most:
        raise BtsHipError("%s: at most %d planes" % (who, at_most))
    for t in planes:
        _need(t, who)
        if t.numel() != npix or not t.is_contiguous():
            raise BtsHipError("%s: every plane must be one contiguous map of %d floats" % (who, npix))
    return planes


class TilePlan(tuple):
    """(bm, bn, workgroups per frame) of a fused kernel's plan query; all 0 = the layer stays on its default kernel."""
    bm = property(lambda self: self[0])
    bn = property(lambda self: self[1])
    workgroups = property(lambda self: self[2])
    eligible = property(lambda self: self[0] > 0)


# ------------------------------------------------------------------------------ binding of the hot-path operators
# The hot-path operators (LPG, reduction_1x1, reduction -> LPG, the fused convolution) are TORCH OPERATORS:
# torch.ops.bts_hip.* (csrc/torch_ops.cpp, a TORCH_LIBRARY shell over the C ABI -- what the reference's native side does
# with REGISTER_OP / OpKernel, local_planar_guidance.cc:31-72, 116-156, 234-239).  BTS_BINDING=ctypes binds the C ABI
# directly instead (A/B, and what a plan recording listens on: bts_amd/plan.py records through the ctypes proxy).
_BINDING = os.environ.get("BTS_BINDING", "torch").strip().lower()
_autograd_registered = False


def torch_ops():
    """torch.ops.bts_hip, or None when this call must go through the ctypes binding."""
    global _autograd_registered
    if _BINDING != "torch" or _lib.is_recording():
        return None
    t = _lib.load_torch_ops()
    if not _autograd_registered:
        _autograd_registered = True

        def _setup(ctx, inputs, output):
            ctx.save_for_backward(inputs[0])
            ctx.upratio = int(inputs[1])

        def _backward(ctx, grad_depth, grad_abs_min):
            return t.lpg_backward(ctx.saved_tensors[0], grad_depth.contiguous(), ctx.upratio), None

        torch.library.register_autograd("bts_hip::lpg", _backward, setup_context=_setup)

        def _loss_setup(ctx, inputs, output):
            est, gt, mask, ctx.gt_min, ctx.kind, ctx.param = inputs
            ctx.save_for_backward(est, gt, mask, output[1])

        def _loss_backward(ctx, grad_loss, grad_stats):
            est, gt, mask, stats = ctx.saved_tensors
            g = t.depth_loss_backward(est, gt, mask, ctx.gt_min, ctx.kind, ctx.param, stats, grad_loss.contiguous())
            return g, None, None, None, None, None

        torch.library.register_autograd("bts_hip::depth_loss", _loss_backward, setup_context=_loss_setup)

        # the out-of-place training forms of the reduction scales: backward = bts_hip::reduc_bwd + one wgrad per layer
        def _reduc_setup(lpg):
            def setup(ctx, inputs, output):
                if lpg:
                    x2d, ctx.B, ctx.h, ctx.w, weights, packs, ctx.md, ctx.k = inputs
                else:
                    x2d, ctx.B, ctx.h, ctx.w, weights, packs, ctx.md = inputs
                    ctx.k = 0
                ctx.save_for_backward(x2d, *weights)
                ctx.packs = list(packs)
                ctx.need = (x2d.requires_grad, [wt.requires_grad for wt in weights])
            return setup

        def _reduc_backward(lpg):
            def backward(ctx, grad_out, *unused):
                x2d, *weights = ctx.saved_tensors
                dx, dws = reduc_train_backward(x2d, ctx.B, ctx.h, ctx.w, weights, ctx.packs, ctx.md, ctx.k, grad_out,
                                               ctx.need[0], ctx.need[1])
                if dx is not None:
                    dx = dx.view(x2d.shape[0], -1)
                    if dx.shape[1] != x2d.shape[1]:                       # a view wider than the chain reads
                        dx = F.pad(dx, (0, x2d.shape[1] - dx.shape[1]))
                return (dx, None, None, None, dws, [None] * len(ctx.packs), None) + ((None,) if lpg else ())
            return backward

        torch.library.register_autograd("bts_hip::reduc_lpg_train", _reduc_backward(True), setup_context=_reduc_setup(True))
        torch.library.register_autograd("bts_hip::reduction_1x1_train", _reduc_backward(False), setup_context=_reduc_setup(False))
    return t


def _op(fn):
    """Run a torch operator; its TORCH_CHECK failures surface as BtsHipError like the ctypes binding's return codes."""
    try:
        fn()
    except BtsHipError:
        raise
    except RuntimeError as e:
        raise BtsHipError(str(e).split("\n")[0]) from None
    return 0


# ------------------------------------------------------------------------------ LPG
def lpg_forward(plane_eq: torch.Tensor, upratio: int, abs_min: Optional[torch.Tensor] = None) -> torch.Tensor:
    """local_planar_guidance.forward (reference bts.py:149-173): [B,4,h,w] -> [B,h*k,w*k]."""
    _need(plane_eq, "lpg_forward")
    if plane_eq.dim() != 4 or plane_eq.shape[1] != 4:
        raise BtsHipError("lpg_forward: plane_eq must be [B,4,h,w]")
    tops = torch_ops()
    if tops is not None:                         # differentiable (autograd registered on bts_hip::lpg)
        box = []
        _op(lambda: box.append(tops.lpg(plane_eq, int(upratio))))
        out, am = box[0]
        if abs_min is not None:
            abs_min.copy_(am.detach())
        return out
    plane_eq = plane_eq.contiguous()
    B, _, h, w = plane_eq.shape
    k = int(upratio)
    out = torch.empty((B, h * k, w * k), dtype=torch.float32, device=plane_eq.device)
    _enqueue("bts_lpg_fwd_f32", plane_eq, (_ptr(plane_eq), B, h, w, k, _ptr(out), _ptr(abs_min)))
    return out


def lpg_backward(plane_eq: torch.Tensor, grad_depth: torch.Tensor, upratio: int) -> torch.Tensor:
    """Gradient of local_planar_guidance.forward w.r.t. plane_eq (what autograd through bts.py:149-173 yields)."""
    _need(plane_eq, "lpg_backward")
    _need(grad_depth, "lpg_backward")
    plane_eq = plane_eq.contiguous()
    grad_depth = grad_depth.contiguous()
    B, _, h, w = plane_eq.shape
    k = int(upratio)
    if tuple(grad_depth.shape) != (B, h * k, w * k):
        raise BtsHipError("lpg_backward: grad_depth must be [B,h*k,w*k]")
    g = torch.empty_like(plane_eq)
    _enqueue("bts_lpg_bwd_f32", plane_eq, (_ptr(plane_eq), _ptr(grad_depth), B, h, w, k, _ptr(g)))
    return g


class LpgFunction(torch.autograd.Function):
    """autograd shell over the two native LPG kernels (the reference pairs LocalPlanarGuidance with a registered
    LocalPlanarGuidanceGrad, tensorflow/custom_layer/_local_planar_guidance_grad.py:22-33)."""

    @staticmethod
    def forward(ctx, plane_eq, upratio, abs_min):
        ctx.save_for_backward(plane_eq)
        ctx.upratio = int(upratio)
        return lpg_forward(plane_eq.detach(), upratio, abs_min=abs_min)

    @staticmethod
    def backward(ctx, grad_depth):
        (plane_eq,) = ctx.saved_tensors
        return lpg_backward(plane_eq, grad_depth, ctx.upratio), None, None


# ------------------------------------------------------------------------------ training losses
_LOSS_KINDS = {"silog": 0, "l1": 1, 0: 0, 1: 1}


def _depth_loss_fwd(est, gt, mask, gt_min, kind, param):
    """ctypes binding of bts_depth_loss_fwd_f32 on checked, contiguous tensors: (loss 0-d fp32, stats [4] fp64)."""
    npix = est.numel()
    nws = _lib.load_real().bts_depth_loss_ws_doubles(npix)
    ws = torch.empty(nws, dtype=torch.float64, device=est.device)
    stats = torch.empty(4, dtype=torch.float64, device=est.device)
    loss = torch.empty((), dtype=torch.float32, device=est.device)
    _enqueue("bts_depth_loss_fwd_f32", est, (_ptr(est), _ptr(gt), _ptr(mask), gt_min, npix, kind, param, _ptr(ws), nws, _ptr(stats),
                                             _ptr(loss)))
    return loss, stats


def _depth_loss_bwd(est, gt, mask, gt_min, kind, param, stats, grad_loss):
    # the gradient starts at est's offset from a 16-byte line, so that the kernel can store 16 bytes per lane next to its loads
    off = (est.data_ptr() & 15) >> 2
    g = torch.empty(est.numel() + off, dtype=torch.float32, device=est.device)[off:].view(est.shape)
    _enqueue("bts_depth_loss_bwd_f32", est, (_ptr(est), _ptr(gt), _ptr(mask), gt_min, est.numel(), kind, param, _ptr(stats),
                                             _ptr(grad_loss), _ptr(g)))
    return g


class DepthLossFunction(torch.autograd.Function):
    """autograd shell over the two native loss kernels for the ctypes binding (the torch binding registers the same
    pair on bts_hip::depth_loss).  The upstream gradient stays on the device: the backward kernel reads it there."""

    @staticmethod
    def forward(ctx, est, gt, mask, gt_min, kind, param):
        loss, stats = _depth_loss_fwd(est, gt, mask, gt_min, kind, param)
        ctx.save_for_backward(est, gt, mask, stats)
        ctx.cfg = (gt_min, kind, param)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, grad_stats):
        est, gt, mask, stats = ctx.saved_tensors
        gt_min, kind, param = ctx.cfg
        g = _depth_loss_bwd(est, gt, mask, gt_min, kind, param, stats, grad_loss.to(torch.float32).contiguous())
        return g, None, None, None, None, None


def depth_loss(est: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, gt_min: float = 1.0,
               kind="silog", param: float = 0.85, return_stats: bool = False):
    """silog_loss / depth_l1_loss of the reference (bts.py:41-63) over the valid pixels of the whole batch, on the native
    kernels of csrc/loss.hip: no boolean gather, so nothing waits for the host; fp64 sums in a fixed order.

    ``kind``: "silog" (``param`` = variance_focus) or "l1" (``param`` = inbalance_to_closer).  A pixel is valid where
    ``mask`` (bool / uint8, est's shape) is set, or -- ``mask=None`` -- where ``gt > gt_min``.  Differentiable in ``est``
    (``gt`` and ``mask`` get no gradient).  Returns the 0-dim fp32 loss; with ``return_stats`` also the [4] fp64 device
    tensor (valid count, mean log error, its second moment, loss).  No valid pixel, or a silog variance <= 0: loss 0 and
    a zero gradient (torch gives NaN there)."""
    _need(est, "depth_loss")
    _need(gt, "depth_loss")
    if kind not in _LOSS_KINDS:
        raise BtsHipError("depth_loss: kind must be 'silog' or 'l1', got %r" % (kind,))
    if est.shape != gt.shape or est.device != gt.device or est.numel() == 0:
        raise BtsHipError("depth_loss: est %s and gt %s must be non-empty maps of one shape on one device" % (tuple(est.shape), tuple(gt.shape)))
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype not in (torch.bool, torch.uint8):
            raise BtsHipError("depth_loss: mask must be a CUDA/ROCm bool or uint8 tensor (or None: gt > gt_min)")
        if mask.shape != est.shape or mask.device != est.device:
            raise BtsHipError("depth_loss: mask %s must have est's shape %s and device" % (tuple(mask.shape), tuple(est.shape)))
        mask = mask.contiguous()
    est_c, gt_c = est.contiguous(), gt.detach().contiguous()     # autograd carries the gradient back into est's own layout
    args = (est_c, gt_c, mask, float(gt_min), _LOSS_KINDS[kind], float(param))
    tops = torch_ops()
    if tops is not None:
        box = []
        _op(lambda: box.append(tops.depth_loss(*args)))
        loss, stats = box[0]
    else:
        loss, stats = DepthLossFunction.apply(*args)
    return (loss, stats.detach()) if return_stats else loss


def lpg_fused_forward(plane4: torch.Tensor, B: int, h: int, w: int, upratio: int, max_depth: float,
                      normalize: bool, depth_scaled: torch.Tensor, ds_out: Optional[torch.Tensor] = None,
                      ds_factor: int = 1, ds_pix_stride: int = 1, abs_min: Optional[torch.Tensor] = None):
    """LPG + glue of bts.forward (reference bts.py:250-256): plane4 [B*h*w,4] -> depth/max_depth."""
    _need(plane4, "lpg_fused_forward")
    _need(depth_scaled, "lpg_fused_forward")
    k = int(upratio)
    if plane4.numel() != B * h * w * 4 or not plane4.is_contiguous():
        raise BtsHipError("lpg_fused_forward: plane4 must be contiguous [B*h*w,4]")
    if depth_scaled.numel() != B * h * k * w * k or not depth_scaled.is_contiguous():
        raise BtsHipError("lpg_fused_forward: depth_scaled must be contiguous [B,1,h*k,w*k]")
    nbytes = 4.0 * (4 * B * h * w + B * h * k * w * k + (B * h * k * w * k // (ds_factor * ds_factor) if ds_out is not None else 0))
    _enqueue("bts_lpg_fused_fwd_f32", plane4,
             (_ptr(plane4), B, h, w, k, int(bool(normalize)), float(max_depth), _ptr(depth_scaled), _ptr(ds_out), int(ds_factor),
              int(ds_pix_stride), _ptr(abs_min)),
             trace=("lpg_fwd_kernel<%d,fused>" % k, "lpg", 8.0 * B * h * k * w * k, nbytes, None))
    return depth_scaled


# ------------------------------------------------------------------------ reduction
def reduc_chain(num_in: int, num_out: int) -> List[Tuple[int, int]]:
    """(cin, cout_real) per layer, mirroring the while-loop of reduction_1x1.__init__ (bts.py:105-122).
    The last entry's cout is filled by the caller's weights (3 or 1)."""
    layers = []
    while num_out >= 4:
        if num_out < 8:
            layers.append((num_in, -1))
            break
        layers.append((num_in, num_out))
        num_in, num_out = num_out, num_out // 2
    return layers


def reduc_uses_mfma16(c_in: int, c_first_out: int) -> bool:
    """The narrow chains (bts_size 512: 2x2 64->32.., 1x1 32->16..; every chain of bts_size 256) run on the 16x16x4-MFMA kernel
    (csrc/reduc.hip)."""
    return (c_in, c_first_out) in ((64, 32), (32, 16), (64, 64), (16, 8))      # the last two: bts_size 256


def _pack_reduc_layers(mats: Sequence[torch.Tensor], narrow: bool) -> torch.Tensor:
    """Fragment order of a chain's [cout, cin] matrices (any dtype: the index tables of reduc_train_packs run through it)."""
    parts = []
    for w in mats:
        cout, cin = w.shape
        assert cin % 8 == 0, "reduction chain widths are multiples of 8"
        if narrow:
            mt, g = (cout + 15) // 16, (cin + 15) // 16
            wp = torch.zeros((mt * 16, g * 16), dtype=w.dtype, device=w.device)
            wp[:cout, :cin] = w
            # (mt, i, g, kq, q4) -> (mt, g, kq, i, q4)
            parts.append(wp.view(mt, 16, g, 4, 4).permute(0, 2, 3, 1, 4).contiguous().view(-1))
        else:
            mt = (cout + 31) // 32
            wp = torch.zeros((mt * 32, cin), dtype=w.dtype, device=w.device)
            wp[:cout] = w
            # (mt, i, g, h, q) -> (mt, g, h, i, q)
            parts.append(wp.view(mt, 32, cin // 8, 2, 4).permute(0, 2, 3, 1, 4).contiguous().view(-1))
    return torch.cat(parts).contiguous()


def pack_reduc_weights(weights: Sequence[torch.Tensor], wide: Optional[bool] = None) -> torch.Tensor:
    """Pack a reduction chain's 1x1 weights ([cout,cin,1,1] each) into MFMA fragment order.

    Wide chains (first layer 128 -> ..): per layer (K=cin, rows padded to 32*MT) float4 index
    ((mt*(K/8)+g)*64 + 32*h + i) holds W[32*mt+i][4*(2g+h) + 0..3] -- lane (i,h) of v_mfma_f32_32x32x2_f32's A operand
    for the four k-steps of group g.  Narrow chains (see reduc_uses_mfma16): rows padded to 16*MT, K to 16*G, float4
    index ((mt*G+g)*64 + 16*kq + i) holds W[16*mt+i][16*g + 4*kq + 0..3] -- lane (i,kq) of v_mfma_f32_16x16x4_f32.
    ``wide=True`` forces the first order for any chain: what the backward kernel (bts_reduc_bwd_f32) reads."""
    narrow = reduc_uses_mfma16(weights[0].shape[1], weights[0].shape[0]) if wide is None else not wide
    return _pack_reduc_layers([w.reshape(w.shape[0], w.shape[1]).float() for w in weights], narrow)


def _reduc_transposed(mats: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """W_l^T in reverse layer order, the last layer's 3 (1) outputs zero-padded to 8 columns."""
    out = []
    for w in reversed(list(mats)):
        wt = w.t()
        if wt.shape[1] % 8:
            wt = F.pad(wt, (0, 8 - wt.shape[1] % 8))
        out.append(wt)
    return out


def pack_reduc_weights_bwd(weights: Sequence[torch.Tensor]) -> torch.Tensor:
    """The second fragment buffer of bts_reduc_bwd_f32: the backward walk dy_{l-1} = W_l^T dpre_l is the forward chain
    mirrored, so its fragments are pack_reduc_weights' wide order applied to W_l^T, last layer first."""
    return _pack_reduc_layers(_reduc_transposed([w.reshape(w.shape[0], w.shape[1]).float() for w in weights]), False)


def unpack_reduc_weights(frag: torch.Tensor, shapes: Sequence[Tuple[int, int]]) -> List[torch.Tensor]:
    """Inverse of the wide fragment order: ``shapes`` = (rows, cols) per packed matrix, in buffer order."""
    out, off = [], 0
    for rows, cols in shapes:
        mt = (rows + 31) // 32
        n = mt * 32 * cols
        out.append(frag[off:off + n].view(mt, cols // 8, 2, 32, 4).permute(0, 3, 1, 2, 4).reshape(mt * 32, cols)[:rows])
        off += n
    assert off == frag.numel(), "fragment buffer does not match the shapes"
    return out


REDUC_TRAIN_CHAINS = ((128, 128, 8), (128, 64, 4), (64, 32, 2), (32, 16, 0))     # (c_in, c_first_out, upratio; 0 = final)


def reduc_train_supported(c_in: int, c_first_out: int, upratio: int) -> bool:
    """Whether bts_reduc_bwd_f32 is built for this chain (bts_size 512's four; upratio 0 = the final chain)."""
    return (int(c_in), int(c_first_out), int(upratio)) in REDUC_TRAIN_CHAINS


def reduc_train_cols(c_in: int, c_first_out: int) -> Tuple[List[Tuple[int, int]], int]:
    """Column table of bts_reduc_bwd_f32's row buffers: ([(first column, width) per layer], YC).  Y holds the hidden
    layers (all entries but the last, YC columns), G every layer (YC + 4 columns: the last layer padded to 4)."""
    cols, c = [], 0
    for _, cout in reduc_chain(c_in, c_first_out):
        width = cout if cout > 0 else 4
        cols.append((c, width))
        c += width
    return cols, c - 4


_TRAIN_PACK_INDEX = {}


def reduc_train_packs(weights: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(w_frag, w_frag_wide, wt_frag) for one chain in TWO launches: pack_reduc_weights(weights),
    pack_reduc_weights(weights, wide=True) and pack_reduc_weights_bwd(weights) are three fixed permutations (with zero
    padding) of the same numbers, so one gather through a cached index table fills all of them.  On the wide chains the
    first two are one buffer."""
    shapes = tuple((w.shape[0], w.shape[1]) for w in weights)
    dev = weights[0].device
    key = (shapes, str(dev))
    hit = _TRAIN_PACK_INDEX.get(key)
    if hit is None:
        fakes, off = [], 1                                     # 0 = the zero every padding position reads
        for co, ci in shapes:
            fakes.append(torch.arange(off, off + co * ci, dtype=torch.int64).view(co, ci))
            off += co * ci
        narrow = reduc_uses_mfma16(shapes[0][1], shapes[0][0])
        wide = _pack_reduc_layers(fakes, False)
        wt = _pack_reduc_layers(_reduc_transposed(fakes), False)
        parts = ([_pack_reduc_layers(fakes, True)] if narrow else []) + [wide, wt]
        hit = _TRAIN_PACK_INDEX[key] = (torch.cat(parts).to(dev), [p.numel() for p in parts])
    idx, sizes = hit
    src = torch.cat([torch.zeros(1, dtype=torch.float32, device=dev)] + [w.detach().reshape(-1).float() for w in weights])
    packs = list(torch.split(src[idx], sizes))
    if len(packs) == 2:
        packs.insert(0, packs[0])
    return tuple(packs)


def reduc_forward_nhwc(x2d: torch.Tensor, c_in: int, c_first_out: int, w_frag: torch.Tensor, max_depth: float,
                       is_final: bool, normalize: bool, out: torch.Tensor):
    """x2d: [npix, >=c_in] NHWC view; out: [npix,4] (non-final) or [npix] (final), contiguous."""
    stride, cview = _rows2d(x2d, "reduc_forward_nhwc")
    _need(out, "reduc_forward_nhwc")
    _need(w_frag, "reduc_forward_nhwc")
    if cview < c_in:
        raise BtsHipError("reduc_forward_nhwc: view has %d channels, chain needs %d" % (cview, c_in))
    npix = x2d.shape[0]
    if out.numel() != npix * (1 if is_final else 4) or not out.is_contiguous():
        raise BtsHipError("reduc_forward_nhwc: bad output size")
    chain = reduc_chain(c_in, c_first_out)
    macs = sum(ci * (co if co > 0 else (1 if is_final else 3)) for ci, co in chain)
    nbytes = 4.0 * (npix * (c_in + (1 if is_final else 4)) + macs)
    tops = torch_ops()
    run = None
    if tops is not None:
        run = lambda: _op(lambda: tops.reduction_1x1(x2d, int(c_in), int(c_first_out), w_frag, float(max_depth), bool(is_final),
                                                     bool(normalize), out))
    _enqueue("bts_reduc_fwd_f32", x2d,
             (_ptr(x2d), stride, npix, int(c_in), int(c_first_out), _ptr(w_frag), w_frag.numel(), float(max_depth), int(bool(is_final)),
              int(bool(normalize)), _ptr(out)),
             trace=("reduc_fwd_kernel<%d,%d>" % (c_in, c_first_out), "reduc", 2.0 * npix * macs, nbytes, None), run=run)
    return out


def reduc_lpg_forward(x2d: torch.Tensor, B: int, h: int, w: int, c_in: int, c_first_out: int, w_frag: torch.Tensor,
                      max_depth: float, upratio: int, depth_scaled: torch.Tensor, ds_out: Optional[torch.Tensor] = None,
                      abs_min: Optional[torch.Tensor] = None, plane4: Optional[torch.Tensor] = None):
    """One scale of the decoder's LPG stage in ONE launch (bts_reduc_lpg_fwd_f32): reduction_1x1 chain -> normalize ->
    LPG -> /max_depth (+ the nearest-downsampled plane, + abs_min).  x2d: [B*h*w, >=c_in] NHWC view; depth_scaled:
    contiguous [B,1,h*k,w*k]; ds_out: contiguous [B*2h*2w] plane (k = 8, 4) or None."""
    stride, cview = _rows2d(x2d, "reduc_lpg_forward")
    _need(depth_scaled, "reduc_lpg_forward")
    _need(w_frag, "reduc_lpg_forward")
    k = int(upratio)
    npix = B * h * w
    if cview < c_in or x2d.shape[0] != npix:
        raise BtsHipError("reduc_lpg_forward: bad input view %s for B=%d %dx%d, %d channels" % (tuple(x2d.shape), B, h, w, c_in))
    if depth_scaled.numel() != npix * k * k or not depth_scaled.is_contiguous():
        raise BtsHipError("reduc_lpg_forward: depth_scaled must be contiguous [B,1,h*k,w*k]")
    if ds_out is not None:
        _need(ds_out, "reduc_lpg_forward")
        if k == 2 or ds_out.numel() != npix * 4 or not ds_out.is_contiguous():
            raise BtsHipError("reduc_lpg_forward: ds_out must be a contiguous [B,2h,2w] plane (k = 8 or 4 only)")
    if plane4 is not None and (plane4.numel() != npix * 4 or not plane4.is_contiguous()):
        raise BtsHipError("reduc_lpg_forward: plane4 must be contiguous [B*h*w,4]")
    chain = reduc_chain(c_in, c_first_out)
    macs = sum(ci * (co if co > 0 else 3) for ci, co in chain)
    nbytes = 4.0 * (npix * c_in + macs + npix * k * k + (npix * 4 if ds_out is not None else 0))
    tops = torch_ops()
    run = None
    if tops is not None:
        run = lambda: _op(lambda: tops.reduc_lpg(x2d, B, h, w, int(c_in), int(c_first_out), w_frag, float(max_depth), k,
                                                 depth_scaled, ds_out, abs_min, plane4))
    _enqueue("bts_reduc_lpg_fwd_f32", x2d,
             (_ptr(x2d), stride, B, h, w, int(c_in), int(c_first_out), _ptr(w_frag), w_frag.numel(), float(max_depth), k, _ptr(plane4),
              _ptr(depth_scaled), _ptr(ds_out), _ptr(abs_min)),
             trace=("reduc_lpg_kernel<%d,%d,k%d>" % (c_in, c_first_out, k), "reduc_lpg", 2.0 * npix * macs + 8.0 * npix * k * k, nbytes, None),
             run=run)
    return depth_scaled


# ------------------------------------------------------------------------ reduction, training
def nhwc_rows(x: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """[B,C,H,W] (any strides) -> ([B*H*W, C4] NHWC rows with C padded to a multiple of 4, C4).
    A channels_last tensor with C % 4 == 0 is viewed, not copied -- and so is a CHANNEL SLICE of one (what autograd hands
    back for the inputs of a torch.cat, and what a dense block's layers read): the kernels take a pixel stride."""
    B, C, H, W = x.shape
    c4 = round_up(C, 4)
    if c4 == C and B * H * W > 0 and x.stride(1) == 1 and W > 1 and H > 1:
        ct = x.stride(3)
        if (ct >= C and ct % 4 == 0 and x.stride(2) == W * ct and (B == 1 or x.stride(0) == H * W * ct)
                and x.data_ptr() % 16 == 0):
            return x.as_strided((B * H * W, C), (ct, 1)), c4
    rows = x.permute(0, 2, 3, 1)
    if c4 != C:
        rows = F.pad(rows, (0, c4 - C))
    return rows.contiguous().view(B * H * W, c4), c4


def reduc_bwd_max_waves(c_in: int, c_first_out: int, upratio: int) -> int:
    """The most waves one bts_reduc_bwd_f32 launch runs for this chain (each walks 32-pixel tiles in a grid-stride loop)."""
    n = _lib.load_real().bts_reduc_bwd_max_waves(int(c_in), int(c_first_out), int(upratio))
    if n < 0:
        _lib.check(n, "bts_reduc_bwd_max_waves")
    return n


def reduc_backward(x2d: torch.Tensor, B: int, h: int, w: int, c_in: int, c_first_out: int, w_frag_wide: torch.Tensor,
                   wt_frag: torch.Tensor, max_depth: float, upratio: int, grad_out: torch.Tensor, Y: torch.Tensor,
                   G: Optional[torch.Tensor] = None, dx2d: Optional[torch.Tensor] = None):
    """Backward-data of one reduction scale in ONE launch (bts_reduc_bwd_f32).  x2d: [B*h*w, >=c_in] NHWC view;
    ``upratio`` 8 / 4 / 2: grad_out is the gradient of depth_scaled [B,1,h*k,w*k]; 0: the final chain, grad_out
    [B,1,h,w].  Fills Y [npix, YC], and when given G [npix, YC+4] and dx2d ([npix, >=c_in] view, any pixel stride that
    is a multiple of 4; columns >= c_in untouched).  Column tables: reduc_train_cols."""
    stride, cview = _rows2d(x2d, "reduc_backward")
    for t in (w_frag_wide, wt_frag, grad_out, Y):
        _need(t, "reduc_backward")
    k = int(upratio)
    npix = B * h * w
    cols, yc = reduc_train_cols(c_in, c_first_out)
    if cview < c_in or x2d.shape[0] != npix:
        raise BtsHipError("reduc_backward: bad input view %s for B=%d %dx%d, %d channels" % (tuple(x2d.shape), B, h, w, c_in))
    if grad_out.numel() != npix * max(k * k, 1) or not grad_out.is_contiguous():
        raise BtsHipError("reduc_backward: grad_out must be contiguous with %d elements" % (npix * max(k * k, 1)))
    if tuple(Y.shape) != (npix, yc) or not Y.is_contiguous():
        raise BtsHipError("reduc_backward: Y must be contiguous [%d, %d]" % (npix, yc))
    if G is not None:
        _need(G, "reduc_backward")
        if tuple(G.shape) != (npix, yc + 4) or not G.is_contiguous():
            raise BtsHipError("reduc_backward: G must be contiguous [%d, %d]" % (npix, yc + 4))
    dxs = 0
    if dx2d is not None:
        dxs, dxc = _rows2d(dx2d, "reduc_backward")
        if dxc < c_in or dx2d.shape[0] != npix or dxs % 4:
            raise BtsHipError("reduc_backward: dx2d must be a [%d, >=%d] view with a pixel stride that is a multiple of 4" % (npix, c_in))
    macs = sum(ci * co for ci, (_, co) in zip([c for c, _ in reduc_chain(c_in, c_first_out)], cols))
    nbytes = 4.0 * (npix * (c_in + yc + (yc + 4 if G is not None else 0) + (c_in if dx2d is not None else 0) + max(k * k, 1)) + 2 * macs)
    tops = torch_ops()
    run = None
    if tops is not None:
        run = lambda: _op(lambda: tops.reduc_bwd(x2d, B, h, w, int(c_in), int(c_first_out), w_frag_wide, wt_frag, float(max_depth), k,
                                                 grad_out, dx2d, G, Y))
    _enqueue("bts_reduc_bwd_f32", x2d,
             (_ptr(x2d), stride, B, h, w, int(c_in), int(c_first_out), _ptr(w_frag_wide), w_frag_wide.numel(), _ptr(wt_frag),
              wt_frag.numel(), float(max_depth), k, _ptr(grad_out), _ptr(dx2d), dxs, _ptr(G), _ptr(Y)),
             trace=("reduc_bwd_kernel<%d,%d,k%d>" % (c_in, c_first_out, k), "reduc_bwd", 4.0 * npix * macs + 12.0 * npix * k * k, nbytes, None),
             run=run)


class BatchCache:
    """A small least-recently-used map from a batch's key to its WgradBatch (plan, host table, device table): bounded,
    so that a run which keeps changing shapes or freeze masks does not accumulate tables."""

    def __init__(self, max_entries: int):
        import collections
        self.max_entries, self._d = max_entries, collections.OrderedDict()

    def __len__(self):
        return len(self._d)

    def get(self, key):
        v = self._d.get(key)
        if v is not None:
            self._d.move_to_end(key)
        return v

    def put(self, key, value):
        self._d[key] = value
        while len(self._d) > self.max_entries:
            self._d.popitem(last=False)
        return value


# (device, x pixel stride, x channels, B, h, w, chain, need mask, workspace floats) -> WgradBatch; the plan depends on the
# workspace size, so it is part of the key
_REDUC_WGRAD_BATCHES = BatchCache(32)


def _reduc_wgrad_batch(x2d, Y, G, B, h, w, weights, cols, need_dw, ws):
    """The weight gradients of one scale's layers as ONE batched launch: bases x2d's storage rows, Y, G and a flat DW.
    The batch (plan + device table) is built once per geometry and need mask; later steps only launch."""
    dev = x2d.device
    widths = [width * wt.shape[1] for wt, (_, width) in zip(weights, cols)]
    total = sum(wd for wd, nd in zip(widths, need_dw) if nd)
    DW = torch.empty(total, dtype=torch.float32, device=dev)
    xs = x2d.stride(0)
    xbase = x2d.as_strided(((x2d.shape[0] - 1) * xs + x2d.shape[1],), (1,))     # the storage span the view covers, flat
    ws_floats = 0 if ws is None else ws.numel()
    key = (str(dev), xs, x2d.shape[1], B, h, w, tuple(tuple(wt.shape[:2]) for wt in weights), tuple(bool(nd) for nd in need_dw), ws_floats)
    batch = _REDUC_WGRAD_BATCHES.get(key)
    if batch is None:
        problems, at = [], 0
        for l, (wt, (c0, width)) in enumerate(zip(weights, cols)):
            if not need_dw[l]:
                continue
            cin_l = wt.shape[1]
            src = x2d[:, :cin_l] if l == 0 else Y[:, cols[l - 1][0]:cols[l - 1][0] + cin_l]
            problems.append(dict(x=src, dy=G[:, c0:c0 + width], dw=DW[at:at + widths[l]], B=B, h_in=h, w_in=w, c_in=cin_l,
                                 c_out=width, ksize=1))
            at += widths[l]
        batch = _REDUC_WGRAD_BATCHES.put(key, WgradBatch(problems, [xbase, Y, G, DW], ws_floats, tag="reduc.wgrad"))
    got = iter(batch.run([xbase, Y, G, DW], ws))
    return [next(got)[:wt.shape[0]].reshape(wt.shape[0], wt.shape[1], 1, 1) if nd else None for wt, nd in zip(weights, need_dw)]


def reduc_train_backward(x2d: torch.Tensor, B: int, h: int, w: int, weights: Sequence[torch.Tensor], packs, max_depth: float,
                         upratio: int, grad_out: torch.Tensor, need_dx: bool, need_dw: Sequence[bool],
                         ws: Optional[torch.Tensor] = None, batched_wgrad: bool = False):
    """All gradients of one scale: one bts_reduc_bwd_f32 launch, then one bts_conv_wgrad_f32 (ksize 1) per layer whose
    weight wants a gradient, on column slices of the row buffers -- or, with ``batched_wgrad``, one
    bts_conv_wgrad_batch_f32 for all of them.  Returns (dx [B,h,w,c_in] or None, [dW or None])."""
    c_in, c_first = weights[0].shape[1], weights[0].shape[0]
    npix = B * h * w
    cols, yc = reduc_train_cols(c_in, c_first)
    dev = x2d.device
    any_dw = any(need_dw)
    Y = torch.empty((npix, yc), dtype=torch.float32, device=dev)
    G = torch.empty((npix, yc + 4), dtype=torch.float32, device=dev) if any_dw else None
    dx = torch.empty((B, h, w, c_in), dtype=torch.float32, device=dev) if need_dx else None
    reduc_backward(x2d, B, h, w, c_in, c_first, packs[1], packs[2], max_depth, upratio, grad_out.contiguous(), Y, G,
                   None if dx is None else dx.view(npix, c_in))
    if batched_wgrad:
        return dx, (_reduc_wgrad_batch(x2d, Y, G, B, h, w, weights, cols, need_dw, ws) if any_dw else [None] * len(weights))
    dws = []
    for l, (wt, (c0, width)) in enumerate(zip(weights, cols)):
        if not need_dw[l]:
            dws.append(None)
            continue
        cin_l = wt.shape[1]
        src = x2d[:, :cin_l] if l == 0 else Y[:, cols[l - 1][0]:cols[l - 1][0] + cin_l]
        g = conv_wgrad(src, B, h, w, cin_l, G[:, c0:c0 + width], width, 1, ws=ws, tag="reduc.wgrad")
        dws.append(g[:wt.shape[0]].reshape(wt.shape[0], cin_l, 1, 1))
    return dx, dws


def _check_train_chain(weights, upratio):
    c_in, c_first = weights[0].shape[1], weights[0].shape[0]
    if not reduc_train_supported(c_in, c_first, upratio):
        raise BtsHipError("reduction training kernels: chain (%d,%d) at upratio %d is not built" % (c_in, c_first, upratio))
    return c_in, c_first


class ReducLpgFunction(torch.autograd.Function):
    """One LPG scale of the decoder in train() mode as ONE autograd node: forward is the inference launch
    (bts_reduc_lpg_fwd_f32, reduction_1x1 -> normalize -> LPG -> /max_depth), backward bts_reduc_bwd_f32 plus one
    bts_conv_wgrad_f32 per layer.  x: [B,C,h,w] (channels_last is read in place); packs: reduc_train_packs(weights);
    abs_min: optional 0-d tensor that receives min |den|; ws: optional wgrad split workspace.  Returns depth_scaled
    [B,1,h*k,w*k]."""

    @staticmethod
    def forward(ctx, x, max_depth, upratio, packs, abs_min, ws, *weights):
        c_in, c_first = _check_train_chain(weights, int(upratio))
        if int(upratio) == 0:
            raise BtsHipError("ReducLpgFunction: upratio must be 8, 4 or 2 (the final chain is ReducFinalFunction)")
        _need(x, "ReducLpgFunction")
        B, C, h, w = x.shape
        if C != c_in:
            raise BtsHipError("ReducLpgFunction: input has %d channels, the chain reads %d" % (C, c_in))
        k = int(upratio)
        x2d, _ = nhwc_rows(x.detach())
        out = torch.empty((B, 1, h * k, w * k), dtype=torch.float32, device=x.device)
        reduc_lpg_forward(x2d[:, :c_in], B, h, w, c_in, c_first, packs[0], max_depth, k, out, abs_min=abs_min)
        ctx.save_for_backward(x2d, *weights)
        ctx.cfg = (B, h, w, float(max_depth), k, packs, ws)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return ReducLpgFunction.backward_impl(ctx, grad_out, False)

    @staticmethod
    def backward_impl(ctx, grad_out, batched_wgrad):
        x2d, *weights = ctx.saved_tensors
        B, h, w, md, k, packs, ws = ctx.cfg
        dx, dws = reduc_train_backward(x2d, B, h, w, weights, packs, md, k, grad_out, ctx.needs_input_grad[0],
                                       ctx.needs_input_grad[6:], ws, batched_wgrad=batched_wgrad)
        return (None if dx is None else dx.permute(0, 3, 1, 2), None, None, None, None, None) + tuple(dws)


class ReducLpgBatchedFunction(torch.autograd.Function):
    """ReducLpgFunction whose backward computes the layers' weight gradients in one batched launch."""
    forward = staticmethod(ReducLpgFunction.forward)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return ReducLpgFunction.backward_impl(ctx, grad_out, True)


class ReducFinalFunction(torch.autograd.Function):
    """reduc1x1 (the final chain, 32 -> 16 -> 8 -> 1 + sigmoid) in train() mode as one autograd node: forward
    bts_reduc_fwd_f32, backward bts_reduc_bwd_f32 + one wgrad per layer.  Returns [B,1,h,w]."""

    @staticmethod
    def forward(ctx, x, max_depth, packs, ws, *weights):
        c_in, c_first = _check_train_chain(weights, 0)
        _need(x, "ReducFinalFunction")
        B, C, h, w = x.shape
        if C != c_in:
            raise BtsHipError("ReducFinalFunction: input has %d channels, the chain reads %d" % (C, c_in))
        x2d, _ = nhwc_rows(x.detach())
        out = torch.empty((B, 1, h, w), dtype=torch.float32, device=x.device)
        reduc_forward_nhwc(x2d[:, :c_in], c_in, c_first, packs[0], max_depth, True, False, out)
        ctx.save_for_backward(x2d, *weights)
        ctx.cfg = (B, h, w, float(max_depth), packs, ws)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return ReducFinalFunction.backward_impl(ctx, grad_out, False)

    @staticmethod
    def backward_impl(ctx, grad_out, batched_wgrad):
        x2d, *weights = ctx.saved_tensors
        B, h, w, md, packs, ws = ctx.cfg
        dx, dws = reduc_train_backward(x2d, B, h, w, weights, packs, md, 0, grad_out, ctx.needs_input_grad[0],
                                       ctx.needs_input_grad[4:], ws, batched_wgrad=batched_wgrad)
        return (None if dx is None else dx.permute(0, 3, 1, 2), None, None, None) + tuple(dws)


class ReducFinalBatchedFunction(torch.autograd.Function):
    """ReducFinalFunction whose backward computes the layers' weight gradients in one batched launch."""
    forward = staticmethod(ReducFinalFunction.forward)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return ReducFinalFunction.backward_impl(ctx, grad_out, True)


# ---------------------------------------------------------------------------- layout
def nchw_to_nhwc(src: torch.Tensor, dst2d: torch.Tensor, relu: bool = False):
    """src [B,C,H,W] contiguous -> dst2d [B*H*W, C] view (channel slice of an NHWC buffer)."""
    _need(src, "nchw_to_nhwc")
    stride, cview = _rows2d(dst2d, "nchw_to_nhwc")
    src = src.contiguous()
    B, Cc, H, W = src.shape
    if cview != Cc or dst2d.shape[0] != B * H * W:
        raise BtsHipError("nchw_to_nhwc: destination view shape mismatch")
    _enqueue("bts_nchw_to_nhwc_f32", src, (_ptr(src), B, Cc, H * W, _ptr(dst2d), stride, int(bool(relu))),
             trace=("nchw_to_nhwc_kernel", "layout", 0.0, 8.0 * src.numel(), None))
    return dst2d


def nhwc_to_nchw(src2d: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    stride, Cc = _rows2d(src2d, "nhwc_to_nchw")
    if src2d.shape[0] != B * H * W:
        raise BtsHipError("nhwc_to_nchw: source view shape mismatch")
    dst = torch.empty((B, Cc, H, W), dtype=torch.float32, device=src2d.device)
    _enqueue("bts_nhwc_to_nchw_f32", src2d, (_ptr(src2d), stride, B, Cc, H * W, _ptr(dst)))
    return dst


# ------------------------------------------------------------------------------ conv
def pack_conv_weight(w: torch.Tensor, perm: Optional[torch.Tensor] = None,
                     c_in_ld: Optional[int] = None) -> Tuple[torch.Tensor, int, int]:
    """[cout,cin,k,k] -> packed [cout_pad][k_pad], K flattened tap-major: k = tap*c_in_ld + c, zero padded
    (c_in_ld = channels the kernel walks per tap, a multiple of 4 >= cin; k_pad = K rounded up to 32).
    ``perm``: optional LongTensor; buffer channel j reads reference input channel perm[j]
    (lets a concat buffer keep its own channel order).  Returns (packed, cout_pad, c_in_ld)."""
    cout, cin, kh, kw = w.shape
    wf = w.float()
    if perm is not None:
        wf = wf[:, perm.to(w.device)]
    if c_in_ld is None:
        c_in_ld = round_up(cin, 4)
    assert c_in_ld % 4 == 0 and c_in_ld >= cin
    cout_pad = round_up(cout, 32)
    k_flat = kh * kw * c_in_ld
    k_pad = round_up(k_flat, 32)
    p = torch.zeros((cout_pad, kh * kw, c_in_ld), dtype=torch.float32, device=w.device)
    p[:cout, :, :cin] = wf.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    out = torch.zeros((cout_pad, k_pad), dtype=torch.float32, device=w.device)
    out[:, :k_flat] = p.reshape(cout_pad, k_flat)
    return out.contiguous(), cout_pad, c_in_ld


def pack_grouped_conv_weight(w: torch.Tensor, groups: int) -> Tuple[torch.Tensor, int, int]:
    """Grouped [c, c/groups, k, k] weight (cin == cout == c, ResNeXt's 3x3) -> [n_bundles, cb, k_pad] for
    conv_forward(n_bundles=...): consecutive groups are packed block-diagonally into bundles of cb = max(32, c/groups)
    channels, so each bundle is an ordinary dense convolution over its own cb input channels.
    Returns (packed, n_bundles, cb)."""
    c, cg, kh, kw = w.shape
    if c != cg * groups:
        raise BtsHipError("pack_grouped_conv_weight: expected cin == cout == groups * channels-per-group")
    cb = max(32, cg)
    if cb % cg or c % cb or cb % 32:
        raise BtsHipError("pack_grouped_conv_weight: unsupported group width %d" % cg)
    nb, gpb = c // cb, cb // cg                             # bundles, groups per bundle
    dense = torch.zeros((nb, cb, cb, kh, kw), dtype=torch.float32, device=w.device)
    wv = w.float().reshape(nb, gpb, cg, cg, kh, kw)         # [bundle, group-in-bundle, out-in-group, in-in-group, k, k]
    for g in range(gpb):
        dense[:, g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] = wv[:, g]
    packed = torch.stack([pack_conv_weight(dense[j], c_in_ld=cb)[0] for j in range(nb)])
    return packed.contiguous(), nb, cb


_SUBPIX_SETS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}   # (parity, tap) -> 3x3 kernel rows summed


def pack_upconv_subpixel(w: torch.Tensor, c_in_ld: Optional[int] = None) -> Tuple[torch.Tensor, int, int]:
    """upconv = nearest-2x + conv3x3 (reference bts.py:90-92) as four 2x2 convolutions on the source.

    Output pixel (2Y+py, 2X+px) only ever sees source rows {Y-1+py, Y+py} and columns {X-1+px, X+px}: the
    three kernel rows collapse onto two source rows (py=0: {k0 | k1+k2}, py=1: {k0+k1 | k2}), same for
    columns.  Returns ([4][cout_pad][k_pad] with class = 2*py+px and k = (ty*2+tx)*c_in_ld + c, cout_pad,
    c_in_ld).  Zero padding of the upsampled map coincides with source out-of-range, so borders are exact."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3
    if c_in_ld is None:
        c_in_ld = round_up(cin, 4)
    cout_pad = round_up(cout, 32)
    k_pad = round_up(4 * c_in_ld, 32)
    wf = w.float()
    out = torch.zeros((4, cout_pad, k_pad), dtype=torch.float32, device=w.device)
    for py in (0, 1):
        for px in (0, 1):
            blk = torch.zeros((cout_pad, 4, c_in_ld), dtype=torch.float32, device=w.device)
            for ty in (0, 1):
                for tx in (0, 1):
                    acc = None
                    for ky in _SUBPIX_SETS[(py, ty)]:
                        for kx in _SUBPIX_SETS[(px, tx)]:
                            acc = wf[:, :, ky, kx] if acc is None else acc + wf[:, :, ky, kx]
                    blk[:cout, ty * 2 + tx, :cin] = acc
            out[2 * py + px, :, :4 * c_in_ld] = blk.reshape(cout_pad, 4 * c_in_ld)
    return out.contiguous(), cout_pad, c_in_ld


def pack_upconv_taps(w: torch.Tensor, c_in_ld: Optional[int] = None) -> Tuple[torch.Tensor, int, int]:
    """upconv as a TAP GEMM (bts_upconv_combine_f32): the 3x3 kernel [cout, cin, 3, 3] as the weight of ONE 1x1
    convolution with 9*cout outputs, row t*cout + n = w[n, :, ky, kx] with t = 3*ky + kx.  Returns
    ([9*cout (padded to 32)][k_pad], 9*cout, c_in_ld); cout must be a multiple of 4."""
    cout, cin, kh, kw = w.shape
    assert kh == 3 and kw == 3 and cout % 4 == 0
    if c_in_ld is None:
        c_in_ld = round_up(cin, 4)
    rows = 9 * cout
    out = torch.zeros((round_up(rows, 32), round_up(c_in_ld, 32)), dtype=torch.float32, device=w.device)
    out[:rows, :cin] = w.float().permute(2, 3, 0, 1).reshape(rows, cin)
    return out.contiguous(), rows, c_in_ld


def upconv_combine(taps2d: torch.Tensor, B: int, h: int, w: int, c: int, y2d: torch.Tensor, act: int = ACT_NONE,
                   e2: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, tag: str = "decoder_upconv_sum"):
    """Second stage of the tap-GEMM upconv (bts_upconv_combine_f32): taps2d [B*h*w, >= 9*c] -> y2d [B*2h*2w, c] NHWC view."""
    ts, tc = _rows2d(taps2d, "upconv_combine")
    ys, yc = _rows2d(y2d, "upconv_combine")
    if tc < 9 * c or yc != c or c % 4 or taps2d.shape[0] != B * h * w or y2d.shape[0] != 4 * B * h * w:
        raise BtsHipError("upconv_combine: views %s / %s do not fit B=%d %dx%d c=%d"
                          % (tuple(taps2d.shape), tuple(y2d.shape), B, h, w, c))
    es, eb = _e2_vectors(e2, c, "upconv_combine")
    npx = B * h * w
    _enqueue("bts_upconv_combine_f32", taps2d, (_ptr(taps2d), ts, B, h, w, c, _ptr(es), _ptr(eb), int(act), _ptr(y2d), ys),
             trace=("upconv_combine_kernel", tag, 0.0, 4.0 * (9 * npx * c + 4 * npx * c), None))
    return y2d


# ---- upconv in shared-patch F(2x2,2x2) form (csrc/conv_up9.inc): 9 products per source pixel instead of the sub-pixel form's 16
_UP9_S = {0: ((1.0, 0.0, 0.0), (0.0, 1.0, 1.0)), 1: ((1.0, 1.0, 0.0), (0.0, 0.0, 1.0))}    # parity -> 2x3 row sums (as _SUBPIX_SETS)
_UP9_G = ((1.0, 0.0), (1.0, 1.0), (0.0, 1.0))


def _up9_fragment_order(U: torch.Tensor) -> torch.Tensor:
    """[cls, n, k, a, b] -> the flat order conv_up9_kernel loads (include/bts_hip.h, bts_upconv_up9_fwd_f32)."""
    _, cout, cin, _, _ = U.shape
    U = U.reshape(4, cout // 32, 32, cin // 32, 4, 2, 4, 3, 3)          # (cls, ct, li, chunk, g, lh, q, a, b)
    return U.permute(7, 8, 3, 1, 0, 4, 5, 2, 6).contiguous().view(-1)   # (a, b, chunk, ct, cls, g, lh, li, q)


def pack_upconv_up9(w: torch.Tensor) -> torch.Tensor:
    """upconv weight [c_out, c_in, 3, 3] (c_in, c_out multiples of 32) -> U = G g_(py,px) G^T for the four parity classes
    of pack_upconv_subpixel (g = the pre-summed 2x2 filters, G = [[1,0],[1,1],[0,1]]), fp32, in the MFMA B-fragment order
    bts_upconv_up9_fwd_f32 loads: 36 * c_in * c_out floats.  Every U element is a plain fp32 sum of at most nine of the
    3x3 weights.  Once per weight (inference weights are constant; upconv.packed caches it)."""
    cout, cin, kh, kw = w.shape
    if kh != 3 or kw != 3 or cin % 32 or cout % 32:
        raise BtsHipError("pack_upconv_up9: needs a [c_out, c_in, 3, 3] weight with c_in and c_out multiples of 32")
    wf = w.detach().float()
    U = torch.empty((4, cout, cin, 3, 3), dtype=torch.float32, device=w.device)
    for py in (0, 1):
        for px in (0, 1):
            g = {}
            for ty in (0, 1):
                for tx in (0, 1):
                    acc = None
                    for ky in _SUBPIX_SETS[(py, ty)]:
                        for kx in _SUBPIX_SETS[(px, tx)]:
                            acc = wf[:, :, ky, kx] if acc is None else acc + wf[:, :, ky, kx]
                    g[(ty, tx)] = acc
            rows = {(0, 0): g[(0, 0)], (0, 1): g[(0, 1)], (2, 0): g[(1, 0)], (2, 1): g[(1, 1)],
                    (1, 0): g[(0, 0)] + g[(1, 0)], (1, 1): g[(0, 1)] + g[(1, 1)]}                # G g
            for a in range(3):
                U[2 * py + px, :, :, a, 0] = rows[(a, 0)]
                U[2 * py + px, :, :, a, 1] = rows[(a, 0)] + rows[(a, 1)]
                U[2 * py + px, :, :, a, 2] = rows[(a, 1)]
    return _up9_fragment_order(U)


def pack_upconv_up9_reference(w: torch.Tensor) -> torch.Tensor:
    """torch fp64 statement of pack_upconv_up9, kept as its test oracle: U_(py,px)[a][b] = sum_(ky,kx) (G S_py)[a][ky]
    w[ky][kx] (G S_px)[b][kx] straight from the 3x3 weight (S_p = the 2x3 row-sum matrix of parity p), computed in fp64
    and rounded once."""
    cout, cin, kh, kw = w.shape
    if kh != 3 or kw != 3 or cin % 32 or cout % 32:
        raise BtsHipError("pack_upconv_up9: needs a [c_out, c_in, 3, 3] weight with c_in and c_out multiples of 32")
    G = torch.tensor(_UP9_G, dtype=torch.float64, device=w.device)
    R = [G @ torch.tensor(_UP9_S[p], dtype=torch.float64, device=w.device) for p in (0, 1)]      # [3, 3] per parity
    wd = w.detach().double()
    U = torch.stack([torch.einsum("ay,nkyx,bx->nkab", R[py], wd, R[px]) for py in (0, 1) for px in (0, 1)])
    return _up9_fragment_order(U.float())


def upconv_up9_reference(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The formulation itself in torch (any dtype, CPU or GPU), window by window as the kernel does it: x [B, c_in, H, W],
    w [c_out, c_in, 3, 3] -> conv3x3(nearest2x(x)) [B, c_out, 2H, 2W].  Test oracle of the identity, not a product path."""
    B, cin, H, W = x.shape
    cout = w.shape[0]
    dt, dev = x.dtype, x.device
    G = torch.tensor(_UP9_G, dtype=dt, device=dev)
    Bt = torch.tensor(((1.0, -1.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 1.0)), dtype=dt, device=dev)
    At = torch.tensor(((1.0, 1.0, 0.0), (0.0, 1.0, 1.0)), dtype=dt, device=dev)
    nwy, nwx = H // 2 + 1, W // 2 + 1
    xp = F.pad(x, (1, 2 * nwx - W, 1, 2 * nwy - H))                                  # source rows -1 .. 2 nwy - 1
    d = xp.unfold(2, 3, 2).unfold(3, 3, 2)                                           # [B, c, nwy, nwx, 3, 3]: window (wy, wx)
    V = torch.einsum("ar,bkyxrc,ec->bkyxae", Bt, d, Bt)
    out = torch.zeros((B, cout, 2 * H + 4, 2 * W + 4), dtype=dt, device=dev)         # output row o lives at o + 1
    cover = torch.zeros((2 * H + 4, 2 * W + 4), dtype=torch.int32, device=dev)
    for py in (0, 1):
        for px in (0, 1):
            Ry = G @ torch.tensor(_UP9_S[py], dtype=dt, device=dev)
            Rx = G @ torch.tensor(_UP9_S[px], dtype=dt, device=dev)
            U = torch.einsum("ay,nkyx,bx->nkab", Ry, w.to(dt), Rx)
            M = torch.einsum("bkyxae,nkae->bnyxae", V, U)
            Y = torch.einsum("ia,bnyxae,je->bnyxij", At, M, At)                      # [B, n, wy, wx, 2, 2]
            for i in (0, 1):
                for j in (0, 1):
                    # source position (2 wy - py + i, 2 wx - px + j) -> output pixel (2 sy + py, 2 sx + px), stored at + 1
                    r0, c0 = 2 * (i - py) + py + 1, 2 * (j - px) + px + 1
                    out[:, :, r0:r0 + 4 * nwy:4, c0:c0 + 4 * nwx:4] += Y[..., i, j]
                    cover[r0:r0 + 4 * nwy:4, c0:c0 + 4 * nwx:4] += 1
    if not bool((cover[1:2 * H + 1, 1:2 * W + 1] == 1).all()):
        raise BtsHipError("upconv_up9_reference: an output pixel is not covered exactly once")
    return out[:, :, 1:2 * H + 1, 1:2 * W + 1].contiguous()


Up9Plan = TilePlan            # of bts_upconv_up9_plan; all 0 = the layer stays on the sub-pixel path


def upconv_up9_plan(h: int, w: int, c_in: int, c_out: int, precision=None, fill_frames: Optional[int] = None) -> Up9Plan:
    """Should this upconv take upconv_up9_forward?  Host-only query (bts_upconv_up9_plan); ``precision`` / ``fill_frames``
    default to the launch_config in force."""
    ff, pr = _resolve_launch(precision, fill_frames, "upconv_up9_plan")
    bm, bn, wgs = C.c_int(0), C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_upconv_up9_plan(int(h), int(w), int(c_in), int(c_out), int(pr), int(ff), C.byref(bm), C.byref(bn),
                                                     C.byref(wgs)), "bts_upconv_up9_plan")
    return Up9Plan((bm.value, bn.value, wgs.value))


def upconv_up9_forward(x2d: torch.Tensor, B: int, h: int, w: int, u: torch.Tensor, c_in: int, c_out: int, y2d: torch.Tensor,
                       act: int = ACT_ELU, e2: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, tag: str = "decoder_upconv",
                       c_in_real: Optional[int] = None):
    """act(conv3x3(nearest2x(x))) [-> e2 affine] in one launch of the F(2x2,2x2) kernel (bts_upconv_up9_fwd_f32):
    x2d [B*h*w, >= c_in] NHWC view, u from pack_upconv_up9, y2d [B*2h*2w, c_out] NHWC view (a channel slice is fine).
    Runs whatever the plan query says: callers ask upconv_up9_plan first."""
    xs, xc = _rows2d(x2d, "upconv_up9_forward")
    ys, yc = _rows2d(y2d, "upconv_up9_forward")
    _need(u, "upconv_up9_forward")
    if c_in % 32 or c_out % 32 or xc < c_in or yc != c_out or x2d.shape[0] != B * h * w or y2d.shape[0] != 4 * B * h * w:
        raise BtsHipError("upconv_up9_forward: views %s / %s do not fit B=%d %dx%d, %d -> %d channels (multiples of 32)"
                          % (tuple(x2d.shape), tuple(y2d.shape), B, h, w, c_in, c_out))
    if u.numel() != 36 * c_in * c_out or not u.is_contiguous():
        raise BtsHipError("upconv_up9_forward: u must come from pack_upconv_up9 (36 * c_in * c_out floats)")
    _check_act3(act, "upconv_up9_forward")
    es, eb = _e2_vectors(e2, c_out, "upconv_up9_forward")
    kern, flops, nbytes, xflops = "conv", 0.0, 0.0, None
    if _trace is not None:
        cin = c_in_real if c_in_real is not None else c_in
        n_ty, n_tx = (h // 2 + 1 + 3) // 4, (w // 2 + 1 + 7) // 8
        kern = "conv_up9_kernel<32>"
        flops = 2.0 * 36 * B * h * w * c_out * cin                                  # the reference's 3x3 on the upsampled map
        nbytes = 4.0 * (B * h * w * cin + 4 * B * h * w * c_out + 9 * c_out * cin)
        xflops = 2.0 * 9 * (B * n_ty * n_tx * 32) * (4 * c_out) * c_in              # what the kernel issues, ragged tiles included
    tops = torch_ops()
    run = None
    if tops is not None:
        run = lambda: _op(lambda: tops.upconv_up9(x2d, u, es, eb, y2d, [B, h, w, c_in, c_out, int(act)]))
    _enqueue("bts_upconv_up9_fwd_f32", x2d, (_ptr(x2d), xs, B, h, w, c_in, _ptr(u), c_out, _ptr(es), _ptr(eb), int(act), _ptr(y2d), ys),
             trace=(kern, tag, flops, nbytes, xflops), run=run)
    return y2d


# ---- planar-tail 3x3 (decoder conv3 / conv2) with bf16 main operands and an fp32 tail (csrc/conv_tail_bf16.inc)
def pack_conv_tail_bf16(weight_oihw: torch.Tensor, n_tail: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """[c_out, c_main + n_tail, 3, 3] -> (w_main, w_tail) as bts_conv_tail_bf16_fwd_f32 reads them.  w_main: bfloat16
    [c_out_pad, 9 * c_main], k = tap * c_main + c, the main-channel weights rounded to the nearest bf16 (ties to even:
    ``Tensor.to(torch.bfloat16)``).  w_tail: float32 [c_out_pad, 9, 4], slot j = tail plane j, the tail weights bit for bit.
    Rows past c_out and unused slots are zero."""
    if weight_oihw.dim() != 4 or tuple(weight_oihw.shape[2:]) != (3, 3) or not 1 <= n_tail <= 4 or weight_oihw.shape[1] <= n_tail:
        raise BtsHipError("pack_conv_tail_bf16: needs a [c_out, c_main + n_tail, 3, 3] weight and 1..4 tail planes")
    cout, cin = weight_oihw.shape[:2]
    c_main = cin - n_tail
    if c_main % 32:
        raise BtsHipError("pack_conv_tail_bf16: %d main channels; the bf16 halo tile needs a multiple of 32" % c_main)
    wf = weight_oihw.detach().float()
    cout_pad = round_up(cout, 32)
    w_main = torch.zeros((cout_pad, 9 * c_main), dtype=torch.bfloat16, device=wf.device)
    w_main[:cout] = wf[:, :c_main].permute(0, 2, 3, 1).reshape(cout, 9 * c_main).to(torch.bfloat16)
    w_tail = torch.zeros((cout_pad, 9, 4), dtype=torch.float32, device=wf.device)
    w_tail[:cout, :, :n_tail] = wf[:, c_main:].permute(0, 2, 3, 1).reshape(cout, 9, n_tail)
    return w_main.contiguous(), w_tail.contiguous()


class TailBf16Plan(tuple):
    """(bn, workgroups of the declared launch) of bts_conv_tail_bf16_plan; all 0 = the layer stays on the fp32 tail kernel."""
    bn = property(lambda self: self[0])
    workgroups = property(lambda self: self[1])
    eligible = property(lambda self: self[0] > 0)


def conv_tail_bf16_plan(h: int, w: int, c_main: int, c_out: int, n_tail: int = 1, fill_frames: Optional[int] = None) -> TailBf16Plan:
    """Should this planar-tail layer take conv_tail_bf16_forward?  Host-only query (bts_conv_tail_bf16_plan);
    ``fill_frames`` defaults to the launch_config in force."""
    ff, _ = _resolve_launch(None, fill_frames, "conv_tail_bf16_plan")
    bn, wgs = C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_conv_tail_bf16_plan(int(h), int(w), int(c_main), int(c_out), int(n_tail), int(ff), C.byref(bn),
                                                         C.byref(wgs)), "bts_conv_tail_bf16_plan")
    return TailBf16Plan((bn.value, wgs.value))


def conv_tail_bf16_forward(x2d: torch.Tensor, B: int, h: int, w: int, w_main: torch.Tensor, w_tail: torch.Tensor,
                           tail_plane: torch.Tensor, c_main: int, c_out: int, y2d: torch.Tensor, act: int = ACT_ELU,
                           e2: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, tag: str = "decoder_conv",
                           c_in_real: Optional[int] = None):
    """act(conv3x3([x | plane])) [-> e2 affine] in one launch of the bf16 halo tile with an fp32 tail
    (bts_conv_tail_bf16_fwd_f32): x2d [B*h*w, >= c_main] NHWC view, (w_main, w_tail) from pack_conv_tail_bf16, tail_plane
    one contiguous [B,h,w] (or [B,1,h,w]) map, y2d [B*h*w, c_out] NHWC view (a channel slice is fine).  Runs whatever the
    plan query says: callers ask conv_tail_bf16_plan first."""
    name = "conv_tail_bf16_forward"
    xs, xc = _rows2d(x2d, name)
    ys, yc = _rows2d(y2d, name)
    _need(w_tail, name)
    if not isinstance(w_main, torch.Tensor) or not w_main.is_cuda or w_main.dtype != torch.bfloat16:
        raise BtsHipError("conv_tail_bf16_forward: w_main must be a bfloat16 CUDA/ROCm tensor (pack_conv_tail_bf16)")
    if c_main % 32 or xc < c_main or yc != c_out or x2d.shape[0] != B * h * w or y2d.shape[0] != B * h * w:
        raise BtsHipError("conv_tail_bf16_forward: views %s / %s do not fit B=%d %dx%d, %d (a multiple of 32) -> %d channels"
                          % (tuple(x2d.shape), tuple(y2d.shape), B, h, w, c_main, c_out))
    if w_main.dim() != 2 or w_main.shape[1] != 9 * c_main or w_main.shape[0] < c_out or w_main.shape[0] % 32 or not w_main.is_contiguous():
        raise BtsHipError("conv_tail_bf16_forward: w_main must be contiguous [c_out_pad, 9 * c_main] (pack_conv_tail_bf16)")
    cout_pad = w_main.shape[0]
    if w_tail.numel() != 36 * cout_pad or not w_tail.is_contiguous():
        raise BtsHipError("conv_tail_bf16_forward: w_tail must be contiguous [c_out_pad, 9, 4] (pack_conv_tail_bf16)")
    _dense_planes([tail_plane], B * h * w, name, at_most=1)
    _check_act3(act, name)
    es, eb = _e2_vectors(e2, c_out, name)
    kern, flops, nbytes, xflops = "conv", 0.0, 0.0, None
    if _trace is not None:
        cin = c_in_real if c_in_real is not None else c_main + 1
        bn = 128 if c_out >= 128 else 64
        kern = conv_plan.tail_bf16_kernel_name(bn)
        flops = 2.0 * 9 * B * h * w * c_out * cin
        nbytes = 4.0 * (B * h * w * (cin + c_out)) + 2.0 * 9 * c_out * c_main + 4.0 * 9 * c_out
        tiles = B * ((h + 3) // 4) * ((w + 31) // 32)
        xflops = 2.0 * 9 * (tiles * 128) * (round_up(c_out, bn)) * (c_main + 1)     # ragged tiles included
    tops = torch_ops()
    run = None
    if tops is not None:
        run = lambda: _op(lambda: tops.conv_tail_bf16(x2d, w_main, w_tail, tail_plane, es, eb, y2d, [B, h, w, c_main, c_out, int(act)]))
    _enqueue("bts_conv_tail_bf16_fwd_f32", x2d,
             (_ptr(x2d), xs, B, h, w, c_main, _ptr(w_main), _ptr(w_tail), _ptr(tail_plane), 1, c_out, cout_pad, _ptr(es), _ptr(eb),
              int(act), _ptr(y2d), ys), trace=(kern, tag, flops, nbytes, xflops), run=run)
    return y2d


# ---- wide 1x1 with bf16 operands, c_out % 192 == 0 (DenseNet161's bottlenecks under conv_precision "bf16"; csrc/conv_1x1_bf16.inc)
def conv1x1_bf16_plan(h: int, w: int, c_in: int, c_out: int, fill_frames: Optional[int] = None) -> TilePlan:
    """Should this 1x1 layer take conv1x1_bf16_forward?  Host-only query (bts_conv1x1_bf16_plan) on the per-frame geometry;
    ``fill_frames`` defaults to the launch_config in force."""
    ff, _ = _resolve_launch(None, fill_frames, "conv1x1_bf16_plan")
    bm, bn, wgs = C.c_int(0), C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_conv1x1_bf16_plan(int(h), int(w), int(c_in), int(c_out), int(ff), C.byref(bm), C.byref(bn),
                                                       C.byref(wgs)), "bts_conv1x1_bf16_plan")
    return TilePlan((bm.value, bn.value, wgs.value))


def conv1x1_bf16_forward(x2d: torch.Tensor, npix: int, c_in: int, w_plane: torch.Tensor, c_out: int, y2d: torch.Tensor,
                         pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pre_relu: bool = False,
                         e1: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, act: int = ACT_NONE, tag: str = "conv1x1_bf16"):
    """act(e1(conv1x1(bf16(pre(x))))) in one launch of the wide bf16 tile (bts_conv1x1_bf16_fwd_f32): x2d [npix, >= c_in] NHWC
    view (c_in channels read), w_plane the one-plane bf16 form of the layer's packed weight (``round_bf16(w_packed)``:
    int16 [1, c_out_pad, k_pad], or the same bits as [c_out_pad, k_pad] / bfloat16), pre / e1 (scale, shift) pairs of >= c_in /
    >= c_out floats, y2d [npix, c_out] NHWC view (a channel slice is fine).  Runs whatever the plan query says: callers ask
    conv1x1_bf16_plan first.

    A ``torch.bfloat16`` y2d is a bf16-resident destination (bts_conv1x1_bf16_fwd_bf16): the same value, rounded once more to
    the nearest bf16 (ties to even) and stored in two bytes -- for a consumer that reads bf16 (conv3x3_bf16in_forward)."""
    name = "conv1x1_bf16_forward"
    xs, xc = _rows2d(x2d, name)
    y_bf16 = isinstance(y2d, torch.Tensor) and y2d.dtype == torch.bfloat16
    ys, yc = _rows2d_bf16(y2d, name) if y_bf16 else _rows2d(y2d, name)
    if not isinstance(w_plane, torch.Tensor) or not w_plane.is_cuda or w_plane.dtype not in (torch.int16, torch.bfloat16):
        raise BtsHipError("conv1x1_bf16_forward: w_plane must be an int16 / bfloat16 CUDA/ROCm tensor (round_bf16 of the packed weight)")
    if c_in <= 0 or c_in % 16 or c_out <= 0 or c_out % 192:
        raise BtsHipError("conv1x1_bf16_forward: %d -> %d channels; needs c_in %% 16 == 0 and c_out %% 192 == 0" % (c_in, c_out))
    if npix <= 0 or xc < c_in or yc != c_out or x2d.shape[0] != npix or y2d.shape[0] != npix:
        raise BtsHipError("conv1x1_bf16_forward: views %s / %s do not fit %d pixels, %d -> %d channels"
                          % (tuple(x2d.shape), tuple(y2d.shape), npix, c_in, c_out))
    if xs % 4 or ys % 4 or x2d.data_ptr() % 16 or y2d.data_ptr() % (8 if y_bf16 else 16):
        raise BtsHipError("conv1x1_bf16_forward: rows must be 16-byte aligned (pixel strides %d / %d, multiples of 4 floats)" % (xs, ys))
    if (w_plane.dim() not in (2, 3) or (w_plane.dim() == 3 and w_plane.shape[0] != 1) or not w_plane.is_contiguous()
            or w_plane.shape[-2] < c_out or w_plane.shape[-1] < c_in or w_plane.shape[-1] % 32):
        raise BtsHipError("conv1x1_bf16_forward: w_plane %s must be contiguous [1, c_out_pad >= %d, k_pad >= %d (a multiple of 32)]"
                          % (tuple(w_plane.shape), c_out, c_in))
    cout_pad, k_pad = int(w_plane.shape[-2]), int(w_plane.shape[-1])
    _check_act3(act, name)
    ps, pb = _e2_vectors(pre, c_in, name, "pre")
    es, eb = _e2_vectors(e1, c_out, name, "e1")
    kern, flops, nbytes, xflops = "conv", 0.0, 0.0, None
    if _trace is not None:
        kern = conv_plan.wide_1x1_bf16_kernel_name(192, y_bf16)
        flops = 2.0 * npix * c_out * c_in
        nbytes = 4.0 * npix * c_in + (2.0 if y_bf16 else 4.0) * npix * c_out + 2.0 * c_out * c_in
        xflops = 2.0 * (round_up(npix, 128)) * c_out * c_in                    # ragged last tile included
    tops = torch_ops()
    run = None
    if tops is not None:
        top = tops.conv1x1_bf16_ybf16 if y_bf16 else tops.conv1x1_bf16
        run = lambda: _op(lambda: top(x2d, w_plane, ps, pb, es, eb, y2d, [npix, c_in, c_out, int(bool(pre_relu)), int(act)]))
    _enqueue("bts_conv1x1_bf16_fwd_bf16" if y_bf16 else "bts_conv1x1_bf16_fwd_f32", x2d,
             (_ptr(x2d), xs, npix, c_in, _ptr(w_plane), k_pad, c_out, cout_pad, _ptr(ps), _ptr(pb), int(bool(pre_relu)), _ptr(es), _ptr(eb),
              int(act), _ptr(y2d), ys), trace=(kern, tag, flops, nbytes, xflops), run=run)
    return y2d


# ---- 3x3 convolution reading a bf16-resident NHWC tensor on the bf16 halo tile (csrc/conv_3x3_bf16in.inc): the growth
#      convolution of a dense layer whose bottleneck intermediate conv1x1_bf16_forward stored as bf16
def conv3x3_bf16in_plan(h: int, w: int, c_in: int, c_out: int, fill_frames: Optional[int] = None) -> TailBf16Plan:
    """Should this 3x3 layer (stride 1, padding 1, no prologue) read its input from a bf16 tensor with conv3x3_bf16in_forward?
    Host-only query (bts_conv3x3_bf16in_plan): the layers conv_forward runs on the bf16 halo tile under precision "bf16",
    less the classes measured to lose; (bn, workgroups of the declared launch), all 0 = stay on conv_forward.  ``fill_frames``
    defaults to the launch_config in force."""
    ff, _ = _resolve_launch(None, fill_frames, "conv3x3_bf16in_plan")
    bn, wgs = C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_conv3x3_bf16in_plan(int(h), int(w), int(c_in), int(c_out), int(ff), C.byref(bn), C.byref(wgs)),
               "bts_conv3x3_bf16in_plan")
    return TailBf16Plan((bn.value, wgs.value))


def conv3x3_bf16in_forward(x2d: torch.Tensor, B: int, h: int, w: int, c_in: int, w_plane: torch.Tensor, c_out: int, y2d: torch.Tensor,
                           e1: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, act: int = ACT_NONE, tag: str = "conv3x3_bf16in"):
    """act(e1(conv3x3(x))) in one launch of the bf16 halo tile fed from a BFLOAT16 tensor (bts_conv3x3_bf16in_fwd_f32): x2d
    [B*h*w, >= c_in] view of a bf16 NHWC buffer (c_in % 32 == 0 channels read), w_plane the one-plane bf16 form of the layer's
    packed 3x3 weight (``round_bf16(w_packed)``: int16 [1, c_out_pad, k_pad], or the same bits as [c_out_pad, k_pad] /
    bfloat16), e1 a (scale, shift) pair of >= c_out_pad floats, y2d [B*h*w, c_out] fp32 NHWC view (a channel slice is fine).
    Bit for bit conv_forward under precision "bf16" on ``x2d.float()`` where that takes the bf16 halo tile.  Runs whatever
    the plan query says: callers ask conv3x3_bf16in_plan first."""
    name = "conv3x3_bf16in_forward"
    xs, xc = _rows2d_bf16(x2d, name)
    ys, yc = _rows2d(y2d, name)
    if not isinstance(w_plane, torch.Tensor) or not w_plane.is_cuda or w_plane.dtype not in (torch.int16, torch.bfloat16):
        raise BtsHipError("conv3x3_bf16in_forward: w_plane must be an int16 / bfloat16 CUDA/ROCm tensor (round_bf16 of the packed weight)")
    if B <= 0 or h <= 0 or w <= 0 or c_in <= 0 or c_in % 32 or c_out <= 0:
        raise BtsHipError("conv3x3_bf16in_forward: B=%d %dx%d, %d -> %d channels; needs c_in %% 32 == 0" % (B, h, w, c_in, c_out))
    if xc < c_in or yc != c_out or x2d.shape[0] != B * h * w or y2d.shape[0] != B * h * w:
        raise BtsHipError("conv3x3_bf16in_forward: views %s / %s do not fit B=%d %dx%d, %d -> %d channels"
                          % (tuple(x2d.shape), tuple(y2d.shape), B, h, w, c_in, c_out))
    if (w_plane.dim() not in (2, 3) or (w_plane.dim() == 3 and w_plane.shape[0] != 1) or not w_plane.is_contiguous()
            or w_plane.shape[-2] < c_out or w_plane.shape[-2] % 32 or w_plane.shape[-1] < 9 * c_in or w_plane.shape[-1] % 8):
        raise BtsHipError("conv3x3_bf16in_forward: w_plane %s must be contiguous [1, c_out_pad >= %d (a multiple of 32), k_pad >= %d]"
                          % (tuple(w_plane.shape), c_out, 9 * c_in))
    cout_pad, k_pad = int(w_plane.shape[-2]), int(w_plane.shape[-1])
    _check_act3(act, name)
    es, eb = _e2_vectors(e1, cout_pad, name, "e1")
    kern, flops, nbytes, xflops = "conv", 0.0, 0.0, None
    if _trace is not None:
        bn = conv_plan.bf16in_3x3_tile(c_out)
        kern = conv_plan.bf16in_3x3_kernel_name(bn)
        flops = 2.0 * 9 * B * h * w * c_out * c_in
        nbytes = 2.0 * B * h * w * c_in + 4.0 * B * h * w * c_out + 2.0 * 9 * c_out * c_in
        tiles = B * ((h + 3) // 4) * ((w + 31) // 32)
        xflops = 2.0 * 9 * (tiles * 128) * round_up(c_out, bn) * c_in             # ragged tiles included
    tops = torch_ops()
    run = None
    if tops is not None:
        run = lambda: _op(lambda: tops.conv3x3_bf16in(x2d, w_plane, es, eb, y2d, [B, h, w, c_in, c_out, int(act)]))
    _enqueue("bts_conv3x3_bf16in_fwd_f32", x2d,
             (_ptr(x2d), xs, B, h, w, c_in, _ptr(w_plane), k_pad, c_out, cout_pad, _ptr(es), _ptr(eb), int(act), _ptr(y2d), ys),
             trace=(kern, tag, flops, nbytes, xflops), run=run)
    return y2d


# ---- the same tile at 128 / 192 / 256 channels per workgroup with the bottleneck epilogue (res, y2): ResNe(X)t's 1x1 layers and
#      DenseNet121's bottlenecks under BtsModel.bf16_wide_1x1 = "all"
def conv1x1_bf16_wide_plan(h: int, w: int, c_in: int, c_out: int, has_res: bool = False, fill_frames: Optional[int] = None) -> TilePlan:
    """Should this 1x1 layer take conv1x1_bf16_wide_forward?  Host-only query (bts_conv1x1_bf16_wide_plan) on the per-frame
    geometry; ``has_res``: the layer adds an identity; ``fill_frames`` defaults to the launch_config in force."""
    ff, _ = _resolve_launch(None, fill_frames, "conv1x1_bf16_wide_plan")
    bm, bn, wgs = C.c_int(0), C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_conv1x1_bf16_wide_plan(int(h), int(w), int(c_in), int(c_out), int(bool(has_res)), int(ff),
                                                            C.byref(bm), C.byref(bn), C.byref(wgs)), "bts_conv1x1_bf16_wide_plan")
    return TilePlan((bm.value, bn.value, wgs.value))


def conv1x1_bf16_wide_forward(x2d: torch.Tensor, npix: int, c_in: int, w_plane: torch.Tensor, c_out: int, y2d: torch.Tensor,
                              pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pre_relu: bool = False,
                              e1: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, res2d: Optional[torch.Tensor] = None,
                              y2_2d: Optional[torch.Tensor] = None, act: int = ACT_NONE, bn: int = 0, tag: str = "conv1x1_bf16_wide"):
    """act(e1(conv1x1(bf16(pre(x)))) + res) in one launch of the wide bf16 tile (bts_conv1x1_bf16_wide_fwd_f32), also written to
    y2: the operands of conv1x1_bf16_forward, plus res2d / y2_2d [npix, c_out] NHWC views (channel slices are fine) and
    ``bn`` = 128 / 192 / 256 to force a tile (0: the library's choice for c_out).  c_out a multiple of 128 or of 192.  Runs
    whatever the plan query says: callers ask conv1x1_bf16_wide_plan first."""
    name = "conv1x1_bf16_wide_forward"
    xs, xc = _rows2d(x2d, name)
    ys, yc = _rows2d(y2d, name)
    if not isinstance(w_plane, torch.Tensor) or not w_plane.is_cuda or w_plane.dtype not in (torch.int16, torch.bfloat16):
        raise BtsHipError("%s: w_plane must be an int16 / bfloat16 CUDA/ROCm tensor (round_bf16 of the packed weight)" % name)
    if c_in <= 0 or c_in % 16 or c_out <= 0 or (c_out % 128 and c_out % 192):
        raise BtsHipError("%s: %d -> %d channels; needs c_in %% 16 == 0 and c_out a multiple of 128 or 192" % (name, c_in, c_out))
    if bn not in (0, 128, 192, 256) or (bn and c_out % bn):
        raise BtsHipError("%s: bn must be 0 or one of 128 / 192 / 256 that divides c_out = %d, got %r" % (name, c_out, bn))
    if npix <= 0 or xc < c_in or yc != c_out or x2d.shape[0] != npix or y2d.shape[0] != npix:
        raise BtsHipError("%s: views %s / %s do not fit %d pixels, %d -> %d channels"
                          % (name, tuple(x2d.shape), tuple(y2d.shape), npix, c_in, c_out))
    if xs % 4 or ys % 4 or x2d.data_ptr() % 16 or y2d.data_ptr() % 16:
        raise BtsHipError("%s: rows must be 16-byte aligned (pixel strides %d / %d, multiples of 4 floats)" % (name, xs, ys))
    strides = []
    for t, what in ((res2d, "res2d"), (y2_2d, "y2_2d")):
        if t is None:
            strides.append(0)
            continue
        ts, tc = _rows2d(t, name)
        if tc != c_out or t.shape[0] != npix or ts % 4 or t.device != x2d.device:
            raise BtsHipError("%s: %s %s must be a [%d, %d] view on x2d's device with a pixel stride that is a multiple of 4 floats"
                              % (name, what, tuple(t.shape), npix, c_out))
        strides.append(ts)
    if (w_plane.dim() not in (2, 3) or (w_plane.dim() == 3 and w_plane.shape[0] != 1) or not w_plane.is_contiguous()
            or w_plane.shape[-2] < c_out or w_plane.shape[-1] < c_in or w_plane.shape[-1] % 32):
        raise BtsHipError("%s: w_plane %s must be contiguous [1, c_out_pad >= %d, k_pad >= %d (a multiple of 32)]"
                          % (name, tuple(w_plane.shape), c_out, c_in))
    cout_pad, k_pad = int(w_plane.shape[-2]), int(w_plane.shape[-1])
    _check_act3(act, name)
    ps, pb = _e2_vectors(pre, c_in, name, "pre")
    es, eb = _e2_vectors(e1, c_out, name, "e1")
    kern, flops, nbytes, xflops = "conv", 0.0, 0.0, None
    if _trace is not None:
        kern = conv_plan.wide_1x1_bf16_kernel_name(bn or conv_plan.wide_1x1_bf16_tile(c_out))
        flops = 2.0 * npix * c_out * c_in
        nbytes = 4.0 * npix * (c_in + c_out * (1 + (res2d is not None) + (y2_2d is not None))) + 2.0 * c_out * c_in
        xflops = 2.0 * (round_up(npix, 128)) * c_out * c_in                    # ragged last tile included
    tops = torch_ops()
    run = None
    if tops is not None:
        run = lambda: _op(lambda: tops.conv1x1_bf16_wide(x2d, w_plane, ps, pb, es, eb, res2d, y2d, y2_2d,
                                                         [npix, c_in, c_out, int(bool(pre_relu)), int(act), int(bn)]))
    _enqueue("bts_conv1x1_bf16_wide_fwd_f32", x2d,
             (_ptr(x2d), xs, npix, c_in, _ptr(w_plane), k_pad, c_out, cout_pad, _ptr(ps), _ptr(pb), int(bool(pre_relu)), _ptr(es), _ptr(eb),
              _ptr(res2d), strides[0], int(act), _ptr(y2d), ys, _ptr(y2_2d), strides[1], int(bn)), trace=(kern, tag, flops, nbytes, xflops),
             run=run)
    return y2d


# ---- conv1 (32 features + planar tail -> 32 channels, NCHW) as a fused Winograd F(2x2,3x3) kernel (csrc/conv_wino_tail.inc)
_WINO_G =((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))
_WINO_BT = ((1.0, 0.0, -1.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, -1.0, 1.0, 0.0), (0.0, 1.0, 0.0, -1.0))
_WINO_AT = ((1.0, 1.0, 1.0, 0.0), (0.0, 1.0, -1.0, -1.0))


def _conv_tail_wino_split(weight_oihw: torch.Tensor, n_tail: int):
    if (weight_oihw.dim() != 4 or tuple(weight_oihw.shape[2:]) != (3, 3) or not 0 <= n_tail <= 4 or weight_oihw.shape[0] != 32
            or weight_oihw.shape[1] != 32 + n_tail):
        raise BtsHipError("pack_conv_tail_wino: needs a [32, 32 + n_tail, 3, 3] weight and 0..4 tail planes")
    wf = weight_oihw.detach()
    return wf[:, :32], wf[:, 32:]


def _conv_tail_wino_order(U: torch.Tensor, wt: torch.Tensor, n_tail: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """U [n, c, 4, 4] fp32, wt [n, n_tail, 3, 3] -> the two flat fragment orders of include/bts_hip.h."""
    u = U.reshape(2, 16, 2, 4, 4, 16)                                   # (cb, lw, half, lg, q, xi)
    u = u.permute(5, 0, 2, 3, 1, 4).contiguous().view(-1)               # (xi, cb, half, lg, lw, q): lane = 16 lg + lw
    t = torch.zeros((32, 9, 4), dtype=torch.float32, device=U.device)   # [n, tap, j]
    t[:, :, :n_tail] = wt.float().permute(0, 2, 3, 1).reshape(32, 9, n_tail)
    t = t.reshape(2, 16, 9, 4).permute(0, 2, 3, 1).contiguous().view(-1)       # (cb, tap, lg = j, lw)
    return u, t


def pack_conv_tail_wino(weight_oihw: torch.Tensor, n_tail: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """[32, 32 + n_tail, 3, 3] -> (u, w_tail) as bts_conv_tail_wino_fwd_f32 reads them (include/bts_hip.h): u = the 32
    main channels in Winograd F(2x2,3x3) form, U = G g G^T computed in fp64 and rounded once, in MFMA A-fragment order
    (16 * 32 * 32 floats); w_tail = the tail weights bit for bit in their fragment order (2 * 9 * 64 floats, unused
    slots zero).  Once per weight (inference weights are constant; bts.packed_conv1_wino caches it)."""
    g, wt = _conv_tail_wino_split(weight_oihw, n_tail)
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=g.device)
    U = (G @ g.double() @ G.t()).float()                                # [n, c, 4, 4], one rounding
    return _conv_tail_wino_order(U, wt, n_tail)


def pack_conv_tail_wino_reference(weight_oihw: torch.Tensor, n_tail: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Element-by-element fp64 statement of pack_conv_tail_wino, kept as its test oracle: U[n][c][a][b] =
    sum_{i,j} G[a][i] g[n][c][i][j] G[b][j], written into the documented float indices one by one."""
    g, wt = _conv_tail_wino_split(weight_oihw, n_tail)
    G = torch.tensor(_WINO_G, dtype=torch.float64)
    U = torch.einsum("ai,ncij,bj->ncab", G, g.double().cpu(), G).float()
    u = torch.zeros(16 * 32 * 32, dtype=torch.float32)
    t = torch.zeros(2 * 9 * 64, dtype=torch.float32)
    idx = torch.arange(16 * 32 * 32)
    q, lane, half, cb, xi = idx % 4, (idx // 4) % 64, (idx // 256) % 2, (idx // 512) % 2, idx // 1024
    u[idx] = U[16 * cb + (lane % 16), 16 * half + 4 * (lane // 16) + q, xi // 4, xi % 4]
    wtc = wt.float().cpu()
    for cb_ in range(2):
        for tap in range(9):
            for ln in range(64):
                if ln // 16 < n_tail:
                    t[(cb_ * 9 + tap) * 64 + ln] = wtc[16 * cb_ + ln % 16, ln // 16, tap // 3, tap % 3]
    return u.to(weight_oihw.device), t.to(weight_oihw.device)


def conv_tail_wino_reference(x: torch.Tensor, planes: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The formulation itself in torch (any dtype, CPU or GPU), window by window as the kernel does it: x [B, c, H, W],
    planes [B, n_tail, H, W], w [n, c + n_tail, 3, 3] -> conv3x3([x | planes]) [B, n, H, W] with the c main channels in
    F(2x2,3x3) form and the tail in direct form.  Test oracle of the identity, not a product path."""
    B, c, H, W = x.shape
    n = w.shape[0]
    dt, dev = x.dtype, x.device
    G, Bt, At = (torch.tensor(m, dtype=dt, device=dev) for m in (_WINO_G, _WINO_BT, _WINO_AT))
    nwy, nwx = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x, (1, 2 * nwx + 1 - W, 1, 2 * nwy + 1 - H))                          # rows -1 .. 2 nwy
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                           # [B, c, nwy, nwx, 4, 4]
    V = torch.einsum("ar,bkyxrc,ec->bkyxae", Bt, d, Bt)
    U = torch.einsum("ai,nkij,bj->nkab", G, w[:, :c].to(dt), G)
    M = torch.einsum("bkyxae,nkae->bnyxae", V, U)
    Y = torch.einsum("ia,bnyxae,je->bnyixj", At, M, At)                              # [B, n, wy, 2, wx, 2]
    out = Y.reshape(B, n, 2 * nwy, 2 * nwx)[:, :, :H, :W].clone()
    if planes is not None and planes.shape[1] > 0:
        out += F.conv2d(planes.to(dt), w[:, c:].to(dt), padding=1)
    return out.contiguous()


TailWinoPlan = TilePlan       # of bts_conv_tail_wino_plan; all 0 = the layer stays on bts_conv_fwd_f32


def conv_tail_wino_plan(h: int, w: int, c_main: int, c_out: int, n_tail: int = 4, precision=None,
                        fill_frames: Optional[int] = None) -> TailWinoPlan:
    """Should this planar-tail layer take conv_tail_wino_forward?  Host-only query (bts_conv_tail_wino_plan);
    ``precision`` / ``fill_frames`` default to the launch_config in force."""
    ff, pr = _resolve_launch(precision, fill_frames, "conv_tail_wino_plan")
    bm, bn, wgs = C.c_int(0), C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_conv_tail_wino_plan(int(h), int(w), int(c_main), int(c_out), int(n_tail), int(pr), int(ff),
                                                         C.byref(bm), C.byref(bn), C.byref(wgs)), "bts_conv_tail_wino_plan")
    return TailWinoPlan((bm.value, bn.value, wgs.value))


def conv_tail_wino_forward(x2d: torch.Tensor, B: int, h: int, w: int, u: torch.Tensor, w_tail: torch.Tensor,
                           tail_planes: Optional[Sequence[torch.Tensor]], y_nchw: torch.Tensor, act: int = ACT_ELU,
                           tag: str = "decoder_conv"):
    """act(conv3x3([x | planes])) in one launch of the fused Winograd kernel (bts_conv_tail_wino_fwd_f32): x2d
    [B*h*w, >= 32] NHWC view (32 channels read), (u, w_tail) from pack_conv_tail_wino, tail_planes 0..4 contiguous
    [B,h,w] (or [B,1,h,w]) maps, y_nchw contiguous [B,32,h,w].  Runs whatever the plan query says: callers ask
    conv_tail_wino_plan first."""
    name = "conv_tail_wino_forward"
    xs, xc = _rows2d(x2d, name)
    _need(u, name)
    _need(w_tail, name)
    _need(y_nchw, name)
    if xc < 32 or x2d.shape[0] != B * h * w or tuple(y_nchw.shape) != (B, 32, h, w) or not y_nchw.is_contiguous():
        raise BtsHipError("conv_tail_wino_forward: views %s / %s do not fit B=%d %dx%d, 32 -> 32 channels (NCHW result)"
                          % (tuple(x2d.shape), tuple(y_nchw.shape), B, h, w))
    if u.numel() != 16 * 32 * 32 or not u.is_contiguous() or w_tail.numel() != 2 * 9 * 64 or not w_tail.is_contiguous():
        raise BtsHipError("conv_tail_wino_forward: (u, w_tail) must come from pack_conv_tail_wino")
    planes = _dense_planes(tail_planes, B * h * w, name)
    _check_act3(act, name)
    kern, flops, nbytes, xflops = "conv", 0.0, 0.0, None
    if _trace is not None:
        kern = conv_plan.tail_wino_kernel_name()
        flops = 2.0 * 9 * B * h * w * 32 * (32 + len(planes))                       # the reference's direct 3x3
        nbytes = 4.0 * (B * h * w * (32 + len(planes) + 32) + 9 * 32 * (32 + len(planes)))
        windows = B * ((h + 3) // 4) * ((w + 31) // 32) * 32                        # ragged tiles included
        xflops = 2.0 * windows * 32 * (16 * 32 + 36 * 4)                            # 16 products per window (main) + the direct tail's k-step of 4
    ptrs = [_ptr(planes[j]) if j < len(planes) else C.c_void_p(0) for j in range(4)]
    _enqueue("bts_conv_tail_wino_fwd_f32", x2d,
             (_ptr(x2d), xs, B, h, w, 32, _ptr(u), _ptr(w_tail), ptrs[0], ptrs[1], ptrs[2], ptrs[3], len(planes), 32, int(act), _ptr(y_nchw)),
             trace=(kern, tag, flops, nbytes, xflops))
    return y_nchw


# ---- ResNeXt's grouped 3x3 on the multi-block fp32 MFMA (csrc/conv_grouped.inc), opt-in beside the bundle path
def _grouped_native_shape(w: torch.Tensor, groups: int) -> Tuple[int, int]:
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or groups <= 0 or w.shape[0] != w.shape[1] * groups:
        raise BtsHipError("pack_grouped_native: needs a [c, c / groups, 3, 3] weight (cin == cout == c)")
    c, cg = int(w.shape[0]), int(w.shape[1])
    if c % 64 or cg not in (4, 8, 16):
        raise BtsHipError("pack_grouped_native: c = %d in groups of %d; needs c %% 64 == 0 and 4, 8 or 16 channels per group" % (c, cg))
    return c, cg


def pack_grouped_native(w: torch.Tensor, groups: int) -> torch.Tensor:
    """Grouped [c, c/groups, 3, 3] weight -> the 144 * c floats bts_conv_grouped_fwd_f32 reads (include/bts_hip.h): index
    ((s*9 + tap)*16 + k)*64 + lane = the weight from input channel 64 s + 16 (lane >> 4) + k to output channel 64 s + lane,
    bit for bit, exact zeros where the two lie in different groups.  Once per weight (ResNetHip.packed caches it)."""
    c, cg = _grouped_native_shape(w, groups)
    wv = w.detach().float().reshape(c // 64, 4, 16, cg, 9)                  # [slab, block, row, k in group, tap]
    k = torch.arange(16, device=w.device)
    full = wv[:, :, :, k % cg, :]                                           # [slab, block, row, k in block, tap]
    same = (k[:, None] // cg) == (k[None, :] // cg)                         # [row, k]: one group
    full = torch.where(same[None, None, :, :, None], full, torch.zeros((), dtype=torch.float32, device=w.device))
    return full.permute(0, 4, 3, 1, 2).contiguous().view(-1)                # (slab, tap, k, block, row): lane = 16 block + row


def pack_grouped_native_reference(w: torch.Tensor, groups: int) -> torch.Tensor:
    """Index-by-index statement of pack_grouped_native, kept as its test oracle: every flat index decoded as the header
    writes it."""
    c, cg = _grouped_native_shape(w, groups)
    wc = w.detach().float().cpu()
    idx = torch.arange(144 * c)
    lane, k, tap, s = idx % 64, (idx // 64) % 16, (idx // 1024) % 9, idx // 9216
    n, ci = 64 * s + lane, 64 * s + 16 * (lane // 16) + k                   # output channel, input channel
    val = wc[n, ci % cg, tap // 3, tap % 3]
    return torch.where(ci // cg == n // cg, val, torch.zeros(())).to(w.device)


GroupedPlan = TilePlan        # of bts_conv_grouped_plan; all 0 = the layer stays on channel bundles


def conv_grouped_plan(h: int, w: int, c: int, groups: int, precision=None, fill_frames: Optional[int] = None) -> GroupedPlan:
    """Should this grouped 3x3 layer take conv_grouped_forward?  Host-only query (bts_conv_grouped_plan); ``precision`` /
    ``fill_frames`` default to the launch_config in force."""
    ff, pr = _resolve_launch(precision, fill_frames, "conv_grouped_plan")
    bm, bn, wgs = C.c_int(0), C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_conv_grouped_plan(int(h), int(w), int(c), int(groups), int(pr), int(ff), C.byref(bm), C.byref(bn),
                                                       C.byref(wgs)), "bts_conv_grouped_plan")
    return GroupedPlan((bm.value, bn.value, wgs.value))


def conv_grouped_forward(x2d: torch.Tensor, B: int, h: int, w: int, w_packed: torch.Tensor, c: int, groups: int,
                         e1: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, act: int = ACT_NONE,
                         y2d: Optional[torch.Tensor] = None, tag: str = "grouped_conv"):
    """act(e1(grouped conv3x3(x))) in one launch of the multi-block MFMA kernel (bts_conv_grouped_fwd_f32): stride 1,
    padding 1, x2d [B*h*w, >= c] NHWC view (c channels read), w_packed from pack_grouped_native, e1 a (scale, shift) pair of
    >= c floats, y2d [B*h*w, c] NHWC view (a channel slice is fine; allocated when None).  Runs whatever the plan query
    says: callers ask conv_grouped_plan first."""
    name = "conv_grouped_forward"
    xs, xc = _rows2d(x2d, name)
    if y2d is None:
        y2d = torch.empty((B * h * w, c), dtype=torch.float32, device=x2d.device)
    ys, yc = _rows2d(y2d, name)
    _need(w_packed, name)
    if c <= 0 or groups <= 0 or c % groups:
        raise BtsHipError("conv_grouped_forward: %d channels do not split into %d groups" % (c, groups))
    cg = c // groups
    if c % 64 or cg not in (4, 8, 16):
        raise BtsHipError("conv_grouped_forward: c = %d in groups of %d; needs c %% 64 == 0 and 4, 8 or 16 channels per group" % (c, cg))
    if xc < c or yc != c or x2d.shape[0] != B * h * w or y2d.shape[0] != B * h * w:
        raise BtsHipError("conv_grouped_forward: views %s / %s do not fit B=%d %dx%d, %d channels"
                          % (tuple(x2d.shape), tuple(y2d.shape), B, h, w, c))
    if w_packed.numel() != 144 * c or not w_packed.is_contiguous():
        raise BtsHipError("conv_grouped_forward: w_packed must come from pack_grouped_native (144 * c floats)")
    _check_act3(act, name)
    es, eb = _e2_vectors(e1, c, name, "e1")
    kern, flops, nbytes, xflops = "conv", 0.0, 0.0, None
    if _trace is not None:
        kern = conv_plan.grouped_kernel_name(cg)
        flops = 2.0 * B * h * w * c * cg * 9
        nbytes = 4.0 * (2 * B * h * w * c + 9 * c * cg)
        xflops = 2.0 * 9 * 16 * (B * ((h + 7) // 8) * ((w + 15) // 16) * 128) * c    # 16-channel blocks, ragged tiles included
    _enqueue("bts_conv_grouped_fwd_f32", x2d,
             (_ptr(x2d), xs, B, h, w, c, groups, _ptr(w_packed), _ptr(es), _ptr(eb), int(act), _ptr(y2d), ys),
             trace=(kern, tag, flops, nbytes, xflops))
    return y2d


# ---- the same layers with bf16 operands (csrc/conv_grouped_bf16.inc), opt-in beside the bundle launch of precision "bf16"
def pack_grouped_native_bf16(w: torch.Tensor, groups: int) -> torch.Tensor:
    """Grouped [c, c/groups, 3, 3] weight -> the 144 * c bfloat16 bts_conv_grouped_bf16_fwd_f32 reads (include/bts_hip.h; no
    padding tap): index (((s*9 + tap)*4 + b)*64 + lane)*4 + j = the weight from input channel 64 s + 16 b + 4 (lane >> 4) + j
    to output channel 64 s + 16 b + (lane & 15), rounded by Tensor.to(torch.bfloat16) (nearest, ties to even), exact zeros
    where the two lie in different groups.  Once per weight (ResNetHip.packed caches it)."""
    c, cg = _grouped_native_shape(w, groups)
    wv = w.detach().float().to(torch.bfloat16).reshape(c // 64, 4, 16, cg, 9)   # [slab, block, row, k in group, tap]
    k = torch.arange(16, device=w.device)
    full = wv[:, :, :, k % cg, :]                                           # [slab, block, row, k in block, tap]
    same = (k[:, None] // cg) == (k[None, :] // cg)                         # [row, k]: one group
    full = torch.where(same[None, None, :, :, None], full, torch.zeros((), dtype=torch.bfloat16, device=w.device))
    full = full.reshape(c // 64, 4, 16, 4, 4, 9)                            # [slab, block, row, k-quad, j, tap]
    return full.permute(0, 5, 1, 3, 2, 4).contiguous().view(-1)             # (slab, tap, block, k-quad, row, j): lane = 16 k-quad + row


def pack_grouped_native_bf16_reference(w: torch.Tensor, groups: int) -> torch.Tensor:
    """Index-by-index statement of pack_grouped_native_bf16, kept as its test oracle: every flat index decoded as the header
    writes it."""
    c, cg = _grouped_native_shape(w, groups)
    wc = w.detach().float().cpu().to(torch.bfloat16)
    idx = torch.arange(144 * c)
    j, lane, b, tap, s = idx % 4, (idx // 4) % 64, (idx // 256) % 4, (idx // 1024) % 9, idx // 9216
    n, ci = 64 * s + 16 * b + lane % 16, 64 * s + 16 * b + 4 * (lane // 16) + j       # output channel, input channel
    val = wc[n, ci % cg, tap // 3, tap % 3]
    return torch.where(ci // cg == n // cg, val, torch.zeros((), dtype=torch.bfloat16)).to(w.device)


def conv_grouped_bf16_plan(h: int, w: int, c: int, groups: int, precision=None, fill_frames: Optional[int] = None) -> GroupedPlan:
    """Should this grouped 3x3 layer take conv_grouped_bf16_forward?  Host-only query (bts_conv_grouped_bf16_plan);
    ``precision`` / ``fill_frames`` default to the launch_config in force; only precision "bf16" is ever eligible."""
    ff, pr = _resolve_launch(precision, fill_frames, "conv_grouped_bf16_plan")
    bm, bn, wgs = C.c_int(0), C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_conv_grouped_bf16_plan(int(h), int(w), int(c), int(groups), int(pr), int(ff), C.byref(bm),
                                                            C.byref(bn), C.byref(wgs)), "bts_conv_grouped_bf16_plan")
    return GroupedPlan((bm.value, bn.value, wgs.value))


def conv_grouped_bf16_forward(x2d: torch.Tensor, B: int, h: int, w: int, w_packed: torch.Tensor, c: int, groups: int,
                              e1: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, act: int = ACT_NONE,
                              y2d: Optional[torch.Tensor] = None, tag: str = "grouped_conv"):
    """act(e1(grouped conv3x3(bf16(x), bf16(w)))) in one launch of the bf16 grouped kernel (bts_conv_grouped_bf16_fwd_f32):
    the views, e1 and y2d of conv_grouped_forward (fp32 in and out), w_packed the 144 * c bfloat16 of
    pack_grouped_native_bf16.  Runs whatever the plan query says: callers ask conv_grouped_bf16_plan first."""
    name = "conv_grouped_bf16_forward"
    xs, xc = _rows2d(x2d, name)
    if y2d is None:
        y2d = torch.empty((B * h * w, c), dtype=torch.float32, device=x2d.device)
    ys, yc = _rows2d(y2d, name)
    cg = _grouped_cg(c, groups, name)
    if xc < c or yc != c or x2d.shape[0] != B * h * w or y2d.shape[0] != B * h * w:
        raise BtsHipError("conv_grouped_bf16_forward: views %s / %s do not fit B=%d %dx%d, %d channels"
                          % (tuple(x2d.shape), tuple(y2d.shape), B, h, w, c))
    if (not isinstance(w_packed, torch.Tensor) or w_packed.dtype != torch.bfloat16 or w_packed.numel() != 144 * c
            or not w_packed.is_contiguous() or w_packed.device != x2d.device):
        raise BtsHipError("conv_grouped_bf16_forward: w_packed must come from pack_grouped_native_bf16 (144 * c bfloat16)")
    _check_act3(act, name)
    es, eb = _e2_vectors(e1, c, name, "e1")
    kern, flops, nbytes, xflops = "conv", 0.0, 0.0, None
    if _trace is not None:
        kern = conv_plan.grouped_bf16_kernel_name(cg)
        flops = 2.0 * B * h * w * c * cg * 9
        nbytes = 4.0 * 2 * B * h * w * c + 2.0 * 9 * c * cg
        xflops = 2.0 * 9 * 16 * (B * ((h + 7) // 8) * ((w + 15) // 16) * 128) * c    # 16-channel blocks, ragged tiles included
    _enqueue("bts_conv_grouped_bf16_fwd_f32", x2d,
             (_ptr(x2d), xs, B, h, w, c, groups, _ptr(w_packed), _ptr(es), _ptr(eb), int(act), _ptr(y2d), ys),
             trace=(kern, tag, flops, nbytes, xflops))
    return y2d


def _grouped_cg(c: int, groups: int, who: str) -> int:
    if c <= 0 or groups <= 0 or c % groups:
        raise BtsHipError("%s: %d channels do not split into %d groups" % (who, c, groups))
    cg = c // groups
    if c % 64 or cg not in (4, 8, 16):
        raise BtsHipError("%s: c = %d in groups of %d; needs c %% 64 == 0 and 4, 8 or 16 channels per group" % (who, c, cg))
    return cg


def grouped_native_supported(c: int, groups: int) -> bool:
    """The shapes bts_conv_grouped_fwd_f32 / bts_conv_grouped_wgrad_f32 run (csrc/conv_grouped.inc: grouped_supported)."""
    return c > 0 and groups > 0 and c % groups == 0 and c % 64 == 0 and c // groups in (4, 8, 16)


def grouped_dgrad_weight(w: torch.Tensor, groups: int) -> torch.Tensor:
    """w_t[cg g + i][o][8 - tap] = w[cg g + o][i][tap]: the grouped weight whose forward convolution is the input gradient of
    ``w``'s (taps flipped, each group's matrix transposed)."""
    c, cg = int(w.shape[0]), int(w.shape[1])
    wg = w.detach().reshape(groups, cg, cg, 9)                              # [g, o, i, tap]
    return wg.permute(0, 2, 1, 3).flip(3).reshape(c, cg, 3, 3).contiguous()


def pack_grouped_train_reference(w: torch.Tensor, groups: int, dgrad: bool) -> torch.Tensor:
    """Index-by-index statement of the two per-step packs train.WeightPacker keeps of a natively run grouped weight
    (bts_pack_weights_f32 gmode 3 / 4, include/bts_hip.h), kept as their test oracle: float ((s*9 + tap)*16 + k)*64 + lane
    pairs output channel n = 64 s + lane with input channel ci = 64 s + 16 (lane >> 4) + k; forward w[n][ci mod cg][tap],
    input gradient w[ci][n mod cg][8 - tap], exact zeros across groups."""
    c, cg = _grouped_native_shape(w, groups)
    wc = w.detach().float().cpu().reshape(c, cg, 9)
    idx = torch.arange(144 * c)
    lane, k, tap, s = idx % 64, (idx // 64) % 16, (idx // 1024) % 9, idx // 9216
    n, ci = 64 * s + lane, 64 * s + 16 * (lane // 16) + k
    val = wc[ci, n % cg, 8 - tap] if dgrad else wc[n, ci % cg, tap]
    return torch.where(ci // cg == n // cg, val, torch.zeros(())).to(w.device)


def conv_grouped_wgrad_plan(B: int, h: int, w: int, c: int, groups: int, ws_floats: int = 0) -> Tuple[int, int]:
    """(splits, workspace floats written) of conv_grouped_wgrad with a workspace of ``ws_floats`` floats (0 = none): the
    library's own rule (bts_conv_grouped_wgrad_plan), host arithmetic only."""
    splits, used = C.c_int(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_conv_grouped_wgrad_plan(int(B), int(h), int(w), int(c), int(groups), int(ws_floats),
                                                             C.byref(splits), C.byref(used)), "bts_conv_grouped_wgrad_plan")
    return splits.value, used.value


def conv_grouped_wgrad(x2d: torch.Tensor, B: int, h: int, w: int, dy2d: torch.Tensor, c: int, groups: int,
                       ws: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None, tag: str = "grouped_wgrad"):
    """Weight gradient of the grouped 3x3 convolution (stride 1, padding 1) on the multi-block MFMA kernel
    (bts_conv_grouped_wgrad_f32): x2d / dy2d [B*h*w, >= c] NHWC views (c channels read), returns dw in the parameter's own
    OIHW layout [c, c/groups, 3, 3] (``dw``: a contiguous tensor of that many floats to write instead).  ``ws``: scratch for
    the split partials; None runs unsplit."""
    name = "conv_grouped_wgrad"
    cg = _grouped_cg(c, groups, name)
    xs, ds = _rows2d_c(x2d, c, B * h * w, name), _rows2d_c(dy2d, c, B * h * w, name)
    if dw is None:
        dw = torch.empty((c, cg, 3, 3), dtype=torch.float32, device=x2d.device)
    _need(dw, name)
    if dw.numel() != c * cg * 9 or not dw.is_contiguous() or dw.data_ptr() % 16:
        raise BtsHipError("conv_grouped_wgrad: dw must be %d contiguous floats, 16-byte aligned" % (c * cg * 9))
    nws = 0
    if ws is not None:
        _need(ws, name)
        if not ws.is_contiguous() or ws.data_ptr() % 16:
            raise BtsHipError("conv_grouped_wgrad: ws must be contiguous and 16-byte aligned")
        nws = ws.numel()
    kern, flops, nbytes, xflops = "wgrad", 0.0, 0.0, None
    if _trace is not None:
        kern = conv_plan.grouped_wgrad_kernel_name(cg)
        flops = 2.0 * B * h * w * c * cg * 9
        nbytes = 4.0 * (2 * B * h * w * c + 9 * c * cg)
        xflops = 2.0 * 9 * 16 * B * h * w * c                                # 16-channel blocks; pixels outside the map are skipped
    _enqueue("bts_conv_grouped_wgrad_f32", x2d, (_ptr(x2d), xs, _ptr(dy2d), ds, B, h, w, c, groups, _ptr(dw), _ptr(ws), nws),
             trace=(kern, tag, flops, nbytes, xflops))
    return dw


def pad_vec(v: Optional[torch.Tensor], n: int, fill: float = 0.0) -> Optional[torch.Tensor]:
    if v is None:
        return None
    out = torch.full((n,), fill, dtype=torch.float32, device=v.device)
    out[: v.numel()] = v.float().reshape(-1)
    return out


def bn_affine(weight, bias, mean, var, eps: float):
    """Eval-mode BatchNorm as y = x*scale + shift (ATen batch_norm_cpu_transform_input form)."""
    invstd = 1.0 / torch.sqrt(var.float() + eps)
    scale = weight.float() * invstd
    shift = bias.float() - mean.float() * scale
    return scale, shift


# ---- per-call launch configuration -----------------------------------------------------------------------------------
# Two facts about a convolution launch belong to the CALLER, not to the process: the arithmetic of the contraction
# (bts_conv_desc.precision: 0 = fp32-input MFMA, 1 = fp32 emulated on the bf16 matrix cores, 2 = bf16 operands with fp32
# accumulation -- an inference mode) and the number of frames
# the caller expects to share the chip (bts_conv_desc.fill_frames, which sizes split-K and the tile family; 0 = the
# library default of 8).  Both change output BITS (fp32 summation order / product rounding), so two models in one
# process must be able to hold different values: they live in a thread-local scope that a model opens around its own
# forward (``BtsModel.fill_frames`` / ``BtsModel.conv_precision``, bts_amd/bts.py) -- there is no process-wide setter.
# Code that calls conv_forward directly (tests, micro-benchmarks) wraps the calls in ``launch_config(...)``.
_cfg_tls = threading.local()
_PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16": 2, 0: 0, 1: 1, 2: 2}


def _resolve_launch(precision, fill_frames, who: str) -> Tuple[int, int]:
    """(fill_frames, precision) a call made now runs under: the launch_config in force with the caller's overrides
    (``None`` keeps the enclosing value); like current_launch_config, $BTS_CONV_PRECISION=1 wins over both."""
    ff, pr = current_launch_config()
    if precision is not None:
        if precision not in _PRECISIONS:
            raise BtsHipError("%s: precision must be 'fp32' / 0, 'bf16x3' / 1 or 'bf16' / 2" % who)
        pr = 1 if _ENV_PRECISION else _PRECISIONS[precision]
    if fill_frames is not None:
        ff = int(fill_frames)
        if ff < 0 or ff > 4096:
            raise BtsHipError("%s: fill_frames must be in 0..4096" % who)
    return ff, pr


class launch_config:
    """``with ops.launch_config(fill_frames=2, precision="bf16x3"): ...`` -- values for every conv_forward call issued by
    this thread inside the block; ``None`` keeps the enclosing value (library defaults outside any block)."""

    def __init__(self, fill_frames: Optional[int] = None, precision=None):
        _resolve_launch(precision, fill_frames, "launch_config")
        self._new = (None if fill_frames is None else int(fill_frames), None if precision is None else _PRECISIONS[precision])

    def __enter__(self):
        self._prev_raw = getattr(_cfg_tls, "value", None)
        self._prev = current_launch_config()
        ff, pr = self._new
        _cfg_tls.value = (self._prev[0] if ff is None else ff, self._prev[1] if pr is None else pr)
        return self

    def __exit__(self, *exc):
        _cfg_tls.value = self._prev_raw
        return False


# Outside any launch_config scope the precision is $BTS_CONV_PRECISION (0 / 1, the knob libbts_hip.so itself reads as an
# override of every descriptor): `BTS_CONV_PRECISION=1 python -m pytest tests -m gpu` runs the WHOLE suite -- module-level
# ops, models, training forward AND backward (autograd runs the backward outside the model's scope) -- in the emulated
# arithmetic, pre-split weights included.
_ENV_PRECISION = 1 if os.environ.get("BTS_CONV_PRECISION", "0").strip() == "1" else 0


def current_launch_config() -> Tuple[int, int]:
    """(fill_frames, precision) in force for this thread."""
    v = getattr(_cfg_tls, "value", None)
    if v is None:
        return (0, _ENV_PRECISION)
    return (v[0], 1 if _ENV_PRECISION else v[1])


def launch_config_active() -> bool:
    """True inside a ``launch_config`` block of this thread (a model called from another model's forward keeps the
    outer declaration)."""
    return getattr(_cfg_tls, "value", None) is not None


def model_launch_config(module, batch: int) -> "launch_config":
    """The scope a model opens around its forward: its ``fill_frames`` attribute (None = ``auto_fill_frames(batch)``)
    and its ``conv_precision`` attribute."""
    ff = getattr(module, "fill_frames", None)
    return launch_config(auto_fill_frames(batch) if ff is None else ff, getattr(module, "conv_precision", 0))


def auto_fill_frames(batch: int) -> int:
    """The frames-per-launch declaration a model makes when its ``fill_frames`` attribute is None: a function of the
    batch it was called with, in three coarse classes (so bits change only between classes, documented in DESIGN 5a):
    single-frame callers (the reference's own test loop, bts_test.py:127-147: B = 1) get the latency setting; small
    batches the library default; chip-filling batches the setting bench.py declares."""
    if batch <= 2:
        return 2
    if batch <= 11:
        return 8
    return 16


def split_bf16x3(w: torch.Tensor) -> torch.Tensor:
    """The emulated mode's three-way truncation split of a float32 tensor, done offline: returns int16 [.., 3, R, K] for a
    [.., R, K] input -- plane 0 = top 16 bits of w, plane 1 = top 16 bits of (w - plane 0), plane 2 = top 16 bits of the
    remainder (both subtractions are exact in fp32; w - (h + m + l) <= 2^-24 |w|).  Bit for bit what the kernels' own
    split_store does to an operand on its way to LDS (csrc/conv_mfma.hip)."""
    _need(w, "split_bf16x3")
    hi = w.view(torch.int32) & -65536
    r1 = w - hi.view(torch.float32)
    mid = r1.view(torch.int32) & -65536
    lo = (r1 - mid.view(torch.float32)).view(torch.int32) & -65536
    planes = torch.stack([hi, mid, lo], dim=-3)
    return (planes >> 16).to(torch.int16).contiguous()


def round_bf16(w: torch.Tensor) -> torch.Tensor:
    """The bf16 mode's weight plane, made offline: int16 [.., 1, R, K] holding the bits of w rounded to the nearest bf16
    (ties to even) for a [.., R, K] float32 input -- ``Tensor.to(torch.bfloat16)``, bit for bit what the kernels' own
    rne_store does to an operand on its way to LDS (csrc/conv_mfma.hip)."""
    _need(w, "round_bf16")
    return w.to(torch.bfloat16).view(torch.int16).unsqueeze(-3).contiguous()


def _derived_weight(w_packed: torch.Tensor, attr: str, make, refill=None):
    """A form of a packed weight made once and cached on it as ``attr``; re-made in place when train.WeightPacker has
    refilled the packed buffer since (``_bts_pack_seq``, bumped whenever it refills the buffer): by ``refill(w_packed,
    cached)`` when the form can be written straight into its buffer, else by a copy of ``make(w_packed)``."""
    cached = getattr(w_packed, attr, None)
    seq = getattr(w_packed, "_bts_pack_seq", 0)
    if cached is None or getattr(w_packed, attr + "_seq", 0) != seq:
        if cached is None:
            cached = make(w_packed)
        elif refill is not None:
            refill(w_packed, cached)
        else:
            cached.copy_(make(w_packed))
        setattr(w_packed, attr, cached)
        setattr(w_packed, attr + "_seq", seq)
    return cached


_WINO = os.environ.get("BTS_CONV_WINO", "1").strip() not in ("", "0")      # fused Winograd F(2x2,3x3) for eligible 3x3 layers (0: direct kernels, A/B)


def pack_wino_weight(w_packed: torch.Tensor, c_in_ld: int, n_tail: int = 0, c_out16: int = 0,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Winograd F(2x2,3x3) form of a packed 3x3 weight ([c_out_pad, round_up(9 * c_in_ld, 32)], tap-major K as
    pack_conv_weight lays it out), in the B-fragment order conv_wino_kernel loads: one launch of bts_pack_wino_f32
    (include/bts_hip.h documents the layout; pack_wino_weight_reference is the torch statement of the same).  ``out``:
    refill an existing buffer (the training step re-transforms its weights every iteration)."""
    _need(w_packed, "pack_wino_weight")
    cop = w_packed.shape[0]
    if w_packed.dim() != 2 or not w_packed.is_contiguous() or w_packed.shape[1] != round_up(9 * c_in_ld, 32):
        raise BtsHipError("pack_wino_weight: needs a packed 3x3 weight [c_out_pad, round_up(9 * c_in_ld, 32)]")
    n = _lib.load_real().bts_pack_wino_floats(cop, c_in_ld, n_tail, c_out16)
    if n <= 0:
        raise BtsHipError("pack_wino_weight: needs a 3x3 weight whose buffer channels are whole 32-channel chunks"
                          " (and c_out16 a multiple of 16 within the packed rows)")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=w_packed.device)
    elif out.numel() != n or not out.is_contiguous() or out.device != w_packed.device:
        raise BtsHipError("pack_wino_weight: `out` does not fit this weight")
    _enqueue("bts_pack_wino_f32", w_packed, (w_packed.data_ptr(), cop, w_packed.shape[1], c_in_ld, n_tail, c_out16, out.data_ptr()))
    return out


def pack_wino_weight_reference(w_packed: torch.Tensor, c_in_ld: int, n_tail: int = 0, c_out16: int = 0) -> torch.Tensor:
    """torch (fp64 einsum) statement of pack_wino_weight, kept as its test oracle.  Winograd F(2x2,3x3) form of a packed 3x3 weight ([c_out_pad, 9 * c_in_ld], tap-major K as pack_conv_weight lays
    it out): U = G g G^T per (output, input) channel, computed in fp64 and rounded once, in the B-fragment order
    conv_wino_kernel loads.  Default (32-wide channel tiles, v_mfma_f32_32x32x2_f32): float index
    (((((xi * nchunks + chunk) * n_ct + ct) * 4 + g) * 64 + lh * 32 + li) * 4 + q = U[xi][n = 32 ct + li][k = 32 chunk + 8 g + 4 lh + q].
    ``c_out16`` > 0 (the 48-wide tile, v_mfma_f32_16x16x4_f32; c_out16 = real output channels, a multiple of 16):
    (((((xi * nchunks + chunk) * n_ct16 + ct) * 2 + g) * 64 + l) * 4 + q = U[xi][n = 16 ct + (l & 15)][k = 32 chunk + 16 g + 4 (l >> 4) + q].
    ``n_tail`` > 0: the last 4 of the c_in_ld input channels are the planar tail operand (bts_conv_desc.tail_planes): U
    covers the c_in_ld - 4 buffer channels only (whole chunks) -- the kernel adds the tail's products directly from the
    packed fp32 weights."""
    _need(w_packed, "pack_wino_weight")
    cop = w_packed.shape[0]
    c_main = c_in_ld - (4 if n_tail else 0)
    if c_main <= 0 or c_main % 32 or cop % 32 or w_packed.shape[1] != round_up(9 * c_in_ld, 32):
        raise BtsHipError("pack_wino_weight: needs a 3x3 weight whose buffer channels are whole 32-channel chunks")
    g = w_packed[:, :9 * c_in_ld].reshape(cop, 3, 3, c_in_ld).permute(0, 3, 1, 2).double()     # [n, k, 3, 3]
    g = g[:, :c_main]
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=w_packed.device)
    U = torch.einsum("ia,nkab,jb->nkij", G, g, G).float().reshape(cop, c_main, 16)              # [n, k, xi = 4 i + j]
    nchunks = c_main // 32
    if c_out16:
        if c_out16 % 16 or c_out16 > cop:
            raise BtsHipError("pack_wino_weight: c_out16 must be a multiple of 16 within the packed rows")
        U = U[:c_out16].reshape(c_out16 // 16, 16, nchunks, 2, 4, 4, 16)                        # (ct, col, chunk, g, kq, q, xi)
        return U.permute(6, 2, 0, 3, 4, 1, 5).contiguous().view(-1)                              # (xi, chunk, ct, g, kq, col, q): lane = 16 kq + col
    U = U.view(cop // 32, 32, nchunks, 4, 2, 4, 16)                                             # (ct, li, chunk, g, lh, q, xi)
    return U.permute(6, 2, 0, 3, 4, 1, 5).contiguous().view(-1)                                  # (xi, chunk, ct, g, lh, li, q)


def _conv_describe(x2d, B, h_in, w_in, w_packed, c_out, ksize, dil, up, c_in_ld, pre, pre_relu, e1, act, e2, y2d, y_nchw,
                   stride, pad, y2_2d, subpixel, splitk_ws, res2d, n_bundles, tail_planes):
    """conv_forward's argument checks and its descriptor: (filled ConvDesc, output tensor, tensors to keep alive)."""
    xs, xc = _rows2d(x2d, "conv_forward")
    _need(w_packed, "conv_forward")
    n_tail = len(tail_planes) if tail_planes else 0
    if c_in_ld is None:
        c_in_ld = xc + (4 if n_tail else 0)
    if subpixel:
        if ksize != 3 or up != 2 or dil != 1 or stride != 1 or w_packed.dim() != 3 or w_packed.shape[0] != 4:
            raise BtsHipError("conv_forward: subpixel needs ksize=3, up=2 and weights from pack_upconv_subpixel")
        _, c_out_pad, k_pad = w_packed.shape
    elif n_bundles > 1:
        if w_packed.dim() != 3 or w_packed.shape[0] != n_bundles or c_in_ld is None:
            raise BtsHipError("conv_forward: bundled weights must be [n_bundles, c_out_pad, k_pad] with c_in_ld per bundle")
        _, c_out_pad, k_pad = w_packed.shape
    else:
        c_out_pad, k_pad = w_packed.shape
    if pad is None:
        pad = dil * (ksize // 2)
    d = conv_plan.geometry_desc(B, h_in, w_in, c_in_ld, c_out, ksize, dil, stride, pad, up, subpixel, n_bundles, n_tail,
                                y_nchw is not None, *current_launch_config(), x_pix_stride=xs, c_out_pad=c_out_pad)
    if k_pad != d.k_pad or not w_packed.is_contiguous():
        raise BtsHipError("conv_forward: packed weight [%d,%d] does not match ksize %d / c_in_ld %d"
                          % (c_out_pad, k_pad, ksize, c_in_ld))
    if c_in_ld % 4 or (c_in_ld - (4 if n_tail else 0)) * n_bundles > xc or x2d.shape[0] != B * h_in * w_in:
        raise BtsHipError("conv_forward: bad input view (c_in_ld %d, view %s)" % (c_in_ld, tuple(x2d.shape)))
    if n_tail:
        if ksize != 3 or stride != 1 or dil != 1 or up != 1 or subpixel or n_bundles > 1:
            raise BtsHipError("conv_forward: tail_planes need a plain 3x3 / stride 1 / dilation 1 convolution")
        for j, t in enumerate(_dense_planes(tail_planes, B * h_in * w_in, "conv_forward")):
            d.tail_planes[j] = t.data_ptr()
    H, W = conv_out_hw(h_in, w_in, ksize, dil, stride, pad, up)
    d.x, d.w = x2d.data_ptr(), w_packed.data_ptr()
    keep = []
    for name, pair, n in (("pre", pre, c_in_ld * n_bundles), ("e1", e1, c_out_pad * n_bundles), ("e2", e2, c_out_pad * n_bundles)):
        if pair is not None:
            s, b = pair
            if s.numel() != n or b.numel() != n:
                raise BtsHipError("conv_forward: %s vectors must have %d elements" % (name, n))
            _need(s, "conv_forward")
            _need(b, "conv_forward")
            keep += [s, b]
            setattr(d, name + "_scale", s.data_ptr())
            setattr(d, name + "_shift", b.data_ptr())
    d.pre_relu, d.act = int(bool(pre_relu)), int(act)
    if (y2d is None) == (y_nchw is None):
        raise BtsHipError("conv_forward: give exactly one of y2d / y_nchw")
    if y2d is not None:
        def rows(t, what):                                 # an NHWC view of the whole output: (pointer, pixel stride)
            ts, tc = _rows2d(t, "conv_forward")
            if tc != c_out * n_bundles or t.shape[0] != B * H * W:
                raise BtsHipError("conv_forward: bad %s" % what)
            return t.data_ptr(), ts

        out = y2d
        d.y, d.y_pix_stride = rows(y2d, "output view")
        if y2_2d is not None:
            d.y2, d.y2_pix_stride = rows(y2_2d, "second output view")
        if res2d is not None:
            d.res, d.res_pix_stride = rows(res2d, "residual view %s" % (tuple(res2d.shape),))
    else:
        if res2d is not None or n_bundles > 1:
            raise BtsHipError("conv_forward: residual / bundled convolutions write NHWC only")
        _need(y_nchw, "conv_forward")
        if tuple(y_nchw.shape) != (B, c_out, H, W) or not y_nchw.is_contiguous():
            raise BtsHipError("conv_forward: y_nchw must be contiguous [B,c_out,H,W]")
        d.y = y_nchw.data_ptr()
        out = y_nchw
    if splitk_ws is not None:
        _need(splitk_ws, "conv_forward")
        if not splitk_ws.is_contiguous():
            raise BtsHipError("conv_forward: splitk_ws must be contiguous")
        d.splitk_ws, d.splitk_ws_floats = splitk_ws.data_ptr(), splitk_ws.numel()
    return d, out, keep


def _conv_derived_weights(d: ConvDesc, w_packed: torch.Tensor, keep: list):
    """The forms of ``w_packed`` this descriptor's mode wants besides the packed fp32 matrix, each made once per packed
    weight tensor and kept on it: (bf16 planes or None, Winograd form or None), also set on ``d``."""
    wsplit_t = uw = None
    c_main = d.c_in_ld - (4 if d.n_tail else 0)
    if d.precision in (1, 2) and not d.n_bundles and not d.n_tail:
        # weights pre-split into bf16 planes (precision 1) or pre-rounded to one bf16 plane (precision 2) for the halo-tile
        # kernels of those modes (LDS-DMA of plain bytes)
        wsplit_t = (_derived_weight(w_packed, "_bts_split3", split_bf16x3) if d.precision == 1 else
                    _derived_weight(w_packed, "_bts_round1", round_bf16))
        keep.append(wsplit_t)
        d.w_split = wsplit_t.data_ptr()
    if (_WINO and d.precision == 0 and d.ksize == 3 and d.stride == 1 and d.dil == 1 and d.pad == 1 and d.up == 1
            and not d.n_bundles and c_main % 32 == 0 and d.c_in_ld > 4 and not d.y_nchw):
        # Winograd-form weights for the fused F(2x2,3x3) kernel
        def make(w):
            # which channel tile the library will use for this layer (its own decision on the COMPLETE descriptor, asked
            # once per weight: the two packings differ): 48 -> the 16x16x4 tile.  (bn is choose_tile's pure function of
            # c_out, whatever kernel family this particular launch ends up on)
            d.w_wino = w.data_ptr()
            w._bts_wino_c16 = d.c_out if conv_plan.query(d).bn == 48 else 0
            return pack_wino_weight(w, d.c_in_ld, d.n_tail, c_out16=w._bts_wino_c16)

        uw = _derived_weight(w_packed, "_bts_wino", make, refill=lambda w, out: pack_wino_weight(
            w, d.c_in_ld, d.n_tail, c_out16=getattr(w, "_bts_wino_c16", 0), out=out))
        keep.append(uw)
        d.w_wino = uw.data_ptr()
    return wsplit_t, uw


def _conv_trace_accounting(d: ConvDesc, c_in_real: Optional[int], algo_flops: Optional[float]):
    """What a KernelTrace records for this launch: (kernel name, algorithmic FLOPs, algorithmic bytes, FLOPs the kernel's
    own formulation issues).  Only called while a trace is active."""
    B, c_in_ld = d.B, d.c_in_ld
    H, W = (2 * d.h_in, 2 * d.w_in) if d.subpixel else conv_out_hw(d.h_in, d.w_in, d.ksize, d.dil, d.stride, d.pad, d.up)
    flops_taps, taps = (9, 4) if d.subpixel else (d.ksize * d.ksize,) * 2
    cin = c_in_real if c_in_real is not None else c_in_ld
    npix_out = B * H * W
    c_out = d.c_out * max(d.n_bundles, 1)                  # algorithmic FLOPs of the grouped conv are passed in c_in_real
    #                                                        (real input channels per OUTPUT channel = channels per group)
    flops = 2.0 * npix_out * c_out * cin * flops_taps      # algorithmic: the reference's 3x3 on the upsampled map
    if algo_flops is not None:
        flops = float(algo_flops)
    nbytes = 4.0 * (B * d.h_in * d.w_in * cin + npix_out * c_out + flops_taps * c_out * cin)
    plan = conv_plan.query(d, ksteps=True)
    variant = conv_plan.kernel_name(plan, bool(d.y_nchw), bool(d.subpixel))
    xflops = 2.0 * npix_out * c_out * (c_in_ld if d.n_bundles > 1 else cin) * taps
    if plan.family == conv_plan.Family.WINO:
        # MFMA products the Winograd kernel ISSUES: 16 transform positions x 32 tiles x BN channels x c_in per workgroup
        # (4 instead of 9 per output and input channel, plus the ragged 8x16-pixel tiles and the channels padded to BN)
        nwg = B * ((H + 7) // 8) * ((W + 15) // 16) * ((c_out + plan.bn - 1) // plan.bn)
        xflops = 2.0 * nwg * 16 * 32 * plan.bn * c_in_ld
    if plan.dense > 0:                                     # tap skipping (dilated ASPP branches): FLOPs really issued
        xflops *= plan.issued / plan.dense
    return variant, flops, nbytes, xflops


# bts_hip::conv_fwd's `geom` argument: these descriptor fields, in the order csrc/torch_ops.cpp unpacks them
_GEOM_FIELDS = ("x_pix_stride", "c_in_ld", "k_pad", "B", "h_in", "w_in", "up", "ksize", "dil", "stride", "pad", "c_out", "c_out_pad",
                "pre_relu", "act", "y_pix_stride", "y_nchw", "subpixel", "y2_pix_stride", "res_pix_stride", "n_bundles", "precision",
                "fill_frames")


def conv_forward(x2d: torch.Tensor, B: int, h_in: int, w_in: int, w_packed: torch.Tensor, c_out: int,
                 ksize: int, dil: int = 1, up: int = 1, c_in_ld: Optional[int] = None,
                 pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pre_relu: bool = False,
                 e1: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, act: int = ACT_NONE,
                 e2: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                 y2d: Optional[torch.Tensor] = None, y_nchw: Optional[torch.Tensor] = None,
                 tag: str = "conv", c_in_real: Optional[int] = None, stride: int = 1, pad: Optional[int] = None,
                 y2_2d: Optional[torch.Tensor] = None, subpixel: bool = False,
                 splitk_ws: Optional[torch.Tensor] = None, res2d: Optional[torch.Tensor] = None, n_bundles: int = 1,
                 tail_planes: Optional[Sequence[torch.Tensor]] = None, algo_flops: Optional[float] = None):
    """One fused convolution (see bts_conv_desc in include/bts_hip.h).
    ``algo_flops``: FLOPs of the reference formulation this launch stands for, when that is not the launch's own count
    (the tap GEMM of an upconv: 9 tap-products per source pixel for the reference's 36); only used by KernelTrace.
    ``tail_planes``: 1..4 contiguous one-channel maps ([B,1,h_in,w_in] or [B,h_in,w_in]) that supply the LAST input
    channels of the reference's concatenated input (bts.py:260, 274, 287) without ever being copied into the NHWC
    buffer: x2d then holds c_in_ld - 4 channels and w_packed is packed with c_in_ld = (buffer channels) + 4.
    ``subpixel``: w_packed comes from pack_upconv_subpixel; computes nearest-2x + conv3x3 (pass ksize=3, up=2).

    x2d: [B*h_in*w_in, C>=c_in_ld] NHWC view.  Exactly one of y2d ([B*H*W, c_out] NHWC view) /
    y_nchw ([B,c_out,H,W] contiguous) receives the result.  pad defaults to dil*(ksize//2).
    ``res2d``: residual [B*H*W, c_out] added after e1, before the activation.  ``n_bundles`` > 1: grouped convolution
    as independent channel bundles (w_packed [n_bundles, c_out_pad, k_pad] from pack_grouped_conv_weight; c_in_ld /
    c_out are PER BUNDLE, x2d / y2d hold all n_bundles*c_in_ld / n_bundles*c_out channels)."""
    d, out, keep = _conv_describe(x2d, B, h_in, w_in, w_packed, c_out, ksize, dil, up, c_in_ld, pre, pre_relu, e1, act, e2,
                                  y2d, y_nchw, stride, pad, y2_2d, subpixel, splitk_ws, res2d, n_bundles, tail_planes)
    wsplit_t, uw_t = _conv_derived_weights(d, w_packed, keep)
    trace = None
    if _trace is not None:
        kern, flops, nbytes, xflops = _conv_trace_accounting(d, c_in_real, algo_flops)
        trace = (kern, tag, flops, nbytes, xflops)
    tops = torch_ops()
    run = None
    if tops is not None:
        geom = [getattr(d, f) for f in _GEOM_FIELDS]
        (pre_s, pre_b), (e1_s, e1_b), (e2_s, e2_b) = (p if p is not None else (None, None) for p in (pre, e1, e2))
        run = lambda: _op(lambda: tops.conv_fwd(x2d, w_packed, pre_s, pre_b, e1_s, e1_b, e2_s, e2_b, out, y2_2d, res2d, splitk_ws,
                                                list(tail_planes) if tail_planes else [], wsplit_t, uw_t, geom))
    _enqueue("bts_conv_fwd_f32", x2d, (C.byref(d),), trace=trace, run=run)
    return out


def _wgrad_desc(B: int, h_in: int, w_in: int, c_in: int, c_out: int, ksize: int, dil: int, stride: int, pad: int, up: int,
                n_bundles: int, x_pix_stride: int, dy_pix_stride: int) -> ConvWgradDesc:
    """The geometry fields of a bts_conv_wgrad_desc; the caller adds the pointers."""
    d = ConvWgradDesc()
    d.n_bundles = n_bundles if n_bundles > 1 else 0
    d.x_pix_stride, d.c_in, d.dy_pix_stride, d.c_out = x_pix_stride, c_in, dy_pix_stride, c_out
    d.B, d.h_in, d.w_in, d.up, d.ksize, d.dil, d.stride, d.pad = B, h_in, w_in, up, ksize, dil, stride, pad
    return d


_WGRAD_PRECISIONS = {None: 0, "fp32": 0, 0: 0, "bf16": 2, 2: 2}


def wgrad_precision(precision, who: str = "conv_wgrad") -> int:
    """The weight-gradient arithmetic a caller names: 0 (``None`` / "fp32" / 0: the fp32-input MFMA) or 2 ("bf16" / 2: bf16
    operands, fp32 accumulation).  An argument of the call, never read from the launch_config in force: autograd runs
    ``backward`` on another thread, where the scope a model opened is not in force."""
    try:
        return _WGRAD_PRECISIONS[precision]
    except (KeyError, TypeError):
        raise BtsHipError("%s: precision must be 'fp32' / 0 or 'bf16' / 2" % who) from None


BTS_ERR_UNSUPPORTED = -2      # include/bts_hip.h


def conv_wgrad_plan_desc(d: ConvWgradDesc, precision=None) -> Optional[Tuple[int, int, int, int]]:
    """bts_conv_wgrad_plan_f32 on a filled descriptor: (bm, bn, split, pix_per_split).  Host arithmetic only.
    ``precision`` "bf16": bts_conv_wgrad_bf16_plan_f32 -- the same answer, or None for a shape class the bf16 body declines
    (the caller then launches in fp32)."""
    bm, bn, split, pps = C.c_int(0), C.c_int(0), C.c_long(0), C.c_long(0)
    name = "bts_conv_wgrad_bf16_plan_f32" if wgrad_precision(precision, "conv_wgrad_plan") == 2 else "bts_conv_wgrad_plan_f32"
    rc = getattr(_lib.load_real(), name)(C.byref(d), C.byref(bm), C.byref(bn), C.byref(split), C.byref(pps))
    if rc == BTS_ERR_UNSUPPORTED and name == "bts_conv_wgrad_bf16_plan_f32" and _lib.load_real().bts_conv_wgrad_plan_f32(
            C.byref(d), None, None, None, None) == 0:
        return None
    _lib.check(rc, name)
    return bm.value, bn.value, split.value, pps.value


_PLAN_DUMMY_PTR = 1 << 20      # non-null, 16-byte aligned; a plan query checks pointers and never follows them


def conv_wgrad_plan(B: int, h_in: int, w_in: int, c_in: int, c_out: int, ksize: int, dil: int = 1, stride: int = 1,
                    pad: Optional[int] = None, up: int = 1, ws_floats: Optional[int] = None, n_bundles: int = 1,
                    pre: bool = False, pre_relu: bool = False, x_pix_stride: Optional[int] = None,
                    dy_pix_stride: Optional[int] = None, precision=None) -> Optional[Tuple[int, int, int, int]]:
    """Which tile and pixel split conv_wgrad will run for this geometry: (bm, bn, split, pix_per_split), from the
    library's own planner (bts_conv_wgrad_plan_f32).  No tensors and no GPU: the geometry arguments are conv_wgrad's,
    ``ws_floats`` is the size of the workspace it would get (None = no workspace), ``pre`` says whether an input
    prologue rides along, and the pixel strides default to the dense ``n_bundles * c``.  ``precision`` "bf16": the bf16
    query (conv_wgrad_plan_desc) -- None where conv_wgrad(..., precision="bf16") runs the fp32 launch."""
    if pad is None:
        pad = dil * (ksize // 2)
    nb = max(n_bundles, 1)
    d = _wgrad_desc(B, h_in, w_in, c_in, c_out, ksize, dil, stride, pad, up, n_bundles,
                    nb * c_in if x_pix_stride is None else x_pix_stride, nb * c_out if dy_pix_stride is None else dy_pix_stride)
    d.x = d.dy = d.dw = _PLAN_DUMMY_PTR
    if pre:
        d.pre_scale = d.pre_shift = _PLAN_DUMMY_PTR
        d.pre_relu = int(bool(pre_relu))
    if ws_floats is not None:
        d.ws, d.ws_floats = _PLAN_DUMMY_PTR, ws_floats
    return conv_wgrad_plan_desc(d, precision)


_WGRAD_BF16_TAKES: Dict[tuple, bool] = {}      # conv_wgrad geometry -> whether bts_conv_wgrad_bf16_plan_f32 takes it


def conv_wgrad(x2d: torch.Tensor, B: int, h_in: int, w_in: int, c_in: int, dy2d: torch.Tensor, c_out: int,
               ksize: int, dil: int = 1, stride: int = 1, pad: Optional[int] = None, up: int = 1,
               ws: Optional[torch.Tensor] = None, tag: str = "wgrad", n_bundles: int = 1,
               pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, pre_relu: bool = False, precision=None,
               dw: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient of one bias-free convolution (bts_conv_wgrad_f32): returns dw as [c_out, ksize*ksize, c_in]
    (OHWI).  x2d: [B*h_in*w_in, >=c_in] NHWC view of the forward input, dy2d: [B*H*W, >=c_out] NHWC view of the
    output gradient; c_in and c_out multiples of 4 (pad with zero channels).  ``n_bundles`` > 1: grouped convolution
    as channel bundles (c_in / c_out per bundle): returns the dense blocks [n_bundles, c_out, ksize*ksize, c_in].
    ``precision`` "bf16": both operands rounded to bf16 (x after its prologue), fp32 accumulation, same tile and split
    (bts_conv_wgrad_bf16_f32); a shape class its plan query declines runs the fp32 launch.  ``dw``: the buffer that
    receives the gradient instead of a fresh tensor, as conv_grouped_wgrad and WgradBatch take one (a contiguous, 16-byte
    aligned view of exactly that many floats, returned reshaped): a caller that keeps one flat gradient buffer per block or
    bucket has the launch write into it."""
    pr = wgrad_precision(precision)
    xs, xc = _rows2d(x2d, "conv_wgrad")
    ds, dc = _rows2d(dy2d, "conv_wgrad")
    if pad is None:
        pad = dil * (ksize // 2)
    H, W = conv_out_hw(h_in, w_in, ksize, dil, stride, pad, up)
    if c_in % 4 or c_out % 4 or c_in * n_bundles > xc or c_out * n_bundles > dc:
        raise BtsHipError("conv_wgrad: c_in/c_out must be multiples of 4 within the views (%d/%d, %d/%d)" % (c_in, xc, c_out, dc))
    if x2d.shape[0] != B * h_in * w_in or dy2d.shape[0] != B * H * W:
        raise BtsHipError("conv_wgrad: views %s / %s do not match B=%d %dx%d -> %dx%d"
                          % (tuple(x2d.shape), tuple(dy2d.shape), B, h_in, w_in, H, W))
    shape = (c_out, ksize * ksize, c_in) if n_bundles <= 1 else (n_bundles, c_out, ksize * ksize, c_in)
    if dw is None:
        dw = torch.empty(shape, dtype=torch.float32, device=x2d.device)
    else:
        _need(dw, "conv_wgrad")
        if dw.numel() != int(torch.Size(shape).numel()) or not dw.is_contiguous() or dw.data_ptr() % 16 or dw.device != x2d.device:
            raise BtsHipError("conv_wgrad: dw must be a contiguous, 16-byte aligned view of %d floats" % int(torch.Size(shape).numel()))
        dw = dw.view(shape)
    d = _wgrad_desc(B, h_in, w_in, c_in, c_out, ksize, dil, stride, pad, up, n_bundles, xs, ds)
    if pre is not None:                       # the forward conv saw [relu](x*scale + shift): gather the same thing
        if pre[0].numel() != c_in * max(n_bundles, 1) or pre[1].numel() != pre[0].numel():
            raise BtsHipError("conv_wgrad: pre vectors must have c_in entries")
        d.pre_scale, d.pre_shift, d.pre_relu = pre[0].data_ptr(), pre[1].data_ptr(), int(bool(pre_relu))
    d.x, d.dy, d.dw = x2d.data_ptr(), dy2d.data_ptr(), dw.data_ptr()
    if ws is not None:
        _need(ws, "conv_wgrad")
        d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
    taps = ksize * ksize
    flops = 2.0 * B * H * W * c_out * c_in * taps * max(n_bundles, 1)
    nbytes = 4.0 * (B * h_in * w_in * c_in + B * H * W * c_out + taps * c_out * c_in) * max(n_bundles, 1)
    if pr == 2:
        # does the bf16 plan query take this shape class?  A function of the geometry and the workspace size alone: asked
        # once per geometry, not once per launch
        key = (B, h_in, w_in, c_in, c_out, ksize, dil, stride, pad, up, n_bundles, xs, ds, pre is not None, bool(pre_relu),
               None if ws is None else ws.numel())
        ok = _WGRAD_BF16_TAKES.get(key)
        if ok is None:
            if len(_WGRAD_BF16_TAKES) >= 4096:
                _WGRAD_BF16_TAKES.clear()
            ok = _WGRAD_BF16_TAKES[key] = conv_wgrad_plan_desc(d, 2) is not None
        if not ok:
            pr = 0
    if pr == 2:
        _enqueue("bts_conv_wgrad_bf16_f32", x2d, (C.byref(d),), trace=("conv_wgrad_kernel<bf16>", tag, flops, nbytes, None))
    else:
        _enqueue("bts_conv_wgrad_f32", x2d, (C.byref(d),), trace=("conv_wgrad_kernel", tag, flops, nbytes, None))
    return dw


# ---- sub-pixel upconv in the training step (bts_upconv_dgrad_f32 / bts_upconv_wgrad_f32 / bts_upconv_train_pack_f32)
_SUBPIX_S = {0: ((1.0, 0.0, 0.0), (0.0, 1.0, 1.0)), 1: ((1.0, 1.0, 0.0), (0.0, 0.0, 1.0))}   # row sums of _SUBPIX_SETS
_SUBPIX_TAU = {0: (0, 1, 1), 1: (0, 0, 1)}                                                   # 3x3 tap -> class tap (the adjoint)


def upconv_subpixel_grads_reference(x: torch.Tensor, w: torch.Tensor, dy: torch.Tensor):
    """The sub-pixel statement of upconv = conv3x3(nearest2x(x), w, padding 1) and of its two gradients, in fp64 on the
    CPU -- the oracle of the training kernels (include/bts_hip.h states the same three identities).  x [B,c_in,h,w],
    w [c_out,c_in,3,3], dy [B,c_out,2h,2w] -> (y [B,c_out,2h,2w], dx like x, dw like w)."""
    x, w, dy = x.detach().double().cpu(), w.detach().double().cpu(), dy.detach().double().cpu()
    B, cin, h, wd = x.shape
    cout = w.shape[0]
    S = {p: torch.tensor(_SUBPIX_S[p], dtype=torch.float64) for p in (0, 1)}
    g = {(py, px): torch.einsum("ta,ncab,ub->nctu", S[py], w, S[px]) for py in (0, 1) for px in (0, 1)}   # [c_out,c_in,2,2]
    xp = F.pad(x, (1, 1, 1, 1))                       # x[Y-1+py+ty, X-1+px+tx] = xp[Y+py+ty, X+px+tx]
    dyp = F.pad(dy, (1, 1, 1, 1))                     # dy[2Y-1+r, 2X-1+s] = dyp[2Y+r, 2X+s]
    y = torch.zeros((B, cout, 2 * h, 2 * wd), dtype=torch.float64)
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for (py, px), gc in g.items():
        for ty in (0, 1):
            for tx in (0, 1):
                xs = xp[:, :, py + ty:py + ty + h, px + tx:px + tx + wd]
                y[:, :, py::2, px::2] += torch.einsum("nc,bchw->bnhw", gc[:, :, ty, tx], xs)
                r, s = 3 - py - 2 * ty, 3 - px - 2 * tx                                  # K[r,s] = g_(py,px)[ty,tx]^T
                dx += torch.einsum("nc,bnhw->bchw", gc[:, :, ty, tx], dyp[:, :, r:r + 2 * h:2, s:s + 2 * wd:2])
                dg = torch.einsum("bnhw,bchw->nc", dy[:, :, py::2, px::2], xs)
                for ky in range(3):
                    for kx in range(3):
                        if _SUBPIX_TAU[py][ky] == ty and _SUBPIX_TAU[px][kx] == tx:
                            dw[:, :, ky, kx] += dg
    return y, dx, dw


def pack_upconv_dgrad_reference(w: torch.Tensor) -> torch.Tensor:
    """Torch statement of the input-gradient pack bts_upconv_train_pack_f32 writes: [round_up(c_in,32)][round_up(16*c_out,32)]
    with element [c][(4r+s)*c_out + n] = K[r,s][c][n], K[3-py-2ty, 3-px-2tx] = g_(py,px)[ty,tx]^T -- each the fp32 sum
    pack_upconv_subpixel computes for its forward twin (c_in and c_out multiples of 4)."""
    cout, cin = w.shape[0], w.shape[1]
    fwd, cop, cld = pack_upconv_subpixel(w, c_in_ld=cin)
    out = torch.zeros((round_up(cin, 32), round_up(16 * cout, 32)), dtype=torch.float32, device=w.device)
    for py in (0, 1):
        for px in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    rs = 4 * (3 - py - 2 * ty) + (3 - px - 2 * tx)
                    t = 2 * ty + tx
                    out[:cin, rs * cout:(rs + 1) * cout] = fwd[2 * py + px, :cout, t * cld:t * cld + cin].t()
    return out


def upconv_train_pack_shapes(c_out: int, c_in: int) -> Tuple[Tuple[int, int, int], Tuple[int, int]]:
    """Shapes of the two packs of one upconv weight: forward [4, c_out_pad, k_pad] (pack_upconv_subpixel with
    c_in_ld = c_in) and input gradient [c_in_pad, k_pad'] (pack_upconv_dgrad_reference)."""
    return (4, round_up(c_out, 32), round_up(4 * c_in, 32)), (round_up(c_in, 32), round_up(16 * c_out, 32))


def upconv_train_pack(weights: Sequence[torch.Tensor], fwd: Sequence[torch.Tensor], dgrad: Sequence[torch.Tensor],
                      table: Optional[Tuple[torch.Tensor, int]] = None) -> Tuple[torch.Tensor, int]:
    """Both training packs of every upconv weight (contiguous OIHW [c_out,c_in,3,3] fp32, channel counts multiples of 4) in
    ONE launch of bts_upconv_train_pack_f32 into the caller's ``fwd`` / ``dgrad`` buffers (upconv_train_pack_shapes).
    Returns the (device table, blocks) it launched with; pass it back as ``table`` to launch again without an upload --
    the table holds addresses, so only for the same tensors."""
    import numpy as np
    if not weights:
        raise BtsHipError("upconv_train_pack: no weights")
    lib = _lib.load_real()
    dev = weights[0].device
    if table is None:
        rows, first = [], 0
        for wt, f, d in zip(weights, fwd, dgrad):
            for t in (wt, f, d):
                _need(t, "upconv_train_pack")
            cout, cin, kh, kw = wt.shape
            fs, ds = upconv_train_pack_shapes(cout, cin)
            if (kh, kw) != (3, 3) or cout % 4 or cin % 4 or not wt.is_contiguous() or tuple(f.shape) != fs or tuple(d.shape) != ds \
                    or not f.is_contiguous() or not d.is_contiguous():
                raise BtsHipError("upconv_train_pack: weight %s / packs %s, %s do not fit" % (tuple(wt.shape), tuple(f.shape), tuple(d.shape)))
            rows.append([wt.data_ptr(), f.data_ptr(), d.data_ptr(), cout, cin, cin, cout, fs[1], fs[2], ds[0], ds[1], first])
            first += int(lib.bts_upconv_train_pack_blocks(fs[1], fs[2], ds[0], ds[1]))
        table = (torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev), first)
    tab, blocks = table
    _enqueue("bts_upconv_train_pack_f32", weights[0], (tab.data_ptr(), tab.shape[0], blocks),
             trace=("upconv_train_pack_kernel", "pack", 0.0, 0.0, None))
    return table


def upconv_dgrad_plan(B: int, h: int, w: int, c_out: int, c_in: int, splitk_ws_floats: int = 0, precision=None,
                      fill_frames: Optional[int] = None) -> Tuple[int, int, int, bool]:
    """Which kernel upconv_dgrad will launch: (bm, bn, kind, splits K).  Host-only (bts_upconv_dgrad_plan)."""
    ff, pr = _resolve_launch(precision, fill_frames, "upconv_dgrad_plan")
    bm, bn, kind = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.load_real().bts_upconv_dgrad_plan(B, h, w, c_out, c_in, int(pr), int(ff), int(splitk_ws_floats), C.byref(bm),
                                                      C.byref(bn), C.byref(kind)), "bts_upconv_dgrad_plan")
    return bm.value, bn.value, kind.value & 15, bool(kind.value & 16)


def upconv_dgrad(dy2d: torch.Tensor, B: int, h: int, w: int, w_dgrad: torch.Tensor, c_out: int, c_in: int, dx2d: torch.Tensor,
                 splitk_ws: Optional[torch.Tensor] = None, tag: str = "upconv.dgrad", precision=None) -> torch.Tensor:
    """Input gradient of the sub-pixel upconv (bts_upconv_dgrad_f32): dy2d [B*2h*2w, >= c_out] NHWC view -> dx2d
    [B*h*w, c_in] NHWC view (channel slices of wider buffers are fine), one 4x4 / stride-2 convolution with ``w_dgrad``
    from upconv_train_pack.  fp32 or bf16x3 by the launch_config in force; ``splitk_ws`` lets small maps split K.
    ``precision=2``: dy and the pack both rounded to bf16, as the node that recorded train_precision "bf16" in its forward
    asks for by name -- never taken from the launch_config, where "bf16" is the inference mode."""
    ds, dc = _rows2d(dy2d, "upconv_dgrad")
    xs, xc = _rows2d(dx2d, "upconv_dgrad")
    _need(w_dgrad, "upconv_dgrad")
    if c_in % 4 or c_out % 4 or dc < c_out or xc != c_in or dy2d.shape[0] != 4 * B * h * w or dx2d.shape[0] != B * h * w:
        raise BtsHipError("upconv_dgrad: views %s / %s do not fit B=%d %dx%d, %d <- %d channels (multiples of 4)"
                          % (tuple(dy2d.shape), tuple(dx2d.shape), B, h, w, c_in, c_out))
    if tuple(w_dgrad.shape) != upconv_train_pack_shapes(c_out, c_in)[1] or not w_dgrad.is_contiguous():
        raise BtsHipError("upconv_dgrad: w_dgrad must be the input-gradient pack of upconv_train_pack")
    ff, pr = current_launch_config()
    if pr == 2:
        raise BtsHipError("upconv_dgrad: conv_precision 'bf16' is an inference mode")
    if precision is not None:
        if precision != 2:
            raise BtsHipError("upconv_dgrad: precision is None (the launch_config in force) or 2")
        pr = 1 if _ENV_PRECISION else 2
    ws_ptr, ws_n = None, 0
    if splitk_ws is not None:
        _need(splitk_ws, "upconv_dgrad")
        if not splitk_ws.is_contiguous():
            raise BtsHipError("upconv_dgrad: splitk_ws must be contiguous")
        ws_ptr, ws_n = splitk_ws.data_ptr(), splitk_ws.numel()
    kern = "conv"
    if _trace is not None:
        bm, bn, _, sk = upconv_dgrad_plan(B, h, w, c_out, c_in, ws_n, precision=pr)
        kern = "conv_fwd_kernel<%d,%d,k4s2>%s" % (bm, bn, "+splitk" if sk else "")
    flops = 2.0 * 36 * B * h * w * c_out * c_in               # the reference's 3x3 adjoint on the upsampled map
    nbytes = 4.0 * (4 * B * h * w * c_out + B * h * w * c_in + 16 * c_out * c_in)
    _enqueue("bts_upconv_dgrad_f32", dy2d, (_ptr(dy2d), ds, B, h, w, c_out, _ptr(w_dgrad), c_in, _ptr(dx2d), xs, int(pr), int(ff), ws_ptr, ws_n),
             trace=(kern, tag, flops, nbytes, 2.0 * 16 * B * h * w * c_out * c_in))
    return dx2d


def upconv_wgrad_plan(B: int, h: int, w: int, c_in: int, c_out: int, ws_floats: int) -> Tuple[int, int, int, int]:
    """Tile and pixel split upconv_wgrad will run under a workspace of ``ws_floats`` floats: (bm, bn, split,
    pix_per_split); the launch writes split * 16 * c_out * c_in floats of it.  Host-only (bts_upconv_wgrad_plan_f32)."""
    bm, bn, split, pps = C.c_int(0), C.c_int(0), C.c_long(0), C.c_long(0)
    _lib.check(_lib.load_real().bts_upconv_wgrad_plan_f32(B, h, w, c_in, c_out, int(ws_floats), C.byref(bm), C.byref(bn), C.byref(split),
                                                          C.byref(pps)), "bts_upconv_wgrad_plan_f32")
    return bm.value, bn.value, split.value, pps.value


def upconv_wgrad(x2d: torch.Tensor, B: int, h: int, w: int, c_in: int, dy2d: torch.Tensor, c_out: int, ws: torch.Tensor,
                 tag: str = "upconv.wgrad") -> torch.Tensor:
    """Weight gradient of the sub-pixel upconv (bts_upconv_wgrad_f32): x2d [B*h*w, >= c_in], dy2d [B*2h*2w, >= c_out] NHWC
    views -> dw [c_out, 9, c_in] (OHWI, as conv_wgrad).  ``ws`` is mandatory (>= 16 * c_out * c_in floats): the sixteen
    class GEMMs land there, split over pixels as conv_wgrad's planner decides, and a fixed-order launch folds them."""
    xs, xc = _rows2d(x2d, "upconv_wgrad")
    ds, dc = _rows2d(dy2d, "upconv_wgrad")
    if ws is None:
        raise BtsHipError("upconv_wgrad: the workspace is mandatory")
    _need(ws, "upconv_wgrad")
    if c_in % 4 or c_out % 4 or c_in > xc or c_out > dc or x2d.shape[0] != B * h * w or dy2d.shape[0] != 4 * B * h * w:
        raise BtsHipError("upconv_wgrad: views %s / %s do not fit B=%d %dx%d, %d -> %d channels (multiples of 4)"
                          % (tuple(x2d.shape), tuple(dy2d.shape), B, h, w, c_in, c_out))
    if not ws.is_contiguous() or ws.numel() < 16 * c_out * c_in:
        raise BtsHipError("upconv_wgrad: the workspace must be contiguous and hold at least %d floats" % (16 * c_out * c_in))
    dw = torch.empty((c_out, 9, c_in), dtype=torch.float32, device=x2d.device)
    flops = 2.0 * 36 * B * h * w * c_out * c_in
    nbytes = 4.0 * (B * h * w * c_in + 4 * B * h * w * c_out + 9 * c_out * c_in)
    _enqueue("bts_upconv_wgrad_f32", x2d, (_ptr(x2d), xs, B, h, w, c_in, _ptr(dy2d), ds, c_out, _ptr(dw), _ptr(ws), ws.numel()),
             trace=("upconv_wgrad_kernel", tag, flops, nbytes, 2.0 * 16 * B * h * w * c_out * c_in))
    return dw


# ---- many weight gradients in one launch (bts_conv_wgrad_batch_*, include/bts_hip.h)
def conv_wgrad_batch_plan_descs(descs: Sequence[ConvWgradDesc], bases: Sequence[Tuple[int, int]], ws_floats: int,
                                with_table: bool = False):
    """bts_conv_wgrad_batch_plan_f32 on filled descriptors.  ``bases``: (address, bytes) of the ranges every pointer of
    every descriptor must lie in.  Returns one (bm, bn, split, pix_per_split, ws_offset) per problem, in the order
    given (ws_offset -1: unsplit); with ``with_table`` also the host table.  Host arithmetic only."""
    lib = _lib.load_real()
    n, nb = len(descs), len(bases)
    arr = (ConvWgradDesc * max(n, 1))(*descs)
    bp = (C.c_void_p * max(nb, 1))(*[int(a) for a, _ in bases])
    bb = (C.c_long * max(nb, 1))(*[int(b) for _, b in bases])
    table = C.create_string_buffer(int(lib.bts_conv_wgrad_batch_table_bytes(n)))
    items = (ConvWgradBatchItem * max(n, 1))()
    _lib.check(lib.bts_conv_wgrad_batch_plan_f32(arr, n, bp, bb, nb, int(ws_floats), table, items), "bts_conv_wgrad_batch_plan_f32")
    plan = [(it.bm, it.bn, it.split, it.pix_per_split, it.ws_offset) for it in items[:n]]
    return (plan, table) if with_table else plan


def conv_wgrad_batch_plan(problems: Sequence[dict], ws_floats: int) -> List[Tuple[int, int, int, int, int]]:
    """Tiles and pixel splits one batched launch will run for these geometries under a workspace of ``ws_floats`` floats:
    one (bm, bn, split, pix_per_split, ws_offset) per problem, from the library's own batch planner.  No tensors and no
    GPU.  Each problem is a dict of conv_wgrad_plan's arguments (B, h_in, w_in, c_in, c_out, ksize and optionally dil,
    stride, pad, up, n_bundles, pre, pre_relu, x_pix_stride, dy_pix_stride)."""
    descs = []
    for pr in problems:
        pr = dict(pr)
        ksize, dil = pr["ksize"], pr.get("dil", 1)
        pad = pr.get("pad")
        nbun = pr.get("n_bundles", 1)
        nb = max(nbun, 1)
        xs, ds = pr.get("x_pix_stride"), pr.get("dy_pix_stride")
        d = _wgrad_desc(pr["B"], pr["h_in"], pr["w_in"], pr["c_in"], pr["c_out"], ksize, dil, pr.get("stride", 1),
                        dil * (ksize // 2) if pad is None else pad, pr.get("up", 1), nbun,
                        nb * pr["c_in"] if xs is None else xs, nb * pr["c_out"] if ds is None else ds)
        d.x = d.dy = d.dw = _PLAN_DUMMY_PTR
        if pr.get("pre", False):
            d.pre_scale = d.pre_shift = _PLAN_DUMMY_PTR
            d.pre_relu = int(bool(pr.get("pre_relu", False)))
        descs.append(d)
    return conv_wgrad_batch_plan_descs(descs, [(_PLAN_DUMMY_PTR, 1 << 60)], ws_floats)


class WgradBatch:
    """The weight gradients of many convolutions as one batched launch (bts_conv_wgrad_batch_f32).

    ``problems``: one dict per convolution -- ``x`` / ``dy`` ([npix, >=c] NHWC views), ``dw`` (contiguous view of
    n_bundles*c_out*ksize^2*c_in floats that receives the OHWI gradient), optional ``pre`` = (scale, shift) views and
    ``pre_relu``, and conv_wgrad's geometry (B, h_in, w_in, c_in, c_out, ksize, dil, stride, pad, up, n_bundles).  Every
    view must lie inside one of ``bases`` (at most 8 contiguous fp32 tensors).  Construction plans the batch and uploads
    its table once; ``run(bases, ws)`` then launches with any buffers of the same sizes -- the table stores offsets, not
    addresses -- uploading nothing and synchronising nothing, and returns the dw views of the bases it was given.
    dw views that overlap are a caller error."""

    def __init__(self, problems: Sequence[dict], bases: Sequence[torch.Tensor], ws_floats: int, tag: str = "wgrad.batch"):
        self.tag, self.n, self.ws_floats = tag, len(problems), int(ws_floats)
        for b in bases:
            _need(b, "WgradBatch")
            if not b.is_contiguous():
                raise BtsHipError("WgradBatch: bases must be contiguous")
        self.base_numel = [b.numel() for b in bases]
        self.device = bases[0].device if bases else None
        ranges = [(b.data_ptr(), 4 * b.numel()) for b in bases]
        descs, self._dw, self.flops, self.nbytes = [], [], 0.0, 0.0
        for pr in problems:
            x2d, dy2d, dw = pr["x"], pr["dy"], pr["dw"]
            B, h_in, w_in, c_in, c_out, ksize = (pr[k] for k in ("B", "h_in", "w_in", "c_in", "c_out", "ksize"))
            dil, stride, up, nbun = pr.get("dil", 1), pr.get("stride", 1), pr.get("up", 1), pr.get("n_bundles", 1)
            pad = pr.get("pad")
            pad = dil * (ksize // 2) if pad is None else pad
            nb = max(nbun, 1)
            xs, xc = _rows2d(x2d, "WgradBatch")
            ds, dc = _rows2d(dy2d, "WgradBatch")
            _need(dw, "WgradBatch")
            H, W = conv_out_hw(h_in, w_in, ksize, dil, stride, pad, up)
            if c_in % 4 or c_out % 4 or c_in * nb > xc or c_out * nb > dc:
                raise BtsHipError("WgradBatch: c_in/c_out must be multiples of 4 within the views (%d/%d, %d/%d)" % (c_in, xc, c_out, dc))
            if x2d.shape[0] != B * h_in * w_in or dy2d.shape[0] != B * H * W:
                raise BtsHipError("WgradBatch: views %s / %s do not match B=%d %dx%d -> %dx%d"
                                  % (tuple(x2d.shape), tuple(dy2d.shape), B, h_in, w_in, H, W))
            taps = ksize * ksize
            shape = (c_out, taps, c_in) if nbun <= 1 else (nbun, c_out, taps, c_in)
            if not dw.is_contiguous() or dw.numel() != nb * c_out * taps * c_in:
                raise BtsHipError("WgradBatch: dw must be a contiguous view of %d floats" % (nb * c_out * taps * c_in))
            d = _wgrad_desc(B, h_in, w_in, c_in, c_out, ksize, dil, stride, pad, up, nbun, xs, ds)
            pre = pr.get("pre")
            if pre is not None:
                if pre[0].numel() != c_in * nb or pre[1].numel() != pre[0].numel():
                    raise BtsHipError("WgradBatch: pre vectors must have c_in entries")
                d.pre_scale, d.pre_shift, d.pre_relu = pre[0].data_ptr(), pre[1].data_ptr(), int(bool(pr.get("pre_relu", False)))
            d.x, d.dy, d.dw = x2d.data_ptr(), dy2d.data_ptr(), dw.data_ptr()
            descs.append(d)
            where = [(j, (dw.data_ptr() - a) // 4) for j, (a, nbytes) in enumerate(ranges) if a <= dw.data_ptr() < a + nbytes]
            if not where:
                raise BtsHipError("WgradBatch: a dw view lies outside every base")
            self._dw.append((where[0][0], where[0][1], shape))
            self.flops += 2.0 * B * H * W * c_out * c_in * taps * nb
            self.nbytes += 4.0 * (B * h_in * w_in * c_in + B * H * W * c_out + taps * c_out * c_in) * nb
        self.plan, self._table = conv_wgrad_batch_plan_descs(descs, ranges, self.ws_floats, with_table=True)
        self.ws_used = sum(p[2] * int(torch.Size(sh).numel()) for p, (_, _, sh) in zip(self.plan, self._dw) if p[2] > 1)
        self._table_dev = None
        if self.n:
            self._table_dev = torch.frombuffer(self._table, dtype=torch.uint8).to(self.device)      # the one upload

    def run(self, bases: Sequence[torch.Tensor], ws: Optional[torch.Tensor], precision=None) -> List[torch.Tensor]:
        """``precision`` "bf16": the same table on bts_conv_wgrad_batch_bf16_f32 (bf16 operands, fp32 accumulation)."""
        pr = wgrad_precision(precision, "WgradBatch.run")
        if len(bases) != len(self.base_numel):
            raise BtsHipError("WgradBatch.run: %d bases, planned with %d" % (len(bases), len(self.base_numel)))
        if self.n == 0:
            return []
        for b, numel in zip(bases, self.base_numel):
            _need(b, "WgradBatch.run")
            if b.numel() < numel or not b.is_contiguous() or b.device != self.device:
                raise BtsHipError("WgradBatch.run: a base is smaller than the one the batch was planned with, not contiguous or on another device")
        if self.ws_used:
            _need(ws, "WgradBatch.run")
            if ws.numel() < self.ws_used or not ws.is_contiguous() or ws.device != self.device:
                raise BtsHipError("WgradBatch.run: the workspace must hold %d floats" % self.ws_used)
        bp = (C.c_void_p * len(bases))(*[b.data_ptr() for b in bases])
        name, kern = (("bts_conv_wgrad_batch_bf16_f32", "conv_wgrad_batch_kernel<bf16>") if pr == 2 else
                      ("bts_conv_wgrad_batch_f32", "conv_wgrad_batch_kernel"))
        _enqueue(name, bases[0], (self._table, self._table_dev.data_ptr(), self.n, bp, len(bases), _ptr(ws)),
                 trace=(kern, self.tag, self.flops, self.nbytes, None))
        return [bases[j].view(-1)[off:off + int(torch.Size(sh).numel())].view(sh) for j, off, sh in self._dw]


# ------------------------------------------------------------------------------ train-mode BN
def bn_train_ws_floats(npix: int, C: int) -> int:
    return int(_lib.load_real().bts_bn_train_ws_floats(npix, C))


def bn_train_stats(x2d: torch.Tensor, C: int, gamma, beta, eps: float, momentum: float, running_mean, running_var,
                   ws: torch.Tensor, out: Optional[torch.Tensor] = None):
    """Batch statistics of NHWC rows (bts_bn_train_stats_f32): returns (mean, invstd, scale, shift), each [C];
    running_mean / running_var (or None) are updated in place.  ``out``: optional [4, C] view (unit channel stride, rows
    16-byte aligned) that receives the four vectors instead of a fresh tensor."""
    xs, xc = _rows2d(x2d, "bn_train_stats")
    if C % 4 or C > xc:
        raise BtsHipError("bn_train_stats: C must be a multiple of 4 within the view (%d/%d)" % (C, xc))
    if out is None:
        out = torch.empty((4, C), dtype=torch.float32, device=x2d.device)
    else:
        _need(out, "bn_train_stats")
        if tuple(out.shape) != (4, C) or out.stride(1) != 1 or out.stride(0) % 4 or out.data_ptr() % 16:
            raise BtsHipError("bn_train_stats: out must be a [4, %d] view with unit channel stride and 16-byte aligned rows" % C)
    _need(ws, "bn_train_stats")
    for v, what in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if v is not None:
            _channel_vec(v, C, "bn_train_stats", what, aligned=False)
    npix = x2d.shape[0]
    _enqueue("bts_bn_train_stats_f32", x2d,
             (x2d.data_ptr(), xs, npix, C, _ptr(gamma), _ptr(beta), float(eps), float(momentum), _ptr(running_mean), _ptr(running_var),
              ws.data_ptr(), ws.numel(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr()),
             trace=("bn_stats_kernel", "bn.stats", 3.0 * npix * C, 4.0 * npix * C, None))
    return out[0], out[1], out[2], out[3]


def bn_apply(x2d: torch.Tensor, C: int, scale: torch.Tensor, shift: torch.Tensor, relu: bool, y2d: torch.Tensor):
    """y = [relu](x*scale + shift) over NHWC rows (bts_bn_apply_nhwc_f32)."""
    npix = x2d.shape[0] if isinstance(x2d, torch.Tensor) and x2d.dim() == 2 else 0
    xs = _rows2d_c(x2d, C, npix, "bn_apply")
    ys = _rows2d_c(y2d, C, npix, "bn_apply")
    _channel_vec(scale, C, "bn_apply", "scale")
    _channel_vec(shift, C, "bn_apply", "shift")
    _enqueue("bts_bn_apply_nhwc_f32", x2d, (x2d.data_ptr(), xs, npix, C, scale.data_ptr(), shift.data_ptr(), int(bool(relu)), y2d.data_ptr(), ys),
             trace=("bn_apply_kernel", "bn.apply", 2.0 * npix * C, 8.0 * npix * C, None))
    return y2d


def bn_train_backward(x2d: torch.Tensor, dy2d: torch.Tensor, C: int, mean, invstd, scale, shift, relu: bool,
                      ws: torch.Tensor, dx2d: Optional[torch.Tensor]):
    """Backward of batch-statistic BN (+ fused ReLU): returns (dgamma, dbeta); dx2d (or None) is filled in place."""
    npix = x2d.shape[0] if isinstance(x2d, torch.Tensor) and x2d.dim() == 2 else 0
    xs = _rows2d_c(x2d, C, npix, "bn_train_backward")
    ds = _rows2d_c(dy2d, C, npix, "bn_train_backward")
    for v, what in ((mean, "mean"), (invstd, "invstd"), (scale, "scale"), (shift, "shift")):
        _channel_vec(v, C, "bn_train_backward", what)
    _need(ws, "bn_train_backward")
    dxs = 0
    if dx2d is not None:
        dxs = _rows2d_c(dx2d, C, npix, "bn_train_backward")
    g = torch.empty((2, C), dtype=torch.float32, device=x2d.device)
    _enqueue("bts_bn_train_bwd_f32", x2d,
             (x2d.data_ptr(), xs, dy2d.data_ptr(), ds, npix, C, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(),
              int(bool(relu)), ws.data_ptr(), ws.numel(), g[0].data_ptr(), g[1].data_ptr(), _ptr(dx2d), dxs),
             trace=("bn_bwd_kernels", "bn.bwd", 10.0 * npix * C, 20.0 * npix * C, None))
    return g[0], g[1]


def bn_frozen_vectors(C: int, gamma, beta, running_mean: torch.Tensor, running_var: torch.Tensor, eps: float,
                      out: Optional[torch.Tensor] = None):
    """The four vectors of a norm layer with frozen statistics (bts_bn_frozen_vectors_f32): returns (mean, invstd, scale,
    shift), each [C], from the running buffers, which are only read.  gamma / beta None = 1 / 0.  ``out``: optional [4, C]
    view (unit channel stride, rows 16-byte aligned) that receives the four vectors instead of a fresh tensor."""
    if not isinstance(C, int) or C <= 0 or C % 4:
        raise BtsHipError("bn_frozen_vectors: C must be a positive multiple of 4, got %r" % (C,))
    for v, what in ((running_mean, "running_mean"), (running_var, "running_var")):
        _channel_vec(v, C, "bn_frozen_vectors", what, aligned=False)
    for v, what in ((gamma, "gamma"), (beta, "beta")):
        if v is not None:
            _channel_vec(v, C, "bn_frozen_vectors", what, aligned=False)
    if out is None:
        out = torch.empty((4, C), dtype=torch.float32, device=running_mean.device)
    else:
        _need(out, "bn_frozen_vectors")
        if tuple(out.shape) != (4, C) or out.stride(1) != 1 or out.stride(0) % 4 or out.data_ptr() % 16:
            raise BtsHipError("bn_frozen_vectors: out must be a [4, %d] view with unit channel stride and 16-byte aligned rows" % C)
    _enqueue("bts_bn_frozen_vectors_f32", running_mean,
             (_ptr(gamma), _ptr(beta), running_mean.data_ptr(), running_var.data_ptr(), float(eps), C,
              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr()),
             trace=("bn_frozen_vectors_kernel", "bn.frozen", 4.0 * C, 32.0 * C, None))
    return out[0], out[1], out[2], out[3]


def bn_frozen_backward(x2d: torch.Tensor, dy2d: torch.Tensor, C: int, mean, invstd, scale, shift, relu: bool,
                       ws: Optional[torch.Tensor], dx2d: Optional[torch.Tensor], sums: bool = True, accumulate: bool = False,
                       out: Optional[torch.Tensor] = None):
    """Backward of a norm layer with frozen statistics (+ fused ReLU), one streaming pass (bts_bn_frozen_bwd_f32):
    dx2d (or None) = scale*dy', added onto dx2d when ``accumulate``; ``sums``: returns (dgamma, dbeta) -- which need ``ws``
    (bn_train_ws_floats) -- else (None, None) and no reduction runs.  ``out``: optional [2, C] view (unit channel stride,
    rows 16-byte aligned) that receives (dgamma, dbeta) instead of a fresh tensor."""
    npix = x2d.shape[0] if isinstance(x2d, torch.Tensor) and x2d.dim() == 2 else 0
    xs = _rows2d_c(x2d, C, npix, "bn_frozen_backward")
    ds = _rows2d_c(dy2d, C, npix, "bn_frozen_backward")
    for v, what in ((mean, "mean"), (invstd, "invstd"), (scale, "scale"), (shift, "shift")):
        _channel_vec(v, C, "bn_frozen_backward", what)
    if not sums and dx2d is None:
        raise BtsHipError("bn_frozen_backward: nothing to compute (no sums and no dx)")
    dxs = 0
    if dx2d is not None:
        dxs = _rows2d_c(dx2d, C, npix, "bn_frozen_backward")
    elif accumulate:
        raise BtsHipError("bn_frozen_backward: accumulate needs dx")
    g = None
    if sums:
        _need(ws, "bn_frozen_backward")
        if ws.numel() < bn_train_ws_floats(npix, C) or not ws.is_contiguous():
            raise BtsHipError("bn_frozen_backward: the workspace must hold %d floats" % bn_train_ws_floats(npix, C))
        if out is None:
            g = torch.empty((2, C), dtype=torch.float32, device=x2d.device)
        else:
            _need(out, "bn_frozen_backward")
            if tuple(out.shape) != (2, C) or out.stride(1) != 1 or out.stride(0) % 4 or out.data_ptr() % 16:
                raise BtsHipError("bn_frozen_backward: out must be a [2, %d] view with unit channel stride and 16-byte aligned rows" % C)
            g = out
    elif out is not None:
        raise BtsHipError("bn_frozen_backward: out is for the sums")
    nbytes = 4.0 * npix * C * (2 + (dx2d is not None) + bool(accumulate))
    _enqueue("bts_bn_frozen_bwd_f32", x2d,
             (x2d.data_ptr(), xs, dy2d.data_ptr(), ds, npix, C, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(),
              int(bool(relu)), _ptr(ws if sums else None), ws.numel() if sums else 0, _ptr(None if g is None else g[0]),
              _ptr(None if g is None else g[1]), _ptr(dx2d), dxs, int(bool(accumulate))),
             trace=("bn_frozen_bwd_kernel", "bn.frozen_bwd", (6.0 if sums else 2.0) * npix * C, nbytes, None))
    return (g[0], g[1]) if sums else (None, None)


# ------------------------------------------------------------------------------ tail
def pack_planes(planes: Sequence[torch.Tensor], dst2d: torch.Tensor):
    """Interleave 1-channel maps ([B,1,H,W] contiguous each) into dst2d [npix, n] (an NHWC slice)."""
    stride, n = _rows2d(dst2d, "pack_planes")
    if n != len(planes) or not 1 <= n <= 4:
        raise BtsHipError("pack_planes: need 1..4 planes matching the destination slice")
    npix = dst2d.shape[0]
    ptrs = [_ptr(p) for p in _dense_planes(planes, npix, "pack_planes")] + [C.c_void_p(0)] * (4 - n)
    _enqueue("bts_pack_planes_f32", dst2d, (ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, npix, _ptr(dst2d), stride))
    return dst2d


def get_depth_forward(iconv1: torch.Tensor, weight: torch.Tensor, max_depth: float,
                      focal: Optional[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """get_depth + scaling (reference bts.py:289-291): iconv1 [B,C,H,W] NCHW -> final_depth [B,1,H,W]."""
    _need(iconv1, "get_depth_forward")
    _need(weight, "get_depth_forward")
    B, Cc, H, W = iconv1.shape
    if not iconv1.is_contiguous() or tuple(weight.shape) != (1, Cc, 3, 3) or not weight.is_contiguous():
        raise BtsHipError("get_depth_forward: need contiguous iconv1 [B,C,H,W] and weight [1,C,3,3]")
    if focal is not None:
        _need(focal, "get_depth_forward")
        if focal.numel() != B or not focal.is_contiguous():
            raise BtsHipError("get_depth_forward: focal must be [B]")
    if out is None:
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=iconv1.device)
    elif tuple(out.shape) != (B, 1, H, W) or not out.is_contiguous():
        raise BtsHipError("get_depth_forward: out must be contiguous [B,1,H,W]")
    _enqueue("bts_get_depth_f32", iconv1, (_ptr(iconv1), _ptr(weight), B, Cc, H, W, float(max_depth), _ptr(focal), _ptr(out)),
             trace=("get_depth_kernel<%d>" % Cc, "get_depth", 2.0 * 9 * Cc * B * H * W, 4.0 * (Cc + 1) * B * H * W, None))
    return out


# --------------------------------------------------------------------------- pooling
def maxpool3x3s2(src2d: torch.Tensor, B: int, h: int, w: int, dst2d: torch.Tensor, dst2_2d: Optional[torch.Tensor] = None):
    ss, Cc = _rows2d(src2d, "maxpool3x3s2")
    ds, dc = _rows2d(dst2d, "maxpool3x3s2")
    ho, wo = (h + 1) // 2, (w + 1) // 2
    if dc != Cc or src2d.shape[0] != B * h * w or dst2d.shape[0] != B * ho * wo:
        raise BtsHipError("maxpool3x3s2: shape mismatch")
    d2p, d2s = C.c_void_p(0), 0
    if dst2_2d is not None:
        d2s, d2c = _rows2d(dst2_2d, "maxpool3x3s2")
        if d2c != Cc or dst2_2d.shape[0] != B * ho * wo:
            raise BtsHipError("maxpool3x3s2: second destination mismatch")
        d2p = _ptr(dst2_2d)
    nbytes = 4.0 * Cc * (B * h * w + B * ho * wo * (2 if dst2_2d is not None else 1))
    _enqueue("bts_maxpool3x3s2_nhwc_f32", src2d, (_ptr(src2d), ss, B, h, w, Cc, _ptr(dst2d), ds, d2p, d2s),
             trace=("maxpool3x3s2_kernel", "encoder_pool", 0.0, nbytes, None))
    return dst2d


def bn_relu_avgpool2(src2d: torch.Tensor, B: int, h: int, w: int, scale: torch.Tensor, shift: torch.Tensor,
                     dst2d: torch.Tensor):
    ss, Cc = _rows2d(src2d, "bn_relu_avgpool2")
    ds, dc = _rows2d(dst2d, "bn_relu_avgpool2")
    _need(scale, "bn_relu_avgpool2")
    _need(shift, "bn_relu_avgpool2")
    if dc != Cc or src2d.shape[0] != B * h * w or dst2d.shape[0] != B * (h // 2) * (w // 2) or scale.numel() != Cc:
        raise BtsHipError("bn_relu_avgpool2: shape mismatch")
    nbytes = 4.0 * Cc * (B * h * w + B * (h // 2) * (w // 2))
    _enqueue("bts_bn_relu_avgpool2_nhwc_f32", src2d, (_ptr(src2d), ss, B, h, w, Cc, _ptr(scale), _ptr(shift), _ptr(dst2d), ds),
             trace=("bn_relu_avgpool2_kernel", "encoder_pool", 0.0, nbytes, None))
    return dst2d
