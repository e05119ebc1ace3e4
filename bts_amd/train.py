"""Training-step graph of the BTS decoder (reference: bts.forward in train() mode,
pytorch/bts.py:223-293, driven by bts_main.py:476-500).

Every convolution of the path -- forward, input gradient and weight gradient -- runs on the hand-written gfx950
kernels of libbts_hip.so:

* forward      : bts_conv_fwd_f32 (the inference kernel, plain epilogue),
* input grad   : the same kernel on the output gradient with flipped/transposed weights
                 (a stride-1 convolution's adjoint is a convolution: pad' = dil*(k-1) - pad),
* weight grad  : bts_conv_wgrad_f32 (K = pixels GEMM with a deterministic split over pixels),
* LPG          : bts_lpg_fwd_f32 / bts_lpg_bwd_f32 through ops.LpgFunction.

What is cheap and memory-bound (batch-statistic BN, ELU/ReLU/sigmoid, sin/cos of the plane parameters, concat,
normalize) stays on PyTorch-ROCm's precompiled elementwise/reduction kernels, kept in channels_last so the HIP
convolutions read and write them in place as NHWC.  MIOpen is bypassed (no gfx950 find-db in this image).

There is no CPU path here: non-CUDA tensors raise.
"""
from __future__ import annotations

import contextlib
import threading
import weakref
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from . import ops
from ._lib import BtsHipError

FUSED_DENSE_BLOCKS = True          # DenseNet blocks as one in-place autograd node (False: layer-by-layer graph with torch.cat)
_WS: Dict[Tuple[str, int], torch.Tensor] = {}
WGRAD_WS_FLOATS = 48 << 20        # 192 MB of split-K partials per (device, stream)


def _workspace(device: torch.device) -> torch.Tensor:
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = torch.empty(WGRAD_WS_FLOATS, dtype=torch.float32, device=device)
    return ws


_SPLITK_WS: Dict[Tuple[str, int], torch.Tensor] = {}
SPLITK_WS_FLOATS = 16 << 20       # 64 MB: lets the forward / input-gradient launches of the deep, pixel-starved layers
                                  # split K (bts_conv_desc.splitk_ws); larger layers never split


def _splitk_workspace(device: torch.device) -> torch.Tensor:
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = _SPLITK_WS[key] = torch.empty(SPLITK_WS_FLOATS, dtype=torch.float32, device=device)
    return ws


_nhwc_rows = ops.nhwc_rows


class WeightPacker:
    """Packed copies of the convolution weights for the training step.

    The optimiser rewrites the OIHW parameters every iteration; the HIP kernels want them as [c_out_pad][k_pad]
    (forward) and as the same layout of the flipped, transposed kernel (input gradient).  Entries are registered on
    first use; ``refresh()`` -- called at the top of each training forward -- re-packs every entry whose parameter
    changed (``Tensor._version``) in ONE launch of bts_pack_weights_f32.  A stale entry met later is re-packed on the
    spot, so correctness never depends on ``refresh`` having been called.

    ``versions_trusted``: whether ``Tensor._version`` tells, right now, which parameters changed.  False by default (torch's
    fused optimisers rewrite the parameters without bumping it: begin_step() then re-packs everything); whoever stepped
    last decides -- ``optim.NativeAdamW.step`` bumps every version it touches, re-packs the entries it can itself and sets
    it True, the post-step hook of ``trainer.make_optimizer`` on a torch optimiser sets it False.  ``epoch`` counts changes
    of the entry set (the native optimiser rebuilds its table when it moves)."""

    FWD, DGRAD = 0, 1
    FWD_NATIVE, DGRAD_NATIVE = 2, 3    # grouped weights in the 144 c-float layout of bts_conv_grouped_fwd_f32 (pack.hip gmode 3 / 4)

    def __init__(self):
        self.entries = {}          # (data_ptr, shape, c_in_ld, mode, groups) -> dict(wref, dst, version, rows)
        self._table = None
        self._table_key = None
        self.versions_trusted = False
        self.epoch = 0

    @staticmethod
    def bundle_channels(weight, groups):
        """Channels per bundle for a grouped weight [C, C/groups, k, k]: consecutive groups packed block-diagonally
        into bundles of max(32, C/groups) channels (ops.pack_grouped_conv_weight uses the same rule)."""
        c, cg = weight.shape[0], weight.shape[1]
        cb = max(32, cg)
        if groups * cg != c or cb % cg or c % cb or cb % 32:
            raise BtsHipError("train.conv2d: grouped convolution %s with %d groups is not built" % (tuple(weight.shape), groups))
        return cb

    @staticmethod
    def _rows(weight, c_in_ld, mode, groups):
        """Table rows (without pointers) + destination shape for one weight: one row for a dense convolution, one per
        channel bundle for a grouped one.  Row = (src offset, dst offset, rows, inner, k, c_in_ld, rows_pad, k_pad,
        s_row, s_c, flip, cg, gmode)."""
        cout, cin_g, k, _ = weight.shape
        kk = k * k
        if mode in (WeightPacker.FWD_NATIVE, WeightPacker.DGRAD_NATIVE):
            if k != 3 or not ops.grouped_native_supported(cout, groups) or cin_g * groups != cout:
                raise BtsHipError("train.conv2d: grouped convolution %s with %d groups has no native pack" % (tuple(weight.shape), groups))
            gmode = 3 if mode == WeightPacker.FWD_NATIVE else 4
            return [(0, 0, 144, 0, 3, 0, 144, cout, 0, 0, 0, cin_g, gmode)], (144 * cout,)
        if groups == 1:
            if mode == WeightPacker.FWD:
                rows, inner, s_row, s_c, flip = cout, cin_g, cin_g * kk, kk, 0
            else:
                rows, inner, s_row, s_c, flip = cin_g, cout, kk, cin_g * kk, 1
            rows_pad, k_pad = ops.round_up(rows, 32), ops.round_up(kk * c_in_ld, 32)
            return [(0, 0, rows, inner, k, c_in_ld, rows_pad, k_pad, s_row, s_c, flip, 0, 0)], (rows_pad, k_pad)
        cb = WeightPacker.bundle_channels(weight, groups)
        if c_in_ld != cb:
            raise BtsHipError("train.conv2d: grouped convolutions are packed with c_in_ld = bundle width")
        nb, k_pad = cout // cb, kk * cb
        if mode == WeightPacker.FWD:
            s_row, s_c, flip, gmode = cin_g * kk, kk, 0, 1
        else:
            s_row, s_c, flip, gmode = kk, cin_g * kk, 1, 2
        rows = [(j * cb * cin_g * kk, j * cb * k_pad, cb, cb, k, cb, cb, k_pad, s_row, s_c, flip, cin_g, gmode)
                for j in range(nb)]
        return rows, (nb, cb, k_pad)

    def _table_for(self, items):
        import numpy as np
        from . import _lib
        lib = _lib.load_real()
        table, first = [], 0
        for e in items:
            src, dst = e["ptr"], e["dst"].data_ptr()
            for (so, do, rows, inner, k, cld, rows_pad, k_pad, s_row, s_c, flip, cg, gmode) in e["rows"]:
                table.append([src + 4 * so, dst + 4 * do, rows, inner, k, cld, rows_pad, k_pad, s_row, s_c, flip, first,
                              cg, gmode])
                first += int(lib.bts_pack_weights_blocks(rows_pad, k_pad))
        return torch.from_numpy(np.asarray(table, dtype=np.int64)).to(items[0]["dst"].device), first, len(table)

    def _launch(self, items, table, blocks, n_rows):
        ops._enqueue("bts_pack_weights_f32", items[0]["dst"], (table.data_ptr(), n_rows, blocks),
                     trace=("pack_weights_kernel", "pack", 0.0, 0.0, None))
        for e in items:
            e["version"] = e["wref"]()._version
            # derived forms cached on the packed buffer (Winograd U, bf16 planes: ops.conv_forward) are now stale
            e["dst"]._bts_pack_seq = getattr(e["dst"], "_bts_pack_seq", 0) + 1

    def get(self, weight, c_in_ld, mode, groups=1):
        """Packed buffer for ``weight`` (an nn.Parameter or any contiguous OIHW CUDA tensor), current with its values:
        [rows_pad, k_pad] for a dense convolution, [n_bundles, cb, k_pad] for a grouped one, 144 * c floats for the native
        grouped modes (``c_in_ld`` is then only part of the key)."""
        key = (weight.data_ptr(), tuple(weight.shape), c_in_ld, mode, groups)
        e = self.entries.get(key)
        if e is not None and e["wref"]() is None:          # the tensor this entry was packed from is gone: the address
            e = None                                        # now belongs to someone else's values
        if e is None:
            if not weight.is_contiguous():
                raise BtsHipError("train.conv2d: weight must be contiguous OIHW")
            rows, shape = self._rows(weight, c_in_ld, mode, groups)
            e = self.entries[key] = dict(wref=weakref.ref(weight), ptr=weight.data_ptr(), rows=rows, version=-1,
                                         dst=torch.empty(shape, dtype=torch.float32, device=weight.device))
            self._table_key = None
            self.epoch += 1
        if e["version"] != e["wref"]()._version:
            table, blocks, n_rows = self._table_for([e])
            self._launch([e], table, blocks, n_rows)
        return e["dst"]

    def refresh(self, force: bool = False):
        """Re-pack every registered weight whose parameter changed since its last packing -- with ``force``: every
        registered weight -- in one launch."""
        # strong references for the duration of the call: a registered weight that is only reachable through a reference
        # cycle (every BtsModel is) can be collected by any allocation below, between this check and the launch
        alive = {k: e["wref"]() for k, e in self.entries.items()}
        dead = [k for k, w in alive.items() if w is None]
        for k in dead:
            del self.entries[k]
        if dead:
            self.epoch += 1
        stale = [e for k, e in self.entries.items() if force or e["version"] != alive[k]._version]
        if not stale:
            return
        key = tuple(id(e) for e in stale)
        if self._table_key != key:                        # the usual case after step 1: the same full set every step
            self._table, self._table_blocks, self._table_rows = self._table_for(stale)
            self._table_key = key
        self._launch(stale, self._table, self._table_blocks, self._table_rows)


_PACKER = WeightPacker()


class UpconvPacker:
    """The two per-step packs of every upconv weight on the sub-pixel training path (decoder.subpixel_upconv_train):
    the four pre-summed 2x2 class filters the forward reads (ops.pack_upconv_subpixel's layout and bits) and the 4x4 /
    stride-2 kernel of the input gradient (ops.pack_upconv_dgrad_reference).  Weights are registered on first use and
    packed on the spot.  Every ``begin_step()`` ages the whole set (``invalidate()``), and the first upconv of the step
    then re-packs ALL registered weights from the OIHW parameters in ONE launch of bts_upconv_train_pack_f32
    (``refresh()``), whatever ``Tensor._version`` or ``WeightPacker.versions_trusted`` say: the packs are current after
    torch's fused optimisers and after ``optim.NativeAdamW`` alike, and a step that runs no sub-pixel upconv (the switch
    off) launches nothing.  Every refill bumps ``_bts_pack_seq`` on the buffers, so the forms ops.conv_forward derives
    from them (the bf16x3 planes) are re-made."""

    def __init__(self):
        self.entries = {}          # (data_ptr, shape) -> dict(wref, ptr, fwd, dgrad, version)
        self._table = None
        self._table_key = None
        self._aged = False

    def invalidate(self):
        """A new step began: nothing packed before it may be used again."""
        self._aged = True

    @staticmethod
    def _stamp(items):
        for e in items:
            e["version"] = e["wref"]()._version
            for buf in (e["fwd"], e["dgrad"]):
                buf._bts_pack_seq = getattr(buf, "_bts_pack_seq", 0) + 1

    def get(self, weight):
        """(forward pack [4, c_out_pad, k_pad], input-gradient pack [c_in_pad, k_pad']) of ``weight``."""
        if self._aged:
            self.refresh()
        key = (weight.data_ptr(), tuple(weight.shape))
        e = self.entries.get(key)
        if e is not None and e["wref"]() is None:          # the address now belongs to someone else's values
            e = None
        if e is None:
            if not weight.is_contiguous():
                raise BtsHipError("train.upconv: weight must be contiguous OIHW")
            fs, ds = ops.upconv_train_pack_shapes(weight.shape[0], weight.shape[1])
            e = self.entries[key] = dict(wref=weakref.ref(weight), ptr=weight.data_ptr(), version=-1,
                                         fwd=torch.empty(fs, dtype=torch.float32, device=weight.device),
                                         dgrad=torch.empty(ds, dtype=torch.float32, device=weight.device))
            self._table_key = None
        if e["version"] != weight._version:                # new, or rewritten in the open since the last begin_step()
            ops.upconv_train_pack([weight.detach()], [e["fwd"]], [e["dgrad"]])
            self._stamp([e])
        return e["fwd"], e["dgrad"]

    def refresh(self):
        """Re-pack every registered weight, changed or not, in one launch per device."""
        self._aged = False
        alive = {k: e["wref"]() for k, e in self.entries.items()}     # strong references for the duration of the call
        for k in [k for k, w in alive.items() if w is None]:
            del self.entries[k]
            self._table_key = None
        if not self.entries:
            return
        items = list(self.entries.values())
        key = tuple(id(e) for e in items)
        if self._table_key != key:
            self._table, self._table_key = {}, key
        by_dev = {}
        for k, e in self.entries.items():
            by_dev.setdefault(str(e["fwd"].device), []).append((alive[k], e))
        for dev, pairs in by_dev.items():
            ws = [w.detach() for w, _ in pairs]
            self._table[dev] = ops.upconv_train_pack(ws, [e["fwd"] for _, e in pairs], [e["dgrad"] for _, e in pairs],
                                                     table=self._table.get(dev))
        self._stamp(items)


_UPCONV_PACKER = UpconvPacker()


def begin_step():
    """Top of a training forward: bring all packed weights up to date with one launch.

    Every registered weight is re-packed, changed or not: ``Tensor._version`` is NOT a reliable change signal in a
    training loop -- torch's fused optimisers (``AdamW(fused=True)``, ``_fused_adamw_``) rewrite the parameters without
    bumping it -- and in steady state the optimiser has touched every weight anyway (one 0.5 ms launch per step).  For
    the same reason a training forward also ages the eval-mode packs and recorded graphs/plans of every model
    (``workspace.invalidate_packs``): the next eval forward re-packs from the current values.

    The exception is ``WeightPacker.versions_trusted``: after a step of ``optim.NativeAdamW`` the versions ARE the change
    signal and the entries it re-packed itself are current, so only what is stale by version goes into the pack launch
    (frozen weights are not touched; often nothing is launched at all).

    The sub-pixel upconv packs (``UpconvPacker``, decoder.subpixel_upconv_train) are never part of that bargain: every
    step ages them all, and the step's first sub-pixel upconv re-packs them from the parameters in one launch."""
    if _STEP_DEPTH[0] > 0:                 # inside model_step(): the model's forward already did this
        return
    from . import workspace
    workspace.invalidate_packs()
    _PACKER.refresh(force=not _PACKER.versions_trusted)
    _UPCONV_PACKER.invalidate()


_STEP_DEPTH = [0]


class model_step:
    """``with train.model_step():`` around a whole-model training forward: one begin_step() for encoder + decoder."""

    def __enter__(self):
        begin_step()
        _STEP_DEPTH[0] += 1

    def __exit__(self, *exc):
        _STEP_DEPTH[0] -= 1
        return False


def refuse_bf16(where: str) -> None:
    """The training path computes in fp32 (or its bf16x3 emulation) only: bf16 operands (precision 2) are an inference
    mode, and a gradient taken through them would be a different function's."""
    if ops.current_launch_config()[1] == 2:
        raise BtsHipError("%s: conv_precision 'bf16' is an inference mode; training runs in 'fp32' or 'bf16x3'" % where)


# ---- train_precision: bf16 operands in all three passes of the training step (opt-in) -----------------------
# ``BtsModel.train_precision = "bf16"`` (forwarded to encoder.train_precision and bts.train_precision) is a switch of its
# own, not a value of conv_precision: a train-mode forward under conv_precision "bf16" still raises (refuse_bf16).  The
# encoder / decoder training forwards open ``precision_scope`` around themselves; every autograd node reads the value in
# force ONCE, in its forward, records what it ran in its ctx and applies that explicitly in backward -- autograd runs
# backward on another thread, where neither this scope nor the model's launch_config is in force.
TRAIN_PRECISIONS = {"fp32": 0, "bf16": 2}
_tp_tls = threading.local()


def check_train_precision(value, who: str = "train_precision") -> str:
    if not isinstance(value, str) or value not in TRAIN_PRECISIONS:
        raise BtsHipError("%s must be 'fp32' or 'bf16', got %r" % (who, value))
    return value


def current_train_precision() -> int:
    """0 (fp32) or 2 (bf16 operands, fp32 accumulation): what a node whose forward runs now on this thread takes."""
    return getattr(_tp_tls, "value", 0)


class precision_scope:
    """``with train.precision_scope("bf16"):`` around a training forward (this thread only).  Only a grad-enabled forward
    reads the switch; "bf16" needs the launch precision "fp32" -- with conv_precision "bf16x3" (or "bf16", which training
    refuses anyway) it raises; $BTS_CONV_PRECISION=1 keeps its precedence: the whole step then runs emulated, as ever."""

    def __init__(self, value):
        self._new = TRAIN_PRECISIONS[check_train_precision(value)]

    def __enter__(self):
        self._prev = getattr(_tp_tls, "value", None)
        new = self._new if torch.is_grad_enabled() and not ops._ENV_PRECISION else 0
        if new == 2 and ops.current_launch_config()[1] != 0:
            raise BtsHipError("train_precision 'bf16' needs conv_precision 'fp32' (the launch precision in force is %r)"
                              % (ops.current_launch_config()[1],))
        _tp_tls.value = new
        return self

    def __exit__(self, *exc):
        if self._prev is None:
            del _tp_tls.value
        else:
            _tp_tls.value = self._prev
        return False


# ---- native_frozen_norm: norm layers with frozen statistics on the HIP kernels (opt-in) ----------------------
# ``BtsModel.native_frozen_norm = True`` (forwarded to encoder.native_frozen_norm and bts.native_frozen_norm): an eval()-mode
# BatchNorm2d inside the train()-mode model (bts_main.py --bn_no_track_stats -> bn_init_as_tf) runs on bn_frozen_vectors /
# bn_apply / bn_frozen_backward instead of ATen, and a dense block with such layers keeps its fused node.  Read once per
# node, in its forward, like the train precision.
_fn_tls = threading.local()


def current_frozen_norm() -> bool:
    """Whether a node whose forward runs now on this thread takes frozen norm layers on the HIP kernels."""
    return getattr(_fn_tls, "value", False)


class frozen_norm_scope:
    """``with train.frozen_norm_scope(True):`` around a training forward (this thread only)."""

    def __init__(self, on):
        self._new = bool(on)

    def __enter__(self):
        self._prev = getattr(_fn_tls, "value", None)
        _fn_tls.value = self._new
        return self

    def __exit__(self, *exc):
        if self._prev is None:
            del _fn_tls.value
        else:
            _fn_tls.value = self._prev
        return False


def _launch_precision(pr: int):
    """The launch_config scope of a node's convolution launches: precision 2 where the node recorded it, else whatever is in
    force (the fp32 / bf16x3 behaviour of before)."""
    return ops.launch_config(precision=2) if pr == 2 else contextlib.nullcontext()


class _ConvFn(torch.autograd.Function):
    """y = conv2d(nearest_up(x, up), w, stride, padding, dilation, groups), bias-free, on libbts_hip.so."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, dilation, up, tag, groups, act=ops.ACT_NONE, grouped_native=False, bf16=True):
        refuse_bf16("train.conv2d")
        ops._need(x, "train.conv2d")
        ops._need(weight, "train.conv2d")
        B, C, h, w = x.shape
        cout, cin_g, k, k2 = weight.shape
        if cin_g * groups != C or k != k2:
            raise BtsHipError("train.conv2d: weight %s (groups %d) does not fit input %s"
                              % (tuple(weight.shape), groups, tuple(x.shape)))
        x2d, c4 = _nhwc_rows(x.detach())
        H, W = ops.conv_out_hw(h, w, k, dilation, stride, padding, up)
        y = torch.empty((B, H, W, cout), dtype=torch.float32, device=x.device)
        if act not in (ops.ACT_NONE, ops.ACT_ELU):
            raise BtsHipError("train.conv2d: only ELU can ride in the epilogue (its derivative is a function of y)")
        native = False
        if groups > 1:
            if up != 1 or cout != C or act != ops.ACT_NONE:
                raise BtsHipError("train.conv2d: grouped convolutions need cin == cout, no upsample, no activation")
            native = _grouped_native_layer(grouped_native, C, groups, k, stride, padding, dilation)
        # train_precision "bf16": every layer but the ones the caller keeps in fp32 (``bf16=False``), the 3-channel stem and
        # the native grouped kernels (their weight gradient is fp32: the layer stays fp32 in all three passes)
        pr = 2 if current_train_precision() == 2 and bf16 and C > 4 and not native else 0
        with _launch_precision(pr):
            if native:
                wp = _PACKER.get(weight, 0, WeightPacker.FWD_NATIVE, groups)
                ops.conv_grouped_forward(x2d, B, h, w, wp, C, groups, y2d=y.view(B * H * W, cout), tag=tag + ".fwd")
            elif groups > 1:
                cb = WeightPacker.bundle_channels(weight, groups)
                wp = _PACKER.get(weight, cb, WeightPacker.FWD, groups)
                ops.conv_forward(x2d, B, h, w, wp, cb, k, dil=dilation, c_in_ld=cb, y2d=y.view(B * H * W, cout), stride=stride,
                                 pad=padding, tag=tag + ".fwd", c_in_real=cin_g, n_bundles=C // cb)
            else:
                wp = _PACKER.get(weight, c4, WeightPacker.FWD)
                ops.conv_forward(x2d, B, h, w, wp, cout, k, dil=dilation, up=up, c_in_ld=c4, y2d=y.view(B * H * W, cout),
                                 stride=stride, pad=padding, tag=tag + ".fwd", c_in_real=C, act=act,
                                 splitk_ws=_splitk_workspace(x.device))
        out = y.permute(0, 3, 1, 2)           # [B,cout,H,W] channels_last view
        if act == ops.ACT_ELU:
            ctx.save_for_backward(x2d, out)   # ELU'(v) = 1 (y > 0) or y + 1: the pre-activation is never stored
        else:
            ctx.save_for_backward(x2d)
        ctx.weight = weight                   # the caller's parameter object: the packer tracks it by identity/version
        ctx.geom = (B, C, h, w, c4, cout, k, stride, padding, dilation, up, H, W, tag, groups)
        ctx.act = act
        ctx.grouped_native = native           # decided once, in forward: all three passes of a layer take the same form
        ctx.precision = pr                    # likewise the arithmetic: backward runs on another thread, outside every scope
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x2d = ctx.saved_tensors[0]
        weight = ctx.weight
        B, C, h, w, c4, cout, k, stride, padding, dilation, up, H, W, tag, groups = ctx.geom
        if ctx.act == ops.ACT_ELU:
            grad_out = torch.ops.aten.elu_backward(grad_out, 1.0, 1.0, 1.0, True, ctx.saved_tensors[1])
        dy2d, co4 = _nhwc_rows(grad_out)
        dev = grad_out.device
        dx = dw = None
        if ctx.needs_input_grad[0]:
            pad_t = dilation * (k - 1) - padding
            if stride not in (1, 2) or pad_t < 0 or (stride == 2 and up != 1):
                raise BtsHipError("train.conv2d: input gradient is built for stride 1 or 2 with padding <= "
                                  "dilation*(k-1); got stride %d padding %d" % (stride, padding))
            Hs, Ws = h * up, w * up
            g2d, gh, gw = dy2d, H, W
            if stride == 2:
                # adjoint of the stride: the gradient sits on the even positions of a zero map of the input's size, and
                # the stride-1 adjoint below runs on that (4x the FLOPs of the handful of strided layers, exact)
                u = torch.zeros((B, Hs, Ws, co4), dtype=torch.float32, device=dev)
                u[:, 0:2 * H:2, 0:2 * W:2] = (dy2d.view(B, H, W, co4) if dy2d.is_contiguous()
                                              else grad_out.permute(0, 2, 3, 1))      # a strided view has co4 == cout
                g2d, gh, gw = u.view(B * Hs * Ws, co4), Hs, Ws
            dxu = torch.empty((B, Hs, Ws, C), dtype=torch.float32, device=dev)
            with _launch_precision(ctx.precision):   # bf16: dy' and the flipped weights both rounded, the forward's kernels
                if ctx.grouped_native:      # the adjoint is the same operator with flipped taps and transposed groups
                    wp = _PACKER.get(weight, 0, WeightPacker.DGRAD_NATIVE, groups)
                    ops.conv_grouped_forward(g2d, B, gh, gw, wp, C, groups, y2d=dxu.view(B * Hs * Ws, C), tag=tag + ".dgrad")
                elif groups > 1:
                    cb = WeightPacker.bundle_channels(weight, groups)
                    wp = _PACKER.get(weight, cb, WeightPacker.DGRAD, groups)
                    ops.conv_forward(g2d, B, gh, gw, wp, cb, k, dil=dilation, c_in_ld=cb, y2d=dxu.view(B * Hs * Ws, C),
                                     pad=pad_t, tag=tag + ".dgrad", c_in_real=weight.shape[1], n_bundles=C // cb)
                else:
                    wp = _PACKER.get(weight, co4, WeightPacker.DGRAD)        # flipped, transposed kernel [cin][taps*co4]
                    ops.conv_forward(g2d, B, gh, gw, wp, C, k, dil=dilation, c_in_ld=co4, y2d=dxu.view(B * Hs * Ws, C),
                                     pad=pad_t, tag=tag + ".dgrad", c_in_real=cout, splitk_ws=_splitk_workspace(dev))
            if up == 2:                                                 # adjoint of the nearest-2x upsample
                dxu = dxu.view(B, h, 2, w, 2, C).sum(dim=(2, 4))
            dx = dxu.permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            if ctx.grouped_native:          # written in the parameter's own OIHW layout: no dense block, no gather
                dw = ops.conv_grouped_wgrad(x2d, B, h, w, dy2d, C, groups, ws=_workspace(dev), tag=tag + ".wgrad")
            elif groups > 1:
                cb = WeightPacker.bundle_channels(weight, groups)
                cg, nb = weight.shape[1], C // cb
                gpb = cb // cg
                g = ops.conv_wgrad(x2d, B, h, w, cb, dy2d, cb, k, dil=dilation, stride=stride, pad=padding, ws=_workspace(dev),
                                   tag=tag + ".wgrad", n_bundles=nb, precision=ctx.precision)   # [nb, cb, taps, cb] dense blocks
                g6 = g.view(nb, gpb, cg, k * k, gpb, cg)
                idx = torch.arange(gpb, device=dev)
                diag = g6[:, idx, :, :, idx, :]                         # [gpb, nb, cg_out, taps, cg_in]: each group's own block
                dw = diag.permute(1, 0, 2, 4, 3).reshape(cout, cg, k, k).contiguous()
            else:
                g = ops.conv_wgrad(x2d, B, h, w, c4, dy2d, co4, k, dil=dilation, stride=stride, pad=padding, up=up,
                                   ws=_workspace(dev), tag=tag + ".wgrad", precision=ctx.precision)
                dw = g[:cout, :, :C].reshape(cout, k, k, C).permute(0, 3, 1, 2).contiguous()   # OIHW, the layout DDP buckets expect
        return dx, dw, None, None, None, None, None, None, None, None, None


def _grouped_native_layer(asked, c, groups, k, stride, padding, dilation) -> bool:
    """Does a grouped layer take the native entry points (bts_conv_grouped_fwd_f32 / bts_conv_grouped_wgrad_f32) in all three
    passes?  Asked for, fp32 launch precision (bf16x3 stays on bundles silently, as the inference switch does for bf16) and
    a shape rule only: stride 1, 3x3, padding = dilation = 1, c % 64 == 0, 4 / 8 / 16 channels per group."""
    return bool(asked) and ops.current_launch_config()[1] == 0 and stride == 1 and k == 3 and padding == 1 and dilation == 1 \
        and ops.grouped_native_supported(c, groups)


def conv2d(x: torch.Tensor, weight: torch.Tensor, padding: int = 0, dilation: int = 1, stride: int = 1,
           up: int = 1, tag: str = "conv", groups: int = 1, act: int = ops.ACT_NONE, grouped_native: bool = False,
           bf16: bool = True) -> torch.Tensor:
    """Differentiable bias-free convolution on the HIP kernels; ``up=2`` folds a nearest-2x upsample of ``x`` into
    the gather (reference upconv, bts.py:90-92); ``groups`` > 1: ResNeXt's grouped 3x3 as channel bundles, or, with
    ``grouped_native`` on the layers _grouped_native_layer names, on the native grouped kernels in all three passes;
    ``act=ops.ACT_ELU``: the ELU that follows every decoder convolution (bts.py:93, 183-221) applied in the epilogue.
    ``bf16=False``: a layer that stays fp32 under train_precision "bf16" (precision_scope); the 3-channel stem and the
    native grouped layers stay fp32 whatever it says.
    Returns a channels_last [B,c_out,H,W] tensor."""
    return _ConvFn.apply(x, weight, stride, padding, dilation, up, tag, groups, act, grouped_native, bf16)


_BN_WS: Dict[Tuple[str, int], torch.Tensor] = {}


def _bn_workspace(device: torch.device, floats: int) -> torch.Tensor:
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _BN_WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = _BN_WS[key] = torch.empty(max(floats, 1 << 20), dtype=torch.float32, device=device)
    return ws


_PENDING_COUNTS: Dict[int, torch.Tensor] = {}
_DEFER_DEPTH = [0]


def _count_batch(bn):
    """``num_batches_tracked += 1`` (nn.BatchNorm2d.forward in train() mode).  Inside an encoder / decoder forward
    (``_deferred_batch_counts``) the ~175 one-element kernels of a step are collected into one multi-tensor add issued
    when the forward returns; a norm layer run on its own counts immediately."""
    t = bn.num_batches_tracked
    if _DEFER_DEPTH[0] == 0:
        t.add_(1)
        return
    if id(t) in _PENDING_COUNTS:          # the same layer twice in one forward: settle the first count now
        flush_batch_counts()
    _PENDING_COUNTS[id(t)] = t


def flush_batch_counts():
    if _PENDING_COUNTS:
        ts = list(_PENDING_COUNTS.values())
        _PENDING_COUNTS.clear()
        with torch.no_grad():
            torch._foreach_add_(ts, 1)


class _deferred_batch_counts:
    def __enter__(self):
        _DEFER_DEPTH[0] += 1

    def __exit__(self, *exc):
        _DEFER_DEPTH[0] -= 1
        if _DEFER_DEPTH[0] == 0:
            flush_batch_counts()
        return False


class _BnFn(torch.autograd.Function):
    """y = [relu](batch_norm(x)) with batch statistics, on libbts_hip.so (bn_train.hip); the module's running
    buffers are updated in place exactly as nn.BatchNorm2d.train() does."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, relu):
        B, C, H, W = x.shape
        x2d, _ = _nhwc_rows(x.detach())
        npix = B * H * W
        ws = _bn_workspace(x.device, ops.bn_train_ws_floats(npix, C))
        track = bn.track_running_stats and bn.running_mean is not None
        mean, invstd, scale, shift = ops.bn_train_stats(
            x2d, C, None if gamma is None else gamma.detach(), None if beta is None else beta.detach(), bn.eps,
            bn.momentum, bn.running_mean if track else None, bn.running_var if track else None, ws)
        if track and bn.num_batches_tracked is not None:
            _count_batch(bn)
        y = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
        ops.bn_apply(x2d, C, scale, shift, relu, y.view(npix, C))
        ctx.save_for_backward(x2d, mean, invstd, scale, shift)
        ctx.meta = (B, C, H, W, relu, gamma is not None)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        x2d, mean, invstd, scale, shift = ctx.saved_tensors
        B, C, H, W, relu, affine = ctx.meta
        dy2d, _ = _nhwc_rows(grad_out)
        npix = B * H * W
        dx = torch.empty((B, H, W, C), dtype=torch.float32, device=grad_out.device) if ctx.needs_input_grad[0] else None
        ws = _bn_workspace(grad_out.device, ops.bn_train_ws_floats(npix, C))
        dgamma, dbeta = ops.bn_train_backward(x2d, dy2d, C, mean, invstd, scale, shift, relu, ws,
                                              None if dx is None else dx.view(npix, C))
        return (None if dx is None else dx.permute(0, 3, 1, 2), dgamma if affine and ctx.needs_input_grad[1] else None,
                dbeta if affine and ctx.needs_input_grad[2] else None, None, None)


class _FrozenBnFn(torch.autograd.Function):
    """y = [relu](batch_norm(x)) with the module's running statistics (an eval()-mode layer), on libbts_hip.so: the buffers
    and the batch counter are only read.  Backward is one streaming pass; the sums run only where gamma / beta take a
    gradient, dx only where the input does."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, relu):
        B, C, H, W = x.shape
        x2d, _ = _nhwc_rows(x.detach())
        npix = B * H * W
        vecs = torch.empty((4, C), dtype=torch.float32, device=x.device)
        ops.bn_frozen_vectors(C, None if gamma is None else gamma.detach(), None if beta is None else beta.detach(),
                              bn.running_mean, bn.running_var, bn.eps, out=vecs)
        y = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
        ops.bn_apply(x2d, C, vecs[2], vecs[3], relu, y.view(npix, C))
        ctx.save_for_backward(x2d, vecs)
        ctx.meta = (B, C, H, W, relu, gamma is not None)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        x2d, vecs = ctx.saved_tensors
        B, C, H, W, relu, affine = ctx.meta
        need = ctx.needs_input_grad
        sums = affine and (need[1] or need[2])
        if not sums and not need[0]:
            return None, None, None, None, None
        dy2d, _ = _nhwc_rows(grad_out)
        npix = B * H * W
        dx = torch.empty((B, H, W, C), dtype=torch.float32, device=grad_out.device) if need[0] else None
        ws = _bn_workspace(grad_out.device, ops.bn_train_ws_floats(npix, C)) if sums else None
        dgamma, dbeta = ops.bn_frozen_backward(x2d, dy2d, C, vecs[0], vecs[1], vecs[2], vecs[3], relu, ws,
                                               None if dx is None else dx.view(npix, C), sums=sums)
        return (None if dx is None else dx.permute(0, 3, 1, 2), dgamma if sums and need[1] else None,
                dbeta if sums and need[2] else None, None, None)


def _frozen_norm_layer(bn) -> bool:
    """An eval()-mode BatchNorm2d that normalises with its running buffers (bn_init_as_tf's layers)."""
    return not bn.training and bn.running_mean is not None and bn.running_var is not None


def _bn(x: torch.Tensor, bn: torch.nn.BatchNorm2d, relu: bool = False) -> torch.Tensor:
    """nn.BatchNorm2d (+ the ReLU that follows it) inside the training graph.  train() mode with a fixed momentum and
    C % 4 == 0 runs on the HIP kernels; so does a frozen (eval-mode) layer under ``frozen_norm_scope`` (native_frozen_norm).
    Without the switch a frozen layer, and always an exotic configuration, runs on ATen's native kernels (MIOpen
    bypassed: no gfx950 find-db in this image)."""
    if bn.training and bn.momentum is not None and x.shape[1] % 4 == 0 and x.is_cuda and x.dtype == torch.float32:
        return _BnFn.apply(x, bn.weight, bn.bias, bn, relu)
    if current_frozen_norm() and _frozen_norm_layer(bn) and x.shape[1] % 4 == 0 and x.is_cuda and x.dtype == torch.float32:
        return _FrozenBnFn.apply(x, bn.weight, bn.bias, bn, relu)
    with torch.backends.cudnn.flags(enabled=False):
        y = bn(x)
    return F.relu(y) if relu else y


# ------------------------------------------------------------------------------------------ module forwards
def atrous_forward(m, x):
    """atrous_conv.forward, bts.py:79-80."""
    seq = m.atrous_conv.aconv_sequence
    x = _bn(x, m.atrous_conv.first_bn, relu=True) if m.apply_bn_first else F.relu(x)
    x = _bn(conv2d(x, seq[1].weight, tag="aspp1x1"), seq[2], relu=True)
    return conv2d(x, seq[4].weight, padding=m.dilation, dilation=m.dilation, tag="aspp3x3")


class _UpconvFn(torch.autograd.Function):
    """y = elu(conv3x3(nearest_2x(x), w, padding 1)) in sub-pixel form in all three passes (include/bts_hip.h states the
    identities): 16 products per source pixel instead of the 36 of ``conv2d(..., up=2)``, no upsampled input gradient and
    no 2x2 sum pass behind it.  ELU' stays on ATen, as in ``_ConvFn``."""

    @staticmethod
    def forward(ctx, x, weight, tag):
        refuse_bf16("train.upconv")
        ops._need(x, "train.upconv")
        ops._need(weight, "train.upconv")
        B, C, h, w = x.shape
        cout, cin, k, k2 = weight.shape
        if cin != C or k != 3 or k2 != 3 or C % 4 or cout % 4:
            raise BtsHipError("train.upconv: weight %s does not fit input %s (3x3, channels multiples of 4)"
                              % (tuple(weight.shape), tuple(x.shape)))
        x2d, _ = _nhwc_rows(x.detach())
        wf, wd = _UPCONV_PACKER.get(weight)
        y = torch.empty((B, 2 * h, 2 * w, cout), dtype=torch.float32, device=x.device)
        pr = current_train_precision()        # bf16: forward and input gradient; the class weight gradients stay fp32
        with _launch_precision(pr):
            ops.conv_forward(x2d, B, h, w, wf, cout, 3, up=2, c_in_ld=C, y2d=y.view(B * 4 * h * w, cout), subpixel=True,
                             act=ops.ACT_ELU, tag=tag + ".fwd", c_in_real=C)
        out = y.permute(0, 3, 1, 2)
        ctx.save_for_backward(x2d, out, wd)   # ELU'(v) = 1 (y > 0) or y + 1; wd: this step's pack (refills happen between steps)
        ctx.geom = (B, C, h, w, cout, tag)
        ctx.precision = pr
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x2d, out, wd = ctx.saved_tensors
        B, C, h, w, cout, tag = ctx.geom
        grad_out = torch.ops.aten.elu_backward(grad_out, 1.0, 1.0, 1.0, True, out)
        dy2d, co4 = _nhwc_rows(grad_out)
        dev = grad_out.device
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dxr = torch.empty((B, h, w, C), dtype=torch.float32, device=dev)
            ops.upconv_dgrad(dy2d, B, h, w, wd, cout, C, dxr.view(B * h * w, C), splitk_ws=_splitk_workspace(dev), tag=tag + ".dgrad",
                             precision=2 if ctx.precision == 2 else None)
            dx = dxr.permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            g = ops.upconv_wgrad(x2d, B, h, w, C, dy2d, cout, _workspace(dev), tag=tag + ".wgrad")
            dw = g.reshape(cout, 3, 3, C).permute(0, 3, 1, 2).contiguous()     # OIHW, the layout DDP buckets expect
        return dx, dw, None


def upconv_forward(m, x, subpixel=None):
    """upconv.forward, bts.py:90-94.  ``subpixel`` (the decoder passes its ``subpixel_upconv_train``; None: the module's
    own ``subpixel_train`` attribute, default False): ratio-2 layers whose channel counts are multiples of 4 run in
    sub-pixel form in all three passes (_UpconvFn); everything else stays on ``conv2d``."""
    if m.ratio not in (1, 2):
        raise BtsHipError("upconv: ratio %r not built (1 or 2)" % (m.ratio,))
    w = m.conv.weight
    if subpixel is None:
        subpixel = getattr(m, "subpixel_train", False)
    if subpixel and m.ratio == 2 and w.shape[0] % 4 == 0 and w.shape[1] % 4 == 0:
        return _UpconvFn.apply(x, w, "upconv")
    return conv2d(x, m.conv.weight, padding=1, up=int(m.ratio), tag="upconv", act=ops.ACT_ELU)


def reduction_forward(m, net):
    """reduction_1x1.forward, bts.py:124-136: the 1x1 stack, then (non-final) the plane-parameter transform."""
    for layer in m.reduc:
        if isinstance(layer, torch.nn.Conv2d):                       # plane_params
            net = conv2d(net, layer.weight, tag="reduc", bf16=False)
        elif isinstance(layer[1], torch.nn.ELU) and layer[1].alpha == 1.0:
            net = conv2d(net, layer[0].weight, tag="reduc", act=ops.ACT_ELU, bf16=False)   # inter_*: ELU in the epilogue
        else:
            net = layer[1](conv2d(net, layer[0].weight, tag="reduc", bf16=False))   # Sigmoid (final)
    if m.is_final:
        return net
    import math
    theta = torch.sigmoid(net[:, 0]) * (math.pi / 3)
    phi = torch.sigmoid(net[:, 1]) * (math.pi * 2)
    dist = torch.sigmoid(net[:, 2]) * m.max_depth
    sin_t = torch.sin(theta)
    return torch.stack([sin_t * torch.cos(phi), sin_t * torch.sin(phi), torch.cos(theta), dist], dim=1)


# ---- fused reduction scales (decoder.fused_reduction_train): one forward launch, one backward-data launch and one
# weight-gradient launch per layer instead of the layer-by-layer graph above
def _reduc_weights(m):
    return [c.weight for c in m.reduc.modules() if isinstance(c, torch.nn.Conv2d)]


def fused_reduction_available(m, upratio: int) -> bool:
    """Whether the fused training kernels cover this reduction_1x1 module at this upratio (0: the final chain).  The
    chains of bts_size 256 are not built: the caller stays on the layer-by-layer path for them."""
    return bool(m.is_final) == (upratio == 0) and ops.reduc_train_supported(m.c_in, m.c_first_out, upratio)


def fused_lpg_scale(reduc_mod, lpg_mod, feat, batched_wgrad=False):
    """reduction_1x1 -> F.normalize -> LPG -> /max_depth of one scale (bts.py:249-256) as one autograd node.
    ``batched_wgrad``: the layers' weight gradients in one batched launch (decoder.batched_wgrad)."""
    refuse_bf16("train.fused_lpg_scale")
    am = torch.empty((), dtype=torch.float32, device=feat.device)
    fn = ops.ReducLpgBatchedFunction if batched_wgrad else ops.ReducLpgFunction
    depth = fn.apply(feat, reduc_mod.max_depth, int(lpg_mod.upratio), reduc_mod.packed_train(), am,
                                       _workspace(feat.device), *_reduc_weights(reduc_mod))
    lpg_mod.abs_min = am
    return depth


def fused_reduction_final(reduc_mod, feat, batched_wgrad=False):
    """reduc1x1 (bts.py:285): the final chain and its sigmoid as one autograd node."""
    refuse_bf16("train.fused_reduction_final")
    fn = ops.ReducFinalBatchedFunction if batched_wgrad else ops.ReducFinalFunction
    return fn.apply(feat, reduc_mod.max_depth, reduc_mod.packed_train(), _workspace(feat.device),
                                        *_reduc_weights(reduc_mod))


def _conv_elu(seq, x, tag, bf16=True):
    return conv2d(x, seq[0].weight, padding=1, tag=tag, act=ops.ACT_ELU, bf16=bf16)


def decoder_forward(dec, features, focal):
    """bts.forward in train() mode (bts.py:223-293): same dataflow as the inference path, as an autograd graph."""
    with _deferred_batch_counts(), precision_scope(getattr(dec, "train_precision", "fp32")), \
            frozen_norm_scope(getattr(dec, "native_frozen_norm", False)):
        return _decoder_forward(dec, features, focal)


def _decoder_forward(dec, features, focal):
    begin_step()
    skip0, skip1, skip2, skip3 = features[1], features[2], features[3], features[4]
    md = dec.params.max_depth
    cl = torch.channels_last
    x = F.relu(features[5]).contiguous(memory_format=cl)
    sub = bool(getattr(dec, "subpixel_upconv_train", False))
    x = _bn(upconv_forward(dec.upconv5, x, sub), dec.bn5)
    iconv5 = _conv_elu(dec.conv5, torch.cat([x, skip3], 1), "conv5")
    x = _bn(upconv_forward(dec.upconv4, iconv5, sub), dec.bn4)
    concat4 = torch.cat([x, skip2], 1)
    iconv4 = _bn(_conv_elu(dec.conv4, concat4, "conv4"), dec.bn4_2)

    grown, branches, inp = concat4, [], iconv4
    for name in ("daspp_3", "daspp_6", "daspp_12", "daspp_18", "daspp_24"):
        d = atrous_forward(getattr(dec, name), inp)
        branches.append(d)
        grown = torch.cat([grown, d], 1)
        inp = grown
    daspp_feat = _conv_elu(dec.daspp_conv, torch.cat([iconv4] + branches, 1), "daspp_conv")

    fused = bool(getattr(dec, "fused_reduction_train", False))
    batched = bool(getattr(dec, "batched_wgrad", False))

    def lpg_scale(reduc_mod, lpg_mod, feat):
        if fused and fused_reduction_available(reduc_mod, int(lpg_mod.upratio)):
            return fused_lpg_scale(reduc_mod, lpg_mod, feat, batched)
        r = reduction_forward(reduc_mod, feat)
        plane_eq = torch.cat([F.normalize(r[:, :3], 2, 1), r[:, 3:4]], 1).contiguous()
        return lpg_mod(plane_eq, focal).unsqueeze(1) / md

    depth_8x8 = lpg_scale(dec.reduc8x8, dec.lpg8x8, daspp_feat)
    x = _bn(upconv_forward(dec.upconv3, daspp_feat, sub), dec.bn3)
    # conv3 / conv2 / conv1 (the planar-tail layers of the inference path), the reduction chains and get_depth are what the
    # inference bf16 mode keeps in fp32: they stay fp32 under train_precision "bf16" too
    iconv3 = _conv_elu(dec.conv3, torch.cat([x, skip1, depth_8x8[:, :, ::4, ::4]], 1), "conv3", bf16=False)
    depth_4x4 = lpg_scale(dec.reduc4x4, dec.lpg4x4, iconv3)
    x = _bn(upconv_forward(dec.upconv2, iconv3, sub), dec.bn2)
    iconv2 = _conv_elu(dec.conv2, torch.cat([x, skip0, depth_4x4[:, :, ::2, ::2]], 1), "conv2", bf16=False)
    depth_2x2 = lpg_scale(dec.reduc2x2, dec.lpg2x2, iconv2)
    upconv1 = upconv_forward(dec.upconv1, iconv2, sub)
    if fused and fused_reduction_available(dec.reduc1x1, 0):
        reduc1x1 = fused_reduction_final(dec.reduc1x1, upconv1, batched)
    else:
        reduc1x1 = reduction_forward(dec.reduc1x1, upconv1)
    iconv1 = _conv_elu(dec.conv1, torch.cat([upconv1, reduc1x1, depth_2x2, depth_4x4, depth_8x8], 1), "conv1", bf16=False)
    final_depth = md * torch.sigmoid(conv2d(iconv1, dec.get_depth[0].weight, padding=1, tag="get_depth", bf16=False))
    if dec.params.dataset == 'kitti':
        final_depth = final_depth * focal.view(-1, 1, 1, 1).float() / 715.0873
    return depth_8x8, depth_4x4, depth_2x2, reduc1x1, final_depth, iconv1


# ------------------------------------------------------------------------------------------ encoder (DenseNet)
class _DenseBlockFn(torch.autograd.Function):
    """One torchvision _DenseBlock in train() mode as a single autograd node working IN PLACE on one NHWC buffer.

    torchvision re-concatenates the whole prefix for every layer (and autograd then splits and re-adds the prefix
    gradient once per layer: O(L^2) copy/add launches, 36 layers in DenseNet161's third block).  Here the block owns one
    [B,H,W,C_total] buffer: layer i normalises the first C_i channels (a strided view), and its 3x3 convolution writes
    its growth channels straight into columns [C_i, C_i + g).  Backward walks the layers in reverse on one gradient
    buffer of the same shape: each layer reads its own columns as dy and adds its input gradient onto the prefix.
    Saved per layer: the 1x1 output and the four BN vectors of both norms; the normalised inputs are never materialised --
    norm + ReLU ride in the prologue of the forward convolutions and of the weight-gradient gather."""

    @staticmethod
    def forward(ctx, x, block, batched, *params):
        refuse_bf16("train.densenet_block")
        B, C0, H, W = x.shape
        layers = list(block.values())
        g = layers[0].conv2.out_channels
        mid = layers[0].conv1.out_channels
        Ct = C0 + len(layers) * g
        npix = B * H * W
        dev = x.device
        buf = torch.empty((npix, Ct), dtype=torch.float32, device=dev)
        buf[:, :C0] = x.detach().permute(0, 2, 3, 1).reshape(npix, C0)
        saved = []
        ws = _bn_workspace(dev, ops.bn_train_ws_floats(npix, Ct))
        sk = _splitk_workspace(dev)
        pr = current_train_precision()
        # per norm layer: frozen statistics (eval mode, under frozen_norm_scope) or batch statistics; mixed blocks are fine
        frozen = tuple((not L.norm1.training, not L.norm2.training) for L in layers)
        if any(f1 or f2 for f1, f2 in frozen) and not current_frozen_norm():
            raise BtsHipError("train.densenet_block: a frozen norm layer needs native_frozen_norm (frozen_norm_scope)")
        if batched:      # one slab per kind, so that the deferred weight gradients of all layers address six buffers
            T1 = torch.empty((len(layers), npix, mid), dtype=torch.float32, device=dev)
            stats = torch.empty((len(layers), 8, max(Ct, mid)), dtype=torch.float32, device=dev)   # rows 0-3 norm1, 4-7 norm2
        for i, L in enumerate(layers):
            Ci = C0 + i * g
            s1 = _dense_vectors(L.norm1, buf[:, :Ci], Ci, ws, stats[i, 0:4, :Ci] if batched else None, frozen[i][0])
            # norm + ReLU ride in the convolutions' prologue (applied on the way to LDS): the normalised tensors are
            # never written in the forward pass
            t1 = T1[i] if batched else torch.empty((npix, mid), dtype=torch.float32, device=dev)
            with _launch_precision(pr):
                ops.conv_forward(buf[:, :Ci], B, H, W, _PACKER.get(L.conv1.weight, Ci, WeightPacker.FWD), mid, 1, c_in_ld=Ci,
                                 pre=(s1[2], s1[3]), pre_relu=True, y2d=t1, tag="enc.fwd", splitk_ws=sk)
            s2 = _dense_vectors(L.norm2, t1, mid, ws, stats[i, 4:8, :mid] if batched else None, frozen[i][1])
            with _launch_precision(pr):
                ops.conv_forward(t1, B, H, W, _PACKER.get(L.conv2.weight, mid, WeightPacker.FWD), g, 3, c_in_ld=mid,
                                 pre=(s2[2], s2[3]), pre_relu=True, y2d=buf[:, Ci:Ci + g], tag="enc.fwd", splitk_ws=sk)
            for bn, fz in zip((L.norm1, L.norm2), frozen[i]):
                if bn.num_batches_tracked is not None and not fz:
                    _count_batch(bn)
            if not batched:
                saved += [t1, torch.stack(s1), torch.stack(s2)]
        if batched:
            saved = [T1, stats]
        ctx.save_for_backward(buf, *saved)
        ctx.block = block
        ctx.batched_wgrad = batched
        ctx.precision = pr
        ctx.frozen = frozen
        ctx.geom = (B, C0, H, W, g, mid, Ct)
        return buf.view(B, H, W, Ct).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        buf, *saved = ctx.saved_tensors
        B, C0, H, W, g, mid, Ct = ctx.geom
        layers = list(ctx.block.values())
        npix = B * H * W
        dev = grad_out.device
        G = torch.empty((npix, Ct), dtype=torch.float32, device=dev)     # private copy: the walk below accumulates into it
        G.view(B, H, W, Ct).copy_(grad_out.permute(0, 2, 3, 1))
        d_a2 = torch.empty((npix, mid), dtype=torch.float32, device=dev)
        batched = ctx.batched_wgrad
        if batched:      # the weight gradients wait for the end of the walk: every layer keeps its d_t1
            T1, stats = saved
            D_T1 = torch.empty((len(layers), npix, mid), dtype=torch.float32, device=dev)
        else:
            d_t1 = torch.empty((npix, mid), dtype=torch.float32, device=dev)
        d_a1 = torch.empty((npix, Ct), dtype=torch.float32, device=dev)
        frozen = ctx.frozen
        dpre = None if all(f1 for f1, _ in frozen) else torch.empty((npix, Ct), dtype=torch.float32, device=dev)
        ws = _bn_workspace(dev, ops.bn_train_ws_floats(npix, Ct))
        wws = _workspace(dev)
        sk = _splitk_workspace(dev)
        grads = [None] * (6 * len(layers))
        need = ctx.needs_input_grad
        pr = ctx.precision
        for i in range(len(layers) - 1, -1, -1):
            L = layers[i]
            Ci = C0 + i * g
            if batched:
                t1, s1, s2, d_t1 = T1[i], stats[i, 0:4, :Ci], stats[i, 4:8, :mid], D_T1[i]
            else:
                t1, s1, s2 = saved[3 * i], saved[3 * i + 1], saved[3 * i + 2]
            gy = G[:, Ci:Ci + g]                                               # this layer's output gradient, in place
            with _launch_precision(pr):
                ops.conv_forward(gy, B, H, W, _PACKER.get(L.conv2.weight, g, WeightPacker.DGRAD), mid, 3, c_in_ld=g, y2d=d_a2,
                                 pad=1, tag="enc.dgrad", splitk_ws=sk)
            if need[3 + 6 * i + 5] and not batched:   # the weight-gradient gather re-applies norm2 + ReLU to t1 on the fly
                w2 = ops.conv_wgrad(t1, B, H, W, mid, gy, g, 3, ws=wws, tag="enc.wgrad", pre=(s2[2], s2[3]), pre_relu=True,
                                    precision=pr)
                grads[6 * i + 5] = w2.reshape(g, 3, 3, mid).permute(0, 3, 1, 2).contiguous()
            if frozen[i][1]:     # dx depends on no sum: one pass, the sums only where gamma / beta take a gradient
                dg2, db2 = ops.bn_frozen_backward(t1, d_a2, mid, s2[0], s2[1], s2[2], s2[3], True, ws, d_t1,
                                                  sums=bool(need[3 + 6 * i + 3] or need[3 + 6 * i + 4]))
            else:
                dg2, db2 = ops.bn_train_backward(t1, d_a2, mid, s2[0], s2[1], s2[2], s2[3], True, ws, d_t1)
            if need[3 + 6 * i + 3]:
                grads[6 * i + 3] = dg2
            if need[3 + 6 * i + 4]:
                grads[6 * i + 4] = db2
            with _launch_precision(pr):
                ops.conv_forward(d_t1, B, H, W, _PACKER.get(L.conv1.weight, mid, WeightPacker.DGRAD), Ci, 1, c_in_ld=mid,
                                 y2d=d_a1[:, :Ci], pad=0, tag="enc.dgrad", splitk_ws=sk)
            if need[3 + 6 * i + 2] and not batched:
                w1 = ops.conv_wgrad(buf[:, :Ci], B, H, W, Ci, d_t1, mid, 1, ws=wws, tag="enc.wgrad", pre=(s1[2], s1[3]),
                                    pre_relu=True, precision=pr)
                grads[6 * i + 2] = w1.reshape(mid, Ci, 1, 1)
            if frozen[i][0]:     # the prefix receives this layer's input gradient straight from the kernel
                dg1, db1 = ops.bn_frozen_backward(buf[:, :Ci], d_a1[:, :Ci], Ci, s1[0], s1[1], s1[2], s1[3], True, ws, G[:, :Ci],
                                                  sums=bool(need[3 + 6 * i + 0] or need[3 + 6 * i + 1]), accumulate=True)
            else:
                dg1, db1 = ops.bn_train_backward(buf[:, :Ci], d_a1[:, :Ci], Ci, s1[0], s1[1], s1[2], s1[3], True, ws, dpre[:, :Ci])
                G[:, :Ci] += dpre[:, :Ci]                                      # the prefix receives this layer's input gradient
            if need[3 + 6 * i + 0]:
                grads[6 * i + 0] = dg1
            if need[3 + 6 * i + 1]:
                grads[6 * i + 1] = db1
        if batched:
            # Deferring is safe: buf, T1 and the norm vectors are read-only in backward, D_T1[i] is written once, and layer
            # i's columns of G are final when layer i is processed (layers below only add onto columns < C_i).
            mask = tuple((bool(need[3 + 6 * i + 2]), bool(need[3 + 6 * i + 5])) for i in range(len(layers)))
            dws = iter(_dense_wgrad_batch(ctx.geom, mask, buf, G, T1, D_T1, stats, wws, pr))
            for i, (n1, n2) in enumerate(mask):
                if n1:
                    grads[6 * i + 2] = next(dws).reshape(mid, C0 + i * g, 1, 1)
                if n2:
                    grads[6 * i + 5] = next(dws).reshape(g, 3, 3, mid).permute(0, 3, 1, 2).contiguous()
        dx = G[:, :C0].reshape(B, H, W, C0).permute(0, 3, 1, 2) if need[0] else None
        return (dx, None, None) + tuple(grads)


def _dense_vectors(bn, x2d, C, ws, out, frozen):
    """(mean, invstd, scale, shift) of one norm layer of a dense block: from the running buffers when ``frozen`` (nothing
    is updated), else the batch statistics with the running-buffer update."""
    if frozen:
        return ops.bn_frozen_vectors(C, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, out=out)
    return ops.bn_train_stats(x2d, C, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, bn.running_mean,
                              bn.running_var, ws, out=out)


# (device, block geometry, need mask, workspace floats) -> ops.WgradBatch; the plan depends on the workspace size, so it
# is part of the key.  Bounded: a run that keeps changing crop size or freeze mask evicts the least recently used table
_DENSE_WGRAD_BATCHES = ops.BatchCache(64)


def _dense_wgrad_batch(geom, mask, buf, G, T1, D_T1, stats, wws, precision=0):
    """Every wanted weight gradient of one dense block in ONE batched launch over the bases buf, G, T1, D_T1, stats and
    a flat DW (the return value's views, in layer order: 1x1 then 3x3).  The batch -- plan and device table -- is built
    on the first step of a (geometry, need mask) and only launched afterwards; frozen layers are not in it, and a block
    with nothing to compute launches nothing.  ``precision`` 2: the same table on the bf16 launch."""
    B, C0, H, W, g, mid, Ct = geom
    sizes = []
    for i, (n1, n2) in enumerate(mask):
        sizes += [mid * (C0 + i * g)] * n1 + [g * 9 * mid] * n2
    if not sizes:
        return []
    DW = torch.empty(sum(sizes), dtype=torch.float32, device=buf.device)
    bases = [buf, G, T1, D_T1, stats, DW]
    key = (str(buf.device), geom, mask, wws.numel())
    batch = _DENSE_WGRAD_BATCHES.get(key)
    if batch is None:
        problems, at = [], 0
        for i, (n1, n2) in enumerate(mask):
            Ci = C0 + i * g
            if n1:
                problems.append(dict(x=buf[:, :Ci], dy=D_T1[i], dw=DW[at:at + mid * Ci], B=B, h_in=H, w_in=W, c_in=Ci, c_out=mid,
                                     ksize=1, pre=(stats[i, 2, :Ci], stats[i, 3, :Ci]), pre_relu=True))
                at += mid * Ci
            if n2:
                problems.append(dict(x=T1[i], dy=G[:, Ci:Ci + g], dw=DW[at:at + g * 9 * mid], B=B, h_in=H, w_in=W, c_in=mid,
                                     c_out=g, ksize=3, pre=(stats[i, 6, :mid], stats[i, 7, :mid]), pre_relu=True))
                at += g * 9 * mid
        batch = _DENSE_WGRAD_BATCHES.put(key, ops.WgradBatch(problems, bases, wws.numel(), tag="enc.wgrad"))
    return batch.run(bases, wws, precision=precision)


def _dense_block(block, x, batched_wgrad=False):
    """Fused in-place dense block when every norm layer is an ordinary train()-mode BatchNorm2d with affine parameters
    and channel counts the kernels take (multiples of 4) -- or, under ``frozen_norm_scope``, a frozen one (eval mode, running
    buffers present, affine), layer by layer; otherwise the generic layer-by-layer graph.
    ``batched_wgrad``: the block's weight gradients in one batched launch at the end of its backward walk."""
    nn = torch.nn
    layers = list(block.values())
    ok = x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 4 == 0
    native = current_frozen_norm()
    for L in layers:
        for bn in (L.norm1, L.norm2):
            live = isinstance(bn, nn.BatchNorm2d) and bn.training and bn.momentum is not None and bn.affine \
                and bn.track_running_stats and bn.running_mean is not None
            ok = ok and (live or (native and isinstance(bn, nn.BatchNorm2d) and bn.affine and _frozen_norm_layer(bn)))
        ok = ok and L.conv1.bias is None and L.conv2.bias is None and L.conv2.out_channels % 4 == 0 \
            and L.conv1.out_channels % 4 == 0 and L.conv2.padding[0] == 1 and L.conv1.kernel_size[0] == 1 \
            and L.conv2.kernel_size[0] == 3
    if not ok:
        return None
    params = []
    for L in layers:
        params += [L.norm1.weight, L.norm1.bias, L.conv1.weight, L.norm2.weight, L.norm2.bias, L.conv2.weight]
    return _DenseBlockFn.apply(x, block, bool(batched_wgrad), *params)


def _run_children(children, x, tapped=None, taps=None, batched_wgrad=False):
    """Run (name, module) pairs in order on the HIP kernels: bias-free ungrouped convolutions, batch-statistic BN
    with the ReLU that follows it fused in; pools and stray activations are the modules themselves.
    ``tapped(name)``: children whose output joins ``taps`` (encoder.forward's skip list)."""
    nn = torch.nn
    i = 0
    while i < len(children):
        name, child = children[i]
        last = name
        if isinstance(child, nn.Conv2d):
            if child.bias is not None or child.groups != 1 or child.kernel_size[0] != child.kernel_size[1]:
                raise BtsHipError("train: convolution %r is not built (bias-free, ungrouped, square only)" % (child,))
            x = conv2d(x, child.weight, padding=child.padding[0], dilation=child.dilation[0], stride=child.stride[0],
                       tag="enc")
        elif isinstance(child, nn.BatchNorm2d):
            fuse = (i + 1 < len(children) and isinstance(children[i + 1][1], nn.ReLU)
                    and not (tapped is not None and tapped(name)))
            x = _bn(x, child, relu=fuse)
            if fuse:
                i += 1
                last = children[i][0]
        elif isinstance(child, nn.ModuleDict):               # _DenseBlock
            fused = _dense_block(child, x, batched_wgrad) if FUSED_DENSE_BLOCKS else None
            if fused is not None:
                x = fused                                    # one autograd node, one NHWC buffer, no torch.cat
            else:                                            # generic graph: each layer sees the concat of all earlier ones
                feats = [x]
                for layer in child.values():
                    y = torch.cat(feats, 1) if len(feats) > 1 else feats[0]
                    feats.append(_run_children(list(layer.named_children()), y))   # norm1 relu1 conv1 norm2 relu2 conv2
                x = torch.cat(feats, 1)
        elif isinstance(child, nn.Sequential):               # _Transition
            x = _run_children(list(child.named_children()), x, batched_wgrad=batched_wgrad)
        else:
            x = child(x)
        if tapped is not None and tapped(last):
            taps.append(x)
        i += 1
    return x


def densenet_encoder_forward(enc, x):
    """encoder.forward (bts.py:327-338) for the DenseNet encoders in train() mode: same tap list, convolutions, norm
    layers and their gradients on libbts_hip.so."""
    ops._need(x, "train.encoder")
    begin_step()
    taps = [x]
    cur = x.float().contiguous(memory_format=torch.channels_last)
    with _deferred_batch_counts(), precision_scope(getattr(enc, "train_precision", "fp32")), \
            frozen_norm_scope(getattr(enc, "native_frozen_norm", False)):
        _run_children(list(enc.base_model.named_children()), cur,
                      tapped=lambda name: any(fragment in name for fragment in enc.feat_names), taps=taps,
                      batched_wgrad=bool(getattr(enc, "batched_wgrad", False)))
    return taps


# ------------------------------------------------------------------------------------------ encoder (ResNet / ResNeXt)
def _bottleneck(blk, x, tag, grouped_native=False):
    """torchvision Bottleneck.forward: 1x1 -> (grouped, strided) 3x3 -> 1x1, + identity, ReLU.  ``grouped_native``:
    encoder.grouped_conv_train."""
    out = _bn(conv2d(x, blk.conv1.weight, tag=tag), blk.bn1, relu=True)
    c2 = blk.conv2
    out = _bn(conv2d(out, c2.weight, padding=c2.padding[0], dilation=c2.dilation[0], stride=c2.stride[0], groups=c2.groups,
                     tag=tag, grouped_native=grouped_native), blk.bn2, relu=True)
    out = _bn(conv2d(out, blk.conv3.weight, tag=tag), blk.bn3)
    if blk.downsample is not None:
        d = blk.downsample[0]
        x = _bn(conv2d(x, d.weight, stride=d.stride[0], tag=tag), blk.downsample[1])
    return F.relu(out + x)


def resnet_encoder_forward(enc, x):
    """encoder.forward (bts.py:327-338) for the ResNet-50/101 and ResNeXt-50/101 encoders in train() mode: taps
    [x, relu, layer1, layer2, layer3, layer4]; every convolution (incl. the grouped and strided ones) and norm layer and
    their gradients on libbts_hip.so, max-pool / residual add on PyTorch-ROCm kernels."""
    ops._need(x, "train.encoder")
    begin_step()
    m = enc.base_model
    cur = x.float().contiguous(memory_format=torch.channels_last)
    c1 = m.conv1
    native = bool(getattr(enc, "grouped_conv_train", False))
    with _deferred_batch_counts(), precision_scope(getattr(enc, "train_precision", "fp32")), \
            frozen_norm_scope(getattr(enc, "native_frozen_norm", False)):
        cur = _bn(conv2d(cur, c1.weight, padding=c1.padding[0], stride=c1.stride[0], tag="enc"), m.bn1, relu=True)
        taps = [x, cur]
        cur = m.maxpool(cur)
        for li, layer in enumerate((m.layer1, m.layer2, m.layer3, m.layer4)):
            for blk in layer:
                cur = _bottleneck(blk, cur, "enc", native)
            taps.append(cur)
    return taps
