"""The CPU statement of train_precision "bf16" (DESIGN 3a): ordinary torch arithmetic -- fp64 for the yardstick, fp32 for
the floor fp32 arithmetic itself has -- with the operand roundings of the bf16 training step INSERTED, as a small
autograd.Function that stands in for F.conv2d:

    forward    y  = conv(bf16(x'), bf16(w))
    backward   dx = conv^T(bf16(dy'), bf16(w)),   dw = corr(bf16(dy'), bf16(x'))

x' is whatever the graph feeds the convolution (after a norm layer + ReLU, after the nearest-2x upsample), dy' whatever
autograd hands back (after the ELU / ReLU mask); bf16() rounds the fp32 value to nearest even; products and sums are the
dtype's.  Nothing here touches the GPU or bts_amd.train."""
import torch
import torch.nn.functional as F
from torch.nn.modules.utils import _pair

_conv2d = F.conv2d                                 # the real one, whatever `rounded_convs` has put in its place


def rb(t):
    """t -> the nearest bf16 of its fp32 value, in t's dtype."""
    return t.detach().to(torch.float32).to(torch.bfloat16).to(t.dtype)


class RoundedConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, padding, dilation, groups):
        xr, wr = rb(x), rb(w)
        ctx.save_for_backward(xr, wr)
        ctx.conf = (stride, padding, dilation, groups)
        return _conv2d(xr, wr, None, stride, padding, dilation, groups)

    @staticmethod
    def backward(ctx, gy):
        xr, wr = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.conf
        gr = rb(gy)
        dx = torch.nn.grad.conv2d_input(xr.shape, wr, gr, stride, padding, dilation, groups) if ctx.needs_input_grad[0] else None
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, gr, stride, padding, dilation, groups) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None, None


def rconv(x, w, stride=1, padding=0, dilation=1, groups=1):
    return RoundedConv.apply(x, w, _pair(stride), _pair(padding), _pair(dilation), groups)


def conv_magnitudes(x, w, gy, stride=1, padding=0, dilation=1, groups=1):
    """sum |terms| of the three products of one rounded convolution: (forward, dx, dw), fp64."""
    xa, wa, ga = rb(x.double()).abs(), rb(w.double()).abs(), rb(gy.double()).abs()
    s, p, d = _pair(stride), _pair(padding), _pair(dilation)
    return (_conv2d(xa, wa, None, s, p, d, groups), torch.nn.grad.conv2d_input(xa.shape, wa, ga, s, p, d, groups),
            torch.nn.grad.conv2d_weight(xa, wa.shape, ga, s, p, d, groups))


class rounded_convs:
    """``with rounded_convs(keep_fp32):`` every bias-free F.conv2d (nn.Conv2d included) runs as RoundedConv, except where
    ``keep_fp32(input, weight)`` says the layer stays in plain arithmetic."""

    def __init__(self, keep_fp32=lambda x, w: False):
        self.keep = keep_fp32
        self.rounded = self.kept = 0

    def _conv(self, input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
        if bias is not None or self.keep(input, weight):
            self.kept += 1
            return _conv2d(input, weight, bias, stride, padding, dilation, groups)
        self.rounded += 1
        return rconv(input, weight, stride, padding, dilation, groups)

    def __enter__(self):
        F.conv2d = self._conv
        return self

    def __exit__(self, *exc):
        F.conv2d = _conv2d
        return False


# what the bf16 training step keeps in fp32: the 3-channel stem by its shape, these decoder layers by name
FP32_DECODER_LAYERS = ("conv3.", "conv2.", "conv1.", "get_depth.", "reduc8x8.", "reduc4x4.", "reduc2x2.", "reduc1x1.")


def model_keep_fp32(decoder_state):
    ids = {id(v) for k, v in decoder_state.items() if k.startswith(FP32_DECODER_LAYERS)}
    return lambda x, w: w.shape[1] <= 4 or id(w) in ids


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))
