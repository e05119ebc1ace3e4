"""Reference side of the fused reduction-training tests: one reduction_1x1 scale (chain -> F.normalize -> LPG -> /max_depth,
or the final chain) from the oracle's arithmetic, differentiated by torch autograd on the CPU in any dtype."""
import numpy as np
import torch
import torch.nn.functional as F

from bts_amd import ops
from oracle import bts_oracle as O

MAX_DEPTH = 80.0
# (c_in, c_first_out, upratio); upratio 0 = the final chain
CHAINS = {"8x8": (128, 128, 8), "4x4": (128, 64, 4), "2x2": (64, 32, 2), "final": (32, 16, 0),
          # bts_size 256 (forward only: bts_reduc_bwd_f32 is not built for these, tests/reduc_lpg_cases.py)
          "8x8/256": (64, 64, 8), "4x4/256": (64, 32, 4), "2x2/256": (32, 16, 2), "final/256": (16, 8, 0)}


def make_case(name, B, h, w, seed, theta_scale=None):
    """Random x [B,c_in,h,w], xavier weights, random output gradient.  ``theta_scale``: multiply the theta row
    of plane_params: its sigmoid saturates and theta -> pi/3 on the cells with a positive logit, where the LPG denominator
    can cross zero in the corners of an 8 x 8 block."""
    c_in, c_first, k = CHAINS[name]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, c_in, h, w, generator=gen)
    ws = []
    for ci, co in ops.reduc_chain(c_in, c_first):
        wt = torch.empty(co if co > 0 else (3 if k else 1), ci, 1, 1)
        bound = float(np.sqrt(6.0 / (wt.shape[0] + wt.shape[1])))                 # xavier_uniform_
        wt.copy_((torch.rand(wt.shape, generator=gen) * 2 - 1) * bound)
        ws.append(wt)
    if theta_scale is not None:
        ws[-1][0] *= theta_scale                          # the theta row of plane_params
    kk = max(k, 1)
    gout = torch.randn(B, 1, h * kk, w * kk, generator=gen)
    return x, ws, gout


def scale_forward(x, ws, k, max_depth=MAX_DEPTH):
    """(output [B,1,h*k,w*k], un-clamped LPG denominator or None) in x's dtype."""
    r = O.reduction_forward(x, ws, max_depth, k == 0)
    if k == 0:
        return r, None
    plane = torch.cat([F.normalize(r[:, :3], 2, 1), r[:, 3:4]], 1)
    depth, _ = O.lpg_forward(plane, k)
    kk = int(k)
    pe = torch.repeat_interleave(torch.repeat_interleave(plane.detach(), kk, 2), kk, 3)
    u = ((torch.arange(kk).to(x.dtype) - (kk - 1) * 0.5) / kk).view(1, 1, kk).repeat(x.shape[0], x.shape[2] * kk, x.shape[3])
    v = ((torch.arange(kk).to(x.dtype) - (kk - 1) * 0.5) / kk).view(1, kk, 1).repeat(x.shape[0], x.shape[2], x.shape[3] * kk)
    den = pe[:, 0] * u + pe[:, 1] * v + pe[:, 2]
    return depth.unsqueeze(1) / max_depth, den


def reference_grads(x, ws, gout, k, dtype):
    """{"dx": ..., "dW0": ..., ...} (numpy float64 arrays) and the denominator, from CPU autograd in ``dtype``."""
    xd = x.to(dtype).requires_grad_(True)
    wd = [wt.to(dtype).requires_grad_(True) for wt in ws]
    out, den = scale_forward(xd, wd, k)
    out.backward(gout.to(dtype))
    g = {"dx": xd.grad.double().numpy()}
    for i, wt in enumerate(wd):
        g["dW%d" % i] = wt.grad.double().numpy()
    return g, (None if den is None else den.double().numpy()), out.detach()


def rel_errors(got, ref):
    """max-abs error over max-abs value, per tensor."""
    return {n: float(np.abs(np.asarray(got[n], dtype=np.float64) - r).max() / np.abs(r).max()) for n, r in ref.items()}


def conv_bar(ref, name=""):
    """The bar tests/test_train_gpu.py::test_conv2d_gradients_vs_torch_cpu applies to one convolution's gradient
    (err <= 2e-5 * scale * sqrt(max(1, elements per leading index // 64)) + 1e-6), as a fraction of the tensor's scale.
    For a weight gradient the leading index is the output channel, as there.  For dx that test's leading index is the
    batch, which would let the bar grow with the map area although a dx element's sum does not: here dx counts the
    elements per PIXEL (c_in), never more than that test allows."""
    scale = float(np.abs(ref).max())
    per = ref.shape[1] if name == "dx" else ref.size // ref.shape[0]
    return 2e-5 * np.sqrt(max(1, per // 64)) + 1e-6 / scale


# ---- the cases of tests/test_reduc_train_gpu.py: name -> (chain, B, h, w, seed, theta_scale) ------------------------------
CLAMP_CASE = ("8x8", 2, 24, 32, 743, 50.0)      # see test_clamp_branch for how the map size and the seed were found
PLAIN_CASES = {"8x8": ("8x8", 2, 5, 7, 0, None), "4x4": ("4x4", 2, 5, 7, 0, None), "2x2": ("2x2", 2, 5, 7, 0, None),
               "final": ("final", 2, 6, 10, 0, None)}


def persistent_shape(max_waves, passes=1):
    """(h, w) with h * w = passes * max_waves * 32 + r, 0 < r < 32: one partial tile more than ``passes`` passes of the
    whole grid (passes = 1: one wave iterates twice; 2: every wave iterates at least twice)."""
    for r in range(1, 32):
        n = passes * max_waves * 32 + r
        for h in range(2, 512):
            if n % h == 0:
                return h, n // h
    raise AssertionError("no shape")


_REF_CACHE = {}


def case_reference(key, case):
    """(x, ws, gout, fp64 gradients, fp64 denominator) of a case, computed once per session and shared."""
    if key not in _REF_CACHE:
        name, B, h, w, seed, ts = case
        x, ws, gout = make_case(name, B, h, w, seed, ts)
        g64, den, _ = reference_grads(x, ws, gout, CHAINS[name][2], torch.float64)
        _REF_CACHE[key] = (x, ws, gout, g64, den)
    return _REF_CACHE[key]
