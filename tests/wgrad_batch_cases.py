"""One table of batches for tests/test_wgrad_batch_host.py (CPU: what the batch planner gives each batch, and that the
table as a whole reaches every tile, split regime and gather mode inside a batch) and tests/test_wgrad_batch_gpu.py
(GPU: every problem of every batch bit-exact against the fp64 statement of tests/test_wgrad_gpu.py).

A batch is (workspace floats, [WgradCase]); the cases are tests/wgrad_cases.py's own type, so its `reference` serves
them unchanged.  Shapes were picked with ops.conv_wgrad_batch_plan, the smallest that reach each item; nothing forces a
tile or a split -- the host test fails, naming the item, when the planner stops choosing it."""
from collections import OrderedDict

import wgrad_cases as wc

MI = wc.MI
_c = wc._c

# ---- a mini dense block: B=2, 5x7 map (70 pixels: three K-steps, a ragged last one), C0=16, g=8, mid=16, L=4.
# Problem 2i is layer i's 1x1 (x = the first Ci columns of the block buffer, dy = layer i's slab of D_T1), problem 2i+1
# its 3x3 (x = layer i's slab of T1, dy = columns [Ci, Ci+g) of G); both with norm + ReLU in the gather.
DENSE = dict(B=2, H=5, W=7, C0=16, g=8, mid=16, L=4)
DENSE_CT = DENSE["C0"] + DENSE["L"] * DENSE["g"]


def dense_block_cases(B, H, W, C0, g, mid, L, prefix="dense"):
    Ct = C0 + L * g
    out = []
    for i in range(L):
        Ci = C0 + i * g
        out.append(_c("%s_l%d_1x1" % (prefix, i), B, H, W, Ci, mid, 1, pre=True, pre_relu=True, x_extra=Ct - Ci))
        out.append(_c("%s_l%d_3x3" % (prefix, i), B, H, W, mid, g, 3, pre=True, pre_relu=True, dy_extra=Ct - g))
    return out


def _tiny(i):
    """70 tiny problems with different channel counts, kernel sizes and pixel counts (lookup depth 7)."""
    k = (1, 3)[i % 2]
    return _c("tiny%02d" % i, 1 + i % 2, 2 + i % 3, 3 + i % 5, 4 * (1 + i % 4), 4 * (1 + i % 3), k,
              pre=i % 7 == 0, pre_relu=i % 14 == 0, x_extra=8 * (i % 3 == 0), dy_extra=8 * (i % 5 == 0))


BATCHES = OrderedDict([
    ("mini_dense", (1 * MI, dense_block_cases(**DENSE))),
    # every geometry of wgrad_cases' t64_* cases in ONE launch: up2, stride-2 k7, dilation 24, W = 3, bundles, pre, slices
    ("t64_geometries", (1 * MI, [c for c in wc.CASES if c.name.startswith("t64_")])),
    ("tiny70", (1 * MI, [_tiny(i) for i in range(70)])),
    # a 128x128 unsplit problem (M = 40) whose 516 tiles leave the rest of the batch to be split to reach the chip
    ("mixed", (4 * MI, [
        wc.BY_NAME["t128_unsplit"],
        _c("mix_64x128", 1, 40, 50, 128, 64, 3),                        # M 2000
        _c("mix_k1_slices", 2, 30, 31, 64, 32, 1, x_extra=8, dy_extra=8),       # M 1860
        wc.BY_NAME["t64_s25"],                                          # M 3965
        _c("mix_bundles", 2, 20, 21, 32, 32, 3, n_bundles=2, pre=True),  # M 840
    ])),
    ("single", (1 * MI, [_c("single_64x64", 1, 25, 41, 64, 64, 1)])),     # n = 1, M 1025
    # the same batch with a workspace too small for the splits it would like
    ("mixed_small_ws", (64 * 1024, [
        _c("sws_64x128", 1, 40, 50, 128, 64, 3),
        _c("sws_64x64", 1, 61, 65, 64, 64, 1),
    ])),
])

FLOAT_BATCHES = ["mini_dense", "mixed"]


def problem_of(c):
    """ops.conv_wgrad_batch_plan's dict for one case."""
    nb = max(c.n_bundles, 1)
    return dict(B=c.B, h_in=c.h, w_in=c.w, c_in=c.c_in, c_out=c.c_out, ksize=c.ksize, dil=c.dil, stride=c.stride, pad=c.pad,
                up=c.up, n_bundles=c.n_bundles, pre=c.pre, pre_relu=c.pre_relu, x_pix_stride=nb * c.c_in + c.x_extra,
                dy_pix_stride=nb * c.c_out + c.dy_extra)


def pixels(c):
    H, W = wc.out_hw(c)
    return c.B * H * W


def dw_floats(c):
    return max(c.n_bundles, 1) * c.c_out * c.ksize * c.ksize * c.c_in


def plan_of(name):
    """[(bm, bn, split, pix_per_split, ws_offset)] from the library's batch planner."""
    from bts_amd import ops
    ws_floats, cases = BATCHES[name]
    return ops.conv_wgrad_batch_plan([problem_of(c) for c in cases], ws_floats)
