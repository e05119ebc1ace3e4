"""One case table for tests/test_wgrad_plan_host.py (CPU: which tile and split the planner gives each case, and that the
table as a whole reaches every tile, split regime and gather mode) and tests/test_wgrad_gpu.py (GPU: every case
bit-exact against an fp64 statement of the weight gradient).

The shapes were picked with ops.conv_wgrad_plan (bts_conv_wgrad_plan_f32), the smallest that reach each item; nothing
here forces a tile -- the host test fails, naming the item, when the planner stops choosing it.  In the comments:
tile bm x bn, s = split, last = K-steps (32 pixels each) of the last split, M = output pixels."""
from collections import namedtuple

MI = 1 << 20

WgradCase = namedtuple("WgradCase", "name B h w c_in c_out ksize dil stride pad up n_bundles pre pre_relu x_extra dy_extra ws_floats")


def _c(name, B, h, w, c_in, c_out, ksize, dil=1, stride=1, pad=None, up=1, n_bundles=1, pre=False, pre_relu=False,
       x_extra=0, dy_extra=0, ws_floats=None):
    """c_in / c_out are per bundle.  x_extra / dy_extra: channels of the wider buffer the slice sits in (a multiple of 8:
    half in front of the slice, half behind).  ws_floats None = no workspace."""
    return WgradCase(name, B, h, w, c_in, c_out, ksize, dil, stride, dil * (ksize // 2) if pad is None else pad, up, n_bundles,
                     pre, pre_relu, x_extra, dy_extra, ws_floats)


CASES = [
    # ---- 128x128 (TM = TN = 2 accumulators, 2x2 waves, PB = 4 gather rows per thread).  The planner takes it with a
    # split only where the workspace caps the split below what 64x128 would want: about 8 k pixels, 8 Mi floats.
    _c("t128_s16_last11", 1, 89, 90, 448, 128, 3, ws_floats=8 * MI),                # M 8010, ragged N (4032 = 31.5 tiles)
    _c("t128_s17_last1", 5, 26, 67, 424, 128, 3, ws_floats=8 * MI),                 # M 8710: 6 pixels in the last split
    _c("t128_s16_last2_up2", 1, 41, 50, 448, 128, 3, up=2, ws_floats=8 * MI),       # M 8200 from a 41x50 map
    _c("t128_s16_last3_w31_b7", 7, 38, 31, 448, 128, 3, ws_floats=8 * MI),          # M 8246, W < 32, seven frames
    _c("t128_s5_cout100_h1", 1, 1, 2003, 1576, 100, 3, ws_floats=8 * MI),           # c_out % 128 != 0, N % 128 != 0, H = 1
    _c("t128_unsplit", 2, 4, 5, 1824, 512, 3),                                      # M 40: two K-steps, no workspace
    _c("t128_unsplit_1step_dil", 1, 4, 5, 1824, 512, 3, dil=6, pre=True, pre_relu=True),   # M 20: one K-step; dilation > map
    # ---- 64x128 (TM = 1, TN = 1, 1x4 waves, PB = 4)
    _c("t64x128_s126_last1", 1, 2801, 10, 128, 256, 1, ws_floats=4 * MI),           # M 28010, split >= 64
    _c("t64x128_s28_stride2", 1, 178, 180, 128, 128, 3, stride=2, ws_floats=4 * MI),   # M 8010 from a 178x180 map
    _c("t64x128_w3_pre", 1, 2670, 3, 128, 128, 3, pre=True, ws_floats=4 * MI),      # M 8010, W = 3: a K-step spans 11 rows
    _c("t64x128_slices_b3", 3, 45, 58, 128, 128, 3, x_extra=24, dy_extra=8, ws_floats=4 * MI),   # M 7830
    _c("t64x128_cout36", 1, 1, 16010, 512, 36, 1, ws_floats=4 * MI),                # c_out % 64 != 0
    _c("t64x128_nrag", 1, 90, 89, 1824, 64, 1, ws_floats=4 * MI),                   # N % 128 != 0
    _c("t64x128_s7", 1, 23, 43, 512, 128, 3, ws_floats=4 * MI),                     # M 989, split < 16
    _c("t64x128_unsplit", 2, 4, 5, 1024, 512, 3),                                   # M 40, no workspace
    # ---- 32x128 (TM = 1, TN = 1, 1x4 waves, PB = 4)
    _c("t32_s151_last1", 1, 245, 98, 132, 32, 1, ws_floats=1 * MI),                 # M 24010, N 132
    _c("t32_s84_k3", 4, 44, 76, 64, 32, 3, ws_floats=8 * MI),
    _c("t32_cout8_k3", 1, 4001, 1, 128, 8, 3, ws_floats=1 * MI),                    # c_out % 32 != 0, W = 1
    _c("t32_k7", 4, 40, 50, 16, 32, 7, ws_floats=4 * MI),
    _c("t32_up2_relu", 1, 34, 58, 64, 32, 3, up=2, pre=True, pre_relu=True, ws_floats=4 * MI),
    _c("t32_dil24", 9, 30, 31, 64, 32, 3, dil=24, ws_floats=4 * MI),                # dilation 24 on a 30x31 map
    _c("t32_bundles", 3, 40, 41, 32, 32, 3, n_bundles=4, ws_floats=4 * MI),
    _c("t32_bundles_pre", 3, 40, 41, 32, 32, 3, n_bundles=4, pre=True, pre_relu=True, x_extra=8, ws_floats=4 * MI),
    # ---- 64x64 (TM = TN = 1, 2x2 waves, PB = 2)
    _c("t64_unsplit", 2, 3, 7, 16, 8, 1),                                           # M 42, ragged everywhere
    _c("t64_unsplit_1step", 1, 1, 20, 64, 64, 3),                                   # M 20: one K-step, H = 1
    _c("t64_s7", 1, 25, 40, 64, 64, 1, ws_floats=1 * MI),                           # M 1000
    _c("t64_s25", 1, 61, 65, 64, 64, 1, ws_floats=1 * MI),                          # M 3965, 16 <= split < 64
    _c("t64_768", 1, 256, 384, 16, 8, 1, ws_floats=1 * MI),                         # M 98304: the 768-split ceiling
    _c("t64_up2", 1, 13, 20, 48, 40, 3, up=2, ws_floats=1 * MI),
    _c("t64_stride2_k7", 2, 32, 48, 4, 96, 7, stride=2, pad=3, ws_floats=1 * MI),
    _c("t64_dil24", 1, 13, 17, 64, 32, 3, dil=24, ws_floats=1 * MI),
    _c("t64_w3_b3", 3, 110, 3, 64, 32, 3, ws_floats=1 * MI),                         # W = 3
    _c("t64_pre", 2, 9, 13, 64, 32, 3, pre=True, ws_floats=1 * MI),
    _c("t64_pre_relu", 2, 9, 13, 64, 32, 1, pre=True, pre_relu=True, ws_floats=1 * MI),
    _c("t64_bundles", 2, 10, 14, 32, 32, 3, stride=2, n_bundles=4, ws_floats=1 * MI),
    _c("t64_bundles_pre", 1, 6, 8, 64, 64, 3, n_bundles=3, pre=True, pre_relu=True, ws_floats=1 * MI),
    _c("t64_slices", 3, 7, 11, 48, 48, 3, x_extra=16, dy_extra=8, pre=True, pre_relu=True, ws_floats=1 * MI),
]

BY_NAME = {c.name: c for c in CASES}

# float-valued test: one case per tile plus the 768-split case (none with `pre`: the bound is for fp32 sums of fp32
# products of the given operands)
FLOAT_CASES = ["t128_s16_last11", "t64x128_s126_last1", "t32_s84_k3", "t64_s7", "t64_768"]

# train.conv2d -> backward against ops.conv_wgrad: one geometry per tile under the training path's own workspace size
# (train.WGRAD_WS_FLOATS); (bm, bn) is the tile the case was chosen for
PATH_WS_FLOATS = 48 * MI
PATH_CASES = [
    ((128, 128), _c("path_t128", 2, 4, 5, 1824, 512, 3, ws_floats=PATH_WS_FLOATS)),
    ((64, 128), _c("path_t64x128", 1, 2, 6005, 448, 64, 3, ws_floats=PATH_WS_FLOATS)),
    ((32, 128), _c("path_t32", 4, 44, 76, 64, 32, 3, ws_floats=PATH_WS_FLOATS)),
    ((64, 64), _c("path_t64", 2, 9, 13, 64, 32, 3, ws_floats=PATH_WS_FLOATS)),
]


def sum_splits(p):
    """The documented fixed-order sum of split partials (csrc/wgrad.hip: sum_splits + the 16-lane finish), restated in
    numpy float32.  p: [split, ...] float32.  Lane j of 16 starts at split j, adds four at a time as
    (p[s] + p[s+16]) + (p[s+32] + p[s+48]) while s + 48 < split, then one at a time in steps of 16; the 16 lane sums are
    added left to right."""
    import numpy as np
    assert p.dtype == np.float32
    split = p.shape[0]
    lanes = []
    for j in range(16):
        v, s = np.zeros(p.shape[1:], np.float32), j
        while s + 48 < split:
            v = v + ((p[s] + p[s + 16]) + (p[s + 32] + p[s + 48]))
            s += 64
        while s < split:
            v = v + p[s]
            s += 16
        lanes.append(v)
    r = lanes[0]
    for v in lanes[1:]:
        r = r + v
    return r


def out_hw(c):
    H = (c.h * c.up + 2 * c.pad - c.dil * (c.ksize - 1) - 1) // c.stride + 1
    W = (c.w * c.up + 2 * c.pad - c.dil * (c.ksize - 1) - 1) // c.stride + 1
    return H, W


def plan_of(c):
    """(bm, bn, split, pix_per_split) from the library's planner for this case."""
    from bts_amd import ops
    nb = max(c.n_bundles, 1)
    return ops.conv_wgrad_plan(c.B, c.h, c.w, c.c_in, c.c_out, c.ksize, dil=c.dil, stride=c.stride, pad=c.pad, up=c.up,
                               ws_floats=c.ws_floats, n_bundles=c.n_bundles, pre=c.pre, pre_relu=c.pre_relu,
                               x_pix_stride=nb * c.c_in + c.x_extra, dy_pix_stride=nb * c.c_out + c.dy_extra)
