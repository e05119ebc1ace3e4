"""One case table for tests/test_upconv_train_host.py (CPU: which tile and split the planner gives each weight-gradient
case, and that the table reaches every tile both split and unsplit) and tests/test_upconv_train_gpu.py (GPU: every case
bit-exact against the fp64 statement ops.upconv_subpixel_grads_reference).

The shapes were picked with ops.upconv_wgrad_plan (bts_upconv_wgrad_plan_f32), the cheapest that reach each item;
nothing here forces a tile -- the host test fails, naming the item, when the planner stops choosing it.  M = B*h*w
source pixels, N = 4*c_in columns, four classes; "unsplit" cases get exactly the 16*c_out*c_in floats the class results
need (the planner then cannot split), or have fewer than 256 pixels."""
from collections import namedtuple

MI = 1 << 20

WgradCase = namedtuple("WgradCase", "name B h w c_in c_out x_extra dy_extra ws_floats tile split")


def _c(name, B, h, w, c_in, c_out, tile, split, ws_floats=None, x_extra=0, dy_extra=0):
    """ws_floats None = exactly 16*c_out*c_in.  x_extra / dy_extra: channels of the wider NaN-filled buffer the slice sits
    in (a multiple of 8).  tile = (bm, bn) and split (True: more than one) are what the case was chosen for."""
    return WgradCase(name, B, h, w, c_in, c_out, x_extra, dy_extra, 16 * c_out * c_in if ws_floats is None else ws_floats, tile, split)


WGRAD_CASES = [
    _c("t128_unsplit_1step", 1, 4, 5, 4096, 100, (128, 128), False),                  # M 20: one K-step; c_out % 128 != 0
    _c("t128_s4", 2, 44, 88, 1024, 100, (128, 128), True, ws_floats=16 * 100 * 1024 * 4),   # M 7744: the workspace caps the split at 4
    _c("t64x128_unsplit", 1, 4, 5, 512, 512, (64, 128), False),
    _c("t64x128_s2", 1, 13, 20, 1024, 100, (64, 128), True, ws_floats=16 * 100 * 1024 * 2, dy_extra=8),   # M 260, ragged rows
    _c("t32_unsplit", 1, 4, 5, 4096, 32, (32, 128), False),
    _c("t32_s16", 2, 30, 41, 128, 32, (32, 128), True, ws_floats=2 * MI, x_extra=8),  # M 2460, odd W
    _c("t64_unsplit_ragged", 2, 6, 9, 48, 40, (64, 64), False, x_extra=8, dy_extra=8),   # M 108: ragged everywhere, odd W
    _c("t64_unsplit_1step", 3, 5, 7, 128, 64, (64, 64), False),                       # M 105, three frames
    _c("t64_s2", 1, 13, 20, 128, 32, (64, 64), True, ws_floats=16 * 32 * 128 * 2),    # M 260: 4 pixels in the last K-step
    _c("t64_w1_h1", 5, 1, 1, 16, 8, (64, 64), False),                                 # a 1x1 map: every tap but one is padding
    _c("t64_s160", 4, 64, 80, 16, 8, (64, 64), True, ws_floats=4 * MI),               # M 20480: 160 splits of 128 pixels, the
                                                                                      # fold's four-at-a-time loop plus its tail
]

BY_NAME = {c.name: c for c in WGRAD_CASES}

# float-valued test: one split case per tile, and the 160-split case (the only one in the fold's four-at-a-time loop)
WGRAD_FLOAT_CASES = ["t128_s4", "t64x128_s2", "t32_s16", "t64_s2", "t64_s160"]

# input gradient: (B, h, w, c_in, c_out)
DGRAD_CASES = [
    (2, 6, 9, 48, 40),          # ragged tiles, odd W
    (1, 13, 20, 64, 32),
    (3, 5, 7, 128, 64),
    (1, 4, 5, 512, 256),        # K = 4096 on 20 pixels: the split-K regime
]
DGRAD_SPLITK_WS = 16 * MI       # train.SPLITK_WS_FLOATS

# the forward / input-gradient packs: weight shapes [c_out, c_in, 3, 3]
PACK_SHAPES = [(40, 48), (32, 64), (512, 2208)]


def plan_of(c):
    """(bm, bn, split, pix_per_split) from the library's planner for this weight-gradient case."""
    from bts_amd import ops
    return ops.upconv_wgrad_plan(c.B, c.h, c.w, c.c_in, c.c_out, c.ws_floats)
