"""One case table for tests/test_conv_cases_host.py (CPU: which kernel the dispatch gives each case, that the table as a
whole reaches every kernel family, tile, flag, ragged edge and epilogue, and that every case keeps fp32 exact) and
tests/test_conv_exact_gpu.py (GPU: every case bit-exact against an fp64 statement of the fused convolution).

The shapes were picked with conv_plan.query (bts_conv_plan_f32), the smallest that reach each item; nothing here forces
a kernel -- the host test fails, naming the item, when the dispatch stops choosing it.  Every gate of the dispatch depends
on per-frame geometry and the declared fill_frames, never on B, so tiny maps reach everything.

    python tests/conv_cases.py [name ...]      # one JSON object {name: plan} for the named (default: all) cases
"""
import zlib
from collections import namedtuple

ConvCase = namedtuple("ConvCase", "name B h w c_in c_out ksize dil stride pad up subpixel n_bundles n_tail nchw fill_frames "
                                  "precision ws_floats pre pre_relu e1 res act e2 y2 x_extra y_extra")

PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16": 2}
ACTS = {"none": 0, "relu": 1, "elu": 2, "sigmoid": 3}
KI = 1 << 10


def _c(name, B, h, w, c_in, c_out, ksize, dil=1, stride=1, pad=None, up=1, subpixel=False, n_bundles=1, n_tail=0, nchw=False,
       fill_frames=0, precision="fp32", ws_floats=None, pre=False, pre_relu=False, e1=False, res=False, act="none", e2=False,
       y2=False, x_extra=0, y_extra=0):
    """c_in = channels the kernel walks per tap and bundle (bts_conv_desc.c_in_ld, a multiple of 4; with n_tail the last
    four are the planar tail, so the NHWC buffer holds c_in - 4); c_out per bundle.  subpixel: ksize 3 / up 2, as
    conv_forward takes it.  x_extra / y_extra: channels of the wider buffer the view is a slice of (a multiple of 8: half in
    front of the slice, half behind; y2 and res sit in buffers of their own, as wide as y's).  ws_floats None = no
    split-K workspace."""
    if subpixel:
        ksize, up = 3, 2
    return ConvCase(name, B, h, w, c_in, c_out, ksize, dil, stride, dil * (ksize // 2) if pad is None else pad, up, subpixel,
                    n_bundles, n_tail, nchw, fill_frames, precision, ws_floats, pre, pre_relu, e1, res, act, e2, y2, x_extra, y_extra)


EPI = dict(e1=True, act="relu", e2=True)                      # the fast NHWC epilogue with everything it fuses
GEN = dict(e1=True, res=True, act="relu", e2=True)            # `res` forces the general epilogue
PRE = dict(pre=True, pre_relu=True)

CASES = [
    # ---- row tiles (conv_fwd_kernel<bm,bn>): bn by c_out, bm by the tile rounds of M (choose_tile)
    _c("row128x128_k1", 1, 33, 63, 32, 1024, 1, **EPI),                           # M 2079 = 16.2 tiles
    _c("row128x128_k1_gen_b3", 3, 33, 21, 32, 1000, 1, y_extra=8, **GEN),          # c_out % 128 != 0, three frames
    _c("row128x128_nchw", 1, 33, 63, 32, 1024, 1, nchw=True, act="relu"),
    _c("row64x128_k1", 1, 5, 7, 32, 128, 1, **EPI),                               # M 35: less than one tile
    _c("row64x128_k5_gen", 3, 5, 7, 16, 100, 5, x_extra=8, y_extra=8, **GEN),      # c_in_ld % 32 != 0: the non-lean gather
    _c("row64x128_nchw_k7", 2, 9, 6, 8, 128, 7, nchw=True, e1=True, act="relu"),
    _c("row128x64_k1", 1, 52, 64, 32, 320, 1, **EPI),
    _c("row128x64_gen_s2", 3, 66, 68, 32, 300, 3, stride=2, **GEN),                # stride 2: M 3366 = 26.3 tiles, c_out 4.7 tiles
    _c("row128x64_nchw", 1, 52, 64, 32, 320, 1, nchw=True),
    _c("row64x64_k1", 1, 5, 7, 32, 64, 1, y2=True, **EPI),                         # y2 without split-K
    _c("row64x64_gen_pre", 3, 5, 7, 32, 40, 3, x_extra=16, y_extra=8, y2=True, **GEN, **PRE),
    _c("row64x64_up2", 2, 5, 7, 32, 64, 3, up=2, **EPI),                           # folded nearest-2x gather
    _c("row64x64_dil24", 1, 9, 11, 32, 64, 3, dil=24, **EPI),                      # dilation larger than the map
    _c("row64x64_tapskip", 1, 9, 11, 32, 64, 3, dil=6, **EPI),                     # tap skipping: issued 12 of 18
    _c("row64x64_subpixel", 1, 3, 5, 32, 64, 3, subpixel=True, **EPI),             # 3x5 fills the halo tile too thinly
    _c("row64x64_subpixel_gen", 2, 3, 5, 36, 40, 3, subpixel=True, **GEN),
    _c("row64x64_nchw", 2, 5, 7, 32, 64, 3, nchw=True, act="relu"),
    _c("row64x64_bundles", 3, 6, 8, 64, 64, 3, n_bundles=3, stride=2, **EPI),      # bundles on a 64-wide tile
    _c("row64x64_bundles_gen", 2, 6, 8, 32, 64, 3, n_bundles=2, **GEN),
    _c("row128x48_k1", 1, 75, 73, 32, 144, 1, **EPI),
    _c("row128x48_gen", 3, 45, 41, 32, 144, 1, y_extra=8, **GEN),
    _c("row128x48_nchw", 1, 75, 73, 32, 144, 1, nchw=True, act="relu"),
    _c("row64x48_k3", 2, 5, 7, 36, 48, 3, **EPI),
    _c("row64x48_gen_pre", 3, 5, 7, 36, 48, 3, pre=True, **GEN),                   # prologue without ReLU
    _c("row64x48_nchw", 2, 5, 7, 36, 48, 3, nchw=True),
    _c("row128x32_k1", 1, 5, 7, 32, 32, 1, **EPI),
    _c("row128x32_gen", 3, 15, 11, 36, 24, 3, x_extra=8, y_extra=16, **GEN),       # M 495, c_out 24
    _c("row128x32_nchw", 2, 5, 7, 32, 32, 1, nchw=True, act="relu"),
    _c("row128x32_bundles_s2", 2, 6, 8, 32, 32, 3, n_bundles=4, stride=2, **EPI),
    _c("row128x32_bundles_gen", 3, 6, 8, 32, 32, 3, n_bundles=4, y2=True, **GEN),
    # ---- split-K (a workspace lent): partials to the workspace, splitk_reduce_kernel applies the epilogue
    _c("split64x64", 1, 5, 7, 512, 64, 3, ws_floats=64 * KI, **EPI),
    _c("split64x64_gen_y2_b3", 3, 5, 7, 512, 40, 3, ws_floats=64 * KI, y2=True, y_extra=8, **GEN),
    _c("split64x64_nchw", 2, 5, 7, 512, 64, 3, ws_floats=64 * KI, nchw=True, act="relu"),
    _c("split64x128", 1, 5, 7, 512, 128, 3, ws_floats=64 * KI, **EPI),
    _c("split64x128_nchw", 1, 5, 7, 512, 128, 3, ws_floats=64 * KI, nchw=True),
    _c("split64x128_k1_pre", 2, 5, 7, 512, 100, 1, ws_floats=64 * KI, **GEN, **PRE),
    _c("split128x32", 1, 5, 7, 512, 32, 3, ws_floats=64 * KI, **EPI),
    _c("split128x32_nchw", 2, 5, 7, 512, 24, 3, ws_floats=64 * KI, nchw=True),
    _c("split64x48", 1, 5, 7, 512, 48, 3, ws_floats=64 * KI, **EPI),
    _c("split64x48_nchw", 1, 5, 7, 512, 48, 3, ws_floats=64 * KI, nchw=True),
    _c("split_halo_map", 1, 8, 32, 36, 128, 3, ws_floats=64 * KI, **EPI),           # the halo map below, a workspace lent
    # ---- halo tiles (conv_halo_kernel<bn,k3|k2>): 4 rows x 32 pixels (8 x 16 for bn 48), map fill >= 0.80
    _c("halo128_k3", 1, 8, 32, 36, 128, 3, **EPI),
    _c("halo128_k3_ws_fill4096", 1, 8, 32, 36, 128, 3, ws_floats=64 * KI, fill_frames=4096, **EPI),
    _c("halo128_k3_gen_b3", 3, 7, 30, 36, 100, 3, x_extra=8, y_extra=8, y2=True, **GEN, **PRE),
    _c("halo128_k3_nchw", 2, 7, 30, 36, 128, 3, nchw=True, act="relu"),
    _c("halo64_k3", 1, 8, 32, 36, 64, 3, **EPI),
    _c("halo64_k3_gen_b3", 3, 7, 61, 36, 40, 3, y_extra=8, **GEN),
    _c("halo64_k3_nchw", 2, 7, 30, 36, 64, 3, nchw=True),
    _c("halo32_k3", 1, 8, 32, 36, 32, 3, **EPI),
    _c("halo32_k3_gen_b3", 3, 7, 61, 36, 24, 3, pre=True, **GEN),
    _c("halo32_k3_nchw", 2, 7, 30, 36, 32, 3, nchw=True, act="relu"),
    _c("halo48_k3", 1, 8, 16, 36, 48, 3, **EPI),
    _c("halo48_k3_gen_b3", 3, 7, 45, 36, 96, 3, y_extra=8, **GEN),
    _c("halo48_k3_nchw", 2, 15, 14, 36, 48, 3, nchw=True),
    _c("halo128_k2", 1, 4, 31, 36, 128, 3, subpixel=True, **EPI),
    _c("halo128_k2_gen_b3", 3, 7, 30, 36, 100, 3, subpixel=True, y_extra=8, **GEN),
    _c("halo64_k2", 1, 4, 31, 36, 64, 3, subpixel=True, y2=True, **EPI),
    _c("halo64_k2_gen", 2, 7, 61, 36, 40, 3, subpixel=True, **GEN, **PRE),
    _c("halo32_k2", 1, 4, 31, 36, 32, 3, subpixel=True, **EPI),
    _c("halo32_k2_gen_b3", 3, 7, 30, 40, 24, 3, subpixel=True, **GEN),
    _c("halo128_dil3", 2, 23, 30, 32, 128, 3, dil=3, **EPI),
    _c("halo128_dil3_gen_b3", 3, 11, 61, 36, 100, 3, dil=3, y_extra=8, **GEN, **PRE),
    # ---- planar tail (conv_halo_kernel<bn,k3,tail>): whatever the map
    _c("tail128", 1, 8, 32, 40, 128, 3, n_tail=1, **EPI),                         # c_in - 4 = 36: no Winograd form
    _c("tail128_gen_b3", 3, 7, 30, 40, 100, 3, n_tail=4, x_extra=8, y_extra=8, **GEN),
    _c("tail64_nchw", 1, 7, 31, 40, 64, 3, n_tail=3, nchw=True, act="relu"),
    _c("tail64", 2, 5, 33, 36, 64, 3, n_tail=2, **EPI),
    _c("tail64_gen_b3", 3, 9, 14, 40, 40, 3, n_tail=1, **GEN),
    _c("tail32", 1, 3, 5, 12, 32, 3, n_tail=2, **EPI),
    _c("tail32_gen_b3", 3, 5, 35, 12, 24, 3, n_tail=3, y2=True, **GEN),
    _c("tail32_nchw", 2, 6, 9, 12, 32, 3, n_tail=4, nchw=True),
    _c("tail128_nchw", 2, 6, 33, 36, 128, 3, n_tail=2, nchw=True),
    # ---- Winograd F(2x2,3x3) (conv_wino_kernel<bn>): 8 rows x 16 pixels, map fill >= 0.70, NHWC only, one epilogue
    _c("wino128", 1, 8, 16, 32, 128, 3, **EPI),
    _c("wino128_gen_b3", 3, 7, 29, 32, 100, 3, x_extra=8, y_extra=8, y2=True, **GEN, **PRE),
    _c("wino64", 2, 15, 30, 64, 64, 3, **EPI),
    _c("wino64_gen_b3", 3, 7, 15, 32, 40, 3, y_extra=8, **GEN),
    _c("wino48", 1, 7, 15, 64, 48, 3, **EPI),
    _c("wino48_gen_b3", 3, 15, 29, 32, 96, 3, y_extra=8, pre=True, **GEN),
    _c("wino128_tail", 1, 8, 16, 36, 128, 3, n_tail=2, **EPI),
    _c("wino128_tail_gen_b3", 3, 7, 29, 36, 128, 3, n_tail=4, y_extra=8, **GEN),
    _c("wino64_tail", 1, 7, 14, 36, 64, 3, n_tail=4, **EPI),
    _c("wino64_tail_gen_b3", 3, 15, 13, 36, 64, 3, n_tail=1, y2=True, **GEN),
    # ---- wide 1x1 (conv1x1_kernel<192,2|4>): a chip-filling declared launch, c_out % 192 == 0
    _c("wide1x1_rows64", 1, 5, 7, 64, 192, 1, fill_frames=4096, **EPI),
    _c("wide1x1_rows64_gen_b3", 3, 9, 11, 36, 384, 1, fill_frames=4096, x_extra=8, y_extra=8, y2=True, **GEN, **PRE),
    _c("wide1x1_rows128", 1, 5, 7, 800, 192, 1, fill_frames=4096, **EPI),
    _c("wide1x1_rows128_gen_b3", 3, 9, 15, 772, 192, 1, fill_frames=4096, **GEN),
    # ---- the encoder stem (conv_stem_kernel<96|64>): 7x7 / stride 2 on the 4-channel image, 8 x 32 output tiles; it has
    # no general epilogue (a residual or sigmoid sends the layer to the row tiles)
    _c("stem96", 2, 20, 36, 4, 96, 7, stride=2, pad=3, **EPI),
    _c("stem96_b3_y2", 3, 9, 70, 4, 96, 7, stride=2, pad=3, y2=True, y_extra=8, e1=True, act="relu"),
    _c("stem64", 1, 17, 67, 4, 64, 7, stride=2, pad=3, **EPI),
    _c("stem64_b3", 3, 20, 36, 4, 64, 7, stride=2, pad=3, y_extra=8),
    _c("stem_res_goes_row", 1, 17, 67, 4, 64, 7, stride=2, pad=3, **GEN),
    # ---- precision bf16x3 (fp32 emulated on the bf16 matrix cores): halo_emu tiles of 4 rows x 32 pixels, row tiles
    _c("emu_halo128_k3", 1, 8, 32, 32, 128, 3, precision="bf16x3", **EPI),
    _c("emu_halo128_k3_gen_b3", 3, 7, 30, 32, 100, 3, precision="bf16x3", x_extra=8, y_extra=8, y2=True, **GEN, **PRE),
    _c("emu_halo64_k3", 2, 7, 30, 64, 64, 3, precision="bf16x3", **EPI),
    _c("emu_halo64_k3_cout48", 2, 7, 30, 64, 48, 3, precision="bf16x3", **GEN),      # no 48-wide twin: padded to 64
    _c("emu_halo128_k2", 1, 4, 31, 32, 128, 3, subpixel=True, precision="bf16x3", **EPI),
    _c("emu_halo64_k2_gen_b3", 3, 7, 30, 32, 40, 3, subpixel=True, precision="bf16x3", **GEN),
    # three 32-channel chunks: the next chunk's patch trickles into the buffer the consumers are not reading, twice over
    _c("emu_halo128_k3_chunks3", 2, 7, 30, 96, 128, 3, precision="bf16x3", **EPI, **PRE),
    _c("emu_halo64_k2_chunks3", 1, 4, 31, 96, 64, 3, subpixel=True, precision="bf16x3", **GEN),
    _c("emu_row64x64_k1", 1, 5, 7, 32, 64, 1, precision="bf16x3", **EPI),
    _c("emu_row128x128_nchw", 1, 33, 63, 32, 1024, 1, precision="bf16x3", nchw=True),
    _c("emu_row128x32_gen", 3, 15, 11, 36, 24, 3, precision="bf16x3", **GEN),
    _c("emu_split64x64", 1, 5, 7, 512, 64, 3, precision="bf16x3", ws_floats=64 * KI, **EPI),
    _c("emu_stem_goes_row", 1, 17, 67, 4, 64, 7, stride=2, pad=3, precision="bf16x3", **EPI),
    # ---- precision bf16 (operands rounded to nearest even, fp32 accumulation): one-plane halo tiles, row tiles ",bf16"
    _c("bf16_halo128_k3", 1, 8, 32, 32, 128, 3, precision="bf16", **EPI),
    _c("bf16_halo64_k3_gen_b3", 3, 7, 30, 64, 48, 3, precision="bf16", y_extra=8, **GEN, **PRE),
    _c("bf16_halo128_k2_gen", 2, 7, 30, 32, 100, 3, subpixel=True, precision="bf16", **GEN),
    _c("bf16_halo64_k2", 1, 4, 31, 32, 64, 3, subpixel=True, precision="bf16", **EPI),
    _c("bf16_halo64_k3_chunks3", 2, 7, 30, 96, 64, 3, precision="bf16", **GEN, **PRE),
    _c("bf16_halo128_k2_chunks3", 1, 4, 31, 96, 128, 3, subpixel=True, precision="bf16", **EPI),
    _c("bf16_row128x128", 1, 33, 63, 32, 1000, 1, precision="bf16", **EPI),
    _c("bf16_row64x128_nchw", 1, 5, 7, 32, 100, 1, precision="bf16", nchw=True),
    _c("bf16_row128x64_gen", 1, 51, 65, 32, 300, 1, precision="bf16", **GEN),
    _c("bf16_row64x64_pre", 3, 5, 7, 32, 40, 3, precision="bf16", **GEN, **PRE),
    _c("bf16_row128x32", 1, 5, 7, 32, 24, 1, precision="bf16", **EPI),
    _c("bf16_split64x64", 1, 5, 7, 512, 64, 3, precision="bf16", ws_floats=64 * KI, **EPI),
    _c("bf16_stem_stays_fp32", 1, 17, 67, 4, 64, 7, stride=2, pad=3, precision="bf16", **EPI),
]

# The dilated halo tiles at dilation 6 and 12 are opt-in (BTS_CONV_HALO_DIL=2, read once per process): planned and run in
# a child process that sets it
DIL2_ENV = {"BTS_CONV_HALO_DIL": "2"}
DIL2_CASES = [
    _c("halo128_dil6", 2, 23, 30, 32, 128, 3, dil=6, **EPI),
    _c("halo128_dil6_gen_b3", 3, 23, 61, 36, 100, 3, dil=6, y_extra=8, **GEN, **PRE),
    _c("halo128_dil12", 1, 47, 30, 32, 128, 3, dil=12, y2=True, **GEN),
]

BY_NAME = {c.name: c for c in CASES + DIL2_CASES}

# ELU / sigmoid cannot be exact: one NHWC case per family that has an epilogue of its own, one NCHW case on the row and
# halo tiles (tests/test_conv_exact_gpu.py::test_conv_float_activations)
FLOAT_CASES = ["row64x64_k1", "row64x64_nchw", "split64x64", "halo64_k3", "halo64_k3_nchw", "tail128", "wino128", "wide1x1_rows64",
               "stem96", "emu_halo128_k3"]


def round_up(v, m):
    return (v + m - 1) // m * m


def out_hw(c):
    """Output extent [H, W] (sub-pixel: of the full 2h x 2w output)."""
    if c.subpixel:
        return 2 * c.h, 2 * c.w
    return ((c.h * c.up + 2 * c.pad - c.dil * (c.ksize - 1) - 1) // c.stride + 1,
            (c.w * c.up + 2 * c.pad - c.dil * (c.ksize - 1) - 1) // c.stride + 1)


def channels(c):
    """(NHWC buffer channels of x, c_out_pad, output channels), over all bundles."""
    nb = max(c.n_bundles, 1)
    return nb * (c.c_in - (4 if c.n_tail else 0)), round_up(c.c_out, 32), nb * c.c_out


def wants_wino_weights(c, precision):
    """ops._conv_derived_weights' condition for handing the library Winograd-form weights."""
    from bts_amd import ops
    c_main = c.c_in - (4 if c.n_tail else 0)
    return (ops._WINO and precision == 0 and c.ksize == 3 and c.stride == 1 and c.dil == 1 and c.pad == 1 and c.up == 1
            and not c.subpixel and c.n_bundles <= 1 and c_main % 32 == 0 and c.c_in > 4 and not c.nchw)


def effective_precision(c):
    """The precision conv_forward declares for this case: BTS_CONV_PRECISION=1 turns every launch into bf16x3."""
    from bts_amd import ops
    return 1 if ops._ENV_PRECISION else PRECISIONS[c.precision]


def plan_of(c, B=None):
    """conv_plan.query on the descriptor conv_forward would build for this case: the same integers, and non-null fake
    pointers exactly where ops._conv_describe / ops._conv_derived_weights / the caller's workspace set real ones."""
    from bts_amd import conv_plan
    P = 0x10000
    prec = effective_precision(c)
    x_ch, c_out_pad, y_ch = channels(c)
    d = conv_plan.geometry_desc(c.B if B is None else B, c.h, c.w, c.c_in, c.c_out, c.ksize, c.dil, c.stride, c.pad, c.up,
                                c.subpixel, c.n_bundles, c.n_tail, c.nchw, c.fill_frames, prec, x_pix_stride=x_ch + c.x_extra,
                                y_pix_stride=0 if c.nchw else y_ch + c.y_extra, c_out_pad=c_out_pad, fake_pointers=True)
    if c.pre:
        d.pre_scale = d.pre_shift = P
    d.pre_relu, d.act = int(c.pre_relu), ACTS[c.act]
    if c.e1:
        d.e1_scale = d.e1_shift = P
    if c.e2:
        d.e2_scale = d.e2_shift = P
    if c.y2:
        d.y2, d.y2_pix_stride = P, y_ch + c.y_extra
    if c.res:
        d.res, d.res_pix_stride = P, y_ch + c.y_extra
    if prec in (1, 2) and c.n_bundles <= 1 and not c.n_tail:
        d.w_split = P
    if wants_wino_weights(c, prec):
        d.w_wino = P
    if c.ws_floats is not None:
        d.splitk_ws, d.splitk_ws_floats = P, c.ws_floats
    return conv_plan.query(d, ksteps=True)


def rounds_to_bf16(c, plan):
    """Does this launch round its operands to bf16?  Only the bf16 kernel families do: under precision 2 the stem stays
    on its fp32 kernel (and BTS_CONV_PRECISION=1 turns the whole launch into bf16x3, which is exact on these operands)."""
    from bts_amd.conv_plan import Family
    return plan.family in (Family.ROW_BF16, Family.HALO_BF16)


# ---------------------------------------------------------------------------------------------- operands and reference
# 271 and up: odd values need nine bits or more, which bf16 does not hold (every bf16x3 / bf16 case stays there); the
# lower rungs are for Winograd plans with a prologue and both affines, whose transform-domain bound is 36x the direct one
XMAX_LADDER = (511, 447, 383, 319, 271, 191, 127, 95)

Operands = namedtuple("Operands", "xmax x w tail pre e1 res e2")


def _draw(c, xmax, wino, e1_pow2=None):
    import torch
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    x_ch, c_out_pad, y_ch = channels(c)
    nb = max(c.n_bundles, 1)
    H, W = out_hw(c)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    scales = lambda n: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]
    pre = None
    if c.pre:                                  # even x, so that a scale of 0.5 keeps it integral
        x = 2.0 * ri(-(xmax // 2), xmax // 2, (c.B, c.h, c.w, x_ch))
        pre = (scales(nb * c.c_in), ri(-9, 9, (nb * c.c_in,)))
        pre[1][0], pre[1][1] = -7.0, 5.0       # a shift that leaks into the zero padding changes the result: the negative
        #                                        one without ReLU, the positive one with it
    else:
        x = ri(-xmax, xmax, (c.B, c.h, c.w, x_ch))
    c_real = c.c_in - (4 - c.n_tail if c.n_tail else 0)          # weights of the unused tail slots are zero (pack_conv_weight)
    w = ri(-1, 1, (nb, c.c_out, c_real, c.ksize, c.ksize)) * 4.0 if wino else ri(-3, 3, (nb, c.c_out, c_real, c.ksize, c.ksize))
    tail = ri(-xmax, xmax, (c.n_tail, c.B, c.h, c.w)) if c.n_tail else None
    e1 = e2 = res = None
    if e1_pow2 is not None:
        e1 = (torch.full((y_ch,), 2.0 ** -e1_pow2, dtype=torch.float64), torch.zeros(y_ch, dtype=torch.float64))
    elif c.e1:
        e1 = (scales(y_ch), ri(-9, 9, (y_ch,)))
    if c.res:
        res = ri(-xmax, xmax, (c.B, H, W, y_ch))
    if c.e2:
        e2 = (scales(y_ch), ri(-9, 9, (y_ch,)))
    return Operands(xmax, x, w, tail, pre, e1, res, e2)


def reference(c, o, bf16=False, act=None):
    """fp64, from the definition: prologue -> nearest-2x -> zero padding after the prologue -> conv2d per bundle -> e1 ->
    + res -> act -> e2.  Returns (y [B, H, W, channels], pre-activation, magnitude bound in units of the smallest dyadic
    step any intermediate can have): the bound is sum |w| * |x_tap| carried through e1, res and e2 -- for a Winograd
    plan taken in the transform domain instead (see wino_bound)."""
    import torch
    import torch.nn.functional as F
    nb = max(c.n_bundles, 1)
    act = c.act if act is None else act
    x = o.x
    if o.tail is not None:                     # the planes are the last channels of the reference's concatenated input
        x = torch.cat([x, o.tail.permute(1, 2, 3, 0)], dim=-1)
    if o.pre is not None:
        n = x.shape[-1]
        x = x * o.pre[0][:n] + o.pre[1][:n]
        if c.pre_relu:
            x = x.clamp_min(0.0)
    w = o.w
    if bf16:
        x, w = x.float().bfloat16().double(), w.float().bfloat16().double()
    if c.up == 2:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    xn = x.permute(0, 3, 1, 2)
    cb = xn.shape[1] // nb
    kw = dict(stride=c.stride, padding=c.pad, dilation=c.dil)
    y = torch.cat([F.conv2d(xn[:, j * cb:(j + 1) * cb], w[j], **kw) for j in range(nb)], dim=1).permute(0, 2, 3, 1)
    mag = torch.cat([F.conv2d(xn[:, j * cb:(j + 1) * cb].abs(), w[j].abs(), **kw) for j in range(nb)], dim=1).permute(0, 2, 3, 1)
    unit = torch.ones(y.shape[-1], dtype=torch.float64)
    worst = mag.max().item()
    if o.e1 is not None:
        y, mag = y * o.e1[0] + o.e1[1], mag * o.e1[0].abs() + o.e1[1].abs()
        unit = unit * o.e1[0].clamp_max(1.0)
        worst = max(worst, (mag / unit).max().item())
    if o.res is not None:
        y, mag = y + o.res, mag + o.res.abs()
        worst = max(worst, (mag / unit).max().item())
    pre_act = y
    if act == "relu":
        y = y.clamp_min(0.0)
    elif act == "elu":
        y = torch.where(y > 0, y, torch.expm1(y))
    elif act == "sigmoid":
        y = torch.sigmoid(y)
    if o.e2 is not None:
        y, mag = y * o.e2[0] + o.e2[1], mag * o.e2[0].abs() + o.e2[1].abs()
        unit = unit * o.e2[0].clamp_max(1.0)
        worst = max(worst, (mag / unit).max().item())
    return y, pre_act, worst


def wino_bound(c, o):
    """The Winograd kernel's own intermediates: V = B^T d B has |V| <= 4 max|x| (after the prologue), U = G g G^T has
    |U| <= 2.25 max|w| (integral, because w is a multiple of 4), the products are summed over the c_in - 4 * (n_tail > 0)
    buffer channels and the output transform adds nine of those sums; the tail planes add 9 * max|w| * max|plane| each,
    directly.  Carried through e1, res and e2 like the direct bound, in the same units."""
    import torch
    x = o.x
    if o.pre is not None:
        n = x.shape[-1]
        x = x * o.pre[0][:n] + o.pre[1][:n]
    c_main = c.c_in - (4 if c.n_tail else 0)
    wmax = o.w.abs().max().item()
    m = 9.0 * c_main * (4.0 * x.abs().max().item()) * (2.25 * wmax)
    if o.tail is not None:
        m += 9.0 * wmax * o.tail.abs().max().item() * c.n_tail
    m = torch.full((o.w.shape[0] * o.w.shape[1],), m, dtype=torch.float64)          # per output channel from here on
    unit = torch.ones_like(m)
    worst = m.max().item()
    for pair, add in ((o.e1, o.res), (o.e2, None)):
        if pair is not None:
            m = m * pair[0].abs() + pair[1].abs()
            unit = unit * pair[0].clamp_max(1.0)
        if add is not None:
            m = m + add.abs().max().item()
        worst = max(worst, (m / unit).max().item())
    return worst


def operands(c, plan=None, e1_pow2=None):
    """The integer operands of a case: |x| <= 511 (or the largest rung of XMAX_LADDER that keeps the case exact), w in
    +-3 (multiples of 4 where the library gets Winograd-form weights, so that G g G^T is integral), scales from
    {0.5, 1, 2}, integer shifts, residual and tail planes.  Returns (operands, worst magnitude / 2^24)."""
    from bts_amd.conv_plan import Family
    plan = plan_of(c) if plan is None else plan
    wino = wants_wino_weights(c, 0)
    for xmax in XMAX_LADDER:
        o = _draw(c, xmax, wino, e1_pow2)
        worst = reference(c, o)[2]
        if plan.family == Family.WINO:
            worst = max(worst, wino_bound(c, o))
        if worst < 2 ** 24:
            break
    return o, worst / 2 ** 24


def main(argv):
    import json
    names = argv or [c.name for c in CASES]
    print(json.dumps({n: list(plan_of(BY_NAME[n])) for n in names}))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(sys.argv[1:])
