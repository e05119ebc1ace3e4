"""CPU: host side of the bf16 inference mode (bts_conv_desc.precision = 2) -- the launch declaration and the kernel
choice, through the library's host-side plan query (no GPU work: the pointers are never dereferenced)."""
import os

import pytest

from bts_amd import conv_plan, ops
from bts_amd._lib import BtsHipError
from bts_amd.conv_plan import Family, Flag

# libbts_hip.so reads BTS_CONV_PRECISION as an override of every descriptor: these tests pin precision 2 itself
pytestmark = pytest.mark.skipif(os.environ.get("BTS_CONV_PRECISION", "").strip() not in ("", "0"),
                                reason="BTS_CONV_PRECISION overrides the descriptor's precision")

def test_launch_config_accepts_bf16_only():
    assert ops.current_launch_config() == (0, 0)
    with ops.launch_config(precision="bf16"):
        assert ops.current_launch_config() == (0, 2)
        with ops.launch_config(precision="fp32"):
            assert ops.current_launch_config() == (0, 0)
        assert ops.current_launch_config() == (0, 2)
    with ops.launch_config(fill_frames=4, precision=2):
        assert ops.current_launch_config() == (4, 2)
    for bad in ("fp16", "bfloat16", 3):
        with pytest.raises(BtsHipError):
            ops.launch_config(precision=bad)


def _plan(cin, cout, h, w, k=3, stride=1, dil=1, precision=2, B=2, fill=16, subpixel=False, n_bundles=0, n_tail=0,
          wino=True, nchw=False, splitk=False, c_in_ld=None):
    d = _desc(cin, cout, h, w, k, stride, dil, precision, B, fill, subpixel, n_bundles, n_tail, nchw, c_in_ld)
    d.w_split = 0x3000                       # the one-plane weights the Python layer always supplies
    if wino:
        d.w_wino = 0x4000                    # offered: precision 2 must still never take Winograd
    if splitk:
        d.splitk_ws, d.splitk_ws_floats = 0x2000, 1 << 28
    p = conv_plan.query(d)
    assert p.rc == 0, p.rc
    return p.kind, p.bm, p.bn


def _desc(cin, cout, h, w, k=3, stride=1, dil=1, precision=2, B=2, fill=16, subpixel=False, n_bundles=0, n_tail=0,
          nchw=False, c_in_ld=None):
    return conv_plan.geometry_desc(B, h, w, c_in_ld or cin, cout, k, dil, stride, up=2 if subpixel else 1, subpixel=subpixel,
                                   n_bundles=n_bundles, n_tail=n_tail, nchw=nchw, fill_frames=fill, precision=precision,
                                   fake_pointers=True)


DECODER = {   # DenseNet161 / ResNeXt101 decoder at 352x1216 / 416x544 (per-frame maps of the layers)
    "upconv2 (sub-pixel, 44x152 -> 88x304)": (dict(cin=128, cout=64, h=44, w=152, subpixel=True), Family.HALO_BF16),
    "upconv3 (sub-pixel)": (dict(cin=256, cout=128, h=22, w=76 * 2, subpixel=True), Family.HALO_BF16),
    "conv4 (3x3, 44x152)": (dict(cin=384, cout=128, h=44, w=152), Family.HALO_BF16),
    "daspp_3 (dilation 3)": (dict(cin=448, cout=128, h=44, w=152, dil=3), Family.ROW_BF16),
    "daspp_24 (dilation 24)": (dict(cin=640, cout=128, h=44, w=152, dil=24), Family.ROW_BF16),
    "aspp 1x1 bottleneck": (dict(cin=640, cout=256, h=44, w=152, k=1), Family.ROW_BF16),
    "upconv5 tap GEMM (1x1, 11x38)": (dict(cin=2208, cout=9 * 512, h=11, w=38, k=1), Family.ROW_BF16),
    "conv3 (planar tail, 88x304)": (dict(cin=64, cout=64, h=88, w=304, n_tail=1, c_in_ld=64 + 4), Family.HALO_TAIL),
    "conv1 (planar tail, 352x1216)": (dict(cin=16, cout=32, h=352, w=1216, n_tail=4, c_in_ld=16 + 4), Family.HALO_TAIL),
}
ENCODER = {
    "stem (7x7 / 2 on the image)": (dict(cin=3, cout=96, h=352, w=1216, k=7, stride=2, c_in_ld=4), Family.STEM),
    "DenseNet growth conv (3x3, c_out 48)": (dict(cin=192, cout=48, h=88, w=304), Family.HALO_BF16),
    "DenseNet bottleneck (1x1, c_out 192)": (dict(cin=1248, cout=192, h=22, w=76, k=1), Family.ROW_BF16),
    "DenseNet transition (1x1)": (dict(cin=768, cout=384, h=88, w=304, k=1), Family.ROW_BF16),
    "ResNeXt grouped 3x3 bundles": (dict(cin=32, cout=32, h=52, w=68, n_bundles=8), Family.ROW_BF16),
    "ResNeXt strided 3x3 bundles": (dict(cin=32, cout=32, h=104, w=136, stride=2, n_bundles=16), Family.ROW_BF16),
    "ResNeXt 1x1 (104x136)": (dict(cin=256, cout=256, h=104, w=136, k=1), Family.ROW_BF16),
    "ResNeXt downsample 1x1 / 2": (dict(cin=512, cout=1024, h=52, w=68, k=1, stride=2), Family.ROW_BF16),
    "deep 3x3, split-K (13x17)": (dict(cin=1024, cout=128, h=13, w=17, fill=2, splitk=True), Family.ROW_BF16 | Flag.SPLITK),
}


@pytest.mark.parametrize("name", sorted(DECODER) + sorted(ENCODER))
def test_bf16_plan_kinds(name):
    """Precision 2 takes the bf16 kernels (ROW_BF16, HALO_BF16) for decoder and encoder layers, never WINO nor the fp32
    wide 1x1; the planar-tail layers stay on the fp32 halo kernel (HALO_TAIL), the stem on its fp32 kernel (STEM)."""
    geo, want = {**DECODER, **ENCODER}[name]
    kind, bm, bn = _plan(**geo)
    assert kind & conv_plan.FAMILY_MASK != Family.WINO
    assert kind & ~Flag.DIL == want, (name, kind, bm, bn)
    if want & conv_plan.FAMILY_MASK == Family.HALO_BF16:
        assert bn in (64, 128)                           # 48-wide growth convs padded to 64, as under precision 1


INT_FIELDS = ("x_pix_stride", "c_in_ld", "k_pad", "B", "h_in", "w_in", "up", "ksize", "dil", "stride", "pad", "c_out", "c_out_pad",
              "pre_relu", "act", "y_pix_stride", "y_nchw", "subpixel", "y2_pix_stride", "splitk_ws_floats", "res_pix_stride",
              "n_bundles", "precision", "n_tail", "fill_frames")


def test_geometry_desc_fills_the_fields_the_layer_tables_mean():
    """conv_plan.geometry_desc against the descriptor these layer tables stand for, every integer field written out by
    hand: K rounded up to 32 over 4 (sub-pixel) or k*k taps, padding dil*(k//2), the sub-pixel form as ksize 2 / pad 0 /
    up 1, pixel strides = the channels the layer reads and writes, fake non-null pointers."""
    for name, nchw in ((n, c) for n in {**DECODER, **ENCODER} for c in (False, True)):
        geo = {**DECODER, **ENCODER}[name][0]
        g = dict(dict(k=3, stride=1, dil=1, precision=2, B=2, fill=16, subpixel=False, n_bundles=0, n_tail=0, c_in_ld=None), **geo)
        g.pop("splitk", None)
        cin, cout, k, nb = g["cin"], g["cout"], g["k"], max(g["n_bundles"], 1)
        c_in_ld = g["c_in_ld"] or cin
        want = dict.fromkeys(INT_FIELDS, 0)
        want.update(c_in_ld=c_in_ld, x_pix_stride=max(cin, c_in_ld - 4 if g["n_tail"] else c_in_ld) * nb,
                    k_pad=((4 if g["subpixel"] else k * k) * c_in_ld + 31) // 32 * 32, B=g["B"], h_in=g["h"], w_in=g["w"], up=1,
                    ksize=2 if g["subpixel"] else k, dil=1 if g["subpixel"] else g["dil"], stride=1 if g["subpixel"] else g["stride"],
                    pad=0 if g["subpixel"] else g["dil"] * (k // 2), subpixel=int(g["subpixel"]), n_bundles=g["n_bundles"],
                    c_out=cout, c_out_pad=cout if g["n_bundles"] else (cout + 31) // 32 * 32, y_pix_stride=0 if nchw else cout * nb,
                    y_nchw=int(nchw), n_tail=g["n_tail"], fill_frames=g["fill"], precision=g["precision"])
        d = _desc(nchw=nchw, **g)
        assert {f: getattr(d, f) for f in INT_FIELDS} == want, name
        assert d.x == d.w == d.y == 0x1000 and [bool(t) for t in d.tail_planes] == [j < g["n_tail"] for j in range(4)], name
        assert not any((d.pre_scale, d.pre_shift, d.e1_scale, d.e1_shift, d.e2_scale, d.e2_shift, d.y2, d.splitk_ws, d.res,
                        d.w_split, d.w_wino)), name


def test_env_override_never_hands_a_one_plane_split_to_the_bf16x3_kernel():
    """BTS_CONV_PRECISION=1 overrides a precision-2 descriptor.  Its w_split is then ONE plane, while the bf16x3 halo tile
    (HALO_EMU) reads three: the library must ignore the buffer and fall back to the kernels that work from `w` alone.  A
    precision-1 descriptor with its own three-plane split keeps the bf16x3 halo tile under the same override.  (The knob
    is read once per process: a child process.)"""
    import json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import json, sys; sys.path[:0] = [%r, %r]; import test_bf16_host as T\n"
            "out = {}\n"
            "for name, (geo, want) in T.DECODER.items():\n"
            "    if want == T.Family.HALO_BF16:\n"
            "        out[name] = [T._plan(precision=p, **geo)[0] for p in (2, 1)]\n"
            "print(json.dumps(out))\n") % (here, os.path.dirname(here))
    env = dict(os.environ, BTS_CONV_PRECISION="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    kinds = json.loads(res.stdout.strip().splitlines()[-1])
    assert kinds, "no halo-tile layers in the table"
    for name, (k2, k1) in kinds.items():
        assert k2 & conv_plan.FAMILY_MASK == Family.ROW, (name, k2)          # precision-2 descriptor under the override: row-tiled bf16x3, w_split unused
        assert k1 & conv_plan.FAMILY_MASK == Family.HALO_EMU, (name, k1)     # precision-1 descriptor: its three planes, the bf16x3 halo tile


def test_precision_out_of_range_is_invalid():
    for p, ok in ((2, True), (3, False), (-1, False)):
        rc = conv_plan.query(conv_plan.geometry_desc(1, 1, 1, 32, 32, 1, precision=p, fake_pointers=True)).rc
        assert (rc == 0) == ok, (p, rc)
