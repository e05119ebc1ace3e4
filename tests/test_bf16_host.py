"""CPU: host side of the bf16 inference mode (bts_conv_desc.precision = 2) -- the launch declaration and the kernel
choice, through the library's host-side plan query (no GPU work: the pointers are never dereferenced)."""
import ctypes as C
import os

import pytest

from bts_amd import ops
from bts_amd._lib import BtsHipError

# libbts_hip.so reads BTS_CONV_PRECISION as an override of every descriptor: these tests pin precision 2 itself
pytestmark = pytest.mark.skipif(os.environ.get("BTS_CONV_PRECISION", "").strip() not in ("", "0"),
                                reason="BTS_CONV_PRECISION overrides the descriptor's precision")

HALO_BF16, ROW_BF16, TAIL_FP32, STEM_FP32, WINO = 8, 7, 2, 4, 6


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
    from bts_amd import _lib
    d = _lib.ConvDesc()
    d.x = d.w = d.y = 0x1000
    d.w_split = 0x3000                       # the one-plane weights the Python layer always supplies
    if wino:
        d.w_wino = 0x4000                    # offered: precision 2 must still never take Winograd
    if splitk:
        d.splitk_ws, d.splitk_ws_floats = 0x2000, 1 << 28
    c_in_ld = c_in_ld or cin
    d.c_in_ld = c_in_ld
    d.x_pix_stride = max(cin, c_in_ld - 4 if n_tail else c_in_ld) * max(n_bundles, 1)
    taps = 4 if subpixel else k * k
    d.k_pad = (taps * c_in_ld + 31) // 32 * 32
    d.B, d.h_in, d.w_in, d.up = B, h, w, 1
    d.ksize, d.dil, d.stride, d.pad = (2, 1, 1, 0) if subpixel else (k, dil, stride, dil * (k // 2))
    d.subpixel = int(subpixel)
    d.n_bundles = n_bundles
    d.c_out, d.c_out_pad = cout, (cout if n_bundles else (cout + 31) // 32 * 32)
    d.y_pix_stride = 0 if nchw else cout * max(n_bundles, 1)
    d.y_nchw = int(nchw)
    d.n_tail = n_tail
    for j in range(n_tail):
        d.tail_planes[j] = 0x5000
    d.fill_frames = fill
    d.precision = precision
    bm, bn, kind = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = _lib.load_real().bts_conv_plan_f32(C.byref(d), C.byref(bm), C.byref(bn), C.byref(kind))
    assert rc == 0, rc
    return kind.value, bm.value, bn.value


DECODER = {   # DenseNet161 / ResNeXt101 decoder at 352x1216 / 416x544 (per-frame maps of the layers)
    "upconv2 (sub-pixel, 44x152 -> 88x304)": (dict(cin=128, cout=64, h=44, w=152, subpixel=True), HALO_BF16),
    "upconv3 (sub-pixel)": (dict(cin=256, cout=128, h=22, w=76 * 2, subpixel=True), HALO_BF16),
    "conv4 (3x3, 44x152)": (dict(cin=384, cout=128, h=44, w=152), HALO_BF16),
    "daspp_3 (dilation 3)": (dict(cin=448, cout=128, h=44, w=152, dil=3), ROW_BF16),
    "daspp_24 (dilation 24)": (dict(cin=640, cout=128, h=44, w=152, dil=24), ROW_BF16),
    "aspp 1x1 bottleneck": (dict(cin=640, cout=256, h=44, w=152, k=1), ROW_BF16),
    "upconv5 tap GEMM (1x1, 11x38)": (dict(cin=2208, cout=9 * 512, h=11, w=38, k=1), ROW_BF16),
    "conv3 (planar tail, 88x304)": (dict(cin=64, cout=64, h=88, w=304, n_tail=1, c_in_ld=64 + 4), TAIL_FP32),
    "conv1 (planar tail, 352x1216)": (dict(cin=16, cout=32, h=352, w=1216, n_tail=4, c_in_ld=16 + 4), TAIL_FP32),
}
ENCODER = {
    "stem (7x7 / 2 on the image)": (dict(cin=3, cout=96, h=352, w=1216, k=7, stride=2, c_in_ld=4), STEM_FP32),
    "DenseNet growth conv (3x3, c_out 48)": (dict(cin=192, cout=48, h=88, w=304), HALO_BF16),
    "DenseNet bottleneck (1x1, c_out 192)": (dict(cin=1248, cout=192, h=22, w=76, k=1), ROW_BF16),
    "DenseNet transition (1x1)": (dict(cin=768, cout=384, h=88, w=304, k=1), ROW_BF16),
    "ResNeXt grouped 3x3 bundles": (dict(cin=32, cout=32, h=52, w=68, n_bundles=8), ROW_BF16),
    "ResNeXt strided 3x3 bundles": (dict(cin=32, cout=32, h=104, w=136, stride=2, n_bundles=16), ROW_BF16),
    "ResNeXt 1x1 (104x136)": (dict(cin=256, cout=256, h=104, w=136, k=1), ROW_BF16),
    "ResNeXt downsample 1x1 / 2": (dict(cin=512, cout=1024, h=52, w=68, k=1, stride=2), ROW_BF16),
    "deep 3x3, split-K (13x17)": (dict(cin=1024, cout=128, h=13, w=17, fill=2, splitk=True), ROW_BF16 | 16),
}


@pytest.mark.parametrize("name", sorted(DECODER) + sorted(ENCODER))
def test_bf16_plan_kinds(name):
    """Precision 2 takes the bf16 kernels (7 row-tiled, 8 halo tile) for decoder and encoder layers, never Winograd (6) nor
    the fp32 wide 1x1; the planar-tail layers stay on the fp32 halo kernel (2), the stem on its fp32 kernel (4)."""
    geo, want = {**DECODER, **ENCODER}[name]
    kind, bm, bn = _plan(**geo)
    assert kind & 15 != WINO
    assert kind & ~64 == want, (name, kind, bm, bn)
    if want & 15 == HALO_BF16:
        assert bn in (64, 128)                           # 48-wide growth convs padded to 64, as under precision 1


def test_env_override_never_hands_a_one_plane_split_to_the_bf16x3_kernel():
    """BTS_CONV_PRECISION=1 overrides a precision-2 descriptor.  Its w_split is then ONE plane, while the bf16x3 halo tile
    (kind 5) reads three: the library must ignore the buffer and fall back to the kernels that work from `w` alone.  A
    precision-1 descriptor with its own three-plane split keeps the bf16x3 halo tile under the same override.  (The knob
    is read once per process: a child process.)"""
    import json
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import json, sys; sys.path[:0] = [%r, %r]; import test_bf16_host as T\n"
            "out = {}\n"
            "for name, (geo, want) in T.DECODER.items():\n"
            "    if want == T.HALO_BF16:\n"
            "        out[name] = [T._plan(precision=p, **geo)[0] for p in (2, 1)]\n"
            "print(json.dumps(out))\n") % (here, os.path.dirname(here))
    env = dict(os.environ, BTS_CONV_PRECISION="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    kinds = json.loads(res.stdout.strip().splitlines()[-1])
    assert kinds, "no halo-tile layers in the table"
    for name, (k2, k1) in kinds.items():
        assert k2 & 15 == 0, (name, k2)          # precision-2 descriptor under the override: row-tiled bf16x3, w_split unused
        assert k1 & 15 == 5, (name, k1)          # precision-1 descriptor: its three planes, the bf16x3 halo tile


def test_precision_out_of_range_is_invalid():
    from bts_amd import _lib
    d = _lib.ConvDesc()
    d.x = d.w = d.y = 0x1000
    d.x_pix_stride = d.c_in_ld = 32
    d.k_pad = 32
    d.B = d.h_in = d.w_in = d.up = d.ksize = d.dil = d.stride = 1
    d.c_out, d.c_out_pad, d.y_pix_stride = 32, 32, 32
    bm, bn, kind = C.c_int(0), C.c_int(0), C.c_int(0)
    for p, ok in ((2, True), (3, False), (-1, False)):
        d.precision = p
        rc = _lib.load_real().bts_conv_plan_f32(C.byref(d), C.byref(bm), C.byref(bn), C.byref(kind))
        assert (rc == 0) == ok, (p, rc)
