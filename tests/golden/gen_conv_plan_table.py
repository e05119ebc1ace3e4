"""Writes conv_plan_table.npz: the convolution dispatch of libbts_hip.so (bts_conv_plan_f32, bts_conv_plan_ksteps_f32)
over a fixed grid of bts_conv_desc values, as tests/test_conv_plan_table.py re-checks it.

The grid holds every convolution shape of the BASELINE.json configs -- DenseNet161 and ResNeXt101 encoders (stem, dense
layers, transitions, bottlenecks with grouped 3x3 bundles and stride-2 downsampling), the BTS decoder (sub-pixel
upconvs, the upconv5 tap GEMM, conv5..conv1 with their planar tails, the dilated ASPP branches) and the training step's
upsampled-gather and data-gradient convolutions -- on the KITTI (352x1216), NYU (416x544) and training-crop (352x704)
maps, each under every batch size, declared frame count, precision, Winograd-weight and split-K-workspace setting below.
Host-side queries only: the pointers are fake and never dereferenced.  The library reads its environment knobs once per
process, so run this with no BTS_* variable set.

    python tests/golden/gen_conv_plan_table.py            # rewrite tests/golden/conv_plan_table.npz
    python tests/golden/gen_conv_plan_table.py --out F    # write F instead

With --rejects it writes conv_reject_table.npz instead: the answers of the same two queries, of bts_upconv_dgrad_plan and
(for arguments rejected before any HIP call) of bts_upconv_dgrad_f32 for malformed descriptors -- one case per check of the
host path, and two-violation cases that record which check answers first (REJECT_CASES below).
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bts_amd import _lib  # noqa: E402
from bts_amd._lib import ConvDesc  # noqa: E402
from bts_amd.conv_plan import FAMILY_MASK, Family as F, query  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.npz")
REJECT_TABLE = os.path.join(ROOT, "tests", "golden", "conv_reject_table.npz")

BATCHES = (1, 2, 16)
FILL_FRAMES = (0, 2, 8, 16)
RESOLUTIONS = ((352, 1216), (416, 544), (352, 704))      # KITTI, NYU, training crop
DILATIONS = (3, 6, 12, 18, 24)
WS_FLOATS = 1 << 34                                      # a split-K workspace that never limits the split
P = 0x10000                                              # every fake pointer: 16-byte aligned, never followed


def r4(c):
    return (c + 3) // 4 * 4


def r32(c):
    return (c + 31) // 32 * 32


def layer(h, w, c_in, c_out, k=3, stride=1, pad=None, dil=1, up=1, subpixel=False, tail=0, bundles=0, pre=False,
          res=False, nchw_too=False):
    """One convolution as conv_forward (bts_amd/ops.py) describes it; c_in / c_out per bundle when bundled."""
    c_in_ld = r4(c_in) + (4 if tail else 0)
    if subpixel:
        k, pad, up = 2, 0, 1
    elif pad is None:
        pad = dil * (k // 2)
    taps = k * k
    n = max(bundles, 1)
    return dict(h_in=h, w_in=w, c_in_ld=c_in_ld, x_pix_stride=n * (c_in_ld - (4 if tail else 0)), k_pad=r32(taps * c_in_ld),
                ksize=k, stride=stride, pad=pad, dil=dil, up=up, subpixel=int(subpixel), c_out=c_out,
                c_out_pad=c_out if bundles else r32(c_out), y_pix_stride=n * c_out, n_tail=tail, n_bundles=bundles,
                pre=int(pre), res=int(res), nchw_too=int(nchw_too))


def densenet161(H, W):
    out = [layer(H, W, 3, 96, k=7, stride=2, pad=3)]                       # stem (4-channel-padded image)
    c, s = 96, 4
    for i, n in enumerate((6, 12, 36, 24)):
        h, w = H // s, W // s
        for j in range(n):
            ci = c + 48 * j
            out.append(layer(h, w, ci, 192, k=1, pre=True))                 # norm1-relu1-conv1x1
            out.append(layer(h, w, 192, 48))                               # norm2-relu2-conv3x3 (growth)
            out.append(layer(h, w, 48, 192))                               # data gradients of the training step
            out.append(layer(h, w, 192, ci, k=1))
        c += 48 * n
        if i < 3:                                                          # transition: pool first, then the 1x1
            out.append(layer(h // 2, w // 2, c, c // 2, k=1, pre=True))
            out.append(layer(h // 2, w // 2, c // 2, c, k=1))
            c, s = c // 2, s * 2
    return out


def resnext101(H, W):
    out = [layer(H, W, 3, 64, k=7, stride=2, pad=3)]
    c, s = 64, 4
    for i, width in enumerate((256, 512, 1024, 2048)):
        stride = 1 if i == 0 else 2
        cb = max(32, width // 32)
        hi, wi = H // (s // stride), W // (s // stride)
        h, w = H // s, W // s
        cout = width
        for first in (True, False):
            cin = c if first else cout
            st = stride if first else 1
            out.append(layer(hi if first else h, wi if first else w, cin, width, k=1))
            out.append(layer(hi if first else h, wi if first else w, cb, cb, stride=st, bundles=width // cb))
            out.append(layer(h, w, width, cout, k=1, res=True))
            if first:
                out.append(layer(hi, wi, cin, cout, k=1, stride=stride, pad=0))      # downsample
        c, s = cout, s * 2
    return out


def decoder(H, W, f, nf=512):
    q = nf // 4
    out = []
    for s, cin, cout, tail, cat in ((16, f[4], nf, 0, nf + f[3]), (8, nf, nf // 2, 0, nf // 2 + f[2]),
                                    (4, q, q, 1, q + f[1]), (2, q, nf // 8, 1, nf // 8 + f[0]), (1, nf // 8, nf // 16, 4, nf // 16)):
        h, w = H // s, W // s
        out.append(layer(h // 2, w // 2, cin, cout, subpixel=True))                   # upconv (sub-pixel)
        out.append(layer(h // 2, w // 2, cin, cout, up=2))                            # upconv (training: folded upsample)
        out.append(layer(h, w, cout, cin))                                            # its data gradient
        if tail:
            for t in range(1, 5):
                out.append(layer(h, w, cat, cout, tail=t, nchw_too=True))             # conv3 / conv2 / conv1 (+ planes)
        else:
            out.append(layer(h, w, cat, cout, nchw_too=True))                         # conv5 / conv4
    out.append(layer(H // 32, W // 32, f[4], 9 * nf, k=1))                            # upconv5 as a tap GEMM
    h8, w8 = H // 8, W // 8
    c_cat4 = nf // 2 + f[2]
    for i, d in enumerate(DILATIONS):                                                 # dense ASPP
        cin = nf // 2 if i == 0 else c_cat4 + i * q
        out.append(layer(h8, w8, cin, nf // 2, k=1, pre=i > 0))
        out.append(layer(h8, w8, nf // 2, q, dil=d, nchw_too=True))
    out.append(layer(h8, w8, 5 * q, q, nchw_too=True))                                # daspp_conv
    return out


def layers():
    out = []
    for H, W in RESOLUTIONS:
        out += densenet161(H, W) + resnext101(H, W)
        out += decoder(H, W, (96, 96, 192, 384, 2208)) + decoder(H, W, (64, 256, 512, 1024, 2048))
    seen, uniq = set(), []
    for L in out:
        key = tuple(sorted(L.items()))
        if key not in seen:
            seen.add(key)
            uniq.append(L)
    return uniq


def describe(L, nchw=0, B=2, ff=0, prec=0, wino=0, ws=0):
    """The descriptor of layer L under one setting of the grid's other axes; fake pointers, never dereferenced."""
    d = ConvDesc()
    d.x = d.w = d.y = P
    for k in ("x_pix_stride", "c_in_ld", "k_pad", "h_in", "w_in", "up", "ksize", "dil", "stride",
              "pad", "c_out", "c_out_pad", "y_pix_stride", "subpixel", "n_tail", "n_bundles"):
        setattr(d, k, L[k])
    d.B, d.fill_frames, d.precision, d.y_nchw = B, ff, prec, nchw
    if nchw:
        d.y_pix_stride = 0
    if L["pre"]:
        d.pre_scale = d.pre_shift = P
    d.pre_relu = L["pre"]
    d.e1_scale = d.e1_shift = P
    d.act = 1
    if L["res"]:
        d.res, d.res_pix_stride = P, d.y_pix_stride
    for j in range(L["n_tail"]):
        d.tail_planes[j] = P
    if prec in (1, 2) and not L["n_tail"] and not L["n_bundles"]:
        d.w_split = P
    if wino:
        d.w_wino = P
    if ws:
        d.splitk_ws, d.splitk_ws_floats = P, WS_FLOATS
    return d


def grid():
    """Yields (desc, key): key = the integers that define the query (hashed into the table)."""
    for L in layers():
        for nchw in ((0, 1) if L["nchw_too"] else (0,)):
            for B in BATCHES:
                for ff in FILL_FRAMES:
                    for prec in (0, 1, 2):
                        for wino in (0, 1):
                            for ws in (0, 1):
                                key = tuple(L[k] for k in sorted(L)) + (nchw, B, ff, prec, wino, ws)
                                yield describe(L, nchw, B, ff, prec, wino, ws), key


def run():
    rows, keys = [], hashlib.sha256()
    for d, key in grid():
        p = query(d, ksteps=True)                     # (asserts that both queries return the same code)
        rows.append((p.rc, p.bm, p.bn, p.kind, p.issued, p.dense))
        keys.update(np.asarray(key, np.int64).tobytes())
    t = np.asarray(rows, np.int64)
    return dict(rc=t[:, 0].astype(np.int32), bm=t[:, 1].astype(np.int16), bn=t[:, 2].astype(np.int16),
                kind=t[:, 3].astype(np.int16), issued=t[:, 4], dense=t[:, 5],
                grid_sha256=np.frombuffer(keys.digest(), np.uint8))


# every (family, bm, bn) the dispatch returns (ROW: fp32 and bf16x3; ROW_BF16 / HALO_BF16: precision 2)
FAMILIES = {(F.ROW, 128, 128), (F.ROW, 64, 128), (F.ROW, 128, 64), (F.ROW, 64, 64), (F.ROW, 128, 48), (F.ROW, 64, 48), (F.ROW, 128, 32),
            (F.HALO, 128, 128), (F.HALO, 128, 64), (F.HALO, 128, 48), (F.HALO, 128, 32),
            (F.HALO_TAIL, 128, 128), (F.HALO_TAIL, 128, 64), (F.HALO_TAIL, 128, 32),
            (F.WIDE_1X1, 64, 192), (F.WIDE_1X1, 128, 192), (F.STEM, 256, 96), (F.STEM, 256, 64),
            (F.HALO_EMU, 128, 128), (F.HALO_EMU, 128, 64), (F.WINO, 128, 128), (F.WINO, 128, 64), (F.WINO, 128, 48),
            (F.ROW_BF16, 128, 128), (F.ROW_BF16, 64, 128), (F.ROW_BF16, 128, 64), (F.ROW_BF16, 64, 64), (F.ROW_BF16, 128, 32),
            (F.HALO_BF16, 128, 128), (F.HALO_BF16, 128, 64)}


def families(t):
    ok = t["rc"] == 0
    return {(int(k) & FAMILY_MASK, int(m), int(n)) for k, m, n in zip(t["kind"][ok], t["bm"][ok], t["bn"][ok])}


# ---- conv_reject_table.npz: what the library answers for malformed descriptors -- the error code, and through descriptors
# with two violations of different codes (BTS_ERR_INVALID -1 / BTS_ERR_UNSUPPORTED -2) which check answers first.
# A case is a valid base descriptor plus named mutations; a mutation is ONE violation (it may set several fields where the
# rest of the descriptor has to stay valid around it).
def reject_bases():
    y2res = describe(layer(44, 152, 128, 128))
    y2res.y2, y2res.y2_pix_stride, y2res.res, y2res.res_pix_stride = P, 128, P, 128
    return {"3x3": describe(layer(44, 152, 128, 128)),                       # c_in_ld 128, k_pad 1152, pixel strides 128
            "1x1": describe(layer(44, 152, 192, 192, k=1, pre=True)),
            "subpixel": describe(layer(22, 76, 128, 64, subpixel=True)),
            "tail": describe(layer(88, 304, 128, 64, tail=1)),               # c_in_ld 132, x_pix_stride 128, k_pad 1216
            "bundles": describe(layer(88, 304, 32, 32, bundles=8)),          # pixel strides 256, c_out_pad 32
            "nchw": describe(layer(44, 152, 128, 128), nchw=1),
            "up2": describe(layer(64, 64, 4, 32, up=2), B=1),                # c_in_ld 4, k_pad 64, x_pix_stride 4
            "y2res": y2res}


MUTATIONS = {
    "x null": dict(x=0), "w null": dict(w=0), "y null": dict(y=0),
    "B 0": dict(B=0), "h_in 0": dict(h_in=0), "w_in -1": dict(w_in=-1), "c_out 0": dict(c_out=0),
    "up 3": dict(up=3), "up 0": dict(up=0),
    "ksize 3": dict(ksize=3), "up 2": dict(up=2), "stride 2": dict(stride=2), "dil 2": dict(dil=2, pad=2), "y_nchw": dict(y_nchw=1),
    "ksize 0": dict(ksize=0), "ksize 4": dict(ksize=4, k_pad=2048), "ksize 8": dict(ksize=8, k_pad=8192),
    "ksize 9": dict(ksize=9, k_pad=10368),
    "dil 0": dict(dil=0), "stride 0": dict(stride=0), "pad -1": dict(pad=-1),
    "up 2 stride 2": dict(up=2, stride=2),
    "c_in_ld 0": dict(c_in_ld=0), "c_in_ld 126": dict(c_in_ld=126), "k_pad 1168": dict(k_pad=1168), "k_pad 1120": dict(k_pad=1120),
    "k_pad 65536": dict(k_pad=65536),
    "x_pix_stride 130": dict(x_pix_stride=130), "x_pix_stride 124": dict(x_pix_stride=124),
    "c_out_pad 100": dict(c_out=96, c_out_pad=100), "c_out_pad 96": dict(c_out_pad=96),
    "x unaligned": dict(x=P + 4), "w unaligned": dict(w=P + 8),
    "pre_scale unaligned": dict(pre_scale=P + 4), "pre_shift null": dict(pre_shift=0), "pre_shift unaligned": dict(pre_shift=P + 4),
    "e1 no shift": dict(e1_shift=0), "e2 no shift": dict(e2_scale=P),
    "y_pix_stride 64": dict(y_pix_stride=64),
    "act -1": dict(act=-1), "act 4": dict(act=4),
    "w_split unaligned": dict(w_split=P + 4), "w_wino unaligned": dict(w_wino=P + 4),
    "x extent": dict(B=64, h_in=1024, w_in=1024),                            # 2^26 pixels x 128 floats = 2^33 elements
    "w extent": dict(c_out_pad=65600, k_pad=65504),                          # 65600 x 65504 >= 2^32
    "w extent x4": dict(c_out_pad=16416, k_pad=65504),                       # sub-pixel: four classes
    "y2": dict(y2=P, y2_pix_stride=128), "y2_pix_stride 64": dict(y2_pix_stride=64), "y2_pix_stride 16": dict(y2_pix_stride=16),
    "kernel larger than map": dict(h_in=2, dil=3, pad=0),
    "M 2^31": dict(B=1 << 17),                                               # on "up2": 2^29 source pixels, 2^31 outputs
    "fill_frames -1": dict(fill_frames=-1), "fill_frames 4097": dict(fill_frames=4097),
    "n_tail -1": dict(n_tail=-1), "n_tail 5": dict(n_tail=5),
    "tail": dict(n_tail=1, tail_planes0=P),                                  # a planar tail on a base that has none
    "tail c_in_ld 4": dict(c_in_ld=4),
    "tail plane null": dict(tail_planes0=0), "tail plane unaligned": dict(tail_planes0=P + 2),
    "tail ksize 1": dict(ksize=1, pad=0), "tail pad 0": dict(pad=0),
    "res": dict(res=P, res_pix_stride=128), "res_pix_stride 64": dict(res_pix_stride=64),
    "n_bundles 4": dict(n_bundles=4, c_out_pad=64),
    "bundles c_out 24": dict(c_out=24),
    "bundles x_pix_stride 32": dict(x_pix_stride=32), "bundles y_pix_stride 32": dict(y_pix_stride=32),
    "bundles y2 short": dict(y2=P, y2_pix_stride=32), "bundles res short": dict(res=P, res_pix_stride=32),
    "bundles extent": dict(n_bundles=4096, k_pad=65504, h_in=8, w_in=8, x_pix_stride=1 << 17, y_pix_stride=1 << 17),     # 4096 x 32 x 65504 >= 2^32
    "n_bundles -1": dict(n_bundles=-1),
    "splitk_ws unaligned": dict(splitk_ws=P + 4, splitk_ws_floats=1 << 20), "splitk_ws_floats -1": dict(splitk_ws=P, splitk_ws_floats=-1),
    "precision 3": dict(precision=3), "precision -1": dict(precision=-1),
}

# (base, mutation, ...) in the order of conv_dispatch's checks; the comment quotes the check a group's single-mutation cases hit.
# Not reachable from a plan query: the null descriptor (the query answers that itself) and the $BTS_CONV_PRECISION range.
REJECT_CASES = [(b,) for b in ("3x3", "1x1", "subpixel", "tail", "bundles", "nchw", "up2", "y2res")] + [   # the bases: accepted
    # !d->x || !d->w || !d->y                                                                -1
    ("3x3", "x null"), ("3x3", "w null"), ("3x3", "y null"), ("nchw", "y null"),
    # B <= 0 || h_in <= 0 || w_in <= 0 || c_out <= 0                                          -1
    ("3x3", "B 0"), ("3x3", "h_in 0"), ("1x1", "w_in -1"), ("3x3", "c_out 0"),
    # up != 1 && up != 2                                                                     -2
    ("3x3", "up 3"), ("1x1", "up 0"),
    # subpixel: ksize != 2 || up != 1 || stride != 1 || dil != 1 || y_nchw                    -1
    ("subpixel", "ksize 3"), ("subpixel", "up 2"), ("subpixel", "stride 2"), ("subpixel", "dil 2"), ("subpixel", "y_nchw"),
    # ksize < 1 || ksize > 7 || even                                                         -2
    ("3x3", "ksize 0"), ("3x3", "ksize 4"), ("3x3", "ksize 8"), ("3x3", "ksize 9"),
    # dil < 1 || stride < 1 || pad < 0                                                       -1
    ("3x3", "dil 0"), ("3x3", "stride 0"), ("3x3", "pad -1"),
    # up == 2 && stride != 1                                                                 -2
    ("3x3", "up 2 stride 2"), ("up2", "stride 2"),
    # c_in_ld <= 0 || c_in_ld & 3 || k_pad % 32 || k_pad < ksize^2 c_in_ld                    -1
    ("3x3", "c_in_ld 0"), ("3x3", "c_in_ld 126"), ("3x3", "k_pad 1168"), ("3x3", "k_pad 1120"),
    # k_pad >= 65536                                                                         -2
    ("3x3", "k_pad 65536"), ("1x1", "k_pad 65536"),
    # x_pix_stride & 3 || x_pix_stride < c_in_ld - (n_tail > 0 ? 4 : 0)                       -1
    ("3x3", "x_pix_stride 130"), ("3x3", "x_pix_stride 124"), ("tail", "x_pix_stride 124"),
    # c_out_pad & 31 || c_out_pad < c_out                                                    -1
    ("3x3", "c_out_pad 100"), ("3x3", "c_out_pad 96"),
    # x or w not 16-byte aligned                                                             -1
    ("3x3", "x unaligned"), ("3x3", "w unaligned"),
    # pre_scale: unaligned, or pre_shift null / unaligned                                    -1
    ("1x1", "pre_scale unaligned"), ("1x1", "pre_shift null"), ("1x1", "pre_shift unaligned"),
    # e1_scale && !e1_shift || e2_scale && !e2_shift                                         -1
    ("3x3", "e1 no shift"), ("3x3", "e2 no shift"),
    # !y_nchw && y_pix_stride < c_out                                                        -1
    ("3x3", "y_pix_stride 64"),
    # act < 0 || act > 3                                                                     -1
    ("3x3", "act -1"), ("3x3", "act 4"),
    # w_split / w_wino not 16-byte aligned                                                   -1
    ("3x3", "w_split unaligned"), ("3x3", "w_wino unaligned"),
    # B h_in w_in x_pix_stride >= 2^32                                                       -2
    ("3x3", "x extent"),
    # c_out_pad k_pad (x4 sub-pixel) >= 2^32                                                 -2
    ("3x3", "w extent"), ("subpixel", "w extent x4"),
    # y2 && (y_nchw || y2_pix_stride < c_out)                                                -1
    ("nchw", "y2"), ("y2res", "y2_pix_stride 64"),
    # H <= 0 || W <= 0                                                                       -1
    ("3x3", "kernel larger than map"),
    # M >= 2^31                                                                              -2
    ("up2", "M 2^31"),
    # fill_frames < 0 || fill_frames > 4096                                                  -1
    ("3x3", "fill_frames -1"), ("3x3", "fill_frames 4097"),
    # n_tail < 0 || n_tail > 4                                                               -1
    ("3x3", "n_tail -1"), ("3x3", "n_tail 5"), ("tail", "n_tail 5"),
    # n_tail > 0 on a layer that is not a plain 3x3 / pad 1                                  -2
    ("1x1", "tail"), ("tail", "tail ksize 1"), ("tail", "stride 2"), ("tail", "dil 2"), ("tail", "up 2"), ("tail", "tail pad 0"),
    ("subpixel", "tail"), ("bundles", "tail"),
    # n_tail > 0: c_in_ld < 8 || x_pix_stride < c_in_ld - 4                                   -1
    ("tail", "tail c_in_ld 4"),
    # a tail plane null or not 4-byte aligned                                                -1
    ("tail", "tail plane null"), ("tail", "tail plane unaligned"),
    # res && (y_nchw || res_pix_stride < c_out)                                              -1
    ("nchw", "res"), ("y2res", "res_pix_stride 64"),
    # bundles: subpixel || y_nchw || up != 1                                                 -1
    ("subpixel", "n_bundles 4"), ("bundles", "y_nchw"), ("bundles", "up 2"),
    # bundles: c_out_pad != c_out                                                            -1
    ("bundles", "bundles c_out 24"),
    # bundles: x_pix_stride < n_bundles c_in_ld || y_pix_stride < n_bundles c_out             -1
    ("bundles", "bundles x_pix_stride 32"), ("bundles", "bundles y_pix_stride 32"),
    # bundles: y2 / res pixel stride < n_bundles c_out                                       -1
    ("bundles", "bundles y2 short"), ("bundles", "bundles res short"),
    # n_bundles c_out_pad k_pad >= 2^32                                                      -2
    ("bundles", "bundles extent"),
    # n_bundles < 0                                                                          -1
    ("3x3", "n_bundles -1"),
    # splitk_ws unaligned || splitk_ws_floats < 0                                            -1
    ("3x3", "splitk_ws unaligned"), ("3x3", "splitk_ws_floats -1"),
    # precision not 0 / 1 / 2                                                                -1
    ("3x3", "precision 3"), ("3x3", "precision -1"), ("tail", "precision 3"),
    # ---- two violations with different codes: the earlier check answers
    ("3x3", "up 3", "act 4"), ("3x3", "k_pad 65536", "act 4"), ("3x3", "x null", "up 3"), ("3x3", "B 0", "up 3"),
    ("3x3", "ksize 9", "dil 0"), ("3x3", "dil 0", "up 2 stride 2"), ("3x3", "up 2 stride 2", "c_in_ld 126"),
    ("3x3", "c_in_ld 126", "k_pad 65536"), ("3x3", "k_pad 65536", "x_pix_stride 130"), ("3x3", "x extent", "fill_frames -1"),
    ("3x3", "act 4", "x extent"), ("3x3", "w extent", "y2", "y2_pix_stride 64"), ("up2", "y2", "y2_pix_stride 16", "M 2^31"),
    ("up2", "M 2^31", "fill_frames 4097"), ("tail", "fill_frames -1", "stride 2"), ("tail", "stride 2", "tail plane null"),
    ("1x1", "n_tail 5"), ("tail", "stride 2", "precision 3"), ("bundles", "bundles extent", "splitk_ws unaligned"),
    ("bundles", "bundles c_out 24", "bundles extent"), ("subpixel", "ksize 3", "up 3"), ("3x3", "up 3", "ksize 9", "x null"),
]

# bts_upconv_dgrad_plan(B, h, w, c_out, c_in, precision, fill_frames, splitk_ws_floats; bm, bn, kind): a valid query plus named
# changes.  "null bm / bn / kind" passes a null output.  Checks of upconv_dgrad_desc that the plan query can violate (it
# supplies aligned pointers and exact strides itself), then those of conv_dispatch behind it.
DGRAD_BASE = dict(B=2, h=44, w=152, c_out=64, c_in=128, precision=0, fill_frames=0, splitk_ws_floats=0)
DGRAD_CASES = [
    {}, dict(splitk_ws_floats=1 << 30), dict(precision=1), dict(precision=2), dict(h=11, w=38, c_out=512, splitk_ws_floats=1 << 30),
    dict(null="bm"), dict(null="bn"), dict(null="kind"),                     # !bm || !bn || !kind                          -1
    dict(B=0), dict(h=0), dict(w=-1), dict(c_in=0), dict(c_out=0),           # B <= 0 || h <= 0 || ... || c_out <= 0        -1
    dict(c_in=126), dict(c_out=66),                                          # c_in & 3 || c_out & 3                        -1
    dict(splitk_ws_floats=-1),                                               # workspace pointer / size mismatch            -1
    dict(h=1 << 29, w=1), dict(h=1, w=1 << 29),                              # 2h or 2w >= 2^30                             -2
    dict(c_out=4096),                                                        # conv_dispatch: k_pad >= 65536                -2
    dict(B=64, h=512, w=512),                                                # conv_dispatch: 2^26 pixels x 64 floats       -2
    dict(fill_frames=-1), dict(fill_frames=4097), dict(precision=3), dict(precision=-1),                                  # -1
    # two violations with different codes
    dict(c_in=126, h=1 << 29, w=1), dict(splitk_ws_floats=-1, h=1 << 29, w=1), dict(h=1 << 29, w=1, precision=3),
    dict(c_out=4096, precision=3), dict(c_out=4096, fill_frames=-1), dict(B=0, c_out=4096), dict(null="kind", h=1 << 29, w=1),
]

# bts_upconv_dgrad_f32 itself, for the checks of upconv_dgrad_desc that only its caller's pointers and strides can violate:
# every one of these is answered before any HIP call.  (dy, dy_pix_stride, dx, dx_pix_stride, w_dgrad, splitk_ws,
# splitk_ws_floats) on top of B 2, h 44, w 152, c_out 64, c_in 128.
DGRAD_LAUNCH_BASE = dict(dy=P, dy_pix_stride=64, w_dgrad=P, dx=P, dx_pix_stride=128, splitk_ws=0, splitk_ws_floats=0)
DGRAD_LAUNCH_CASES = [
    dict(dy=0), dict(w_dgrad=0), dict(dx=0),                                                   # null pointers                -1
    dict(dy_pix_stride=66), dict(dy_pix_stride=60), dict(dx_pix_stride=130), dict(dx_pix_stride=124),       # strides          -1
    dict(dy=P + 4), dict(w_dgrad=P + 4), dict(dx=P + 4),                                       # 16-byte alignment            -1
    dict(splitk_ws=P), dict(splitk_ws_floats=16), dict(splitk_ws=P + 4, splitk_ws_floats=16),  # workspace pointer / size     -1
]


def mutate(d, fields):
    for k, v in fields.items():
        if k.startswith("tail_planes"):
            d.tail_planes[int(k[-1])] = v
        else:
            setattr(d, k, v)


def run_rejects():
    """name, rc, bm, bn, kind, issued, dense per case (issued / dense: 0 where the entry point does not report them)."""
    lib = _lib.load_real()
    names, rows, keys = [], [], hashlib.sha256()
    for case in REJECT_CASES:
        d = ConvDesc.from_buffer_copy(reject_bases()[case[0]])
        for m in case[1:]:
            mutate(d, MUTATIONS[m])
        p = query(d, ksteps=True)
        assert (p.rc == 0) == (len(case) == 1), (case, p.rc)                 # the bases are valid, every mutation is rejected
        names.append("conv: " + " + ".join(case))
        rows.append((p.rc, p.bm, p.bn, p.kind, p.issued, p.dense))
        keys.update(bytes(d))
    for ch in DGRAD_CASES:
        a = dict(DGRAD_BASE, **ch)
        out = {k: C.c_int(-7) for k in ("bm", "bn", "kind")}                 # -7: an output the query left alone
        ptr = [None if a.get("null") == k else C.byref(out[k]) for k in ("bm", "bn", "kind")]
        rc = lib.bts_upconv_dgrad_plan(a["B"], a["h"], a["w"], a["c_out"], a["c_in"], a["precision"], a["fill_frames"],
                                       a["splitk_ws_floats"], *ptr)
        names.append("upconv_dgrad_plan: " + (", ".join("%s %s" % kv for kv in ch.items()) or "base"))
        rows.append((rc, out["bm"].value, out["bn"].value, out["kind"].value, 0, 0))
        keys.update(repr(sorted(a.items())).encode())
    for ch in DGRAD_LAUNCH_CASES:
        a = dict(DGRAD_LAUNCH_BASE, **ch)
        rc = lib.bts_upconv_dgrad_f32(a["dy"], a["dy_pix_stride"], 2, 44, 152, 64, a["w_dgrad"], 128, a["dx"], a["dx_pix_stride"],
                                      0, 0, a["splitk_ws"], a["splitk_ws_floats"], None)
        assert rc == -1, (ch, rc)                                            # anything else would have reached the launch path
        names.append("upconv_dgrad_f32: " + ", ".join("%s %s" % kv for kv in ch.items()))
        rows.append((rc, 0, 0, 0, 0, 0))
        keys.update(repr(sorted(a.items())).encode())
    t = np.asarray(rows, np.int64)
    return dict(name=np.asarray(names), rc=t[:, 0].astype(np.int32), bm=t[:, 1].astype(np.int16), bn=t[:, 2].astype(np.int16),
                kind=t[:, 3].astype(np.int16), issued=t[:, 4], dense=t[:, 5], grid_sha256=np.frombuffer(keys.digest(), np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rejects", action="store_true", help="write conv_reject_table.npz instead")
    args = ap.parse_args()
    assert not any(k.startswith("BTS_") for k in os.environ), "run with no BTS_* variable set"
    if args.rejects:
        t = run_rejects()
        np.savez_compressed(args.out or REJECT_TABLE, **t)
        print("%d descriptors, %d rejected -> %s" % (len(t["rc"]), int((t["rc"] != 0).sum()), args.out or REJECT_TABLE))
        return
    args.out = args.out or TABLE
    t = run()
    got = families(t)
    assert got == FAMILIES, ("missing", FAMILIES - got, "unexpected", got - FAMILIES)
    np.savez_compressed(args.out, **t)
    print("%d queries, %d rejected, %d kernel families -> %s" % (len(t["rc"]), int((t["rc"] != 0).sum()), len(got), args.out))


if __name__ == "__main__":
    main()
