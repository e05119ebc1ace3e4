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
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bts_amd._lib import ConvDesc  # noqa: E402
from bts_amd.conv_plan import FAMILY_MASK, Family as F, query  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.npz")

BATCHES = (1, 2, 16)
FILL_FRAMES = (0, 2, 8, 16)
RESOLUTIONS = ((352, 1216), (416, 544), (352, 704))      # KITTI, NYU, training crop
DILATIONS = (3, 6, 12, 18, 24)
WS_FLOATS = 1 << 34                                      # a split-K workspace that never limits the split


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


def grid():
    """Yields (desc, key): key = the integers that define the query (hashed into the table)."""
    P = 0x10000
    for L in layers():
        for nchw in ((0, 1) if L["nchw_too"] else (0,)):
            for B in BATCHES:
                for ff in FILL_FRAMES:
                    for prec in (0, 1):
                        for wino in (0, 1):
                            for ws in (0, 1):
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
                                if prec == 1 and not L["n_tail"] and not L["n_bundles"]:
                                    d.w_split = P
                                if wino:
                                    d.w_wino = P
                                if ws:
                                    d.splitk_ws, d.splitk_ws_floats = P, WS_FLOATS
                                key = tuple(L[k] for k in sorted(L)) + (nchw, B, ff, prec, wino, ws)
                                yield d, key


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


# every (family, bm, bn) the dispatch returns (ROW: fp32 and bf16x3; the grid holds no precision-2 query)
FAMILIES = {(F.ROW, 128, 128), (F.ROW, 64, 128), (F.ROW, 128, 64), (F.ROW, 64, 64), (F.ROW, 128, 48), (F.ROW, 64, 48), (F.ROW, 128, 32),
            (F.HALO, 128, 128), (F.HALO, 128, 64), (F.HALO, 128, 48), (F.HALO, 128, 32),
            (F.HALO_TAIL, 128, 128), (F.HALO_TAIL, 128, 64), (F.HALO_TAIL, 128, 32),
            (F.WIDE_1X1, 64, 192), (F.WIDE_1X1, 128, 192), (F.STEM, 256, 96), (F.STEM, 256, 64),
            (F.HALO_EMU, 128, 128), (F.HALO_EMU, 128, 64), (F.WINO, 128, 128), (F.WINO, 128, 64), (F.WINO, 128, 48)}


def families(t):
    ok = t["rc"] == 0
    return {(int(k) & FAMILY_MASK, int(m), int(n)) for k, m, n in zip(t["kind"][ok], t["bm"][ok], t["bn"][ok])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=TABLE)
    args = ap.parse_args()
    assert not any(k.startswith("BTS_") for k in os.environ), "run with no BTS_* variable set"
    t = run()
    got = families(t)
    assert got == FAMILIES, ("missing", FAMILIES - got, "unexpected", got - FAMILIES)
    np.savez_compressed(args.out, **t)
    print("%d queries, %d rejected, %d kernel families -> %s" % (len(t["rc"]), int((t["rc"] != 0).sum()), len(got), args.out))


if __name__ == "__main__":
    main()
