#!/usr/bin/env python3
"""Per-shape timing of bts_conv_wgrad_f32 on the training configuration's layers (B=4, 352x704, DenseNet161-BTS), then
one line per DenseNet161 block: the block's 2*L weight gradients as single launches against one batched launch
(bts_conv_wgrad_batch_f32) on the same buffers.

``--precision fp32 | bf16 | both`` (default fp32): the arithmetic -- "bf16" times bts_conv_wgrad_bf16_f32 /
bts_conv_wgrad_batch_bf16_f32 (train_precision "bf16"), "both" times the two in turn on the same buffers and prints the
ratio.  ``--json PATH`` writes the per-shape and per-block figures."""
import argparse
import json
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bts_amd import _lib, ops

SHAPES = [  # name, B, h, w, cin, cout, k, dil, up
    ("b1 1x1", 4, 88, 176, 192, 192, 1, 1, 1), ("b1 3x3", 4, 88, 176, 192, 48, 3, 1, 1),
    ("b2 1x1", 4, 44, 88, 480, 192, 1, 1, 1), ("b2 3x3", 4, 44, 88, 192, 48, 3, 1, 1),
    ("b3 1x1", 4, 22, 44, 1248, 192, 1, 1, 1), ("b3 3x3", 4, 22, 44, 192, 48, 3, 1, 1),
    ("b4 1x1", 4, 11, 22, 1632, 192, 1, 1, 1), ("b4 3x3", 4, 11, 22, 192, 48, 3, 1, 1),
    ("aspp 1x1", 4, 44, 88, 704, 256, 1, 1, 1), ("aspp 3x3 d12", 4, 44, 88, 256, 128, 3, 12, 1),
    ("upconv5", 4, 11, 22, 2208, 512, 3, 1, 2), ("conv5", 4, 22, 44, 896, 512, 3, 1, 1),
    ("upconv3", 4, 44, 88, 128, 128, 3, 1, 2), ("conv3", 4, 88, 176, 228, 128, 3, 1, 1),
    ("conv2", 4, 176, 352, 164, 64, 3, 1, 1), ("upconv1", 4, 176, 352, 64, 32, 3, 1, 2),
    ("conv1", 4, 352, 704, 36, 32, 3, 1, 1), ("reduc 32->16", 4, 352, 704, 32, 16, 1, 1, 1),
    ("reduc 8->4", 4, 352, 704, 8, 4, 1, 1, 1), ("reduc 128->64", 4, 88, 176, 128, 64, 1, 1, 1),
]

BLOCKS = [("block 1", 88, 176, 96, 6), ("block 2", 44, 88, 192, 12), ("block 3", 22, 44, 384, 36), ("block 4", 11, 22, 1056, 24)]


def _time(fn, n=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def blocks(dev, ws, precisions, out, B=4, g=48, mid=192):
    """The problems train._DenseBlockFn hands the weight-gradient kernels, on buffers laid out as it lays them out."""
    for name, H, W, C0, L in BLOCKS:
        npix, Ct = B * H * W, C0 + L * g
        buf, G = torch.randn(npix, Ct, device=dev), torch.randn(npix, Ct, device=dev)
        T1, D_T1 = torch.randn(L, npix, mid, device=dev), torch.randn(L, npix, mid, device=dev)
        stats = torch.rand(L, 8, Ct, device=dev) + 0.5
        DW = torch.empty(sum(mid * (C0 + i * g) + g * 9 * mid for i in range(L)), device=dev)
        problems, at = [], 0
        for i in range(L):
            Ci = C0 + i * g
            problems.append(dict(x=buf[:, :Ci], dy=D_T1[i], dw=DW[at:at + mid * Ci], B=B, h_in=H, w_in=W, c_in=Ci, c_out=mid, ksize=1,
                                 pre=(stats[i, 2, :Ci], stats[i, 3, :Ci]), pre_relu=True))
            at += mid * Ci
            problems.append(dict(x=T1[i], dy=G[:, Ci:Ci + g], dw=DW[at:at + g * 9 * mid], B=B, h_in=H, w_in=W, c_in=mid, c_out=g, ksize=3,
                                 pre=(stats[i, 6, :mid], stats[i, 7, :mid]), pre_relu=True))
            at += g * 9 * mid
        bases = [buf, G, T1, D_T1, stats, DW]
        batch = ops.WgradBatch(problems, bases, ws.numel())

        def singles(pr):
            for p in problems:
                ops.conv_wgrad(p["x"], B, H, W, p["c_in"], p["dy"], p["c_out"], p["ksize"], ws=ws, pre=p["pre"], pre_relu=True,
                               precision=pr)

        splits = sorted({p[2] for p in batch.plan})
        wgs = sum(-(-p["c_out"] // pl[0]) * -(-(p["c_in"] * p["ksize"] ** 2) // pl[1]) * pl[2] for p, pl in zip(problems, batch.plan))
        row = dict(name=name, pixels=npix, problems=len(problems), workgroups=wgs)
        for pr in precisions:
            us_single, us_batch = _time(lambda: singles(pr)), _time(lambda: batch.run(bases, ws, precision=pr))
            row[pr] = dict(single_us=us_single, batch_us=us_batch)
            print("%-8s %-4s px %6d  %2d problems  single launches %8.1f us  one batch %8.1f us  (x%.2f)  batch: %d workgroups, "
                  "split %s, %.1f MB of partials" % (name, pr, npix, len(problems), us_single, us_batch, us_single / us_batch, wgs,
                                                     "-".join(str(v) for v in (splits[0], splits[-1])) if len(splits) > 1 else splits[0],
                                                     4e-6 * batch.ws_used), flush=True)
        out.append(row)
        del buf, G, T1, D_T1, stats, DW, batch, problems


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="fp32")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    precisions = ("fp32", "bf16") if a.precision == "both" else (a.precision,)
    dev = torch.device("cuda:0")
    ws = torch.empty(48 << 20, device=dev)
    shapes, per_block = [], []
    for name, B, h, w, cin, cout, k, dil, up in SHAPES:
        H, W = h * up, w * up
        x = torch.randn(B * h * w, cin, device=dev)
        dy = torch.randn(B * H * W, cout, device=dev)
        fl = 2.0 * B * H * W * cout * cin * k * k
        by = 4.0 * (B * h * w * cin + B * H * W * cout)
        bm, bn, split, pps = ops.conv_wgrad_plan(B, h, w, cin, cout, k, dil=dil, up=up, ws_floats=ws.numel())
        row = dict(name=name, pixels=B * H * W, M=cout, N=cin * k * k, tile=[bm, bn], split=split)
        for pr in precisions:
            us = _time(lambda: ops.conv_wgrad(x, B, h, w, cin, dy, cout, k, dil=dil, up=up, ws=ws, precision=pr), n=20)
            row[pr] = us
            print("%-14s %-4s px %7d  M=%4d N=%6d  tile %3dx%3d split %4d  %8.1f us  %6.1f TF/s  %6.0f GB/s"
                  % (name, pr, B * H * W, cout, cin * k * k, bm, bn, split, us, fl / us / 1e6, by / us / 1e3), flush=True)
        if len(precisions) == 2:
            print("%-14s fp32 / bf16 = %.2f" % (name, row["fp32"] / row["bf16"]), flush=True)
        shapes.append(row)
    blocks(dev, ws, precisions, per_block)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(source_hash=_lib.source_hash(), shapes=shapes, blocks=per_block), fh, indent=1)

if __name__ == "__main__":
    main()
