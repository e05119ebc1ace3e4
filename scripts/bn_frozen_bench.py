#!/usr/bin/env python3
"""Isolated timing of the frozen-statistics norm backward (bts_bn_frozen_bwd_f32) next to the batch-statistic backward
(bts_bn_train_bwd_f32) on the same buffers, against the HBM roof at each form's bytes per element.

Shapes: DenseNet161's widest block-2 prefix at B=4, 352x704 (4*352*704/16 pixels x 384 channels) and its stem-resolution
norm (4*88*176 x 96).  Device events around ``--iters`` back-to-back launches after ``--warmup``; prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bts_amd import ops  # noqa: E402

HBM_TBPS = 6.3            # what a float4 copy reaches on an MI355X (8.0 TB/s is the HBM3E peak): the roof the trainer's other rows use
SHAPES = [(4 * 352 * 704 // 16, 384), (4 * 88 * 176, 96)]


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    rows = []
    for npix, C in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((npix, C), device="cuda", generator=g)
        dy = torch.randn((npix, C), device="cuda", generator=g)
        dx = torch.zeros((npix, C), device="cuda")
        rm, rv = torch.randn(C, device="cuda", generator=g), 0.5 + torch.rand(C, device="cuda", generator=g)
        gamma, beta = 0.5 + torch.rand(C, device="cuda", generator=g), torch.randn(C, device="cuda", generator=g)
        v = ops.bn_frozen_vectors(C, gamma, beta, rm, rv, 1e-5)
        ws = torch.empty(ops.bn_train_ws_floats(npix, C), device="cuda")
        forms = [
            ("bn_train_bwd (dx + sums)", 20, lambda: ops.bn_train_backward(x, dy, C, v[0], v[1], v[2], v[3], True, ws, dx)),
            ("bn_frozen_bwd dx", 12, lambda: ops.bn_frozen_backward(x, dy, C, v[0], v[1], v[2], v[3], True, None, dx, sums=False)),
            ("bn_frozen_bwd dx + sums", 12, lambda: ops.bn_frozen_backward(x, dy, C, v[0], v[1], v[2], v[3], True, ws, dx)),
            ("bn_frozen_bwd accumulate", 16,
             lambda: ops.bn_frozen_backward(x, dy, C, v[0], v[1], v[2], v[3], True, None, dx, sums=False, accumulate=True)),
            ("bn_frozen_bwd accumulate + sums", 16,
             lambda: ops.bn_frozen_backward(x, dy, C, v[0], v[1], v[2], v[3], True, ws, dx, accumulate=True)),
            ("bn_frozen_bwd sums only", 8, lambda: ops.bn_frozen_backward(x, dy, C, v[0], v[1], v[2], v[3], True, ws, None)),
        ]
        for name, bytes_per, fn in forms:
            ms = timed(fn, a.warmup, a.iters)
            nbytes = float(bytes_per) * npix * C
            rows.append(dict(npix=npix, C=C, form=name, bytes_per_element=bytes_per, us=ms * 1e3,
                             tbps=nbytes / (ms * 1e-3) / 1e12, roof_us=nbytes / (HBM_TBPS * 1e12) * 1e6,
                             share_of_roof=nbytes / (HBM_TBPS * 1e12) / (ms * 1e-3)))
            print("%7d x %-4d %-34s %2d B/el %8.1f us  %5.2f TB/s  roof %6.1f us" % (npix, C, name, bytes_per, ms * 1e3,
                                                                                      rows[-1]["tbps"], rows[-1]["roof_us"]),
                  file=sys.stderr)
    print(json.dumps(dict(metric="bn backward kernels, isolated", hbm_roof_tbps=HBM_TBPS, rows=rows)))


if __name__ == "__main__":
    main()
