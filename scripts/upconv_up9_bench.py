#!/usr/bin/env python3
"""Isolated launches of the KITTI decoder's upconv3 / 2 / 1 at B = 16 and B = 4 (a sub-batch of the bench's four streams):
the sub-pixel halo kernel (ops.conv_forward(subpixel=True)) against the shared-patch F(2x2,2x2) kernel
(ops.upconv_up9_forward) on the same operands, HIP events, 15 launches each (min / median / max, ms).
    python scripts/upconv_up9_bench.py [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bts_amd import ops
torch.manual_seed(0)
out = {}
for B in (16, 4):
    for name, h, w, cin, cout in (("upconv3", 44, 152, 128, 128), ("upconv2", 88, 304, 128, 64), ("upconv1", 176, 608, 64, 32)):
        x = torch.randn(B * h * w, cin, device="cuda")
        wt = torch.randn(cout, cin, 3, 3, device="cuda") / (cin * 9) ** 0.5
        wp = ops.pack_upconv_subpixel(wt)[0]
        u = ops.pack_upconv_up9(wt)
        y = torch.empty(4 * B * h * w, cout, device="cuda")
        def halo():
            with ops.launch_config(fill_frames=16, precision="fp32"):
                ops.conv_forward(x, B, h, w, wp, cout, 3, up=2, act=ops.ACT_ELU, y2d=y, subpixel=True)
        def up9():
            ops.upconv_up9_forward(x, B, h, w, u, cin, cout, y, act=ops.ACT_ELU)
        res = {}
        for label, fn in (("halo", halo), ("up9", up9)):
            for _ in range(3): fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(15):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); fn(); e.record(); torch.cuda.synchronize()
                ts.append(s.elapsed_time(e))
            ts.sort()
            res[label] = dict(min=round(ts[0], 4), med=round(ts[len(ts) // 2], 4), max=round(ts[-1], 4))
        out["%s_B%d" % (name, B)] = res
        print(name, B, res, flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
