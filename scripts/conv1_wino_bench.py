#!/usr/bin/env python3
"""Isolated launches of the KITTI decoder's conv1 (352x1216, 32 features + 4 depth planes -> 32 channels, ELU, NCHW) at
B = 16 and B = 4 (a sub-batch of the bench's four streams): the halo kernel (ops.conv_forward with tail_planes) against
the fused Winograd kernel (ops.conv_tail_wino_forward) on the same operands.  20 warm-ups, HIP events, 15 launches each
(min / median / max, ms) and executed TFLOP/s at the median.
    python scripts/conv1_wino_bench.py [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bts_amd import ops
torch.manual_seed(0)
h, w = 352, 1216
out = {}
for B in (16, 4):
    x = torch.randn(B * h * w, 32, device="cuda")
    planes = [torch.randn(B, h, w, device="cuda") for _ in range(4)]
    wt = torch.randn(32, 36, 3, 3, device="cuda") / (36 * 9) ** 0.5
    wp = ops.pack_conv_weight(wt, c_in_ld=36)[0]
    u, wtail = ops.pack_conv_tail_wino(wt, 4)
    y = torch.empty(B, 32, h, w, device="cuda")
    def halo():
        with ops.launch_config(fill_frames=16, precision="fp32"):
            ops.conv_forward(x, B, h, w, wp, 32, 3, act=ops.ACT_ELU, y_nchw=y, tail_planes=planes, tag="decoder_conv")
    def wino():
        ops.conv_tail_wino_forward(x, B, h, w, u, wtail, planes, y, act=ops.ACT_ELU)
    res = {}
    for label, fn in (("halo", halo), ("wino", wino)):
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        fn()
        ops.set_trace(None)
        (kern, rec), = tr.summary().items()
        for _ in range(20): fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(15):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            ts.append(s.elapsed_time(e))
        ts.sort()
        med = ts[len(ts) // 2]
        res[label] = dict(kernel=kern, min=round(ts[0], 4), med=round(med, 4), max=round(ts[-1], 4),
                          executed_tflops=round(rec["xflops"] / med * 1e-9, 1), reference_tflops=round(rec["flops"] / med * 1e-9, 1))
    res["speedup_med"] = round(res["halo"]["med"] / res["wino"]["med"], 3)
    out["conv1_B%d" % B] = res
    print("conv1", B, res, flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
