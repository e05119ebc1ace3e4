#!/usr/bin/env python3
"""ResNeXt's grouped 3x3, bundle launch (ops.conv_forward, n_bundles) against native launch (ops.conv_grouped_forward) on
the same operands, BN + ReLU epilogue, B = 16: every stride-1 layer class with <= 16 channels per group of ResNeXt-101
32x8d and ResNeXt-50 32x4d at 416x544 and 352x1216.  One process, the two forms ALTERNATED: 10 warm-up pairs, then 21
timed pairs with HIP events; per form min / median / max (ms), algorithmic and executed TFLOP/s at the median and the
median's share of the larger of the FLOP bound (157.3 TF) and the byte bound (6.3 TB/s).  spread = the larger of the two
forms' (max - min) over their 21 identical launches; "pass" = the native median beats the bundle median by more than it.
Then the whole BASELINE configs[2] forward (ResNeXt-101, B = 16, 416x544) with grouped_conv "bundles" and "auto",
alternated, 3 warm-up and 9 timed pairs.
    python scripts/grouped_conv_bench.py [out.json]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bts_amd import _lib, ops

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.3e12
B, FILL = 16, 16
NETS = {"resnext101_32x8d": ((1, 256, 8), (2, 512, 16)), "resnext50_32x4d": ((1, 128, 4), (2, 256, 8), (3, 512, 16))}
torch.manual_seed(0)


def timed_pairs(fa, fb, warm, n):
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(n):
        for fn, ts in ((fa, ta), (fb, tb)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            ts.append(s.elapsed_time(e))
    return sorted(ta), sorted(tb)


def traced(fn):
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    fn()
    ops.set_trace(None)
    (kern, rec), = tr.summary().items()
    return kern, rec


out = {"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0), "B": B, "fill_frames": FILL, "layers": {}}
for (H, W) in ((416, 544), (352, 1216)):
    for net, layers in NETS.items():
        for li, c, cg in layers:
            h, w, groups = H >> (li + 1), W >> (li + 1), c // cg
            x = torch.randn(B * h * w, c, device="cuda")
            wt = torch.randn(c, cg, 3, 3, device="cuda") / (9 * cg) ** 0.5
            e1 = (torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.1)
            wb, nb, cb = ops.pack_grouped_conv_weight(wt, groups)
            wn = ops.pack_grouped_native(wt, groups)
            yb, yn = torch.empty(B * h * w, c, device="cuda"), torch.empty(B * h * w, c, device="cuda")

            def bundles():
                with ops.launch_config(fill_frames=FILL, precision="fp32"):
                    ops.conv_forward(x, B, h, w, wb, cb, 3, pad=1, c_in_ld=cb, e1=e1, act=ops.ACT_RELU, y2d=yb, n_bundles=nb,
                                     tag="g3x3", c_in_real=cg)

            def native():
                ops.conv_grouped_forward(x, B, h, w, wn, c, groups, e1=e1, act=ops.ACT_RELU, y2d=yn, tag="g3x3")

            recs = {"bundles": traced(bundles), "native": traced(native)}
            diff = float((yb - yn).abs().max() / yb.abs().max())
            tb, tn = timed_pairs(bundles, native, 10, 21)
            res = {"h": h, "w": w, "c": c, "cg": cg, "max_diff_rel": diff}
            for label, ts in (("bundles", tb), ("native", tn)):
                kern, rec = recs[label]
                med = ts[len(ts) // 2] * 1e-3
                bound = max(rec["flops"] / PEAK_FLOPS, rec["bytes"] / PEAK_BYTES)
                res[label] = dict(kernel=kern, min_ms=round(ts[0], 4), med_ms=round(med * 1e3, 4), max_ms=round(ts[-1], 4),
                                  algorithmic_tflops=round(rec["flops"] / med * 1e-12, 2),
                                  executed_tflops=round(rec["xflops"] / med * 1e-12, 2), share_of_bound=round(bound / med, 3),
                                  bound="flops" if rec["flops"] / PEAK_FLOPS >= rec["bytes"] / PEAK_BYTES else "bytes")
            res["spread_ms"] = round(max(tb[-1] - tb[0], tn[-1] - tn[0]), 4)
            res["gain_ms"] = round(res["bundles"]["med_ms"] - res["native"]["med_ms"], 4)
            res["pass"] = res["gain_ms"] > res["spread_ms"]
            res["plan_eligible"] = bool(ops.conv_grouped_plan(h, w, c, groups, precision="fp32", fill_frames=FILL).eligible)
            out["layers"]["%s_l%d_%dx%d" % (net, li, H, W)] = res
            print(net, "layer%d" % li, (H, W), json.dumps(res), flush=True)
            del x, yb, yn

# ---- the whole configs[2] forward
import bench
Params = type("Params", (), {})
p = Params()
p.encoder, p.bts_size, p.max_depth, p.dataset = "resnext101_bts", 512, 10.0, "nyu"
model = bench.build_model(p, torch.device("cuda"))
xi = torch.randn(B, 3, 416, 544, device="cuda")
focal = torch.full((B,), 518.8579, device="cuda")


def forward(mode):
    def run():
        model.grouped_conv = mode
        with torch.no_grad():
            return model(xi, focal)
    return run


ref, got = forward("bundles")(), forward("auto")()
tb, ta = timed_pairs(forward("bundles"), forward("auto"), 3, 9)
out["configs2_forward"] = dict(bundles_ms=[round(t, 3) for t in (tb[0], tb[len(tb) // 2], tb[-1])],
                               auto_ms=[round(t, 3) for t in (ta[0], ta[len(ta) // 2], ta[-1])],
                               final_depth_max_rel_diff=float(((ref[4] - got[4]).abs() / ref[4].abs().clamp_min(1e-30)).max()))
print("configs[2] forward (min, median, max ms):", json.dumps(out["configs2_forward"]), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
