#!/usr/bin/env python3
"""Isolated launches of the decoder's planar-tail layers conv3 / conv2 at the configs[1] (DenseNet161, 352x1216) and
configs[2] (ResNeXt101, 416x544) shapes, B = 16: the fp32 tail kernel these layers run under ``conv_precision = "bf16"``
(ops.conv_forward with tail_planes -> conv_halo_kernel<..,tail>) against the bf16 halo tile with an fp32 tail
(ops.conv_tail_bf16_forward) on the same operands, alternating in one process.  Per layer: warm-up, then ``--rounds``
rounds of ``--iters`` back-to-back launches per kernel between two device events (the order of the two kernels flips every
round).  Prints a table and one JSON document; ``--out`` / ``--table`` also write them.
    python scripts/conv_tail_bf16_bench.py [--iters 200] [--rounds 3] [--out o.json] [--table t.txt]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                  # noqa: E402
from bts_amd import ops                                                       # noqa: E402

LAYERS = (   # name, h, w, c_main, c_out
    ("configs[1] conv3", 88, 304, 224, 128), ("configs[1] conv2", 176, 608, 160, 64),
    ("configs[2] conv3", 104, 136, 384, 128), ("configs[2] conv2", 208, 272, 128, 64),
)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "conv_tail_bf16_bench.py needs a GPU"
    torch.manual_seed(0)
    B = args.batch
    rows, doc = [], {"batch": B, "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "layers": {}}
    for name, h, w, c_main, cout in LAYERS:
        x = torch.randn(B * h * w, c_main, device="cuda")
        plane = torch.randn(B, h, w, device="cuda")
        wt = torch.randn(cout, c_main + 1, 3, 3, device="cuda") / (9.0 * (c_main + 1)) ** 0.5
        wp = ops.pack_conv_weight(wt, c_in_ld=c_main + 4)[0]
        w_main, w_tail = ops.pack_conv_tail_bf16(wt, 1)
        y32, y16 = torch.empty(B * h * w, cout, device="cuda"), torch.empty(B * h * w, cout, device="cuda")

        def fp32_tail():
            with ops.launch_config(fill_frames=16, precision="bf16"):       # the mode's own path for these layers
                ops.conv_forward(x, B, h, w, wp, cout, 3, act=ops.ACT_ELU, y2d=y32, tail_planes=[plane])

        def bf16_tail():
            ops.conv_tail_bf16_forward(x, B, h, w, w_main, w_tail, plane, c_main, cout, y16, act=ops.ACT_ELU)

        fns = (("fp32_tail", fp32_tail), ("bf16_tail", bf16_tail))
        for _, fn in fns:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        diff = float((y16 - y32).abs().max() / y32.abs().max())
        ms = {k: [] for k, _ in fns}
        for r in range(args.rounds):
            for k, fn in (fns if r % 2 == 0 else fns[::-1]):
                ms[k].append(timed(fn, args.iters))
        flops = 2.0 * 9 * B * h * w * cout * (c_main + 1)
        rec = {"h": h, "w": w, "c_main": c_main, "c_out": cout, "max_abs_diff_over_max": diff}
        for k in ms:
            rec[k] = {"ms_rounds": [round(v, 4) for v in ms[k]], "ms_min": min(ms[k]), "ms_max": max(ms[k]),
                      "tflops_at_min": flops / min(ms[k]) * 1e-9}
        spread = max((max(v) - min(v)) / min(v) for v in ms.values())
        rec["spread_rel"] = spread
        rec["speedup_min_over_min"] = min(ms["fp32_tail"]) / min(ms["bf16_tail"])
        rec["speedup_worst_case"] = min(ms["fp32_tail"]) / max(ms["bf16_tail"])
        rec["plan_eligible"] = bool(ops.conv_tail_bf16_plan(h, w, c_main, cout, 1, fill_frames=16).eligible)
        doc["layers"][name] = rec
        rows.append("%-17s %3dx%-4d %3d->%-3d  fp32 tail %s ms   bf16 tail %s ms   x%.2f (worst round x%.2f, spread %.1f %%)  |y16-y32|/max %.1e"
                    % (name, h, w, c_main, cout, " / ".join("%.3f" % v for v in ms["fp32_tail"]),
                       " / ".join("%.3f" % v for v in ms["bf16_tail"]), rec["speedup_min_over_min"], rec["speedup_worst_case"],
                       100 * spread, diff))
        print(rows[-1], flush=True)
    head = "planar-tail layers, B=%d, %d launches per round, %d alternating rounds, ms per launch (%s)" % (
        B, args.iters, args.rounds, doc["device"])
    table = "\n".join([head] + rows) + "\n"
    print(json.dumps(doc, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    if args.table:
        with open(args.table, "w") as f:
            f.write(table)


if __name__ == "__main__":
    main()
