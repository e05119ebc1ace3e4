#!/usr/bin/env python3
"""ResNeXt's grouped 3x3 under the bf16 launch precision: the bundle launch (ops.conv_forward, n_bundles, precision
"bf16" -- the path the encoder takes with grouped_conv_bf16 = "bundles") against the bf16 grouped kernel
(ops.conv_grouped_bf16_forward) on the same operands, BN + ReLU epilogue, fill_frames 16.

Per layer: every stride-1 class with <= 16 channels per group of ResNeXt-101 32x8d and ResNeXt-50 32x4d at 416x544 and
352x1216, once as the B = 16 launch and once as the B = 4 sub-batch launch.  One process, the two forms ALTERNATED: 10 warm-up
pairs, then 21 timed pairs with HIP events; per form min / median / max (ms).  spread = the larger of the two forms'
(max - min) over their 21 identical launches.  The entry rule for "auto": a class enters if at B = 16 the native median beats
the bundle median by more than the spread ("pass16") and at B = 4 the native median is not above the bundle median ("ok4").

Whole model: configs[2] (ResNeXt-101, B = 16, 416x544), conv_precision "bf16", bf16_wide_1x1 "all", one model and two
hipGraphs (GraphedModel keys on the switch) with grouped_conv_bf16 "bundles" and "auto", replayed in alternating pairs whose
order flips every round; medians, the larger spread, a verdict by the same rule.

    python scripts/grouped_bf16_bench.py [--table layers|model|both] [--out profiles/grouped_bf16_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_bench as BB                                                       # noqa: E402  (puts the repository root on sys.path)
from bts_amd import _lib, ops                                                 # noqa: E402

FILL = 16
NETS = {"resnext101_32x8d": ((1, 256, 8), (2, 512, 16)), "resnext50_32x4d": ((1, 128, 4), (2, 256, 8), (3, 512, 16))}


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
    try:
        fn()
    finally:
        ops.set_trace(None)
    (kern, _), = tr.summary().items()
    return kern


def layer_table():
    torch.manual_seed(0)
    table = {}
    for (H, W) in ((416, 544), (352, 1216)):
        for net, layers in NETS.items():
            for li, c, cg in layers:
                h, w, groups = H >> (li + 1), W >> (li + 1), c // cg
                wt = torch.randn(c, cg, 3, 3, device="cuda") / (9 * cg) ** 0.5
                e1 = (torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.1)
                wb, nb, cb = ops.pack_grouped_conv_weight(wt, groups)
                wn = ops.pack_grouped_native_bf16(wt, groups)
                res = {"h": h, "w": w, "c": c, "cg": cg}
                for B in (16, 4):
                    x = torch.randn(B * h * w, c, device="cuda")
                    yb, yn = torch.empty(B * h * w, c, device="cuda"), torch.empty(B * h * w, c, device="cuda")

                    def bundles():
                        with ops.launch_config(fill_frames=FILL, precision="bf16"):
                            ops.conv_forward(x, B, h, w, wb, cb, 3, pad=1, c_in_ld=cb, e1=e1, act=ops.ACT_RELU, y2d=yb, n_bundles=nb,
                                             tag="g3x3", c_in_real=cg)

                    def native():
                        ops.conv_grouped_bf16_forward(x, B, h, w, wn, c, groups, e1=e1, act=ops.ACT_RELU, y2d=yn, tag="g3x3")

                    kb, kn = traced(bundles), traced(native)
                    torch.cuda.synchronize()
                    diff = float((yb - yn).abs().max() / yb.abs().max())
                    tb, tn = timed_pairs(bundles, native, 10, 21)
                    r = {"max_diff_rel": diff}
                    for label, kern, ts in (("bundles", kb, tb), ("native", kn, tn)):
                        r[label] = dict(kernel=kern, min_ms=round(ts[0], 4), med_ms=round(ts[len(ts) // 2], 4), max_ms=round(ts[-1], 4))
                    r["spread_ms"] = round(max(tb[-1] - tb[0], tn[-1] - tn[0]), 4)
                    r["gain_ms"] = round(r["bundles"]["med_ms"] - r["native"]["med_ms"], 4)
                    r["speedup"] = round(r["bundles"]["med_ms"] / r["native"]["med_ms"], 3)
                    res["B%d" % B] = r
                    del x, yb, yn
                res["pass16"] = res["B16"]["gain_ms"] > res["B16"]["spread_ms"]
                res["ok4"] = res["B4"]["gain_ms"] >= 0
                res["enters_auto"] = res["pass16"] and res["ok4"]
                n_ty, n_tx = (h + 7) // 8, (w + 15) // 16
                res["tile_fill"] = round(h * w / (n_ty * 8 * n_tx * 16), 3)
                res["declared_pairs"] = FILL * n_ty * n_tx * (c // 64)
                res["plan_eligible"] = bool(ops.conv_grouped_bf16_plan(h, w, c, groups, precision="bf16", fill_frames=FILL).eligible)
                table["%s_l%d_%dx%d" % (net, li, H, W)] = res
                print(net, "layer%d" % li, (H, W), json.dumps(res), flush=True)
    return table


def whole_model(args):
    from bts_amd import synth
    from bts_amd.graph import GraphedModel
    device = torch.device("cuda", 0)
    cfg = BB.CONFIGS[2]
    model, params = BB.make_model(cfg, device)
    B, H, W = cfg["B"], cfg["H"], cfg["W"]
    image = torch.from_numpy(synth.image_batch(B, H, W, 1234)).to(device)
    focal = torch.from_numpy(synth.focal_values(B, params.dataset, 1234)).to(device)
    model.conv_precision, model.bf16_wide_1x1 = "bf16", "all"
    variants = ("bundles", "auto")
    moved = {}
    with torch.no_grad():
        for v in variants:                           # which launches the switch moves (eager, traced, untimed)
            model.grouped_conv_bf16 = v
            model(image, focal)
            tr = ops.KernelTrace()
            ops.set_trace(tr)
            try:
                model(image, focal)
            finally:
                ops.set_trace(None)
            torch.cuda.synchronize()
            moved[v] = sum(1 for r in tr.records if r[0].startswith("conv_grouped_bf16_kernel<"))
        gm = GraphedModel(model)
        outs, times = {}, {v: [] for v in variants}
        for v in variants:
            model.grouped_conv_bf16 = v
            for _ in range(args.warmup):
                o = gm(image, focal)
            torch.cuda.synchronize()
            outs[v] = [t.clone() for t in o]
        for r in range(args.rounds):
            for v in (variants if r % 2 == 0 else variants[::-1]):
                model.grouped_conv_bf16 = v
                gm(image, focal)                     # one untimed replay: the switch itself is not measured
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                for _ in range(args.steps):
                    gm(image, focal)
                e.record()
                e.synchronize()
                times[v].append(s.elapsed_time(e) / args.steps)
    res = {"run": "configs[2]", "encoder": cfg["encoder"], "batch": B, "height": H, "width": W, "bf16_wide_1x1": "all",
           "steps_per_round": args.steps, "rounds": args.rounds, "hipgraph": True, "captures": gm.captures,
           "sub_batch_streams": model.sub_batches, "launches_on_the_new_kernel_per_forward": moved}
    for v in variants:
        med = statistics.median(times[v])
        res[v] = {"ms_per_step_median": med, "ms_per_step_rounds": [round(x, 3) for x in times[v]],
                  "spread_rel": (max(times[v]) - min(times[v])) / med, "frames_per_s": B * 1000.0 / med}
    gain = res["bundles"]["ms_per_step_median"] / res["auto"]["ms_per_step_median"] - 1.0
    noise = max(res["bundles"]["spread_rel"], res["auto"]["spread_rel"])
    res["gain_of_medians"], res["noise"] = gain, noise
    res["verdict"] = "wins" if gain > noise else ("loses" if -gain > noise else "within spread")
    res["auto_vs_bundles_outputs"] = BB.accuracy(outs["auto"], outs["bundles"])
    print("configs[2]:", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--table", default="both", choices=("layers", "model", "both"))
    ap.add_argument("--steps", type=int, default=8, help="graph replays per timed round")
    ap.add_argument("--rounds", type=int, default=6, help="alternating bundles / auto pairs (at least 3)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "grouped_bf16_bench.py needs a GPU"
    assert args.rounds >= 3
    torch.cuda.set_device(0)
    doc = {"what": "ResNeXt grouped 3x3 under precision bf16: bundle launch vs bf16 grouped kernel, alternating in one process",
           "source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0), "fill_frames": FILL}
    if args.out and os.path.exists(args.out):        # the two tables may be run one at a time into one file
        with open(args.out) as f:
            old = json.load(f)
        doc.update({k: old[k] for k in ("layers", "configs2") if k in old})
    if args.table in ("layers", "both"):
        doc["layers"] = layer_table()
    if args.table in ("model", "both"):
        doc["configs2"] = whole_model(args)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
