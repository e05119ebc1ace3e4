#!/usr/bin/env python3
"""Whole-model frames/s of the bf16 inference mode with ``BtsModel.bf16_wide_1x1`` off and at "all" (DESIGN 3c): one model,
two hipGraphs (GraphedModel keys on the switch), replayed in alternating pairs in one process -- the order of the pair flips
every round.  configs[2] (ResNeXt-101, B = 16, 416x544) and DenseNet121 at 352x1216, B = 16.  Reports the median and the
run-to-run spread ((max - min) / median over the rounds) of both, the gain of the medians, a verdict by the rule of the
per-layer bench (a win only outside the larger spread), and whether the outputs are bit-identical.

    python scripts/bf16_wide_all_bench.py [--rounds 6] [--steps 8] [--out profiles/bf16_wide_1x1_all_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_bench as BB                                                       # noqa: E402  (puts the repository root on sys.path)

RUNS = {
    "configs[2]": BB.CONFIGS[2],
    "densenet121": dict(encoder="densenet121_bts", dataset="kitti", max_depth=80.0, B=16, H=352, W=1216),
}


def run(name, cfg, args, device):
    from bts_amd import ops, synth
    from bts_amd.graph import GraphedModel
    model, params = BB.make_model(cfg, device)
    B, H, W = cfg["B"], cfg["H"], cfg["W"]
    image = torch.from_numpy(synth.image_batch(B, H, W, 1234)).to(device)
    focal = torch.from_numpy(synth.focal_values(B, params.dataset, 1234)).to(device)
    model.conv_precision = "bf16"
    variants = (("off", False), ("all", "all"))
    moved = {}
    with torch.no_grad():
        for key, v in variants:                      # which launches the switch moves (eager, traced, untimed)
            model.bf16_wide_1x1 = v
            model(image, focal)
            tr = ops.KernelTrace()
            ops.set_trace(tr)
            try:
                model(image, focal)
            finally:
                ops.set_trace(None)
            torch.cuda.synchronize()
            for r in tr.records:
                if r[0].startswith("conv1x1_bf16_kernel<"):
                    moved.setdefault(key, {}).setdefault(r[1], 0)
                    moved[key][r[1]] += 1
        gm = GraphedModel(model)
        outs, times = {}, {k: [] for k, _ in variants}
        for key, v in variants:
            model.bf16_wide_1x1 = v
            for _ in range(args.warmup):
                o = gm(image, focal)
            torch.cuda.synchronize()
            outs[key] = [t.clone() for t in o]
        for r in range(args.rounds):
            for key, v in (variants if r % 2 == 0 else variants[::-1]):
                model.bf16_wide_1x1 = v
                gm(image, focal)                     # one untimed replay: the switch itself is not measured
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                for _ in range(args.steps):
                    gm(image, focal)
                e.record()
                e.synchronize()
                times[key].append(s.elapsed_time(e) / args.steps)
    res = {"run": name, "encoder": cfg["encoder"], "batch": B, "height": H, "width": W, "steps_per_round": args.steps,
           "rounds": args.rounds, "hipgraph": True, "captures": gm.captures, "sub_batch_streams": model.sub_batches,
           "launches_on_the_wide_tile_per_forward": moved.get("all", {}), "with_the_switch_off": moved.get("off", {})}
    for key, _ in variants:
        med = statistics.median(times[key])
        res[key] = {"ms_per_step_median": med, "ms_per_step_rounds": [round(v, 3) for v in times[key]],
                    "spread_rel": (max(times[key]) - min(times[key])) / med, "frames_per_s": B * 1000.0 / med}
    gain = res["off"]["ms_per_step_median"] / res["all"]["ms_per_step_median"] - 1.0
    noise = max(res["off"]["spread_rel"], res["all"]["spread_rel"])
    res["gain_of_medians"] = gain
    res["noise"] = noise
    res["verdict"] = "wins" if gain > noise else ("loses" if -gain > noise else "within spread")
    res["outputs_bit_identical"] = all(torch.equal(a, b) for a, b in zip(outs["off"], outs["all"]))
    res["all_vs_off_outputs"] = BB.accuracy(outs["all"], outs["off"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", default="configs[2],densenet121")
    ap.add_argument("--steps", type=int, default=8, help="graph replays per timed round")
    ap.add_argument("--rounds", type=int, default=6, help="alternating off / all pairs (at least 3)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bf16_wide_all_bench.py needs a GPU"
    assert args.rounds >= 3
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    t0 = time.time()
    results = [run(n, RUNS[n], args, device) for n in args.runs.split(",") if n.strip()]
    doc = {"what": 'whole-model frames/s, bf16 inference mode, BtsModel.bf16_wide_1x1 off vs "all", alternating pairs in one process',
           "device": torch.cuda.get_device_name(device), "wall_s": round(time.time() - t0, 1), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
