#!/usr/bin/env python3
"""What keeping DenseNet161's bottleneck intermediate in bf16 buys (``BtsModel.bf16_mid_storage``).

PER LAYER: a dense layer's pair of launches -- bottleneck 1x1 (BN + ReLU prologue and epilogue, 192 channels) into the
intermediate, 3x3 growth convolution (192 -> 48) out of it into a slice of the block's concat buffer -- at the configs[1]
shapes (352x1216), blocks 1-4, K of the first / a middle / the last-but-one layer.  Form "fp32": the wide bf16 tile writing an
fp32 intermediate (ops.conv1x1_bf16_forward) and ops.conv_forward under precision "bf16" reading it -- the mode with
bf16_wide_1x1 on.  Form "bf16": the same tile writing a bf16 intermediate and ops.conv3x3_bf16in_forward reading it.  Both
alternate in one process: warm-up, then ``--rounds`` rounds of ``--iters`` back-to-back pairs per form between two device
events (the order of the two forms flips every round).  B = 16 and B = 4 (the per-stream sub-batch BtsModel launches), both
declared as fill_frames 16.  Blocks 3 and 4 are measured through the entry points although neither plan query takes them.

WHOLE MODEL: configs[1] in the bf16 mode with bf16_tail_convs and bf16_wide_1x1 on, the switch off and on as two hipGraphs
(GraphedModel keys on it) replayed in alternating pairs in one process.

Decision rule (fixed before measuring, DESIGN 3d's): a class WINS if the gain of its median over the baseline's median
exceeds the larger of the two forms' run-to-run spreads ((max - min) / median over the rounds) in the same run.
Prints a table and one JSON document; ``--out`` / ``--table`` also write them.
    python scripts/bf16_mid_bench.py [--iters 200] [--rounds 5] [--out profiles/bf16_mid_bench.json] [--table profiles/bf16_mid_bench.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_bench as BB                                                       # noqa: E402  (puts the repository root on sys.path)
from bts_amd import ops                                                       # noqa: E402

C_MID, GROWTH = 192, 48
BLOCKS = (   # name, h, w, channels of the block's concat buffer, K of the first / a middle / the last-but-one bottleneck
    ("block1", 88, 304, 384, (96, 240, 336)), ("block2", 44, 152, 768, (192, 480, 720)),
    ("block3", 22, 76, 2112, (384, 1248, 2064)), ("block4", 11, 38, 2208, (1056, 1632, 2160)),
)
HBM_BYTES_PER_S = 6.3e12       # the figure DESIGN uses for the memory bound


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def verdict_of(gain, noise):
    return "wins" if gain > noise else ("loses" if -gain > noise else "within spread")


def layer_pairs(args, doc, rows):
    torch.manual_seed(0)
    for B in args.batches:
        ws = torch.empty(8 * B * 22 * 76 * 512, device="cuda")                # the split-K workspace DenseNetHip lends every layer
        for bname, h, w, cbuf, ks in BLOCKS:
            npix = B * h * w
            buf = torch.randn(npix, cbuf, device="cuda")
            mid32 = torch.empty(npix, C_MID, device="cuda")
            mid16 = torch.empty(npix, C_MID, device="cuda", dtype=torch.bfloat16)
            w2 = ops.pack_conv_weight(torch.randn(GROWTH, C_MID, 3, 3, device="cuda") / (9 * C_MID) ** 0.5)[0]
            plane2 = ops._derived_weight(w2, "_bts_round1", ops.round_bf16)
            with ops.launch_config(fill_frames=16, precision="bf16"):
                takes3 = bool(ops.conv3x3_bf16in_plan(h, w, C_MID, GROWTH).eligible)
            for K in ks:
                x = buf[:, :K]
                wp = ops.pack_conv_weight(torch.randn(C_MID, K, 1, 1, device="cuda") / K ** 0.5)[0]
                plane = ops.round_bf16(wp)
                pre = (torch.rand(K, device="cuda") + 0.5, torch.randn(K, device="cuda") * 0.3)
                e1 = (torch.rand(wp.shape[0], device="cuda") + 0.5, torch.randn(wp.shape[0], device="cuda") * 0.1)
                y_old = torch.empty(npix, cbuf, device="cuda")[:, K:K + GROWTH]
                y_new = torch.empty(npix, cbuf, device="cuda")[:, K:K + GROWTH]

                def fp32_mid():
                    ops.conv1x1_bf16_forward(x, npix, K, plane, C_MID, mid32, pre=pre, pre_relu=True, e1=e1, act=ops.ACT_RELU)
                    with ops.launch_config(fill_frames=16, precision="bf16"):
                        ops.conv_forward(mid32, B, h, w, w2, GROWTH, 3, y2d=y_old, splitk_ws=ws)

                def bf16_mid():
                    ops.conv1x1_bf16_forward(x, npix, K, plane, C_MID, mid16, pre=pre, pre_relu=True, e1=e1, act=ops.ACT_RELU)
                    ops.conv3x3_bf16in_forward(mid16, B, h, w, C_MID, plane2, GROWTH, y_new)

                fns = (("fp32", fp32_mid), ("bf16", bf16_mid))
                for _, fn in fns:
                    for _ in range(10):
                        fn()
                torch.cuda.synchronize()
                identical = bool(torch.equal(y_new, y_old))
                ms = {k: [] for k, _ in fns}
                for r in range(args.rounds):
                    for k, fn in (fns if r % 2 == 0 else fns[::-1]):
                        ms[k].append(timed(fn, args.iters))
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
                gain = med["fp32"] / med["bf16"] - 1.0
                noise = max(spread.values())
                halo = (6.0 / 4.0) * (34.0 / 32.0)                            # the 4x32 tile's patch over its outputs
                nbytes = {k: npix * (4.0 * K + m * C_MID * (1.0 + halo) + 4.0 * GROWTH) + 2.0 * C_MID * (K + 9 * GROWTH)
                          for k, m in (("fp32", 4.0), ("bf16", 2.0))}
                bound_ms = {k: v / HBM_BYTES_PER_S * 1e3 for k, v in nbytes.items()}
                with ops.launch_config(fill_frames=16, precision="bf16"):
                    takes = takes3 and bool(ops.conv1x1_bf16_plan(h, w, K, C_MID).eligible)
                v = verdict_of(gain, noise)
                doc["classes"]["B%d %s K%d" % (B, bname, K)] = {
                    "B": B, "h": h, "w": w, "c_in": K, "x_pix_stride": cbuf, "outputs_bit_identical": identical,
                    "ms_rounds": {k: [round(t, 5) for t in ms[k]] for k in ms}, "ms_median": med, "spread_rel": spread,
                    "gain_of_medians": gain, "verdict": v, "memory_bound_ms": bound_ms,
                    "share_of_memory_bound": {k: bound_ms[k] / med[k] for k in med}, "both_queries_take_it": takes}
                rows.append("B=%-2d %s %3dx%-3d K %4d  fp32 mid %.4f ms (spread %4.1f %%)  bf16 mid %.4f ms (spread %4.1f %%)  gain %+6.1f %%  %-13s"
                            "  mem bound %.4f -> %.4f ms: %3.0f %% -> %3.0f %%  queries %s  bits %s"
                            % (B, bname, h, w, K, med["fp32"], 100 * spread["fp32"], med["bf16"], 100 * spread["bf16"], 100 * gain, v,
                               bound_ms["fp32"], bound_ms["bf16"], 100 * bound_ms["fp32"] / med["fp32"], 100 * bound_ms["bf16"] / med["bf16"],
                               "take" if takes else "leave", "identical" if identical else "DIFFER"))
                print(rows[-1], flush=True)
            del buf, mid32, mid16
        del ws


def whole_model(args, device):
    from bts_amd import synth
    from bts_amd.graph import GraphedModel
    cfg = BB.CONFIGS[1]
    model, params = BB.make_model(cfg, device)
    B, H, W = cfg["B"], cfg["H"], cfg["W"]
    image = torch.from_numpy(synth.image_batch(B, H, W, 1234)).to(device)
    focal = torch.from_numpy(synth.focal_values(B, params.dataset, 1234)).to(device)
    model.conv_precision, model.bf16_tail_convs, model.bf16_wide_1x1 = "bf16", True, True
    variants = (("off", False), ("on", True))
    moved = {}
    with torch.no_grad():
        for key, v in variants:                      # which launches the switch moves (eager, traced, untimed)
            model.bf16_mid_storage = v
            model(image, focal)
            tr = ops.KernelTrace()
            ops.set_trace(tr)
            try:
                model(image, focal)
            finally:
                ops.set_trace(None)
            torch.cuda.synchronize()
            for r in tr.records:
                if r[1].endswith("_mid16"):
                    moved.setdefault(key, {}).setdefault(r[1], 0)
                    moved[key][r[1]] += 1
        gm = GraphedModel(model)
        outs, times = {}, {k: [] for k, _ in variants}
        for key, v in variants:
            model.bf16_mid_storage = v
            for _ in range(args.warmup):
                o = gm(image, focal)
            torch.cuda.synchronize()
            outs[key] = [t.clone() for t in o]
        for r in range(args.model_rounds):
            for key, v in (variants if r % 2 == 0 else variants[::-1]):
                model.bf16_mid_storage = v
                gm(image, focal)                     # one untimed replay: the switch itself is not measured
                times[key].append(timed(lambda: gm(image, focal), args.steps))
    res = {"run": "configs[1]", "encoder": cfg["encoder"], "batch": B, "height": H, "width": W, "steps_per_round": args.steps,
           "rounds": args.model_rounds, "hipgraph": True, "captures": gm.captures, "sub_batch_streams": model.sub_batches,
           "bf16_tail_convs": True, "bf16_wide_1x1": True, "launches_on_the_bf16_intermediate_per_forward": moved.get("on", {}),
           "with_the_switch_off": moved.get("off", {})}
    for key, _ in variants:
        med = statistics.median(times[key])
        res[key] = {"ms_per_step_median": med, "ms_per_step_rounds": [round(v, 3) for v in times[key]],
                    "spread_rel": (max(times[key]) - min(times[key])) / med, "frames_per_s": B * 1000.0 / med}
    gain = res["off"]["ms_per_step_median"] / res["on"]["ms_per_step_median"] - 1.0
    noise = max(res["off"]["spread_rel"], res["on"]["spread_rel"])
    res["gain_of_medians"], res["noise"], res["verdict"] = gain, noise, verdict_of(gain, noise)
    res["outputs_bit_identical"] = all(torch.equal(a, b) for a, b in zip(outs["off"], outs["on"]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200, help="layer pairs per timed round")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds per layer class (at least 3)")
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 4])
    ap.add_argument("--steps", type=int, default=8, help="whole model: graph replays per timed round")
    ap.add_argument("--model-rounds", type=int, default=6, help="whole model: alternating off / on pairs (at least 3; 0 skips it)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bf16_mid_bench.py needs a GPU"
    assert args.rounds >= 3 and (args.model_rounds == 0 or args.model_rounds >= 3)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    t0 = time.time()
    rows = []
    doc = {"what": "DenseNet161 bottleneck intermediate in fp32 vs bf16 (BtsModel.bf16_mid_storage), alternating in one process",
           "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(device), "fill_frames": 16, "classes": {}}
    layer_pairs(args, doc, rows)
    head = ("DenseNet161 dense layer: bottleneck 1x1 (wide bf16 tile, BN+ReLU prologue and epilogue) + 3x3 growth conv, intermediate in "
            "fp32 / in bf16; %d pairs per round, %d alternating rounds, median ms per pair (%s); memory bound = input + intermediate "
            "written and read with the 4x32 tile's halo (x1.59) + slice + bf16 weights at 6.3 TB/s"
            % (args.iters, args.rounds, doc["device"]))
    if args.model_rounds:
        doc["whole_model"] = m = whole_model(args, device)
        rows.append("whole model %s B=%d %dx%d, bf16 + bf16_tail_convs + bf16_wide_1x1, two hipGraphs alternating: off %.3f ms (spread %.1f %%, "
                    "%.1f frames/s)  on %.3f ms (spread %.1f %%, %.1f frames/s)  gain %+.2f %%  %s  outputs %s"
                    % (m["run"], m["batch"], m["height"], m["width"], m["off"]["ms_per_step_median"], 100 * m["off"]["spread_rel"],
                       m["off"]["frames_per_s"], m["on"]["ms_per_step_median"], 100 * m["on"]["spread_rel"], m["on"]["frames_per_s"],
                       100 * m["gain_of_medians"], m["verdict"], "bit-identical" if m["outputs_bit_identical"] else "DIFFER"))
        print(rows[-1], flush=True)
    doc["wall_s"] = round(time.time() - t0, 1)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.table:
        with open(args.table, "w") as f:
            f.write("\n".join([head] + rows) + "\n")


if __name__ == "__main__":
    main()
