#!/usr/bin/env python3
"""Isolated launches of DenseNet161's bottleneck 1x1 layers (c_out 192) at the configs[1] shapes (352x1216): the path they
run under ``conv_precision = "bf16"`` today (ops.conv_forward under precision 2 -> the row-tiled bf16 kernel) against the
wide bf16 tile (ops.conv1x1_bf16_forward) on the same operands, alternating in one process.  Per class: the input is a
channel-prefix view of a buffer as wide as the block's concat buffer, BN + ReLU prologue and epilogue on; warm-up, then
``--rounds`` rounds of ``--iters`` back-to-back launches per form between two device events (the order of the two forms
flips every round).  B = 16 and B = 4 (the per-stream sub-batch BtsModel launches), both declared as fill_frames 16.

Decision rule (fixed before measuring, DESIGN 3d's): a class WINS if the gain of its median over the baseline's median
exceeds the larger of the two forms' run-to-run spreads ((max - min) / median over the rounds) in the same run.
Prints a table and one JSON document; ``--out`` / ``--table`` also write them.
    python scripts/conv1x1_bf16_bench.py [--iters 500] [--rounds 5] [--out o.json] [--table t.txt]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                  # noqa: E402
from bts_amd import ops                                                       # noqa: E402

C_OUT = 192
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 4])
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "conv1x1_bf16_bench.py needs a GPU"
    assert args.rounds >= 3
    torch.manual_seed(0)
    rows = []
    doc = {"iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "fill_frames": 16, "classes": {}}
    for B in args.batches:
        ws = torch.empty(8 * B * 22 * 76 * 512, device="cuda")                # the split-K workspace DenseNetHip lends every layer
        for bname, h, w, cbuf, ks in BLOCKS:
            npix = B * h * w
            buf = torch.randn(npix, cbuf, device="cuda")
            for K in ks:
                x = buf[:, :K]
                wt = torch.randn(C_OUT, K, 1, 1, device="cuda") / K ** 0.5
                wp = ops.pack_conv_weight(wt)[0]
                plane = ops.round_bf16(wp)
                pre = (torch.rand(K, device="cuda") + 0.5, torch.randn(K, device="cuda") * 0.3)
                e1 = (torch.rand(wp.shape[0], device="cuda") + 0.5, torch.randn(wp.shape[0], device="cuda") * 0.1)
                y_old, y_new = torch.empty(npix, C_OUT, device="cuda"), torch.empty(npix, C_OUT, device="cuda")

                def row_tiled():
                    with ops.launch_config(fill_frames=16, precision="bf16"):
                        ops.conv_forward(x, B, h, w, wp, C_OUT, 1, pre=pre, pre_relu=True, e1=e1, act=ops.ACT_RELU, y2d=y_old,
                                         splitk_ws=ws)

                def wide():
                    ops.conv1x1_bf16_forward(x, npix, K, plane, C_OUT, y_new, pre=pre, pre_relu=True, e1=e1, act=ops.ACT_RELU)

                fns = (("row_tiled", row_tiled), ("wide", wide))
                for _, fn in fns:
                    for _ in range(10):
                        fn()
                torch.cuda.synchronize()
                diff = float((y_new - y_old).abs().max() / y_old.abs().max())
                ms = {k: [] for k, _ in fns}
                for r in range(args.rounds):
                    for k, fn in (fns if r % 2 == 0 else fns[::-1]):
                        ms[k].append(timed(fn, args.iters))
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
                gain = med["row_tiled"] / med["wide"] - 1.0
                noise = max(spread.values())
                nbytes = 4.0 * npix * (K + C_OUT) + 2.0 * C_OUT * K
                bound_ms = nbytes / HBM_BYTES_PER_S * 1e3
                with ops.launch_config(fill_frames=16, precision="bf16"):
                    eligible = bool(ops.conv1x1_bf16_plan(h, w, K, C_OUT).eligible)
                verdict = "wins" if gain > noise else ("loses" if -gain > noise else "within spread")
                rec = {"B": B, "h": h, "w": w, "c_in": K, "x_pix_stride": cbuf, "max_abs_diff_over_max": diff,
                       "ms_rounds": {k: [round(v, 5) for v in ms[k]] for k in ms}, "ms_median": med, "spread_rel": spread,
                       "gain_of_medians": gain, "verdict": verdict, "memory_bound_ms": bound_ms,
                       "share_of_memory_bound": {k: bound_ms / med[k] for k in med}, "plan_eligible": eligible}
                doc["classes"]["B%d %s K%d" % (B, bname, K)] = rec
                rows.append("B=%-2d %s %3dx%-3d K %4d  row-tiled %.4f ms (spread %4.1f %%)  wide %.4f ms (spread %4.1f %%)  gain %+6.1f %%  %-13s"
                            "  mem bound %.4f ms: %3.0f %% -> %3.0f %%  plan %s  |new-old|/max %.1e"
                            % (B, bname, h, w, K, med["row_tiled"], 100 * spread["row_tiled"], med["wide"], 100 * spread["wide"],
                               100 * gain, verdict, bound_ms, 100 * bound_ms / med["row_tiled"], 100 * bound_ms / med["wide"],
                               "takes" if eligible else "leaves", diff))
                print(rows[-1], flush=True)
    head = ("DenseNet161 bottleneck 1x1 (c_out 192), prefix view of the block buffer, BN+ReLU prologue and epilogue; %d launches per "
            "round, %d alternating rounds, median ms per launch (%s); memory bound = fp32 activations + bf16 weights at 6.3 TB/s"
            % (args.iters, args.rounds, doc["device"]))
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
