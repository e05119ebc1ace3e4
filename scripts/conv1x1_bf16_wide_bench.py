#!/usr/bin/env python3
"""Per-layer bench of the wide bf16 1x1 tile at 128 / 256 output channels per workgroup (ops.conv1x1_bf16_wide_forward) on the
1x1 layers of ResNeXt-101 and ResNet-50 (416x544) and DenseNet121 (352x1216) against the path they run under
``conv_precision = "bf16"`` today (ops.conv_forward under precision 2), on the same operands, alternating in one process.

``--share``: first, one eager bf16 forward of configs[2] (ResNeXt-101, B = 16, 416x544) under ops.KernelTrace, and the time of
the launches tagged ``enc_l*_1x1`` / ``enc_l*_down`` as a share of all launches of the step (a profiler's kernel table names
kernels, not tags: profiles/bf16_config2_forward_kernel_stats.csv cannot separate these layers from the others on the same kernels).
The same figure in kernel time: ``rocprofv3 --kernel-trace --stats ... -- python scripts/conv1x1_bf16_wide_bench.py --trace-records
r.json``, then ``--join-kernel-trace <the run's kernel_trace.csv> --trace-records r.json`` lines the dispatches up with the tags.

Per class (encoder, stage, layer form, K): warm-up, then ``--rounds`` rounds of ``--iters`` back-to-back launches per form
between two device events (the order of the forms flips every round), as the B = 16 launch and as the B = 4 sub-batch launch
BtsModel really enqueues per stream, both declared as fill_frames 16.

Decision rule (fixed before measuring; the one that set kC1bMinWgs): a tile WINS a class if the gain of its median over the
baseline's median exceeds the larger run-to-run spread ((max - min) / median over the rounds) of the two forms at B = 16 AND
it does not lose by more than the spread at B = 4.  The same rule settles 128 against 256 for a width.
    python scripts/conv1x1_bf16_wide_bench.py [--share] [--iters 300] [--rounds 5] [--out o.json] [--table t.txt]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                  # noqa: E402
from bts_amd import ops                                                       # noqa: E402

R = (104, 136), (52, 68), (26, 34), (13, 17)        # ResNe(X)t stage maps of a 416x544 image
D = (88, 304), (44, 152), (22, 76), (11, 38)        # DenseNet block maps of a 352x1216 image
# (encoder, stage, form, (h, w), c_in, c_out, x_pix_stride).  Forms: conv1 = e1 + ReLU; conv3 = e1 + identity + ReLU (+ the skip
# tap on the stage's last block: "conv3+y2"); down = e1 only (stride 1: layer 1); dense = BN+ReLU prologue, e1 + ReLU, a
# channel-prefix view of the block's concat buffer.
CLASSES = (
    ("resnext101", "l1", "conv1", R[0], 64, 256, 64), ("resnext101", "l1", "conv1", R[0], 256, 256, 256),
    ("resnext101", "l1", "down", R[0], 64, 256, 64), ("resnext101", "l1", "conv3", R[0], 256, 256, 256),
    ("resnext101", "l1", "conv3+y2", R[0], 256, 256, 256),
    ("resnext101", "l2", "conv1", R[0], 256, 512, 256), ("resnext101", "l2", "conv1", R[1], 512, 512, 512),
    ("resnext101", "l2", "conv3", R[1], 512, 512, 512),
    ("resnext101", "l3", "conv1", R[1], 512, 1024, 512), ("resnext101", "l3", "conv1", R[2], 1024, 1024, 1024),
    ("resnext101", "l3", "conv3", R[2], 1024, 1024, 1024),
    ("resnext101", "l4", "conv1", R[2], 1024, 2048, 1024), ("resnext101", "l4", "conv1", R[3], 2048, 2048, 2048),
    ("resnext101", "l4", "conv3", R[3], 2048, 2048, 2048),
    ("resnet50", "l1", "down", R[0], 64, 256, 64), ("resnet50", "l1", "conv3", R[0], 64, 256, 64),
    ("resnet50", "l2", "conv1", R[0], 256, 128, 256), ("resnet50", "l2", "conv1", R[1], 512, 128, 512),
    ("resnet50", "l2", "conv3", R[1], 128, 512, 128),
    ("resnet50", "l3", "conv1", R[1], 512, 256, 512), ("resnet50", "l3", "conv1", R[2], 1024, 256, 1024),
    ("resnet50", "l3", "conv3", R[2], 256, 1024, 256),
    ("resnet50", "l4", "conv1", R[2], 1024, 512, 1024), ("resnet50", "l4", "conv1", R[3], 2048, 512, 2048),
    ("resnet50", "l4", "conv3", R[3], 512, 2048, 512),
    ("densenet121", "b1", "dense", D[0], 64, 128, 256), ("densenet121", "b1", "dense", D[0], 224, 128, 256),
    ("densenet121", "b2", "dense", D[1], 128, 128, 512), ("densenet121", "b2", "dense", D[1], 480, 128, 512),
    ("densenet121", "b3", "dense", D[2], 256, 128, 1024), ("densenet121", "b3", "dense", D[2], 992, 128, 1024),
    ("densenet121", "b4", "dense", D[3], 512, 128, 1024), ("densenet121", "b4", "dense", D[3], 992, 128, 1024),
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


def share_of_step():
    """The 1x1 layers' own share of an eager bf16 configs[2] forward, by launch tag (per-launch HIP events)."""
    model, image, focal = _configs2_bf16()
    with torch.no_grad():
        for _ in range(2):
            model(image, focal)
        torch.cuda.synchronize()
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            model(image, focal)
        finally:
            ops.set_trace(None)
    tags = {}
    for kern, d in tr.summary().items():
        for tag, t in d["tags"].items():
            e = tags.setdefault(tag, {"ms": 0.0, "launches": 0, "kernels": {}})
            e["ms"] += t["ms"]
            e["launches"] += t["launches"]
            e["kernels"][kern] = round(e["kernels"].get(kern, 0.0) + t["ms"], 4)
    total = sum(t["ms"] for t in tags.values())
    one = {k: v for k, v in tags.items() if k.startswith("enc_l") and (k.endswith("_1x1") or k.endswith("_down"))}
    doc = {"config": 2, "sub_batch_streams": model.sub_batches, "sum_of_launch_ms": total,
           "enc_1x1_and_down_ms": sum(v["ms"] for v in one.values()),
           "share": sum(v["ms"] for v in one.values()) / total, "tags": {k: tags[k] for k in sorted(one)}}
    lines = ["1x1 layers' share of one eager bf16 configs[2] forward (ResNeXt-101, B = 16, 416x544; per-launch events, %d sub-batch "
             "streams): %.3f ms of %.3f ms summed over all launches = %.1f %%"
             % (model.sub_batches, doc["enc_1x1_and_down_ms"], total, 100 * doc["share"])]
    for k in sorted(one):
        lines.append("  %-12s %4d launches %8.3f ms  %5.1f %%  %s" % (k, one[k]["launches"], one[k]["ms"], 100 * one[k]["ms"] / total,
                                                                     one[k]["kernels"]))
    return doc, lines


def _configs2_bf16():
    import bf16_bench as BB
    from bts_amd import synth
    dev = torch.device("cuda", 0)
    cfg = BB.CONFIGS[2]
    model, params = BB.make_model(cfg, dev)
    B, H, W = cfg["B"], cfg["H"], cfg["W"]
    image = torch.from_numpy(synth.image_batch(B, H, W, 1234)).to(dev)
    focal = torch.from_numpy(synth.focal_values(B, params.dataset, 1234)).to(dev)
    BB.set_variant(model, "bf16")
    return model, image, focal


def write_records(path, forwards=3):
    """The program to run under ``rocprofv3 --kernel-trace``: ``forwards`` eager bf16 configs[2] forwards, every launch recorded
    (kernel, tag) in enqueue order -- what join_kernel_trace() lines up with the profiler's dispatches."""
    model, image, focal = _configs2_bf16()
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        with torch.no_grad():
            for _ in range(forwards):
                model(image, focal)
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump({"forwards": forwards, "records": [[r[0], r[1]] for r in tr.records]}, f)


def join_kernel_trace(csv_path, records_path):
    """Host only.  The row-tiled conv launches of the recorded forwards, in enqueue order, against the profiler's
    ``conv_fwd_kernel`` dispatches in dispatch order: same count, same <BM, BN> pair by pair, or this raises.  Then kernel time by
    launch tag over the LAST forward, against the kernel time of every dispatch from that forward's first conv on."""
    import csv
    import re
    doc = json.load(open(records_path))
    recs = [(k, t) for k, t in doc["records"] if k.startswith("conv_fwd_kernel<")]
    rows = list(csv.DictReader(open(csv_path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    disp = [(i, r) for i, r in enumerate(rows) if "conv_fwd_kernel<" in r["Kernel_Name"]]
    assert len(disp) == len(recs), "dispatches %d != recorded launches %d" % (len(disp), len(recs))
    tile = lambda name: tuple(int(v) for v in re.search(r"conv_fwd_kernel<\s*(\d+)\s*,\s*(\d+)", name).groups())
    for (_, r), (k, _) in zip(disp, recs):
        assert tile(r["Kernel_Name"]) == tile(k), (r["Kernel_Name"], k)
    n = len(recs) // doc["forwards"]
    last = list(zip(disp, recs))[-n:]
    ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
    total = sum(ms(r) for r in rows[last[0][0][0]:])
    tags = {}
    for (_, r), (k, t) in last:
        e = tags.setdefault(t, [0, 0.0])
        e[0] += 1
        e[1] += ms(r)
    one = {t: v for t, v in tags.items() if t.startswith("enc_l") and (t.endswith("_1x1") or t.endswith("_down"))}
    part = sum(v[1] for v in one.values())
    lines = ["rocprofv3 --kernel-trace of the same forward: the launches tagged enc_l*_1x1 / enc_l*_down take %.3f ms of %.3f ms "
             "kernel time = %.1f %% (%d row-tiled conv dispatches matched to their launches one to one)" % (part, total, 100 * part / total, n)]
    for t in sorted(one):
        lines.append("  %-12s %4d launches %8.3f ms  %5.1f %%" % (t, one[t][0], one[t][1], 100 * one[t][1] / total))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-records", default=None, help="run the forwards to profile and write their (kernel, tag) list here")
    ap.add_argument("--join-kernel-trace", default=None, help="host only: rocprofv3's kernel-trace CSV to join with --trace-records")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 4])
    ap.add_argument("--share", action="store_true", help="first measure the 1x1 layers' share of the bf16 configs[2] forward")
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", default=None)
    args = ap.parse_args()
    if args.join_kernel_trace:
        text = "\n".join(join_kernel_trace(args.join_kernel_trace, args.trace_records))
        print(text)
        if args.table:
            with open(args.table, "w") as f:
                f.write(text + "\n")
        return
    assert torch.cuda.is_available(), "conv1x1_bf16_wide_bench.py needs a GPU"
    if args.trace_records:
        return write_records(args.trace_records)
    assert args.rounds >= 3
    torch.manual_seed(0)
    doc = {"iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "fill_frames": 16, "classes": {}}
    rows = []
    if args.share:
        doc["share"], lines = share_of_step()
        rows += lines
        print("\n".join(lines), flush=True)
    verdicts = {}
    for enc, stage, form, (h, w), K, N, xs in CLASSES:
        bns = [b for b in (128, 256) if N % b == 0]                          # every width here is a multiple of 128
        for B in args.batches:
            npix = B * h * w
            ws = torch.empty(8 * B * 52 * 68 * 512, device="cuda")            # the split-K workspace the encoders lend every layer
            buf = torch.randn(npix, xs, device="cuda")
            x = buf[:, :K]
            wt = torch.randn(N, K, 1, 1, device="cuda") / K ** 0.5
            wp = ops.pack_conv_weight(wt)[0]
            plane = ops.round_bf16(wp)
            pre = (torch.rand(K, device="cuda") + 0.5, torch.randn(K, device="cuda") * 0.3) if form == "dense" else None
            e1 = (torch.rand(wp.shape[0], device="cuda") + 0.5, torch.randn(wp.shape[0], device="cuda") * 0.1)
            res = torch.randn(npix, N, device="cuda") if form.startswith("conv3") else None
            y2_old = torch.empty(npix, N, device="cuda") if form.endswith("+y2") else None
            y2_new = torch.empty(npix, N, device="cuda") if form.endswith("+y2") else None
            act = ops.ACT_NONE if form == "down" else ops.ACT_RELU
            y_old, y_new = torch.empty(npix, N, device="cuda"), torch.empty(npix, N, device="cuda")

            def base():
                with ops.launch_config(fill_frames=16, precision="bf16"):
                    ops.conv_forward(x, B, h, w, wp, N, 1, pre=pre, pre_relu=pre is not None, e1=e1, act=act, y2d=y_old, res2d=res,
                                     y2_2d=y2_old, splitk_ws=ws)

            def wide(bn):
                return lambda: ops.conv1x1_bf16_wide_forward(x, npix, K, plane, N, y_new, pre=pre, pre_relu=pre is not None, e1=e1,
                                                             res2d=res, y2_2d=y2_new, act=act, bn=bn)

            fns = [("base", base)] + [("bn%d" % b, wide(b)) for b in bns]
            diff = {}
            for k, fn in fns:
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                if k != "base":
                    diff[k] = float((y_new - y_old).abs().max() / y_old.abs().max())
            ms = {k: [] for k, _ in fns}
            for r in range(args.rounds):
                for k, fn in (fns if r % 2 == 0 else fns[::-1]):
                    ms[k].append(timed(fn, args.iters))
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
            with ops.launch_config(fill_frames=16, precision="bf16"):
                plan = tuple(ops.conv1x1_bf16_wide_plan(h, w, K, N, has_res=res is not None))
            name = "%s %s %s %dx%d K%d N%d" % (enc, stage, form, h, w, K, N)
            rec = {"B": B, "ms_rounds": {k: [round(v, 5) for v in ms[k]] for k in ms}, "ms_median": med, "spread_rel": spread,
                   "max_abs_diff_over_max": diff, "plan": plan, "tiles": {}}
            cells = []
            for b in bns:
                k = "bn%d" % b
                gain = med["base"] / med[k] - 1.0
                noise = max(spread["base"], spread[k])
                v = "wins" if gain > noise else ("loses" if -gain > noise else "within spread")
                rec["tiles"][k] = {"gain_of_medians": gain, "noise": noise, "verdict": v,
                                   "declared_workgroups": 16 * ((h * w + 127) // 128) * (N // b)}
                verdicts.setdefault(name, {}).setdefault(b, {})[B] = v
                cells.append("bn%d %.4f ms (spread %4.1f %%) gain %+6.1f %% %-13s" % (b, med[k], 100 * spread[k], 100 * gain, v))
            if len(bns) == 2:
                g = med["bn128"] / med["bn256"] - 1.0
                n = max(spread["bn128"], spread["bn256"])
                rec["bn256_over_bn128"] = {"gain_of_medians": g, "noise": n,
                                           "verdict": "wins" if g > n else ("loses" if -g > n else "within spread")}
                cells.append("256 over 128 %+6.1f %% %s" % (100 * g, rec["bn256_over_bn128"]["verdict"]))
            doc["classes"]["B%d %s" % (B, name)] = rec
            rows.append("B=%-2d %-46s base %.4f ms (spread %4.1f %%)  %s  plan %s  |new-old|/max %.1e"
                        % (B, name, med["base"], 100 * spread["base"], "  ".join(cells), plan, max(diff.values())))
            print(rows[-1], flush=True)
    for name, per_bn in verdicts.items():
        for b, v in per_bn.items():
            ok = v.get(16) == "wins" and v.get(4) in ("wins", "within spread")
            rows.append("class %-46s bn%d: B=16 %-13s B=4 %-13s -> %s" % (name, b, v.get(16), v.get(4), "ENTERS" if ok else "stays"))
            print(rows[-1], flush=True)
    head = ("1x1 layers on the wide bf16 tile at bn 128 / 256 (ops.conv1x1_bf16_wide_forward) against ops.conv_forward under precision "
            "bf16, fill_frames 16; %d launches per round, %d alternating rounds, median ms per launch (%s)"
            % (args.iters, args.rounds, doc["device"]))
    table = "\n".join([head] + rows) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    if args.table:
        with open(args.table, "w") as f:
            f.write(table)


if __name__ == "__main__":
    main()
