#!/usr/bin/env python3
"""ResNeXt's grouped 3x3 in the TRAINING step, bundle form against native form on the same operands, at the training
configuration's maps (B = 4, 352x704): the five stride-1 layer classes with <= 16 channels per group of ResNeXt-101 32x8d and
ResNeXt-50 32x4d, each pass on its own --

  forward  ops.conv_forward(n_bundles)                          |  ops.conv_grouped_forward
  dgrad    the same two on dy with the input-gradient packs     (train.WeightPacker DGRAD | DGRAD_NATIVE)
  wgrad    ops.conv_wgrad(n_bundles) + its reduce + the torch gather / permute / contiguous of train._ConvFn
                                                                |  ops.conv_grouped_wgrad + its reduce

One process, the two forms ALTERNATED: 10 warm-up pairs, then 21 timed pairs with HIP events; per form min / median / max (ms),
algorithmic and executed TFLOP/s at the median against the 157.3 TF fp32-MFMA figure.  spread = the larger of the two forms'
(max - min); "pass" = the native median beats the bundle median by more than it (the rule train._grouped_native_layer's
shape rule was checked against).

--whole-step: scripts/train_bench.py as fresh child processes, with and without --grouped-native in alternating pairs
(3 pairs per encoder, resnext101_bts and resnext50_bts), median step time of each form.

    python scripts/grouped_train_bench.py [--whole-step [--encoders=a,b]] [out.json]     (an existing out.json is extended)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = 157.3e12
B, H, W = 4, 352, 704
NETS = {"resnext101_32x8d": ((1, 256, 8), (2, 512, 16)), "resnext50_32x4d": ((1, 128, 4), (2, 256, 8), (3, 512, 16))}


def whole_step(encoders, pairs=3):
    res = {}
    for enc in encoders:
        ms = {"bundles": [], "native": []}
        for _ in range(pairs):
            for label, extra in (("bundles", []), ("native", ["--grouped-native"])):
                cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_bench.py"), "--encoder", enc, "--batch", str(B),
                       "--height", str(H), "--width", str(W), "--steps", "10", "--warmup", "3"] + extra
                line = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=240).stdout.decode().strip().splitlines()[-1]
                ms[label].append(round(json.loads(line)["ms_per_step"], 2))
                print(enc, label, ms[label][-1], "ms/step", flush=True)
        res[enc] = {k: dict(ms_per_step=v, median=sorted(v)[len(v) // 2]) for k, v in ms.items()}
        res[enc]["gain_ms"] = round(res[enc]["bundles"]["median"] - res[enc]["native"]["median"], 2)
    return res


def layers():
    import torch
    from bts_amd import _lib, ops, train
    torch.manual_seed(0)
    P = train.WeightPacker

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
        """(kernel names, executed flops) of the library launches of one call."""
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        fn()
        ops.set_trace(None)
        summ = tr.summary()
        return sorted(summ), sum(d["xflops"] for d in summ.values())

    out = {"source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0), "B": B, "image": [H, W], "layers": {}}
    ws = train._workspace(torch.device("cuda", 0))
    for net, ls in NETS.items():
        for li, c, cg in ls:
            h, w, groups = H >> (li + 1), W >> (li + 1), c // cg
            x = torch.randn(B * h * w, c, device="cuda")
            dy = torch.randn(B * h * w, c, device="cuda")
            wt = torch.randn(c, cg, 3, 3, device="cuda") / (9 * cg) ** 0.5
            cb = P.bundle_channels(wt, groups)
            nb, gpb = c // cb, cb // cg
            packs = {m: train._PACKER.get(wt, 0 if m >= 2 else cb, m, groups) for m in (P.FWD, P.DGRAD, P.FWD_NATIVE, P.DGRAD_NATIVE)}
            yb, yn = torch.empty(B * h * w, c, device="cuda"), torch.empty(B * h * w, c, device="cuda")
            keep = {}

            def conv_bundles(src, mode):
                def run():
                    with ops.launch_config(fill_frames=ops.auto_fill_frames(B), precision="fp32"):   # the training model's declaration
                        ops.conv_forward(src, B, h, w, packs[mode], cb, 3, pad=1, c_in_ld=cb, y2d=yb, n_bundles=nb, c_in_real=cg)
                    keep["b"] = yb
                return run

            def conv_native(src, mode):
                def run():
                    ops.conv_grouped_forward(src, B, h, w, packs[mode], c, groups, y2d=yn)
                    keep["n"] = yn
                return run

            def wgrad_bundles():
                g = ops.conv_wgrad(x, B, h, w, cb, dy, cb, 3, pad=1, ws=ws, n_bundles=nb)
                idx = torch.arange(gpb, device="cuda")
                diag = g.view(nb, gpb, cg, 9, gpb, cg)[:, idx, :, :, idx, :]
                keep["b"] = diag.permute(1, 0, 2, 4, 3).reshape(c, cg, 3, 3).contiguous()

            def wgrad_native():
                keep["n"] = ops.conv_grouped_wgrad(x, B, h, w, dy, c, groups, ws=ws)

            res = {"h": h, "w": w, "c": c, "cg": cg,
                   "wgrad_splits": ops.conv_grouped_wgrad_plan(B, h, w, c, groups, ws.numel())[0]}
            for pname, fb, fn in (("forward", conv_bundles(x, P.FWD), conv_native(x, P.FWD_NATIVE)),
                                  ("dgrad", conv_bundles(dy, P.DGRAD), conv_native(dy, P.DGRAD_NATIVE)),
                                  ("wgrad", wgrad_bundles, wgrad_native)):
                recs = {"bundles": traced(fb), "native": traced(fn)}
                r = {"max_diff_rel": float((keep["b"] - keep["n"]).abs().max() / keep["b"].abs().max())}
                tb, tn = timed_pairs(fb, fn, 10, 21)
                for label, ts in (("bundles", tb), ("native", tn)):
                    kerns, xflops = recs[label]
                    flops = 2.0 * B * h * w * c * cg * 9              # algorithmic: the grouped operator's own products
                    med = ts[len(ts) // 2] * 1e-3
                    r[label] = dict(kernels=kerns, min_ms=round(ts[0], 4), med_ms=round(med * 1e3, 4), max_ms=round(ts[-1], 4),
                                    algorithmic_tflops=round(flops / med * 1e-12, 2), executed_tflops=round(xflops / med * 1e-12, 2),
                                    executed_share_of_157_tf=round(xflops / med / PEAK_FLOPS, 3))
                r["spread_ms"] = round(max(tb[-1] - tb[0], tn[-1] - tn[0]), 4)
                r["gain_ms"] = round(r["bundles"]["med_ms"] - r["native"]["med_ms"], 4)
                r["pass"] = r["gain_ms"] > r["spread_ms"]
                res[pname] = r
                print(net, "layer%d" % li, pname, json.dumps(r), flush=True)
            out["layers"]["%s_l%d" % (net, li)] = res
            del x, dy, yb, yn
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else None
    out = json.load(open(path)) if path and os.path.exists(path) else {}
    if "--whole-step" in sys.argv[1:]:
        encs = [a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--encoders=")]
        out.setdefault("whole_step", {}).update(whole_step(encs[0] if encs else ("resnext101_bts", "resnext50_bts")))
    else:
        out.update(layers())
    if path:
        json.dump(out, open(path, "w"), indent=1)
