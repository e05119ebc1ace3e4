#!/usr/bin/env python3
"""Whole-model frames/s of the bf16 inference mode (``conv_precision = "bf16"``) against the fp32 mode, in ONE process.

For each configuration the same model (random-init encoder, PCG64 synthetic decoder state, as bench.py builds it) is
captured once per precision as a hipGraph (bts_amd.graph.GraphedModel keys its graphs on the precision); after warm-up
the two graphs are timed in alternating rounds with device events, so drift of the shared machine hits both modes
alike.  The bf16 outputs are then compared with the fp32 outputs of the same inputs.  One JSON document goes to stdout
(and to --out).

    python scripts/bf16_bench.py                          # configs[1] (DenseNet161, B=16, 352x1216) and configs[2]
    python scripts/bf16_bench.py --configs 1 --rounds 5
    python scripts/bf16_bench.py --only bf16 --configs 1 --steps 3   # bf16 forwards only (run under rocprofv3)
    python scripts/bf16_bench.py --bf16-tail                 # a third graph: bf16 with conv3 / conv2 on the bf16 tail kernel
    python scripts/bf16_bench.py --wide-1x1 [--bf16-tail]    # one more graph per bf16 variant: the same with BtsModel.bf16_wide_1x1 on
"""
import argparse
import json
import os
import sys
import time
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {   # BASELINE.json numbering
    1: dict(encoder="densenet161_bts", dataset="kitti", max_depth=80.0, B=16, H=352, W=1216),
    2: dict(encoder="resnext101_bts", dataset="nyu", max_depth=10.0, B=16, H=416, W=544),
}
NAMES = ("depth_8x8_scaled", "depth_4x4_scaled", "depth_2x2_scaled", "reduc1x1", "final_depth", "iconv1")


Params = namedtuple("Params", "encoder bts_size max_depth dataset")      # the fields of the reference's argparse namespace


def _params(cfg):
    return Params(cfg["encoder"], 512, cfg["max_depth"], cfg["dataset"])


def make_model(cfg, device):
    """Random-init encoder + PCG64(0) synthetic decoder state, eval mode (bench.py's build_model)."""
    from bts_amd import bts as M, synth
    params = _params(cfg)
    torch.manual_seed(0)
    model = M.BtsModel(params)
    sd = {k: (torch.tensor(v) if np.ndim(v) == 0 else torch.from_numpy(v.copy()))
          for k, v in synth.decoder_state(synth.ENCODER_CHANNELS[cfg["encoder"]], 512, 0).items()}
    model.decoder.load_state_dict(sd, strict=True)
    return model.eval().to(device), params


def accuracy(got, ref):
    """bf16 outputs against the fp32 outputs of the same inputs: median / 99th percentile / max relative error per depth
    map (pixels with |ref| < 1e-6 of the map's max excluded), max-abs / max|ref| for iconv1."""
    rep = {}
    for i, name in enumerate(NAMES):
        g = got[i].double().cpu().numpy().ravel()
        r = ref[i].double().cpu().numpy().ravel()
        if name == "iconv1":
            rep[name] = {"max_abs_over_max_ref": float(np.abs(g - r).max() / np.abs(r).max())}
            continue
        m = np.abs(r) > 1e-6 * np.abs(r).max()
        rel = np.abs(g[m] - r[m]) / np.abs(r[m])
        rep[name] = {"median_rel": float(np.median(rel)), "p99_rel": float(np.percentile(rel, 99)), "max_rel": float(rel.max())}
    return rep


def set_variant(model, p):
    """"fp32" / "bf16": the precision with both switches off; "bf16_tail": bf16 with the decoder's bf16_tail_convs on;
    "bf16_wide" / "bf16_tail_wide": the same two with BtsModel.bf16_wide_1x1 on."""
    model.conv_precision = "bf16" if p.startswith("bf16") else p
    model.bf16_tail_convs = p.startswith("bf16_tail")
    model.bf16_wide_1x1 = p.endswith("_wide")


def run_config(idx, args, device):
    from bts_amd import synth
    from bts_amd.graph import GraphedModel
    cfg = CONFIGS[idx]
    model, params = make_model(cfg, device)
    B, H, W = cfg["B"], cfg["H"], cfg["W"]
    image = torch.from_numpy(synth.image_batch(B, H, W, 1234)).to(device)
    focal = torch.from_numpy(synth.focal_values(B, params.dataset, 1234)).to(device)
    precs = [args.only] if args.only else ["fp32", "bf16"] + (["bf16_tail"] if args.bf16_tail else [])
    if args.wide_1x1 and not args.only:
        precs += [p + "_wide" for p in precs if p.startswith("bf16")]
    if args.only:                                   # profiling run: eager forwards, no timing claims
        v = "bf16_tail" if (args.bf16_tail and args.only == "bf16") else args.only
        set_variant(model, v + "_wide" if (args.wide_1x1 and args.only == "bf16") else v)
        with torch.no_grad():
            for _ in range(args.steps):
                model(image, focal)
        torch.cuda.synchronize()
        return {"config": idx, "only": args.only, "steps": args.steps}
    gm = GraphedModel(model)
    outs = {}
    with torch.no_grad():
        for p in precs:                              # capture (two eager passes inside) + warm-up replays
            set_variant(model, p)
            for _ in range(args.warmup):
                o = gm(image, focal)
            torch.cuda.synchronize()
            outs[p] = [t.clone() for t in o]
        times = {p: [] for p in precs}
        for r in range(args.rounds):
            for p in (precs if r % 2 == 0 else precs[::-1]):
                set_variant(model, p)
                gm(image, focal)                     # one untimed replay: the switch itself is not measured
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                s.record()
                for _ in range(args.steps):
                    gm(image, focal)
                e.record()
                e.synchronize()
                times[p].append(s.elapsed_time(e) / args.steps)
        set_variant(model, "bf16")
        again = [t.clone() for t in gm(image, focal)]
    res = {"config": idx, "encoder": cfg["encoder"], "batch": B, "height": H, "width": W, "steps_per_round": args.steps,
           "rounds": args.rounds, "warmup": args.warmup, "hipgraph": True, "sub_batch_streams": model.sub_batches}
    for p in precs:
        ms = float(np.median(times[p]))
        res[p] = {"ms_per_step_median": ms, "ms_per_step_rounds": [round(v, 3) for v in times[p]], "frames_per_s": B * 1000.0 / ms}
    res["speedup_bf16_over_fp32"] = res["bf16"]["frames_per_s"] / res["fp32"]["frames_per_s"]
    res["bf16_vs_fp32_outputs"] = accuracy(outs["bf16"], outs["fp32"])
    res["bf16_repeat_bit_identical"] = all(torch.equal(a, b) for a, b in zip(outs["bf16"], again))
    if "bf16_tail" in outs:
        res["speedup_bf16_tail_over_bf16"] = res["bf16_tail"]["frames_per_s"] / res["bf16"]["frames_per_s"]
        res["bf16_tail_vs_fp32_outputs"] = accuracy(outs["bf16_tail"], outs["fp32"])
    for p in precs:
        if p.endswith("_wide"):
            base = p[:-len("_wide")]
            res["speedup_%s_over_%s" % (p, base)] = res[p]["frames_per_s"] / res[base]["frames_per_s"]
            res["%s_vs_fp32_outputs" % p] = accuracy(outs[p], outs["fp32"])
            res["%s_vs_%s_outputs_bit_identical" % (p, base)] = all(torch.equal(a, b) for a, b in zip(outs[p], outs[base]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="1,2", help="comma-separated BASELINE.json config numbers (1, 2)")
    ap.add_argument("--steps", type=int, default=10, help="graph replays per timed round")
    ap.add_argument("--rounds", type=int, default=6, help="alternating fp32 / bf16 rounds")
    ap.add_argument("--warmup", type=int, default=3, help="replays per precision before timing (after the capture)")
    ap.add_argument("--only", choices=("fp32", "bf16"), default=None, help="run one precision eagerly (profiling)")
    ap.add_argument("--bf16-tail", action="store_true",
                    help="also time bf16 with the decoder's bf16_tail_convs switch on (a third graph in the same alternation)")
    ap.add_argument("--wide-1x1", action="store_true",
                    help="also time every bf16 variant with BtsModel.bf16_wide_1x1 on (one more graph each in the same alternation)")
    ap.add_argument("--out", default=None, help="also write the JSON document here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bf16_bench.py needs a GPU"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    t0 = time.time()
    results = [run_config(int(c), args, device) for c in args.configs.split(",") if c.strip()]
    doc = {"what": "whole-model frames/s, bf16 inference mode vs fp32, alternating in one process",
           "device": torch.cuda.get_device_name(device), "wall_s": round(time.time() - t0, 1), "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
