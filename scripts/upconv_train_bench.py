"""The decoder's five upconv layers x three passes (forward, input gradient, weight gradient) in isolation, in both
training forms: the gather form of train.conv2d(..., up=2) (a 3x3 on the upsampled grid, 36 products per source pixel;
its input gradient includes the ATen 2x2 sum behind it) and the sub-pixel form of train._UpconvFn (16 products).
200 timed launches after 20 warm-ups, HIP events around every launch; rates are TFLOP/s of the 36-product count for
both forms, so they compare directly.  One JSON line per (layer, pass), then a table.

    python scripts/upconv_train_bench.py [--batch 4 --height 352 --width 704]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bts_amd import ops, train  # noqa: E402

LAYERS = (("upconv5", 32, 2208, 512), ("upconv4", 16, 512, 256), ("upconv3", 8, 256, 128), ("upconv2", 4, 128, 64),
          ("upconv1", 2, 64, 32))       # name, stride of the source map, c_in, c_out (DenseNet161, bts_size 512)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return dict(median_ms=ms[len(ms) // 2], p10_ms=ms[len(ms) // 10], p90_ms=ms[(9 * len(ms)) // 10])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=704)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    B = a.batch
    wws, sk = train._workspace(dev), train._splitk_workspace(dev)
    rows = []
    for name, stride, C, cout in LAYERS:
        h, w = a.height // stride, a.width // stride
        x2d = torch.randn(B * h * w, C, device=dev)
        dy2d = torch.randn(4 * B * h * w, cout, device=dev)
        wt = (torch.randn(cout, C, 3, 3, device=dev) / (9 * C) ** 0.5).contiguous()
        y2d = torch.empty(4 * B * h * w, cout, device=dev)
        dxu = torch.empty(4 * B * h * w, C, device=dev)
        dx2d = torch.empty(B * h * w, C, device=dev)
        packer = train.WeightPacker()
        wf, wd = packer.get(wt, C, train.WeightPacker.FWD), packer.get(wt, cout, train.WeightPacker.DGRAD)
        sf, sd = train.UpconvPacker().get(wt)
        fwd_cfg = lambda: ops.launch_config(fill_frames=ops.auto_fill_frames(B), precision="fp32")   # as BtsModel.forward declares
        bwd_cfg = lambda: ops.launch_config(precision="fp32")                                       # autograd runs outside that scope

        def g_fwd():
            with fwd_cfg():
                ops.conv_forward(x2d, B, h, w, wf, cout, 3, up=2, c_in_ld=C, y2d=y2d, pad=1, act=ops.ACT_ELU, splitk_ws=sk)

        def s_fwd():
            with fwd_cfg():
                ops.conv_forward(x2d, B, h, w, sf, cout, 3, up=2, c_in_ld=C, y2d=y2d, subpixel=True, act=ops.ACT_ELU)

        def g_dgrad():
            with bwd_cfg():
                ops.conv_forward(dy2d, B, 2 * h, 2 * w, wd, C, 3, c_in_ld=cout, y2d=dxu, pad=1, splitk_ws=sk)
            return dxu.view(B, h, 2, w, 2, C).sum(dim=(2, 4))

        def s_dgrad():
            with bwd_cfg():
                ops.upconv_dgrad(dy2d, B, h, w, sd, cout, C, dx2d, splitk_ws=sk)

        def g_wgrad():
            return ops.conv_wgrad(x2d, B, h, w, C, dy2d, cout, 3, pad=1, up=2, ws=wws)

        def s_wgrad():
            return ops.upconv_wgrad(x2d, B, h, w, C, dy2d, cout, wws)

        flops = 2.0 * 36 * B * h * w * C * cout
        for pas, gf, sf_ in (("forward", g_fwd, s_fwd), ("dgrad", g_dgrad, s_dgrad), ("wgrad", g_wgrad, s_wgrad)):
            g, s = timed(gf, a.iters, a.warmup), timed(sf_, a.iters, a.warmup)
            rec = dict(layer=name, map=[h, w], c_in=C, c_out=cout, batch=B, precision="fp32", gflop36=flops / 1e9)
            rec["pass"] = pas
            rec["gather"] = dict(g, tflops36=flops / g["median_ms"] / 1e9)
            rec["subpixel"] = dict(s, tflops36=flops / s["median_ms"] / 1e9)
            rec["speedup"] = g["median_ms"] / s["median_ms"]
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    print("\n%-8s %-8s %9s | %-31s | %-31s | %s" % ("layer", "pass", "map", "gather: ms (p10..p90)  TF/s", "sub-pixel: ms (p10..p90)  TF/s",
                                                   "gather/sub-pixel"))
    for r in rows:
        g, s = r["gather"], r["subpixel"]
        print("%-8s %-8s %4dx%-4d | %7.3f (%6.3f..%6.3f) %6.1f | %7.3f (%6.3f..%6.3f) %6.1f | %5.2fx"
              % (r["layer"], r["pass"], r["map"][0], r["map"][1], g["median_ms"], g["p10_ms"], g["p90_ms"], g["tflops36"],
                 s["median_ms"], s["p10_ms"], s["p90_ms"], s["tflops36"], r["speedup"]))
    tot_g = sum(r["gather"]["median_ms"] for r in rows)
    tot_s = sum(r["subpixel"]["median_ms"] for r in rows)
    print("sum of medians: gather %.3f ms, sub-pixel %.3f ms" % (tot_g, tot_s))


if __name__ == "__main__":
    main()
