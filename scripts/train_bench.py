#!/usr/bin/env python3
"""Training-step timing of BtsModel on one MI355X (the reference's training
configuration: DenseNet161, batch 4 per GPU, 352x704 crops, bts_main.py / arguments_train_eigen.txt).

Prints step time (forward + silog loss + backward + AdamW update) and, with --trace, the per-kernel split of the
HIP convolutions (forward / dgrad / wgrad) with their algorithmic TFLOP/s.  A tool for the perf loop; the headline
bench.py metric stays the inference frames/s.
"""
import argparse
import json
import sys
import time
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from bts_amd import bts as M, ops, synth, trainer  # noqa: E402

Params = namedtuple("Params", "encoder bts_size max_depth dataset")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=352)
    ap.add_argument("--width", type=int, default=704)
    ap.add_argument("--encoder", default="densenet161_bts")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--decoder-only", action="store_true")
    ap.add_argument("--no-freeze", action="store_true", help="train every encoder parameter (the reference freezes some)")
    ap.add_argument("--native-loss", action="store_true", help="silog on the HIP loss kernels (no host sync) instead of torch")
    ap.add_argument("--fused-reduc", action="store_true",
                    help="reduction_1x1 -> LPG scales and reduc1x1 as single autograd nodes on the fused kernels (fused_reduction_train)")
    ap.add_argument("--batched-wgrad", action="store_true",
                    help="one multi-problem weight-gradient launch per DenseNet block (and per fused reduction scale) instead "
                         "of one launch per layer (BtsModel.batched_wgrad)")
    ap.add_argument("--native-optim", action="store_true",
                    help="AdamW as one HIP launch that also re-packs the conv weights it updates (optim.NativeAdamW) instead "
                         "of torch's fused AdamW + a full re-pack")
    ap.add_argument("--subpixel-upconv", action="store_true",
                    help="the decoder's ratio-2 upconvs in sub-pixel form in all three passes (BtsModel.subpixel_upconv_train)")
    ap.add_argument("--grouped-native", action="store_true",
                    help="ResNeXt's stride-1 grouped 3x3 layers on the native grouped kernels in all three passes "
                         "(BtsModel.grouped_conv_train)")
    ap.add_argument("--train-precision", choices=("fp32", "bf16"), default="fp32",
                    help="bf16: bf16 operands, fp32 accumulation in the forward, input-gradient and weight-gradient pass of "
                         "the convolutions (BtsModel.train_precision)")
    ap.add_argument("--bn-no-track-stats", action="store_true",
                    help="every norm layer in eval mode inside the train()-mode model (bts_main.py --bn_no_track_stats; "
                         "set_misc(bn_no_track_stats=True))")
    ap.add_argument("--native-frozen-norm", action="store_true",
                    help="frozen norm layers on the HIP kernels, dense blocks that hold them on the fused node "
                         "(BtsModel.native_frozen_norm)")
    a = ap.parse_args()
    # BASELINE config 5 (B=32 over 8 GPUs = 4 per GPU, DDP): launch with
    #   python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 scripts/train_bench.py
    import os
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_dist = world > 1 or os.environ.get("BTS_BENCH_FORCE_DIST") == "1"
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    saved_stdout = os.dup(1)                 # RCCL prints a banner on stdout: keep the JSON line clean
    os.dup2(2, 1)
    torch.manual_seed(0)
    params = Params(a.encoder, 512, 80.0, "kitti")
    model = M.BtsModel(params).train().to(dev)
    model.fused_reduction_train = a.fused_reduc
    model.batched_wgrad = a.batched_wgrad
    model.subpixel_upconv_train = a.subpixel_upconv
    model.grouped_conv_train = a.grouped_native
    model.train_precision = a.train_precision
    if a.native_frozen_norm:
        model.native_frozen_norm = True
    loss_fn = M.silog_loss(0.85, native=a.native_loss)
    if not a.no_freeze:
        # the reference freezes the stem conv and the encoder norm affines
        trainer.set_misc(model, a.encoder, bn_no_track_stats=a.bn_no_track_stats)
    elif a.bn_no_track_stats:
        model.apply(M.bn_init_as_tf)
    opt = trainer.make_optimizer(model, 1e-4, 1e-2, 1e-3, native=a.native_optim)
    core = model
    if use_dist:
        model = trainer.wrap_ddp(model, dev)   # gradient all-reduce over RCCL, overlapped with backward by DDP's buckets
    B, H, W = a.batch, a.height, a.width
    x = torch.from_numpy(synth.image_batch(B, H, W, 1)).to(dev)
    focal = torch.from_numpy(synth.focal_values(B, "kitti", 1)).to(dev)
    gt, mask = synth.train_targets(B, H, W, 80.0, 2)
    gt, mask = torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)
    feats = None
    if a.decoder_only:
        fs = synth.encoder_features(synth.ENCODER_CHANNELS[a.encoder], B, H, W, seed=3)
        feats = [None] + [torch.from_numpy(f).to(dev).requires_grad_(True) for f in fs[1:]]

    opt_events = []          # --trace: (start, end) events around optimizer.step(), whatever implementation it is

    def step(timed=False):
        opt.zero_grad(set_to_none=True)
        outs = core.decoder(feats, focal) if a.decoder_only else model(x, focal)
        loss = loss_fn(outs[4], gt, mask)
        loss.backward()
        if timed:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            opt.step()
            ev[1].record()
            opt_events.append(ev)
        else:
            opt.step()
        return loss

    for i in range(a.warmup):
        t0 = time.time()
        l = step()
        torch.cuda.synchronize()
        print("warmup %d: %.1f ms loss %.4f" % (i, (time.time() - t0) * 1e3, l.item()), file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    t0 = time.time()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    ms = (time.time() - t0) * 1e3 / a.steps
    if use_dist:
        dist.barrier()
        tmax = torch.tensor([ms], device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        ms = tmax.item()
    res = dict(metric="training step ms (fwd+loss+bwd+AdamW)", ms_per_step=ms, frames_per_s=world * B / ms * 1e3,
               n_gpus=world, ddp=use_dist,
               loss="silog native (HIP)" if a.native_loss else "silog torch",
               config=dict(encoder=a.encoder, batch_per_gpu=B, height=H, width=W, decoder_only=a.decoder_only,
                           fused_reduc=a.fused_reduc, batched_wgrad=a.batched_wgrad, native_optim=a.native_optim,
                           subpixel_upconv=a.subpixel_upconv, grouped_native=a.grouped_native,
                           train_precision=a.train_precision, bn_no_track_stats=a.bn_no_track_stats,
                           native_frozen_norm=a.native_frozen_norm),
               peak_mem_gb=torch.cuda.max_memory_allocated() / 2**30)
    if a.trace:
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        step(timed=True)
        ops.set_trace(None)
        summ = tr.summary()
        # the whole optimiser step on the stream (torch's fused AdamW is not a library launch, so it has no trace tag); the
        # native launch alone is the `adamw` row below (tag optim.adamw), set against 36 B per updated parameter
        res["optimizer_step_ms"] = opt_events[0][0].elapsed_time(opt_events[0][1])
        n_upd = sum(p.numel() for g in opt.param_groups for p in g["params"] if p.grad is not None)
        res["updated_parameters"] = n_upd
        res["adamw_bound_ms_at_6.3TBps"] = 36.0 * n_upd / 6.3e12 * 1e3
        rows = {}
        for kern, d in summ.items():
            for tag, v in d["tags"].items():
                kind = tag.rsplit(".", 1)[-1] if "." in tag else kern
                r = rows.setdefault(kind, dict(ms=0.0, flops=0.0, launches=0))
                r["ms"] += v["ms"]
                r["flops"] += v["flops"]
                r["launches"] += v["launches"]
        for k, r in rows.items():
            r["tflops"] = r["flops"] / max(r["ms"], 1e-9) / 1e9
        res["kernels"] = rows
        res["library_launches_per_step"] = len(tr.records)
        # the reduction scales on their own (library launches only: the torch elementwise kernels between them are not traced)
        res["reduction_launches"] = {"%s %s" % (kern, tag): dict(ms=v["ms"], launches=v["launches"])
                                     for kern, d in summ.items() for tag, v in d["tags"].items() if tag.startswith("reduc")}
        top = []
        for kern, d in summ.items():
            for tag, v in d["tags"].items():
                top.append((v["ms"], kern, tag, v["launches"], v["flops"] / max(v["ms"], 1e-9) / 1e9))
        top.sort(reverse=True)
        for ms_, kern, tag, n, tf in top[:25]:
            print("%8.2f ms  %-34s %-22s x%-4d %6.1f TF/s" % (ms_, kern, tag, n, tf), file=sys.stderr)
    if rank == 0:
        os.write(saved_stdout, (json.dumps(res) + "\n").encode())
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
