"""GPU: train_precision "bf16" through the training graph (bts_amd/train.py) -- bf16 operands and fp32 accumulation in the
forward, input-gradient and weight-gradient pass of every convolution the mode takes.

The whole-model gradient amplifies rounding by about 10^4 (tests/conftest.py), so a bf16 gradient is never held against a
plain fp64 gradient here: every reference is the fp64 CPU run of the graph WITH THE SAME OPERAND ROUNDINGS INSERTED
(tests/train_bf16_ref.py).

* one node per convolution family: forward, dx and dw each within the project's bf16 bound 2e-6 * sum|terms|
  (tests/test_bf16_gpu.py) of that statement.  The operands a convolution rounds are given data there, so no rounding
  decision hangs on a last-bit difference between the GPU's fp32 and the reference's fp64.
* the two-layer dense block and the whole model round values that are themselves computed (norm layers with batch
  statistics, ReLU / ELU masks, earlier layers): a value within fp32 distance of a rounding tie goes the other way on the
  GPU than in fp64, a 2^-9 relative difference of that operand, and sum|terms| is defined per convolution, not through a norm
  layer.  Their bar is therefore the rule tests/conftest.py documents for the fp32 step: relative L2 per tensor against the
  fp64 rounded graph, at most 2x what a CPU fp32 run of the SAME rounded graph scores against it -- per class of tensors,
  because which tensor a flipped decision lands in differs from run to run.  The dense block's TIGHT check -- each of its
  launches against the rounded statement on the operands the GPU itself handed it -- is in
  tests/test_train_bf16_nodes_gpu.py, with the sub-pixel upconv node, the batched block and the nodes that stay fp32."""
import copy
import functools

import numpy as np
import pytest
import torch

import train_bf16_ref as R
import train_node_cases as nc
from bts_amd import encoders as E
from bts_amd import ops, synth, train
from bts_amd._lib import BtsHipError
from conftest import fp32_only
from parity_util import LARGE_TENSOR, t

pytestmark = [pytest.mark.gpu, fp32_only]

BF16_BOUND = 2e-6


class Params:
    def __init__(self, enc, bts_size, max_depth, dataset):
        self.encoder, self.bts_size, self.max_depth, self.dataset = enc, bts_size, max_depth, dataset


# name -> (c_in, c_out, conv2d keywords, (B, h, w)): 2 x 9 x 13 maps (234 pixels: eight K-steps of the weight gradient, a ragged
# last one) -- except the halo tile, which the library takes from 1 x 64 x 64 on at 64 channels (smaller maps split K on the
# row-tiled kernel: the "3x3" case)
SMALL = (2, 9, 13)
FAMILIES = {
    "1x1": (64, 48, dict(), SMALL),
    "3x3": (64, 64, dict(padding=1), SMALL),
    "3x3_halo": (64, 64, dict(padding=1), (1, 64, 64)),
    "dilated": (64, 32, dict(padding=6, dilation=6), SMALL),
    "stride2": (32, 64, dict(padding=1, stride=2), SMALL),
    "up2": (48, 40, dict(padding=1, up=2), SMALL),
    "bundles": (64, 64, dict(padding=1, groups=8), SMALL),
}


def _gpu_conv(x, w, gy, scope, kw):
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        with train.precision_scope(scope):
            y = train.conv2d(xg, wg, tag="node", **kw)
        y.backward(gy.cuda())
        torch.cuda.synchronize()
    finally:
        ops.set_trace(None)
    return [v.detach().cpu().double() for v in (y, xg.grad, wg.grad)], [(r[0], r[1]) for r in tr.records if r[1].startswith("node.")]


@pytest.mark.parametrize("name", list(FAMILIES))
def test_conv_node_matches_the_rounded_statement_in_all_three_passes(name):
    cin, cout, kw, (nb, h, w_) = FAMILIES[name]
    groups, up = kw.get("groups", 1), kw.get("up", 1)
    k = 1 if name == "1x1" else 3
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(nb, cin, h, w_, generator=g)
    w = torch.randn(cout, cin // groups, k, k, generator=g) / (cin // groups * k * k) ** 0.5
    ckw = dict(stride=kw.get("stride", 1), padding=kw.get("padding", 0), dilation=kw.get("dilation", 1), groups=groups)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    xu = x64.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if up == 2 else x64
    y64 = R.rconv(xu, w64, **ckw)
    gy = torch.randn(y64.shape, generator=g)
    y64.backward(gy.double())
    mag_y, mag_dx, mag_dw = R.conv_magnitudes(xu.detach(), w, gy, **ckw)
    if up == 2:
        mag_dx = mag_dx.view(nb, cin, h, 2, w_, 2).sum(dim=(3, 5))
    refs, mags = (y64.detach(), x64.grad, w64.grad), (mag_y, mag_dx, mag_dw)

    got, kernels = _gpu_conv(x, w, gy, "bf16", kw)
    plain, kernels32 = _gpu_conv(x, w, gy, "fp32", kw)
    print(name, "kernels:", kernels)
    assert [tag for _, tag in kernels] == ["node.fwd", "node.dgrad", "node.wgrad"] == [tag for _, tag in kernels32]
    assert kernels[2][0] == "conv_wgrad_kernel<bf16>" and kernels32[2][0] == "conv_wgrad_kernel"
    assert all("bf16" in kern for kern, _ in kernels) and not any("bf16" in kern for kern, _ in kernels32)
    if name == "3x3_halo":
        assert kernels[0][0] == kernels[1][0] == "conv_halo_emu_kernel<64,k3,bf16>"
    for what, a, p, ref, mag in zip(("forward", "dx", "dw"), got, plain, refs, mags):
        assert a.shape == ref.shape and torch.isfinite(a).all(), (name, what)
        bound = BF16_BOUND * mag + 2.0 ** -22 * ref.abs()          # + the fp32 sums behind the kernel (up=2's 2x2 fold)
        worst = float(((a - ref).abs() / bound.clamp_min(1e-300)).max())
        worst32 = float(((p - ref).abs() / bound.clamp_min(1e-300)).max())
        print("  %s: max |err| / bound: bf16 %.4f, fp32 step %.1f" % (what, worst, worst32))
        assert worst <= 1.0, (name, what, worst)
        assert worst32 > 1.0, (name, what, "the fp32 step must miss the rounded statement", worst32)


def _block_run(block, x, gy, scope):
    """One step of train._dense_block on the GPU: (output, dx, {parameter name: gradient}, running statistics)."""
    m = copy.deepcopy(block).cuda().train()
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    with train.precision_scope(scope):
        y = train._dense_block(m, xg)
    assert y is not None
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    return y.detach().cpu(), xg.grad.cpu(), {n: p.grad.cpu() for n, p in m.named_parameters()}


def _block_reference(block, x, gy, dtype):
    m = copy.deepcopy(block).to(dtype).train()
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    with R.rounded_convs() as rc:
        y = m(xr)
        y.backward(gy.to(dtype))
    assert rc.rounded == 2 * len(m) and rc.kept == 0
    return y.detach(), xr.grad, {n: p.grad for n, p in m.named_parameters()}


def test_dense_block_with_batch_statistics_matches_the_rounded_graph():
    """Two layers of DenseNet121's first block (64 + 2 x 32 channels, 2 x 9 x 13) through train._DenseBlockFn: norm + ReLU in
    the prologue of both convolutions and of the weight-gradient gather, rounding after it.  Relative L2 of the output, dx and
    every parameter gradient against the fp64 rounded graph; bar: 2x the worst figure of the CPU fp32 run of the same graph
    (module docstring), and never below 2^-13.  Where that floor comes from: operand rounding errors are independent of the
    terms, so a step that leaves the roundings out (or rounds twice, or the wrong operand) sits at about 2^-9 / sqrt(3) *
    sqrt(2) = 1.6e-3 relative L2 in EVERY tensor, whatever the length of its sums -- the fp32 step, asserted below; one
    rounding decision taken the other way moves a tensor of N rounded elements by about 2^-8 / sqrt(N), 3e-5 here.  2^-13
    = 1.2e-4 lies 13x below the first and 4x above the second.
    Measured on the MI355X (relative L2 against the fp64 rounded graph): bf16 step 1.2e-7 .. 9.2e-4 over the 14 tensors
    (forward 7.2e-5, dx 3.6e-4, conv weights 7.2e-5 .. 7.7e-4), CPU fp32 run of the rounded graph 1.5e-4 .. 2.0e-3 (the bar:
    4.0e-3), the fp32 step 2.3e-3 (forward) and 4.5e-3 .. 9.4e-2 (every gradient)."""
    gen = torch.Generator().manual_seed(11)
    block = E._DenseBlock(2, 64, 4, 32).train()
    nc.randomise(block, gen)
    x = torch.randn(2, 64, 9, 13, generator=gen)
    gy = torch.randn(2, 128, 9, 13, generator=gen)
    y64, dx64, g64 = _block_reference(block, x, gy, torch.float64)
    y32, dx32, g32 = _block_reference(block, x, gy, torch.float32)
    y, dx, gp = _block_run(block, x, gy, "bf16")
    yp, dxp, gpp = _block_run(block, x, gy, "fp32")
    assert set(gp) == set(g64) and all(torch.isfinite(v).all() for v in gp.values())
    names = ["forward", "dx"] + sorted(g64)
    e = dict(zip(names, [R.rel_l2(y, y64), R.rel_l2(dx, dx64)] + [R.rel_l2(gp[n], g64[n]) for n in sorted(g64)]))
    f = dict(zip(names, [R.rel_l2(y32, y64), R.rel_l2(dx32, dx64)] + [R.rel_l2(g32[n], g64[n]) for n in sorted(g64)]))
    p = dict(zip(names, [R.rel_l2(yp, y64), R.rel_l2(dxp, dx64)] + [R.rel_l2(gpp[n], g64[n]) for n in sorted(g64)]))
    bar = max(2.0 * max(f.values()), 2.0 ** -13)
    for n in names:
        print("%-28s rel L2 vs fp64 rounded graph: bf16 step %.2e, cpu fp32 rounded %.2e, fp32 step %.2e" % (n, e[n], f[n], p[n]))
    print("bar %.2e" % bar)
    for n in names:
        assert e[n] <= bar, (n, e[n], bar)
    convs = [n for n in names if n.endswith("conv1.weight") or n.endswith("conv2.weight")]
    assert len(convs) == 4 and all(p[n] > bar for n in convs + ["dx"]), ("the fp32 step's gradients must miss the rounded graph", p)


# ------------------------------------------------------------------------------------------ whole model
B, H, W = 2, 64, 96


def _inputs():
    x = torch.from_numpy(synth.image_batch(B, H, W, 5))
    focal = torch.from_numpy(synth.focal_values(B, "kitti", 5))
    gt, mask = synth.train_targets(B, H, W, 80.0, 9)
    return x, focal, t(gt), t(mask)


def _model(seed=21):
    from bts_amd import bts as M
    torch.manual_seed(seed)
    return M.BtsModel(Params("densenet121_bts", 512, 80.0, "kitti")).train()


@functools.lru_cache(maxsize=None)
def _cpu_rounded_step(dtype):
    """One step of the rounded graph on the CPU (the torch encoder modules + the oracle decoder, as
    tests/test_train_gpu.py's whole-model test runs them, under train_bf16_ref.rounded_convs): (loss, {name: gradient}).
    Computed once per dtype and never modified."""
    from oracle import bts_oracle as O
    model = _model()
    x, focal, gt, mask = _inputs()
    enc = copy.deepcopy(model.encoder).to(dtype)
    state = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in model.decoder.state_dict().items()}
    for k, v in state.items():
        if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    with R.rounded_convs(R.model_keep_fp32(state)) as rc:
        outs = O.decoder_forward(state, enc(x.to(dtype)), focal.to(dtype), 80.0, "kitti", training=True)
        loss = O.silog_loss(outs[4], gt.to(dtype), mask, 0.85)
        loss.backward()
    assert rc.rounded > 120 and rc.kept >= 9                   # kept: the stem, conv3 / conv2 / conv1 / get_depth, the four chains
    grads = {"encoder." + n: p.grad for n, p in enc.named_parameters()}
    grads.update({"decoder." + n: v.grad for n, v in state.items() if v.requires_grad})
    return loss.item(), {n: v.detach() for n, v in grads.items() if v is not None}


def _gpu_step(m, x, focal, gt, mask):
    from bts_amd import bts as M
    for p in m.parameters():
        p.grad = None
    outs = m(x, focal)
    loss = M.silog_loss(0.85)(outs[4], gt, mask)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), outs, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _class_bars(floor, sizes):
    small = [e for n, e in floor.items() if sizes[n] < LARGE_TENSOR]
    large = [e for n, e in floor.items() if sizes[n] >= LARGE_TENSOR]
    return 2.0 * max(small), 2.0 * max(large)


def test_whole_model_step_densenet121_against_the_rounded_graph():
    """DenseNet121 + decoder, 2 x 64 x 96, silog loss, one step with train_precision "bf16".  Every parameter that gets a
    gradient in the fp32 step gets a finite one; relative L2 per parameter tensor against the fp64 CPU run of the rounded graph
    at most 2x what the CPU fp32 run of that graph scores, per class of tensors (below / from parity_util.LARGE_TENSOR
    elements) and over the whole gradient.
    Measured on the MI355X: global relative L2 of the gradient against the fp64 rounded graph 4.0e-1 for the bf16 step and
    3.9e-1 for the CPU fp32 run of the same graph (bar 7.9e-1); per tensor, median / max 4.5e-1 / 6.9e-1 against 4.2e-1 / 5.5e-1
    (bars 1.09 small tensors, 1.01 large).  The figures say what this test can and cannot see: on this randomly
    initialised 160-layer net with 6 to 1536 samples per norm-layer channel, a rounding decision that flips on a last-bit
    difference is amplified until two runs of the SAME rounded graph in different arithmetic are 40 % apart, so the bar holds
    finiteness, coverage and gross errors only; the roundings themselves are pinned by the node and dense-block tests above
    and by tests/test_wgrad_bf16_gpu.py."""
    loss64, g64 = _cpu_rounded_step(torch.float64)
    loss32, g32 = _cpu_rounded_step(torch.float32)
    x, focal, gt, mask = (v.cuda() for v in _inputs())
    m = _model().cuda()
    _, _, gplain = _gpu_step(m, x, focal, gt, mask)
    m.train_precision = "bf16"
    loss, outs, got = _gpu_step(m, x, focal, gt, mask)
    assert set(got) == set(gplain) == set(g64) and len(got) > 400
    assert all(torch.isfinite(v).all() for v in got.values()) and all(torch.isfinite(o).all() for o in outs)
    sizes = {n: v.numel() for n, v in g64.items()}
    e = {n: R.rel_l2(got[n], g64[n]) for n in g64}
    f = {n: R.rel_l2(g32[n], g64[n]) for n in g64}
    p = {n: R.rel_l2(gplain[n], g64[n]) for n in g64}
    glob = lambda d: float(np.sqrt(sum(float((d[n].double().cpu() - g64[n]).norm()) ** 2 for n in g64)
                                   / sum(float(g64[n].norm()) ** 2 for n in g64)))
    l2, l2_32, l2_plain = glob(got), glob(g32), glob(gplain)
    bar_small, bar_large = _class_bars(f, sizes)
    q = lambda d: float(np.median(list(d.values())))
    print("loss: fp64 rounded %.6f, cpu fp32 rounded %.6f, bf16 step %.6f" % (loss64, loss32, loss))
    print("global rel L2 vs fp64 rounded graph: bf16 step %.2e, cpu fp32 rounded %.2e, fp32 step %.2e" % (l2, l2_32, l2_plain))
    print("per tensor, median / max: bf16 step %.2e / %.2e, cpu fp32 rounded %.2e / %.2e, fp32 step %.2e / %.2e"
          % (q(e), max(e.values()), q(f), max(f.values()), q(p), max(p.values())))
    print("bars (2x the cpu fp32 floor): small tensors %.2e, large tensors %.2e, global %.2e" % (bar_small, bar_large, 2 * l2_32))
    assert abs(loss - loss64) <= max(2e-4 * abs(loss64), 4 * abs(loss32 - loss64)), (loss, loss64, loss32)
    worst = sorted(((e[n] / (bar_large if sizes[n] >= LARGE_TENSOR else bar_small), n, sizes[n], e[n]) for n in e), reverse=True)[:3]
    for n in e:
        assert e[n] <= (bar_large if sizes[n] >= LARGE_TENSOR else bar_small), (n, sizes[n], e[n], worst)
    assert l2 <= 2.0 * l2_32, (l2, l2_32, worst)


@functools.lru_cache(maxsize=None)
def _cpu_rounded_decoder_step(dtype):
    """One decoder-only step of the rounded graph on the CPU (synthetic encoder taps in, oracle decoder, silog loss)."""
    from oracle import bts_oracle as O
    dec = _model().decoder
    _, focal, gt, mask = _inputs()
    fs = synth.encoder_features(synth.ENCODER_CHANNELS["densenet121_bts"], B, H, W, seed=3)
    state = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in dec.state_dict().items()}
    for k, v in state.items():
        if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    with R.rounded_convs(R.model_keep_fp32(state)) as rc:
        outs = O.decoder_forward(state, [None] + [torch.from_numpy(f).to(dtype) for f in fs[1:]], focal.to(dtype), 80.0, "kitti",
                                 training=True)
        loss = O.silog_loss(outs[4], gt.to(dtype), mask, 0.85)
        loss.backward()
    assert rc.rounded == 18 and rc.kept == 22
    return loss.item(), {n: v.grad.detach() for n, v in state.items() if v.requires_grad and v.grad is not None}


def test_decoder_step_against_the_rounded_graph_per_tensor():
    """The decoder on its own (bts.train_precision, synthetic encoder taps, 2 x 64 x 96): 40 layers instead of 160 and norm
    layers that see 48 samples or more, so the rounded graph is not chaotic -- the CPU fp32 run of it scores 1.3e-2 median /
    7.1e-2 max relative L2 per parameter tensor against its fp64 run -- and the rule of the whole-model test has teeth per
    tensor: every parameter gradient within 2x the worst floor figure of its size class (an all-zero, missing or mis-wired
    gradient scores 1.0 or more), the whole gradient within 2x the global floor.
    Measured on the MI355X: bf16 step 1.3e-2 global, 1.5e-2 median / 8.4e-2 max per tensor; CPU fp32 run of the rounded graph
    1.1e-2 global, 1.3e-2 / 7.1e-2; bars 1.4e-1 (small tensors) and 1.2e-1 (large)."""
    from bts_amd import bts as M
    loss64, g64 = _cpu_rounded_decoder_step(torch.float64)
    loss32, g32 = _cpu_rounded_decoder_step(torch.float32)
    _, focal, gt, mask = (v.cuda() for v in _inputs())
    dec = _model().decoder.cuda().train()
    dec.train_precision = "bf16"
    fs = synth.encoder_features(synth.ENCODER_CHANNELS["densenet121_bts"], B, H, W, seed=3)
    feats = [None] + [torch.from_numpy(f).cuda() for f in fs[1:]]
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        outs = dec(feats, focal)
        loss = M.silog_loss(0.85)(outs[4], gt, mask)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_trace(None)
    got = {n: p.grad for n, p in dec.named_parameters() if p.grad is not None}
    assert set(got) == set(g64) and all(torch.isfinite(v).all() for v in got.values())
    # which launches ran in bf16: every convolution pass but conv3 / conv2 / conv1, get_depth and the reduction chains
    fp32_tags = ("conv3.", "conv2.", "conv1.", "get_depth.", "reduc.")
    for kern, tag in [(r[0], r[1]) for r in tr.records if r[1].endswith((".fwd", ".dgrad", ".wgrad")) and r[0].startswith("conv_")]:
        assert ("bf16" in kern) == (not tag.startswith(fp32_tags)), (kern, tag)
    sizes = {n: v.numel() for n, v in g64.items()}
    e = {n: R.rel_l2(got[n], g64[n]) for n in g64}
    f = {n: R.rel_l2(g32[n], g64[n]) for n in g64}
    bar_small, bar_large = _class_bars(f, sizes)
    glob = lambda d: float(np.sqrt(sum(float((d[n].double().cpu() - g64[n]).norm()) ** 2 for n in g64)
                                   / sum(float(g64[n].norm()) ** 2 for n in g64)))
    l2, l2_32 = glob(got), glob(g32)
    print("decoder step, rel L2 vs fp64 rounded graph: global bf16 %.2e, cpu fp32 rounded %.2e; per tensor median / max bf16 %.2e / %.2e, "
          "cpu fp32 rounded %.2e / %.2e; bars small %.2e large %.2e" % (l2, l2_32, float(np.median(list(e.values()))), max(e.values()),
                                                                   float(np.median(list(f.values()))), max(f.values()), bar_small, bar_large))
    assert bar_small < 0.5 and bar_large < 0.5                 # the premise: a bar that an all-zero gradient cannot pass
    assert abs(loss.item() - loss64) <= max(2e-4 * abs(loss64), 4 * abs(loss32 - loss64)), (loss.item(), loss64, loss32)
    for n in e:
        assert e[n] <= (bar_large if sizes[n] >= LARGE_TENSOR else bar_small), (n, sizes[n], e[n], bar_small, bar_large)
    assert l2 <= 2.0 * l2_32, (l2, l2_32)


def test_second_step_uses_the_new_weights_bf16_planes():
    """Two steps with an in-place update of every parameter between them.  The packed weights, and the bf16 planes
    ops.conv_forward derives from them for the forward and the input-gradient launches, must follow the update (the stale-U bug
    class): the second step has the bits of the first step of a fresh model that was given the updated values -- whose packs
    and planes did not exist before."""
    x, focal, gt, mask = (v.cuda() for v in _inputs())
    m = _model().cuda()
    m.train_precision = "bf16"
    loss1, outs1, g1 = _gpu_step(m, x, focal, gt, mask)
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 4:
                p.mul_(0.9).add_(torch.randn(p.shape, generator=gen).cuda() * (0.02 * p.abs().mean()))
    loss2, outs2, g2 = _gpu_step(m, x, focal, gt, mask)
    fresh = _model(seed=99).cuda()
    fresh.load_state_dict(m.state_dict())
    fresh.train_precision = "bf16"
    loss3, outs3, g3 = _gpu_step(fresh, x, focal, gt, mask)
    assert not torch.equal(outs1[4], outs2[4])
    for a, b in zip(outs2, outs3):
        assert torch.equal(a, b)
    assert loss2 == loss3 and set(g2) == set(g3)
    bad = [n for n in g2 if not torch.equal(g2[n], g3[n])]
    assert not bad, bad[:5]


def test_eval_and_the_other_switches_keep_their_bits():
    """Eval forwards never read the switch; a train-mode forward without grad does not either; setting it back and calling
    eval() gives the bits from before it was touched; with conv_precision "bf16x3" it raises, and the refusal of
    conv_precision "bf16" in train mode is the one of before."""
    x, focal, gt, mask = (v.cuda() for v in _inputs())
    m = _model().cuda()
    state = copy.deepcopy(m.state_dict())
    m.eval()
    with torch.no_grad():
        before = [o.clone() for o in m(x, focal)]
        m.train_precision = "bf16"
        during = [o.clone() for o in m(x, focal)]
    assert all(torch.equal(a, b) for a, b in zip(before, during))
    m.train()
    with torch.no_grad():
        nograd_bf16 = [o.clone() for o in m(x, focal)]
        m.train_precision = "fp32"
        nograd_fp32 = [o.clone() for o in m(x, focal)]
        m.train_precision = "bf16"
    assert all(torch.equal(a, b) for a, b in zip(nograd_bf16, nograd_fp32))
    _, outs, _ = _gpu_step(m, x, focal, gt, mask)                      # a real bf16 step in between
    assert not torch.equal(outs[4], nograd_fp32[4])
    m.conv_precision = "bf16x3"
    with pytest.raises(BtsHipError, match="conv_precision 'fp32'"):
        m(x, focal)
    m.conv_precision = "bf16"
    with pytest.raises(BtsHipError, match="inference"):
        m(x, focal)
    m.conv_precision = "fp32"
    m.train_precision = "fp32"
    m.load_state_dict(state)                                           # the running statistics the train-mode forwards moved
    m.eval()
    with torch.no_grad():
        after = m(x, focal)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert train.current_train_precision() == 0
