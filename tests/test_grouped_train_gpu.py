"""GPU: ResNeXt's grouped 3x3 natively in the training step -- the weight-gradient kernel (csrc/conv_grouped_wgrad.inc,
ops.conv_grouped_wgrad) exactly against fp64 autograd inside poisoned buffers, the input gradient on the forward kernel
through train.conv2d(grouped_native=True), float cases beside the bundle path, the per-step packs after optimiser steps,
and one whole-model step of BtsModel with ``grouped_conv_train`` set."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bts_amd import synth
from oracle import bts_oracle as O
from parity_util import Params, assert_grads_close, grad_error_report, t

from conftest import fp32_only

pytestmark = pytest.mark.gpu

PAD, OFF = 8, 4                 # both views are 8 floats wider than c and start at column 4
GUARD = 64                      # floats in front of and behind dw
POISON = -12345.0


def _fwd_kernel(cg):
    return "conv_grouped_kernel<%d>" % cg


def _wgrad_kernel(cg):
    return "conv_grouped_wgrad_kernel<%d>" % cg


def _reference(x, wt, dy, groups):
    """fp64 autograd of F.conv2d(groups=): (y, dx, dw)."""
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = F.conv2d(x64, w64, padding=1, groups=groups)
    y.backward(dy.double())
    return y.detach(), x64.grad, w64.grad


def _wide(v):
    """[B, c, h, w] host tensor -> a [B*h*w, c] NHWC device view inside a buffer 8 floats wider, junk around it."""
    B, c, h, w = v.shape
    buf = torch.full((B * h * w, c + PAD), 7.0e4, device="cuda")
    buf[:, OFF:OFF + c] = v.permute(0, 2, 3, 1).reshape(B * h * w, c).cuda()
    return buf[:, OFF:OFF + c]


def _run_wgrad(x, dy, groups, ws, trace=None):
    """ops.conv_grouped_wgrad on strided views, dw written into a poisoned buffer: (dw on the host, poison intact?)."""
    from bts_amd import ops
    B, c, h, w = x.shape
    n = c * (c // groups) * 9
    flat = torch.full((2 * GUARD + n,), POISON, device="cuda")
    dw = flat[GUARD:GUARD + n].view(c, c // groups, 3, 3)
    ops.set_trace(trace)
    try:
        out = ops.conv_grouped_wgrad(_wide(x), B, h, w, _wide(dy), c, groups, ws=ws, dw=dw)
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    assert out.data_ptr() == dw.data_ptr()
    intact = bool((flat[:GUARD] == POISON).all()) and bool((flat[GUARD + n:] == POISON).all())
    return dw.cpu().clone(), intact


def _train_ws():
    from bts_amd import train
    return train._workspace(torch.device("cuda", torch.cuda.current_device()))


WGRAD_CASES = [
    # B, h, w, c, groups
    (1, 1, 1, 64, 16),            # one pixel: three waves of the workgroup see no pixel at all
    (1, 3, 5, 64, 8),             # smaller than a tile
    (2, 7, 33, 128, 8),           # ragged both ways, 6 tiles
    (3, 17, 9, 128, 32),          # 4 channels per group
    (2, 9, 17, 192, 48),          # three slabs
    (3, 35, 250, 256, 16),        # 240 tiles: split over 120 workgroups per slab with the training workspace
]


@pytest.mark.parametrize("B,h,w,c,groups", WGRAD_CASES, ids=lambda v: str(v))
def test_weight_gradient_exact_integer_cases(B, h, w, c, groups):
    """Integer x, dy in [-15, 15]: every partial sum is an integer below 2^24, so any summation order is exact and dw must
    equal fp64 autograd bit for bit -- with the training workspace (split where the planner splits) and with ws=None (one
    workgroup per slab), x and dy read from wider buffers, dw written between guard bands that keep their poison."""
    from bts_amd import ops
    assert 225 * 26250 < 2 ** 24 and B * h * w <= 26250
    g = torch.Generator().manual_seed(1000 * h + 10 * w + groups)
    x = torch.randint(-15, 16, (B, c, h, w), generator=g).float()
    dy = torch.randint(-15, 16, (B, c, h, w), generator=g).float()
    ref = _reference(x, torch.zeros(c, c // groups, 3, 3), dy, groups)[2].float()
    ws = _train_ws()
    splits, used = ops.conv_grouped_wgrad_plan(B, h, w, c, groups, ws.numel())
    tiles = B * ((h + 7) // 8) * ((w + 15) // 16)
    assert splits == -(-tiles // -(-tiles // min(tiles, -(-512 // (c // 64))))) and used <= ws.numel()
    if (B, h, w) == (3, 35, 250):
        assert splits == 120
    got, intact = _run_wgrad(x, dy, groups, ws)
    assert torch.equal(got, ref), "split %d: max |diff| %g" % (splits, float((got - ref).abs().max()))
    assert intact
    one, intact = _run_wgrad(x, dy, groups, None)
    assert torch.equal(one, ref), "unsplit: max |diff| %g" % float((one - ref).abs().max())
    assert intact
    if splits > 2:                 # a workspace with room for two partials only: the split drops, never an error
        two, intact = _run_wgrad(x, dy, groups, ws[:2 * 144 * c])
        assert ops.conv_grouped_wgrad_plan(B, h, w, c, groups, 2 * 144 * c)[0] == 2
        assert torch.equal(two, ref) and intact


@pytest.mark.parametrize("cg", [4, 8, 16])
def test_one_hot_dy_channel_reaches_its_own_rows_only(cg):
    c, h, w, ch, B = 128, 9, 20, 77, 2
    groups = c // cg
    g = torch.Generator().manual_seed(cg)
    x = torch.randint(1, 9, (B, c, h, w), generator=g).float()            # no zero: every entry of the row is hit
    dy = torch.zeros((B, c, h, w))
    dy[:, ch] = torch.randint(1, 9, (B, h, w), generator=g).float()
    got, intact = _run_wgrad(x, dy, groups, _train_ws())
    rows = torch.zeros(c, dtype=torch.bool)
    rows[ch] = True
    assert intact and bool((got[~rows] == 0).all()) and bool((got[rows] != 0).all())
    assert torch.equal(got, _reference(x, torch.zeros(c, cg, 3, 3), dy, groups)[2].float())


def test_one_infinite_value_stays_in_its_group():
    """cg 8 on a ragged map: +inf in one x channel reaches only the dw entries (output channel of its group, that input
    channel); +inf in one dy channel only that output channel's rows.  Everything else has the bits of the clean run: the
    cross-group products of the 16-channel block never reach dw, and pixels of ragged tiles outside the map add nothing."""
    B, c, groups, h, w, ch = 1, 128, 16, 9, 20, 37
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, c, h, w), generator=g)
    dy = torch.randn((B, c, h, w), generator=g)
    clean, _ = _run_wgrad(x, dy, groups, None)
    assert bool(torch.isfinite(clean).all())
    xi = x.clone()
    xi[0, ch, 8, 19] = float("inf")                                       # the map's last pixel: next to the ragged edge
    got, _ = _run_wgrad(xi, dy, groups, None)
    hit = torch.zeros((c, 8, 3, 3), dtype=torch.bool)
    hit[ch // 8 * 8:ch // 8 * 8 + 8, ch % 8] = True
    assert torch.equal(got[~hit], clean[~hit]) and not bool(torch.isfinite(got[hit]).all())
    di = dy.clone()
    di[0, ch, 4, 7] = float("inf")
    got, _ = _run_wgrad(x, di, groups, None)
    hit = torch.zeros((c, 8, 3, 3), dtype=torch.bool)
    hit[ch] = True
    assert torch.equal(got[~hit], clean[~hit]) and not bool(torch.isfinite(got[hit]).any())


def _conv2d_step(x, wt, dy, groups, native, trace=None):
    """train.conv2d forward + backward on device copies: (y, dx, dw) on the host."""
    from bts_amd import ops, train
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = wt.cuda().requires_grad_(True)
    ops.set_trace(trace)
    try:
        with ops.launch_config(fill_frames=16, precision="fp32"):
            y = train.conv2d(xd, wd, padding=1, groups=groups, grouped_native=native, tag="l")
            y.backward(dy.cuda())
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    return y.detach().cpu(), xd.grad.cpu(), wd.grad.cpu()


@fp32_only            # the native layers are an fp32 path: the emulated run keeps them on bundles
@pytest.mark.parametrize("B,h,w,c,groups", WGRAD_CASES[1:5], ids=lambda v: str(v))
def test_input_gradient_exact_through_conv2d(B, h, w, c, groups):
    """train.conv2d(grouped_native=True): integer x and dy in [-15, 15], weights in {-1, 0, 1}: y, dx (the forward kernel on dy
    with the flipped, group-transposed pack) and dw are bit-equal to fp64 autograd."""
    g = torch.Generator().manual_seed(7 * h + w + groups)
    x = torch.randint(-15, 16, (B, c, h, w), generator=g).float()
    dy = torch.randint(-15, 16, (B, c, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (c, c // groups, 3, 3), generator=g).float()
    assert 9 * 16 * 15 < 2 ** 24 and 225 * B * h * w < 2 ** 24
    y_ref, dx_ref, dw_ref = _reference(x, wt, dy, groups)
    y, dx, dw = _conv2d_step(x, wt, dy, groups, True)
    assert dw.shape == wt.shape and dw.is_contiguous()
    assert torch.equal(y, y_ref.float()) and torch.equal(dx, dx_ref.float()) and torch.equal(dw, dw_ref.float())


@fp32_only            # the native layers are an fp32 path: the emulated run keeps them on bundles
@pytest.mark.parametrize("B,h,w,c,groups", [(2, 26, 34, 512, 32), (2, 10, 14, 128, 32)])
def test_float_vs_fp64_beside_the_bundle_path(B, h, w, c, groups):
    """randn operands: y, dx and dw against fp64 within 5e-5 of max|ref| (the bar
    test_grouped_and_strided_conv_gradients_vs_torch_cpu sets for these layers), the bundle path's errors printed beside
    them; two native runs are bit-identical; the trace shows the forward kernel twice, the weight-gradient kernel once and
    no bundle launch."""
    from bts_amd import ops
    cg = c // groups
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn((B, c, h, w), generator=g)
    wt = torch.randn((c, cg, 3, 3), generator=g) / np.sqrt(9.0 * cg)
    dy = torch.randn((B, c, h, w), generator=g)
    refs = _reference(x, wt, dy, groups)
    tr = ops.KernelTrace()
    got = _conv2d_step(x, wt, dy, groups, True, trace=tr)
    summ = tr.summary()
    assert set(summ) <= {_fwd_kernel(cg), _wgrad_kernel(cg), "pack_weights_kernel"}, sorted(summ)
    assert summ[_fwd_kernel(cg)]["launches"] == 2 and set(summ[_fwd_kernel(cg)]["tags"]) == {"l.fwd", "l.dgrad"}
    assert summ[_wgrad_kernel(cg)]["launches"] == 1 and set(summ[_wgrad_kernel(cg)]["tags"]) == {"l.wgrad"}
    assert summ[_wgrad_kernel(cg)]["flops"] == 2.0 * B * h * w * c * cg * 9
    again = _conv2d_step(x, wt, dy, groups, True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    tr = ops.KernelTrace()
    bundles = _conv2d_step(x, wt, dy, groups, False, trace=tr)
    assert not any(k.startswith("conv_grouped") for k in tr.summary())
    for what, a, b, r in zip(("y", "dx", "dw"), got, bundles, refs):
        scale = r.abs().max().item()
        err, err_b = (a.double() - r).abs().max().item() / scale, (b.double() - r).abs().max().item() / scale
        print((B, h, w, c, groups), what, "max error / max|ref|: native %.3g, bundles %.3g" % (err, err_b))
        assert err <= 5e-5, (what, err)


@fp32_only            # the native layers are an fp32 path: the emulated run keeps them on bundles
@pytest.mark.parametrize("native_optim", [False, True], ids=["torch_adamw", "native_adamw"])
def test_packs_follow_the_optimiser(native_optim):
    """Two optimiser steps on one grouped layer plus a loss.  Every begin_step() issues ONE pack launch, after which both
    native packs hold the index-by-index layout of the CURRENT parameter and the native forward equals a forward from
    freshly packed weights bit for bit; a weight rewritten in the open after begin_step() is re-packed on the spot."""
    from bts_amd import ops, optim, train
    B, c, groups, h, w = 2, 128, 32, 10, 14
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, c, h, w), generator=g).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tgt = torch.randn((B, c, h, w), generator=g).cuda()
    wt = torch.nn.Parameter((torch.randn((c, c // groups, 3, 3), generator=g) / 6.0).cuda())
    if native_optim:
        opt = optim.NativeAdamW([wt], lr=1e-2)
    else:
        opt = torch.optim.AdamW([wt], lr=1e-2, fused=True)
        opt.register_step_post_hook(lambda *a: setattr(train._PACKER, "versions_trusted", False))   # trainer.make_optimizer's hook

    def begin():
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            train.begin_step()
        finally:
            ops.set_trace(None)
        return sum(1 for r in tr.records if r[0] == "pack_weights_kernel")

    def forward():
        with ops.launch_config(fill_frames=16, precision="fp32"):
            return train.conv2d(x, wt, padding=1, groups=groups, grouped_native=True)

    seen = [wt.detach().clone()]
    for step in range(2):
        n_pack = begin()
        assert n_pack == (1 if step else n_pack)                           # step 0: the layer is not registered yet
        opt.zero_grad(set_to_none=True)
        ((forward() - tgt) ** 2).mean().backward()
        opt.step()
        seen.append(wt.detach().clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert begin() == 1
    P = train.WeightPacker
    for mode, dgrad in ((P.FWD_NATIVE, False), (P.DGRAD_NATIVE, True)):
        e = train._PACKER.entries[(wt.data_ptr(), tuple(wt.shape), 0, mode, groups)]
        assert torch.equal(e["dst"], ops.pack_grouped_train_reference(wt.detach(), groups, dgrad))
    y = forward().detach()
    x2d = x.detach().permute(0, 2, 3, 1).reshape(B * h * w, c)
    fresh = ops.conv_grouped_forward(x2d, B, h, w, ops.pack_grouped_native(wt.detach(), groups), c, groups)
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(B * h * w, c), fresh)
    with torch.no_grad():                                                  # a stale entry met later: re-packed on the spot
        wt.mul_(0.5)
    y = forward().detach()
    fresh = ops.conv_grouped_forward(x2d, B, h, w, ops.pack_grouped_native(wt.detach(), groups), c, groups)
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(B * h * w, c), fresh)


def _native_launches(summ):
    fwd = sum(d["launches"] for k, d in summ.items() if k.startswith("conv_grouped_kernel"))
    wgrad = sum(d["launches"] for k, d in summ.items() if k.startswith("conv_grouped_wgrad_kernel"))
    return fwd, wgrad


def _tag_launches(summ, suffix):
    return sum(v["launches"] for d in summ.values() for tag, v in d["tags"].items() if tag.endswith(suffix))


@fp32_only            # the native layers are an fp32 path: the emulated run keeps them on bundles
def test_btsmodel_train_step_resnext50_native_grouped_vs_cpu():
    """The recipe and bar of test_btsmodel_train_step_resnext50_vs_cpu with ``grouped_conv_train = True``: 11 of the 16
    grouped layers (stride 1, <= 16 channels per group) run natively in all three passes -- 22 launches of the forward
    kernel, 11 of the weight-gradient kernel -- and the other five stay on bundles; the default issues no native launch, and
    neither does thread precision bf16x3 with the switch on."""
    from bts_amd import bts as M, ops
    params = Params("resnext50_bts", 512, 10.0, "nyu")
    torch.manual_seed(31)
    model = M.BtsModel(params).train()
    B, H, W = 2, 64, 96
    x = torch.from_numpy(synth.image_batch(B, H, W, 15))
    focal = torch.from_numpy(synth.focal_values(B, "nyu", 15))
    gt, mask = synth.train_targets(B, H, W, 10.0, 19)

    def cpu_step(dtype):
        enc = copy.deepcopy(model.encoder).to(dtype)
        state = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone())
                 for k, v in model.decoder.state_dict().items()}
        for k, v in state.items():
            if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
                v.requires_grad_(True)
        outs = O.decoder_forward(state, enc(x.to(dtype)), focal.to(dtype), 10.0, "nyu", training=True)
        loss = O.silog_loss(outs[4], t(gt).to(dtype), t(mask), 0.85)
        loss.backward()
        grads = {"encoder." + n: p.grad for n, p in enc.named_parameters() if p.grad is not None}
        grads.update({"decoder." + n: v.grad for n, v in state.items() if v.requires_grad})
        return loss.item(), grads

    loss64, g64 = cpu_step(torch.float64)
    loss32, g32 = cpu_step(torch.float32)
    mg = model.cuda()
    assert mg.grouped_conv_train is False

    def gpu_step(precision=None):
        mg.zero_grad(set_to_none=True)
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            if precision is None:
                outs = mg(x.cuda(), focal.cuda())
                loss = M.silog_loss(0.85)(outs[4], t(gt).cuda(), t(mask).cuda())
                loss.backward()
            else:
                with ops.launch_config(precision=precision):
                    outs = mg(x.cuda(), focal.cuda())
                    loss = M.silog_loss(0.85)(outs[4], t(gt).cuda(), t(mask).cuda())
                    loss.backward()
        finally:
            ops.set_trace(None)
        torch.cuda.synchronize()
        return loss, tr.summary()

    mg.grouped_conv_train = True
    loss, summ = gpu_step()
    assert _native_launches(summ) == (22, 11)
    assert abs(loss.item() - loss64) <= max(2e-4 * abs(loss64), 4 * abs(loss32 - loss64)), (loss.item(), loss64, loss32)
    got = {n: p.grad.cpu().numpy() for n, p in mg.named_parameters() if p.grad is not None}
    assert set(got) == set(g64), set(got) ^ set(g64)          # the unused fc head gets no gradient on either side
    ref = {n: v.numpy() for n, v in g64.items()}
    per, l2 = grad_error_report(got, ref)
    per32, l2_32 = grad_error_report({n: v.numpy() for n, v in g32.items()}, ref)
    print("ResNeXt50 whole-model step, native grouped, global rel-L2 vs fp64: hip %.2e, cpu fp32 %.2e; worst tensor hip %.2e, "
          "cpu fp32 %.2e" % (l2, l2_32, max(per.values()), max(per32.values())))
    assert_grads_close(per, l2, "resnext50 whole model, native grouped / fp64", fp32_floor=(per32, l2_32))
    enc_launches = {s: _tag_launches(summ, s) for s in ("enc.fwd", "enc.dgrad", "enc.wgrad")}

    mg.grouped_conv_train = False
    _, summ = gpu_step()
    assert _native_launches(summ) == (0, 0)
    # the same layers launch once per pass either way: with the switch on, 16 - 11 = 5 grouped layers stayed on bundles
    assert {s: _tag_launches(summ, s) for s in enc_launches} == enc_launches

    mg.grouped_conv_train = True
    _, summ = gpu_step("bf16x3")
    assert _native_launches(summ) == (0, 0)
    assert all(bool(torch.isfinite(p.grad).all()) for p in mg.parameters() if p.grad is not None)
