"""Fused reduction_1x1 -> LPG training path on the GPU: bts_reduc_bwd_f32 + per-layer bts_conv_wgrad_f32 against the
oracle's arithmetic differentiated in fp64 on the CPU (tests/reduc_train_ref.py), the torch operators, the decoder
switch ``fused_reduction_train`` and the launch count.

Bar of the gradient comparisons (max-abs error over max-abs value, per tensor): the larger of 4x the distance of CPU fp32
autograd of the same oracle from fp64 (FLOORS below, measured once on the CPU -- the reference run, never the code under
test) and the bar tests/test_train_gpu.py::test_conv2d_gradients_vs_torch_cpu applies to one convolution (for dx counted per pixel, so that it does not grow with
the map: reduc_train_ref.conv_bar).  The 4x covers a
different fp32 summation order (MFMA accumulation, wgrad pixel split) and the <= 1e-7 absolute error of the common.h
intrinsics; a dropped term or a wrong mask is percent-level."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import reduc_train_ref as R
from bts_amd import ops, synth
from parity_util import CONFIGS, TRAIN_CASE, Params, assert_grads_close, grad_error_report, make_inputs, t

pytestmark = pytest.mark.gpu

MD = R.MAX_DEPTH

# CPU fp32 autograd vs CPU fp64 autograd of the oracle, max-abs error / max-abs value per tensor
FLOORS = {
    "8x8": {"dx": 4.45e-07, "dW0": 5.79e-07, "dW1": 6.28e-07, "dW2": 4.9e-07, "dW3": 7.79e-07, "dW4": 4.74e-07, "dW5": 4.39e-07},
    "4x4": {"dx": 1.38e-06, "dW0": 6.4e-07, "dW1": 6.25e-07, "dW2": 5.43e-07, "dW3": 4.99e-07, "dW4": 8.03e-07},
    "2x2": {"dx": 7.98e-07, "dW0": 7.37e-07, "dW1": 4.93e-07, "dW2": 3.92e-07, "dW3": 3.02e-07},
    "final": {"dx": 1.61e-07, "dW0": 1.62e-07, "dW1": 1.59e-07, "dW2": 2.42e-07},
    "clamp": {"dx": 1.18e-04, "dW0": 1.08e-04, "dW1": 1.0e-04, "dW2": 1.19e-04, "dW3": 6.16e-05, "dW4": 1.06e-04, "dW5": 8.8e-05},
    "persistent": {"dx": 2.59e-06, "dW0": 8.46e-07, "dW1": 7.86e-07, "dW2": 6.42e-07, "dW3": 3.95e-07},
    "persistent2": {"dx": 8.88e-07, "dW0": 7.06e-07, "dW1": 5.6e-07, "dW2": 6.2e-07, "dW3": 4.43e-07},
}


def _gpu_inputs(x, ws, grad=True):
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(grad)
    wd = [wt.cuda().requires_grad_(grad) for wt in ws]
    return xd, wd


def _function_grads(name, x, ws, gout):
    """Gradients of one scale through the autograd.Function path: ({"dx", "dW0", ...} as numpy, output, abs_min)."""
    k = R.CHAINS[name][2]
    xd, wd = _gpu_inputs(x, ws)
    packs = ops.reduc_train_packs(wd)
    am = torch.empty((), dtype=torch.float32, device="cuda")
    if k:
        out = ops.ReducLpgFunction.apply(xd, MD, k, packs, am, None, *wd)
    else:
        out = ops.ReducFinalFunction.apply(xd, MD, packs, None, *wd)
    out.backward(gout.cuda())
    torch.cuda.synchronize()
    g = {"dx": xd.grad.cpu().numpy()}
    for i, wt in enumerate(wd):
        g["dW%d" % i] = wt.grad.cpu().numpy()
    return g, out.detach(), am


def _assert_within_bar(got, ref, floors, what):
    errs = R.rel_errors(got, ref)
    bars = {n: max(4.0 * floors[n], R.conv_bar(ref[n], n)) for n in ref}
    print(what, "rel errors", {n: float("%.2e" % e) for n, e in errs.items()}, "bars", {n: float("%.2e" % b) for n, b in bars.items()})
    for n in ref:
        assert got[n].shape == ref[n].shape, (what, n, got[n].shape, ref[n].shape)
        assert errs[n] <= bars[n], (what, n, errs[n], bars[n])


# ------------------------------------------------------------------------------------------ 1. per-chain gradients
@pytest.mark.parametrize("name", list(R.PLAIN_CASES))
def test_chain_gradients_vs_fp64_oracle(name):
    """70 cells (k = 8, 4, 2) = three wave tiles, the last partial, straddling row ends and the batch boundary; the final
    chain at 2 x 6 x 10."""
    x, ws, gout, g64, den = R.case_reference(name, R.PLAIN_CASES[name])
    if den is not None:
        assert np.abs(den).min() >= 1e-2, "a pixel of the reference sits near the LPG clamp"
    got, _, _ = _function_grads(name, x, ws, gout)
    _assert_within_bar(got, g64, FLOORS[name], name)


# ------------------------------------------------------------------------------------------ 2. clamp branch
def test_clamp_branch():
    """theta -> pi/3 (theta row of plane_params x 50): the denominator crosses zero in block corners of the 8x8 scale.
    Seed search on the CPU against the fp64 oracle: over seeds 0..999 no map of 2 x 5 x 7 or 2 x 9 x 11 cells has 8 pixels
    with |den| < 5e-4 at all (at most 3 and 5: a cell's denominator is a plane of slope <= 0.11 per pixel, so about one
    corner pixel in a hundred lands that close to zero); 2 x 24 x 32 cells average 4.9 such pixels, and seed 743 is the
    one seed there with >= 8 of them and none within 20 % of 1e-3 or below 1e-6."""
    name = R.CLAMP_CASE[0]
    x, ws, gout, g64, den = R.case_reference("clamp", R.CLAMP_CASE)
    a = np.abs(den)
    assert (a < 5e-4).sum() >= 8
    assert not ((a > 0.8e-3) & (a < 1.2e-3)).any() and not (a < 1e-6).any()
    got, _, _ = _function_grads(name, x, ws, gout)
    _assert_within_bar(got, g64, FLOORS["clamp"], "clamp")


# ------------------------------------------------------------------------------------------ 3. strides and poison
def _raw_backward(name, B, h, w, x2d, wd, gout, dx2d):
    c_in, c_first, k = R.CHAINS[name]
    npix = B * h * w
    _, yc = ops.reduc_train_cols(c_in, c_first)
    packs = ops.reduc_train_packs(wd)
    Y = torch.full((npix, yc), 7.0, device="cuda")
    G = torch.full((npix, yc + 4), 7.0, device="cuda")
    ops.reduc_backward(x2d, B, h, w, c_in, c_first, packs[1], packs[2], MD, k, gout, Y, G, dx2d)
    torch.cuda.synchronize()
    return Y, G


@pytest.mark.parametrize("name", list(R.PLAIN_CASES))
def test_strided_poisoned_input_bit_identical(name):
    case = R.PLAIN_CASES[name]
    _, B, h, w, _, _ = case
    c_in = R.CHAINS[name][0]
    x, ws, gout, _, _ = R.case_reference(name, case)
    npix = B * h * w
    rows = x.permute(0, 2, 3, 1).reshape(npix, c_in).cuda().contiguous()
    wd = [wt.cuda() for wt in ws]
    g = gout.cuda().contiguous()
    dx_dense = torch.empty((npix, c_in), device="cuda")
    Y0, G0 = _raw_backward(name, B, h, w, rows, wd, g, dx_dense)
    xbuf = torch.full((npix, c_in + 8), float("nan"), device="cuda")
    xbuf[:, :c_in] = rows
    SENT = -12345.0
    dxbuf = torch.full((npix, c_in + 12), SENT, device="cuda")
    Y1, G1 = _raw_backward(name, B, h, w, xbuf[:, :c_in], wd, g, dxbuf[:, :c_in])
    assert torch.equal(Y0, Y1) and torch.equal(G0, G1)
    assert torch.equal(dxbuf[:, :c_in], dx_dense)
    assert (dxbuf[:, c_in:] == SENT).all()
    assert torch.isfinite(dx_dense).all() and torch.isfinite(G0).all() and torch.isfinite(Y0).all()
    assert (G0[:, -1] == 0).all()                            # the last layer's columns are zero-padded to 4


# ------------------------------------------------------------------------------------------ 4. persistent loop
@pytest.mark.parametrize("passes", [1, 2])
def test_persistent_loop(passes):
    """One partial tile more than one pass of the whole grid (the grid-stride loop of the 2x2 chain wraps on one wave),
    and more than two passes (every wave iterates at least twice)."""
    waves = ops.reduc_bwd_max_waves(64, 32, 2)
    h, w = R.persistent_shape(waves, passes)
    assert 0 < h * w - passes * waves * 32 < 32
    key = "persistent" if passes == 1 else "persistent2"
    x, ws, gout, g64, den = R.case_reference(key, ("2x2", 1, h, w, 0, None))
    assert np.abs(den).min() >= 1e-2
    got, _, _ = _function_grads("2x2", x, ws, gout)
    _assert_within_bar(got, g64, FLOORS[key], key)


# ------------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("name", list(R.PLAIN_CASES))
def test_backward_is_deterministic(name):
    x, ws, gout, _, _ = R.case_reference(name, R.PLAIN_CASES[name])
    a, _, _ = _function_grads(name, x, ws, gout)
    b, _, _ = _function_grads(name, x, ws, gout)
    for n in a:
        assert np.array_equal(a[n], b[n]), n


# ------------------------------------------------------------------------------------------ 6. forward == inference
@pytest.mark.parametrize("name", ["8x8", "4x4", "2x2"])
def test_training_forward_equals_inference_forward(name):
    from bts_amd import bts as M
    from bts_amd import train
    c_in, c_first, k = R.CHAINS[name]
    _, B, h, w, _, _ = R.PLAIN_CASES[name]
    x, ws, _, _, _ = R.case_reference(name, R.PLAIN_CASES[name])
    red = M.reduction_1x1(c_in, c_first, MD).train().cuda()
    convs = [m for m in red.reduc.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        for m, wt in zip(convs, ws):
            m.weight.copy_(wt.cuda())
    lpg = M.local_planar_guidance(k)
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    depth = train.fused_lpg_scale(red, lpg, xd)
    assert depth.requires_grad and tuple(depth.shape) == (B, 1, h * k, w * k)
    rows = x.permute(0, 2, 3, 1).reshape(B * h * w, c_in).cuda().contiguous()
    ref = torch.empty((B, 1, h * k, w * k), device="cuda")
    am = torch.empty((), device="cuda")
    ops.reduc_lpg_forward(rows, B, h, w, c_in, c_first, ops.pack_reduc_weights([wt.cuda() for wt in ws]), MD, k, ref, abs_min=am)
    torch.cuda.synchronize()
    assert torch.equal(depth.detach(), ref)
    assert torch.equal(lpg.abs_min, am)


# ------------------------------------------------------------------------------------------ 7. torch operators
@pytest.mark.parametrize("name", ["8x8", "2x2", "final"])
def test_torch_ops_match_function_path(name):
    """torch.ops.bts_hip.reduc_lpg_train / reduction_1x1_train + .sum().backward() == the autograd.Function path, bit
    for bit.  (The operators do not exist before this feature.)"""
    tops = ops.torch_ops()
    assert tops is not None
    c_in, c_first, k = R.CHAINS[name]
    _, B, h, w, _, _ = R.PLAIN_CASES[name]
    x, ws, _, _, _ = R.case_reference(name, R.PLAIN_CASES[name])
    kk = max(k, 1)
    ones = torch.ones(B, 1, h * kk, w * kk)
    ref, out_ref, am_ref = _function_grads(name, x, ws, ones)
    x2d = x.permute(0, 2, 3, 1).reshape(B * h * w, c_in).cuda().contiguous().requires_grad_(True)
    wd = [wt.cuda().requires_grad_(True) for wt in ws]
    packs = list(ops.reduc_train_packs(wd))
    if k:
        out, am = torch.ops.bts_hip.reduc_lpg_train(x2d, B, h, w, wd, packs, MD, k)
        assert torch.equal(am, am_ref)
    else:
        out = torch.ops.bts_hip.reduction_1x1_train(x2d, B, h, w, wd, packs, MD)
    assert out.requires_grad and torch.equal(out.detach(), out_ref)
    out.sum().backward()
    torch.cuda.synchronize()
    dx = x2d.grad.view(B, h, w, c_in).permute(0, 3, 1, 2).cpu().numpy()
    assert np.array_equal(dx, ref["dx"])
    for i, wt in enumerate(wd):
        assert np.array_equal(wt.grad.cpu().numpy(), ref["dW%d" % i]), i


# ------------------------------------------------------------------------------------------ 8. whole decoder
def _decoder_step(fused):
    from bts_amd import bts as M
    c = TRAIN_CASE
    enc, md, ds, _, _ = CONFIGS[c["cname"]]
    feat = synth.ENCODER_CHANNELS[enc]
    dec = M.bts(Params(enc, 512, md, ds), feat, 512)
    sd = {k: (torch.tensor(v) if np.ndim(v) == 0 else t(v)) for k, v in synth.decoder_state(feat, 512, 0).items()}
    dec.load_state_dict(sd, strict=True)
    dec = dec.train().cuda()
    dec.fused_reduction_train = fused
    feats, focal = make_inputs(c["cname"], c["B"], c["H"], c["W"], c["feat_seed"])
    feats = [None] + [f.cuda().requires_grad_(True) for f in feats[1:]]
    gt, mask = synth.train_targets(c["B"], c["H"], c["W"], md, c["target_seed"])
    outs = dec(feats, focal.cuda())
    loss = M.silog_loss(variance_focus=c["variance_focus"])(outs[4], t(gt).cuda(), t(mask).cuda())
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": np.array([loss.item()])}
    for i, o in enumerate(outs):
        res["out%d" % i] = o.detach().cpu().numpy()
    for i, f in enumerate(feats[1:]):
        res["feat%d" % i] = f.grad.cpu().numpy()
    for n, p in dec.named_parameters():
        assert p.grad is not None, n
        res[n] = p.grad.cpu().numpy()
    am = [dec.lpg8x8.abs_min.item(), dec.lpg4x4.abs_min.item(), dec.lpg2x2.abs_min.item()]
    return res, am


def test_whole_decoder_flag_on_equals_flag_off():
    off, am_off = _decoder_step(False)
    on, am_on = _decoder_step(True)
    per, l2 = grad_error_report(on, off)
    print("fused vs layer-by-layer: global rel-L2 %.2e, worst tensor %.2e" % (l2, max(per.values())))
    assert_grads_close(per, l2, "fused reduction training vs the layer-by-layer graph")
    np.testing.assert_allclose(am_on, am_off, rtol=1e-3)


# ------------------------------------------------------------------------------------------ 9. launch count
def test_launch_count_of_one_scale():
    from bts_amd import bts as M
    from bts_amd import train
    name = "8x8"
    c_in, c_first, k = R.CHAINS[name]
    x, ws, gout, _, _ = R.case_reference(name, R.PLAIN_CASES[name])
    n_layers = len(ws)
    red = M.reduction_1x1(c_in, c_first, MD).train().cuda()
    lpg = M.local_planar_guidance(k)

    def run(fused):
        xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        red.zero_grad()
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            if fused:
                depth = train.fused_lpg_scale(red, lpg, xd)
            else:
                r = train.reduction_forward(red, xd)
                plane_eq = torch.cat([F.normalize(r[:, :3], 2, 1), r[:, 3:4]], 1).contiguous()
                depth = lpg(plane_eq, None).unsqueeze(1) / MD
            fwd = len(tr.records)
            depth.backward(gout.cuda())
            torch.cuda.synchronize()
            return fwd, len(tr.records) - fwd
        finally:
            ops.set_trace(None)

    run(False)                                  # first use packs the layer-by-layer path's weights: not counted
    fwd_off, bwd_off = run(False)
    fwd_on, bwd_on = run(True)
    print("library calls fwd/bwd: fused %d/%d, layer-by-layer %d/%d" % (fwd_on, bwd_on, fwd_off, bwd_off))
    assert fwd_on == 1
    assert bwd_on <= 2 + n_layers
    assert fwd_off + bwd_off > fwd_on + bwd_on and bwd_off > bwd_on
