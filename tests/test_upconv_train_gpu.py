"""The sub-pixel upconv training path on the GPU (decoder.subpixel_upconv_train): the per-step packs, the input gradient
(bts_upconv_dgrad_f32: a 4x4 / stride-2 gather on the row-tiled convolution kernel), the weight gradient
(bts_upconv_wgrad_f32: wgrad_tile per class + the fixed-order fold) and the autograd node over them, against
ops.upconv_subpixel_grads_reference (fp64, CPU; itself checked against autograd in tests/test_upconv_train_host.py).

The exact tests feed small integers, so that every partial sum is an integer below 2^24 and fp32 accumulation is exact
in any order: tile, split and summation order cannot change a bit, and the assertion is torch.equal.  The float tests
pin fp32 products of standard-normal operands under worst-case summation bounds."""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upconv_train_cases as uc
from bts_amd import ops, synth
from parity_util import (CONFIGS, TRAIN_CASE, Params, assert_grads_close, check_train_against_golden, grad_error_report,
                         make_inputs, oracle_train_step, t)

from conftest import fp32_only

pytestmark = pytest.mark.gpu

SENTINEL = -12345.671875          # not an integer: no exact-test partial sum can equal it
U = 2.0 ** -24                    # one fp32 rounding, relative


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(str(name).encode()))


def _slice_of_wider(values, extra):
    """`values` [rows, C] as a channel slice, at a non-zero offset, of a CUDA buffer `extra` channels wider whose other
    channels are NaN (any read outside the slice poisons the result).  Returns (view, whole buffer)."""
    rows, C = values.shape
    if extra == 0:
        v = values.cuda()
        return v, v
    assert extra % 8 == 0
    buf = torch.full((rows, C + extra), float("nan"), device="cuda")
    view = buf[:, extra // 2:extra // 2 + C]
    view.copy_(values)
    return view, buf


def _rows(x):
    """[B,C,H,W] -> NHWC rows [B*H*W, C] (CPU)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


# ------------------------------------------------------------------------------------------------------------ packs
@pytest.mark.parametrize("cout,cin", uc.PACK_SHAPES, ids=lambda v: str(v))
def test_packs_are_bit_identical_to_their_torch_statements(cout, cin):
    """Float weights: the forward pack has the bits of ops.pack_upconv_subpixel (the same fp32 additions in the same
    order), the input-gradient pack those of ops.pack_upconv_dgrad_reference (each element its forward twin's sum);
    padding is zero; a second launch from the cached table after an in-place update follows the new values."""
    w = torch.randn((cout, cin, 3, 3), generator=_gen((cout, cin))).cuda()
    fs, ds = ops.upconv_train_pack_shapes(cout, cin)
    fwd = torch.full(fs, SENTINEL, device="cuda")
    dg = torch.full(ds, SENTINEL, device="cuda")
    table = ops.upconv_train_pack([w], [fwd], [dg])
    want_f = ops.pack_upconv_subpixel(w)[0]
    assert want_f.shape == fwd.shape and torch.equal(fwd, want_f)
    assert torch.equal(dg, ops.pack_upconv_dgrad_reference(w))
    w.mul_(-0.75).add_(0.125)
    ops.upconv_train_pack([w], [fwd], [dg], table=table)
    assert torch.equal(fwd, ops.pack_upconv_subpixel(w)[0]) and torch.equal(dg, ops.pack_upconv_dgrad_reference(w))


def test_one_launch_packs_several_weights():
    ws = [torch.randn((co, ci, 3, 3), generator=_gen(("multi", co, ci))).cuda() for co, ci in ((40, 48), (32, 64), (8, 4))]
    shapes = [ops.upconv_train_pack_shapes(w.shape[0], w.shape[1]) for w in ws]
    fwd = [torch.full(s[0], SENTINEL, device="cuda") for s in shapes]
    dg = [torch.full(s[1], SENTINEL, device="cuda") for s in shapes]
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        ops.upconv_train_pack(ws, fwd, dg)
    finally:
        ops.set_trace(None)
    assert [r[0] for r in tr.records] == ["upconv_train_pack_kernel"]
    for w, f, d in zip(ws, fwd, dg):
        assert torch.equal(f, ops.pack_upconv_subpixel(w)[0]) and torch.equal(d, ops.pack_upconv_dgrad_reference(w))


# --------------------------------------------------------------------------------------------------- input gradient
def _dgrad_operands(case, integer):
    B, h, w, cin, cout = case
    g = _gen(("dgrad", case, integer))
    if integer:
        wt = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).double()
        dy = torch.randint(-1, 2, (B, cout, 2 * h, 2 * w), generator=g).double()
    else:
        wt = (torch.randn((cout, cin, 3, 3), generator=g) / float(np.sqrt(9 * cin))).double()      # fp32 values
        dy = torch.randn((B, cout, 2 * h, 2 * w), generator=g).double()
    x0 = torch.zeros((B, cin, h, w), dtype=torch.float64)
    ref = ops.upconv_subpixel_grads_reference(x0, wt, dy)[1]
    mag = ops.upconv_subpixel_grads_reference(x0, wt.abs(), dy.abs())[1]        # sum of |w terms| * |dy| per element
    return wt, dy, ref, mag


def _run_dgrad(case, wt, dy, extra=8):
    B, h, w, cin, cout = case
    wc = wt.float().cuda()
    fs, ds = ops.upconv_train_pack_shapes(cout, cin)
    fwd, wd = torch.empty(fs, device="cuda"), torch.empty(ds, device="cuda")
    ops.upconv_train_pack([wc], [fwd], [wd])
    dy2d, _ = _slice_of_wider(_rows(dy).float(), extra)
    dx2d, dxbuf = _slice_of_wider(torch.full((B * h * w, cin), SENTINEL), extra)
    ws = torch.full((uc.DGRAD_SPLITK_WS,), SENTINEL, device="cuda")
    call = lambda: ops.upconv_dgrad(dy2d, B, h, w, wd, cout, cin, dx2d, splitk_ws=ws)
    return call, dx2d, dxbuf


@pytest.mark.parametrize("case", uc.DGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dgrad_is_exact_on_small_integers(case):
    B, h, w, cin, cout = case
    wt, dy, ref, mag = _dgrad_operands(case, True)
    assert mag.max().item() < 2 ** 24, "case breaks the exactness precondition"
    if case == uc.DGRAD_CASES[-1]:
        assert ops.upconv_dgrad_plan(B, h, w, cout, cin, uc.DGRAD_SPLITK_WS)[3], "the split-K case no longer splits K"
    call, dx2d, dxbuf = _run_dgrad(case, wt, dy)
    call()
    first = dx2d.cpu().double()
    assert torch.isnan(dxbuf[:, :4]).all() and torch.isnan(dxbuf[:, 4 + cin:]).all(), "wrote outside the channel slice"
    want = _rows(ref)
    assert torch.equal(first, want), "%d of %d elements differ" % (int((first != want).sum()), want.numel())
    dx2d.fill_(SENTINEL)
    call()
    assert torch.equal(dx2d.cpu().double(), want), "second call differs"


@pytest.mark.parametrize("case", uc.DGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dgrad_fp32_products_within_the_summation_bound(case):
    """Standard-normal dy, weights scaled by 1/sqrt(9 c_in).  The row-tiled kernel has no epilogue here, so an element is an
    fp32 sum of n = 16 c_out fp32 products, in at most 8 split-K parts: per element
        |got - ref| <= (n + 8 + 5) * 2^-24 * sum |w terms| * |dy|
    -- one rounding per product and a chain of at most n additions (the summation bound of the weight-gradient test,
    tests/test_wgrad_gpu.py), at most 8 more across the split-K partials, plus the 3 roundings of a packed K element (a
    sum of up to four weights, which the fp64 reference adds exactly) and 2 of margin for the conversions."""
    B, h, w, cin, cout = case
    wt, dy, ref, mag = _dgrad_operands(case, False)
    call, dx2d, _ = _run_dgrad(case, wt, dy)
    call()
    got, want = dx2d.cpu().double(), _rows(ref)
    bound = (16 * cout + 8 + 5) * U * _rows(mag)
    err = (got - want).abs()
    ratio = (err / bound).max().item()
    print("dgrad %s: max |err| / bound = %.4f" % (case, ratio))
    assert bool((err <= bound).all()), (case, ratio)


# -------------------------------------------------------------------------------------------------- weight gradient
def _wgrad_reference(c, x, dy):
    """fp64 dw as OHWI [c_out, 9, c_in] and the matching sum of |dy| * |x| over the contributing terms."""
    w0 = torch.zeros((c.c_out, c.c_in, 3, 3), dtype=torch.float64)
    ref = ops.upconv_subpixel_grads_reference(x, w0, dy)[2]
    mag = ops.upconv_subpixel_grads_reference(x.abs(), w0, dy.abs())[2]
    ohwi = lambda d: d.permute(0, 2, 3, 1).reshape(c.c_out, 9, c.c_in)
    return ohwi(ref), ohwi(mag)


def _run_wgrad(c, x, dy, ws):
    x2d, _ = _slice_of_wider(_rows(x).float(), c.x_extra)
    dy2d, _ = _slice_of_wider(_rows(dy).float(), c.dy_extra)
    return lambda: ops.upconv_wgrad(x2d, c.B, c.h, c.w, c.c_in, dy2d, c.c_out, ws)


@pytest.mark.parametrize("c", uc.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_is_exact_on_small_integers(c):
    g = _gen(c.name)
    M = c.B * c.h * c.w
    bm, bn, split, pps = uc.plan_of(c)
    # every dw tap sums 4 M terms; |x| <= 511 (10 bits: not representable in bf16) unless that many could reach 2^24
    xmax = min(511, int(0.6 * 2 ** 24 * 3 / (4 * M)))
    assert xmax >= 300
    x = torch.randint(-xmax, xmax + 1, (c.B, c.c_in, c.h, c.w), generator=g).double()
    dy = torch.randint(-1, 2, (c.B, c.c_out, 2 * c.h, 2 * c.w), generator=g).double()
    ref, mag = _wgrad_reference(c, x, dy)
    assert mag.max().item() < 2 ** 24, "case breaks the exactness precondition: shrink the range of x"
    whole = torch.full((c.ws_floats + 64,), SENTINEL, device="cuda")          # 64 floats of guard behind the workspace
    ws = whole[:c.ws_floats]
    call = _run_wgrad(c, x, dy, ws)
    first = call().cpu().double()
    used = split * 16 * c.c_out * c.c_in
    assert used <= c.ws_floats
    assert bool((whole[used:] == SENTINEL).all()), "the launch wrote workspace beyond split * 16 * c_out * c_in"
    assert not bool((ws[:used] == SENTINEL).any()), "a class block inside the workspace was never written"
    second = call().cpu().double()          # same workspace, now holding the first call's partials
    for got, what in ((first, "first call"), (second, "second call into the same workspace")):
        if not torch.equal(got, ref):
            bad = ~(got == ref)
            co, tap, ci = bad.nonzero()[0].tolist()
            pytest.fail("%s, %s: %d wrong of %d; first (co %d, tap %d, ci %d); tile %dx%d, split %d x %d pixels"
                        % (c.name, what, int(bad.sum()), bad.numel(), co, tap, ci, bm, bn, split, pps))


@pytest.mark.parametrize("name", uc.WGRAD_FLOAT_CASES)
def test_wgrad_fp32_products_within_the_summation_bound(name):
    """Standard-normal operands.  Per element |got - ref| <= (pix_per_split + split + 5) * 2^-24 * sum |dy| * |x| over the
    contributing terms: the bound of tests/test_wgrad_gpu.py (one rounding per product, a chain of at most pix_per_split
    additions inside a split and split more across them) plus three additions for the four-way fold."""
    c = uc.BY_NAME[name]
    g = _gen(name)
    bm, bn, split, pps = uc.plan_of(c)
    x = torch.randn((c.B, c.c_in, c.h, c.w), generator=g)
    dy = torch.randn((c.B, c.c_out, 2 * c.h, 2 * c.w), generator=g)
    ref, mag = _wgrad_reference(c, x.double(), dy.double())
    ws = torch.empty(c.ws_floats, device="cuda")
    got = _run_wgrad(c, x, dy, ws)().cpu().double()
    bound = (pps + split + 5) * U * mag
    err = (got - ref).abs()
    ratio = (err / bound).max().item()
    print("%s: tile %dx%d split %d x %d pixels: max |err| / bound = %.4f" % (name, bm, bn, split, pps, ratio))
    assert bool((err <= bound).all()), (name, ratio)


@pytest.mark.parametrize("name", ["t32_s16", "t64_s160"])
def test_dw_is_the_documented_fixed_order_fold_of_the_partials(name):
    """Float operands, where the summation order shows: after the launch the workspace holds the class partials as
    [split][class][c_out][4*c_in]; dw[co][3*ky+kx][ci] has the bits of ((r0 + r1) + r2) + r3, r_cls = wgrad_cases.sum_splits
    over the splits of class cls = 2*py + px at its tap (tau_py(ky), tau_px(kx)), tau_0 = (0,1,1), tau_1 = (0,0,1).
    16 splits stay in the one-at-a-time loop, 160 run the four-at-a-time loop and its tail."""
    from wgrad_cases import sum_splits
    c = uc.BY_NAME[name]
    g = _gen(name)
    bm, bn, split, pps = uc.plan_of(c)
    assert split == int(name.rsplit("_s", 1)[1])
    x = torch.randn((c.B, c.c_in, c.h, c.w), generator=g)
    dy = torch.randn((c.B, c.c_out, 2 * c.h, 2 * c.w), generator=g)
    ws = torch.full((c.ws_floats,), SENTINEL, device="cuda")
    dw = _run_wgrad(c, x, dy, ws)().cpu()
    p = ws[:split * 16 * c.c_out * c.c_in].cpu().numpy().reshape(split, 4, c.c_out, 4, c.c_in)
    tau = ops._SUBPIX_TAU
    want = np.empty((c.c_out, 9, c.c_in), np.float32)
    for ky in range(3):
        for kx in range(3):
            r = [sum_splits(p[:, cls, :, 2 * tau[cls >> 1][ky] + tau[cls & 1][kx], :]) for cls in range(4)]
            want[:, 3 * ky + kx, :] = ((r[0] + r[1]) + r[2]) + r[3]
    want = torch.from_numpy(want)
    assert torch.equal(dw, want), "%s, split %d: %d of %d elements differ" % (name, split, int((dw != want).sum()), dw.numel())


# ------------------------------------------------------------------------------------------------- node and path
def _upconv_module(cin, cout, wt):
    from bts_amd import bts as M
    m = M.upconv(cin, cout, ratio=2).cuda().train()
    with torch.no_grad():
        m.conv.weight.copy_(wt)
    return m


@pytest.mark.parametrize("case", [(2, 48, 40, 6, 9), (2, 64, 32, 13, 20)], ids=lambda c: "x".join(map(str, c)))
def test_upconv_forward_with_the_flag_on_vs_torch_cpu(case):
    """train.upconv_forward(subpixel=True): ELU(conv3x3(nearest2x(x))) and both gradients against fp64 torch on the CPU
    under the close() rule of test_conv2d_gradients_vs_torch_cpu; the forward also within the project's bar for this
    operation, 1e-5 of max|ref| (tests/test_upconv_up9_gpu.py)."""
    from bts_amd import train
    B, cin, cout, h, w = case
    gen = _gen(("path", case))
    x = torch.randn(B, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) / np.sqrt(cin * 9)
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.elu(F.conv2d(F.interpolate(x64, scale_factor=2, mode="nearest"), w64, padding=1))
    gy = torch.randn(y_ref.shape, generator=gen)
    y_ref.backward(gy.double())
    m = _upconv_module(cin, cout, wt)
    xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        y = train.upconv_forward(m, xd, subpixel=True)
        assert tuple(y.shape) == tuple(y_ref.shape)
        y.backward(gy.cuda())
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    assert {r[1] for r in tr.records} >= {"upconv.fwd", "upconv.dgrad", "upconv.wgrad"}
    assert "upconv_wgrad_kernel" in [r[0] for r in tr.records]

    def close(got, ref, what):
        ref = ref.float()
        scale = ref.abs().max().item()
        err = (got.cpu() - ref).abs().max().item()
        print("%s %s: max |err| / max|ref| = %.3g" % (case, what, err / scale))
        assert err <= 2e-5 * scale * np.sqrt(max(1, ref.numel() // ref.shape[0] // 64)) + 1e-6, (what, err, scale)
        return err / scale

    assert close(y.detach(), y_ref.detach(), "forward") <= 1e-5
    close(m.conv.weight.grad, w64.grad, "weight grad")
    close(xd.grad, x64.grad, "input grad")
    # the same ops give identical bits when run twice
    m.conv.weight.grad = None
    xd2 = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y2 = train.upconv_forward(m, xd2, subpixel=True)
    y2.backward(gy.cuda())
    assert torch.equal(y2, y) and torch.equal(xd2.grad, xd.grad)
    # flag off (the default), odd channel counts and ratio 1 stay on conv2d
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        train.upconv_forward(m, xd2.detach().requires_grad_(True)).sum().backward()
    finally:
        ops.set_trace(None)
    assert "upconv_wgrad_kernel" not in [r[0] for r in tr.records] and "conv_wgrad_kernel" in [r[0] for r in tr.records]


def _train_decoder(state=None, **flags):
    from bts_amd import bts as M
    c = TRAIN_CASE
    enc, md, ds, _, _ = CONFIGS[c["cname"]]
    feat = synth.ENCODER_CHANNELS[enc]
    dec = M.bts(Params(enc, 512, md, ds), feat, 512)
    if state is None:
        state = {k: (torch.tensor(v) if np.ndim(v) == 0 else t(v)) for k, v in synth.decoder_state(feat, 512, 0).items()}
    dec.load_state_dict(state, strict=True)
    dec = dec.train().cuda()
    for k, v in flags.items():
        assert hasattr(dec, k)
        setattr(dec, k, v)
    return dec


def _step(dec):
    """One decoder training step on TRAIN_CASE: (loss, outs, feature gradients, parameter gradients)."""
    from bts_amd import bts as M
    c = TRAIN_CASE
    _, md, ds, _, _ = CONFIGS[c["cname"]]
    feats, focal = make_inputs(c["cname"], c["B"], c["H"], c["W"], c["feat_seed"])
    feats = [None] + [f.cuda().requires_grad_(True) for f in feats[1:]]
    gt, mask = synth.train_targets(c["B"], c["H"], c["W"], md, c["target_seed"])
    for p in dec.parameters():
        p.grad = None
    outs = dec(feats, focal.cuda())
    loss = M.silog_loss(variance_focus=c["variance_focus"])(outs[4], t(gt).cuda(), t(mask).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss, outs, [f.grad for f in feats[1:]], {n: p.grad.clone() for n, p in dec.named_parameters()}


def _ratio2_upconvs(dec):
    from bts_amd import bts as M
    return [m for m in dec.modules() if isinstance(m, M.upconv) and m.ratio == 2 and m.conv.in_channels % 4 == 0
            and m.conv.out_channels % 4 == 0]


@pytest.fixture(scope="module")
def oracle_refs():
    r64, r32 = oracle_train_step(torch.float64), oracle_train_step()
    ref = {n: v.numpy() for n, v in r64["param_grads"].items()}
    return ref, grad_error_report({n: v.numpy() for n, v in r32["param_grads"].items()}, ref)


@fp32_only
@pytest.mark.parametrize("fused", [False, True], ids=["layer_graph", "fused_reduction"])
def test_decoder_train_step_with_the_flag_on_vs_golden_and_oracle(golden_dir, oracle_refs, fused):
    g = np.load(os.path.join(golden_dir, "decoder_train.npz"))
    dec = _train_decoder(subpixel_upconv_train=True, fused_reduction_train=fused)
    loss, outs, fgrads, pgrads = _step(dec)
    pg = {n: v.cpu().numpy() for n, v in pgrads.items()}
    bufs = {n: b.cpu().numpy() for n, b in dec.named_buffers() if n.endswith(("running_mean", "running_var"))}
    check_train_against_golden(g, loss.item(), [o.detach().cpu().numpy() for o in outs], [f.cpu().numpy() for f in fgrads], pg, bufs,
                               what="sub-pixel upconvs/golden", robust=True)
    ref, floor = oracle_refs
    per, l2 = grad_error_report(pg, ref)
    print("global rel-L2 vs fp64: hip %.2e, cpu fp32 oracle %.2e" % (l2, floor[1]))
    assert_grads_close(per, l2, "sub-pixel upconvs/fp64 oracle", fp32_floor=floor)


def _sums_over_upsampled_gradient(fn):
    """Shapes of the inputs of every aten::sum that reduces a 6-D tensor (the [B,h,2,w,2,C] view of an upsampled input
    gradient) while ``fn`` runs; host-side operator records only."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as prof:
        fn()
    return [e.input_shapes[0] for e in prof.events() if e.name == "aten::sum" and e.input_shapes and len(e.input_shapes[0]) == 6]


@fp32_only
def test_kernel_trace_of_the_decoder_step_flag_on_and_off():
    """Flag on: every ratio-2 upconv runs the three sub-pixel launches (its forward and input gradient issue 16 of the 36
    algorithmic products, its weight gradient is upconv_wgrad_kernel), there is no conv_wgrad launch under an upconv tag
    and no ATen sum over an upsampled gradient.  Flag off (the default): none of the new kernels, and the sums are there."""
    for on in (True, False):
        dec = _train_decoder() if not on else _train_decoder(subpixel_upconv_train=True)
        assert dec.subpixel_upconv_train is on
        n = len(_ratio2_upconvs(dec))
        assert n >= 4
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            sums = _sums_over_upsampled_gradient(lambda: _step(dec))
        finally:
            ops.set_trace(None)
        recs = [r for r in tr.records if r[1].startswith("upconv.")]
        kerns = [r[0] for r in tr.records]
        by_tag = {tag: [r for r in recs if r[1] == tag] for tag in ("upconv.fwd", "upconv.dgrad", "upconv.wgrad")}
        if on:
            assert len(sums) == 0, sums
            assert "upconv_train_pack_kernel" in kerns
            sub_fwd = [r for r in by_tag["upconv.fwd"] if r[6] <= r[2] * 16 / 36 * 1.001]      # executed vs algorithmic FLOPs
            assert len(sub_fwd) == n, "a ratio-2 upconv forward ran the up=2 gather"
            assert sum("k4s2" in r[0] for r in by_tag["upconv.dgrad"]) == n
            wg = [r[0] for r in by_tag["upconv.wgrad"]]
            assert wg.count("upconv_wgrad_kernel") == n and wg.count("conv_wgrad_kernel") == len(wg) - n
            assert len(by_tag["upconv.fwd"]) == len(by_tag["upconv.dgrad"]) == len(wg)
        else:
            assert len(sums) >= 4, sums
            for k in kerns:
                assert "upconv_wgrad" not in k and "k4s2" not in k and "upconv_train_pack" not in k, k


@fp32_only
@pytest.mark.parametrize("native", [False, True], ids=["torch_fused_adamw", "native_adamw"])
def test_packs_follow_an_in_place_optimiser_update(native):
    """Step 1, an in-place optimiser update, step 2: outputs and gradients of step 2 equal, bit for bit, those of a freshly
    built decoder loaded with the updated weights -- under torch's fused AdamW (which does not bump Tensor._version) and
    under NativeAdamW (after which the generic packer trusts versions)."""
    from bts_amd import train
    from bts_amd.optim import NativeAdamW
    try:
        dec = _train_decoder(subpixel_upconv_train=True)
        opt = (NativeAdamW(dec.parameters(), lr=1e-2, eps=1e-3, weight_decay=0.0) if native
               else torch.optim.AdamW(dec.parameters(), lr=1e-2, eps=1e-3, weight_decay=0.0, fused=True))
        _step(dec)
        before = {n: p.detach().clone() for n, p in dec.named_parameters()}
        opt.step()
        if not native:
            train._PACKER.versions_trusted = False      # trainer.make_optimizer's post-step hook for torch optimisers
        changed = [n for n, p in dec.named_parameters() if "upconv" in n and not torch.equal(p, before[n])]
        assert len(changed) >= 4, "the update did not move the upconv weights"
        # train()-mode outputs and gradients do not read the running statistics: the state as it is now is all a fresh
        # decoder needs (new parameter objects at new addresses: nothing of it is known to any packer)
        fresh = _train_decoder(state={k: v.detach().clone() for k, v in dec.state_dict().items()}, subpixel_upconv_train=True)
        loss2, outs2, fg2, pg2 = _step(dec)
        loss3, outs3, fg3, pg3 = _step(fresh)
        assert torch.equal(loss2, loss3)
        for a, b in zip(outs2, outs3):
            assert torch.equal(a, b)
        for a, b in zip(fg2, fg3):
            assert torch.equal(a, b)
        for n in pg2:
            assert torch.equal(pg2[n], pg3[n]), n
    finally:
        train._PACKER.versions_trusted = False
