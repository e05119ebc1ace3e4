"""GPU: the bf16 grouped 3x3 kernel (csrc/conv_grouped_bf16.inc, ops.conv_grouped_bf16_forward) -- exact integer cases against
fp64 F.conv2d(groups=) inside poisoned buffers, nearest-even rounding of the input, group leakage, confinement of a non-finite
value, float cases at the bf16 mode's bar beside the bundle path of that mode, and the ResNeXt encoders / BtsModel with
``grouped_conv_bf16`` set."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bts_amd import synth
from oracle import bts_oracle as O
from parity_util import OUT_NAMES, Params, singular_masks, t
from test_conv_grouped_gpu import EXACT_CASES

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 1}
PAD, OFF = 8, 4                 # both views are 8 floats wider than c and start at column 4
GUARD = 64                      # floats in front of and behind the output rows
POISON = -12345.0


def _kernel(cg):
    return "conv_grouped_bf16_kernel<%d>" % cg


def _rne(v):
    """fp32 -> bf16 (round to nearest even) -> fp64: the operand the kernel contracts."""
    return v.float().to(torch.bfloat16).double()


def _affine_act(ref, e1, act):
    if e1 is not None:
        ref = ref * e1[0].double().view(1, -1, 1, 1) + e1[1].double().view(1, -1, 1, 1)
    return torch.relu(ref) if act == "relu" else ref


def _reference(x, wt, groups, e1, act):
    """fp64 grouped conv3x3 of the operands as given -> e1 affine -> activation, [B, c, h, w]."""
    return _affine_act(F.conv2d(x.double(), wt.double(), padding=1, groups=groups), e1, act)


def _run_native(x, wt, groups, e1, act, trace=None, tag=None):
    """The new op on NCHW host tensors, x read from and y written into channel slices of wider buffers: the result
    [B, c, h, w] on the host and the whole poisoned output buffer with the mask of the floats the op owns."""
    from bts_amd import ops
    B, c, h, w = x.shape
    npix = B * h * w
    xbuf = torch.full((npix, c + PAD), 7.0e4, device="cuda")
    xbuf[:, OFF:OFF + c] = x.permute(0, 2, 3, 1).reshape(npix, c).cuda()
    flat = torch.full((2 * GUARD + npix * (c + PAD),), POISON, device="cuda")
    ybuf = flat[GUARD:GUARD + npix * (c + PAD)].view(npix, c + PAD)
    y2d = ybuf[:, OFF:OFF + c]
    wp = ops.pack_grouped_native_bf16(wt.cuda(), groups)
    e1d = None if e1 is None else (e1[0].cuda(), e1[1].cuda())
    ops.set_trace(trace)
    try:
        kw = {} if tag is None else dict(tag=tag)
        ops.conv_grouped_bf16_forward(xbuf[:, OFF:OFF + c], B, h, w, wp, c, groups, e1=e1d, act=ACTS[act], y2d=y2d, **kw)
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    owned = torch.zeros_like(flat, dtype=torch.bool)
    owned[GUARD:GUARD + npix * (c + PAD)].view(npix, c + PAD)[:, OFF:OFF + c] = True
    return y2d.view(B, h, w, c).permute(0, 3, 1, 2).cpu().contiguous(), flat, owned


def _run_fp32_native(x, wt, groups, e1, act):
    """The fp32 native kernel (ops.conv_grouped_forward) on the same operands."""
    from bts_amd import ops
    B, c, h, w = x.shape
    x2d = x.cuda().permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous()
    y = ops.conv_grouped_forward(x2d, B, h, w, ops.pack_grouped_native(wt.cuda(), groups), c, groups,
                                 e1=(e1[0].cuda(), e1[1].cuda()), act=ACTS[act])
    return y.view(B, h, w, c).permute(0, 3, 1, 2).cpu().contiguous()


def _run_bundles_bf16(x, wt, groups, e1, act):
    """The bundle path (ops.conv_forward with n_bundles) under precision bf16 on the same operands: the parent's path."""
    from bts_amd import ops
    B, c, h, w = x.shape
    x2d = x.cuda().permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous()
    wp, nb, cb = ops.pack_grouped_conv_weight(wt.cuda(), groups)
    y = torch.empty(B * h * w, c, device="cuda")
    with ops.launch_config(fill_frames=16, precision="bf16"):
        ops.conv_forward(x2d, B, h, w, wp, cb, 3, pad=1, c_in_ld=cb, e1=(e1[0].cuda(), e1[1].cuda()), act=ACTS[act], y2d=y,
                         n_bundles=nb, c_in_real=c // groups)
    return y.view(B, h, w, c).permute(0, 3, 1, 2).cpu().contiguous()


@pytest.mark.parametrize("B,h,w,c,groups,act", EXACT_CASES, ids=lambda v: str(v))
def test_exact_integer_cases(B, h, w, c, groups, act):
    """Integer x (|x| <= 127: exact in bf16), weights in {-1, 0, 1}, e1 scale in {0.5, 1, 2}, integer shift (|.| <= 8): a sum
    is at most 9 * 16 * 127 and every value a multiple of 0.5 below 2^24, so the kernel must reproduce the fp64 reference bit
    for bit -- x read from a wider buffer, y written into a channel slice of a poisoned buffer whose other floats (guard bands
    included) keep the poison, and frame by frame independent of B."""
    g = torch.Generator().manual_seed(1000 * h + 10 * w + groups)
    cg = c // groups
    x = torch.randint(-127, 128, (B, c, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (c, cg, 3, 3), generator=g).float()
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g)]
    shift = torch.randint(-8, 9, (c,), generator=g).float()
    assert 2 * (9 * 16 * 127 * 2 + 8) < 2 ** 24
    assert torch.equal(x.to(torch.bfloat16).float(), x)
    ref = _reference(x, wt, groups, (scale, shift), act).float()
    got, flat, owned = _run_native(x, wt, groups, (scale, shift), act)
    assert torch.equal(got, ref), "max |diff| %g" % float((got - ref).abs().max())
    assert bool((flat[~owned] == POISON).all())
    if B > 1:
        one, _, _ = _run_native(x[B - 1:], wt, groups, (scale, shift), act)
        assert torch.equal(one[0], got[B - 1])


def test_every_odd_integer_in_257_511_is_a_tie_that_truncation_gets_wrong_half_the_time():
    """The premise of the rounding test, on the CPU: Tensor.to(torch.bfloat16) sends each of the 128 odd integers to the
    neighbouring multiple of 4 (ties to even), and dropping the low 16 bits differs on half of them."""
    v = torch.arange(257, 512, 2).float()
    r = v.to(torch.bfloat16).float()
    assert v.numel() == 128 and bool(((r - v).abs() == 1).all()) and bool((r % 4 == 0).all())
    trunc = (v.view(torch.int32) & -65536).view(torch.float32)
    assert int((trunc != r).sum()) == 64


@pytest.mark.parametrize("B,h,w,c,groups", [(1, 9, 19, 64, 16), (2, 7, 33, 128, 16), (1, 11, 17, 64, 4)], ids=lambda v: str(v))
def test_input_rounding_is_nearest_even_not_truncation(B, h, w, c, groups):
    """x takes odd integers in [257, 511]: every one is a bf16 tie.  Weights in {-1, 0, 1}; sums <= 144 * 512 < 2^24, so the
    result is bit-equal to the fp64 convolution of x.to(bfloat16) -- and not to that of the unrounded x."""
    g = torch.Generator().manual_seed(7 * c + groups)
    cg = c // groups
    x = (2 * torch.randint(128, 256, (B, c, h, w), generator=g) + 1).float()
    assert int(x.min()) >= 257 and int(x.max()) <= 511 and 144 * 512 < 2 ** 24
    wt = torch.randint(-1, 2, (c, cg, 3, 3), generator=g).float()
    got, _, _ = _run_native(x, wt, groups, None, "none")
    ref_rounded = F.conv2d(_rne(x), wt.double(), padding=1, groups=groups).float()
    ref_plain = _reference(x, wt, groups, None, "none").float()
    assert not torch.equal(ref_rounded, ref_plain)
    assert torch.equal(got, ref_rounded), "max |diff| %g" % float((got - ref_rounded).abs().max())
    assert not torch.equal(got, ref_plain)


@pytest.mark.parametrize("cg", [4, 8, 16])
def test_one_hot_input_channel_reaches_its_own_group_only(cg):
    c, h, w, ch = 128, 9, 20, 77
    groups = c // cg
    g = torch.Generator().manual_seed(cg)
    x = torch.zeros((1, c, h, w))
    x[0, ch] = torch.randint(1, 9, (h, w), generator=g).float()
    wt = torch.randint(1, 4, (c, cg, 3, 3), generator=g).float()          # no zero weight: every in-group output is hit
    got, _, _ = _run_native(x, wt, groups, None, "none")
    lo = ch // cg * cg
    inside = torch.zeros(c, dtype=torch.bool)
    inside[lo:lo + cg] = True
    assert bool((got[0, ~inside] == 0).all())
    assert bool((got[0, inside] != 0).all())
    assert torch.equal(got, _reference(x, wt, groups, None, "none").float())


def test_one_infinite_value_stays_in_its_block_and_neighbourhood():
    """cg 16: +inf at one interior pixel and channel.  Outputs of every other 16-channel block, and outputs outside the 3x3
    neighbourhood, are bit-identical to the run without it."""
    B, c, groups, h, w, py, px, ch = 1, 128, 8, 12, 21, 5, 17, 37
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, c, h, w), generator=g)
    wt = torch.randn((c, 16, 3, 3), generator=g) / 12.0
    clean, _, _ = _run_native(x, wt, groups, None, "none")
    x[0, ch, py, px] = float("inf")
    got, _, _ = _run_native(x, wt, groups, None, "none")
    hit = torch.zeros((B, c, h, w), dtype=torch.bool)
    hit[:, ch // 16 * 16:ch // 16 * 16 + 16, py - 1:py + 2, px - 1:px + 2] = True
    assert bool(torch.isfinite(clean).all())
    assert torch.equal(got[~hit], clean[~hit])
    assert not bool(torch.isfinite(got[hit]).any())                        # randn weights: no zero, the value arrived everywhere


def _float_case(B, h, w, c, groups, xscale=1.0, wscale=1.0):
    """randn operands scaled by 1 / sqrt(9 cg), BN + ReLU: (x, wt, e1, reference, bound), the reference the fp64 convolution
    of the RNE-rounded operands and the bound tests/test_bf16_gpu.py::test_bf16_conv_is_exact_on_rounded_operands' per
    output: 2e-6 * sum|terms| + 2^-22 |ref| (the e1 scale multiplies the terms)."""
    cg = c // groups
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn((B, c, h, w), generator=g) * xscale
    wt = torch.randn((c, cg, 3, 3), generator=g) / np.sqrt(9.0 * cg) * wscale
    e1 = (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1)
    xr, wr = _rne(x), _rne(wt)
    ref = _affine_act(F.conv2d(xr, wr, padding=1, groups=groups), e1, "relu")
    mag = F.conv2d(xr.abs(), wr.abs(), padding=1, groups=groups) * e1[0].double().abs().view(1, -1, 1, 1)
    mag = mag + e1[1].double().abs().view(1, -1, 1, 1)
    return x, wt, e1, ref, 2e-6 * mag + 2.0 ** -22 * ref.abs()


@pytest.mark.parametrize("B,h,w,c,groups", [(2, 26, 34, 512, 32), (1, 52, 68, 256, 32)])
def test_float_is_exact_on_rounded_operands(B, h, w, c, groups):
    """Within the bf16 mode's bound of the fp64 convolution of the rounded operands, and so is the bundle path of that mode on
    the same operands (both errors printed); the fp32 native kernel misses that reference by more than 10x the bound
    somewhere (control: the bound tells the arithmetics apart); the trace names the kernel, the tag and the algorithmic flops."""
    from bts_amd import ops
    cg = c // groups
    x, wt, e1, ref, bound = _float_case(B, h, w, c, groups)
    tr = ops.KernelTrace()
    got, _, _ = _run_native(x, wt, groups, e1, "relu", trace=tr, tag="enc_l2_g3x3")
    summ = tr.summary()
    assert sorted(summ) == [_kernel(cg)] and set(summ[_kernel(cg)]["tags"]) == {"enc_l2_g3x3"}
    assert summ[_kernel(cg)]["flops"] == 2.0 * B * h * w * c * cg * 9
    floor = bound.clamp_min(1e-300)
    err = (got.double() - ref).abs()
    err_bundles = (_run_bundles_bf16(x, wt, groups, e1, "relu").double() - ref).abs()
    err_fp32 = (_run_fp32_native(x, wt, groups, e1, "relu").double() - ref).abs()
    worst, worst_bundles, worst_fp32 = (float((e / floor).max()) for e in (err, err_bundles, err_fp32))
    print((B, h, w, c, groups), "worst err / bound: bf16 native %.3g, bf16 bundles %.3g, fp32 native %.3g" % (worst, worst_bundles, worst_fp32))
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bound).all()), worst
    assert bool((err_bundles <= bound).all()), worst_bundles
    assert worst_fp32 > 10.0, worst_fp32


def test_float_range_2_to_the_40():
    """Activations x 2^40 with weights x 2^-40 (bf16 keeps fp32's exponent range): finite and within the same bound."""
    B, h, w, c, groups = 1, 26, 34, 256, 32
    x, wt, e1, ref, bound = _float_case(B, h, w, c, groups, xscale=2.0 ** 40, wscale=2.0 ** -40)
    got, _, _ = _run_native(x, wt, groups, e1, "relu")
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------------- encoders and model
def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.empty_like(m.weight).uniform_(0.8, 1.2, generator=g)
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.05
            m.running_mean = torch.randn(m.running_mean.shape, generator=g) * 0.05
            m.running_var = torch.empty_like(m.running_var).uniform_(0.8, 1.2, generator=g)


def _g3x3_launches(summary):
    """(new-kernel launches, fp32-native launches, bundle launches) under the *_g3x3 tags of a KernelTrace summary."""
    new = fp32 = bundles = 0
    for kern, d in summary.items():
        n = sum(tg["launches"] for tag, tg in d["tags"].items() if tag.endswith("_g3x3"))
        if kern.startswith("conv_grouped_bf16_kernel"):
            assert n == d["launches"], kern                               # the new kernel runs under no other tag
            new += n
        elif kern.startswith("conv_grouped_kernel"):
            fp32 += n
        else:
            bundles += n
    return new, fp32, bundles


def _traced(fn):
    from bts_amd import ops
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        with torch.no_grad():
            got = fn()
    finally:
        ops.set_trace(None)
    return got, tr.summary()


# One conv of the bf16 mode rounds both operands to 8 significant bits: 2^-9 relative per operand, about 2^-9 of the output
# scale per layer once the K >= 36 products of random sign are summed; the errors of L layers in sequence add in quadrature,
# and the deepest tap of ResNeXt-101 lies behind about 100 of them: 2e-3 * 10 = 2e-2 of max|tap|, the order of the 3e-2
# tests/test_bf16_gpu.py allows final_depth for the same encoder.  The taps are held at that 3e-2 of max|tap|.
TAP_BAR = 3e-2


@pytest.mark.parametrize("enc,shape,n_native,n_blocks", [("resnext50_bts", (1, 96, 64), 11, 16), ("resnext101_bts", (2, 64, 96), 6, 33)])
def test_resnext_taps_bf16_native_vs_torch_cpu(enc, shape, n_native, n_blocks):
    """The encoders under launch precision bf16 with grouped_conv_bf16 = "native" against the same nn modules in fp32 on the
    CPU: the new kernel runs exactly the stride-1 blocks with <= 16 channels per group, every other grouped launch stays on
    the bundle kernel, "bundles" issues none, and grouped_conv = "native" at the same time issues no fp32-native launch; under
    fp32 the switch issues none either."""
    from bts_amd import bts as M
    from bts_amd import ops
    from bts_amd.encoder_hip import ResNetHip
    torch.manual_seed(3)
    e = M.encoder(Params(enc, 512, 80.0, "kitti")).eval()
    _randomise_bn(e, 5)
    B, H, W = shape
    x = torch.from_numpy(synth.image_batch(B, H, W, 21))
    with torch.no_grad():
        ref = e(x)
    eg = M.encoder(Params(enc, 512, 80.0, "kitti")).eval()
    eg.load_state_dict(e.state_dict())
    eg = eg.cuda()
    plan = ResNetHip(eg.base_model)
    assert plan.grouped_conv_bf16 == "bundles"

    def run(mode, prec="bf16", fp32_mode="bundles"):
        plan.grouped_conv_bf16, plan.grouped_conv = mode, fp32_mode
        with ops.launch_config(precision=prec):
            return _traced(lambda: plan.taps_nchw(x.cuda()))

    base, summ = run("bundles")
    assert _g3x3_launches(summ) == (0, 0, n_blocks)
    got, summ = run("native")
    assert _g3x3_launches(summ) == (n_native, 0, n_blocks - n_native)
    both, summ = run("native", fp32_mode="native")
    assert _g3x3_launches(summ) == (n_native, 0, n_blocks - n_native)
    assert all(torch.equal(a, b) for a, b in zip(got, both))
    _, summ = run("native", prec="fp32")
    assert _g3x3_launches(summ) == (0, 0, n_blocks)
    _, summ = run("native", prec="bf16x3")
    assert _g3x3_launches(summ) == (0, 0, n_blocks)
    assert len(got) == len(ref) == 6
    for i in range(1, 6):
        r, g, b = ref[i], got[i].cpu(), base[i].cpu()
        assert r.shape == g.shape
        scale = r.abs().max().item()
        err, err_base = (r - g).abs().max().item(), (r - b).abs().max().item()
        print(enc, "tap %d: max abs err / max|ref|: native %.3g, bundles %.3g" % (i, err / scale, err_base / scale))
        assert err <= TAP_BAR * scale, "tap %d: max abs err %g (scale %g)" % (i, err, scale)
    plan.grouped_conv_bf16, plan.grouped_conv = "sometimes", "bundles"
    with ops.launch_config(precision="bf16"):
        with pytest.raises(ops.BtsHipError, match="grouped_conv_bf16"):
            plan.taps_nchw(x.cuda())


@functools.lru_cache(maxsize=None)
def _model():
    """tests/test_bf16_gpu.py's recipe for resnext101_bts / nyu at 2 x 64 x 96: the CPU fp32 model's oracle outputs and a GPU
    copy."""
    from bts_amd import bts as M
    params = Params("resnext101_bts", 512, 10.0, "nyu")
    torch.manual_seed(11)
    model = M.BtsModel(params).eval()
    _randomise_bn(model.encoder, 7)
    state_np = synth.decoder_state(synth.ENCODER_CHANNELS[params.encoder], 512, 0)
    model.decoder.load_state_dict({k: (torch.tensor(v) if np.ndim(v) == 0 else t(v)) for k, v in state_np.items()})
    x = torch.from_numpy(synth.image_batch(2, 64, 96, 5))
    f = torch.from_numpy(synth.focal_values(2, params.dataset, 5))
    with torch.no_grad():
        ref_outs, inter = O.decoder_forward(O.state_from_numpy(state_np), model.encoder(x), f, params.max_depth, params.dataset,
                                            want_intermediates=True)
    mg = M.BtsModel(params).eval()
    mg.load_state_dict(model.state_dict())
    return mg.cuda(), x.cuda(), f.cuda(), ref_outs, inter


def _forward(m, x, f, mode, prec="bf16"):
    m.grouped_conv_bf16, m.conv_precision = mode, prec
    try:
        with torch.no_grad():
            return [o.clone() for o in m(x, f)]
    finally:
        m.grouped_conv_bf16, m.conv_precision = "bundles", "fp32"


def _depth_stats(got, ref_outs, inter):
    B, _, H, W = ref_outs[0].shape
    masks = singular_masks(inter, B, H, W)
    rep = {}
    for i, k in ((0, 8), (1, 4), (2, 2), (3, None), (4, None)):
        g = got[i].detach().cpu().double().numpy()
        r = ref_outs[i].double().numpy()
        m = masks[k] if k else np.ones_like(r, dtype=bool)
        rel = np.abs(g[m] - r[m]) / np.maximum(np.abs(r[m]), 1e-30)
        rep[OUT_NAMES[i]] = (float(np.median(rel)), float(rel.max()))
    return rep


def test_btsmodel_resnext101_bf16_native_grouped_vs_cpu():
    """BtsModel(resnext101_bts, nyu) under conv_precision bf16 with grouped_conv_bf16 = "native" at the whole-model bars of
    tests/test_bf16_gpu.py; two forwards give the same bits and the sub-batched first forward (which packs the weights, its
    sub-batches on their own streams) equals the sub_batches = 1 forward; use_plans refuses the launch by name; under fp32 the
    switch changes no bit and issues no launch of the new kernel."""
    from bts_amd import ops
    m, x, f, ref_outs, inter = _model()
    assert m.grouped_conv_bf16 == "bundles"
    subs = m.sub_batches
    try:
        first = _forward(m, x, f, "native")
        second = _forward(m, x, f, "native")
        m.sub_batches = 1
        whole, summ = _traced(lambda: _forward(m, x, f, "native"))
        assert _g3x3_launches(summ) == (6, 0, 27)
        for i in range(6):
            assert torch.equal(first[i], second[i]) and torch.equal(first[i], whole[i]), i
        _, summ = _traced(lambda: _forward(m, x, f, "bundles"))
        assert _g3x3_launches(summ) == (0, 0, 33)
        rep = _depth_stats(whole, ref_outs, inter)
        print("resnext101 bf16 + native grouped:", rep, "bundles:", _depth_stats(_forward(m, x, f, "bundles"), ref_outs, inter))
        for name in OUT_NAMES[:5]:
            med, mx = rep[name]
            assert med <= 1.5e-2 and mx <= 1e-1, (name, med, mx)
        assert rep["final_depth"][1] <= 3e-2, rep["final_depth"]
        fp32_off = _forward(m, x, f, "bundles", "fp32")
        fp32_on, summ = _traced(lambda: _forward(m, x, f, "native", "fp32"))
        assert _g3x3_launches(summ) == (0, 0, 33)
        for i in range(6):
            assert torch.equal(fp32_off[i], fp32_on[i]), i
        assert not torch.equal(fp32_off[5], whole[5])
        m.use_plans = True
        try:
            with pytest.raises(ops.BtsHipError, match="bts_conv_grouped_bf16_fwd_f32"):
                _forward(m, x, f, "native")
        finally:
            m.use_plans = False
    finally:
        m.sub_batches = subs


def test_graphs_key_on_the_switch():
    """GraphedModel: flipping the switch adds one capture; flipping back adds none and replays the first capture's bits."""
    from bts_amd.graph import GraphedModel
    m, x, f, _, _ = _model()
    eager = {mode: _forward(m, x, f, mode) for mode in ("bundles", "native")}
    gm = GraphedModel(m)
    try:
        for n, mode in enumerate(("bundles", "native", "bundles", "native")):
            m.grouped_conv_bf16, m.conv_precision = mode, "bf16"
            with torch.no_grad():
                got = [o.clone() for o in gm(x, f)]
            torch.cuda.synchronize()
            assert gm.captures == min(n + 1, 2), (n, mode, gm.captures)
            for i in range(6):
                assert torch.equal(got[i], eager[mode][i]), ("graph", mode, i)
    finally:
        m.grouped_conv_bf16, m.conv_precision = "bundles", "fp32"
