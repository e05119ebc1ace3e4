"""GPU: the native grouped 3x3 kernel (csrc/conv_grouped.inc, ops.conv_grouped_forward) -- exact integer cases against fp64
F.conv2d(groups=) inside poisoned buffers, group leakage, confinement of a non-finite value, float cases beside the bundle
path, and the ResNeXt encoders / BtsModel with ``grouped_conv`` set."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bts_amd import synth
from parity_util import Params, check_outputs

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 1}
PAD, OFF = 8, 4                 # both views are 8 floats wider than c and start at column 4
GUARD = 64                      # floats in front of and behind the output rows
POISON = -12345.0


def _kernel(cg):
    return "conv_grouped_kernel<%d>" % cg


def _reference(x, wt, groups, e1, act):
    """fp64 grouped conv3x3 -> e1 affine -> activation, [B, c, h, w]."""
    ref = F.conv2d(x.double(), wt.double(), padding=1, groups=groups)
    if e1 is not None:
        ref = ref * e1[0].double().view(1, -1, 1, 1) + e1[1].double().view(1, -1, 1, 1)
    return torch.relu(ref) if act == "relu" else ref


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
    wp = ops.pack_grouped_native(wt.cuda(), groups)
    e1d = None if e1 is None else (e1[0].cuda(), e1[1].cuda())
    ops.set_trace(trace)
    try:
        kw = {} if tag is None else dict(tag=tag)
        ops.conv_grouped_forward(xbuf[:, OFF:OFF + c], B, h, w, wp, c, groups, e1=e1d, act=ACTS[act], y2d=y2d, **kw)
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    owned = torch.zeros_like(flat, dtype=torch.bool)
    owned[GUARD:GUARD + npix * (c + PAD)].view(npix, c + PAD)[:, OFF:OFF + c] = True
    return y2d.view(B, h, w, c).permute(0, 3, 1, 2).cpu().contiguous(), flat, owned


def _run_bundles(x, wt, groups, e1, act):
    """The bundle path (ops.conv_forward with n_bundles) on the same operands."""
    from bts_amd import ops
    B, c, h, w = x.shape
    x2d = x.cuda().permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous()
    wp, nb, cb = ops.pack_grouped_conv_weight(wt.cuda(), groups)
    y = torch.empty(B * h * w, c, device="cuda")
    with ops.launch_config(fill_frames=16, precision="fp32"):
        ops.conv_forward(x2d, B, h, w, wp, cb, 3, pad=1, c_in_ld=cb, e1=(e1[0].cuda(), e1[1].cuda()), act=ACTS[act], y2d=y,
                         n_bundles=nb, c_in_real=c // groups)
    return y.view(B, h, w, c).permute(0, 3, 1, 2).cpu().contiguous()


EXACT_CASES = [
    # B, h, w, c, groups, act
    (1, 16, 32, 64, 4, "relu"),       # whole tiles for any 4x32 / 8x16 / 16x8 tile
    (1, 3, 5, 64, 8, "none"),         # smaller than a tile
    (2, 7, 33, 128, 8, "relu"),       # ragged both ways
    (3, 17, 9, 128, 32, "none"),
    (2, 9, 17, 192, 48, "relu"),      # 4 channels per group, three slabs
    (1, 1, 1, 64, 16, "none"),
    (3, 35, 250, 256, 16, "relu"),    # 240 tiles on the 128 persistent workgroups of a slab: two each for most, ragged
]


@pytest.mark.parametrize("B,h,w,c,groups,act", EXACT_CASES, ids=lambda v: str(v))
def test_exact_integer_cases(B, h, w, c, groups, act):
    """Integer x (|x| <= 127), weights in {-1, 0, 1}, e1 scale in {0.5, 1, 2}, integer shift (|.| <= 8): a sum is at most
    9 * 16 * 127 and every value a multiple of 0.5 below 2^24, so the kernel must reproduce the fp64 reference bit for bit --
    x read from a wider buffer, y written into a channel slice of a poisoned buffer whose other floats (guard bands
    included) keep the poison, and frame by frame independent of B."""
    g = torch.Generator().manual_seed(1000 * h + 10 * w + groups)
    cg = c // groups
    x = torch.randint(-127, 128, (B, c, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (c, cg, 3, 3), generator=g).float()
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=g)]
    shift = torch.randint(-8, 9, (c,), generator=g).float()
    assert 2 * (9 * 16 * 127 * 2 + 8) < 2 ** 24
    ref = _reference(x, wt, groups, (scale, shift), act).float()
    got, flat, owned = _run_native(x, wt, groups, (scale, shift), act)
    assert torch.equal(got, ref), "max |diff| %g" % float((got - ref).abs().max())
    assert bool((flat[~owned] == POISON).all())
    if B > 1:
        one, _, _ = _run_native(x[B - 1:], wt, groups, (scale, shift), act)
        assert torch.equal(one[0], got[B - 1])


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


def test_one_infinite_value_stays_in_its_group_and_neighbourhood():
    """cg 16: +inf at one interior pixel and channel.  Outputs of every other group, and outputs outside the 3x3
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


@pytest.mark.parametrize("B,h,w,c,groups", [(2, 26, 34, 512, 32), (1, 52, 68, 256, 32)])
def test_float_vs_fp64_beside_the_bundle_path(B, h, w, c, groups):
    """randn operands scaled by 1 / sqrt(9 cg), BN + ReLU: error against fp64 within the bar
    test_grouped_conv_bundles_and_residual_vs_torch sets for these layers (2e-5 of max|ref|), the bundle path's error on
    the same operands printed beside it; the trace names the kernel, the tag and the algorithmic flops."""
    from bts_amd import ops
    cg = c // groups
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn((B, c, h, w), generator=g)
    wt = torch.randn((c, cg, 3, 3), generator=g) / np.sqrt(9.0 * cg)
    e1 = (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1)
    ref = _reference(x, wt, groups, e1, "relu")
    tr = ops.KernelTrace()
    got, _, _ = _run_native(x, wt, groups, e1, "relu", trace=tr, tag="enc_l2_g3x3")
    summ = tr.summary()
    assert sorted(summ) == [_kernel(cg)] and set(summ[_kernel(cg)]["tags"]) == {"enc_l2_g3x3"}
    assert summ[_kernel(cg)]["flops"] == 2.0 * B * h * w * c * cg * 9
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item() / scale
    err_bundles = (_run_bundles(x, wt, groups, e1, "relu").double() - ref).abs().max().item() / scale
    print((B, h, w, c, groups), "max error / max|ref|: native %.3g, bundles %.3g" % (err, err_bundles))
    assert err <= 2e-5, err


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.empty_like(m.weight).uniform_(0.8, 1.2, generator=g)
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.05
            m.running_mean = torch.randn(m.running_mean.shape, generator=g) * 0.05
            m.running_var = torch.empty_like(m.running_var).uniform_(0.8, 1.2, generator=g)


def _g3x3_launches(summary):
    """(native launches, bundle launches) under the *_g3x3 tags of a KernelTrace summary."""
    native = bundles = 0
    for kern, d in summary.items():
        n = sum(t["launches"] for tag, t in d["tags"].items() if tag.endswith("_g3x3"))
        if kern.startswith("conv_grouped_kernel"):
            assert n == d["launches"], kern                               # the native kernel runs under no other tag
            native += n
        else:
            bundles += n
    return native, bundles


@pytest.mark.parametrize("enc,shape,n_native,n_blocks", [("resnext50_bts", (1, 96, 64), 11, 16), ("resnext101_bts", (2, 64, 96), 6, 33)])
def test_resnext_taps_native_vs_torch_cpu(enc, shape, n_native, n_blocks):
    """The encoders with grouped_conv = "native" against the same nn modules on the CPU, by the rule of
    test_resnet_hip_taps_vs_torch_cpu; the native kernel runs exactly the stride-1 blocks with <= 16 channels per group and
    every other grouped launch stays on the bundle kernel; the default mode issues no native launch."""
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

    def run(mode):
        plan.grouped_conv = mode
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            with torch.no_grad():
                got = plan.taps_nchw(x.cuda())
        finally:
            ops.set_trace(None)
        return got, tr.summary()

    assert plan.grouped_conv == "bundles"
    _, summ = run("bundles")
    assert _g3x3_launches(summ) == (0, n_blocks)
    got, summ = run("native")
    assert _g3x3_launches(summ) == (n_native, n_blocks - n_native)
    assert len(got) == len(ref) == 6
    for i in range(1, 6):
        r, g = ref[i], got[i].cpu()
        assert r.shape == g.shape
        scale = r.abs().max().item()
        err = (r - g).abs().max().item()
        assert err <= 3e-4 * scale + 1e-5, "tap %d: max abs err %g (scale %g)" % (i, err, scale)
    plan.grouped_conv = "sometimes"
    with pytest.raises(ops.BtsHipError, match="grouped_conv"):
        plan.taps_nchw(x.cuda())


def test_btsmodel_resnext101_native_grouped_vs_cpu():
    """BtsModel(resnext101_bts, nyu) with grouped_conv = "native" == CPU torch encoder + oracle at the tolerance of
    test_btsmodel_resnext101_fused_forward_vs_cpu; with use_plans the recorder refuses the launch by name; with
    conv_precision "bf16" the forward runs and issues no native launch."""
    from bts_amd import bts as M
    from bts_amd import ops
    from oracle import bts_oracle as O
    params = Params("resnext101_bts", 512, 10.0, "nyu")
    torch.manual_seed(12)
    model = M.BtsModel(params).eval()
    _randomise_bn(model.encoder, 8)
    feat = synth.ENCODER_CHANNELS[params.encoder]
    state_np = synth.decoder_state(feat, 512, 0)
    model.decoder.load_state_dict({k: (torch.tensor(v) if np.ndim(v) == 0 else torch.from_numpy(v.copy())) for k, v in state_np.items()})
    B, H, W = 2, 64, 96
    x = torch.from_numpy(synth.image_batch(B, H, W, 6))
    focal = torch.from_numpy(synth.focal_values(B, "nyu", 6))
    with torch.no_grad():
        ref_outs, inter = O.decoder_forward(O.state_from_numpy(state_np), model.encoder(x), focal, 10.0, "nyu",
                                            want_intermediates=True)
    mg = M.BtsModel(params).eval()
    mg.load_state_dict(model.state_dict())
    mg = mg.cuda()
    assert mg.grouped_conv == "bundles"
    mg.grouped_conv = "native"
    with torch.no_grad():           # the first native forward packs the weights, with the sub-batches on their own streams
        first = [o.clone() for o in mg(x.cuda(), focal.cuda())]
    mg.sub_batches = 1              # one forward of the whole batch: launch counts are per network

    def run():
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            with torch.no_grad():
                got = mg(x.cuda(), focal.cuda())
        finally:
            ops.set_trace(None)
        return got, tr.summary()

    got, summ = run()
    assert _g3x3_launches(summ) == (6, 27)
    assert all(torch.equal(a, b) for a, b in zip(first, got))              # frames are independent: the same bits either way
    rep = check_outputs(got, ref_outs, inter, rel_tol=5e-4, what="ResNeXt101 BtsModel, native grouped conv")
    print("native grouped ResNeXt101 model max-rel:", rep)
    mg.use_plans = True
    with pytest.raises(ops.BtsHipError, match="bts_conv_grouped_fwd_f32"):
        with torch.no_grad():
            mg(x.cuda(), focal.cuda())
    mg.use_plans = False
    mg.conv_precision = "bf16"
    got_bf16, summ = run()
    assert _g3x3_launches(summ)[0] == 0 and _g3x3_launches(summ)[1] > 0
    assert all(bool(torch.isfinite(o).all()) for o in got_bf16)
