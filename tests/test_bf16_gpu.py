"""GPU: the bf16 inference mode (bts_conv_desc.precision = 2, ``conv_precision = "bf16"``): both contraction operands
rounded to bf16 (nearest, ties to even), exact bf16 products, fp32 accumulation, fp32 epilogue."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bts_amd import synth
from oracle import bts_oracle as O
from parity_util import OUT_NAMES, Params, build_hip_decoder, hip_run, oracle_run, singular_masks, t

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("BTS_CONV_PRECISION", "0").strip() == "1",
                                 reason="BTS_CONV_PRECISION=1 forces precision 1 inside every scope")]


def _rne(v: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 (round to nearest even) -> fp64: the operand the mode contracts."""
    return v.float().to(torch.bfloat16).double()


def _traced(fn):
    from bts_amd import ops
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        fn()
    finally:
        ops.set_trace(None)
    return sorted(tr.summary())


def _unpack_subpixel(wp, cout, cin):
    """pack_upconv_subpixel's [4][c_out_pad][k_pad] -> four [cout, cin, 2, 2] kernels (class = 2*py + px)."""
    return [wp[c, :cout, :4 * cin].reshape(cout, 2, 2, cin).permute(0, 3, 1, 2) for c in range(4)]


def _subpixel_conv(x, ws):
    """The sub-pixel upconv in fp64 from its four 2x2 class kernels: output (2Y+py, 2X+px) reads source rows
    Y-1+py .. Y+py and columns X-1+px .. X+px."""
    B, _, h, w = x.shape
    out = torch.zeros((B, ws[0].shape[0], 2 * h, 2 * w), dtype=x.dtype)
    for c in range(4):
        py, px = c >> 1, c & 1
        xp = F.pad(x, (1 - px, px, 1 - py, py))
        out[:, :, py::2, px::2] = F.conv2d(xp, ws[c])
    return out


# name: (B, cin, cout, h, w, k, stride, dil, options, expected kernel)
CASES = {
    "1x1": (2, 256, 128, 22, 38, 1, 1, 1, {}, "row"),
    "3x3": (2, 128, 128, 44, 152, 3, 1, 1, {"act": "elu"}, "halo"),
    "3x3_prologue": (2, 64, 128, 44, 152, 3, 1, 1, {"pre": True}, "halo"),
    "1x1_prologue": (2, 96, 64, 22, 38, 1, 1, 1, {"pre": True}, "row"),
    "stride2": (2, 64, 128, 44, 76, 3, 2, 1, {}, "row"),
    "dil3": (1, 128, 128, 22, 76, 3, 1, 3, {}, "row"),
    "dil6": (1, 128, 128, 22, 76, 3, 1, 6, {}, "row"),
    "dil24": (1, 128, 128, 44, 76, 3, 1, 24, {}, "row"),
    "subpixel128": (2, 128, 128, 22, 152, 3, 1, 1, {"sub": True, "act": "elu"}, "halo"),
    "subpixel64": (1, 256, 64, 22, 152, 3, 1, 1, {"sub": True}, "halo"),
    "grouped": (2, 256, 256, 22, 38, 3, 1, 1, {"groups": 32}, "row"),
    "splitk": (1, 1024, 128, 11, 38, 3, 1, 1, {"splitk": True, "fill": 2}, "row_splitk"),
    "nchw": (2, 64, 32, 22, 38, 3, 1, 1, {"nchw": True}, "row"),
    "residual": (2, 128, 128, 22, 38, 1, 1, 1, {"res": True, "act": "relu"}, "row"),
    "cout48_halo": (1, 192, 48, 88, 152, 3, 1, 1, {"pre": True}, "halo"),
    "cout48_1x1": (2, 96, 48, 22, 38, 1, 1, 1, {}, "row"),
    "dynamic_range": (1, 256, 64, 12, 16, 3, 1, 1, {"dyn": True}, "row"),
    "dynamic_range_halo": (1, 256, 64, 44, 152, 3, 1, 1, {"dyn": True}, "halo"),
    "scale_2^40": (1, 128, 128, 44, 152, 3, 1, 1, {"xscale": 2.0 ** 40, "wscale": 2.0 ** -40}, "halo"),
    "scale_2^40_row": (2, 256, 128, 22, 38, 1, 1, 1, {"xscale": 2.0 ** 40, "wscale": 2.0 ** -40}, "row"),
}


def _run_case(name, precision="bf16", binding=None):
    from bts_amd import ops
    B, cin, cout, h, w, k, stride, dil, o, _ = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    groups = o.get("groups", 1)
    cing = cin // groups
    x = torch.randn((B, cin, h, w), generator=g) * o.get("xscale", 1.0)
    wt = torch.randn((cout, cing, k, k), generator=g) / np.sqrt(cing * k * k) * o.get("wscale", 1.0)
    if o.get("dyn"):       # test_conv_bf16x3_wide_dynamic_range's ranges: activations over ten decades, weights over six
        x = torch.randn((B, cin, h, w), generator=g) * torch.pow(10.0, torch.empty(B, cin, 1, 1).uniform_(-6, 4, generator=g))
        wt = torch.randn((cout, cin, k, k), generator=g) * torch.pow(10.0, torch.empty(cout, 1, 1, 1).uniform_(-4, 2, generator=g))
    pre = o.get("pre", False)
    ps, pb = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.1
    sub = o.get("sub", False)
    pad = dil * (k // 2)
    if sub:
        H, W = 2 * h, 2 * w
    else:
        H, W = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res = torch.randn((B, cout, H, W), generator=g) if o.get("res") else None
    act = {"elu": ops.ACT_ELU, "relu": ops.ACT_RELU}.get(o.get("act"), ops.ACT_NONE)

    # the conv input after the fp32 prologue (one rounding, as the kernel's fma) and the weights in their packed form
    xin = (x.double() * ps.double().view(1, -1, 1, 1) + pb.double().view(1, -1, 1, 1)).float().relu() if pre else x
    xr = _rne(xin)
    dev_w = wt.cuda()
    if sub:
        wp = ops.pack_upconv_subpixel(dev_w)[0]
        wr = [_rne(c) for c in _unpack_subpixel(wp.cpu(), cout, cin)]
        ref = _subpixel_conv(xr, wr)
        mag = _subpixel_conv(xr.abs(), [c.abs() for c in wr])
    else:
        wr = _rne(wt)
        ref = F.conv2d(xr, wr, stride=stride, padding=pad, dilation=dil, groups=groups)
        mag = F.conv2d(xr.abs(), wr.abs(), stride=stride, padding=pad, dilation=dil, groups=groups)
    if res is not None:
        ref = ref + res.double()
    ref = {ops.ACT_ELU: F.elu, ops.ACT_RELU: F.relu}.get(act, lambda v: v)(ref)

    x2d = x.permute(0, 2, 3, 1).reshape(B * h * w, cin).contiguous().cuda()
    kw = dict(act=act, dil=dil, stride=stride, pad=pad)
    if groups > 1:
        wp, nb, cb = ops.pack_grouped_conv_weight(dev_w, groups)
        kw.update(n_bundles=nb, c_in_ld=cb, c_in_real=cing)
        c_arg = cb
    else:
        if not sub:
            wp = ops.pack_conv_weight(dev_w)[0]
        c_arg = cout
    if pre:
        kw.update(pre=(ps.cuda(), pb.cuda()), pre_relu=True)
    if sub:
        kw.update(subpixel=True, up=2)
        del kw["pad"], kw["dil"], kw["stride"]
    if o.get("splitk"):
        kw["splitk_ws"] = torch.empty(1 << 22, device="cuda")
    if o.get("nchw"):
        y = torch.full((B, cout, H, W), float("nan"), device="cuda")
        kw["y_nchw"] = y
    else:
        ybuf = torch.full((B * H * W, cout + 32), float("nan"), device="cuda")
        y = ybuf[:, 16:16 + cout]
        kw["y2d"] = y
        if res is not None:
            kw["res2d"] = res.permute(0, 2, 3, 1).reshape(B * H * W, cout).contiguous().cuda()

    def go():
        with ops.launch_config(fill_frames=o.get("fill", 16), precision=precision):
            ops.conv_forward(x2d, B, h, w, wp, c_arg, 3 if sub else k, **kw)

    old = ops._BINDING
    if binding is not None:
        ops._BINDING = binding
    try:
        kern = _traced(go)
    finally:
        ops._BINDING = old
    got = (y if o.get("nchw") else y.reshape(B, H, W, cout).permute(0, 3, 1, 2)).cpu().double()
    if not o.get("nchw"):
        assert torch.isnan(ybuf[:, :16]).all() and torch.isnan(ybuf[:, 16 + cout:]).all()      # only the slice is written
    if res is not None:
        mag = mag + res.double().abs()
    return got, ref, mag, kern, y


def _kind_ok(kern, expect):
    assert len(kern) == 1, kern
    kname = kern[0]
    if expect == "halo":
        return kname.startswith("conv_halo_emu_kernel<") and kname.endswith(",bf16>")
    if expect == "row_splitk":
        return kname.startswith("conv_fwd_kernel<") and kname.endswith(",splitk,bf16>")
    return kname.startswith("conv_fwd_kernel<") and kname.endswith(",bf16>") and ",splitk" not in kname


@pytest.mark.parametrize("name", sorted(CASES))
def test_bf16_conv_is_exact_on_rounded_operands(name):
    """Every bf16 product is exact and accumulates in fp32, so the result equals an fp64 convolution of the RNE-rounded
    operands (input rounded after the prologue and zero padding, weights in their packed form) up to fp32 summation
    rounding: |got - ref| <= 2e-6 * sum|terms| per output (+ 2^-22 |ref| for the fp32 epilogue).  A truncating
    conversion, the fp32 path or bf16x3 miss the rounded operands by ~2^-9 / sqrt(K) of sum|terms|: > 10x the bound."""
    got, ref, mag, kern, _ = _run_case(name)
    expect = CASES[name][-1]
    assert _kind_ok(kern, expect), (name, kern, expect)
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs()
    bound = 2e-6 * mag + 2.0 ** -22 * ref.abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(name, kern, "worst err / bound:", worst)
    assert (err <= bound).all(), (name, worst)


def test_bf16_mode_differs_from_fp32_by_operand_rounding_only():
    """Control for the bound above: the fp32 mode on the same case misses the rounded-operand reference by far more than
    the bound (so the bound does tell the modes apart) while the bf16 mode meets it."""
    got32, ref, mag, _, _ = _run_case("3x3", precision="fp32")
    assert float(((got32 - ref).abs() / mag.clamp_min(1e-300)).max()) > 2e-5


def test_round_bf16_matches_torch_rne():
    from bts_amd import ops
    g = torch.Generator().manual_seed(1)
    w = torch.randn((4, 64, 96), generator=g) * torch.pow(10.0, torch.empty((4, 64, 1)).uniform_(-30, 30, generator=g))
    w[0, 0, :5] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.0e-39])    # ties (to even), a denormal
    r = ops.round_bf16(w.cuda()).cpu()
    assert r.shape == (4, 1, 64, 96) and r.dtype == torch.int16
    assert torch.equal(r.squeeze(1), w.to(torch.bfloat16).view(torch.int16))
    assert float((r[0, 0, 0, 2:4].view(torch.bfloat16)).float()[0]) == 1.0


def test_bf16_torch_op_equals_ctypes():
    """torch.ops.bts_hip.conv_fwd (one-plane w_split) and the ctypes binding give the same bits on both kernels."""
    for name in ("3x3", "subpixel64", "1x1", "splitk"):
        a = _run_case(name, binding="torch")[4].clone()
        b = _run_case(name, binding="ctypes")[4].clone()
        assert torch.equal(a, b), name


def test_bf16_conv_runs_are_deterministic():
    for name in ("3x3", "splitk", "grouped"):
        a = _run_case(name)[4].clone()
        b = _run_case(name)[4].clone()
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------- decoder and whole model accuracy
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
    g5, r5 = got[5].detach().cpu().double().numpy(), ref_outs[5].double().numpy()
    rep["iconv1"] = float(np.abs(g5 - r5).max() / np.abs(r5).max())
    return rep


@pytest.mark.parametrize("cname", ["K", "N"])
def test_bf16_decoder_vs_fp32_oracle(cname):
    """The decoder alone at 2x64x96 in bf16 mode against the fp32 oracle: about 3x the CPU estimate of DESIGN 3c."""
    dec = build_hip_decoder(cname, "cuda")
    dec.conv_precision = "bf16"
    got = hip_run(dec, cname, 2, 64, 96, 4321)
    ref_outs, inter = oracle_run(cname, 2, 64, 96, 4321)
    rep = _depth_stats(got, ref_outs, inter)
    print(cname, rep)
    for name in OUT_NAMES[:5]:
        med, mx = rep[name]
        assert med <= 5e-3 and mx <= 5e-2, (name, med, mx)
    assert rep["iconv1"] <= 2e-2, rep["iconv1"]
    # and it is really the bf16 mode: not bit-equal to the fp32 decoder
    dec.conv_precision = "fp32"
    got32 = hip_run(dec, cname, 2, 64, 96, 4321)
    assert not torch.equal(got32[5], got[5])


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.empty_like(m.weight).uniform_(0.8, 1.2, generator=g)
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.05
            m.running_mean = torch.randn(m.running_mean.shape, generator=g) * 0.05
            m.running_var = torch.empty_like(m.running_var).uniform_(0.8, 1.2, generator=g)


def _model(enc, seed=11):
    from bts_amd import bts as M
    ds, md = ("kitti", 80.0) if enc.startswith("densenet") else ("nyu", 10.0)
    params = Params(enc, 512, md, ds)
    torch.manual_seed(seed)
    model = M.BtsModel(params).eval()
    _randomise_bn(model.encoder, 7)
    state_np = synth.decoder_state(synth.ENCODER_CHANNELS[enc], 512, 0)
    model.decoder.load_state_dict({k: (torch.tensor(v) if np.ndim(v) == 0 else t(v)) for k, v in state_np.items()})
    return model, state_np, params


@pytest.mark.parametrize("enc", ["densenet161_bts", "resnext101_bts"])
def test_bf16_whole_model_vs_cpu(enc):
    """Whole BtsModel (native encoder + decoder) at 2x64x96 in bf16 mode against the CPU fp32 encoder + oracle decoder;
    switching the same model back to fp32 reproduces its earlier fp32 bits."""
    from bts_amd import bts as M
    model, state_np, params = _model(enc)
    B, H, W = 2, 64, 96
    x = torch.from_numpy(synth.image_batch(B, H, W, 5))
    focal = torch.from_numpy(synth.focal_values(B, params.dataset, 5))
    with torch.no_grad():
        feats = model.encoder(x)
        ref_outs, inter = O.decoder_forward(O.state_from_numpy(state_np), feats, focal, params.max_depth, params.dataset,
                                            want_intermediates=True)
    mg = M.BtsModel(params).eval()
    mg.load_state_dict(model.state_dict())
    mg = mg.cuda()
    xc, fc = x.cuda(), focal.cuda()
    with torch.no_grad():
        fp32_a = [o.clone() for o in mg(xc, fc)]
        mg.conv_precision = "bf16"
        got = [o.clone() for o in mg(xc, fc)]
        mg.conv_precision = "fp32"
        fp32_b = [o.clone() for o in mg(xc, fc)]
    for i in range(6):
        assert torch.equal(fp32_a[i], fp32_b[i]), "fp32 bits changed after a bf16 forward (output %d)" % i
    assert not torch.equal(fp32_a[5], got[5])
    rep = _depth_stats(got, ref_outs, inter)
    print(enc, rep)
    for name in OUT_NAMES[:5]:
        med, mx = rep[name]
        assert med <= 1.5e-2 and mx <= 1e-1, (name, med, mx)
    assert rep["final_depth"][1] <= 3e-2, rep["final_depth"]


def test_bf16_frames_independent_and_deterministic():
    """At a pinned fill_frames, frame i of a batch of 4 equals the same frame run alone, bit for bit; two runs agree."""
    model, _, params = _model("densenet161_bts", seed=3)
    m = model.cuda()
    m.conv_precision = "bf16"
    m.fill_frames = 8
    x = torch.from_numpy(synth.image_batch(4, 64, 96, 9)).cuda()
    f = torch.from_numpy(synth.focal_values(4, params.dataset, 9)).cuda()
    with torch.no_grad():
        a = [o.clone() for o in m(x, f)]
        b = [o.clone() for o in m(x, f)]
        for i in range(6):
            assert torch.equal(a[i], b[i]), i
        for fr in (0, 3):
            one = m(x[fr:fr + 1], f[fr:fr + 1])
            for i in range(6):
                assert torch.equal(one[i], a[i][fr:fr + 1]), (fr, i)


def test_plans_and_graphs_never_replay_another_precision():
    """A recorded plan (use_plans) and a captured hipGraph (GraphedModel) key on the precision: each of fp32 / bf16x3 /
    bf16 replays its own bits, whatever was recorded or captured before."""
    from bts_amd.graph import GraphedModel
    model, _, params = _model("densenet161_bts", seed=4)
    m = model.cuda()
    m.fill_frames = 2
    x = torch.from_numpy(synth.image_batch(2, 64, 96, 13)).cuda()
    f = torch.from_numpy(synth.focal_values(2, params.dataset, 13)).cuda()
    precs = ("fp32", "bf16x3", "bf16")
    eager = {}
    with torch.no_grad():
        for p in precs:
            m.conv_precision = p
            eager[p] = [o.clone() for o in m(x, f)]
        assert not torch.equal(eager["fp32"][5], eager["bf16"][5])
        assert not torch.equal(eager["bf16x3"][5], eager["bf16"][5])
        m.use_plans = True
        for p in precs + precs[::-1]:
            m.conv_precision = p
            got = m(x, f)
            for i in range(6):
                assert torch.equal(got[i], eager[p][i]), ("plan", p, i)
        m.use_plans = False
        gm = GraphedModel(m)
        for p in precs + precs[::-1]:
            m.conv_precision = p
            got = [o.clone() for o in gm(x, f)]
            torch.cuda.synchronize()
            for i in range(6):
                assert torch.equal(got[i], eager[p][i]), ("graph", p, i)
        assert gm.captures == 3


def test_training_refuses_bf16():
    from bts_amd import train
    from bts_amd._lib import BtsHipError
    model, _, params = _model("densenet161_bts", seed=5)
    m = model.cuda().train()
    m.conv_precision = "bf16"
    x = torch.from_numpy(synth.image_batch(2, 64, 96, 1)).cuda()
    f = torch.from_numpy(synth.focal_values(2, params.dataset, 1)).cuda()
    with pytest.raises(BtsHipError, match="inference"):
        m(x, f)
    from bts_amd import ops
    w = torch.randn(32, 32, 3, 3, device="cuda", requires_grad=True)
    xi = torch.randn(1, 32, 8, 8, device="cuda", requires_grad=True)
    with ops.launch_config(precision="bf16"):
        with pytest.raises(BtsHipError, match="inference"):
            train.conv2d(xi, w, padding=1)


def test_bf16_weight_plane_follows_a_refilled_pack():
    """The one-plane rounding cached on a packed weight (``_bts_round1``) is re-made when train.WeightPacker refills the
    pack in place (``_bts_pack_seq``): after the parameter changes, a bf16 forward on the same packed buffer gives the
    bits of a freshly packed copy of the new values, not the old rounding."""
    from bts_amd import ops, train
    B, cin, cout, h, w = 1, 64, 128, 44, 152
    g = torch.Generator().manual_seed(21)
    x2d = torch.randn((B * h * w, cin), generator=g).cuda()
    wt = (torch.randn((cout, cin, 3, 3), generator=g) / np.sqrt(9.0 * cin)).cuda()

    def run(wp):
        y = torch.empty((B * h * w, cout), device="cuda")

        def go():
            with ops.launch_config(fill_frames=16, precision="bf16"):
                ops.conv_forward(x2d, B, h, w, wp, cout, 3, y2d=y)
        assert _kind_ok(_traced(go), "halo")                  # the kernel that streams the cached plane
        return y.clone()

    wp = train._PACKER.get(wt, cin, train.WeightPacker.FWD)
    old = run(wp)
    assert getattr(wp, "_bts_round1", None) is not None
    with torch.no_grad():
        wt.mul_(-0.75).add_(1e-3)                              # in place: the packer sees a new _version
    assert train._PACKER.get(wt, cin, train.WeightPacker.FWD) is wp
    fresh = ops.pack_conv_weight(wt)[0]
    assert torch.equal(wp, fresh)                              # the refill itself is right: same packed values
    new = run(wp)
    assert torch.equal(new, run(fresh))
    assert not torch.equal(new, old)
