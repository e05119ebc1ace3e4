"""GPU: the wide bf16 1x1 tile at 128 / 192 / 256 output channels per workgroup with the bottleneck epilogue
(bts_conv1x1_bf16_wide_fwd_f32, csrc/conv_1x1_bf16.inc) and the third value of the model switch, ``BtsModel.bf16_wide_1x1 =
"all"``, that sends ResNe(X)t's and DenseNet121's 1x1 layers there.  The entry point is called directly, so the
plan query's thresholds do not limit the shapes."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bts_amd import synth
from oracle import bts_oracle as O
from parity_util import OUT_NAMES, Params, singular_masks, t

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("BTS_CONV_PRECISION", "0").strip() == "1",
                                 reason="BTS_CONV_PRECISION=1 forces precision 1 inside every scope")]

BM = 128        # pixels per workgroup: asserted against the plan query's answer below
FAMILY = "conv1x1_bf16_kernel<"
HW = 9 * 13
BOTTLENECK = dict(e1=True, res=320, act="relu", y2=True)

# name: (npix, c_in, c_out, options).  The smallest shapes at which each mechanism can fail.
CASES = {
    "one_kstep_128": (35, 16, 128, {}),                                              # one 16-k block, less than one tile
    "one_kstep_256": (35, 16, 256, {}),
    "ragged_bm-1": (BM - 1, 48, 128, {"xs": 96}),                                    # ragged tiles, odd number of 16-k blocks,
    "ragged_bm": (BM, 48, 128, {"xs": 96}),                                          # a channel-prefix view of a wider buffer
    "ragged_bm+1": (BM + 1, 48, 128, {"xs": 96}),
    "ragged_2bm+3": (2 * BM + 3, 48, 128, {"xs": 96}),
    "resnet_conv3": (2 * HW, 64, 256, BOTTLENECK),                                   # e1, identity, ReLU, skip tap; two frames
    "downsample": (2 * HW, 64, 256, {"e1": True}),                                   # stride-1 downsample: e1 only
    "res_only": (2 * HW, 64, 256, {"res": 320}),                                     # res without e1 or act
    "densenet121_form": (2 * HW, 224, 128, {"xs": 384, "pre": "relu", "e1": True, "act": "relu"}),
    "longest_k": (40, 2048, 128, {"bn": 128}),                                       # longest K, many ring turns
    "longest_k_pre": (40, 992, 128, {"bn": 128, "pre": "relu"}),
    "two_n_tiles_256": (150, 96, 512, {"bn": 256}),                                  # second N tile
    "two_n_tiles_128": (150, 96, 256, {"bn": 128}),
    "pad_rows": (33, 32, 128, {"cout_pad": 160}),                                    # c_out_pad > c_out
    "range": (64, 64, 128, {"xscale": 2.0 ** 40, "wscale": 2.0 ** -40}),             # as test_bf16_gpu's scale_2^40
    "n384": (150, 96, 384, {"e1": True, "res": 400, "act": "relu"}),               # identities only: bn 128 against 192
    "old_densenet_form": (2 * HW, 240, 192, {"xs": 384, "pre": "relu", "e1": True, "act": "relu"}),   # the sibling's case
}
CHECKED = sorted(set(CASES) - {"n384", "old_densenet_form"})


def _rne(v):
    return v.float().to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of a case and its fp64 reference, made once: the conv of the RNE-rounded prologue output (ONE fp32 fma) with the
    RNE-rounded weights, then e1, + res, act in fp64; ``mag`` = sum |terms| of an output, |e1_shift| and |res| included."""
    npix, c_in, c_out, o = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    xs, ws = o.get("xscale", 1.0), o.get("wscale", 1.0)
    x = torch.randn((npix, c_in), generator=g) * xs
    wt = torch.randn((c_out, c_in), generator=g) / np.sqrt(float(c_in)) * ws
    pre = e1 = res = None
    p = x
    if o.get("pre"):
        pre = (torch.rand(c_in, generator=g) + 0.5, torch.randn(c_in, generator=g) * 0.3)
        p = torch.from_numpy(np.asarray(np.float32(x.double().numpy() * pre[0].double().numpy() + pre[1].double().numpy())))   # one rounding
        if o["pre"] == "relu":
            p = p.clamp_min(0.0)
    act = {"elu": 2, "relu": 1}.get(o.get("act"), 0)
    pr, wr = _rne(p), _rne(wt)
    ref = pr @ wr.t()
    mag = pr.abs() @ wr.abs().t()
    if o.get("e1"):
        e1 = (torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g) * 0.1)
        ref = ref * e1[0].double() + e1[1].double()
        mag = mag * e1[0].double().abs() + e1[1].double().abs()
    if o.get("res"):
        res = torch.randn((npix, c_out), generator=g)
        ref = ref + res.double()
        mag = mag + res.double().abs()
    ref = {2: F.elu, 1: F.relu}.get(act, lambda v: v)(ref)       # 1-Lipschitz: the bound on the pre-activation holds after it
    return dict(x=x, wt=wt, pre=pre, e1=e1, res=res, act=act, ref=ref, mag=mag)


def _traced(fn):
    """[(kernel, tag)] of the launches ``fn`` makes."""
    from bts_amd import ops
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        fn()
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    return [(r[0], r[1]) for r in tr.records]


def _run(name, binding=None, rows=None, bn=None, y2=None, res_nan=None, old_entry=False):
    """The case through ops.conv1x1_bf16_wide_forward: NaN-filled input buffer (NaN behind c_in); y, y2 and res channel slices
    of wider buffers, y and y2 surrounded by NaN that must survive.  ``rows``: a (first, count) run of pixels; ``bn`` / ``y2``
    override the case's; ``res_nan`` = (p, n) poisons one residual value.  Returns (y fp64 on the CPU, kernel names, y, y2)."""
    from bts_amd import ops
    npix, c_in, c_out, o = CASES[name]
    c = _case(name)
    r0, n = rows if rows else (0, npix)
    xstride = o.get("xs", c_in + 16)                                           # always something NaN behind c_in
    xbuf = torch.full((n, xstride), float("nan"))
    xbuf[:, :c_in] = c["x"][r0:r0 + n]
    x2d = xbuf.cuda()[:, :c_in]
    wp = ops.pack_conv_weight(c["wt"].reshape(c_out, c_in, 1, 1).cuda())[0]
    plane = ops.round_bf16(wp)                                                 # int16 [1, c_out_pad, k_pad]
    if o.get("cout_pad"):                                                      # zero rows beyond c_out: may be read, never stored
        big = torch.zeros((1, o["cout_pad"], plane.shape[2]), dtype=torch.int16, device="cuda")
        big[:, :plane.shape[1]] = plane
        plane = big
    ybuf = torch.full((n, c_out + 32), float("nan"), device="cuda")
    y = ybuf[:, 16:16 + c_out]
    want_y2 = o.get("y2", False) if y2 is None else y2
    y2buf = torch.full((n, c_out + 40), float("nan"), device="cuda")
    y2v = y2buf[:, 8:8 + c_out] if want_y2 else None
    res = None
    if c["res"] is not None:
        rbuf = torch.full((n, o["res"]), float("nan"))
        rbuf[:, 4:4 + c_out] = c["res"][r0:r0 + n]
        if res_nan is not None:
            rbuf[res_nan[0], 4 + res_nan[1]] = float("nan")
        res = rbuf.cuda()[:, 4:4 + c_out]
    pre = tuple(v.cuda() for v in c["pre"]) if c["pre"] is not None else None
    e1 = tuple(v.cuda() for v in c["e1"]) if c["e1"] is not None else None
    tile = o.get("bn", 0) if bn is None else bn

    def go():
        if old_entry:
            ops.conv1x1_bf16_forward(x2d, n, c_in, plane, c_out, y, pre=pre, pre_relu=o.get("pre") == "relu", e1=e1, act=c["act"])
        else:
            ops.conv1x1_bf16_wide_forward(x2d, n, c_in, plane, c_out, y, pre=pre, pre_relu=o.get("pre") == "relu", e1=e1, res2d=res,
                                          y2_2d=y2v, act=c["act"], bn=tile)

    old = ops._BINDING
    if binding is not None:
        ops._BINDING = binding
    try:
        kern = [k for k, _ in _traced(go)]
    finally:
        ops._BINDING = old
    assert torch.isnan(ybuf[:, :16]).all() and torch.isnan(ybuf[:, 16 + c_out:]).all(), name      # only the slice is written
    assert torch.isnan(y2buf[:, :8]).all() and torch.isnan(y2buf[:, 8 + c_out:]).all(), name
    if not want_y2:
        assert torch.isnan(y2buf).all(), name
    return y.cpu().double(), kern, y.clone(), (y2v.clone() if want_y2 else None)


def _worst(got, ref, mag):
    """max over outputs of |got - ref| / (2e-6 * sum|terms| + 2^-22 * |ref|): tests/test_bf16_gpu.py's bound."""
    bound = 2e-6 * mag + 2.0 ** -22 * ref.abs()
    return float(((got - ref).abs() / bound.clamp_min(1e-300)).max())


def test_plan_query_names_the_tile_these_cases_assume():
    from bts_amd import conv_plan, ops
    for c_out in (128, 256, 384, 512):
        p = ops.conv1x1_bf16_wide_plan(88, 304, 96, c_out, fill_frames=4096)
        if p.eligible:                                   # a refused class answers zeros; an accepted one names the tile of bn = 0
            assert p.bm == BM and p.bn == conv_plan.wide_1x1_bf16_tile(c_out), (c_out, tuple(p))
            assert p.workgroups == (88 * 304 + BM - 1) // BM * (c_out // p.bn)


@pytest.mark.parametrize("name", CHECKED)
def test_exact_on_rounded_operands(name):
    """Products are exact products of the RNE-rounded prologue output and the RNE-rounded weights and sum in fp32:
    |got - ref| <= 2e-6 * sum|terms| + 2^-22 |ref| per output (|res| and |e1_shift| among the terms); NaN behind c_in and around
    the y / y2 slices stays where it is; y2 holds y's bits."""
    from bts_amd import conv_plan
    got, kern, y, y2 = _run(name)
    c = _case(name)
    o = CASES[name][3]
    assert kern == [conv_plan.wide_1x1_bf16_kernel_name(o.get("bn") or conv_plan.wide_1x1_bf16_tile(CASES[name][2]))], kern
    assert torch.isfinite(got).all(), name
    if o.get("y2"):
        assert torch.equal(y, y2), name
    worst = _worst(got, c["ref"], c["mag"])
    print(name, kern, "worst err / bound:", worst)
    assert worst <= 1.0, (name, worst)


def test_todays_bf16_path_meets_the_same_reference_and_fp32_misses_it():
    """Control for the bound: ops.conv_forward with res2d under precision "bf16" (what a ResNet conv3 runs without the switch)
    meets the same reference within the same bound; under "fp32" it misses it -- the bound tests the mode, not the kernel."""
    from bts_amd import ops
    name = "resnet_conv3"
    npix, c_in, c_out, o = CASES[name]
    c = _case(name)
    x2d = c["x"].contiguous().cuda()
    res = c["res"].contiguous().cuda()
    wp = ops.pack_conv_weight(c["wt"].reshape(c_out, c_in, 1, 1).cuda())[0]
    e1 = tuple(ops.pad_vec(v.cuda(), wp.shape[0], f) for v, f in zip(c["e1"], (1.0, 0.0)))
    worst = {}
    for prec in ("bf16", "fp32"):
        y = torch.empty((npix, c_out), device="cuda")
        with ops.launch_config(fill_frames=16, precision=prec):
            ops.conv_forward(x2d, 2, 9, 13, wp, c_out, 1, c_in_ld=c_in, e1=e1, act=ops.ACT_RELU, y2d=y, res2d=res)
        worst[prec] = _worst(y.cpu().double(), c["ref"], c["mag"])
    print("ops.conv_forward, worst err / bound:", worst)
    assert worst["bf16"] <= 1.0 and worst["fp32"] > 1.0, worst


def test_bits_do_not_depend_on_the_tile():
    a = _run("resnet_conv3", bn=128)
    b = _run("resnet_conv3", bn=256)
    assert a[1] == [FAMILY + "128>"] and b[1] == [FAMILY + "256>"], (a[1], b[1])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    a, b = _run("n384", bn=128), _run("n384", bn=192)
    assert a[1] == [FAMILY + "128>"] and b[1] == [FAMILY + "192>"], (a[1], b[1])
    assert torch.equal(a[2], b[2])
    c = _case("n384")
    assert _worst(a[0], c["ref"], c["mag"]) <= 1.0


def test_second_destination_changes_nothing_and_holds_the_same_values():
    w = _run("resnet_conv3", y2=True)
    wo = _run("resnet_conv3", y2=False)
    assert torch.equal(w[2], wo[2]) and torch.equal(w[2], w[3]) and wo[3] is None
    w, wo = _run("downsample", y2=True), _run("downsample", y2=False)      # y2 without res
    assert torch.equal(w[2], wo[2]) and torch.equal(w[2], w[3])


def test_a_frame_has_the_same_bits_alone_and_in_a_batch_and_runs_agree():
    for name in ("resnet_conv3", "densenet121_form"):
        both = _run(name)[2]
        assert torch.equal(both, _run(name)[2])
        alone = _run(name, rows=(HW, HW))[2]
        assert torch.equal(alone, both[HW:]), name


def test_torch_op_equals_ctypes():
    for name in ("resnet_conv3", "densenet121_form", "ragged_2bm+3", "res_only"):
        a = _run(name, binding="torch")
        b = _run(name, binding="ctypes")
        assert torch.equal(a[2], b[2]), name
        if a[3] is not None:
            assert torch.equal(a[3], b[3]), name


def test_tile_192_without_res_is_the_old_entry_point():
    new = _run("old_densenet_form", bn=192)
    old = _run("old_densenet_form", old_entry=True)
    assert new[1] == old[1] == [FAMILY + "192>"]
    assert torch.equal(new[2], old[2])
    c = _case("old_densenet_form")
    assert _worst(new[0], c["ref"], c["mag"]) <= 1.0


def test_a_nan_in_the_residual_reaches_its_own_output_only():
    name = "res_only"                                    # no activation: the library's ReLU maps NaN to 0 (max(NaN, 0) = 0)
    p, n = 2 * HW - 2, 129                               # in the ragged last tile, second 128-channel half
    clean = _run(name, y2=True)
    bad = _run(name, y2=True, res_nan=(p, n))
    for i in (2, 3):                                     # y and y2
        assert torch.isnan(bad[i][p, n])
        mask = torch.ones_like(bad[i], dtype=torch.bool)
        mask[p, n] = False
        assert torch.equal(bad[i][mask], clean[i][mask])


def test_python_layer_refuses_what_the_kernel_does_not_take():
    from bts_amd import ops
    from bts_amd._lib import BtsHipError
    x = torch.zeros((40, 64), device="cuda")
    y = torch.zeros((40, 256), device="cuda")
    w = torch.zeros((1, 256, 64), dtype=torch.int16, device="cuda")
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_wide_forward(x, 40, 64, w.float(), 256, y)                               # fp32 weights
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_wide_forward(x, 40, 64, w, 256, y, act=ops.ACT_SIGMOID)
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_wide_forward(x, 40, 64, w[:, :64], 64, y[:, :64])                        # c_out 64
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_wide_forward(x, 40, 64, w, 256, y, bn=192)                               # a tile that does not divide c_out
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_wide_forward(x, 40, 64, w, 256, y, res2d=y[:, :128])                     # res narrower than c_out
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_wide_forward(x, 40, 64, w, 256, y, y2_2d=torch.zeros((39, 256), device="cuda"))


# ------------------------------------------------------------------------------------------------------------ model switch
H_IMG, W_IMG = 64, 96
FILL = 4096      # pinned so that the plan queries judge the small maps of a 64x96 image by their class alone


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.empty_like(m.weight).uniform_(0.8, 1.2, generator=g)
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.05
            m.running_mean = torch.randn(m.running_mean.shape, generator=g) * 0.05
            m.running_var = torch.empty_like(m.running_var).uniform_(0.8, 1.2, generator=g)


@functools.lru_cache(maxsize=None)
def _model(enc):
    """tests/test_bf16_gpu.py's recipe: random BN statistics, synthetic decoder state; the CPU fp32 model's oracle outputs, and a
    GPU copy with fill_frames pinned."""
    from bts_amd import bts as M
    ds, md = ("kitti", 80.0) if enc.startswith("densenet") else ("nyu", 10.0)
    params = Params(enc, 512, md, ds)
    torch.manual_seed(11)
    model = M.BtsModel(params).eval()
    _randomise_bn(model.encoder, 7)
    state_np = synth.decoder_state(synth.ENCODER_CHANNELS[enc], 512, 0)
    model.decoder.load_state_dict({k: (torch.tensor(v) if np.ndim(v) == 0 else t(v)) for k, v in state_np.items()})
    x = torch.from_numpy(synth.image_batch(2, H_IMG, W_IMG, 5))
    f = torch.from_numpy(synth.focal_values(2, params.dataset, 5))
    with torch.no_grad():
        feats = model.encoder(x)
        ref_outs, inter = O.decoder_forward(O.state_from_numpy(state_np), feats, f, params.max_depth, params.dataset,
                                            want_intermediates=True)
    mg = M.BtsModel(params).eval()
    mg.load_state_dict(model.state_dict())
    mg = mg.cuda()
    mg.fill_frames = FILL
    return mg, x.cuda(), f.cuda(), ref_outs, inter


def _forward(m, x, f, on, prec="bf16"):
    m.bf16_wide_1x1, m.conv_precision = on, prec
    try:
        with torch.no_grad():
            return [o.clone() for o in m(x, f)]
    finally:
        m.bf16_wide_1x1, m.conv_precision = False, "fp32"


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


def _expected_moves(m):
    """{launch tag: layers per sub-batch forward that "all" moves} from the module tree and the plan queries alone."""
    from bts_amd import encoders, ops
    base = m.encoder.base_model
    exp = {}

    def add(tag, ok):
        exp[tag] = exp.get(tag, 0) + int(bool(ok))

    with ops.launch_config(fill_frames=FILL, precision="bf16"):
        if isinstance(base, encoders.ResNet):
            h, w = H_IMG // 4, W_IMG // 4
            for li, layer in enumerate((base.layer1, base.layer2, base.layer3, base.layer4)):
                tag = "enc_l%d" % (li + 1)
                for blk in layer:
                    s = blk.conv2.stride[0]
                    c_in, width, c_out = blk.conv1.in_channels, blk.conv1.out_channels, blk.conv3.out_channels
                    add(tag + "_1x1", ops.conv1x1_bf16_wide_plan(h, w, c_in, width).eligible)            # 64-wide: refused
                    if blk.downsample is not None:
                        add(tag + "_down", blk.downsample[0].stride[0] == 1 and ops.conv1x1_bf16_wide_plan(h, w, c_in, c_out).eligible)
                    h, w = h // s, w // s
                    add(tag + "_1x1", ops.conv1x1_bf16_wide_plan(h, w, width, c_out, has_res=True).eligible)
        else:
            blocks = [b for n, b in base.named_children() if n.startswith("denseblock")]
            for bi, blk in enumerate(blocks):
                h, w = H_IMG >> (bi + 2), W_IMG >> (bi + 2)
                for layer in blk.values():
                    c_in, c_mid = layer.conv1.in_channels, layer.conv1.out_channels
                    add("enc_b%d_1x1" % (bi + 1), ops.conv1x1_bf16_plan(h, w, c_in, c_mid).eligible
                        or ops.conv1x1_bf16_wide_plan(h, w, c_in, c_mid).eligible)
    return exp


BARS = {name: (1.5e-2, 1e-1) for name in OUT_NAMES[:5]}       # tests/test_bf16_gpu.py: (median, max) of the five depth maps
FINAL_MAX = 3e-2                                             # and final_depth's max


@pytest.mark.parametrize("enc", ["resnext101_bts", "resnet50_bts", "densenet121_bts"])
def test_model_switch_moves_the_accepted_1x1_layers_and_nothing_else(enc):
    m, x, f, ref_outs, inter = _model(enc)
    exp = _expected_moves(m)
    fp32_a = _forward(m, x, f, False, "fp32")
    on = _forward(m, x, f, "all")                       # the first forward with the switch: the weight planes are made here
    off = _forward(m, x, f, False)
    k_off = _traced(lambda: _forward(m, x, f, False))
    k_on = _traced(lambda: _forward(m, x, f, "all"))
    k_true = _traced(lambda: _forward(m, x, f, True))
    off2 = _forward(m, x, f, False)
    fp32_on = _forward(m, x, f, "all", "fp32")
    k32_on = _traced(lambda: _forward(m, x, f, "all", "fp32"))
    k32_off = _traced(lambda: _forward(m, x, f, False, "fp32"))
    assert k32_on == k32_off and k_true == k_off           # nothing outside the bf16 mode; True means DenseNet161 only
    assert not any(k.startswith(FAMILY) for k, _ in k_off)
    assert len(k_on) == len(k_off)
    moved = {}
    for (ka, ta), (kb, tb) in zip(k_off, k_on):
        assert ta == tb
        if ka != kb:
            assert kb.startswith(FAMILY) and (ta.endswith("_1x1") or ta.endswith("_down")), (ka, kb, ta)
            moved[ta] = moved.get(ta, 0) + 1
        else:
            assert not kb.startswith(FAMILY)
    per_sub = sum(exp.values())
    n = sum(moved.values())
    print(enc, "expected per sub-batch", exp, "moved", moved)
    assert n == sum(1 for k, _ in k_on if k.startswith(FAMILY))
    if per_sub == 0:
        assert n == 0                                   # the bench admitted no class of this encoder: the switch moves nothing
    else:
        assert n > 0 and n % per_sub == 0, (n, per_sub)
        subs = n // per_sub
        assert moved == {tag: c * subs for tag, c in exp.items() if c}, (moved, exp, subs)
    # off is the mode as it was; fp32 with the switch on is fp32 as it was
    for i in range(6):
        assert torch.equal(off[i], off2[i]), i
        assert torch.equal(fp32_a[i], fp32_on[i]), i
    assert not torch.equal(fp32_a[5], on[5])
    rep, rep_off = _depth_stats(on, ref_outs, inter), _depth_stats(off, ref_outs, inter)
    print(enc, 'bf16 + "all"', rep, "bf16", rep_off)
    for name in OUT_NAMES[:5]:
        med, mx = rep[name]
        bar_med, bar_max = BARS[name]
        if enc != "resnext101_bts":                      # the parent's path in the same test is the yardstick of the other two
            bar_med, bar_max = max(bar_med, 1.5 * rep_off[name][0]), max(bar_max, 1.5 * rep_off[name][1])
        assert med <= bar_med and mx <= bar_max, (name, med, mx, rep_off[name])
    final_bar = FINAL_MAX if enc == "resnext101_bts" else max(FINAL_MAX, 1.5 * rep_off["final_depth"][1])
    assert rep["final_depth"][1] <= final_bar, (rep["final_depth"], rep_off["final_depth"])


def test_all_moves_at_least_what_true_moves_on_densenet161():
    m, x, f, _, _ = _model("densenet161_bts")
    k_off = _traced(lambda: _forward(m, x, f, False))
    k_true = _traced(lambda: _forward(m, x, f, True))
    k_all = _traced(lambda: _forward(m, x, f, "all"))
    assert len(k_off) == len(k_true) == len(k_all)
    n_true = 0
    for a, b, c in zip(k_off, k_true, k_all):
        if a != b:
            n_true += 1
            assert b[0] == FAMILY + "192>" and c == b, (a, b, c)
    assert n_true > 0 and n_true % 78 == 0, n_true      # True is unchanged: every bottleneck (6 + 12 + 36 + 24 per sub-batch)
    t1, t2 = _forward(m, x, f, True), _forward(m, x, f, "all")
    for i in range(6):
        assert torch.equal(t1[i], t2[i]), i


def test_graphs_key_on_the_three_values():
    from bts_amd.graph import GraphedModel
    m, x, f, _, _ = _model("densenet161_bts")
    eager = {on: _forward(m, x, f, on) for on in (False, True, "all")}
    gm = GraphedModel(m)
    try:
        for on in (False, "all", True, "all"):
            m.bf16_wide_1x1, m.conv_precision = on, "bf16"
            with torch.no_grad():
                got = [o.clone() for o in gm(x, f)]
            torch.cuda.synchronize()
            for i in range(6):
                assert torch.equal(got[i], eager[on][i]), ("graph", on, i)
        assert gm.captures == 3                          # one per value; the second "all" replayed its own capture
    finally:
        m.bf16_wide_1x1, m.conv_precision = False, "fp32"


def test_plans_refuse_all_in_bf16_mode():
    from bts_amd._lib import BtsHipError
    m, x, f, _, _ = _model("resnet50_bts")
    m.use_plans = True
    try:
        with pytest.raises(BtsHipError, match="bf16_wide_1x1"):
            _forward(m, x, f, "all")
        _forward(m, x, f, "all", "fp32")                 # the switch changes nothing outside the bf16 mode: a plan records
    finally:
        m.use_plans = False


def test_weight_plane_follows_a_refilled_pack():
    """The plane the new path streams is the ``_bts_round1`` cached on the packed weight: after train.WeightPacker refills
    the pack in place, the encoder's own lookup returns the rounding of the NEW values (in the same buffer)."""
    from bts_amd import ops, train
    c_in, c_out, npix = 96, 256, 200
    g = torch.Generator().manual_seed(33)
    x2d = torch.randn((npix, c_in), generator=g).cuda()
    wt = (torch.randn((c_out, c_in, 1, 1), generator=g) / np.sqrt(float(c_in))).cuda()

    def run(wp):
        y = torch.empty((npix, c_out), device="cuda")
        ops.conv1x1_bf16_wide_forward(x2d, npix, c_in, ops._derived_weight(wp, "_bts_round1", ops.round_bf16), c_out, y)
        return y.clone()

    wp = train._PACKER.get(wt, c_in, train.WeightPacker.FWD)
    old = run(wp)
    plane = wp._bts_round1
    with torch.no_grad():
        wt.mul_(-0.75).add_(1e-3)
    assert train._PACKER.get(wt, c_in, train.WeightPacker.FWD) is wp
    new = run(wp)
    assert wp._bts_round1 is plane                                             # re-made in place
    assert torch.equal(new, run(ops.pack_conv_weight(wt)[0])) and not torch.equal(new, old)
