"""GPU: the wide 1x1 convolution with bf16 operands (bts_conv1x1_bf16_fwd_f32, csrc/conv_1x1_bf16.inc) and the model switch
that sends DenseNet161's bottleneck 1x1 layers there (``BtsModel.bf16_wide_1x1``).  The entry point is called
directly, so the plan query's thresholds do not limit the shapes."""
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

KERNEL = "conv1x1_bf16_kernel<192>"
BM = 128        # pixels per workgroup: asserted against the plan query's answer below

# name: (npix, c_in, c_out, options).  The smallest shapes at which each mechanism can fail.
CASES = {
    "one_kstep": (35, 16, 192, {}),                                                  # one 16-k block, less than one tile
    "ragged_bm-1": (BM - 1, 48, 192, {"xs": 96}),                                    # ragged tiles, odd number of 16-k blocks,
    "ragged_bm": (BM, 48, 192, {"xs": 96}),                                          # a channel-prefix view of a wider buffer
    "ragged_bm+1": (BM + 1, 48, 192, {"xs": 96}),
    "ragged_2bm+3": (2 * BM + 3, 48, 192, {"xs": 96}),
    "densenet_form": (2 * 9 * 13, 240, 192, {"xs": 384, "pre": "relu", "e1": True, "act": "relu", "frames": 2}),      # ring wraps
    "longest_k": (40, 2112, 192, {"pre": "relu", "e1": True, "act": "relu"}),        # longest K of the model, many ring turns
    "two_n_tiles": (150, 96, 384, {"pre": "relu"}),                                  # second N tile
    "pre_no_relu_elu": (70, 64, 192, {"pre": "affine", "act": "elu"}),               # negative values survive the prologue
    "range": (64, 64, 192, {"xscale": 2.0 ** 40, "wscale": 2.0 ** -40}),             # as test_bf16_gpu's scale_2^40
    "pad_rows": (33, 32, 192, {"cout_pad": 224}),                                    # c_out_pad > c_out
}


def _rne(v):
    return v.float().to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of a case and its fp64 reference, made once: the conv of the RNE-rounded prologue output (ONE fp32 fma, as the
    kernel's contract says) with the RNE-rounded weights, then e1 / act in fp64; ``mag`` = sum |terms| of an output."""
    npix, c_in, c_out, o = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    xs, ws = o.get("xscale", 1.0), o.get("wscale", 1.0)
    x = torch.randn((npix, c_in), generator=g) * xs
    wt = torch.randn((c_out, c_in), generator=g) / np.sqrt(float(c_in)) * ws
    pre = e1 = None
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
    ref = {2: F.elu, 1: F.relu}.get(act, lambda v: v)(ref)       # 1-Lipschitz: the bound on the pre-activation holds after it
    return dict(x=x, wt=wt, pre=pre, e1=e1, act=act, ref=ref, mag=mag)


def _traced(fn):
    from bts_amd import ops
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        fn()
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    return [r[0] for r in tr.records]


def _run(name, binding=None, rows=None):
    """The case through ops.conv1x1_bf16_forward: NaN-filled input buffer (NaN behind c_in), the output a channel slice of a
    NaN-filled buffer; ``rows``: a (first, count) run of pixels.  Returns (output fp64 on the CPU, kernel names, raw slice)."""
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
    pre = tuple(v.cuda() for v in c["pre"]) if c["pre"] is not None else None
    e1 = tuple(v.cuda() for v in c["e1"]) if c["e1"] is not None else None

    def go():
        ops.conv1x1_bf16_forward(x2d, n, c_in, plane, c_out, y, pre=pre, pre_relu=o.get("pre") == "relu", e1=e1, act=c["act"])

    old = ops._BINDING
    if binding is not None:
        ops._BINDING = binding
    try:
        kern = _traced(go)
    finally:
        ops._BINDING = old
    assert torch.isnan(ybuf[:, :16]).all() and torch.isnan(ybuf[:, 16 + c_out:]).all(), name      # only the slice is written
    return y.cpu().double(), kern, y.clone()


def _worst(got, ref, mag):
    """max over outputs of |got - ref| / (2e-6 * sum|terms| + 2^-22 * |ref|): tests/test_bf16_gpu.py's bound."""
    bound = 2e-6 * mag + 2.0 ** -22 * ref.abs()
    return float(((got - ref).abs() / bound.clamp_min(1e-300)).max())


def test_plan_query_names_the_tile_these_cases_assume():
    from bts_amd import ops
    p = ops.conv1x1_bf16_plan(88, 304, 96, 192, fill_frames=4096)
    assert (p.bm, p.bn) == (BM, 192), tuple(p)


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_on_rounded_operands(name):
    """Products are exact products of the RNE-rounded prologue output and the RNE-rounded weights and sum in fp32:
    |got - ref| <= 2e-6 * sum|terms| + 2^-22 |ref| per output; NaN behind c_in and around the slice stays where it is."""
    got, kern, _ = _run(name)
    c = _case(name)
    assert kern == [KERNEL], kern
    assert torch.isfinite(got).all(), name
    worst = _worst(got, c["ref"], c["mag"])
    print(name, kern, "worst err / bound:", worst)
    assert worst <= 1.0, (name, worst)


def test_todays_bf16_path_meets_the_same_reference_and_fp32_misses_it():
    """Control for the bound: ops.conv_forward under precision "bf16" (what these layers run without the switch) meets the
    same reference within the same bound; under "fp32" it misses it -- the bound tests the mode, not the kernel."""
    from bts_amd import ops
    name = "densenet_form"
    npix, c_in, c_out, o = CASES[name]
    c = _case(name)
    x2d = c["x"].contiguous().cuda()
    wp = ops.pack_conv_weight(c["wt"].reshape(c_out, c_in, 1, 1).cuda())[0]
    pre = tuple(v.cuda() for v in c["pre"])                                    # c_in_ld = c_in elements
    e1 = tuple(ops.pad_vec(v.cuda(), wp.shape[0], f) for v, f in zip(c["e1"], (1.0, 0.0)))
    worst = {}
    for prec in ("bf16", "fp32"):
        y = torch.empty((npix, c_out), device="cuda")
        with ops.launch_config(fill_frames=16, precision=prec):
            ops.conv_forward(x2d, 2, 9, 13, wp, c_out, 1, c_in_ld=c_in, pre=pre, pre_relu=True, e1=e1, act=ops.ACT_RELU, y2d=y)
        worst[prec] = _worst(y.cpu().double(), c["ref"], c["mag"])
    print("ops.conv_forward, worst err / bound:", worst)
    assert worst["bf16"] <= 1.0 and worst["fp32"] > 1.0, worst


def test_torch_op_equals_ctypes():
    for name in ("densenet_form", "ragged_2bm+3", "pre_no_relu_elu"):
        a = _run(name, binding="torch")[2]
        b = _run(name, binding="ctypes")[2]
        assert torch.equal(a, b), name


def test_a_frame_has_the_same_bits_alone_and_in_a_batch_and_runs_agree():
    name = "densenet_form"
    hw = 9 * 13
    both = _run(name)[2]
    assert torch.equal(both, _run(name)[2])
    alone = _run(name, rows=(hw, hw))[2]
    assert torch.equal(alone, both[hw:])


def test_python_layer_refuses_what_the_kernel_does_not_take():
    from bts_amd import ops
    from bts_amd._lib import BtsHipError
    x = torch.zeros((40, 64), device="cuda")
    y = torch.zeros((40, 192), device="cuda")
    w = torch.zeros((1, 192, 64), dtype=torch.int16, device="cuda")
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_forward(x, 40, 64, w.float(), 192, y)                                    # fp32 weights
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_forward(x, 40, 64, w, 192, y, act=ops.ACT_SIGMOID)
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_forward(x, 40, 64, w[:, :128], 128, y[:, :128])                          # c_out 128
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_forward(x, 40, 72, w, 192, y)                                            # c_in % 16, wider than the view
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_forward(x, 40, 64, w, 192, y, pre=(torch.ones(32, device="cuda"), torch.zeros(32, device="cuda")))


# ------------------------------------------------------------------------------------------------------------ model switch
H_IMG, W_IMG = 64, 96
FILL = 4096      # pinned so that the plan query accepts the small maps of a 64x96 image (its threshold counts declared tiles)


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.empty_like(m.weight).uniform_(0.8, 1.2, generator=g)
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.05
            m.running_mean = torch.randn(m.running_mean.shape, generator=g) * 0.05
            m.running_var = torch.empty_like(m.running_var).uniform_(0.8, 1.2, generator=g)


@functools.lru_cache(maxsize=None)
def _model():
    """tests/test_bf16_gpu.py's recipe: DenseNet161, random BN statistics, synthetic decoder state; the CPU fp32 model and its
    oracle outputs, and a GPU copy with fill_frames pinned."""
    from bts_amd import bts as M
    enc = "densenet161_bts"
    params = Params(enc, 512, 80.0, "kitti")
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


def test_model_switch_moves_the_bottlenecks_and_nothing_else():
    from bts_amd import ops
    m, x, f, ref_outs, inter = _model()
    with ops.launch_config(fill_frames=FILL, precision="bf16"):
        accepted = [ops.conv1x1_bf16_plan(H_IMG >> s, W_IMG >> s, 96, 192).eligible for s in (2, 3, 4, 5)]
    assert all(accepted), accepted                      # FILL is large enough for every block's map
    fp32_a = _forward(m, x, f, False, "fp32")
    on = _forward(m, x, f, True)                        # the model's first bf16 forward: the weight planes are made here
    off = _forward(m, x, f, False)
    k_off = _traced(lambda: _forward(m, x, f, False))
    k_on = _traced(lambda: _forward(m, x, f, True))
    off2 = _forward(m, x, f, False)
    fp32_on = _forward(m, x, f, True, "fp32")
    k32_on = _traced(lambda: _forward(m, x, f, True, "fp32"))
    # the switch on: every bottleneck 1x1 of DenseNet161 (6 + 12 + 36 + 24 layers per sub-batch), and only those launches
    n = k_on.count(KERNEL)
    assert KERNEL not in k_off and KERNEL not in k32_on
    assert n > 0 and n % 78 == 0, n
    assert len(k_on) == len(k_off)
    moved = [a for a, b in zip(k_off, k_on) if a != b]
    assert len(moved) == n and all(b == KERNEL for a, b in zip(k_off, k_on) if a != b)
    assert all(a.startswith("conv_fwd_kernel<") or a.startswith("conv_") for a in moved), sorted(set(moved))
    # off is the mode as it was; fp32 with the switch on is fp32 as it was
    for i in range(6):
        assert torch.equal(off[i], off2[i]), i
        assert torch.equal(fp32_a[i], fp32_on[i]), i
    assert not torch.equal(fp32_a[5], on[5])
    # the existing whole-model bars of the bf16 mode (tests/test_bf16_gpu.py) hold with the switch on
    rep = _depth_stats(on, ref_outs, inter)
    print("bf16 + bf16_wide_1x1", rep)
    for name in OUT_NAMES[:5]:
        med, mx = rep[name]
        assert med <= 1.5e-2 and mx <= 1e-1, (name, med, mx)
    assert rep["final_depth"][1] <= 3e-2, rep["final_depth"]


def test_graphs_key_on_the_switch():
    from bts_amd.graph import GraphedModel
    m, x, f, _, _ = _model()
    eager = {on: _forward(m, x, f, on) for on in (False, True)}
    gm = GraphedModel(m)
    try:
        first = None
        for on in (False, True, True, False):
            m.bf16_wide_1x1, m.conv_precision = on, "bf16"
            with torch.no_grad():
                got = [o.clone() for o in gm(x, f)]
            torch.cuda.synchronize()
            first = got if first is None else first
            for i in range(6):
                assert torch.equal(got[i], eager[on][i]), ("graph", on, i)
        assert gm.captures == 2                          # the flip captured again, the flip back replayed the first capture
        for i in range(6):
            assert torch.equal(got[i], first[i]), i
    finally:
        m.bf16_wide_1x1, m.conv_precision = False, "fp32"


def test_plans_refuse_the_switch_in_bf16_mode():
    from bts_amd._lib import BtsHipError
    m, x, f, _, _ = _model()
    m.use_plans = True
    try:
        with pytest.raises(BtsHipError, match="bf16_wide_1x1"):
            _forward(m, x, f, True)
        _forward(m, x, f, True, "fp32")                  # the switch changes nothing outside the bf16 mode: a plan records
    finally:
        m.use_plans = False


def test_weight_plane_follows_a_refilled_pack():
    """The plane the new path streams is the ``_bts_round1`` cached on the packed weight: after train.WeightPacker refills
    the pack in place, the encoder's own lookup returns the rounding of the NEW values (in the same buffer)."""
    from bts_amd import ops, train
    c_in, c_out, npix = 96, 192, 200
    g = torch.Generator().manual_seed(33)
    x2d = torch.randn((npix, c_in), generator=g).cuda()
    wt = (torch.randn((c_out, c_in, 1, 1), generator=g) / np.sqrt(float(c_in))).cuda()

    def run(wp):
        y = torch.empty((npix, c_out), device="cuda")
        ops.conv1x1_bf16_forward(x2d, npix, c_in, ops._derived_weight(wp, "_bts_round1", ops.round_bf16), c_out, y)
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
