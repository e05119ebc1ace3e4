"""GPU: the bf16-resident bottleneck intermediate of a dense layer (``BtsModel.bf16_mid_storage``).

  * the producer: bts_conv1x1_bf16_fwd_bf16 stores exactly the nearest-even bf16 rounding of what bts_conv1x1_bf16_fwd_f32
    stores, into a channel slice of a bf16 buffer and nowhere else;
  * the consumer: bts_conv3x3_bf16in_fwd_f32 is bit for bit ops.conv_forward under precision "bf16" on the same values held
    in fp32 wherever that runs the bf16 halo tile, and meets the mode's fp64 bound on ragged maps too;
  * the model: every output bit of DenseNet161 + decoder is the same with the switch on.
Both entry points are called directly, so the plan queries' thresholds do not limit the shapes."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity_util import Params

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("BTS_CONV_PRECISION", "0").strip() == "1",
                                 reason="BTS_CONV_PRECISION=1 forces precision 1 inside every scope")]

SENTINEL = 0x7FC1                # int16 bits of a quiet NaN with a payload no kernel produces


def _traced(fn):
    from bts_amd import ops
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        fn()
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    return [(r[0], r[1], r[3]) for r in tr.records]          # kernel, tag, bytes


def _with_binding(binding, fn):
    from bts_amd import ops
    old = ops._BINDING
    ops._BINDING = binding
    try:
        return fn()
    finally:
        ops._BINDING = old


# ---------------------------------------------------------------------------------------------------------------- producer
# name: (npix, c_in, c_out, options): a ragged last tile (33, 129, 257), an exact one (128), a partial last K step (16, 48,
# 240 are odd multiples of 16), two N tiles (384), with and without pre / e1, ReLU and ELU
PRODUCER = {
    "33_16_192_plain": (33, 16, 192, {}),
    "128_48_192_dense": (128, 48, 192, {"pre": "relu", "e1": True, "act": "relu"}),
    "129_240_192_dense": (129, 240, 192, {"pre": "relu", "e1": True, "act": "relu"}),
    "257_48_384_elu": (257, 48, 384, {"pre": "affine", "act": "elu"}),
    "257_240_384_e1": (257, 240, 384, {"e1": True}),
    "129_16_384_e1_elu": (129, 16, 384, {"e1": True, "act": "elu"}),
}


@functools.lru_cache(maxsize=None)
def _producer_case(name):
    """Operands on the GPU (x a channel-prefix view with NaN behind c_in) and the fp32 entry point's output on them."""
    from bts_amd import ops
    npix, c_in, c_out, o = PRODUCER[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    xbuf = torch.full((npix, c_in + 16), float("nan"))
    xbuf[:, :c_in] = torch.randn((npix, c_in), generator=g)
    x2d = xbuf.cuda()[:, :c_in]
    wt = torch.randn((c_out, c_in, 1, 1), generator=g) / np.sqrt(float(c_in))
    plane = ops.round_bf16(ops.pack_conv_weight(wt.cuda())[0])
    pre = e1 = None
    if o.get("pre"):
        pre = ((torch.rand(c_in, generator=g) + 0.5).cuda(), (torch.randn(c_in, generator=g) * 0.3).cuda())
    if o.get("e1"):
        e1 = ((torch.rand(c_out, generator=g) + 0.5).cuda(), (torch.randn(c_out, generator=g) * 0.1).cuda())
    kw = dict(pre=pre, pre_relu=o.get("pre") == "relu", e1=e1, act={"elu": 2, "relu": 1}.get(o.get("act"), 0))
    y32 = torch.empty((npix, c_out), device="cuda")
    ops.conv1x1_bf16_forward(x2d, npix, c_in, plane, c_out, y32, **kw)
    torch.cuda.synchronize()
    return x2d, plane, kw, y32


def _produce(name, binding):
    from bts_amd import ops
    npix, c_in, c_out, _ = PRODUCER[name]
    x2d, plane, kw, _ = _producer_case(name)
    ybuf = torch.full((npix, c_out + 40), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    y = ybuf[:, 16:16 + c_out]
    recs = _with_binding(binding, lambda: _traced(lambda: ops.conv1x1_bf16_forward(x2d, npix, c_in, plane, c_out, y, **kw)))
    return ybuf.view(torch.int16), recs


@pytest.mark.parametrize("name", sorted(PRODUCER))
def test_producer_stores_the_rounding_of_the_fp32_entry_points_output(name):
    npix, c_in, c_out, _ = PRODUCER[name]
    y32 = _producer_case(name)[3]
    assert torch.isfinite(y32).all()
    want = y32.to(torch.bfloat16).view(torch.int16)                       # nearest even
    got, recs = _produce(name, "torch")
    assert [r[0] for r in recs] == ["conv1x1_bf16_ybf16_kernel<192>"], recs
    assert recs[0][2] == 4.0 * npix * c_in + 2.0 * npix * c_out + 2.0 * c_out * c_in      # the bf16 tensor counts 2 bytes
    assert torch.equal(got[:, 16:16 + c_out], want), name
    assert (got[:, :16] == SENTINEL).all() and (got[:, 16 + c_out:] == SENTINEL).all(), name      # only the slice is written
    assert torch.equal(got, _produce(name, "ctypes")[0]), name            # both bindings, the same bits


# ---------------------------------------------------------------------------------------------------------------- consumer
# name: (B, h, w, c_in, c_out, e1 + ReLU).  ELIGIBLE: maps of whole 4x32 tiles, which conv_forward runs on the bf16 halo tile;
# RAGGED: maps it leaves to the row-tiled kernel (under 0.80 real pixels), through the entry point only
ELIGIBLE = {
    "4x32_b1_32_48": (1, 4, 32, 32, 48, False),
    "8x64_b2_64_64_e1": (2, 8, 64, 64, 64, True),
    "16x32_b1_192_128_e1": (1, 16, 32, 192, 128, True),
    "8x64_b2_192_48": (2, 8, 64, 192, 48, False),                         # the growth convolution's own form
    "4x32_b2_64_128": (2, 4, 32, 64, 128, False),
}
RAGGED = {
    "5x31_b2_32_48": (2, 5, 31, 32, 48, False),
    "9x33_b1_64_128_e1": (1, 9, 33, 64, 128, True),
    "12x40_b1_192_64": (1, 12, 40, 192, 64, False),
}
CONSUMER = dict(ELIGIBLE, **RAGGED)


@functools.lru_cache(maxsize=None)
def _consumer_case(name):
    """The bf16 input (a prefix view of a wider buffer, NaN behind c_in), the packed weight, e1, and the fp64 convolution of
    the bf16 input with the rounded weights: ``ref`` and ``mag`` = sum |terms| per output, NHWC rows."""
    from bts_amd import ops
    B, h, w, c_in, c_out, full = CONSUMER[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    xb = torch.randn((B, h, w, c_in), generator=g).to(torch.bfloat16)
    wt = torch.randn((c_out, c_in, 3, 3), generator=g) / np.sqrt(9.0 * c_in)
    buf = torch.full((B * h * w, c_in + 8), float("nan"), dtype=torch.bfloat16)
    buf[:, :c_in] = xb.reshape(-1, c_in)
    wp = ops.pack_conv_weight(wt.cuda())[0]
    e1 = None
    xd, wd = xb.double().permute(0, 3, 1, 2), wt.to(torch.bfloat16).double()
    ref = F.conv2d(xd, wd, padding=1)
    mag = F.conv2d(xd.abs(), wd.abs(), padding=1)
    if full:
        s, b = torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g) * 0.1
        e1 = (ops.pad_vec(s.cuda(), wp.shape[0], 1.0), ops.pad_vec(b.cuda(), wp.shape[0], 0.0))
        ref = ref * s.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1)
        mag = mag * s.double().view(1, -1, 1, 1) + b.double().abs().view(1, -1, 1, 1)
        ref = F.relu(ref)                                                 # 1-Lipschitz: the bound holds after it
    rows = lambda v: v.permute(0, 2, 3, 1).reshape(B * h * w, c_out)
    return buf.cuda()[:, :c_in], wp, e1, rows(ref), rows(mag)


def _consume(name, binding="torch"):
    from bts_amd import ops
    B, h, w, c_in, c_out, full = CONSUMER[name]
    x2d, wp, e1, _, _ = _consumer_case(name)
    ybuf = torch.full((B * h * w, c_out + 24), float("nan"), device="cuda")
    y = ybuf[:, 8:8 + c_out]
    plane = ops._derived_weight(wp, "_bts_round1", ops.round_bf16)
    recs = _with_binding(binding, lambda: _traced(lambda: ops.conv3x3_bf16in_forward(
        x2d, B, h, w, c_in, plane, c_out, y, e1=e1, act=ops.ACT_RELU if full else ops.ACT_NONE)))
    assert torch.isnan(ybuf[:, :8]).all() and torch.isnan(ybuf[:, 8 + c_out:]).all(), name        # only the slice is written
    return y.clone(), recs


@pytest.mark.parametrize("name", sorted(ELIGIBLE))
def test_consumer_is_bit_for_bit_todays_bf16_halo_tile(name):
    from bts_amd import ops
    B, h, w, c_in, c_out, full = CONSUMER[name]
    x2d, wp, e1, _, _ = _consumer_case(name)
    x32 = x2d.float().contiguous()
    bn = ops.conv_plan.bf16in_3x3_tile(c_out)
    ybuf = torch.full((B * h * w, c_out + 24), float("nan"), device="cuda")
    y_ref = ybuf[:, 8:8 + c_out]
    with ops.launch_config(fill_frames=16, precision="bf16"):
        today = _traced(lambda: ops.conv_forward(x32, B, h, w, wp, c_out, 3, c_in_ld=c_in, e1=e1, act=ops.ACT_RELU if full else ops.ACT_NONE,
                                                 y2d=y_ref))
    # ops.conv_plan (bts_conv_plan_f32 on the call's own descriptor) names today's path: BTS_CONV_KIND_HALO_BF16
    assert [r[0] for r in today] == ["conv_halo_emu_kernel<%d,k3,bf16>" % bn], today
    got, recs = _consume(name)
    assert [r[0] for r in recs] == ["conv3x3_bf16in_kernel<%d>" % bn], recs
    assert recs[0][2] == 2.0 * B * h * w * c_in + 4.0 * B * h * w * c_out + 2.0 * 9 * c_out * c_in     # the bf16 tensor: 2 bytes
    assert torch.isfinite(got).all()
    assert torch.equal(got, y_ref), (name, float((got - y_ref).abs().max()))
    assert torch.equal(got, _consume(name, "ctypes")[0]), name


@pytest.mark.parametrize("name", sorted(CONSUMER))
def test_consumer_meets_the_modes_fp64_bound(name):
    """Products are exact products of the bf16 inputs and the RNE-rounded weights and sum in fp32:
    |got - ref| <= 2e-6 * sum|terms| + 2^-22 |ref| per output (tests/test_conv_tail_bf16_gpu.py's bound)."""
    _, _, _, ref, mag = _consumer_case(name)
    got = _consume(name)[0].cpu().double()
    assert torch.isfinite(got).all(), name
    bound = 2e-6 * mag + 2.0 ** -22 * ref.abs()
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    print(name, "worst err / bound:", worst)
    assert worst <= 1.0, (name, worst)


def test_consumer_wrapper_refuses_what_the_kernel_does_not_take():
    from bts_amd import ops
    from bts_amd._lib import BtsHipError
    x = torch.zeros((128, 64), dtype=torch.bfloat16, device="cuda")
    y = torch.zeros((128, 48), device="cuda")
    w = torch.zeros((1, 64, 9 * 64), dtype=torch.int16, device="cuda")
    with pytest.raises(BtsHipError):
        ops.conv3x3_bf16in_forward(x.float(), 1, 4, 32, 64, w, 48, y)                             # an fp32 input
    with pytest.raises(BtsHipError):
        ops.conv3x3_bf16in_forward(x, 1, 4, 32, 64, w, 48, y, act=ops.ACT_SIGMOID)
    with pytest.raises(BtsHipError):
        ops.conv3x3_bf16in_forward(x, 1, 4, 32, 48, w, 48, y)                                     # c_in % 32
    with pytest.raises(BtsHipError):
        ops.conv3x3_bf16in_forward(x[:, 2:], 1, 4, 32, 32, w[:, :, :288].contiguous(), 48, y)     # a 4-byte aligned base
    with pytest.raises(BtsHipError):
        ops.conv3x3_bf16in_forward(x, 1, 4, 32, 64, w, 48, y, e1=(torch.ones(48, device="cuda"), torch.zeros(48, device="cuda")))
    with pytest.raises(BtsHipError):
        ops.conv1x1_bf16_forward(torch.zeros((40, 64), device="cuda"), 40, 64, torch.zeros((1, 192, 64), dtype=torch.int16, device="cuda"),
                                 192, torch.zeros((40, 194), dtype=torch.bfloat16, device="cuda")[:, 1:193])   # a 2-byte aligned slice


# ------------------------------------------------------------------------------------------------------------------- model
# The smallest input at which, at fill_frames 16, a layer of block 2 takes BOTH queries: the wide 1x1 tile wants a declared
# launch of 512 workgroups, 16 x ceil(h w / 128) >= 512, i.e. more than 31 x 128 = 3968 pixels on block 2's map (H/8 x W/8, both
# multiples of 4), and the halo tile wants 4x32 tiles that are 0.80 real pixels: 64 x 64 = 4096 is the smallest such map, a
# 512 x 512 image (block 1, 128 x 128, then takes both as well; blocks 3 and 4 neither).  One frame.
H_IMG = W_IMG = 512
FILL = 16


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
    from bts_amd import bts as M
    torch.manual_seed(23)
    m = M.BtsModel(Params("densenet161_bts", 512, 80.0, "kitti")).eval()
    _randomise_bn(m, 9)
    m = m.cuda()
    m.fill_frames = FILL
    g = torch.Generator().manual_seed(5)
    x = torch.rand((1, 3, H_IMG, W_IMG), generator=g).cuda()
    f = torch.tensor([715.0873]).cuda()
    return m, x, f


def _forward(m, x, f, mid, prec="bf16", wide=True):
    m.bf16_mid_storage, m.bf16_wide_1x1, m.conv_precision = mid, wide, prec
    try:
        with torch.no_grad():
            return [o.clone() for o in m(x, f)]
    finally:
        m.bf16_mid_storage, m.bf16_wide_1x1, m.conv_precision = False, False, "fp32"


def _mid_tags(recs):
    return sorted(r[1] for r in recs if r[1].endswith("_mid16"))


def test_model_outputs_do_not_change_by_a_bit():
    from bts_amd import ops
    m, x, f = _model()
    with ops.launch_config(fill_frames=FILL, precision="bf16"):
        both = [ops.conv1x1_bf16_plan(H_IMG >> s, W_IMG >> s, 192, 192).eligible and
                ops.conv3x3_bf16in_plan(H_IMG >> s, W_IMG >> s, 192, 48).eligible for s in (2, 3, 4, 5)]
    assert both == [True, True, False, False], both
    off = _forward(m, x, f, False)                       # the model's first bf16 forward: the weight planes are made here
    on = _forward(m, x, f, True)
    k_on = _traced(lambda: _forward(m, x, f, True))
    k_off = _traced(lambda: _forward(m, x, f, False))
    # the switch moved layers of block 1 and of block 2, each as a (producer, consumer) pair, and nothing else
    tags = _mid_tags(k_on)
    n1, n2 = tags.count("enc_b1_1x1_mid16"), tags.count("enc_b2_1x1_mid16")
    print("bf16 mid layers: block 1", n1, "block 2", n2)
    assert n1 > 0 and n2 > 0, tags
    assert tags.count("enc_b1_3x3_mid16") == n1 and tags.count("enc_b2_3x3_mid16") == n2 and len(tags) == 2 * (n1 + n2), tags
    assert not _mid_tags(k_off)
    assert len(k_on) == len(k_off)
    moved = sorted(set((a[0], b[0]) for a, b in zip(k_off, k_on) if a[0] != b[0]))
    assert moved == [("conv1x1_bf16_kernel<192>", "conv1x1_bf16_ybf16_kernel<192>"),
                     ("conv_halo_emu_kernel<64,k3,bf16>", "conv3x3_bf16in_kernel<64>")], moved
    for i in range(6):
        assert torch.isfinite(on[i]).all()
        assert torch.equal(on[i], off[i]), ("bf16, bf16_wide_1x1", i)
    # ignored by the other precisions and without the wide tile
    for prec, wide in (("fp32", True), ("bf16x3", True), ("bf16", False)):
        a, b = _forward(m, x, f, False, prec, wide), _forward(m, x, f, True, prec, wide)
        assert not _mid_tags(_traced(lambda: _forward(m, x, f, True, prec, wide))), (prec, wide)
        for i in range(6):
            assert torch.equal(a[i], b[i]), (prec, wide, i)


def test_encoder_taps_do_not_change_by_a_bit():
    from bts_amd import ops
    from bts_amd.encoder_hip import DenseNetHip
    m, x, _ = _model()
    plan = DenseNetHip(m.encoder.base_model)
    plan.bf16_wide_1x1 = True
    taps = {}
    with ops.launch_config(fill_frames=FILL, precision="bf16"), torch.no_grad():
        for mid in (False, True, False):
            plan.bf16_mid_storage = mid
            taps[mid] = [t.clone() for t in plan.taps_nchw(x)]
            ws = plan._workspace(1, H_IMG, W_IMG, x.device)
            assert ("mid_bf16" in ws) == (True in taps)               # allocated when the switch is first used, then kept
    assert ws["mid_bf16"].dtype == torch.bfloat16 and ws["mid_bf16"].shape == ws["mid"].shape
    for i, (a, b) in enumerate(zip(taps[False], taps[True])):
        assert torch.equal(a, b), i


def test_graphs_key_on_the_switch():
    from bts_amd.graph import GraphedModel
    m, x, f = _model()
    eager = _forward(m, x, f, False)
    gm = GraphedModel(m)
    try:
        first = None
        for mid in (False, True, True, False):
            m.bf16_mid_storage, m.bf16_wide_1x1, m.conv_precision = mid, True, "bf16"
            with torch.no_grad():
                got = [o.clone() for o in gm(x, f)]
            torch.cuda.synchronize()
            first = got if first is None else first
            for i in range(6):
                assert torch.equal(got[i], eager[i]), ("graph", mid, i)
        assert gm.captures == 2                          # the flip captured again, the flip back replayed the first capture
        for i in range(6):
            assert torch.equal(got[i], first[i]), i
    finally:
        m.bf16_mid_storage, m.bf16_wide_1x1, m.conv_precision = False, False, "fp32"


def test_plans_refuse_the_switch_in_bf16_mode():
    from bts_amd._lib import BtsHipError
    m, x, f = _model()
    m.use_plans = True
    try:
        with pytest.raises(BtsHipError, match="bf16_mid_storage"):
            _forward(m, x, f, True)
    finally:
        m.use_plans = False
