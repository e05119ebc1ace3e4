"""GPU: the planar-tail 3x3 convolution with bf16 main operands and an fp32 tail (bts_conv_tail_bf16_fwd_f32,
csrc/conv_tail_bf16.inc) and the decoder switch that sends conv3 / conv2 there (``bf16_tail_convs``).  The entry
point is called directly, so the plan query's thresholds do not limit the shapes."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bts_amd import synth
from parity_util import OUT_NAMES, Params, build_hip_decoder, hip_run, oracle_run, singular_masks, t

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("BTS_CONV_PRECISION", "0").strip() == "1",
                                 reason="BTS_CONV_PRECISION=1 forces precision 1 inside every scope")]

# name: (B, c_main, c_out, h, w, options).  The smallest shapes at which each mechanism can fail.
CASES = {
    "one_chunk": (1, 32, 128, 7, 33, {}),                                     # single-chunk pipeline, H % 4 != 0, one-pixel last tile column
    "two_chunks": (2, 64, 64, 12, 40, {}),                                    # frame offset of the plane, partial tile, BN 64
    "odd_chunks_strided_x": (2, 224, 128, 8, 64, {"xs": 232, "act": "elu"}),  # x_pix_stride 232, ELU, BN 128
    "narrow_map": (1, 160, 64, 5, 31, {"act": "elu", "e2": True}),            # W < tile width, ELU + e2
    "two_channel_tiles": (1, 64, 96, 8, 32, {"cout_pad": 128}),               # second n-tile half filled, pad rows beyond c_out
    "tail_only": (1, 32, 64, 9, 35, {"x0": True}),                            # x = 0: the fp32 tail alone
    "range": (1, 64, 64, 8, 32, {"xscale": 2.0 ** 40, "wscale": 2.0 ** -40}),  # as test_bf16_gpu's scale_2^40
}


def _rne(v):
    return v.float().to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of a case and its fp64 reference, made once: conv of the RNE-rounded main input and weights plus conv of the
    unrounded plane with the unrounded tail weights, then act / e2; ``mag`` = sum |terms| of an output, tail included."""
    B, c_main, cout, h, w, o = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    xs, ws = o.get("xscale", 1.0), o.get("wscale", 1.0)
    x = torch.randn((B, c_main, h, w), generator=g) * xs
    if o.get("x0"):
        x = torch.zeros_like(x)
    plane = (torch.randn((B, 1, h, w), generator=g) * 1.7 + 0.3) * xs      # not bf16-representable
    wt = torch.randn((cout, c_main + 1, 3, 3), generator=g) / np.sqrt(9.0 * (c_main + 1)) * ws
    act = {"elu": 2, "relu": 1}.get(o.get("act"), 0)
    e2 = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1) if o.get("e2") else None
    xr, wr = _rne(x), _rne(wt[:, :c_main])
    pre = F.conv2d(xr, wr, padding=1) + F.conv2d(plane.double(), wt[:, c_main:].double(), padding=1)
    mag = F.conv2d(xr.abs(), wr.abs(), padding=1) + F.conv2d(plane.double().abs(), wt[:, c_main:].double().abs(), padding=1)
    ref = {2: F.elu, 1: F.relu}.get(act, lambda v: v)(pre)
    if e2 is not None:                                   # the activations are 1-Lipschitz: the terms of an output scale with |s|
        ref = ref * e2[0].double().view(1, -1, 1, 1) + e2[1].double().view(1, -1, 1, 1)
        mag = mag * e2[0].double().abs().view(1, -1, 1, 1)
    return dict(x=x, plane=plane, wt=wt, act=act, e2=e2, ref=ref, mag=mag)


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


def _run(name, binding=None, frames=None):
    """The case through ops.conv_tail_bf16_forward into a channel slice of a NaN-filled buffer; ``frames``: a (first, count)
    sub-batch.  Returns (output [b, cout, h, w] fp64 on the CPU, kernel names, the raw output slice)."""
    from bts_amd import ops
    B, c_main, cout, h, w, o = CASES[name]
    c = _case(name)
    f0, b = frames if frames else (0, B)
    x, plane = c["x"][f0:f0 + b], c["plane"][f0:f0 + b]
    xstride = o.get("xs", c_main)
    xbuf = torch.full((b * h * w, xstride), float("nan"))                      # channels past c_main are never read
    xbuf[:, :c_main] = x.permute(0, 2, 3, 1).reshape(b * h * w, c_main)
    x2d = xbuf.cuda()[:, :c_main]
    w_main, w_tail = ops.pack_conv_tail_bf16(c["wt"].cuda(), 1)
    if o.get("cout_pad"):                                                      # rows beyond round_up(c_out, 32): zero, read, never stored
        pad = o["cout_pad"]
        wm = torch.zeros((pad, w_main.shape[1]), dtype=torch.bfloat16, device="cuda")
        wm[:w_main.shape[0]] = w_main
        wtl = torch.zeros((pad, 9, 4), device="cuda")
        wtl[:w_tail.shape[0]] = w_tail
        w_main, w_tail = wm, wtl
    ybuf = torch.full((b * h * w, cout + 32), float("nan"), device="cuda")
    y = ybuf[:, 16:16 + cout]
    e2 = tuple(v.cuda() for v in c["e2"]) if c["e2"] is not None else None
    pl = plane.reshape(b, h, w).contiguous().cuda()

    def go():
        ops.conv_tail_bf16_forward(x2d, b, h, w, w_main, w_tail, pl, c_main, cout, y, act=c["act"], e2=e2)

    old = ops._BINDING
    if binding is not None:
        ops._BINDING = binding
    try:
        kern = _traced(go)
    finally:
        ops._BINDING = old
    assert torch.isnan(ybuf[:, :16]).all() and torch.isnan(ybuf[:, 16 + cout:]).all(), name      # only the slice is written
    return y.reshape(b, h, w, cout).permute(0, 3, 1, 2).cpu().double(), kern, y.clone()


def _worst(got, ref, mag):
    """max over outputs of |got - ref| / (2e-6 * sum|terms| + 2^-22 * |ref|): tests/test_bf16_gpu.py's bound."""
    bound = 2e-6 * mag + 2.0 ** -22 * ref.abs()
    return float(((got - ref).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_on_rounded_main_operands_and_an_fp32_tail(name):
    """Main products are exact products of RNE-rounded operands, the tail is nine unrounded fp32 FMAs, everything sums in
    fp32: |got - ref| <= 2e-6 * sum|terms| + 2^-22 |ref| per output.  In the tail-only case (x = 0, plane values that are
    not bf16-representable) sum|terms| is the tail's alone: a tail rounded to bf16 (2^-9 of its terms) or shifted by a pixel
    fails it."""
    got, kern, _ = _run(name)
    c = _case(name)
    cout = CASES[name][2]
    assert kern == ["conv_tail_bf16_kernel<%d>" % (128 if cout >= 128 else 64)], kern
    assert torch.isfinite(got).all(), name
    worst = _worst(got, c["ref"], c["mag"])
    print(name, kern, "worst err / bound:", worst)
    assert worst <= 1.0, (name, worst)


def test_fp32_tail_kernel_misses_this_reference():
    """Control for the bound: the fp32 planar-tail path (ops.conv_forward with tail_planes, what precision 2 runs for these
    layers without the switch) on the two-chunk case misses the rounded-operand reference by more than the bound."""
    from bts_amd import ops
    name = "two_chunks"
    B, c_main, cout, h, w, _ = CASES[name]
    c = _case(name)
    x2d = c["x"].permute(0, 2, 3, 1).reshape(B * h * w, c_main).contiguous().cuda()
    wp = ops.pack_conv_weight(c["wt"].cuda(), c_in_ld=c_main + 4)[0]
    y = torch.empty((B * h * w, cout), device="cuda")
    with ops.launch_config(fill_frames=16, precision="fp32"):
        ops.conv_forward(x2d, B, h, w, wp, cout, 3, act=ops.ACT_NONE, y2d=y, tail_planes=[c["plane"].reshape(B, h, w).contiguous().cuda()])
    got = y.reshape(B, h, w, cout).permute(0, 3, 1, 2).cpu().double()
    worst = _worst(got, c["ref"], c["mag"])
    print("fp32 tail kernel, worst err / bound:", worst)
    assert worst > 1.0, worst
    # ... while it does compute this layer: against the UNROUNDED operands it is an fp32 convolution
    exact = F.conv2d(torch.cat([c["x"], c["plane"]], 1).double(), c["wt"].double(), padding=1)
    assert float((got - exact).abs().max()) <= 1e-4 * float(exact.abs().max())


def test_torch_op_equals_ctypes():
    for name in ("two_chunks", "narrow_map", "one_chunk"):
        a = _run(name, binding="torch")[2]
        b = _run(name, binding="ctypes")[2]
        assert torch.equal(a, b), name


def test_runs_are_deterministic():
    for name in ("odd_chunks_strided_x", "two_channel_tiles"):
        assert torch.equal(_run(name)[2], _run(name)[2]), name


def test_a_frame_has_the_same_bits_alone_and_in_a_batch():
    B, _, cout, h, w, _ = CASES["two_chunks"]
    both = _run("two_chunks")[2].reshape(B, h * w, cout)
    alone = _run("two_chunks", frames=(1, 1))[2].reshape(1, h * w, cout)
    assert torch.equal(alone[0], both[1])


def test_python_layer_refuses_what_the_kernel_does_not_take():
    from bts_amd import ops
    from bts_amd._lib import BtsHipError
    x = torch.zeros((8 * 32, 64), device="cuda")
    y = torch.zeros((8 * 32, 64), device="cuda")
    pl = torch.zeros((1, 8, 32), device="cuda")
    w_main, w_tail = ops.pack_conv_tail_bf16(torch.zeros(64, 65, 3, 3, device="cuda"), 1)
    with pytest.raises(BtsHipError):
        ops.conv_tail_bf16_forward(x, 1, 8, 32, w_main.float(), w_tail, pl, 64, 64, y)            # fp32 w_main
    with pytest.raises(BtsHipError):
        ops.conv_tail_bf16_forward(x, 1, 8, 32, w_main, w_tail, pl[:, :4], 64, 64, y)             # short plane
    with pytest.raises(BtsHipError):
        ops.conv_tail_bf16_forward(x, 1, 8, 32, w_main, w_tail, pl, 64, 64, y, act=ops.ACT_SIGMOID)


# ------------------------------------------------------------------------------------------------ decoder / model switch
H_IMG, W_IMG = 64, 128      # conv3 runs at 16x32 and conv2 at 32x64: full 4x32 tiles, the smallest input the plan query takes


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
    enc = "densenet161_bts"
    params = Params(enc, 512, 80.0, "kitti")
    torch.manual_seed(11)
    model = M.BtsModel(params).eval()
    _randomise_bn(model.encoder, 7)
    state_np = synth.decoder_state(synth.ENCODER_CHANNELS[enc], 512, 0)
    model.decoder.load_state_dict({k: (torch.tensor(v) if np.ndim(v) == 0 else t(v)) for k, v in state_np.items()})
    m = model.cuda()
    m.conv_precision = "bf16"
    m.fill_frames = 16
    x = torch.from_numpy(synth.image_batch(2, H_IMG, W_IMG, 5)).cuda()
    f = torch.from_numpy(synth.focal_values(2, params.dataset, 5)).cuda()
    return m, x, f


def _forward(m, x, f, on):
    m.bf16_tail_convs = on
    with torch.no_grad():
        return [o.clone() for o in m(x, f)]


NEW = ("conv_tail_bf16_kernel<128>", "conv_tail_bf16_kernel<64>")         # conv3 (c_out 128), conv2 (c_out 64)
OLD = ("conv_halo_kernel<128,k3,nhwc,tail>", "conv_halo_kernel<64,k3,nhwc,tail>")


def test_model_switch_moves_conv3_and_conv2_and_nothing_else():
    from bts_amd import ops
    m, x, f = _model()
    with ops.launch_config(fill_frames=16, precision="bf16"):
        assert ops.conv_tail_bf16_plan(H_IMG // 4, W_IMG // 4, 224, 128).eligible
        assert ops.conv_tail_bf16_plan(H_IMG // 2, W_IMG // 2, 160, 64).eligible
    try:
        off = _forward(m, x, f, False)
        on = _forward(m, x, f, True)
        k_off = _traced(lambda: _forward(m, x, f, False))
        k_on = _traced(lambda: _forward(m, x, f, True))
        off2 = _forward(m, x, f, False)
    finally:
        m.bf16_tail_convs = False
    n = k_off.count(OLD[0])
    assert n >= 1 and k_off.count(OLD[1]) == n and not any(k in k_off for k in NEW), sorted(set(k_off))
    assert k_on.count(NEW[0]) == n and k_on.count(NEW[1]) == n and not any(k in k_on for k in OLD), sorted(set(k_on))
    # every other launch is the same kernel in the same place (conv1 keeps its fp32 NCHW tail kernel)
    swap = dict(zip(OLD, NEW))
    assert [swap.get(k, k) for k in k_off] == k_on
    assert "conv_halo_kernel<32,k3,nchw,tail>" in k_on
    # off is the mode as it was: flipping the switch on and back reproduces its bits; on changes what follows conv3
    for i in range(6):
        assert torch.equal(off[i], off2[i]), i
    assert torch.equal(off[0], on[0])                        # depth_8x8 is computed before conv3
    assert not torch.equal(off[1], on[1]) and not torch.equal(off[5], on[5])
    # another declaration in the mode's other direction: fp32 never takes the new kernel
    m.conv_precision = "fp32"
    try:
        k32 = _traced(lambda: _forward(m, x, f, True))
    finally:
        m.conv_precision, m.bf16_tail_convs = "bf16", False
    assert not any(k in k32 for k in NEW)


def test_training_forward_never_takes_the_switch():
    from bts_amd._lib import BtsHipError
    m, x, f = _model()
    dec = m.decoder
    dec.bf16_tail_convs = True
    dec.train()
    try:
        with pytest.raises(BtsHipError):
            dec.forward_nhwc(None, 2, H_IMG, W_IMG, f, x, None, False)
    finally:
        dec.eval()
        dec.bf16_tail_convs = False


def test_plans_and_graphs_never_replay_the_other_setting():
    from bts_amd.graph import GraphedModel
    m, x, f = _model()
    try:
        eager = {on: _forward(m, x, f, on) for on in (False, True)}
        assert not torch.equal(eager[False][5], eager[True][5])
        m.use_plans = True
        before, counts = m._plans.recordings, []
        for on in (False, True, True, False):
            got = _forward(m, x, f, on)
            for i in range(6):
                assert torch.equal(got[i], eager[on][i]), ("plan", on, i)
            counts.append(m._plans.recordings - before)
        # one recording per sub-batch slot and setting: the first flip records again, flipping back replays
        assert counts[0] >= 1 and counts[1:] == [2 * counts[0]] * 3, counts
        m.use_plans = False
        gm = GraphedModel(m)
        for on in (False, True, True, False):
            m.bf16_tail_convs = on
            with torch.no_grad():
                got = [o.clone() for o in gm(x, f)]
            torch.cuda.synchronize()
            for i in range(6):
                assert torch.equal(got[i], eager[on][i]), ("graph", on, i)
        assert gm.captures == 2
    finally:
        m.use_plans = False
        m.bf16_tail_convs = False


# CPU estimate (scripts/bf16_tail_cpu_estimate.py, 2x64x128, seed 4321): every convolution of the bf16 mode on operands
# rounded by Tensor.to(torch.bfloat16), conv3 / conv2 main channels included, against the fp32 oracle; (median, max) relative
# change per depth map, near-singular LPG pixels masked.  The GPU is held to TWICE these (fp32 summation order; LPG amplifies
# pixels near the mask's edge).
CPU_ESTIMATE = {
    "K": {"depth_8x8_scaled": (7.549e-04, 7.067e-03), "depth_4x4_scaled": (1.555e-03, 9.148e-03),
          "depth_2x2_scaled": (7.393e-04, 1.015e-02), "reduc1x1": (7.915e-04, 7.201e-03), "final_depth": (6.506e-04, 6.854e-03)},
    "N": {"depth_8x8_scaled": (7.319e-04, 5.762e-03), "depth_4x4_scaled": (4.526e-04, 6.485e-03),
          "depth_2x2_scaled": (9.714e-04, 6.772e-03), "reduc1x1": (5.550e-04, 6.501e-03), "final_depth": (9.059e-04, 6.955e-03)},
}


@pytest.mark.parametrize("cname", ["K", "N"])
def test_decoder_accuracy_against_the_fp32_oracle(cname):
    """The decoder at 2x64x128 in bf16 mode with the switch on against the fp32 oracle: at most twice the CPU estimate."""
    dec = build_hip_decoder(cname, "cuda")
    dec.conv_precision, dec.fill_frames, dec.bf16_tail_convs = "bf16", 16, True
    kern = _traced(lambda: hip_run(dec, cname, 2, H_IMG, W_IMG, 4321))
    assert sum(k.startswith("conv_tail_bf16_kernel<") for k in kern) == 2, sorted(set(kern))
    got = hip_run(dec, cname, 2, H_IMG, W_IMG, 4321)
    ref_outs, inter = oracle_run(cname, 2, H_IMG, W_IMG, 4321)
    masks = singular_masks(inter, 2, H_IMG, W_IMG)
    bad = []
    for i, k in ((0, 8), (1, 4), (2, 2), (3, None), (4, None)):
        g = got[i].detach().cpu().double().numpy()
        r = ref_outs[i].double().numpy()
        msk = masks[k] if k else np.ones_like(r, dtype=bool)
        rel = np.abs(g[msk] - r[msk]) / np.maximum(np.abs(r[msk]), 1e-30)
        med, mx = float(np.median(rel)), float(rel.max())
        cmed, cmx = CPU_ESTIMATE[cname][OUT_NAMES[i]]
        print("%s %-18s median %.3e (bound %.3e)  max %.3e (bound %.3e)" % (cname, OUT_NAMES[i], med, 2 * cmed, mx, 2 * cmx))
        if med > 2 * cmed or mx > 2 * cmx:
            bad.append((OUT_NAMES[i], med, 2 * cmed, mx, 2 * cmx))
    assert not bad, bad
