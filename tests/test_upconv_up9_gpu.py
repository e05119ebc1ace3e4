"""GPU: the shared-patch F(2x2,2x2) upconv kernel (csrc/conv_up9.inc, ops.upconv_up9_forward) -- exact integer cases
against fp64, float cases beside the sub-pixel halo kernel, and the decoder with the three eligible upconvs on it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity_util import OUT_NAMES, build_hip_decoder, make_inputs

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 1, "elu": 2}


def _reference(x, wt, act, e2):
    """fp64 conv3x3(nearest2x(x)) -> activation -> e2 affine, [B, c_out, 2h, 2w]."""
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), wt.double(), padding=1)
    if act == "relu":
        ref = torch.relu(ref)
    elif act == "elu":
        ref = F.elu(ref)
    if e2 is not None:
        ref = ref * e2[0].double().view(1, -1, 1, 1) + e2[1].double().view(1, -1, 1, 1)
    return ref


def _run_up9(x, wt, act, e2, off=16, guard=32, trace=None):
    """The new op on NCHW host tensors: the result [B, c_out, 2h, 2w] on the host and the whole (wider) output buffer."""
    from bts_amd import ops
    B, cin, h, w = x.shape
    cout = wt.shape[0]
    x2d = x.permute(0, 2, 3, 1).reshape(B * h * w, cin).contiguous().cuda()
    u = ops.pack_upconv_up9(wt.cuda())
    ybuf = torch.zeros((4 * B * h * w, cout + guard), device="cuda")
    y = ybuf[:, off:off + cout]
    e2d = None if e2 is None else (e2[0].cuda(), e2[1].cuda())
    ops.set_trace(trace)
    try:
        ops.upconv_up9_forward(x2d, B, h, w, u, cin, cout, y, act=ACTS[act], e2=e2d)
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    return y.reshape(B, 2 * h, 2 * w, cout).permute(0, 3, 1, 2).cpu(), ybuf


EXACT_CASES = [
    # B, h, w, c_in, c_out, act, e2
    (1, 3, 5, 32, 32, "none", False),        # smaller than one workgroup tile
    (1, 8, 16, 64, 64, "relu", True),        # exactly one tile of source pixels; two chunks, two channel tiles
    (2, 7, 15, 96, 32, "none", True),        # odd, ragged both ways; three chunks
    (3, 9, 33, 32, 128, "relu", False),      # odd, ragged both ways; four channel tiles (upconv3's split over workgroups)
    (1, 16, 32, 96, 64, "none", False),      # even: the last window row / column gives a single output row / column
    (2, 16, 32, 128, 128, "relu", True),     # four chunks x four channel tiles
]


@pytest.mark.parametrize("B,h,w,cin,cout,act,with_e2", EXACT_CASES, ids=lambda v: str(v))
def test_up9_exact_integer_cases(B, h, w, cin, cout, act, with_e2):
    """Integer x (|x| <= 127), weights in {-1, 0, 1}: every U (<= 9 weights), V (<= 4 inputs), channel sum and 4-term
    output transform stays an integer below 2^24, so the kernel must reproduce the fp64 reference bit for bit -- through
    a 16-channel-offset slice of a wider buffer whose guard columns stay zero, and frame by frame independent of B."""
    g = torch.Generator().manual_seed(1000 * cin + cout + h)
    x = torch.randint(-127, 128, (B, cin, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float()
    bound = 144.0 * cin * float(wt.abs().max()) * float(x.abs().max())
    assert bound < 2 ** 24, bound
    e2 = None
    if with_e2:                                      # powers of two (and a sign): the affine stays exact
        e2 = (torch.tensor([2.0, -0.5, 4.0, 0.25]).repeat(cout // 4), torch.tensor([1.0, -2.0, 0.0, 8.0]).repeat(cout // 4))
    ref = _reference(x, wt, act, e2).float()
    got, ybuf = _run_up9(x, wt, act, e2)
    assert torch.equal(got, ref), "max |diff| %g" % float((got - ref).abs().max())
    assert float(ybuf[:, :16].abs().max()) == 0.0 and float(ybuf[:, 16 + cout:].abs().max()) == 0.0      # only the slice is written
    if B > 1:
        one, _ = _run_up9(x[B - 1:], wt, act, e2)
        assert torch.equal(one[0], got[B - 1])


@pytest.mark.parametrize("cin,cout,shape", [(128, 128, (2, 44, 152)), (64, 32, (1, 40, 70))])
def test_up9_float_vs_fp64_beside_the_halo_kernel(cin, cout, shape):
    """randn operands, ELU + e2: error relative to max|ref| against fp64, beside the sub-pixel halo kernel's on the same
    inputs.  The project's bar for this operation: <= 1e-5, and <= 3 x the halo kernel's error + 2e-7."""
    from bts_amd import ops
    B, h, w = shape
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn((B, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, 3, 3), generator=g) / np.sqrt(cin * 9.0)
    e2 = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1)
    ref = _reference(x, wt, "elu", e2)
    tr = ops.KernelTrace()
    got, _ = _run_up9(x, wt, "elu", e2, trace=tr)
    assert sorted(tr.summary()) == ["conv_up9_kernel<32>"]
    errs = {"up9": (got.double() - ref).abs().max().item() / ref.abs().max().item()}
    x2d = x.permute(0, 2, 3, 1).reshape(B * h * w, cin).contiguous().cuda()
    wp = ops.pack_upconv_subpixel(wt.cuda())[0]
    y = torch.zeros((4 * B * h * w, cout), device="cuda")
    with ops.launch_config(fill_frames=16, precision="fp32"):
        ops.conv_forward(x2d, B, h, w, wp, cout, 3, up=2, act=ops.ACT_ELU, e2=(e2[0].cuda(), e2[1].cuda()), y2d=y, subpixel=True)
    halo = y.reshape(B, 2 * h, 2 * w, cout).permute(0, 3, 1, 2).cpu().double()
    errs["halo"] = (halo - ref).abs().max().item() / ref.abs().max().item()
    print((cin, cout, shape), errs)
    assert errs["up9"] <= 1e-5 and errs["halo"] <= 1e-5, errs
    assert errs["up9"] <= 3.0 * errs["halo"] + 2e-7, errs


def test_up9_in_the_decoder(golden_dir):
    """One KITTI frame (352x1216, the input of the golden full-size samples) through the decoder with a chip-filling launch
    declared: upconv3 / 2 / 1 run the new kernel (KernelTrace), and the six outputs match the same forward with the new
    form switched off within the tolerances the decoder's oracle tests use."""
    import os
    from bts_amd import ops
    gold = np.load(os.path.join(golden_dir, "decoder_full_samples.npz"))
    from bts_amd import bts as M
    dec = build_hip_decoder("K")
    dec.fill_frames = 16
    feats, focal = make_inputs("K", 1, 352, 1216, 1234)
    feats = [None] + [f.cuda() for f in feats[1:]]

    def run():
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            with torch.no_grad():
                outs = [o.clone() for o in dec(feats, focal.cuda())]
        finally:
            ops.set_trace(None)
        return outs, tr.summary()

    assert M.upconv.up9
    got, kern = run()
    assert kern["conv_up9_kernel<32>"]["launches"] == 3 and set(kern["conv_up9_kernel<32>"]["tags"]) == {"decoder_upconv"}
    M.upconv.up9 = False
    try:
        ref, kern_off = run()
    finally:
        M.upconv.up9 = True
    assert "conv_up9_kernel<32>" not in kern_off
    for i, name in enumerate(OUT_NAMES):
        g, r = got[i].cpu().double().numpy(), ref[i].cpu().double().numpy()
        if i < 3:
            # the LPG maps by the rule of test_decoder_full_size_vs_golden_samples: the golden file holds, for this very
            # input, 4096 sampled pixels per map with |denominator| of the reference's own plane equations; pixels with
            # |denominator| <= 2e-3 are set aside (more than 99 % must remain), every other sample within 1e-4 relative --
            # against the form-off forward, and against the reference's recorded values themselves
            idx, val = gold["K_%s_idx" % name], gold["K_%s_val" % name]
            keep = gold["K_%s_absden" % name] > 2e-3
            assert keep.mean() > 0.99
            gs, rs = g.reshape(-1)[idx][keep], r.reshape(-1)[idx][keep]
            rel = np.abs(gs - rs) / np.maximum(np.abs(rs), 1e-30)
            rel_gold = np.abs(gs - val[keep]) / np.maximum(np.abs(val[keep]), 1e-30)
            print(name, "kept %.4f of %d samples" % (keep.mean(), idx.size), "max rel vs form off %.3g" % rel.max(),
                  "vs golden %.3g" % rel_gold.max(), "(whole map, vs form off: %.3g)" % (np.abs(g - r) / np.maximum(np.abs(r), 1e-30)).max())
            assert rel.max() <= 1e-4, (name, rel.max())
            assert rel_gold.max() <= 1e-4, (name, rel_gold.max())
        elif i < 5:
            assert (np.abs(g - r) / np.maximum(np.abs(r), 1e-30)).max() <= 1e-4, name
        else:
            assert (np.abs(g - r) <= 1e-4 + 1e-3 * np.abs(r)).all(), name


def test_up9_is_recorded_and_replayed_by_a_plan():
    """bts_amd/plan.py records the new entry point like every other launch (BTS_OP_UPCONV_UP9) and bts_plan_run replays it
    into another output tensor, bit for bit."""
    from bts_amd import _lib, ops, plan
    B, h, w, cin, cout = 2, 9, 20, 64, 64
    g = torch.Generator().manual_seed(7)
    x2d = torch.randn((B * h * w, cin), generator=g).cuda()
    u = ops.pack_upconv_up9(torch.randn((cout, cin, 3, 3), generator=g).cuda())
    e2 = (torch.rand(cout, generator=g).cuda() + 0.5, torch.randn(cout, generator=g).cuda())
    direct, rec_out, replay = (torch.zeros((4 * B * h * w, cout), device="cuda") for _ in range(3))
    ops.upconv_up9_forward(x2d, B, h, w, u, cin, cout, direct, e2=e2)
    rec = plan._Recorder()
    with _lib.recording(plan._Proxy(_lib.load_real(), rec)):
        ops.upconv_up9_forward(x2d, B, h, w, u, cin, cout, rec_out, e2=e2)
    assert [c[0] for c in rec.calls] == ["bts_upconv_up9_fwd_f32"] and not rec.foreign
    stream = torch.cuda.current_stream().cuda_stream
    p = plan.Plan(rec.calls, [x2d, rec_out], stream)
    assert p.n_ops == 1 and p.ops[0].kind == 12 and p.n_patches == 2
    p.run([x2d, replay], stream)
    torch.cuda.synchronize()
    assert torch.equal(rec_out, direct) and torch.equal(replay, direct)
