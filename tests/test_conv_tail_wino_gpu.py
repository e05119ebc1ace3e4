"""GPU: the fused Winograd conv1 kernel (csrc/conv_wino_tail.inc, ops.conv_tail_wino_forward) -- exact integer cases against
fp64, float cases beside the halo kernel, propagation of a non-finite plane value, plan record / replay, and the decoder
with conv1 on it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity_util import OUT_NAMES, build_hip_decoder, make_inputs

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 1, "elu": 2}
KERNEL = "conv_wino_tail_kernel<32>"
GUARD = 64                      # floats in front of and behind the NCHW result
POISON = -12345.0


def _reference(x, planes, wt, act):
    """fp64 conv3x3([x | planes]) -> activation, [B, 32, h, w]."""
    ref = F.conv2d(torch.cat([x, planes], 1).double(), wt.double(), padding=1)
    return torch.relu(ref) if act == "relu" else F.elu(ref) if act == "elu" else ref


def _operands(x, planes):
    B, c, h, w = x.shape
    x2d = x.permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous().cuda()
    return x2d, [planes[:, j].contiguous().cuda() for j in range(planes.shape[1])]


def _run_wino(x, planes, wt, act, trace=None):
    """The new op on NCHW host tensors: the result [B, 32, h, w] on the host and the whole poisoned buffer around it."""
    from bts_amd import ops
    B, _, h, w = x.shape
    n_tail = planes.shape[1]
    x2d, pl = _operands(x, planes)
    u, wtail = ops.pack_conv_tail_wino(wt.cuda(), n_tail)
    buf = torch.full((2 * GUARD + B * 32 * h * w,), POISON, device="cuda")
    y = buf[GUARD:GUARD + B * 32 * h * w].view(B, 32, h, w)
    ops.set_trace(trace)
    try:
        ops.conv_tail_wino_forward(x2d, B, h, w, u, wtail, pl, y, act=ACTS[act])
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    return y.cpu(), buf


def _run_halo(x, planes, wt, act):
    """The halo kernel (ops.conv_forward with tail_planes, NCHW result) on the same operands."""
    from bts_amd import ops
    B, _, h, w = x.shape
    x2d, pl = _operands(x, planes)
    wp = ops.pack_conv_weight(wt.cuda(), c_in_ld=36)[0]
    y = torch.zeros((B, 32, h, w), device="cuda")
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        with ops.launch_config(fill_frames=16, precision="fp32"):
            ops.conv_forward(x2d, B, h, w, wp, 32, 3, act=ACTS[act], y_nchw=y, tail_planes=pl)
    finally:
        ops.set_trace(None)
    kern = sorted(tr.summary())
    assert len(kern) == 1 and kern[0].startswith("conv_halo_kernel"), kern
    return y.cpu()


EXACT_CASES = [
    # B, h, w, n_tail, act
    (1, 4, 32, 4, "none"),       # exactly one tile
    (1, 3, 5, 4, "relu"),        # smaller than a tile, odd
    (2, 7, 33, 4, "none"),       # ragged both ways, single last row / column
    (3, 8, 64, 1, "relu"),
    (1, 6, 40, 0, "none"),
]


@pytest.mark.parametrize("B,h,w,n_tail,act", EXACT_CASES, ids=lambda v: str(v))
def test_exact_integer_cases(B, h, w, n_tail, act):
    """Integer x and planes (|.| <= 127), weights in {-1, 0, 1}: U is in quarters (|U| <= 9/4), V sums four inputs, a
    transform position sums 32 channels, an output nine positions, the tail 36 products: everything stays an integer
    below 2^24 in quarter units, so the kernel must reproduce the fp64 reference bit for bit -- inside a poisoned
    buffer whose guard bands stay untouched, and frame by frame independent of B."""
    g = torch.Generator().manual_seed(1000 * h + w + n_tail)
    x = torch.randint(-127, 128, (B, 32, h, w), generator=g).float()
    planes = torch.randint(-127, 128, (B, n_tail, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (32, 32 + n_tail, 3, 3), generator=g).float()
    xmax = max(float(x.abs().max()), float(planes.abs().max()) if n_tail else 0.0)
    bound = 9 * (32 * 9 * 4 * xmax) + 4 * 36 * xmax                  # quarter units
    assert bound < 2 ** 24, bound
    ref = _reference(x, planes, wt, act).float()
    got, buf = _run_wino(x, planes, wt, act)
    assert torch.equal(got, ref), "max |diff| %g" % float((got - ref).abs().max())
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[-GUARD:] == POISON).all())
    if B > 1:
        one, _ = _run_wino(x[B - 1:], planes[B - 1:], wt, act)
        assert torch.equal(one[0], got[B - 1])


@pytest.mark.parametrize("shape", [(2, 44, 152), (1, 40, 70)])
def test_float_vs_fp64_beside_the_halo_kernel(shape):
    """randn operands, ELU, four planes: error relative to max|ref| against fp64, beside the halo kernel's on the same
    operands.  The project's Winograd bars (test_winograd_kernel_vs_fp64_and_direct): <= max(1e-5, 4 x the direct
    kernel's), and both kernels within 2e-5 of each other."""
    from bts_amd import ops
    B, h, w = shape
    g = torch.Generator().manual_seed(h + w)
    x = torch.randn((B, 32, h, w), generator=g)
    planes = torch.randn((B, 4, h, w), generator=g)
    wt = torch.randn((32, 36, 3, 3), generator=g) / np.sqrt(36 * 9.0)
    ref = _reference(x, planes, wt, "elu")
    tr = ops.KernelTrace()
    got, _ = _run_wino(x, planes, wt, "elu", trace=tr)
    summ = tr.summary()
    assert sorted(summ) == [KERNEL] and set(summ[KERNEL]["tags"]) == {"decoder_conv"}
    assert summ[KERNEL]["flops"] == 2.0 * B * h * w * 36 * 9 * 32
    halo = _run_halo(x, planes, wt, "elu")
    scale = ref.abs().max().item()
    err_wino, err_halo = (got.double() - ref).abs().max().item() / scale, (halo.double() - ref).abs().max().item() / scale
    between = (got - halo).abs().max().item() / halo.abs().max().item()
    print(shape, "max error / max|ref|: winograd %.3g, halo %.3g; between the two %.3g" % (err_wino, err_halo, between))
    assert err_wino <= max(1e-5, 4 * err_halo), (err_wino, err_halo)
    assert between <= 2e-5, between


def test_one_infinite_plane_value_reaches_its_nine_outputs_only():
    """+inf at one interior pixel of one plane: outputs outside its 3x3 neighbourhood are bit-identical to the run without
    it; inside, the inf / NaN pattern equals the halo kernel's (the tail runs in direct form in both)."""
    B, h, w, py, px = 1, 12, 40, 5, 17
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, 32, h, w), generator=g)
    planes = torch.randn((B, 4, h, w), generator=g)
    wt = torch.randn((32, 36, 3, 3), generator=g) / np.sqrt(36 * 9.0)
    clean, _ = _run_wino(x, planes, wt, "elu")
    planes[0, 2, py, px] = float("inf")
    got, _ = _run_wino(x, planes, wt, "elu")
    halo = _run_halo(x, planes, wt, "elu")
    inside = torch.zeros((B, 32, h, w), dtype=torch.bool)
    inside[:, :, py - 1:py + 2, px - 1:px + 2] = True
    assert torch.equal(got[~inside], clean[~inside])
    assert bool(torch.isfinite(clean).all())
    gi, hi = got[inside], halo[inside]
    assert torch.equal(torch.isnan(gi), torch.isnan(hi))
    assert torch.equal(torch.isposinf(gi), torch.isposinf(hi)) and torch.equal(torch.isneginf(gi), torch.isneginf(hi))
    assert not bool(torch.isfinite(gi).all())                          # the value did arrive
    fin = torch.isfinite(gi)
    assert torch.allclose(gi[fin], hi[fin], rtol=0, atol=1e-5)         # ELU(-inf) = -1 in both


def test_it_is_recorded_and_replayed_by_a_plan():
    """bts_amd/plan.py records the new entry point like every other launch (BTS_OP_CONV_TAIL_WINO) and bts_plan_run replays
    it into another output tensor, bit for bit."""
    from bts_amd import _lib, ops, plan
    B, h, w = 2, 9, 40
    g = torch.Generator().manual_seed(7)
    x2d = torch.randn((B * h * w, 32), generator=g).cuda()
    pl = [torch.randn((B, h, w), generator=g).cuda() for _ in range(4)]
    u, wtail = ops.pack_conv_tail_wino(torch.randn((32, 36, 3, 3), generator=g).cuda(), 4)
    direct, rec_out, replay = (torch.zeros((B, 32, h, w), device="cuda") for _ in range(3))
    ops.conv_tail_wino_forward(x2d, B, h, w, u, wtail, pl, direct)
    rec = plan._Recorder()
    with _lib.recording(plan._Proxy(_lib.load_real(), rec)):
        ops.conv_tail_wino_forward(x2d, B, h, w, u, wtail, pl, rec_out)
    assert [c[0] for c in rec.calls] == ["bts_conv_tail_wino_fwd_f32"] and not rec.foreign
    stream = torch.cuda.current_stream().cuda_stream
    p = plan.Plan(rec.calls, [x2d, rec_out, pl[1]], stream)
    assert p.n_ops == 1 and p.ops[0].kind == 14 and p.n_patches == 3
    p.run([x2d, replay, pl[1]], stream)
    torch.cuda.synchronize()
    assert torch.equal(rec_out, direct) and torch.equal(replay, direct)


def test_conv1_in_the_decoder(golden_dir):
    """One KITTI frame (352x1216, the input of the golden full-size samples) through the decoder with a chip-filling launch
    declared: conv1 runs the new kernel once under decoder_conv and the halo tail kernel is gone; with the switch off the
    reverse; the six outputs match the switch-off forward and the golden samples within the decoder tests' tolerances."""
    import os
    from bts_amd import ops
    from bts_amd import bts as M
    gold = np.load(os.path.join(golden_dir, "decoder_full_samples.npz"))
    dec = build_hip_decoder("K")
    dec.fill_frames = 16
    feats, focal = make_inputs("K", 1, 352, 1216, 1234)
    feats = [None] + [f.cuda() for f in feats[1:]]
    HALO = "conv_halo_kernel<32,k3,nchw,tail>"

    def run():
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            with torch.no_grad():
                outs = [o.clone() for o in dec(feats, focal.cuda())]
        finally:
            ops.set_trace(None)
        return outs, tr.summary()

    assert M.bts.conv1_wino
    got, kern = run()
    assert kern[KERNEL]["launches"] == 1 and set(kern[KERNEL]["tags"]) == {"decoder_conv"}
    assert HALO not in kern
    M.bts.conv1_wino = False
    try:
        ref, kern_off = run()
    finally:
        M.bts.conv1_wino = True
    assert KERNEL not in kern_off and kern_off[HALO]["launches"] == 1
    for i, name in enumerate(OUT_NAMES):
        g, r = got[i].cpu().double().numpy(), ref[i].cpu().double().numpy()
        if i < 3:
            # the LPG maps by the rule of test_decoder_full_size_vs_golden_samples (conv1 runs after them: they must not move)
            idx, val = gold["K_%s_idx" % name], gold["K_%s_val" % name]
            keep = gold["K_%s_absden" % name] > 2e-3
            assert keep.mean() > 0.99
            gs, rs = g.reshape(-1)[idx][keep], r.reshape(-1)[idx][keep]
            rel = np.abs(gs - rs) / np.maximum(np.abs(rs), 1e-30)
            rel_gold = np.abs(gs - val[keep]) / np.maximum(np.abs(val[keep]), 1e-30)
            assert rel.max() <= 1e-4, (name, rel.max())
            assert rel_gold.max() <= 1e-4, (name, rel_gold.max())
        elif i < 5:
            idx, val = gold["K_%s_idx" % name], gold["K_%s_val" % name]
            rel = (np.abs(g - r) / np.maximum(np.abs(r), 1e-30)).max()
            rel_gold = (np.abs(g.reshape(-1)[idx] - val) / np.maximum(np.abs(val), 1e-30)).max()
            print(name, "max rel vs switch off %.3g, vs golden %.3g" % (rel, rel_gold))
            assert rel <= 1e-4 and rel_gold <= 1e-4, name
        else:
            idx, val = gold["K_%s_idx" % name], gold["K_%s_val" % name]
            print(name, "max |diff| vs switch off %.3g, vs golden %.3g" % (np.abs(g - r).max(), np.abs(g.reshape(-1)[idx] - val).max()))
            assert (np.abs(g - r) <= 1e-4 + 1e-3 * np.abs(r)).all(), name
            assert (np.abs(g.reshape(-1)[idx] - val) <= 1e-4 + 1e-3 * np.abs(val)).all(), name
