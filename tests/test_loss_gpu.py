"""GPU: the native training losses (csrc/loss.hip through ops.depth_loss / silog_loss(native=True) /
depth_l1_loss(native=True)) against the reference formulas in FLOAT64 ON THE CPU with autograd -- never the code under
test, never the fp32 torch loss.

Tolerances follow from the arithmetic, not from a measurement: the kernels compute in fp64 from the fp32 inputs and
round once to fp32 (2^-24 = 6e-8 relative), so the loss is held to rtol 5e-7 and each gradient element to
|g - g64| <= 5e-7 |g64| + 1e-9 max|g64| (the absolute term covers elements where d - vf * mean(d) cancels).  Gradients at
invalid pixels are exactly 0."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from bts_amd import synth
from oracle import bts_oracle as O
from parity_util import CONFIGS, TRAIN_CASE, Params, make_inputs, t

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1, 1, 1), (1, 1, 7, 9), (2, 1, 33, 61), (3, 1, 353, 517)]
LARGE = SHAPES[3]
KINDS = [("silog", 0.85), ("silog", 1.0), ("l1", 1), ("l1", 2.5)]
GT_MIN = 1.0


@functools.lru_cache(maxsize=None)
def inputs(shape, use_mask=True, seed=0):
    """train_targets-style case: gt uniform in (0.5, 80), ~70 % valid, est = gt * U(0.5, 1.6).  Returns CPU fp32
    (est, gt, valid) -- shared, never modified.  ``use_mask=False``: the invalid pixels carry gt = 0 (as missing lidar
    returns do) and validity is the rule gt > GT_MIN, which also drops the few valid pixels nearer than 1 m."""
    B, _, H, W = shape
    gt, mask = synth.train_targets(B, H, W, 80.0, seed=1000 + seed + H * W)
    rng = np.random.Generator(np.random.PCG64(2000 + seed + H * W))
    if gt.size == 1:
        gt[...] = 7.5
        mask[...] = True
    ratio = rng.uniform(0.5, 1.6, size=gt.shape)
    if gt.size == 1:
        ratio[...] = 1.3 + 0.1 * seed            # n = 1: v = (1 - vf) d^2 = 0.15 * log(1.3)^2 = 1.0e-2, clear of the clamp
    est = (gt * ratio).astype(np.float32)
    if not use_mask:
        gt = np.where(mask, gt, np.float32(0.0)).astype(np.float32)
        mask = gt > GT_MIN
    return t(est), t(gt), t(mask)


def ref_loss64(est64, gt64, valid, kind, param):
    """The reference formulas (pytorch/bts.py:41-63), written for any float dtype."""
    if kind == "silog":
        return O.silog_loss(est64, gt64, valid, param)
    err = est64[valid] - gt64[valid]
    if param == 1:
        return err.abs().mean()
    return torch.where(err > 0, param * err, -err).sum() / err.numel()


@functools.lru_cache(maxsize=None)
def reference(shape, use_mask, kind, param, seed=0):
    """(loss64, grad64 [shape], v64) of the fp64 CPU reference; loss 0 / zero gradient in the documented case v <= 0."""
    est, gt, valid = inputs(shape, use_mask, seed)
    e64 = est.double().requires_grad_(True)
    g64 = gt.double()
    v = None
    if kind == "silog":
        d = (e64[valid].log() - g64[valid].log()).detach()
        v = float((d ** 2).mean() - param * d.mean() ** 2)
        if v <= 0.0:
            return 0.0, torch.zeros_like(g64), v
    loss = ref_loss64(e64, g64, valid, kind, param)
    loss.backward()
    return float(loss.detach()), e64.grad, v


def criterion(kind, param):
    from bts_amd import bts as M
    return M.silog_loss(param, native=True) if kind == "silog" else M.depth_l1_loss(param, native=True)


def run_native(est, gt, valid, use_mask, kind, param, scale=None):
    """Forward + backward of the native criterion on device tensors: (loss 0-d, grad, stats, criterion)."""
    est = est.detach().requires_grad_(True)
    crit = criterion(kind, param)
    loss = crit(est, gt, valid, gt_min=GT_MIN) if use_mask else crit(est, gt, None, gt_min=GT_MIN)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), est.grad, crit.last_stats, crit


def check_loss(loss, loss64):
    got = float(loss)
    print("loss %.9g, fp64 reference %.12g" % (got, loss64))
    assert abs(got - loss64) <= 5e-7 * abs(loss64), (got, loss64)


def check_grad(g, g64, valid, scale=1.0):
    g = g.detach().cpu()
    g64 = g64 * scale
    assert g.shape == g64.shape and g.dtype == torch.float32
    assert bool((g[~valid] == 0).all()), "gradient at an invalid pixel is not exactly 0"
    err = (g.double() - g64).abs()
    bound = 5e-7 * g64.abs() + 1e-9 * g64.abs().max()
    print("gradient: max |g - g64| %.3g, max |g64| %.3g" % (float(err.max()), float(g64.abs().max())))
    assert bool((err <= bound).all()), "max excess %g" % float((err - bound).max())


def misaligned(x):
    """x's values in a contiguous view that starts one element into its buffer: 4-byte (float) / 1-byte (mask) offset."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
    buf[1:].copy_(x.reshape(-1))
    v = buf[1:1 + x.numel()].view(x.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == x.element_size()
    return v


@pytest.mark.parametrize("use_mask", [True, False], ids=["mask", "gt_min"])
@pytest.mark.parametrize("kind,param", KINDS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_vs_fp64_reference(shape, kind, param, use_mask):
    est, gt, valid = inputs(shape, use_mask)
    loss64, g64, v = reference(shape, use_mask, kind, param)
    if kind == "silog" and param == 0.85:
        assert v > 1e-3, "this case would sit on the variance clamp: v = %g" % v
    loss, g, stats, _ = run_native(est.cuda(), gt.cuda(), valid.cuda(), use_mask, kind, param)
    stats = stats.cpu()
    assert stats.dtype == torch.float64 and int(stats[0]) == int(valid.sum())
    assert float(stats[3]) == pytest.approx(loss64, rel=2e-7, abs=0.0)         # fp64, but `param` crosses the C ABI as fp32
    if shape == (1, 1, 1, 1) and kind == "silog" and param == 1.0:
        # n = 1, vf = 1: v = d^2 - d^2 = 0 -- the documented case, loss 0 and a zero gradient (torch: 0 and NaN)
        assert v == 0.0 and float(loss) == 0.0 and bool((g == 0).all())
        return
    check_loss(loss, loss64)
    check_grad(g, g64, valid)
    # an upstream gradient other than 1 reaches the backward kernel as a device scalar
    _, g3, _, _ = run_native(est.cuda(), gt.cuda(), valid.cuda(), use_mask, kind, param, scale=3.0)
    check_grad(g3, g64, valid, scale=3.0)


@pytest.mark.parametrize("kind,param", KINDS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [SHAPES[2], LARGE], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_base_pointers(shape, kind, param):
    """est, gt and mask each start one element into their buffer (contiguous, 4-byte / 1-byte offset): the 16-byte
    loads begin three pixels in, the head and the tail go one element per lane.  Also a mask alone that does not share
    est's offset (the scalar path) -- same bars."""
    est, gt, valid = inputs(shape, True)
    loss64, g64, _ = reference(shape, True, kind, param)
    e, g, m = misaligned(est.cuda()), misaligned(gt.cuda()), misaligned(valid.cuda())
    loss, grad, _, _ = run_native(e, g, m, True, kind, param)
    check_loss(loss, loss64)
    check_grad(grad, g64, valid)
    loss, grad, _, _ = run_native(e, g, valid.cuda(), True, kind, param)          # mask aligned, est / gt not: no common split
    check_loss(loss, loss64)
    check_grad(grad, g64, valid)
    loss, grad, _, _ = run_native(e, g, None, False, kind, param)                  # no mask: rule gt > GT_MIN on the same maps
    assert np.isfinite(float(loss))


def test_non_contiguous_estimate_gets_its_gradient_in_its_own_shape():
    shape = SHAPES[2]
    est, gt, valid = inputs(shape, True)
    loss64, g64, _ = reference(shape, True, "silog", 0.85)
    base = est.cuda().transpose(2, 3).contiguous().requires_grad_(True)           # [B,1,W,H] leaf
    view = base.transpose(2, 3)                                                  # est's values, not contiguous
    assert not view.is_contiguous()
    loss = criterion("silog", 0.85)(view, gt.cuda(), valid.cuda())
    loss.backward()
    check_loss(loss.detach(), loss64)
    assert base.grad.shape == base.shape
    check_grad(base.grad.transpose(2, 3), g64, valid)


@pytest.mark.parametrize("use_mask", [True, False], ids=["mask", "gt_min"])
@pytest.mark.parametrize("kind,param", [("silog", 0.85), ("l1", 2.5)], ids=lambda v: str(v))
def test_poisoned_invalid_pixels_change_nothing(kind, param, use_mask):
    """est in {0, -1, NaN, +inf} and gt in {0, NaN} at the invalid pixels: loss, stats and gradient are finite and bit-equal
    to the same case with benign values there.  One VALID pixel with est = NaN makes the loss NaN, as in torch."""
    shape = SHAPES[2]
    est, gt, valid = inputs(shape, use_mask)
    inv = (~valid).reshape(-1).nonzero().reshape(-1)
    assert inv.numel() > 100
    pe, pg = est.clone().reshape(-1), gt.clone().reshape(-1)
    pe[inv] = torch.tensor([0.0, -1.0, float("nan"), float("inf")]).repeat(inv.numel() // 4 + 1)[:inv.numel()]
    pg[inv] = torch.tensor([0.0, float("nan")]).repeat(inv.numel() // 2 + 1)[:inv.numel()]
    pe, pg = pe.view(shape), pg.view(shape)
    a = run_native(est.cuda(), gt.cuda(), valid.cuda(), use_mask, kind, param)
    b = run_native(pe.cuda(), pg.cuda(), valid.cuda(), use_mask, kind, param)
    assert np.isfinite(float(b[0])) and bool(torch.isfinite(b[1]).all())
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    check_loss(b[0], reference(shape, use_mask, kind, param)[0])
    first_valid = int(valid.reshape(-1).nonzero()[0])
    pe.view(-1)[first_valid] = float("nan")
    c = run_native(pe.cuda(), pg.cuda(), valid.cuda(), use_mask, kind, param)
    assert np.isnan(float(c[0]))


@pytest.mark.parametrize("kind,param", [("silog", 0.85), ("l1", 1)], ids=lambda v: str(v))
def test_empty_mask_gives_zero_loss_and_zero_gradient(kind, param):
    est, gt, valid = inputs(SHAPES[2], True)
    none = torch.zeros_like(valid)
    loss, g, stats, crit = run_native(est.cuda(), gt.cuda(), none.cuda(), True, kind, param)
    assert float(loss) == 0.0 and bool((g == 0).all())
    assert float(crit.last_stats[0]) == 0.0 and crit.last_stats is stats
    # the rule form: no gt above the threshold
    loss, g, stats, crit = run_native(est.cuda(), (gt * 0.0 + 0.5).cuda(), None, False, kind, param)
    assert float(loss) == 0.0 and bool((g == 0).all()) and float(crit.last_stats[0]) == 0.0


def test_reference_pinned_loss_of_the_golden_training_step(golden_dir):
    """est = the reference's own final_depth of the committed training step, gt / mask = its targets: the native silog
    must land on the loss the reference recorded (its fp32 value, 9.7602596; the fp64 formula on these arrays gives
    9.760259665, 3.8e-9 relative from it -- the bar is one fp32 rounding plus that distance)."""
    g = np.load(os.path.join(golden_dir, "decoder_train.npz"))
    est = t(g["out_final_depth"])
    gt, mask = synth.train_targets(2, 64, 96, 80.0, seed=77)
    assert int(mask.sum()) == 8577
    loss, _, stats, _ = run_native(est.cuda(), t(gt).cuda(), t(mask).cuda(), True, "silog", 0.85)
    print("native %.9g, recorded %.9g" % (float(loss), float(g["loss"])))
    assert int(stats[0]) == 8577
    assert abs(float(loss) - float(g["loss"])) <= 5e-7 * float(g["loss"])


def test_two_runs_are_bit_equal():
    est, gt, valid = inputs(LARGE, True)
    e, g, m = est.cuda(), gt.cuda(), valid.cuda()
    for kind, param in (("silog", 0.85), ("l1", 2.5)):
        a = run_native(e, g, m, True, kind, param)
        b = run_native(e, g, m, True, kind, param)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _binding_leg(path=None):
    """loss, stats and gradient of two cases through whichever binding this process uses (saved to ``path`` if given)."""
    out = []
    for shape, use_mask, kind, param in ((SHAPES[2], True, "silog", 0.85), (SHAPES[2], False, "l1", 2.5)):
        est, gt, valid = inputs(shape, use_mask)
        loss, g, stats, _ = run_native(est.cuda(), gt.cuda(), valid.cuda(), use_mask, kind, param, scale=3.0)
        out += [loss.cpu(), stats.cpu(), g.cpu()]
    if path is not None:
        torch.save(out, path)
    return out


def test_torch_operator_and_ctypes_binding_are_bit_equal():
    from bts_amd import ops
    tops = ops.torch_ops()
    assert tops is not None, "this test compares the default (torch operator) binding with a BTS_BINDING=ctypes child"
    got = _binding_leg()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); from bts_amd import ops; assert ops.torch_ops() is None; "
            "import test_loss_gpu as T; T._binding_leg(sys.argv[1])" % (os.path.dirname(HERE), HERE))
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "o.pt")
        subprocess.run([sys.executable, "-c", code, out], env=dict(os.environ, BTS_BINDING="ctypes"), check=True, timeout=120)
        other = torch.load(out, weights_only=True)
    assert len(got) == len(other) == 6
    for a, b in zip(got, other):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                                                  b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))
    # the operator's own argument checks
    est, gt, valid = (x.cuda() for x in inputs(SHAPES[1], True))
    with pytest.raises(RuntimeError, match="est must be float32"):
        tops.depth_loss(est.double(), gt, valid, 1.0, 0, 0.85)
    with pytest.raises(RuntimeError, match="gt must be a CUDA"):
        tops.depth_loss(est, gt.cpu(), valid, 1.0, 0, 0.85)
    with pytest.raises(RuntimeError, match="must have the same shape"):
        tops.depth_loss(est, gt[:, :, :5], valid, 1.0, 0, 0.85)
    with pytest.raises(RuntimeError, match="mask must be bool or uint8"):
        tops.depth_loss(est, gt, valid.float(), 1.0, 0, 0.85)
    with pytest.raises(RuntimeError, match="kind must be 0"):
        tops.depth_loss(est, gt, valid, 1.0, 2, 0.85)
    with pytest.raises(ops.BtsHipError, match="est and gt must be contiguous"):
        ops._op(lambda: tops.depth_loss(est.transpose(2, 3), gt.transpose(2, 3), None, 1.0, 0, 0.85))


def test_native_step_does_not_wait_for_the_device():
    """Under torch's sync debug mode the reference formulation raises on its boolean gather (``nonzero`` waits for the
    device); the native forward + backward raises nothing."""
    from bts_amd import bts as M
    est, gt, valid = (x.cuda() for x in inputs(SHAPES[2], True))
    run_native(est, gt, valid, True, "silog", 0.85)                              # library load, autograd registration
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            M.silog_loss(0.85)(est, gt, valid)
            raised = False
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("this torch build does not raise on the mask gather under set_sync_debug_mode('error')")
        e = est.detach().requires_grad_(True)
        crit = M.silog_loss(0.85, native=True)
        crit(e, gt, valid).backward()
        e2 = est.detach().requires_grad_(True)
        (2.0 * M.depth_l1_loss(2.5, native=True)(e2, gt, None, gt_min=GT_MIN)).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    check_grad(e.grad, reference(SHAPES[2], True, "silog", 0.85)[1], inputs(SHAPES[2], True)[2])
    assert int(crit.last_stats[0]) == int(valid.sum())


def test_forward_is_capturable_in_a_graph():
    """Warm-up on a side stream, capture the native forward (one linear stream), refill the static inputs with a second
    case, replay: the loss is bit-equal to the eager loss of the second case."""
    from bts_amd import ops
    shape = SHAPES[2]
    first = [x.cuda() for x in inputs(shape, True, seed=0)]
    second = [x.cuda() for x in inputs(shape, True, seed=1)]
    assert not torch.equal(first[0], second[0])
    static = [x.clone() for x in first]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        ops.depth_loss(static[0], static[1], static[2], GT_MIN, "silog", 0.85)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        loss, stats = ops.depth_loss(static[0], static[1], static[2], GT_MIN, "silog", 0.85, return_stats=True)
    for s, x in zip(static, second):
        s.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        eager, eager_stats = ops.depth_loss(second[0], second[1], second[2], GT_MIN, "silog", 0.85, return_stats=True)
        eager_first = ops.depth_loss(first[0], first[1], first[2], GT_MIN, "silog", 0.85)
    assert float(eager) != float(eager_first)
    assert torch.equal(loss.view(torch.int32), eager.view(torch.int32))
    assert torch.equal(stats.view(torch.int64), eager_stats.view(torch.int64))


def _fresh_train_decoder():
    from bts_amd import bts as M
    enc, md, ds, _, _ = CONFIGS[TRAIN_CASE["cname"]]
    feat = synth.ENCODER_CHANNELS[enc]
    dec = M.bts(Params(enc, 512, md, ds), feat, 512)
    sd = {k: (torch.tensor(v) if np.ndim(v) == 0 else t(v)) for k, v in synth.decoder_state(feat, 512, 0).items()}
    dec.load_state_dict(sd, strict=True)
    return dec.train().cuda()


def test_trainer_step_with_native_loss_matches_the_torch_criterion():
    """trainer.train_step on the decoder-training configuration (K channel plan, 2x64x96), once with the native silog and
    mask=None (the rule gt > 1.0 applied in the kernel), once with the torch criterion and the explicit mask, from the
    same initial state.  Loss within rtol 2e-6 (the torch side is fp32: its own distance to fp64 dominates); every
    parameter gradient within 1e-4 of the largest gradient element, the bar the one-step decoder-training tests hold
    against the oracle."""
    from bts_amd import bts as M, trainer
    c = TRAIN_CASE
    _, md, _, _, _ = CONFIGS[c["cname"]]
    feats, focal = make_inputs(c["cname"], c["B"], c["H"], c["W"], c["feat_seed"])
    gt, mask = synth.train_targets(c["B"], c["H"], c["W"], md, c["target_seed"])
    gt = t(np.where(mask, gt, np.float32(0.0)).astype(np.float32)).cuda()         # invalid pixels: no lidar return
    rule = gt > 1.0

    def step(crit, m):
        dec = _fresh_train_decoder()
        opt = torch.optim.SGD(dec.parameters(), lr=1e-6)
        fs = [None] + [f.cuda().requires_grad_(True) for f in feats[1:]]
        loss, outs = trainer.train_step(dec, opt, crit, fs, focal.cuda(), gt, mask=m, dataset="kitti")
        torch.cuda.synchronize()
        # every parameter of the decoder takes part in the step: a missing gradient (None) fails right here
        return float(loss.detach()), {n: p.grad.detach().cpu() for n, p in dec.named_parameters()}

    native = M.silog_loss(c["variance_focus"], native=True)
    loss_n, g_n = step(native, None)
    loss_t, g_t = step(M.silog_loss(c["variance_focus"]), rule)
    assert int(native.last_stats[0]) == int(rule.sum())
    print("loss native %.9g torch %.9g" % (loss_n, loss_t))
    assert abs(loss_n - loss_t) <= 2e-6 * abs(loss_t)
    assert g_n.keys() == g_t.keys() and len(g_t) > 0
    r = max(float((g_n[k] - g_t[k]).abs().max()) for k in g_t)
    s = max(float(g_t[k].abs().max()) for k in g_t)
    print("max |g_native - g_torch| %.3g, max |g_torch| %.3g" % (r, s))
    assert r <= 1e-4 * s
