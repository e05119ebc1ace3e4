"""GPU: the composite nodes of the training graph under train_precision "bf16" -- the fused dense block launch by launch,
its batched weight gradients, the sub-pixel upconv node, and the nodes that must keep their fp32 bits.

The dense block rounds values that are themselves computed (norm + ReLU of batch statistics, gradients that went through
earlier layers), so a statement of the whole block cannot be held to a per-element bound: a value within fp32 distance of
a rounding tie rounds the other way in fp64.  Each of its twelve convolution launches CAN: the launches are recorded with the
operands the GPU itself handed them (`recorded_launches`), and each result is held to the project's bf16 bound
2e-6 * sum|terms| (tests/test_bf16_gpu.py) of the fp64 statement on exactly those operands, rounded on the CPU.  The one
thing computed before the rounding inside a launch is the prologue x * scale + shift, which fp32 evaluates in one rounding
(fused) or two; the statement admits either, the same one for the whole launch."""
import copy

import pytest
import torch
import torch.nn.functional as F

import reduc_train_ref as RT
import train_bf16_ref as R
import train_node_cases as nc
from bts_amd import bts as M
from bts_amd import encoders as E
from bts_amd import ops, train
from conftest import fp32_only

pytestmark = [pytest.mark.gpu, fp32_only]

BF16_BOUND = 2e-6


class recorded_launches:
    """While active, every ops.conv_forward / ops.conv_wgrad call (train.py reaches them as attributes of `ops`, from the
    autograd thread too) is recorded with clones of its operands and of its result, and the arithmetic it was asked for."""

    def __enter__(self):
        self.calls = []
        self._cf, self._cw = ops.conv_forward, ops.conv_wgrad
        rec = self

        def pair(p):
            return None if p is None else (p[0].detach().clone().cpu(), p[1].detach().clone().cpu())

        def conv_forward(x2d, B, h, w, w_packed, c_out, ksize, **kw):
            x = x2d.detach().clone()
            out = rec._cf(x2d, B, h, w, w_packed, c_out, ksize, **kw)
            rec.calls.append(dict(kind="conv", tag=kw.get("tag"), x=x.cpu(), geom=(B, h, w), k=ksize, pre=pair(kw.get("pre")),
                                  pre_relu=bool(kw.get("pre_relu", False)), out=kw["y2d"].detach().clone().cpu(),
                                  precision=ops.current_launch_config()[1]))
            return out

        def conv_wgrad(x2d, B, h, w, c_in, dy2d, c_out, ksize, **kw):
            out = rec._cw(x2d, B, h, w, c_in, dy2d, c_out, ksize, **kw)
            rec.calls.append(dict(kind="wgrad", tag=kw.get("tag"), x=x2d.detach().clone().cpu(), dy=dy2d.detach().clone().cpu(),
                                  geom=(B, h, w), k=ksize, pre=pair(kw.get("pre")), pre_relu=bool(kw.get("pre_relu", False)),
                                  out=out.detach().clone().cpu(), precision=ops.wgrad_precision(kw.get("precision"))))
            return out

        ops.conv_forward, ops.conv_wgrad = conv_forward, conv_wgrad
        return self

    def __exit__(self, *exc):
        ops.conv_forward, ops.conv_wgrad = self._cf, self._cw
        return False


def _nchw(t2d, geom):
    B, h, w = geom
    return t2d.view(B, h, w, -1).permute(0, 3, 1, 2).contiguous()


def _prologue_variants(c):
    """The launch's gathered operand x' in fp64: one candidate without a prologue, else the two fp32 evaluations of
    [relu](x * scale + shift) -- fused (one rounding: exact in fp64, then rounded to fp32) and separate (two roundings)."""
    x = _nchw(c["x"], c["geom"])
    if c["pre"] is None:
        return [x.double()]
    s, b = (v.view(1, -1, 1, 1) for v in c["pre"])
    outs = [(x.double() * s.double() + b.double()).float(), x * s + b]
    if c["pre_relu"]:
        outs = [o.clamp_min(0.0) for o in outs]
    return [o.double() for o in outs]


def _ratio(got, ref, mag):
    return float(((got.double() - ref).abs() / (BF16_BOUND * mag + 2.0 ** -22 * ref.abs()).clamp_min(1e-300)).max())


def launch_ratio(c, weight, role):
    """max |launch result - rounded fp64 statement on the launch's own operands| / bound, the better of the admissible
    prologue evaluations.  role: "fwd" (y = conv(x', w)), "dgrad" (the launch's x is dy: dx = conv^T(dy, w)), "wgrad"."""
    k = c["k"]
    pad = (k // 2, k // 2)
    wr = R.rb(weight.detach().cpu().double())
    best = float("inf")
    for xv in _prologue_variants(c):
        xr = R.rb(xv)
        if role == "fwd":
            ref, mag = R._conv2d(xr, wr, None, 1, pad), R._conv2d(xr.abs(), wr.abs(), None, 1, pad)
            got = _nchw(c["out"], c["geom"])
        elif role == "dgrad":
            shape = (xr.shape[0], weight.shape[1], xr.shape[2], xr.shape[3])
            ref = torch.nn.grad.conv2d_input(shape, wr, xr, 1, pad)
            mag = torch.nn.grad.conv2d_input(shape, wr.abs(), xr.abs(), 1, pad)
            got = _nchw(c["out"], c["geom"])
        else:
            dy = R.rb(_nchw(c["dy"], c["geom"]).double())
            ref = torch.nn.grad.conv2d_weight(xr, wr.shape, dy, 1, pad)
            mag = torch.nn.grad.conv2d_weight(xr.abs(), wr.shape, dy.abs(), 1, pad)
            got = c["out"].view(wr.shape[0], k, k, wr.shape[1]).permute(0, 3, 1, 2)      # OHWI -> OIHW
        assert got.shape == ref.shape, (c["tag"], role, got.shape, ref.shape)
        best = min(best, _ratio(got, ref, mag))
    return best


def _block_step(block, x, gy, scope, batched=False, record=False):
    """One step of train._dense_block: (output, dx, {name: gradient}, recorded launches, [(kernel, tag)] of the trace)."""
    m = copy.deepcopy(block).cuda().train()
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tr = ops.KernelTrace()
    rec = recorded_launches() if record else None
    ops.set_trace(tr)
    try:
        if rec is not None:
            rec.__enter__()
        with train.precision_scope(scope):
            y = train._dense_block(m, xg, batched_wgrad=batched)
        assert y is not None
        y.backward(gy.cuda())
        torch.cuda.synchronize()
    finally:
        if rec is not None:
            rec.__exit__(None, None, None)
        ops.set_trace(None)
    kernels = [(r[0], r[1]) for r in tr.records if r[1].startswith("enc.")]
    return y.detach(), xg.grad, {n: p.grad for n, p in m.named_parameters()}, ([] if rec is None else rec.calls), kernels, m


def _block_case():
    gen = torch.Generator().manual_seed(11)
    block = E._DenseBlock(2, 64, 4, 32).train()
    nc.randomise(block, gen)
    return block, torch.randn(2, 64, 9, 13, generator=gen), torch.randn(2, 128, 9, 13, generator=gen)


def _expected_launches(m):
    """(tag, kind, role, weight) of the twelve convolution launches of a two-layer block in the order _DenseBlockFn issues them."""
    L = list(m.values())
    fwd = [("enc.fwd", "conv", "fwd", layer.conv1.weight) if j == 0 else ("enc.fwd", "conv", "fwd", layer.conv2.weight)
           for layer in L for j in (0, 1)]
    bwd = []
    for layer in reversed(L):
        bwd += [("enc.dgrad", "conv", "dgrad", layer.conv2.weight), ("enc.wgrad", "wgrad", "wgrad", layer.conv2.weight),
                ("enc.dgrad", "conv", "dgrad", layer.conv1.weight), ("enc.wgrad", "wgrad", "wgrad", layer.conv1.weight)]
    return fwd + bwd


def test_every_launch_of_the_dense_block_is_the_rounded_statement_on_its_own_operands():
    """Two layers of DenseNet121's first block (64 + 2 x 32 channels, 2 x 9 x 13, batch-statistic BN) through
    train._DenseBlockFn under train_precision "bf16": four forward, four input-gradient and four weight-gradient launches,
    each asked for precision 2, each a bf16 kernel in the trace, each within 2e-6 * sum|terms| of the rounded statement on the
    operands it was given.  The same twelve launches of the fp32 step miss that statement, every one: a pass left in fp32 -- a
    dropped scope, a missing precision= -- fails here by name."""
    block, x, gy = _block_case()
    for scope in ("bf16", "fp32"):
        _, _, _, calls, kernels, m = _block_step(block, x, gy, scope, record=True)
        want = _expected_launches(m)
        assert [(c["tag"], c["kind"]) for c in calls] == [(tag, kind) for tag, kind, _, _ in want]
        assert [tag for _, tag in kernels] == [tag for tag, _, _, _ in want]
        if scope == "bf16":
            assert all(c["precision"] == 2 for c in calls), [c["precision"] for c in calls]
            assert all("bf16" in kern for kern, _ in kernels), kernels
        else:
            assert all(c["precision"] == 0 for c in calls) and not any("bf16" in kern for kern, _ in kernels), kernels
        for i, (c, (tag, _, role, weight)) in enumerate(zip(calls, want)):
            r = launch_ratio(c, weight, role)
            print("%s launch %2d %-9s %s k%d: max |err| / bound %.4g" % (scope, i, tag, role, c["k"], r))
            if scope == "bf16":
                assert r <= 1.0, (i, tag, role, r)
            else:
                assert r > 1.0, ("the fp32 launch must miss the rounded statement", i, tag, role, r)


def test_batched_dense_block_has_the_bits_of_the_unbatched_bf16_block():
    """batched_wgrad under train_precision "bf16": ONE bts_conv_wgrad_batch_bf16_f32 launch for the block's four weight
    gradients.  At 234 pixels neither planner splits, and inside a tile every element sums its pixels in the same order
    whatever the tile, so output, dx and every parameter gradient have the bits of the unbatched bf16 block -- and not those
    of the batched fp32 block."""
    block, x, gy = _block_case()
    y, dx, g, _, kernels, _ = _block_step(block, x, gy, "bf16")
    yb, dxb, gb, _, kernels_b, _ = _block_step(block, x, gy, "bf16", batched=True)
    _, _, g32, _, kernels_32, _ = _block_step(block, x, gy, "fp32", batched=True)
    assert [k for k in kernels_b if "wgrad" in k[1]] == [("conv_wgrad_batch_kernel<bf16>", "enc.wgrad")]
    assert [k for k in kernels_32 if "wgrad" in k[1]] == [("conv_wgrad_batch_kernel", "enc.wgrad")]
    assert [k for k in kernels if "wgrad" in k[1]] == [("conv_wgrad_kernel<bf16>", "enc.wgrad")] * 4
    assert [k for k in kernels_b if "wgrad" not in k[1]] == [k for k in kernels if "wgrad" not in k[1]]
    assert torch.equal(yb, y) and torch.equal(dxb, dx)
    assert set(gb) == set(g)
    bad = [n for n in g if not torch.equal(gb[n], g[n])]
    assert not bad, bad
    convs = [n for n in g if n.endswith(("conv1.weight", "conv2.weight"))]
    assert len(convs) == 4 and all(not torch.equal(gb[n], g32[n]) for n in convs)


# ------------------------------------------------------------------------------------------ sub-pixel upconv node
def _class_weights(w):
    """g_(py,px)[ty][tx] of ops.pack_upconv_subpixel: the 3x3 taps a class tap covers, added in fp32, ky outer, kx inner."""
    sets = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    g = {}
    for py in (0, 1):
        for px in (0, 1):
            k = torch.zeros(w.shape[0], w.shape[1], 2, 2)
            for ty in (0, 1):
                for tx in (0, 1):
                    acc = None
                    for ky in sets[(py, ty)]:
                        for kx in sets[(px, tx)]:
                            acc = w[:, :, ky, kx] if acc is None else acc + w[:, :, ky, kx]
                    k[:, :, ty, tx] = acc
            g[(py, px)] = k
    return g


def _upconv_run(x, w, gy, scope):
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        with train.precision_scope(scope):
            y = train._UpconvFn.apply(xg, wg, "node")
        y.backward(gy.cuda())
        torch.cuda.synchronize()
    finally:
        ops.set_trace(None)
    return y.detach(), xg.grad, wg.grad, [(r[0], r[1]) for r in tr.records if r[1].startswith("node.")]


def test_subpixel_upconv_node_rounds_forward_and_input_gradient_and_keeps_its_fp32_weight_gradient():
    """train._UpconvFn (decoder.subpixel_upconv_train) under train_precision "bf16", 48 -> 40 channels, 2 x 5 x 7 -> 10 x 14.
    Forward: the four 2x2 class convolutions with x and the packed class weights (each a fp32 sum of 3x3 taps) rounded, then
    ELU (|ELU'| <= 1: the bound holds behind it).  Input gradient (bts_upconv_dgrad_f32, precision 2): dy' = ELU'(y) * gy --
    taken from the GPU's own y, so no rounding decision can differ -- and the class weights, both rounded.  Both within
    2e-6 * sum|terms|; the fp32 node misses both.  The weight gradient stays fp32: the bits of ops.upconv_wgrad on the same
    x and dy'."""
    gen = torch.Generator().manual_seed(5)
    Bn, cin, cout, h, w_ = 2, 48, 40, 5, 7
    x = torch.randn(Bn, cin, h, w_, generator=gen)
    w = torch.randn(cout, cin, 3, 3, generator=gen) / (cin * 9) ** 0.5
    gy = torch.randn(Bn, cout, 2 * h, 2 * w_, generator=gen)
    g = _class_weights(w)
    xp = F.pad(R.rb(x.double()), (1, 1, 1, 1))
    pre, mag = torch.zeros(Bn, cout, 2 * h, 2 * w_, dtype=torch.float64), torch.zeros(Bn, cout, 2 * h, 2 * w_, dtype=torch.float64)
    for (py, px), k in g.items():
        kr = R.rb(k.double())
        sl = xp[:, :, py:py + h + 1, px:px + w_ + 1]
        pre[:, :, py::2, px::2] = R._conv2d(sl, kr)
        mag[:, :, py::2, px::2] = R._conv2d(sl.abs(), kr.abs())
    results = {}
    for scope in ("bf16", "fp32"):
        y, dx, dw, kernels = _upconv_run(x, w, gy, scope)
        assert [tag for _, tag in kernels] == ["node.fwd", "node.dgrad", "node.wgrad"]
        assert kernels[2][0] == "upconv_wgrad_kernel" and ("bf16" in kernels[0][0]) == (scope == "bf16"), kernels
        r_fwd = float(((y.cpu().double() - F.elu(pre)).abs() / (BF16_BOUND * mag + 2.0 ** -22 * pre.abs())).max())
        # dx on the node's own dy'
        dyp = torch.ops.aten.elu_backward(gy.cuda(), 1.0, 1.0, 1.0, True, y)
        dr = R.rb(dyp.cpu().double())
        ref, rmag = torch.zeros(Bn, cin, h + 2, w_ + 2, dtype=torch.float64), torch.zeros(Bn, cin, h + 2, w_ + 2, dtype=torch.float64)
        for (py, px), k in g.items():
            kr = R.rb(k.double())
            shape = (Bn, cin, h + 1, w_ + 1)
            ref[:, :, py:py + h + 1, px:px + w_ + 1] += torch.nn.grad.conv2d_input(shape, kr, dr[:, :, py::2, px::2])
            rmag[:, :, py:py + h + 1, px:px + w_ + 1] += torch.nn.grad.conv2d_input(shape, kr.abs(), dr[:, :, py::2, px::2].abs())
        ref, rmag = ref[:, :, 1:-1, 1:-1], rmag[:, :, 1:-1, 1:-1]
        r_dx = _ratio(dx.cpu(), ref, rmag)
        print("%s: forward max |err| / bound %.4g, dx %.4g; kernels %s" % (scope, r_fwd, r_dx, kernels))
        # dw: the fp32 class gradients of the same operands
        x2d, _ = train._nhwc_rows(x.cuda().contiguous(memory_format=torch.channels_last))
        dy2d, _ = train._nhwc_rows(dyp)
        want = ops.upconv_wgrad(x2d, Bn, h, w_, cin, dy2d, cout, train._workspace(dx.device))
        assert torch.equal(dw, want.reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)), scope
        results[scope] = (r_fwd, r_dx)
    assert results["bf16"][0] <= 1.0 and results["bf16"][1] <= 1.0, results
    assert results["fp32"][0] > 1.0 and results["fp32"][1] > 1.0, ("the fp32 node must miss the rounded statement", results)


# ------------------------------------------------------------------------------------------ what stays fp32
def _reduc_modules(name):
    c_in, c_first, k = RT.CHAINS[name]
    x, ws, _, _, _ = RT.case_reference(name, RT.PLAIN_CASES[name])
    red = M.reduction_1x1(c_in, c_first, RT.MAX_DEPTH, is_final=(k == 0)).train().cuda()
    convs = [m for m in red.reduc.modules() if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        for m, wt in zip(convs, ws):
            m.weight.copy_(wt.cuda())
    return red, x, k


@pytest.mark.parametrize("name", ["8x8", "final"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layers"])
def test_reduction_nodes_keep_their_fp32_bits_under_the_scope(name, fused):
    """The reduction chains stay fp32 under train_precision "bf16": the fused nodes (train.fused_lpg_scale /
    fused_reduction_final) and the layer-by-layer graph (train.reduction_forward) give the same output, dx and weight
    gradients, bit for bit, inside and outside the scope."""
    red, x, k = _reduc_modules(name)
    outs = {}
    for scope in ("fp32", "bf16"):
        for p in red.parameters():
            p.grad = None
        xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        with train.precision_scope(scope):
            if not fused:
                out = train.reduction_forward(red, xd)
            elif k:
                out = train.fused_lpg_scale(red, M.local_planar_guidance(k), xd)
            else:
                out = train.fused_reduction_final(red, xd)
        gen = torch.Generator().manual_seed(3)
        out.backward(torch.randn(out.shape, generator=gen).cuda())
        torch.cuda.synchronize()
        outs[scope] = [out.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in red.parameters()]
    assert len(outs["fp32"]) == len(outs["bf16"]) > 3
    assert all(torch.equal(a, b) for a, b in zip(outs["fp32"], outs["bf16"]))
