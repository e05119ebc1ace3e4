"""The frozen-statistics norm kernels (csrc/bn_train.hip: bn_frozen_vectors_kernel, bn_frozen_bwd_kernel) against the fp64
statements of tests/bn_frozen_cases.py, through ops.bn_frozen_vectors / ops.bn_frozen_backward.

Conventions of tests/test_stream_kernels_gpu.py: inputs and outputs are channel slices of wider buffers, NaN around the
inputs (and in guard rows behind them), the non-integer SENTINEL around the outputs, a workspace exactly as long as the size
query says with a sentinel tail, every launch twice with the same bits.  The backward design is an integer one: dx is
compared bit for bit, the sums with torch.equal."""
import pytest
import torch

import bn_frozen_cases as fc
import stream_cases as sc
from bts_amd import ops
from test_conv_exact_gpu import SENTINEL
from test_stream_kernels_gpu import GUARD_ROWS, NAN, Wide, assert_tail, dev, twice, workspace

pytestmark = pytest.mark.gpu


# ================================================================================================== backward
def check_frozen_bwd(shape, relu, form):
    npix, C = shape
    what = "bn_frozen_backward %s relu=%s %s" % (shape, relu, form)
    x, dy, mean, invstd, scale, shift, dx_old = fc.frozen_bwd_case(npix, C)
    ref = fc.frozen_bwd_ref(x, dy, mean, invstd, scale, shift, dx_old, relu)
    sums = form in ("dx_sums", "sums", "accumulate_sums", "shared")
    acc = form in ("accumulate", "accumulate_sums")
    xin = Wide(npix, C, NAN, values=x, pre=1, post=GUARD_ROWS)
    also = ()
    if form == "shared":             # dx in the same wide buffer as dy, in other columns
        dxw = Wide(npix, C, SENTINEL, extra=C + 12, off=4)
        gin_view, dx_view = dxw.view, dxw.buf[:, C + 8:2 * C + 8]
        also = ((0, npix, C + 8, 2 * C + 8),)
    else:
        gin_view = Wide(npix, C, NAN, values=dy, pre=1, post=GUARD_ROWS).view
        dxw = None if form == "sums" else Wide(npix, C, SENTINEL, extra=16, pre=1, post=GUARD_ROWS)
        dx_view = None if dxw is None else dxw.view
    n = ops.bn_train_ws_floats(npix, C)
    ws, whole = workspace(n)
    vecs = [dev(v) for v in (mean, invstd, scale, shift)]
    old_d = dx_old.cuda()
    trace = ops.KernelTrace()

    def launch():
        whole.fill_(SENTINEL)
        if dxw is not None:
            dxw.reset()
        if form == "shared":
            gin_view.copy_(dy)
        if acc:
            dx_view.copy_(old_d)
        ops.set_trace(trace)
        try:
            dg, db = ops.bn_frozen_backward(xin.view, gin_view, C, vecs[0], vecs[1], vecs[2], vecs[3], relu,
                                            ws if sums else None, dx_view, sums=sums, accumulate=acc)
        finally:
            ops.set_trace(None)
        torch.cuda.synchronize()
        if sums:
            assert_tail(whole, n, what)
        else:
            assert dg is None and db is None
            assert bool((whole == SENTINEL).all()), what + ": no sums were asked for, yet the workspace was written"
        if dxw is not None:
            dxw.assert_outside_untouched(what, also=also)
        return ((dg, db) if sums else ()) + (() if dx_view is None else (dx_view,))

    got = twice(launch, what)
    assert [r[0] for r in trace.records] == ["bn_frozen_bwd_kernel"] * 2 and {r[1] for r in trace.records} == {"bn.frozen_bwd"}
    per_element = 8 + (4 if dx_view is not None else 0) + (4 if acc else 0)
    assert trace.records[0][3] == float(per_element) * npix * C, what + ": traced bytes"
    if sums:
        assert torch.equal(got[0].double(), ref["dgamma"]), what + ": dgamma"
        assert torch.equal(got[1].double(), ref["dbeta"]), what + ": dbeta"
    assert torch.equal(sc.bits(gin_view.cpu()), sc.bits(dy)) and torch.equal(sc.bits(xin.view.cpu()), sc.bits(x)), \
        what + ": an input changed"
    if dx_view is not None:
        want = (ref["dx_acc"] if acc else ref["dx"]).float()
        # bit for bit, the sign of a zero included: a negative scale times a masked dy' (+0) is -0 in fp64 and in the kernel
        assert torch.equal(got[-1], want), what + ": dx"
        assert torch.equal(sc.bits(got[-1]), sc.bits(want)), what + ": dx bits"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("form", fc.BWD_FORMS)
@pytest.mark.parametrize("shape", fc.BWD_SHAPES)
def test_bn_frozen_backward(shape, form, relu):
    check_frozen_bwd(shape, relu, form)


# =================================================================================================== vectors
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("C", fc.VEC_C)
def test_bn_frozen_vectors(C, affine):
    gamma, beta, rm, rv = fc.frozen_vectors_case(C)
    if not affine:
        gamma = beta = None
    g_d, b_d, rm_d, rv_d = dev(gamma), dev(beta), dev(rm), dev(rv)
    for eps in fc.VEC_EPS:
        for use_out in (False, True):
            what = "bn_frozen_vectors C=%d affine=%s eps=%g out=%s" % (C, affine, eps, use_out)
            ref, bound = fc.frozen_vectors_ref(gamma, beta, rm, rv, eps)

            def launch():
                slab = out = None
                if use_out:                      # the dense block's stats[i, 4:8, :mid]
                    slab = torch.full((8, C + 12), SENTINEL, device="cuda")
                    out = slab[4:8, :C]
                got = ops.bn_frozen_vectors(C, g_d, b_d, rm_d, rv_d, eps, out=out)
                torch.cuda.synchronize()
                if use_out:
                    assert bool((slab[:4] == SENTINEL).all()) and bool((slab[4:, C:] == SENTINEL).all()), what + ": wrote outside out="
                    assert all(got[i].data_ptr() == slab[4 + i].data_ptr() for i in range(4))
                return list(got)

            got = dict(zip(("mean", "invstd", "scale", "shift"), twice(launch, what)))
            assert torch.equal(sc.bits(got["mean"]), sc.bits(rm)), what + ": mean is a copy"
            for k in ("invstd", "scale", "shift"):
                err = (got[k].double() - ref[k]).abs()
                worst = float((err / bound[k].clamp_min(1e-300)).max())
                print("%s %-6s worst error / bound %.3f" % (what, k, worst))
                assert bool((err <= bound[k]).all()), "%s: %s beyond its rounding bound (worst %.3f of it)" % (what, k, worst)
    # the running buffers (and the affine parameters) are inputs only
    assert torch.equal(sc.bits(rm_d.cpu()), sc.bits(rm)) and torch.equal(sc.bits(rv_d.cpu()), sc.bits(rv))
    if affine:
        assert torch.equal(sc.bits(g_d.cpu()), sc.bits(gamma)) and torch.equal(sc.bits(b_d.cpu()), sc.bits(beta))


def test_trace_entries():
    C = 8
    gamma, beta, rm, rv = (dev(t) for t in fc.frozen_vectors_case(C))
    trace = ops.KernelTrace()
    ops.set_trace(trace)
    try:
        ops.bn_frozen_vectors(C, gamma, beta, rm, rv, 1e-5)
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    assert [(r[0], r[1]) for r in trace.records] == [("bn_frozen_vectors_kernel", "bn.frozen")]
