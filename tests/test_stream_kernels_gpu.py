"""The streaming kernels around the MFMA ones -- csrc/bn_train.hip, pool.hip, layout.hip, tail.hip and the tap-sum stage of
upconv.hip -- each against the plain fp64 statement of tests/stream_cases.py, driven through their own wrappers in ops.

Conventions (tests/test_stream_cases_host.py asserts the preconditions on the CPU): inputs and outputs are channel slices,
at a non-zero channel offset, of wider buffers; the other channels of an input hold NaN, the surroundings of an output the
non-integer SENTINEL, which must survive; a workspace is exactly as long as the size query says, with a sentinel tail;
every launch runs twice and must give the same bits.  Where the design is an integer one the comparison is torch.equal."""
import pytest
import torch

import stream_cases as sc
from bts_amd import _lib, ops
from bts_amd._lib import BtsHipError
from test_conv_exact_gpu import SENTINEL

pytestmark = pytest.mark.gpu

NAN = float("nan")
ALL_BN = [s for s, _ in sc.BN_SHAPES]
VARIANT_SHAPES = [(129, 44), (1537, 132)]        # 8-lane / 32-lane kernel, 3 / 25 chunks, partial channel groups
GUARD_ROWS = 128             # NaN rows behind a BN input: a reduction that walks past npix (a full last chunk) reads them


def dev(t):
    return None if t is None else t.cuda()


class Wide:
    """A [rows, C] view at channel `off` (default extra // 2) of a CUDA buffer `extra` channels wider and `pre` / `post`
    rows longer, filled with `fill`; `values` (CPU) are copied into the view."""

    def __init__(self, rows, C, fill, extra=sc.BN_EXTRA, off=None, pre=0, post=0, values=None):
        self.buf = torch.full((pre + rows + post, C + extra), fill, device="cuda")
        c0 = extra // 2 if off is None else off
        self.box = (pre, pre + rows, c0, c0 + C)
        self.view = self.buf[pre:pre + rows, c0:c0 + C]
        if values is not None:
            self.view.copy_(values)

    def reset(self):
        self.buf.fill_(SENTINEL)

    def assert_outside_untouched(self, what, also=()):
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for r0, r1, c0, c1 in (self.box,) + tuple(also):
            keep[r0:r1, c0:c1] = False
        assert bool((self.buf[keep] == SENTINEL).all()), "%s: wrote outside its slice" % what


def workspace(n):
    """(ws of exactly n floats, the buffer behind it with a sentinel tail)."""
    whole = torch.full((n + 1024,), SENTINEL, device="cuda")
    return whole[:n], whole


def assert_tail(whole, n, what):
    assert bool((whole[n:] == SENTINEL).all()), "%s: wrote past the workspace the size query asked for" % what


def twice(launch, what):
    """launch() -> tuple of tensors; run it twice, demand the same bits, return the first result on the CPU."""
    a = [t.detach().clone().cpu() for t in launch()]
    b = [t.detach().clone().cpu() for t in launch()]
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(sc.bits(u), sc.bits(v)), "%s: output %d differs between two identical launches" % (what, i)
    return a


def no_launch(fn, in_wrapper=True):
    """fn() must raise BtsHipError before it enqueues anything.  `in_wrapper`: the Python wrapper itself refuses, so the C
    entry point is not even called (a KernelTrace sees no call); otherwise the entry point refuses, and the caller checks
    that its outputs kept the sentinel."""
    trace = ops.KernelTrace()
    ops.set_trace(trace)
    try:
        with pytest.raises(BtsHipError):
            fn()
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    assert not (in_wrapper and trace.records)


# =================================================================================================== BN-train: stats
def run_stats(x, gamma, beta, rm, rv, momentum, what, use_out=False, pass_running=True):
    """bn_train_stats on x [npix, C] inside a NaN-padded buffer, twice -> {quantity: CPU fp32}."""
    npix, C = x.shape
    xin = Wide(npix, C, NAN, values=x, pre=1, post=GUARD_ROWS)
    n = ops.bn_train_ws_floats(npix, C)
    ws, whole = workspace(n)
    g, b = dev(gamma), dev(beta)
    keys = ["mean", "invstd", "scale", "shift"] + (["running_mean"] if rm is not None else []) + (["running_var"] if rv is not None else [])

    def launch():
        whole.fill_(SENTINEL)
        rm_d, rv_d = dev(rm), dev(rv)
        slab = out = None
        if use_out:                      # the dense block's stats[i, 0:4, :Ci]
            slab = torch.full((8, C + 12), SENTINEL, device="cuda")
            out = slab[0:4, :C]
        got = ops.bn_train_stats(xin.view, C, g, b, sc.BN_EPS, momentum, rm_d if pass_running else None,
                                 rv_d if pass_running else None, ws, out=out)
        torch.cuda.synchronize()
        assert_tail(whole, n, what)
        if use_out:
            assert bool((slab[4:] == SENTINEL).all()) and bool((slab[:4, C:] == SENTINEL).all()), "%s: wrote outside out=" % what
            assert all(got[i].data_ptr() == slab[i].data_ptr() for i in range(4))
        return list(got) + [t for t in (rm_d, rv_d) if t is not None]

    res = dict(zip(keys, twice(launch, what)))
    assert torch.equal(sc.bits(xin.view.cpu()), sc.bits(x)), "%s: the input changed" % what
    return res


def check_stats(got, x, gamma, beta, rm, rv, momentum, what):
    r64, e32, tol = sc.bn_stats_floor(x, gamma, beta, rm, rv, momentum)
    bad = []
    for k in e32:
        err = (got[k].double() - r64[k]).abs()
        ratio = float(err.max()) / e32[k] if e32[k] > 0 else (0.0 if float(err.max()) == 0 else float("inf"))
        print("stats %-34s %-12s E32 %.3e  kernel %.3e  ratio %6.2f  worst err/tol %.3f"
              % (what, k, e32[k], float(err.max()), ratio, float((err / tol[k]).max())))
        if not bool((err <= tol[k]).all()):
            bad.append(k)
    assert not bad, "%s: %s beyond max(4 x fp32 two-pass error, 2 ulp)" % (what, bad)


@pytest.mark.parametrize("kind", sc.STATS_KINDS)
@pytest.mark.parametrize("shape", ALL_BN)
def test_bn_stats(shape, kind):
    """mean, invstd, scale, shift and the running buffers against fp64 on the same fp32 values.  Tolerance per case and
    quantity: max(4 * E32, 2 ulp of the value), E32 = the error of a plain two-pass fp32 CPU statement (torch.sum) against
    fp64, the largest over the channels.  The run prints E32, the kernel's error and their ratio per case; the table
    measured on an MI355X stands in STATS_FLOOR_TABLE below."""
    x, gamma, beta, rm, rv = sc.bn_stats_input(shape[0], shape[1], kind)
    what = "%dx%d %s" % (shape[0], shape[1], kind)
    got = run_stats(x, gamma, beta, rm, rv, 0.1, what)
    check_stats(got, x, gamma, beta, rm, rv, 0.1, what)


# Measured on an MI355X: per case and quantity, E32 (largest absolute error over the channels of the fp32 two-pass CPU
# statement against fp64) and the kernel's largest error as a multiple of it.  The bar is 4 (or 2 ulp of the value).
# In the "cancel" rows the two-pass fp32 statement itself loses digits in x - mean (invstd is near 100, shift near 1e5); the
# kernel subtracts the first row before anything is rounded and sits far below it.  Before the statistics were merged in
# the shifted domain, invstd of "33x8 cancel" was at 27.6 x E32.
STATS_FLOOR_TABLE = """
case             | mean           | invstd         | scale          | shift          | running_mean   | running_var   
2x4 gauss        | 6.0e-08  1.00 | 1.8e-07  1.00 | 1.4e-07  1.00 | 2.4e-07  0.51 | 5.7e-08  1.00 | 3.9e-08  1.00
2x4 cancel       | 6.1e-05  1.00 | 1.8e-03  0.01 | 1.7e-03  0.00 | 1.7e+00  0.01 | 1.1e-05  1.00 | 3.5e-08  0.70
33x8 gauss       | 5.1e-08  1.47 | 5.9e-08  0.62 | 3.9e-08  0.65 | 5.1e-08  0.79 | 6.5e-08  1.00 | 1.0e-07  0.76
33x8 cancel      | 1.0e-04  0.24 | 6.3e-03  0.00 | 5.1e-03  0.00 | 5.1e+00  0.00 | 8.9e-06  0.49 | 1.3e-07  0.33
64x32 gauss      | 7.3e-08  1.24 | 1.0e-07  0.74 | 8.4e-08  1.14 | 7.8e-08  1.06 | 1.3e-07  1.00 | 9.3e-08  1.22
64x32 cancel     | 8.5e-05  0.70 | 2.9e-03  0.01 | 2.9e-03  0.01 | 3.0e+00  0.01 | 1.0e-05  0.89 | 1.1e-07  0.79
65x32 gauss      | 9.0e-08  1.31 | 6.2e-08  0.85 | 9.0e-08  0.82 | 1.1e-07  1.47 | 1.8e-07  1.00 | 8.8e-08  1.04
65x32 cancel     | 1.5e-04  0.38 | 8.7e-03  0.00 | 1.1e-02  0.00 | 1.1e+01  0.00 | 1.4e-05  0.59 | 1.1e-07  0.78
70x48 gauss      | 8.1e-08  1.43 | 7.3e-08  1.44 | 8.4e-08  1.22 | 8.1e-08  0.76 | 1.3e-07  1.00 | 1.2e-07  0.83
70x48 cancel     | 1.4e-04  0.23 | 7.5e-03  0.00 | 9.0e-03  0.00 | 9.1e+00  0.00 | 2.0e-05  0.55 | 1.2e-07  0.77
129x44 gauss     | 9.7e-08  0.73 | 5.0e-08  1.53 | 9.8e-08  1.12 | 1.4e-07  0.78 | 1.0e-07  1.00 | 9.7e-08  1.55
129x44 cancel    | 1.2e-04  0.50 | 9.4e-03  0.00 | 7.5e-03  0.00 | 7.7e+00  0.00 | 1.7e-05  0.56 | 1.2e-07  0.53
515x108 gauss    | 6.0e-08  0.88 | 8.7e-08  0.99 | 1.1e-07  1.01 | 7.0e-08  1.10 | 1.3e-07  1.00 | 1.3e-07  0.73
515x108 cancel   | 2.1e-04  0.27 | 1.8e-02  0.00 | 1.5e-02  0.00 | 1.5e+01  0.00 | 2.0e-05  0.46 | 1.3e-07  0.64
577x112 gauss    | 5.7e-08  1.06 | 7.0e-08  1.05 | 1.2e-07  1.00 | 1.4e-07  0.86 | 1.2e-07  1.00 | 1.2e-07  0.90
577x112 cancel   | 1.5e-04  0.41 | 1.1e-02  0.00 | 9.9e-03  0.00 | 1.0e+01  0.00 | 2.1e-05  0.56 | 1.2e-07  0.77
1537x132 gauss   | 5.3e-08  1.14 | 8.2e-08  0.80 | 1.3e-07  0.82 | 1.1e-07  1.00 | 2.2e-07  1.00 | 1.4e-07  0.88
1537x132 cancel  | 1.4e-04  0.41 | 7.9e-03  0.00 | 1.1e-02  0.00 | 1.2e+01  0.00 | 1.8e-05  0.57 | 1.2e-07  0.76
1601x64 gauss    | 6.5e-08  0.97 | 7.1e-08  1.00 | 8.0e-08  0.92 | 8.2e-08  0.94 | 1.4e-07  1.00 | 1.3e-07  0.65
1601x64 cancel   | 1.6e-04  0.38 | 1.1e-02  0.00 | 1.2e-02  0.00 | 1.3e+01  0.00 | 2.4e-05  0.44 | 1.3e-07  0.65
2049x8 gauss     | 5.8e-08  0.95 | 7.2e-08  0.89 | 7.9e-08  0.79 | 5.9e-08  0.46 | 6.5e-08  1.00 | 9.3e-08  0.78
2049x8 cancel    | 6.1e-05  0.37 | 1.6e-03  0.00 | 1.2e-03  0.01 | 1.2e+00  0.00 | 6.4e-06  0.71 | 6.0e-08  1.00
3650x16 gauss    | 3.5e-08  1.75 | 5.8e-08  1.04 | 5.3e-08  0.92 | 8.1e-08  0.94 | 4.1e-08  1.00 | 8.2e-08  0.78
3650x16 cancel   | 9.0e-05  0.47 | 3.5e-03  0.00 | 3.5e-03  0.01 | 3.6e+00  0.01 | 1.4e-05  0.67 | 5.3e-08  1.61
12x2208 gauss    | 2.1e-07  0.97 | 1.8e-07  1.20 | 2.3e-07  0.94 | 3.4e-07  0.87 | 2.6e-07  1.00 | 1.8e-07  1.29
12x2208 cancel   | 2.1e-04  0.29 | 5.8e-02  0.00 | 7.4e-02  0.00 | 7.8e+01  0.00 | 2.3e-05  0.61 | 1.4e-07  0.66
98304x8 gauss    | 2.7e-08  2.25 | 6.5e-08  0.50 | 7.7e-08  0.76 | 7.6e-08  0.68 | 4.9e-08  1.00 | 4.8e-08  1.00
98304x8 cancel   | 1.1e-04  0.51 | 5.1e-03  0.00 | 6.5e-03  0.00 | 6.8e+00  0.00 | 1.4e-05  0.68 | 7.7e-08  1.13
"""


@pytest.mark.parametrize("shape", VARIANT_SHAPES)
@pytest.mark.parametrize("variant", ["no_affine", "no_running", "momentum_0.01", "momentum_1", "out_view"])
def test_bn_stats_variants(shape, variant):
    x, gamma, beta, rm, rv = sc.bn_stats_input(shape[0], shape[1], "gauss")
    what = "%dx%d %s" % (shape[0], shape[1], variant)
    momentum = {"momentum_0.01": 0.01, "momentum_1": 1.0}.get(variant, 0.1)
    if variant == "no_affine":
        gamma = beta = None
    if variant == "no_running":
        # the buffers exist on the device but are not passed: they keep their bits (run_stats returns them)
        got = run_stats(x, gamma, beta, rm, rv, momentum, what, pass_running=False)
        assert torch.equal(got.pop("running_mean"), rm) and torch.equal(got.pop("running_var"), rv)
        check_stats(got, x, gamma, beta, None, None, momentum, what)
        return
    got = run_stats(x, gamma, beta, rm, rv, momentum, what, use_out=variant == "out_view")
    check_stats(got, x, gamma, beta, rm, rv, momentum, what)


@pytest.mark.parametrize("shape", [(129, 44), (1601, 64), (98304, 8)])
def test_bn_stats_constant_channel(shape):
    """A constant channel: every shifted value is 0, so m2 == 0 and mean == the constant exactly, through every merge."""
    npix, C = shape
    x, gamma, beta, rm, rv = sc.bn_stats_input(npix, C, "gauss")
    consts = {1: 3.25, 2: float(torch.tensor(1000.1, dtype=torch.float32)), C - 1: -7.0}
    for c, v in consts.items():
        x[:, c] = v
    got = run_stats(x, gamma, beta, rm, rv, 1.0, "%dx%d constant" % shape)
    want_invstd = (1.0 / torch.sqrt(torch.tensor(sc.BN_EPS, dtype=torch.float32))).double()
    for c, v in consts.items():
        assert float(got["mean"][c]) == v
        assert float(got["running_var"][c]) == 0.0              # momentum 1: running_var = m2 / (n - 1)
        assert float(got["running_mean"][c]) == v
        assert abs(float(got["invstd"][c]) - float(want_invstd)) <= float(sc.ulp32(want_invstd))
    check_stats(got, x, gamma, beta, rm, rv, 1.0, "%dx%d constant" % shape)


# =================================================================================================== BN-train: apply
@pytest.mark.parametrize("shape", ALL_BN + [sc.BN_GRID_STRIDE])
def test_bn_apply_exact(shape):
    npix, C = shape
    x, scale, shift = sc.bn_apply_case(npix, C)
    xin = Wide(npix, C, NAN, values=x)
    y = Wide(npix, C, SENTINEL, extra=16)                        # another stride and offset than the input's
    s_d, b_d = dev(scale), dev(shift)
    for relu in (False, True):
        want = sc.bn_apply_ref(x, scale, shift, relu).float().cuda()

        def launch():
            y.reset()
            ops.bn_apply(xin.view, C, s_d, b_d, relu, y.view)
            torch.cuda.synchronize()
            assert torch.equal(y.view, want), "bn_apply %s relu=%s" % (shape, relu)
            y.assert_outside_untouched("bn_apply %s" % (shape,))
            return (y.view,)

        twice(launch, "bn_apply %s" % (shape,))


# ================================================================================================ BN-train: backward
def check_bwd(shape, relu, form):
    npix, C = shape
    what = "bn_train_backward %s relu=%s %s" % (shape, relu, form)
    x, dy, mean, invstd, scale, shift = sc.bn_bwd_case(npix, C)
    ref = sc.bn_bwd_ref(x, dy, mean, invstd, scale, shift, relu)
    xin = Wide(npix, C, NAN, values=x, pre=1, post=GUARD_ROWS)
    also = ()
    if form == "shared":             # dx in the same wide buffer as dy, in other columns
        both = Wide(npix, C, SENTINEL, extra=C + 12, off=4)
        gin_view, dx_view = both.view, both.buf[:, C + 8:2 * C + 8]
        also = ((0, npix, C + 8, 2 * C + 8),)
        dxw = both
    else:
        gin_view = Wide(npix, C, NAN, values=dy, pre=1, post=GUARD_ROWS).view
        dxw = Wide(npix, C, SENTINEL, extra=16) if form == "dx" else None
        dx_view = None if dxw is None else dxw.view
    n = ops.bn_train_ws_floats(npix, C)
    ws, whole = workspace(n)
    vecs = [dev(v) for v in (mean, invstd, scale, shift)]

    def launch():
        whole.fill_(SENTINEL)
        if dxw is not None:
            dxw.reset()
        if form == "shared":
            gin_view.copy_(dy)
        dg, db = ops.bn_train_backward(xin.view, gin_view, C, vecs[0], vecs[1], vecs[2], vecs[3], relu, ws, dx_view)
        torch.cuda.synchronize()
        assert_tail(whole, n, what)
        if dxw is not None:
            dxw.assert_outside_untouched(what, also=also)
        return (dg, db) + (() if dx_view is None else (dx_view,))

    got = twice(launch, what)
    assert torch.equal(got[0].double(), ref["dgamma"]), what + ": dgamma"
    assert torch.equal(got[1].double(), ref["dbeta"]), what + ": dbeta"
    assert torch.equal(gin_view.cpu(), dy) and torch.equal(xin.view.cpu(), x), what + ": an input changed"
    if dx_view is not None:
        err = (got[2].double() - ref["dx"]).abs()
        worst = float((err / ref["bound"].clamp_min(1e-300)).max())
        print("%s: worst dx error / bound %.3f" % (what, worst))
        assert bool((err <= ref["bound"]).all()), "%s: dx beyond its rounding bound (worst %.3f of it)" % (what, worst)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", ALL_BN + [sc.BN_GRID_STRIDE])
def test_bn_backward(shape, relu):
    check_bwd(shape, relu, "dx")


@pytest.mark.parametrize("form", ["no_dx", "shared"])
@pytest.mark.parametrize("shape", VARIANT_SHAPES + [(2, 4)])
def test_bn_backward_forms(shape, form):
    check_bwd(shape, True, form)


# =========================================================================================================== pooling
def check_maxpool(shape):
    B, h, w, C = shape
    x = sc.maxpool_case(B, h, w, C)
    want = sc.maxpool_ref(x).float().view(-1, C).cuda()
    ho, wo = (h + 1) // 2, (w + 1) // 2
    src = Wide(B * h * w, C, NAN, values=x.view(-1, C))
    d1 = Wide(B * ho * wo, C, SENTINEL, extra=8)
    d2 = Wide(B * ho * wo, C, SENTINEL, extra=24, off=16)

    def launch(second):
        def go():
            d1.reset(), d2.reset()
            ops.maxpool3x3s2(src.view, B, h, w, d1.view, d2.view if second else None)
            torch.cuda.synchronize()
            assert torch.equal(d1.view, want), "maxpool %s" % (shape,)
            d1.assert_outside_untouched("maxpool %s" % (shape,))
            if second:
                assert torch.equal(d2.view, want), "maxpool %s, second destination" % (shape,)
                d2.assert_outside_untouched("maxpool %s, second destination" % (shape,))
            else:
                assert bool((d2.buf == SENTINEL).all())
            return (d1.view, d2.view)
        return go

    twice(launch(True), "maxpool %s" % (shape,))
    twice(launch(False), "maxpool %s, one destination" % (shape,))


@pytest.mark.parametrize("shape", sc.MAXPOOL_SHAPES)
def test_maxpool_exact(shape):
    check_maxpool(shape)


def test_maxpool_grid_stride():
    check_maxpool(sc.POOL_GRID_STRIDE)


def check_avgpool(shape):
    B, h, w, C = shape
    x, scale, shift = sc.avgpool_case(B, h, w, C)
    want = sc.avgpool_ref(x, scale, shift).float().view(-1, C).cuda()
    src = Wide(B * h * w, C, NAN, values=x.view(-1, C))
    dst = Wide(B * (h // 2) * (w // 2), C, SENTINEL, extra=16)
    s_d, b_d = dev(scale), dev(shift)

    def launch():
        dst.reset()
        ops.bn_relu_avgpool2(src.view, B, h, w, s_d, b_d, dst.view)
        torch.cuda.synchronize()
        assert torch.equal(dst.view, want), "bn_relu_avgpool2 %s" % (shape,)
        dst.assert_outside_untouched("bn_relu_avgpool2 %s" % (shape,))
        return (dst.view,)

    twice(launch, "bn_relu_avgpool2 %s" % (shape,))


@pytest.mark.parametrize("shape", sc.AVGPOOL_SHAPES)
def test_avgpool_exact(shape):
    check_avgpool(shape)


def test_avgpool_grid_stride():
    check_avgpool(sc.POOL_GRID_STRIDE)


@pytest.mark.parametrize("h,w", [(3, 2), (2, 3), (5, 5)])
def test_avgpool_odd_size_raises(h, w):
    C = 8
    src = Wide(h * w, C, NAN, values=torch.ones(h * w, C))
    dst = Wide(max((h // 2) * (w // 2), 1), C, SENTINEL)
    s = torch.ones(C, device="cuda")
    no_launch(lambda: ops.bn_relu_avgpool2(src.view, 1, h, w, s, s, dst.view[:(h // 2) * (w // 2)]), in_wrapper=False)
    assert bool((dst.buf == SENTINEL).all())


def test_pool_entry_points_reject_a_stride_below_C():
    """The C entry points themselves (ops' view checks would stop these first): rows of C floats at a pixel stride < C
    overlap.  The buffers are large enough for any walk at these sizes."""
    lib = _lib.load_real()
    src = torch.zeros(4096, device="cuda")
    dst = torch.full((4096,), SENTINEL, device="cuda")
    dst2 = torch.full((4096,), SENTINEL, device="cuda")
    vec = torch.ones(8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    B, h, w, C = 1, 4, 4, 8
    for ss, ds, d2s in ((4, 8, 8), (8, 4, 8), (8, 8, 4)):
        rc = lib.bts_maxpool3x3s2_nhwc_f32(src.data_ptr(), ss, B, h, w, C, dst.data_ptr(), ds, dst2.data_ptr(), d2s, stream)
        assert rc == -1, (ss, ds, d2s, rc)
        with pytest.raises(BtsHipError):
            _lib.check(rc, "bts_maxpool3x3s2_nhwc_f32")
    assert lib.bts_maxpool3x3s2_nhwc_f32(src.data_ptr(), 8, B, h, w, C, dst.data_ptr(), 8, None, 0, stream) == 0   # unused dst2 stride
    torch.cuda.synchronize()
    dst.fill_(SENTINEL)
    for ss, ds in ((4, 8), (8, 4)):
        rc = lib.bts_bn_relu_avgpool2_nhwc_f32(src.data_ptr(), ss, B, h, w, C, vec.data_ptr(), vec.data_ptr(), dst.data_ptr(), ds, stream)
        assert rc == -1, (ss, ds, rc)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((dst2 == SENTINEL).all())


# ============================================================================================================ layout
def nchw_input(x):
    """x [B,C,1,HW] as the middle frames of a NaN-filled [B+2,C,1,HW] CUDA buffer (contiguous)."""
    buf = torch.full((x.shape[0] + 2,) + tuple(x.shape[1:]), NAN, device="cuda")
    buf[1:-1].copy_(x)
    return buf[1:-1]


def check_to_nhwc(B, C, HW, extra=8, off=None):
    x = sc.layout_case(B, C, HW)
    rows = x.permute(0, 2, 3, 1).reshape(B * HW, C)
    src = nchw_input(x)
    dst = Wide(B * HW, C, SENTINEL, extra=extra, off=off, pre=3, post=40)        # rows around it: the tile's masked p >= HW
    what = "nchw_to_nhwc B=%d C=%d HW=%d stride %d" % (B, C, HW, C + extra)
    for relu in (False, True):
        def launch():
            dst.reset()
            ops.nchw_to_nhwc(src, dst.view, relu=relu)
            torch.cuda.synchronize()
            dst.assert_outside_untouched(what)
            return (dst.view,)
        got = twice(launch, what)[0]
        if relu:
            assert torch.equal(got, rows.clamp_min(0.0)), what + " relu"
        else:
            assert torch.equal(sc.bits(got), sc.bits(rows)), what              # -0.0 keeps its sign bit


def check_to_nchw(B, C, HW):
    x = sc.layout_case(B, C, HW)
    src = Wide(B * HW, C, NAN, pre=3, post=40, values=x.permute(0, 2, 3, 1).reshape(B * HW, C))
    what = "nhwc_to_nchw B=%d C=%d HW=%d" % (B, C, HW)
    got = twice(lambda: (ops.nhwc_to_nchw(src.view, B, 1, HW),), what)[0]
    assert torch.equal(sc.bits(got), sc.bits(x)), what


@pytest.mark.parametrize("C", sc.LAYOUT_C)
def test_layout_exact(C):
    for B in sc.LAYOUT_B:
        for HW in sc.LAYOUT_HW:
            check_to_nhwc(B, C, HW)
            check_to_nchw(B, C, HW)


@pytest.mark.parametrize("C", [3, 4])
def test_layout_small_c_grid_stride(C):
    check_to_nhwc(sc.LAYOUT_GRID_STRIDE[0], C, sc.LAYOUT_GRID_STRIDE[1])


@pytest.mark.parametrize("extra,off", [(6, 2), (8, 2), (6, 4)])
def test_layout_c4_unaligned_destination(extra, off):
    """C == 4 into a destination that cannot take 16-byte stores -- channel offset 2 of a stride-10 buffer, an aligned stride
    at a misaligned offset, an aligned offset at stride 10 -- goes through scalar stores and is exact."""
    for B, HW in ((1, 1), (3, 45), (2, 300)):
        check_to_nhwc(B, 4, HW, extra=extra, off=off)


# ======================================================================================================== depth tail
@pytest.mark.parametrize("C,H,W", sc.DEPTH_CASES)
def test_get_depth(C, H, W):
    """The integer pre-activation, recovered through the logit, equals the fp64 stencil wherever |acc| <= 8 (at least 95 % of
    the pixels and some on every border: host test); the rest within 1e-5 * max_depth of fp64."""
    B, md = sc.DEPTH_B, sc.DEPTH_MAX[C]
    x, w, acc = sc.depth_case(C, H, W)
    inbuf = torch.full((B + 2, C, H, W), NAN, device="cuda")
    inbuf[1:-1].copy_(x)
    outbuf = torch.full((B + 2, 1, H, W), SENTINEL, device="cuda")
    fbuf = torch.full((B + 2,), NAN, device="cuda")
    fbuf[1:-1].copy_(torch.tensor(sc.DEPTH_FOCAL))
    w_d = w.cuda()
    small = acc.abs() <= sc.DEPTH_EXACT_ACC
    for focal in (None, torch.tensor(sc.DEPTH_FOCAL)):
        what = "get_depth C=%d %dx%d focal=%s" % (C, H, W, focal is not None)

        def launch():
            outbuf.fill_(SENTINEL)
            ops.get_depth_forward(inbuf[1:-1], w_d, md, None if focal is None else fbuf[1:-1], out=outbuf[1:-1])
            torch.cuda.synchronize()
            assert bool((outbuf[0] == SENTINEL).all()) and bool((outbuf[-1] == SENTINEL).all()), what + ": wrote outside the output"
            return (outbuf[1:-1],)

        got = twice(launch, what)[0]
        assert bool(torch.isfinite(got).all()), what
        rec = sc.depth_recover(got, md, focal)
        wrong = small & (rec != acc)
        assert not bool(wrong.any()), "%s: %d pixels with another integer, first at %s" % (what, int(wrong.sum()), wrong.nonzero()[0].tolist())
        err = (got.double() - sc.depth_ref(acc, md, focal)).abs()
        assert float(err.max()) <= 1e-5 * md, "%s: %.3e" % (what, float(err.max()))


@pytest.mark.parametrize("n", sc.PACK_N)
def test_pack_planes(n):
    for npix in sc.PACK_NPIX + (sc.PACK_GRID_STRIDE,):
        planes = sc.pack_case(n, npix)
        bufs = [torch.full((npix + 8,), NAN, device="cuda") for _ in planes]
        srcs = []
        for b, p in zip(bufs, planes):
            b[4:4 + npix].copy_(p)
            srcs.append(b[4:4 + npix])
        dst = Wide(npix, n, SENTINEL, extra=8, off=4) if n == 4 else Wide(npix, n, SENTINEL, extra=5, off=3)
        what = "pack_planes n=%d npix=%d" % (n, npix)
        want = torch.stack(planes, dim=1).cuda()

        def launch():
            dst.reset()
            ops.pack_planes(srcs, dst.view)
            torch.cuda.synchronize()
            assert torch.equal(dst.view, want), what
            dst.assert_outside_untouched(what)
            return (dst.view,)

        twice(launch, what)
    if n == 4:                                   # 16-byte stores: a misaligned slice is refused, nothing written
        bad = Wide(257, 4, SENTINEL, extra=6, off=2)
        four = [torch.zeros(257, device="cuda") for _ in range(4)]
        no_launch(lambda: ops.pack_planes(four, bad.view), in_wrapper=False)
        assert bool((bad.buf == SENTINEL).all())


# ==================================================================================================== upconv_combine
def check_combine(shape, configs):
    B, h, w, c = shape
    taps, es, eb = sc.combine_case(B, h, w, c)
    tin = Wide(B * h * w, 9 * c, NAN, extra=4 + sc.COMBINE_PAD, off=4, values=taps)
    assert tin.view.stride(0) > 9 * c
    y = Wide(4 * B * h * w, c, SENTINEL, extra=16)
    e2_d = (es.cuda(), eb.cuda())
    for act, with_e2 in configs:
        what = "upconv_combine %s act=%d e2=%s" % (shape, act, with_e2)
        want, v = sc.combine_ref(taps, B, h, w, c, act, (es, eb) if with_e2 else None)
        want, v = want.view(-1, c), v.view(-1, c)

        def launch():
            y.reset()
            ops.upconv_combine(tin.view, B, h, w, c, y.view, act=act, e2=e2_d if with_e2 else None)
            torch.cuda.synchronize()
            y.assert_outside_untouched(what)
            return (y.view,)

        got = twice(launch, what)[0].double()
        if act == ops.ACT_ELU:                   # exact where the sum is non-negative, 1e-6 absolute where ELU bends it
            pos = v >= 0
            assert torch.equal(got[pos], want[pos]), what
            assert float((got[~pos] - want[~pos]).abs().max()) <= sc.ELU_ABS_TOL, what
        else:
            assert torch.equal(got, want), what


@pytest.mark.parametrize("shape", sc.COMBINE_SHAPES)
def test_upconv_combine_exact(shape):
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_ELU) == (0, 1, 2)
    check_combine(shape, [(act, e2) for act in (0, 1, 2) for e2 in (False, True)])


def test_upconv_combine_grid_stride():
    check_combine(sc.COMBINE_GRID_STRIDE, [(1, True)])


# ================================================================================= host-side checks of the BN wrappers
def test_bn_wrappers_reject_bad_views_before_launch():
    npix, C = 33, 8
    x = Wide(npix, C, NAN, values=torch.ones(npix, C))
    y = Wide(npix, C, SENTINEL)
    short = Wide(npix - 1, C, SENTINEL)
    vec = torch.ones(C, device="cuda")
    vec_short = torch.ones(C - 4, device="cuda")
    vec_odd = torch.ones(C + 4, device="cuda")[1:1 + C]              # right length, not 16-byte aligned
    ws, whole = workspace(ops.bn_train_ws_floats(npix, C))
    apply_bad = [
        lambda: ops.bn_apply(x.view, C + 4, vec_odd, vec_odd, False, y.view),            # C beyond the view widths
        lambda: ops.bn_apply(x.view, C - 2, vec, vec, False, y.view),                    # C not a multiple of 4
        lambda: ops.bn_apply(x.view, C, vec, vec, False, short.view),                    # y2d one row short
        lambda: ops.bn_apply(x.view[:, :4], 4, vec, vec, False, y.view[:, 1:5]),         # misaligned rows
        lambda: ops.bn_apply(x.view, C, vec_short, vec, False, y.view),                  # short vectors
        lambda: ops.bn_apply(x.view, C, vec, vec_short, False, y.view),
        lambda: ops.bn_apply(x.view, C, vec_odd, vec, False, y.view),                    # misaligned vector
        lambda: ops.bn_apply(x.view, C, vec, vec.double(), False, y.view),               # not fp32
    ]
    for fn in apply_bad:
        no_launch(fn)
    v = [vec, vec, vec, vec]
    bwd_bad = [
        lambda: ops.bn_train_backward(x.view, x.view, C + 4, *v, True, ws, y.view),
        lambda: ops.bn_train_backward(x.view, x.view[:, :4], C, *v, True, ws, y.view),   # dy narrower than C
        lambda: ops.bn_train_backward(x.view, x.view[:-1], C, *v, True, ws, y.view),     # dy one row short
        lambda: ops.bn_train_backward(x.view, x.view, C, *v, True, ws, short.view),      # dx2d one row short
        lambda: ops.bn_train_backward(x.view, x.view, C, *v, True, ws, y.view[:, :4]),   # dx2d narrower than C
    ] + [(lambda i, bad: lambda: ops.bn_train_backward(x.view, x.view, C, *(v[:i] + [bad] + v[i + 1:]), True, ws, y.view))(i, bad)
         for i in range(4) for bad in (vec_short, vec_odd)]
    for fn in bwd_bad:
        no_launch(fn)
    stats_bad = [lambda: ops.bn_train_stats(x.view, C, vec_short, vec, sc.BN_EPS, 0.1, None, None, ws),
                 lambda: ops.bn_train_stats(x.view, C, vec, vec, sc.BN_EPS, 0.1, vec, vec_short, ws)]
    for fn in stats_bad:
        no_launch(fn)
    assert bool((y.buf == SENTINEL).all()) and bool((short.buf == SENTINEL).all()) and bool((whole == SENTINEL).all())
    # and the same calls with good operands go through
    ops.bn_apply(x.view, C, vec, vec, False, y.view)
    ops.bn_train_backward(x.view, x.view, C, *v, True, ws, y.view)
    torch.cuda.synchronize()
    assert not bool((y.view == SENTINEL).any())
