"""bts_conv_fwd_f32 (csrc/conv_mfma.hip and its .inc files: every kernel family, tile and epilogue the dispatch can
choose) against a plain fp64 statement of the fused convolution on the CPU, on every case of tests/conv_cases.py.

The exact test feeds small integers, so that every partial sum is exactly representable in fp32 (the precondition is
asserted on the CPU by tests/test_conv_cases_host.py): the kernel family, the tile, split-K and the summation order cannot
change a bit, and the assertion is torch.equal -- under fp32, under bf16x3 (three bf16 pieces hold 24 bits) and, against
operands rounded to bf16 first, under bf16.  Which kernel ran comes from a KernelTrace and must be the one the case
table's plan names.  Nothing is forced: the dispatch chooses."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # run as a script (the child process below): the package sits one level up
    sys.path.insert(0, ROOT)

import conv_cases as cc  # noqa: E402
from bts_amd import conv_plan, ops  # noqa: E402
from bts_amd.conv_plan import Family  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.671875          # not an integer (nor a multiple of 1/4): no exact result can equal it


def _slice_of_wider(values, extra, fill):
    """`values` [rows, C] as a channel slice, at a non-zero offset, of a CUDA buffer `extra` channels wider whose other
    channels hold `fill`.  Returns (view, buffer)."""
    rows, C = values.shape
    buf = torch.full((rows, C + extra), fill, device="cuda")
    view = buf[:, extra // 2:extra // 2 + C]
    view.copy_(values)
    return view, buf


def _pack(c, o):
    if c.subpixel:
        return ops.pack_upconv_subpixel(o.w[0].float(), c_in_ld=c.c_in)[0].cuda()
    if c.n_bundles > 1:
        return torch.stack([ops.pack_conv_weight(o.w[j].float(), c_in_ld=c.c_in)[0] for j in range(c.n_bundles)]).cuda()
    return ops.pack_conv_weight(o.w[0].float(), c_in_ld=c.c_in)[0].cuda()


class Launch:
    """The device side of one case: operands in their (wider) buffers, sentinel-filled outputs, and `run(frames)`."""

    def __init__(self, c, o, act=None):
        self.c, self.o, self.act = c, o, ops.ACT_NONE if act is None else act
        x_ch, c_out_pad, y_ch = cc.channels(c)
        self.H, self.W = cc.out_hw(c)
        self.y_ch = y_ch
        self.x, _ = _slice_of_wider(o.x.reshape(-1, x_ch).float(), c.x_extra, float("nan"))
        self.w = _pack(c, o)
        vec = lambda v: v.float().cuda() if c.n_bundles > 1 else ops.pad_vec(v.float().cuda(), c_out_pad)
        self.pre = None if o.pre is None else (o.pre[0].float().cuda(), o.pre[1].float().cuda())
        self.e1 = None if o.e1 is None else (vec(o.e1[0]), vec(o.e1[1]))
        self.e2 = None if o.e2 is None else (vec(o.e2[0]), vec(o.e2[1]))
        self.res = None if o.res is None else _slice_of_wider(o.res.reshape(-1, y_ch).float(), c.y_extra, float("nan"))[0]
        self.tail = None if o.tail is None else [o.tail[j].float().cuda().contiguous() for j in range(c.n_tail)]
        self.ws = self.ws_all = None
        if c.ws_floats is not None:
            self.ws_all = torch.full((c.ws_floats + 4096,), SENTINEL, device="cuda")
            self.ws = self.ws_all[:c.ws_floats]

    def outputs(self, B):
        """Fresh sentinel-filled destinations for B frames: (y view, y buffer, y2 view or None, y2 buffer or None)."""
        c, M = self.c, B * self.H * self.W
        if c.nchw:                                             # a sentinel frame before and after
            buf = torch.full((B + 2, c.c_out, self.H, self.W), SENTINEL, device="cuda")
            return buf[1:B + 1], buf, None, None
        y, ybuf = _slice_of_wider(torch.full((M, self.y_ch), SENTINEL), c.y_extra, SENTINEL)
        y2 = y2buf = None
        if c.y2:
            y2, y2buf = _slice_of_wider(torch.full((M, self.y_ch), SENTINEL), c.y_extra, SENTINEL)
        return y, ybuf, y2, y2buf

    def run(self, out, first_frame=0):
        """One launch of frames [first_frame, B) into `out` (from outputs()); returns the kernel name of the trace."""
        c = self.c
        y, _, y2, _ = out
        B = c.B - first_frame
        px, po = first_frame * c.h * c.w, first_frame * self.H * self.W
        trace = ops.KernelTrace()
        ops.set_trace(trace)
        try:
            with ops.launch_config(fill_frames=c.fill_frames, precision=c.precision):
                ops.conv_forward(self.x[px:], B, c.h, c.w, self.w, c.c_out, c.ksize, dil=c.dil, up=c.up, c_in_ld=c.c_in, pre=self.pre,
                                 pre_relu=c.pre_relu, e1=self.e1, act=self.act, e2=self.e2, y2d=None if c.nchw else y,
                                 y_nchw=y if c.nchw else None, stride=c.stride, pad=c.pad, y2_2d=y2, subpixel=c.subpixel,
                                 splitk_ws=self.ws, res2d=None if self.res is None else self.res[po:], n_bundles=c.n_bundles,
                                 tail_planes=None if self.tail is None else [t[first_frame:] for t in self.tail])
        finally:
            ops.set_trace(None)
        torch.cuda.synchronize()
        assert len(trace.records) == 1
        return trace.records[0][0]

    def read(self, out, B):
        """(y, y2 or None) as fp64 [B, H, W, channels] on the CPU."""
        y, _, y2, _ = out
        if self.c.nchw:
            return y.permute(0, 2, 3, 1).cpu().double(), None
        shape = (B, self.H, self.W, self.y_ch)
        return y.cpu().double().reshape(shape), None if y2 is None else y2.cpu().double().reshape(shape)

    def assert_surroundings_untouched(self, out, what):
        c = self.c
        y, ybuf, y2, y2buf = out
        if c.nchw:
            assert bool((ybuf[0] == SENTINEL).all()) and bool((ybuf[-1] == SENTINEL).all()), \
                "%s, %s: wrote a frame before or after the NCHW output" % (c.name, what)
            return
        for buf, name in ((ybuf, "y"), (y2buf, "y2")):
            if buf is not None and c.y_extra:
                lo = c.y_extra // 2
                outside = torch.cat([buf[:, :lo], buf[:, lo + self.y_ch:]], dim=1)
                assert bool((outside == SENTINEL).all()), "%s, %s: wrote channels outside the %s slice" % (c.name, what, name)


def _where(c, plan, bad, H, W):
    """First wrong element, its tile coordinates and whether that tile is ragged, for the failure message."""
    b, y, x, n = bad.nonzero()[0].tolist()
    nl = n % c.c_out                                           # channel inside its bundle
    msg = "%d wrong of %d; first (b %d, y %d, x %d, n %d): %s tile %dx%d, channel tile %d (%s)" % (
        int(bad.sum()), bad.numel(), b, y, x, n, plan.family.name, plan.bm, plan.bn, nl // plan.bn,
        "ragged" if (nl // plan.bn + 1) * plan.bn > c.c_out else "full")
    if plan.family in (Family.ROW, Family.ROW_BF16, Family.WIDE_1X1):
        Hm, Wm, ym, xm = (c.h, c.w, y // 2, x // 2) if c.subpixel else (H, W, y, x)      # sub-pixel tiles walk source pixels
        m, M = (b * Hm + ym) * Wm + xm, c.B * Hm * Wm
        return msg + ", row tile %d of %d (%s)" % (m // plan.bm, -(-M // plan.bm), "ragged" if (m // plan.bm + 1) * plan.bm > M else "full")
    th, tw = {Family.WINO: (8, 16), Family.STEM: (8, 32)}.get(plan.family, (8, 16) if plan.bn == 48 else (4, 32))
    Hm, Wm, ym, xm = (c.h, c.w, y // 2, x // 2) if c.subpixel else (H, W, y, x)
    ty, tx = ym // (th * (c.dil if plan.dil else 1)), xm // tw
    ragged = (ty + 1) * th * (c.dil if plan.dil else 1) > Hm or (tx + 1) * tw > Wm
    return msg + ", spatial tile (%d, %d) of %dx%d pixels (%s)" % (ty, tx, th, tw, "ragged" if ragged else "interior")


def check_case(c):
    """Everything test_conv_is_exact_on_small_integers asserts for one case (also run from the child process of the
    dilation-6 / 12 cases)."""
    plan = cc.plan_of(c)
    assert plan.rc == 0
    o, worst = cc.operands(c, plan=plan)
    assert worst < 1.0
    ref = cc.reference(c, o, bf16=cc.rounds_to_bf16(c, plan))[0]
    L = Launch(c, o, act=cc.ACTS[c.act])
    out = L.outputs(c.B)
    name = L.run(out)
    assert name == conv_plan.kernel_name(plan, c.nchw, c.subpixel), (c.name, name, "the case table's plan_of does not describe the real launch")
    first = L.read(out, c.B)
    L.assert_surroundings_untouched(out, "first launch")
    if L.ws is not None:
        assert bool((L.ws_all[c.ws_floats:] == SENTINEL).all()), "%s: wrote past the %d floats of workspace it was lent" % (c.name, c.ws_floats)
        if plan.splitk:
            assert not bool((L.ws == SENTINEL).all())
    # a second launch into the same buffers (stale partials in the workspace) gives the same bits
    assert L.run(out) == name
    second = L.read(out, c.B)
    L.assert_surroundings_untouched(out, "second launch")
    for got, what in ((first, "first launch"), (second, "second launch into the same buffers")):
        for t, tname in zip(got, ("y", "y2")):
            if t is not None and not torch.equal(t, ref):
                raise AssertionError("%s, %s, %s [%s]: %s" % (c.name, what, tname, name, _where(c, plan, ~(t == ref), L.H, L.W)))   # NaN counts as wrong
    assert (first[1] is not None) == bool(c.y2)
    if c.B > 1:                                                # frames are independent: the last one alone, same bits
        out1 = L.outputs(1)
        L.run(out1, first_frame=c.B - 1)
        L.assert_surroundings_untouched(out1, "last frame alone")
        for t, tname in zip(L.read(out1, 1), ("y", "y2")):
            if t is not None and not torch.equal(t, ref[c.B - 1:]):
                raise AssertionError("%s, last frame alone, %s: %s" % (c.name, tname, _where(c._replace(B=1), plan, ~(t == ref[c.B - 1:]), L.H, L.W)))
    return name


@pytest.mark.parametrize("c", cc.CASES, ids=lambda c: c.name)
def test_conv_is_exact_on_small_integers(c):
    print("%s -> %s" % (c.name, check_case(c)))


def test_dilated_halo_tiles_at_dilation_6_and_12_are_exact():
    """The dilation-6 / 12 halo tiles are opt-in through BTS_CONV_HALO_DIL=2, which the library reads once per process:
    their cases run together in one fresh child process that sets it."""
    env = dict(os.environ, **cc.DIL2_ENV)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [c.name for c in cc.DIL2_CASES], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    txt = r.stdout.decode()
    print(txt)
    assert r.returncode == 0, txt[-4000:]
    if not os.environ.get("BTS_CONV_PRECISION", "0").strip() == "1":
        assert txt.count(",dil>") == len(cc.DIL2_CASES), txt


U = 2.0 ** -24                    # one fp32 rounding, relative
E_ACT = {"elu": 8.0 + 0.37 + 2.0 + 1.0, "sigmoid": 2.0 + 13.0}


@pytest.mark.parametrize("act", ["elu", "sigmoid"])
@pytest.mark.parametrize("name", cc.FLOAT_CASES)
def test_conv_float_activations(name, act):
    """ELU / sigmoid behind an exact pre-activation: the case's integer operands with e1 = (2^-k, 0), k the smallest that
    puts the exact pre-activation v in [-8, 8], and the case's own e2 (|scale| <= 2).  Against fp64 ELU / sigmoid of v,
    per element, in units of U = 2^-24 and relative to max(1, |ref|):

        |got - ref| <= (|e2 scale| * E_act + 1.01 * max(1, |ref|)) * U

    E_act, the absolute error of the activation, term by term (common.h: elu1 = __expf(x) - 1 for x <= 0, sigmoid1 =
    __frcp_rn(1 + __expf(-x)); __expf(x) is the hardware 2^t, documented at 1 ulp = 2 U relative, of t = x * log2(e)):
      one fp32 rounding of the e1 result: |v| <= 8, so 8 U (on these operands e1 is exact; the term stays), through an
        activation of slope <= 1 (ELU) or <= 1/4 (sigmoid): 8 U or 2 U;
      ELU: rounding t moves e^x by |x| U relative, |x| e^x <= 1/e: 0.37 U; the 1-ulp exponential, e^x <= 1: 2 U; the
        subtraction, result in (-1, 0]: 1 U.  E_elu = 8 + 0.37 + 2 + 1 = 11.37 U.
      sigmoid: e = e^-x carries (|x| + 2) U <= 10 U relative; 1 + e one rounding, U relative; the hardware reciprocal is
        documented at 1 ulp, 2 U relative (a correctly rounded division would be U); the result s = 1 / (1 + e) <= 1 so
        carries at most (10 e / (1 + e) + 1 + 2) U <= 13 U.  E_sigmoid = 2 + 13 = 15 U.
    then e2 scales that error by |scale| and rounds once: U * |result|, 1.01 covering result vs ref.
    Observed max error / bound on the MI355X (information, not a threshold): see DESIGN.md."""
    c0 = cc.BY_NAME[name]
    c = c0._replace(e1=True, act=act, res=False)
    plan = cc.plan_of(c)
    assert plan.rc == 0
    vmax = cc.reference(c, cc.operands(c, plan=plan, e1_pow2=0)[0])[1].abs().max().item()      # the pre-activation at e1 = (1, 0)
    k = 0
    while vmax * 2.0 ** -k > 8.0:
        k += 1
    o, _ = cc.operands(c, plan=plan, e1_pow2=k)
    ref, v, _ = cc.reference(c, o)
    assert v.abs().max().item() <= 8.0 and v.abs().max().item() > 2.0
    L = Launch(c, o, act=cc.ACTS[act])
    out = L.outputs(c.B)
    kern = L.run(out)
    got = L.read(out, c.B)[0]
    s2 = o.e2[0].abs() if o.e2 is not None else torch.ones(ref.shape[-1], dtype=torch.float64)
    bound = (s2 * E_ACT[act] + 1.01 * ref.abs().clamp_min(1.0)) * U
    err = (got - ref).abs()
    ratio = (err / bound).max().item()
    print("%s %s [%s] e1 = 2^-%d: max |err| / bound = %.4f" % (name, act, kern, k, ratio))
    assert bool((err <= bound).all()), (name, act, kern, ratio)


# train.conv2d(...).backward: (name, B, C, h, w, c_out, k, stride, pad, dil, up, groups, kernel the dgrad launch must be on)
DGRAD_CASES = [
    ("k1", 2, 32, 5, 7, 64, 1, 1, 0, 1, 1, 1, None),
    # 544 nominal 64-row tiles: no split-K; 64 input channels: a tile width that Winograd (fp32) and the bf16x3 halo tile both have
    ("k3_on_a_geometry_kernel", 1, 64, 68, 64, 32, 3, 1, 1, 1, 1, 1, ("conv_wino", "conv_halo")),
    ("k3_row_tiled", 2, 32, 5, 7, 32, 3, 1, 1, 1, 1, 1, ("conv_fwd",)),
    ("k3_dil3", 1, 32, 9, 11, 64, 3, 1, 3, 3, 1, 1, None),
    ("k3_stride2", 2, 32, 9, 13, 64, 3, 2, 1, 1, 1, 1, None),
    ("k1_stride2_downsample", 2, 64, 9, 13, 128, 1, 2, 0, 1, 1, 1, None),
    ("k3_up2", 2, 32, 5, 7, 32, 3, 1, 1, 1, 2, 1, None),
    ("grouped_4_per_group", 2, 128, 6, 8, 128, 3, 1, 1, 1, 1, 32, None),
    ("grouped_32_per_group", 2, 64, 6, 8, 64, 3, 1, 1, 1, 1, 2, None),
]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda v: v[0])
def test_input_gradient_is_exact(case):
    """x.grad of train.conv2d on integer x, w and gy equals fp64 autograd of F.conv2d bit for bit: pins the flipped,
    transposed packing (WeightPacker.DGRAD), pad' = dil * (k - 1) - pad, the zero-inserted adjoint of stride 2, the sum
    over the 2x2 block of up = 2 and the block-diagonal bundles of grouped weights."""
    from bts_amd import train
    name, B, C, h, w, cout, k, stride, pad, dil, up, groups, kernels = case
    g = torch.Generator().manual_seed(cc.zlib.crc32(name.encode()))
    H, W = conv_plan.conv_out_hw(h, w, k, dil, stride, pad, up)
    x = torch.randint(-511, 512, (B, C, h, w), generator=g).double()
    wt = torch.randint(-3, 4, (cout, C // groups, k, k), generator=g).double()
    gy = torch.randint(-511, 512, (B, cout, H, W), generator=g).double()

    def autograd(x, wt, gy):
        x = x.clone().requires_grad_(True)
        xu = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if up == 2 else x
        F.conv2d(xu, wt, stride=stride, padding=pad, dilation=dil, groups=groups).backward(gy)
        return x.grad
    ref = autograd(x, wt, gy)
    assert autograd(x, wt.abs(), gy.abs()).max().item() < 2 ** 24          # sum |w| * |gy| per input element: fp32 stays exact
    xd = x.float().cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wd = wt.float().cuda().requires_grad_(True)
    trace = ops.KernelTrace()
    ops.set_trace(trace)
    try:
        y = train.conv2d(xd, wd, padding=pad, dilation=dil, stride=stride, up=up, groups=groups)
        y.backward(gy.float().cuda().contiguous(memory_format=torch.channels_last))
    finally:
        ops.set_trace(None)
    torch.cuda.synchronize()
    dgrad = [r[0] for r in trace.records if r[1].endswith(".dgrad")]
    assert len(dgrad) == 1
    print("%s: dgrad on %s" % (name, dgrad[0]))
    if kernels is not None:
        assert dgrad[0].startswith(kernels), dgrad[0]
    got = xd.grad.cpu().double()
    if not torch.equal(got, ref):
        bad = ~(got == ref)
        raise AssertionError("%s [%s]: %d wrong of %d, first (b, c, y, x) = %s" % (name, dgrad[0], int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist()))


if __name__ == "__main__":
    for case_name in sys.argv[1:]:
        print("%s -> %s" % (case_name, check_case(cc.BY_NAME[case_name])), flush=True)
