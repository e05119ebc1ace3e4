"""bts_conv_wgrad_f32 (csrc/wgrad.hip: conv_wgrad_kernel in its four tiles + wgrad_reduce_kernel) against a plain fp64
statement of the weight gradient on the CPU, on every case of tests/wgrad_cases.py -- each tile split and unsplit, ragged
tile edges, short last splits, every gather mode, channel slices of wider buffers.

The exact test feeds small integers, so that every partial sum is an integer below 2^24 and fp32 accumulation is exact
in any order: the tile, the split and the reduction order cannot change a bit, and the assertion is torch.equal.  The
float-valued test pins fp32 products (small integers are exact in lower precision too) under the worst-case bound of
an fp32 summation chain.  Which tile and split ran comes from ops.conv_wgrad_plan."""
import zlib

import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as wc
from bts_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -12345.671875          # not an integer: no exact-test partial sum can equal it


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()))


def reference(c, x, dy, scale=None, shift=None):
    """fp64 dw [nb, c_out, taps, c_in] and the matching sum of |dy| * |x_tap|, from the definition: per tap, the shifted
    view of [relu](x * scale + shift) -> nearest-2x -> zero padding, sampled with stride and dilation, then dy^T @ view.
    x: [B, h, w, nb * c_in], dy: [B, H, W, nb * c_out], both fp64."""
    H, W = wc.out_hw(c)
    nb = max(c.n_bundles, 1)
    if scale is not None:
        x = x * scale + shift
        if c.pre_relu:
            x = x.clamp_min(0.0)
    if c.up == 2:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    xp = F.pad(x, (0, 0, c.pad, c.pad, c.pad, c.pad))                # zero padding after the prologue
    M = c.B * H * W
    taps = c.ksize * c.ksize
    ref = torch.empty(nb, c.c_out, taps, c.c_in, dtype=torch.float64)
    mag = torch.empty_like(ref)
    dy2 = dy.reshape(M, nb * c.c_out)
    for ky in range(c.ksize):
        for kx in range(c.ksize):
            y0, x0 = ky * c.dil, kx * c.dil
            view = xp[:, y0:y0 + (H - 1) * c.stride + 1:c.stride, x0:x0 + (W - 1) * c.stride + 1:c.stride, :]
            assert view.shape[1:3] == (H, W)
            v2 = view.reshape(M, nb * c.c_in)
            for j in range(nb):
                d, v = dy2[:, j * c.c_out:(j + 1) * c.c_out], v2[:, j * c.c_in:(j + 1) * c.c_in]
                ref[j, :, ky * c.ksize + kx, :] = d.t() @ v
                mag[j, :, ky * c.ksize + kx, :] = d.abs().t() @ v.abs()
    return ref, mag


def _slice_of_wider(values, extra):
    """`values` [rows, C] as a channel slice, at a non-zero offset, of a CUDA buffer `extra` channels wider whose other
    channels are NaN (any read outside the slice poisons the result)."""
    rows, C = values.shape
    if extra == 0:
        return values.cuda()
    assert extra % 8 == 0
    buf = torch.full((rows, C + extra), float("nan"), device="cuda")
    view = buf[:, extra // 2:extra // 2 + C]
    view.copy_(values)
    return view


def _run(c, x, dy, scale, shift, ws):
    nb = max(c.n_bundles, 1)
    x2d = _slice_of_wider(x.reshape(-1, nb * c.c_in).float(), c.x_extra)
    dy2d = _slice_of_wider(dy.reshape(-1, nb * c.c_out).float(), c.dy_extra)
    pre = None if scale is None else (scale.float().cuda(), shift.float().cuda())
    call = lambda: ops.conv_wgrad(x2d, c.B, c.h, c.w, c.c_in, dy2d, c.c_out, c.ksize, dil=c.dil, stride=c.stride, pad=c.pad,
                                  up=c.up, ws=ws, n_bundles=c.n_bundles, pre=pre, pre_relu=c.pre_relu)
    return call


def _where(c, plan, bad):
    """First wrong element, its 32x32 sub-tile and the split geometry, for the failure message."""
    bm, bn, split, pps = plan
    idx = bad.nonzero()[0].tolist()
    j, co, tap, ci = idx
    n = tap * c.c_in + ci
    return ("%d wrong of %d; first (bundle %d, co %d, tap %d, ci %d): tile %dx%d at (m %d, n %d), 32x32 sub-tile (%d, %d), "
            "split %d x %d pixels" % (int(bad.sum()), bad.numel(), j, co, tap, ci, bm, bn, co // bm, n // bn, (co % bm) // 32,
                                     (n % bn) // 32, split, pps))


@pytest.mark.parametrize("c", wc.CASES, ids=lambda c: c.name)
def test_wgrad_is_exact_on_small_integers(c):
    g = _gen(c)
    H, W = wc.out_hw(c)
    M = c.B * H * W
    nb = max(c.n_bundles, 1)
    plan = wc.plan_of(c)
    split = plan[2]
    # |x| <= 511 (10 bits: not representable in bf16) unless that many pixels could reach 2^24; the precondition is asserted below
    xmax = min(511, int(0.6 * 2 ** 24 * 3 / (M * (2 if c.pre else 1))))
    assert xmax >= 300
    scale = shift = None
    if c.pre:
        x = 2.0 * torch.randint(-(xmax // 2), xmax // 2 + 1, (c.B, c.h, c.w, nb * c.c_in), generator=g).double()
        scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (nb * c.c_in,), generator=g)]
        shift = torch.randint(-9, 10, (nb * c.c_in,), generator=g).double()
        assert (shift < 0).any() and (shift > 0).any()
    else:
        x = torch.randint(-xmax, xmax + 1, (c.B, c.h, c.w, nb * c.c_in), generator=g).double()
    dy = torch.randint(-1, 2, (c.B, H, W, nb * c.c_out), generator=g).double()
    ref, mag = reference(c, x, dy, scale, shift)
    assert mag.max().item() < 2 ** 24, "case breaks the exactness precondition: shrink the range of x"

    ws = None if c.ws_floats is None else torch.full((c.ws_floats,), SENTINEL, device="cuda")
    call = _run(c, x, dy, scale, shift, ws)
    first = call().cpu().double().reshape(ref.shape)
    if ws is not None:
        used = split * nb * c.c_out * c.ksize * c.ksize * c.c_in if split > 1 else 0
        assert used <= c.ws_floats
        assert bool((ws[used:] == SENTINEL).all()), "the launch wrote workspace beyond split * c_out * N * n_bundles"
        assert not bool((ws[:used] == SENTINEL).any()), "a partial tile inside the workspace was never written"
    second = call().cpu().double().reshape(ref.shape)          # same workspace, now holding the first call's partials
    for got, what in ((first, "first call"), (second, "second call into the same workspace")):
        if not torch.equal(got, ref):
            bad = ~(got == ref)                                 # NaN counts as wrong
            pytest.fail("%s, %s: %s" % (c.name, what, _where(c, plan, bad)))


@pytest.mark.parametrize("name", wc.FLOAT_CASES)
def test_wgrad_fp32_products_within_the_summation_bound(name):
    """Standard-normal operands.  Per element |got - ref| <= (pix_per_split + split + 2) * 2^-24 * sum |dy| * |x_tap|: the
    worst case of one fp32 rounding per product, a chain of at most pix_per_split additions inside a split and split
    more across them.  Observed max error / bound on the MI355X (information, not a threshold): see DESIGN.md."""
    c = wc.BY_NAME[name]
    g = _gen(c)
    H, W = wc.out_hw(c)
    bm, bn, split, pps = wc.plan_of(c)
    x = torch.randn(c.B, c.h, c.w, c.c_in, generator=g)
    dy = torch.randn(c.B, H, W, c.c_out, generator=g)
    ref, mag = reference(c, x.double(), dy.double())
    ws = None if c.ws_floats is None else torch.empty(c.ws_floats, device="cuda")
    got = _run(c, x, dy, None, None, ws)().cpu().double().reshape(ref.shape)
    bound = (pps + split + 2) * 2.0 ** -24 * mag
    err = (got - ref).abs()
    ratio = (err / bound).max().item()
    print("%s: tile %dx%d split %d x %d pixels: max |err| / bound = %.4f" % (name, bm, bn, split, pps, ratio))
    assert bool((err <= bound).all()), (name, ratio)


@pytest.mark.parametrize("name", wc.FLOAT_CASES)
def test_dw_is_the_documented_fixed_order_sum_of_the_partials(name):
    """Float operands, where the summation order shows: after a split launch the workspace still holds the partials as
    [split][bundle][c_out][N]; dw has the bits of wc.sum_splits over them.  The splits (16, 126, 84, 7, 768) reach fewer
    splits than lanes, the one-at-a-time loop alone and the four-at-a-time loop with a tail."""
    c = wc.BY_NAME[name]
    g = _gen(c)
    H, W = wc.out_hw(c)
    bm, bn, split, pps = wc.plan_of(c)
    assert split > 1
    x = torch.randn(c.B, c.h, c.w, c.c_in, generator=g)
    dy = torch.randn(c.B, H, W, c.c_out, generator=g)
    ws = torch.full((c.ws_floats,), SENTINEL, device="cuda")
    dw = _run(c, x, dy, None, None, ws)().cpu()
    partials = ws[:split * dw.numel()].cpu().numpy().reshape(split, -1)
    want = torch.from_numpy(wc.sum_splits(partials)).reshape(dw.shape)
    assert torch.equal(dw, want), "%s, split %d: %d of %d elements differ" % (name, split, int((dw != want).sum()), dw.numel())


@pytest.mark.parametrize("tile,c", wc.PATH_CASES, ids=lambda v: v.name if hasattr(v, "name") else "%dx%d" % v)
def test_training_path_hands_wgrad_the_same_problem(tile, c):
    """train.conv2d(...).backward gives the same weight.grad bits as ops.conv_wgrad on the same views with a workspace
    of the training path's size, on the tile the case was chosen for."""
    from bts_amd import train
    assert wc.plan_of(c)[:2] == tile
    g = _gen(c)
    H, W = wc.out_hw(c)
    x_rows = torch.randn(c.B, c.h, c.w, c.c_in, generator=g).cuda()           # NHWC storage: train.conv2d takes views of it
    gy_rows = torch.randn(c.B, H, W, c.c_out, generator=g).cuda()
    wt = (torch.randn(c.c_out, c.c_in, c.ksize, c.ksize, generator=g) / (c.c_in * c.ksize * c.ksize) ** 0.5).cuda().requires_grad_(True)
    y = train.conv2d(x_rows.permute(0, 3, 1, 2), wt, padding=c.pad, dilation=c.dil, stride=c.stride, up=c.up)
    assert tuple(y.shape) == (c.B, c.c_out, H, W)
    y.backward(gy_rows.permute(0, 3, 1, 2))
    ws = torch.empty(train.WGRAD_WS_FLOATS, device="cuda")
    dw = ops.conv_wgrad(x_rows.view(-1, c.c_in), c.B, c.h, c.w, c.c_in, gy_rows.view(-1, c.c_out), c.c_out, c.ksize, dil=c.dil,
                        stride=c.stride, pad=c.pad, up=c.up, ws=ws)
    want = dw.reshape(c.c_out, c.ksize, c.ksize, c.c_in).permute(0, 3, 1, 2)
    assert torch.equal(wt.grad, want)
