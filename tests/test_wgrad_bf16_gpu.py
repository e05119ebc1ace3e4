"""bts_conv_wgrad_bf16_f32 / bts_conv_wgrad_batch_bf16_f32 (csrc/wgrad.hip: wgrad_tile's BF16 body in its four tiles) on
the case tables of tests/wgrad_cases.py and tests/wgrad_batch_cases.py.

The statement under test:  dw = sum_p bf16(dy[p][co]) * bf16(x'[q][ci]),  x' = the gathered input after its prologue with
zero padding applied after it, both operands rounded to nearest even, fp32 accumulation, and tile, split, pix_per_split
and the fixed-order split sum of the fp32 entry point.  The reference is therefore never a plain fp64 gradient but fp64
arithmetic on operands rounded on the CPU with ``.to(torch.bfloat16)`` (tests/test_wgrad_gpu.py's `reference` on them).

* exact: integers |v| <= 127 are bf16 values, every partial sum is an integer below 2^24, so neither the rounding nor any
  summation order can change a bit: torch.equal on every case -- any mistake in the pixel pairing, the operand map, a
  loader role or a ragged tail shows on the tile and split it lives in.
* rounding: operands that are not bf16 values, within the project's bf16 bound 2e-6 * sum|terms| (tests/test_bf16_gpu.py)
  of the rounded-operand reference; the fp32 entry point misses that reference by more than the bound.
* the split sum, the exponent range and the batch launch."""
import zlib

import numpy as np
import pytest
import torch

import wgrad_batch_cases as bc
import wgrad_cases as wc
from bts_amd import ops
from conftest import fp32_only
from test_wgrad_batch_gpu import _build
from test_wgrad_gpu import SENTINEL, _slice_of_wider, reference

pytestmark = [pytest.mark.gpu, fp32_only]

BAND = 1024                      # sentinel floats on either side of dw
BF16_BOUND = 2e-6                # x sum|terms|: fp32 accumulation of exact bf16 products (tests/test_bf16_gpu.py)


def _gen(c, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + 77 + salt)


def _bf16(t):
    """fp64 -> the fp64 value of the nearest bf16 (ties to even) of its fp32 value."""
    return t.float().to(torch.bfloat16).double()


def rounded_reference(c, x, dy, scale=None, shift=None):
    """(fp64 dw, sum |terms|) of the bf16 statement: prologue in fp64 (the tests keep it exact in fp32), rounding, then
    the plain definition -- whose zero padding comes after."""
    if scale is not None:
        x = x * scale + shift
        if c.pre_relu:
            x = x.clamp_min(0.0)
    return reference(c, _bf16(x), _bf16(dy))


def _launch(c, x, dy, scale, shift, ws, precision="bf16", band=False):
    """One ops.conv_wgrad launch of case `c`; with `band`, dw sits between two sentinel bands: returns (dw, whole buffer)."""
    nb = max(c.n_bundles, 1)
    x2d = _slice_of_wider(x.reshape(-1, nb * c.c_in).float(), c.x_extra)
    dy2d = _slice_of_wider(dy.reshape(-1, nb * c.c_out).float(), c.dy_extra)
    pre = None if scale is None else (scale.float().cuda(), shift.float().cuda())
    n = nb * c.c_out * c.ksize * c.ksize * c.c_in
    buf = torch.full((n + 2 * BAND,), SENTINEL, device="cuda") if band else None
    dw = ops.conv_wgrad(x2d, c.B, c.h, c.w, c.c_in, dy2d, c.c_out, c.ksize, dil=c.dil, stride=c.stride, pad=c.pad, up=c.up,
                        ws=ws, n_bundles=c.n_bundles, pre=pre, pre_relu=c.pre_relu, precision=precision,
                        dw=None if buf is None else buf[BAND:BAND + n])
    return (dw, buf) if band else dw


def _integer_operands(c, g):
    """|x'| <= 127 and |dy| <= 1 as integers: x in [-59, 59], scale 1 or 2, shift in [-9, 9] where a prologue rides along."""
    H, W = wc.out_hw(c)
    nb = max(c.n_bundles, 1)
    scale = shift = None
    if c.pre:
        x = torch.randint(-59, 60, (c.B, c.h, c.w, nb * c.c_in), generator=g).double()
        scale = torch.randint(1, 3, (nb * c.c_in,), generator=g).double()
        shift = torch.randint(-9, 10, (nb * c.c_in,), generator=g).double()
    else:
        x = torch.randint(-127, 128, (c.B, c.h, c.w, nb * c.c_in), generator=g).double()
    dy = torch.randint(-1, 2, (c.B, H, W, nb * c.c_out), generator=g).double()
    return x, dy, scale, shift


@pytest.mark.parametrize("c", wc.CASES, ids=lambda c: c.name)
def test_bf16_wgrad_is_exact_on_small_integers(c):
    x, dy, scale, shift = _integer_operands(c, _gen(c))
    nb = max(c.n_bundles, 1)
    ref, mag = reference(c, x, dy, scale, shift)
    xq = x if scale is None else x * scale + shift
    assert xq.abs().max().item() <= 127 and torch.equal(_bf16(xq), xq), "operands must be bf16 values"
    assert mag.max().item() < 2 ** 24, "case breaks the exactness precondition"
    plan = ops.conv_wgrad_plan(c.B, c.h, c.w, c.c_in, c.c_out, c.ksize, dil=c.dil, stride=c.stride, pad=c.pad, up=c.up,
                               ws_floats=c.ws_floats, n_bundles=c.n_bundles, pre=c.pre, pre_relu=c.pre_relu,
                               x_pix_stride=nb * c.c_in + c.x_extra, dy_pix_stride=nb * c.c_out + c.dy_extra, precision="bf16")
    assert plan == wc.plan_of(c)
    split = plan[2]
    ws = None if c.ws_floats is None else torch.full((c.ws_floats,), SENTINEL, device="cuda")
    dw, buf = _launch(c, x, dy, scale, shift, ws, band=True)
    got = dw.cpu().double().reshape(ref.shape)
    assert bool((buf[:BAND] == SENTINEL).all()) and bool((buf[BAND + dw.numel():] == SENTINEL).all()), "the launch wrote outside dw"
    if ws is not None:
        used = split * dw.numel() if split > 1 else 0
        assert used <= c.ws_floats
        assert bool((ws[used:] == SENTINEL).all()), "the launch wrote workspace beyond split * c_out * N * n_bundles"
        assert not bool((ws[:used] == SENTINEL).any()), "a partial tile inside the workspace was never written"
    if not torch.equal(got, ref):
        bad = ~(got == ref)                                     # NaN counts as wrong
        j, co, tap, ci = bad.nonzero()[0].tolist()
        bm, bn = plan[:2]
        n = tap * c.c_in + ci
        pytest.fail("%s: %d wrong of %d; first (bundle %d, co %d, tap %d, ci %d): tile %dx%d at (m %d, n %d), 32x32 sub-tile "
                    "(%d, %d), split %d x %d pixels" % (c.name, int(bad.sum()), bad.numel(), j, co, tap, ci, bm, bn, co // bm,
                                                        n // bn, (co % bm) // 32, (n % bn) // 32, split, plan[3]))


def _float_operands(c, g):
    """Standard-normal dy; x standard-normal too, or -- where a prologue rides along -- on a 2^-10 grid with scale in
    {0.5, 1, 2} and shift on the same grid, so that relu(x * scale + shift) is exact in fp32, fused or not, and the
    rounding the test is about is the only one (17 significant bits: not a bf16 value)."""
    H, W = wc.out_hw(c)
    nb = max(c.n_bundles, 1)
    x = torch.randn(c.B, c.h, c.w, nb * c.c_in, generator=g).double()
    dy = torch.randn(c.B, H, W, nb * c.c_out, generator=g).double()
    scale = shift = None
    if c.pre:
        q = lambda t: (t.double().clamp(-8.0, 8.0) * 1024.0).round() / 1024.0
        x = q(x)
        scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (nb * c.c_in,), generator=g)]
        shift = q(torch.randn(nb * c.c_in, generator=g))
    return x, dy, scale, shift


ROUNDING_CASES = wc.FLOAT_CASES + ["t32_up2_relu"]


@pytest.mark.parametrize("name", ROUNDING_CASES)
def test_bf16_wgrad_rounds_both_operands_to_nearest_even_after_the_prologue(name):
    c = wc.BY_NAME[name]
    assert (name == "t32_up2_relu") == bool(c.pre and c.pre_relu)
    x, dy, scale, shift = _float_operands(c, _gen(c))
    ref, mag = rounded_reference(c, x, dy, scale, shift)
    ws = None if c.ws_floats is None else torch.empty(c.ws_floats, device="cuda")
    got = _launch(c, x, dy, scale, shift, ws).cpu().double().reshape(ref.shape)
    fp32 = _launch(c, x, dy, scale, shift, ws, precision="fp32").cpu().double().reshape(ref.shape)
    bound = BF16_BOUND * mag
    err, err32 = (got - ref).abs(), (fp32 - ref).abs()
    worst, worst32 = (err / bound.clamp_min(1e-300)).max().item(), (err32 / bound.clamp_min(1e-300)).max().item()
    print("%s: max |err| / bound: bf16 %.4f, fp32 entry point %.2f" % (name, worst, worst32))
    assert torch.isfinite(got).all()
    assert bool((err <= bound).all()), (name, worst)
    assert worst32 > 1.0, "the fp32 entry point must miss the rounded-operand reference: %r" % ((name, worst32),)


@pytest.mark.parametrize("name", wc.FLOAT_CASES)
def test_bf16_dw_is_the_documented_fixed_order_sum_of_the_partials(name):
    c = wc.BY_NAME[name]
    x, dy, _, _ = _float_operands(c, _gen(c, 1))
    split = wc.plan_of(c)[2]
    assert split > 1
    ws = torch.full((c.ws_floats,), SENTINEL, device="cuda")
    dw = _launch(c, x, dy, None, None, ws).cpu()
    partials = ws[:split * dw.numel()].cpu().numpy().reshape(split, -1)
    assert not np.isnan(partials).any() and not (partials == np.float32(SENTINEL)).any()
    want = torch.from_numpy(wc.sum_splits(partials)).reshape(dw.shape)
    assert torch.equal(dw, want), "%s, split %d: %d of %d elements differ" % (name, split, int((dw != want).sum()), dw.numel())


@pytest.mark.parametrize("name", ["t64_s7", "t32_s84_k3"])
def test_bf16_wgrad_has_the_exponent_range_of_fp32(name):
    """Both operands scaled by 2^40, and by 2^-40: finite, and exactly the unscaled result times 2^80 / 2^-80 (a bf16 has
    fp32's exponent; scaling by a power of two commutes with every rounding while nothing overflows or goes subnormal)."""
    c = wc.BY_NAME[name]
    x, dy, _, _ = _float_operands(c, _gen(c, 2))
    ws = torch.empty(c.ws_floats, device="cuda")
    base = _launch(c, x, dy, None, None, ws).cpu()
    assert torch.isfinite(base).all() and float(base.abs().max()) > 1.0
    for e in (40, -40):
        got = _launch(c, x * 2.0 ** e, dy * 2.0 ** e, None, None, ws).cpu()
        assert torch.isfinite(got).all(), (name, e)
        assert torch.equal(got, base * 2.0 ** (2 * e)), (name, e, int((got != base * 2.0 ** (2 * e)).sum()))


@pytest.mark.parametrize("name", list(bc.BATCHES))
def test_bf16_batch_launch_has_the_bits_of_the_single_launches(name):
    """The batch of tests/test_wgrad_batch_gpu.py's exact data: integers up to 511 (more bits than a bf16 holds, so the
    rounding shows) times {-1, 0, 1}.  Rounded integers are integers and every partial sum stays below 2^24, so the split --
    which the batch planner and the single planner choose differently -- cannot change a bit: the batched bf16 launch, the
    single bf16 launches on the same views and the fp64 statement on rounded operands agree bitwise."""
    ws_floats, cases = bc.BATCHES[name]
    problems, bases = _build(name, True)
    batch = ops.WgradBatch(problems, bases, ws_floats)
    ws = torch.full((ws_floats,), SENTINEL, device="cuda")
    dws = [d.clone() for d in batch.run(bases, ws, precision="bf16")]
    planned = torch.zeros(ws_floats, dtype=torch.bool, device="cuda")
    for c, (_, _, split, _, off) in zip(cases, batch.plan):
        if split > 1:
            planned[off:off + split * bc.dw_floats(c)] = True
    assert bool(((ws != SENTINEL) == planned).all()), "the launch must write exactly the planned workspace regions"
    ws1 = torch.empty(1 << 20, device="cuda")
    differs = False
    for c, pr, dw in zip(cases, problems, dws):
        single = ops.conv_wgrad(pr["x"], c.B, c.h, c.w, c.c_in, pr["dy"], c.c_out, c.ksize, dil=c.dil, stride=c.stride, pad=c.pad,
                                up=c.up, ws=ws1, n_bundles=c.n_bundles, pre=pr.get("pre"), pre_relu=c.pre_relu, precision="bf16")
        assert torch.equal(dw.view(-1), single.view(-1)), "%s / %s: %d elements differ" % (name, c.name, int((dw.view(-1) != single.view(-1)).sum()))
        nb = max(c.n_bundles, 1)
        x = pr["x"].cpu().double().reshape(c.B, c.h, c.w, -1)[..., :nb * c.c_in]
        dy = pr["dy"].cpu().double().reshape(c.B, *wc.out_hw(c), -1)[..., :nb * c.c_out]
        pre = pr.get("pre")
        scale, shift = (None, None) if pre is None else (pre[0].cpu().double(), pre[1].cpu().double())
        ref, _ = rounded_reference(c, x, dy, scale, shift)
        assert torch.equal(dw.cpu().double().reshape(ref.shape), ref), (name, c.name)
        differs = differs or not torch.equal(ref, reference(c, x, dy, scale, shift)[0])
    assert differs, "the batch's data must show the rounding"
