"""The forward half of the decoder's LPG stage on the GPU against fp64: every dispatch row of bts_reduc_fwd_f32 and
bts_reduc_lpg_fwd_f32 (csrc/reduc.hip), every branch of launch_lpg behind bts_lpg_fused_fwd_f32 and bts_lpg_bwd_f32
(csrc/lpg.hip), with the clamp of csrc/lpg_math.h inside every comparison.  Cases, references, metrics and the derived
bounds are in tests/reduc_lpg_cases.py; tests/test_reduc_lpg_cases_host.py asserts their preconditions on the CPU.

Bars.  Chain-fed outputs: 4 x FLOORS (the CPU fp32 oracle's distance from the fp64 oracle on the same case -- the margin
this project gives a different fp32 summation order, here MFMA accumulation, and one hardware reciprocal) plus
reduc_lpg_cases.activation_terms: what the stated error of elu1 / sigmoid1 (csrc/common.h) can do to that output, first
order and worst case through the case's own chain; derivation in that function's docstring.  Given-plane outputs: the
per-pixel rounding bound of reduc_lpg_cases.given_bound.  No pixel is left out of any comparison: the references keep
every denominator 20 % away from +-1e-3 and 1e-6 away from 0, the constructed zero cell excepted, which must come out as
the oracle's signed infinity.  Every output lives in a slab of sentinels that must survive."""
import numpy as np
import pytest
import torch

import reduc_lpg_cases as C
from bts_amd import ops

pytestmark = pytest.mark.gpu

MD = C.MD
PAD = 64                            # sentinel floats on both sides of an output: a multiple of 4, so the view stays 16-byte aligned


class Slab:
    """n floats in the middle of a flat sentinel buffer."""

    def __init__(self, n, fill=C.SENTINEL):
        self.whole = torch.full((n + 2 * PAD,), C.SENTINEL, device="cuda")
        self.view = self.whole[PAD:PAD + n]
        self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 0

    def check(self, what):
        assert bool((self.whole[:PAD] == C.SENTINEL).all()) and bool((self.whole[-PAD:] == C.SENTINEL).all()), what + ": wrote outside its output"


def _x_view(x):
    """[B,c,h,w] -> a [npix, c] column slice of a buffer X_PAD columns wider whose other columns are NaN."""
    B, c, h, w = x.shape
    buf = torch.full((B * h * w, c + C.X_PAD), float("nan"), device="cuda")
    buf[:, C.X_OFF:C.X_OFF + c] = x.permute(0, 2, 3, 1).reshape(-1, c).cuda()
    return buf[:, C.X_OFF:C.X_OFF + c]


def _frag(ws):
    return ops.pack_reduc_weights([wt.cuda() for wt in ws])


def run_fwd(row, x, ws, normalize, strided=True):
    """bts_reduc_fwd_f32: [B,4,h,w] planes or the final [B,1,h,w] map, on the CPU."""
    B, c, h, w = x.shape
    xv = _x_view(x) if strided else x.permute(0, 2, 3, 1).reshape(-1, c).cuda().contiguous()
    out = Slab(B * h * w * (1 if row.final else 4))
    ops.reduc_forward_nhwc(xv, row.c_in, row.c_first, _frag(ws), MD, row.final, bool(normalize), out.view)
    torch.cuda.synchronize()
    out.check(row.name)
    o = out.view.cpu()
    return o.view(B, 1, h, w) if row.final else o.view(B, h, w, 4).permute(0, 3, 1, 2).contiguous()


def run_lpg(row, x, ws, full=True, strided=True):
    """bts_reduc_lpg_fwd_f32 with all three optional outputs or none: dict of CPU tensors."""
    B, c, h, w = x.shape
    k = row.k
    xv = _x_view(x) if strided else x.permute(0, 2, 3, 1).reshape(-1, c).cuda().contiguous()
    depth = Slab(B * h * k * w * k)
    ds = Slab(B * 4 * h * w) if full and k > 2 else None
    p4 = Slab(B * h * w * 4) if full else None
    am = torch.full((), 123.0, device="cuda") if full else None
    ops.reduc_lpg_forward(xv, B, h, w, row.c_in, row.c_first, _frag(ws), MD, k, depth.view.view(B, 1, h * k, w * k),
                          ds_out=None if ds is None else ds.view, abs_min=am, plane4=None if p4 is None else p4.view)
    torch.cuda.synchronize()
    out = {"depth": depth.view.cpu().view(B, 1, h * k, w * k)}
    for s in (depth, ds, p4):
        if s is not None:
            s.check(row.name)
    if full:
        out["abs_min"] = am.cpu()
        out["plane4"] = p4.view.cpu().view(B, h, w, 4).permute(0, 3, 1, 2).contiguous()
        if ds is not None:
            out["ds"] = ds.view.cpu().view(B, 1, 2 * h, 2 * w)
    return out


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_planes(what, got, ref, floors, terms):
    errs = C.plane_errors(got, ref)
    bars = [4.0 * f + t for f, t in zip(floors, terms)]
    print(what, "plane errors", ["%.2e" % e for e in errs], "bars", ["%.2e" % b for b in bars])
    for c, (e, b) in enumerate(zip(errs, bars)):
        assert e <= b, (what, c, e, b)


def _check_lpg_outputs(what, row, got, ref, floors, terms):
    """depth, ds, plane4 and abs_min of a full bts_reduc_lpg_fwd_f32 run against the fp64 reference."""
    k = row.k
    assert bool(torch.isfinite(ref["depth"]).all())
    err = C.den_weighted_error(got["depth"], ref["depth"], ref["den"])
    bar = 4.0 * floors["depth"] + terms["depth"]
    print(what, "depth den-weighted error %.2e bar %.2e (4 x floor %.2e + activations %.2e)" % (err, bar, 4 * floors["depth"], terms["depth"]))
    assert err <= bar, (what, err, bar)
    _check_planes(what + " plane4", got["plane4"], ref["plane1"], floors["planes1"], terms["planes1"])
    if k > 2:
        f = k // 2
        assert _bits_equal(got["ds"], got["depth"][:, :, ::f, ::f]), what + ": ds is not depth[::f, ::f]"
        e_ds = C.den_weighted_error(got["ds"], ref["depth"][:, :, ::f, ::f], ref["den"][:, ::f, ::f])
        assert e_ds <= bar, (what, "ds", e_ds, bar)
    # |den| minimum: a plane component is within (4 floor_c + term_c) max|n_c| of fp64, |u|, |v| < 1/2, and the FMAs
    am_bar = terms["den_abs"] + 4.0 * sum(wgt * fl * float(ref["plane1"][:, c].abs().max())
                                          for c, (wgt, fl) in enumerate(zip((0.5, 0.5, 1.0), floors["planes1"])))
    am_err = abs(float(got["abs_min"]) - float(ref["abs_min"]))
    print(what, "abs_min error %.2e bar %.2e" % (am_err, am_bar))
    assert am_err <= am_bar, (what, am_err, am_bar)


# ------------------------------------------------------------------------------------------ 1. bts_reduc_fwd_f32 rows
@pytest.mark.parametrize("name,normalize", [(r.name, n) for r in C.FWD_ROWS for n in ((0,) if r.final else (0, 1))])
def test_reduc_fwd_row(name, normalize):
    row, ref = C.ROWS[name], C.row_reference(name)
    terms, fl = C.cached(("terms", name), lambda: C.activation_terms(ref, row)), C.FLOORS[name]
    got = run_fwd(row, ref["x"], ref["ws"], normalize)
    if row.final:
        err = C.plane_errors(got, ref["out"])[0]
        bar = 4.0 * fl["out"] + terms["out"]
        print(name, "error %.2e bar %.2e" % (err, bar))
        assert err <= bar, (name, err, bar)
    else:
        key = "planes%d" % normalize
        _check_planes(name, got, ref["plane%d" % normalize], fl[key], terms[key])
    one = run_fwd(row, ref["x"][1:2], ref["ws"], normalize)          # frame 1 alone: other lanes and tiles, same bits
    assert _bits_equal(one, got[1:2]), name + ": frame 1 of B = 3 differs from the B = 1 run"


# ------------------------------------------------------------------------------------------ 2. bts_reduc_lpg_fwd_f32 rows
@pytest.mark.parametrize("name", [r.name for r in C.LPG_ROWS])
def test_reduc_lpg_row(name):
    row, ref = C.ROWS[name], C.row_reference(name)
    terms = C.cached(("terms", name), lambda: C.activation_terms(ref, row))
    got = run_lpg(row, ref["x"], ref["ws"])
    _check_lpg_outputs(name, row, got, ref, C.FLOORS[name], terms)
    bare = run_lpg(row, ref["x"], ref["ws"], full=False)
    assert _bits_equal(bare["depth"], got["depth"]), name + ": depth changes with the optional outputs"
    dense = run_lpg(row, ref["x"], ref["ws"], strided=False)
    assert all(_bits_equal(dense[n], got[n]) for n in got), name + ": a strided x changes the result"
    one = run_lpg(row, ref["x"][1:2], ref["ws"])
    for n in ("depth", "plane4") + (("ds",) if row.k > 2 else ()):
        assert _bits_equal(one[n], got[n][1:2]), "%s: %s of frame 1 differs between B = 3 and B = 1" % (name, n)


# ------------------------------------------------------------------------------------------ 3. clamp through the chain
def test_clamp_through_the_chain():
    """reduc_train_ref.CLAMP_CASE forward: the +-1e-3 clamp of lpg_cell_outputs as lpg_emit<8> reaches it, compared on
    every pixel.  Only K = 8 can get there through a chain (reduc_lpg_cases.CLAMP_ROW)."""
    row, ref, r32 = C.CLAMP_ROW, C.clamp_reference(), C.clamp_reference(torch.float32)
    pos, neg, margin, tiny, zeros = C.zone_counts(ref["den"])
    assert pos + neg >= C.CLAMP_MIN_PIXELS and margin == 0 and tiny == 0 and zeros == 0
    assert torch.equal(C.clamp_decisions(ref["den"]), C.clamp_decisions(r32["den"]))
    terms = C.activation_terms(ref, row)
    got = run_lpg(row, ref["x"], ref["ws"])
    _check_lpg_outputs("clamp", row, got, ref, C.FLOORS["clamp"], terms)
    # the clamped pixels on their own: n4 / (+-1e-3 max_depth), a well-conditioned value
    cl = (C.clamp_decisions(ref["den"]) != 0).unsqueeze(1)
    rel = ((got["depth"].double() - ref["depth"]).abs() / ref["depth"].abs())[cl]
    print("clamp: %d clamped pixels, max relative error %.2e" % (int(cl.sum()), float(rel.max())))
    assert float(rel.max()) <= 4.0 * C.FLOORS["clamp"]["depth"] + terms["depth"]


# ------------------------------------------------------------------------------------------ 4. given planes
@pytest.mark.parametrize("name", list(C.GIVEN))
def test_lpg_fused_given_planes(name):
    case, ref = C.GIVEN[name], C.given_reference(C.GIVEN[name])
    k, B, h, w = case.k, case.B, case.h, case.w
    H, W = h * k, w * k
    assert C.lpg_kernel(k, B, h, w, case.normalize, case.ds > 0, case.ds, case.ds_stride) == case.kernel
    plane4 = ref["planes"].permute(0, 2, 3, 1).reshape(-1, 4).cuda().contiguous()
    depth = Slab(B * H * W)
    am = torch.full((), 123.0, device="cuda")
    ds, dsv, slot = None, None, 0
    if case.ds:
        nds = B * (H // case.ds) * (W // case.ds)
        ds = Slab(nds * case.ds_stride, fill=0.0)
        slot = 3 if case.ds_stride > 3 else 0
        dsv = ds.view.view(nds, case.ds_stride)
    ops.lpg_fused_forward(plane4, B, h, w, k, MD, bool(case.normalize), depth.view.view(B, 1, H, W),
                          ds_out=None if ds is None else dsv[:, slot], ds_factor=max(case.ds, 1), ds_pix_stride=case.ds_stride, abs_min=am)
    torch.cuda.synchronize()
    depth.check(name)
    got = depth.view.cpu().view(B, 1, H, W)
    bound, am_bound = C.given_bound(case, ref)
    fin = torch.isfinite(ref["depth"])
    assert _bits_equal(got[~fin], ref["depth"][~fin].float()), name + ": the zero cell is not the oracle's infinity"
    err = (got.double() - ref["depth"]).abs()
    ratio = float((err[fin] / bound[fin]).max())
    cl = (C.clamp_decisions(ref["den"]) != 0).unsqueeze(1)
    print(name, "[%s] max |err| / bound %.3f over %d pixels, %d of them clamped (%.3f there)"
          % (case.kernel, ratio, int(fin.sum()), int(cl.sum()), float((err[cl] / bound[cl]).max())))
    assert bool((err[fin] <= bound[fin]).all()), (name, ratio)
    am_err = abs(float(am) - float(ref["abs_min"]))
    print(name, "abs_min", float(am), "reference", float(ref["abs_min"]), "bound %.2e" % am_bound)
    assert am_err <= am_bound, (name, am_err, am_bound)
    if ds is not None:
        ds.check(name)
        d = dsv.cpu()
        assert _bits_equal(d[:, slot].reshape(B, 1, H // case.ds, W // case.ds), got[:, :, ::case.ds, ::case.ds]), name + ": ds is not depth[::f, ::f]"
        others = [c for c in range(case.ds_stride) if c != slot]
        assert torch.count_nonzero(d[:, others]).item() == 0, name + ": neighbours of the strided slot were written"


# ------------------------------------------------------------------------------------------ 5. NaN
@pytest.mark.parametrize("name", C.NAN_ROWS)
def test_nan_row_reaches_abs_min_and_nothing_else(name):
    """The entry point the model calls (lpg_publish_key): one x row of NaN makes abs_min NaN (bts.py:167) and leaves
    every other cell's bits alone."""
    row, ref = C.ROWS[name], C.row_reference(name)
    k = row.k
    clean = run_lpg(row, ref["x"], ref["ws"])
    assert float(clean["abs_min"]) == float(clean["abs_min"])
    b, y, x0 = C.NAN_CELL
    xn = ref["x"].clone()
    xn[b, :, y, x0] = float("nan")
    got = run_lpg(row, xn, ref["ws"])
    assert bool(torch.isnan(got["abs_min"])), name + ": abs_min does not report the NaN"
    keep = torch.ones_like(clean["depth"], dtype=torch.bool)
    keep[b, :, y * k:(y + 1) * k, x0 * k:(x0 + 1) * k] = False
    assert _bits_equal(got["depth"][keep], clean["depth"][keep])
    assert bool(torch.isnan(got["depth"][~keep]).all())
    keep4 = torch.ones_like(clean["plane4"], dtype=torch.bool)
    keep4[b, :, y, x0] = False
    assert _bits_equal(got["plane4"][keep4], clean["plane4"][keep4])
    if k > 2:
        keepd = torch.ones_like(clean["ds"], dtype=torch.bool)
        keepd[b, :, 2 * y:2 * y + 2, 2 * x0:2 * x0 + 2] = False
        assert _bits_equal(got["ds"][keepd], clean["ds"][keepd])


# ------------------------------------------------------------------------------------------ 6. grid-stride wrap
@pytest.mark.parametrize("case", C.WRAP_CASES, ids=lambda c: c.name)
def test_forward_grid_stride_wraps(case):
    """Just over two passes of the launch's block cap with a ragged last tile, value-checked on every pixel."""
    row, ref = C.ROWS[case.row], C.wrap_reference(case)
    h, w = C.wrap_shape(case)
    assert 0 < h * w - 2 * case.cap_blocks * C.WAVES_PER_BLOCK * case.tile < case.tile
    terms, fl = C.activation_terms(ref, row), C.FLOORS[case.name]
    if row.final:
        got = run_fwd(row, ref["x"], ref["ws"], 0, strided=False)
        err = C.plane_errors(got, ref["out"])[0]
        bar = 4.0 * fl["out"] + terms["out"]
        print(case.name, "error %.2e bar %.2e" % (err, bar))
        assert err <= bar, (case.name, err, bar)
    else:
        assert float(ref["den"].abs().min()) >= C.ORDINARY
        got = run_lpg(row, ref["x"], ref["ws"], strided=False)
        _check_lpg_outputs(case.name, row, got, ref, fl, terms)


# ------------------------------------------------------------------------------------------ 7. LPG backward
@pytest.mark.parametrize("k", C.BWD_KS)
def test_lpg_backward_vs_fp64_autograd(k):
    """bts_lpg_bwd_f32 over three blocks (558 cells) against fp64 autograd through O.lpg_forward.  Bar per plane
    component: 4 x the CPU fp32-autograd floor or the 2e-5 of test_lpg_backward_vs_autograd, whichever is smaller."""
    ref = C.bwd_reference(k)
    B, h, w = C.BWD_SHAPE
    got = ops.lpg_backward(ref["plane"].cuda(), ref["gout"].cuda(), k).cpu()
    errs = C.plane_errors(got, ref["grad"])
    bars = [min(4.0 * f, C.BWD_TODAY) for f in C.FLOORS["bwd_k%d" % k]]
    print("lpg backward k=%d errors" % k, ["%.2e" % e for e in errs], "bars", ["%.2e" % b for b in bars])
    for c, (e, b) in enumerate(zip(errs, bars)):
        assert e <= b, (k, c, e, b)
    for cell, _ in C.BWD_CLAMPED:
        b, r = divmod(cell, h * w)
        assert np.array_equal(got[b, :3, r // w, r % w].numpy(), np.zeros(3, np.float32)), "a clamped cell has a gradient to its normal"
        assert float(got[b, 3, r // w, r % w]) != 0
