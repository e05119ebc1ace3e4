"""CPU: the case table of tests/conv_cases.py against the library's own dispatch (conv_plan.query, bts_conv_plan_f32): the
table reaches every kernel family and tile, every flag and layout, ragged edges, both epilogues and every gather mode
tests/test_conv_exact_gpu.py is meant to check -- item by item, so a dispatch change that moves cases off a kernel
fails by name -- and every case keeps fp32 arithmetic exact on its integer operands (the reference alone shows that)."""
import json
import os
import subprocess
import sys
from functools import lru_cache

import pytest

import conv_cases as cc
from bts_amd import conv_plan
from bts_amd.conv_plan import Family as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorded_families():
    """FAMILIES of tests/golden/gen_conv_plan_table.py, read without leaving a bytecode cache next to the fixtures."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_conv_plan_table", os.path.join(ROOT, "tests", "golden", "gen_conv_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    keep, sys.dont_write_bytecode = sys.dont_write_bytecode, True
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.dont_write_bytecode = keep
    return mod.FAMILIES


FAMILIES = _recorded_families()

ROW_BF16_TILES = [(128, 128), (64, 128), (128, 64), (64, 64), (128, 32)]
ALL_CASES = cc.CASES + cc.DIL2_CASES


@lru_cache(maxsize=None)
def plans():
    """{name: Plan}, asked in fresh processes without any BTS_* variable (the library reads its knobs once per process);
    the dilation-6 / 12 halo cases in one that sets BTS_CONV_HALO_DIL=2."""
    base = {k: v for k, v in os.environ.items() if not k.startswith("BTS_")}
    out = {}
    for cases, extra in ((cc.CASES, {}), (cc.DIL2_CASES, cc.DIL2_ENV)):
        txt = subprocess.check_output([sys.executable, os.path.join(ROOT, "tests", "conv_cases.py")] + [c.name for c in cases],
                                      env=dict(base, **extra), cwd=ROOT, timeout=300)
        out.update({n: conv_plan.Plan(*(v[:1] + [F(v[1])] + v[2:])) for n, v in json.loads(txt).items()})
    return out


def spatial_tile(p):
    """(rows, pixels) of the family's spatial tile, None for the kernels that tile the flat pixel axis."""
    if p.family in (F.HALO, F.HALO_TAIL):
        return (8, 16) if p.bn == 48 else (4, 32)
    if p.family in (F.HALO_EMU, F.HALO_BF16):
        return (4, 32)
    return {F.WINO: (8, 16), F.STEM: (8, 32)}.get(p.family)


def facts(c, p):
    H, W = (c.h, c.w) if c.subpixel else cc.out_hw(c)          # sub-pixel kernels walk source pixels, per parity class
    f = dict(case=c, plan=p, key=(p.family, p.bm, p.bn), H=H, W=W, M=c.B * H * W, tile=spatial_tile(p),
             name=conv_plan.kernel_name(p, c.nchw, c.subpixel))
    nhwc_fused = not c.nchw and not p.splitk
    f["fast"] = nhwc_fused and not c.res and c.act != "sigmoid"
    f["general"] = nhwc_fused and c.res
    return f


@lru_cache(maxsize=None)
def all_facts():
    return tuple(facts(c, plans()[c.name]) for c in ALL_CASES)


def test_table_is_well_formed():
    assert len(cc.BY_NAME) == len(ALL_CASES)
    assert 80 <= len(ALL_CASES) <= 130
    for c in ALL_CASES:
        assert c.c_in % 4 == 0 and c.x_extra % 8 == 0 and c.y_extra % 8 == 0, c.name
        assert c.precision in cc.PRECISIONS and c.act in ("none", "relu"), c.name
    for n in cc.FLOAT_CASES:
        assert n in cc.BY_NAME and not cc.BY_NAME[n].res, n


def test_library_accepts_every_case():
    bad = [f["case"].name for f in all_facts() if f["plan"].rc != 0]
    assert not bad, bad


def test_what_the_library_rejects_stays_out_of_the_gpu_table():
    """Rejections (rc != 0) are pinned here; none of these combinations may sit in CASES."""
    for c in (cc._c("res_into_nchw", 1, 5, 7, 32, 64, 1, nchw=True, res=True),
              cc._c("y2_into_nchw", 1, 5, 7, 32, 64, 1, nchw=True, y2=True),
              cc._c("tail_on_dilated", 1, 8, 32, 40, 64, 3, dil=2, n_tail=1),
              cc._c("tail_on_1x1", 1, 8, 32, 40, 64, 1, n_tail=1),
              cc._c("bundles_into_nchw", 1, 6, 8, 32, 32, 3, n_bundles=4, nchw=True),
              cc._c("up2_with_stride2", 1, 6, 8, 32, 32, 3, up=2, stride=2),
              cc._c("even_ksize", 1, 6, 8, 32, 32, 4, pad=2)):
        assert cc.plan_of(c).rc != 0, c.name


def _coverage_items():
    """[(what the table must reach, predicate on one case's facts)]"""
    items = []
    on = lambda key: (lambda f: f["key"] == key)
    fam = lambda *fs: (lambda f: f["plan"].family in fs)
    both = lambda a, b: (lambda f: a(f) and b(f))
    nhwc, nchw = (lambda f: not f["case"].nchw), (lambda f: f["case"].nchw)
    sub = lambda f: f["case"].subpixel
    k3 = lambda f: not f["case"].subpixel
    keys = sorted(FAMILIES) + [(F.ROW_BF16,) + t for t in ROW_BF16_TILES] + [(F.HALO_BF16, 128, 128), (F.HALO_BF16, 128, 64)]
    for key in keys:
        what = "%s %dx%d" % (key[0].name, key[1], key[2])
        items.append((what, on(key)))
        if key[0] in (F.HALO_EMU, F.HALO_BF16):
            items.append((what + " k3", both(on(key), k3)))
            items.append((what + " k2 (sub-pixel)", both(on(key), sub)))
        if key[0] in (F.ROW, F.HALO, F.HALO_TAIL):               # the families that take both layouts
            items.append((what + " NHWC", both(on(key), nhwc)))
            items.append((what + " NCHW", both(on(key), nchw)))
        if key[0] == F.HALO and key[2] != 48:                   # (the 48-wide halo tile has no sub-pixel form)
            items.append((what + " k2 (sub-pixel)", both(on(key), sub)))
        # ragged edges.  Exceptions: a 48-wide tile, the stem and the wide 1x1 only ever see c_out % bn == 0 (choose_tile,
        # stem_eligible, conv1x1_eligible).
        if key[2] != 48 and key[0] not in (F.STEM, F.WIDE_1X1):
            items.append((what + " with c_out % bn != 0", both(on(key), lambda f: f["case"].c_out % f["plan"].bn != 0)))
        if key[0] in (F.ROW, F.ROW_BF16, F.WIDE_1X1):
            items.append((what + " with M % bm != 0", both(on(key), lambda f: f["M"] % f["plan"].bm != 0)))
        else:
            items.append((what + " on a map ragged in height and in width",
                          both(on(key), lambda f: f["H"] % f["tile"][0] != 0 and f["W"] % f["tile"][1] != 0)))
        if key[0] != F.ROW_BF16:                                 # NHWC epilogues (STEM: dispatch guarantees the fast one)
            items.append((what + " through fast_epilogue_nhwc", both(on(key), lambda f: f["fast"])))
            if key[0] != F.STEM:
                items.append((what + " through the general epilogue (res)", both(on(key), lambda f: f["general"])))
    # a map smaller than one spatial tile (in at least one direction: the fill gates of the halo and Winograd kernels
    # keep out maps smaller in both -- except under a planar tail, which takes the halo tile whatever the map)
    for fm in (F.HALO, F.HALO_TAIL, F.HALO_EMU, F.HALO_BF16, F.WINO, F.STEM):
        items.append(("%s on a map smaller than one tile" % fm.name,
                      both(fam(fm), lambda f: f["H"] < f["tile"][0] or f["W"] < f["tile"][1])))
    items.append(("HALO_TAIL on a map smaller than one tile in both directions",
                  both(fam(F.HALO_TAIL), lambda f: f["H"] < f["tile"][0] and f["W"] < f["tile"][1])))
    # fewer pixels than one row tile (choose_tile takes 128 rows only where 64-row tiles would overfill the chip, so
    # among the 128-row tiles only 128x32 can see it)
    for key in ((F.ROW, 64, 128), (F.ROW, 64, 64), (F.ROW, 64, 48), (F.ROW, 128, 32), (F.WIDE_1X1, 64, 192), (F.WIDE_1X1, 128, 192)):
        items.append(("%s %dx%d with M < bm" % (key[0].name, key[1], key[2]), both(on(key), lambda f: f["M"] < f["plan"].bm)))
    for fm in (F.ROW_BF16,):
        items.append(("ROW_BF16 through fast_epilogue_nhwc", both(fam(fm), lambda f: f["fast"])))
        items.append(("ROW_BF16 through the general epilogue (res)", both(fam(fm), lambda f: f["general"])))
        items.append(("ROW_BF16 NCHW", both(fam(fm), nchw)))
    for fm in F:
        items.append(("%s with B >= 3" % fm.name, both(fam(fm), lambda f: f["case"].B >= 3)))
    # flags
    items.append(("SPLITK", lambda f: f["plan"].splitk))
    items.append(("W8", lambda f: f["plan"].w8))
    items.append(("DIL at dilation 3", lambda f: f["plan"].dil and f["case"].dil == 3))
    items.append(("DIL at dilation 6", lambda f: f["plan"].dil and f["case"].dil == 6))
    items.append(("DIL at dilation 12", lambda f: f["plan"].dil and f["case"].dil == 12))
    items.append(("SPLITK into NCHW on bf16", both(fam(F.ROW_BF16), lambda f: f["plan"].splitk)))
    for bn in (128, 64):
        items.append(("Winograd tail variant at %d" % bn, both(on((F.WINO, 128, bn)), lambda f: f["case"].n_tail > 0)))
        items.append(("Winograd tail variant at %d on a ragged map" % bn,
                      both(on((F.WINO, 128, bn)), lambda f: f["case"].n_tail > 0 and f["H"] % 8 != 0 and f["W"] % 16 != 0)))
    for n in (1, 2, 3, 4):
        items.append(("%d tail plane(s)" % n, lambda f, n=n: f["case"].n_tail == n))
    # the row family's gather modes
    row = fam(F.ROW)
    for k in (1, 3, 5, 7):
        items.append(("row tiles with ksize %d" % k, both(row, lambda f, k=k: f["case"].ksize == k and not f["case"].subpixel)))
    items += [
        ("row tiles with stride 2", both(row, lambda f: f["case"].stride == 2)),
        ("row tiles with a dilation larger than the map", both(row, lambda f: f["case"].dil > max(f["case"].h, f["case"].w))),
        ("row tiles with up = 2", both(row, lambda f: f["case"].up == 2 and not f["case"].subpixel)),
        ("row tiles sub-pixel", both(row, sub)),
        ("row tiles with bundles on a 64-wide tile", both(row, lambda f: f["case"].n_bundles > 1 and f["plan"].bn == 64)),
        ("row tiles with bundles on 128x32", both(on((F.ROW, 128, 32)), lambda f: f["case"].n_bundles > 1)),
        ("row tiles skipping taps (issued < dense)", both(row, lambda f: 0 < f["plan"].issued < f["plan"].dense)),
        ("row tiles with c_in_ld % 32 != 0 (the non-lean gather)", both(row, lambda f: f["case"].c_in % 32 != 0)),
        ("row tiles with c_in_ld % 32 == 0 (the lean gather)", both(row, lambda f: f["case"].c_in % 32 == 0)),
    ]
    # split-K on four row tiles (the issue asks for three), into both layouts
    for key in ((F.ROW, 64, 128), (F.ROW, 64, 64), (F.ROW, 64, 48), (F.ROW, 128, 32)):
        what = "split-K on ROW %dx%d" % key[1:]
        items.append((what + " NHWC", both(on(key), lambda f: f["plan"].splitk and not f["case"].nchw)))
        items.append((what + " NCHW", both(on(key), lambda f: f["plan"].splitk and f["case"].nchw)))
    # the workspace alone does not decide: the same map splits K by default and returns to the halo tile at fill_frames 4096
    same_map = lambda f: (f["case"].h, f["case"].w, f["case"].c_in, f["case"].c_out) == (8, 32, 36, 128) and f["case"].ws_floats
    items.append(("a halo map that splits K once a workspace is lent", both(same_map, lambda f: f["plan"].splitk)))
    items.append(("the same map back on the halo tile at fill_frames 4096", both(same_map, fam(F.HALO))))
    # what is fused
    items += [
        ("y2 with split-K", lambda f: f["case"].y2 and f["plan"].splitk),
        ("y2 without split-K", lambda f: f["case"].y2 and not f["plan"].splitk),
        ("res with split-K", lambda f: f["case"].res and f["plan"].splitk),
        ("e1, act and e2 together", lambda f: f["case"].e1 and f["case"].act == "relu" and f["case"].e2),
        ("no epilogue at all", lambda f: not (f["case"].e1 or f["case"].e2 or f["case"].res) and f["case"].act == "none"),
        ("pre with pre_relu on a padded convolution", lambda f: f["case"].pre and f["case"].pre_relu and f["case"].pad > 0),
        ("pre without ReLU on a padded convolution", lambda f: f["case"].pre and not f["case"].pre_relu and f["case"].pad > 0),
        ("x and y as slices of wider buffers", lambda f: f["case"].x_extra > 0 and f["case"].y_extra > 0),
    ]
    for fm in (F.ROW, F.HALO, F.WINO, F.WIDE_1X1, F.HALO_EMU, F.HALO_BF16):
        items.append(("%s with pre" % fm.name, both(fam(fm), lambda f: f["case"].pre)))
    for fm in (F.ROW, F.HALO, F.HALO_TAIL, F.WINO, F.WIDE_1X1, F.STEM, F.HALO_EMU):
        items.append(("%s with y2" % fm.name, both(fam(fm), lambda f: f["case"].y2)))
        items.append(("%s into a slice of a wider buffer" % fm.name, both(fam(fm), lambda f: f["case"].y_extra > 0)))
    # halo-emu / halo-bf16 with at least three chunks, for each of KS 3 and KS 2: only from the third chunk on does the
    # patch trickle into a buffer that an earlier chunk has already used
    for fm in (F.HALO_EMU, F.HALO_BF16):
        for what, ks in (("k3", k3), ("k2 (sub-pixel)", sub)):
            items.append(("%s %s with at least three 32-channel chunks" % (fm.name, what),
                          both(fam(fm), lambda f, ks=ks: ks(f) and f["case"].c_in >= 96)))
    # precision 1 and 2 off their own kernels
    items.append(("the stem under bf16x3 on the row tiles", lambda f: f["case"].precision == "bf16x3" and f["case"].ksize == 7 and f["plan"].family == F.ROW))
    items.append(("the stem under bf16 still on the stem kernel", lambda f: f["case"].precision == "bf16" and f["plan"].family == F.STEM))
    items.append(("c_out 48 under bf16x3 padded to the 64-wide tile", lambda f: f["case"].precision == "bf16x3" and f["case"].c_out == 48 and f["plan"].bn == 64))
    return items


def missing_items(fs):
    return [what for what, pred in _coverage_items() if not any(pred(f) for f in fs)]


def test_table_reaches_every_family_tile_edge_and_epilogue():
    missing = missing_items(all_facts())
    assert not missing, "tests/conv_cases.py no longer reaches: " + "; ".join(missing)


def test_coverage_check_names_what_a_removed_case_covered():
    """The check above is not vacuous: without the only 48-wide Winograd cases, or the one W8 family, it names them."""
    missing = missing_items([f for f in all_facts() if f["key"] != (F.WINO, 128, 48)])
    assert "WINO 128x48" in missing and "WINO 128x48 through the general epilogue (res)" in missing
    missing = missing_items([f for f in all_facts() if not f["plan"].w8])
    assert "W8" in missing


def test_kernel_names_the_table_reaches():
    """At least thirty distinct instantiations, as the profiler names them."""
    names = {f["name"] for f in all_facts()}
    assert len(names) >= 30, sorted(names)


@pytest.mark.parametrize("c", ALL_CASES, ids=lambda c: c.name)
def test_case_keeps_fp32_exact(c):
    """The reference's own magnitude sum -- sum |w| * |x_tap| carried through e1, res and e2, in units of the smallest
    dyadic step; for a Winograd plan also the transform-domain bound -- stays below 2^24: every intermediate of every
    summation order is an exactly representable fp32 number."""
    p = plans()[c.name]
    o, worst = cc.operands(c, plan=p)
    assert worst < 1.0, "case breaks the exactness precondition even at |x| <= %d" % o.xmax
    assert o.xmax in cc.XMAX_LADDER and o.x.abs().max().item() > 0.9 * o.xmax
    if c.precision != "fp32":
        assert o.xmax > 256                                    # operands that bf16 cannot hold
    if p.family == F.WINO:
        assert bool((o.w % 4 == 0).all())                      # G g G^T is integral
    if c.pre:
        assert bool((o.pre[1] < 0).any()) and bool((o.pre[1] > 0).any())
    # the rounded (bf16) statement of the same case is bounded by the same sums: rounding to nearest moves |x| by at
    # most 2^-9 relative, and 512 * 3 * K stays far inside the margin asserted here
    if c.precision == "bf16":
        assert worst < 0.99
