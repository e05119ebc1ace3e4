"""CPU: bts_conv_wgrad_plan_f32 (ops.conv_wgrad_plan) -- the tile and pixel split bts_conv_wgrad_f32 will use -- on the
case table of tests/wgrad_cases.py: every plan is well-formed, the table reaches every tile, split regime, ragged edge
and gather mode tests/test_wgrad_gpu.py is meant to check, and the query rejects what the launch rejects."""
import os
import subprocess
import sys

import pytest

import wgrad_cases as wc
from bts_amd import ops
from bts_amd._lib import BtsHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = [(128, 128), (64, 128), (32, 128), (64, 64)]
WBK = 32          # pixels per K-step (csrc/wgrad.hip)


def _facts(c):
    bm, bn, split, pps = wc.plan_of(c)
    H, W = wc.out_hw(c)
    M = c.B * H * W
    N = c.ksize * c.ksize * c.c_in
    return dict(case=c, tile=(bm, bn), bn=bn, split=split, pps=pps, M=M, N=N, H=H, W=W,
                last_steps=(M - (split - 1) * pps + WBK - 1) // WBK)


FACTS = [_facts(c) for c in wc.CASES]


@pytest.mark.parametrize("f", FACTS, ids=lambda f: f["case"].name)
def test_plan_is_well_formed(f):
    c, split, pps, M = f["case"], f["split"], f["pps"], f["M"]
    assert f["tile"] in TILES
    assert pps > 0 and pps % WBK == 0
    assert (split - 1) * pps < M <= split * pps
    if c.ws_floats is None:
        assert split == 1
    if split > 1:
        assert split * c.c_out * f["N"] * max(c.n_bundles, 1) <= c.ws_floats


def test_case_names_are_unique_and_lists_resolve():
    assert len(wc.BY_NAME) == len(wc.CASES)
    for name in wc.FLOAT_CASES:
        assert name in wc.BY_NAME, name
    assert {f["tile"] for f in FACTS if f["case"].name in wc.FLOAT_CASES} == set(TILES)
    assert not any(wc.BY_NAME[n].pre for n in wc.FLOAT_CASES)


def _coverage_items():
    """[(what the table must reach, predicate on one case's facts)]"""
    items = []
    for t in TILES:
        on = lambda f, t=t: f["tile"] == t
        items.append(("%dx%d with split > 1" % t, lambda f, on=on: on(f) and f["split"] > 1))
        items.append(("%dx%d with a pixel count that is no multiple of 32" % t, lambda f, on=on: on(f) and f["M"] % WBK != 0))
        for n in (1, 2, 3):
            items.append(("%dx%d split with a last split of %d K-step(s)" % (t + (n,)),
                          lambda f, on=on, n=n: on(f) and f["split"] > 1 and f["last_steps"] == n))
        # the planner picks every tile with ragged edges on both axes (nothing to except)
        items.append(("%dx%d with N %% bn != 0" % t, lambda f, on=on: on(f) and f["N"] % f["tile"][1] != 0))
        items.append(("%dx%d with c_out %% bm != 0" % t, lambda f, on=on: on(f) and f["case"].c_out % f["tile"][0] != 0))
    for t in ((128, 128), (64, 64)):
        items.append(("%dx%d with split == 1" % t, lambda f, t=t: f["tile"] == t and f["split"] == 1))
        items.append(("%dx%d unsplit with a single K-step" % t, lambda f, t=t: f["tile"] == t and f["split"] == 1 and f["M"] <= WBK))
    items.append(("reduce kernel with split < 16", lambda f: 1 < f["split"] < 16))
    items.append(("reduce kernel with 16 <= split < 64", lambda f: 16 <= f["split"] < 64))
    items.append(("reduce kernel with split >= 64", lambda f: f["split"] >= 64))
    items.append(("the 768-split ceiling of a single-tile output", lambda f: f["split"] == 768))
    modes = [
        ("up = 2", lambda f: f["case"].up == 2),
        ("stride 2", lambda f: f["case"].stride == 2),
        ("dilation larger than the map", lambda f: f["case"].dil > max(f["case"].h, f["case"].w)),
        ("k = 7 with pad 3", lambda f: f["case"].ksize == 7 and f["case"].pad == 3),
        ("W < 32", lambda f: f["W"] < 32),
        ("W = 3", lambda f: f["W"] == 3),
        ("H = 1", lambda f: f["H"] == 1),
        ("B >= 3", lambda f: f["case"].B >= 3),
        ("pre without ReLU", lambda f: f["case"].pre and not f["case"].pre_relu),
        ("pre with ReLU", lambda f: f["case"].pre and f["case"].pre_relu),
        ("n_bundles > 1 without pre", lambda f: f["case"].n_bundles > 1 and not f["case"].pre),
        ("n_bundles > 1 with pre", lambda f: f["case"].n_bundles > 1 and f["case"].pre),
        ("x_extra > 0 and dy_extra > 0", lambda f: f["case"].x_extra > 0 and f["case"].dy_extra > 0),
    ]
    for what, pred in modes:
        items.append((what + " on a tile with bn = 128", lambda f, pred=pred: pred(f) and f["bn"] == 128))
        items.append((what + " on 64x64", lambda f, pred=pred: pred(f) and f["tile"] == (64, 64)))
    return items


def missing_items(facts):
    return [what for what, pred in _coverage_items() if not any(pred(f) for f in facts)]


def test_table_reaches_every_tile_split_and_gather_mode():
    missing = missing_items(FACTS)
    assert not missing, "tests/wgrad_cases.py no longer reaches: " + "; ".join(missing)


def test_coverage_check_names_what_a_removed_case_covered():
    """The check above is not vacuous: without the only 768-split case it names that item."""
    missing = missing_items([f for f in FACTS if f["split"] != 768])
    assert "the 768-split ceiling of a single-tile output" in missing


def test_path_cases_plan_to_their_tiles():
    from bts_amd import train
    assert wc.PATH_WS_FLOATS == train.WGRAD_WS_FLOATS
    assert [t for t, _ in wc.PATH_CASES] == TILES
    for tile, c in wc.PATH_CASES:
        assert wc.plan_of(c)[:2] == tile, c.name
        assert c.c_in % 4 == 0 and c.c_out % 4 == 0 and c.h > 1 and c.w > 1      # train.conv2d hands these over as views


def _good_desc():
    d = ops._wgrad_desc(2, 9, 13, 64, 32, 3, 1, 1, 1, 1, 1, 64, 32)
    d.x = d.dy = d.dw = ops._PLAN_DUMMY_PTR
    return d


def test_query_rejects_what_the_launch_rejects():
    assert ops.conv_wgrad_plan_desc(_good_desc())[:2] == (64, 64)
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan(2, 9, 13, 62, 32, 3)                                  # c_in % 4
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan(2, 9, 13, 64, 30, 3)                                  # c_out % 4
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan(2, 9, 13, 64, 32, 3, up=2, stride=2)
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan(2, 9, 13, 64, 32, 2, pad=1)                           # even ksize
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan(2, 9, 13, 64, 32, 3, n_bundles=2, x_pix_stride=64)    # needs 2 * 64
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan(2, 9, 13, 64, 32, 3, n_bundles=2, dy_pix_stride=32)
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan(2, 9, 13, 64, 32, 3, x_pix_stride=60)
    for field in ("pre_scale", "pre_shift"):
        d = _good_desc()
        d.pre_scale = d.pre_shift = ops._PLAN_DUMMY_PTR
        assert ops.conv_wgrad_plan_desc(d)[:2] == (64, 64)
        setattr(d, field, ops._PLAN_DUMMY_PTR + 4)                                # 4-byte aligned only
        with pytest.raises(BtsHipError):
            ops.conv_wgrad_plan_desc(d)
    d = _good_desc()
    d.pre_scale = ops._PLAN_DUMMY_PTR                                             # scale without shift
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan_desc(d)
    d = _good_desc()
    d.x = 0
    with pytest.raises(BtsHipError):
        ops.conv_wgrad_plan_desc(d)


def test_query_is_host_only():
    """With no visible device the query still answers, and gives the same plan."""
    c = wc.BY_NAME["t128_s16_last11"]
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import wgrad_cases as wc\n"
            "print(*wc.plan_of(wc.BY_NAME[%r]))\n" % (ROOT, os.path.join(ROOT, "tests"), c.name))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.check_output([sys.executable, "-c", code], env=env).decode().split()
    assert tuple(int(v) for v in out) == wc.plan_of(c)


def test_plan_recording_does_not_see_the_query():
    from bts_amd import _lib, plan
    rec = plan._Recorder()
    with _lib.recording(plan._Proxy(_lib.load_real(), rec)):
        assert wc.plan_of(wc.BY_NAME["t64_s7"])[:2] == (64, 64)
    assert rec.calls == [] and rec.foreign == []
