"""The batch planner of the multi-problem weight-gradient launch (bts_conv_wgrad_batch_plan_f32 through
ops.conv_wgrad_batch_plan): host arithmetic only, no GPU.  The batches are tests/wgrad_batch_cases.py's, the ones
tests/test_wgrad_batch_gpu.py runs."""
import ctypes as C
import random

import pytest

import wgrad_batch_cases as bc
import wgrad_cases as wc
from bts_amd import _lib, ops

MI = 1 << 20
PLANS = {name: bc.plan_of(name) for name in bc.BATCHES}


def _last_ksteps(c, p):
    return -(-(bc.pixels(c) - (p[2] - 1) * p[3]) // 32)


def test_the_table_reaches_every_item():
    reached = set()
    for name, (ws_floats, cases) in bc.BATCHES.items():
        plan = PLANS[name]
        splits = [p[2] for p in plan]
        for c, p in zip(cases, plan):
            reached.add("tile %dx%d" % p[:2])
            if p[2] > 1 and 1 <= _last_ksteps(c, p) <= 3:
                reached.add("a short last split")
            if c.n_bundles > 1:
                reached.add("a bundled problem")
            if c.pre and c.pre_relu:
                reached.add("pre + relu")
            if c.pre and not c.pre_relu:
                reached.add("pre without relu")
            if c.x_extra and c.dy_extra:
                reached.add("column slices of wider buffers")
        if min(splits) == 1 and max(splits) > 1:
            reached.add("split 1 and split > 1 in one batch")
        if len({bc.pixels(c) for c in cases}) > 1:
            reached.add("different pixel counts in one batch")
        if len(cases) == 1:
            reached.add("n = 1")
        if len(cases) >= 65:
            reached.add("n >= 65")
    wanted = {"tile 128x128", "tile 64x128", "tile 32x128", "tile 64x64", "a short last split", "a bundled problem", "pre + relu",
              "pre without relu", "column slices of wider buffers", "split 1 and split > 1 in one batch",
              "different pixel counts in one batch", "n = 1", "n >= 65"}
    assert not wanted - reached, "the batch table no longer reaches: %s" % sorted(wanted - reached)


@pytest.mark.parametrize("name", list(bc.BATCHES))
def test_split_invariants_and_workspace_accounting(name):
    ws_floats, cases = bc.BATCHES[name]
    spans = []
    for c, (bm, bn, split, pps, off) in zip(cases, PLANS[name]):
        M = bc.pixels(c)
        assert (bm, bn) in ((128, 128), (64, 128), (32, 128), (64, 64))
        assert pps % 32 == 0 and 1 <= split <= 1024
        assert (split - 1) * pps < M <= split * pps, "an empty split"
        assert split == 1 or pps >= 128, "fewer than 4 K-steps per split"
        if split > 1:
            assert off >= 0 and off % 4 == 0
            spans.append((off, off + split * bc.dw_floats(c)))
        else:
            assert off == -1
    spans.sort()
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, "workspace regions overlap"
    assert sum(b - a for a, b in spans) <= ws_floats
    assert not spans or spans[-1][1] <= ws_floats


def test_a_small_workspace_lowers_the_splits_and_none_means_no_split():
    ws_floats, cases = bc.BATCHES["mixed_small_ws"]
    roomy = ops.conv_wgrad_batch_plan([bc.problem_of(c) for c in cases], 4 * MI)
    tight = PLANS["mixed_small_ws"]
    assert all(t[2] <= r[2] for t, r in zip(tight, roomy)) and any(t[2] < r[2] for t, r in zip(tight, roomy))
    assert any(t[2] > 1 for t in tight)                       # lowered, not given up
    for name, (_, cs) in bc.BATCHES.items():
        assert all(p[2] == 1 and p[4] == -1 for p in ops.conv_wgrad_batch_plan([bc.problem_of(c) for c in cs], 0)), name


def _descs(cases, base, stride=1 << 24):
    """Filled descriptors whose pointers sit at distinct offsets of one range starting at `base`."""
    out = []
    for i, c in enumerate(cases):
        p = bc.problem_of(c)
        d = ops._wgrad_desc(p["B"], p["h_in"], p["w_in"], p["c_in"], p["c_out"], p["ksize"], p["dil"], p["stride"], p["pad"], p["up"],
                            p["n_bundles"], p["x_pix_stride"], p["dy_pix_stride"])
        at = base + 4 * i * stride
        d.x, d.dy, d.dw = at, at + stride, at + 2 * stride
        if c.pre:
            d.pre_scale, d.pre_shift, d.pre_relu = at + 3 * stride, at + 3 * stride + 65536, int(c.pre_relu)
        out.append(d)
    return out


@pytest.mark.parametrize("name", ["mixed", "t64_geometries", "tiny70"])
def test_plan_depends_on_shapes_only(name):
    ws_floats, cases = bc.BATCHES[name]
    want = PLANS[name]
    span = 4 * len(cases) * (1 << 24) + (1 << 30)
    for base in (1 << 20, (1 << 40) + 4096):
        assert ops.conv_wgrad_batch_plan_descs(_descs(cases, base), [(base, span)], ws_floats) == want
    # two bases instead of one: same plan
    assert ops.conv_wgrad_batch_plan_descs(_descs(cases, 1 << 20), [(1 << 20, 1 << 24), (1 << 20, span)], ws_floats) == want
    order = list(range(len(cases)))
    random.Random(7).shuffle(order)
    shuffled = ops.conv_wgrad_batch_plan([bc.problem_of(cases[i]) for i in order], ws_floats)
    # tile, split and pixels per split follow the problem; the workspace offsets are the same set of regions (two
    # problems of one shape may swap theirs)
    assert [p[:4] for p in shuffled] == [want[i][:4] for i in order]
    key = lambda c, p: (bc.problem_of(c)["c_out"], bc.dw_floats(c), bc.pixels(c), p)
    assert sorted(key(cases[i], p) for i, p in zip(order, shuffled)) == sorted(key(c, p) for c, p in zip(cases, want))


def _rc(descs, bases, ws_floats=MI):
    lib = _lib.load()
    n = len(descs)
    arr = (_lib.ConvWgradDesc * n)(*descs)
    bp = (C.c_void_p * len(bases))(*[a for a, _ in bases])
    bb = (C.c_long * len(bases))(*[b for _, b in bases])
    table = C.create_string_buffer(int(lib.bts_conv_wgrad_batch_table_bytes(n)))
    return lib.bts_conv_wgrad_batch_plan_f32(arr, n, bp, bb, len(bases), ws_floats, table, None)


def test_one_bad_item_fails_the_plan_with_its_own_error():
    _, cases = bc.BATCHES["mixed"]
    base, span = 1 << 20, 1 << 40
    single = lambda d: _lib.load().bts_conv_wgrad_plan_f32(C.byref(d), None, None, None, None)
    assert _rc(_descs(cases, base), [(base, span)]) == 0
    INVALID = -1

    def broken(change):
        ds = _descs(cases, base)
        change(ds[2])
        return ds

    def misaligned_x(d): d.x += 4
    def cin_not_4(d): d.c_in, d.x_pix_stride = 62, 64
    def outside(d): d.dy = base + span + 4096
    def own_ws(d): d.ws, d.ws_floats = base, 1024

    for change in (misaligned_x, cin_not_4):
        ds = broken(change)
        assert single(ds[2]) == INVALID                       # what the single launch says of this descriptor
        assert _rc(ds, [(base, span)]) == INVALID, change.__name__
    ds = broken(outside)
    assert single(ds[2]) == 0 and _rc(ds, [(base, span)]) == INVALID
    ds = broken(lambda d: setattr(d, "dw", base + span - 64))     # starts inside, its extent ends outside
    assert _rc(ds, [(base, span)]) == INVALID
    ds = broken(own_ws)
    assert single(ds[2]) == 0 and _rc(ds, [(base, span)]) == INVALID
    ds = broken(lambda d: setattr(d, "up", 3))                    # the single launch's UNSUPPORTED stays UNSUPPORTED
    assert single(ds[2]) == -2 and _rc(ds, [(base, span)]) == -2
    assert _rc(_descs(cases, base), [(base + 8, span)]) == INVALID    # a misaligned base
    assert _rc(_descs(cases, base), [(base, span)] * 9) == INVALID    # more than 8 bases
    assert _rc([], [], 0) == 0                                        # an empty batch is valid


def test_densenet161_block3_moves_less_partial_traffic_than_its_single_launches():
    """The 72 problems of DenseNet161's third block at 4x22x44 (3 872 pixels) under the training path's workspace."""
    ws_floats = wc.PATH_WS_FLOATS
    cases = bc.dense_block_cases(4, 22, 44, 384, 48, 192, 36, prefix="b3")
    assert len(cases) == 72
    batch = ops.conv_wgrad_batch_plan([bc.problem_of(c) for c in cases], ws_floats)
    traffic = lambda c, split: 8 * split * bc.dw_floats(c) if split > 1 else 0          # written once, read once
    batched = sum(traffic(c, p[2]) for c, p in zip(cases, batch))
    singles = 0
    for c in cases:
        one = c._replace(ws_floats=ws_floats)
        singles += traffic(c, wc.plan_of(one)[2])
    print("block 3 partial-tile bytes: batch %d, single launches %d" % (batched, singles))
    assert singles > 0 and batched < singles
