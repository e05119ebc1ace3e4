"""What tests/reduc_lpg_cases.py promises, asserted on the CPU (no GPU): the table covers every dispatch row and every
launch_lpg branch, every reference-side precondition of tests/test_reduc_lpg_fp64_gpu.py holds, the wrap cases are sized
against the caps that csrc/reduc.hip has today, and the committed floors are what the CPU measures."""
import os
import re

import pytest
import torch

import reduc_lpg_cases as C
import reduc_train_ref as R
from bts_amd import ops


def _source(name):
    with open(os.path.join(C.CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ coverage
def test_table_names_all_13_dispatch_rows():
    assert [(r.c_in, r.c_first, r.final) for r in C.FWD_ROWS] == C.DISPATCH_FWD
    assert [(r.c_in, r.c_first, r.k) for r in C.LPG_ROWS] == C.DISPATCH_LPG
    assert len(C.ROWS) == 13
    src = _source("reduc.hip")
    # the ladders in the source, in order: launch_reduc<C0, M0, FINAL[, K]> / launch_reduc16<C0, M0, FINAL, RTn[, K]>
    found = re.findall(r"return (launch_reduc(?:16)?)<(\d+), (\d+), (true|false)(?:, RT[12])?(?:, (\d))?>\(", src)
    fwd = [(int(a), int(b), f == "true") for _, a, b, f, k in found if not k]
    lpg = [(int(a), int(b), int(k)) for _, a, b, f, k in found if k]
    assert fwd == C.DISPATCH_FWD and lpg == C.DISPATCH_LPG, "csrc/reduc.hip dispatches other rows than the table: add them"
    body = {(int(a), int(b), f == "true", int(k or 0)): ("narrow" if fn.endswith("16") else "wide") for fn, a, b, f, k in found}
    for r in C.FWD_ROWS:
        assert body[(r.c_in, r.c_first, r.final, 0)] == r.body, r.name
        assert ops.reduc_uses_mfma16(r.c_in, r.c_first) == (r.body == "narrow"), r.name       # the weight pack agrees
    for r in C.LPG_ROWS:
        assert body[(r.c_in, r.c_first, False, r.k)] == r.body, r.name
    # every LPG K is fed by both kernel bodies, except K = 4 / 2 on the bodies the source does not build
    served = {(r.k, r.body) for r in C.LPG_ROWS}
    assert served == {(8, "wide"), (4, "wide"), (2, "narrow"), (8, "narrow"), (4, "narrow")}
    for r in C.ROWS.values():
        assert R.CHAINS[r.chain][:2] == (r.c_in, r.c_first) and (R.CHAINS[r.chain][2] == 0) == r.final
        if not r.final and r.entry == "bts_reduc_lpg_fwd_f32":
            assert R.CHAINS[r.chain][2] == r.k
    assert {C.ROWS[n].body for n in C.NAN_ROWS} == {"wide", "narrow"}
    assert {(C.ROWS[c.row].body, C.ROWS[c.row].final) for c in C.WRAP_CASES} == {("wide", False), ("narrow", False), ("narrow", True)}


def test_chain_shape_is_ragged_and_straddles():
    B, h, w = C.SHAPE
    n = B * h * w
    assert n == 105 and n // 32 == 3 and n % 32 and n % 16                    # three full wave tiles and a partial one
    assert all((b * h * w) % 32 and (b * h * w) % 16 for b in range(1, B))    # frame boundaries inside tiles
    assert w % 16 and C.X_OFF % 4 == 0 and C.X_PAD % 4 == 0 and C.X_OFF < C.X_PAD
    b, y, x = C.NAN_CELL
    assert b == 1 and y < h and x < w


def test_given_cases_name_every_launch_lpg_branch():
    got = set()
    for c in C.GIVEN_CASES:
        kern = C.lpg_kernel(c.k, c.B, c.h, c.w, c.normalize, c.ds > 0, c.ds, c.ds_stride)
        assert kern == c.kernel, c.name
        if c.ds:
            assert (c.h * c.k) % c.ds == 0 and (c.w * c.k) % c.ds == 0, c.name
        got.add((kern, c.k, bool(c.normalize), c.ds, c.ds_stride > 1))
    lean = {g for g in got if g[0] == "lean"}
    assert {g[1] for g in lean} == {2, 4, 8}
    assert {g[3] for g in lean} == {0, 1, 2, 4}                               # no ds_out, and each factor the lean kernel takes
    assert any(g[4] for g in lean if g[3] == 1) and any(g[4] for g in lean if g[3] == 2) and any(g[4] for g in lean if g[3] == 4)
    assert any(not g[4] for g in lean if g[3])
    assert ("general_v4", 8, False, 8, False) in got                          # a factor outside {1, 2, 4}
    assert any(g[0] == "general_v4" and g[2] for g in got)                    # normalize
    assert any(g[0] == "general_v1" and g[3] for g in got)                    # width not a multiple of 4, with a ds_out
    # the predicate's text in the source (a change there means lpg_kernel must be restated)
    src = _source("lpg.hip")
    assert "if (FUSED && !PLANAR && !normalize && vec4 && k >= 2 && (ds_out == nullptr || ds_factor == 1 || ds_factor == 2 || ds_factor == 4) &&" in src
    assert "const bool vec4 = (((long)w * k) % 4) == 0;" in src


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("name", [r.name for r in C.FWD_ROWS + C.LPG_ROWS if not r.final])
def test_chain_cases_are_ordinary(name):
    r64, r32 = C.row_reference(name), C.row_reference(name, torch.float32)
    assert float(r64["den"].abs().min()) >= 1e-2
    assert torch.equal(C.clamp_decisions(r64["den"]), C.clamp_decisions(r32["den"]))
    assert bool(torch.isfinite(r64["depth"]).all()) and float(r64["plane1"][:, 3].min()) > 0


def test_clamp_case_reaches_the_clamp():
    r64, r32 = C.clamp_reference(), C.clamp_reference(torch.float32)
    pos, neg, margin, tiny, zeros = C.zone_counts(r64["den"])
    assert pos + neg >= C.CLAMP_MIN_PIXELS, (pos, neg)
    assert margin == 0 and tiny == 0 and zeros == 0
    assert torch.equal(C.clamp_decisions(r64["den"]), C.clamp_decisions(r32["den"]))


@pytest.mark.parametrize("name", list(C.GIVEN))
def test_given_case_zones(name):
    case = C.GIVEN[name]
    r64, r32 = C.given_reference(case), C.given_reference(case, torch.float32)
    den = r64["den"]
    pos, neg, margin, tiny, zeros = C.zone_counts(den)
    assert pos >= 16 and neg >= 16 and pos + neg >= 32
    assert margin == 0 and tiny == 0
    assert zeros == case.k * case.k and bool((den[0, :case.k, :case.k] == 0).all())          # the constructed cell alone
    ordinary = den.abs() >= C.ZONE_HI
    assert float(den.abs()[ordinary].min()) >= 1e-2
    assert torch.equal(C.clamp_decisions(den), C.clamp_decisions(r32["den"]))
    # the zero cell: a signed infinity from the oracle, and abs_min == 0
    blk = r64["depth"][0, 0, :case.k, :case.k]
    assert bool((blk == float("-inf")).all()) and float(r64["abs_min"]) == 0.0
    fin = torch.isfinite(r64["depth"])
    assert int((~fin).sum()) == case.k * case.k
    bound, am_bound = C.given_bound(case, r64)
    assert bool(torch.isfinite(bound[fin]).all()) and am_bound < 1e-6
    # the bound is a rounding bound: nowhere looser than 1e-4 relative, and 5 U on the clamped pixels
    rel = (bound / r64["depth"].abs())[fin]
    assert float(rel.max()) < 1e-4
    clamped = (C.clamp_decisions(den) != 0).unsqueeze(1)
    assert float((bound / r64["depth"].abs())[clamped].max()) <= 1.02 * 5 * C.U


@pytest.mark.parametrize("k", C.BWD_KS)
def test_backward_cases(k):
    B, h, w = C.BWD_SHAPE
    assert B * h * w == 558 == 2 * 256 + 46
    ref = C.bwd_reference(k)
    den = ref["den"]
    assert float(den.abs().min()) > C.DEN_MIN
    dec = C.clamp_decisions(den)
    for (cell, n3), want in zip(C.BWD_CLAMPED, (1, -1)):
        b, r = divmod(cell, h * w)
        blk = dec[b, (r // w) * k:(r // w + 1) * k, (r % w) * k:(r % w + 1) * k]
        assert bool((blk == want).all())
        assert bool((ref["grad"][b, :3, r // w, r % w] == 0).all()) and float(ref["grad"][b, 3, r // w, r % w]) != 0
    assert int((dec != 0).sum()) == 2 * k * k
    assert float(den.abs()[dec == 0].min()) >= 0.1
    assert torch.equal(dec, C.clamp_decisions(C.bwd_reference(k, torch.float32)["den"]))


# ------------------------------------------------------------------------------------------------ wrap sizes and caps
@pytest.mark.parametrize("case", C.WRAP_CASES, ids=lambda c: c.name)
def test_wrap_case_exceeds_twice_the_cap_by_less_than_a_tile(case):
    src = _source("reduc.hip")
    resize = "csrc/reduc.hip no longer holds %%r: resize %s (tests/reduc_lpg_cases.py WRAP_CASES)" % ", ".join(c.name for c in C.WRAP_CASES)
    for expr in (case.cap_expr, case.tile_expr) + C.WRAP_SOURCE_EXPRS:
        assert expr in src, resize % expr
    row = C.ROWS[case.row]
    if row.body == "wide":
        assert C.chain_lds_bytes(row.c_in, row.c_first) > 80 * 1024               # per_cu = 1: the cap is 256 blocks
        assert C.chain_lds_bytes(128, 64) <= 80 * 1024
    h, w = C.wrap_shape(case)
    per_pass = case.cap_blocks * C.WAVES_PER_BLOCK * case.tile
    assert 0 < h * w - 2 * per_pass < case.tile
    assert (h * w + case.tile - 1) // case.tile > 2 * case.cap_blocks * C.WAVES_PER_BLOCK      # the launch is capped
    if not row.final:
        ref = C.wrap_reference(case)
        assert float(ref["den"].abs().min()) >= 1e-2
        assert torch.equal(C.clamp_decisions(ref["den"]), C.clamp_decisions(C.wrap_reference(case, torch.float32)["den"]))


# ------------------------------------------------------------------------------------------------ floors
def _flat(v):
    if isinstance(v, dict):
        return [x for k in sorted(v) for x in _flat(v[k])]
    return list(v) if isinstance(v, (list, tuple)) else [v]


def test_committed_floors_are_what_the_cpu_measures():
    """fp32 sums depend on the host's BLAS blocking and thread count, so a re-measurement may differ from the committed
    figure in its leading digit; more than a factor of two means the cases or the oracle changed: re-run
    `python tests/reduc_lpg_cases.py` and commit what it prints."""
    now = C.measure_floors()
    assert sorted(now) == sorted(C.FLOORS)
    for name in now:
        a, b = _flat(now[name]), _flat(C.FLOORS[name])
        assert len(a) == len(b), name
        for x, y in zip(a, b):
            assert (x == y == 0.0) or 0.5 * y <= x <= 2.0 * y, (name, now[name], C.FLOORS[name])
    # for orientation: the floors sit at the arithmetic's own noise, far below the 1e-4 / 3e-4 of the early tests
    assert max(_flat({n: v for n, v in C.FLOORS.items() if n != "clamp"})) < 3e-6
