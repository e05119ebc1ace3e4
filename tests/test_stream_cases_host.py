"""CPU: the preconditions that tests/test_stream_kernels_gpu.py relies on, for the case table of tests/stream_cases.py --
which chunk count and finalize walk each BN shape takes (asked of the library's own plan_chunks), that the integer designs
keep every fp32 partial result exact (so torch.equal is the right comparison), that the depth-tail cases recover their
integer pre-activation on enough pixels and on every border, and that the grid-stride cases are larger than one launch's
threads, with the block caps read out of the kernel sources."""
import pytest
import torch

import stream_cases as sc
from bts_amd import _lib

ALL_BN = [s for s, _ in sc.BN_SHAPES]


def _exact32(t):
    return torch.equal(t.float().double(), t)


def chunks(npix, C):
    n = int(_lib.load_real().bts_bn_train_ws_floats(npix, C))
    assert n > 0 and n % (3 * C) == 0
    return n // (3 * C)


@pytest.mark.parametrize("shape,expected", sc.BN_SHAPES)
def test_bn_chunk_counts(shape, expected):
    assert chunks(*shape) == expected


def test_bn_shapes_reach_every_path():
    counts = dict(sc.BN_SHAPES)
    # the three reduce kernels, each with more than one channel group and a partial last one somewhere
    for lanes in (8, 16, 32):
        mine = [(n, C) for n, C in ALL_BN if sc.lanes_for(C) == lanes]
        assert mine, lanes
        assert any(C > 4 * lanes and C % (4 * lanes) for _, C in mine), "no partial second channel group at %d lanes" % lanes
    assert sc.lanes_for(108) == 16 and sc.lanes_for(112) == 32 and sc.lanes_for(44) == 8 and sc.lanes_for(48) == 16
    assert max(C for _, C in ALL_BN) // 128 + 1 == 18                              # 2208 channels: 18 groups
    # a ragged last chunk: the chunk rows do not divide npix
    assert any(counts[s] > 1 and s[0] % counts[s] for s in ALL_BN)
    # the finalize walk: every chunk exactly once, and the counts sit where the issue of each path begins
    for n in sorted(set(counts.values())):
        walk = sc.finalize_walk(n)
        seen = sorted(k for u, r in walk for k in u + r)
        assert seen == list(range(n)), n
    unrolled = {n: [lane for lane, (u, _) in enumerate(sc.finalize_walk(n)) if u] for n in counts.values()}
    assert all(not unrolled[n] for n in counts.values() if n <= 24) and sum(1 for n in counts.values() if 1 < n <= 24) >= 4
    assert unrolled[25] == [0] and sc.finalize_walk(25)[0][1] == []              # lane 0 alone, nothing after the trip
    assert unrolled[26] == [0, 1]
    assert unrolled[33] == list(range(8)) and sc.finalize_walk(33)[0][1] == [32]   # a remainder step after an unrolled trip
    assert len(unrolled[58]) == 8 and len(sc.finalize_walk(58)[1][0]) == 8        # two unrolled trips
    assert all(len(u) == 128 and not r for u, r in sc.finalize_walk(1024))
    assert chunks(98304 * 4, 8) == 1024                                            # the cap holds beyond this size
    # chunks * rows_per_chunk overshoots npix by less than the NaN guard rows the GPU tests put behind the input
    # (rows_per_chunk = the chunk size rounded up to the block's rows: 256 / lanes)
    for (npix, C), n in sc.BN_SHAPES:
        ry = 256 // sc.lanes_for(C)
        rows = -(-(-(-npix // n)) // ry) * ry
        assert -(-npix // rows) == n and 0 <= n * rows - npix < 128, (npix, C, rows)


def test_grid_stride_cases_exceed_one_launch():
    caps = sc.block_caps()
    assert caps == {"bn_train.hip": 8192, "pool.hip": 4096, "layout.hip": 4096, "tail.hip": 4096, "upconv.hip": 8192}
    T = sc.THREADS
    npix, C = sc.BN_GRID_STRIDE
    assert npix * (C // 4) > caps["bn_train.hip"] * T
    B, h, w, C = sc.POOL_GRID_STRIDE
    assert B * ((h + 1) // 2) * ((w + 1) // 2) * (C // 4) > caps["pool.hip"] * T          # maxpool
    assert h % 2 == 0 and w % 2 == 0 and B * (h // 2) * (w // 2) * (C // 4) > caps["pool.hip"] * T
    B, HW = sc.LAYOUT_GRID_STRIDE
    assert B * HW > caps["layout.hip"] * T
    assert sc.PACK_GRID_STRIDE > caps["tail.hip"] * T
    B, h, w, c = sc.COMBINE_GRID_STRIDE
    assert B * 2 * h * 2 * w * (c // 4) > caps["upconv.hip"] * T
    # none of the regular cases does: they stay quick
    for n, C in ALL_BN:
        assert n * (C // 4) <= caps["bn_train.hip"] * T


@pytest.mark.parametrize("shape", ALL_BN + [sc.BN_GRID_STRIDE])
def test_bn_apply_design_is_exact(shape):
    x, scale, shift = sc.bn_apply_case(*shape)
    assert x.abs().max() <= 64 and x.abs().max() >= min(32, shape[0]) and set(scale.abs().tolist()) <= {0.5, 1.0, 2.0}
    assert _exact32(x.double() * scale.double())                       # the product alone (no FMA) ...
    for relu in (False, True):
        assert _exact32(sc.bn_apply_ref(x, scale, shift, relu))         # ... and the sum


@pytest.mark.parametrize("shape", ALL_BN + [sc.BN_GRID_STRIDE])
def test_bn_backward_design_is_exact(shape):
    x, dy, mean, invstd, scale, shift = sc.bn_bwd_case(*shape)
    for relu in (False, True):
        r = sc.bn_bwd_ref(x, dy, mean, invstd, scale, shift, relu)
        assert _exact32(r["z"]) and torch.equal(2 * r["z"], torch.round(2 * r["z"]))      # multiples of 1/2, exact
        assert torch.equal(shift, torch.round(shift))
        # xhat and g*xhat are multiples of 1/4; every partial sum of any summation order is bounded by the sum of
        # magnitudes, so 4 * sum |g*xhat| < 2^24 keeps all of them exact in fp32
        assert torch.equal(4 * r["xhat"], torch.round(4 * r["xhat"]))
        abs_g, abs_gx = r["abs_sums"]
        assert float(abs_g.max()) < 2 ** 24 and 4 * float(abs_gx.max()) < 2 ** 24
        assert _exact32(r["dbeta"]) and _exact32(r["dgamma"])
    if shape[0] * shape[1] >= 2048:          # pre-activations that are exactly 0, under a non-zero gradient
        at_zero = (r["z"] == 0) & (dy != 0)
        assert int(at_zero.sum()) >= 8
        assert bool((r["g"][at_zero] == 0).all())
    # the 2-pixel case still has the mask both ways
    x, dy, mean, invstd, scale, shift = sc.bn_bwd_case(2, 4)
    z = sc.bn_bwd_ref(x, dy, mean, invstd, scale, shift, True)["z"]
    assert bool((z > 0).any()) and bool((z <= 0).any())


def test_pool_designs_are_exact():
    for shape in sc.MAXPOOL_SHAPES:
        x = sc.maxpool_case(*shape)
        assert x.unique().numel() == x.numel() and float(x.abs().max()) < 2 ** 24
    B, h, w, C = sc.POOL_GRID_STRIDE
    assert B * h * w * C // 2 + 1 < 2 ** 24                               # randperm(n) - n // 2 stays exact in fp32
    for shape in sc.AVGPOOL_SHAPES:
        x, scale, shift = sc.avgpool_case(*shape)
        assert shape[1] % 2 == 0 and shape[2] % 2 == 0
        assert _exact32(x.double() * scale.double()) and _exact32(sc.avgpool_ref(x, scale, shift))
    assert any(C > 128 for _, _, _, C in sc.MAXPOOL_SHAPES) and any(h == 1 for _, h, _, _ in sc.MAXPOOL_SHAPES)
    assert any(w == 1 for _, _, w, _ in sc.MAXPOOL_SHAPES) and any(h % 2 and h > 1 for _, h, _, _ in sc.MAXPOOL_SHAPES)


def test_layout_cases_cover_the_tile_edges():
    assert {1, 2, 3, 4} <= set(sc.LAYOUT_C) and {5, 31, 32, 33, 64} <= set(sc.LAYOUT_C)      # both kernels, tile edges
    assert {1, 31, 32, 33} <= set(sc.LAYOUT_HW)
    x = sc.layout_case(3, 5, 45)
    neg0 = (sc.bits(x) == -2 ** 31)
    assert bool(neg0.any()) and bool((x < 0).any()) and bool((sc.bits(x) == 0).any())


@pytest.mark.parametrize("C,H,W", sc.DEPTH_CASES)
def test_depth_cases_recover_their_integers(C, H, W):
    x, w, acc = sc.depth_case(C, H, W)
    assert torch.equal(acc, torch.round(acc)) and float(acc.abs().max()) < 2 ** 24
    assert W % 8 == 0
    small = acc.abs() <= sc.DEPTH_EXACT_ACC
    assert float(small.double().mean()) >= 0.95, float(small.double().mean())
    for b in range(sc.DEPTH_B):                  # every border row and column holds exactly-checked pixels
        s = small[b, 0]
        assert bool(s[0].any()) and bool(s[-1].any()) and bool(s[:, 0].any()) and bool(s[:, -1].any())
    focal = torch.tensor(sc.DEPTH_FOCAL)
    for f in (None, focal):
        # the fp64 statement rounded to fp32 (what a perfect kernel stores) gives the integer back where |acc| <= 8
        out = sc.depth_ref(acc, sc.DEPTH_MAX[C], f).float()
        assert torch.equal(sc.depth_recover(out, sc.DEPTH_MAX[C], f)[small], acc[small])
    # a missing tap moves the logit by at least 1: at |acc| <= 8 + 2 the depth moves by more than 3e-4 * max_depth
    a = torch.tensor(float(sc.DEPTH_EXACT_ACC))
    assert float(torch.sigmoid(a + 1) - torch.sigmoid(a)) > 2e-4


def test_depth_cases_have_border_taps():
    """Some input sits next to every edge somewhere, so the edge scalars p[-1] / p[8] and the row guards matter."""
    x, _, _ = sc.depth_case(32, 35, 136)
    assert bool(x[..., 0].any()) and bool(x[..., -1].any()) and bool(x[..., 0, :].any()) and bool(x[..., -1, :].any())
    assert bool(x[..., 7].any()) and bool(x[..., 8].any()) and bool(x[..., 127].any()) and bool(x[..., 128].any())
    assert (35 + 1) // 2 > 16 and 136 // 8 > 16          # more than one block in both directions, the last one ragged


def test_combine_design_is_exact():
    for B, h, w, c in sc.COMBINE_SHAPES:
        taps, es, eb = sc.combine_case(B, h, w, c)
        for act in (0, 1, 2):
            for e2 in (None, (es, eb)):
                y, v = sc.combine_ref(taps, B, h, w, c, act, e2)
                assert torch.equal(v, torch.round(v)) and float(v.abs().max()) <= 72
                keep = (v >= 0) if act == 2 else torch.ones_like(v, dtype=torch.bool)
                assert _exact32(y[keep])
        assert bool((v < 0).any()) and bool((v > 0).any())
        assert float(es.abs().max()) <= 1.0                  # the ELU error is not amplified by e2
    # the statement against the layer it restates: nearest-2x upsample + 3x3 convolution
    B, h, w, c = 2, 3, 5, 4
    g = sc._gen(99)
    x = sc._ints(g, -3, 3, (B, 6, h, w)).double()
    wt = sc._ints(g, -2, 2, (c, 6, 3, 3)).double()
    P = torch.einsum("bkyx,nkt->byxtn", x, wt.view(c, 6, 9)).reshape(B * h * w, 9 * c)
    want = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    assert torch.equal(sc.combine_ref(P, B, h, w, c, 0, None)[0], want.permute(0, 2, 3, 1))


def test_stats_floor_is_a_function_of_the_case():
    """The tolerance of the stats test comes from the fp32 two-pass statement alone; the cancellation case must be one
    where the unshifted one-pass formula has no correct digit (so the shift is what the test sees)."""
    x, gamma, beta, rm, rv = sc.bn_stats_input(515, 108, "cancel")
    r64, e32, tol = sc.bn_stats_floor(x, gamma, beta, rm, rv, 0.1)
    assert set(e32) == set(sc.STATS_KEYS)
    x32 = x.float()
    naive_var = (x32 * x32).sum(0) / 515 - (x32.sum(0) / 515) ** 2          # E[x^2] - E[x]^2 in fp32
    true_var = r64["m2"] / 515
    assert float(((naive_var.double() - true_var).abs() / true_var).median()) > 10.0
    naive_invstd = 1.0 / torch.sqrt(naive_var.clamp_min(0) + sc.BN_EPS).double()
    assert float(((naive_invstd - r64["invstd"]).abs() > tol["invstd"]).double().mean()) > 0.9
    assert float(tol["invstd"].max() / r64["invstd"].abs().min()) < 1e-3
