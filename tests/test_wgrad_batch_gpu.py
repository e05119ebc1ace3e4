"""bts_conv_wgrad_batch_f32 (csrc/wgrad.hip: conv_wgrad_batch_kernel in its four tiles + wgrad_reduce_batch_kernel)
through ops.WgradBatch, on the batches of tests/wgrad_batch_cases.py, against the fp64 statement of the weight gradient
of tests/test_wgrad_gpu.py.

As there, the exact test feeds small integers, so that every partial sum is an integer below 2^24 and fp32 accumulation
is exact in any order: tile, split, workspace layout and reduction order cannot change a bit and the assertion is
torch.equal.  The float-valued test holds fp32 products under the worst-case bound of an fp32 summation chain, with the
split geometry taken from the batch plan."""
import functools
import zlib

import pytest
import torch

import wgrad_batch_cases as bc
import wgrad_cases as wc
from bts_amd import ops
from test_wgrad_gpu import SENTINEL, reference

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _operands(c, g, exact):
    """(x [B,h,w,nb*c_in], dy [B,H,W,nb*c_out], scale, shift) in fp64 on the CPU."""
    H, W = wc.out_hw(c)
    nb = max(c.n_bundles, 1)
    if not exact:
        x = torch.randn(c.B, c.h, c.w, nb * c.c_in, generator=g).double()
        dy = torch.randn(c.B, H, W, nb * c.c_out, generator=g).double()
        scale = shift = None
        if c.pre:
            x, scale, shift = _exact_prologue(x, nb * c.c_in, g)
        return x, dy, scale, shift
    M = c.B * H * W
    xmax = min(511, int(0.6 * 2 ** 24 * 3 / (M * (2 if c.pre else 1))))
    assert xmax >= 300
    scale = shift = None
    if c.pre:
        x = 2.0 * torch.randint(-(xmax // 2), xmax // 2 + 1, (c.B, c.h, c.w, nb * c.c_in), generator=g).double()
        scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (nb * c.c_in,), generator=g)]
        shift = torch.randint(-9, 10, (nb * c.c_in,), generator=g).double()
    else:
        x = torch.randint(-xmax, xmax + 1, (c.B, c.h, c.w, nb * c.c_in), generator=g).double()
    dy = torch.randint(-1, 2, (c.B, H, W, nb * c.c_out), generator=g).double()
    return x, dy, scale, shift


def _exact_prologue(x, n, g):
    """The bound of the float test is for fp32 sums of fp32 products of the GIVEN operands, so where a prologue rides
    along it must not round: x on a 2^-10 grid, scale in {0.5, 1, 2} and shift on the same grid (|x*scale + shift| < 64
    on a 2^-11 grid: 17 bits) make relu(x*scale + shift) exact in fp32, fused or not."""
    q = lambda t: (t.double().clamp(-8.0, 8.0) * 1024.0).round() / 1024.0
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]
    return q(x), scale, q(torch.randn(n, generator=g))


def _dense_operands(g, exact):
    """The mini dense block's shared buffers: every 1x1 reads a prefix of `buf`, every 3x3 a slab of T1; the gradients
    are column slices of G and slabs of D_T1."""
    D = bc.DENSE
    npix, Ct, L, mid, gr = D["B"] * D["H"] * D["W"], bc.DENSE_CT, D["L"], D["mid"], D["g"]
    if exact:
        buf = 2.0 * torch.randint(-200, 201, (npix, Ct), generator=g).double()
        T1 = 2.0 * torch.randint(-200, 201, (L, npix, mid), generator=g).double()
        G = torch.randint(-1, 2, (npix, Ct), generator=g).double()
        D_T1 = torch.randint(-1, 2, (L, npix, mid), generator=g).double()
        pick = lambda n: torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]
        off = lambda n: torch.randint(-9, 10, (n,), generator=g).double()
    else:
        buf, _, _ = _exact_prologue(torch.randn(npix, Ct, generator=g), 1, g)
        T1, _, _ = _exact_prologue(torch.randn(L, npix, mid, generator=g), 1, g)
        G, D_T1 = torch.randn(npix, Ct, generator=g).double(), torch.randn(L, npix, mid, generator=g).double()
        pick = lambda n: _exact_prologue(torch.zeros(1), n, g)[1]
        off = lambda n: _exact_prologue(torch.zeros(1), n, g)[2]
    stats = torch.zeros(L, 4, Ct, dtype=torch.float64)          # rows: scale1, shift1 (Ci entries), scale2, shift2 (mid entries)
    per_case = []
    for i in range(L):
        Ci = D["C0"] + i * gr
        stats[i, 0, :Ci], stats[i, 1, :Ci], stats[i, 2, :mid], stats[i, 3, :mid] = pick(Ci), off(Ci), pick(mid), off(mid)
        shp = (D["B"], D["H"], D["W"], -1)
        per_case.append((buf[:, :Ci].reshape(shp), D_T1[i].reshape(shp), stats[i, 0, :Ci], stats[i, 1, :Ci]))
        per_case.append((T1[i].reshape(shp), G[:, Ci:Ci + gr].reshape(shp), stats[i, 2, :mid], stats[i, 3, :mid]))
    return dict(buf=buf, T1=T1, G=G, D_T1=D_T1, stats=stats), per_case


@functools.lru_cache(maxsize=None)
def _data(name, exact):
    """Operands and fp64 reference of every problem of a batch, computed once and never modified."""
    _, cases = bc.BATCHES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + int(exact))
    shared = None
    if name == "mini_dense":
        shared, ops_ = _dense_operands(g, exact)
    else:
        ops_ = [_operands(c, g, exact) for c in cases]
    out = []
    for c, (x, dy, scale, shift) in zip(cases, ops_):
        ref, mag = reference(c, x, dy, scale, shift)
        if exact:
            assert mag.max().item() < 2 ** 24, "%s breaks the exactness precondition: shrink the range of x" % c.name
        out.append((x, dy, scale, shift, ref, mag))
    return shared, out


def _carve(flat, cursor, values, extra):
    """`values` [rows, C] as a channel slice, at a non-zero offset, of a region `extra` channels wider inside `flat`
    (NaN elsewhere)."""
    rows, Cc = values.shape
    width = Cc + extra
    region = flat[cursor:cursor + rows * width].view(rows, width)
    view = region[:, extra // 2:extra // 2 + Cc]
    view.copy_(values)
    return view, cursor + (rows * width + 3) // 4 * 4


def _build(name, exact):
    """(problems for ops.WgradBatch, bases) on the GPU."""
    _, cases = bc.BATCHES[name]
    shared, data = _data(name, exact)
    geo = lambda c: dict(B=c.B, h_in=c.h, w_in=c.w, c_in=c.c_in, c_out=c.c_out, ksize=c.ksize, dil=c.dil, stride=c.stride,
                         pad=c.pad, up=c.up, n_bundles=c.n_bundles, pre_relu=c.pre_relu)
    n_dw = sum(bc.dw_floats(c) for c in cases)
    DW = torch.full((n_dw,), SENTINEL, device="cuda")
    problems, at = [], 0
    if name == "mini_dense":
        D = bc.DENSE
        dev = {k: v.float().cuda() for k, v in shared.items()}
        for j, c in enumerate(cases):
            i, Ci = j // 2, D["C0"] + (j // 2) * D["g"]
            if j % 2 == 0:
                x, dy, pre = dev["buf"][:, :Ci], dev["D_T1"][i], (dev["stats"][i, 0, :Ci], dev["stats"][i, 1, :Ci])
            else:
                x, dy = dev["T1"][i], dev["G"][:, Ci:Ci + D["g"]]
                pre = (dev["stats"][i, 2, :D["mid"]], dev["stats"][i, 3, :D["mid"]])
            problems.append(dict(geo(c), x=x, dy=dy, pre=pre, dw=DW[at:at + bc.dw_floats(c)]))
            at += bc.dw_floats(c)
        return problems, [dev["buf"], dev["G"], dev["T1"], dev["D_T1"], dev["stats"], DW]
    size = lambda which, extra: sum((d[which].numel() // d[which].shape[-1] * (d[which].shape[-1] + getattr(c, extra)) + 3) // 4 * 4
                                    for c, d in zip(cases, data))
    X = torch.full((size(0, "x_extra"),), NAN, device="cuda")
    DY = torch.full((size(1, "dy_extra"),), NAN, device="cuda")
    PRE = torch.full((max(sum(2 * d[2].numel() for d in data if d[2] is not None), 4),), NAN, device="cuda")
    cx = cy = cp = 0
    for c, (x, dy, scale, shift, _, _) in zip(cases, data):
        xv, cx = _carve(X, cx, x.reshape(-1, x.shape[-1]).float(), c.x_extra)
        dv, cy = _carve(DY, cy, dy.reshape(-1, dy.shape[-1]).float(), c.dy_extra)
        pre = None
        if scale is not None:
            n = scale.numel()
            PRE[cp:cp + n], PRE[cp + n:cp + 2 * n] = scale.float(), shift.float()
            pre = (PRE[cp:cp + n], PRE[cp + n:cp + 2 * n])
            cp += 2 * n
        problems.append(dict(geo(c), x=xv, dy=dv, pre=pre, dw=DW[at:at + bc.dw_floats(c)]))
        at += bc.dw_floats(c)
    return problems, [X, DY, PRE, DW]


def _check_exact(name, dws, what):
    _, cases = bc.BATCHES[name]
    for c, dw, d in zip(cases, dws, _data(name, True)[1]):
        ref = d[4]
        got = dw.cpu().double().reshape(ref.shape)
        if not torch.equal(got, ref):
            bad = ~(got == ref)                                 # NaN counts as wrong
            pytest.fail("%s / %s, %s: %d wrong of %d, first at %s" % (name, c.name, what, int(bad.sum()), bad.numel(),
                                                                    bad.nonzero()[0].tolist()))


@pytest.mark.parametrize("name", list(bc.BATCHES))
def test_every_problem_of_the_batch_is_exact_on_small_integers(name):
    ws_floats, cases = bc.BATCHES[name]
    problems, bases = _build(name, True)
    batch = ops.WgradBatch(problems, bases, ws_floats)
    assert batch.plan == bc.plan_of(name)                      # real addresses, same plan
    ws = torch.full((ws_floats,), SENTINEL, device="cuda")
    first = [d.clone() for d in batch.run(bases, ws)]
    written = torch.zeros(ws_floats, dtype=torch.bool, device="cuda")
    for c, (_, _, split, _, off) in zip(cases, batch.plan):
        if split > 1:
            written[off:off + split * bc.dw_floats(c)] = True
    touched = ws != SENTINEL
    assert not bool((touched & ~written).any()), "the launch wrote workspace outside the planned regions"
    assert not bool((~touched & written).any()), "a partial tile inside a planned region was never written"
    bases[-1].fill_(SENTINEL)
    second = batch.run(bases, ws)                              # same workspace, now holding the first run's partials
    _check_exact(name, first, "first run")
    _check_exact(name, second, "second run into the same workspace")


@pytest.mark.parametrize("name", bc.FLOAT_BATCHES)
def test_fp32_products_within_the_summation_bound(name):
    """Standard-normal operands -- with one departure, stated here: where a prologue rides along (every problem of
    mini_dense, mix_bundles of mixed) x is the standard-normal draw clamped to +-8 and rounded to a 2^-10 grid, scale is one
    of 0.5 / 1 / 2 and shift lies on the same grid, so that relu(x*scale + shift) is exact in fp32 (_exact_prologue); dy is a
    full-mantissa standard-normal everywhere and so is x of the problems without a prologue (four of the five of mixed).
    The bound is for fp32 sums of fp32 products of the given operands; a prologue that rounds would add an error the bound
    does not describe, and the single-launch float test has no prologue at all.  Per element |got - ref| <= (pix_per_split + split + 2) * 2^-24 * sum |dy| * |x_tap|, the
    worst-case bound of tests/test_wgrad_gpu.py with the split geometry of the batch plan (operands with a prologue
    are standard-normal on a grid that keeps the prologue exact, see _exact_prologue).  Two runs give identical bits whatever the workspace held."""
    ws_floats, cases = bc.BATCHES[name]
    problems, bases = _build(name, False)
    batch = ops.WgradBatch(problems, bases, ws_floats)
    ws = torch.full((ws_floats,), 1.0e30, device="cuda")
    first = [d.clone() for d in batch.run(bases, ws)]
    ws.fill_(NAN)
    second = batch.run(bases, ws)
    for c, a, b, d, (bm, bn, split, pps, _) in zip(cases, first, second, _data(name, False)[1], batch.plan):
        assert torch.equal(a, b), c.name
        ref, mag = d[4], d[5]
        err = (a.cpu().double().reshape(ref.shape) - ref).abs()
        bound = (pps + split + 2) * 2.0 ** -24 * mag
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        print("%s / %s: tile %dx%d split %d x %d pixels: max |err| / bound = %.4f" % (name, c.name, bm, bn, split, pps, ratio))
        assert bool((err <= bound).all()), (c.name, ratio)


@pytest.mark.parametrize("name", ["t64_geometries", "mixed"])
def test_dw_is_the_documented_fixed_order_sum_of_the_partials(name):
    """Float operands, where the summation order shows: after the launch each split problem's partials sit at its plan's
    ws_offset as [split][bundle][c_out][N], and its dw has the bits of wc.sum_splits over them.  t64_geometries splits up
    to 615 ways (the four-at-a-time loop), mixed 6 to 25 ways beside an unsplit problem; the workspace outside the planned
    regions -- all of it, for an unsplit problem -- keeps its sentinel."""
    ws_floats, cases = bc.BATCHES[name]
    problems, bases = _build(name, False)
    batch = ops.WgradBatch(problems, bases, ws_floats)
    splits = [p[2] for p in batch.plan]
    assert min(splits) == 1 and max(splits) > (64 if name == "t64_geometries" else 16)
    ws = torch.full((ws_floats,), SENTINEL, device="cuda")
    dws = batch.run(bases, ws)
    planned = torch.zeros(ws_floats, dtype=torch.bool, device="cuda")
    for c, dw, (_, _, split, _, off) in zip(cases, dws, batch.plan):
        if split == 1:
            assert off == -1
            continue
        n = bc.dw_floats(c)
        planned[off:off + split * n] = True
        want = torch.from_numpy(wc.sum_splits(ws[off:off + split * n].cpu().numpy().reshape(split, n))).reshape(dw.shape)
        got = dw.cpu()
        assert torch.equal(got, want), "%s / %s, split %d: %d of %d elements differ" % (name, c.name, split, int((got != want).sum()), n)
    assert bool((ws[~planned] == SENTINEL).all()), "the launch wrote workspace outside the split problems' regions"


def test_one_table_serves_buffers_at_other_addresses_without_a_sync():
    name = "mixed_small_ws"
    ws_floats, cases = bc.BATCHES[name]
    problems, bases = _build(name, True)
    batch = ops.WgradBatch(problems, bases, ws_floats)
    ws = torch.empty(ws_floats, device="cuda")
    _check_exact(name, batch.run(bases, ws), "the buffers the batch was built on")
    moved = [b.clone() for b in bases]                         # `bases` stay alive: these sit elsewhere
    assert all(m.data_ptr() != b.data_ptr() for m, b in zip(moved, bases))
    moved[-1].fill_(SENTINEL)
    ws2 = torch.empty(ws_floats, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dws = batch.run(moved, ws2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(d.data_ptr() >= moved[-1].data_ptr() for d in dws)
    bases[-1].fill_(SENTINEL)                                  # the second run must not have written the first run's dw
    _check_exact(name, dws, "other buffers, same table")
    assert bool((bases[-1] == SENTINEL).all())


def test_an_empty_batch_launches_nothing():
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        assert ops.WgradBatch([], [torch.zeros(4, device="cuda")], 0).run([torch.zeros(4, device="cuda")], None) == []
    finally:
        ops.set_trace(None)
    assert tr.records == []


def test_a_batch_is_one_trace_record_with_the_summed_work():
    name = "single"
    ws_floats, cases = bc.BATCHES[name]
    problems, bases = _build(name, True)
    batch = ops.WgradBatch(problems, bases, ws_floats, tag="some.wgrad")
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        batch.run(bases, torch.empty(ws_floats, device="cuda"))
    finally:
        ops.set_trace(None)
    assert [(r[0], r[1]) for r in tr.records] == [("conv_wgrad_batch_kernel", "some.wgrad")]
    c = cases[0]
    assert tr.records[0][2] == 2.0 * bc.pixels(c) * bc.dw_floats(c)
