"""GPU: the weight packs of the training step against the plain statements of tests/pack_cases.py, bit for bit.

pack_weights_kernel (csrc/pack.hip) through the C ABI -- each layout alone, then one table of every record in three
orders and in sub-tables around a power of two (bts_table_find) -- and through train.WeightPacker; pack_wino_kernel on an
integer design where U = G g G^T is exact in fp32.  Every launch writes into memory pre-filled with a NaN pattern and
fenced by sentinel floats; every comparison is equality of int32 views (tests/test_adamw_gpu.py holds AdamW's in-kernel
re-pack against the same statements)."""
import numpy as np
import pytest
import torch

import pack_cases as PC
from bts_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in PC.CASES]


def _i32(pattern):
    return int(np.uint32(pattern).astype(np.int32))


class _Slab:
    """One device buffer: a region per record, pre-filled with the NaN poison, sentinel floats everywhere else."""

    def __init__(self, recs):
        self.recs = recs
        self.offs, self.floats = PC.slab_layout(recs)
        self.bits = torch.empty(self.floats, dtype=torch.int32, device="cuda")
        assert self.bits.data_ptr() % 16 == 0
        inside = torch.zeros(self.floats, dtype=torch.bool)
        for o, r in zip(self.offs, recs):
            inside[o:o + r.floats] = True
        self.inside = inside.cuda()
        self.reset()

    def reset(self):
        self.bits.fill_(_i32(PC.FENCE))
        self.bits[self.inside] = _i32(PC.POISON)

    def ptr(self, i):
        return self.bits.data_ptr() + 4 * self.offs[i]

    def region(self, i):
        return self.bits[self.offs[i]:self.offs[i] + self.recs[i].floats]

    def fences_intact(self):
        return bool((self.bits[~self.inside] == _i32(PC.FENCE)).all())


@pytest.fixture(scope="module")
def sources():
    """The cases' weights on the device, one tensor per shape (_assert_sources_unchanged: no launch may write them)."""
    out = {}
    for c in PC.CASES:
        if c.shape not in out:
            out[c.shape] = PC.weight(c.shape).cuda()
    return out


def _launch(slab, sources, which):
    """One launch of bts_pack_weights_f32 over the records slab.recs[i], i in `which`, in that order."""
    recs = [slab.recs[i] for i in which]
    table, blocks = PC.table_array(recs, [sources[PC.BY_NAME[r.case].shape].data_ptr() for r in recs], [slab.ptr(i) for i in which])
    dev = torch.from_numpy(table).cuda()
    rc = _lib.load_real().bts_pack_weights_f32(dev.data_ptr(), len(recs), blocks, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()


def _assert_slab(slab, written, what):
    """Regions in `written` hold their statements, every other region still its poison, every fence its sentinel."""
    for i, r in enumerate(slab.recs):
        got = slab.region(i).cpu().numpy()
        if i in written:
            assert np.array_equal(got, PC.record_statement(r)), (what, r.case, r.index)
        else:
            assert (got == _i32(PC.POISON)).all(), (what, "wrote a record that is not in the table", r.case, r.index)
    assert slab.fences_intact(), what


def _assert_sources_unchanged(sources):
    for shape, t in sources.items():
        assert torch.equal(t.cpu().view(torch.int32), PC.weight(shape).view(torch.int32)), shape


# ------------------------------------------------------------------------------------------------ a. each layout alone
@pytest.mark.parametrize("name", NAMES)
def test_each_layout_alone_equals_its_statement_in_a_fenced_region(name, sources):
    recs = [r for r in PC.records() if r.case == name]
    slab = _Slab(recs)
    for i in range(len(recs)):                               # one-record tables: every bundle is a launch of its own
        _launch(slab, sources, [i])
        _assert_slab(slab, set(range(i + 1)), "record %d" % i)
    first = slab.bits.clone()
    for i in range(len(recs)):                               # a second launch into the same regions
        _launch(slab, sources, [i])
    assert torch.equal(slab.bits, first)
    _assert_sources_unchanged({PC.BY_NAME[name].shape: sources[PC.BY_NAME[name].shape]})


# ------------------------------------------------------------------------------------------------ b. one table of everything
@pytest.mark.parametrize("order", ["listed", "reversed", "interleaved"])
def test_one_table_of_every_record(order, sources):
    recs = PC.orders()[order]
    slab = _Slab(recs)
    _launch(slab, sources, list(range(len(recs))))
    _assert_slab(slab, set(range(len(recs))), order)
    _assert_sources_unchanged(sources)


@pytest.mark.parametrize("n", PC.SUBTABLE_SIZES)
def test_subtables_around_a_power_of_two(n, sources):
    recs = PC.orders()["interleaved"]
    slab = _Slab(recs)
    for start in (0, len(recs) - n):                          # the first n records, then the last n, of the interleaved order
        which = list(range(start, start + n))
        slab.reset()
        _launch(slab, sources, which)
        _assert_slab(slab, set(which), "records %d..%d" % (start, start + n - 1))


# ------------------------------------------------------------------------------------------------ c. train.WeightPacker
def _assert_buffer(buf, w, case, what):
    from bts_amd import train
    rows, shape = train.WeightPacker._rows(w, case.c_in_ld, case.mode, case.groups)
    assert tuple(buf.shape) == tuple(shape) == tuple(case.dst_shape)
    want = PC.statement(w.detach().cpu(), rows, shape, case.groups)
    got = buf.cpu().view(torch.int32).numpy()
    assert np.array_equal(got, want), (what, case.name)
    if case.mode in (PC.FWD, PC.DGRAD):                      # said once more on its own: the padding is +0.0 bits
        pad = ~np.stack([PC.real_mask(r) for r in rows]).reshape(shape)
        assert not got[pad].any(), (what, case.name)


@pytest.mark.parametrize("name", NAMES)
def test_weight_packer_follows_in_place_changes(name):
    from bts_amd import train
    case = PC.BY_NAME[name]
    w = torch.nn.Parameter(PC.weight(case.shape).cuda())
    packer = train.WeightPacker()
    buf = packer.get(w, case.c_in_ld, case.mode, case.groups)
    _assert_buffer(buf, w, case, "first get")
    seq = buf._bts_pack_seq
    ptr, storage = w.data_ptr(), buf.data_ptr()
    buf.view(torch.int32).fill_(_i32(PC.POISON))             # the next pack must write every float, padding included
    with torch.no_grad():
        w.mul_(-1.5).add_(0.25)                               # same storage, version bumped
    assert w.data_ptr() == ptr
    again = packer.get(w, case.c_in_ld, case.mode, case.groups)
    assert again is buf and buf.data_ptr() == storage and buf._bts_pack_seq > seq
    _assert_buffer(buf, w, case, "get after mul_/add_")
    seq, version = buf._bts_pack_seq, w._version
    buf.view(torch.int32).fill_(_i32(PC.POISON))
    w.data.mul_(0.5)                                          # as torch's fused optimisers write: no version bump
    assert w._version == version and w.data_ptr() == ptr
    packer.refresh(force=True)
    assert packer.get(w, case.c_in_ld, case.mode, case.groups) is buf and buf._bts_pack_seq == seq + 1
    _assert_buffer(buf, w, case, "refresh(force=True)")


# ------------------------------------------------------------------------------------------------ e. Winograd form on integers
@pytest.mark.parametrize("cout,cin_ld,n_tail,c16", PC.WINO)
def test_pack_wino_weight_is_exact_on_integers(cout, cin_ld, n_tail, c16):
    from bts_amd import ops
    wp = PC.wino_integer_weight(cout, cin_ld).cuda()
    ref = ops.pack_wino_weight_reference(wp, cin_ld, n_tail, c_out16=c16)
    n = ref.numel()
    assert n == int(_lib.load_real().bts_pack_wino_floats(cout, cin_ld, n_tail, c16))
    slab = torch.full((n + 2 * PC.GUARD,), _i32(PC.FENCE), dtype=torch.int32, device="cuda")
    slab[PC.GUARD:PC.GUARD + n] = _i32(PC.POISON)
    out = slab.view(torch.float32)[PC.GUARD:PC.GUARD + n]
    got = ops.pack_wino_weight(wp, cin_ld, n_tail, c_out16=c16, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))          # -0.0 against +0.0 would show here
    assert bool((got * 4 == (got * 4).round()).all()) and float(got.abs().max()) <= 72
    assert bool((slab[:PC.GUARD] == _i32(PC.FENCE)).all()) and bool((slab[PC.GUARD + n:] == _i32(PC.FENCE)).all())
    assert torch.equal(wp.cpu(), PC.wino_integer_weight(cout, cin_ld))
