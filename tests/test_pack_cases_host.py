"""What tests/pack_cases.py promises, asserted on the CPU (no GPU): its statements agree with the torch packers of
bts_amd.ops on every case, its rows and shapes are train.WeightPacker's, its block figures are bts_pack_weights_blocks',
every planted bit pattern lands on a real element, and the record orders have the edges the GPU tests rely on."""
import numpy as np
import pytest
import torch

import pack_cases as PC
from bts_amd import _lib, ops, train

NAMES = [c.name for c in PC.CASES]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).numpy()


def test_the_table_is_the_one_the_issue_states():
    assert len(PC.DENSE) == 6 and len(PC.BUNDLES) == 5 and len(PC.NATIVE) == 3
    assert len(PC.CASES) == 2 * 14 and len(set(NAMES)) == len(NAMES)
    recs = PC.records()
    assert len(recs) == 46                                                    # 12 dense, 28 bundles, 6 native
    assert max(r.floats for r in recs) == PC.LARGEST_DST
    assert PC.BY_NAME["dense33x5k3_fwd"].c_in_ld == 8 > 5                     # c_in_ld > inner
    assert [max(32, c // g) for c, g in PC.BUNDLES] == [32, 32, 32, 32, 64]
    assert [c // g for c, g in PC.BUNDLES] == [4, 8, 16, 32, 64]              # several groups, one group, cg = cb = 64


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_shapes_are_weight_packers(name):
    c = PC.BY_NAME[name]
    rows, shape = train.WeightPacker._rows(PC.weight(c.shape), c.c_in_ld, c.mode, c.groups)
    assert [tuple(r) for r in rows] == PC.table_rows(c)
    assert tuple(shape) == tuple(c.dst_shape)
    assert all(len(r) == 13 for r in rows)
    assert sum(r[6] * r[7] for r in rows) == int(np.prod(c.dst_shape))
    for r in rows:                                                            # what the kernel's 16-byte stores need
        assert (r[6] * r[7]) % 4 == 0 and r[1] % 4 == 0
    if c.groups > 1 and c.mode in (PC.FWD, PC.DGRAD):
        assert train.WeightPacker.bundle_channels(PC.weight(c.shape), c.groups) == c.c_in_ld


def test_block_figures_come_from_the_library():
    lib = _lib.load_real()
    assert int(lib.bts_pack_weights_blocks(64, 64)) == 1 and int(lib.bts_pack_weights_blocks(64, 65)) == 2
    for d, (bf, bd) in zip(PC.DENSE, PC.DENSE_BLOCKS):
        for shape, frac in ((d.fwd_dst, bf), (d.dgrad_dst, bd)):
            assert shape[0] * shape[1] == frac * PC.BLOCK
            assert int(lib.bts_pack_weights_blocks(*shape)) == int(np.ceil(frac))
    for r in PC.records():
        assert int(lib.bts_pack_weights_blocks(r.row[6], r.row[7])) == r.blocks, r
    whole = [r.case for r in PC.records() if r.floats % PC.BLOCK == 0]       # entries that end on a block edge
    assert {"dense48x36k1_fwd", "dense48x36k1_dgrad", "dense64x128k1_fwd", "dense64x128k1_dgrad", "bundle128g2_fwd"} <= set(whole)


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("native")])
def test_the_gather_statement_is_the_three_loops(name):
    c = PC.BY_NAME[name]
    w = PC.weight(c.shape)
    for row in PC.table_rows(c):
        a, b = PC.dense_statement(w, row), PC.dense_statement_loops(w, row)
        assert a.dtype == np.float32 and a.shape == (row[6], row[7])
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
        mask = PC.real_mask(row)
        assert not a.view(np.int32)[~mask].any()                              # +0.0 bits everywhere else


@pytest.mark.parametrize("name", NAMES)
def test_statement_agrees_with_the_torch_packers(name):
    c = PC.BY_NAME[name]
    w = PC.weight(c.shape)
    got = PC.case_statement(name)
    if c.mode == PC.FWD_NATIVE:
        want = ops.pack_grouped_native(w, c.groups)
    elif c.mode == PC.DGRAD_NATIVE:
        want = ops.pack_grouped_native(ops.grouped_dgrad_weight(w, c.groups), c.groups)
    elif c.groups == 1:
        src = w if c.mode == PC.FWD else w.flip(2, 3).transpose(0, 1)
        want = ops.pack_conv_weight(src, c_in_ld=c.c_in_ld)[0]
    else:
        want = ops.pack_grouped_conv_weight(w if c.mode == PC.FWD else ops.grouped_dgrad_weight(w, c.groups), c.groups)[0]
    assert tuple(want.shape) == tuple(c.dst_shape)
    assert np.array_equal(got, _bits(want))


@pytest.mark.parametrize("name", NAMES)
def test_every_planted_bit_pattern_lands_on_a_real_element(name):
    c = PC.BY_NAME[name]
    w = PC.weight(c.shape)
    wbits = _bits(w).reshape(-1)
    pos = PC.special_positions(w.numel())
    assert len(set(pos)) == 4 and all(0 <= p < w.numel() for p in pos)
    got = PC.case_statement(name).reshape(-1)
    if c.mode in (PC.FWD, PC.DGRAD):
        real = np.concatenate([PC.real_mask(r).reshape(-1) for r in PC.table_rows(c)])
    else:                                                                     # native: same-group pairs, from the header's index
        idx = np.arange(144 * c.shape[0])
        lane, k, s = idx % 64, (idx // 64) % 16, idx // 9216
        real = (64 * s + lane) // c.shape[1] == (64 * s + 16 * (lane // 16) + k) // c.shape[1]
    assert real.shape == got.shape and int(real.sum()) == w.numel()          # every source element exactly once
    assert not got[~real].any()
    for p, (what, pattern) in zip(pos, PC.SPECIALS):
        b = np.uint32(pattern).astype(np.int32)
        assert wbits[p] == b and int((wbits == b).sum()) == 1, what
        at = np.flatnonzero(got == b)
        assert at.size == 1 and real[at[0]], (what, at)
    assert np.array_equal(np.sort(got[real]), np.sort(wbits))                 # a permutation of the source bits
    assert np.unique(wbits).size > 0.99 * wbits.size                          # mostly distinct: a swapped pair shows


def test_orders_and_subtables_have_the_edges():
    od = PC.orders()
    recs = od["listed"]
    assert od["reversed"] == recs[::-1] and sorted(od["interleaved"]) == sorted(recs)
    inter = od["interleaved"]
    ones = [i for i, r in enumerate(inter) if r.blocks == 1]
    assert len(ones) == 4
    for i in ones:
        assert 0 < i < len(inter) - 1 and inter[i - 1].blocks > 1 and inter[i + 1].blocks > 1
    assert any(r.blocks == 1 for r in inter[:2]) and PC.SUBTABLE_SIZES == (1, 2, 7, 8, 9)
    offs, total = PC.slab_layout(recs)
    assert all(o % 4 == 0 for o in offs) and total == sum(r.floats for r in recs) + PC.GUARD * (len(recs) + 1)
    table, blocks = PC.table_array(recs, [0x1000] * len(recs), [0x100000 + 4 * o for o in offs])
    assert table.shape == (len(recs), 14) and blocks == sum(r.blocks for r in recs)
    assert list(table[:, 11]) == list(np.cumsum([0] + [r.blocks for r in recs[:-1]]))


def test_wino_integer_design_is_exact_in_fp32():
    G = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])
    assert np.abs(G).sum(1).max() ** 2 * 8 <= 72                              # |U| <= 72, a multiple of 1/4: 9 bits
    assert (64, 64, 0, 32) in PC.WINO and len(PC.WINO) == 5
    for cop, ld, n_tail, c16 in PC.WINO:
        wp = PC.wino_integer_weight(cop, ld)
        assert wp.shape == (cop, PC.round_up(9 * ld, 32))
        real = wp[:, :9 * ld]
        assert set(real.unique().tolist()) == set(float(v) for v in range(-8, 9))
        assert not wp[:, 9 * ld:].any()
        assert int(_lib.load_real().bts_pack_wino_floats(cop, ld, n_tail, c16)) == 16 * (ld - (4 if n_tail else 0)) * (c16 or cop)
