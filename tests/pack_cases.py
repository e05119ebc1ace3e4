"""Shared cases of the weight-pack tests (csrc/pack.hip: pack_weights_kernel; csrc/optim.hip: the TILE records' re-pack):
the shapes, the values, the table rows as include/bts_hip.h words them, and plain NumPy statements of every layout.
Nothing here calls a packer of bts_amd.ops, so the statements are independent of the code they judge; the one exception
is the native grouped form (gmode 3 / 4), whose statement is the existing index-by-index
ops.pack_grouped_train_reference.

Packs are data movement: every comparison downstream is bit equality on int32 views, and padding is +0.0 bits."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

FWD, DGRAD, FWD_NATIVE, DGRAD_NATIVE = 0, 1, 2, 3      # train.WeightPacker's modes
BLOCK = 4096                                           # floats one workgroup of pack_weights_kernel writes
POISON = 0x7FA5A5A5                                    # destination prefill: a NaN with a recognisable payload
FENCE = 0x4B7FACED                                     # sentinel floats between two regions of a slab
GUARD = 64                                             # floats of fence on either side of a region (keeps 16-byte lines)

# bit patterns a copy must carry over unchanged, planted at fixed flat positions of every weight
SPECIALS = (("-0.0", 0x80000000), ("denormal", 0x00000123), ("inf", 0x7F800000), ("nan+payload", 0x7FC12345))


def round_up(a, b):
    return (a + b - 1) // b * b


def special_positions(numel):
    return (0, numel // 3, numel // 2 + 1, numel - 1)


# ---------------------------------------------------------------------------------------------------- the case table
# dense: (c_out, c_in, k, forward c_in_ld or None = round_up(c_in, 4), forward dst, input-gradient dst, why)
Dense = namedtuple("Dense", "c_out c_in k fwd_ld fwd_dst dgrad_dst why")
DENSE = [
    Dense(33, 5, 3, 8, (64, 96), (32, 352), "ragged rows, c_in_ld > inner, K pad, flip with k = 3"),
    Dense(48, 36, 1, None, (64, 64), (64, 64), "entry ends on a block edge"),
    Dense(64, 128, 1, None, (64, 128), (128, 64), "the same, two blocks"),
    Dense(96, 3, 7, None, (96, 224), (32, 4704), "stem: 49 taps, flip with k = 7, 1 and 3 real inner channels"),
    Dense(32, 32, 3, None, (32, 288), (32, 288), "no padding anywhere"),
    Dense(1, 8, 1, None, (32, 32), (32, 32), "one real row or one real inner channel"),
]
# blocks of 4096 floats each destination above takes (forward, input gradient): the entry's last block is partial
# unless the figure is whole
DENSE_BLOCKS = [(1.5, 2.75), (1.0, 1.0), (2.0, 2.0), (5.25, 36.75), (2.25, 2.25), (0.25, 0.25)]
LARGEST_DST = 150528

# block-diagonal bundles (gmode 1 / 2): (c, groups), k = 3, c_in_ld = cb = max(32, c / groups)
BUNDLES = [(128, 32), (64, 8), (128, 8), (64, 2), (128, 2)]
# native grouped form (gmode 3 / 4): (c, channels per group)
NATIVE = [(64, 4), (64, 8), (128, 16)]

Case = namedtuple("Case", "name shape groups mode c_in_ld dst_shape")


def _cases():
    out = []
    for d in DENSE:
        shape = (d.c_out, d.c_in, d.k, d.k)
        name = "dense%dx%dk%d" % (d.c_out, d.c_in, d.k)
        out.append(Case(name + "_fwd", shape, 1, FWD, d.fwd_ld or round_up(d.c_in, 4), d.fwd_dst))
        out.append(Case(name + "_dgrad", shape, 1, DGRAD, round_up(d.c_out, 4), d.dgrad_dst))
    for c, groups in BUNDLES:
        cg = c // groups
        cb = max(32, cg)
        for mode, tag in ((FWD, "fwd"), (DGRAD, "dgrad")):
            out.append(Case("bundle%dg%d_%s" % (c, groups, tag), (c, cg, 3, 3), groups, mode, cb, (c // cb, cb, 9 * cb)))
    for c, cg in NATIVE:
        for mode, tag in ((FWD_NATIVE, "fwd"), (DGRAD_NATIVE, "dgrad")):
            out.append(Case("native%dcg%d_%s" % (c, cg, tag), (c, cg, 3, 3), c // cg, mode, 0, (144 * c,)))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


@lru_cache(maxsize=None)
def weight(shape):
    """The OIHW values of a case (both modes of a shape share them; never modified): distinct-looking random normals with
    the special bit patterns planted."""
    g = torch.Generator().manual_seed(1000003 * shape[0] + 1009 * shape[1] + shape[2])
    w = torch.randn(shape, generator=g)
    bits = w.view(-1).view(torch.int32).numpy()
    for pos, (_, pattern) in zip(special_positions(w.numel()), SPECIALS):
        bits[pos] = np.uint32(pattern).astype(np.int32)
    return w


# ---------------------------------------------------------------------------------------------------- the table rows
def table_rows(case):
    """The 13-field rows (src offset, dst offset, rows, inner, k, c_in_ld, rows_pad, k_pad, s_row, s_c, flip, cg, gmode) of
    one case as include/bts_hip.h describes the two layouts: one row for a dense weight, one per bundle for a grouped
    one (src at the bundle's first output channel, dst at the bundle's [cb][k_pad] matrix), one for a native form."""
    c_out, c_in_g, k, _ = case.shape
    kk = k * k
    if case.mode in (FWD_NATIVE, DGRAD_NATIVE):
        return [(0, 0, 144, 0, 3, 0, 144, c_out, 0, 0, 0, c_in_g, 3 if case.mode == FWD_NATIVE else 4)]
    fwd = case.mode == FWD
    s_row, s_c, flip = (c_in_g * kk, kk, 0) if fwd else (kk, c_in_g * kk, 1)
    ld = case.c_in_ld
    if case.groups == 1:
        rows, inner = (c_out, c_in_g) if fwd else (c_in_g, c_out)
        return [(0, 0, rows, inner, k, ld, round_up(rows, 32), round_up(kk * ld, 32), s_row, s_c, flip, 0, 0)]
    cb = ld
    return [(j * cb * c_in_g * kk, j * cb * kk * cb, cb, cb, k, cb, cb, kk * cb, s_row, s_c, flip, c_in_g, 1 if fwd else 2)
            for j in range(c_out // cb)]


def dense_row(shape, mode, c_in_ld):
    """The one row of a dense OIHW weight `shape` packed with `c_in_ld` (what the AdamW tests need)."""
    return table_rows(Case("", tuple(shape), 1, mode, c_in_ld, None))[0]


# ---------------------------------------------------------------------------------------------------- the statements
def _flat_bits(w):
    """The weight's floats as a flat int32 NumPy array (a view where possible): bits, not values, are moved below."""
    if isinstance(w, torch.Tensor):
        w = w.detach().cpu().contiguous().view(-1).view(torch.int32).numpy()
    else:
        w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1).view(np.int32)
    return w


def _index(row):
    """(source index, is-copied) of every (packed row, tap, inner channel) of one table row, each [rows][k*k][inner]:
    dst[row][tap*c_in_ld + c] = src[row*s_row + c*s_c + (flip ? k*k-1-tap : tap)]; a bundle copies only where row and c
    lie in one group, with the bundle-local index taken off the inner channel (gmode 1) or off the row (gmode 2)."""
    so, do, rows, inner, k, ld, rows_pad, k_pad, s_row, s_c, flip, cg, gmode = row
    kk = k * k
    r = np.arange(rows, dtype=np.int64)[:, None, None]
    tap = np.arange(kk, dtype=np.int64)[None, :, None]
    c = np.arange(inner, dtype=np.int64)[None, None, :]
    t = kk - 1 - tap if flip else tap
    if gmode == 0:
        return so + r * s_row + c * s_c + t, np.ones((rows, kk, inner), dtype=bool)
    assert gmode in (1, 2)
    same = np.broadcast_to((r // cg) == (c // cg), (rows, kk, inner))
    g0 = (r // cg) * cg
    rr, cc = (r, c - g0) if gmode == 1 else (r - g0, c)
    return so + rr * s_row + cc * s_c + t, same


def real_mask(row):
    """[rows_pad][k_pad] bool: the elements that are a copy of a source element (everything else must be +0.0)."""
    so, do, rows, inner, k, ld, rows_pad, k_pad = row[:8]
    m = np.zeros((rows_pad, k_pad), dtype=bool)
    m[:rows, :k * k * ld].reshape(rows, k * k, ld)[:, :, :inner] = _index(row)[1]
    return m


def dense_statement(w, row):
    """[rows_pad][k_pad] float32 of one dense or bundle row (gmode 0, 1, 2) from the whole OIHW weight `w`, written from
    the sentence in include/bts_hip.h: index arithmetic and one gather, bits untouched."""
    so, do, rows, inner, k, ld, rows_pad, k_pad = row[:8]
    src = _flat_bits(w)
    idx, copied = _index(row)
    assert k * k * ld <= k_pad and inner <= ld and rows <= rows_pad
    assert int(idx[copied].min()) >= 0 and int(idx[copied].max()) < src.size
    out = np.zeros((rows_pad, k_pad), dtype=np.int32)                       # +0.0 bits
    out[:rows, :k * k * ld].reshape(rows, k * k, ld)[:, :, :inner] = np.where(copied, src[np.where(copied, idx, 0)], 0)
    return out.view(np.float32)


def dense_statement_loops(w, row):
    """The same statement as three Python loops, element by element (the host tests hold the two against each other on
    every case; too slow for whole-model weights)."""
    so, do, rows, inner, k, ld, rows_pad, k_pad, s_row, s_c, flip, cg, gmode = row
    src = _flat_bits(w)[so:]
    kk = k * k
    out = np.zeros((rows_pad, k_pad), dtype=np.int32)
    for r in range(rows):
        for tap in range(kk):
            t = kk - 1 - tap if flip else tap
            for c in range(inner):
                if gmode == 0:
                    out[r, tap * ld + c] = src[r * s_row + c * s_c + t]
                elif r // cg == c // cg:
                    g0 = (r // cg) * cg
                    if gmode == 1:
                        out[r, tap * ld + c] = src[r * s_row + (c - g0) * s_c + t]
                    else:
                        out[r, tap * ld + c] = src[(r - g0) * s_row + c * s_c + t]
    return out.view(np.float32)


def statement(w, rows, dst_shape, groups=1):
    """The whole destination of one weight (every row of it) as int32 bits in `dst_shape`."""
    if rows[0][12] >= 3:
        from bts_amd import ops
        wt = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.asarray(w, dtype=np.float32))
        ref = ops.pack_grouped_train_reference(wt.detach().cpu(), groups, dgrad=rows[0][12] == 4)
        return ref.contiguous().view(torch.int32).numpy().reshape(dst_shape)
    return np.stack([dense_statement(w, r).view(np.int32) for r in rows]).reshape(dst_shape)


@lru_cache(maxsize=None)
def case_statement(name):
    """int32 bits of a case's destination from its own `weight` (computed once, shared, never modified)."""
    c = BY_NAME[name]
    out = statement(weight(c.shape), table_rows(c), c.dst_shape, c.groups)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- records and orders
Record = namedtuple("Record", "case index row floats blocks")       # one table record: bundle `index` of `case`


def records():
    """Every table record of every case, as listed: dense both ways, every bundle of every grouped weight both ways, the
    native forms."""
    out = []
    for c in CASES:
        for j, row in enumerate(table_rows(c)):
            floats = row[6] * row[7]
            out.append(Record(c.name, j, row, floats, -(-floats // BLOCK)))
    return out


def record_statement(rec):
    """int32 bits, flat, of one record's destination region."""
    c = BY_NAME[rec.case]
    full = case_statement(rec.case)
    return (full[rec.index] if c.groups > 1 and c.mode in (FWD, DGRAD) else full).reshape(-1)


def orders():
    """The three record orders of the one-table test: as listed, reversed, and interleaved so that every one-block
    record sits between two multi-block ones."""
    recs = records()
    one = [r for r in recs if r.blocks == 1]
    many = [r for r in recs if r.blocks > 1]
    inter = []
    for i, m in enumerate(many):
        inter.append(m)
        if i < len(one):
            inter.append(one[i])
    assert len(one) < len(many)
    return {"listed": recs, "reversed": recs[::-1], "interleaved": inter}


SUBTABLE_SIZES = (1, 2, 7, 8, 9)            # both sides of a power of two for bts_table_find's binary search


def slab_layout(recs):
    """(float offset of each record's region, slab floats): regions in order, GUARD fence floats before, between and after."""
    offs, cur = [], GUARD
    for r in recs:
        offs.append(cur)
        cur += r.floats + GUARD
    return offs, cur


def table_array(recs, src_ptrs, dst_ptrs):
    """[n][14] int64 as train.WeightPacker._table_for builds it; src_ptrs[i] = address of record i's whole weight,
    dst_ptrs[i] = address of record i's own region.  Returns (table, total blocks)."""
    table, first = [], 0
    for r, src, dst in zip(recs, src_ptrs, dst_ptrs):
        so, do, rows, inner, k, ld, rows_pad, k_pad, s_row, s_c, flip, cg, gmode = r.row
        table.append([src + 4 * so, dst, rows, inner, k, ld, rows_pad, k_pad, s_row, s_c, flip, first, cg, gmode])
        first += r.blocks
    return np.asarray(table, dtype=np.int64), first


# ---------------------------------------------------------------------------------------------------- Winograd on integers
# (c_out_pad, c_in_ld, n_tail, c_out16): the four geometries of test_pack_wino_weight_kernel_matches_the_torch_statement
# and one with two chunks and two channel tiles in the 16-wide form
WINO = [(64, 64, 0, 0), (96, 192, 0, 48), (128, 228, 1, 0), (64, 36, 4, 0), (64, 64, 0, 32)]


def wino_integer_weight(c_out_pad, c_in_ld):
    """A packed 3x3 weight [c_out_pad][round_up(9 c_in_ld, 32)] of integers in [-8, 8] (every one of them somewhere): U = G g G^T
    is then a multiple of 1/4 of magnitude <= 72, exact in fp32 in any summation order."""
    g = torch.Generator().manual_seed(7 * c_out_pad + c_in_ld)
    wp = torch.zeros((c_out_pad, round_up(9 * c_in_ld, 32)))
    wp[:, :9 * c_in_ld] = torch.randint(-8, 9, (c_out_pad, 9 * c_in_ld), generator=g).float()
    return wp
