"""Shared cases of the native AdamW tests (csrc/optim.hip): the parameter shapes of one launch, the pack geometry the
training step's WeightPacker would give them, and the item array of bts_adamw_plan_f32."""
import numpy as np

from bts_amd import _lib

# (c_out, c_in, k): partial tiles both ways, one output channel, c_in below / above / across the 64- and 32-wide tiles
TILES = [(3, 8, 1), (1, 8, 1), (33, 65, 1), (48, 36, 3), (1, 32, 3), (128, 33, 3)]
FWD, DGRAD = 0, 1
VARIANTS = {"both": (FWD, DGRAD), "fwd": (FWD,), "dgrad": (DGRAD,), "none": ()}


def flat_numels(span):
    return [1, 3, 4, 5, span - 1, span, span + 1]


def cases(span):
    """[(name, shape, pack modes)]: every flat size, every tile shape with both packs, and each tile shape once more with
    one pack or none (none: a conv weight that is a FLAT record)."""
    out = [("flat%d" % n, (n,), ()) for n in flat_numels(span)]
    out += [("w%dx%dk%d_both" % t, (t[0], t[1], t[2], t[2]), VARIANTS["both"]) for t in TILES]
    for t, var in zip(TILES, ("fwd", "dgrad", "fwd", "none", "fwd", "dgrad")):
        out.append(("w%dx%dk%d_%s" % (t + (var,)), (t[0], t[1], t[2], t[2]), VARIANTS[var]))
    return out


def round_up(a, b):
    return (a + b - 1) // b * b


def pack_geometry(shape, mode):
    """(rows, inner, c_in_ld, rows_pad, k_pad) as train.WeightPacker lays a dense weight out: channels padded to 4 (33 -> 36,
    3 -> 4 and 1 -> 4 on the input-gradient side), rows and K padded to 32."""
    co, ci, k, _ = shape
    rows, inner = (co, ci) if mode == FWD else (ci, co)
    ld = round_up(inner, 4)
    return rows, inner, ld, round_up(rows, 32), round_up(k * k * ld, 32)


def expected_plan(shape, modes, span):
    """(kind, n_blocks) from the documented tiling: a flat block covers `span` floats; a tile is 32 x 32 channels x 9 taps
    for a 3x3 weight and 64 x 64 channels for a 1x1."""
    n = int(np.prod(shape))
    if not modes:
        return 0, -(-n // span)
    t = 32 if shape[2] == 3 else 64
    return 1, -(-shape[0] // t) * -(-shape[1] // t)


def make_items(case_list, ptrs, hyper):
    """ptrs[i] = (p, g, m, v, [dst per pack]) addresses; hyper[i] = hyper record index."""
    items = np.zeros(len(case_list), dtype=np.dtype(_lib.AdamwItem))
    for i, (_, shape, modes) in enumerate(case_list):
        p, g, m, v, dsts = ptrs[i]
        items["p"][i], items["g"][i], items["m"][i], items["v"][i] = p, g, m, v
        items["numel"][i] = int(np.prod(shape))
        items["hyper"][i] = hyper[i]
        if len(shape) == 4:
            items["c_out"][i], items["c_in"][i], items["ksize"][i] = shape[0], shape[1], shape[2]
        items["n_packs"][i] = len(modes)
        for k, mode in enumerate(modes):
            _, _, ld, _, k_pad = pack_geometry(shape, mode)
            items["packs"]["dst"][i, k] = dsts[k]
            items["packs"]["k_pad"][i, k] = k_pad
            items["packs"]["c_in_ld"][i, k] = ld
            items["packs"]["mode"][i, k] = mode
    return items


def plan(items, want_plan=True):
    """(rc, total_blocks, [(kind, first_block, n_blocks)], host table bytes)"""
    import ctypes as C
    lib = _lib.load_real()
    n = len(items)
    table = np.zeros(max(int(lib.bts_adamw_table_bytes(n)), 8), dtype=np.uint8)
    total = C.c_long(-7)
    out = (_lib.AdamwPlanItem * max(n, 1))()
    rc = lib.bts_adamw_plan_f32(items.ctypes.data if n else None, n, table.ctypes.data, C.byref(total),
                                C.addressof(out) if want_plan else None)
    return rc, total.value, [(out[i].kind, out[i].first_block, out[i].n_blocks) for i in range(n)], table
