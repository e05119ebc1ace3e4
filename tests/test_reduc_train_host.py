"""Host side of the fused reduction training path (no GPU): the transposed weight pack, the column tables of the
backward kernel's row buffers, the new C entry point and ABI version, and the bts_size 256 fallback."""
import ctypes
import os
import re

import pytest
import torch

from bts_amd import _lib, ops, train
from parity_util import CONFIGS, Params
from bts_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(c_in, c_first, k, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(co if co > 0 else (3 if k else 1), ci, 1, 1, generator=gen) for ci, co in ops.reduc_chain(c_in, c_first)]


@pytest.mark.parametrize("chain", ops.REDUC_TRAIN_CHAINS, ids=lambda c: "x".join(map(str, c)))
def test_transposed_pack_round_trips(chain):
    """Unpacking pack_reduc_weights_bwd gives W_l^T in reverse layer order, the last layer zero-padded to 8 columns."""
    c_in, c_first, k = chain
    ws = _weights(c_in, c_first, k)
    frag = ops.pack_reduc_weights_bwd(ws)
    shapes = [(wt.shape[1], max(8, wt.shape[0])) for wt in reversed(ws)]
    mats = ops.unpack_reduc_weights(frag, shapes)
    assert len(mats) == len(ws)
    for m, wt in zip(mats, reversed(ws)):
        cout, cin = wt.shape[0], wt.shape[1]
        assert torch.equal(m[:, :cout], wt.view(cout, cin).t())
        assert (m[:, cout:] == 0).all()
    # the forward pack in the same (wide) order round-trips too, and the one-gather form equals the three packers
    fwd = ops.unpack_reduc_weights(ops.pack_reduc_weights(ws, wide=True), [(wt.shape[0], wt.shape[1]) for wt in ws])
    for m, wt in zip(fwd, ws):
        assert torch.equal(m, wt.view(wt.shape[0], wt.shape[1]))
    a, b, c = ops.reduc_train_packs(ws)
    assert torch.equal(a, ops.pack_reduc_weights(ws)) and torch.equal(b, ops.pack_reduc_weights(ws, wide=True)) and torch.equal(c, frag)
    assert all(t.data_ptr() % 16 == 0 for t in (a, b, c))


# include/bts_hip.h, bts_reduc_bwd_f32: (first column, width) per layer and YC
HEADER_TABLES = {
    (128, 128): ([(0, 128), (128, 64), (192, 32), (224, 16), (240, 8), (248, 4)], 248),
    (128, 64): ([(0, 64), (64, 32), (96, 16), (112, 8), (120, 4)], 120),
    (64, 32): ([(0, 32), (32, 16), (48, 8), (56, 4)], 56),
    (32, 16): ([(0, 16), (16, 8), (24, 4)], 24),
}


@pytest.mark.parametrize("chain", ops.REDUC_TRAIN_CHAINS, ids=lambda c: "x".join(map(str, c)))
def test_column_tables_match_chain(chain):
    c_in, c_first, _ = chain
    cols, yc = ops.reduc_train_cols(c_in, c_first)
    layers = ops.reduc_chain(c_in, c_first)
    assert len(cols) == len(layers)
    col = 0
    for (first, width), (_, cout) in zip(cols, layers):
        assert first == col and width == (cout if cout > 0 else 4)
        col += width
    assert yc == sum(co for _, co in layers if co > 0) == col - 4
    assert (cols, yc) == HEADER_TABLES[(c_in, c_first)]
    assert all(first % 4 == 0 and width % 4 == 0 for first, width in cols)      # float4 rows, wgrad's channel rule


def test_library_exports_reduc_bwd_and_abi_17():
    hdr = open(os.path.join(ROOT, "include", "bts_hip.h")).read()
    assert "bts_reduc_bwd_f32" in _lib.ABI
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "bts_reduc_bwd_f32") and hasattr(lib, "bts_reduc_bwd_max_waves")
    lib.bts_hip_abi_version.restype = ctypes.c_int
    assert lib.bts_hip_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define BTS_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 17
    assert "int bts_reduc_bwd_f32(" in hdr
    # a chain the library does not build is refused before anything is launched
    loaded = _lib.load_real()
    assert loaded.bts_reduc_bwd_max_waves(64, 64, 8) == -2
    assert loaded.bts_reduc_bwd_max_waves(64, 32, 2) > 0
    one = ctypes.c_void_p(1 << 20)
    rc = loaded.bts_reduc_bwd_f32(one, 64, 1, 4, 4, 64, 64, one, 16, one, 16, 80.0, 8, one, one, 64, one, one, None)
    assert rc == -2


def _decoder(bts_size):
    from bts_amd import bts as M
    enc, md, ds, _, _ = CONFIGS["K"]
    return M.bts(Params(enc, bts_size, md, ds), synth.ENCODER_CHANNELS[enc], bts_size)


def test_bts_size_256_selects_the_fallback():
    dec = _decoder(256)
    dec.fused_reduction_train = True
    scales = ((dec.reduc8x8, 8), (dec.reduc4x4, 4), (dec.reduc2x2, 2), (dec.reduc1x1, 0))
    assert not any(train.fused_reduction_available(m, k) for m, k in scales)
    dec = _decoder(512)
    assert dec.fused_reduction_train is False                 # the default path is the layer-by-layer graph
    scales = ((dec.reduc8x8, 8), (dec.reduc4x4, 4), (dec.reduc2x2, 2), (dec.reduc1x1, 0))
    assert all(train.fused_reduction_available(m, k) for m, k in scales)
    assert not train.fused_reduction_available(dec.reduc8x8, 4)
