"""Host side of the frozen-statistics norm layers: the C ABI rows and prototypes, every rejection of the two entry points and
the two wrappers before anything is launched, the exactness claims of tests/bn_frozen_cases.py re-derived in fp32 on the
CPU, and the kink rule (tests/train_node_cases.py) for every seed the frozen-norm node tests use."""
import ctypes
import os
import re

import pytest
import torch

import bn_frozen_cases as fc
import stream_cases as sc
import train_node_cases as T
from bts_amd import _lib, ops, train
from bts_amd._lib import BtsHipError

HEADER = os.path.join(sc.ROOT, "include", "bts_hip.h")
INVALID = -1
NAMES = {"bts_bn_frozen_vectors_f32": 11, "bts_bn_frozen_bwd_f32": 19}        # arguments, the stream included


def header_text():
    with open(HEADER) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------ ABI
def test_abi_version_is_still_17():
    assert re.search(r"#define BTS_HIP_ABI_VERSION (\d+)", header_text()).group(1) == "17"
    assert _lib.ABI_VERSION == 17
    assert _lib.load_real().bts_hip_abi_version() == 17


@pytest.mark.parametrize("name", sorted(NAMES))
def test_prototype_and_abi_row_agree(name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header_text())
    assert m, "%s: no prototype in the header" % name
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == NAMES[name] and args[-1] == "bts_stream_t stream"
    e = _lib.ABI[name]
    assert e.role == _lib.LAUNCH and e.plan is None and e.restype is ctypes.c_int
    assert len(e.argtypes) == NAMES[name] and name in _lib.SYMBOLS
    for a, t in zip(args, e.argtypes):
        want = (ctypes.c_void_p if "*" in a or a.startswith("bts_stream_t") else ctypes.c_long if a.startswith("long ")
                else ctypes.c_float if a.startswith("float ") else ctypes.c_int)
        assert t is want, (name, a, t)
    assert hasattr(_lib.load_real(), name)


def test_error_code_of_a_bad_argument():
    assert re.search(r"#define BTS_ERR_INVALID\s+\((-?\d+)\)", header_text()).group(1) == str(INVALID)


# ------------------------------------------------------------------------- entry points: rejected before any GPU work
P = 0x10000          # a 16-byte aligned non-NULL address that a rejected call never dereferences


def vectors_args(**kw):
    a = dict(gamma=P, beta=P, rm=P, rv=P, eps=1e-5, C=8, mean=P, invstd=P + 64, scale=P + 128, shift=P + 192)
    a.update(kw)
    return [a[k] for k in ("gamma", "beta", "rm", "rv", "eps", "C", "mean", "invstd", "scale", "shift")] + [None]


@pytest.mark.parametrize("bad", [dict(C=0), dict(C=-4), dict(C=6), dict(C=9), dict(rm=None), dict(rv=None), dict(mean=None),
                                 dict(invstd=None), dict(scale=None), dict(shift=None), dict(mean=P + 4), dict(invstd=P + 8),
                                 dict(scale=P + 12), dict(shift=P + 20)], ids=str)
def test_vectors_entry_point_rejects(bad):
    assert _lib.load_real().bts_bn_frozen_vectors_f32(*vectors_args(**bad)) == INVALID


def bwd_args(**kw):
    a = dict(x=P, xs=16, dy=P, dys=16, npix=64, C=8, mean=P, invstd=P, scale=P, shift=P, relu=1, ws=P, ws_floats=1 << 20,
             dgamma=P, dbeta=P, dx=P, dxs=16, accumulate=0)
    a.update(kw)
    return [a[k] for k in ("x", "xs", "dy", "dys", "npix", "C", "mean", "invstd", "scale", "shift", "relu", "ws", "ws_floats",
                           "dgamma", "dbeta", "dx", "dxs", "accumulate")] + [None]


BWD_BAD = [dict(C=6), dict(C=0), dict(npix=0), dict(xs=4), dict(dys=4), dict(dxs=4), dict(xs=18), dict(dys=18), dict(dxs=18),
           dict(x=None), dict(dy=None), dict(x=P + 4), dict(dy=P + 8), dict(dx=P + 4),
           dict(mean=None), dict(invstd=None), dict(scale=None), dict(shift=None),
           dict(mean=P + 4), dict(invstd=P + 4), dict(scale=P + 4), dict(shift=P + 4),
           dict(dgamma=None), dict(dbeta=None),                              # one of the pair without the other
           dict(dgamma=P + 4), dict(dbeta=P + 4),
           dict(dgamma=None, dbeta=None, dx=None),                           # nothing to compute
           dict(ws=None), dict(ws_floats=2 * 8 - 1),                         # 64 x 8: one chunk, 2 * C floats of partials
           dict(dx=None, ws_floats=0)]


@pytest.mark.parametrize("bad", BWD_BAD, ids=str)
def test_backward_entry_point_rejects(bad):
    assert _lib.load_real().bts_bn_frozen_bwd_f32(*bwd_args(**bad)) == INVALID


def test_backward_workspace_demand_is_the_chunk_plan():
    """The sums need 2 * C floats per chunk of the plan bts_bn_train_ws_floats reports (3 * C per chunk): one float less is
    rejected for every test shape.  Without sums no workspace is asked for -- that call is not made here (it would launch)."""
    lib = _lib.load_real()
    for (npix, C), chunks in sc.BN_SHAPES:
        assert lib.bts_bn_train_ws_floats(npix, C) == 3 * C * chunks
        a = bwd_args(npix=npix, C=C, xs=C, dys=C, dxs=C, ws_floats=2 * C * chunks - 1)
        assert lib.bts_bn_frozen_bwd_f32(*a) == INVALID


# ----------------------------------------------------------------------------- wrappers: rejected before any launch
class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the wrappers' own argument checks run."""
    @staticmethod
    def make(t):
        return t.as_subclass(_FakeCuda)

    @property
    def is_cuda(self):
        return True


@pytest.fixture
def no_enqueue(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a rejected call reached the launch")
    monkeypatch.setattr(ops, "_enqueue", boom)


def test_wrappers_refuse_cpu_tensors(no_enqueue):
    v = torch.zeros(8)
    with pytest.raises(BtsHipError):
        ops.bn_frozen_vectors(8, v, v, v, v, 1e-5)
    x = torch.zeros(64, 8)
    with pytest.raises(BtsHipError):
        ops.bn_frozen_backward(x, x, 8, v, v, v, v, True, torch.zeros(1024), x.clone())


def test_vectors_wrapper_argument_checks(no_enqueue):
    f = _FakeCuda.make
    v = f(torch.zeros(8))
    slab = f(torch.zeros(8, 16))
    bad = [
        dict(C=6), dict(C=0), dict(C=12),                                          # C % 4, C <= 0, vectors shorter than C
        dict(running_mean=f(torch.zeros(4))), dict(running_var=f(torch.zeros(16))[::2]), dict(gamma=f(torch.zeros(4))),
        dict(beta=f(torch.zeros(8, dtype=torch.float64))), dict(running_mean=None), dict(running_var=torch.zeros(8)),
        dict(out=slab[0:4, 1:9]),                                                  # rows not 16-byte aligned
        dict(out=slab[0:3, :8]), dict(out=slab[0:4, :4]), dict(out=f(torch.zeros(4, 16))[:, ::2]),
        dict(out=f(torch.zeros(4, 10))[:, :8]),                                    # row stride not a multiple of 4
        dict(out=torch.zeros(4, 8)),
    ]
    for kw in bad:
        a = dict(C=8, gamma=v, beta=v, running_mean=v, running_var=v, eps=1e-5)
        a.update(kw)
        with pytest.raises(BtsHipError):
            ops.bn_frozen_vectors(**a)


def test_backward_wrapper_argument_checks(no_enqueue):
    f = _FakeCuda.make
    npix, C = 64, 8
    wide = f(torch.zeros(npix, 24))
    x, dy, dx = wide[:, 4:12], f(torch.zeros(npix, C)), wide[:, 12:20]
    v = f(torch.zeros(C))
    ws = f(torch.zeros(ops.bn_train_ws_floats(npix, C)))
    bad = [
        dict(C=6), dict(C=12), dict(C=0),
        dict(x2d=wide[:, 1:9]),                                                    # rows not 16-byte aligned
        dict(x2d=f(torch.zeros(npix, 10))[:, :8]),                                 # stride not a multiple of 4
        dict(dy2d=dy[:-1]), dict(dy2d=dy[:, :4]), dict(dy2d=f(torch.zeros(npix, 16))[:, ::2]), dict(dy2d=torch.zeros(npix, C)),
        dict(dx2d=wide[:-1, 12:20]), dict(dx2d=wide[:, 12:16]), dict(dx2d=wide[:, 13:21]),
        dict(mean=f(torch.zeros(12))[1:9]), dict(invstd=f(torch.zeros(4))), dict(scale=f(torch.zeros(16))[::2]),
        dict(shift=f(torch.zeros(12))[1:9]),                                       # misaligned / short / strided vectors
        dict(ws=None), dict(ws=ws[:-1]), dict(ws=torch.zeros(ws.numel())),         # sums asked: ws missing, too small, CPU
        dict(sums=False, dx2d=None),                                               # nothing to compute
        dict(dx2d=None, accumulate=True),
        dict(out=f(torch.zeros(2, 16))[:, 1:9]), dict(out=f(torch.zeros(3, 8))), dict(sums=False, out=f(torch.zeros(2, 8))),
    ]
    for kw in bad:
        a = dict(x2d=x, dy2d=dy, C=C, mean=v, invstd=v, scale=v, shift=v, relu=True, ws=ws, dx2d=dx)
        a.update(kw)
        with pytest.raises(BtsHipError):
            ops.bn_frozen_backward(**a)


# ------------------------------------------------------------------------------------------------ the case module
@pytest.mark.parametrize("shape", [(2, 4), (129, 44), (1537, 132), (12, 2208), (98304, 8)])
def test_backward_design_is_exact_in_fp32(shape):
    """What lets dx be compared bit for bit and the sums with torch.equal: the pre-activation, scale * dy', dx_old + scale * dy'
    and every term of both sums are exact in fp32, every partial sum stays below 2^24 quarters (exact in any order), and the kink
    z == 0 occurs -- the mask `z > 0` is exercised at the value where `>=` would differ."""
    x, dy, mean, invstd, scale, shift, dx_old = fc.frozen_bwd_case(*shape)
    for relu in (False, True):
        r = fc.frozen_bwd_ref(x, dy, mean, invstd, scale, shift, dx_old, relu)
        z32 = x * scale + shift
        assert torch.equal(z32.double(), r["z"]) and torch.equal(torch.addcmul(shift, x, scale).double(), r["z"])
        assert shape[0] * shape[1] < 1000 or bool((r["z"] == 0).any())
        g32 = torch.where(z32 > 0, dy, torch.zeros_like(dy)) if relu else dy
        assert torch.equal(g32.double(), r["g"])
        assert torch.equal((scale * g32).double(), r["dx"])
        assert torch.equal((dx_old + scale * g32).double(), r["dx_acc"])
        assert torch.equal(torch.addcmul(dx_old, g32, scale.expand_as(g32)).double(), r["dx_acc"])
        xhat32 = (x - mean) * invstd
        assert torch.equal(xhat32.double(), r["xhat"]) and torch.equal((g32 * xhat32).double(), r["g"] * r["xhat"])
        for terms in (r["g"], r["g"] * r["xhat"]):
            assert torch.equal(terms * 4, torch.round(terms * 4))
            assert float(terms.abs().sum(0).max()) * 4 < 2 ** 24
        assert torch.equal(g32.sum(0).double(), r["dbeta"]) and torch.equal((g32 * xhat32).sum(0).double(), r["dgamma"])
    assert dx_old.min() >= -8 and dx_old.max() <= 8 and torch.equal(dx_old, dx_old.round())
    assert bool((dx_old != dy).any())


def test_backward_shapes_cover_every_kernel_and_walk():
    lanes = {sc.lanes_for(C) for _, C in fc.BWD_SHAPES}
    assert lanes == {8, 16, 32}
    chunks = dict(sc.BN_SHAPES)
    assert {1, 2, 1024} <= set(chunks.values()) and (2, 4) in chunks
    # a partial last channel group for each lane width
    assert any(C % (4 * sc.lanes_for(C)) for _, C in fc.BWD_SHAPES if sc.lanes_for(C) == 8)
    assert any(C % (4 * sc.lanes_for(C)) for _, C in fc.BWD_SHAPES if sc.lanes_for(C) == 16)
    assert any(C % (4 * sc.lanes_for(C)) for _, C in fc.BWD_SHAPES if sc.lanes_for(C) == 32)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("C", fc.VEC_C)
def test_vectors_bounds_hold_for_the_fp32_statement(C, affine):
    """The counted bounds are bounds: the same formulas evaluated in fp32 on the CPU (torch rounds each operation, no
    contraction) stay within them -- and they are tight enough to mean something (under 1e-6 relative)."""
    gamma, beta, rm, rv = fc.frozen_vectors_case(C)
    assert float(rv[1]) == 0.0 and float(rv[2]) == float(torch.tensor(1e-12))
    if not affine:
        gamma = beta = None
    for eps in fc.VEC_EPS:
        ref, bound = fc.frozen_vectors_ref(gamma, beta, rm, rv, eps)
        invstd = 1.0 / torch.sqrt(rv + eps)
        g = torch.ones(C) if gamma is None else gamma
        b = torch.zeros(C) if beta is None else beta
        got = dict(mean=rm, invstd=invstd, scale=g * invstd, shift=b - rm * g * invstd)
        for k in ref:
            assert bool(((got[k].double() - ref[k]).abs() <= bound[k]).all()), k
        assert float((bound["invstd"] / ref["invstd"].abs()).max()) < 1e-6
        assert float((bound["scale"] / ref["scale"].abs()).max()) < 1e-6


# --------------------------------------------------------------------------------------------------- kink rule
def test_frozen_seed_table_is_the_issue_s():
    assert fc.FROZEN_SEEDS["d161"] == T.SEEDS["d161"] and fc.FROZEN_SEEDS["d121_tiny"] == T.SEEDS["d121_tiny"]
    assert set(fc.FROZEN_SEEDS) == set(fc.FROZEN_RATIOS)
    for n in T.BN_EVAL_CASES:
        assert n not in fc.FROZEN_SEEDS                 # those keep their stored seeds (train_node_cases.SEED_RATIOS)


@pytest.mark.parametrize("name", sorted(fc.FROZEN_SEEDS))
def test_kink_rule_with_frozen_norms(name):
    m, d, n = T.kink(T.Case(name, fc.FROZEN_SEEDS[name]), bn_eval=True)
    print("%s seed %d: m %.3e d %.3e ratio %.1f (recorded %.1f)" % (name, fc.FROZEN_SEEDS[name], m, d, m / d, fc.FROZEN_RATIOS[name]))
    assert n > 0 and m >= T.KINK_RATIO * d


def test_kink_rule_second_step_and_mixed_block():
    c = T.Case("d121", fc.FROZEN_SEEDS["d121"])
    m, d, _ = T.kink(c, bn_eval=True, step2_seed=fc.FROZEN_STEP2_SEED["d121"], second_step=True)
    assert m >= T.KINK_RATIO * d, m / d
    m, d, n = fc.kink_mixed(T.Case("d121", fc.MIXED_SEED["d121"]))
    assert n > 0 and m >= T.KINK_RATIO * d, m / d


# ------------------------------------------------------------------------------------------------------ switches
def test_model_switch_defaults_off_and_forwards():
    from bts_amd import bts as M
    from parity_util import Params
    m = M.BtsModel(Params("densenet121_bts", 512, 10.0, "nyu"))
    assert m.native_frozen_norm is False and m.encoder.native_frozen_norm is False and m.decoder.native_frozen_norm is False
    m.native_frozen_norm = True
    assert m.native_frozen_norm is True and m.encoder.native_frozen_norm is True and m.decoder.native_frozen_norm is True
    m.native_frozen_norm = 0
    assert m.native_frozen_norm is False


def test_scope_is_thread_local_and_nests():
    import threading
    assert train.current_frozen_norm() is False
    seen = []
    with train.frozen_norm_scope(True):
        assert train.current_frozen_norm() is True
        t = threading.Thread(target=lambda: seen.append(train.current_frozen_norm()))
        t.start()
        t.join()
        with train.frozen_norm_scope(False):
            assert train.current_frozen_norm() is False
        assert train.current_frozen_norm() is True
    assert train.current_frozen_norm() is False and seen == [False]
