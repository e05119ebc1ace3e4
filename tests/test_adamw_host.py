"""CPU: host side of the native AdamW step (csrc/optim.hip, bts_amd/optim.py) -- the plan query of the C ABI (host only,
no device), NativeAdamW's state_dict compatibility with torch.optim.AdamW, the trainer's flags and the packer's
``versions_trusted`` default."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import adamw_cases as AC
from bts_amd import _lib

BTS_ERR_INVALID = -1
NAMES = ("bts_adamw_table_bytes", "bts_adamw_flat_span", "bts_adamw_plan_f32", "bts_adamw_step_f32")


def _span():
    return int(_lib.load_real().bts_adamw_flat_span())


def _dummy_ptrs(case_list, base=0x100000, shift=0):
    """Non-null, never dereferenced addresses: p / g / m / v 16-byte aligned (+ shift), destinations 16-byte aligned."""
    out, a = [], base
    for _, shape, modes in case_list:
        n = AC.round_up(int(np.prod(shape)) * 4, 256)
        four = [a + j * n + shift for j in range(4)]
        a += 4 * n
        dsts = []
        for mode in modes:
            _, _, _, rows_pad, k_pad = AC.pack_geometry(shape, mode)
            dsts.append(a)
            a += rows_pad * k_pad * 4
        out.append(tuple(four) + (dsts,))
    return out


def test_symbols_are_exported_declared_and_host_only_ones_bypass_the_recorder():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = C.CDLL(os.path.join(root, "bts_amd", "libbts_hip.so"))
    lib = _lib.load_real()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.ABI               # the prototypes themselves: test_host_logic's table-driven test
    assert C.sizeof(_lib.AdamwItem) == 112 and C.sizeof(_lib.AdamwPack) == 24 and C.sizeof(_lib.AdamwHyper) == 48
    assert _lib.AdamwItem.packs.offset == 64 and C.sizeof(_lib.AdamwPlanItem) == 24
    from bts_amd import plan

    class Rec:
        calls, foreign = [], []

    proxy = plan._Proxy(lib, Rec())
    for name in NAMES[:3]:
        assert getattr(proxy, name) is getattr(lib, name), "%s must not be recorded: it is a host-only query" % name
    assert lib.bts_hip_abi_version() == 17


def test_plan_kinds_blocks_and_prefix_sums():
    span = _span()
    assert span > 8 and span % 4 == 0
    lib = _lib.load_real()
    assert lib.bts_adamw_table_bytes(0) == 0 and lib.bts_adamw_table_bytes(3) == 3 * lib.bts_adamw_table_bytes(1) > 0
    case_list = AC.cases(span)
    hyper = [i % 2 for i in range(len(case_list))]
    items = AC.make_items(case_list, _dummy_ptrs(case_list), hyper)
    rc, total, got, table = AC.plan(items)
    assert rc == 0
    first = 0
    for (name, shape, modes), (kind, fb, nb) in zip(case_list, got):
        want_kind, want_nb = AC.expected_plan(shape, modes, span)
        assert (kind, nb) == (want_kind, want_nb), name
        assert fb == first, name
        first += nb
    assert total == first
    # both packs, forward only, input gradient only and none all occur; so do c_in_ld > c_in (33 -> 36) and 3 -> 4
    assert {m for _, _, m in case_list} == {(0, 1), (0,), (1,), ()}
    assert AC.pack_geometry((128, 33, 3, 3), AC.FWD)[2] == 36 and AC.pack_geometry((3, 8, 1, 1), AC.DGRAD)[2] == 4
    # the plan is a function of the shapes, not of the pointers (other addresses, another alignment) nor of the plan output
    items2 = AC.make_items(case_list, _dummy_ptrs(case_list, base=0x7f0000000000, shift=4), hyper)
    rc2, total2, got2, table2 = AC.plan(items2)
    assert (rc2, total2, got2) == (0, total, got)
    rc3, total3, _, table3 = AC.plan(items, want_plan=False)
    assert (rc3, total3) == (0, total) and np.array_equal(table, table3)
    assert not np.array_equal(table, table2)            # the table itself does carry the pointers
    # items follow their shapes whatever the order
    rev = list(reversed(range(len(case_list))))
    items4 = AC.make_items([case_list[i] for i in rev], [_dummy_ptrs(case_list)[i] for i in rev], [hyper[i] for i in rev])
    _, total4, got4, _ = AC.plan(items4)
    assert total4 == total and [(k, nb) for k, _, nb in got4] == [(got[i][0], got[i][2]) for i in rev]


def test_plan_of_nothing_is_valid():
    rc, total, got, _ = AC.plan(np.zeros(0, dtype=np.dtype(_lib.AdamwItem)))
    assert (rc, total, got) == (0, 0, [])
    assert _lib.load_real().bts_adamw_step_f32(None, 0, 0, None, 0, None, None) == 0       # n = 0 launches nothing


def _one(shape=(48, 36, 3, 3), modes=(0, 1), **edit):
    case = [("w", shape, modes)]
    items = AC.make_items(case, _dummy_ptrs(case), [0])
    for k, v in edit.items():
        if k.startswith("pack"):
            idx, field = int(k[4]), k[6:]
            items["packs"][field][0, idx] = v
        else:
            items[k][0] = v
    return items


BAD = {
    "null p": dict(p=0), "null g": dict(g=0), "null m": dict(m=0), "null v": dict(v=0),
    "numel 0": dict(numel=0), "numel < 0": dict(numel=-4),
    "product != numel": dict(numel=48 * 36 * 9 + 1), "product != numel (c_out)": dict(c_out=47),
    "ksize 5 with packs": dict(ksize=5, numel=48 * 36 * 25), "ksize 2 with packs": dict(ksize=2, numel=48 * 36 * 4),
    "3 packs": dict(n_packs=3), "negative packs": dict(n_packs=-1),
    "fwd c_in_ld < c_in": dict(pack0_c_in_ld=35), "dgrad c_in_ld < c_out": dict(pack1_c_in_ld=47),
    "fwd k_pad < 9 c_in_ld": dict(pack0_k_pad=9 * 36 - 1), "dgrad k_pad < 9 c_in_ld": dict(pack1_k_pad=9 * 48 - 4),
    "null dst": dict(pack1_dst=0), "dst not 16-byte aligned": dict(pack0_dst=0x200008), "dst 4 off": dict(pack1_dst=0x300004),
    "mode 2": dict(pack0_mode=2),
    "hyper 8": dict(hyper=8), "hyper -1": dict(hyper=-1),
    "p not 4-byte aligned": dict(p=0x100002),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_plan_rejects(name):
    rc, total, _, _ = AC.plan(_one(**BAD[name]))
    assert rc == BTS_ERR_INVALID, name


def test_plan_rejects_null_arrays_flat_geometry_and_block_overflow():
    lib = _lib.load_real()
    items = _one()
    total = C.c_long(0)
    table = np.zeros(int(lib.bts_adamw_table_bytes(1)), dtype=np.uint8)
    assert lib.bts_adamw_plan_f32(None, 1, table.ctypes.data, C.byref(total), None) == BTS_ERR_INVALID
    assert lib.bts_adamw_plan_f32(items.ctypes.data, 1, None, C.byref(total), None) == BTS_ERR_INVALID
    assert lib.bts_adamw_plan_f32(items.ctypes.data, 1, table.ctypes.data, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_plan_f32(items.ctypes.data, -1, table.ctypes.data, C.byref(total), None) == BTS_ERR_INVALID
    # the valid base case, a 7x7 weight without packs (flat) and with a wrong product
    assert AC.plan(_one())[0] == 0
    assert AC.plan(_one(shape=(96, 3, 7, 7), modes=()))[0] == 0
    assert AC.plan(_one(shape=(96, 3, 7, 7), modes=(), numel=96 * 3 * 49 - 1))[0] == BTS_ERR_INVALID
    # block count: 2^31 - 1 blocks fit the grid, one more does not (two flat items; nothing is dereferenced)
    span = _span()
    case = [("a", (7,), ()), ("b", (9,), ())]
    items = AC.make_items(case, _dummy_ptrs(case), [0, 1])
    items["numel"][0] = (2**31 - 2) * span
    items["numel"][1] = span
    rc, total, got, _ = AC.plan(items)
    assert (rc, total) == (0, 2**31 - 1) and got[1][1] == 2**31 - 2
    items["numel"][1] = span + 1
    assert AC.plan(items)[0] == BTS_ERR_INVALID


def test_launch_validates_before_any_hip_call():
    lib = _lib.load_real()
    hy = (_lib.AdamwHyper * 1)()
    hy[0].lr, hy[0].beta1, hy[0].beta2, hy[0].eps, hy[0].weight_decay, hy[0].step = 1e-4, 0.9, 0.999, 1e-3, 1e-2, 1.0
    A = 0x100000
    h = C.addressof(hy)
    assert lib.bts_adamw_step_f32(None, 1, 1, h, 1, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_step_f32(A + 8, 1, 1, h, 1, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_step_f32(A, -1, 1, h, 1, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_step_f32(A, 1, 0, h, 1, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_step_f32(A, 1, 2**31, h, 1, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_step_f32(A, 1, 1, None, 1, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_step_f32(A, 1, 1, h, 0, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_step_f32(A, 1, 1, h, 9, None, None) == BTS_ERR_INVALID
    assert lib.bts_adamw_step_f32(A, 1, 1, h, 1, A + 2, None) == BTS_ERR_INVALID
    hy[0].step = 0.0                                           # the bias corrections divide by 1 - beta^step
    assert lib.bts_adamw_step_f32(A, 1, 1, h, 1, None, None) == BTS_ERR_INVALID


# ------------------------------------------------------------------------------------------------- NativeAdamW on the CPU
def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5,), (4, 3, 3, 3), (7, 2, 1, 1), (1,))]


def _groups(ps):
    return [{"params": ps[:2], "weight_decay": 1e-2}, {"params": ps[2:], "weight_decay": 0}]


def _set_grads(ps, seed):
    g = torch.Generator().manual_seed(seed)
    for p in ps[:-1]:                                         # the last parameter never gets a gradient
        p.grad = torch.randn(p.shape, generator=g)


def _assert_same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (k, name)


def test_state_dicts_travel_between_torch_adamw_and_native_both_ways():
    from bts_amd.optim import NativeAdamW
    ps = _params()
    ref = torch.optim.AdamW(_groups(ps), lr=1e-4, eps=1e-3, foreach=False, fused=False)
    for s in (1, 2):
        _set_grads(ps, s)
        ref.step()
    sd = copy.deepcopy(ref.state_dict())
    assert len(sd["state"]) == 3
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    nat = NativeAdamW(_groups(ps2), lr=5e-2, eps=1e-8)
    assert nat.param_groups[0].keys() == ref.param_groups[0].keys()           # the same group keys before any load
    nat.load_state_dict(sd)
    out = nat.state_dict()
    _assert_same_state_dict(sd, out)
    assert all(st["step"].device.type == "cpu" and float(st["step"]) == 2.0 for st in nat.state.values())
    # and back: torch's AdamW takes the native optimiser's checkpoint and goes on exactly where the first one would
    ps3 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    back = torch.optim.AdamW(_groups(ps3), lr=3e-3, eps=1e-6, foreach=False, fused=False)
    back.load_state_dict(copy.deepcopy(out))
    _assert_same_state_dict(out, back.state_dict())
    _set_grads(ps, 3)
    _set_grads(ps3, 3)
    ref.step()
    back.step()
    for a, b in zip(ps, ps3):
        assert torch.equal(a, b)
    _assert_same_state_dict(ref.state_dict(), back.state_dict())


def test_native_step_on_cpu_parameters_raises_and_changes_nothing():
    from bts_amd._lib import BtsHipError
    from bts_amd.optim import NativeAdamW
    ps = _params()
    nat = NativeAdamW(_groups(ps), lr=1e-4, eps=1e-3)
    nat.step()                                                  # no gradients at all: nothing to do, nothing to refuse
    _set_grads(ps, 1)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(BtsHipError, match="no CPU fallback"):
        nat.step()
    assert all(torch.equal(a, b) for a, b in zip(before, ps)) and len(nat.state) == 0
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(fused=True), dict(capturable=True), dict(betas=(1.0, 0.9)), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            NativeAdamW(_groups(_params()), **kw)


# ------------------------------------------------------------------------------------------------------ trainer and packer
class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
        self.decoder = torch.nn.Conv2d(4, 1, 1)


def test_make_optimizer_native_has_the_reference_groups_and_refuses_fused():
    from bts_amd import trainer
    from bts_amd.optim import NativeAdamW
    m = _Model()
    with pytest.raises(ValueError):
        trainer.make_optimizer(m, native=True, fused=True)
    opt = trainer.make_optimizer(m, 2e-4, 3e-2, 1e-3, native=True)
    assert isinstance(opt, NativeAdamW)
    enc, dec = opt.param_groups                                   # bts_main.py:354-356: decay on the encoder only
    assert [id(p) for p in enc["params"]] == [id(p) for p in m.encoder.parameters()]
    assert [id(p) for p in dec["params"]] == [id(p) for p in m.decoder.parameters()]
    assert enc["weight_decay"] == 3e-2 and dec["weight_decay"] == 0
    assert enc["lr"] == dec["lr"] == 2e-4 and enc["eps"] == dec["eps"] == 1e-3 and enc["betas"] == (0.9, 0.999)
    ref = trainer.make_optimizer(m, 2e-4, 3e-2, 1e-3, fused=False)
    assert type(ref) is torch.optim.AdamW                         # the default is what it was
    assert [g["weight_decay"] for g in ref.param_groups] == [3e-2, 0]
    assert trainer.make_optimizer(m, native=True, fused=False).__class__ is NativeAdamW


def test_guard_nonfinite_needs_the_native_optimiser():
    from bts_amd import trainer
    m = _Model()
    opt = trainer.make_optimizer(m, fused=False)
    with pytest.raises(ValueError, match="guard_nonfinite"):
        trainer.train_step(m, opt, None, None, None, None, guard_nonfinite=True)


def test_packer_distrusts_versions_by_default_and_a_torch_step_restores_that(monkeypatch):
    from bts_amd import train, trainer
    assert train.WeightPacker().versions_trusted is False
    assert train._PACKER.versions_trusted is False
    seen = []
    monkeypatch.setattr(train._PACKER, "refresh", lambda force=False: seen.append(force))
    train.begin_step()
    assert seen == [True]                                         # the parent's behaviour: everything is re-packed
    monkeypatch.setattr(train._PACKER, "versions_trusted", True)  # what NativeAdamW.step leaves behind
    train.begin_step()
    assert seen == [True, False]
    m = _Model()
    opt = trainer.make_optimizer(m, fused=False)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()                                                    # whoever stepped last decides
    assert train._PACKER.versions_trusted is False
    train.begin_step()
    assert seen == [True, False, True]
