"""CPU: host side of the native training losses (csrc/loss.hip) -- exported symbols, the workspace query, argument
validation of the C ABI (which happens before any HIP call, so it runs without a GPU), and the untouched torch path of
``silog_loss`` / ``depth_l1_loss``."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bts_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bts_depth_loss_ws_doubles", "bts_depth_loss_fwd_f32", "bts_depth_loss_bwd_f32")
BTS_ERR_INVALID = -1
A = 0x10000                # a dummy, 16-byte aligned, non-null "device address": never dereferenced, nothing is launched


def test_library_exports_and_binding_declares_the_loss_entry_points():
    raw = ctypes.CDLL(os.path.join(ROOT, "bts_amd", "libbts_hip.so"))
    from bts_amd import _lib
    lib = _lib.load_real()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.ABI               # the prototypes themselves: test_host_logic's table-driven test
    t = _lib.load_torch_ops()
    assert str(t.depth_loss.default._schema) == ("bts_hip::depth_loss(Tensor est, Tensor gt, Tensor? mask, float gt_min, int kind, "
                                                 "float param) -> (Tensor loss, Tensor stats)")
    assert str(t.depth_loss_backward.default._schema) == (
        "bts_hip::depth_loss_backward(Tensor est, Tensor gt, Tensor? mask, float gt_min, int kind, float param, Tensor stats, "
        "Tensor grad_loss) -> Tensor")


def test_workspace_query_is_positive_and_monotonic():
    from bts_amd import _lib
    q = _lib.load_real().bts_depth_loss_ws_doubles
    for n in (0, -1, -2**40):
        assert q(n) <= 0
    sizes = [1, 2, 63, 64, 255, 256, 1023, 4096, 4097, 2013, 33 * 61 * 2, 547503, 4 * 352 * 704, 2**24, 2**31 + 5, 2**40]
    vals = [q(n) for n in sorted(sizes)]
    assert all(v > 0 for v in vals), vals
    assert all(b >= a for a, b in zip(vals, vals[1:])), vals
    assert vals[-1] < 1 << 20            # bounded: the block count is capped


def _fwd(**kw):
    a = dict(est=A, gt=A, mask=None, gt_min=1.0, npix=1000, kind=0, param=0.85, ws=A, ws_doubles=None, stats=A, loss=A)
    a.update(kw)
    from bts_amd import _lib
    lib = _lib.load_real()
    if a["ws_doubles"] is None:
        a["ws_doubles"] = max(lib.bts_depth_loss_ws_doubles(a["npix"]), 0)
    return lib.bts_depth_loss_fwd_f32(a["est"], a["gt"], a["mask"], a["gt_min"], a["npix"], a["kind"], a["param"], a["ws"],
                                      a["ws_doubles"], a["stats"], a["loss"], None)


def _bwd(**kw):
    a = dict(est=A, gt=A, mask=None, gt_min=1.0, npix=1000, kind=0, param=0.85, stats=A, grad_loss=A, grad_est=A)
    a.update(kw)
    from bts_amd import _lib
    return _lib.load_real().bts_depth_loss_bwd_f32(a["est"], a["gt"], a["mask"], a["gt_min"], a["npix"], a["kind"], a["param"],
                                                   a["stats"], a["grad_loss"], a["grad_est"], None)


FWD_BAD = [dict(est=None), dict(gt=None), dict(ws=None), dict(stats=None), dict(loss=None), dict(npix=0), dict(npix=-5),
           dict(kind=2), dict(kind=-1), dict(ws_doubles=0), dict(npix=547503, ws_doubles=401), dict(ws=A + 4), dict(stats=A + 4),
           dict(est=A + 2), dict(gt=A + 1), dict(loss=A + 2)]
BWD_BAD = [dict(est=None), dict(gt=None), dict(stats=None), dict(grad_loss=None), dict(grad_est=None), dict(npix=0),
           dict(npix=-1), dict(kind=2), dict(kind=-1), dict(stats=A + 4), dict(est=A + 2), dict(gt=A + 3), dict(grad_est=A + 1)]


@pytest.mark.parametrize("bad", FWD_BAD, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_forward_rejects_invalid_arguments_before_any_launch(bad):
    assert _fwd(**bad) == BTS_ERR_INVALID


@pytest.mark.parametrize("bad", BWD_BAD, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_backward_rejects_invalid_arguments_before_any_launch(bad):
    assert _bwd(**bad) == BTS_ERR_INVALID


def _cpu_case():
    gt, mask = synth.train_targets(2, 9, 13, 80.0, seed=5)
    rng = np.random.Generator(np.random.PCG64(6))
    est = (gt * rng.uniform(0.5, 1.6, size=gt.shape)).astype(np.float32)
    return torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mask)


def test_default_criteria_are_todays_torch_formulas_on_cpu():
    from bts_amd import bts as M
    est, gt, mask = _cpu_case()
    crit = M.silog_loss(0.85)
    assert crit.native is False
    d = torch.log(est[mask]) - torch.log(gt[mask])
    want = torch.sqrt((d ** 2).mean() - 0.85 * (d.mean() ** 2)) * 10.0
    assert torch.equal(crit(est, gt, mask), want)
    l1 = M.depth_l1_loss(2.0)
    assert l1.native is False
    err = est[mask] - gt[mask]
    want = torch.where(err > 0, 2.0 * err, -err).sum() / err.numel()
    assert torch.equal(l1(est, gt, mask), want)
    assert torch.equal(M.depth_l1_loss(1)(est, gt, mask), err.abs().mean())


def test_native_criteria_refuse_cpu_tensors():
    from bts_amd import bts as M
    from bts_amd._lib import BtsHipError
    est, gt, mask = _cpu_case()
    with pytest.raises(BtsHipError):
        M.silog_loss(0.85, native=True)(est, gt, mask)
    with pytest.raises(BtsHipError):
        M.silog_loss(0.85, native=True)(est, gt, None, gt_min=1.0)
    with pytest.raises(BtsHipError):
        M.depth_l1_loss(2.0, native=True)(est, gt, mask)


def test_trainer_hands_the_validity_rule_to_a_native_criterion():
    """train_step with a native criterion and no mask builds no mask tensor: the criterion receives mask=None and the
    dataset's threshold.  With the torch criterion (or an explicit mask) the call is the one it always was."""
    from bts_amd import trainer

    class Opt:
        param_groups = []

        def zero_grad(self, set_to_none=True):
            pass

        def step(self):
            pass

    seen = []

    class Crit:
        def __init__(self, native):
            if native is not None:
                self.native = native

        def __call__(self, est, gt, mask, **kw):
            seen.append((mask, kw))
            return (est * 1.0).sum()

    w = torch.ones(1, requires_grad=True)
    model = lambda image, focal: [None] * 4 + [image * w, None]
    gt = torch.tensor([[0.5, 2.0, 0.05]])
    for native, dataset, mask, want_kw in ((True, "kitti", None, dict(gt_min=1.0)), (True, "nyu", None, dict(gt_min=0.1)),
                                           (True, "kitti", gt > 0, {}), (False, "kitti", None, {}), (None, "nyu", None, {})):
        seen.clear()
        trainer.train_step(model, Opt(), Crit(native), torch.ones(1, 3), None, gt, mask=mask, dataset=dataset)
        got_mask, kw = seen[0]
        assert kw == want_kw
        if want_kw:
            assert got_mask is None
        else:
            want = mask if mask is not None else gt > (1.0 if dataset == "kitti" else 0.1)
            assert got_mask.dtype == torch.bool and torch.equal(got_mask, want)
