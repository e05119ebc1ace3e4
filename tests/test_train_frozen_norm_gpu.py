"""Norm layers with frozen statistics (eval() mode inside a train()-mode module: set_misc(bn_no_track_stats=True)) on the HIP
kernels -- train.frozen_norm_scope / BtsModel.native_frozen_norm: _FrozenBnFn behind train._bn, and _DenseBlockFn keeping
blocks that hold such layers.

Node tests: the cases of tests/train_node_cases.py with every norm layer frozen (seeds: bn_frozen_cases.FROZEN_SEEDS, kink
rule re-checked on the CPU by tests/test_bn_frozen_host.py) against the fp64 twin set up the same way, at train_node_cases'
bars (forward 2e-5, gradients 2e-4; none from the code under test).  Buffers and counters must keep their bits.
Whole-model tests: one silog step with the switch on against the same model with the switch off.

The GPU step runner (_module, _step, _mode) is tests/test_train_nodes_gpu.py's own, imported under its private names so that
both files run a case through exactly the same code."""
import copy
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import bn_frozen_cases as fc
import train_node_cases as T
from bts_amd import ops, synth, train
from conftest import fp32_only
from parity_util import Params, assert_grads_close, grad_error_report, t
from test_train_nodes_gpu import _mode, _module, _step

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def frozen_case(name):
    return T.Case(name, fc.FROZEN_SEEDS[name]) if name in fc.FROZEN_SEEDS else T.case(name)


@functools.lru_cache(maxsize=None)
def frozen_ref(name, freeze=(), input_grad=True):
    """fp64 step of the case with every norm layer frozen; computed once, shared, read-only."""
    c = frozen_case(name)
    return T.reference_step(c, T.twin(c, torch.float64, True, freeze), input_grad)


class traced:
    """KernelTrace around a block, plus a spy on ops.bn_frozen_backward: ``calls`` = [(C, sums, accumulate, dx given)]."""

    def __enter__(self):
        self.trace, self.calls = ops.KernelTrace(), []
        self._orig = ops.bn_frozen_backward
        me = self

        def spy(x2d, dy2d, C, mean, invstd, scale, shift, relu, ws, dx2d, sums=True, accumulate=False, out=None):
            me.calls.append((C, bool(sums), bool(accumulate), dx2d is not None))
            return me._orig(x2d, dy2d, C, mean, invstd, scale, shift, relu, ws, dx2d, sums=sums, accumulate=accumulate, out=out)

        ops.bn_frozen_backward = spy
        ops.set_trace(self.trace)
        return self

    def __exit__(self, *exc):
        ops.set_trace(None)
        ops.bn_frozen_backward = self._orig
        return False

    @property
    def kernels(self):
        return [r[0] for r in self.trace.records]


def step_on(c, mod, **kw):
    with train.frozen_norm_scope(True):
        return _step(c, mod, **kw)


def buffers_of(mod):
    return {n: b.detach().clone() for n, b in mod.named_buffers()}


def assert_buffers_kept(mod, before, only=None):
    for n, b in mod.named_buffers():
        if only is None or only(n):
            assert torch.equal(b, before[n]) and b.dtype == before[n].dtype, "%s moved" % n


class no_aten_batch_norm:
    """While active, torch.nn.functional.batch_norm raises: no norm layer of the step inside can reach ATen.  (The fp64
    references are torch.nn modules and are computed outside.)"""

    def __enter__(self):
        self._orig = torch.nn.functional.batch_norm

        def boom(*a, **k):
            raise AssertionError("a norm layer reached torch.nn.functional.batch_norm")
        torch.nn.functional.batch_norm = boom
        return self

    def __exit__(self, *exc):
        torch.nn.functional.batch_norm = self._orig
        return False


# ------------------------------------------------------------------------------------------ dense blocks
@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
@pytest.mark.parametrize("name", T.DENSE_CASES)
def test_frozen_dense_block_step_vs_fp64(name, batched):
    c = frozen_case(name)
    ref = frozen_ref(name)
    mod = _module(c, bn_eval=True)
    before = buffers_of(mod)
    with traced() as tr, no_aten_batch_norm():
        got = step_on(c, mod, batched=batched)           # _forward asserts that the node is _DenseBlockFn (y is not None)
    T.compare(name, got, ref, "%s frozen, %s" % (name, _mode(batched)))
    assert_buffers_kept(mod, before)
    k = tr.kernels
    L = len(mod)
    assert k.count("bn_frozen_bwd_kernel") == 2 * L and k.count("bn_frozen_vectors_kernel") == 2 * L
    assert "bn_stats_kernel" not in k and "bn_bwd_kernels" not in k
    assert (k.count("conv_wgrad_kernel"), k.count("conv_wgrad_batch_kernel")) == ((0, 1) if batched else (2 * L, 0))
    # backward walks the layers in reverse: norm2 (dx written), then norm1 (added onto the prefix gradient), all with sums
    assert [(s, a) for _, s, a, _ in tr.calls] == [(True, False), (True, True)] * L


@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
@pytest.mark.parametrize("mask", ["x_no_grad", "frozen"])
@pytest.mark.parametrize("name", T.DENSE_CASES)
def test_frozen_dense_block_need_masks_vs_fp64(name, mask, batched):
    """A frozen gamma / beta pair gets no gradient and no sums pass: its launch is the dx-only form (2 flops and 12 bytes per
    element in the trace)."""
    c = frozen_case(name)
    L = len(c.module)
    if mask == "x_no_grad":
        with traced() as tr:
            got = step_on(c, _module(c, bn_eval=True), input_grad=False, batched=batched)
        ref = frozen_ref(name, (), False)
        assert "grad:x" not in got
        assert [(s, a) for _, s, a, _ in tr.calls] == [(True, False), (True, True)] * L
    else:
        freeze = T.dense_freeze_set(name)
        with traced() as tr:
            got = step_on(c, _module(c, bn_eval=True, freeze=freeze), batched=batched)
        ref = frozen_ref(name, freeze)
        assert not any("grad:" + n in got for n in freeze)
        want = [(True, False), (True, True)] * L
        want[2 * (L - 1)] = (False, False)                 # denselayer1.norm2: the second call from the end
        assert [(s, a) for _, s, a, _ in tr.calls] == want
        recs = [r for r in tr.trace.records if r[0] == "bn_frozen_bwd_kernel"]
        npix = c.inputs["x"].shape[0] * c.inputs["x"].shape[2] * c.inputs["x"].shape[3]
        mid = c.module["denselayer1"].conv1.out_channels
        dx_only = [r for r in recs if r[2] == 2.0 * npix * mid and r[3] == 12.0 * npix * mid]
        assert len(dx_only) == 1 and recs.index(dx_only[0]) == 2 * (L - 1)
    T.compare(name, got, ref, "%s frozen, %s, %s" % (name, mask, _mode(batched)))


@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
def test_mixed_dense_block_vs_fp64(batched):
    """denselayer1's norm layers frozen, the others in train() mode: the live layers' running statistics and counters move as
    the fp64 twin's do (T.compare holds them to its bars, counters exactly), the frozen layer's keep their bits."""
    c = T.Case("d121", fc.MIXED_SEED["d121"])
    ref = T.reference_step(c, fc.set_mixed(T.twin(c, torch.float64)))
    mod = fc.set_mixed(_module(c))
    before = buffers_of(mod)
    with traced() as tr:
        got = step_on(c, mod, batched=batched)
    T.compare("d121", got, ref, "d121 mixed, %s" % _mode(batched))
    assert_buffers_kept(mod, before, only=lambda n: n.startswith("denselayer1."))
    for n, b in mod.named_buffers():
        if not n.startswith("denselayer1."):
            assert not torch.equal(b, before[n]), "%s did not move" % n
    k = tr.kernels
    L = len(mod)
    assert k.count("bn_frozen_bwd_kernel") == 2 and k.count("bn_frozen_vectors_kernel") == 2
    assert k.count("bn_stats_kernel") == 2 * (L - 1) and k.count("bn_bwd_kernels") == 2 * (L - 1)


@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
@pytest.mark.parametrize("x_layout,gy_layout", [("slice", "cl"), ("nchw", "nchw"), ("cl", "nchw")])
def test_frozen_dense_block_layouts_vs_fp64(x_layout, gy_layout, batched):
    c = frozen_case("d121")
    got = step_on(c, _module(c, bn_eval=True), x_layout=x_layout, gy_layout=gy_layout, batched=batched)
    T.compare("d121", got, frozen_ref("d121"), "d121 frozen, x %s, gy %s, %s" % (x_layout, gy_layout, _mode(batched)))


@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
def test_frozen_dense_block_second_step_vs_fp64(batched):
    """Step, rewrite every parameter in place, begin_step(), step again: the vectors of step two come from the new gamma /
    beta (and the unchanged buffers), the weight packs from the new weights."""
    c = frozen_case("d121")
    values = c.step2_values(fc.FROZEN_STEP2_SEED["d121"])
    twin = T.twin(c, torch.float64, True)
    ref1 = T.reference_step(c, twin)
    T.set_parameters(twin, values)
    ref2 = T.reference_step(c, twin)
    mod = _module(c, bn_eval=True)
    before = buffers_of(mod)
    T.compare("d121", step_on(c, mod, batched=batched), ref1, "d121 frozen, step 1, %s" % _mode(batched))
    T.set_parameters(mod, values)
    train.begin_step()
    T.compare("d121", step_on(c, mod, batched=batched), ref2, "d121 frozen, step 2, %s" % _mode(batched))
    assert_buffers_kept(mod, before)


@fp32_only
def test_frozen_batched_dense_block_has_the_bits_of_the_unbatched_bf16_block():
    """Under precision_scope("bf16") the frozen block composes as the batch-statistic one does
    (test_train_bf16_nodes_gpu.py): at 234 pixels neither weight-gradient planner splits, so batched == unbatched, bit for bit."""
    from test_train_bf16_nodes_gpu import _block_case
    block, x, gy = _block_case()

    def run(batched):
        m = copy.deepcopy(block).cuda().train()
        T.set_bn_eval(m)
        xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        with traced() as tr, train.precision_scope("bf16"), train.frozen_norm_scope(True):
            y = train._dense_block(m, xg, batched_wgrad=batched)
            assert y is not None
            y.backward(gy.cuda())
            torch.cuda.synchronize()
        return y.detach(), xg.grad, {n: p.grad for n, p in m.named_parameters()}, tr.kernels

    y, dx, g, k = run(False)
    yb, dxb, gb, kb = run(True)
    assert k.count("conv_wgrad_kernel<bf16>") == 4 and kb.count("conv_wgrad_batch_kernel<bf16>") == 1
    assert k.count("bn_frozen_bwd_kernel") == 4 == kb.count("bn_frozen_bwd_kernel") and "bn_stats_kernel" not in k + kb
    assert torch.equal(yb, y) and torch.equal(dxb, dx) and set(g) == set(gb)
    bad = [n for n in g if not torch.equal(gb[n], g[n])]
    assert not bad, bad


# ------------------------------------------------------------------------------------------ every other node
NODE_CASES = T.BOTTLENECK_CASES + T.CHILDREN_CASES + ["atrous_bn", "daspp2", "upconv_elu_bn"]


@pytest.mark.parametrize("name", NODE_CASES)
def test_frozen_node_step_vs_fp64(name):
    c = frozen_case(name)
    ref = frozen_ref(name)
    mod = _module(c, bn_eval=True)
    before = buffers_of(mod)
    with traced() as tr, no_aten_batch_norm():
        got = step_on(c, mod)
    T.compare(name, got, ref, name + ", norm layers frozen, switch on")
    assert_buffers_kept(mod, before)
    n_bn = sum(isinstance(m, torch.nn.BatchNorm2d) for m in mod.modules())
    k = tr.kernels
    assert k.count("bn_frozen_vectors_kernel") == n_bn and k.count("bn_frozen_bwd_kernel") == n_bn
    assert "bn_stats_kernel" not in k and "bn_bwd_kernels" not in k
    if name == "stem":
        assert "grad:x" not in got


def test_frozen_norm_need_masks():
    """_FrozenBnFn: gamma / beta frozen -> the dx-only launch; the input without a gradient as well -> no launch at all."""
    name = "transition_even"
    c = frozen_case(name)
    freeze = ("norm.weight", "norm.bias")
    with traced() as tr, no_aten_batch_norm():
        got = step_on(c, _module(c, bn_eval=True, freeze=freeze))
    assert tr.calls == [(96, False, False, True)]
    T.compare(name, got, frozen_ref(name, freeze), name + ", frozen affine")
    with traced() as tr, no_aten_batch_norm():
        got = step_on(c, _module(c, bn_eval=True, freeze=freeze), input_grad=False)
    assert tr.calls == [] and "bn_frozen_bwd_kernel" not in tr.kernels
    T.compare(name, got, frozen_ref(name, freeze, False), name + ", frozen affine, no input gradient")
    with traced() as tr, no_aten_batch_norm():                                         # sums only
        got = step_on(c, _module(c, bn_eval=True), input_grad=False)
    assert tr.calls == [(96, True, False, False)]
    T.compare(name, got, frozen_ref(name, (), False), name + ", no input gradient")


def test_switch_off_keeps_todays_paths(monkeypatch):
    c = frozen_case("d121")
    mod = _module(c, bn_eval=True)
    x = c.inputs["x"].cuda().contiguous(memory_format=torch.channels_last)
    assert train.current_frozen_norm() is False
    assert train._dense_block(mod, x, False) is None and train._dense_block(mod, x, True) is None
    with train.frozen_norm_scope(True):
        assert train._dense_block(mod, x, False) is not None

    class Reached(Exception):
        pass

    def boom(*a, **k):
        raise Reached()
    monkeypatch.setattr(torch.nn.functional, "batch_norm", boom)
    with pytest.raises(Reached):
        train._bn(x, mod["denselayer1"].norm1, relu=True)


# ------------------------------------------------------------------------------------------ whole models
def _model_step(encoder, native, monkeypatch):
    from bts_amd import bts as M, trainer
    B, H, W = 1, 64, 96
    torch.manual_seed(31)
    m = M.BtsModel(Params(encoder, 512, 80.0, "kitti")).train()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():                          # buffers off their defaults, mildly: no norm layer renormalises in this mode
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.num_features, generator=gen))
                mod.running_var.copy_(0.8 + 0.4 * torch.rand(mod.num_features, generator=gen))
                mod.num_batches_tracked.fill_(3)
    m = m.cuda()
    trainer.set_misc(m, encoder, bn_no_track_stats=True)
    assert not any(mod.training for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    assert m.native_frozen_norm is False
    m.native_frozen_norm = native
    x = torch.from_numpy(synth.image_batch(B, H, W, 3)).cuda()
    focal = torch.from_numpy(synth.focal_values(B, "kitti", 3)).cuda()
    gt, mask = synth.train_targets(B, H, W, 80.0, 4)
    before = {n: b.detach().clone() for n, b in m.named_buffers()}
    if native:
        def boom(*a, **k):
            raise AssertionError("a norm layer reached torch.nn.functional.batch_norm")
        monkeypatch.setattr(torch.nn.functional, "batch_norm", boom)
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        outs = m(x, focal)
        loss = M.silog_loss(0.85)(outs[4], t(gt).cuda(), t(mask).cuda())
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_trace(None)
        monkeypatch.undo()
    for n, b in m.named_buffers():
        assert torch.equal(b, before[n]), "%s moved" % n
    # every trainable parameter the forward uses (torchvision's ResNet carries its unused classifier `fc` along)
    unused = [n for n, p in m.named_parameters() if p.requires_grad and p.grad is None]
    assert all(".fc." in n for n in unused), unused
    assert not (unused and encoder.startswith("densenet")), unused      # DenseNet has no such passenger: nothing may be missing
    grads = OrderedDict((n, p.grad.cpu().numpy()) for n, p in m.named_parameters() if p.requires_grad and p.grad is not None)
    assert grads
    return [o.detach().cpu().numpy() for o in outs], grads, [r[0] for r in tr.records]


@pytest.mark.parametrize("encoder", ["densenet121_bts", "resnet50_bts"])
def test_whole_model_step_switch_on_vs_off(encoder, monkeypatch):
    outs_off, g_off, k_off = _model_step(encoder, False, monkeypatch)
    outs_on, g_on, k_on = _model_step(encoder, True, monkeypatch)
    assert "bn_frozen_bwd_kernel" not in k_off and "bn_frozen_vectors_kernel" not in k_off
    assert "bn_frozen_bwd_kernel" in k_on and "bn_stats_kernel" not in k_on and "bn_bwd_kernels" not in k_on
    assert len(outs_on) == len(outs_off) == 6
    for i, (a, b) in enumerate(zip(outs_on, outs_off)):
        err = T.rel_error(a, b)
        print("%s output %d: switch on vs off %.2e" % (encoder, i, err))
        assert np.isfinite(a).all() and err <= 2e-5, (encoder, i, err)
    assert set(g_on) == set(g_off)
    for n, g in g_on.items():
        assert np.isfinite(g).all(), n
    per, l2 = grad_error_report(g_on, g_off)
    print("%s gradients, switch on vs off (%d tensors): global rel-L2 %.2e, worst tensor %.2e" % (encoder, len(per), l2, max(per.values())))
    assert_grads_close(per, l2, "%s: native frozen norm vs ATen" % encoder)
