"""Composite autograd nodes of the training graph (bts_amd/train.py: _ConvFn, _BnFn, _DenseBlockFn, _bottleneck, _run_children,
atrous_forward, _conv_elu's pattern) on the GPU against the fp64 torch.nn references of tests/train_node_cases.py: one
training step per case, and of every step the output, every input and parameter gradient, every running statistic and every
batch counter, per tensor as max-abs error over max-abs reference value.

Bars (train_node_cases.bar; none is taken from the code under test): forward 2e-5, running statistics 1e-5 and every
gradient 2e-4 -- what test_train_gpu.py::test_bn_train_forward_backward_vs_torch asks of one norm layer, the loosest
single-kernel bar on these paths -- reduc_train_ref.conv_bar for the gradients of the norm-free conv3_pattern, counters exact.
They hold for whole nodes because the seeds keep every ReLU input of the reference at least 32 fp32-deviations away from zero
(the kink rule, checked on the CPU by test_train_node_cases_host.py): no mask can flip, so the error is rounding only.
A skipped prefix term, a wrong statistics row, a stale weight pack or a missing ELU' is percent-level in some tensor."""
import copy
from collections import OrderedDict

import numpy as np
import pytest
import torch

import train_node_cases as T

from conftest import fp32_only

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _module(c, bn_eval=False, freeze=()):
    mod = copy.deepcopy(c.module).cuda().train()
    if bn_eval:
        T.set_bn_eval(mod)
    params = dict(mod.named_parameters())
    for n in freeze:
        params[n].requires_grad_(False)
    return mod


def _inputs(c, input_grad=True, x_layout="cl"):
    out = OrderedDict()
    for k, v in c.inputs.items():
        g = bool(input_grad and c.wants_grad[k])
        if x_layout == "slice":                 # a channel slice of a wider channels_last buffer, junk on both sides
            C = v.shape[1]
            wide = torch.full((v.shape[0], C + 8, v.shape[2], v.shape[3]), 7.0e4, device="cuda").contiguous(memory_format=CL)
            wide[:, 4:4 + C] = v.cuda()
            d = wide[:, 4:4 + C].detach()
            assert not d.is_contiguous() and not d.is_contiguous(memory_format=CL)
        elif x_layout == "nchw":
            d = v.cuda().contiguous()
        else:
            d = v.cuda().contiguous(memory_format=CL)
        out[k] = d.requires_grad_(g)
    return out


def _forward(c, mod, inp, batched=False, native=False):
    from bts_amd import ops, train
    if c.kind == "dense":
        y = train._dense_block(mod, inp["x"], batched)
        assert y is not None, "the fused node declined the block"
        return y
    if c.name in T.BOTTLENECK_CASES:
        return train._bottleneck(mod, inp["x"], "t", native)
    if c.kind == "module":
        return train._run_children(list(mod.named_children()), inp["x"])
    if c.kind == "atrous":
        return train.atrous_forward(mod, inp["x"])
    if c.kind == "daspp2":                      # the decoder's growth pattern (train._decoder_forward), two branches
        iconv4, concat4 = inp["iconv4"], inp["concat4"]
        d3 = train.atrous_forward(mod["d3"], iconv4)
        d6 = train.atrous_forward(mod["d6"], torch.cat([concat4, d3], 1))
        return torch.cat([iconv4, d3, d6], 1)
    if c.kind == "conv3":                       # iconv3 = _conv_elu(cat([x, skip1, depth_8x8[:, :, ::4, ::4]]))
        return train.conv2d(torch.cat([inp["a"], inp["b"], inp["d"][:, :, ::4, ::4]], 1), mod["conv"].weight, padding=1,
                            act=ops.ACT_ELU)
    if c.kind == "upconv_bn":
        return train._bn(train.upconv_forward(mod["up"], inp["x"], subpixel=False), mod["bn"])
    raise KeyError(c.kind)


def _step(c, mod, input_grad=True, x_layout="cl", gy_layout="cl", **how):
    """One forward + backward(gy) on the GPU, collected like train_node_cases.reference_step."""
    inp = _inputs(c, input_grad, x_layout)
    for p in mod.parameters():
        p.grad = None
    out = _forward(c, mod, inp, **how)
    gy = c.gy.cuda()
    out.backward(gy.contiguous() if gy_layout == "nchw" else gy.contiguous(memory_format=CL))
    torch.cuda.synchronize()
    res = OrderedDict(out=out.detach().cpu().numpy())
    for k, v in inp.items():
        if v.grad is not None:
            res["grad:" + k] = v.grad.cpu().numpy()
    for n, p in mod.named_parameters():
        if p.grad is not None:
            res["grad:" + n] = p.grad.cpu().numpy()
    for n, b in mod.named_buffers():
        res["buf:" + n] = b.detach().cpu().numpy()
    return res


def _mode(batched):
    return "batched wgrad" if batched else "per-layer wgrad"


# ------------------------------------------------------------------------------------------ A. dense block
@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
@pytest.mark.parametrize("name", T.DENSE_CASES)
def test_dense_block_step_vs_fp64(name, batched):
    from bts_amd import ops
    c = T.case(name)
    mod = _module(c)
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        got = _step(c, mod, batched=batched)
    finally:
        ops.set_trace(None)
    T.compare(name, got, T.reference(name), "%s, %s" % (name, _mode(batched)))
    C0 = c.inputs["x"].shape[1]
    assert np.array_equal(got["out"][:, :C0], c.inputs["x"].numpy())          # the prefix is the input itself
    kernels = [r[0] for r in tr.records]        # the mode asked for is the mode that ran
    one, many = kernels.count("conv_wgrad_kernel"), kernels.count("conv_wgrad_batch_kernel")
    assert (one, many) == ((0, 1) if batched else (2 * len(mod), 0)), (one, many)


@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
@pytest.mark.parametrize("mask", ["x_no_grad", "frozen"])
@pytest.mark.parametrize("name", T.DENSE_CASES)
def test_dense_block_need_masks_vs_fp64(name, mask, batched):
    """A frozen tensor gets no gradient (T.compare wants the reference's key set, which has none for it) and everything
    else still meets its bar."""
    c = T.case(name)
    if mask == "x_no_grad":
        got = _step(c, _module(c), input_grad=False, batched=batched)
        ref = T.reference(name, input_grad=False)
        assert "grad:x" not in got
    else:
        freeze = T.dense_freeze_set(name)
        got = _step(c, _module(c, freeze=freeze), batched=batched)
        ref = T.reference(name, freeze=freeze)
        assert not any("grad:" + n in got for n in freeze)
    T.compare(name, got, ref, "%s, %s, %s" % (name, mask, _mode(batched)))


@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
@pytest.mark.parametrize("x_layout,gy_layout", [("slice", "cl"), ("nchw", "nchw"), ("cl", "nchw")])
def test_dense_block_layouts_vs_fp64(x_layout, gy_layout, batched):
    c = T.case("d121")
    got = _step(c, _module(c), x_layout=x_layout, gy_layout=gy_layout, batched=batched)
    T.compare("d121", got, T.reference("d121"), "d121, x %s, gy %s, %s" % (x_layout, gy_layout, _mode(batched)))


@pytest.mark.parametrize("batched", [False, True], ids=["per_layer", "batched"])
def test_dense_block_second_step_vs_fp64(batched):
    """Step, rewrite every parameter in place, begin_step(), step again: the second step's gradients, the running statistics
    after two momentum updates and the counters against the fp64 twin that took the same two steps.  A weight pack or a
    statistic left over from step one fails here."""
    from bts_amd import train
    c = T.case("d121")
    ref1, ref2 = T.reference_two_steps("d121")
    mod = _module(c)
    T.compare("d121", _step(c, mod, batched=batched), ref1, "d121, step 1, %s" % _mode(batched))
    T.set_parameters(mod, c.step2_values())
    train.begin_step()
    T.compare("d121", _step(c, mod, batched=batched), ref2, "d121, step 2, %s" % _mode(batched))


# ------------------------------------------------------------------------------------------ B. bottleneck
def _grouped_launches(summ):
    fwd, wgrad = {}, {}
    for kern, d in summ.items():
        if kern.startswith("conv_grouped_wgrad_kernel"):
            wgrad.update({tag: v["launches"] for tag, v in d["tags"].items()})
        elif kern.startswith("conv_grouped_kernel"):
            fwd.update({tag: v["launches"] for tag, v in d["tags"].items()})
    return fwd, wgrad


@pytest.mark.parametrize("native", [False, pytest.param(True, marks=fp32_only)], ids=["bundles", "grouped_native"])
@pytest.mark.parametrize("name", T.BOTTLENECK_CASES)
def test_bottleneck_step_vs_fp64(name, native):
    """Both settings of ``grouped_native`` against fp64; the launch trace says which form each pass of the 3x3 took: rx_id
    (stride 1, 4 channels per group) runs natively in all three passes when asked, the strided rx_ds and the ungrouped rn_ds
    never do."""
    from bts_amd import ops
    c = T.case(name)
    mod = _module(c)
    tr = ops.KernelTrace()
    ops.set_trace(tr)
    try:
        got = _step(c, mod, native=native)
    finally:
        ops.set_trace(None)
    T.compare(name, got, T.reference(name), "%s, grouped_native %s" % (name, native))
    fwd, wgrad = _grouped_launches(tr.summary())
    if native and name == "rx_id":
        assert fwd == {"t.fwd": 1, "t.dgrad": 1} and wgrad == {"t.wgrad": 1}, (fwd, wgrad)
    else:
        assert not fwd and not wgrad, (fwd, wgrad)


# ------------------------------------------------------------------------------------------ C. encoder glue, D. decoder nodes
@pytest.mark.parametrize("name", T.CHILDREN_CASES + ["atrous_bn", "atrous_nobn", "daspp2", "conv3_pattern", "upconv_elu_bn"])
def test_node_step_vs_fp64(name):
    c = T.case(name)
    got = _step(c, _module(c))
    T.compare(name, got, T.reference(name), name)
    if name == "stem":
        assert "grad:x" not in got
    if name == "conv3_pattern":                 # the gradient of d lands on the strided positions and is zero elsewhere
        on = np.zeros(got["grad:d"].shape, dtype=bool)
        on[:, :, ::4, ::4] = True
        assert (got["grad:d"][~on] == 0).all()


@pytest.mark.parametrize("name", T.BN_EVAL_CASES)
def test_node_step_with_frozen_norm_layers_vs_fp64(name):
    """Norm layers in eval mode inside a train()-mode module (train._bn's ATen branch): running statistics normalise, the
    buffers stay as they were, the gradients still meet the bars."""
    c = T.case(name)
    mod = _module(c, bn_eval=True)
    before = {n: b.clone() for n, b in mod.named_buffers()}
    got = _step(c, mod)
    T.compare(name, got, T.reference(name, bn_eval=True), name + ", norm layers frozen")
    for n, b in mod.named_buffers():
        assert torch.equal(b, before[n]), n
