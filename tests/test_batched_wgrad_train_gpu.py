"""The per-model switch ``batched_wgrad`` (BtsModel / encoder / bts): one multi-problem weight-gradient launch per DenseNet
block (train._DenseBlockFn defers the weight gradients to the end of its backward walk) and per fused reduction scale
(ops.reduc_train_backward), against the same model with the switch off.

With the switch on every launch but the weight gradients is issued as before -- same kernels, same order, same
operands -- so everything that is not a batched weight gradient must come out with the same bits; the batched weight
gradients sum the same products under another split of the pixel axis and are held to the bars of
tests/test_train_gpu.py::test_fused_dense_block_equals_layer_by_layer_graph."""
import copy
import functools
import re

import numpy as np
import pytest
import torch

import reduc_train_ref as R
from bts_amd import ops, synth
from parity_util import CONFIGS, TRAIN_CASE, Params, assert_grads_close, grad_error_report, make_inputs, t

pytestmark = pytest.mark.gpu

DENSE_CONV = re.compile(r"^encoder\.base_model\.denseblock\d+\.denselayer\d+\.conv[12]\.weight$")


@functools.lru_cache(maxsize=None)
def _base_model():
    from bts_amd import bts as M
    torch.manual_seed(77)
    return M.BtsModel(Params("densenet121_bts", 512, 80.0, "kitti")).train()


@functools.lru_cache(maxsize=None)
def _step(batched, frozen):
    """One training step of densenet121 at 2x64x96: (loss, {name: grad or None}, {name: running statistic}, frozen names)."""
    from bts_amd import bts as M, trainer
    B, H, W = 2, 64, 96
    x = torch.from_numpy(synth.image_batch(B, H, W, 3)).cuda()
    focal = torch.from_numpy(synth.focal_values(B, "kitti", 3)).cuda()
    gt, mask = synth.train_targets(B, H, W, 80.0, 4)
    m = copy.deepcopy(_base_model()).cuda()
    names = trainer.set_misc(m, "densenet121_bts", fix_first_conv_blocks=True) if frozen else []
    assert m.batched_wgrad is False and m.encoder.batched_wgrad is False and m.decoder.batched_wgrad is False
    m.batched_wgrad = batched
    loss = M.silog_loss(0.85)(m(x, focal)[4], t(gt).cuda(), t(mask).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return (loss.detach().cpu(), {n: None if p.grad is None else p.grad.cpu() for n, p in m.named_parameters()},
            {n: b.cpu() for n, b in m.named_buffers() if "running" in n}, tuple(names))


def _compare(frozen):
    loss_off, g_off, rs_off, _ = _step(False, frozen)
    loss_on, g_on, rs_on, names = _step(True, frozen)
    assert torch.equal(loss_on, loss_off)
    for n, v in rs_off.items():
        assert torch.equal(rs_on[n], v), n
    dense_on, dense_off = {}, {}
    for n, v in g_off.items():
        if v is None:
            assert g_on[n] is None, n
        elif DENSE_CONV.match(n):
            dense_on[n], dense_off[n] = g_on[n].numpy(), v.numpy()
        else:
            assert torch.equal(g_on[n], v), "%s is not a batched weight gradient and must keep its bits" % n
    per, l2 = grad_error_report(dense_on, dense_off)
    print("batched vs single weight gradients (%d tensors): global rel-L2 %.2e, worst tensor %.2e" % (len(per), l2, max(per.values())))
    assert_grads_close(per, l2, "batched vs per-layer weight gradients", typical=1e-4, worst=2e-3, l2=1e-4)
    return g_on, names, len(dense_off)


def test_switch_on_equals_switch_off_densenet121():
    g_on, _, n_dense = _compare(False)
    assert n_dense == 2 * (6 + 12 + 24 + 16)
    assert all(v is not None for v in g_on.values())


def test_frozen_layers_drop_out_of_the_batch():
    g_on, names, n_dense = _compare(True)
    assert names and any(DENSE_CONV.match("encoder." + n) for n in names), "the freeze no longer reaches a dense block"
    for n in names:
        assert g_on["encoder." + n] is None, n
    assert 0 < n_dense < 2 * (6 + 12 + 24 + 16)


def test_one_dense_block_backward_is_one_batched_wgrad_call():
    from bts_amd import train
    block = copy.deepcopy(_base_model().encoder.base_model.denseblock1).cuda().train()
    L = len(block)
    torch.manual_seed(3)
    x0 = torch.randn(2, 64, 12, 20, device="cuda")          # a map no other test of this module gives the block: fresh cache key
    gout = torch.randn(2, 64 + 32 * L, 12, 20, device="cuda")

    def run(batched):
        block.zero_grad()
        x = x0.clone().requires_grad_(True)
        y = train._dense_block(block, x, batched_wgrad=batched)
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            y.backward(gout)
            torch.cuda.synchronize()
        finally:
            ops.set_trace(None)
        return [(r[0], r[1]) for r in tr.records], {n: p.grad.clone() for n, p in block.named_parameters()}, x.grad

    run(False)                                   # first use packs the input-gradient weights: not counted
    rec_off, g_off, dx_off = run(False)
    cached = len(train._DENSE_WGRAD_BATCHES)
    rec_on, g_on, dx_on = run(True)
    assert len(train._DENSE_WGRAD_BATCHES) == cached + 1
    rec_on2, g_on2, _ = run(True)
    assert len(train._DENSE_WGRAD_BATCHES) == cached + 1, "the second step built a new batch table"
    assert rec_off.count(("conv_wgrad_kernel", "enc.wgrad")) == 2 * L
    assert not [r for r in rec_off if r[0] == "conv_wgrad_batch_kernel"]
    assert [r for r in rec_on if "wgrad" in r[0] or "wgrad" in r[1]] == [("conv_wgrad_batch_kernel", "enc.wgrad")]
    assert rec_on2 == rec_on
    strip = lambda rec: [r for r in rec if "wgrad" not in r[0]]
    assert strip(rec_on) == strip(rec_off), "the walk issues other launches than before"
    assert torch.equal(dx_on, dx_off)
    for n, v in g_off.items():
        if "conv" in n:
            assert torch.equal(g_on[n], g_on2[n]), n
            err = (g_on[n] - v).abs().max().item() / v.abs().max().item()
            assert err <= 1e-4, (n, err)
        else:
            assert torch.equal(g_on[n], v), n


def _decoder_step(batched):
    from bts_amd import bts as M
    c = TRAIN_CASE
    enc, md, ds, _, _ = CONFIGS[c["cname"]]
    feat = synth.ENCODER_CHANNELS[enc]
    dec = M.bts(Params(enc, 512, md, ds), feat, 512)
    sd = {k: (torch.tensor(v) if np.ndim(v) == 0 else t(v)) for k, v in synth.decoder_state(feat, 512, 0).items()}
    dec.load_state_dict(sd, strict=True)
    dec = dec.train().cuda()
    assert dec.batched_wgrad is False
    dec.fused_reduction_train, dec.batched_wgrad = True, batched
    feats, focal = make_inputs(c["cname"], c["B"], c["H"], c["W"], c["feat_seed"])
    feats = [None] + [f.cuda().requires_grad_(True) for f in feats[1:]]
    gt, mask = synth.train_targets(c["B"], c["H"], c["W"], md, c["target_seed"])
    outs = dec(feats, focal.cuda())
    loss = M.silog_loss(variance_focus=c["variance_focus"])(outs[4], t(gt).cuda(), t(mask).cuda())
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": np.array([loss.item()])}
    for i, f in enumerate(feats[1:]):
        res["feat%d" % i] = f.grad.cpu().numpy()
    for n, p in dec.named_parameters():
        assert p.grad is not None, n
        res[n] = p.grad.cpu().numpy()
    return res


def test_fused_reduction_scales_switch_on_equals_switch_off():
    off, on = _decoder_step(False), _decoder_step(True)
    for n, v in off.items():
        if "reduc" not in n:
            assert np.array_equal(on[n], v), "%s is not a batched weight gradient and must keep its bits" % n
    per, l2 = grad_error_report(on, off)
    print("batched vs per-layer reduction weight gradients: global rel-L2 %.2e, worst tensor %.2e" % (l2, max(per.values())))
    assert_grads_close(per, l2, "batched weight gradients of the fused reduction scales")


def test_one_wgrad_call_per_fused_reduction_scale():
    from bts_amd import bts as M
    from bts_amd import train
    name = "8x8"
    c_in, c_first, k = R.CHAINS[name]
    x, ws, gout, _, _ = R.case_reference(name, R.PLAIN_CASES[name])
    red = M.reduction_1x1(c_in, c_first, R.MAX_DEPTH).train().cuda()
    lpg = M.local_planar_guidance(k)

    def run(batched):
        xd = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        red.zero_grad()
        depth = train.fused_lpg_scale(red, lpg, xd, batched_wgrad=batched)
        tr = ops.KernelTrace()
        ops.set_trace(tr)
        try:
            depth.backward(gout.cuda())
            torch.cuda.synchronize()
        finally:
            ops.set_trace(None)
        return [(r[0], r[1]) for r in tr.records if r[1] == "reduc.wgrad"], [p.grad.clone() for p in red.parameters()], xd.grad

    rec_off, g_off, dx_off = run(False)
    rec_on, g_on, dx_on = run(True)
    assert rec_off == [("conv_wgrad_kernel", "reduc.wgrad")] * len(ws)
    assert rec_on == [("conv_wgrad_batch_kernel", "reduc.wgrad")]
    assert torch.equal(dx_on, dx_off)
    for a, b in zip(g_on, g_off):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item()
