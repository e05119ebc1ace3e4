"""The inference encoder graph (bts_amd/encoder_hip.py: DenseNetHip.run, ResNetHip.run) on the GPU against the fp64 torch.nn
references of tests/enc_node_cases.py, on tiny instances of the real networks:

  A. every node from its own GPU input: after plan.run(x) the workspace is read back, and each node's output is compared with
     the module's fp64 forward OF THE BUFFER THE GPU READ, under the derived fp32 bound (enc_node_cases' docstring); the
     max-pool and every skip tap bit-equal, the guard columns around the skip slots untouched;
  B. end to end: all taps and every surviving buffer against the fp64 run from the image, at 4x the CPU fp32 floor;
  C. the other branches of run() (bf16 precision and its switches, the native grouped kernel): the launch trace says which
     entry point every layer took, and the numerics are checked as far as they are observable;
  D. stale buffers: a forward is independent of what the same object forwarded before (another image, another shape), and
     of whatever its workspaces hold -- every buffer poisoned with NaN between two forwards, except the regions of
     ZERO_CONTRACT, whose allocation-time zeros the graph relies on."""
import copy
import functools
import os
from collections import OrderedDict

import pytest
import torch

import enc_node_cases as T
from parity_util import Params

from conftest import fp32_only

pytestmark = pytest.mark.gpu

EMULATED = os.environ.get("BTS_CONV_PRECISION", "0").strip() == "1"
GUARD = 7.0e4
BIG = 3.0e4                       # a large finite poison for regions that only ever meet zero weights
BF16_END_TO_END = 2e-2            # tests/test_bf16_gpu.py's bar for a max-abs / max-abs figure of the bf16 mode (iconv1)

# The zeros the graph depends on: (owner, buffer) -> (columns, poison, the product code that relies on them).  Everything else
# a forward touches takes NaN between two forwards.  ``BIG``: the region is read, and only ever multiplied by zero weights.
ZERO_CONTRACT = {
    ("DenseNetHip", "img"): ((3, 4), BIG, "encoder_hip.py DenseNetHip.run: nchw_to_nhwc writes img[:, :3] only; the stem reads 4 "
                                          "channels per pixel against pack_conv_weight(conv0, c_in_ld=4), whose fourth column is zero"),
    ("ResNetHip", "img"): ((3, 4), BIG, "encoder_hip.py ResNetHip.run: the same stem form (pack_conv_weight(conv1, c_in_ld=4))"),
}


# ------------------------------------------------------------------------------------------------------------ plumbing
def _new_plan(c, attrs=None):
    from bts_amd.encoder_hip import DenseNetHip, ResNetHip
    model = copy.deepcopy(c.model).cuda().eval()
    plan = (DenseNetHip if c.kind == "densenet" else ResNetHip)(model)
    for k, v in (attrs or {}).items():
        assert hasattr(plan, k), k
        setattr(plan, k, v)
    return plan


def _tap_channels(plan, c):
    return [plan.c_stem, plan.c_stem, plan.c_in[1], plan.c_in[2]] if c.kind == "densenet" else [plan.c_stem] + plan.c_out[:3]


class Slots:
    """The four skip destinations as the decoder hands them over: channel slices of wider buffers, GUARD on both sides."""

    def __init__(self, plan, c, B, H, W):
        self.wide, self.views = [], []
        for i, ch in enumerate(_tap_channels(plan, c)):
            wide = torch.full((B * (H >> (i + 1)) * (W >> (i + 1)), ch + 8), GUARD, device="cuda")
            self.wide.append(wide)
            self.views.append(wide[:, 4:4 + ch])

    def guards_untouched(self):
        return all(bool((w[:, :4] == GUARD).all()) and bool((w[:, 4 + v.shape[1]:] == GUARD).all())
                   for w, v in zip(self.wide, self.views))


def _forward(plan, x, precision="fp32", fill=T.FILL_FP32, slots=None, trace=False):
    from bts_amd import ops
    tr = ops.KernelTrace() if trace else None
    if trace:
        ops.set_trace(tr)
    try:
        with ops.launch_config(fill_frames=fill, precision=precision):
            r = plan.run(x, skip_dst=slots.views if slots is not None else None)
    finally:
        if trace:
            ops.set_trace(None)
    torch.cuda.synchronize()
    return r, ([(rec[0], rec[1]) for rec in tr.records] if trace else None)


def _readback(c, plan, r):
    """name -> NCHW CPU tensor of everything the forward left behind, under enc_node_cases.walk's names (+ DenseNet's "mid":
    the last dense layer's bottleneck intermediate)."""
    B, H, W = r["B"], r["H"], r["W"]
    ws = plan._workspace(B, H, W, r["dense"].device)
    t = OrderedDict()

    def put(name, rows, like=None):
        h, w = T.map_hw(c, like or name, H, W)
        assert rows.shape[0] >= B * h * w, (name, tuple(rows.shape), B, h, w)
        t[name] = T.rows_to_nchw(rows[:B * h * w].detach().float().cpu(), B, h, w)

    put("img", ws["img"][:, :3])
    for i, s in enumerate(r["skips"]):
        put("skip%d" % i, s)
    if c.kind == "densenet":
        for i in range(4):
            put("blk%d" % i, ws["blk%d" % i])
        for i in range(3):
            put("pool%d" % i, ws["pool%d" % i])
        put("mid", ws["mid"], like="blk3")
        assert r["dense"].data_ptr() == ws["blk3"].data_ptr() and r["dense"].shape == ws["blk3"].shape
        sc, sh = (v.detach().cpu().double() for v in r["norm5"])
        C = ws["blk3"].shape[1]
        assert sc.numel() == sh.numel() >= C
        t["norm5"] = t["blk3"].double() * T._v(sc[:C]) + T._v(sh[:C])      # norm5 is fused into the decoder: its vectors, applied here
        return t
    assert r["norm5"] is None
    put("x0", ws["x0"])
    for li, layer in enumerate(plan.layers):
        for k in ("t1", "t2", "idn"):
            put("%s_%d" % (k, li), ws["%s_%d" % (k, li)])
        n = len(layer)
        for bi in range(max(n - 2, 0), n):
            put("l%db%d" % (li, bi), ws["%s_%d" % ("a" if bi % 2 == 0 else "b", li)])
    assert torch.equal(T.rows_to_nchw(r["dense"].cpu(), B, H // 32, W // 32), t["l3b%d" % (len(plan.layers[3]) - 1)])
    return t


def _run_case(c, attrs=None, precision="fp32", fill=T.FILL_FP32, trace=False, x=None):
    plan = _new_plan(c, attrs)
    x = (c.x if x is None else x).cuda()
    slots = Slots(plan, c, *x.shape[:1], *x.shape[2:])
    r, recs = _forward(plan, x, precision, fill, slots, trace)
    t = _readback(c, plan, r)
    assert slots.guards_untouched(), "%s: a skip tap wrote outside its slot" % c.name
    return dict(plan=plan, tensors=t, launches=recs, ws=plan._workspace(r["B"], r["H"], r["W"], x.device))


@functools.lru_cache(maxsize=None)
def _fp32_run(name):
    return _run_case(T.case(name))["tensors"]


def _check_nodes(c, tensors, what, bf16=False):
    """Every node of the case from its own input.  fp32 (and the emulated fp32): the derived bound.  ``bf16``: the
    single-launch convolutions under the mode's bound on rounded operands; the stem (fp32 under every precision:
    csrc/conv_mfma.hip conv_choose), the pools and norm5 keep their fp32 statement; dense layers and whole transitions
    are not single launches."""
    worst, bad = [], []
    for n in T.nodes(c.name):
        got = T.cut(tensors, n.dst)
        if bf16 and n.op == "conv" and n.name != "stem":
            m = n.mods
            mod = lambda key: c.model.get_submodule(m[key]) if isinstance(m.get(key), str) else None
            res = T.cut(tensors, n.res) if n.res is not None else None
            ref, mag = T.conv_bf16_node(T.cut(tensors, n.src), mod("conv"), post=mod("post"), res=res,
                                        relu=m.get("relu", mod("post") is not None))
            ratio = T.bf16_check(got, ref, mag)
        elif bf16 and n.op in ("dense", "trans", "block"):
            continue
        else:
            ref, bound = T.node_eval(c, n, tensors)
            ratio = T.check(got, ref, bound)
        worst.append("%s %.3g" % (n.name, ratio))
        if not ratio <= 1.0:
            bad.append((n.name, n.kind, ratio))
        if n.skip is not None and not torch.equal(tensors[n.skip], got):
            bad.append((n.name, "skip tap %s differs from the primary output" % n.skip))
    print("%s: max |err| / bound per node: %s" % (what, ", ".join(worst)))
    assert not bad, (what, bad)


def _check_end_to_end(c, tensors, what, factor=T.FLOOR_FACTOR):
    ref, bad, seen = T.reference(c.name), [], []
    for k in T.survivors(c):
        e = float((tensors[k].double() - ref[k]).abs().max() / ref[k].abs().max())
        seen.append("%s %.2e/%.2e" % (k, e, T.FLOORS[c.name][k]))
        if not e <= factor * T.FLOORS[c.name][k]:
            bad.append((k, e, T.FLOORS[c.name][k]))
    print("%s: max|err|/max|ref| over the CPU fp32 floor: %s" % (what, ", ".join(seen)))
    assert not bad, (what, bad)


# --------------------------------------------------------------------------------------- A. every node, B. end to end
@pytest.mark.parametrize("name", list(T.CASES))
def test_every_node_from_its_own_gpu_input(name):
    c = T.case(name)
    t = _fp32_run(name)
    assert torch.equal(t["img"], c.x), "the NHWC image is not the input"
    _check_nodes(c, t, name)


@fp32_only
@pytest.mark.parametrize("name", list(T.CASES))
def test_every_surviving_tensor_end_to_end_vs_fp64(name):
    """4x the CPU fp32 floor is a statement about fp32 arithmetic: measured at most 2.6 floors on the fp32-input MFMA kernels.
    The emulated fp32 of a BTS_CONV_PRECISION=1 run (three bf16 planes, six products) is up to 5.6 floors away on the tensor
    with the smallest floor (d121_tall blk3: 5.9e-7 against 1.06e-7) and is held to the node bounds above instead."""
    _check_end_to_end(T.case(name), _fp32_run(name), name)


# ----------------------------------------------------------------------------------------------------------- C. branches
def _branch_marks(b):
    if b["precision"] == "fp32":
        return [fp32_only]
    return [pytest.mark.skipif(EMULATED, reason="BTS_CONV_PRECISION=1 forces precision 1 inside every scope")]


def _same_tensors(a, b, what, keys=None):
    diff = [k for k in (keys or a) if not torch.equal(a[k], b[k])]
    assert not diff, "%s: differ in %s" % (what, diff)


def _last_dense_layer_in_two_steps(c, run):
    """The last layer of the last block keeps its ``mid``: 1x1 (prologue, norm2, ReLU) from blk3's prefix, then the 3x3 from
    that very mid, each under the bf16 bound.  With bf16_mid_storage the last layer of a block that took the bf16 twin is
    checked the same way from ``mid_bf16``; the stored value is rounded once more (bf16 keeps 8 significant bits: 2^-8 of it)."""
    t, ws = run["tensors"], run["ws"]
    f = c.model
    todo = [(3, t["mid"], None)]
    if "mid_bf16" in ws:
        B, (h, w) = t["blk0"].shape[0], t["blk0"].shape[2:]
        todo.append((0, T.rows_to_nchw(ws["mid_bf16"][:B * h * w].float().cpu(), B, h, w), 2.0 ** -8))
    for bi, mid, rnd in todo:
        L = list(getattr(f, "denseblock%d" % (bi + 1)).values())[-1]
        cin, g = L.conv1.in_channels, L.conv2.out_channels
        blk = t["blk%d" % bi]
        ref, mag = T.conv_bf16_node(blk[:, :cin], L.conv1, pre=L.norm1, post=L.norm2)
        r1 = T.bf16_check(mid, ref, mag, extra=None if rnd is None else rnd * (ref.abs() + 2e-6 * mag))
        ref2, mag2 = T.conv_bf16_node(mid, L.conv2, relu=False)
        r2 = T.bf16_check(blk[:, cin:cin + g], ref2, mag2)
        print("%s block %d last layer: 1x1 %.3g, 3x3 %.3g of the bf16 bound" % (c.name, bi + 1, r1, r2))
        assert r1 <= 1.0 and r2 <= 1.0, (c.name, bi, r1, r2)


@pytest.mark.parametrize("branch", [pytest.param(n, marks=_branch_marks(b)) for n, b in T.BRANCHES.items()])
def test_branch_takes_the_intended_entry_points_and_keeps_its_numerics(branch):
    b = T.BRANCHES[branch]
    c = T.case(b["case"])
    run = _run_case(c, b["attrs"], b["precision"], T.FILL_BRANCH, trace=True)
    t = run["tensors"]
    # 1. the launch trace: tag by tag the entry point the docstrings and the plan queries name
    got = [(tag, T.entry_of_kernel(kern)) for kern, tag in run["launches"] if tag.startswith("enc_")]
    want = [(tag, "wide*" if e in ("wide", "wide192") else e) for tag, e, _ in T.expected_launches(branch)]
    assert got == want, (branch, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w], len(got), len(want))
    # 2. the numerics
    if b["precision"] == "fp32":
        _check_nodes(c, t, branch)
        _check_end_to_end(c, t, branch)
        return
    if b["precision"] == "bf16x3" or "ignored" in branch:       # the switches are inert: the bits of the run without them
        _same_tensors(t, _run_case(c, None, b["precision"], T.FILL_BRANCH)["tensors"], branch)
        if b["precision"] == "bf16x3":
            _check_nodes(c, t, branch)
        return
    _check_nodes(c, t, branch, bf16=True)
    if c.kind == "densenet":
        _last_dense_layer_in_two_steps(c, run)
    if b["attrs"].get("bf16_mid_storage"):                      # bit-identical to the same switches without it, per growth slice
        off = _run_case(c, dict(b["attrs"], bf16_mid_storage=False), b["precision"], T.FILL_BRANCH)["tensors"]
        _same_tensors(t, off, branch, keys=[k for k in t if k != "mid"])
    ref32, far = _fp32_run(b["case"]), []
    for k in T.survivors(c):
        e = float((t[k].double() - ref32[k].double()).abs().max() / ref32[k].double().abs().max())
        if not e <= BF16_END_TO_END:
            far.append((k, e))
    assert not far, (branch, far)


# ------------------------------------------------------------------------------------------------- D. stale buffers
HISTORY = [(n, None) for n in ("d161", "d121_tall", "r3211", "rx4")] + [(T.BRANCHES[n]["case"], n) for n in T.BRANCHES]


def _history_id(v):
    return v[1] or v[0] + "_fp32"


def _how(branch):
    b = T.BRANCHES[branch] if branch else dict(attrs=None, precision="fp32")
    return b["attrs"], b["precision"], (T.FILL_BRANCH if branch else T.FILL_FP32)


def _marks(branch):
    return _branch_marks(T.BRANCHES[branch]) if branch else []


@pytest.mark.parametrize("name,branch", [pytest.param(*v, marks=_marks(v[1]), id=_history_id(v)) for v in HISTORY])
def test_forward_is_independent_of_what_the_plan_forwarded_before(name, branch):
    """Image A, a forward at another shape and batch size, then image B through one plan: every tap and every workspace
    region the forward writes has the bits B gives in a fresh plan with fresh workspaces."""
    c = T.case(name)
    attrs, precision, fill = _how(branch)
    fresh = _run_case(c, attrs, precision, fill, x=c.image(1))["tensors"]
    plan = _new_plan(c, attrs)
    other = c.image(2, B=3 - c.B if c.B < 3 else 1, H=c.W, W=c.H) if c.H != c.W else c.image(2, B=c.B + 1)
    for x in (c.x, other, c.x):
        _forward(plan, x.cuda(), precision, fill)
    slots = Slots(plan, c, c.B, c.H, c.W)
    r, _ = _forward(plan, c.image(1).cuda(), precision, fill, slots)
    _same_tensors(fresh, _readback(c, plan, r), "%s after other forwards" % _history_id((name, branch)))
    assert slots.guards_untouched()


def _poison(ws, owner):
    for key, buf in ws.items():
        cols = ZERO_CONTRACT.get((owner, key))
        if not buf.is_floating_point():
            continue
        if cols is None:
            buf.fill_(float("nan"))
        else:
            (lo, hi), value, _ = cols
            keep = buf[:, lo:hi].clone()
            buf.fill_(float("nan"))
            buf[:, lo:hi] = keep if value is None else value


@pytest.mark.parametrize("name,branch", [pytest.param(*v, marks=_marks(v[1]), id=_history_id(v)) for v in HISTORY])
def test_forward_reads_nothing_it_has_not_written(name, branch):
    """Every workspace the forward touches (workspace.recording) is overwritten between two forwards of one image: NaN
    everywhere, a large finite value in the ZERO_CONTRACT regions that only meet zero weights.  Same bits, no NaN."""
    from bts_amd import workspace
    c = T.case(name)
    attrs, precision, fill = _how(branch)
    plan = _new_plan(c, attrs)
    x = c.x.cuda()
    with workspace.recording() as touched:
        r, _ = _forward(plan, x, precision, fill)
    first = _readback(c, plan, r)
    assert touched and all(cache is plan._ws for cache, _ in touched)
    for cache, key in touched:
        _poison(cache._entries[key], type(plan).__name__)
    torch.cuda.synchronize()
    r, _ = _forward(plan, x, precision, fill)
    again = _readback(c, plan, r)
    nan = [k for k, v in again.items() if not bool(torch.isfinite(v).all())]
    assert not nan, "%s: read before written, NaN reached %s" % (name, nan)
    _same_tensors(first, again, "%s after poisoning" % _history_id((name, branch)))


# ---- the whole model: encoder plan + decoder workspaces (bts._bufs), one stream and two sub-batches
MODELS = ["densenet121_bts", "resnet50_bts"]


@functools.lru_cache(maxsize=None)
def _model_state(enc):
    from bts_amd import bts as M
    ds, md = ("kitti", 80.0) if enc.startswith("densenet") else ("nyu", 10.0)
    params = Params(enc, 512, md, ds)
    torch.manual_seed(5)
    model = M.BtsModel(params).eval()
    T.randomise(model.encoder, torch.Generator().manual_seed(9))
    return params, model.state_dict()


# conv_precision and switches of the model forwards: fp32, and the bf16 mode with every encoder switch it has
MODES = {"fp32": ("fp32", {}), "bf16": ("bf16", dict(bf16_wide_1x1="all", bf16_mid_storage=True))}
MODE_PARAMS = [pytest.param("fp32"), pytest.param("bf16", marks=pytest.mark.skipif(EMULATED, reason="BTS_CONV_PRECISION=1 forces precision 1"))]


def _model(enc, sub_batches, mode="fp32"):
    from bts_amd import bts as M
    params, state = _model_state(enc)
    m = M.BtsModel(params).eval()
    m.load_state_dict(state)
    m = m.cuda()
    m.sub_batches = sub_batches
    m.conv_precision = MODES[mode][0]
    for k, v in MODES[mode][1].items():
        setattr(m, k, v)
    return m


def _images(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, 3, H, W), generator=g).cuda(), (500.0 + 300.0 * torch.rand(B, generator=g)).cuda()


def _outs(m, x, focal):
    with torch.no_grad():
        out = [o.clone() for o in m(x, focal)]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in out), "a NaN or Inf in the outputs"
    return out


@pytest.mark.parametrize("mode", MODE_PARAMS)
@pytest.mark.parametrize("sub_batches", [1, 2])
@pytest.mark.parametrize("enc", MODELS)
def test_model_forward_is_independent_of_earlier_forwards(enc, sub_batches, mode):
    a, b, other = _images(2, 32, 64, 1), _images(2, 32, 64, 2), _images(3, 64, 32, 3)
    fresh = _outs(_model(enc, sub_batches, mode), *b)
    m = _model(enc, sub_batches, mode)
    for x in (a, other, a):
        _outs(m, *x)
    got = _outs(m, *b)
    diff = [i for i in range(6) if not torch.equal(fresh[i], got[i])]
    assert not diff, (enc, sub_batches, mode, diff)


def _owner(cache, m):
    return "bts" if cache is m.decoder._bufs else type(next(iter(m._enc_plans.values()))).__name__


@pytest.mark.parametrize("mode", MODE_PARAMS)
@pytest.mark.parametrize("sub_batches", [1, 2])
@pytest.mark.parametrize("enc", MODELS)
def test_model_forward_reads_nothing_it_has_not_written(enc, sub_batches, mode):
    """The encoder plan's and the decoder's workspaces of every sub-batch slot, poisoned between two forwards of one batch.
    The decoder's buffers take NaN everywhere: bts._alloc_workspace pads f5 and cat5 to multiples of 4 channels against zero
    weight columns, and for every encoder the model supports those pads have no width (asserted here)."""
    from bts_amd import workspace
    m = _model(enc, sub_batches, mode)
    x = _images(2, 32, 64, 4)
    with workspace.recording() as touched:
        first = _outs(m, *x)
    entries = {(id(cc), k): (cc, k) for cc, k in touched}
    owners = {_owner(cache, m) for cache, _ in entries.values()}
    assert "bts" in owners and len(owners) == 2 and len(entries) == 2 * sub_batches, touched
    dec = m.decoder
    for cache, key in entries.values():
        ws = cache._entries[key]
        if cache is dec._bufs:
            assert ws["f5"].shape[1] == dec.feat_out_channels[4] and ws["cat5"].shape[1] == dec.num_features + dec.feat_out_channels[3]
        _poison(ws, _owner(cache, m))
    torch.cuda.synchronize()
    got = _outs(m, *x)
    diff = [i for i in range(6) if not torch.equal(first[i], got[i])]
    assert not diff, (enc, sub_batches, mode, diff)
