"""Case tables, builders, fp64 references and bounds for the nodes of the inference encoder graph (bts_amd/encoder_hip.py:
DenseNetHip.run, ResNetHip.run): tiny instances of the very modules the plans walk (encoders.densenet_features,
encoders.ResNet), small enough that one fp64 run on the CPU is the yardstick for every buffer a forward leaves behind.

The reference of a node is the module's own torch.nn forward in fp64 (never encoder_hip.py), computed FROM THE INPUT THE GPU
ITSELF READ (the workspace buffer), so the comparison isolates one node: a fold that takes another layer's norm, a slice that
is off by a growth, a stale ping-pong buffer is percent-level there however deep the layer sits.  Nothing here touches the GPU.

Bound of a node (``node_eval`` returns it per element next to the reference), U = 2^-24, worst case and to first order:
  * a folded norm layer, y = s x + t with s = g / sqrt(v + eps), t = b - m s, everything in fp32: s carries 4 roundings (add,
    sqrt, divide, multiply; 4.5 U with a square root that is one ulp off), t = fl(b - fl(m s)) then 6 U |m s| + U |b|, the
    evaluation fl(fl(x s) + t) another U |x s| + U |y|: 6.5 U |s x| + 7.5 U |m s| + 2 U |b| <= ``bn_err`` =
    8 U (|s| (|x| + |m|) + |b|);
  * a convolution of n = k^2 c_in / groups terms: (n + 8 + 5) U sum |w| |x| -- one rounding per product and a chain of at most
    n additions, 8 more across split-K partials, 5 of margin: the bound of
    tests/test_upconv_train_gpu.py::test_dgrad_fp32_products_within_the_summation_bound -- plus sum |w| e_x for an input
    that carries the error e_x itself (the prologue's, or the unobservable intermediate's: the dense layer's ``mid`` enters the
    3x3 through |w2|, a bottleneck's t1 / t2 through |w2| / |w3|);
  * the epilogue norm: |s| e_acc + bn_err(acc); the identity: + e_idn + U (|norm(acc)| + |idn|); ReLU is 1-Lipschitz;
  * bn_relu_avgpool2, 0.25 (z0 + z1 + z2 + z3) with z = relu(s x + t) as tests/stream_cases.py states the kernel
    (avgpool_ref): the mean of bn_err over the window plus 3 U mean(z) for the three additions (the quarter is exact);
  * the max-pool selects: bit-equal.
tests/test_enc_node_cases_host.py shows on the CPU that the bound is neither vacuous nor too tight: the CPU fp32 evaluation of
every node stays inside it, and a reference with one channel's folded shift times 1.01 (or a rotated growth slice) leaves it.

End to end (``FLOORS``): per case and tensor the distance max|fp32 - fp64| / max|fp64| of the CPU fp32 run of the same modules
from the fp64 run, measured once (``measure_floors``; the host test re-measures); the GPU may be FLOOR_FACTOR = 4 times as
far -- another summation order, folded against unfolded norm layers -- as in tests/test_reduc_train_gpu.py."""
import copy
import functools
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from bts_amd import encoders as E

U = 2.0 ** -24
FLOOR_FACTOR = 4.0
FILL_FP32 = 2               # what a BtsModel declares for B <= 2 (ops.auto_fill_frames): split-K on the deep layers
FILL_BRANCH = 4096          # the largest declaration: the plan queries of section "branches" count fill_frames x workgroups

# every channel count on the way is a multiple of 4 (the NHWC kernels' row alignment): (3,2,2,2) at growth 48 gives 102
NETS = OrderedDict([
    ("d161", dict(kind="densenet", build=lambda: E.densenet_features(48, (4, 2, 2, 2), 96))),      # c_in 144 (% 32), 120 (% 16)
    ("d121", dict(kind="densenet", build=lambda: E.densenet_features(32, (2, 2, 2, 2), 64))),
    ("r1111", dict(kind="resnet", build=lambda: E.ResNet((1, 1, 1, 1)))),                         # every block a downsample
    ("r3211", dict(kind="resnet", build=lambda: E.ResNet((3, 2, 1, 1)))),                         # identity at both parities
    ("rx4", dict(kind="resnet", build=lambda: E.ResNet((2, 1, 1, 1), groups=32, width_per_group=4))),
    ("rx8", dict(kind="resnet", build=lambda: E.ResNet((1, 2, 2, 1), groups=32, width_per_group=8))),
])
# case -> (net, B, H, W): the deepest stage of 32x64 is 1x2 pixels, and B = 2 has a frame boundary
CASES = OrderedDict([
    ("d161", ("d161", 2, 32, 64)), ("d121", ("d121", 2, 32, 64)), ("d121_tall", ("d121", 1, 64, 32)),
    ("d161_wide", ("d161", 1, 32, 128)),        # block 1 on an 8x32 map: whole 4x32 tiles, which ops.conv3x3_bf16in_plan asks for
    ("r1111", ("r1111", 2, 32, 64)), ("r3211", ("r3211", 2, 32, 64)), ("rx4", ("rx4", 2, 32, 64)), ("rx8", ("rx8", 2, 32, 64)),
])


def randomise(module, gen):
    """Convolutions N(0, 1/fan_in); every norm layer well away from the identity: gamma in [0.5, 1.5], beta and running mean
    0.3 N(0, 1), running variance in [0.5, 1.5] -- a swapped or mis-padded vector changes values."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) / np.sqrt(m.weight[0].numel()))
            elif isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(torch.rand(c, generator=gen) + 0.5)
                m.bias.copy_(0.3 * torch.randn(c, generator=gen))
                m.running_mean.copy_(0.3 * torch.randn(c, generator=gen))
                m.running_var.copy_(torch.rand(c, generator=gen) + 0.5)


class Case:
    """``model`` (CPU fp32, eval mode, randomised) and the image ``x``; ``image(k)``: another image of the same shape."""

    def __init__(self, name):
        net, self.B, self.H, self.W = CASES[name]
        self.name, self.net, self.kind = name, net, NETS[net]["kind"]
        gen = torch.Generator().manual_seed(1000 + list(NETS).index(net))
        self.model = NETS[net]["build"]().eval()
        randomise(self.model, gen)
        self.x = self.image(0)

    def image(self, k, B=None, H=None, W=None):
        gen = torch.Generator().manual_seed(77 + 131 * k + list(CASES).index(self.name))
        return torch.randn((B or self.B, 3, H or self.H, W or self.W), generator=gen)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def widths(model):
    """Every channel count a buffer of the plan holds."""
    return sorted({m.num_features for m in model.modules() if isinstance(m, nn.BatchNorm2d)}
                  | {c for m in model.modules() if isinstance(m, nn.Conv2d) and m.in_channels != 3 for c in (m.in_channels, m.out_channels)})


# ---------------------------------------------------------------------------------------------- whole-network references
def _walk_densenet(f, x):
    t = OrderedDict(img=x)
    y = f.relu0(f.norm0(f.conv0(x)))
    t["skip0"] = y
    y = f.pool0(y)
    t["skip1"] = y
    blocks = [m for n, m in f.named_children() if n.startswith("denseblock")]
    trans = [m for n, m in f.named_children() if n.startswith("transition")]
    for bi, blk in enumerate(blocks):
        y = blk(y)
        t["blk%d" % bi] = y
        if bi < len(trans):
            t["pool%d" % bi] = F.avg_pool2d(F.relu(trans[bi].norm(y)), 2, 2)     # what the plan keeps: pooled before the 1x1
            y = trans[bi](y)
            if bi < 2:
                t["skip%d" % (bi + 2)] = y
    t["norm5"] = f.norm5(y)
    return t


def _walk_resnet(m, x):
    t = OrderedDict(img=x)
    y = m.relu(m.bn1(m.conv1(x)))
    t["skip0"] = y
    y = m.maxpool(y)
    t["x0"] = y
    for li, layer in enumerate((m.layer1, m.layer2, m.layer3, m.layer4)):
        t["idn_%d" % li] = layer[0].downsample(y)
        for bi, blk in enumerate(layer):
            if bi == len(layer) - 1:
                t["t1_%d" % li] = blk.relu(blk.bn1(blk.conv1(y)))
                t["t2_%d" % li] = blk.relu(blk.bn2(blk.conv2(t["t1_%d" % li])))
            y = blk(y)
            t["l%db%d" % (li, bi)] = y
        if li < 3:
            t["skip%d" % (li + 1)] = y
    return t


def walk(c, dtype, x=None):
    """name -> NCHW tensor of every buffer a forward of the plan leaves behind (and, for ResNet, every block output), from the
    modules' own forwards in ``dtype``."""
    model = copy.deepcopy(c.model).to(dtype)
    x = (c.x if x is None else x).to(dtype)
    with torch.no_grad():
        t = (_walk_densenet if c.kind == "densenet" else _walk_resnet)(model, x)
    return OrderedDict((k, v.detach().clone()) for k, v in t.items())


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    return walk(case(name), dtype)


def survivors(c):
    """The tensors of ``walk`` a finished forward still holds (ResNetHip keeps the last two block outputs of a stage)."""
    if c.kind == "densenet":
        return [k for k in reference(c.name) if k != "img"]
    keep = []
    for k in reference(c.name):
        if k == "img":
            continue
        if k[0] == "l" and k[2] == "b":
            n = len(getattr(c.model, "layer%d" % (int(k[1]) + 1)))
            if int(k[3:]) < n - 2:
                continue
        keep.append(k)
    return keep


def measure_floors(name):
    r64, r32 = reference(name), walk(case(name), torch.float32)
    return OrderedDict((k, float((r32[k].double() - r64[k]).abs().max() / r64[k].abs().max())) for k in r64 if k != "img")


# measure_floors() on the CPU of the build container (one seed per network, above)
FLOORS = {
    "d161": {"skip0": 3.90e-07, "skip1": 3.90e-07, "blk0": 3.90e-07, "pool0": 3.43e-07, "skip2": 3.56e-07,
        "blk1": 3.56e-07, "pool1": 2.24e-07, "skip3": 3.42e-07, "blk2": 3.42e-07, "pool2": 1.74e-07, "blk3": 3.61e-07,
        "norm5": 1.91e-07},
    "d121": {"skip0": 4.36e-07, "skip1": 4.36e-07, "blk0": 4.36e-07, "pool0": 3.00e-07, "skip2": 2.65e-07,
        "blk1": 2.65e-07, "pool1": 1.42e-07, "skip3": 2.20e-07, "blk2": 2.20e-07, "pool2": 1.08e-07, "blk3": 1.77e-07,
        "norm5": 1.89e-07},
    "d121_tall": {"skip0": 3.24e-07, "skip1": 3.24e-07, "blk0": 3.65e-07, "pool0": 1.67e-07, "skip2": 1.88e-07,
        "blk1": 1.94e-07, "pool1": 1.60e-07, "skip3": 1.66e-07, "blk2": 1.66e-07, "pool2": 1.04e-07, "blk3": 1.06e-07,
        "norm5": 1.03e-07},
    "d161_wide": {"skip0": 3.91e-07, "skip1": 3.91e-07, "blk0": 3.91e-07, "pool0": 3.37e-07, "skip2": 3.70e-07,
        "blk1": 3.70e-07, "pool1": 2.02e-07, "skip3": 2.81e-07, "blk2": 2.81e-07, "pool2": 1.59e-07, "blk3": 2.19e-07,
        "norm5": 2.99e-07},
    "r1111": {"skip0": 3.05e-07, "x0": 3.05e-07, "idn_0": 4.25e-07, "t1_0": 3.28e-07, "t2_0": 3.31e-07, "l0b0": 3.81e-07,
        "skip1": 3.81e-07, "idn_1": 6.27e-07, "t1_1": 4.83e-07, "t2_1": 4.44e-07, "l1b0": 5.37e-07, "skip2": 5.37e-07,
        "idn_2": 3.40e-07, "t1_2": 4.93e-07, "t2_2": 4.98e-07, "l2b0": 3.94e-07, "skip3": 3.94e-07, "idn_3": 3.46e-07,
        "t1_3": 4.74e-07, "t2_3": 6.05e-07, "l3b0": 3.88e-07},
    "r3211": {"skip0": 4.38e-07, "x0": 4.38e-07, "idn_0": 3.98e-07, "l0b0": 3.58e-07, "l0b1": 3.92e-07, "t1_0": 6.03e-07,
        "t2_0": 9.77e-07, "l0b2": 4.00e-07, "skip1": 4.00e-07, "idn_1": 7.63e-07, "l1b0": 5.24e-07, "t1_1": 4.83e-07,
        "t2_1": 4.93e-07, "l1b1": 5.00e-07, "skip2": 5.00e-07, "idn_2": 6.76e-07, "t1_2": 4.02e-07, "t2_2": 6.18e-07,
        "l2b0": 5.34e-07, "skip3": 5.34e-07, "idn_3": 4.76e-07, "t1_3": 7.01e-07, "t2_3": 5.76e-07, "l3b0": 4.67e-07},
    "rx4": {"skip0": 3.76e-07, "x0": 3.76e-07, "idn_0": 4.03e-07, "l0b0": 3.92e-07, "t1_0": 5.62e-07, "t2_0": 6.60e-07,
        "l0b1": 4.22e-07, "skip1": 4.22e-07, "idn_1": 5.05e-07, "t1_1": 6.20e-07, "t2_1": 5.14e-07, "l1b0": 4.44e-07,
        "skip2": 4.44e-07, "idn_2": 5.48e-07, "t1_2": 5.67e-07, "t2_2": 5.50e-07, "l2b0": 4.93e-07, "skip3": 4.93e-07,
        "idn_3": 4.44e-07, "t1_3": 5.14e-07, "t2_3": 4.65e-07, "l3b0": 4.05e-07},
    "rx8": {"skip0": 4.66e-07, "x0": 4.66e-07, "idn_0": 3.17e-07, "t1_0": 3.26e-07, "t2_0": 3.72e-07, "l0b0": 3.42e-07,
        "skip1": 3.42e-07, "idn_1": 5.35e-07, "l1b0": 3.54e-07, "t1_1": 5.62e-07, "t2_1": 5.35e-07, "l1b1": 3.60e-07,
        "skip2": 3.60e-07, "idn_2": 3.50e-07, "l2b0": 4.98e-07, "t1_2": 5.40e-07, "t2_2": 5.40e-07, "l2b1": 4.73e-07,
        "skip3": 4.73e-07, "idn_3": 3.69e-07, "t1_3": 5.06e-07, "t2_3": 5.96e-07, "l3b0": 4.14e-07},
}


# ------------------------------------------------------------------------------------------------------------- bounds
def _v(t):
    return t.reshape(1, -1, 1, 1)


def fold(bn):
    """(scale, shift) of an eval-mode norm layer, in the dtype of its tensors."""
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return s, bn.bias - bn.running_mean * s


def bn_err(bn, x):
    s, _ = fold(bn)
    return 8.0 * U * (_v(s.abs()) * (x.abs() + _v(bn.running_mean.abs())) + _v(bn.bias.abs()))


def conv_terms(conv):
    return conv.kernel_size[0] * conv.kernel_size[1] * conv.in_channels // conv.groups


def conv_abs(conv, t):
    return F.conv2d(t, conv.weight.abs(), None, conv.stride, conv.padding, conv.dilation, conv.groups)


def conv_node(x, conv, pre=None, post=None, relu=True, res=None, res_err=None, x_err=None):
    """act(post(conv(relu(pre(x)))) + res) by the modules themselves, and its fp32 bound (module docstring).  ``x_err``: the
    error the input itself carries."""
    e = torch.zeros_like(x) if x_err is None else x_err
    p = x
    if pre is not None:
        e = _v(fold(pre)[0].abs()) * e + bn_err(pre, x)
        p = F.relu(pre(x))
    acc = conv(p)
    e = conv_abs(conv, e) + (conv_terms(conv) + 8 + 5) * U * conv_abs(conv, p.abs())
    y = acc
    if post is not None:
        y = post(acc)
        e = _v(fold(post)[0].abs()) * e + bn_err(post, acc)
    if res is not None:
        e = e + (0.0 if res_err is None else res_err) + U * (y.abs() + res.abs())
        y = y + res
    return (F.relu(y) if relu else y), e


def avgpool_node(x, norm):
    z = F.relu(norm(x))
    return F.avg_pool2d(z, 2, 2), F.avg_pool2d(bn_err(norm, x), 2, 2) + 3.0 * U * F.avg_pool2d(z, 2, 2)


def bottleneck_node(blk, x):
    t1, e1 = conv_node(x, blk.conv1, post=blk.bn1)
    t2, e2 = conv_node(t1, blk.conv2, post=blk.bn2, x_err=e1)
    if blk.downsample is not None:
        idn, ei = conv_node(x, blk.downsample[0], post=blk.downsample[1], relu=False)
    else:
        idn, ei = x, None
    _, e3 = conv_node(t2, blk.conv3, post=blk.bn3, res=idn, res_err=ei, x_err=e2)
    return blk(x), e3


# --------------------------------------------------------------------------------------------------------------- nodes
# ``src`` / ``dst`` / ``res``: (tensor name, first channel, end channel or None) of ``walk``'s names; ``mods``: dotted paths of
# the modules the op uses; ``op`` selects the evaluation in node_eval; ``skip``: the tensor the node's second destination is
Node = namedtuple("Node", "name kind op mods src dst res skip")
NODE_KINDS = ("stem", "maxpool_1dst", "maxpool_2dst", "dense", "avgpool", "transition_skip", "transition_noskip", "norm5",
              "bott_ds1", "bott_ds2", "bott_id_a", "bott_id_b", "gconv_s1", "gconv_s2")


def _dense_nodes(c):
    f = c.model
    nodes = [Node("stem", "stem", "conv", dict(conv="conv0", post="norm0"), ("img", 0, None), ("skip0", 0, None), None, None),
             Node("pool0", "maxpool_2dst", "maxpool", {}, ("skip0", 0, None), ("blk0", 0, f.conv0.out_channels), None, "skip1")]
    blocks = [(n, m) for n, m in f.named_children() if n.startswith("denseblock")]
    for bi, (bn_, blk) in enumerate(blocks):
        for ln, layer in blk.items():
            cin, g = layer.conv1.in_channels, layer.conv2.out_channels
            nodes.append(Node("%s.%s" % (bn_, ln), "dense", "dense", dict(layer="%s.%s" % (bn_, ln)),
                              ("blk%d" % bi, 0, cin), ("blk%d" % bi, cin, cin + g), None, None))
        if bi < 3:
            tr = "transition%d" % (bi + 1)
            co = getattr(f, tr).conv.out_channels
            nodes.append(Node(tr + ".pool", "avgpool", "avgpool", dict(norm=tr + ".norm"), ("blk%d" % bi, 0, None),
                              ("pool%d" % bi, 0, None), None, None))
            kind = "transition_skip" if bi < 2 else "transition_noskip"
            skip = "skip%d" % (bi + 2) if bi < 2 else None
            nodes.append(Node(tr + ".conv", kind, "conv", dict(conv=tr + ".conv"), ("pool%d" % bi, 0, None),
                              ("blk%d" % (bi + 1), 0, co), None, skip))
            nodes.append(Node(tr, kind, "trans", dict(tr=tr), ("blk%d" % bi, 0, None), ("blk%d" % (bi + 1), 0, co), None, skip))
    nodes.append(Node("norm5", "norm5", "norm", dict(norm="norm5"), ("blk3", 0, None), ("norm5", 0, None), None, None))
    return nodes


def _resnet_nodes(c):
    m = c.model
    A = ("x0", 0, None)
    nodes = [Node("stem", "stem", "conv", dict(conv="conv1", post="bn1"), ("img", 0, None), ("skip0", 0, None), None, None),
             Node("maxpool", "maxpool_1dst", "maxpool", {}, ("skip0", 0, None), A, None, None)]
    prev = "x0"
    for li in range(4):
        layer = getattr(m, "layer%d" % (li + 1))
        n = len(layer)
        skip = "skip%d" % (li + 1) if li < 3 else None
        s = layer[0].conv2.stride[0]
        ds_kind = "bott_ds1" if s == 1 else "bott_ds2"
        path = "layer%d" % (li + 1)
        # block 0's downsample: ``idn`` survives whatever follows
        nodes.append(Node("%s.0.down" % path, ds_kind, "conv", dict(conv="%s.0.downsample.0" % path, post="%s.0.downsample.1" % path,
                                                                    relu=False), (prev, 0, None), ("idn_%d" % li, 0, None), None, None))
        if n == 2:                                              # block 0 of two: its input and its output both survive
            nodes.append(Node("%s.0" % path, ds_kind, "block", dict(blk="%s.0" % path), (prev, 0, None), ("l%db0" % li, 0, None),
                              None, None))
        last = n - 1
        src = prev if n == 1 else "l%db%d" % (li, last - 1)
        kind = ds_kind if n == 1 else ("bott_id_a" if last % 2 == 0 else "bott_id_b")
        bp = "%s.%d" % (path, last)
        t1, t2, out = "t1_%d" % li, "t2_%d" % li, "l%db%d" % (li, last)
        nodes.append(Node(bp + ".conv1", kind, "conv", dict(conv=bp + ".conv1", post=bp + ".bn1"), (src, 0, None), (t1, 0, None), None, None))
        g = layer[last].conv2.groups
        k2 = kind if g == 1 else ("gconv_s1" if layer[last].conv2.stride[0] == 1 else "gconv_s2")
        nodes.append(Node(bp + ".conv2", k2, "conv", dict(conv=bp + ".conv2", post=bp + ".bn2"), (t1, 0, None), (t2, 0, None), None, None))
        res = ("idn_%d" % li, 0, None) if n == 1 else (src, 0, None)
        nodes.append(Node(bp + ".conv3", kind, "conv", dict(conv=bp + ".conv3", post=bp + ".bn3"), (t2, 0, None), (out, 0, None), res, skip))
        prev = out
    return nodes


@functools.lru_cache(maxsize=None)
def nodes(name):
    c = case(name)
    return tuple(_dense_nodes(c) if c.kind == "densenet" else _resnet_nodes(c))


def cut(tensors, ref):
    name, lo, hi = ref
    return tensors[name][:, lo:hi]


def _mod(c, path, dtype, cache):
    if path not in cache:
        cache[path] = copy.deepcopy(c.model.get_submodule(path)).to(dtype)
    return cache[path]


def _shift_target(node, get):
    """The node's last norm layer in front of its output: the one whose folded shift the host test's wrong reference moves."""
    if node.op == "conv":
        return get("post") if get("post") is not None else get("pre")
    return {"dense": lambda: get("layer").norm2, "trans": lambda: get("tr").norm, "block": lambda: get("blk").bn3,
            "avgpool": lambda: get("norm"), "norm": lambda: get("norm")}[node.op]()


def _eval(c, node, tensors, dtype, shift_ch):
    cache = {}
    get = lambda key: _mod(c, node.mods[key], dtype, cache) if isinstance(node.mods.get(key), str) else None
    x = cut(tensors, node.src).to(dtype)
    if shift_ch is not None:
        bn = _shift_target(node, get)
        with torch.no_grad():
            bn.bias[shift_ch] += 0.01 * fold(bn)[1][shift_ch]
    with torch.no_grad():
        if node.op == "conv":
            res = cut(tensors, node.res).to(dtype) if node.res is not None else None
            ref, bound = conv_node(x, get("conv"), pre=get("pre"), post=get("post"), res=res,
                                   relu=node.mods.get("relu", get("post") is not None))
            aux = ref
        elif node.op == "dense":
            L = get("layer")
            aux, e = conv_node(x, L.conv1, pre=L.norm1, post=L.norm2)
            _, bound = conv_node(aux, L.conv2, relu=False, x_err=e)
            ref = L(x)
        elif node.op == "maxpool":
            ref, bound = F.max_pool2d(x, 3, 2, 1), None
            aux = ref
        elif node.op == "avgpool":
            ref, bound = avgpool_node(x, get("norm"))
            aux = ref
        elif node.op == "trans":
            tr = get("tr")
            aux, e = avgpool_node(x, tr.norm)
            _, bound = conv_node(aux, tr.conv, relu=False, x_err=e)
            ref = tr(x.clone())
        elif node.op == "block":
            ref, bound = bottleneck_node(get("blk"), x)
            aux = ref
        elif node.op == "norm":
            ref, bound = get("norm")(x), bn_err(get("norm"), x)
            aux = ref
        else:
            raise KeyError(node.op)
    return ref, bound, aux


def node_eval(c, node, tensors, dtype=torch.float64, mutate=None):
    """(reference, bound) of ``node`` from ITS OWN input ``cut(tensors, node.src)`` (and identity ``node.res``), the modules
    evaluated in ``dtype``.  ``mutate``, the wrong references of the host test: "shift" multiplies by 1.01 the folded shift of
    one channel of the node's last norm layer (the channel with the largest mean value behind that layer, so that no ReLU
    hides it; where the layer stands at the node's output, the channel where 1 % of |shift| is largest against the bound);
    "rotate" rotates the output channels by one."""
    ch = None
    if mutate == "shift":
        ref, bound, aux = _eval(c, node, tensors, torch.float64, None)
        if aux is ref and bound is not None:      # the layer stands at the output: where 1 % of |shift| is largest over the bound
            cache = {}
            t = fold(_shift_target(node, lambda key: _mod(c, node.mods[key], torch.float64, cache)
                                   if isinstance(node.mods.get(key), str) else None))[1]
            live = (ref != 0) if node.op != "norm" else torch.ones_like(ref, dtype=torch.bool)
            ch = int((_v(t.abs()) * live / bound).amax(dim=(0, 2, 3)).argmax())
        else:
            ch = int(aux.mean(dim=(0, 2, 3)).argmax())
    ref, bound, _ = _eval(c, node, tensors, dtype, ch)
    if mutate == "rotate":
        ref = ref.roll(1, dims=1)
    return ref, bound


def mutations(node):
    """The wrong references the bound of ``node`` must reject, each of them.  A node with an unobservable intermediate (the
    dense layer's ``mid``, t1 / t2 of a whole bottleneck) carries that intermediate's worst-case error through |w|: a bound
    some sqrt(n) wider per hidden layer than what rounding really does, under which 1 % of one channel's shift can hide
    (measured on the CPU: 0.03 .. 5 times the bound).  Those nodes are held to the rotated slice; every single-launch node to
    the shift."""
    if node.op == "maxpool":
        return ()
    if node.op == "conv" and not any(k in node.mods for k in ("pre", "post")):
        return ("rotate",)                                       # the transition's 1x1: no norm layer of its own
    return ("rotate",) if node.op in ("dense", "block") else ("shift",)


def check(got, ref, bound):
    """max |got - ref| / bound over the elements (0/0 = 0); bound None: bit-equality, inf where a bit differs."""
    got, ref = got.double(), ref.double()
    if bound is None:
        return 0.0 if torch.equal(got.float(), ref.float()) else float("inf")
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.double().clamp_min(1e-300))
    return float(ratio.max()) if bool(torch.isfinite(got).all()) else float("inf")


def rows_to_nchw(rows, B, h, w):
    """An NHWC [B*h*w, C] buffer (CPU tensor) as NCHW."""
    return rows.reshape(B, h, w, rows.shape[1]).permute(0, 3, 1, 2).contiguous()


def map_hw(c, name, H=None, W=None):
    """(h, w) of the map the buffer ``name`` holds for an H x W image."""
    H, W = H or c.H, W or c.W
    if c.kind == "densenet":
        s = {"img": 1, "skip0": 2, "skip1": 4, "skip2": 8, "skip3": 16, "blk0": 4, "blk1": 8, "blk2": 16, "blk3": 32,
             "pool0": 8, "pool1": 16, "pool2": 32, "norm5": 32}[name]
    elif name in ("img", "skip0", "x0") or name.startswith("skip"):
        s = {"img": 1, "skip0": 2, "x0": 4, "skip1": 4, "skip2": 8, "skip3": 16}[name]
    else:
        li = int(name[1]) if name[0] == "l" else int(name.split("_")[1])
        s = 4 << li
        if name.startswith("t1_") and li > 0 and len(getattr(c.model, "layer%d" % (li + 1))) == 1:
            s //= 2                                             # conv1 of a strided block runs on the input map
    return H // s, W // s


# ------------------------------------------------------------------------------------------------------------ branches
# name -> case, launch precision, plan attributes: the other branches of run().  ``expected_entry`` says from the docstrings of
# DenseNetHip / ResNetHip and the plan queries (host arithmetic, at FILL_BRANCH) which entry point each launch takes
BRANCHES = OrderedDict([
    ("d161_bf16", dict(case="d161", precision="bf16", attrs={})),
    ("d161_bf16_wide", dict(case="d161", precision="bf16", attrs=dict(bf16_wide_1x1=True))),
    ("d161_bf16_all", dict(case="d161", precision="bf16", attrs=dict(bf16_wide_1x1="all"))),
    ("d121_bf16_wide", dict(case="d121", precision="bf16", attrs=dict(bf16_wide_1x1=True))),
    ("d121_bf16_all", dict(case="d121", precision="bf16", attrs=dict(bf16_wide_1x1="all"))),
    ("d161_bf16_mid", dict(case="d161_wide", precision="bf16", attrs=dict(bf16_wide_1x1=True, bf16_mid_storage=True))),
    ("d161_bf16x3_inert", dict(case="d161", precision="bf16x3", attrs=dict(bf16_wide_1x1="all", bf16_mid_storage=True))),
    ("r1111_bf16", dict(case="r1111", precision="bf16", attrs={})),
    ("r1111_bf16_wide", dict(case="r1111", precision="bf16", attrs=dict(bf16_wide_1x1=True))),
    ("r3211_bf16_wide", dict(case="r3211", precision="bf16", attrs=dict(bf16_wide_1x1=True))),
    ("rx4_native", dict(case="rx4", precision="fp32", attrs=dict(grouped_conv="native"))),
    ("rx4_auto", dict(case="rx4", precision="fp32", attrs=dict(grouped_conv="auto"))),
    ("rx8_native", dict(case="rx8", precision="fp32", attrs=dict(grouped_conv="native"))),
    ("rx8_auto", dict(case="rx8", precision="fp32", attrs=dict(grouped_conv="auto"))),
    ("rx4_bf16_native_ignored", dict(case="rx4", precision="bf16", attrs=dict(grouped_conv="native"))),
    ("rx4_bf16_auto_ignored", dict(case="rx4", precision="bf16", attrs=dict(grouped_conv="auto"))),
])
ENTRIES = ("conv_forward", "wide192", "wide192_bf16", "bf16in_3x3", "wide", "grouped")


def entry_of_kernel(kern):
    """The entry point a KernelTrace kernel name belongs to."""
    if kern.startswith("conv1x1_bf16_ybf16_kernel"):
        return "wide192_bf16"
    if kern.startswith("conv1x1_bf16_kernel"):
        return "wide*"                                           # both wide entry points launch this kernel family
    if kern.startswith("conv3x3_bf16in_kernel"):
        return "bf16in_3x3"
    if kern.startswith("conv_grouped_kernel"):
        return "grouped"
    return "conv_forward"


def expected_launches(branch):
    """[(tag, entry, why)] of every convolution launch of the branch, in launch order.  ``why`` names the rule of the
    docstrings that keeps a layer on conv_forward ("" where nothing does)."""
    from bts_amd import ops
    b = BRANCHES[branch]
    c = case(b["case"])
    a = b["attrs"]
    bf16 = b["precision"] == "bf16"
    out = [("enc_stem", "conv_forward", "stem")]
    ff = FILL_BRANCH
    if c.kind == "densenet":
        f = c.model
        wide = a.get("bf16_wide_1x1", False) if bf16 else False
        blocks = [m for n, m in f.named_children() if n.startswith("denseblock")]
        c_mid = next(iter(blocks[0].values())).conv1.out_channels
        growth = blocks[0].growth_rate
        for bi, blk in enumerate(blocks):
            h, w = c.H >> (bi + 2), c.W >> (bi + 2)
            tag = "enc_b%d" % (bi + 1)
            mid16 = bool(a.get("bf16_mid_storage")) and bool(wide) and ops.conv3x3_bf16in_plan(h, w, c_mid, growth, fill_frames=ff).eligible
            for layer in blk.values():
                cin = layer.conv1.in_channels
                if wide and ops.conv1x1_bf16_plan(h, w, cin, c_mid, fill_frames=ff).eligible:
                    if mid16:
                        out += [(tag + "_1x1_mid16", "wide192_bf16", ""), (tag + "_3x3_mid16", "bf16in_3x3", "")]
                        continue
                    out.append((tag + "_1x1", "wide192", ""))
                elif wide == "all" and ops.conv1x1_bf16_wide_plan(h, w, cin, c_mid, fill_frames=ff).eligible:
                    out.append((tag + "_1x1", "wide", ""))
                else:
                    why = "" if not wide else ("c_in % 16" if cin % 16 else "width" if c_mid % 192 and wide is True else "plan")
                    out.append((tag + "_1x1", "conv_forward", why))
                out.append((tag + "_3x3", "conv_forward", ""))
            if bi < 3:
                out.append(("enc_trans", "conv_forward", "transition" if wide else ""))
        return out
    m = c.model
    wide = bool(a.get("bf16_wide_1x1")) and bf16
    mode = a.get("grouped_conv", "bundles")
    h, w = c.H // 4, c.W // 4
    c_cur = m.conv1.out_channels

    def one_by_one(tag, hh, ww, cin, cout, why_not="", has_res=False):
        if wide and not why_not and cin % 16 == 0 and ops.conv1x1_bf16_wide_plan(hh, ww, cin, cout, has_res=has_res, fill_frames=ff).eligible:
            return (tag, "wide", "")
        if wide and not why_not:
            why_not = "width" if (cout % 128 and cout % 192) else "plan"
        return (tag, "conv_forward", why_not if wide else "")

    for li, layer in enumerate((m.layer1, m.layer2, m.layer3, m.layer4)):
        tag = "enc_l%d" % (li + 1)
        for blk in layer:
            s, width, g = blk.conv2.stride[0], blk.conv2.out_channels, blk.conv2.groups
            ho, wo = h // s, w // s
            out.append(one_by_one(tag + "_1x1", h, w, c_cur, width))
            if g > 1:
                cg = width // g
                why = ("precision" if b["precision"] != "fp32" else "stride 2" if s != 1 else "channels per group" if cg > 16
                       else "width % 64" if width % 64 else "")
                native = mode != "bundles" and not why and (mode == "native" or ops.conv_grouped_plan(
                    h, w, width, g, precision=0, fill_frames=ff).eligible)
                out.append((tag + "_g3x3", "grouped" if native else "conv_forward", why if mode != "bundles" else ""))
            else:
                out.append((tag + "_3x3", "conv_forward", ""))
            if blk.downsample is not None:
                out.append(one_by_one(tag + "_down", h, w, c_cur, blk.conv3.out_channels, "stride 2" if s != 1 else ""))
            out.append(one_by_one(tag + "_1x1", ho, wo, width, blk.conv3.out_channels, has_res=True))
            c_cur, h, w = blk.conv3.out_channels, ho, wo
    return out


# ------------------------------------------------------------------------------------------------- bf16 operand rounding
def bf16_round(t):
    """Nearest-even bf16 rounding of an fp32 / fp64-held-fp32 tensor, returned in fp64."""
    return t.float().to(torch.bfloat16).double()


def fold32(bn):
    """ops.bn_affine's own fp32 steps on the CPU (IEEE square root and division: the bits the GPU folds)."""
    invstd = 1.0 / torch.sqrt(bn.running_var.float() + bn.eps)
    scale = bn.weight.detach().float() * invstd
    return scale, bn.bias.detach().float() - bn.running_mean.float() * scale


def conv_bf16_node(x, conv, pre=None, post=None, relu=True, res=None):
    """The bf16 mode's statement of one launch (tests/test_bf16_gpu.py, tests/test_conv1x1_bf16_gpu.py): the fp32 prologue
    relu(x s + t) in one rounding, both operands rounded to bf16 (nearest even), exact products summed in fp32, the epilogue in
    fp32.  ``conv`` / ``pre`` / ``post``: the fp32 modules.  Returns (ref, mag): the fp64 value on the rounded operands and
    sum |terms| carried through the epilogue, for |got - ref| <= 2e-6 mag + 2^-22 |ref|."""
    p = x.double()
    with torch.no_grad():
        if pre is not None:
            s, t = fold32(pre)
            p = F.relu((p * _v(s.double()) + _v(t.double())).float()).double()      # one rounding, as an FMA gives
        p = bf16_round(p)
        wq = bf16_round(conv.weight.detach())
        acc = F.conv2d(p, wq, None, conv.stride, conv.padding, conv.dilation, conv.groups)
        mag = F.conv2d(p.abs(), wq.abs(), None, conv.stride, conv.padding, conv.dilation, conv.groups)
        y = acc
        if post is not None:
            s, t = fold32(post)
            y = acc * _v(s.double()) + _v(t.double())
            mag = mag * _v(s.double().abs()) + _v(t.double().abs())
        if res is not None:
            y = y + res.double()
            mag = mag + res.double().abs()
    return (F.relu(y) if relu else y), mag


def bf16_check(got, ref, mag, extra=None):
    """max |got - ref| / (2e-6 mag + 2^-22 |ref| [+ extra])."""
    bound = 2e-6 * mag + 2.0 ** -22 * ref.abs()
    if extra is not None:
        bound = bound + extra
    got = got.double()
    return float(((got - ref).abs() / bound.clamp_min(1e-300)).max()) if bool(torch.isfinite(got).all()) else float("inf")
