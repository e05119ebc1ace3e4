"""CPU side of the encoder-node checks (tests/enc_node_cases.py): the tables reach every node kind and every branch of
DenseNetHip.run / ResNetHip.run (asked of the plan queries, item by item, so a dispatch change that moves a layer off an entry
point fails by name), the stored floors are what this CPU measures, the references are what they claim to be, and the derived
bound of every node is neither vacuous nor too tight."""
import copy

import pytest
import torch

import enc_node_cases as T

ALL = list(T.CASES)


@pytest.mark.parametrize("name", ALL)
def test_every_width_is_a_multiple_of_4(name):
    c = T.case(name)
    assert c.H % 32 == 0 and c.W % 32 == 0
    assert [w for w in T.widths(c.model) if w % 4] == []


def test_the_networks_are_the_ones_the_issue_names():
    d161, d121 = T.case("d161").model, T.case("d121").model
    cins = [L.conv1.in_channels for n, b in d161.named_children() if n.startswith("denseblock") for L in b.values()]
    assert max(len(b) for n, b in d161.named_children() if n.startswith("denseblock")) >= 4
    assert d161.denseblock1.growth_rate == 48 and d161.conv0.out_channels == 96 and d161.denseblock1.denselayer1.conv1.out_channels == 192
    assert 144 in cins and 120 in cins and 144 % 32 and 120 % 16
    assert d121.denseblock1.growth_rate == 32 and d121.conv0.out_channels == 64 and d121.denseblock1.denselayer1.conv1.out_channels == 128
    assert [len(getattr(T.case("r1111").model, "layer%d" % i)) for i in (1, 2, 3, 4)] == [1, 1, 1, 1]
    assert sorted(len(getattr(T.case("r3211").model, "layer%d" % i)) for i in (1, 2, 3, 4))[-2:] == [2, 3]
    assert {T.case(n).model.base_width for n in ("rx4", "rx8")} == {4, 8} and T.case("rx4").model.groups == 32
    shapes = {(c.B, c.H, c.W) for c in map(T.case, ALL)}
    assert (2, 32, 64) in shapes and (1, 64, 32) in shapes


@pytest.mark.parametrize("name", ALL)
def test_the_walk_is_the_modules_own_forward(name):
    """The tensors of ``walk`` come from whole-module forwards; its last one is what the network itself returns."""
    c = T.case(name)
    ref = T.reference(name)
    model = copy.deepcopy(c.model).double()
    with torch.no_grad():
        if c.kind == "densenet":
            assert torch.equal(model(c.x.double()), ref["norm5"])
        else:
            y = model.maxpool(model.relu(model.bn1(model.conv1(c.x.double()))))
            assert torch.equal(model.layer4(model.layer3(model.layer2(model.layer1(y)))), ref["l3b%d" % (len(model.layer4) - 1)])
    assert set(T.survivors(c)) <= set(ref) and set(T.FLOORS[name]) == set(ref) - {"img"}
    for n in T.nodes(name):                                      # a node's buffers are buffers a forward leaves behind
        for r in (n.src, n.dst, n.res):
            assert r is None or r[0] == "img" or r[0] in T.survivors(c), (n.name, r)
        assert n.skip is None or n.skip in T.survivors(c)


def test_the_table_reaches_every_node_kind():
    reached = {n.kind for name in ALL for n in T.nodes(name)}
    assert [k for k in T.NODE_KINDS if k not in reached] == []
    # a transition with and one without the skip tap, a pool with one and with two destinations
    skips = {(n.kind, n.skip is not None) for name in ALL for n in T.nodes(name)}
    assert {("transition_skip", True), ("transition_noskip", False), ("maxpool_2dst", True), ("maxpool_1dst", False)} <= skips


def _entries(branch):
    return {(e, why) for _, e, why in T.expected_launches(branch)}


# item -> (branch, (entry, why)): what the dispatch must keep choosing at FILL_BRANCH for the GPU file to test it
REACH = {
    "DenseNet bottleneck on the 192-wide bf16 tile": ("d161_bf16_wide", ("wide192", "")),
    "... not where c_in % 16 != 0": ("d161_bf16_wide", ("conv_forward", "c_in % 16")),
    "... not the transitions": ("d161_bf16_wide", ("conv_forward", "transition")),
    "... not DenseNet121's 128-wide bottlenecks under True": ("d121_bf16_wide", ("conv_forward", "width")),
    "DenseNet121 bottleneck on the wide tile under \"all\"": ("d121_bf16_all", ("wide", "")),
    "\"all\" keeps the 192-wide tile where it is eligible": ("d161_bf16_all", ("wide192", "")),
    "bf16 mid: the producer": ("d161_bf16_mid", ("wide192_bf16", "")),
    "bf16 mid: the consumer": ("d161_bf16_mid", ("bf16in_3x3", "")),
    "bf16 mid: a block that keeps the fp32 mid": ("d161_bf16_mid", ("wide192", "")),
    "ResNet 1x1 on the wide tile": ("r1111_bf16_wide", ("wide", "")),
    "... not a stride-2 downsample": ("r1111_bf16_wide", ("conv_forward", "stride 2")),
    "... not the 64-wide conv1": ("r1111_bf16_wide", ("conv_forward", "width")),
    "native grouped 3x3, 4 channels per group": ("rx4_native", ("grouped", "")),
    "native grouped 3x3, width_per_group 8": ("rx8_native", ("grouped", "")),
    "native grouped 3x3 under \"auto\", width_per_group 4": ("rx4_auto", ("grouped", "")),
    "native grouped 3x3 under \"auto\", width_per_group 8": ("rx8_auto", ("grouped", "")),
    "... not a stride-2 block": ("rx4_native", ("conv_forward", "stride 2")),
    "... not 32 channels per group": ("rx8_native", ("conv_forward", "channels per group")),
    "... not under the bf16 precision": ("rx4_bf16_native_ignored", ("conv_forward", "precision")),
}


@pytest.mark.parametrize("item", list(REACH))
def test_the_table_reaches_every_branch(item):
    branch, want = REACH[item]
    assert want in _entries(branch), "%s: branch %s no longer has a launch on %s" % (item, branch, want)


def test_inert_branches_expect_conv_forward_only():
    for branch in ("d161_bf16", "d161_bf16x3_inert", "r1111_bf16", "rx4_bf16_native_ignored", "rx4_bf16_auto_ignored"):
        assert {e for e, _ in _entries(branch)} == {"conv_forward"}, branch
    assert set(T.ENTRIES) == {e for b in T.BRANCHES for e, _ in _entries(b)}


def test_the_native_grouped_layers_are_checkable_nodes():
    """The bundled and the native grouped 3x3 each stand in front of a node with its input and output alive."""
    for branch in ("rx4_native", "rx8_native"):
        c = T.case(T.BRANCHES[branch]["case"])
        native_tags = {tag for tag, e, _ in T.expected_launches(branch) if e == "grouped"}
        nodes = [n for n in T.nodes(c.name) if n.kind == "gconv_s1"]
        assert nodes and any("enc_l%s_g3x3" % n.name.split(".")[0][5:] in native_tags for n in nodes), branch
    assert any(n.kind == "gconv_s2" for n in T.nodes("rx4"))     # always bundles


@pytest.mark.parametrize("name", ALL)
def test_stored_floors_are_what_this_cpu_measures(name):
    now = T.measure_floors(name)
    off = {k: (v, T.FLOORS[name][k]) for k, v in now.items() if not 0.5 * T.FLOORS[name][k] <= v <= 2.0 * T.FLOORS[name][k]}
    print(name, {k: float("%.3g" % v) for k, v in now.items()})
    assert not off, (name, off)


@pytest.mark.parametrize("name", ALL)
def test_the_bound_is_neither_vacuous_nor_too_tight(name):
    """From the fp32 buffers of the CPU fp32 run (the stand-in for what the GPU would have read): the CPU fp32 evaluation of
    every node -- a reference run -- stays inside the bound for every element, and each wrong reference of
    enc_node_cases.mutations (one channel's folded shift times 1.01; one growth slice rotated by a channel) leaves it."""
    c = T.case(name)
    t32 = T.walk(c, torch.float32)
    loose, tight = [], []
    for n in T.nodes(name):
        ref, bound = T.node_eval(c, n, t32)
        got, _ = T.node_eval(c, n, t32, dtype=torch.float32)
        inside = T.check(got, ref, bound)
        if not inside <= 1.0:
            tight.append((n.name, inside))
        if bound is not None:
            assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all()), n.name
        for mu in T.mutations(n):
            wrong, _ = T.node_eval(c, n, t32, mutate=mu)
            if not T.check(got, wrong, bound) > 1.0:
                loose.append((n.name, mu, T.check(got, wrong, bound)))
    assert not tight, ("the CPU fp32 evaluation leaves the bound", tight)
    assert not loose, ("a wrong reference stays inside the bound", loose)


def test_the_bf16_statement_rounds_both_operands():
    """conv_bf16_node on operands that bf16 holds exactly is the plain convolution; on others it differs at 2^-9."""
    c = T.case("d121")
    conv = c.model.transition1.conv
    x = torch.randn((1, conv.in_channels, 2, 2), generator=torch.Generator().manual_seed(3))
    ref, mag = T.conv_bf16_node(x, conv, relu=False)
    plain = torch.nn.functional.conv2d(x.double(), conv.weight.detach().double())
    assert 1e-4 < float((ref - plain).abs().max() / mag.max()) < 2.0 ** -7
    xq = x.to(torch.bfloat16).float()
    q = copy.deepcopy(conv)
    with torch.no_grad():
        q.weight.copy_(q.weight.to(torch.bfloat16).float())
    assert torch.equal(T.conv_bf16_node(xq, q, relu=False)[0], torch.nn.functional.conv2d(xq.double(), q.weight.detach().double()))
