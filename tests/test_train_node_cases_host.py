"""CPU side of the training-node checks (tests/train_node_cases.py): the stored seeds meet the kink rule, the fp32 CPU run of
every reference sits within a quarter of every bar the GPU is held to, and the references are what they claim to be."""
import numpy as np
import pytest
import torch

import train_node_cases as T

ALL = list(T.CASES)


@pytest.mark.parametrize("name", ALL)
def test_stored_seed_meets_the_kink_rule(name):
    """m >= 32 d for every run of the case whose ReLU inputs differ (plain step, norm layers frozen, second step)."""
    c = T.case(name)
    runs = [(run, T.kink(c, **kw)) for run, kw in T.kink_runs(name)]
    if name in T.STEP2_SEED:
        runs.append(("step2", T.kink(c, second_step=True)))
    for run, (m, d, n) in runs:
        if name in T.RELU_FREE_CASES:
            assert n == 0
            continue
        assert n > 0
        print("%s/%s: seed %d, %d hooked tensors, m %.3g, d %.3g, m/d %.1f" % (name, run, c.seed, n, m, d, m / d))
        assert m >= T.KINK_RATIO * d, (name, run, m, d)
        assert run in T.SEED_RATIOS[name]


def test_kink_hooks_see_every_relu():
    """Hooked tensors per case: 2 per dense layer; 3 in a bottleneck; 1 in a transition and in the stem (+ its max-pool);
    2 per atrous branch, the functional leading ReLU of a branch without first_bn included."""
    want = {"d121": 6, "d161": 4, "d121_tiny": 4, "rx_ds": 3, "rx_id": 3, "rn_ds": 3, "transition_even": 1, "transition_odd": 1,
            "stem": 2, "atrous_bn": 2, "atrous_nobn": 2, "daspp2": 4, "conv3_pattern": 0, "upconv_elu_bn": 0}
    assert {n: T.kink(T.case(n))[2] for n in ALL} == want


def _fp32_floor(name, ref32, ref64, what):
    return T.compare(name, ref32, ref64, what + ", CPU fp32 vs fp64, a quarter of the bars", scale=0.25)


@pytest.mark.parametrize("name", ALL)
def test_cpu_fp32_reference_sits_within_a_quarter_of_every_bar(name):
    _fp32_floor(name, T.reference(name, torch.float32), T.reference(name), name)
    if name in T.BN_EVAL_CASES:
        _fp32_floor(name, T.reference(name, torch.float32, bn_eval=True), T.reference(name, bn_eval=True), name + "/bn_eval")
    if name in T.STEP2_SEED:
        for i, (a, b) in enumerate(zip(T.reference_two_steps(name, torch.float32), T.reference_two_steps(name))):
            _fp32_floor(name, a, b, "%s/step%d" % (name, i + 1))


def _close(a, b, what, tol=1e-11):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300), (what, np.abs(a - b).max())


@pytest.mark.parametrize("name", T.DENSE_CASES)
def test_dense_reference_is_the_concat_of_its_layers(name):
    """The first C0 channels of the fp64 output are x; channels [Ci, Ci + g) are layer i applied to the prefix before them."""
    c = T.case(name)
    out = torch.from_numpy(T.reference(name)["out"])
    x = c.inputs["x"].double()
    C0 = x.shape[1]
    assert torch.equal(out[:, :C0], x)
    block = T.twin(c, torch.float64)
    g = block.growth_rate
    assert out.shape[1] == C0 + len(block) * g
    with torch.no_grad():
        for i, layer in enumerate(block.values()):
            Ci = C0 + i * g
            _close(out[:, Ci:Ci + g], layer(out[:, :Ci].clone()), (name, i))


@pytest.mark.parametrize("name", ["daspp2", "conv3_pattern"])
def test_second_composition_agrees(name):
    """The same function written differently (T.forward_second): output, every gradient and the running statistics."""
    c = T.case(name)
    ref = T.reference(name)
    other = T.reference_step(c, T.twin(c, torch.float64), forward=T.forward_second)
    keys = [k for k in ref if not k.endswith("num_batches_tracked")]
    assert set(k for k in other if not k.endswith("num_batches_tracked")) == set(keys)
    for k in keys:
        _close(other[k], ref[k], (name, k))


def test_conv3_pattern_gradient_lands_on_the_strided_positions():
    gd = T.reference("conv3_pattern")["grad:d"]
    on = np.zeros(gd.shape, dtype=bool)
    on[:, :, ::4, ::4] = True
    assert (gd[~on] == 0).all() and (gd[on] != 0).all()


def test_stem_image_gets_no_gradient():
    ref = T.reference("stem")
    assert "grad:x" not in ref and "grad:conv0.weight" in ref
    assert tuple(ref["out"].shape) == (2, 64, 5, 7)


@pytest.mark.parametrize("name", ["transition_even", "transition_odd"])
def test_transition_pool_floors_the_map(name):
    h, w = T.case(name).inputs["x"].shape[2:]
    assert tuple(T.reference(name)["out"].shape) == (2, 48, h // 2, w // 2)


@pytest.mark.parametrize("name", T.DENSE_CASES)
def test_frozen_references_lose_exactly_the_frozen_gradients(name):
    full = T.reference(name)
    freeze = T.dense_freeze_set(name)
    params = [n for n, _ in T.case(name).module.named_parameters()]
    assert all(n in params for n in freeze) and len(set(freeze)) == len(freeze)
    frozen = T.reference(name, freeze=freeze)
    assert set(full) - set(frozen) == {"grad:" + n for n in freeze}
    nox = T.reference(name, input_grad=False)
    assert set(full) - set(nox) == {"grad:x"}
    for other in (frozen, nox):                    # what is still computed is the same number
        for k, v in other.items():
            _close(v, full[k], (name, k), tol=1e-12)


@pytest.mark.parametrize("name", T.BN_EVAL_CASES)
def test_norm_frozen_references_leave_the_buffers_alone(name):
    c = T.case(name)
    ref = T.reference(name, bn_eval=True)
    for n, b in c.module.named_buffers():
        assert np.array_equal(ref["buf:" + n], b.double().numpy() if b.is_floating_point() else b.numpy()), n
    plain = T.reference(name)
    assert any(not np.array_equal(plain[k], ref[k]) for k in ref if k.startswith("buf:"))
    assert T.rel_error(ref["out"], plain["out"]) > 1e-2          # another function: running, not batch, statistics


def test_two_step_reference_advances_statistics_and_counters():
    c = T.case("d121")
    first, second = T.reference_two_steps("d121")
    for n, b in c.module.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(first["buf:" + n]) == int(b) + 1 and int(second["buf:" + n]) == int(b) + 2
        else:
            assert not np.array_equal(first["buf:" + n], second["buf:" + n])
    assert T.rel_error(second["grad:x"], first["grad:x"]) > 1e-2
    vals = c.step2_values()
    assert all(v.dtype == torch.float32 and not torch.equal(v, p) for (_, p), v in zip(c.module.named_parameters(), vals.values()))
