"""CPU: tests/kbnet_grad_oracle.py against oracle/kbnet_oracle.py (forward, fp32, bit for bit), against the reference's own autograd
(tests/golden/kbnet_grad_*.npz), and the measurement behind its gate."""
import math

import pytest
import torch

import kbnet_amd as kb
import kbnet_grad_cases as cases
import kbnet_grad_oracle as kgo
from oracle import kbnet_oracle as orc

CEILING = 1e-3      # the loss backward's gate


def test_the_kitti_preset_has_34_activations():
    names = kgo.activation_names(kb.kitti_config().resolutions_backprojection)
    assert len(names) == 34 == len(set(names))
    assert len(kgo.activation_names((0, 2))) == 30 and len(kgo.activation_names((0, 1, 2, 3, 4))) == 36


@pytest.mark.parametrize("name", list(cases.MODEL))
def test_fp32_forward_is_the_forward_oracle_bit_for_bit(name):
    c = cases.MODEL[name]
    cfg = c["cfg"]
    args = cases.inputs(c)
    with torch.no_grad():
        out = kgo.forward(*args[:7], cfg)
    want = orc.kbnet_forward(*args[:7], cfg.min_pools, cfg.max_pools, cfg.min_predict_depth, cfg.max_predict_depth,
                             cfg.resolutions_backprojection, orc.activation_slope(cfg.activation_func))
    assert out["depth"].dtype == torch.float32 and torch.equal(out["depth"], want)
    assert list(out["pre"]) == kgo.activation_names(cfg.resolutions_backprojection, cfg.n_convolution_sparse_to_dense_pool)
    assert 0.02 < float(out["logits"].abs().max()) < 30.0      # the depth mapping is neither flat nor saturated


def test_resize_of_the_oracle_is_torchs_in_both_directions():
    x = torch.randn(2, 3, 5, 7, dtype=torch.float64, requires_grad=True)
    y = torch.randn(2, 3, 5, 7, dtype=torch.float64)
    y.data.copy_(x.data)
    y.requires_grad_(True)
    g = torch.randn(2, 3, 9, 20, dtype=torch.float64)
    a = kgo._Resize.apply(x, 9, 20, False, False)
    b = torch.nn.functional.interpolate(y, size=(9, 20), mode="nearest")
    assert torch.equal(a, b)
    a.backward(g)
    b.backward(g)
    assert float((x.grad - y.grad).abs().max()) <= 1e-15 * float(y.grad.abs().max())


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_oracle_against_the_references_autograd(name):
    c = cases.GOLDEN[name]
    gold = cases.golden(name)
    args = cases.inputs(c)
    for k, v in cases.checksums(*args[:7]).items():
        assert float(gold["sum::" + k]) == v, k          # the regenerated inputs are the generator's
    assert torch.equal(gold["cotangent"], args[7]) and int(gold["seed"]) == c["seed"]
    got = kgo.gradients(*args, c["cfg"])
    keys = kgo.gradient_keys(gold)
    assert sorted(keys) == sorted(kgo.gradient_keys(got))
    # a parameter the forward never touches has no gradient, in the reference's autograd and here
    absent = sorted(set(kgo.parameter_keys(*args[4:7])) - set(keys))
    assert absent == sorted(cases.untouched(c)) and len(absent) == {"kbnet_grad_kitti_odd": 1, "kbnet_grad_relu_kb02": 2}[name]
    for k in keys + ["depth"]:
        assert float((got[k] - gold[k]).abs().max()) <= 1e-9 * float(gold[k].abs().max()), k


@pytest.mark.parametrize("name", list(cases.MODEL))
def test_parameters_without_a_gradient(name):
    c = cases.MODEL[name]
    args = cases.inputs(c)
    got = kgo.gradients(*args, c["cfg"])
    absent = sorted(set(kgo.parameter_keys(*args[4:7])) - set(kgo.gradient_keys(got)))
    assert absent == sorted(cases.untouched(c))
    assert len(absent) == {"level4_listed": 4, "kbnet_grad_relu_kb02": 2, "linear": 1}.get(name, 1)
    for k in kgo.gradient_keys(got):
        assert torch.isfinite(got[k]).all() and float(got[k].abs().max()) > 0, k


@pytest.fixture(scope="module")
def measured():
    """Per case: the worst fraction of the oracle's fp32 autograd against its fp64 autograd, both on the branches of the fp32
    forward, the tensor it sits at, and the number of activations whose fp32 branch differs from fp64's."""
    out = {}
    for name, c in cases.MODEL.items():
        masks = cases.fp32_masks(c)
        args = cases.inputs(c)
        o64 = kgo.gradients(*args, c["cfg"], masks=masks)
        kinks = kgo.check_kinks(masks, o64["pre"])
        o32 = kgo.gradients(*args, c["cfg"], dtype=torch.float32, masks=masks)
        figures = {k: kgo.fraction(o32[k], o64[k]) for k in kgo.gradient_keys(o64)}
        worst = max(figures, key=figures.get)
        out[name] = (figures[worst], worst, kinks)
        print(f"{name}: fp32 autograd at {figures[worst]:.2e} of |b| + rms(b) ({worst}); {kinks} branches on the other side of the kink")
    return out


def test_the_gate_is_three_times_the_fp32_oracles_own_error(measured):
    worst = max(v[0] for v in measured.values())
    digit = 10.0 ** math.floor(math.log10(3.0 * worst))
    assert kgo.TOL == pytest.approx(math.ceil(3.0 * worst / digit) * digit, rel=1e-12), (worst, kgo.TOL)
    assert kgo.TOL <= CEILING


def test_every_case_is_well_conditioned(measured):
    for name, (figure, where, kinks) in measured.items():
        assert 3.0 * figure <= CEILING, (name, figure, where)
        assert kinks == 0, name      # kink_check holds for the reference alone: no fp32 branch differs from fp64's


@pytest.mark.parametrize("name", ["tiny_n3", "tiny_n5"])
def test_frame_axis_cases_keep_the_seed_rule(measured, name):
    """The rule written in resnet_pose_grad_cases.py: (a) the oracle's own fp32 autograd under a third of the gate (measured: 1.3e-5
    and 7.3e-6), (b) no activation with more fp64 pre-activations near 0 than kink_check lets flip."""
    c = cases.MODEL[name]
    assert c["n"] in (3, 5)
    figure, where, kinks = measured[name]
    assert 3.0 * figure <= kgo.TOL and kinks == 0, (name, figure, where, kinks)
    pre = kgo.gradients(*cases.inputs(c), c["cfg"])["pre"]
    kgo.kink_room(pre.values())


def test_the_depth_mappings_gate_is_three_times_torchs_fp32_autograd():
    logits, g = cases.depth_map_inputs()
    assert float(logits.min()) == -30.0 and float(logits.max()) == 30.0 and torch.equal(logits, logits.float().double())
    worst = 0.0
    for cfg in (kb.kitti_config(), kb.void_config()):
        grads = []
        for dtype in (torch.float64, torch.float32):
            leaf = logits.to(dtype).clone().requires_grad_(True)
            depth = cfg.min_predict_depth / (torch.sigmoid(leaf) + cfg.min_predict_depth / cfg.max_predict_depth)
            depth.backward(g.to(dtype))
            grads.append(leaf.grad)
        figure = kgo.fraction(grads[1], grads[0])
        print(f"depth mapping [{cfg.min_predict_depth}, {cfg.max_predict_depth}]: torch's fp32 autograd at {figure:.2e} of |b| + rms(b)")
        worst = max(worst, figure)
    digit = 10.0 ** math.floor(math.log10(3.0 * worst))
    assert kgo.DEPTH_MAP_TOL == pytest.approx(math.ceil(3.0 * worst / digit) * digit, rel=1e-12), (worst, kgo.DEPTH_MAP_TOL)
