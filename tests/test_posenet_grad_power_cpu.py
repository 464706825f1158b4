"""Proof that the gate of the pose network's backward tests (posenet_grad_oracle.TOL) rejects the mistakes such a backward
pass can make, each planted in the oracle on the GPU tests' own cases (the role tests/test_loss_grad_power_cpu.py has for the loss)."""
import pytest
import torch

import posenet_grad_cases as cases
import posenet_grad_oracle as pgo
import posenet_oracle as po

TRAIN = cases.GOLDEN["posenet_grad_train"]


@pytest.fixture(scope="module")
def train_case():
    inputs = cases.inputs(TRAIN)
    return inputs, pgo.gradients(*inputs, batch_norm="batch")


def failing(got, want):
    return [k for k in want if k.startswith(("enc::", "dec::")) and not pgo.passes(got[k], want[k])]


def test_the_unplanted_oracle_passes(train_case):
    inputs, want = train_case
    assert failing(pgo.gradients(*inputs, batch_norm="batch"), want) == []


def test_batch_statistics_treated_as_constants(train_case):
    inputs, want = train_case
    bad = failing(pgo.gradients(*inputs, batch_norm="batch", detach_stats=True), want)
    assert len(bad) >= 7, bad          # every conv weight at least


def test_biased_running_variance(train_case):
    inputs, want = train_case
    got = pgo.gradients(*inputs, batch_norm="batch", biased_running_var=True)
    bad = [k for k in want if k.endswith("running_var") and po.gate_fraction(got[k], want[k], po.layer_floor(want[k])) > 1.0]
    assert "run::conv7.batch_norm.running_var" in bad and len(bad) >= 3, bad     # the maps of few values show it


def test_head_factor_dropped(train_case):
    inputs, want = train_case
    got = pgo.gradients(*inputs, batch_norm="batch", factor=1.0)
    assert not pgo.passes(got["dof"], want["dof"])
    assert failing(got, want)


@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_slope_branch_at_exactly_zero(slope):
    c = cases.bn_case(slope, False, zeros=True)
    assert int((c["z"] == 0).sum()) >= 3 * 5 * 12
    u = c["u"].clone().requires_grad_(True)
    y, _, _, _ = pgo.batch_norm_act(u, c["gamma"], c["beta"], c["mean"], c["var"], slope=slope, slope_at_zero=True)
    (bad,) = torch.autograd.grad(y, [u], c["grad_y"])
    assert not pgo.passes(bad, c["grad_u"])


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("shape", cases.CONV_SHAPES[2:4])
def test_data_gradient_parity_swapped_and_padding(shape, k):
    xs, weight, grad_out, grad_xs, _ = cases.conv_case(*shape, k)
    h, w = xs[0].shape[2:]
    want = torch.cat(grad_xs, 1)
    assert pgo.fraction(pgo.conv_backward_data(grad_out, weight, h, w), want) < 1e-12       # the written-out form is the gradient
    assert not pgo.passes(pgo.conv_backward_data(grad_out, weight, h, w, swap_parity=True), want)
    assert not pgo.passes(pgo.conv_backward_data(grad_out, weight, h, w, pad=k // 2 - 1), want)


@pytest.mark.parametrize("shape", cases.WGRAD_SPLIT_SHAPES + [cases.CONV_SHAPES[3] + (5,)])
def test_weight_gradient_without_its_last_partial_chunk(shape):
    xs, weight, grad_out, _, grad_w = cases.conv_case(*shape)
    x = torch.cat(xs, 1)
    assert grad_out.shape[0] * grad_out.shape[2] * grad_out.shape[3] % pgo.WG_CHUNK
    assert pgo.fraction(pgo.conv_backward_weight(x, grad_out, shape[5]), grad_w) < 1e-12
    assert not pgo.passes(pgo.conv_backward_weight(x, grad_out, shape[5], drop_last_chunk=True), grad_w)
