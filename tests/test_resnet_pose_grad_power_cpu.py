"""CPU: proof that the gate of the ResNet pose networks' backward tests sees the mistakes a backward pass of this network can
make -- each planted in tests/resnet_pose_grad_oracle.py (or, for the pool's tie rule, in the operator's own reference) fails the
gate by a wide factor on a tensor named here."""
import pytest
import torch

import posenet_oracle as po
import resnet_pose_grad_cases as cases
import resnet_pose_grad_oracle as rgo

WIDE = 100.0      # times the gate


@pytest.fixture(scope="module")
def train_case():
    c = cases.GOLDEN["resnet_pose_grad_18_train"]
    inputs = cases.inputs(c)
    return inputs, rgo.gradients(*inputs, n_layer=18, batch_norm="batch")


def _figures(good, bad):
    return {k: (rgo.fraction(bad[k], good[k]) if k in bad else float("inf")) for k in rgo.gradient_keys(good)}


@pytest.mark.parametrize("mistake, tensor, still_right", [
    (dict(drop_skip_grad=True), "enc::blocks2.1.conv1.conv.weight", "dec::conv.2.conv.weight"),
    (dict(drop_projection_grad=True), "enc::blocks3.0.projection.conv.weight", "enc::conv1.conv.weight"),
    (dict(conv2_act_in_backward=False), "enc::blocks2.0.conv2.conv.weight", "dec::conv.2.conv.weight"),
    (dict(detach_stats=True), "enc::conv1.conv.weight", "dec::conv.2.conv.weight"),
], ids=lambda v: next(iter(v)) if isinstance(v, dict) else None)
def test_planted_mistake_fails_the_gate(train_case, mistake, tensor, still_right):
    inputs, good = train_case
    bad = rgo.gradients(*inputs, n_layer=18, batch_norm="batch", **mistake)
    figures = _figures(good, bad)
    print(f"{mistake}: {tensor} at {figures[tensor]:.2e} (gate {rgo.TOL:.0e}); {sum(v > rgo.TOL for v in figures.values())} of "
          f"{len(figures)} tensors fail")
    assert figures[tensor] > WIDE * rgo.TOL, (mistake, tensor, figures[tensor])
    assert figures[still_right] <= rgo.TOL        # the mistake is where it was planted, not everywhere
    assert rgo.fraction(bad["dof"], good["dof"]) < 1e-12     # the forward is untouched: only a gradient test sees these


def test_dropping_the_skips_gradient_leaves_the_projections_without_one(train_case):
    inputs, good = train_case
    bad = rgo.gradients(*inputs, n_layer=18, batch_norm="batch", drop_skip_grad=True)
    assert "enc::blocks3.0.projection.conv.weight" in good and "enc::blocks3.0.projection.conv.weight" not in bad


def test_the_biased_running_variance_fails_the_statistics_rule(train_case):
    inputs, good = train_case
    bad = rgo.gradients(*inputs, n_layer=18, batch_norm="batch", biased_running_var=True)
    key = "run::dec::conv.1.batch_norm.running_var"      # 8 values per channel: 8 / 7 of the biased variance
    f = po.gate_fraction(bad[key].float(), good[key], po.layer_floor(good[key]))
    print(f"biased running variance: {key} at {f:.2f} of the 1e-4 rule")
    assert f > 5.0
    key = "run::enc::conv1.batch_norm.running_var"       # 8840 values: 1.0001 of it, times the momentum: inside the rule
    assert po.gate_fraction(bad[key].float(), good[key], po.layer_floor(good[key])) <= 1.0
    assert max(_figures(good, bad).values()) == 0.0      # no gradient sees it


def test_the_pools_tie_rule_is_invisible_in_the_model_and_fails_the_operators_gate(train_case):
    """Behind leaky_relu no window ties; behind relu the ties are exact zeros whose activation passes no gradient on: the model's
    gradients cannot tell the first maximum from the last.  The operator test can: its inputs are quantised to three levels, and
    its bound per element is 4 x 2^-24 x the sum of |g| over the windows routed to it."""
    inputs, _ = train_case
    for slope in (0.2, 0.0):
        good = rgo.gradients(*inputs, n_layer=18, batch_norm="batch", slope=slope)
        bad = rgo.gradients(*inputs, n_layer=18, batch_norm="batch", slope=slope, pool_last_max=True)
        assert max(_figures(good, bad).values()) == 0.0
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 3, (2, 3, 5, 7), generator=g).double().requires_grad_(True)
    grad = torch.randn(2, 3, 3, 4, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(torch.nn.functional.max_pool2d(x, 3, stride=2, padding=1), x, grad)
    (routed,) = torch.autograd.grad(torch.nn.functional.max_pool2d(x, 3, stride=2, padding=1), x, grad.abs())
    leaf = x.detach().clone().requires_grad_(True)
    (got,) = torch.autograd.grad(rgo.pool(leaf, rgo.pool_argmax(leaf.detach(), last=True)), leaf, grad)
    bound = 4.0 * 2.0 ** -24 * routed
    assert int(((got - want).abs() > bound).sum()) > 10
    leaf = x.detach().clone().requires_grad_(True)
    (same,) = torch.autograd.grad(rgo.pool(leaf, rgo.pool_argmax(leaf.detach())), leaf, grad)
    assert bool(((same - want).abs() <= bound).all())
