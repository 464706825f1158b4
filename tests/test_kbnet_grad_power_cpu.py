"""CPU: the gate of the depth network's backward tests rejects the mistakes a backward pass of this network can make.  Each is
planted in the fp64 oracle (a keyword of kbnet_grad_oracle.forward) on a narrow case and compared with the unplanted fp64 oracle:
some parameter's gradient must leave the gate, by a wide margin; without a mistake the same comparison is exact."""
import pytest
import torch

import kbnet_grad_cases as cases
import kbnet_grad_oracle as kgo

# mistake -> (case, a parameter whose gradient it must spoil)
PLANTED = {
    "drop_skip_depth": ("kbnet_grad_kitti_odd", "enc::calibrated_backprojection1.conv_depth.conv_block.0.conv.weight"),
    "drop_fused_xyz": ("kbnet_grad_kitti_odd", "enc::calibrated_backprojection1.proj_depth.conv.weight"),
    "xyz_without_act_grad": ("kbnet_grad_kitti_odd", "enc::calibrated_backprojection1.proj_depth.conv.weight"),
    "resize_one_pixel": ("kbnet_grad_kitti_odd", "dec::deconv1.conv.conv.weight"),
    "depth_map_without_sigmoid_grad": ("kbnet_grad_kitti_odd", "dec::output0.conv.weight"),
    "fused_slice_offset": ("kbnet_grad_kitti_odd", "enc::calibrated_backprojection1.conv_fused.conv.weight"),
    "second_use_not_accumulated": ("level4_listed", "enc::calibrated_backprojection4.conv_fused.conv.weight"),
}
MARGIN = 10.0     # a planted mistake leaves the gate by at least this factor


@pytest.fixture(scope="module")
def clean():
    out = {}
    for name in {case for case, _ in PLANTED.values()}:
        c = cases.MODEL[name]
        args = cases.inputs(c)
        out[name] = (c, args, kgo.gradients(*args, c["cfg"]))
    return out


def test_every_mistake_of_the_oracle_is_planted():
    assert sorted(list(PLANTED) + ["resize_half_map"]) == sorted(kgo.MISTAKES)


def test_without_a_mistake_the_comparison_is_exact(clean):
    for name, (c, args, want) in clean.items():
        got = kgo.gradients(*args, c["cfg"], masks=kgo.masks_of(want["pre"]))
        assert all(torch.equal(got[k], want[k]) for k in kgo.gradient_keys(want)), name


@pytest.mark.parametrize("mistake", list(PLANTED))
def test_the_gate_rejects(clean, mistake):
    name, where = PLANTED[mistake]
    c, args, want = clean[name]
    got = kgo.gradients(*args, c["cfg"], **{mistake: True})
    assert torch.equal(got["depth"], want["depth"])          # the forward is untouched: only a gradient test can see it
    keys = kgo.gradient_keys(want)
    assert set(kgo.gradient_keys(got)) <= set(keys)
    # (a dropped path can leave a parameter without any gradient: that counts as zeros)
    figures = {k: kgo.fraction(got.get(k, torch.zeros_like(want[k])), want[k]) for k in keys}
    worst = max(figures, key=figures.get)
    print(f"{mistake}: worst {figures[worst]:.2e} at {worst}; {where} {figures[where]:.2e} (gate {kgo.TOL:.0e})")
    assert figures[where] > MARGIN * kgo.TOL, (mistake, where, figures[where])
    assert figures[worst] > MARGIN * kgo.TOL


def test_the_gate_rejects_a_halving_resize_map_where_it_differs_from_torchs():
    """dst // 2 instead of torch's rule.  Inside KBNet's decoder every resize has H in {2h - 1, 2h} and W in {2w - 1, 2w} (a skip is
    the ceil-half of the map below it), and for those sizes dst // 2 IS torch's rule -- asserted here -- so no network case can see this
    mistake, odd sizes included.  A free size can, deconv0's `shape` or the operator test's (2, 3) -> (7, 8): there the gate rejects it."""
    for h in range(1, 40):
        for H in (2 * h - 1, 2 * h):
            assert torch.equal(kgo.nearest_map(h, H), (torch.arange(H) // 2).clamp(max=h - 1)), (h, H)
    c = cases.MODEL["kbnet_grad_kitti_odd"]
    args = cases.inputs(c)
    want, got = kgo.gradients(*args, c["cfg"]), kgo.gradients(*args, c["cfg"], resize_half_map=True)
    assert all(torch.equal(got[k], want[k]) for k in kgo.gradient_keys(want))
    g = torch.Generator().manual_seed(3)
    grad = torch.randn(2, 3, 7, 8, generator=g, dtype=torch.float64)
    grads = []
    for half_map in (False, True):
        x = torch.zeros(2, 3, 2, 3, dtype=torch.float64, requires_grad=True)
        kgo._Resize.apply(x, 7, 8, False, half_map).backward(grad)
        grads.append(x.grad)
    figure = kgo.fraction(grads[1], grads[0])
    print(f"resize_half_map at (2, 3) -> (7, 8): {figure:.2e} (gate {kgo.TOL:.0e})")
    assert figure > MARGIN * kgo.TOL
