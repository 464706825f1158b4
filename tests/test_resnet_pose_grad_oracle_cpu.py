"""CPU: tests/resnet_pose_grad_oracle.py against the reference's own autograd (tests/golden/resnet_pose_grad_18_*.npz), the
measurement behind its gate, and what its kink_check accepts and rejects."""
import math
import os

import numpy as np
import pytest
import torch

import posenet_oracle as po
import resnet_pose_grad_cases as cases
import resnet_pose_grad_oracle as rgo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CEILING = 1e-3      # the loss backward's gate


def _golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_oracle_against_the_references_autograd(name):
    c = cases.GOLDEN[name]
    gold = _golden(name)
    image0, image1, enc, dec, cot = cases.inputs(c)
    for k, v in cases.checksums(image0, image1, enc, dec).items():
        assert float(gold["sum::" + k]) == v, k          # the regenerated inputs are the generator's
    assert torch.equal(gold["cotangent"], cot)
    got = rgo.gradients(image0, image1, enc, dec, cot, n_layer=c["n_layer"], batch_norm=c["batch_norm"])
    keys = [k for k in gold if k.startswith(("enc::", "dec::"))]
    assert sorted(keys) == sorted(rgo.gradient_keys(got)) and len(keys) == 62
    for k in cases.unused_projections(c):
        assert k not in gold and k not in got            # an identity skip leaves its projection without a gradient
    assert len(cases.unused_projections(c)) == 4
    for k in keys + ["dof", "pose"] + [k for k in gold if k.startswith("run::") and "num_batches" not in k]:
        assert float((got[k] - gold[k]).abs().max()) <= 1e-9 * float(gold[k].abs().max()), k
    for k in gold:
        if "num_batches" in k:
            assert int(got[k]) == int(gold[k]) == 1000 + (c["batch_norm"] == "batch")


@pytest.fixture(scope="module")
def measured():
    """Per model case: the worst fraction of the oracle's fp32 autograd against its fp64 autograd, both on the branches (masks,
    pool indices) of the fp32 forward, and the tensor it sits at."""
    out = {}
    for name, c in cases.MODEL.items():
        masks, indices = cases.fp32_branches(c)
        inputs = cases.inputs(c)
        kw = dict(n_layer=c["n_layer"], batch_norm=c["batch_norm"], masks=masks, pool_indices=indices)
        o64 = rgo.gradients(*inputs, **kw)
        kinks = rgo.kink_check(masks, o64["pre"], indices, o64["pool_in"])
        o32 = rgo.gradients(*inputs, dtype=torch.float32, **kw)
        figures = {k: rgo.fraction(o32[k], o64[k]) for k in rgo.gradient_keys(o64) + ["dof"]}
        worst = max(figures, key=figures.get)
        out[name] = (figures[worst], worst, kinks)
        print(f"{name}: fp32 autograd at {figures[worst]:.2e} of |b| + rms(b) ({worst}); {kinks} branches on the other side of the kink")
    return out


def test_the_gate_is_three_times_the_fp32_oracles_own_error(measured):
    worst = max(v[0] for v in measured.values())
    digit = 10.0 ** math.floor(math.log10(3.0 * worst))
    assert rgo.TOL == pytest.approx(math.ceil(3.0 * worst / digit) * digit, rel=1e-12), (worst, rgo.TOL)
    assert rgo.TOL <= CEILING


def test_every_case_is_well_conditioned(measured):
    for name, (figure, where, _) in measured.items():
        assert 3.0 * figure <= CEILING, (name, figure, where)
    for name, c in cases.MODEL.items():
        if c["batch_norm"] == "batch":
            assert cases.last_map_values(c) >= 8, name


FRAME_AXIS = ["narrow_18_n3_running", "narrow_18_n5_running", "narrow_18_n3_batch"]     # the cases with three and five frames


@pytest.mark.parametrize("name", FRAME_AXIS)
def test_frame_axis_cases_keep_the_seed_rule(measured, name):
    """The rule written in resnet_pose_grad_cases.py: (a) the oracle's own fp32 autograd under a third of the gate (measured: 1.0e-4,
    8.9e-5 and 5.8e-5), (b) no activation with more fp64 pre-activations near 0 than kink_check lets flip."""
    c = cases.MODEL[name]
    assert c["n"] in (3, 5)
    figure, where, kinks = measured[name]
    assert 3.0 * figure <= rgo.TOL and kinks == 0, (name, figure, where, kinks)
    image0, image1, enc, dec, _ = cases.inputs(c)
    with torch.no_grad():
        ref = rgo.forward(image0.double(), image1.double(), *po.to64(enc, dec), n_layer=c["n_layer"], batch_norm=c["batch_norm"])
    rgo.pgo.kink_room(ref["pre"].values())


def test_kink_check_accepts_the_fp32_branches_and_rejects_wrong_ones():
    c = cases.MODEL["narrow_34_running"]
    masks, indices = cases.fp32_branches(c)
    image0, image1, enc, dec, _ = cases.inputs(c)
    with torch.no_grad():
        ref = rgo.forward(image0.double(), image1.double(), *po.to64(enc, dec), n_layer=34)
    assert sorted(masks) == sorted(rgo.activation_names(34)) == sorted(ref["pre"])
    assert rgo.kink_check(masks, ref["pre"], indices, ref["pool_in"]) <= 2
    # an element far from 0 on the wrong branch
    z = ref["pre"]["blocks3.1.conv2"]
    at = int(z.abs().flatten().argmax())
    bad = {k: v.clone() for k, v in masks.items()}
    bad["blocks3.1.conv2"].view(-1)[at] ^= True
    with pytest.raises(AssertionError):
        rgo.kink_check(bad, ref["pre"], indices, ref["pool_in"])
    # a handful of elements flipped, every one of them close to 0: too many
    near = z.abs().flatten().argsort()[:3]
    bad = {k: v.clone() for k, v in masks.items()}
    bad["blocks3.1.conv2"].view(-1)[near] ^= True
    with pytest.raises(AssertionError):
        rgo.kink_check(bad, ref["pre"], indices, ref["pool_in"])
    # a pool window routed to a pixel that is not its maximum
    x = ref["pool_in"]
    first, last = rgo.pool_argmax(x), rgo.pool_argmax(x, last=True)
    assert torch.equal(first, last)                      # leaky_relu: no ties in this map
    wrong = first.clone()
    wrong.view(-1)[0] = first.view(-1)[0] + 1            # the window's next pixel
    with pytest.raises(AssertionError):
        rgo.kink_check(masks, ref["pre"], wrong, x)
    # a missing mask is an error, not a default
    with pytest.raises(AssertionError):
        rgo.kink_check({k: v for k, v in masks.items() if k != "conv1"}, ref["pre"], indices, x)


def test_pool_argmax_is_torchs_first_maximum_under_ties():
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 3, (2, 3, 9, 12), generator=g).double()
    _, idx = torch.nn.functional.max_pool2d(x, 3, stride=2, padding=1, return_indices=True)
    assert torch.equal(rgo.pool_argmax(x), idx)
    assert not torch.equal(rgo.pool_argmax(x, last=True), idx)
    assert torch.equal(rgo.pool(x, idx), torch.nn.functional.max_pool2d(x, 3, stride=2, padding=1))
