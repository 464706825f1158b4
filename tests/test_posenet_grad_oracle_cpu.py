"""The pose network's differentiable oracle (tests/posenet_grad_oracle.py) against the reference's own autograd
(tests/golden/posenet_grad_*.npz, made by tests/golden/gen_posenet_grad_golden.py), and the measurement behind the gate's TOL."""
import os

import numpy as np
import pytest
import torch

import posenet_grad_cases as cases
import posenet_grad_oracle as pgo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-9   # of each tensor's largest entry: the bar DESIGN section 8 f2''' records for the loss oracle


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_oracle_fp64_autograd_equals_the_reference(name):
    c = cases.GOLDEN[name]
    gold = load(name)
    image0, image1, sd_enc, sd_dec, cot = cases.inputs(c)
    for k, v in cases.checksums(image0, image1, sd_enc, sd_dec).items():      # the regenerated inputs are the golden's inputs
        assert abs(v - float(gold["sum::" + k])) <= 1e-12 * abs(v), (k, v, float(gold["sum::" + k]))
    assert torch.equal(cot, gold["cotangent"])
    got = pgo.gradients(image0, image1, sd_enc, sd_dec, cot, batch_norm=c["batch_norm"])
    keys = [k for k in gold if k.startswith(("enc::", "dec::", "run::"))] + ["dof", "pose"]
    assert sum(k.startswith("enc::") for k in keys) == 21 and sum(k.startswith("run::") for k in keys) == 21
    for k in keys:
        a, b = got[k], gold[k]
        if not b.is_floating_point():
            assert torch.equal(a, b), k                                       # num_batches_tracked
            continue
        worst = float((a - b).abs().max() / b.abs().max())
        assert worst <= BAR, (name, k, worst)
    if c["batch_norm"] == "batch":
        assert all(int(gold[f"run::conv{i}.batch_norm.num_batches_tracked"]) == 1001 for i in range(1, 8))


def test_tol_is_three_times_the_fp32_oracle_rounded_up():
    """The gate |a - b| <= TOL |b| + TOL rms(b): over every case of the GPU model tests the oracle's fp32 autograd stays within
    TOL / 3 of its fp64 autograd (on the activation branches the fp32 run took: see posenet_grad_oracle.forward), and TOL is that
    figure tripled, rounded up to one digit, and no more than the loss backward's 1e-3.  Measured: 2.4e-5, 2.3e-5, 1.5e-5, 3.4e-5
    and 6.4e-5 (full width, batch statistics, enc::conv7.conv.weight) -> 3 x 6.4e-5 = 1.9e-4 -> 2e-4."""
    worst = {}
    for name, c in cases.MODEL.items():
        if c["batch_norm"] == "batch":
            assert cases.last_map_values(c) >= 8, name
        image0, image1, sd_enc, sd_dec, cot = cases.inputs(c)
        o32 = pgo.gradients(image0, image1, sd_enc, sd_dec, cot, dtype=torch.float32, batch_norm=c["batch_norm"])
        masks = [z > 0 for z in o32["pre"]]
        o64 = pgo.gradients(image0, image1, sd_enc, sd_dec, cot, batch_norm=c["batch_norm"], masks=masks)
        pgo.kink_check(masks, o64["pre"])
        keys = [k for k in o64 if k.startswith(("enc::", "dec::"))] + ["dof"]
        worst[name] = max((pgo.fraction(o32[k], o64[k]), k) for k in keys)
    print(worst)
    top = max(v[0] for v in worst.values())
    assert pgo.TOL <= 1e-3
    assert 3.0 * top <= pgo.TOL, worst
    assert pgo.TOL <= 2.0 * 3.0 * top or pgo.TOL == 1e-3, worst     # "rounded up to one digit", not a wider bound


FRAME_AXIS = ["narrow_n3_running", "narrow_n5_running", "narrow_n3_batch"]     # the cases with three and five frames


@pytest.mark.parametrize("name", FRAME_AXIS)
def test_frame_axis_cases_keep_the_seed_rule(name):
    """The rule written in resnet_pose_grad_cases.py, from the fp64 oracle alone: (a) the oracle's own fp32 autograd under a third
    of the gate, (b) no activation with more pre-activations near 0 than kink_check lets flip.  Measured (a): 1.3e-5, 5.7e-6 and
    4.1e-5 (batch statistics over 9 values, enc::conv7.conv.weight)."""
    c = cases.MODEL[name]
    assert c["n"] in (3, 5)
    if c["batch_norm"] == "batch":
        assert cases.last_map_values(c) >= 8
    image0, image1, sd_enc, sd_dec, cot = cases.inputs(c)
    o32 = pgo.gradients(image0, image1, sd_enc, sd_dec, cot, dtype=torch.float32, batch_norm=c["batch_norm"])
    masks = [z > 0 for z in o32["pre"]]
    o64 = pgo.gradients(image0, image1, sd_enc, sd_dec, cot, batch_norm=c["batch_norm"], masks=masks)
    assert pgo.kink_check(masks, o64["pre"]) == 0
    keys = [k for k in o64 if k.startswith(("enc::", "dec::"))] + ["dof"]
    figure, where = max((pgo.fraction(o32[k], o64[k]), k) for k in keys)
    print(f"{name}: fp32 autograd at {figure:.2e} of |b| + rms(b) ({where})")
    assert 3.0 * figure <= pgo.TOL, (name, figure, where)
    pgo.kink_room(pgo.gradients(image0, image1, sd_enc, sd_dec, cot, batch_norm=c["batch_norm"])["pre"])
