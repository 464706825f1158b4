"""GPU: ResNetPoseNetModel(trainable=True) with gradients on -- requires_grad_(True), set_batch_norm('running' | 'batch') -- against
the reference's own autograd (tests/golden/resnet_pose_grad_18_*.npz) and the fp64 oracle (tests/resnet_pose_grad_oracle.py).

Gate: |a - b| <= TOL |b| + TOL rms(b) per parameter gradient and for dof (resnet_pose_grad_oracle.TOL); the running statistics after
a batch-mode forward at the forward's 1e-4 rule.  Against the goldens the comparison is direct.  Against the oracle the fp64 network
is differentiated on the activation branches and pool windows the device took, after resnet_pose_grad_oracle.kink_check has shown
that the ones that differ from fp64 are a handful AT the kink.

    python -m pytest tests -m gpu -q
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kbnet_amd as kb
KbnError = kb._lib.KbnError

import posenet_oracle as po
import resnet_pose_grad_cases as cases
import resnet_pose_grad_oracle as rgo
import resnet_pose_oracle as ro

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP = 1e-4      # the learning rate of the SGD step below: on the CPU oracle it moves dof to a thousand times the forward's gate


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _model(dev, c, enc, dec, mode, trainable=True):
    m = kb.posenet_resnet.ResNetPoseNetModel(n_layer=c["n_layer"], device=dev, n_filters=c["filters"], decoder_filters=c["decoder_filters"],
                                             trainable=trainable)
    m.load_state_dicts(enc, dec)
    if trainable:
        assert m.requires_grad_(True) is m and m.set_batch_norm(mode) is m
    return m


def _grads(m, dof, c):
    """dof and every parameter's .grad; the projections no forward touched must have none."""
    got = {"dof": dof.detach()}
    unused = cases.unused_projections(c)
    for grp, mod in (("enc", m.encoder), ("dec", m.decoder)):
        for k, p in mod.named_parameters():
            key = f"{grp}::{k}"
            if key in unused:
                assert p.grad is None, key
            else:
                assert p.grad is not None, key
                got[key] = p.grad
    return got


def _compare(label, got, want):
    keys = [k for k in want if k.startswith(("enc::", "dec::"))]
    assert sorted(keys) == sorted(k for k in got if k != "dof"), label
    figures = {k: rgo.fraction(got[k], want[k]) for k in keys + ["dof"]}
    worst = max(figures, key=figures.get)
    print(f"{label}: worst {figures[worst]:.2e} at {worst} (gate {rgo.TOL:.0e}); conv1 {figures['enc::conv1.conv.weight']:.1e}, "
          f"blocks2.0.projection {figures['enc::blocks2.0.projection.conv.weight']:.1e}, blocks3.0.projection "
          f"{figures['enc::blocks3.0.projection.conv.weight']:.1e}; dof {figures['dof']:.1e}")
    for k, v in figures.items():
        assert v <= rgo.TOL, (label, k, v)
        assert torch.isfinite(got[k]).all() and float(got[k].abs().max()) > 0, (label, k)


def _running(label, m, want, before, mode):
    """The running statistics after the forward: untouched on 'running', torch.nn.BatchNorm2d's update on 'batch'."""
    count = 0
    for grp, mod, sd in (("enc", m.encoder, before[0]), ("dec", m.decoder, before[1])):
        for k, a in mod.state_dict().items():
            if k.endswith(("running_mean", "running_var")):
                if mode == "running":
                    assert torch.equal(a.cpu(), sd[k]), (label, k)
                else:
                    b = want[f"run::{grp}::{k}"]
                    f = po.gate_fraction(a, b, po.layer_floor(b))
                    assert f <= 1.0, (label, k, f)
                count += 1
            elif k.endswith("num_batches_tracked"):
                assert int(a) == 1000 + (mode == "batch"), (label, k)
        for mod_ in mod.modules():
            assert mod_.training is False
    assert count == 2 * (1 + 2 * sum(ro.BLOCKS[m.n_layer]) + 2)


def _branches(c, layers, inner):
    """(masks, pool indices) of the device's run: name -> y > 0 for every activation (y > 0 exactly where z > 0 for a slope >= 0),
    and torch's argmax of every pool window over the device's fp32 conv1 output."""
    names = ro.names(c["n_layer"], len(c["decoder_filters"]))
    assert len(names) == len(layers)
    masks = {name: (t > 0).cpu() for name, t in zip(names, layers) if name != "pool"}
    masks.update({name: (t > 0).cpu() for name, t in inner.items()})
    _, indices = F.max_pool2d(layers[0].detach().cpu(), 3, stride=2, padding=1, return_indices=True)
    assert torch.equal(F.max_pool2d(layers[0].detach().cpu(), 3, stride=2, padding=1), layers[1].detach().cpu())
    return masks, indices


def _run(dev, c, mode):
    image0, image1, enc, dec, cot = cases.inputs(c)
    m = _model(dev, c, enc, dec, mode)
    pose, dof, layers, inner = m.forward(image0.to(dev), image1.to(dev), return_all=True, return_inner=True)
    assert pose.grad_fn is not None and pose.dtype == torch.float32 and tuple(pose.shape) == (c["n"], 4, 4)
    assert sorted(inner) == sorted(f"{n}.conv{i}" for n in ro.names(c["n_layer"], 0)[2:] for i in (1, 2))
    (pose * cot.float().to(dev)).sum().backward()
    return m, _grads(m, dof, c), layers, inner, (image0, image1, enc, dec, cot)


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_narrow_model_against_the_references_autograd(dev, name):
    c = cases.GOLDEN[name]
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        gold = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    m, got, _, _, inputs = _run(dev, c, c["batch_norm"])
    _compare(name, got, gold)
    _running(name, m, gold, inputs[2:4], c["batch_norm"])


@pytest.mark.parametrize("name", ["narrow_34_running", "narrow_34_batch", "full_18_running", "full_18_batch", "narrow_18_n3_running",
                                  "narrow_18_n5_running", "narrow_18_n3_batch"])
def test_model_against_the_fp64_oracle(dev, name):
    c = cases.MODEL[name]
    if c["batch_norm"] == "batch":
        assert cases.last_map_values(c) >= 8
    m, got, layers, inner, inputs = _run(dev, c, c["batch_norm"])
    masks, indices = _branches(c, layers, inner)
    want = rgo.gradients(*inputs, n_layer=c["n_layer"], batch_norm=c["batch_norm"], masks=masks, pool_indices=indices)
    kinks = rgo.kink_check(masks, want["pre"], indices, want["pool_in"])
    print(f"{name}: {kinks} activations / pool windows on the other side of the kink than in fp64")
    _compare(name, got, want)
    _running(name, m, want, inputs[2:4], c["batch_norm"])


def test_frame_order_leaves_the_gradients_inside_the_gate(dev):
    """Five frames in another order (no frame keeps its place), the cotangent with them: every parameter gradient is a sum over the
    frames in another order, so it stays within the gate of the SAME oracle result, and dof moves with its frame."""
    c = cases.MODEL["narrow_18_n5_running"]
    image0, image1, enc, dec, cot = cases.inputs(c)
    perm = torch.roll(torch.arange(c["n"]), 2)
    inv = torch.argsort(perm)
    assert not bool((perm == torch.arange(c["n"])).any())
    m = _model(dev, c, enc, dec, "running")
    pose, dof, layers, inner = m.forward(image0[perm].to(dev), image1[perm].to(dev), return_all=True, return_inner=True)
    (pose * cot[perm].float().to(dev)).sum().backward()
    got = _grads(m, dof.detach().cpu()[inv], c)
    masks, indices = _branches(c, [t.detach().cpu()[inv] for t in layers], {k: t.detach().cpu()[inv] for k, t in inner.items()})
    want = rgo.gradients(image0, image1, enc, dec, cot, n_layer=c["n_layer"], batch_norm="running", masks=masks, pool_indices=indices)
    rgo.kink_check(masks, want["pre"], indices, want["pool_in"])
    _compare("narrow_18_n5_running, frames permuted", got, want)


def test_trainable_without_gradients_is_the_default_models_fused_forward(dev):
    c = cases.MODEL["full_18_running"]
    image0, image1, enc, dec, _ = cases.inputs(c)
    d0, d1 = image0.to(dev), image1.to(dev)
    plain = _model(dev, c, enc, dec, "running", trainable=False)
    want, want_dof, want_layers = plain.forward(d0, d1, return_all=True)
    m = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, trainable=True)
    m.load_state_dicts(enc, dec)
    assert all(not p.requires_grad for p in m.parameters()) and m.batch_norm_mode == "running"
    ops = kb.ops
    ops.PROFILE = []
    try:
        pose = m.forward(d0, d1)
        launches = len(ops.PROFILE)
    finally:
        ops.PROFILE = None
    assert launches == 25 and pose.grad_fn is None and torch.equal(pose, want)
    m.requires_grad_(True)
    with torch.no_grad():
        quiet, dof, layers = m.forward(d0, d1, return_all=True)
    assert quiet.grad_fn is None and torch.equal(quiet, want) and torch.equal(dof, want_dof)
    assert all(torch.equal(a, b) for a, b in zip(layers, want_layers))
    recorded, dof, layers = m.forward(d0, d1, return_all=True)
    assert recorded.grad_fn is not None and len(layers) == len(want_layers)
    ref = rgo.forward(image0.double(), image1.double(), *po.to64(enc, dec))
    assert po.gate_fraction(dof, want_dof, po.dof_floor(ref["map"])) <= 1.0       # the layer-by-layer forward against the fused one
    for a, b in zip(layers, ref["layers"]):
        assert po.gate_fraction(a, b, po.layer_floor(b)) <= 1.0
    m.requires_grad_(False)
    assert m.forward(d0, d1).grad_fn is None
    with pytest.raises(KbnError, match="inference only"):
        m.train()


def test_batch_mode_without_gradients_still_uses_and_updates_the_statistics(dev):
    c = cases.GOLDEN["resnet_pose_grad_18_train"]
    image0, image1, enc, dec, cot = cases.inputs(c)
    m = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, n_filters=c["filters"], decoder_filters=c["decoder_filters"],
                                             trainable=True)
    m.load_state_dicts(enc, dec)
    m.set_batch_norm("batch")
    pose, dof, layers, inner = m.forward(image0.to(dev), image1.to(dev), return_all=True, return_inner=True)
    assert pose.grad_fn is None and all(t.grad_fn is None for t in layers) and len(inner) == 16
    want = rgo.gradients(image0, image1, enc, dec, cot, n_layer=18, batch_norm="batch")
    ref = rgo.forward(image0.double(), image1.double(), *po.to64(enc, dec), batch_norm="batch")
    assert po.gate_fraction(dof, want["dof"], po.dof_floor(ref["map"])) <= 1.0
    running = rgo.forward(image0.double(), image1.double(), *po.to64(enc, dec), batch_norm="running")
    assert po.gate_fraction(dof, running["dof"], po.dof_floor(ref["map"])) > 10.0      # not the running statistics' pose
    _running("batch, no grad", m, want, (enc, dec), "batch")


def test_refusals(dev):
    c = cases.GOLDEN["resnet_pose_grad_18_eval"]
    image0, image1, enc, dec, _ = cases.inputs(c)
    m = _model(dev, c, enc, dec, "running")
    with pytest.raises(KbnError, match="image0"):
        m.forward(image0.to(dev).requires_grad_(True), image1.to(dev))
    with pytest.raises(KbnError, match="image1"):
        m.forward(image0.to(dev), image1.to(dev).requires_grad_(True))
    with pytest.raises(KbnError):
        m.set_batch_norm("train")
    with torch.no_grad():
        with pytest.raises(KbnError, match="return_inner"):
            m.forward(image0.to(dev), image1.to(dev), return_inner=True)
    m.set_batch_norm("batch")
    with pytest.raises(KbnError, match="one value per channel"):
        m.forward(image0[:1].to(dev), image1[:1].to(dev))      # the last map of one 61 x 77 frame is 1 x 1
    plain = _model(dev, c, enc, dec, "running", trainable=False)
    with pytest.raises(KbnError, match="posenet"):
        plain.requires_grad_(True)
    with pytest.raises(KbnError, match="trainable=True"):
        plain.set_batch_norm("batch")


def test_gradients_reach_the_parameters_through_compute_loss(dev):
    """compute_loss on poses from the recording model, two forwards accumulating: loss.backward() fills every used parameter's
    .grad, and those gradients are the oracle's chain fed with the d loss / d pose the HIP loss backward delivered."""
    c = cases.MODEL["full_18_running"]
    _, _, enc, dec, _ = cases.inputs(c)
    i0, i1, i2, depth, sparse, validity, k, _, _ = kb.synthetic.make_triplet(2, 64, 96, "kitti", seed=12)
    m = _model(dev, c, enc, dec, "running")
    d0, d1, d2 = i0.to(dev), i1.to(dev), i2.to(dev)
    pose01, dof01, layers01, inner01 = m.forward(d0, d1, return_all=True, return_inner=True)
    pose02, dof02, layers02, inner02 = m.forward(d0, d2, return_all=True, return_inner=True)
    pose01.retain_grad()
    pose02.retain_grad()
    kbnet = kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), dev)
    loss, _ = kbnet.compute_loss(d0, d1, d2, depth.to(dev), sparse.to(dev), validity.to(dev), k.to(dev), pose01, pose02)
    loss.backward()
    got = _grads(m, dof01, c)
    want = None
    for other, pose, layers, inner in ((i1, pose01, layers01, inner01), (i2, pose02, layers02, inner02)):
        assert pose.grad is not None and float(pose.grad.abs().max()) > 0
        masks, indices = _branches(c, layers, inner)
        part = rgo.gradients(i0, other, enc, dec, pose.grad.double().cpu(), n_layer=18, masks=masks, pool_indices=indices)
        rgo.kink_check(masks, part["pre"], indices, part["pool_in"])
        if want is None:
            want = part
        else:
            for key in rgo.gradient_keys(part):
                want[key] = want[key] + part[key]
    _compare("through compute_loss", got, want)


def test_an_optimizer_step_reaches_the_next_forward(dev):
    """One SGD step changes every used weight in place; the next forward (recorded and fused) runs on the new weights: the packed
    blobs follow the parameters' versions."""
    c = cases.GOLDEN["resnet_pose_grad_18_eval"]
    image0, image1, enc, dec, cot = cases.inputs(c)
    m = _model(dev, c, enc, dec, "running")
    d0, d1 = image0.to(dev), image1.to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=STEP)
    pose, dof_before, _ = m.forward(d0, d1, return_all=True)
    (pose * cot.float().to(dev)).sum().backward()
    opt.step()
    opt.zero_grad()
    sd_enc = {k: v.detach().cpu() for k, v in m.encoder.state_dict().items()}
    sd_dec = {k: v.detach().cpu() for k, v in m.decoder.state_dict().items()}
    for key in ("blocks2.0.conv2.conv.weight", "blocks2.0.projection.conv.weight", "blocks3.0.projection.conv.weight", "conv1.conv.weight"):
        assert not torch.equal(sd_enc[key], enc[key]), key
    assert torch.equal(sd_enc["blocks2.1.projection.conv.weight"], enc["blocks2.1.projection.conv.weight"])     # never used: no gradient
    ref = rgo.forward(image0.double(), image1.double(), *po.to64(sd_enc, sd_dec))
    floor = po.dof_floor(ref["map"])
    assert po.gate_fraction(dof_before, ref["dof"], floor) > 10.0          # the step moved the pose far outside the gate
    _, dof_recorded, _ = m.forward(d0, d1, return_all=True)
    with torch.no_grad():
        _, dof_fused, _ = m.forward(d0, d1, return_all=True)
    for label, dof in (("recorded", dof_recorded), ("fused", dof_fused)):
        f = po.gate_fraction(dof, ref["dof"], floor)
        print(f"after the step, {label}: dof at {f:.3f} of the gate")
        assert f <= 1.0, (label, f)

