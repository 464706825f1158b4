"""GPU: PoseNetModel with gradients on -- requires_grad_(True), set_batch_norm('running' | 'batch') -- against the reference's own
autograd (tests/golden/posenet_grad_*.npz) and the fp64 oracle (tests/posenet_grad_oracle.py).

Gate: |a - b| <= TOL |b| + TOL rms(b) per parameter gradient and for dof (posenet_grad_oracle.TOL); the running statistics after
a batch-mode forward at the forward's 1e-4 rule.  Against the goldens the comparison is direct.  Against the oracle (the
full-width cases, the chain behind the loss) the fp64 network is differentiated on the activation branches the device took, after
posenet_grad_oracle.kink_check has shown that the elements whose branch differs from the fp64 sign are a handful AT the kink.

    python -m pytest tests -m gpu -q
"""
import os

import numpy as np
import pytest
import torch

import kbnet_amd as kb
KbnError = kb._lib.KbnError

import posenet_grad_cases as cases
import posenet_grad_oracle as pgo
import posenet_oracle as po

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _model(dev, c, enc, dec, mode):
    m = kb.modules.PoseNetModel(device=dev, n_filters=c["filters"])
    m.load_state_dicts(enc, dec)
    assert m.requires_grad_(True) is m and m.set_batch_norm(mode) is m
    return m


def _grads(m, dof):
    got = {"dof": dof.detach()}
    for grp, mod in (("enc", m.encoder), ("dec", m.decoder)):
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            got[f"{grp}::{k}"] = p.grad
    return got


def _compare(label, got, want):
    keys = [k for k in want if k.startswith(("enc::", "dec::"))] + ["dof"]
    assert len(keys) == 23
    figures = {k: pgo.fraction(got[k], want[k]) for k in keys}
    worst = max(figures, key=figures.get)
    print(f"{label}: worst {figures[worst]:.2e} at {worst} (gate {pgo.TOL:.0e}); conv weights "
          + " ".join(f"{figures[f'enc::conv{i}.conv.weight']:.1e}" for i in range(1, 8)) + f"; dof {figures['dof']:.1e}")
    for k, v in figures.items():
        assert v <= pgo.TOL, (label, k, v)
        assert torch.isfinite(got[k]).all() and float(got[k].abs().max()) > 0, (label, k)


def _running(label, m, want, before, mode):
    for i in range(1, 8):
        bn = getattr(m.encoder, f"conv{i}").batch_norm
        assert bn.training is False
        for key in ("running_mean", "running_var"):
            b = want[f"run::conv{i}.batch_norm.{key}"]
            a = getattr(bn, key)
            if mode == "running":
                assert torch.equal(a.cpu(), before[f"conv{i}.batch_norm.{key}"]), (label, i, key)
            else:
                f = po.gate_fraction(a, b, po.layer_floor(b))
                assert f <= 1.0, (label, i, key, f)
        assert int(bn.num_batches_tracked) == 1000 + (mode == "batch")


def _run(dev, c, mode):
    image0, image1, enc, dec, cot = cases.inputs(c)
    m = _model(dev, c, enc, dec, mode)
    pose, dof, layers = m.forward(image0.to(dev), image1.to(dev), return_all=True)
    assert pose.grad_fn is not None and pose.dtype == torch.float32 and tuple(pose.shape) == (c["n"], 4, 4)
    (pose * cot.float().to(dev)).sum().backward()
    return m, _grads(m, dof), layers, (image0, image1, enc, dec, cot)


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_narrow_model_against_the_references_autograd(dev, name):
    c = cases.GOLDEN[name]
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        gold = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    m, got, _, inputs = _run(dev, c, c["batch_norm"])
    _compare(name, got, gold)
    _running(name, m, gold, inputs[2], c["batch_norm"])


@pytest.mark.parametrize("name", ["narrow_train_shape_running", "full_running", "full_batch", "narrow_n3_running", "narrow_n5_running",
                                  "narrow_n3_batch"])
def test_model_against_the_fp64_oracle(dev, name):
    c = cases.MODEL[name]
    if c["batch_norm"] == "batch":
        assert cases.last_map_values(c) >= 8
    m, got, layers, inputs = _run(dev, c, c["batch_norm"])
    masks = [(t > 0).cpu() for t in layers]
    want = pgo.gradients(*inputs, batch_norm=c["batch_norm"], masks=masks)
    print(f"{name}: {pgo.kink_check(masks, want['pre'])} activations on the other side of the kink than in fp64")
    _compare(name, got, want)
    _running(name, m, want, inputs[2], c["batch_norm"])


def test_frame_order_leaves_the_gradients_inside_the_gate(dev):
    """Five frames in another order (no frame keeps its place), the cotangent with them: every parameter gradient is a sum over the
    frames in another order, so it stays within the gate of the SAME oracle result, and dof moves with its frame."""
    c = cases.MODEL["narrow_n5_running"]
    image0, image1, enc, dec, cot = cases.inputs(c)
    perm = torch.roll(torch.arange(c["n"]), 2)
    inv = torch.argsort(perm)
    assert not bool((perm == torch.arange(c["n"])).any())
    m = _model(dev, c, enc, dec, "running")
    pose, dof, layers = m.forward(image0[perm].to(dev), image1[perm].to(dev), return_all=True)
    (pose * cot[perm].float().to(dev)).sum().backward()
    got = _grads(m, dof.detach().cpu()[inv])
    masks = [(t.detach().cpu()[inv] > 0) for t in layers]
    want = pgo.gradients(image0, image1, enc, dec, cot, batch_norm="running", masks=masks)
    pgo.kink_check(masks, want["pre"])
    _compare("narrow_n5_running, frames permuted", got, want)


def test_defaults_are_unchanged(dev):
    c = cases.MODEL["full_running"]
    image0, image1, enc, dec, _ = cases.inputs(c)
    d0, d1 = image0.to(dev), image1.to(dev)
    m = kb.modules.PoseNetModel(device=dev)
    m.load_state_dicts(enc, dec)
    assert all(not p.requires_grad for p in m.parameters()) and m.batch_norm_mode == "running"
    # the parent's path: seven fused launches and the head kernel, called directly
    x = [d0, d1]
    for layer in m.encoder.layers():
        scale, shift = layer.affine()
        x = [kb.ops.conv2d_s2_affine(x, layer.packed(), scale, shift, layer.out_channels, layer.kernel_size, negative_slope=layer.slope)]
    want = kb.ops.pose_head(x[0], m.decoder.conv.conv.weight)
    pose = m.forward(d0, d1)
    assert pose.grad_fn is None and not pose.requires_grad and torch.equal(pose, want)
    m.requires_grad_(True)
    assert all(p.requires_grad for p in m.parameters()) and len(m.parameters()) == 22
    with torch.no_grad():
        quiet = m.forward(d0, d1)
    assert quiet.grad_fn is None and torch.equal(quiet, want)
    recorded, dof, _ = m.forward(d0, d1, return_all=True)
    assert recorded.grad_fn is not None
    _, dof_kernel = kb.ops.pose_head(x[0], m.decoder.conv.conv.weight, return_dof=True)
    ref = pgo.forward(image0.double(), image1.double(), *po.to64(enc, dec))
    assert po.gate_fraction(dof, dof_kernel, po.dof_floor(ref["map"])) <= 1.0     # the recorded head against the kernel's dof
    m.requires_grad_(False)
    assert m.forward(d0, d1).grad_fn is None
    with pytest.raises(KbnError, match="inference only"):
        m.train()


def test_batch_mode_without_gradients_still_uses_and_updates_the_statistics(dev):
    c = cases.GOLDEN["posenet_grad_train"]
    image0, image1, enc, dec, cot = cases.inputs(c)
    m = kb.modules.PoseNetModel(device=dev, n_filters=c["filters"])
    m.load_state_dicts(enc, dec)
    m.set_batch_norm("batch")
    pose, dof, _ = m.forward(image0.to(dev), image1.to(dev), return_all=True)
    assert pose.grad_fn is None
    want = pgo.gradients(image0, image1, enc, dec, cot, batch_norm="batch")
    ref = pgo.forward(image0.double(), image1.double(), *po.to64(enc, dec), batch_norm="batch")
    assert po.gate_fraction(dof, want["dof"], po.dof_floor(ref["map"])) <= 1.0
    _running("batch, no grad", m, want, enc, "batch")


def test_refusals(dev):
    c = cases.GOLDEN["posenet_grad_eval"]
    image0, image1, enc, dec, _ = cases.inputs(c)
    m = _model(dev, c, enc, dec, "running")
    with pytest.raises(KbnError, match="image0"):
        m.forward(image0.to(dev).requires_grad_(True), image1.to(dev))
    with pytest.raises(KbnError, match="image1"):
        m.forward(image0.to(dev), image1.to(dev).requires_grad_(True))
    with pytest.raises(KbnError):
        m.set_batch_norm("train")
    m.set_batch_norm("batch")
    with pytest.raises(KbnError, match="one value per channel"):
        m.forward(image0[:1].to(dev), image1[:1].to(dev))      # the last map of one 61 x 77 frame is 1 x 1
    r = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, n_filters=[8, 8, 16, 16, 32], decoder_filters=[16, 16])
    with pytest.raises(KbnError, match="posenet"):
        r.requires_grad_(True)
    r.requires_grad_(False)


def test_gradients_reach_the_parameters_through_compute_loss(dev):
    """compute_loss on poses from the recording PoseNetModel: loss.backward() fills every parameter's .grad, and those gradients
    are the oracle's chain fed with the d loss / d pose the HIP loss backward delivered -- the pose network's part, not the loss again."""
    c = cases.MODEL["full_running"]
    _, _, enc, dec, _ = cases.inputs(c)
    i0, i1, i2, depth, sparse, validity, k, _, _ = kb.synthetic.make_triplet(2, 64, 96, "kitti", seed=12)
    m = _model(dev, c, enc, dec, "running")
    d0, d1, d2 = i0.to(dev), i1.to(dev), i2.to(dev)
    pose01, dof01, layers01 = m.forward(d0, d1, return_all=True)
    pose02, dof02, layers02 = m.forward(d0, d2, return_all=True)
    pose01.retain_grad()
    pose02.retain_grad()
    kbnet = kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), dev)
    loss, _ = kbnet.compute_loss(d0, d1, d2, depth.to(dev), sparse.to(dev), validity.to(dev), k.to(dev), pose01, pose02)
    loss.backward()
    got = _grads(m, dof01)
    want = None
    for other, pose, layers in ((i1, pose01, layers01), (i2, pose02, layers02)):
        assert pose.grad is not None and float(pose.grad.abs().max()) > 0
        masks = [(t > 0).cpu() for t in layers]
        part = pgo.pose_gradients(i0, other, enc, dec, pose.grad.double().cpu(), masks=masks)
        pgo.kink_check(masks, part["pre"])
        if want is None:
            want = part
        else:
            for key in part:
                if key.startswith(("enc::", "dec::")):
                    want[key] = want[key] + part[key]
    _compare("through compute_loss", got, want)


def test_an_optimizer_step_reaches_the_next_forward(dev):
    """One SGD step changes every weight in place; the next forward (recorded and fused) runs on the new weights: the packed
    blobs follow the parameters' versions."""
    c = cases.GOLDEN["posenet_grad_eval"]
    image0, image1, enc, dec, cot = cases.inputs(c)
    m = _model(dev, c, enc, dec, "running")
    d0, d1 = image0.to(dev), image1.to(dev)
    opt = torch.optim.SGD(m.parameters(), lr=1e-5)      # (the 1e-3-variance channels make the gradients large)
    pose, dof_before, _ = m.forward(d0, d1, return_all=True)
    (pose * cot.float().to(dev)).sum().backward()
    opt.step()
    opt.zero_grad()
    sd_enc = {k: v.detach().cpu() for k, v in m.encoder.state_dict().items()}
    sd_dec = {k: v.detach().cpu() for k, v in m.decoder.state_dict().items()}
    assert not torch.equal(sd_enc["conv3.conv.weight"], enc["conv3.conv.weight"])
    ref = pgo.forward(image0.double(), image1.double(), *po.to64(sd_enc, sd_dec))
    floor = po.dof_floor(ref["map"])
    assert po.gate_fraction(dof_before, ref["dof"], floor) > 10.0          # the step moved the pose far outside the gate
    _, dof_recorded, _ = m.forward(d0, d1, return_all=True)
    with torch.no_grad():
        _, dof_fused, _ = m.forward(d0, d1, return_all=True)
    for label, dof in (("recorded", dof_recorded), ("fused", dof_fused)):
        f = po.gate_fraction(dof, ref["dof"], floor)
        print(f"after the step, {label}: dof at {f:.3f} of the gate")
        assert f <= 1.0, (label, f)
