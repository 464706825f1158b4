"""GPU: PoseNetModel (csrc/posenet.hip: kbn_conv2d_s2_affine_forward, kbn_pose_head_forward) against the vectors captured from the
reference's PoseEncoder / PoseDecoder in eval mode (fp64 evaluation) and against tests/posenet_oracle.py in fp64.

Gate (the element-wise rule of test_hip_parity.py::test_intermediate_tensors_elementwise_full_size): |a - b| <= 1e-4 |b| + floor
  layers   floor = 1e-4 x the layer tensor's RMS
  dof      and the translation column of the pose: floor = 1e-4 x 0.01 x RMS of the 6-channel map (the tensor that is averaged)
  pose     equals ops.pose_matrix(dof of the kernel) bit for bit: the rotation block has no tolerance of its own
The head averages the latent BEFORE the 6 x C product (another summation order of the same sum), so the kernels never hold the
6-channel map; `dof`, its mean, is what they are compared on.  tests/test_posenet_cpu.py proves that the dof gate sees a swapped
image pair, a dropped eps, slope 0.10, a narrower first padding and an omitted 0.01.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch

import kbnet_amd as kb
from conftest import load_golden

import loss_oracle as lo
import posenet_oracle as po

pytestmark = pytest.mark.gpu

NARROW = [8, 16, 16, 32, 32, 24, 40]
SENTINEL = -7.25e30
GUARD = 1024


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def full(dev):
    """The default-width model with synthetic weights, and those weights in fp64 for the oracle (shared, never modified)."""
    enc, dec = kb.synthetic.make_posenet_weights(seed=5)
    m = kb.modules.PoseNetModel(device=dev)
    m.load_state_dicts(enc, dec)
    return m, po.to64(enc, dec)


def _narrow(dev, enc, dec):
    m = kb.modules.PoseNetModel(device=dev, n_filters=NARROW)
    m.load_state_dicts(enc, dec)
    return m


def _check(label, got, want):
    """`got`: (pose, dof, layers) of PoseNetModel.forward(return_all=True); `want`: fp64 'layers' / 'map' / 'dof' / 'pose'.
    Prints every figure (as a fraction of its gate) before it asserts."""
    pose, dof, layers = got
    assert pose.dtype == torch.float32 and tuple(pose.shape) == (dof.shape[0], 4, 4) and tuple(dof.shape) == (dof.shape[0], 6)
    figures = {}
    for i, (a, b) in enumerate(zip(layers, want["layers"]), 1):
        assert tuple(a.shape) == tuple(b.shape), (label, i, a.shape, b.shape)
        figures[f"layer{i}"] = po.gate_fraction(a, b, po.layer_floor(b))
    floor = po.dof_floor(want["map"])
    figures["dof"] = po.gate_fraction(dof, want["dof"], floor)
    figures["translation"] = po.gate_fraction(pose[:, :3, 3], want["pose"][:, :3, 3], floor)
    rotation = float((pose[:, :3, :3].double().cpu() - want["pose"][:, :3, :3]).abs().max())
    exact = torch.equal(pose, kb.ops.pose_matrix(dof))
    print(label, " ".join(f"{k} {v:.3f}" for k, v in figures.items()), f"(fractions of the gate)  rotation block {rotation:.2e} from fp64,"
          f" pose == pose_matrix(dof): {exact}")
    assert len(layers) == len(want["layers"]) == 7
    for k, v in figures.items():
        assert v <= 1.0, (label, k, v)
    assert exact, (label, pose, kb.ops.pose_matrix(dof))
    assert torch.equal(pose[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(pose.shape[0], 4))


@pytest.mark.parametrize("name", ["posenet_odd", "posenet_wide"])
def test_posenet_golden(dev, name):
    g = load_golden(name)
    enc = {k: torch.as_tensor(v) for k, v in g["enc"].items()}
    dec = {k: torch.as_tensor(v) for k, v in g["dec"].items()}
    m = _narrow(dev, enc, dec)
    got = m.forward(g["image0"].to(dev), g["image1"].to(dev), return_all=True)
    want = {"layers": [g["ref64"][f"layer{i}"] for i in range(1, 8)], "map": g["ref64"]["map"], "dof": g["ref64"]["dof"],
            "pose": g["ref64"]["pose"]}
    _check(name, got, want)
    assert torch.equal(m.forward(g["image0"].to(dev), g["image1"].to(dev)), got[0])


@pytest.mark.parametrize("shape", [(2, 197, 325), (3, 61, 77), (1, 128, 416), (1, 352, 1216)], ids=lambda s: "x".join(map(str, s)))
def test_posenet_full_width_vs_oracle(dev, full, shape):
    m, (enc64, dec64) = full
    n, h, w = shape
    i0, i1 = kb.synthetic.make_image_pair(n, h, w, seed=20 + n + h)
    want = po.forward(i0.double(), i1.double(), enc64, dec64)
    _check("x".join(map(str, shape)), m.forward(i0.to(dev), i1.to(dev), return_all=True), want)
    if n > 1:
        assert float((want["dof"][0] - want["dof"][1]).abs().max()) > 100 * po.dof_floor(want["map"])    # the frames differ


def test_frame_permutation_permutes_the_poses_bit_for_bit(dev, full):
    m, _ = full
    i0, i1 = [t.to(dev) for t in kb.synthetic.make_image_pair(5, 61, 77, seed=31)]
    perm = torch.tensor([3, 0, 4, 1, 2], device=dev)
    pose, dof, layers = m.forward(i0, i1, return_all=True)
    ppose, pdof, players = m.forward(i0[perm].contiguous(), i1[perm].contiguous(), return_all=True)
    assert torch.equal(ppose, pose[perm]) and torch.equal(pdof, dof[perm])
    assert all(torch.equal(a, b[perm]) for a, b in zip(players, layers))
    assert len({tuple(r.tolist()) for r in dof.cpu()}) == 5          # a permutation that is ignored would show
    alone = m.forward(i0[2:3], i1[2:3])
    assert torch.equal(alone[0], pose[2])                            # a frame alone = that frame in the batch


def test_another_frame_does_not_change_this_frames_bits(dev, full):
    m, _ = full
    i0, i1 = [t.to(dev) for t in kb.synthetic.make_image_pair(2, 61, 77, seed=32)]
    pose, dof, layers = m.forward(i0, i1, return_all=True)
    j1 = i1.clone()
    j1[1] = i0[1]                                                    # frame 1 alone: image1 == image0
    pose2, dof2, layers2 = m.forward(i0, j1, return_all=True)
    assert torch.equal(pose2[0], pose[0]) and torch.equal(dof2[0], dof[0])
    assert all(torch.equal(a[0], b[0]) for a, b in zip(layers2, layers))
    assert not torch.equal(dof2[1], dof[1])


def test_outputs_stay_inside_guarded_buffers(dev):
    """Every layer of the narrow model at an odd size (pixel counts that are no multiple of the 128-pixel tile, filter counts
    that are no multiple of the filter tile, maps down to 1 x 1) and the head write into the middle of a buffer of sentinels."""
    g = load_golden("posenet_odd")
    enc = {k: torch.as_tensor(v) for k, v in g["enc"].items()}
    dec = {k: torch.as_tensor(v) for k, v in g["dec"].items()}
    m = _narrow(dev, enc, dec)
    free = m.forward(g["image0"].to(dev), g["image1"].to(dev), return_all=True)

    def guarded(shape):
        count = 1
        for s in shape:
            count *= s
        flat = torch.full((count + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.float32)
        return flat, flat[GUARD:GUARD + count].view(shape)

    def intact(flat):
        return bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all())

    x = [g["image0"].to(dev), g["image1"].to(dev)]
    for i, layer in enumerate(m.encoder.layers()):
        flat, out = guarded(tuple(free[2][i].shape))
        layer.run(x, out=out)
        torch.cuda.synchronize()
        assert intact(flat), f"layer {i + 1} wrote outside its output"
        assert torch.equal(out, free[2][i]) and not bool((out == SENTINEL).any())
        x = [out]
    pflat, pose = guarded((2, 4, 4))
    dflat, dof = guarded((2, 6))
    kb.ops.pose_head(x[0], m.decoder.conv.conv.weight, out=pose, dof_out=dof)
    torch.cuda.synchronize()
    assert intact(pflat) and intact(dflat)
    assert torch.equal(pose, free[0]) and torch.equal(dof, free[1])


def test_wrappers_refuse_what_the_kernels_do_not_take(dev, full):
    m, _ = full
    layer = m.encoder.conv3
    x = torch.zeros(1, 32, 8, 8, device=dev)
    scale, shift = layer.affine()
    with pytest.raises(kb._lib.KbnError):
        kb.ops.conv2d_s2_affine([x.cpu()], layer.packed(), scale, shift, 64, 3)
    with pytest.raises(kb._lib.KbnError):
        kb.ops.conv2d_s2_affine([x], layer.packed(), scale[:-1], shift, 64, 3)
    with pytest.raises(kb._lib.KbnError):
        kb.ops.conv2d_s2_affine([x, x], layer.packed(), scale, shift, 64, 3)        # 64 input channels: another packed size
    with pytest.raises(kb._lib.KbnError):
        kb.ops.conv2d_s2_affine([x], layer.packed(), scale, shift, 64, 1)
    with pytest.raises(kb._lib.KbnError):
        kb.ops.pose_head(torch.zeros(1, 256, 2, 2, device=dev), torch.zeros(6, 128, 1, 1, device=dev))
    with pytest.raises(kb._lib.KbnError):
        m.forward(torch.zeros(1, 3, 16, 16, device=dev), torch.zeros(1, 3, 16, 18, device=dev))


def test_changed_weights_and_statistics_are_repacked(dev):
    enc, dec = kb.synthetic.make_posenet_weights(NARROW, seed=6)
    m = _narrow(dev, enc, dec)
    i0, i1 = [t.to(dev) for t in kb.synthetic.make_image_pair(1, 40, 56, seed=33)]
    first = m.forward(i0, i1).clone()
    m.encoder.conv2.batch_norm.running_var.mul_(2.0)
    second = m.forward(i0, i1).clone()
    assert not torch.equal(first, second)
    m.encoder.conv4.conv.weight.mul_(0.5)
    third = m.forward(i0, i1).clone()
    assert not torch.equal(second, third)
    m.load_state_dicts(enc, dec)
    assert torch.equal(m.forward(i0, i1), first)


def test_poses_feed_compute_loss(dev, full):
    """image0 / image1 / image2 -> two poses from PoseNetModel -> KBNetModel.compute_loss, against the loss oracle fed the pose
    oracle's poses, at the gates of tests/test_loss_gpu.py (terms 2e-5 relative; images 3 x the oracle's own fp32 distance and 1e-4)."""
    m, (enc64, dec64) = full
    i0, i1, i2, depth, sparse, validity, k, _, _ = kb.synthetic.make_triplet(2, 64, 96, "kitti", seed=12)
    poses64 = [po.forward(i0.double(), other.double(), enc64, dec64)["pose"] for other in (i1, i2)]
    assert all(float(p[:, :3, 3].abs().max()) < 0.5 * float(depth.min()) for p in poses64)        # every point stays in front
    args = [i0, i1, i2, depth, sparse, validity, k]
    want64 = lo.compute_loss(*[a.double() for a in args], *poses64)
    own32 = lo.compute_loss(*args, *[p.float() for p in poses64])
    d0, d1, d2 = i0.to(dev), i1.to(dev), i2.to(dev)
    pose01, pose02 = m.forward(d0, d1), m.forward(d0, d2)
    kbnet = kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), dev)
    loss, info = kbnet.compute_loss(d0, d1, d2, depth.to(dev), sparse.to(dev), validity.to(dev), k.to(dev), pose01, pose02)
    terms = {t: abs(float(info[t]) - float(want64[t])) / abs(float(want64[t]))
             for t in ("loss_color", "loss_structure", "loss_sparse_depth", "loss_smoothness", "loss")}
    images = {t: (float((info[t].double().cpu() - want64[t]).abs().max()), float((own32[t].double() - want64[t]).abs().max()))
              for t in ("image01", "image02")}
    print("poses -> loss:", " ".join(f"{t} {v:.2e}" for t, v in terms.items()),
          " ".join(f"{t} {v:.2e} (fp32 oracle {d:.2e})" for t, (v, d) in images.items()))
    for t, v in terms.items():
        assert v <= 2e-5, (t, v)
    for t, (v, d) in images.items():
        assert v <= 3 * d and v <= 1e-4, (t, v, d)
