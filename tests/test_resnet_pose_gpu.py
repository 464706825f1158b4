"""GPU: ResNetPoseNetModel (csrc/conv_affine.hip: kbn_conv2d_affine_forward, kbn_maxpool3x3s2_forward; the head of csrc/posenet.hip)
against the vectors captured from the reference's ResNetEncoder / PoseDecoder in eval mode (fp64 evaluation) and against
tests/resnet_pose_oracle.py in fp64, and the two new operators against torch in fp64.

Gate (tests/posenet_oracle.py, the one of tests/test_posenet_gpu.py): |a - b| <= 1e-4 |b| + floor
  layers   floor = 1e-4 x the layer tensor's RMS (conv1, the pool, every block, the decoder's hidden layers)
  dof      and the translation column of the pose: floor = 1e-4 x 0.01 x RMS of the 6-channel map (the tensor that is averaged)
  pose     equals ops.pose_matrix(dof of the kernel) bit for bit: the rotation block has no tolerance of its own
The operator tests use the layer rule on the operator's output (fp32 sums of at most 20 x 49 exact products stay orders below it);
the pool selects, so it equals torch exactly.  tests/test_resnet_pose_cpu.py proves that the dof gate sees a skipped projection, a
dropped activation on conv2 or after the add, zero pool padding, slope 0.10, a dropped eps and a stride-2 block in stage 1.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch
import torch.nn.functional as F

import kbnet_amd as kb
from conftest import load_golden

import loss_oracle as lo
import posenet_oracle as po
import resnet_pose_oracle as ro

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e30
GUARD = 1024
KbnError = kb._lib.KbnError


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _full(dev, n_layer):
    enc, dec = kb.synthetic.make_resnet_pose_weights(n_layer, seed=5)
    m = kb.modules.ResNetPoseNetModel(n_layer, device=dev)
    m.load_state_dicts(enc, dec)
    return m, po.to64(enc, dec)


@pytest.fixture(scope="module")
def full18(dev):
    """The default-width ResNet-18 model with synthetic weights, and those weights in fp64 for the oracle (shared, never modified)."""
    return _full(dev, 18)


@pytest.fixture(scope="module")
def full34(dev):
    return _full(dev, 34)


def _golden_model(dev, name):
    g = load_golden(name)
    enc = {k: torch.as_tensor(v) for k, v in g["enc"].items()}
    dec = {k: torch.as_tensor(v) for k, v in g["dec"].items()}
    n_layer = int(g["n_layer"])
    filters = [enc["conv1.conv.weight"].shape[0]] + [enc[f"blocks{s}.0.conv1.conv.weight"].shape[0] for s in range(2, 6)]
    m = kb.modules.ResNetPoseNetModel(n_layer, device=dev, n_filters=filters,
                                      decoder_filters=[dec["conv.0.conv.weight"].shape[0], dec["conv.1.conv.weight"].shape[0]])
    m.load_state_dicts(enc, dec)
    return g, m, n_layer, (enc, dec)


def _check(label, got, want, n_layer):
    """`got`: (pose, dof, layers) of ResNetPoseNetModel.forward(return_all=True); `want`: fp64 'layers' / 'map' / 'dof' / 'pose'.
    Prints every figure (as a fraction of its gate) before it asserts."""
    pose, dof, layers = got
    assert pose.dtype == torch.float32 and tuple(pose.shape) == (dof.shape[0], 4, 4) and tuple(dof.shape) == (dof.shape[0], 6)
    layer_names = ro.names(n_layer)
    figures = {}
    assert len(layers) == len(want["layers"]) == len(layer_names)
    for k, a, b in zip(layer_names, layers, want["layers"]):
        assert tuple(a.shape) == tuple(b.shape), (label, k, a.shape, b.shape)
        figures[k] = po.gate_fraction(a, b, po.layer_floor(b))
    floor = po.dof_floor(want["map"])
    figures["dof"] = po.gate_fraction(dof, want["dof"], floor)
    figures["translation"] = po.gate_fraction(pose[:, :3, 3], want["pose"][:, :3, 3], floor)
    rotation = float((pose[:, :3, :3].double().cpu() - want["pose"][:, :3, :3]).abs().max())
    exact = torch.equal(pose, kb.ops.pose_matrix(dof))
    print(label, " ".join(f"{k} {v:.3f}" for k, v in figures.items()), f"(fractions of the gate)  rotation block {rotation:.2e} from fp64,"
          f" pose == pose_matrix(dof): {exact}")
    for k, v in figures.items():
        assert v <= 1.0, (label, k, v)
    assert exact, (label, pose, kb.ops.pose_matrix(dof))
    assert torch.equal(pose[:, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(pose.shape[0], 4))


@pytest.mark.parametrize("name", ["resnet_pose_18_odd", "resnet_pose_34_wide"])
def test_resnet_pose_golden(dev, name):
    g, m, n_layer, _ = _golden_model(dev, name)
    got = m.forward(g["image0"].to(dev), g["image1"].to(dev), return_all=True)
    want = {"layers": [g["ref64"][k] for k in ro.names(n_layer)], "map": g["ref64"]["map"], "dof": g["ref64"]["dof"],
            "pose": g["ref64"]["pose"]}
    _check(name, got, want, n_layer)
    assert torch.equal(m.forward(g["image0"].to(dev), g["image1"].to(dev)), got[0])


@pytest.mark.parametrize("shape", [(2, 61, 77), (1, 128, 416), (1, 352, 1216)], ids=lambda s: "x".join(map(str, s)))
def test_resnet18_full_width_vs_oracle(dev, full18, shape):
    m, (enc64, dec64) = full18
    n, h, w = shape
    i0, i1 = kb.synthetic.make_image_pair(n, h, w, seed=20 + n + h)
    want = ro.forward(i0.double(), i1.double(), enc64, dec64, 18)
    _check("resnet18 " + "x".join(map(str, shape)), m.forward(i0.to(dev), i1.to(dev), return_all=True), want, 18)
    if n > 1:
        assert float((want["dof"][0] - want["dof"][1]).abs().max()) > 100 * po.dof_floor(want["map"])    # the frames differ


def test_resnet34_full_width_vs_oracle(dev, full34):
    m, (enc64, dec64) = full34
    i0, i1 = kb.synthetic.make_image_pair(1, 61, 77, seed=82)
    want = ro.forward(i0.double(), i1.double(), enc64, dec64, 34)
    _check("resnet34 1x61x77", m.forward(i0.to(dev), i1.to(dev), return_all=True), want, 34)


# ---------------------------------------------------------------- the operators
def _conv_case(dev, k, stride, residual, n=3, cin=(20,), cout=24, h=13, w=19, seed=0):
    """conv2d_affine on the device and the same in fp64 with torch: (got, want)."""
    g = torch.Generator().manual_seed(1000 * k + 10 * stride + int(residual) + seed)
    xs = [torch.randn(n, c, h, w, generator=g) for c in cin]
    weight = torch.randn(cout, sum(cin), k, k, generator=g) / (sum(cin) * k * k) ** 0.5
    scale, shift = 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g)
    oh, ow = -(-h // stride), -(-w // stride)
    res = torch.randn(n, cout, oh, ow, generator=g) if residual else None
    y = F.conv2d(torch.cat(xs, 1).double(), weight.double(), None, stride=stride, padding=k // 2)
    y = F.leaky_relu(y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1), 0.2)
    if residual:
        y = F.leaky_relu(y + res.double(), 0.2)
    got = kb.ops.conv2d_affine([x.to(dev) for x in xs], kb.ops.pack_conv2d_affine_weight(weight.to(dev)), scale.to(dev), shift.to(dev),
                               cout, k, stride=stride, negative_slope=0.2, residual=res.to(dev) if residual else None)
    return got, y


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_conv2d_affine_against_torch_fp64(dev, k, stride, residual):
    """20 -> 24 channels on 3 x 13 x 19: K = 20, 180, 980 (none a multiple of the 32-deep chunk), 24 filters in a 32-filter tile,
    741 or 210 pixels (six or two 128-pixel tiles, the last one partial and spanning frames)."""
    got, want = _conv_case(dev, k, stride, residual)
    assert tuple(got.shape) == tuple(want.shape) == (3, 24, -(-13 // stride), -(-19 // stride))
    fraction = po.gate_fraction(got, want, po.layer_floor(want))
    print(f"conv2d_affine k {k} stride {stride} residual {residual}: {fraction:.4f} of the gate")
    assert fraction <= 1.0


def test_conv2d_affine_two_sources_and_no_activation(dev):
    """Two sources read in place (3 + 3 channels, as conv1 reads the two images) equal the concat; 70 filters take two 64-filter
    tiles; negative_slope=None applies no activation, before or after the residual."""
    got, want = _conv_case(dev, 7, 2, False, n=2, cin=(3, 3), cout=70, h=21, w=30, seed=5)
    assert po.gate_fraction(got, want, po.layer_floor(want)) <= 1.0
    g = torch.Generator().manual_seed(77)
    a, b = torch.randn(2, 3, 9, 11, generator=g).to(dev), torch.randn(2, 5, 9, 11, generator=g).to(dev)
    weight = torch.randn(12, 8, 3, 3, generator=g)
    res = torch.randn(2, 12, 9, 11, generator=g)
    packed = kb.ops.pack_conv2d_affine_weight(weight.to(dev))
    ones, zeros = torch.ones(12, device=dev), torch.zeros(12, device=dev)
    two = kb.ops.conv2d_affine([a, b], packed, ones, zeros, 12, 3, stride=1, negative_slope=None, residual=res.to(dev))
    one = kb.ops.conv2d_affine([torch.cat([a, b], 1)], packed, ones, zeros, 12, 3, stride=1, negative_slope=None, residual=res.to(dev))
    assert torch.equal(two, one)
    want = F.conv2d(torch.cat([a, b], 1).double().cpu(), weight.double(), None, padding=1) + res.double()
    assert float(want.min()) < -1.0 and po.gate_fraction(two, want, po.layer_floor(want)) <= 1.0


@pytest.mark.parametrize("shape", [(2, 5, 13, 19), (1, 3, 8, 6), (2, 2, 1, 7), (1, 1, 2, 1)], ids=lambda s: "x".join(map(str, s)))
def test_maxpool3x3s2_equals_torch(dev, shape):
    """Odd and even sizes; every value negative, so a zero (padding that wins) would show; one NaN, which torch propagates."""
    g = torch.Generator().manual_seed(sum(shape))
    x = -0.5 - torch.rand(shape, generator=g)
    x[0, 0, shape[2] // 2, shape[3] // 2] = float("nan")
    want = F.max_pool2d(x.double(), 3, stride=2, padding=1)
    got = kb.ops.maxpool3x3s2(x.to(dev))
    assert tuple(got.shape) == tuple(want.shape) == (shape[0], shape[1], (shape[2] + 1) // 2, (shape[3] + 1) // 2)
    assert int(torch.isnan(want).sum()) >= 1 and bool((want[~torch.isnan(want)] < 0).all())
    assert torch.equal(torch.isnan(got).cpu(), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got.double().cpu(), nan=0.0), torch.nan_to_num(want, nan=0.0))


# ---------------------------------------------------------------- the batch axis
def test_frame_permutation_permutes_the_outputs_bit_for_bit(dev, full18):
    m, _ = full18
    i0, i1 = [t.to(dev) for t in kb.synthetic.make_image_pair(5, 61, 77, seed=31)]
    perm = torch.tensor([3, 0, 4, 1, 2], device=dev)
    pose, dof, layers = m.forward(i0, i1, return_all=True)
    ppose, pdof, players = m.forward(i0[perm].contiguous(), i1[perm].contiguous(), return_all=True)
    assert torch.equal(ppose, pose[perm]) and torch.equal(pdof, dof[perm])
    assert all(torch.equal(a, b[perm]) for a, b in zip(players, layers))
    assert len({tuple(r.tolist()) for r in dof.cpu()}) == 5          # a permutation that is ignored would show
    apose, adof, alayers = m.forward(i0[2:3], i1[2:3], return_all=True)
    assert torch.equal(apose[0], pose[2]) and torch.equal(adof[0], dof[2])       # a frame alone = that frame in the batch
    assert all(torch.equal(a[0], b[2]) for a, b in zip(alayers, layers))


# ---------------------------------------------------------------- memory
def test_outputs_stay_inside_guarded_buffers(dev):
    """Every launch of the narrow ResNet-18 at an odd size (pixel counts that are no multiple of the 128-pixel tile, filter counts
    that are no multiple of the filter tile, maps down to 1 x 1) -- conv1, the pool, each block's conv1, projection and conv2, the
    decoder's convs and the head -- writes into the middle of a buffer of sentinels."""
    g, m, n_layer, _ = _golden_model(dev, "resnet_pose_18_odd")
    i0, i1 = g["image0"].to(dev), g["image1"].to(dev)
    free = m.forward(i0, i1, return_all=True)

    def guarded(shape):
        count = 1
        for s in shape:
            count *= s
        flat = torch.full((count + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.float32)
        return flat, flat[GUARD:GUARD + count].view(shape)

    def intact(flat):
        return bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all())

    def run(what, shape, launch, want=None):
        flat, out = guarded(tuple(shape))
        launch(out)
        torch.cuda.synchronize()
        assert intact(flat), f"{what} wrote outside its output"
        assert not bool((out == SENTINEL).any()), f"{what} left part of its output unwritten"
        if want is not None:
            assert torch.equal(out, want), what
        return out

    layers = free[2]
    x = run("conv1", layers[0].shape, lambda out: m.encoder.conv1.run([i0, i1], out=out), layers[0])
    x = run("pool", layers[1].shape, lambda out: kb.ops.maxpool3x3s2(x, out=out), layers[1])
    projections = 0
    for block, want in zip(m.encoder.blocks(), layers[2:]):
        h = run("block conv1", want.shape, lambda out: block.conv1.run([x], out=out))
        skip = x
        if block.projects(x):
            skip = run("block projection", want.shape, lambda out: block.projection.run([x], out=out))
            projections += 1
        x = run("block conv2", want.shape, lambda out: block.conv2.run([h], residual=skip, out=out), want)
    assert projections == 4
    for layer, want in zip(m.decoder.hidden(), layers[2 + len(m.encoder.blocks()):]):
        x = run("decoder conv", want.shape, lambda out: layer.run([x], out=out), want)
    pflat, pose = guarded((2, 4, 4))
    dflat, dof = guarded((2, 6))
    kb.ops.pose_head(x, m.decoder.conv[-1].conv.weight, out=pose, dof_out=dof)
    torch.cuda.synchronize()
    assert intact(pflat) and intact(dflat)
    assert torch.equal(pose, free[0]) and torch.equal(dof, free[1])


# ---------------------------------------------------------------- the host mirror
def test_changed_weights_and_statistics_are_repacked(dev):
    g, m, n_layer, (enc, dec) = _golden_model(dev, "resnet_pose_34_wide")
    i0, i1 = g["image0"].to(dev), g["image1"].to(dev)
    first = m.forward(i0, i1).clone()
    m.encoder.blocks3[1].conv2.batch_norm.running_var.mul_(2.0)
    second = m.forward(i0, i1).clone()
    assert not torch.equal(first, second)
    m.encoder.blocks4[0].projection.conv.weight.mul_(0.5)
    third = m.forward(i0, i1).clone()
    assert not torch.equal(second, third)
    m.decoder.conv[1].conv.weight.mul_(0.5)
    fourth = m.forward(i0, i1).clone()
    assert not torch.equal(third, fourth)
    m.load_state_dicts(enc, dec)
    m.refresh_packed()
    assert torch.equal(m.forward(i0, i1), first)


def test_wrappers_refuse_what_the_kernels_do_not_take(dev, full18):
    m, _ = full18
    layer = m.encoder.blocks3[0].conv1                       # 32 -> 64, 3 x 3, stride 2
    x = torch.zeros(1, 32, 8, 8, device=dev)
    scale, shift = layer.affine()
    args = (layer.packed(), scale, shift, 64, 3)
    kb.ops.conv2d_affine([x], *args, stride=2)
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x.cpu()], *args, stride=2)
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x], layer.packed(), scale[:-1], shift, 64, 3, stride=2)
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x, x], *args, stride=2)                            # 64 input channels: another packed size
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x], layer.packed(), scale, shift, 64, 5, stride=2)
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x], *args, stride=3)
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x], *args, stride=2, residual=torch.zeros(1, 64, 8, 8, device=dev))     # the output is 4 x 4
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x], *args, stride=2, out=torch.zeros(1, 64, 8, 8, device=dev))
    with pytest.raises(KbnError):
        kb.ops.conv2d_affine([x], m.encoder.conv1.packed(), scale, shift, 64, 3, stride=2)            # another layer's blob
    with pytest.raises(KbnError):
        kb.ops.pack_conv2d_affine_weight(torch.zeros(8, 8, 5, 5, device=dev))
    with pytest.raises(KbnError):
        kb.ops.maxpool3x3s2(torch.zeros(4, 8, 8, device=dev))
    with pytest.raises(KbnError):
        kb.ops.maxpool3x3s2(x, out=torch.zeros(1, 32, 8, 8, device=dev))
    with pytest.raises(KbnError):
        kb.ops.maxpool3x3s2(x.double())
    with pytest.raises(KbnError):
        m.forward(torch.zeros(1, 3, 16, 16, device=dev), torch.zeros(1, 3, 16, 18, device=dev))


def test_resnet_poses_feed_compute_loss(dev, full18):
    """image0 / image1 / image2 -> two poses from ResNetPoseNetModel -> KBNetModel.compute_loss, against the loss oracle fed the pose
    oracle's poses, at the gates of tests/test_posenet_gpu.py::test_poses_feed_compute_loss (terms 2e-5 relative; images 3 x the
    oracle's own fp32 distance and 1e-4)."""
    m, (enc64, dec64) = full18
    i0, i1, i2, depth, sparse, validity, k, _, _ = kb.synthetic.make_triplet(2, 64, 96, "kitti", seed=12)
    poses64 = [ro.forward(i0.double(), other.double(), enc64, dec64, 18)["pose"] for other in (i1, i2)]
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
    print("resnet poses -> loss:", " ".join(f"{t} {v:.2e}" for t, v in terms.items()),
          " ".join(f"{t} {v:.2e} (fp32 oracle {d:.2e})" for t, (v, d) in images.items()))
    for t, v in terms.items():
        assert v <= 2e-5, (t, v)
    for t, (v, d) in images.items():
        assert v <= 3 * d and v <= 1e-4, (t, v, d)
