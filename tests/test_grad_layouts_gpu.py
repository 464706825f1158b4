"""GPU: the gradient layouts autograd hands to the recorded nodes of ops.py, and the training step on a side stream.

Every test of the backward passes calls y.backward(g) with a dense g.  Autograd also hands over an expanded stride-0 tensor (what
.sum().backward() produces), channels-last tensors, channel slices of wider tensors and slices with a step in W.  Every node must give
the bits of its dense call on each of them: a backward that reads the strides it was not written for is wrong, one that refuses them
breaks loss.backward().  The problems are 2 x C x 9 x 13 with values exactly representable in fp32; the yardstick is the node's own
dense call, whose values the operator tests hold against fp64.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch

import kbnet_amd as kb

import kbnet_grad_cases as kcases
import posenet_grad_cases as pcases
import posenet_grad_oracle as pgo
import resnet_pose_grad_cases as rcases

pytestmark = pytest.mark.gpu
ops = kb.ops
N, H, W = 2, 9, 13


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).float()


def _leaf(shape, seed, dev, scale=1.0):
    return _rand(shape, seed, scale).to(dev).requires_grad_(True)


def _conv(fn, channels, oc, k, seed, **kw):
    def build(dev):
        xs = [_leaf((N, c, H, W), seed + i, dev) for i, c in enumerate(channels)]
        weight = _leaf((oc, sum(channels), k, k), seed + 10, dev, 1.0 / (sum(channels) * k * k) ** 0.5)
        return fn(xs, weight, **kw), xs + [weight]
    return build


def _batch_norm(batch):
    def build(dev):
        c = pcases.bn_case(0.2, batch, n=N, c=5, h=H, w=W)
        u, gamma, beta = (c[k].float().to(dev).requires_grad_(True) for k in ("u", "gamma", "beta"))
        mean, var = ops.batch_norm_stats(u.detach()) if batch else (c["mean"].float().to(dev), c["var"].float().to(dev))
        return ops.batch_norm_act(u, gamma, beta, mean, var, pgo.EPS, 0.2, batch), [u, gamma, beta]
    return build


def _maxpool(dev):
    x = _leaf((N, 5, H, W), 21, dev)
    return ops.maxpool3x3s2(x), [x]


def _add_act(dev):
    a, b = _leaf((N, 5, H, W), 22, dev), _leaf((N, 5, H, W), 23, dev)
    return ops.add_act(a, b, 0.2), [a, b]


def _resize(dev):
    x = _leaf((N, 5, H, W), 24, dev)
    return ops.resize_nearest(x, 17, 25), [x]


def _kb_xyz(dev):
    depth, weight = _leaf((N, 5, H, W), 25, dev), _leaf((1, 5, 1, 1), 26, dev, 0.5)
    return ops.kb_xyz(depth, weight, _rand((N, 3, H, W), 27).to(dev), 0.2)[0], [depth, weight]


def _depth_map(dev):
    logits = _leaf((N, 1, H, W), 28, dev, 3.0)
    return ops.depth_map(logits, 1.5, 100.0), [logits]


def _loss(dev):
    *frames, v01, v02 = kb.synthetic.make_triplet(N, H, W, "kitti", seed=12)
    args = [t.to(dev) for t in frames] + [ops.pose_matrix(v01).to(dev), ops.pose_matrix(v02).to(dev)]
    leaves = [args[i].detach().clone().requires_grad_(True) for i in (3, 7, 8)]
    args[3], args[7], args[8] = leaves
    return ops.photometric_loss(*args), leaves


NODES = {
    "conv2d_s2 k3 one input": _conv(ops.conv2d_s2, (5,), 19, 3, 100),
    "conv2d_s2 k5 two inputs": _conv(ops.conv2d_s2, (5, 4), 19, 5, 110),
    "conv2d_s2 k7 two inputs": _conv(ops.conv2d_s2, (3, 3), 10, 7, 120),
    "conv2d_pose k3 s1": _conv(ops.conv2d_pose, (5,), 19, 3, 130, stride=1),
    "conv2d_pose k1 s1": _conv(ops.conv2d_pose, (5,), 19, 1, 140, stride=1),
    "conv2d_pose k1 s2": _conv(ops.conv2d_pose, (5,), 19, 1, 150, stride=2),
    "conv2d_pose k3 s2 two inputs": _conv(ops.conv2d_pose, (5, 4), 19, 3, 160, stride=2),
    "conv2d_kbnet k3 s1 act one input": _conv(ops.conv2d_kbnet, (5,), 19, 3, 170, stride=1, negative_slope=0.2),
    "conv2d_kbnet k3 s2 linear two inputs": _conv(ops.conv2d_kbnet, (5, 4), 19, 3, 180, stride=2, negative_slope=None),
    "conv2d_kbnet k1 s1 relu three inputs": _conv(ops.conv2d_kbnet, (3, 5, 7), 19, 1, 190, stride=1, negative_slope=0.0),
    "conv2d_kbnet k1 s2 act three inputs": _conv(ops.conv2d_kbnet, (3, 5, 7), 19, 1, 200, stride=2, negative_slope=0.2),
    "conv2d_kbnet k3 s2 act three inputs": _conv(ops.conv2d_kbnet, (3, 5, 7), 19, 3, 210, stride=2, negative_slope=0.2),
    "batch_norm_act running": _batch_norm(False),
    "batch_norm_act batch": _batch_norm(True),
    "maxpool3x3s2": _maxpool,
    "add_act": _add_act,
    "resize_nearest": _resize,
    "kb_xyz": _kb_xyz,
    "depth_map": _depth_map,
    "photometric_loss": _loss,
}


def _layouts(g):
    """The values of the dense `g` in the layouts autograd hands over -> name -> tensor."""
    out = {}
    if g.dim() == 4:
        n, c, h, w = g.shape
        out["channels-last"] = g.contiguous(memory_format=torch.channels_last)
        wide = torch.full((n, c + 5, h, w), -7.0, device=g.device, dtype=g.dtype)
        wide[:, 2:2 + c] = g
        out["a channel slice"] = wide[:, 2:2 + c]
    else:
        out["transposed"] = g.t().contiguous().t()
        wide = torch.full((g.shape[0], g.shape[1] + 5), -7.0, device=g.device, dtype=g.dtype)
        wide[:, 2:2 + g.shape[1]] = g
        out["a column slice"] = wide[:, 2:2 + g.shape[1]]
    stepped = torch.full(tuple(g.shape[:-1]) + (2 * g.shape[-1],), -7.0, device=g.device, dtype=g.dtype)
    stepped[..., ::2] = g
    out["a step in the last axis"] = stepped[..., ::2]
    for name, t in out.items():
        assert torch.equal(t, g) and (g.numel() == 1 or name == "channels-last" or not t.is_contiguous()), name
    return out


def _backward(build, dev, cotangent):
    """One forward and one backward of the node -> its leaves' gradients.  `cotangent`: y -> the tensor for y.backward, or None for
    the real y.sum().backward()."""
    y, leaves = build(dev)
    assert y.grad_fn is not None
    if cotangent is None:
        y.sum().backward()
    else:
        y.backward(cotangent(y))
    assert all(t.grad is not None for t in leaves)
    return [t.grad.clone() for t in leaves]


def _same(label, got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), f"{label}: the gradient of leaf {i} differs from the dense cotangent's"


@pytest.mark.parametrize("name", list(NODES))
def test_every_cotangent_layout_gives_the_dense_calls_bits(dev, name):
    build = NODES[name]
    y, _ = build(dev)
    g = _rand(tuple(y.shape), 99).to(dev).to(y.dtype)
    assert (tuple(y.shape) == (N, 8)) == (name == "photometric_loss") and (y.dim() == 4 or name == "photometric_loss")
    dense = _backward(build, dev, lambda y: g)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in dense), name
    _same(f"{name}, the dense cotangent again", _backward(build, dev, lambda y: g.clone()), dense)
    for layout, t in _layouts(g).items():
        _same(f"{name}, {layout}", _backward(build, dev, lambda y: t), dense)
    # a constant: dense, the stride-0 expand of a scalar, and what .sum().backward() hands over
    ones = _backward(build, dev, lambda y: torch.ones_like(y))
    scalar = torch.ones((), device=dev, dtype=y.dtype)
    assert scalar.expand(y.shape).stride() == (0,) * y.dim()
    _same(f"{name}, an expanded scalar", _backward(build, dev, lambda y: scalar.expand(y.shape)), ones)
    _same(f"{name}, .sum().backward()", _backward(build, dev, None), ones)


def _spy(monkeypatch, name, seen, what):
    real = getattr(ops, name)

    def wrapper(*args, **kwargs):
        out = real(*args, **kwargs)
        seen.append(what(args, out))
        return out
    monkeypatch.setattr(ops, name, wrapper)


def test_kb_xyz_reads_the_fused_convs_channel_slice_in_place(dev, monkeypatch):
    """A KB level as kbnet_train._kb_block builds it: xyz is the middle input of conv_fused, so its gradient arrives as a channel
    slice of that conv's one data-gradient buffer.  _KbXyz.backward must hand THAT tensor to kb_xyz_backward (no dense copy), in one
    kb_xyz_bwd launch."""
    image, depth, fused = _leaf((N, 6, H, W), 1, dev), _leaf((N, 5, H, W), 2, dev), _leaf((N, 7, H, W), 3, dev)
    w_proj, w_fused = _leaf((1, 5, 1, 1), 4, dev, 0.5), _leaf((19, 16, 3, 3), 5, dev, 1.0 / 12.0)
    coords = _rand((N, 3, H, W), 6).to(dev)
    buffers, handed = [], []
    _spy(monkeypatch, "conv2d_s2_backward_data", buffers, lambda args, out: out[0])
    _spy(monkeypatch, "kb_xyz_backward", handed, lambda args, out: args[2])
    xyz, _ = ops.kb_xyz(depth, w_proj, coords, 0.2)
    y = ops.conv2d_kbnet([image, xyz, fused], w_fused, 2, 0.2)
    ops.PROFILE = []
    try:
        y.backward(_rand(tuple(y.shape), 7).to(dev))
        names = [r[0].split("<")[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert names.count("kb_xyz_bwd") == 1, names
    assert names == ["add_act_bwd", "conv_s2_bwd_weight", "conv_s2_bwd_weight", "conv_s2_bwd_data", "kb_xyz_bwd", "conv_bwd_weight",
                     "conv_affine"], names
    assert len(buffers) == 1 and len(handed) == 1
    buf, g = buffers[0], handed[0]
    assert tuple(buf.shape) == (N, 16, H, W) and tuple(g.shape) == (N, 3, H, W)
    assert g.data_ptr() == buf[:, 6:9].data_ptr() and g.stride() == buf.stride() and not g.is_contiguous()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (image, depth, fused, w_proj, w_fused))


def test_the_depth_network_hands_kb_xyz_slices_and_nothing_is_copied(dev, monkeypatch):
    """The same through KBNetModel(trainable=True): one kb_xyz_bwd launch per KB level, every one on a channel slice read in place."""
    c = kcases.MODEL["tiny_n3"]
    args = kcases.inputs(c)
    m = kb.modules.KBNetModel.from_config(c["cfg"], dev, trainable=True)
    m.load_state_dicts(*args[4:7])
    handed = []
    _spy(monkeypatch, "kb_xyz_backward", handed, lambda a, out: a[2])
    depth = m.forward(*[t.to(dev) for t in args[:4]])
    ops.PROFILE = []
    try:
        (depth * args[7].float().to(dev)).sum().backward()
        names = [r[0].split("<")[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    levels = len(c["cfg"].resolutions_backprojection)
    assert levels == 4 and names.count("kb_xyz_bwd") == levels == len(handed), names
    for g in handed:
        n, ch, h, w = g.shape
        assert ch == 3 and g.stride(1) == h * w and g.stride(2) == w and g.stride(3) == 1      # dense planes ...
        assert g.stride(0) > 3 * h * w                                                          # ... of a wider buffer: read in place, no copy


# ---------------------------------------------------------------- the training step on a side stream
def _pose_step(model, dev):
    i0, i1, i2, depth, sparse, validity, k, _, _ = [t.to(dev) for t in kb.synthetic.make_triplet(3, 33, 47, "kitti", seed=12)]
    loss_of = kb.modules.KBNetModel.from_config(kb.kitti_config().narrow(), dev)

    def step():
        pose01, pose02 = model.forward(i0, i1), model.forward(i0, i2)
        assert pose01.grad_fn is not None
        loss, _ = loss_of.compute_loss(i0, i1, i2, depth, sparse, validity, k, pose01, pose02)
        loss.backward()
    return step


def _posenet(dev):
    c = pcases.MODEL["narrow_n3_running"]
    _, _, enc, dec, _ = pcases.inputs(c)
    m = kb.modules.PoseNetModel(device=dev, n_filters=c["filters"])
    m.load_state_dicts(enc, dec)
    m.requires_grad_(True).set_batch_norm("running")
    return m, _pose_step(m, dev)


def _resnet(dev):
    c = rcases.MODEL["narrow_18_n3_running"]
    _, _, enc, dec, _ = rcases.inputs(c)
    m = kb.posenet_resnet.ResNetPoseNetModel(n_layer=18, device=dev, n_filters=c["filters"], decoder_filters=c["decoder_filters"], trainable=True)
    m.load_state_dicts(enc, dec)
    m.requires_grad_(True).set_batch_norm("running")
    return m, _pose_step(m, dev)


def _kbnet(dev):
    c = kcases.MODEL["tiny_n3"]
    m = kb.modules.KBNetModel.from_config(c["cfg"], dev, trainable=True)
    m.load_state_dicts(*kcases.inputs(c)[4:7])
    i0, i1, i2, _, sparse, validity, k, v01, v02 = [t.to(dev) for t in kb.synthetic.make_triplet(3, 33, 47, "kitti", seed=12)]
    pose01, pose02 = ops.pose_matrix(v01), ops.pose_matrix(v02)

    def step():
        depth = m.forward(i0, sparse, validity, k)
        assert depth.grad_fn is not None
        loss, _ = m.compute_loss(i0, i1, i2, depth, sparse, validity, k, pose01, pose02)
        loss.backward()
    return m, step


def _take_grads(model):
    out = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    for p in model.parameters():
        p.grad = None
    return out


@pytest.mark.parametrize("make", [_posenet, _resnet, _kbnet], ids=["PoseNetModel", "ResNetPoseNetModel", "KBNetModel"])
def test_a_training_step_on_a_side_stream_gives_the_default_streams_bits(dev, make):
    """forward, compute_loss and backward inside torch.cuda.stream(side): every launch follows torch's current stream,
    so the parameter gradients are the default stream's, bit for bit."""
    model, step = make(dev)
    step()
    torch.cuda.synchronize()
    want = _take_grads(model)
    assert sum(g is not None for g in want) >= 20 and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in want if g is not None)
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    side.synchronize()
    torch.cuda.synchronize()
    got = _take_grads(model)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f"parameter {i} differs on the side stream"
