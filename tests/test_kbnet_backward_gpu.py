"""GPU: the operators of the depth network's backward pass (csrc/kbnet_backward.hip and the conv node ops.conv2d_kbnet) one by one.
Inputs are exactly representable in fp32; the yardsticks are fp64 torch autograd on the CPU.

  resize forward            bit-equal to F.interpolate(mode='nearest')
  resize backward           per element within (m - 1) 2^-24 sum|addends| for a pixel with m addends: the fixed-order fp32 sum
  kb_xyz_backward           per element within 8 x 2^-24 sum|terms|: three products and two sums, each rounded once, with room
  depth_map_backward        kbnet_grad_oracle.DEPTH_MAP_TOL of |b| + rms(b): 3 x torch's own fp32 autograd of the expression
  conv node                 posenet_grad_oracle.TOL of |b| + rms(b), the bar of the operator tests of these gradient kernels
Every output is written exactly once (guard values around the output buffers stay intact) and two runs give equal bits.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch
import torch.nn.functional as F

import kbnet_amd as kb
KbnError = kb._lib.KbnError

import kbnet_grad_cases as cases
import kbnet_grad_oracle as kgo
import posenet_grad_oracle as pgo
import posenet_oracle as po

pytestmark = pytest.mark.gpu
ops = kb.ops
EPS = 2.0 ** -24
GUARD = 12345.0

RESIZE_SHAPES = [  # (n, c, h, w, H, W)
    (1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 2, 2), (1, 2, 2, 3, 4, 6), (2, 2, 3, 5, 5, 9), (1, 3, 12, 20, 23, 39), (1, 2, 23, 39, 45, 77),
    (1, 1, 2, 3, 7, 8), (3, 5, 6, 8, 11, 16), (2, 3, 5, 8, 5, 8), (1, 2, 4, 8, 8, 13),
]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).float().double()


def _guarded(shape, dev, channels_extra=2):
    """A channel slice of a larger buffer full of GUARD, with a frame of slack before and after -> (the whole buffer, the view)."""
    n, c, h, w = shape
    whole = torch.full((n + 2, c + channels_extra, h, w), GUARD, device=dev, dtype=torch.float32)
    return whole, whole[1:n + 1, 1:c + 1]


def _guards_intact(whole, shape):
    n, c = shape[:2]
    mask = torch.ones_like(whole, dtype=torch.bool)
    mask[1:n + 1, 1:c + 1] = False
    return bool((whole[mask] == GUARD).all())


@pytest.mark.parametrize("shape", RESIZE_SHAPES)
def test_resize_forward_is_torchs_nearest(dev, shape):
    n, c, h, w, H, W = shape
    x = _rand((n, c, h, w), 1)
    want = F.interpolate(x.float(), size=(H, W), mode="nearest")
    got = ops.resize_nearest_forward(x.float().to(dev), H, W)
    assert torch.equal(got.cpu(), want)
    whole, view = _guarded((n, c, H, W), dev)
    src_whole, src = _guarded((n, c, h, w), dev)
    src.copy_(x.float())
    assert ops.resize_nearest_forward(src, H, W, out=view) is view
    assert torch.equal(view.cpu(), want) and _guards_intact(whole, (n, c, H, W))


@pytest.mark.parametrize("shape", RESIZE_SHAPES)
def test_resize_backward_sums_the_destination_pixels_in_a_fixed_order(dev, shape):
    n, c, h, w, H, W = shape
    g = _rand((n, c, H, W), 2)
    x = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, size=(H, W), mode="nearest").backward(g)
    count = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(count, size=(H, W), mode="nearest").backward(torch.ones_like(g))
    mag = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(mag, size=(H, W), mode="nearest").backward(g.abs())
    assert float(count.grad.min()) >= 1
    bound = (count.grad - 1) * EPS * mag.grad
    got = ops.resize_nearest_backward(g.float().to(dev), h, w)
    assert bool(((got.double().cpu() - x.grad).abs() <= bound).all())
    again = ops.resize_nearest_backward(g.float().to(dev), h, w)
    assert torch.equal(got, again)
    whole, view = _guarded((n, c, h, w), dev)
    g_whole, g_view = _guarded((n, c, H, W), dev)
    g_view.copy_(g.float())
    assert ops.resize_nearest_backward(g_view, h, w, out=view) is view
    assert torch.equal(view, got) and _guards_intact(whole, (n, c, h, w))
    # as a node
    xd = x.detach().float().to(dev).requires_grad_(True)
    ops.resize_nearest(xd, H, W).backward(g.float().to(dev))
    assert torch.equal(xd.grad, got)


def test_resize_refuses_a_smaller_map(dev):
    x = torch.zeros(1, 1, 4, 4, device=dev)
    with pytest.raises(KbnError):
        ops.resize_nearest_forward(x, 3, 4)
    with pytest.raises(KbnError):
        ops.resize_nearest_backward(x, 5, 4)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (2, 23, 39), (2, 8, 12)])
@pytest.mark.parametrize("slope", [0.2, 0.0, None])
def test_kb_xyz_backward(dev, shape, slope):
    n, h, w = shape
    z = _rand((n, 1, h, w), 3)
    z = (torch.where(z < 0, -torch.ones_like(z), torch.ones_like(z)) * (z.abs() + 0.05)).float().double()      # away from the kink
    assert float(z.abs().min()) >= 1e-3 * po.rms(z)          # no element at the kink: exact zeros are tested apart
    coords = _rand((n, 3, h, w), 4)
    wide = _rand((n, 7, h, w), 5)                             # g_xyz is a channel slice of a wider buffer
    g = wide[:, 2:5]
    dz = torch.ones_like(z) if slope is None else torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    terms = coords * g
    want = dz * terms.sum(dim=1, keepdim=True)
    bound = 8 * EPS * (dz.abs() * terms.abs().sum(dim=1, keepdim=True))
    wide_d = wide.float().to(dev)
    got = ops.kb_xyz_backward(z.float().to(dev), coords.float().to(dev), wide_d[:, 2:5], slope)
    assert bool(((got.double().cpu() - want).abs() <= bound).all())
    assert torch.equal(got, ops.kb_xyz_backward(z.float().to(dev), coords.float().to(dev), wide_d[:, 2:5], slope))
    whole, view = _guarded((n, 1, h, w), dev)
    assert ops.kb_xyz_backward(z.float().to(dev), coords.float().to(dev), wide_d[:, 2:5], slope, out=view) is view
    assert torch.equal(view, got) and _guards_intact(whole, (n, 1, h, w))


@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_kb_xyz_backward_takes_the_slope_at_exact_zeros(dev, slope):
    z = torch.tensor([0.0, -0.0, 1.0, -1.0], device=dev).view(1, 1, 2, 2)
    coords = torch.ones(1, 3, 2, 2, device=dev)
    g = torch.ones(1, 3, 2, 2, device=dev)
    got = ops.kb_xyz_backward(z, coords, g, slope).flatten().tolist()
    assert got == pytest.approx([3 * slope, 3 * slope, 3.0, 3 * slope], rel=1e-6)      # z <= 0 takes the slope, as leaky_relu at 0


def test_kb_xyz_node_against_autograd(dev):
    """ops.kb_xyz: the 1 x 1 conv, the activation and the product as one node, against fp64 autograd of the same expression."""
    n, cd, h, w = 2, 5, 9, 13
    depth, weight, coords, g = _rand((n, cd, h, w), 6), _rand((1, cd, 1, 1), 7, 0.5), _rand((n, 3, h, w), 8), _rand((n, 3, h, w), 9)
    d64, w64 = depth.clone().requires_grad_(True), weight.clone().requires_grad_(True)
    u = F.conv2d(d64, w64)
    xyz = coords * torch.where(u > 0, u, 0.2 * u)
    xyz.backward(g)
    dd, wd = depth.float().to(dev).requires_grad_(True), weight.float().to(dev).requires_grad_(True)
    got, z = ops.kb_xyz(dd, wd, coords.float().to(dev), 0.2)
    assert not z.requires_grad and pgo.fraction(got, xyz) <= 1e-5
    got.backward(g.float().to(dev))
    assert pgo.fraction(dd.grad, d64.grad) <= pgo.TOL and pgo.fraction(wd.grad, w64.grad) <= pgo.TOL


@pytest.mark.parametrize("cfg", [kb.kitti_config(), kb.void_config()], ids=["kitti", "void"])
def test_depth_map_backward(dev, cfg):
    logits, g = cases.depth_map_inputs()
    dmin, dmax = cfg.min_predict_depth, cfg.max_predict_depth
    l64 = logits.clone().requires_grad_(True)
    depth = dmin / (torch.sigmoid(l64) + dmin / dmax)
    depth.backward(g)
    ld = logits.float().to(dev).requires_grad_(True)
    got = ops.depth_map(ld, dmin, dmax)
    assert float(((got.detach().double().cpu() - depth.detach()).abs() / depth.detach().abs()).max()) < 1e-5
    got.backward(g.float().to(dev))
    f = pgo.fraction(ld.grad, l64.grad)
    print(f"depth_map_backward [{dmin}, {dmax}]: {f:.2e} of |b| + rms(b) (gate {kgo.DEPTH_MAP_TOL:.0e})")
    assert f <= kgo.DEPTH_MAP_TOL
    assert torch.isfinite(ld.grad).all()
    whole = torch.full((logits.numel() + 8,), GUARD, device=dev)
    view = whole[4:-4].view(logits.shape)
    d32 = got.detach()
    assert ops.depth_map_backward(ld.detach(), d32, g.float().to(dev), dmin, out=view) is view
    assert torch.equal(view, ld.grad) and bool((whole[:4] == GUARD).all()) and bool((whole[-4:] == GUARD).all())


CONV_CHANNELS = [(3, 5, 7), (70, 3, 19)]
CONV_FRAMES = [(2, 9, 13), (3, 17, 23)]


def _conv_case(channels, frame, k, stride, oc, seed):
    n, h, w = frame
    xs = [_rand((n, c, h, w), seed + i) for i, c in enumerate(channels)]
    cin = sum(channels)
    weight = _rand((oc, cin, k, k), seed + 10, 1.0 / (cin * k * k) ** 0.5)
    oh, ow = -(-h // stride), -(-w // stride)
    return xs, weight, _rand((n, oc, oh, ow), seed + 11)


def _reference(xs, weight, g, stride, slope, need, mask=None):
    """fp64 autograd of act(conv(cat(xs))) on the branches `mask` (None: the signs of the fp64 pre-activation u) ->
    (y, u, grad_weight, [grad_x or None])."""
    leaves = [x.clone().requires_grad_(flag) for x, flag in zip(xs, need)]
    w64 = weight.clone().requires_grad_(True)
    u = F.conv2d(torch.cat(leaves, dim=1), w64, None, stride=stride, padding=weight.shape[-1] // 2)
    y = u if slope is None else torch.where(u > 0 if mask is None else mask, u, slope * u)
    y.backward(g)
    return y.detach(), u.detach(), w64.grad, [x.grad for x in leaves]


@pytest.mark.parametrize("ks", [(3, 1), (3, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("channels", CONV_CHANNELS)
@pytest.mark.parametrize("frame", CONV_FRAMES)
def test_conv_node_with_one_two_and_three_inputs(dev, ks, channels, frame):
    k, stride = ks
    oc = 70 if channels[0] < 8 else 10
    for count, need, slope in ((1, (True,), 0.2), (2, (False, True), 0.0), (2, (True, False), None), (3, (True, True, True), 0.2),
                               (3, (True, False, True), 0.2), (3, (False, True, False), 0.0)):
        xs, weight, g = _conv_case(channels[:count], frame, k, stride, oc, 100 * k + 10 * stride + count)
        ins = [x.float().to(dev).requires_grad_(flag) for x, flag in zip(xs, need)]
        wd = weight.float().to(dev).requires_grad_(True)
        got = ops.conv2d_kbnet(ins, wd, stride, slope)
        # the fp64 yardstick on the branches the device took, once kink_check has shown that any that differ sit AT the kink
        mask = (got.detach() > 0).cpu()
        y, u, gw, gxs = _reference(xs, weight, g, stride, slope, need, mask)
        if slope is not None:
            pgo.kink_check([mask], [u])
        assert pgo.fraction(got, y) <= 1e-5
        got.backward(g.float().to(dev))
        label = f"conv node k {k} stride {stride} inputs {channels[:count]} need {need} slope {slope}"
        f = pgo.fraction(wd.grad, gw)
        assert f <= pgo.TOL, (label, "weight", f)
        for x, flag, want in zip(ins, need, gxs):
            if flag:
                f = pgo.fraction(x.grad, want)
                assert f <= pgo.TOL, (label, "data", f)
            else:
                assert x.grad is None, label


@pytest.mark.parametrize("ks", [(3, 1), (3, 2), (1, 1), (1, 2)])
def test_three_input_weight_gradient_is_the_single_input_one_on_the_concat(dev, ks):
    """The weight gradient is linear in the input-channel blocks and the sum over the output pixels is split by `splits` alone: with
    one split plan the two calls of a three-input conv, joined along dim 1, ARE the single call on the materialised concat, bit for
    bit.  With the plan each call picks for itself the node's result is those two calls' and agrees with the concat's within the
    gate; two runs give equal bits."""
    k, stride = ks
    xs, weight, g = _conv_case((3, 5, 7), (2, 9, 13), k, stride, 19, 7)
    ins = [x.float().to(dev) for x in xs]
    gd = g.float().to(dev)
    cat = torch.cat(ins, dim=1)
    fn = (lambda t, s=None: ops.conv2d_s2_backward_weight(t, gd, k, splits=s)) if ks == (3, 2) else \
        (lambda t, s=None: ops.conv2d_backward_weight(t, gd, k, stride, splits=s))
    for splits in (1, 3):
        joined = torch.cat([fn(ins[:2], splits), fn(ins[2:], splits)], dim=1)
        assert torch.equal(joined, fn([cat], splits)), splits
    wd = weight.float().to(dev).requires_grad_(True)
    ops.conv2d_kbnet(ins, wd, stride, None).backward(gd)
    first = wd.grad.clone()
    wd.grad = None
    ops.conv2d_kbnet(ins, wd, stride, None).backward(gd)
    assert torch.equal(first, wd.grad)                       # two runs, equal bits
    assert torch.equal(first, torch.cat([fn(ins[:2]), fn(ins[2:])], dim=1))
    assert pgo.fraction(first, fn([cat]).double()) <= pgo.TOL


def test_conv_node_refusals(dev):
    x = torch.zeros(1, 3, 4, 4, device=dev)
    with pytest.raises(KbnError, match="one to three"):
        ops.conv2d_kbnet([x] * 4, torch.zeros(2, 12, 3, 3, device=dev), 1)
    with pytest.raises(KbnError, match="kernel size"):
        ops.conv2d_kbnet([x], torch.zeros(2, 3, 5, 5, device=dev), 1)
    with pytest.raises(KbnError, match="channels"):
        ops.conv2d_kbnet([x], torch.zeros(2, 4, 3, 3, device=dev), 1)
    with pytest.raises(KbnError, match="negative_slope"):
        ops.conv2d_kbnet([x], torch.zeros(2, 3, 3, 3, device=dev), 1, -0.1)
