"""GPU: the operators of csrc/conv_affine_backward.hip, each against torch under autograd in fp64 on the CPU.

Gate of the conv gradients: |a - b| <= TOL |b| + TOL rms(b) per tensor with the operator gate of tests/test_posenet_backward_gpu.py
(posenet_grad_oracle.TOL).  The pool's gradient: per element 4 x 2^-24 x the sum of |g| over the windows routed to it (at most four
fp32 terms are added).  add_act: bit for bit.  Every `out` buffer is pre-filled with NaN: an element the launch leaves out shows.
Every backward operator runs twice and must repeat its bits.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch
import torch.nn.functional as F

import kbnet_amd as kb
KbnError = kb._lib.KbnError

import posenet_grad_cases as pcases
import posenet_grad_oracle as pgo
import resnet_pose_grad_cases as cases

pytestmark = pytest.mark.gpu
ops = kb.ops
SENTINEL = -7.25e30


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _close(label, got, want):
    assert tuple(got.shape) == tuple(want.shape), (label, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{label}: an element was not written"
    f = pgo.fraction(got, want)
    print(f"{label}: {f:.2e} of |b| + rms(b) (gate {pgo.TOL:.0e})")
    assert f <= pgo.TOL, (label, f)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


CONV_CASES = [s + ks for s in cases.CONV_SHAPES for ks in cases.CONV_KS]


@pytest.mark.parametrize("shape", CONV_CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv_gradients(dev, shape):
    n, cin, h, w, oc, k, stride = shape
    x, weight, grad_out, grad_x, grad_w = cases.conv_case(*shape)
    g, dx, dw = grad_out.float().to(dev), x.float().to(dev), weight.float().to(dev)
    packed_t = ops.pack_conv2d_backward_data_weight(dw, stride)
    got = ops.conv2d_backward_data(g, packed_t, cin, k, stride, h, w, out=_nan((n, cin, h, w), dev))
    _close(f"data gradient {shape}", got, grad_x)
    if stride == 2:     # the pixels the conv never read: exact zeros, written by the launch
        assert float(got[:, :, 1::2].abs().sum()) == 0.0 and float(got[:, :, :, 1::2].abs().sum()) == 0.0
    assert torch.equal(got, ops.conv2d_backward_data(g, packed_t, cin, k, stride, h, w)), "the data gradient must repeat its bits"
    for splits in (None, 1, 3):
        gw = ops.conv2d_backward_weight([dx], g, k, stride, splits=splits, out=_nan((oc, cin, k, k), dev))
        _close(f"weight gradient {shape} splits {splits}", gw, grad_w)
        assert torch.equal(gw, ops.conv2d_backward_weight([dx], g, k, stride, splits=splits)), "the weight gradient must repeat its bits"


@pytest.mark.parametrize("shape", cases.WGRAD_SPLIT_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_weight_gradient_split_paths(dev, shape):
    """A long K over a small M x N (the split chosen from the shape crosses many workgroups) and a short K (less than one chunk)
    under a wide M x N: with the split the wrapper chooses, without one, with three, and with more splits than there are chunks."""
    n, cin, h, w, oc = shape
    x, weight, grad_out, _, grad_w = cases.conv_case(n, cin, h, w, oc, 3, 1)
    g, dx = grad_out.float().to(dev), x.float().to(dev)
    lib = kb._lib.load()
    auto = lib.kbn_conv2d_backward_weight_scratch_bytes(n, oc, cin, 3, 1, h, w, 0) // (4 * oc * cin * 9)
    print(f"{shape}: the wrapper's own split is {max(auto, 1)}")
    assert (auto > 8) == (n * h * w > 1000)
    assert lib.kbn_conv2d_backward_weight_scratch_bytes(n, oc, cin, 3, 1, h, w, 1 << 20) == 4 * oc * cin * 9 * (-(-n * h * w // 32)) * (n * h * w > 32)
    for splits in (None, 1, 3, 1 << 20):
        gw = ops.conv2d_backward_weight([dx], g, 3, 1, splits=splits, out=_nan((oc, cin, 3, 3), dev))
        _close(f"weight gradient {shape} splits {splits}", gw, grad_w)
        assert torch.equal(gw, ops.conv2d_backward_weight([dx], g, 3, 1, splits=splits))


@pytest.mark.parametrize("ks", cases.CONV_KS, ids=lambda ks: f"k{ks[0]}s{ks[1]}")
def test_conv_gradients_on_channel_slices(dev, ks):
    """grad_out, the input and the data gradient's output as channel slices of larger tensors: nothing outside the slice is written."""
    k, stride = ks
    n, cin, h, w, oc = cases.CONV_SHAPES[2]
    x, weight, grad_out, grad_x, grad_w = cases.conv_case(n, cin, h, w, oc, k, stride)

    def embedded(t, extra=3):
        whole = torch.full((t.shape[0], t.shape[1] + 2 * extra) + tuple(t.shape[2:]), SENTINEL, device=dev)
        whole[:, extra:extra + t.shape[1]] = t.float().to(dev)
        return whole[:, extra:extra + t.shape[1]], whole

    g, _ = embedded(grad_out)
    dx, _ = embedded(x)
    out, whole = embedded(torch.zeros_like(x))
    got = ops.conv2d_backward_data(g, ops.pack_conv2d_backward_data_weight(weight.float().to(dev), stride), cin, k, stride, h, w, out=out)
    assert got.data_ptr() == out.data_ptr()
    _close(f"data gradient into a slice {ks}", got, grad_x)
    assert bool((whole[:, :3] == SENTINEL).all()) and bool((whole[:, 3 + cin:] == SENTINEL).all())
    _close(f"weight gradient from slices {ks}", ops.conv2d_backward_weight([dx], g, k, stride), grad_w)


@pytest.mark.parametrize("k", [3, 7])
def test_conv2d_pose_at_stride_2_is_the_existing_backward_bit_for_bit(dev, k):
    xs, weight, grad_out, _, _ = pcases.conv_case(*pcases.CONV_SHAPES[3], k)
    n, cins, h, w, oc = pcases.CONV_SHAPES[3]
    g = grad_out.float().to(dev)
    dx = xs[0].float().to(dev).requires_grad_(True)
    dw = weight.float().to(dev).requires_grad_(True)
    u = ops.conv2d_pose([dx], dw, 2)
    assert u.grad_fn is not None
    ones, zeros = torch.ones(oc, device=dev), torch.zeros(oc, device=dev)
    assert torch.equal(u, ops.conv2d_affine([dx.detach()], ops.pack_conv2d_affine_weight(dw.detach()), ones, zeros, oc, k, stride=2,
                                            negative_slope=None))
    u.backward(g)
    assert torch.equal(dw.grad, ops.conv2d_s2_backward_weight([dx.detach()], g, k))
    want = ops.conv2d_s2_backward_data(g, ops.pack_conv2d_s2_backward_data_weight(dw.detach()), cins, k, h, w)[0]
    assert torch.equal(dx.grad, want)


@pytest.mark.parametrize("ks", cases.CONV_KS, ids=lambda ks: f"k{ks[0]}s{ks[1]}")
def test_conv2d_pose_through_autograd(dev, ks):
    """The node's two gradients against fp64 autograd, and no data-gradient launch when the input does not ask."""
    k, stride = ks
    shape = cases.CONV_SHAPES[2] + ks
    x, weight, grad_out, grad_x, grad_w = cases.conv_case(*shape)
    g = grad_out.float().to(dev)
    dx, dw = x.float().to(dev).requires_grad_(True), weight.float().to(dev).requires_grad_(True)
    u = ops.conv2d_pose([dx], dw, stride)
    want = F.conv2d(x, weight, None, stride=stride, padding=k // 2)
    assert pgo.fraction(u, want) <= 1e-5
    u.backward(g)
    _close(f"conv2d_pose {ks}: input", dx.grad, grad_x)
    _close(f"conv2d_pose {ks}: weight", dw.grad, grad_w)
    dw2 = weight.float().to(dev).requires_grad_(True)
    ops.PROFILE = []
    try:
        ops.conv2d_pose([x.float().to(dev)], dw2, stride).backward(g)
        names = [r[0].split("<")[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert names == ["conv_affine", "conv_bwd_weight"], names
    assert torch.equal(dw2.grad, dw.grad)
    with torch.no_grad():
        assert ops.conv2d_pose([dx], dw, stride).grad_fn is None


def _pool_inputs(shape, kind, seed):
    g = torch.Generator().manual_seed(seed + sum(shape))
    if kind == "levels":         # three levels: most windows tie
        x = torch.randint(0, 3, shape, generator=g).float() - 1.0
    else:                        # behind a relu: exact zeros and positive values
        x = torch.randn(shape, generator=g).clamp_min(0.0)
    n, c, h, w = shape
    grad = torch.randn(n, c, (h + 1) // 2, (w + 1) // 2, generator=g)
    return x, grad


@pytest.mark.parametrize("kind", ["levels", "relu"])
@pytest.mark.parametrize("shape", cases.POOL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_maxpool_backward(dev, shape, kind):
    x, grad = _pool_inputs(shape, kind, 3)
    leaf = x.double().requires_grad_(True)
    y = F.max_pool2d(leaf, 3, stride=2, padding=1)
    (want,) = torch.autograd.grad(y, leaf, grad.double(), retain_graph=True)
    (routed,) = torch.autograd.grad(y, leaf, grad.double().abs())
    if kind == "levels" and x.numel() > 9:
        _, idx = F.max_pool2d(x, 3, stride=2, padding=1, return_indices=True)
        assert not torch.equal(idx, F.max_pool2d(x + 1e-3 * torch.rand_like(x), 3, stride=2, padding=1, return_indices=True)[1])   # ties decide
    dx, dg = x.to(dev), grad.to(dev)
    got = ops.maxpool3x3s2_backward(dx, dg, out=_nan(shape, dev))
    assert bool(torch.isfinite(got).all())
    over = (got.double().cpu() - want).abs() - 4.0 * 2.0 ** -24 * routed
    assert float(over.max()) <= 0.0, (shape, kind, float(over.max()))
    assert float(got.abs().sum()) > 0
    assert torch.equal(got, ops.maxpool3x3s2_backward(dx, dg)), "the pool's gradient must repeat its bits"
    # the node: the forward's bits are the no-grad call's, the backward is the operator
    plain = ops.maxpool3x3s2(dx)
    leaf = dx.clone().requires_grad_(True)
    out = ops.maxpool3x3s2(leaf)
    assert out.grad_fn is not None and torch.equal(out, plain) and plain.grad_fn is None
    out.backward(dg)
    assert torch.equal(leaf.grad, got)
    with torch.no_grad():
        assert ops.maxpool3x3s2(leaf).grad_fn is None


@pytest.mark.parametrize("slope", [0.2, 0.0, None])
def test_add_act_forward_and_backward_bit_for_bit(dev, slope):
    g = torch.Generator().manual_seed(9)
    a = torch.randn(2, 5, 9, 13, generator=g)
    b = torch.randn(2, 5, 9, 13, generator=g)
    b[:, :, :3, :4] = -a[:, :, :3, :4]              # a + b exactly 0: the slope branch
    gy = torch.randn(2, 5, 9, 13, generator=g)
    s = a + b
    assert int((s == 0).sum()) >= 2 * 5 * 12
    y = s if slope is None else torch.where(s > 0, s, slope * s)
    want = gy if slope is None else torch.where(y > 0, gy, slope * gy)
    da, db, dgy = a.to(dev), b.to(dev), gy.to(dev)
    got_y = ops.add_act(da, db, slope)
    assert got_y.grad_fn is None and torch.equal(got_y.cpu(), y)
    got = ops.add_act_backward(got_y, dgy, slope)
    assert torch.equal(got.cpu(), want)
    if slope == 0.0:
        assert float(got.cpu()[:, :, :3, :4].abs().sum()) == 0.0     # exact zeros on the slope branch
    la, lb = da.clone().requires_grad_(True), db.clone().requires_grad_(True)
    out = ops.add_act(la, lb, slope)
    assert out.grad_fn is not None and torch.equal(out, got_y)
    out.backward(dgy)
    assert torch.equal(la.grad, got) and torch.equal(lb.grad, got)
    only = da.clone().requires_grad_(True)
    ops.add_act(only, db, slope).backward(dgy)
    assert torch.equal(only.grad, got)


def test_refusals_raise_without_launching(dev):
    n, cin, h, w, oc = cases.CONV_SHAPES[2]
    x, weight, grad_out, _, _ = cases.conv_case(n, cin, h, w, oc, 3, 1)
    dx, g, wt = x.float().to(dev), grad_out.float().to(dev), weight.float().to(dev)
    packed_t = ops.pack_conv2d_backward_data_weight(wt, 1)
    pool_g = torch.zeros(n, cin, 5, 7, device=dev)
    ops.PROFILE = []
    try:
        bad = [
            lambda: ops.conv2d_backward_data(g, packed_t, cin, 3, 2, h, w),               # (3, 2) is conv2d_s2_backward_data's
            lambda: ops.conv2d_backward_data(g, packed_t, cin, 5, 1, h, w),
            lambda: ops.conv2d_backward_data(g, packed_t, cin, 3, 1, h + 1, w),
            lambda: ops.conv2d_backward_data(g, packed_t[:-1], cin, 3, 1, h, w),
            lambda: ops.conv2d_backward_data(g, packed_t, cin + 1, 3, 1, h, w),
            lambda: ops.conv2d_backward_data(g.cpu(), packed_t, cin, 3, 1, h, w),
            lambda: ops.conv2d_backward_data(g, packed_t, cin, 3, 1, h, w, out=torch.zeros(n, cin, h, w + 1, device=dev)),
            lambda: ops.conv2d_backward_weight([dx], g, 3, 2),
            lambda: ops.conv2d_backward_weight([dx], g, 7, 1),
            lambda: ops.conv2d_backward_weight([dx], g[:, :, :-1], 3, 1),
            lambda: ops.conv2d_backward_weight([dx], g, 3, 1, splits=0),
            lambda: ops.conv2d_backward_weight([dx.double()], g, 3, 1),
            lambda: ops.conv2d_backward_weight([dx, dx, dx], g, 3, 1),
            lambda: ops.pack_conv2d_backward_data_weight(wt, 2),
            lambda: ops.pack_conv2d_backward_data_weight(torch.zeros(4, 4, 5, 5, device=dev), 1),
            lambda: ops.conv2d_pose([dx], wt[:, :-1], 1),
            lambda: ops.conv2d_pose([dx], torch.zeros(4, cin, 5, 5, device=dev), 1),
            lambda: ops.conv2d_pose([dx], wt, 3),
            lambda: ops.conv2d_pose([dx.clone().requires_grad_(True), dx], torch.zeros(4, 2 * cin, 3, 3, device=dev), 1),
            lambda: ops.maxpool3x3s2_backward(dx, pool_g[:, :, :-1]),
            lambda: ops.maxpool3x3s2_backward(dx.cpu(), pool_g),
            lambda: ops.maxpool3x3s2(dx.clone().requires_grad_(True), out=pool_g),
            lambda: ops.add_act(dx, dx[:, :-1], 0.2),
            lambda: ops.add_act(dx, dx, -0.1),
            lambda: ops.add_act(dx[:, :, ::2], dx[:, :, ::2], 0.2),
            lambda: ops.add_act_backward(dx, dx.cpu(), 0.2),
        ]
        for i, fn in enumerate(bad):
            with pytest.raises(KbnError):
                fn()
            assert ops.PROFILE == [], i
    finally:
        ops.PROFILE = None
