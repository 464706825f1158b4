"""GPU: the conv and BatchNorm gradients at a training-size pixel count.  Every case of tests/grad_extent_cases.py sums over 71 806
output pixels (2 frames of 161 x 223): the weight gradient's split plan at its 512-workgroup cap (449 splits of 5 chunks), at its
1024-split clamp (748 splits of 3 chunks), with a ragged last split, a ragged last chunk and a chunk across the frame boundary; the
one-workgroup-per-channel BatchNorm reductions over 71 806 values each.  tests/test_grad_extents_cpu.py reads the split counts from
the library, holds torch's own fp32 under a third of the gate and proves what the gate rejects at this extent.

References: torch autograd in fp64 on the CPU from inputs exactly representable in fp32.  Gates: the operator gate of
tests/test_posenet_backward_gpu.py (|a - b| <= 2e-4 |b| + 2e-4 rms(b) per tensor), and for BatchNorm's statistics and forward the
ones of test_batch_norm_stats_cancellation and test_batch_norm_act_forward_and_backward.  Every gradient runs twice and must repeat
its bits.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch

import kbnet_amd as kb

import grad_extent_cases as ext
import posenet_grad_oracle as pgo
import posenet_oracle as po

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
    f = pgo.fraction(got, want)
    print(f"{label}: {f:.2e} of |b| + rms(b) (gate {pgo.TOL:.0e})")
    assert f <= pgo.TOL, (label, f)


def _embedded(t, dev, extra=3):
    """`t` (fp64 CPU) as an fp32 channel slice of a larger device tensor full of sentinels: its batch stride exceeds C H W."""
    n, c, h, w = t.shape
    whole = torch.full((n, c + 2 * extra, h, w), SENTINEL, device=dev)
    whole[:, extra:extra + c] = t.float().to(dev)
    return whole[:, extra:extra + c]


def _s2(c):
    return (c["k"], c["stride"]) in ext.S2_ENTRY


@pytest.mark.parametrize("name", [c["name"] for c in ext.WGRAD])
def test_weight_gradient(dev, name):
    c = ext.by_name(name)
    xs, _, grad_out = ext.conv_inputs(c)
    want = ext.weight_gradient(name)
    put = (lambda t: _embedded(t, dev)) if c["sliced"] else (lambda t: t.float().to(dev))
    g, dxs = put(grad_out), [put(x) for x in xs]
    if c["sliced"]:
        assert g.stride(0) > g.shape[1] * ext.OH * ext.OW and all(x.stride(0) > x.shape[1] * x.shape[2] * x.shape[3] for x in dxs)
    run = (lambda s: ops.conv2d_s2_backward_weight(dxs, g, c["k"], splits=s)) if _s2(c) else \
        (lambda s: ops.conv2d_backward_weight(dxs, g, c["k"], c["stride"], splits=s))
    for splits in ext.SPLITS:
        gw = run(splits)
        assert tuple(gw.shape) == tuple(want.shape)
        _close(f"weight gradient {name} splits {splits}", gw, want)
        assert torch.equal(gw, run(splits)), "the weight gradient must repeat its bits"


@pytest.mark.parametrize("name", [c["name"] for c in ext.DGRAD])
def test_data_gradient(dev, name):
    c = ext.by_name(name)
    _, weight, grad_out = ext.conv_inputs(c)
    want = ext.data_gradient(name)
    (cin,), k, stride, (h, w) = c["cins"], c["k"], c["stride"], c["size"]
    g, wd = grad_out.float().to(dev), weight.float().to(dev)
    if _s2(c):
        blob = ops.pack_conv2d_s2_backward_data_weight(wd)
        run = lambda: ops.conv2d_s2_backward_data(g, blob, [cin], k, h, w)[0]
    else:
        blob = ops.pack_conv2d_backward_data_weight(wd, stride)
        run = lambda: ops.conv2d_backward_data(g, blob, cin, k, stride, h, w)
    got = run()
    assert tuple(got.shape) == tuple(want.shape)
    _close(f"data gradient {name}", got, want)
    assert torch.equal(got, run()), "the data gradient must repeat its bits"


def _relative(a, b):
    return float(((a.double().cpu() - b).abs() / b.abs()).max())


@pytest.mark.parametrize("batch", [False, True], ids=["running", "batch"])
def test_batch_norm_stats(dev, batch):
    """71 806 values per channel whose mean lies 4 to 64 spreads from 0, dense and as a channel slice: the bars of the cancellation
    test (the mean to 1e-7, the variance to 1e-6, relative) and of the forward-and-backward test (1e-4 of the vector's rms)."""
    u = ext.bn_inputs(batch)["u"]
    m64, v64 = u.mean(dim=(0, 2, 3)), u.var(dim=(0, 2, 3), unbiased=False)
    for label, view in (("dense", u.float().to(dev)), ("slice", _embedded(u, dev))):
        mean, var = ops.batch_norm_stats(view)
        em, ev = _relative(mean, m64), _relative(var, v64)
        print(f"batch_norm_stats ({label}): mean {em:.2e}, variance {ev:.2e} relative")
        assert em <= 1e-7 and ev <= 1e-6
        for a, b in ((mean, m64), (var, v64)):
            assert po.gate_fraction(a, b, 1e-4 * po.rms(b)) <= 1.0
        again = ops.batch_norm_stats(view)
        assert torch.equal(mean, again[0]) and torch.equal(var, again[1])


@pytest.mark.parametrize("batch", [False, True], ids=["running", "batch"])
@pytest.mark.parametrize("slope", [None, 0.2])
def test_batch_norm_act_forward_and_backward(dev, slope, batch):
    c = ext.bn_inputs(batch)
    d = {k: v.float().to(dev) for k, v in c.items()}
    mean, var = ops.batch_norm_stats(d["u"]) if batch else (d["mean"], d["var"])
    y = ops.batch_norm_act(d["u"], d["gamma"], d["beta"], mean, var, ext.BN_EPS, slope, batch)
    mask = None
    if slope is not None:
        # the branches the device took.  No fp64 pre-activation lies closer to 0 than fp32 resolves (bn_kink_margin > 1, asserted on
        # the CPU), so they are the fp64 branches, every one
        mask = (y > 0).cpu()
        z64 = ext.bn_pre_activation(c, batch)[0]
        assert torch.equal(mask, z64 > 0), int((mask != (z64 > 0)).sum())
    want = ext.bn_gradients(c, slope, batch, mask=mask)
    f = po.gate_fraction(y, want["y"], po.layer_floor(want["y"]))
    print(f"batch_norm_act slope {slope} batch {batch}: forward at {f:.2e} of its gate")
    assert f <= 1.0
    args = (d["u"], d["grad_y"], d["gamma"], d["beta"], mean, var, ext.BN_EPS, slope, batch)
    got, again = ops.batch_norm_act_backward(*args), ops.batch_norm_act_backward(*args)
    for key, a, b in zip(("grad_u", "grad_gamma", "grad_beta"), got, again):
        _close(f"batch_norm_act_backward slope {slope} batch {batch} {key}", a, want[key])
        assert torch.equal(a, b), "batch_norm_act_backward must repeat its bits"


def test_one_recorded_conv_through_autograd(dev):
    """ops.conv2d_kbnet with three inputs and the activation in its epilogue: the weight gradient (two calls, 250 and 449 splits,
    joined) and the three data gradients (one launch, sliced) against fp64 autograd on the branches the device took."""
    c = ext.NODE
    xs, weight, grad_out = ext.conv_inputs(c)
    ins = [x.float().to(dev).requires_grad_(True) for x in xs]
    wd = weight.float().to(dev).requires_grad_(True)
    got = ops.conv2d_kbnet(ins, wd, c["stride"], c["slope"])
    mask = (got.detach() > 0).cpu()
    gw, gxs, u = ext.conv_gradients(c, data_grad=True, mask=mask)
    flipped = pgo.kink_check([mask], [u])      # any branch that differs from fp64's sits AT the kink, and there are a handful at most
    print(f"recorded conv: {flipped} branches on the other side of the kink")
    y = torch.where(mask, u, c["slope"] * u)
    assert pgo.fraction(got, y) <= 1e-5
    g = grad_out.float().to(dev)
    got.backward(g)
    first = [wd.grad.clone()] + [x.grad.clone() for x in ins]
    _close("recorded conv: weight gradient", wd.grad, gw)
    for i, (x, want) in enumerate(zip(ins, gxs)):
        _close(f"recorded conv: data gradient of input {i}", x.grad, want)
    for t in [wd] + ins:
        t.grad = None
    ops.conv2d_kbnet(ins, wd, c["stride"], c["slope"]).backward(g)
    for a, t in zip(first, [wd] + ins):
        assert torch.equal(a, t.grad), "the recorded conv's gradients must repeat their bits"
