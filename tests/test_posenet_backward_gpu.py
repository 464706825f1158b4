"""GPU: the operators of csrc/posenet_backward.hip, each against torch.nn.functional under autograd in fp64 on the CPU.

Gate: |a - b| <= TOL |b| + TOL rms(b) per tensor (posenet_grad_oracle.TOL; tests/test_posenet_grad_oracle_cpu.py measures it,
tests/test_posenet_grad_power_cpu.py proves what it rejects).  Forward values: the 1e-4 rule of tests/test_posenet_gpu.py.
Every backward operator runs twice and must repeat its bits: no sum in it depends on the order workgroups finish in.

    python -m pytest tests -m gpu -q
"""
import pytest
import torch

import kbnet_amd as kb
KbnError = kb._lib.KbnError

import posenet_grad_cases as cases
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
    """`t` (fp64 CPU) as an fp32 channel slice of a larger device tensor full of sentinels -> (slice, whole tensor)."""
    n, c, h, w = t.shape
    whole = torch.full((n, c + 2 * extra, h, w), SENTINEL, device=dev)
    whole[:, extra:extra + c] = t.float().to(dev)
    return whole[:, extra:extra + c], whole


def _outside_untouched(whole, c, extra=3):
    return bool((whole[:, :extra] == SENTINEL).all()) and bool((whole[:, extra + c:] == SENTINEL).all())


CONV_CASES = [s + (k,) for s in cases.CONV_SHAPES for k in (3, 5, 7)]


@pytest.mark.parametrize("shape", CONV_CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv_gradients(dev, shape):
    xs, weight, grad_out, grad_xs, grad_w = cases.conv_case(*shape)
    n, cins, h, w, oc, k = shape
    g = grad_out.float().to(dev)
    dxs = [x.float().to(dev) for x in xs]
    packed_t = ops.pack_conv2d_s2_backward_data_weight(weight.float().to(dev))
    got = ops.conv2d_s2_backward_data(g, packed_t, cins, k, h, w)
    again = ops.conv2d_s2_backward_data(g, packed_t, cins, k, h, w)
    for i, (a, b, want) in enumerate(zip(got, again, grad_xs)):
        assert tuple(a.shape) == tuple(want.shape)
        _close(f"data gradient {shape} input {i}", a, want)
        assert torch.equal(a, b), "the data gradient must repeat its bits"
    for splits in (None, 1, 3):
        gw = ops.conv2d_s2_backward_weight(dxs, g, k, splits=splits)
        assert tuple(gw.shape) == (oc, sum(cins), k, k)
        _close(f"weight gradient {shape} splits {splits}", gw, grad_w)
        assert torch.equal(gw, ops.conv2d_s2_backward_weight(dxs, g, k, splits=splits)), "the weight gradient must repeat its bits"


@pytest.mark.parametrize("shape", cases.WGRAD_SPLIT_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_weight_gradient_split_paths(dev, shape):
    """A long K over a small M x N (the split chosen from the shape crosses many workgroups) and a short K (less than one chunk)
    under a wide M x N: with the split the wrapper chooses, without one, and with more splits asked than there are chunks."""
    xs, weight, grad_out, _, grad_w = cases.conv_case(*shape)
    n, cins, h, w, oc, k = shape
    g = grad_out.float().to(dev)
    dxs = [x.float().to(dev) for x in xs]
    lib = kb._lib.load()
    auto = lib.kbn_conv2d_s2_backward_weight_scratch_bytes(n, oc, sum(cins), k, h, w, 0) // (4 * oc * sum(cins) * k * k)
    print(f"{shape}: the wrapper's own split is {max(auto, 1)}")
    assert (auto > 8) == (n * ((h + 1) // 2) * ((w + 1) // 2) > 1000)
    for splits in (None, 1, 2, 7, 1 << 20):
        gw = ops.conv2d_s2_backward_weight(dxs, g, k, splits=splits)
        _close(f"weight gradient {shape} splits {splits}", gw, grad_w)
        assert torch.equal(gw, ops.conv2d_s2_backward_weight(dxs, g, k, splits=splits))


@pytest.mark.parametrize("k", [3, 5, 7])
def test_conv_gradients_on_channel_slices(dev, k):
    """Inputs, grad_out and the data gradient's outputs as channel slices of larger tensors: nothing outside the slices is written."""
    shape = cases.CONV_SHAPES[4] + (k,)
    xs, weight, grad_out, grad_xs, grad_w = cases.conv_case(*shape)
    n, cins, h, w, oc, _ = shape
    g, _ = _embedded(grad_out, dev)
    dxs = [_embedded(x, dev)[0] for x in xs]
    outs = [_embedded(torch.zeros_like(x), dev) for x in xs]
    packed_t = ops.pack_conv2d_s2_backward_data_weight(weight.float().to(dev))
    got = ops.conv2d_s2_backward_data(g, packed_t, cins, k, h, w, out=[o[0] for o in outs])
    for i, (a, want) in enumerate(zip(got, grad_xs)):
        assert a.data_ptr() == outs[i][0].data_ptr()
        _close(f"data gradient into a slice, k {k} input {i}", a, want)
        assert _outside_untouched(outs[i][1], cins[i])
    _close(f"weight gradient from slices, k {k}", ops.conv2d_s2_backward_weight(dxs, g, k), grad_w)


def test_batch_norm_stats_cancellation(dev):
    """Mean 100, standard deviation 1e-2: E[x^2] - mean^2 in fp32 loses every digit of the variance (1e4 x 6e-8 = 6e-4 against
    1e-4).  Two fp64 passes leave the rounding of the result: 1e-6 of the variance is ten fp32 roundings."""
    g = torch.Generator().manual_seed(3)
    x = (100.0 + 1e-2 * torch.randn(4, 6, 33, 35, generator=g, dtype=torch.float64)).float()
    whole = torch.full((4, 10, 33, 35), SENTINEL, device=dev)
    whole[:, 2:8] = x.to(dev)
    for view in (x.to(dev), whole[:, 2:8]):
        mean, var = ops.batch_norm_stats(view)
        m64, v64 = x.double().mean(dim=(0, 2, 3)), x.double().var(dim=(0, 2, 3), unbiased=False)
        em = float(((mean.double().cpu() - m64).abs() / m64).max())
        ev = float(((var.double().cpu() - v64).abs() / v64).max())
        print(f"batch_norm_stats: mean {em:.2e}, variance {ev:.2e} relative")
        assert em <= 1e-7 and ev <= 1e-6
        again = ops.batch_norm_stats(view)
        assert torch.equal(mean, again[0]) and torch.equal(var, again[1])


@pytest.mark.parametrize("batch", [False, True], ids=["running", "batch"])
@pytest.mark.parametrize("slope", [None, 0.0, 0.2])
def test_batch_norm_act_forward_and_backward(dev, slope, batch):
    c = cases.bn_case(slope, batch)
    if slope is not None:
        assert float(c["z"].abs().min()) > 1e-3 * po.rms(c["z"])      # no element near the kink, none left out
    d = {k: v.float().to(dev) for k, v in c.items()}
    if batch:
        mean, var = ops.batch_norm_stats(d["u"])
        u64 = c["u"]
        for a, b in ((mean, u64.mean(dim=(0, 2, 3))), (var, u64.var(dim=(0, 2, 3), unbiased=False))):
            assert po.gate_fraction(a, b, 1e-4 * po.rms(b)) <= 1.0
    else:
        mean, var = d["mean"], d["var"]
    y = ops.batch_norm_act(d["u"], d["gamma"], d["beta"], mean, var, pgo.EPS, slope, batch)
    assert y.grad_fn is None
    assert po.gate_fraction(y, c["y"], po.layer_floor(c["y"])) <= 1.0
    got = ops.batch_norm_act_backward(d["u"], d["grad_y"], d["gamma"], d["beta"], mean, var, pgo.EPS, slope, batch)
    again = ops.batch_norm_act_backward(d["u"], d["grad_y"], d["gamma"], d["beta"], mean, var, pgo.EPS, slope, batch)
    for name, a, b in zip(("grad_u", "grad_gamma", "grad_beta"), got, again):
        _close(f"batch_norm_act_backward slope {slope} batch {batch} {name}", a, c[name])
        assert torch.equal(a, b), "batch_norm_act_backward must repeat its bits"
    # the same through the autograd node
    leaves = [d[k].clone().requires_grad_(True) for k in ("u", "gamma", "beta")]
    out = ops.batch_norm_act(leaves[0], leaves[1], leaves[2], mean, var, pgo.EPS, slope, batch)
    assert out.grad_fn is not None and torch.equal(out, y)
    out.backward(d["grad_y"])
    for leaf, a in zip(leaves, got):
        assert torch.equal(leaf.grad, a)


@pytest.mark.parametrize("slope", [0.0, 0.2])
def test_slope_branch_at_exactly_zero(dev, slope):
    c = cases.bn_case(slope, False, zeros=True)
    assert int((c["z"] == 0).sum()) >= 3 * 5 * 12
    d = {k: v.float().to(dev) for k, v in c.items()}
    y = ops.batch_norm_act(d["u"], d["gamma"], d["beta"], d["mean"], d["var"], pgo.EPS, slope, False)
    assert bool(((y == 0).cpu() == (c["y"] == 0)).all())
    got = ops.batch_norm_act_backward(d["u"], d["grad_y"], d["gamma"], d["beta"], d["mean"], d["var"], pgo.EPS, slope, False)
    _close(f"grad_u with exact zeros, slope {slope}", got[0], c["grad_u"])


def test_conv_then_batch_norm_through_autograd(dev):
    """conv2d_s2 and batch_norm_act recorded together, the input asking for its gradient too (a data gradient THROUGH an
    activation), against torch's autograd in fp64.  The seed is the first whose pre-activations all keep 1e-3 rms(z) from 0."""
    n, cins, h, w, oc = cases.CONV_SHAPES[2]
    for seed in range(1, 200):
        xs, weight, grad_out, _, _ = cases.conv_case(n, cins, h, w, oc, 3, seed=seed)
        bn = cases.bn_case(0.2, True, n=1, c=oc, h=1, w=1, seed=seed)
        x = xs[0].clone().requires_grad_(True)
        wt, gamma, beta = (t.clone().requires_grad_(True) for t in (weight, bn["gamma"], bn["beta"]))
        u = torch.nn.functional.conv2d(x, wt, None, stride=2, padding=1)
        y, _, _, z = pgo.batch_norm_act(u, gamma, beta, None, None, slope=0.2, batch=True)
        z = z.detach()
        if float(z.abs().min()) > 1e-3 * po.rms(z):
            break
    assert float(z.abs().min()) > 1e-3 * po.rms(z)
    want = torch.autograd.grad(y, [x, wt, gamma, beta], grad_out)
    dx, dw, dg, db = (t.detach().float().to(dev).requires_grad_(True) for t in (x, wt, gamma, beta))
    du = ops.conv2d_s2([dx], dw)
    assert du.grad_fn is not None
    mean, var = ops.batch_norm_stats(du.detach())
    out = ops.batch_norm_act(du, dg, db, mean, var, pgo.EPS, 0.2, True)
    assert po.gate_fraction(out, y, po.layer_floor(y.detach())) <= 1.0
    out.backward(grad_out.float().to(dev))
    for name, leaf, b in zip(("input", "weight", "gamma", "beta"), (dx, dw, dg, db), want):
        _close(f"conv + batch norm through autograd: {name}", leaf.grad, b)


def test_no_data_gradient_launch_when_no_input_asks(dev):
    xs, weight, grad_out, _, grad_w = cases.conv_case(*cases.CONV_SHAPES[2], 5)
    dw = weight.float().to(dev).requires_grad_(True)
    ops.PROFILE = []
    try:
        u = ops.conv2d_s2([xs[0].float().to(dev)], dw)
        u.backward(grad_out.float().to(dev))
        names = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert [n.split("<")[0] for n in names] == ["conv_s2_affine", "conv_s2_bwd_weight"], names
    _close("weight gradient through autograd", dw.grad, grad_w)


def test_refusals_raise_without_launching(dev):
    xs, weight, grad_out, _, _ = cases.conv_case(*cases.CONV_SHAPES[2], 3)
    n, cins, h, w, oc = cases.CONV_SHAPES[2]
    x, g, wt = xs[0].float().to(dev), grad_out.float().to(dev), weight.float().to(dev)
    packed_t = ops.pack_conv2d_s2_backward_data_weight(wt)
    vec = torch.ones(oc, device=dev)
    u = torch.zeros(n, oc, 5, 7, device=dev)
    ops.PROFILE = []
    try:
        bad = [
            lambda: ops.conv2d_s2_backward_data(g, packed_t, cins, 4, h, w),
            lambda: ops.conv2d_s2_backward_data(g, packed_t, cins, 3, h + 2, w),
            lambda: ops.conv2d_s2_backward_data(g, packed_t[:-16], cins, 3, h, w),
            lambda: ops.conv2d_s2_backward_data(g.cpu(), packed_t, cins, 3, h, w),
            lambda: ops.conv2d_s2_backward_data(g, packed_t, (2, 2, 1), 3, h, w),
            lambda: ops.conv2d_s2_backward_data(g, packed_t, cins, 3, h, w, out=[torch.zeros(n, 5, h, w + 1, device=dev)]),
            lambda: ops.conv2d_s2_backward_weight([x], g, 6),
            lambda: ops.conv2d_s2_backward_weight([x], g[:, :, :-1], 3),
            lambda: ops.conv2d_s2_backward_weight([x], g, 3, splits=0),
            lambda: ops.conv2d_s2_backward_weight([x.double()], g, 3),
            lambda: ops.conv2d_s2_backward_weight([x, x, x], g, 3),
            lambda: ops.pack_conv2d_s2_backward_data_weight(torch.zeros(4, 4, 2, 2, device=dev)),
            lambda: ops.batch_norm_stats(x.cpu()),
            lambda: ops.batch_norm_stats(x[:, :, ::2]),
            lambda: ops.batch_norm_act(u, vec[:-1], vec, vec, vec),
            lambda: ops.batch_norm_act(u, vec, vec, vec.clone().requires_grad_(True), vec),
            lambda: ops.batch_norm_act_backward(u, u[:, :-1], vec, vec, vec, vec),
            lambda: ops.conv2d_s2([x], wt[:, :-1]),
        ]
        for i, fn in enumerate(bad):
            with pytest.raises(KbnError):
                fn()
            assert ops.PROFILE == [], i
    finally:
        ops.PROFILE = None
