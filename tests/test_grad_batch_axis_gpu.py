"""GPU: the gradient operators over the frame axis -- what tests/test_batch_axis_gpu.py is for the forward path.

Every gradient kernel flattens the batch into one index, m = (frame * H + y) * W + x: a 128-pixel tile of a data gradient and a
32-pixel K chunk of the weight gradient span frames.  The shapes are the smallest at which that index can still go wrong, at 3 and
5 frames:

  5 x 7     12 output pixels per frame at stride 2 (one 32-pixel chunk holds three frames), 35 at stride 1 (a 128-pixel tile four)
  9 x 13    117 pixels per frame: with three frames the tile boundaries at 128 and 256 fall inside a frame and inside a row
  channels  (5,) -> 19; (12, 9) -> 20: two inputs and a channel tile that is not full; (5,) -> 70: two filter tiles

Properties (inputs exactly representable in fp32; every reference is fp64 torch autograd on the CPU):

  1  a frame alone     frame i of a batched data gradient IS the call on frame i alone (torch.equal): a GEMM row or a thread per pixel
  2  frame order       permuting the frames of every batched argument permutes the result (torch.equal); no frame keeps its place
  3  batch strides     every tensor a channel slice of a wider buffer, no two batch strides equal: the dense call's bits, the guard
                       values around every output intact (the inputs' surroundings are NaN: a read outside a slice would show)
  4  containment       one NaN / +Inf / -Inf in the middle frame's grad_out: the other frames keep the clean run's bits; inside
                       the frame the non-finite elements are exactly the receptive field index arithmetic gives (a load that is
                       multiplied by an exact zero instead of being predicated away would spread it); under a conv an infinity
                       arrives with the sign of the one weight it meets.  The arithmetic mask is cross-checked against fp64 autograd.
  5  containment, weight gradient: a NaN in grad_out stays in its filter's row, a NaN in an input in its channel's columns at the
                       taps that reach the pixel; with splits None, 1 and 3 (the split reduce must not mix rows)
  6  values            the batched results of 1 to 3 meet the operator gates that exist (posenet_grad_oracle.TOL for the convs and
                       the BatchNorm, the per-element bounds of tests/test_kbnet_backward_gpu.py and tests/test_resnet_pose_backward_gpu.py
                       for the rest): every frame wrong in the same way would pass 1 to 5.  No new tolerance.

add_act_backward and depth_map_backward take contiguous tensors only (they refuse a slice), so property 3 has nothing to vary there.

    python -m pytest tests -m gpu -q
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import kbnet_amd as kb

import kbnet_grad_oracle as kgo
import posenet_grad_cases as pcases
import posenet_grad_oracle as pgo
import resnet_pose_grad_oracle as rgo

pytestmark = pytest.mark.gpu
ops = kb.ops
EPS = 2.0 ** -24
GUARD = 12345.0
NAN = float("nan")
FRAMES = [3, 5]
MAPS = [(5, 7), (9, 13)]
# (channels of the inputs, filters, height, width)
CONV_PROBLEMS = [((5,), 19, 5, 7), ((12, 9), 20, 5, 7), ((5,), 19, 9, 13), ((12, 9), 20, 9, 13), ((5,), 70, 5, 7)]
S2_KS = [(3, 2), (5, 2), (7, 2)]                # conv2d_s2_backward_data / conv2d_s2_backward_weight
S1_KS = [(3, 1), (1, 1), (1, 2)]                # conv2d_backward_data / conv2d_backward_weight
CONV_CASES = [p + (n,) + ks for p in CONV_PROBLEMS for n in FRAMES for ks in S2_KS + S1_KS]
# containment: the 9 x 13 map, where an output pixel with every tap of a 7 x 7 kernel inside the image exists
POISON_CASES = [p + (3,) + ks for p in CONV_PROBLEMS[2:4] for ks in S2_KS + S1_KS]
_conv_id = lambda s: "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in s)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a visible MI355X (run with -m gpu on a GPU box)")
    kb._lib.load()   # a missing extension is an error on a GPU box, never a skip
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).float().double()


def _guarded(shape, dev, extra, fill=GUARD):
    """A channel slice of a larger buffer full of `fill`, with a frame of slack before and after -> (the whole buffer, the view)."""
    n, c, h, w = shape
    whole = torch.full((n + 2, c + extra, h, w), fill, device=dev, dtype=torch.float32)
    return whole, whole[1:n + 1, 1:c + 1]


def _guards_intact(whole, shape):
    n, c = shape[:2]
    mask = torch.ones_like(whole, dtype=torch.bool)
    mask[1:n + 1, 1:c + 1] = False
    return bool((whole[mask] == GUARD).all())


class _Strides:
    """Hands out channel slices whose batch strides all differ."""

    def __init__(self, dev):
        self.dev, self.used = dev, set()

    def view(self, shape, fill):
        n, c, h, w = shape
        extra = 2
        while (c + extra) * h * w in self.used:
            extra += 1
        self.used.add((c + extra) * h * w)
        return _guarded(shape, self.dev, extra, fill)

    def holding(self, t):
        _, view = self.view(tuple(t.shape), NAN)
        view.copy_(t)
        assert view.stride(0) != t.stride(0) and not view.is_contiguous()
        return view


# ---------------------------------------------------------------- the data-gradient operators, in one form
class Op:
    """A data-gradient operator over the frame axis.  `args`: name -> fp32 CPU tensor, frames first, every one batched; `call(d, out)`:
    the launch on device tensors `d` (into the list `out`, or into new tensors) -> the list of results, frames first; `check(got)`:
    property 6; `sliced`: the arguments that may be channel slices; `out_shapes`: of the results that take `out` (None: no `out`)."""

    def __init__(self, label, args, call, check, sliced, out_shapes):
        self.label, self.args, self.call, self.check, self.sliced, self.out_shapes = label, args, call, check, sliced, out_shapes
        self.n = next(iter(args.values())).shape[0]

    def on(self, dev, args=None):
        return {k: v.to(dev) for k, v in (self.args if args is None else args).items()}


_OPS = {}


def _cached(fn):
    @functools.wraps(fn)
    def wrapper(dev, *key):
        if (fn.__name__,) + key not in _OPS:
            _OPS[(fn.__name__,) + key] = fn(dev, *key)
        return _OPS[(fn.__name__,) + key]
    return wrapper


@functools.lru_cache(maxsize=None)
def _conv_problem(cins, oc, h, w, n, k, stride):
    """Inputs, weight and grad_out in fp64 (exactly representable in fp32) and the gradients fp64 autograd gives."""
    g = torch.Generator().manual_seed(97 * n + 13 * h + w + 7 * k + stride + 1000 * len(cins) + oc)
    xs = [torch.randn(n, c, h, w, generator=g, dtype=torch.float64).float().double().requires_grad_(True) for c in cins]
    cin = sum(cins)
    weight = (torch.randn(oc, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5).float().double().requires_grad_(True)
    u = F.conv2d(torch.cat(xs, 1), weight, None, stride=stride, padding=k // 2)
    grad_out = torch.randn(u.shape, generator=g, dtype=torch.float64).float().double()
    grads = torch.autograd.grad(u, xs + [weight], grad_out)
    assert float(weight.detach().abs().min()) > 0
    return dict(xs=[x.detach() for x in xs], weight=weight.detach(), grad_out=grad_out, grad_xs=list(grads[:-1]), grad_w=grads[-1])


def _fractions(label, got, want, tol):
    for i, (a, b) in enumerate(zip(got, want)):
        assert tuple(a.shape) == tuple(b.shape) and bool(torch.isfinite(a).all()), (label, i)
        f = pgo.fraction(a, b)
        print(f"{label} result {i}: {f:.2e} of |b| + rms(b) (gate {tol:.0e})")
        assert f <= tol, (label, i, f)


@_cached
def conv_data_op(dev, cins, oc, h, w, n, k, stride):
    c = _conv_problem(cins, oc, h, w, n, k, stride)
    label = f"data gradient {cins} -> {oc}, {n} x {h} x {w}, k {k} stride {stride}"
    blob = ops.pack_conv2d_data_gradient_weight(c["weight"].float().to(dev), stride)
    if stride == 2 and k > 1:      # one or two results, as the conv had one or two inputs
        want, shapes = c["grad_xs"], [(n, ch, h, w) for ch in cins]
        call = lambda d, out=None: ops.conv2d_s2_backward_data(d["grad_out"], blob, cins, k, h, w, out=out)
    else:                          # one input of all the channels
        want, shapes = [torch.cat(c["grad_xs"], 1)], [(n, sum(cins), h, w)]
        call = lambda d, out=None: [ops.conv2d_backward_data(d["grad_out"], blob, sum(cins), k, stride, h, w, out=None if out is None else out[0])]
    return Op(label, {"grad_out": c["grad_out"].float()}, call, lambda got: _fractions(label, got, want, pgo.TOL), ("grad_out",), shapes)


@_cached
def pool_op(dev, n, h, w):
    g = torch.Generator().manual_seed(31 * n + h + w)
    x = torch.randn(n, 5, h, w, generator=g).clamp_min(0.0)            # behind a relu: exact zeros, ties
    grad = torch.randn(n, 5, (h + 1) // 2, (w + 1) // 2, generator=g)
    leaf = x.double().requires_grad_(True)
    y = F.max_pool2d(leaf, 3, stride=2, padding=1)
    (want,) = torch.autograd.grad(y, leaf, grad.double(), retain_graph=True)
    (routed,) = torch.autograd.grad(y, leaf, grad.double().abs())

    def check(got):
        over = (got[0].double().cpu() - want).abs() - 4.0 * EPS * routed
        assert float(over.max()) <= 0.0 and float(got[0].abs().sum()) > 0, float(over.max())
    return Op(f"maxpool3x3s2_backward {n} x 5 x {h} x {w}", {"x": x, "grad_out": grad},
              lambda d, out=None: [ops.maxpool3x3s2_backward(d["x"], d["grad_out"], out=None if out is None else out[0])],
              check, ("x", "grad_out"), [(n, 5, h, w)])


@_cached
def resize_op(dev, n, h, w):
    H, W = 2 * h - 1, 2 * w + 1
    g = _rand((n, 5, H, W), 41 * n + h + w)
    wants = []
    for cot in (g, torch.ones_like(g), g.abs()):
        x = torch.zeros(n, 5, h, w, dtype=torch.float64, requires_grad=True)
        F.interpolate(x, size=(H, W), mode="nearest").backward(cot)
        wants.append(x.grad)
    want, count, mag = wants
    assert float(count.min()) >= 1

    def check(got):
        assert bool(((got[0].double().cpu() - want).abs() <= (count - 1) * EPS * mag).all())
    return Op(f"resize_nearest_backward {n} x 5 x {H} x {W} -> {h} x {w}", {"grad_out": g.float()},
              lambda d, out=None: [ops.resize_nearest_backward(d["grad_out"], h, w, out=None if out is None else out[0])],
              check, ("grad_out",), [(n, 5, h, w)])


@_cached
def kb_xyz_op(dev, n, h, w):
    z = _rand((n, 1, h, w), 51 * n + h)
    z = (torch.where(z < 0, -torch.ones_like(z), torch.ones_like(z)) * (z.abs() + 0.05)).float().double()      # away from the kink
    coords, g = _rand((n, 3, h, w), 52 * n + h), _rand((n, 3, h, w), 53 * n + h)
    dz = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.2))
    terms = coords * g
    want = dz * terms.sum(dim=1, keepdim=True)
    bound = 8 * EPS * (dz.abs() * terms.abs().sum(dim=1, keepdim=True))

    def check(got):
        assert bool(((got[0].double().cpu() - want).abs() <= bound).all())
    return Op(f"kb_xyz_backward {n} x {h} x {w}", {"z": z.float(), "coordinates": coords.float(), "grad_xyz": g.float()},
              lambda d, out=None: [ops.kb_xyz_backward(d["z"], d["coordinates"], d["grad_xyz"], 0.2, out=None if out is None else out[0])],
              check, ("z", "coordinates", "grad_xyz"), [(n, 1, h, w)])


@_cached
def add_act_op(dev, n, h, w):
    y, gy = _rand((n, 5, h, w), 61 * n + h).float(), _rand((n, 5, h, w), 62 * n + h).float()
    y[:, :, :2, :3] = 0.0                                              # the slope branch AT 0
    want = torch.where(y > 0, gy, 0.2 * gy)

    def check(got):
        assert torch.equal(got[0].cpu(), want)
    return Op(f"add_act_backward {n} x 5 x {h} x {w}", {"y": y, "grad_y": gy},
              lambda d, out=None: [ops.add_act_backward(d["y"].contiguous(), d["grad_y"].contiguous(), 0.2)], check, (), None)


@_cached
def depth_map_op(dev, n, h, w):
    dmin, dmax = 1.5, 100.0
    g = torch.Generator().manual_seed(71 * n + h)
    logits = (16 * torch.rand(n, 1, h, w, generator=g, dtype=torch.float64) - 8).float().double()
    cot = _rand((n, 1, h, w), 72 * n + h)
    leaf = logits.clone().requires_grad_(True)
    (dmin / (torch.sigmoid(leaf) + dmin / dmax)).backward(cot)
    depth = ops.depth_map(logits.float().to(dev), dmin, dmax).detach().cpu()      # what the forward saved: per element, frames apart

    def check(got):
        f = kgo.fraction(got[0], leaf.grad)
        print(f"depth_map_backward {n} x {h} x {w}: {f:.2e} of |b| + rms(b) (gate {kgo.DEPTH_MAP_TOL:.0e})")
        assert f <= kgo.DEPTH_MAP_TOL
    return Op(f"depth_map_backward {n} x 1 x {h} x {w}", {"logits": logits.float(), "depth": depth, "grad_depth": cot.float()},
              lambda d, out=None: [ops.depth_map_backward(d["logits"].contiguous(), d["depth"].contiguous(), d["grad_depth"].contiguous(), dmin)],
              check, (), None)


@_cached
def bn_op(dev, n, h, w):
    """batch_norm_act_backward on the running statistics: grad_u (a thread per element); grad_gamma and grad_beta sum over frames."""
    c = pcases.bn_case(0.2, False, n=n, c=5, h=h, w=w, seed=n)
    vec = {k: c[k].float().to(dev) for k in ("gamma", "beta", "mean", "var")}
    label = f"batch_norm_act_backward {n} x 5 x {h} x {w}"

    def call(d, out=None, full=False):
        got = ops.batch_norm_act_backward(d["u"], d["grad_y"], vec["gamma"], vec["beta"], vec["mean"], vec["var"], pgo.EPS, 0.2, False)
        return list(got) if full else [got[0]]
    return Op(label, {"u": c["u"].float(), "grad_y": c["grad_y"].float()}, call, lambda got: _fractions(label, got, [c["grad_u"]], pgo.TOL),
              ("u", "grad_y"), None)


ELEMENTWISE = [(fn, n, h, w) for fn in (pool_op, resize_op, kb_xyz_op, add_act_op, depth_map_op, bn_op) for n in FRAMES for h, w in MAPS]
_op_id = lambda s: f"{s[0].__name__}-{s[1]}x{s[2]}x{s[3]}"


def _make(dev, spec):
    return spec[0](dev, *spec[1:])


# ---------------------------------------------------------------- properties 1, 2, 3 (and 6 on their batched results)
def _frame_alone(dev, op):
    args = op.on(dev)
    batched = op.call(args)
    op.check(batched)
    for i in range(op.n):
        alone = op.call({k: v[i:i + 1] for k, v in args.items()})
        for j, (a, b) in enumerate(zip(batched, alone)):
            assert tuple(b.shape) == (1,) + tuple(a.shape[1:]) and torch.equal(a[i:i + 1], b), f"{op.label}: frame {i} of result {j} is not the frame alone"


def _frame_order(dev, op):
    args = op.on(dev)
    batched = op.call(args)
    perm = torch.roll(torch.arange(op.n), 1).to(dev)
    assert not bool((perm.cpu() == torch.arange(op.n)).any())
    moved = op.call({k: v[perm] for k, v in args.items()})
    op.check([t[torch.argsort(perm)] for t in moved])
    for j, (a, b) in enumerate(zip(batched, moved)):
        assert torch.equal(a[perm], b), f"{op.label}: result {j} does not move with its frames"


def _batch_strides(dev, op):
    args = op.on(dev)
    dense = op.call(args)
    strides = _Strides(dev)
    sliced = {k: (strides.holding(v) if k in op.sliced else v) for k, v in args.items()}
    outs = None if op.out_shapes is None else [strides.view(s, GUARD) for s in op.out_shapes]
    got = op.call(sliced, None if outs is None else [view for _, view in outs])
    op.check(got)
    for j, (a, b) in enumerate(zip(got, dense)):
        assert torch.equal(a, b), f"{op.label}: result {j} on channel slices differs from the dense call"
    if outs is not None:
        seen = {t.stride(0) for k, t in sliced.items() if k in op.sliced} | {view.stride(0) for _, view in outs}
        assert len(seen) == len(op.sliced) + len(outs)                 # no two batch strides agree
        for (whole, view), a, shape in zip(outs, got, op.out_shapes):
            assert a.data_ptr() == view.data_ptr() and _guards_intact(whole, shape), f"{op.label}: a guard value was overwritten"


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_conv_data_gradient_of_a_frame_alone(dev, case):
    _frame_alone(dev, conv_data_op(dev, *case))


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_conv_data_gradient_moves_with_the_frame_order(dev, case):
    _frame_order(dev, conv_data_op(dev, *case))


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_conv_data_gradient_on_unequal_batch_strides(dev, case):
    _batch_strides(dev, conv_data_op(dev, *case))


@pytest.mark.parametrize("spec", ELEMENTWISE, ids=_op_id)
def test_gradient_of_a_frame_alone(dev, spec):
    _frame_alone(dev, _make(dev, spec))


@pytest.mark.parametrize("spec", ELEMENTWISE, ids=_op_id)
def test_gradient_moves_with_the_frame_order(dev, spec):
    _frame_order(dev, _make(dev, spec))


@pytest.mark.parametrize("spec", [s for s in ELEMENTWISE if s[0] not in (add_act_op, depth_map_op)], ids=_op_id)
def test_gradient_on_unequal_batch_strides(dev, spec):
    _batch_strides(dev, _make(dev, spec))


def _weight_gradient(dev, d_xs, d_g, k, stride, splits=None, out=None):
    if stride == 2 and k > 1:
        return ops.conv2d_s2_backward_weight(d_xs, d_g, k, splits=splits, out=out)
    return ops.conv2d_backward_weight(d_xs, d_g, k, stride, splits=splits, out=out)


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_weight_gradient_on_unequal_batch_strides(dev, case):
    """The one or two inputs and grad_out as channel slices with three different batch strides, the result inside a guarded buffer:
    the dense call's bits, within the operator gate of fp64 autograd, with every split."""
    cins, oc, h, w, n, k, stride = case
    c = _conv_problem(*case)
    xs, g = [x.float().to(dev) for x in c["xs"]], c["grad_out"].float().to(dev)
    strides = _Strides(dev)
    sliced_xs, sliced_g = [strides.holding(x) for x in xs], strides.holding(g)
    assert len({t.stride(0) for t in sliced_xs + [sliced_g]}) == len(xs) + 1
    count = oc * sum(cins) * k * k
    for splits in (None, 1, 3):
        dense = _weight_gradient(dev, xs, g, k, stride, splits)
        _fractions(f"weight gradient {case} splits {splits}", [dense], [c["grad_w"]], pgo.TOL)
        whole = torch.full((count + 8,), GUARD, device=dev)
        view = whole[4:-4].view(oc, sum(cins), k, k)
        got = _weight_gradient(dev, sliced_xs, sliced_g, k, stride, splits, out=view)
        assert got.data_ptr() == view.data_ptr() and torch.equal(got, dense), (case, splits)
        assert bool((whole[:4] == GUARD).all()) and bool((whole[-4:] == GUARD).all()), (case, splits)


# ---------------------------------------------------------------- property 4: containment of non-finite values, data gradients
def _tap_axis(size, k, stride, o):
    """Along one axis: for every input position the tap that joins it to output position `o` (position + k // 2 - tap == stride o),
    or -1 where no tap does."""
    tap = torch.arange(size) + k // 2 - stride * o
    return torch.where((tap >= 0) & (tap < k), tap, torch.full_like(tap, -1))


def _receptive_field(h, w, k, stride, oy, ox):
    """(mask h x w of the input pixels that output pixel (oy, ox) reads, ky h x 1, kx 1 x w): index arithmetic, the specification."""
    ky, kx = _tap_axis(h, k, stride, oy).view(h, 1), _tap_axis(w, k, stride, ox).view(1, w)
    return (ky >= 0) & (kx >= 0), ky, kx


def _interior(h, w, k, stride):
    """An output pixel with every tap inside the image, near the middle."""
    oh, ow = -(-h // stride), -(-w // stride)
    oy, ox = oh // 2, ow // 2
    for o, size in ((oy, h), (ox, w)):
        assert stride * o - k // 2 >= 0 and stride * o + k // 2 < size
    return oy, ox


def _contained(label, got, clean, mid, masks, bad, expect=None):
    """`got` against `clean` (lists of results): the frames other than `mid` keep their bits, and so does everything outside `masks`
    (one bool tensor C x H x W per result) in frame `mid`; inside, NaN for a NaN, `expect` (or anything non-finite) for an infinity."""
    for j, (a, c, mask) in enumerate(zip(got, clean, masks)):
        assert bool(torch.isfinite(c).all()) and int(mask.sum()) > 0
        for i in range(a.shape[0]):
            if i != mid:
                assert torch.equal(a[i], c[i]), f"{label}: frame {i} of result {j} changed"
        m = mask.to(a.device)
        assert torch.equal(a[mid][~m], c[mid][~m]), f"{label}: result {j} changed outside the receptive field"
        inside = a[mid][m]
        if math.isnan(bad):
            assert bool(torch.isnan(inside).all()), f"{label}: result {j} has a number inside the receptive field"
        elif expect is None:
            assert not bool(torch.isfinite(inside).any()), f"{label}: result {j} has a finite value inside the receptive field"
        else:
            assert torch.equal(inside, expect[j].to(a.device)[m].float()), f"{label}: result {j} has the wrong infinities"


@pytest.mark.parametrize("case", POISON_CASES, ids=_conv_id)
def test_conv_data_gradient_contains_a_non_finite_gradient(dev, case):
    cins, oc, h, w, n, k, stride = case
    op = conv_data_op(dev, *case)
    c = _conv_problem(*case)
    mid, f = n // 2, oc // 2
    oy, ox = _interior(h, w, k, stride)
    field, ky, kx = _receptive_field(h, w, k, stride, oy, ox)
    assert int(field.sum()) == k * k                          # every tap inside the image: k x k input pixels, one tap each
    met = c["weight"][f][:, ky.clamp_min(0), kx.clamp_min(0)].reshape(sum(cins), h, w)      # the one weight every element meets
    split = list(cins) if len(op.out_shapes) == 2 else [sum(cins)]
    masks = [field.expand(ch, h, w) for ch in split]
    clean = op.call(op.on(dev))
    for bad in (NAN, math.inf, -math.inf):
        args = {"grad_out": op.args["grad_out"].clone()}
        args["grad_out"][mid, f, oy, ox] = bad
        expect = None if math.isnan(bad) else list(torch.split(torch.sign(met) * bad, split, dim=0))
        _contained(f"{op.label}, {bad} at {(mid, f, oy, ox)}", op.call(op.on(dev, args)), clean, mid, masks, bad, expect)
        # the arithmetic mask against fp64 autograd on the same inputs
        leaf = torch.cat(c["xs"], 1).clone().requires_grad_(True)
        u = F.conv2d(leaf, c["weight"], None, stride=stride, padding=k // 2)
        (ref,) = torch.autograd.grad(u, leaf, args["grad_out"].double())
        assert torch.equal(~torch.isfinite(ref[mid]), field.expand(sum(cins), h, w)) and bool(torch.isfinite(ref[:mid]).all()) \
            and bool(torch.isfinite(ref[mid + 1:]).all()), f"{op.label}: fp64 autograd's non-finite mask is not the arithmetic one"


@pytest.mark.parametrize("bad", [NAN, math.inf, -math.inf], ids=["nan", "inf", "-inf"])
def test_pool_gradient_contains_a_non_finite_gradient(dev, bad):
    """The window's gradient goes to its first maximum and nowhere else; an infinity keeps its sign through the sum of four windows."""
    n, h, w = 3, 9, 13
    op = pool_op(dev, n, h, w)
    mid, ch, oy, ox = 1, 2, 2, 3
    at = int(rgo.pool_argmax(op.args["x"].double())[mid, ch, oy, ox])
    mask = torch.zeros(5, h, w, dtype=torch.bool)
    mask[ch, at // w, at % w] = True
    args = {k: v.clone() for k, v in op.args.items()}
    args["grad_out"][mid, ch, oy, ox] = bad
    expect = None if math.isnan(bad) else [torch.full((5, h, w), bad)]
    _contained(f"{op.label}, {bad}", op.call(op.on(dev, args)), op.call(op.on(dev)), mid, [mask], bad, expect)
    leaf = args["x"].double().requires_grad_(True)
    (ref,) = torch.autograd.grad(F.max_pool2d(leaf, 3, stride=2, padding=1), leaf, args["grad_out"].double())
    assert torch.equal(~torch.isfinite(ref[mid]), mask) and int((~torch.isfinite(ref)).sum()) == 1


@pytest.mark.parametrize("bad", [NAN, math.inf, -math.inf], ids=["nan", "inf", "-inf"])
def test_resize_gradient_contains_a_non_finite_gradient(dev, bad):
    n, h, w = 3, 9, 13
    op = resize_op(dev, n, h, w)
    H, W = op.args["grad_out"].shape[2:]
    mid, ch, oy, ox = 1, 2, H // 2 + 1, W // 2 + 2
    source = F.interpolate(torch.arange(h * w, dtype=torch.float64).view(1, 1, h, w), size=(H, W), mode="nearest")
    at = int(source[0, 0, oy, ox])
    mask = torch.zeros(5, h, w, dtype=torch.bool)
    mask[ch, at // w, at % w] = True
    args = {"grad_out": op.args["grad_out"].clone()}
    args["grad_out"][mid, ch, oy, ox] = bad
    expect = None if math.isnan(bad) else [torch.full((5, h, w), bad)]
    _contained(f"{op.label}, {bad}", op.call(op.on(dev, args)), op.call(op.on(dev)), mid, [mask], bad, expect)
    leaf = torch.zeros(n, 5, h, w, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(F.interpolate(leaf, size=(H, W), mode="nearest"), leaf, args["grad_out"].double())
    assert torch.equal(~torch.isfinite(ref[mid]), mask) and int((~torch.isfinite(ref)).sum()) == 1


@pytest.mark.parametrize("bad", [NAN, math.inf, -math.inf], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("make, name, channels", [(kb_xyz_op, "grad_xyz", 3), (add_act_op, "grad_y", 5), (depth_map_op, "grad_depth", 1),
                                                  (bn_op, "grad_y", 5)], ids=["kb_xyz", "add_act", "depth_map", "batch_norm_act"])
def test_pixelwise_gradient_contains_a_non_finite_gradient(dev, make, name, channels, bad):
    """A thread per pixel: one bad element of the incoming gradient is one bad element of the result (kb_xyz sums its three channels).
    batch_norm_act_backward also sums over the batch: grad_gamma and grad_beta are non-finite in that channel alone."""
    n, h, w = 3, 9, 13
    op = make(dev, n, h, w)
    mid, ch, y, x = 1, channels // 2, 4, 6
    args = {k: v.clone() for k, v in op.args.items()}
    args[name][mid, ch, y, x] = bad
    out_channels = op.call(op.on(dev))[0].shape[1]
    mask = torch.zeros(out_channels, h, w, dtype=torch.bool)
    mask[ch if out_channels > 1 else 0, y, x] = True
    _contained(f"{op.label}, {bad}", op.call(op.on(dev, args)), op.call(op.on(dev)), mid, [mask], bad)
    if make is bn_op:
        clean, dirty = op.call(op.on(dev), full=True), op.call(op.on(dev, args), full=True)
        for label, a, c in zip(("grad_gamma", "grad_beta"), dirty[1:], clean[1:]):
            keep = torch.arange(5, device=dev) != ch
            assert bool(torch.isfinite(c).all()) and torch.equal(a[keep], c[keep]) and not bool(torch.isfinite(a[ch])), (label, bad)
            if math.isnan(bad):
                assert bool(torch.isnan(a[ch])), label


# ---------------------------------------------------------------- property 5: containment, weight gradient
@pytest.mark.parametrize("case", POISON_CASES, ids=_conv_id)
def test_weight_gradient_contains_a_nan(dev, case):
    cins, oc, h, w, n, k, stride = case
    c = _conv_problem(*case)
    xs, g = [x.float().to(dev) for x in c["xs"]], c["grad_out"].float().to(dev)
    mid, f = n // 2, oc // 2
    oy, ox = _interior(h, w, k, stride)
    # a NaN in grad_out at filter f, at an output pixel whose every tap lies inside the image: row f, and row f alone
    bad_g = g.clone()
    bad_g[mid, f, oy, ox] = NAN
    # a NaN in the last input at its channel cstar, k // 2 or more from every border: the columns of that channel at the taps that reach it
    cstar, iy, ix = cins[-1] // 2, h // 2, w // 2
    assert min(iy, ix, h - 1 - iy, w - 1 - ix) >= k // 2
    bad_xs = [x.clone() for x in xs]
    bad_xs[-1][mid, cstar, iy, ix] = NAN
    column = sum(cins[:-1]) + cstar
    reach_y = [(iy + k // 2 - t) % stride == 0 and 0 <= (iy + k // 2 - t) // stride < -(-h // stride) for t in range(k)]
    reach_x = [(ix + k // 2 - t) % stride == 0 and 0 <= (ix + k // 2 - t) // stride < -(-w // stride) for t in range(k)]
    reached = torch.zeros(oc, sum(cins), k, k, dtype=torch.bool)
    reached[:, column] = torch.tensor(reach_y).view(k, 1) & torch.tensor(reach_x).view(1, k)
    assert 1 <= int(reached[0].sum()) <= k * k
    reached = reached.to(dev)
    for splits in (None, 1, 3):
        clean = _weight_gradient(dev, xs, g, k, stride, splits)
        assert bool(torch.isfinite(clean).all())
        got = _weight_gradient(dev, xs, bad_g, k, stride, splits)
        rows = torch.arange(oc, device=dev) != f
        assert bool(torch.isnan(got[f]).all()), (case, splits, "row f* of the weight gradient must be NaN")
        assert torch.equal(got[rows], clean[rows]), (case, splits, "a NaN of filter f* reached another row")
        got = _weight_gradient(dev, bad_xs, g, k, stride, splits)
        assert bool(torch.isnan(got[reached]).all()), (case, splits, "the columns of the channel must be NaN where a tap reaches the pixel")
        assert torch.equal(got[~reached], clean[~reached]), (case, splits, "a NaN of one channel reached another column")
