"""The cases of tests/test_grad_extents_gpu.py and tests/test_grad_extents_cpu.py: the conv and BatchNorm gradients summed over a
training-size pixel count.  Every operator case sums over M = 71 806 output pixels, 2 frames of 161 x 223: 2243.9 chunks of 32 (the
last chunk ragged, chunk 1121 across the frame boundary), above the 65 536 pixels at which bwd_weight_plan's aimed-for split count
reaches its 512-workgroup cap with one tile, above the 32 768 past which more than BW_MAX_SPLITS = 1024 chunks exist, and small
enough that ONE dropped or doubled term of size 1 is 1 / (|b| + rms(b)) = 4e-3 with rms(b) = sqrt(M) = 268: 20 x the 2e-4 gate.
Inputs are regenerated from seeds and exactly representable in fp32; the references are torch autograd in fp64 on the CPU, computed
once per case (functools.lru_cache) and never written to."""
import functools

import torch
import torch.nn.functional as F

import posenet_grad_oracle as pgo

N, OH, OW = 2, 161, 223
M = N * OH * OW                       # 71 806
CHUNK, CHUNKS = 32, -(-M // 32)       # 2244
ODD, EVEN = (321, 445), (322, 446)    # the stride-2 inputs of a 161 x 223 map: the last row and column read by the centre tap, or never
SAME = (OH, OW)
SPLITS = (None, 1, 7, 1 << 20)
assert M == 71806 and CHUNKS == 2244 and M % CHUNK == 30 and (OH * OW) % CHUNK != 0


def _w(name, k, stride, cins, oc, size, auto, most, sliced=False):
    return dict(name=name, k=k, stride=stride, cins=cins, oc=oc, size=size, auto=auto, most=most, sliced=sliced)


# The weight gradient.  `auto`: the split count bwd_weight_plan picks from the shape, `most`: the one it makes of splits = 1 << 20 --
# tests/test_grad_extents_cpu.py reads both from the library.  Splits aimed for: ceil(512 / tiles), tiles = ceil(C k k / 64) (one
# filter tile in every case); cps = ceil(2244 / aimed) chunks per split; splits = ceil(2244 / cps).  One tile: 512 -> 5 -> 449;
# two: 256 -> 9 -> 250; three: 171 -> 14 -> 161; four: 128 -> 18 -> 125; 1 << 20: 1024 -> 3 -> 748.  splits = 7 stays 7 (of 321).
# 8, 24, 40 filters: bw_mb's 16-, 32- and 64-row tiles (MB = 1, 2, 4), the last with 24 empty rows.
WGRAD = [
    _w("k3s1_f8", 3, 1, (3,), 8, SAME, 449, 748), _w("k3s1_f24", 3, 1, (3,), 24, SAME, 449, 748), _w("k3s1_f40", 3, 1, (3,), 40, SAME, 449, 748),
    _w("k1s1_f8", 1, 1, (3,), 8, SAME, 449, 748), _w("k1s1_f24", 1, 1, (3,), 24, SAME, 449, 748), _w("k1s1_f40", 1, 1, (3,), 40, SAME, 449, 748),
    _w("k1s2_f8", 1, 2, (3,), 8, ODD, 449, 748), _w("k1s2_f24", 1, 2, (3,), 24, EVEN, 449, 748), _w("k1s2_f40", 1, 2, (3,), 40, ODD, 449, 748),
    _w("k3s2_f8", 3, 2, (3,), 8, EVEN, 449, 748), _w("k3s2_f24", 3, 2, (3,), 24, ODD, 449, 748), _w("k3s2_f40", 3, 2, (3,), 40, EVEN, 449, 748),
    _w("k5s2_f8", 5, 2, (3,), 8, ODD, 250, 748), _w("k5s2_f24", 5, 2, (3,), 24, EVEN, 250, 748), _w("k5s2_f40", 5, 2, (3,), 40, ODD, 250, 748),
    _w("k7s2_f8", 7, 2, (3,), 8, EVEN, 161, 748), _w("k7s2_f24", 7, 2, (3,), 24, ODD, 161, 748), _w("k7s2_f40", 7, 2, (3,), 40, EVEN, 161, 748),
    # two inputs, one per entry point: 72 and 200 columns
    _w("k3s1_two_inputs", 3, 1, (3, 5), 24, SAME, 250, 748), _w("k5s2_two_inputs", 5, 2, (3, 5), 8, EVEN, 125, 748),
    # inputs and grad_out as channel slices of wider tensors, one per entry point: every batch stride exceeds C H W
    _w("k3s1_slices", 3, 1, (3,), 8, SAME, 449, 748, sliced=True), _w("k7s2_slices", 7, 2, (3,), 8, ODD, 161, 748, sliced=True),
]
# The data gradient: (filters of grad_out) -> (channels of the gradient) 8 -> 3 and 40 -> 19: at 40 filters k = 1 has 2.5 chunks of 16
# filters, 19 is no multiple of 4.  At stride 1 the 128-pixel tiles cover M: 561, the last ragged; at stride 2 they cover the INPUT
# pixels (2 x 321 x 445 = 285 690 or 2 x 322 x 446 = 287 224: 2232 and 2244 tiles, the first count ragged) and gather from the M.
DGRAD = [dict(name=f"k{k}s{s}_f{oc}_c{c}", k=k, stride=s, cins=(c,), oc=oc, size=size)
         for (k, s), sizes in (((3, 1), (SAME, SAME)), ((1, 1), (SAME, SAME)), ((1, 2), (ODD, EVEN)), ((3, 2), (EVEN, ODD)), ((5, 2), (ODD, EVEN)),
                               ((7, 2), (EVEN, ODD)))
         for (oc, c), size in zip(((8, 3), (40, 19)), sizes)]
# One recorded conv (ops.conv2d_kbnet): three inputs, the activation in the epilogue, every gradient asked for
NODE = dict(name="node_k3s1", k=3, stride=1, cins=(3, 5, 7), oc=24, size=SAME, slope=0.2)
S2_ENTRY = ((3, 2), (5, 2), (7, 2))     # ops.conv2d_s2_backward_*; the rest: ops.conv2d_backward_*


def _seed(c):
    return 7000 + 100 * c["k"] + 10 * c["stride"] + sum(c["cins"]) + c["oc"] + c["size"][0]


def _rand(shape, g, scale=1.0):
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).float().double()


@functools.lru_cache(maxsize=None)
def _conv_inputs(name):
    c = by_name(name)
    g = torch.Generator().manual_seed(_seed(c))
    h, w = c["size"]
    xs = tuple(_rand((N, ci, h, w), g) for ci in c["cins"])
    cin, k = sum(c["cins"]), c["k"]
    weight = _rand((c["oc"], cin, k, k), g, 1.0 / (cin * k * k) ** 0.5)
    grad_out = _rand((N, c["oc"], OH, OW), g)
    assert (-(-h // c["stride"]), -(-w // c["stride"])) == (OH, OW)
    return xs, weight, grad_out


def by_name(name):
    return next(c for c in WGRAD + DGRAD + [NODE] if c["name"] == name)


def conv_inputs(c):
    """(inputs, weight, grad_out) fp64 CPU, exactly representable in fp32.  Shared: do not write to them."""
    return _conv_inputs(c["name"])


def conv_gradients(c, dtype=torch.float64, weight_grad=True, data_grad=False, mask=None):
    """torch autograd in `dtype` of [act](conv(cat(inputs))) -> (grad_weight or None, [grad_input] or None, pre-activation u).
    `mask`: the branches of the case's activation (True: the identity) instead of the signs of u."""
    xs, weight, grad_out = conv_inputs(c)
    leaves = [x.to(dtype).clone().requires_grad_(data_grad) for x in xs]
    wt = weight.to(dtype).clone().requires_grad_(weight_grad)
    u = F.conv2d(torch.cat(leaves, dim=1), wt, None, stride=c["stride"], padding=c["k"] // 2)
    slope = c.get("slope")
    y = u if slope is None else torch.where(u > 0 if mask is None else mask, u, slope * u)
    wanted = ([wt] if weight_grad else []) + (leaves if data_grad else [])
    grads = list(torch.autograd.grad(y, wanted, grad_out.to(dtype)))
    gw = grads.pop(0) if weight_grad else None
    return gw, (grads if data_grad else None), u.detach()


@functools.lru_cache(maxsize=None)
def weight_gradient(name):
    return conv_gradients(by_name(name))[0]


@functools.lru_cache(maxsize=None)
def data_gradient(name):
    return conv_gradients(by_name(name), weight_grad=False, data_grad=True)[1][0]


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------
BN_C = 5
BN_RATIO = (4.0, -8.0, 16.0, -32.0, 64.0)    # a channel's mean over its spread: E[x^2] - mean^2 in fp32 would lose up to 64^2 2^-24 = 2e-4
#                                              of the variance, 200 x the 1e-6 bar; z = u scale + shift in fp32 keeps 64 x 2^-24 = 4e-6 of z
BN_EPS = pgo.EPS
# seeds by mode, the first from 1 on at which bn_kink_margin exceeds 1 (tests/test_grad_extents_cpu.py asserts it)
BN_SEED = {False: 3, True: 1}


@functools.lru_cache(maxsize=None)
def _bn_inputs(batch, seed):
    g = torch.Generator().manual_seed(9000 + 2 * seed + int(batch))
    sigma = 0.5 + torch.rand(BN_C, generator=g, dtype=torch.float64)
    centre = sigma * torch.tensor(BN_RATIO, dtype=torch.float64)
    u = (centre.view(1, -1, 1, 1) + sigma.view(1, -1, 1, 1) * torch.randn(N, BN_C, OH, OW, generator=g, dtype=torch.float64)).float().double()
    gamma = (0.5 + torch.rand(BN_C, generator=g, dtype=torch.float64)).float().double()
    beta = (0.2 * torch.randn(BN_C, generator=g, dtype=torch.float64)).float().double()
    mean = (centre + 0.1 * sigma * torch.randn(BN_C, generator=g, dtype=torch.float64)).float().double()
    var = (sigma ** 2 * (0.8 + 0.4 * torch.rand(BN_C, generator=g, dtype=torch.float64))).float().double()
    grad_y = _rand((N, BN_C, OH, OW), g)
    return dict(u=u, gamma=gamma, beta=beta, mean=mean, var=var, grad_y=grad_y)


def bn_inputs(batch, seed=None):
    """u 2 x 5 x 161 x 223 with channel means 4 to 64 spreads from 0, gamma, beta, the running mean and variance (used without
    `batch`) and grad_y: fp64 CPU, exactly representable in fp32.  Shared: do not write to them."""
    return _bn_inputs(bool(batch), BN_SEED[bool(batch)] if seed is None else seed)


def bn_pre_activation(c, batch):
    """(z, scale, shift) in fp64: z = u scale + shift, the pre-activation on the case's statistics."""
    mean, var = (c["u"].mean(dim=(0, 2, 3)), c["u"].var(dim=(0, 2, 3), unbiased=False)) if batch else (c["mean"], c["var"])
    scale = c["gamma"] * torch.rsqrt(var + BN_EPS)
    shift = c["beta"] - mean * scale
    return c["u"] * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), scale, shift


def bn_kink_margin(c, batch):
    """min over the elements of |z| / band, band = 4 x 2^-24 (|u scale| + |shift|): what an fp32 run can resolve of z.  The device
    forms z = fma(u, scale, shift) from fp32 scale and shift; an error of scale moves u scale and mean scale alike, which leaves
    the rounding of shift (2^-24 |shift|), of the mean and variance it came from (as much again) and of the sum itself: two to three
    of these units, taken as four.  Above 1, the sign of every fp32 z IS the sign of the fp64 one: a device mask must equal it."""
    z, scale, shift = bn_pre_activation(c, batch)
    band = 4.0 * 2.0 ** -24 * ((c["u"] * scale.view(1, -1, 1, 1)).abs() + shift.abs().view(1, -1, 1, 1))
    return float((z.abs() / band).min())


def bn_gradients(c, slope, batch, dtype=torch.float64, mask=None):
    """torch autograd in `dtype` -> dict y, z, mean, var (the statistics used), grad_u, grad_gamma, grad_beta."""
    leaves = [c[k].to(dtype).clone().requires_grad_(True) for k in ("u", "gamma", "beta")]
    y, mean, var, z = pgo.batch_norm_act(leaves[0], leaves[1], leaves[2], c["mean"].to(dtype), c["var"].to(dtype), eps=BN_EPS, slope=slope,
                                         batch=batch, mask=mask)
    gu, gg, gb = torch.autograd.grad(y, leaves, c["grad_y"].to(dtype))
    return dict(y=y.detach(), z=z.detach(), mean=mean.detach(), var=var.detach(), grad_u=gu, grad_gamma=gg, grad_beta=gb)


# ---- the split sum written out (tests/test_grad_extents_cpu.py plants its mistakes here) ----------------------------------
def gemm_operands(c):
    """The weight gradient as grad_w[oc, col] = sum_m A[m, oc] B[m, col] over the M output pixels in (frame, oy, ox) order:
    A = grad_out, B = the input at the column's (channel, ky, kx) tap, zero outside the map.  -> (A M x F, B M x C k k), fp64."""
    xs, _, grad_out = conv_inputs(c)
    x = torch.cat(xs, dim=1)
    cols = F.unfold(x, c["k"], padding=c["k"] // 2, stride=c["stride"])          # N x C k k x OH OW
    return grad_out.permute(0, 2, 3, 1).reshape(M, c["oc"]), cols.permute(0, 2, 1).reshape(M, -1)
