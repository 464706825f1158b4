"""The cases the pose network's backward tests share (CPU oracle / power tests, the GPU model tests, the golden generator): what
each is, and its inputs regenerated from seeds (kbnet_amd.synthetic) instead of stored."""
import numpy as np
import torch

import kbnet_amd as kb
import posenet_grad_oracle as pgo

FULL = list(kb.posenet.POSENET_FILTERS)

# the two goldens (tests/golden/posenet_grad_*.npz): the reference's own autograd
GOLDEN = {
    "posenet_grad_eval": dict(filters=pgo.FILTERS, n=2, h=61, w=77, seed=71, batch_norm="running"),
    "posenet_grad_train": dict(filters=pgo.FILTERS, n=2, h=130, w=136, seed=73, batch_norm="batch"),
}
# every (network, shape, mode) the GPU model tests run: the gate's TOL is measured over these
MODEL = dict(GOLDEN)
MODEL.update({
    "narrow_train_shape_running": dict(filters=pgo.FILTERS, n=2, h=130, w=136, seed=73, batch_norm="running"),
    "full_running": dict(filters=FULL, n=2, h=64, w=96, seed=75, batch_norm="running"),
    "full_batch": dict(filters=FULL, n=2, h=192, w=256, seed=77, batch_norm="batch"),   # last map 2 x 2: 8 values per channel
    # three and five frames on tiny maps: a 128-pixel tile or a 32-pixel K chunk of the deepest levels holds three or more frames, and
    # frames straddle tiles.  Seeds by the rule written in resnet_pose_grad_cases.py, the first from 78 on with both properties.
    "narrow_n3_running": dict(filters=pgo.FILTERS, n=3, h=20, w=36, seed=78, batch_norm="running"),   # maps 10 x 18, 5 x 9, 3 x 5, 2 x 3, 1 x 2, 1 x 1, 1 x 1
    "narrow_n5_running": dict(filters=pgo.FILTERS, n=5, h=21, w=43, seed=80, batch_norm="running"),   # maps 11 x 22, 6 x 11, 3 x 6, 2 x 3, 1 x 2, 1 x 1, 1 x 1
    "narrow_n3_batch": dict(filters=pgo.FILTERS, n=3, h=33, w=260, seed=78, batch_norm="batch"),      # last map 1 x 3: 9 values per channel
})


def inputs(c):
    """(image0, image1, encoder state dict, decoder state dict, cotangent N x 4 x 4 fp64), CPU."""
    sd_enc, sd_dec = kb.synthetic.make_posenet_weights(c["filters"], seed=c["seed"])
    image0, image1 = kb.synthetic.make_image_pair(c["n"], c["h"], c["w"], seed=c["seed"] + 100)
    cot = torch.from_numpy(np.random.default_rng(c["seed"] + 200).standard_normal((c["n"], 4, 4)))
    return image0, image1, sd_enc, sd_dec, cot


def checksums(image0, image1, sd_enc, sd_dec):
    """Sums (fp64) that tie regenerated inputs to the ones a golden was made from."""
    out = {"image0": float(image0.double().sum()), "image1": float(image1.double().sum())}
    for grp, sd in (("enc", sd_enc), ("dec", sd_dec)):
        out[grp] = float(sum(v.double().abs().sum() for v in sd.values() if v.is_floating_point()))
    return out


def last_map_values(c):
    h, w = c["h"], c["w"]
    for _ in range(7):
        h, w = (h + 1) // 2, (w + 1) // 2
    return c["n"] * h * w


# ---- operator cases (tests/test_posenet_backward_gpu.py; the power tests plant their mistakes on the same ones) ----
# (frames, channels of the one or two inputs, height, width, filters): every one runs at k = 3, 5 and 7
CONV_SHAPES = [
    (1, (1,), 1, 1, 3),         # only the centre tap
    (1, (2,), 2, 3, 5),
    (2, (5,), 9, 13, 19),       # neither channel count a multiple of 16 or 4
    (3, (7,), 17, 23, 70),      # 324 output pixels: 128-pixel tiles span rows and frames; two filter tiles; unequal parity classes
    (2, (3, 3), 8, 10, 10),     # two inputs, even sizes
]
# (frames, channels, height, width, filters, k): the weight gradient's K split at its two ends
WGRAD_SPLIT_SHAPES = [
    (4, (3,), 65, 129, 8, 7),   # long K (8580 output pixels, no multiple of 32), small M x N
    (2, (40,), 3, 5, 72, 3),    # short K (12 output pixels: less than one chunk), wide M x N
]


def conv_case(n, cins, h, w, oc, k, seed=0):
    """(inputs, weight, grad_out) fp64 CPU, and the fp64 gradients torch.autograd gives: (grad_inputs, grad_weight)."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * n + 13 * h + w + k)
    xs = [torch.randn(n, c, h, w, generator=g, dtype=torch.float64).float().double().requires_grad_(True) for c in cins]
    weight = (torch.randn(oc, sum(cins), k, k, generator=g, dtype=torch.float64) / (sum(cins) * k * k) ** 0.5).float().double().requires_grad_(True)
    out = torch.nn.functional.conv2d(torch.cat(xs, 1), weight, None, stride=2, padding=k // 2)
    grad_out = torch.randn(out.shape, generator=g, dtype=torch.float64).float().double()
    grads = torch.autograd.grad(out, xs + [weight], grad_out)
    return [x.detach() for x in xs], weight.detach(), grad_out, list(grads[:-1]), grads[-1]


def bn_case(slope, batch, n=3, c=5, h=7, w=9, seed=0, zeros=False):
    """One batch_norm_act problem in fp64 (values exactly representable in fp32): dict with u, grad_y, gamma, beta, mean, var and
    the fp64 autograd gradients.  Every |z| exceeds 1e-3 rms(z) (elements closer to the kink are pushed away from it, none is left
    out) -- or, with `zeros`, a region of z is EXACTLY 0 in both precisions (u = 0, mean = 0, beta = 0: the slope branch at 0)."""
    g = torch.Generator().manual_seed(500 + seed + (7 if batch else 0))
    u = (0.7 * torch.randn(n, c, h, w, generator=g, dtype=torch.float64) + 0.3).float().double()
    gamma = (0.5 + torch.rand(c, generator=g, dtype=torch.float64)).float().double()
    beta = (0.2 * torch.randn(c, generator=g, dtype=torch.float64)).float().double()
    mean = (0.2 * torch.randn(c, generator=g, dtype=torch.float64)).float().double()
    var = (0.25 + torch.rand(c, generator=g, dtype=torch.float64)).float().double()
    if zeros:
        assert not batch
        mean.zero_()
        beta.zero_()
        u[:, :, :3, :4] = 0.0
    else:
        for _ in range(4):   # move what sits near the kink away from it (the statistics of a batch move a little with it)
            _, _, _, z = pgo.batch_norm_act(u, gamma, beta, mean, var, slope=slope, batch=batch)
            near = z.abs() <= 4e-3 * po_rms(z)
            if not near.any():
                break
            u = torch.where(near, u + 0.05, u).float().double()
    grad_y = torch.randn(n, c, h, w, generator=g, dtype=torch.float64).float().double()
    leaves = [t.clone().requires_grad_(True) for t in (u, gamma, beta)]
    y, _, _, z = pgo.batch_norm_act(leaves[0], leaves[1], leaves[2], mean, var, slope=slope, batch=batch)
    gu, gg, gb = torch.autograd.grad(y, leaves, grad_y)
    return dict(u=u, grad_y=grad_y, gamma=gamma, beta=beta, mean=mean, var=var, z=z.detach(), y=y.detach(), grad_u=gu, grad_gamma=gg,
                grad_beta=gb)


def po_rms(t):
    return float(t.double().pow(2).mean().sqrt())
