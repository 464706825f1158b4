"""The cases the ResNet pose networks' backward tests share (CPU oracle / power tests, the GPU model tests, the golden generator):
what each is, and its inputs regenerated from seeds (kbnet_amd.synthetic) instead of stored."""
import numpy as np
import torch

import kbnet_amd as kb
import posenet_grad_cases as pcases
import resnet_pose_grad_oracle as rgo

NARROW = dict(filters=rgo.FILTERS, decoder_filters=rgo.DECODER_FILTERS)
FULL = dict(filters=list(kb.posenet_resnet.RESNET_FILTERS), decoder_filters=list(kb.posenet_resnet.RESNET_DECODER_FILTERS))

# the two goldens (tests/golden/resnet_pose_grad_18_*.npz): the reference's own autograd
GOLDEN = {
    "resnet_pose_grad_18_eval": dict(NARROW, n_layer=18, n=2, h=61, w=77, seed=81, batch_norm="running"),
    "resnet_pose_grad_18_train": dict(NARROW, n_layer=18, n=2, h=130, w=136, seed=83, batch_norm="batch"),
}
# every (network, shape, mode) the GPU model tests run against the fp64 oracle: the gate's TOL is measured over these and the goldens.
# The seeds were picked on the CPU, from the fp64 oracle alone, for two properties: (a) the oracle's own fp32 autograd stays under a
# third of the gate's ceiling (1e-3 / 3: the 8-value BatchNorm2d that ends full_18_batch puts most seeds between 2e-4 and 5e-4 at
# dec::conv.1.conv.weight, one of 36 at 1.5e-3), and (b) no activation has more pre-activations within 5e-6 rms(z) of 0 than
# kink_check lets flip -- a property of the fp64 values, so that an fp32 run's few branch flips cannot exceed kink_check's share by
# bad luck.  85 and 96 are the first from 85 on with both; of 89 .. 124, 91, 94 and 113 have both for full_18_batch.
MODEL = dict(GOLDEN)
MODEL.update({
    "narrow_34_running": dict(NARROW, n_layer=34, n=2, h=130, w=136, seed=85, batch_norm="running"),
    "narrow_34_batch": dict(NARROW, n_layer=34, n=2, h=130, w=136, seed=85, batch_norm="batch"),
    "full_18_running": dict(FULL, n_layer=18, n=2, h=64, w=96, seed=96, batch_norm="running"),
    "full_18_batch": dict(FULL, n_layer=18, n=2, h=256, w=256, seed=113, batch_norm="batch"),     # last map 2 x 2: 8 values per channel
    # three and five frames on tiny maps (5 x 9 behind the pool, then 3 x 5, 2 x 3, 1 x 2 and the decoder's 1 x 1): a tile or a K chunk
    # of the deepest levels holds three or more frames, and frames straddle tiles.  The first seeds from 114 on with (a) and (b).
    "narrow_18_n3_running": dict(NARROW, n_layer=18, n=3, h=20, w=36, seed=114, batch_norm="running"),
    "narrow_18_n5_running": dict(NARROW, n_layer=18, n=5, h=21, w=43, seed=115, batch_norm="running"),
    "narrow_18_n3_batch": dict(NARROW, n_layer=18, n=3, h=33, w=260, seed=114, batch_norm="batch"),   # last map 1 x 3: 9 values per channel
})


def inputs(c):
    """(image0, image1, encoder state dict, decoder state dict, cotangent N x 4 x 4 fp64), CPU."""
    sd_enc, sd_dec = kb.synthetic.make_resnet_pose_weights(c["n_layer"], c["filters"], c["decoder_filters"], seed=c["seed"])
    image0, image1 = kb.synthetic.make_image_pair(c["n"], c["h"], c["w"], seed=c["seed"] + 100)
    cot = torch.from_numpy(np.random.default_rng(c["seed"] + 200).standard_normal((c["n"], 4, 4)))
    return image0, image1, sd_enc, sd_dec, cot


checksums = pcases.checksums


def last_map_values(c):
    """Values per channel the last BatchNorm2d sees: conv1, the pool, three stride-2 stages and the decoder's hidden layers halve."""
    h, w = c["h"], c["w"]
    for _ in range(5 + len(c["decoder_filters"])):
        h, w = (h + 1) // 2, (w + 1) // 2
    return c["n"] * h * w


def unused_projections(c):
    """The projection weights no forward touches: every block whose skip is the identity."""
    out, cin = [], c["filters"][0]
    for stage, (count, f) in enumerate(zip(kb.posenet_resnet.RESNET_BLOCKS[c["n_layer"]], c["filters"][1:]), 2):
        for b in range(count):
            if not ((stage > 2 and b == 0) or cin != f):
                out.append(f"enc::blocks{stage}.{b}.projection.conv.weight")
            cin = f
    return out


def fp32_branches(c):
    """The branches an fp32 run takes, as the GPU tests read them from the device: (masks, pool indices) from the oracle's own
    fp32 forward.  Used on the CPU to measure TOL with the same masks on both sides."""
    image0, image1, enc, dec, _ = inputs(c)
    with torch.no_grad():
        out = rgo.forward(image0, image1, enc, dec, n_layer=c["n_layer"], batch_norm=c["batch_norm"])
    return {k: z > 0 for k, z in out["pre"].items()}, out["pool_indices"]


# ---- operator cases (tests/test_resnet_pose_backward_gpu.py) ----
CONV_KS = [(3, 1), (1, 1), (1, 2)]      # (kernel size, stride) of the gradients csrc/conv_affine_backward.hip adds
# (frames, channels, height, width, filters): every one runs at every (k, stride) of CONV_KS
CONV_SHAPES = [
    (1, 1, 1, 1, 3),
    (1, 2, 2, 3, 5),
    (2, 5, 9, 13, 19),          # stride 2: the last row and column are even, they hold an output pixel
    (3, 7, 17, 23, 70),         # 1173 pixels at stride 1: tiles span rows and frames; two filter tiles
    (2, 70, 8, 10, 10),         # two input-channel tiles for the data gradient; stride 2: the last row and column are odd, all zeros
]
# (frames, channels, height, width, filters) at (3, 1): the weight gradient's K split at its two ends
WGRAD_SPLIT_SHAPES = [
    (4, 3, 33, 65, 8),          # 8580 pixels, no multiple of 32, under a small M x N
    (2, 40, 3, 2, 72),          # 12 pixels: less than one chunk, under a wide M x N
]
POOL_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (2, 5, 8, 10), (1, 2, 17, 130)]


def conv_case(n, cin, h, w, oc, k, stride, seed=0):
    """(input, weight, grad_out) fp64 CPU with values exactly representable in fp32, and the fp64 gradients torch.autograd gives:
    (grad_input, grad_weight)."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * n + 13 * h + w + 7 * k + stride)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
    weight = (torch.randn(oc, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5).float().double().requires_grad_(True)
    out = torch.nn.functional.conv2d(x, weight, None, stride=stride, padding=k // 2)
    grad_out = torch.randn(out.shape, generator=g, dtype=torch.float64).float().double()
    gx, gw = torch.autograd.grad(out, [x, weight], grad_out)
    return x.detach(), weight.detach(), grad_out, gx, gw
