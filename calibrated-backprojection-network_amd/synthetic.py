"""Deterministic synthetic frames and weights.

Everything is drawn from `numpy.random.Generator(numpy.random.Philox(seed))`
so the build container and the GPU box regenerate identical tensors.
Frame statistics follow the reference's data conventions: images are /255
normalised (`src/transforms.py:201-204`), sparse depth is a multiple of 1/256 m
(16-bit PNG / 256, `src/data_utils.py:137-141`), validity = depth > 0
(`src/kbnet.py:899-902`).
"""

from __future__ import annotations

import zlib
from typing import Dict, Tuple

import numpy as np
import torch

from .config import (KBNetConfig, decoder_param_shapes, encoder_param_shapes,
                     s2d_param_shapes)

# name -> (density, depth range in metres, intrinsics fx, fy, cx, cy)
FRAME_STATS = {
    "kitti": (0.05, (1.0, 80.0), (721.5377, 721.5377, 609.5593, 172.854)),
    "void": (0.005, (0.3, 5.0), (514.6, 514.6, 320.0, 240.0)),
    # reference setup/setup_dataset_nyu_v2.py:329-349 (crop-adjusted principal point)
    "nyu_v2": (0.0063, (0.3, 5.0), (518.8579, 519.4696, 325.5824 - 32.0, 253.7362 - 32.0)),
}


# Gain of the synthetic xavier weights per preset, for every parity test at BASELINE's sizes, the parity-margin reports and the bench.
# Random weights have no trained scale: each conv multiplies the activations by ~gain, so the gain alone sets the magnitude of the
# logits -- and with it how far ANY fp32 evaluation order lands from the exact depth map (the head's sensitivity is
# sigma(1-sigma) / (sigma + d_min/d_max) <= 0.8 per unit of absolute logit error, and that error grows with the logits).
# tests/analysis/gain_study.py (CPU, oracle fp32 vs fp64, the worst seeds of the 32-seed reports):
#     KITTI  gain 1.30: logits std 6.4-11, max 52-85 (most pixels saturated), fp32 oracle up to 7.7e-5 from fp64  <- rounds 1-4
#            gain 1.10: logits std 1.0-1.9, max 8-18,  oracle <= 1.4e-5 from fp64                                 <- now
#     VOID   gain 1.45: std 1.6-3.9, max 9-29, oracle 2.7e-5;   gain 1.30: std 0.45-1.0, max 3-5, oracle 6.0e-6    <- now
#     NYUv2  gain 1.30: std 0.43-0.98, oracle 6.2e-6
# At these gains the sigmoid is exercised over its whole range (std ~ 1, no all-0.5 plateau: the tests assert std > 0.1) and the
# 1e-4 gate of north_star has a >= 2x margin that belongs to the KERNELS, not to the oracle's own rounding.
PARITY_GAIN = {"kitti": 1.1, "void": 1.3, "nyu_v2": 1.3}


def _rng(seed: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(seed))


def make_frames(n: int, height: int, width: int, kind: str = "kitti", seed: int = 1,
                jitter_intrinsics: float = 0.0):
    """Returns (image N3HW, sparse_depth N1HW, validity N1HW, intrinsics N33), CPU fp32."""
    density, (lo, hi), (fx, fy, cx, cy) = FRAME_STATS[kind]
    g = _rng(seed)
    image = g.random((n, 3, height, width), dtype=np.float32)
    mask = g.random((n, 1, height, width), dtype=np.float32) < density
    depth = lo + (hi - lo) * g.random((n, 1, height, width), dtype=np.float32)
    depth = np.round(depth * 256.0) / 256.0
    sparse = (depth * mask).astype(np.float32)
    validity = (sparse > 0).astype(np.float32)
    k = np.zeros((n, 3, 3), dtype=np.float32)
    scale = 1.0 + jitter_intrinsics * (2.0 * g.random((n, 4), dtype=np.float32) - 1.0)
    k[:, 0, 0] = fx * scale[:, 0]
    k[:, 1, 1] = fy * scale[:, 1]
    k[:, 0, 2] = cx * scale[:, 2]
    k[:, 1, 2] = cy * scale[:, 3]
    k[:, 2, 2] = 1.0
    return tuple(torch.from_numpy(a) for a in (image, sparse, validity, k))


def _xavier_normal(name: str, shape: Tuple[int, ...], seed: int) -> torch.Tensor:
    """N(0, 2/(fan_in+fan_out)) keyed by parameter name (order independent);
    the reference initialises every conv with `xavier_normal_`
    (`src/net_utils.py:98-99`)."""
    fan_in = shape[1] * shape[2] * shape[3]
    fan_out = shape[0] * shape[2] * shape[3]
    std = (2.0 / (fan_in + fan_out)) ** 0.5
    g = _rng((seed << 32) ^ zlib.crc32(name.encode()))
    return torch.from_numpy((std * g.standard_normal(shape)).astype(np.float32))


def _trained_like(name: str, shape: Tuple[int, ...], seed: int, spread_log2: float, dead_fraction: float) -> torch.Tensor:
    """A weight tensor with the statistics trained conv nets show and xavier noise does not: heavy-tailed entries
    (Student-t, 3 degrees of freedom), a per-filter scale drawn log-uniformly over 2^spread_log2 (a few filters dominate
    a layer's output range, most sit binades below it), and `dead_fraction` of the filters exactly zero (dead channels:
    all-zero activation planes downstream).  The layer keeps xavier's Frobenius norm, so the network's activations stay
    O(1) and the sigmoid head off saturation.  Single-filter layers (proj_depth, output0) keep their filter alive."""
    fan_in = shape[1] * shape[2] * shape[3]
    fan_out = shape[0] * shape[2] * shape[3]
    std = (2.0 / (fan_in + fan_out)) ** 0.5
    g = _rng((seed << 32) ^ zlib.crc32(("trained/" + name).encode()))
    w = g.standard_t(3.0, shape) / np.sqrt(3.0)
    f = shape[0]
    w *= np.exp2(spread_log2 * (g.random((f, 1, 1, 1)) - 0.5))
    if f > 1:
        dead = g.random(f) < dead_fraction
        dead[int(g.integers(f))] = False            # never all of them
        w[dead] = 0.0
    w *= std * np.sqrt(w.size) / max(float(np.sqrt((w * w).sum())), 1e-30)
    return torch.from_numpy(w.astype(np.float32))


def make_state_dicts(cfg: KBNetConfig, seed: int = 0, gain: float = 1.0, trained_like: bool = False,
                     spread_log2: float = 7.0, dead_fraction: float = 0.10):
    """Three dicts (S2D, encoder, decoder) keyed like the reference's state_dicts
    (without the DataParallel `module.` prefix).  `trained_like`: the stress statistics of `_trained_like` instead of
    xavier noise (the pretrained checkpoints of reference README.md:205-217 are external files; this is the stand-in
    that drives the fp16 windows of the split-operand kernels the way trained weights would)."""
    out = []
    for part, shapes in (("s2d", s2d_param_shapes(cfg)), ("enc", encoder_param_shapes(cfg)),
                         ("dec", decoder_param_shapes(cfg))):
        if trained_like:
            out.append({k: gain * _trained_like(part + "/" + k, s, seed, spread_log2, dead_fraction) for k, s in shapes.items()})
        else:
            out.append({k: gain * _xavier_normal(part + "/" + k, s, seed) for k, s in shapes.items()})
    return tuple(out)


def _box2(a: np.ndarray, radius: int) -> np.ndarray:
    """Two passes of a (2 radius + 1)^2 box mean over the last two axes, 'valid' (each pass trims `radius` per side), in fp64."""
    k = 2 * radius + 1
    for _ in range(2):
        for axis in (-2, -1):
            c = np.cumsum(np.insert(a, 0, 0.0, axis=axis), axis=axis)
            n = c.shape[axis]
            a = (np.take(c, range(k, n), axis=axis) - np.take(c, range(0, n - k), axis=axis)) / k
    return a


def _smooth_field(g: np.random.Generator, shape, height: int, width: int, radius: int) -> np.ndarray:
    """Band-limited noise, shape + (height, width), each map stretched to span [0, 1]."""
    a = _box2(g.random(tuple(shape) + (height + 4 * radius, width + 4 * radius)), radius) if radius > 0 else g.random(tuple(shape) + (height, width))
    lo, hi = a.min(axis=(-2, -1), keepdims=True), a.max(axis=(-2, -1), keepdims=True)
    return (a - lo) / np.maximum(hi - lo, 1e-12)


def make_triplet(n: int, height: int, width: int, kind: str = "kitti", seed: int = 1, radius: int = 4):
    """Inputs of KBNetModel.compute_loss: (image0, image1, image2 N3HW in [0, 1], output_depth N1HW, sparse_depth N1HW,
    validity N1HW, intrinsics N33, pose01, pose02 N6: axis-angle rotation first, translation last, as ops.pose_matrix reads them),
    CPU fp32.  The images are BAND-LIMITED (uniform noise box-filtered twice with `radius`, the three frames sharing 80 % of
    their content at small offsets): a warped pixel inherits the rounding of its sample position (about W 2^-23 pixels in fp32)
    times the local image gradient, and on independent pixels (make_frames) that alone puts two correct fp32 evaluations 2e-4
    apart.  The dense depth is smooth inside the preset's range (its nearer fifth, where a 0.5 m translation moves pixels);
    the sparse depth samples it at the preset's density (at least one point per frame) with 1 % noise, rounded to 1/256 m like the 16-bit PNGs.  The principal
    point and focal length follow the frame size (focal 0.6 x the longer side: a 40 degree half field of view)."""
    density, (lo, hi), _ = FRAME_STATS[kind]
    g = _rng(seed)
    off = 2
    scene = _smooth_field(g, (n, 3), height + 2 * off, width + 2 * off, radius)
    images = []
    for dy, dx in ((0, 0), (1, -2), (-1, 2)):
        own = _smooth_field(g, (n, 3), height, width, radius)
        images.append(0.8 * scene[..., off + dy:off + dy + height, off + dx:off + dx + width] + 0.2 * own)
    near, far = lo + 0.02 * (hi - lo), lo + 0.27 * (hi - lo)
    depth = near + (far - near) * _smooth_field(g, (n, 1), height, width, 2 * radius)
    mask = g.random((n, 1, height, width)) < density
    mask.reshape(n, -1)[np.arange(n), g.integers(height * width, size=n)] = True   # never a frame without a point (tiny frames)
    noisy = depth * (1.0 + 0.01 * g.standard_normal((n, 1, height, width)))
    sparse = np.round(noisy * 256.0) / 256.0 * mask
    validity = sparse > 0
    k = np.zeros((n, 3, 3))
    k[:, 0, 0] = k[:, 1, 1] = 0.6 * max(width, height)
    k[:, 0, 2] = 0.5 * (width - 1)
    k[:, 1, 2] = 0.5 * (height - 1)
    k[:, 2, 2] = 1.0
    step = 0.025 * (near + far)          # translation that moves a mid-range point by ~0.03 W pixels
    poses = []
    for sign in (1.0, -1.0):
        p = np.concatenate([0.02 * (2.0 * g.random((n, 3)) - 1.0), step * (2.0 * g.random((n, 3)) - 1.0)], axis=1)
        p[:, 5] = sign * np.abs(p[:, 5])   # one neighbour frame ahead, one behind
        poses.append(p)
    arrays = images + [depth, sparse, validity, k] + poses
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in arrays)


POSENET_KERNELS = (7, 5, 3, 3, 3, 3, 3)


def make_posenet_weights(filters=(16, 32, 64, 128, 256, 256, 256), seed: int = 0, gain: float = 0.5):
    """Two dicts (encoder, decoder) keyed like the state_dicts of the reference's PoseEncoder(use_batch_norm=True) /
    PoseDecoder(n_filters=[]) (src/networks.py:536-671, 1992-2075; no `module.` prefix).  Conv weights: xavier normal (x gain).
    BatchNorm2d: gamma uniform in [0.5, 1.5], beta and running mean 0.2 N(0, 1), running variance uniform in [0.25, 1.75] with
    TWO channels of every layer at 1e-3 -- there eps = 1e-5 is 1 % of the variance, so a forward that drops it is 0.5 % off in
    those channels, far outside any parity gate.  Those channels also amplify 30-fold, layer after layer; gain = 0.5 keeps
    the activations O(1) to O(100) and the pose vector between 1e-3 and a few radians / metres at both the full and a narrow width."""
    enc, dec = {}, {}
    cin = 6
    for i, (f, k) in enumerate(zip(filters, POSENET_KERNELS), 1):
        enc[f"conv{i}.conv.weight"] = gain * _xavier_normal(f"pose/conv{i}.conv.weight", (f, cin, k, k), seed)
        g = _rng((seed << 32) ^ zlib.crc32(f"pose/conv{i}.batch_norm".encode()))
        var = 0.25 + 1.5 * g.random(f)
        var[g.choice(f, size=min(2, f), replace=False)] = 1e-3
        enc[f"conv{i}.batch_norm.weight"] = torch.from_numpy((0.5 + g.random(f)).astype(np.float32))
        enc[f"conv{i}.batch_norm.bias"] = torch.from_numpy((0.2 * g.standard_normal(f)).astype(np.float32))
        enc[f"conv{i}.batch_norm.running_mean"] = torch.from_numpy((0.2 * g.standard_normal(f)).astype(np.float32))
        enc[f"conv{i}.batch_norm.running_var"] = torch.from_numpy(var.astype(np.float32))
        enc[f"conv{i}.batch_norm.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)
        cin = f
    dec["conv.conv.weight"] = gain * _xavier_normal("pose/conv.conv.weight", (6, cin, 1, 1), seed)
    return enc, dec


def make_image_pair(n: int, height: int, width: int, seed: int = 1, radius: int = 2):
    """(image0, image1) N x 3 x H x W in [0, 1], CPU fp32: band-limited noise, image1 sharing 80 % of image0's content two
    pixels to the side -- every frame its own images."""
    g = _rng(seed)
    scene = _smooth_field(g, (n, 3), height, width + 2, radius)
    own = _smooth_field(g, (n, 3), height, width, radius)
    image0 = scene[..., :, :width]
    image1 = 0.8 * scene[..., :, 2:] + 0.2 * own
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in (image0, image1))


from .posenet_resnet import RESNET_BLOCKS  # noqa: E402  (the block counts of ResNet-18 / 34: one copy in the package)


def make_resnet_pose_weights(n_layer: int = 18, filters=(16, 32, 64, 128, 256), decoder_filters=(256, 256), seed: int = 0,
                             gain: float = 0.35):
    """Two dicts (encoder, decoder) keyed like the state_dicts of the reference's ResNetEncoder(n_layer, use_batch_norm=True) /
    PoseDecoder(n_filters=decoder_filters, use_batch_norm=True) (src/networks.py:674-996, 1992-2075; no `module.` prefix), every
    block with its `projection.conv.weight`, used or not.  Conv weights: xavier normal (x gain).  BatchNorm2d as
    make_posenet_weights: gamma in [0.5, 1.5], beta and running mean 0.2 N(0, 1), running variance in [0.25, 1.75], with
    max(1, f // 32) channels of every f-channel layer at 1e-3 (eps = 1e-5 is 1 % of it: a forward that drops eps is 0.5 % off
    there).  Such a channel amplifies 30-fold and a block ADDS its input to its output, so the activations' size is exponential
    in the gain along 17 or 33 convs (gain 0.5 reaches 1e3 at 34 layers, 0.7 reaches 1e7): fewer such channels than the plain
    network's two per layer, the second conv of every block and the projections at half the gain, and gain = 0.35 keep the
    activations O(1) to O(100) and the pose vector between 1e-3 and a few radians / metres at both depths, full and narrow."""
    if n_layer not in RESNET_BLOCKS or len(filters) != 5:
        raise ValueError(f"make_resnet_pose_weights: n_layer 18 or 34 and five filter counts, got {n_layer}, {tuple(filters)}")
    enc, dec = {}, {}

    def conv_bn(sd, prefix, f, cin, k, scale=1.0):
        sd[f"{prefix}.conv.weight"] = scale * gain * _xavier_normal(f"resnet{n_layer}/{prefix}.conv.weight", (f, cin, k, k), seed)
        g = _rng((seed << 32) ^ zlib.crc32(f"resnet{n_layer}/{prefix}.batch_norm".encode()))
        var = 0.25 + 1.5 * g.random(f)
        var[g.choice(f, size=max(1, f // 32), replace=False)] = 1e-3
        sd[f"{prefix}.batch_norm.weight"] = torch.from_numpy((0.5 + g.random(f)).astype(np.float32))
        sd[f"{prefix}.batch_norm.bias"] = torch.from_numpy((0.2 * g.standard_normal(f)).astype(np.float32))
        sd[f"{prefix}.batch_norm.running_mean"] = torch.from_numpy((0.2 * g.standard_normal(f)).astype(np.float32))
        sd[f"{prefix}.batch_norm.running_var"] = torch.from_numpy(var.astype(np.float32))
        sd[f"{prefix}.batch_norm.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)

    conv_bn(enc, "conv1", filters[0], 6, 7)
    cin = filters[0]
    for stage, (count, f) in enumerate(zip(RESNET_BLOCKS[n_layer], filters[1:]), 2):
        for b in range(count):
            prefix = f"blocks{stage}.{b}"
            conv_bn(enc, prefix + ".conv1", f, cin, 3)
            conv_bn(enc, prefix + ".conv2", f, f, 3, scale=0.5)
            enc[prefix + ".projection.conv.weight"] = 0.5 * gain * _xavier_normal(f"resnet{n_layer}/{prefix}.projection.conv.weight",
                                                                                  (f, cin, 1, 1), seed)
            cin = f
    for i, f in enumerate(decoder_filters):
        conv_bn(dec, f"conv.{i}", f, cin, 3)
        cin = f
    dec[f"conv.{len(decoder_filters)}.conv.weight"] = gain * _xavier_normal(f"resnet{n_layer}/conv.{len(decoder_filters)}.conv.weight",
                                                                            (6, cin, 1, 1), seed)
    return enc, dec
