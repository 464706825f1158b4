#!/usr/bin/env python3
"""One SHA-256 per case over the output bytes of the pose networks' three implicit-GEMM convs (csrc/pose_igemm.h:
conv2d_s2_affine, conv2d_affine, conv2d_s2_backward_data) and of one golden forward of each pose network.  Two builds of the
library compute the same bits exactly when their outputs are equal line for line:

    python tools/pose_conv_digest.py > new.txt
    KBN_LIB_PATH=/path/to/other/libkbnet_hip.so python tools/pose_conv_digest.py > other.txt      (a fresh process per library)
    python tools/pose_conv_digest.py --write tests/golden/pose_conv_digests.json                  (what tests/test_pose_conv_digest_gpu.py pins)

Inputs and weights are a closed-form integer hash of the element index (int64 arithmetic, no random generator), scaled into
(-1, 1).  Every operator case runs n = 3 frames of 13 x 21: odd in both axes, stride-2 maps of 7 x 11, so M = 231 is two
workgroup tiles, the second partial, both spanning frames.  Reads nothing outside the repository.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kbnet_amd as kb  # noqa: E402

N, H, W = 3, 13, 21
SENTINEL = -7.25e30
POSENET_ODD_FILTERS = [8, 16, 16, 32, 32, 24, 40]      # the widths of tests/golden/posenet_odd.npz


def hashed(shape, salt, dev):
    """fp32 tensor of `shape`, element i = an odd multiple of 2^-24 in (-1, 1) from a 32-bit mix of i and `salt`."""
    numel = int(np.prod(shape))
    x = (torch.arange(numel, dtype=torch.int64) + salt * 0x9E3779B1) & 0xFFFFFFFF
    for _ in range(2):
        x = ((x ^ (x >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
    x = (x ^ (x >> 16)) & 0xFFFFFF
    return ((2 * x + 1 - (1 << 24)).double() / (1 << 24)).float().reshape(shape).to(dev)


def _affine(dev, filters, salt):
    return 1.0 + 0.5 * hashed((filters,), salt + 1, dev), hashed((filters,), salt + 2, dev)


def _inputs(dev, channels, h, w, salt):
    return [hashed((N, c, h, w), salt + 10 + i, dev) for i, c in enumerate(channels)]


def _sliced(dev, channels, h, w):
    """A tensor with `channels` + 5 planes per frame, filled with a sentinel, and the slice [2 : 2 + channels] of it."""
    wide = torch.full((N, channels + 5, h, w), SENTINEL, device=dev)
    return wide, wide[:, 2:2 + channels]


def s2_affine_case(k, channels, filters, slope=0.2, sliced=False):
    def run(dev):
        salt = 1000 * k + 10 * filters + len(channels)
        weight = hashed((filters, sum(channels), k, k), salt, dev)
        scale, shift = _affine(dev, filters, salt)
        wide, out = _sliced(dev, filters, (H + 1) // 2, (W + 1) // 2) if sliced else (None, None)
        y = kb.ops.conv2d_s2_affine(_inputs(dev, channels, H, W, salt), kb.ops.pack_conv2d_s2_affine_weight(weight), scale, shift,
                                    filters, k, negative_slope=slope, out=out)
        return [wide if sliced else y]
    return run


def affine_case(k, stride, channels, filters, slope=0.2, residual=False):
    def run(dev):
        salt = 100000 + 1000 * k + 100 * stride + 10 * filters + len(channels)
        weight = hashed((filters, sum(channels), k, k), salt, dev)
        scale, shift = _affine(dev, filters, salt)
        res = hashed((N, filters, -(-H // stride), -(-W // stride)), salt + 3, dev) if residual else None
        return [kb.ops.conv2d_affine(_inputs(dev, channels, H, W, salt), kb.ops.pack_conv2d_affine_weight(weight), scale, shift,
                                     filters, k, stride=stride, negative_slope=slope, residual=res)]
    return run


def bwd_data_case(k, channels, filters, sliced=False):
    def run(dev):
        salt = 200000 + 1000 * k + 10 * filters + len(channels)
        weight = hashed((filters, sum(channels), k, k), salt, dev)
        grad_out = hashed((N, filters, (H + 1) // 2, (W + 1) // 2), salt + 4, dev)
        pairs = [_sliced(dev, c, H, W) for c in channels] if sliced else None
        grads = kb.ops.conv2d_s2_backward_data(grad_out, kb.ops.pack_conv2d_s2_backward_data_weight(weight), channels, k, H, W,
                                               out=[s for _, s in pairs] if sliced else None)
        return [wide for wide, _ in pairs] if sliced else grads
    return run


def _golden(name):
    out = {}
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as raw:
        for key in raw.files:
            v = raw[key]
            v = torch.from_numpy(v) if v.dtype.kind == "f" else v
            if "::" in key:
                group, sub = key.split("::", 1)
                out.setdefault(group, {})[sub] = v
            else:
                out[key] = v
    return out


def _model_forward(make):
    def run(dev):
        g = _golden(make.golden)
        enc = {k: torch.as_tensor(v) for k, v in g["enc"].items()}
        dec = {k: torch.as_tensor(v) for k, v in g["dec"].items()}
        m = make(dev, g, enc, dec)
        m.load_state_dicts(enc, dec)
        pose, dof, _ = m.forward(g["image0"].to(dev), g["image1"].to(dev), return_all=True)
        return [pose, dof]
    return run


def _posenet(dev, g, enc, dec):
    return kb.modules.PoseNetModel(device=dev, n_filters=POSENET_ODD_FILTERS)


def _resnet18(dev, g, enc, dec):
    filters = [enc["conv1.conv.weight"].shape[0]] + [enc[f"blocks{s}.0.conv1.conv.weight"].shape[0] for s in range(2, 6)]
    return kb.modules.ResNetPoseNetModel(int(g["n_layer"]), device=dev, n_filters=filters,
                                         decoder_filters=[dec["conv.0.conv.weight"].shape[0], dec["conv.1.conv.weight"].shape[0]])


_posenet.golden = "posenet_odd"
_resnet18.golden = "resnet_pose_18_odd"


def cases():
    """[(name, run)]: run(device) -> the tensors whose bytes the case's digest covers, in order."""
    out = []
    forward_pairs = [([5], 12), ([3, 4], 24), ([9], 72)]          # every NB; K never a multiple of 16; a second source off a 16 boundary
    for k in (3, 5, 7):
        for channels, filters in forward_pairs:
            out.append((f"conv2d_s2_affine k{k} c{channels} f{filters}", s2_affine_case(k, channels, filters)))
    out.append(("conv2d_s2_affine k3 c[3, 4] f24 no activation, into a channel slice", s2_affine_case(3, [3, 4], 24, slope=None, sliced=True)))
    for k in (1, 3, 7):
        for stride in (1, 2):
            for channels, filters in forward_pairs:
                for residual in ((False, True) if filters == 24 else (False,)):
                    out.append((f"conv2d_affine k{k} s{stride} c{channels} f{filters}" + (" residual" if residual else ""),
                                affine_case(k, stride, channels, filters, residual=residual)))
    out.append(("conv2d_affine k3 s1 c[3, 4] f24 no activation", affine_case(3, 1, [3, 4], 24, slope=None)))
    for k in (3, 5, 7):
        for channels, filters in [([5], 9), ([12, 9], 20), ([72], 10)]:
            out.append((f"conv2d_s2_backward_data k{k} c{channels} f{filters}", bwd_data_case(k, channels, filters)))
    out.append(("conv2d_s2_backward_data k3 c[12, 9] f20 into channel slices", bwd_data_case(3, [12, 9], 20, sliced=True)))
    out.append(("PoseNetModel posenet_odd pose dof", _model_forward(_posenet)))
    out.append(("ResNetPoseNetModel(18) resnet_pose_18_odd pose dof", _model_forward(_resnet18)))
    return out


def digest(run, dev):
    h = hashlib.sha256()
    for t in run(dev):
        assert t.dtype == torch.float32
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def digests(dev):
    return {name: digest(run, dev) for name, run in cases()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", metavar="FILE", help="also write the digests to FILE as JSON")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pose_conv_digest: needs a GPU")
    kb._lib.load()
    got = digests(torch.device("cuda:0"))
    for name, d in got.items():
        print(f"{d}  {name}")
    if args.write:
        with open(args.write, "w") as f:
            json.dump(got, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
