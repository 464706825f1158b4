#!/usr/bin/env python3
"""One SHA-256 per case over the output bytes of the pose networks' three implicit-GEMM convs (csrc/pose_igemm.h:
conv2d_s2_affine, conv2d_affine, conv2d_s2_backward_data) and of one golden forward of each pose network.  Two builds of the
library compute the same bits exactly when their outputs are equal line for line:

    python tools/pose_conv_digest.py > new.txt
    KBN_LIB_PATH=/path/to/other/libkbnet_hip.so python tools/pose_conv_digest.py > other.txt      (a fresh process per library)
    python tools/pose_conv_digest.py --write tests/golden/pose_conv_digests.json                  (what tests/test_pose_conv_digest_gpu.py pins)

`--grad` selects a second case list, the conv GRADIENTS (what tests/test_conv_grad_digest_gpu.py pins): the two weight-gradient
entry points at every (kernel size, stride), filter tile and split; conv2d_backward_data; the recorded conv nodes (output and
every .grad); and one backward through each trainable model from a gradient golden's regenerated inputs and cotangent, hashing
every parameter's .grad in state_dict order:

    python tools/pose_conv_digest.py --grad --write tests/golden/conv_grad_digests.json

Inputs and weights are a closed-form integer hash of the element index (int64 arithmetic, no random generator), scaled into
(-1, 1).  Every operator case runs n = 3 frames of 13 x 21: odd in both axes, stride-2 maps of 7 x 11, so M = 231 is two
workgroup tiles, the second partial, both spanning frames; for a weight gradient that is 8 chunks of 32 output pixels, the last
partial, and 26 chunks (M = 819) at stride 1: enough for the split plan to choose more than one split.  Reads nothing outside the
repository.
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
sys.path.insert(1, os.path.join(ROOT, "tests"))      # the gradient goldens' case tables (inputs regenerated from seeds)
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


# ---- gradients -----------------------------------------------------------------------------------------------------------
GRAD_PAIRS = [([5], 9), ([12, 9], 20), ([72], 40)]      # filter tiles of 16, 32 and 64; a second source off a 16 boundary
S2_KS = [(3, 2), (5, 2), (7, 2)]                        # conv2d_s2_backward_*
PLAIN_KS = [(3, 1), (1, 1), (1, 2)]                     # conv2d_backward_*


def _maps(stride):
    return -(-H // stride), -(-W // stride)


def bwd_weight_case(k, stride, channels, filters, splits):
    def run(dev):
        salt = 300000 + 1000 * k + 100 * stride + 10 * filters + len(channels)
        inputs = _inputs(dev, channels, H, W, salt)
        grad_out = hashed((N, filters, *_maps(stride)), salt + 4, dev)
        if (k, stride) in S2_KS:
            return [kb.ops.conv2d_s2_backward_weight(inputs, grad_out, k, splits=splits)]
        return [kb.ops.conv2d_backward_weight(inputs, grad_out, k, stride, splits=splits)]
    return run


def plain_bwd_data_case(k, stride, cin, filters):
    def run(dev):
        salt = 400000 + 1000 * k + 100 * stride + 10 * filters
        weight = hashed((filters, cin, k, k), salt, dev)
        grad_out = hashed((N, filters, *_maps(stride)), salt + 4, dev)
        return [kb.ops.conv2d_backward_data(grad_out, kb.ops.pack_conv2d_backward_data_weight(weight, stride), cin, k, stride, H, W)]
    return run


def node_case(call, k, stride, channels, filters, data=()):
    """A recorded conv: `call(inputs, weight)` -> y; y.backward(a hashed cotangent).  The inputs listed in `data` do not require
    grad.  -> y, the weight's .grad and every other input's."""
    def run(dev):
        salt = 500000 + 1000 * k + 100 * stride + 10 * filters + len(channels)
        weight = hashed((filters, sum(channels), k, k), salt, dev).requires_grad_(True)
        inputs = [t.requires_grad_(i not in data) for i, t in enumerate(_inputs(dev, channels, H, W, salt))]
        y = call(inputs, weight)
        y.backward(hashed(tuple(y.shape), salt + 4, dev))
        return [y, weight.grad] + [t.grad for t in inputs if t.requires_grad]
    return run


def kb_xyz_case(channels):
    def run(dev):
        salt = 600000 + channels
        depth = hashed((N, channels, H, W), salt + 10, dev).requires_grad_(True)
        weight = hashed((1, channels, 1, 1), salt, dev).requires_grad_(True)
        xyz, z = kb.ops.kb_xyz(depth, weight, hashed((N, 3, H, W), salt + 3, dev))
        xyz.backward(hashed((N, 3, H, W), salt + 4, dev))
        return [xyz, z, depth.grad, weight.grad]
    return run


def _parameter_grads(modules):
    """Every parameter's .grad in state_dict order; a parameter no forward touched contributes one zero in its place."""
    return [p.grad if p.grad is not None else torch.zeros(1, device=p.device) for mod in modules for _, p in mod.named_parameters()]


def _pose_model_backward(table, name, make):
    def run(dev):
        c = __import__(table).GOLDEN[name]
        image0, image1, enc, dec, cot = __import__(table).inputs(c)
        m = make(dev, c)
        m.load_state_dicts(enc, dec)
        m.requires_grad_(True).set_batch_norm(c["batch_norm"])
        pose = m.forward(image0.to(dev), image1.to(dev))
        (pose * cot.float().to(dev)).sum().backward()
        return [pose] + _parameter_grads((m.encoder, m.decoder))
    return run


def _kbnet_model_backward(name):
    def run(dev):
        import kbnet_grad_cases as cases
        c = cases.GOLDEN[name]
        args = cases.inputs(c)
        m = kb.modules.KBNetModel.from_config(c["cfg"], dev, trainable=True)
        m.load_state_dicts(*args[4:7])
        depth = m.forward(*[t.to(dev) for t in args[:4]])
        (depth * args[7].float().to(dev)).sum().backward()
        return [depth] + _parameter_grads(m.modules())
    return run


def grad_cases():
    """[(name, run)] like cases(), for the conv gradients."""
    ops = kb.ops
    out = []
    for fn, ks in (("conv2d_s2_backward_weight", S2_KS), ("conv2d_backward_weight", PLAIN_KS)):
        for k, stride in ks:
            for channels, filters in GRAD_PAIRS:
                for splits in (None, 1, 3):
                    out.append((f"{fn} k{k} s{stride} c{channels} f{filters} splits {splits}", bwd_weight_case(k, stride, channels, filters, splits)))
    for k, stride in PLAIN_KS:
        for cin, filters in [(5, 9), (21, 20), (72, 10)]:
            out.append((f"conv2d_backward_data k{k} s{stride} c{cin} f{filters}", plain_bwd_data_case(k, stride, cin, filters)))
    out.append(("conv2d_s2 k5 c[12, 9] f20", node_case(lambda xs, w: ops.conv2d_s2(xs, w), 5, 2, [12, 9], 20)))
    for k, stride, channels in ((3, 1, [21]), (1, 2, [21]), (7, 2, [12, 9])):
        out.append((f"conv2d_pose k{k} s{stride} c{channels} f20", node_case(lambda xs, w, s=stride: ops.conv2d_pose(xs, w, s), k, stride, channels, 20)))
    for k, stride in ((3, 1), (3, 2), (1, 1), (1, 2)):
        for slope in (0.2, None):
            out.append((f"conv2d_kbnet k{k} s{stride} c[12, 3, 9] f20 slope {slope}, the middle input data",
                        node_case(lambda xs, w, s=stride, a=slope: ops.conv2d_kbnet(xs, w, s, negative_slope=a), k, stride, [12, 3, 9], 20, data=(1,))))
    out.append(("kb_xyz c9", kb_xyz_case(9)))
    posenet = lambda dev, c: kb.modules.PoseNetModel(device=dev, n_filters=c["filters"])
    resnet = lambda dev, c: kb.posenet_resnet.ResNetPoseNetModel(n_layer=c["n_layer"], device=dev, n_filters=c["filters"],
                                                                 decoder_filters=c["decoder_filters"], trainable=True)
    for name in ("posenet_grad_eval", "posenet_grad_train"):
        out.append((f"PoseNetModel {name} pose and parameter gradients", _pose_model_backward("posenet_grad_cases", name, posenet)))
    out.append(("ResNetPoseNetModel(18) resnet_pose_grad_18_train pose and parameter gradients",
                _pose_model_backward("resnet_pose_grad_cases", "resnet_pose_grad_18_train", resnet)))
    out.append(("KBNetModel kbnet_grad_kitti_odd depth and parameter gradients", _kbnet_model_backward("kbnet_grad_kitti_odd")))
    return out


def digest(run, dev):
    h = hashlib.sha256()
    for t in run(dev):
        assert t.dtype == torch.float32
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def digests(dev, grad=False):
    return {name: digest(run, dev) for name, run in (grad_cases() if grad else cases())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grad", action="store_true", help="the gradient case list instead of the forward one")
    ap.add_argument("--write", metavar="FILE", help="also write the digests to FILE as JSON")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pose_conv_digest: needs a GPU")
    kb._lib.load()
    got = digests(torch.device("cuda:0"), grad=args.grad)
    for name, d in got.items():
        print(f"{d}  {name}")
    if args.write:
        with open(args.write, "w") as f:
            json.dump(got, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
