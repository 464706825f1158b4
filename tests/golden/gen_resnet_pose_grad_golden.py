#!/usr/bin/env python3
"""Generate the golden vectors of the ResNet-18 pose network's BACKWARD pass by RUNNING THE REFERENCE on CPU under torch.autograd.

Needs a checkout of the reference (read-only); give the path of its `src` directory:

    python tests/golden/gen_resnet_pose_grad_golden.py <reference>/src

It imports the reference's `networks`, builds ResNetEncoder(n_layer=18, use_batch_norm=True) and PoseDecoder(n_filters=...,
use_batch_norm=True) the way its PoseNetModel does for encoder_type 'resnet18' (src/posenet_model.py:55-87) with n_filters =
[8, 12, 16, 16, 32] and decoder filters [16, 16], loads synthetic.make_resnet_pose_weights into them, casts them and the images to
fp64, and differentiates L = sum(pose * cotangent) for a seeded N x 4 x 4 cotangent.  Written next to this script as
`resnet_pose_grad_18_*.npz`: the fp64 gradient of every parameter the forward used (`enc::*`, `dec::*`; the projection of a block with
the identity skip has no gradient and is ABSENT), `dof`, `pose`, the cotangent, the running statistics after the forward (`run::*`)
-- and, instead of the images and the weights, the seeds that regenerate them with a checksum of each (`sum::*`).  Nothing of the
reference's source is stored: the fixtures are data.

  resnet_pose_grad_18_eval    2 x 3 x 61 x 77     .eval(): running statistics
  resnet_pose_grad_18_train   2 x 3 x 130 x 136   .train(): batch statistics, running statistics updated.  Maps 65x68, 33x34, 33x34,
                                                  17x17, 9x9, 5x5, decoder 3x3, 2x2: the last BatchNorm2d sees 8 values per channel

Asserted here: the oracle (tests/resnet_pose_grad_oracle.py) agrees with the reference to 1e-9 of each tensor's largest element, every
batch variance exceeds 1e-4 (train), dof lies in (1e-3, 3), each file stays under 1 MiB.  A seed that fails one is replaced, the
assertion stays.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "networks.py")):
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])

import kbnet_amd as kb  # noqa: E402,F401
import resnet_pose_grad_oracle as rgo  # noqa: E402
import resnet_pose_grad_cases as cases  # noqa: E402
import networks  # noqa: E402  (reference)


def reference_gradients(c, image0, image1, sd_enc, sd_dec, cotangent, train):
    encoder = networks.ResNetEncoder(n_layer=c["n_layer"], input_channels=6, n_filters=c["filters"], weight_initializer="xavier_normal",
                                     activation_func="leaky_relu", use_batch_norm=True)
    decoder = networks.PoseDecoder(rotation_parameterization="axis", input_channels=c["filters"][-1], n_filters=c["decoder_filters"],
                                   weight_initializer="xavier_normal", activation_func="leaky_relu", use_batch_norm=True)
    encoder.load_state_dict(sd_enc, strict=True)
    decoder.load_state_dict(sd_dec, strict=True)
    encoder, decoder = encoder.double(), decoder.double()
    encoder.train(train)
    decoder.train(train)
    seen, variances = {}, []
    hooks = [decoder.conv[len(c["decoder_filters"])].register_forward_hook(lambda m, a, out: seen.__setitem__("map", out.detach()))]
    for mod in list(encoder.modules()) + list(decoder.modules()):
        if isinstance(mod, torch.nn.BatchNorm2d):
            hooks.append(mod.register_forward_hook(
                lambda m, a, out: variances.append((tuple(a[0].shape), float(a[0].detach().var(dim=(0, 2, 3), unbiased=False).min())))))
    torch.set_default_dtype(torch.float64)      # pose_matrix builds its constant rows in the default dtype
    try:
        latent, _ = encoder(torch.cat([image0.double(), image1.double()], dim=1))   # src/posenet_model.py:109-110
        pose = decoder(latent)
        (pose * cotangent).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
    for h in hooks:
        h.remove()
    out = {"pose": pose.detach(), "dof": 0.01 * torch.mean(seen["map"], [2, 3])}   # src/networks.py:2069-2070
    for grp, mod in (("enc", encoder), ("dec", decoder)):
        for k, p in mod.named_parameters():
            if p.grad is not None:
                out[f"{grp}::{k}"] = p.grad
        for k, v in mod.state_dict().items():
            if "running" in k or "num_batches" in k:
                out[f"run::{grp}::{k}"] = v.detach().clone()
    return out, variances


def case(name):
    c = cases.GOLDEN[name]
    image0, image1, sd_enc, sd_dec, cotangent = cases.inputs(c)
    train = c["batch_norm"] == "batch"
    ref, variances = reference_gradients(c, image0, image1, sd_enc, sd_dec, cotangent, train)
    assert 1e-3 < float(ref["dof"].abs().max()) < 3.0, (name, ref["dof"])
    if train:
        assert variances[-1][0][2:] == (2, 2) and cases.last_map_values(c) == 8, variances[-1]
        for shape, v in variances:
            assert v > 1e-4, (name, shape, v)
    absent = [k for k in cases.unused_projections(c)]
    assert absent and not any(k in ref for k in absent), absent
    flat = {k: v.numpy() for k, v in ref.items()}
    flat["cotangent"] = cotangent.numpy()
    flat.update({"sum::" + k: np.float64(v) for k, v in cases.checksums(image0, image1, sd_enc, sd_dec).items()})
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **flat)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    o64 = rgo.gradients(image0, image1, sd_enc, sd_dec, cotangent, n_layer=c["n_layer"], batch_norm=c["batch_norm"])
    keys = [k for k in ref if "::" in k and "num_batches" not in k] + ["dof", "pose"]
    assert sorted(rgo.gradient_keys(o64)) == sorted(k for k in ref if k.startswith(("enc::", "dec::")))
    worst_o = max(float((o64[k] - ref[k]).abs().max() / ref[k].abs().max()) for k in keys)
    shapes = " ".join("x".join(str(s) for s in shape[2:]) for shape, _ in variances)
    print(f"{name}: {size / 1024:.0f} KiB  {len(keys)} tensors  BatchNorm maps {shapes}  dof {ref['dof'][0].tolist()}  oracle fp64 within "
          f"{worst_o:.1e} of the reference")
    assert worst_o < 1e-9, worst_o


def main():
    for name in cases.GOLDEN:
        case(name)


if __name__ == "__main__":
    main()
