#!/usr/bin/env python3
"""Generate the golden vectors of the pose network's BACKWARD pass by RUNNING THE REFERENCE on CPU under torch.autograd.

Run in the build container only (needs /root/reference):

    python tests/golden/gen_posenet_grad_golden.py

It imports the reference's `networks` (read-only), builds PoseEncoder(use_batch_norm=True) and PoseDecoder the way its
PoseNetModel does (src/posenet_model.py:47-79) with n_filters = [8, 16, 16, 32, 32, 24, 40], loads
synthetic.make_posenet_weights into them, casts them and the images to fp64, and differentiates L = sum(pose * cotangent) for a
seeded N x 4 x 4 cotangent.  Written next to this script as `posenet_grad_*.npz`: the fp64 gradient of every parameter
(`enc::*`, `dec::*`), `dof`, `pose`, the cotangent, the running statistics after the forward (`run::*`) -- and, instead of the
images and the weights, the seeds that regenerate them with a checksum of each (`sum::*`).  Nothing of the reference's source is
stored: the fixtures are data.

  posenet_grad_eval    2 x 3 x 61 x 77     .eval(): running statistics.  Maps 31x39 ... 1x2, 1x1: the 3 x 3 convs at their centre tap
  posenet_grad_train   2 x 3 x 130 x 136   .train(): batch statistics, running statistics updated.  Maps 65x68 ... 3x3, 2x2

Asserted here for the train case: the last map has at least 2 x 2 pixels (batch statistics over >= 8 values) and every layer's
batch variance is above 1e-4, so that rstd is well conditioned.
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
sys.path.insert(0, "/root/reference/src")

import kbnet_amd as kb  # noqa: E402
import posenet_grad_oracle as pgo  # noqa: E402  (tests/: the case table and the checksums only)
import posenet_grad_cases as cases  # noqa: E402
import networks  # noqa: E402  (reference)

FILTERS = pgo.FILTERS


def reference_gradients(image0, image1, sd_enc, sd_dec, cotangent, train):
    encoder = networks.PoseEncoder(input_channels=6, n_filters=FILTERS, weight_initializer="xavier_normal",
                                   activation_func="leaky_relu", use_batch_norm=True)
    decoder = networks.PoseDecoder(rotation_parameterization="axis", weight_initializer="xavier_normal", input_channels=FILTERS[-1])
    encoder.load_state_dict(sd_enc, strict=True)
    decoder.load_state_dict(sd_dec, strict=True)
    encoder, decoder = encoder.double(), decoder.double()
    encoder.train(train)
    decoder.train(train)
    seen = {}
    hooks = [getattr(encoder, f"conv{i}").conv.register_forward_hook(lambda m, a, out, i=i: seen.__setitem__(i, out.detach()))
             for i in range(1, 8)]
    hooks.append(decoder.conv.register_forward_hook(lambda m, a, out: seen.__setitem__("map", out.detach())))
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
            out[f"{grp}::{k}"] = p.grad
    for k, v in encoder.state_dict().items():
        if "running" in k or "num_batches" in k:
            out["run::" + k] = v.detach().clone()
    return out, [seen[i] for i in range(1, 8)]


def case(name):
    c = cases.GOLDEN[name]
    image0, image1, sd_enc, sd_dec, cotangent = cases.inputs(c)
    train = c["batch_norm"] == "batch"
    ref, convs = reference_gradients(image0, image1, sd_enc, sd_dec, cotangent, train)
    assert 1e-3 < float(ref["dof"].abs().max()) < 3.0, (name, ref["dof"])
    if train:
        assert convs[-1].shape[2] >= 2 and convs[-1].shape[3] >= 2, convs[-1].shape
        for i, u in enumerate(convs, 1):
            v = float(u.var(dim=(0, 2, 3), unbiased=False).min())
            assert v > 1e-4, (name, i, v)
    flat = {k: v.numpy() for k, v in ref.items()}
    flat["cotangent"] = cotangent.numpy()
    flat.update({"sum::" + k: np.float64(v) for k, v in cases.checksums(image0, image1, sd_enc, sd_dec).items()})
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **flat)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    # the oracle against the reference, and the oracle's fp32 autograd against its fp64 one (what the gate's TOL is 3 x of)
    o64 = pgo.gradients(image0, image1, sd_enc, sd_dec, cotangent, batch_norm=c["batch_norm"])
    o32 = pgo.gradients(image0, image1, sd_enc, sd_dec, cotangent, dtype=torch.float32, batch_norm=c["batch_norm"])
    keys = [k for k in ref if "::" in k and not k.startswith("run::")] + ["dof"]
    worst_o = max(float((o64[k] - ref[k]).abs().max() / ref[k].abs().max()) for k in keys)
    worst32 = max((pgo.fraction(o32[k], o64[k]), k) for k in keys)
    shapes = " ".join("x".join(str(s) for s in u.shape[2:]) for u in convs)
    print(f"{name}: {size / 1024:.0f} KiB  maps {shapes}  oracle fp64 within {worst_o:.1e} of the reference; its fp32 autograd at "
          f"{worst32[0]:.2e} ({worst32[1]}) of |b| + rms(b)")
    assert worst_o < 1e-9, worst_o


def main():
    for name in cases.GOLDEN:
        case(name)


if __name__ == "__main__":
    main()
