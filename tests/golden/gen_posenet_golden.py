#!/usr/bin/env python3
"""Generate the golden vectors of the pose network's eval-mode forward by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/gen_posenet_golden.py

It imports the reference's `networks` (read-only), builds PoseEncoder(use_batch_norm=True) and PoseDecoder the way its
PoseNetModel does (src/posenet_model.py:47-79), loads synthetic.make_posenet_weights into them, puts them in .eval() and
writes `posenet_*.npz` next to this script: the state dicts (`enc::*`, `dec::*`), the two images, and every layer's output, the
6-channel map, `dof` and the pose as the reference computes them in fp32 (`ref32::*`) and in fp64 (`ref64::*`: modules and inputs
cast up).  Nothing of the reference's source is stored: the fixtures are data.

The full-width weights are 6.3 MB, too big for a fixture: the goldens use n_filters = [8, 16, 16, 32, 32, 24, 40] (an argument
PoseEncoder takes), which also puts filter counts that are no multiple of 16 in front of the kernels.

  posenet_odd    2 x 6 x 61 x 77    maps 31x39, 16x20, 8x10, 4x5, 2x3, 1x2, 1x1: a 3 x 3 conv that sees only its centre tap
  posenet_wide   1 x 6 x 40 x 136   maps 20x68 ... 1x3, 1x2

The gate of the tests is |a - b| <= 1e-4 |b| + floor (tests/posenet_oracle.py); asserted here: the reference's own fp32 result
stays below a third of it from its fp64 result, for every stored tensor.
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
import posenet_oracle as po  # noqa: E402  (tests/: the gate's helpers only)
import networks  # noqa: E402  (reference)

torch.set_grad_enabled(False)
FILTERS = [8, 16, 16, 32, 32, 24, 40]


def reference_forward(image0, image1, sd_enc, sd_dec, double):
    encoder = networks.PoseEncoder(input_channels=6, n_filters=FILTERS, weight_initializer="xavier_normal",
                                   activation_func="leaky_relu", use_batch_norm=True)
    decoder = networks.PoseDecoder(rotation_parameterization="axis", weight_initializer="xavier_normal", input_channels=FILTERS[-1])
    encoder.load_state_dict(sd_enc, strict=True)
    decoder.load_state_dict(sd_dec, strict=True)
    if double:
        encoder, decoder = encoder.double(), decoder.double()
        image0, image1 = image0.double(), image1.double()
    encoder.eval()
    decoder.eval()
    seen = {}
    hooks = [getattr(encoder, f"conv{i}").register_forward_hook(lambda m, a, out, i=i: seen.__setitem__(f"layer{i}", out.clone()))
             for i in range(1, 8)]
    hooks.append(decoder.conv.register_forward_hook(lambda m, a, out: seen.__setitem__("map", out.clone())))
    if double:
        torch.set_default_dtype(torch.float64)      # pose_matrix builds its constant rows in the default dtype
    try:
        latent, _ = encoder(torch.cat([image0, image1], dim=1))         # src/posenet_model.py:109-110
        seen["pose"] = decoder(latent)
    finally:
        torch.set_default_dtype(torch.float32)
    for h in hooks:
        h.remove()
    seen["dof"] = 0.01 * torch.mean(seen["map"], [2, 3])                # src/networks.py:2069-2070
    return seen, list(encoder.state_dict().keys()), list(decoder.state_dict().keys())


def case(name, n, h, w, seed):
    sd_enc, sd_dec = kb.synthetic.make_posenet_weights(FILTERS, seed=seed)
    image0, image1 = kb.synthetic.make_image_pair(n, h, w, seed=seed + 100)
    r32, keys_enc, keys_dec = reference_forward(image0, image1, sd_enc, sd_dec, False)
    r64, _, _ = reference_forward(image0, image1, sd_enc, sd_dec, True)
    assert 1e-3 < float(r64["dof"].abs().max()) < 3.0, (name, r64["dof"])      # a pose of sensible size: sin / cos stay well conditioned
    assert keys_enc == list(sd_enc.keys()) and keys_dec == list(sd_dec.keys())
    flat = {"image0": image0.numpy(), "image1": image1.numpy()}
    for grp, sd in (("enc", sd_enc), ("dec", sd_dec)):
        for k, v in sd.items():
            flat[f"{grp}::{k}"] = v.numpy()
    for grp, d in (("ref32", r32), ("ref64", r64)):
        for k, v in d.items():
            flat[f"{grp}::{k}"] = v.numpy()
    worst = {}
    for k in r32:
        floor = po.dof_floor(r64["map"]) if k in ("dof", "pose") else po.layer_floor(r64[k])
        if k == "pose":
            worst[k] = po.gate_fraction(r32[k][:, :3, 3], r64[k][:, :3, 3], floor)
        else:
            worst[k] = po.gate_fraction(r32[k], r64[k], floor)
        assert worst[k] < 1.0 / 3.0, (name, k, worst[k])
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **flat)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    shapes = " ".join("x".join(str(s) for s in r32[f"layer{i}"].shape[2:]) for i in range(1, 8))
    print(f"{name}: {size / 1024:.0f} KiB  maps {shapes}  dof {r64['dof'][0].tolist()}  fp32 reference at "
          + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + " of the gate")


def main():
    case("posenet_odd", 2, 61, 77, 71)
    case("posenet_wide", 1, 40, 136, 72)


if __name__ == "__main__":
    main()
