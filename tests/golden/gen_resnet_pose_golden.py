#!/usr/bin/env python3
"""Generate the golden vectors of the ResNet-18 / 34 pose networks' eval-mode forward by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/gen_resnet_pose_golden.py

It imports the reference's `networks` (read-only), builds ResNetEncoder(n_layer, use_batch_norm=True) and PoseDecoder(n_filters=...,
use_batch_norm=True) the way its PoseNetModel does for encoder_type 'resnet18' / 'resnet34' (src/posenet_model.py:55-87), loads
synthetic.make_resnet_pose_weights into them, puts them in .eval() and writes `resnet_pose_*.npz` next to this script: the state dicts
(`enc::*`, `dec::*`), the two images, and every layer's output (tests/resnet_pose_oracle.py `names`: conv1, the pool, every block, the
decoder's hidden layers), the 6-channel map, `dof` and the pose as the reference computes them in fp32 (`ref32::*`) and in fp64
(`ref64::*`: modules and inputs cast up).  Nothing of the reference's source is stored: the fixtures are data.

The full-width weights are 11 and 22 MB, too big for a fixture: the goldens use n_filters = [4, 8, 16, 24, 40] with decoder filters
[24, 40] for ResNet-18 and [4, 8, 8, 12, 20] with [12, 20] for ResNet-34 (arguments the reference's classes take; the widths that
keep each file under 1 MiB), which also puts filter counts that are no multiple of 16 in front of the kernels.

  resnet_pose_18_odd    ResNet-18, 2 x 6 x 61 x 77    maps 31x39, pool 16x20, 8x10, 4x5, 2x3, decoder 1x2, 1x1: odd sizes under the
                                                      1 x 1 stride-2 projections, 3 x 3 convs that see part of their window only
  resnet_pose_34_wide   ResNet-34, 1 x 6 x 40 x 136   maps 20x68, pool 10x34, 5x17, 3x9, 2x5, decoder 1x3, 1x2

The gate of the tests is |a - b| <= 1e-4 |b| + floor (tests/posenet_oracle.py); asserted here: the reference's own fp32 result
stays below a third of it from its fp64 result, for every stored tensor, and its key lists equal the synthetic ones.
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
import resnet_pose_oracle as ro  # noqa: E402  (tests/: the layer names only)
import networks  # noqa: E402  (reference)

torch.set_grad_enabled(False)
FILTERS = {18: [4, 8, 16, 24, 40], 34: [4, 8, 8, 12, 20]}      # + the decoder's hidden layers
DECODER_FILTERS = {18: [24, 40], 34: [12, 20]}


def reference_forward(n_layer, image0, image1, sd_enc, sd_dec, double):
    encoder = networks.ResNetEncoder(n_layer=n_layer, input_channels=6, n_filters=FILTERS[n_layer], weight_initializer="xavier_normal",
                                     activation_func="leaky_relu", use_batch_norm=True)
    decoder = networks.PoseDecoder(rotation_parameterization="axis", input_channels=FILTERS[n_layer][-1], n_filters=DECODER_FILTERS[n_layer],
                                   weight_initializer="xavier_normal", activation_func="leaky_relu", use_batch_norm=True)
    encoder.load_state_dict(sd_enc, strict=True)
    decoder.load_state_dict(sd_dec, strict=True)
    if double:
        encoder, decoder = encoder.double(), decoder.double()
        image0, image1 = image0.double(), image1.double()
    encoder.eval()
    decoder.eval()
    seen = {}

    def keep(name):
        return lambda m, a, out: seen.__setitem__(name, out.clone())

    hooks = [encoder.conv1.register_forward_hook(keep("conv1")), encoder.max_pool.register_forward_hook(keep("pool"))]
    for stage in range(2, 6):
        for b, block in enumerate(getattr(encoder, f"blocks{stage}")):
            hooks.append(block.register_forward_hook(keep(f"blocks{stage}.{b}")))
    for i in range(len(DECODER_FILTERS[n_layer])):
        hooks.append(decoder.conv[i].register_forward_hook(keep(f"decoder{i}")))
    hooks.append(decoder.conv[len(DECODER_FILTERS[n_layer])].register_forward_hook(keep("map")))
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


def case(name, n_layer, n, h, w, seed):
    sd_enc, sd_dec = kb.synthetic.make_resnet_pose_weights(n_layer, FILTERS[n_layer], DECODER_FILTERS[n_layer], seed=seed)
    image0, image1 = kb.synthetic.make_image_pair(n, h, w, seed=seed + 100)
    r32, keys_enc, keys_dec = reference_forward(n_layer, image0, image1, sd_enc, sd_dec, False)
    r64, _, _ = reference_forward(n_layer, image0, image1, sd_enc, sd_dec, True)
    layer_names = ro.names(n_layer, len(DECODER_FILTERS[n_layer]))
    assert sorted(r32) == sorted(layer_names + ["map", "dof", "pose"]), sorted(r32)
    assert 1e-3 < float(r64["dof"].abs().max()) < 3.0, (name, r64["dof"])      # a pose of sensible size: sin / cos stay well conditioned
    assert keys_enc == list(sd_enc.keys()) and keys_dec == list(sd_dec.keys())
    flat = {"image0": image0.numpy(), "image1": image1.numpy(), "n_layer": np.int64(n_layer)}
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
    sizes = [max(float(r64[k].abs().max()) for k in layer_names), min(po.rms(r64[k]) for k in layer_names)]
    assert sizes[0] < 1e3 and sizes[1] > 1e-2, (name, sizes)                    # no layer explodes or dies along 17 / 33 convs
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **flat)
    size = os.path.getsize(path)
    assert size < 1 << 20, (name, size)
    shapes = " ".join("x".join(str(s) for s in r32[k].shape[2:]) for k in layer_names)
    print(f"{name}: {size / 1024:.0f} KiB  maps {shapes}  dof {r64['dof'][0].tolist()}  activations: largest {sizes[0]:.3g}, "
          f"smallest layer RMS {sizes[1]:.3g}  fp32 reference at most {max(worst.values()):.2e} of the gate ({max(worst, key=worst.get)})")


def main():
    case("resnet_pose_18_odd", 18, 2, 61, 77, 72)
    case("resnet_pose_34_wide", 34, 1, 40, 136, 73)


if __name__ == "__main__":
    main()
