#!/usr/bin/env python
"""Generate tests/golden/transforms.npz by RUNNING THE REFERENCE's Transforms (src/transforms.py) on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/gen_transforms_golden.py

Nothing of the reference's source is stored: the fixture is data.  Inputs: N = 6, one image tensor 6 x 3 x 8 x 12 with whole
values in 0 .. 255, one sparse depth map 6 x 1 x 8 x 12 with about 40 positive points a frame, its validity map.  A run is a
(np.random.seed, torch.manual_seed, options, probability); recorded per run: the reference's three outputs, and the
torch.rand(N) and densities the reference drew under that torch seed (its first torch draw).  The reference writes into its
arguments, so every run gets clones."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference/src")
import transforms as ref_transforms  # noqa: E402  (reference)

# the NumPy seeds of the p = 0.5 runs were chosen for decisions that differ between frames (frames left alone among them)
RUNS = [
    dict(name="flips", np_seed=1, torch_seed=11, p=1.0, range=[0, 1], flip=["horizontal", "vertical"], remove=[-1, -1], noise="none", spread=-1),
    dict(name="remove", np_seed=2, torch_seed=12, p=1.0, range=[-1, 1], flip=["none"], remove=[0.6, 0.7], noise="none", spread=-1),
    dict(name="uniform", np_seed=3, torch_seed=13, p=1.0, range=[0, 1], flip=["horizontal"], remove=[-1, -1], noise="uniform", spread=0.5),
    dict(name="all", np_seed=15, torch_seed=14, p=0.5, range=[0, 255], flip=["horizontal", "vertical"], remove=[0.3, 0.6], noise="gaussian", spread=0.1),
    dict(name="all2", np_seed=21, torch_seed=15, p=0.5, range=[0, 1], flip=["horizontal", "vertical"], remove=[0.6, 0.7], noise="uniform", spread=0.25),
]


def inputs():
    rng = np.random.default_rng(2021)
    image = rng.integers(0, 256, size=(6, 3, 8, 12)).astype(np.float32)
    depth = np.round(rng.uniform(1.0, 80.0, size=(6, 1, 8, 12)) * 256.0) / 256.0
    depth = np.where(rng.random(depth.shape) < 0.42, depth, 0.0).astype(np.float32)
    return image, depth, (depth > 0).astype(np.float32)


def main():
    image, depth, validity = inputs()
    out = {"image": image, "depth": depth, "validity": validity, "runs": np.frombuffer(json.dumps(RUNS).encode(), dtype=np.uint8)}
    for run in RUNS:
        t = ref_transforms.Transforms(normalized_image_range=run["range"], random_flip_type=run["flip"], random_remove_points=run["remove"],
                                      random_noise_type=run["noise"], random_noise_spread=run["spread"])
        torch.manual_seed(run["torch_seed"])
        values = torch.rand(6)
        lo, hi = run["remove"]
        densities = (hi - lo) * values + lo
        np.random.seed(run["np_seed"])
        torch.manual_seed(run["torch_seed"])
        [o_image], [o_depth], [o_validity] = t.transform(images_arr=[torch.from_numpy(image.copy())], range_maps_arr=[torch.from_numpy(depth.copy())],
                                                         validity_maps_arr=[torch.from_numpy(validity.copy())],
                                                         random_transform_probability=run["p"])
        name = run["name"]
        out[name + "::image"], out[name + "::depth"], out[name + "::validity"] = o_image.numpy(), o_depth.numpy(), o_validity.numpy()
        out[name + "::rand"], out[name + "::densities"] = values.numpy(), densities.numpy()
    path = os.path.join(HERE, "transforms.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; positives a frame:", (depth > 0).sum(axis=(1, 2, 3)))


if __name__ == "__main__":
    main()
