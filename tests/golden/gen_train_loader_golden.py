#!/usr/bin/env python
"""Generate tests/golden/train_io/* and tests/golden/train_loader.npz by RUNNING THE REFERENCE's KBNetTrainingDataset
(src/datasets.py:161-228) on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/gen_train_loader_golden.py

Nothing of the reference's source is stored: the fixtures are data.

train_io/: four samples written with PIL -- RGB triplets whose frames are 24 x 40, 26 x 44, 25 x 43 and 24 x 40 (odd widths, two
sizes that differ in both axes, two equal ones), 16-bit depth PNGs of the same sizes with about 40 % positive points, and four
distinct intrinsics k_i.npy (a sample is recognisable from its k alone).

train_loader.npz: a run is (crop type, shape, np.random.seed); the dataset is read at indices 0..3 in order, three passes without
reseeding.  Recorded per run: the adjusted intrinsics of all twelve draws, and the five outputs of the first pass (the images as
uint8 -- asserted whole -- and the depth as float32).  One more run has shape=None over the two 24 x 40 samples.

The seeds are fixed; the script asserts what makes them worth keeping: every 'vertical' run without 'bottom' has draws on both
sides of the 0.30 decision, every 'horizontal' run has at least two different x_start, and some x_start is odd."""
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
IO = os.path.join(HERE, "train_io")
sys.path.insert(0, "/root/reference/src")
import datasets as ref_datasets  # noqa: E402  (reference)

SIZES = [(24, 40), (26, 44), (25, 43), (24, 40)]
CROP_TYPES = [["none"], ["horizontal"], ["horizontal", "anchored"], ["vertical"], ["horizontal", "vertical"],
              ["horizontal", "vertical", "anchored"], ["horizontal", "vertical", "anchored", "bottom"], ["bottom"]]
SHAPES = [(16, 24), (13, 21)]
# one seed a (crop type, shape), in the order of the two loops below
SEEDS = [1, 2, 3, 4, 5, 6, 7, 1, 9, 10, 1, 1, 13, 14, 15, 16]      # (the 'vertical' ones move a crop of the first pass already)
PASSES = 3


def paths(indices=range(4)):
    return ([os.path.join(IO, f"triplet_{i}.png") for i in indices], [os.path.join(IO, f"depth_{i}.png") for i in indices],
            [os.path.join(IO, f"k_{i}.npy") for i in indices])


def write_inputs():
    os.makedirs(IO, exist_ok=True)
    rng = np.random.default_rng(2024)
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, size=(h, 3 * w, 3), dtype=np.uint8), mode="RGB").save(os.path.join(IO, f"triplet_{i}.png"))
        z = rng.integers(256, 80 * 256, size=(h, w)).astype(np.uint32)
        z[rng.random((h, w)) >= 0.40] = 0
        Image.fromarray(z, mode="I").save(os.path.join(IO, f"depth_{i}.png"))
        k = np.array([[700.0 + 10 * i, 0.0, w / 2 + 0.25 * i], [0.0, 710.0 + 10 * i, h / 2 + 0.5 * i], [0.0, 0.0, 1.0]], dtype=np.float64)
        np.save(os.path.join(IO, f"k_{i}.npy"), k)


def run_reference(crop_type, shape, seed, indices=range(4), passes=PASSES):
    """-> (the samples in draw order, the values np.random.rand returned)."""
    dataset = ref_datasets.KBNetTrainingDataset(*paths(indices), shape=shape, random_crop_type=crop_type)
    drawn, rand = [], np.random.rand

    def logged(*args):
        v = rand(*args)
        drawn.append(v)
        return v

    np.random.seed(seed)
    np.random.rand = logged
    try:
        samples = [dataset[i] for _ in range(passes) for i in range(len(dataset))]
    finally:
        np.random.rand = rand
    return samples, drawn


def starts(samples, indices=range(4)):
    """(y_start, x_start) of every draw, from the adjusted intrinsics."""
    ks = [np.load(p).astype(np.float32) for p in paths(indices)[2]]
    out = []
    for j, s in enumerate(samples):
        k = ks[j % len(ks)]
        out.append((int(round(float(k[1, 2]) - float(s[4][1, 2]))), int(round(float(k[0, 2]) - float(s[4][0, 2])))))
    return out


def record(out, name, samples, first):
    out[name + "::k"] = np.stack([s[4] for s in samples])
    for slot, key in enumerate(("image0", "image1", "image2")):
        a = np.stack([s[slot] for s in samples[:first]])
        assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and a.min() >= 0 and a.max() <= 255
        out[name + "::" + key] = a.astype(np.uint8)
    depth = np.stack([s[3] for s in samples[:first]])
    assert depth.dtype == np.float32 and all(s[4].dtype == np.float32 for s in samples)
    out[name + "::depth"] = depth


def main():
    write_inputs()
    out, runs, odd = {}, [], False
    seeds = iter(SEEDS)
    for crop_type in CROP_TYPES:
        for shape in SHAPES:
            seed = next(seeds)
            samples, drawn = run_reference(crop_type, list(shape), seed)
            yx = starts(samples)
            if "vertical" in crop_type and "bottom" not in crop_type:
                assert len(drawn) == len(samples) and min(drawn) <= 0.30 < max(drawn), (crop_type, shape, seed, drawn)
                assert any(y != (h - shape[0]) // 2 for (y, _), (h, _) in zip(yx, SIZES)), "no crop of the first pass moved vertically"
            else:
                assert not drawn
            if "horizontal" in crop_type:
                assert len(set(x for _, x in yx)) >= 2, (crop_type, shape, seed, yx)
            odd = odd or any(x % 2 for _, x in yx)
            name = f"r{len(runs)}"
            runs.append(dict(name=name, crop_type=crop_type, shape=list(shape), np_seed=seed, starts=[list(v) for v in yx]))
            record(out, name, samples, len(SIZES))
    assert odd, "no odd x_start in any run"
    same = [0, 3]      # the two 24 x 40 samples: no crop, one batch
    samples, drawn = run_reference(["horizontal", "vertical"], None, 99, indices=same, passes=1)
    assert not drawn and all(s[0].shape == (3, 24, 40) for s in samples)
    runs.append(dict(name="full", crop_type=["horizontal", "vertical"], shape=None, np_seed=99, indices=same, starts=[[0, 0], [0, 0]]))
    record(out, "full", samples, len(same))
    out["runs"] = np.frombuffer(json.dumps(runs).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "train_loader.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(runs), "runs")


if __name__ == "__main__":
    main()
