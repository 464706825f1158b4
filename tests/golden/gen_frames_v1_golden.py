#!/usr/bin/env python
"""Generate tests/golden/frames_v1/*: two tiny packed frames, version 1, written by the NumPy encoder of tests/frame_pack_oracle.py,
and the samples they hold.  The library must go on decoding these files: they pin version 1 of the format.

  rgb8_21x11.kbf / .npy     11 x 21 x 3 uint8: a smooth ramp with a little noise; a short last segment (5 samples), a short last group
  depth16_21x11.kbf / .npy  11 x 21 uint16: sparse depth samples, among them 65535 beside 0
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frame_pack_oracle as orc  # noqa: E402

OUT = os.path.join(HERE, "frames_v1")


def main():
    os.makedirs(OUT, exist_ok=True)
    g = np.random.Generator(np.random.Philox(20))
    y, x = np.mgrid[0:11, 0:21]
    rgb = np.stack([(6 * x + 3 * y + c * 40 + g.integers(0, 3, size=x.shape)) % 256 for c in range(3)], axis=2).astype(np.uint8)
    depth = np.where(g.random((11, 21)) < 0.1, g.integers(1, 65536, size=(11, 21)), 0).astype(np.uint16)
    depth[3, 4], depth[3, 5], depth[4, 4] = 65535, 0, 0
    for name, a in (("rgb8_21x11", rgb), ("depth16_21x11", depth)):
        with open(os.path.join(OUT, name + ".kbf"), "wb") as f:
            f.write(orc.encode(a))
        np.save(os.path.join(OUT, name + ".npy"), a)
        print(name, os.path.getsize(os.path.join(OUT, name + ".kbf")), "bytes")


if __name__ == "__main__":
    main()
