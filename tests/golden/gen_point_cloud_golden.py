"""Writes tests/golden/point_cloud_backproject.npz: the reference's backprojection of a small case, in float64.

    python tests/golden/gen_point_cloud_golden.py <the reference's src directory>

Run where the reference exists.  Nothing of the reference's source is stored: the fixture is data --
  depth       2 x 1 x 7 x 9 float64    tests/point_cloud_cases.golden_case()
  intrinsics  2 x 3 x 3 float64        with skew, another camera a frame
  points      2 x 3 x 7 x 9 float64    net_utils.backproject_to_camera(depth, intrinsics, shape)[:, :3], reshaped to the frame
tests/test_point_cloud_cpu.py holds the oracle's fp64 form against `points`: the pixel convention (x the column, y the row, integer
coordinates from 0) and the axis order of the point clouds are the reference's."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import point_cloud_cases as pc  # noqa: E402


def main(reference_src):
    sys.path.insert(0, reference_src)
    import net_utils  # noqa: E402  (reference)

    depth, intrinsics = pc.golden_case()
    n, _, h, w = depth.shape
    torch.set_default_dtype(torch.float64)      # the reference's meshgrid takes the default dtype
    with torch.no_grad():
        points = net_utils.backproject_to_camera(torch.from_numpy(depth), torch.from_numpy(intrinsics), [n, 1, h, w])
    assert points.dtype == torch.float64 and tuple(points.shape) == (n, 4, h * w)
    assert torch.all(points[:, 3] == 1.0)
    np.savez(pc.GOLDEN, depth=depth, intrinsics=intrinsics, points=points[:, :3].reshape(n, 3, h, w).numpy())
    print(pc.GOLDEN, os.path.getsize(pc.GOLDEN), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
