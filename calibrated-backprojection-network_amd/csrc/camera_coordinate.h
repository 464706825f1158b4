// camera_coordinate.h -- the camera-frame coordinate of a pixel, stated once: component j of K^-1 [x y 1]^T (reference
// src/networks.py:317-331) for integer pixel coordinates x = 0 .. W-1, y = 0 .. H-1.  kbn_camera_coordinates (kb.hip) stores it and
// kbn_point_cloud_forward (point_cloud.hip) multiplies it by the depth: both include this, so that a point is bit for bit
// coordinate * depth.  One product rounded to fp32, one FMA, one sum -- the order tests/golden pins (test_coordinates_golden).
#pragma once

#include <hip/hip_runtime.h>

namespace kbn {

// k: the 9 floats of one frame's K^-1, row-major
__device__ __forceinline__ float camera_coordinate(const float* __restrict__ k, int j, int x, int y) {
    return fmaf(k[j * 3 + 1], (float)y, k[j * 3 + 0] * (float)x) + k[j * 3 + 2];
}

}  // namespace kbn
