// loss_common.h -- what the forward (loss.hip) and the backward (loss_backward.hip) of the objective must compute alike: the
// SSIM stretch weights, K^-1, the projection T = rows 0-2 of (K | 0) pose, and the way from a pixel and its depth to the
// border-clamped sample position.  One copy, so that the backward differentiates the positions the forward sampled at.
#pragma once
#include <math.h>

#include "kbn_common.h"

namespace kbn {

constexpr int LS_TW = 64, LS_TH = 16;   // the tile of output pixels a workgroup owns, in both kernels

// how many pixels of the H-long (W-long) output axis torch's nearest interpolation maps to score `s` of the
// (size - 2)-long SSIM axis: interpolate(scores, size, mode='nearest'), reference src/losses.py:58
__device__ __forceinline__ int ssim_axis_weight(int s, int size) {
    int cnt = 0;
    for (int d = s; d <= s + 3 && d < size; ++d) cnt += nearest_src_index(d, size - 2, size) == s;
    return cnt;
}

// K^-1 and the top three rows of (K | 0) * pose, in fp64 from the fp32 inputs, rounded once
__device__ __forceinline__ void loss_kinv(const float* __restrict__ k, float* kinv) {
    const double A = k[0], B = k[1], C = k[2], D = k[3], E = k[4], F = k[5], G = k[6], H = k[7], I = k[8];
    const double c00 = E * I - F * H, c01 = -(D * I - F * G), c02 = D * H - E * G;
    const double r = 1.0 / (A * c00 + B * c01 + C * c02);
    kinv[0] = (float)(c00 * r);
    kinv[1] = (float)(-(B * I - C * H) * r);
    kinv[2] = (float)((B * F - C * E) * r);
    kinv[3] = (float)(c01 * r);
    kinv[4] = (float)((A * I - C * G) * r);
    kinv[5] = (float)(-(A * F - C * D) * r);
    kinv[6] = (float)(c02 * r);
    kinv[7] = (float)(-(A * H - B * G) * r);
    kinv[8] = (float)((A * E - B * D) * r);
}
__device__ __forceinline__ void loss_projection(const float* __restrict__ k, const float* __restrict__ pose, float* t) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            t[i * 4 + j] = (float)((double)k[i * 3] * pose[j] + (double)k[i * 3 + 1] * pose[4 + j] + (double)k[i * 3 + 2] * pose[8 + j]);
}

// pixel (x, y) at depth z: its ray K^-1 (x, y, 1)^T, the camera point P = ray * z, and q = T (P, 1) with d = q2 + 1e-7
struct LossPoint {
    float rx, ry, rz;   // ray
    float X, Y, Z;      // ray * z
    float q0, q1, d;
};
__device__ __forceinline__ LossPoint loss_project_point(const float* kinv, const float* t, float x, float y, float z) {
    LossPoint p;
    p.rx = fmaf(kinv[1], y, kinv[0] * x) + kinv[2];
    p.ry = fmaf(kinv[4], y, kinv[3] * x) + kinv[5];
    p.rz = fmaf(kinv[7], y, kinv[6] * x) + kinv[8];
    p.X = p.rx * z; p.Y = p.ry * z; p.Z = p.rz * z;
    p.q0 = fmaf(t[2], p.Z, fmaf(t[1], p.Y, t[0] * p.X)) + t[3];
    p.q1 = fmaf(t[6], p.Z, fmaf(t[5], p.Y, t[4] * p.X)) + t[7];
    const float q2 = fmaf(t[10], p.Z, fmaf(t[9], p.Y, t[8] * p.X)) + t[11];
    p.d = q2 + 1e-7f;
    return p;
}

// the un-normalised, border-clamped sample position torch's grid_sample arrives at (align_corners=True), in the reference's
// fp32 operation order: divide by size - 1, 2 (t - 0.5), ((g + 1) / 2) (size - 1).  NaN -> 0.
__device__ __forceinline__ void loss_clamped_position(const LossPoint& p, float wm1, float hm1, float& ix, float& iy) {
    const float gx = 2.0f * (p.q0 / p.d / wm1 - 0.5f);
    const float gy = 2.0f * (p.q1 / p.d / hm1 - 0.5f);
    ix = ((gx + 1.0f) / 2.0f) * wm1;
    iy = ((gy + 1.0f) / 2.0f) * hm1;
    ix = ix >= 0.f ? ix : 0.f;       // false for NaN: NaN -> 0
    iy = iy >= 0.f ? iy : 0.f;
    ix = ix <= wm1 ? ix : wm1;
    iy = iy <= hm1 ? iy : hm1;
}
__device__ __forceinline__ void loss_sample_position(const float* kinv, const float* t, float x, float y, float z, float wm1, float hm1,
                                                     float& ix, float& iy) {
    loss_clamped_position(loss_project_point(kinv, t, x, y, z), wm1, hm1, ix, iy);
}

// the four bilinear taps of a clamped position: integer addresses clamped AGAIN into the plane, and the weights, a tap outside
// the image weighing 0 (torch skips it).  ix, iy are finite and inside [0, W-1] x [0, H-1]; the integer clamp makes the
// addresses safe whatever they are.
struct LossTaps {
    int xa, xb, ya, yb;
    float wnw, wne, wsw, wse;
    float fx0, fy0;
};
__device__ __forceinline__ LossTaps loss_taps(float ix, float iy, int W, int H) {
    LossTaps s;
    s.fx0 = floorf(ix); s.fy0 = floorf(iy);
    const float fx1 = s.fx0 + 1.0f, fy1 = s.fy0 + 1.0f;
    s.wnw = (fx1 - ix) * (fy1 - iy); s.wne = (ix - s.fx0) * (fy1 - iy);
    s.wsw = (fx1 - ix) * (iy - s.fy0); s.wse = (ix - s.fx0) * (iy - s.fy0);
    int xa = (int)s.fx0, ya = (int)s.fy0;
    xa = xa < 0 ? 0 : (xa > W - 1 ? W - 1 : xa);
    ya = ya < 0 ? 0 : (ya > H - 1 ? H - 1 : ya);
    int xb = xa + 1, yb = ya + 1;
    if (xb > W - 1) { xb = W - 1; s.wne = 0.f; s.wse = 0.f; }
    if (yb > H - 1) { yb = H - 1; s.wsw = 0.f; s.wse = 0.f; }
    s.xa = xa; s.xb = xb; s.ya = ya; s.yb = yb;
    return s;
}

}  // namespace kbn
