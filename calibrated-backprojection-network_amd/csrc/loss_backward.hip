// loss_backward.hip -- the gradient of KBNet's objective (KBNetModel.compute_loss) as ONE image-sized kernel.
//
//  kbn_photometric_loss_backward : torch.autograd's backward of     reference src/net_utils.py:1638-1739 (project, grid_sample)
//                                  every operation of               reference src/losses.py:23-158       (the four terms)
//                                                                   reference src/kbnet_model.py:188-304 (composition)
//
// Gradients exist for what the reference trains through: the depth (per pixel) and the two relative poses (per frame, as
// dL/dT with T = rows 0-2 of (K | 0) pose; the caller multiplies by K^T).  With that scope every gradient is a GATHER: a
// pixel's depth gradient needs its own warp and the SSIM windows that contain it (centres up to 1 pixel away, their pixels up
// to 2 away), so nothing is scattered into image1 / image2 and no atomic touches image-sized data.
//
//   tile          64 x 16 output pixels (+ halo 2 -> 68 x 20 staged), 256 threads = 4 waves; a thread takes the staged
//                 elements tid + 256 k (k < 6) in EVERY pass, so what it keeps of a pixel between passes stays in registers
//   LDS           image0 3 planes + warped 3 planes + depth + 3 SSIM coefficient planes (one channel at a time) of 68 x 20
//                 floats + 84 stretch weights + 48 doubles = 55 128 B with alignment -> 2 workgroups = 8 waves per CU
//   HBM           12 fp32 planes read once (+ 33 % halo re-reads that hit L2), 1 plane written: each pixel of grad_depth
//                 exactly once, coalesced, no memset, no atomics
//   pose          12 entries of dL/dT per pair: fp32 per pixel, fp64 across pixels, registers -> wave shuffle -> LDS -> one
//                 atomicAdd(double) per entry per workgroup (as the forward's sums)
//
// SSIM: dv/dx_p = A + B x_p + C y_p inside a window (x the warped image, y image0); pass 1 writes A, B, C of every window
// centre (times the upstream gradient, the stretch weight and the clamp mask), pass 2 sums the up to nine windows of a pixel.
// The moments are taken of x - x_c, y - y_c (the centre pixel) as in the forward, for the same reason.
//
// Kinks follow torch: sgn(0) = 0; the clamp passes gradient on [0, 1], both ends; the sample position has no gradient where
// the forward clamped it to the border (ix <= 0 or ix >= W - 1, NaN included).
//
// Addressing: the forward's rule.  A sample position comes from a division by z + 1e-7 and may be huge, negative, infinite or
// NaN.  It is clamped as a float with comparisons that send NaN to 0, converted, and then clamped AGAIN as an integer into
// [0, W-1] x [0, H-1] (loss_common.h); every other address is a function of the tile index alone.
#include "loss_common.h"

namespace kbn {

constexpr int LB_ZW = LS_TW + 4, LB_ZH = LS_TH + 4, LB_ZN = LB_ZW * LB_ZH;   // the tile and a two-pixel halo
constexpr int LB_K = (LB_ZN + 255) / 256;                                    // staged elements per thread

__device__ __forceinline__ float sgnf(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }   // 0 for 0 and for NaN

__global__ __launch_bounds__(256) void photometric_loss_backward_kernel(
    const float* __restrict__ image0, const float* __restrict__ image1, const float* __restrict__ image2,
    const float* __restrict__ depth, const float* __restrict__ sparse, const float* __restrict__ validity,
    const float* __restrict__ intrinsics, const float* __restrict__ pose01, const float* __restrict__ pose02,
    const double* __restrict__ grad_sums, float* __restrict__ grad_depth, double* __restrict__ grad_proj, int H, int W, int tilesX,
    int tilesY) {
    __shared__ float s_img0[3][LB_ZN];
    __shared__ float s_warp[3][LB_ZN];
    __shared__ float s_depth[LB_ZN];
    __shared__ float s_a[LB_ZN], s_b[LB_ZN], s_c[LB_ZN];
    __shared__ float s_wy[LB_ZH - 2], s_wx[LB_ZW - 2];   // of the window centres: staged rows / columns 1 .. size - 2
    __shared__ double s_red[4][12];

    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int tx = bid % tilesX; bid /= tilesX;
    const int ty = bid % tilesY;
    const int n = bid / tilesY;
    const int y0 = ty * LS_TH, x0 = tx * LS_TW;
    const long long HW = (long long)H * W;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float* i0 = image0 + (long long)n * 3 * HW;
    const float* dp = depth + (long long)n * HW;

    float kinv[9];
    loss_kinv(intrinsics + (long long)n * 9, kinv);
    float gs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) gs[k] = (float)grad_sums[(long long)n * 8 + k];

    // ---- stage image0 and the depth of the tile and its halo; pixels outside the image are zeros nobody weighs
#pragma unroll
    for (int k = 0; k < LB_K; ++k) {
        const int e = tid + 256 * k;
        if (e >= LB_ZN) continue;
        const int r = e / LB_ZW, c = e - r * LB_ZW;
        const int Y = y0 - 2 + r, X = x0 - 2 + c;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, z = 0.f;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
            const long long o = (long long)Y * W + X;
            a0 = i0[o]; a1 = i0[HW + o]; a2 = i0[2 * HW + o]; z = dp[o];
        }
        s_img0[0][e] = a0; s_img0[1][e] = a1; s_img0[2][e] = a2; s_depth[e] = z;
    }
    // weight of each SSIM window = the number of output pixels torch's nearest up-sampling copies its score to; 0 where the
    // 3 x 3 window of the unpadded average pool does not fit (centres on the image border) and beyond the image
    if (tid < LB_ZH - 2) {
        const int Y = y0 - 1 + tid;
        s_wy[tid] = (Y >= 1 && Y <= H - 2) ? (float)ssim_axis_weight(Y - 1, H) : 0.f;
    } else if (tid >= 64 && tid < 64 + LB_ZW - 2) {
        const int X = x0 - 1 + tid - 64;
        s_wx[tid - 64] = (X >= 1 && X <= W - 2) ? (float)ssim_axis_weight(X - 1, W) : 0.f;
    }
    __syncthreads();

    float gz[LB_K];   // the depth gradient of the thread's owned pixels
#pragma unroll
    for (int k = 0; k < LB_K; ++k) gz[k] = 0.f;

    for (int pair = 0; pair < 2; ++pair) {
        const float gs_c = gs[pair], gs_s = gs[2 + pair];
        if (gs_c == 0.f && gs_s == 0.f) continue;   // the same for the whole workgroup: nothing of this pair is asked for
        const float* src = (pair ? image2 : image1) + (long long)n * 3 * HW;
        float t[12];
        loss_projection(intrinsics + (long long)n * 9, (pair ? pose02 : pose01) + (long long)n * 16, t);

        // d warped[ch] / d ix, d iy of the owned pixels (zero where the forward clamped the position), and the gradient of the
        // loss with respect to ix, iy as far as it is known
        float dwx[LB_K][3], dwy[LB_K][3], gix[LB_K], giy[LB_K];

        // ---- warp the tile and its halo into LDS; the owned pixels keep their taps' differences and take the colour term
#pragma unroll
        for (int k = 0; k < LB_K; ++k) {
            gix[k] = 0.f; giy[k] = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { dwx[k][ch] = 0.f; dwy[k][ch] = 0.f; }
            const int e = tid + 256 * k;
            if (e >= LB_ZN) continue;
            const int r = e / LB_ZW, c = e - r * LB_ZW;
            const int Y = y0 - 2 + r, X = x0 - 2 + c;
            float v[3] = {0.f, 0.f, 0.f};
            if (Y >= 0 && Y < H && X >= 0 && X < W) {
                float ix, iy;
                loss_clamped_position(loss_project_point(kinv, t, (float)X, (float)Y, s_depth[e]), wm1, hm1, ix, iy);
                const LossTaps tp = loss_taps(ix, iy, W, H);
                const long long oa = (long long)tp.ya * W, ob = (long long)tp.yb * W;
                const bool owned = r >= 2 && r < 2 + LS_TH && c >= 2 && c < 2 + LS_TW;
                const bool east = tp.xa + 1 <= W - 1, south = tp.ya + 1 <= H - 1;   // a tap outside the image counts as 0
                const float mx = (ix > 0.f && ix < wm1) ? 1.f : 0.f, my = (iy > 0.f && iy < hm1) ? 1.f : 0.f;
                const float ax = ix - tp.fx0, ay = iy - tp.fy0, bx = (tp.fx0 + 1.0f) - ix, by = (tp.fy0 + 1.0f) - iy;
                const float* s = src;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch, s += HW) {
                    const float nw = s[oa + tp.xa], ne = s[oa + tp.xb], sw = s[ob + tp.xa], se = s[ob + tp.xb];
                    v[ch] = nw * tp.wnw + ne * tp.wne + sw * tp.wsw + se * tp.wse;
                    if (owned) {
                        const float ne0 = east ? ne : 0.f, sw0 = south ? sw : 0.f, se0 = (east && south) ? se : 0.f;
                        dwx[k][ch] = mx * ((ne0 - nw) * by + (se0 - sw0) * ay);
                        dwy[k][ch] = my * ((sw0 - nw) * bx + (se0 - ne0) * ax);
                        if (gs_c != 0.f) {
                            const float g = gs_c * sgnf(v[ch] - s_img0[ch][e]);
                            gix[k] = fmaf(g, dwx[k][ch], gix[k]);
                            giy[k] = fmaf(g, dwy[k][ch], giy[k]);
                        }
                    }
                }
            }
            s_warp[0][e] = v[0]; s_warp[1][e] = v[1]; s_warp[2][e] = v[2];
        }
        __syncthreads();

        // ---- SSIM, one channel at a time through the three coefficient planes
        if (gs_s != 0.f) {
            for (int ch = 0; ch < 3; ++ch) {
                // pass 1: a thread per window centre (staged rows 1 .. 18, columns 1 .. 66)
#pragma unroll
                for (int k = 0; k < LB_K; ++k) {
                    const int e = tid + 256 * k;
                    if (e >= LB_ZN) continue;
                    const int r = e / LB_ZW, c = e - r * LB_ZW;
                    if (r < 1 || r > LB_ZH - 2 || c < 1 || c > LB_ZW - 2) continue;
                    const float wgt = s_wy[r - 1] * s_wx[c - 1];
                    float A = 0.f, B = 0.f, C = 0.f;
                    if (wgt > 0.f) {
                        const float* xr = &s_warp[ch][e - LB_ZW - 1];
                        const float* yr = &s_img0[ch][e - LB_ZW - 1];
                        const float cx = s_warp[ch][e], cy = s_img0[ch][e];
                        float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
                        for (int j = 0; j < 3; ++j)
#pragma unroll
                            for (int i = 0; i < 3; ++i) {
                                const float xv = xr[j * LB_ZW + i] - cx, yv = yr[j * LB_ZW + i] - cy;
                                sx += xv; sy += yv;
                                sxx = fmaf(xv, xv, sxx); syy = fmaf(yv, yv, syy); sxy = fmaf(xv, yv, sxy);
                            }
                        const float dx = sx / 9.0f, dy = sy / 9.0f;
                        const float mu_x = cx + dx, mu_y = cy + dy;
                        const float sg_x = sxx / 9.0f - dx * dx, sg_y = syy / 9.0f - dy * dy, sg_xy = sxy / 9.0f - dx * dy;
                        const float n1 = 2.0f * mu_x * mu_y + 1e-4f, n2 = 2.0f * sg_xy + 9e-4f;
                        const float d1 = mu_x * mu_x + mu_y * mu_y + 1e-4f, d2 = sg_x + sg_y + 9e-4f;
                        const float den = d1 * d2;
                        const float score = n1 * n2 / den;
                        const float val = (1.0f - score) / 2.0f;
                        // torch.clamp's backward: the gradient passes on [0, 1], both ends; not for NaN
                        const float coef = (val >= 0.f && val <= 1.f) ? (-0.5f * wgt * gs_s) / (9.0f * den) : 0.f;
                        B = coef * (-2.0f * score * d1);
                        C = coef * (2.0f * n1);
                        // the gradient at the centre pixel, then the intercept at x = y = 0
                        const float at_centre = coef * (2.0f * mu_y * n2 - 2.0f * score * mu_x * d2) - B * dx - C * dy;
                        A = at_centre - B * cx - C * cy;
                    }
                    s_a[e] = A; s_b[e] = B; s_c[e] = C;
                }
                __syncthreads();
                // pass 2: an owned pixel sums the windows that contain it
#pragma unroll
                for (int k = 0; k < LB_K; ++k) {
                    const int e = tid + 256 * k;
                    if (e >= LB_ZN) continue;
                    const int r = e / LB_ZW, c = e - r * LB_ZW;
                    if (r < 2 || r >= 2 + LS_TH || c < 2 || c >= 2 + LS_TW || y0 - 2 + r >= H || x0 - 2 + c >= W) continue;
                    float sa = 0.f, sb = 0.f, sc = 0.f;
#pragma unroll
                    for (int j = -1; j <= 1; ++j)
#pragma unroll
                        for (int i = -1; i <= 1; ++i) {
                            const int q = e + j * LB_ZW + i;
                            sa += s_a[q]; sb += s_b[q]; sc += s_c[q];
                        }
                    const float g = fmaf(s_img0[ch][e], sc, fmaf(s_warp[ch][e], sb, sa));
                    gix[k] = fmaf(g, dwx[k][ch], gix[k]);
                    giy[k] = fmaf(g, dwy[k][ch], giy[k]);
                }
                __syncthreads();   // the next channel's pass 1 (or the next frame's warp) overwrites what pass 2 read
            }
        }

        // ---- from the sample position back through the projection: u = q0 / d, v = q1 / d, q = T (ray z, 1)
        double acc[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) acc[j] = 0.0;
#pragma unroll
        for (int k = 0; k < LB_K; ++k) {
            const int e = tid + 256 * k;
            if (e >= LB_ZN) continue;
            const float gu = gix[k], gv = giy[k];
            if (gu == 0.f && gv == 0.f) continue;   // not an owned pixel, or clamped in both directions, or no gradient
            const int r = e / LB_ZW, c = e - r * LB_ZW;
            const LossPoint p = loss_project_point(kinv, t, (float)(x0 - 2 + c), (float)(y0 - 2 + r), s_depth[e]);
            const float u = p.q0 / p.d, v = p.q1 / p.d;
            const float gq0 = gu / p.d, gq1 = gv / p.d;
            const float gq2 = -((gu != 0.f ? gu * u : 0.f) + (gv != 0.f ? gv * v : 0.f)) / p.d;
            gz[k] += gq0 * fmaf(t[2], p.rz, fmaf(t[1], p.ry, t[0] * p.rx)) + gq1 * fmaf(t[6], p.rz, fmaf(t[5], p.ry, t[4] * p.rx)) +
                     gq2 * fmaf(t[10], p.rz, fmaf(t[9], p.ry, t[8] * p.rx));
            acc[0] += (double)(gq0 * p.X); acc[1] += (double)(gq0 * p.Y); acc[2] += (double)(gq0 * p.Z); acc[3] += (double)gq0;
            acc[4] += (double)(gq1 * p.X); acc[5] += (double)(gq1 * p.Y); acc[6] += (double)(gq1 * p.Z); acc[7] += (double)gq1;
            acc[8] += (double)(gq2 * p.X); acc[9] += (double)(gq2 * p.Y); acc[10] += (double)(gq2 * p.Z); acc[11] += (double)gq2;
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            double a = acc[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
            if ((tid & 63) == 0) s_red[tid >> 6][j] = a;
        }
        __syncthreads();
        if (tid < 12)
            atomicAdd(grad_proj + ((long long)n * 2 + pair) * 12 + tid, s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid]);
        __syncthreads();   // s_red and s_warp are free again
    }

    // ---- sparse-depth term and edge-aware smoothness; every owned pixel of grad_depth is written exactly once
    {
        const float* sp = sparse + (long long)n * HW;
        const float* vl = validity + (long long)n * HW;
        float* out = grad_depth + (long long)n * HW;
#pragma unroll
        for (int k = 0; k < LB_K; ++k) {
            const int e = tid + 256 * k;
            if (e >= LB_ZN) continue;
            const int r = e / LB_ZW, c = e - r * LB_ZW;
            const int Y = y0 - 2 + r, X = x0 - 2 + c;
            if (r < 2 || r >= 2 + LS_TH || c < 2 || c >= 2 + LS_TW || Y >= H || X >= W) continue;
            const long long o = (long long)Y * W + X;
            const float z = s_depth[e];
            float g = gz[k];
            if (gs[4] != 0.f) g = fmaf(gs[4] * vl[o], sgnf(z - sp[o]), g);
            const float a0 = s_img0[0][e], a1 = s_img0[1][e], a2 = s_img0[2][e];
            if (gs[6] != 0.f) {
                if (X < W - 1) {
                    const float d = (fabsf(a0 - s_img0[0][e + 1]) + fabsf(a1 - s_img0[1][e + 1]) + fabsf(a2 - s_img0[2][e + 1])) / 3.0f;
                    g = fmaf(gs[6] * expf(-d), sgnf(z - s_depth[e + 1]), g);
                }
                if (X >= 1) {
                    const float d = (fabsf(s_img0[0][e - 1] - a0) + fabsf(s_img0[1][e - 1] - a1) + fabsf(s_img0[2][e - 1] - a2)) / 3.0f;
                    g = fmaf(-gs[6] * expf(-d), sgnf(s_depth[e - 1] - z), g);
                }
            }
            if (gs[7] != 0.f) {
                if (Y < H - 1) {
                    const float d = (fabsf(a0 - s_img0[0][e + LB_ZW]) + fabsf(a1 - s_img0[1][e + LB_ZW]) + fabsf(a2 - s_img0[2][e + LB_ZW])) / 3.0f;
                    g = fmaf(gs[7] * expf(-d), sgnf(z - s_depth[e + LB_ZW]), g);
                }
                if (Y >= 1) {
                    const float d = (fabsf(s_img0[0][e - LB_ZW] - a0) + fabsf(s_img0[1][e - LB_ZW] - a1) + fabsf(s_img0[2][e - LB_ZW] - a2)) / 3.0f;
                    g = fmaf(-gs[7] * expf(-d), sgnf(s_depth[e - LB_ZW] - z), g);
                }
            }
            out[o] = g;
        }
    }
}

}  // namespace kbn

extern "C" int kbn_photometric_loss_backward(const float* image0, const float* image1, const float* image2,
                                             const float* output_depth, const float* sparse_depth, const float* validity_map,
                                             const float* intrinsics, const float* pose01, const float* pose02,
                                             const double* grad_sums, float* grad_depth, double* grad_proj, int n, int height, int width,
                                             kbn_stream_t stream) {
    using namespace kbn;
    if (!image0 || !image1 || !image2 || !output_depth || !sparse_depth || !validity_map || !intrinsics || !pose01 || !pose02 ||
        !grad_sums || !grad_depth || !grad_proj)
        return KBN_ERR_INVALID_ARGUMENT;
    if (n < 1 || height < 3 || width < 3) return KBN_ERR_INVALID_ARGUMENT;   // as the forward: SSIM pools 3 x 3 without padding
    const int tilesX = ceil_div(width, LS_TW), tilesY = ceil_div(height, LS_TH);
    const long long blocks = (long long)tilesX * tilesY * n;
    if (blocks > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(grad_proj, 0, (size_t)n * 24 * sizeof(double), st) != hipSuccess) return KBN_ERR_LAUNCH;
    hipLaunchKernelGGL(photometric_loss_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, st, image0, image1, image2, output_depth,
                       sparse_depth, validity_map, intrinsics, pose01, pose02, grad_sums, grad_depth, grad_proj, height, width, tilesX,
                       tilesY);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
