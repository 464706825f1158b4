// loss.hip -- the forward value of KBNet's objective (KBNetModel.compute_loss) as ONE image-sized kernel.
//
//  kbn_photometric_loss_forward : backproject / reproject          reference src/net_utils.py:1638-1704
//                                 bilinear border sampling          reference src/net_utils.py:1706-1739
//                                 colour L1, SSIM, sparse L1,       reference src/losses.py:23-158
//                                 edge-aware smoothness
//                                 (composition)                     reference src/kbnet_model.py:188-304
//
// The reference composes this from ~40 torch launches and ~30 image-sized intermediates (point clouds, coordinate grids,
// two warped images, five average pools per SSIM per pair).  Here nothing image-sized is written unless the caller asks
// for the warped images: a workgroup owns a 64 x 16 tile of output pixels, warps the tile and a one-pixel halo into LDS
// (the four bilinear taps gather from image1 / image2 in HBM, indices clamped as integers), and takes every term from LDS.
//
//   tile          64 x 16 output pixels (+ halo 1 -> 66 x 18 staged), 256 threads = 4 waves
//   LDS           image0 3 planes + warped 3 planes + depth 1 plane of 66 x 18 floats + 80 SSIM weights = 33 584 B
//                 (the two neighbour frames take turns in the warped planes) -> 4 workgroups = 16 waves per CU
//   HBM           12 fp32 planes read once (+ 16 % halo re-reads that hit L2), 6 planes written when images are asked for
//   reduction     fp32 per pixel as the reference computes it, fp64 across pixels: registers -> wave shuffle -> LDS ->
//                 one atomicAdd(double) per term per workgroup (as eval_kernel, pre_eval.hip)
//
// Addressing: a sample position comes from a division by z + 1e-7 and may be huge, negative, infinite or NaN.  It is
// clamped as a float with comparisons that send NaN to 0, converted, and then clamped AGAIN as an integer into
// [0, W-1] x [0, H-1]; every other address is a function of the tile index alone.
#include "loss_common.h"   // K^-1, T and the sample position: shared with loss_backward.hip

namespace kbn {

constexpr int LS_ZW = LS_TW + 2, LS_ZH = LS_TH + 2, LS_ZN = LS_ZW * LS_ZH;   // the tile and a one-pixel halo
constexpr int LS_ROWS = LS_TH / 4;   // SSIM: one thread takes a column strip of 4 output rows

// sums[n * 8 + k] += { sum |image01 - image0|, sum |image02 - image0|, sum ssim01, sum ssim02, sum v |sparse - depth|, sum v,
//                      sum wx |dx depth|, sum wy |dy depth| }
__global__ __launch_bounds__(256) void photometric_loss_kernel(
    const float* __restrict__ image0, const float* __restrict__ image1, const float* __restrict__ image2,
    const float* __restrict__ depth, const float* __restrict__ sparse, const float* __restrict__ validity,
    const float* __restrict__ intrinsics, const float* __restrict__ pose01, const float* __restrict__ pose02,
    double* __restrict__ sums, float* __restrict__ image01, float* __restrict__ image02, int H, int W, int tilesX, int tilesY) {
    __shared__ float s_img0[3][LS_ZN];
    __shared__ float s_warp[3][LS_ZN];
    __shared__ float s_depth[LS_ZN];
    __shared__ float s_wy[LS_TH], s_wx[LS_TW];
    __shared__ double s_red[4][8];

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

    // ---- stage image0 and the depth of the tile and its halo; pixels outside the image are zeros nobody weighs
    for (int e = tid; e < LS_ZN; e += 256) {
        const int r = e / LS_ZW, c = e - r * LS_ZW;
        const int Y = y0 - 1 + r, X = x0 - 1 + c;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, z = 0.f;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
            const long long o = (long long)Y * W + X;
            a0 = i0[o]; a1 = i0[HW + o]; a2 = i0[2 * HW + o]; z = dp[o];
        }
        s_img0[0][e] = a0; s_img0[1][e] = a1; s_img0[2][e] = a2; s_depth[e] = z;
    }
    // weight of each SSIM score = the number of output pixels torch's nearest up-sampling copies it to; 0 where the 3 x 3
    // window of the unpadded average pool does not fit (centres on the image border) and beyond the image
    if (tid < LS_TH) {
        const int Y = y0 + tid;
        s_wy[tid] = (Y >= 1 && Y <= H - 2) ? (float)ssim_axis_weight(Y - 1, H) : 0.f;
    } else if (tid >= 64 && tid < 64 + LS_TW) {
        const int X = x0 + tid - 64;
        s_wx[tid - 64] = (X >= 1 && X <= W - 2) ? (float)ssim_axis_weight(X - 1, W) : 0.f;
    }
    __syncthreads();

    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    for (int pair = 0; pair < 2; ++pair) {
        const float* src = (pair ? image2 : image1) + (long long)n * 3 * HW;
        float* dst = pair ? image02 : image01;
        float t[12];
        loss_projection(intrinsics + (long long)n * 9, (pair ? pose02 : pose01) + (long long)n * 16, t);

        // ---- warp the tile and its halo into LDS; the owned pixels give the colour term and the optional image output
        float l1 = 0.f;
        for (int e = tid; e < LS_ZN; e += 256) {
            const int r = e / LS_ZW, c = e - r * LS_ZW;
            const int Y = y0 - 1 + r, X = x0 - 1 + c;
            float v0 = 0.f, v1 = 0.f, v2 = 0.f;
            if (Y >= 0 && Y < H && X >= 0 && X < W) {
                float ix, iy;
                loss_sample_position(kinv, t, (float)X, (float)Y, s_depth[e], wm1, hm1, ix, iy);
                // ix, iy are finite and inside [0, W-1] x [0, H-1] here; loss_taps clamps the addresses again as integers
                const LossTaps tp = loss_taps(ix, iy, W, H);
                const int xa = tp.xa, xb = tp.xb, ya = tp.ya, yb = tp.yb;
                const float wnw = tp.wnw, wne = tp.wne, wsw = tp.wsw, wse = tp.wse;
                const long long oa = (long long)ya * W, ob = (long long)yb * W;
                const float* s = src;
                v0 = s[oa + xa] * wnw + s[oa + xb] * wne + s[ob + xa] * wsw + s[ob + xb] * wse; s += HW;
                v1 = s[oa + xa] * wnw + s[oa + xb] * wne + s[ob + xa] * wsw + s[ob + xb] * wse; s += HW;
                v2 = s[oa + xa] * wnw + s[oa + xb] * wne + s[ob + xa] * wsw + s[ob + xb] * wse;
                if (r >= 1 && r <= LS_TH && c >= 1 && c <= LS_TW) {
                    l1 += fabsf(s_img0[0][e] - v0) + fabsf(s_img0[1][e] - v1) + fabsf(s_img0[2][e] - v2);
                    if (dst) {
                        float* o = dst + (long long)n * 3 * HW + (long long)Y * W + X;
                        o[0] = v0; o[HW] = v1; o[2 * HW] = v2;
                    }
                }
            }
            s_warp[0][e] = v0; s_warp[1][e] = v1; s_warp[2][e] = v2;
        }
        acc[pair] += (double)l1;
        __syncthreads();

        // ---- SSIM over 3 x 3 windows: a thread owns one column and 4 rows, so that the 6 row sums it forms serve 4 windows.
        // The moments are taken of x - bx, y - by (bx, by: one pixel of the strip): variances and the covariance do not change
        // with a shift, and without it E[x^2] - mu^2 cancels ~0.25 down to the ~1e-3 a smooth image's 3 x 3 window holds,
        // leaving fp32's rounding of 0.25 (1.5e-8) to stand against C2 = 9e-4.
        {
            const int c = tid & (LS_TW - 1), r0 = (tid >> 6) * LS_ROWS;
            const float wxv = s_wx[c];
            float ss = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float rx[LS_ROWS + 2], ry[LS_ROWS + 2], rxx[LS_ROWS + 2], ryy[LS_ROWS + 2], rxy[LS_ROWS + 2];
                const float bx = s_warp[ch][(r0 + 2) * LS_ZW + c + 1], by = s_img0[ch][(r0 + 2) * LS_ZW + c + 1];
#pragma unroll
                for (int j = 0; j < LS_ROWS + 2; ++j) {
                    const float* xr = &s_warp[ch][(r0 + j) * LS_ZW + c];
                    const float* yr = &s_img0[ch][(r0 + j) * LS_ZW + c];
                    const float xa = xr[0] - bx, xb = xr[1] - bx, xc = xr[2] - bx, ya = yr[0] - by, yb = yr[1] - by, yc = yr[2] - by;
                    rx[j] = xa + xb + xc;
                    ry[j] = ya + yb + yc;
                    rxx[j] = xa * xa + xb * xb + xc * xc;
                    ryy[j] = ya * ya + yb * yb + yc * yc;
                    rxy[j] = xa * ya + xb * yb + xc * yc;
                }
#pragma unroll
                for (int j = 0; j < LS_ROWS; ++j) {
                    const float wgt = s_wy[r0 + j] * wxv;
                    const float dx = (rx[j] + rx[j + 1] + rx[j + 2]) / 9.0f, dy = (ry[j] + ry[j + 1] + ry[j + 2]) / 9.0f;
                    const float mu_x = bx + dx, mu_y = by + dy;
                    const float mu_xy = mu_x * mu_y, mu_xx = mu_x * mu_x, mu_yy = mu_y * mu_y;
                    const float sg_x = (rxx[j] + rxx[j + 1] + rxx[j + 2]) / 9.0f - dx * dx;
                    const float sg_y = (ryy[j] + ryy[j + 1] + ryy[j + 2]) / 9.0f - dy * dy;
                    const float sg_xy = (rxy[j] + rxy[j + 1] + rxy[j + 2]) / 9.0f - dx * dy;
                    const float numer = (2.0f * mu_xy + 1e-4f) * (2.0f * sg_xy + 9e-4f);
                    const float denom = (mu_xx + mu_yy + 1e-4f) * (sg_x + sg_y + 9e-4f);
                    float v = (1.0f - numer / denom) / 2.0f;
                    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);   // torch.clamp keeps NaN; fminf(fmaxf()) would turn it into 0
                    if (wgt > 0.f) ss += v * wgt;
                }
            }
            acc[2 + pair] += (double)ss;
        }
        __syncthreads();   // the next frame's warp overwrites s_warp
    }

    // ---- sparse-depth term and edge-aware smoothness on the owned pixels
    {
        const float* sp = sparse + (long long)n * HW;
        const float* vl = validity + (long long)n * HW;
        float sd = 0.f, sv = 0.f, smx = 0.f, smy = 0.f;
        for (int e = tid; e < LS_TH * LS_TW; e += 256) {
            const int r = e / LS_TW, c = e - r * LS_TW;
            const int Y = y0 + r, X = x0 + c;
            if (Y >= H || X >= W) continue;
            const int q = (r + 1) * LS_ZW + c + 1;
            const long long o = (long long)Y * W + X;
            const float z = s_depth[q], v = vl[o];
            sd += v * fabsf(sp[o] - z);
            sv += v;
            const float a0 = s_img0[0][q], a1 = s_img0[1][q], a2 = s_img0[2][q];
            if (X < W - 1) {
                const float g = (fabsf(a0 - s_img0[0][q + 1]) + fabsf(a1 - s_img0[1][q + 1]) + fabsf(a2 - s_img0[2][q + 1])) / 3.0f;
                smx += expf(-g) * fabsf(z - s_depth[q + 1]);
            }
            if (Y < H - 1) {
                const float g = (fabsf(a0 - s_img0[0][q + LS_ZW]) + fabsf(a1 - s_img0[1][q + LS_ZW]) + fabsf(a2 - s_img0[2][q + LS_ZW])) / 3.0f;
                smy += expf(-g) * fabsf(z - s_depth[q + LS_ZW]);
            }
        }
        acc[4] = sd; acc[5] = sv; acc[6] = smx; acc[7] = smy;
    }

#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double a = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if ((tid & 63) == 0) s_red[tid >> 6][k] = a;
    }
    __syncthreads();
    if (tid < 8) atomicAdd(sums + (long long)n * 8 + tid, s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid]);
}

}  // namespace kbn

extern "C" int kbn_photometric_loss_forward(const float* image0, const float* image1, const float* image2,
                                            const float* output_depth, const float* sparse_depth, const float* validity_map,
                                            const float* intrinsics, const float* pose01, const float* pose02, double* sums,
                                            float* image01, float* image02, int n, int height, int width, kbn_stream_t stream) {
    using namespace kbn;
    if (!image0 || !image1 || !image2 || !output_depth || !sparse_depth || !validity_map || !intrinsics || !pose01 || !pose02 || !sums)
        return KBN_ERR_INVALID_ARGUMENT;
    if ((image01 == nullptr) != (image02 == nullptr)) return KBN_ERR_INVALID_ARGUMENT;
    if (n < 1 || height < 3 || width < 3) return KBN_ERR_INVALID_ARGUMENT;   // SSIM pools 3 x 3 without padding
    const int tilesX = ceil_div(width, LS_TW), tilesY = ceil_div(height, LS_TH);
    const long long blocks = (long long)tilesX * tilesY * n;
    if (blocks > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)n * 8 * sizeof(double), st) != hipSuccess) return KBN_ERR_LAUNCH;
    hipLaunchKernelGGL(photometric_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, st, image0, image1, image2, output_depth,
                       sparse_depth, validity_map, intrinsics, pose01, pose02, sums, image01, image02, height, width, tilesX, tilesY);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
