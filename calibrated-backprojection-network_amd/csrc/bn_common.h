// bn_common.h -- what the two BatchNorm files share: posenet_backward.hip (the statistics and gradients of one process's batch) and
// bn_sync.hip (the same over the frames of several ranks).  The fp64 fixed-order block sum, a channel's two-pass moments, the
// activation's gradient factor; and, defined in posenet_backward.hip, the shape check and the launch of the backward's per-channel sums.
#pragma once

#include "kbn_common.h"

namespace kbn {

// ---- fixed-order block sum of two doubles (256 threads) -----------------------------------------------------------------
constexpr int BN_RT = 256;

__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds /* 2 * BN_RT / 64 doubles */) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();   // the previous use of `lds` is over
    if (lane == 0) {
        lds[wave] = a;
        lds[BN_RT / 64 + wave] = b;
    }
    __syncthreads();
    a = 0.0;
    b = 0.0;
#pragma unroll
    for (int w = 0; w < BN_RT / 64; ++w) {
        a += lds[w];
        b += lds[BN_RT / 64 + w];
    }
}

// mean and sum of centred squares of one channel (xc: its plane in frame 0, frames bs apart) over N, H, W, in every thread of a
// BN_RT-thread workgroup: two passes in fp64 (the mean, then the centred squares).
__device__ __forceinline__ void bn_channel_moments(const float* __restrict__ xc, long long bs, int N, int HW, double* red, double& mu,
                                                   double& q) {
    double s = 0.0, unused = 0.0;
    for (int n = 0; n < N; ++n) {
        const float* plane = xc + (long long)n * bs;
        for (int i = threadIdx.x; i < HW; i += BN_RT) s += (double)plane[i];
    }
    block_sum2(s, unused, red);
    mu = s / ((double)N * (double)HW);
    q = 0.0;
    for (int n = 0; n < N; ++n) {
        const float* plane = xc + (long long)n * bs;
        for (int i = threadIdx.x; i < HW; i += BN_RT) {
            const double d = (double)plane[i] - mu;
            q += d * d;
        }
    }
    block_sum2(q, unused, red);
}

// g_z = g_y (z > 0 ? 1 : slope), z = u scale + shift exactly as bn_act_kernel forms it; xhat = (u - mean) rstd
__device__ __forceinline__ float bn_gz(float u, float gy, float sc, float sh, int act, float slope) {
    if (!act) return gy;
    return fmaf(u, sc, sh) > 0.f ? gy : gy * slope;
}

// ---- host side, defined in posenet_backward.hip ---------------------------------------------------------------------------
// n, c, h, w positive and within what the elementwise kernels index: *total = n c h w
bool bn_shape_ok(int n, int c, int h, int w, long long* total);

// sums[c] = sum g_z, sums[C + c] = sum g_z xhat over N, H, W: one workgroup per channel, fp64, a fixed tree.  The caller has
// checked the arguments and checks the launch.
void bn_bwd_sums_launch(const float* u, long long ubs, const float* gy, long long gybs, const float* scale, const float* shift,
                        const float* mean, const float* rstd, double* sums, int n, int channels, int hw, int act, float slope,
                        hipStream_t stream);

}  // namespace kbn
