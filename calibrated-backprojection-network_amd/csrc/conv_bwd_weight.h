// conv_bwd_weight.h -- what the two weight-gradient kernel families share: the tile constants, the launch parameters, the split
// plan and the launch that adds the split planes.
//   conv_s2_bwd_weight_kernel<KS, MB>        posenet_backward.hip       k in {3, 5, 7} at stride 2
//   conv_bwd_weight_kernel<KS, STRIDE, MB>   conv_affine_backward.hip   (3, 1), (1, 1), (1, 2)
// M = 16 MB filters, N = 64 (input channel, tap) columns, K = the output pixels of the batch in chunks of 32, split over grid.z.
// Host side and verbatim code only: each kernel keeps its own K loop (pose_igemm.h says why).
#pragma once

#include "pose_igemm.h"

namespace kbn {

constexpr int BW_BN = 64, BW_KC = 32, BW_BP = BW_BN + 17;
constexpr int BW_TARGET_WORKGROUPS = 512;   // two per CU of a 256-CU device; a constant, so that the split (and the bits) do not follow the device
constexpr int BW_MIN_CHUNKS = 4, BW_MAX_SPLITS = 1024;

__host__ __device__ inline int bw_mb(int oc) { return oc <= 16 ? 1 : (oc <= 32 ? 2 : 4); }
__host__ __device__ constexpr int bw_ap(int mb) { return mb == 1 ? 49 : 16 * mb + 17; }   // = 17 mod 32

struct BwParams {
    const float* g;
    long long gbs;
    const float* src0;
    const float* src1;
    long long bs0, bs1;
    int C0, Ctot;
    float* out;   // the weight gradient (one split) or the scratch planes
    int N, OC, H, W, OH, OW;
    int M;        // N * OH * OW
    int CK;       // Ctot k k
    int nchunks, cps;   // chunks of 32 pixels; chunks per split
};

static __global__ void sum_splits_kernel(const float* __restrict__ planes, float* __restrict__ out, long long total, int splits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float s = planes[i];
    for (int z = 1; z < splits; ++z) s += planes[(long long)z * total + i];   // split order, always
    out[i] = s;
}

struct BwPlan {
    int ok, OH, OW, M, CK, nchunks, cps, splits, mb;
    unsigned ntn, ntm;
};

// The caller has checked (ks, stride).  `splits` <= 0: chosen here (enough workgroups for the chip, at least BW_MIN_CHUNKS chunks
// each); > 0: as asked, at most one per chunk
inline BwPlan bwd_weight_plan(int n, int oc, int cin, int ks, int stride, int h, int w, int splits) {
    BwPlan pl{};
    if (n <= 0 || oc <= 0 || cin <= 0 || h <= 0 || w <= 0 || ks <= 0 || stride <= 0) return pl;
    pl.OH = ceil_div(h, stride);
    pl.OW = ceil_div(w, stride);
    const long long M = (long long)n * pl.OH * pl.OW;
    const long long CK = (long long)cin * ks * ks;
    if (M > 0x7fffffffLL - BW_KC || CK > (1 << 24) || (long long)h * w > 0x7fffffffLL || (long long)oc * CK > 0x7fffffffLL) return pl;
    pl.M = (int)M;
    pl.CK = (int)CK;
    pl.nchunks = ceil_div(pl.M, BW_KC);
    pl.mb = bw_mb(oc);
    pl.ntn = (unsigned)ceil_div(pl.CK, BW_BN);
    pl.ntm = (unsigned)ceil_div(oc, 16 * pl.mb);
    if (pl.ntm > 65535u) return pl;
    if (splits <= 0) {
        const long long tiles = (long long)pl.ntn * pl.ntm;
        long long s = (BW_TARGET_WORKGROUPS + tiles - 1) / tiles;
        s = s < pl.nchunks / BW_MIN_CHUNKS ? s : pl.nchunks / BW_MIN_CHUNKS;
        splits = (int)(s < 1 ? 1 : s);
    }
    if (splits > BW_MAX_SPLITS) splits = BW_MAX_SPLITS;
    if (splits > pl.nchunks) splits = pl.nchunks;
    pl.cps = ceil_div(pl.nchunks, splits);
    pl.splits = ceil_div(pl.nchunks, pl.cps);   // no empty split
    pl.ok = 1;
    return pl;
}

// The launch that ends a split weight gradient: grad_weight = the planes of `scratch` added in split order
inline void sum_splits_launch(const float* scratch, float* grad_weight, long long total, int splits, hipStream_t stream) {
    hipLaunchKernelGGL(sum_splits_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, scratch, grad_weight, total,
                       splits);
}

}  // namespace kbn
