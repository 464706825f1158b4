// pose_igemm.h -- what the pose networks' three gather-form implicit-GEMM convs share: the tile geometry, the straight-copy weight
// pack, the NB dispatch and the host-side source checks.
//   conv_s2_affine_kernel<KS, NB>          posenet.hip            K chunk 16, static LDS
//   conv_affine_kernel<KS, STRIDE, NB>     conv_affine.hip        K chunk 32, dynamic LDS
//   conv_s2_bwd_data_kernel<KS, NB>        posenet_backward.hip   K chunk 16, static LDS
// M = 128 pixels of the batch per workgroup, N = 16 NB channels (NB in {1, 2, 4}), LDS A[2][KC][144] + B[2][KC][BP] floats with
// pitches = 16 mod 32; each kernel's own comment explains its mapping.  The K loop itself is NOT here: folded into one
// __forceinline__ template with a gather functor it gave the same bits, LDS and occupancy but other register assignments, and
// the gathers then waited on in-flight loads more often (profiles/r10/pose_igemm_ab.md: the stride-2 kernels 1 - 8 % slower).
#pragma once

#include "kbn_common.h"

namespace kbn {

constexpr int PI_BM = 128, PI_AP = PI_BM + 16;

__host__ __device__ inline int pose_igemm_nb(int channels) { return channels <= 16 ? 1 : (channels <= 32 ? 2 : 4); }
__host__ __device__ constexpr int pose_igemm_bp(int nb) { return nb == 1 ? 16 : 16 * nb + 16; }
__host__ __device__ constexpr int pose_igemm_lds_floats(int kc, int nb) { return 2 * kc * (PI_AP + pose_igemm_bp(nb)); }

// ---- host side ------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, NB>) for the run-time nb in {1, 2, 4}
template <class F>
int dispatch_nb(int nb, F&& f) {
    switch (nb) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

// The one or two tensor sources of n frames of h x w that a pose conv reads in place; *ctot: their channels together.
inline int check_tensor_srcs(const kbn_conv_src* srcs, int n_src, int n, int h, int w, int* ctot) {
    *ctot = 0;
    for (int s = 0; s < n_src; ++s) {
        const kbn_conv_src& src = srcs[s];
        if (src.kind != KBN_SRC_TENSOR) return KBN_ERR_UNSUPPORTED;
        if (!src.data || src.channels <= 0) return KBN_ERR_INVALID_ARGUMENT;
        if (src.src_height != h || src.src_width != w) return KBN_ERR_INVALID_ARGUMENT;
        if (src.batch_stride < (long long)src.channels * h * w && n > 1) return KBN_ERR_INVALID_ARGUMENT;
        *ctot += src.channels;
    }
    return KBN_OK;
}

// Bytes of a weight of `cols` GEMM columns and K rows packed as [n-tile][K chunk][kc][16 NB]; 0: outside the common range of
// include/kbnet_hip.h (columns, K, or their product, the weight's elements)
inline size_t pose_igemm_packed_bytes(int cols, long long K, int kc) {
    if (cols < 1 || K < 1 || cols > KBN_MAX_CHANNELS || K > (1 << 24) || cols * K > (long long)KBN_MAX_WEIGHT_ELEMENTS) return 0;
    const int nb = pose_igemm_nb(cols);
    return (size_t)((long long)ceil_div(cols, 16 * nb) * round_up((int)K, kc) * (16 * nb)) * sizeof(float);
}

// OIHW -> [filter tile][K chunk][kc][16 NB filters], zero-padded: (c, ky, kx) is already the flat k, a straight copy
static __global__ void pose_igemm_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int oc, int K, int nchunks,
                                              int kc, int nb, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bn = 16 * nb;
    const int col = (int)(i % bn);
    const long long row = i / bn;                       // n-tile * (nchunks * kc) + k
    const int k = (int)(row % ((long long)nchunks * kc));
    const int nt = (int)(row / ((long long)nchunks * kc));
    const int o = nt * bn + col;
    packed[i] = (o < oc && k < K) ? w[(long long)o * K + k] : 0.f;
}

// The body of the two forward families' kbn_*_pack_weight: `bytes` = their kbn_*_packed_weight_bytes of the same arguments
inline int pose_igemm_pack_weight(const float* weight, float* packed, int out_channels, int in_channels, int kernel_size, int kc,
                                  size_t bytes, hipStream_t stream) {
    if (!weight || !packed) return KBN_ERR_INVALID_ARGUMENT;
    if (out_channels <= 0 || in_channels <= 0) return KBN_ERR_INVALID_ARGUMENT;
    if (bytes == 0) return KBN_ERR_UNSUPPORTED;
    const int K = in_channels * kernel_size * kernel_size;
    const long long total = (long long)(bytes / sizeof(float));
    hipLaunchKernelGGL(pose_igemm_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, weight, packed,
                       out_channels, K, ceil_div(K, kc), kc, pose_igemm_nb(out_channels), total);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

}  // namespace kbn
