// posenet_backward.hip -- the backward pass of a PoseEncoder layer, and BatchNorm2d on batch statistics.
//
//   net_utils.Conv2d           reference src/net_utils.py:51-141    bias-free conv (stride 2, padding k / 2), BatchNorm2d, LeakyReLU
//   networks.PoseEncoder       reference src/networks.py:536-671    seven of them; src/kbnet.py:392-453 trains through them
//
// Everything is fp32 in and out; the matrix products run on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 sums), the
// per-channel sums of BatchNorm in fp64.  NO floating-point atomics: every sum has a fixed order, two runs give the same bits.
//
// conv_s2_bwd_data_kernel<KS, NB>: the gradient with respect to the conv's input, in GATHER form: the structure of
//   conv_s2_affine_kernel (posenet.hip) with the roles turned round.
//   M = every INPUT pixel of the batch, m = (frame * H + iy) * W + ix, 128 per workgroup;
//   N = input channels, 16 NB per workgroup;   K = (output channel, ky, kx), OC k k, zero-padded to a multiple of 16.
//   A[m][k] = g[frame, oc, (iy + k/2 - ky) / 2, (ix + k/2 - kx) / 2] where both numerators are even, non-negative and inside the
//   output map, else 0 BY PREDICATE (no address outside the planes is formed into a load).  This is the PREDICATED form: all k k
//   taps run and about three quarters of them multiply zeros (only taps of the pixel's parity meet it).
//   B = the weight in [n-tile][K chunk][16][16 NB] order with k = (oc, tap) and the column = input channel
//   (conv_s2_bwd_data_pack_kernel).  The epilogue writes channel c of the gradient to the first tensor (c < C0) or the second.
//
// The gradient with respect to the OIHW weight: conv_bwd_weight.hip (the one kernel family and host body of every conv's weight
//   gradient); kbn_conv2d_s2_backward_weight here is this file's case check (k in {3, 5, 7}, stride 2) in front of it.
//
// bn_stats_kernel, bn_bwd_sums_kernel: one workgroup per channel, fp64, a fixed tree.  bn_act_kernel, bn_bwd_apply_kernel: elementwise.
//   The block sum, the two-pass moments and g_z live in bn_common.h, which bn_sync.hip (the same over several ranks' frames) shares.
#include "bn_common.h"
#include "conv_bwd_weight.h"

namespace kbn {
namespace {

// ---- data gradient ------------------------------------------------------------------------------------------------------
constexpr int BD_KC = 16;

struct BdParams {
    const float* g;
    long long gbs;
    const float* wp;
    float* dst0;
    float* dst1;
    long long bs0, bs1;
    int C0, Ctot;
    int N, OC, H, W, OH, OW;
    int M;        // N * H * W
    int K, nchunks;
};

template <int KS, int NB>
__global__ __launch_bounds__(256) void conv_s2_bwd_data_kernel(const BdParams p) {
    constexpr int KK = KS * KS, PAD = KS / 2, BN = 16 * NB, BP = pose_igemm_bp(NB);
    __shared__ float As[2][BD_KC * PI_AP];
    __shared__ float Bs[2][BD_KC * BP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int mt = blockIdx.x, nt = blockIdx.y;
    const int HW = p.H * p.W, OHW = p.OH * p.OW;

    const int pm = tid & (PI_BM - 1);
    const int khalf = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int m = mt * PI_BM + pm;
    const bool mvalid = m < p.M;
    int fn = 0, iyp = 0, ixp = 0;
    if (mvalid) {
        fn = m / HW;
        const int rem = m - fn * HW;
        const int iy = rem / p.W, ix = rem - iy * p.W;
        iyp = iy + PAD;
        ixp = ix + PAD;
    }
    const float* gf = p.g + (long long)fn * p.gbs;
    const float* wtile = p.wp + (long long)nt * p.nchunks * (BD_KC * BN);

    float va[8];
    float vb[NB];
    auto load_chunk = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = chunk * BD_KC + khalf + 2 * j;      // wave-uniform
            const int oc = k / KK, t = k - oc * KK;
            const int ky = t / KS, kx = t - ky * KS;
            const int ty = iyp - ky, tx = ixp - kx;
            float v = 0.f;
            if (mvalid && k < p.K && ty >= 0 && tx >= 0 && ((ty | tx) & 1) == 0) {
                const int oy = ty >> 1, ox = tx >> 1;
                if (oy < p.OH && ox < p.OW) v = gf[(long long)oc * OHW + oy * p.OW + ox];
            }
            va[j] = v;
        }
        const float* wc = wtile + (long long)chunk * (BD_KC * BN);
#pragma unroll
        for (int j = 0; j < NB; ++j) vb[j] = wc[tid + 256 * j];
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 8; ++j) As[buf][(khalf + 2 * j) * PI_AP + pm] = va[j];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int e = tid + 256 * j;
            Bs[buf][(e / BN) * BP + (e % BN)] = vb[j];
        }
    };

    f32x4 acc[2][NB];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mi][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int chunk = 0; chunk < p.nchunks; ++chunk) {
        const int buf = chunk & 1;
        const bool more = chunk + 1 < p.nchunks;
        if (more) load_chunk(chunk + 1);
        const float* Ab = As[buf] + lk * PI_AP + wave * 32 + li;
        const float* Bb = Bs[buf] + lk * BP + li;
#pragma unroll
        for (int k4 = 0; k4 < BD_KC / 4; ++k4) {
            float a[2], b[NB];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[mi] = Ab[k4 * 4 * PI_AP + mi * 16];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) b[nb] = Bb[k4 * 4 * BP + nb * 16];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[mi][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi], b[nb], acc[mi][nb], 0, 0, 0);
        }
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // lane (li, lk) holds pixels 4 lk + r (r < 4) of each m-block for input channel li of each n-block
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c = nt * BN + nb * 16 + li;
        if (c >= p.Ctot) continue;
        const bool first = c < p.C0;
        float* base = first ? p.dst0 + (long long)c * HW : p.dst1 + (long long)(c - p.C0) * HW;
        const long long bs = first ? p.bs0 : p.bs1;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int om = mt * PI_BM + (wave * 2 + mi) * 16 + lk * 4 + r;
                if (om >= p.M) continue;
                const int n = om / HW, rem = om - n * HW;
                base[(long long)n * bs + rem] = acc[mi][nb][r];
            }
        }
    }
}

// OIHW -> [n-tile of input channels][k = (oc, tap), padded to chunks][16 NB input channels]
__global__ void conv_s2_bwd_data_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int cin, int kk, int K,
                                             int nchunks, int nb, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bn = 16 * nb;
    const int col = (int)(i % bn);
    const long long row = i / bn;
    const int k = (int)(row % ((long long)nchunks * BD_KC));
    const int nt = (int)(row / ((long long)nchunks * BD_KC));
    const int c = nt * bn + col;
    float v = 0.f;
    if (c < cin && k < K) {
        const int oc = k / kk, t = k - oc * kk;
        v = w[((long long)oc * cin + c) * kk + t];
    }
    packed[i] = v;
}

template <int KS>
int bwd_data_launch(const BdParams& p, int nb, dim3 grid, hipStream_t stream) {
    return dispatch_nb(nb, [&](auto nbc) {
        hipLaunchKernelGGL((conv_s2_bwd_data_kernel<KS, decltype(nbc)::value>), grid, dim3(256), 0, stream, p);
        return KBN_OK;
    });
}

bool ks_ok(int ks) { return ks == 3 || ks == 5 || ks == 7; }

// ---- BatchNorm2d --------------------------------------------------------------------------------------------------------
// mean and BIASED variance of channel blockIdx.x over N, H, W: two passes in fp64 (the mean, then the centred squares).
__global__ __launch_bounds__(BN_RT) void bn_stats_kernel(const float* __restrict__ x, long long bs, float* __restrict__ mean,
                                                         float* __restrict__ var, int N, int HW) {
    __shared__ double red[2 * BN_RT / 64];
    const int c = blockIdx.x;
    double mu, q;
    bn_channel_moments(x + (long long)c * HW, bs, N, HW, red, mu, q);
    if (threadIdx.x == 0) {
        mean[c] = (float)mu;
        var[c] = (float)(q / ((double)N * (double)HW));
    }
}

// y = act(u * scale[c] + shift[c])
__global__ void bn_act_kernel(const float* __restrict__ u, long long ubs, const float* __restrict__ scale,
                              const float* __restrict__ shift, float* __restrict__ y, long long ybs, int C, int HW, long long total,
                              int act, float slope) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long plane = i / HW;
    const int rem = (int)(i - plane * HW);
    const int n = (int)(plane / C), c = (int)(plane - (long long)n * C);
    float v = fmaf(u[(long long)n * ubs + (long long)c * HW + rem], scale[c], shift[c]);
    if (act) v = leaky_relu(v, slope);
    y[(long long)n * ybs + (long long)c * HW + rem] = v;
}

// sums[c] = sum g_z, sums[C + c] = sum g_z xhat over N, H, W of channel c = blockIdx.x: fp64, a fixed tree
__global__ __launch_bounds__(BN_RT) void bn_bwd_sums_kernel(const float* __restrict__ u, long long ubs, const float* __restrict__ gy,
                                                         long long gybs, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, double* __restrict__ sums, int N, int C,
                                                         int HW, int act, float slope) {
    __shared__ double red[2 * BN_RT / 64];
    const int c = blockIdx.x;
    const float sc = scale[c], sh = shift[c], mu = mean[c], rs = rstd[c];
    double s1 = 0.0, s2 = 0.0;
    for (int n = 0; n < N; ++n) {
        const float* up = u + (long long)n * ubs + (long long)c * HW;
        const float* gp = gy + (long long)n * gybs + (long long)c * HW;
        for (int i = threadIdx.x; i < HW; i += BN_RT) {
            const float uv = up[i];
            const float gz = bn_gz(uv, gp[i], sc, sh, act, slope);
            const float xh = (uv - mu) * rs;
            s1 += (double)gz;
            s2 += (double)gz * (double)xh;
        }
    }
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
        sums[c] = s1;
        sums[C + c] = s2;
    }
}

// g_u = scale (g_z - (sum g_z + xhat sum g_z xhat) / count) on batch statistics; g_u = scale g_z on running ones
__global__ void bn_bwd_apply_kernel(const float* __restrict__ u, long long ubs, const float* __restrict__ gy, long long gybs,
                                    const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
                                    const float* __restrict__ rstd, const double* __restrict__ sums, float* __restrict__ gu,
                                    long long gubs, int C, int HW, long long total, double count, int act, float slope, int batch) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long plane = i / HW;
    const int rem = (int)(i - plane * HW);
    const int n = (int)(plane / C), c = (int)(plane - (long long)n * C);
    const long long off = (long long)c * HW + rem;
    const float uv = u[(long long)n * ubs + off];
    const float sc = scale[c];
    float gz = bn_gz(uv, gy[(long long)n * gybs + off], sc, shift[c], act, slope);
    if (batch) {
        const float m1 = (float)(sums[c] / count), m2 = (float)(sums[C + c] / count);
        const float xh = (uv - mean[c]) * rstd[c];
        gz = gz - fmaf(xh, m2, m1);
    }
    gu[(long long)n * gubs + off] = sc * gz;
}

}  // namespace

bool bn_shape_ok(int n, int c, int h, int w, long long* total) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return false;
    const long long hw = (long long)h * w;
    if (hw > 0x7fffffffLL || (long long)n * c > 0x7fffffffLL) return false;
    *total = (long long)n * c * hw;
    return *total <= 0x7fffffffLL * 256LL;
}

void bn_bwd_sums_launch(const float* u, long long ubs, const float* gy, long long gybs, const float* scale, const float* shift,
                        const float* mean, const float* rstd, double* sums, int n, int channels, int hw, int act, float slope,
                        hipStream_t stream) {
    hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3((unsigned)channels), dim3(BN_RT), 0, stream, u, ubs, gy, gybs, scale, shift, mean, rstd,
                       sums, n, channels, hw, act, slope);
}

}  // namespace kbn

using namespace kbn;

extern "C" size_t kbn_conv2d_s2_backward_data_packed_weight_bytes(int out_channels, int in_channels, int kernel_size) {
    if (out_channels <= 0 || in_channels <= 0 || !ks_ok(kernel_size)) return 0;
    return pose_igemm_packed_bytes(in_channels, (long long)out_channels * kernel_size * kernel_size, BD_KC);
}

extern "C" int kbn_conv2d_s2_backward_data_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                                                       int kernel_size, kbn_stream_t stream) {
    if (!weight || !packed) return KBN_ERR_INVALID_ARGUMENT;
    if (out_channels <= 0 || in_channels <= 0) return KBN_ERR_INVALID_ARGUMENT;
    const size_t bytes = kbn_conv2d_s2_backward_data_packed_weight_bytes(out_channels, in_channels, kernel_size);
    if (bytes == 0) return KBN_ERR_UNSUPPORTED;
    const int kk = kernel_size * kernel_size, K = out_channels * kk;
    const long long total = (long long)(bytes / sizeof(float));
    hipLaunchKernelGGL(conv_s2_bwd_data_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       weight, packed, in_channels, kk, K, ceil_div(K, BD_KC), pose_igemm_nb(in_channels), total);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_conv2d_s2_backward_data(const float* grad_out, long long grad_out_batch_stride, const float* packed_weight,
                                           float* grad_in0, long long grad_in0_batch_stride, int channels0, float* grad_in1,
                                           long long grad_in1_batch_stride, int channels1, int n, int out_channels,
                                           int kernel_size, int in_height, int in_width, kbn_stream_t stream) {
    if (!grad_out || !packed_weight || !grad_in0) return KBN_ERR_INVALID_ARGUMENT;
    if (n <= 0 || out_channels <= 0 || in_height <= 0 || in_width <= 0 || channels0 <= 0 || channels1 < 0) return KBN_ERR_INVALID_ARGUMENT;
    if ((channels1 > 0) != (grad_in1 != nullptr)) return KBN_ERR_INVALID_ARGUMENT;
    if (!ks_ok(kernel_size)) return KBN_ERR_UNSUPPORTED;
    const long long HW = (long long)in_height * in_width;
    const long long M = (long long)n * HW;
    const long long K = (long long)out_channels * kernel_size * kernel_size;
    if (M > 0x7fffffffLL - PI_BM || K > (1 << 24)) return KBN_ERR_UNSUPPORTED;
    BdParams p{};
    p.OH = ceil_div(in_height, 2);
    p.OW = ceil_div(in_width, 2);
    if (n > 1) {
        if (grad_out_batch_stride < (long long)out_channels * p.OH * p.OW) return KBN_ERR_INVALID_ARGUMENT;
        if (grad_in0_batch_stride < channels0 * HW) return KBN_ERR_INVALID_ARGUMENT;
        if (channels1 > 0 && grad_in1_batch_stride < channels1 * HW) return KBN_ERR_INVALID_ARGUMENT;
    }
    p.g = grad_out;
    p.gbs = grad_out_batch_stride;
    p.wp = packed_weight;
    p.dst0 = grad_in0;
    p.dst1 = grad_in1;
    p.bs0 = grad_in0_batch_stride;
    p.bs1 = grad_in1_batch_stride;
    p.C0 = channels0;
    p.Ctot = channels0 + channels1;
    p.N = n;
    p.OC = out_channels;
    p.H = in_height;
    p.W = in_width;
    p.M = (int)M;
    p.K = (int)K;
    if (pose_igemm_packed_bytes(p.Ctot, K, BD_KC) == 0) return KBN_ERR_UNSUPPORTED;   // no blob exists for this shape
    p.nchunks = ceil_div((int)K, BD_KC);
    const int nb = pose_igemm_nb(p.Ctot);
    const unsigned ntn = (unsigned)ceil_div(p.Ctot, 16 * nb);
    if (ntn > 65535u) return KBN_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)ceil_div((int)M, PI_BM), ntn);
    switch (kernel_size) {
        case 3: bwd_data_launch<3>(p, nb, grid, (hipStream_t)stream); break;
        case 5: bwd_data_launch<5>(p, nb, grid, (hipStream_t)stream); break;
        default: bwd_data_launch<7>(p, nb, grid, (hipStream_t)stream); break;
    }
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

// ---- weight gradient: conv_bwd_weight.hip behind this file's case check, the stride fixed at 2 ----------------------------
extern "C" size_t kbn_conv2d_s2_backward_weight_scratch_bytes(int n, int out_channels, int in_channels, int kernel_size,
                                                              int in_height, int in_width, int splits) {
    if (!ks_ok(kernel_size)) return 0;
    return conv_bwd_weight_scratch_bytes(n, out_channels, in_channels, kernel_size, 2, in_height, in_width, splits);
}

extern "C" int kbn_conv2d_s2_backward_weight(const kbn_conv_src* srcs, int n_src, const float* grad_out,
                                             long long grad_out_batch_stride, float* grad_weight, int n, int out_channels,
                                             int kernel_size, int in_height, int in_width, int splits, float* scratch,
                                             size_t scratch_bytes, kbn_stream_t stream) {
    return conv_bwd_weight(ks_ok(kernel_size), srcs, n_src, grad_out, grad_out_batch_stride, grad_weight, n, out_channels, kernel_size, 2,
                           in_height, in_width, splits, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int kbn_bn_stats_forward(const float* x, long long batch_stride, float* mean, float* var, int n, int channels,
                                    int height, int width, kbn_stream_t stream) {
    if (!x || !mean || !var) return KBN_ERR_INVALID_ARGUMENT;
    long long total = 0;
    if (!bn_shape_ok(n, channels, height, width, &total)) return KBN_ERR_INVALID_ARGUMENT;
    const long long hw = (long long)height * width;
    if (batch_stride < channels * hw && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)channels), dim3(BN_RT), 0, (hipStream_t)stream, x, batch_stride, mean, var, n,
                       (int)hw);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_bn_act_forward(const float* u, long long u_batch_stride, const float* scale, const float* shift, float* y,
                                  long long y_batch_stride, int n, int channels, int height, int width, int apply_activation,
                                  float negative_slope, kbn_stream_t stream) {
    if (!u || !scale || !shift || !y) return KBN_ERR_INVALID_ARGUMENT;
    long long total = 0;
    if (!bn_shape_ok(n, channels, height, width, &total)) return KBN_ERR_INVALID_ARGUMENT;
    const long long hw = (long long)height * width;
    if (n > 1 && (u_batch_stride < channels * hw || y_batch_stride < channels * hw)) return KBN_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(bn_act_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u, u_batch_stride,
                       scale, shift, y, y_batch_stride, channels, (int)hw, total, apply_activation ? 1 : 0, negative_slope);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_bn_act_backward(const float* u, long long u_batch_stride, const float* grad_y, long long grad_y_batch_stride,
                                   const float* scale, const float* shift, const float* mean, const float* rstd, double* sums,
                                   float* grad_u, long long grad_u_batch_stride, int n, int channels, int height, int width,
                                   int apply_activation, float negative_slope, int batch_statistics, kbn_stream_t stream) {
    if (!u || !grad_y || !scale || !shift || !mean || !rstd || !sums || !grad_u) return KBN_ERR_INVALID_ARGUMENT;
    long long total = 0;
    if (!bn_shape_ok(n, channels, height, width, &total)) return KBN_ERR_INVALID_ARGUMENT;
    const long long hw = (long long)height * width;
    if (n > 1 && (u_batch_stride < channels * hw || grad_y_batch_stride < channels * hw || grad_u_batch_stride < channels * hw))
        return KBN_ERR_INVALID_ARGUMENT;
    const int act = apply_activation ? 1 : 0;
    bn_bwd_sums_launch(u, u_batch_stride, grad_y, grad_y_batch_stride, scale, shift, mean, rstd, sums, n, channels, (int)hw, act,
                       negative_slope, (hipStream_t)stream);
    KBN_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u,
                       u_batch_stride, grad_y, grad_y_batch_stride, scale, shift, mean, rstd, sums, grad_u, grad_u_batch_stride,
                       channels, (int)hw, total, (double)n * (double)hw, act, negative_slope, batch_statistics ? 1 : 0);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
