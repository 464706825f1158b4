// bn_sync.hip -- BatchNorm2d on batch statistics over the frames of SEVERAL ranks: the kernels on either side of the two collectives.
//
//   torch.nn.BatchNorm2d in train mode   reference src/net_utils.py:103-104, 128-141
//   under torch.nn.DataParallel          reference src/kbnet_model.py:408-415 -- there each replica normalises with its own shard's
//                                        statistics; here every rank normalises with the statistics of the whole batch, which is what
//                                        one process computes.
//
// Rank r holds n_r frames, c_r = n_r H W values per channel; M = sum c_r.
//   forward:   bn_moments_kernel           the rank's record (c_r, mean_r[C], q_r[C]) in fp64, q = sum (u - mean_r)^2     [gather]
//              bn_moments_merge_kernel     the gathered records merged in rank order with the pairwise update -> mean, q / M, q / (M - 1)
//   backward:  bn_bwd_sums_kernel          (posenet_backward.hip) s_r = (sum g_z, sum g_z xhat) in fp64                   [gather]
//              bn_bwd_sync_apply_kernel    S = sum_r (c_r / M) s_r in rank order; grad_u = scale (g_z - (S1 + xhat S2) / c_r)
// The divisor of the last line is the rank's OWN count: grad_u stays in the units of the rank's loss (the mean over its own frames),
// and the weights n_r / n that GradientAverager applies afterwards make the sum over ranks the global gradient.
//
// Everything between the ranks is fp64 and summed in rank order: every rank forms the same bits, whatever the backend's reduction
// order.  NO floating-point atomics; no host synchronisation (the counts travel in the records).
#include "bn_common.h"

namespace kbn {
namespace {

// record[0] = N HW, record[1 + c] = the mean of channel c = blockIdx.x, record[1 + C + c] = its sum of centred squares
__global__ __launch_bounds__(BN_RT) void bn_moments_kernel(const float* __restrict__ x, long long bs, double* __restrict__ record,
                                                           int N, int C, int HW) {
    __shared__ double red[2 * BN_RT / 64];
    const int c = blockIdx.x;
    double mu, q;
    bn_channel_moments(x + (long long)c * HW, bs, N, HW, red, mu, q);
    if (threadIdx.x == 0) {
        if (c == 0) record[0] = (double)N * (double)HW;
        record[1 + c] = mu;
        record[1 + C + c] = q;
    }
}

// one thread per channel: records 0 .. world - 1 (2 C + 1 doubles each) merged in that order
__global__ void bn_moments_merge_kernel(const double* __restrict__ records, int world, int C, float* __restrict__ mean,
                                        float* __restrict__ var, float* __restrict__ var_unbiased) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long long stride = 2LL * C + 1;
    double cnt = records[0], m = records[1 + c], q = records[1 + C + c];
    for (int r = 1; r < world; ++r) {
        const double* rec = records + r * stride;
        const double cb = rec[0], tot = cnt + cb;
        const double d = rec[1 + c] - m;
        m += d * cb / tot;
        q += rec[1 + C + c] + d * d * cnt * cb / tot;
        cnt = tot;
    }
    mean[c] = (float)m;
    var[c] = (float)(q / cnt);
    var_unbiased[c] = (float)(q / (cnt - 1.0));
}

// bn_bwd_apply_kernel (posenet_backward.hip) with the two sums taken over every rank's frames
__global__ void bn_bwd_sync_apply_kernel(const float* __restrict__ u, long long ubs, const float* __restrict__ gy, long long gybs,
                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                         const double* __restrict__ sums /* world x 2 C */,
                                         const double* __restrict__ records /* world x (2 C + 1): the counts */, int world, int rank,
                                         float* __restrict__ gu, long long gubs, int C, int HW, long long total, int act, float slope) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long plane = i / HW;
    const int rem = (int)(i - plane * HW);
    const int n = (int)(plane / C), c = (int)(plane - (long long)n * C);
    const long long off = (long long)c * HW + rem;
    const long long rstride = 2LL * C + 1;
    // S = sum_r c_r s_r / M with one division: the counts are whole numbers, M is exact
    double M = 0.0, s1 = 0.0, s2 = 0.0;
    for (int r = 0; r < world; ++r) {
        const double cr = records[r * rstride];
        M += cr;
        s1 += cr * sums[(long long)r * 2 * C + c];
        s2 += cr * sums[(long long)r * 2 * C + C + c];
    }
    const double count = records[rank * rstride];
    const float m1 = (float)(s1 / M / count), m2 = (float)(s2 / M / count);
    const float uv = u[(long long)n * ubs + off];
    const float sc = scale[c];
    const float gz = bn_gz(uv, gy[(long long)n * gybs + off], sc, shift[c], act, slope);
    const float xh = (uv - mean[c]) * rstd[c];
    gu[(long long)n * gubs + off] = sc * (gz - fmaf(xh, m2, m1));
}

}  // namespace
}  // namespace kbn

using namespace kbn;

extern "C" int kbn_bn_moments_forward(const float* x, long long batch_stride, double* record, int n, int channels, int height,
                                      int width, kbn_stream_t stream) {
    if (!x || !record) return KBN_ERR_INVALID_ARGUMENT;
    long long total = 0;
    if (!bn_shape_ok(n, channels, height, width, &total)) return KBN_ERR_INVALID_ARGUMENT;
    const long long hw = (long long)height * width;
    if (batch_stride < channels * hw && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(bn_moments_kernel, dim3((unsigned)channels), dim3(BN_RT), 0, (hipStream_t)stream, x, batch_stride, record, n,
                       channels, (int)hw);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_bn_moments_merge(const double* records, int world, int channels, float* mean, float* var, float* var_unbiased,
                                    kbn_stream_t stream) {
    if (!records || !mean || !var || !var_unbiased) return KBN_ERR_INVALID_ARGUMENT;
    if (world <= 0 || channels <= 0) return KBN_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(bn_moments_merge_kernel, dim3((unsigned)ceil_div(channels, 64)), dim3(64), 0, (hipStream_t)stream, records, world,
                       channels, mean, var, var_unbiased);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_bn_act_backward_sums(const float* u, long long u_batch_stride, const float* grad_y, long long grad_y_batch_stride,
                                        const float* scale, const float* shift, const float* mean, const float* rstd, double* sums,
                                        int n, int channels, int height, int width, int apply_activation, float negative_slope,
                                        kbn_stream_t stream) {
    if (!u || !grad_y || !scale || !shift || !mean || !rstd || !sums) return KBN_ERR_INVALID_ARGUMENT;
    long long total = 0;
    if (!bn_shape_ok(n, channels, height, width, &total)) return KBN_ERR_INVALID_ARGUMENT;
    const long long hw = (long long)height * width;
    if (n > 1 && (u_batch_stride < channels * hw || grad_y_batch_stride < channels * hw)) return KBN_ERR_INVALID_ARGUMENT;
    bn_bwd_sums_launch(u, u_batch_stride, grad_y, grad_y_batch_stride, scale, shift, mean, rstd, sums, n, channels, (int)hw,
                       apply_activation ? 1 : 0, negative_slope, (hipStream_t)stream);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_bn_act_backward_sync_apply(const float* u, long long u_batch_stride, const float* grad_y,
                                              long long grad_y_batch_stride, const float* scale, const float* shift, const float* mean,
                                              const float* rstd, const double* gathered_sums, const double* gathered_records, int world,
                                              int rank, float* grad_u, long long grad_u_batch_stride, int n, int channels, int height,
                                              int width, int apply_activation, float negative_slope, kbn_stream_t stream) {
    if (!u || !grad_y || !scale || !shift || !mean || !rstd || !gathered_sums || !gathered_records || !grad_u)
        return KBN_ERR_INVALID_ARGUMENT;
    if (world <= 0 || rank < 0 || rank >= world) return KBN_ERR_INVALID_ARGUMENT;
    long long total = 0;
    if (!bn_shape_ok(n, channels, height, width, &total)) return KBN_ERR_INVALID_ARGUMENT;
    const long long hw = (long long)height * width;
    if (n > 1 && (u_batch_stride < channels * hw || grad_y_batch_stride < channels * hw || grad_u_batch_stride < channels * hw))
        return KBN_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(bn_bwd_sync_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u,
                       u_batch_stride, grad_y, grad_y_batch_stride, scale, shift, mean, rstd, gathered_sums, gathered_records, world, rank,
                       grad_u, grad_u_batch_stride, channels, (int)hw, total, apply_activation ? 1 : 0, negative_slope);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
