// conv_affine_backward.hip -- the backward pass of the ResNet-18/34 pose networks' layers that posenet_backward.hip does not have.
//
//   net_utils.ResNetBlock      reference src/net_utils.py:572-667    act(act(bn(conv2(act(bn(conv1(x)))))) + X), X = x or a 1 x 1 projection
//   networks.ResNetEncoder     reference src/networks.py:674-996     conv1, MaxPool2d(3, 2, 1), blocks2 .. blocks5; src/kbnet.py:392-453 trains it
//
// fp32 in and out; NO floating-point atomics: every sum has a fixed order, two runs give the same bits.  The stride-2 3 x 3 and 7 x 7
// convs keep the gradients of posenet_backward.hip; BatchNorm2d keeps its kernels there too.
//
// The OIHW weight gradient for (k, stride) in {(3, 1), (1, 1), (1, 2)}: conv_bwd_weight.hip (the one kernel family and host body of
//   every conv's weight gradient); kbn_conv2d_backward_weight here is this file's case check in front of it.
//
// The data gradient at stride 1 (k odd, padding k / 2) IS the forward conv of grad_out with the weight transposed (O <-> I) and both
//   tap axes flipped: conv_bwd_data_pack_kernel writes that weight in conv_affine_kernel's packed order, with the unit scale and
//   the zero shift behind it, and kbn_conv2d_backward_data calls kbn_conv2d_affine_forward.  No second stride-1 implicit GEMM.
//
// conv1x1s2_bwd_data_kernel: the 1 x 1 stride-2 projection.  One thread per (frame, input channel, output pixel) = per 2 x 2 cell of
//   the input map: W^T g goes to the even-even pixel, zeros to the cell's other pixels inside the map -- every element of the
//   result is written by exactly one thread, nothing is cleared beforehand.
//
// maxpool3x3s2_bwd_kernel: gather form, one thread per input pixel: for each of the at most four windows that hold it, in (oy, ox)
//   order, the window is rescanned with the forward's rule (v > m || isnan(v), row-major, padding never wins) and the window's
//   gradient is added if its first maximum is this pixel.  No atomics, no index tensor.
//
// add_act_kernel / add_act_bwd_kernel: y = act(a + b); g = grad_y where y > 0, slope grad_y elsewhere (the slope branch AT 0).
#include "conv_bwd_weight.h"

namespace kbn {
namespace {

constexpr int CA_KC = 32;   // conv_affine.hip's K chunk: the packed order of the stride-1 data gradient's weight

bool bw_case_ok(int ks, int stride) { return (ks == 3 && stride == 1) || (ks == 1 && (stride == 1 || stride == 2)); }

// ---- data gradient ------------------------------------------------------------------------------------------------------
// OIHW -> conv_affine_kernel's [tile of input channels][K chunk][CA_KC][16 NB] with k = (filter, ky, kx) and the taps flipped:
// the weight of the forward conv that IS the stride-1 data gradient.  Behind it: `cin` ones (scale), `cin` zeros (shift).
__global__ void conv_bwd_data_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int oc, int cin, int kk, int nchunks,
                                          int nb, long long blob, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (i >= blob) {
        packed[i] = i < blob + cin ? 1.f : 0.f;
        return;
    }
    const int bn = 16 * nb;
    const int col = (int)(i % bn);
    const long long row = i / bn;
    const int k = (int)(row % ((long long)nchunks * CA_KC));
    const int nt = (int)(row / ((long long)nchunks * CA_KC));
    const int c = nt * bn + col;
    float v = 0.f;
    if (c < cin && k < oc * kk) {
        const int o = k / kk, t = k - o * kk;
        v = w[((long long)o * cin + c) * kk + (kk - 1 - t)];
    }
    packed[i] = v;
}

// grad_in[n, c, 2 oy, 2 ox] = sum_o W[o, c] g[n, o, oy, ox]; the other pixels of the 2 x 2 cell inside the map: 0
__global__ __launch_bounds__(256) void conv1x1s2_bwd_data_kernel(const float* __restrict__ g, long long gbs, const float* __restrict__ w,
                                                                 float* __restrict__ out, long long obs, int OC, int C, int H, int W,
                                                                 int OH, int OW, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % OW);
    long long t = i / OW;
    const int oy = (int)(t % OH);
    t /= OH;
    const int c = (int)(t % C);
    const long long n = t / C;
    const int OHW = OH * OW;
    const float* gp = g + n * gbs + oy * OW + ox;
    float s = 0.f;
    for (int o = 0; o < OC; ++o) s = fmaf(w[(long long)o * C + c], gp[(long long)o * OHW], s);   // filter order, always
    const int iy = 2 * oy, ix = 2 * ox;
    float* o = out + n * obs + ((long long)c * H + iy) * W + ix;
    const bool right = ix + 1 < W, below = iy + 1 < H;
    o[0] = s;
    if (right) o[1] = 0.f;
    if (below) {
        o[W] = 0.f;
        if (right) o[W + 1] = 0.f;
    }
}

// ---- max pool -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const float* __restrict__ x, long long xbs, const float* __restrict__ g,
                                                               long long gbs, float* __restrict__ out, long long obs, int C, int H,
                                                               int W, int OH, int OW, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ix = (int)(i % W);
    long long t = i / W;
    const int iy = (int)(t % H);
    t /= H;
    const int c = (int)(t % C);
    const long long n = t / C;
    const float* plane = x + n * xbs + (long long)c * H * W;
    const float* gp = g + n * gbs + (long long)c * OH * OW;
    const int me = iy * W + ix;
    float s = 0.f;
    // the windows of rows oy hold input rows 2 oy - 1 .. 2 oy + 1: an even row lies in one, an odd row in two
    for (int oy = iy >> 1; oy <= ((iy + 1) >> 1) && oy < OH; ++oy) {
        for (int ox = ix >> 1; ox <= ((ix + 1) >> 1) && ox < OW; ++ox) {
            float m = -__builtin_inff();
            int at = -1;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int y = 2 * oy - 1 + ky;
                if (y < 0 || y >= H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = 2 * ox - 1 + kx;
                    if (xx < 0 || xx >= W) continue;
                    const float v = plane[y * W + xx];
                    if (v > m || v != v) {
                        m = v;
                        at = y * W + xx;
                    }
                }
            }
            if (at == me) s += gp[oy * OW + ox];
        }
    }
    out[n * obs + (long long)c * H * W + me] = s;
}

// ---- the block's add ------------------------------------------------------------------------------------------------------
__global__ void add_act_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, long long total, int act,
                               float slope) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float v = a[i] + b[i];
    y[i] = act ? leaky_relu(v, slope) : v;
}

__global__ void add_act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gy, float* __restrict__ g, long long total,
                                   int act, float slope) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float v = gy[i];
    g[i] = (!act || y[i] > 0.f) ? v : v * slope;
}

constexpr long long MAX_ELEMENTS = 0x7fffffffLL * 256LL;   // blocks of 256 threads in grid.x

}  // namespace
}  // namespace kbn

using namespace kbn;

// ---- weight gradient: conv_bwd_weight.hip behind this file's case check ---------------------------------------------------
extern "C" size_t kbn_conv2d_backward_weight_scratch_bytes(int n, int out_channels, int in_channels, int kernel_size, int stride,
                                                           int in_height, int in_width, int splits) {
    if (!bw_case_ok(kernel_size, stride)) return 0;
    return conv_bwd_weight_scratch_bytes(n, out_channels, in_channels, kernel_size, stride, in_height, in_width, splits);
}

extern "C" int kbn_conv2d_backward_weight(const kbn_conv_src* srcs, int n_src, const float* grad_out, long long grad_out_batch_stride,
                                          float* grad_weight, int n, int out_channels, int kernel_size, int stride, int in_height,
                                          int in_width, int splits, float* scratch, size_t scratch_bytes, kbn_stream_t stream) {
    return conv_bwd_weight(bw_case_ok(kernel_size, stride), srcs, n_src, grad_out, grad_out_batch_stride, grad_weight, n, out_channels,
                           kernel_size, stride, in_height, in_width, splits, scratch, scratch_bytes, (hipStream_t)stream);
}

static bool bd_case_ok(int ks, int stride) { return bw_case_ok(ks, stride); }

extern "C" size_t kbn_conv2d_backward_data_packed_weight_bytes(int out_channels, int in_channels, int kernel_size, int stride) {
    if (!kbn::layer_shape_ok(out_channels, in_channels, kernel_size) || !bd_case_ok(kernel_size, stride)) return 0;
    if (stride == 2) return (long long)out_channels * in_channels > 0x7fffffffLL ? 0 : (size_t)out_channels * in_channels * sizeof(float);
    // the forward conv of grad_out: `in_channels` filters over `out_channels` channels, and its scale and shift vectors
    const size_t blob = kbn_conv2d_affine_packed_weight_bytes(in_channels, out_channels, kernel_size);
    return blob ? blob + 2 * (size_t)in_channels * sizeof(float) : 0;
}

extern "C" int kbn_conv2d_backward_data_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                                                    int kernel_size, int stride, kbn_stream_t stream) {
    if (!weight || !packed) return KBN_ERR_INVALID_ARGUMENT;
    if (out_channels <= 0 || in_channels <= 0) return KBN_ERR_INVALID_ARGUMENT;
    const size_t bytes = kbn_conv2d_backward_data_packed_weight_bytes(out_channels, in_channels, kernel_size, stride);
    if (bytes == 0) return KBN_ERR_UNSUPPORTED;
    if (stride == 2) {   // the 1 x 1 projection's kernel reads the weight as it is
        if (hipMemcpyAsync(packed, weight, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return KBN_ERR_LAUNCH;
        return KBN_OK;
    }
    const int kk = kernel_size * kernel_size;
    const long long total = (long long)(bytes / sizeof(float));
    const long long blob = total - 2LL * in_channels;
    hipLaunchKernelGGL(conv_bwd_data_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, weight,
                       packed, out_channels, in_channels, kk, ceil_div(out_channels * kk, CA_KC), pose_igemm_nb(in_channels), blob,
                       total);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_conv2d_backward_data(const float* grad_out, long long grad_out_batch_stride, const float* packed_weight,
                                        float* grad_in, long long grad_in_batch_stride, int n, int out_channels, int in_channels,
                                        int kernel_size, int stride, int in_height, int in_width, kbn_stream_t stream) {
    if (!grad_out || !packed_weight || !grad_in) return KBN_ERR_INVALID_ARGUMENT;
    if (n <= 0 || out_channels <= 0 || in_channels <= 0 || in_height <= 0 || in_width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    if (!bd_case_ok(kernel_size, stride)) return KBN_ERR_UNSUPPORTED;
    const size_t bytes = kbn_conv2d_backward_data_packed_weight_bytes(out_channels, in_channels, kernel_size, stride);
    if (bytes == 0) return KBN_ERR_UNSUPPORTED;
    const int oh = ceil_div(in_height, stride), ow = ceil_div(in_width, stride);
    if (n > 1 && (grad_out_batch_stride < (long long)out_channels * oh * ow ||
                  grad_in_batch_stride < (long long)in_channels * in_height * in_width))
        return KBN_ERR_INVALID_ARGUMENT;
    if (stride == 1) {
        kbn_conv_src src{};
        src.kind = KBN_SRC_TENSOR;
        src.channels = out_channels;
        src.data = grad_out;
        src.batch_stride = grad_out_batch_stride;
        src.src_height = in_height;
        src.src_width = in_width;
        const float* scale = packed_weight + (bytes / sizeof(float) - 2 * (size_t)in_channels);
        return kbn_conv2d_affine_forward(&src, 1, packed_weight, scale, scale + in_channels, nullptr, 0, grad_in, grad_in_batch_stride, n,
                                         in_channels, kernel_size, 1, in_height, in_width, 0, 0.f, stream);
    }
    if ((long long)in_height * in_width > 0x7fffffffLL || (long long)oh * ow > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    if ((long long)in_channels * oh * ow > MAX_ELEMENTS / n) return KBN_ERR_UNSUPPORTED;
    const long long total = (long long)n * in_channels * oh * ow;
    hipLaunchKernelGGL(conv1x1s2_bwd_data_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_out,
                       grad_out_batch_stride, packed_weight, grad_in, grad_in_batch_stride, out_channels, in_channels, in_height,
                       in_width, oh, ow, total);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_maxpool3x3s2_backward(const float* x, long long x_batch_stride, const float* grad_out,
                                         long long grad_out_batch_stride, float* grad_in, long long grad_in_batch_stride, int n,
                                         int channels, int height, int width, kbn_stream_t stream) {
    if (!x || !grad_out || !grad_in) return KBN_ERR_INVALID_ARGUMENT;
    if (n <= 0 || channels <= 0 || height <= 0 || width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    const long long hw = (long long)height * width;
    if (hw > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    const int oh = ceil_div(height, 2), ow = ceil_div(width, 2);
    if (n > 1 && (x_batch_stride < channels * hw || grad_in_batch_stride < channels * hw ||
                  grad_out_batch_stride < (long long)channels * oh * ow))
        return KBN_ERR_INVALID_ARGUMENT;
    if (channels * hw > MAX_ELEMENTS / n) return KBN_ERR_UNSUPPORTED;
    const long long total = (long long)n * channels * hw;
    hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                       x_batch_stride, grad_out, grad_out_batch_stride, grad_in, grad_in_batch_stride, channels, height, width, oh, ow,
                       total);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_add_act_forward(const float* a, const float* b, float* y, long long count, int apply_activation,
                                   float negative_slope, kbn_stream_t stream) {
    if (!a || !b || !y) return KBN_ERR_INVALID_ARGUMENT;
    if (count <= 0 || count > MAX_ELEMENTS) return KBN_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(add_act_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, y, count,
                       apply_activation ? 1 : 0, negative_slope);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_add_act_backward(const float* y, const float* grad_y, float* grad, long long count, int apply_activation,
                                    float negative_slope, kbn_stream_t stream) {
    if (!y || !grad_y || !grad) return KBN_ERR_INVALID_ARGUMENT;
    if (count <= 0 || count > MAX_ELEMENTS) return KBN_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(add_act_bwd_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, grad_y, grad,
                       count, apply_activation ? 1 : 0, negative_slope);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
