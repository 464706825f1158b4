// kbnet_backward.hip -- what the depth network's backward pass needs beside the conv gradients of csrc/posenet_backward.hip and
// csrc/conv_affine_backward.hip (KBNetModel(trainable=True), kbnet_train.py):
//   kbn_resize_nearest_forward / _backward   the nearest resize in front of an up-conv (reference src/net_utils.py:484-499) as a tensor
//                                            of its own, and its gradient as a GATHER: a source pixel sums the destination pixels that
//                                            nearest_src_index (kbn_common.h, the rule the forward convs resize by) maps to it
//   kbn_kb_xyz_backward                      z = act(proj_depth(depth)), xyz = coordinates * z (src/net_utils.py:1352-1359):
//                                            g_pre = act'(z) * sum_c coordinates_c g_xyz_c
//   kbn_depth_map_backward                   depth = d_min / (sigmoid(l) + d_min / d_max) (src/kbnet_model.py:181-184):
//                                            g_l = -g_depth depth^2 / d_min * s (1 - s)
// All byte-bound: one read of every input and one write of every output element, 16-byte accesses where the planes allow with a
// scalar form for the rest.  No atomics, nothing cleared beforehand, every output element written exactly once; sums in a fixed order.
#include <math.h>

#include "kbn_common.h"

namespace kbn {

constexpr long long KT_MAX_ITEMS = 0x7fffffffLL * 256LL;   // blocks of 256 threads in grid.x

// [lo, hi): the destination indices d with nearest_src_index(d, in_size, out_size) == s.  The rule is monotone in d (a float product
// and a floor), so both ends are binary searches over it: the rule itself is stated once, in kbn_common.h.
__device__ __forceinline__ int nearest_first_at_least(int s, int in_size, int out_size) {
    int a = 0, b = out_size;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (nearest_src_index(m, in_size, out_size) < s) a = m + 1;
        else b = m;
    }
    return a;
}
__device__ __forceinline__ void nearest_dst_range(int s, int in_size, int out_size, int& lo, int& hi) {
    lo = nearest_first_at_least(s, in_size, out_size);
    hi = nearest_first_at_least(s + 1, in_size, out_size);
}

// one thread per V destination pixels of a row
template <int V>
__global__ __launch_bounds__(256) void resize_nearest_fwd_kernel(const float* __restrict__ x, long long x_bs, float* __restrict__ out,
                                                                 long long out_bs, int C, int h, int w, int H, int W, long long total) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int Wq = W / V;
    const int xq = (int)(id % Wq);
    long long r = id / Wq;
    const int Y = (int)(r % H);
    r /= H;
    const int c = (int)(r % C), n = (int)(r / C);
    const float* src = x + (long long)n * x_bs + (long long)c * h * w + (long long)nearest_src_index(Y, h, H) * w;
    float* dst = out + (long long)n * out_bs + (long long)c * H * W + (long long)Y * W + xq * V;
    if constexpr (V == 4) {
        float4 v;
        v.x = src[nearest_src_index(xq * 4 + 0, w, W)];
        v.y = src[nearest_src_index(xq * 4 + 1, w, W)];
        v.z = src[nearest_src_index(xq * 4 + 2, w, W)];
        v.w = src[nearest_src_index(xq * 4 + 3, w, W)];
        *reinterpret_cast<float4*>(dst) = v;
    } else {
        dst[0] = src[nearest_src_index(xq, w, W)];
    }
}

// one thread per V source pixels of a row: each sums its destination pixels in row-major order
template <int V>
__global__ __launch_bounds__(256) void resize_nearest_bwd_kernel(const float* __restrict__ g, long long g_bs, float* __restrict__ gin,
                                                                 long long gin_bs, int C, int h, int w, int H, int W, long long total) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int wq = w / V;
    const int xq = (int)(id % wq);
    long long r = id / wq;
    const int y = (int)(r % h);
    r /= h;
    const int c = (int)(r % C), n = (int)(r / C);
    const float* gp = g + (long long)n * g_bs + (long long)c * H * W;
    float* dst = gin + (long long)n * gin_bs + (long long)c * h * w + (long long)y * w + xq * V;
    int ylo, yhi;
    nearest_dst_range(y, h, H, ylo, yhi);
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        int xlo, xhi;
        nearest_dst_range(xq * V + j, w, W, xlo, xhi);
        float s = 0.f;
        for (int Y = ylo; Y < yhi; ++Y)
            for (int X = xlo; X < xhi; ++X) s += gp[(long long)Y * W + X];
        acc[j] = s;
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else dst[0] = acc[0];
}

__device__ __forceinline__ float kb_xyz_grad(float z, float c0, float c1, float c2, float g0, float g1, float g2, int act, float slope) {
    float s = c0 * g0;
    s = fmaf(c1, g1, s);
    s = fmaf(c2, g2, s);
    return (!act || z > 0.f) ? s : slope * s;   // z <= 0 takes the slope, as kbn_add_act_backward
}

// one thread per V pixels of a frame's plane
template <int V>
__global__ __launch_bounds__(256) void kb_xyz_bwd_kernel(const float* __restrict__ z, long long z_bs, const float* __restrict__ coords,
                                                         long long c_bs, const float* __restrict__ g, long long g_bs,
                                                         float* __restrict__ out, long long out_bs, long long plane, long long per_frame,
                                                         long long total, int act, float slope) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const long long n = id / per_frame, i = (id - n * per_frame) * V;
    const float* zn = z + n * z_bs + i;
    const float* cn = coords + n * c_bs + i;
    const float* gn = g + n * g_bs + i;
    float* on = out + n * out_bs + i;
    if constexpr (V == 4) {
        const float4 zv = *reinterpret_cast<const float4*>(zn);
        const float4 c0 = *reinterpret_cast<const float4*>(cn), c1 = *reinterpret_cast<const float4*>(cn + plane),
                     c2 = *reinterpret_cast<const float4*>(cn + 2 * plane);
        const float4 g0 = *reinterpret_cast<const float4*>(gn), g1 = *reinterpret_cast<const float4*>(gn + plane),
                     g2 = *reinterpret_cast<const float4*>(gn + 2 * plane);
        float4 o;
        o.x = kb_xyz_grad(zv.x, c0.x, c1.x, c2.x, g0.x, g1.x, g2.x, act, slope);
        o.y = kb_xyz_grad(zv.y, c0.y, c1.y, c2.y, g0.y, g1.y, g2.y, act, slope);
        o.z = kb_xyz_grad(zv.z, c0.z, c1.z, c2.z, g0.z, g1.z, g2.z, act, slope);
        o.w = kb_xyz_grad(zv.w, c0.w, c1.w, c2.w, g0.w, g1.w, g2.w, act, slope);
        *reinterpret_cast<float4*>(on) = o;
    } else {
        on[0] = kb_xyz_grad(zn[0], cn[0], cn[plane], cn[2 * plane], gn[0], gn[plane], gn[2 * plane], act, slope);
    }
}

// s (1 - s) = e / (1 + e)^2 with e = exp(-|l|): no cancellation where the sigmoid saturates
__device__ __forceinline__ float depth_map_grad(float l, float d, float g, float dmin) {
    const float e = expf(-fabsf(l));
    const float t = 1.0f / (1.0f + e);
    return -(g * d * d / dmin) * (e * t * t);
}

template <bool VEC>
__global__ __launch_bounds__(256) void depth_map_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ depth,
                                                            const float* __restrict__ g, float* __restrict__ out, long long count,
                                                            float dmin) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if constexpr (VEC) {
        const long long quads = count >> 2;
        if (id < quads) {
            const float4 l = reinterpret_cast<const float4*>(logits)[id], d = reinterpret_cast<const float4*>(depth)[id],
                         gv = reinterpret_cast<const float4*>(g)[id];
            float4 o;
            o.x = depth_map_grad(l.x, d.x, gv.x, dmin);
            o.y = depth_map_grad(l.y, d.y, gv.y, dmin);
            o.z = depth_map_grad(l.z, d.z, gv.z, dmin);
            o.w = depth_map_grad(l.w, d.w, gv.w, dmin);
            reinterpret_cast<float4*>(out)[id] = o;
        } else {
            const long long i = (quads << 2) + (id - quads);   // the scalar tail: at most three elements
            if (i < count) out[i] = depth_map_grad(logits[i], depth[i], g[i], dmin);
        }
    } else {
        if (id < count) out[id] = depth_map_grad(logits[id], depth[id], g[id], dmin);
    }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks the two resize entries share -> KBN_OK, or the status to return
static int resize_args(const void* a, const void* b, long long small_bs, long long large_bs, int n, int channels, int in_height,
                       int in_width, int out_height, int out_width) {
    if (!a || !b) return KBN_ERR_INVALID_ARGUMENT;
    if (n <= 0 || channels <= 0 || in_height <= 0 || in_width <= 0 || out_height <= 0 || out_width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    if (out_height < in_height || out_width < in_width) return KBN_ERR_UNSUPPORTED;
    const long long hw = (long long)in_height * in_width, HW = (long long)out_height * out_width;
    if (HW > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    if (n > 1 && (small_bs < channels * hw || large_bs < channels * HW)) return KBN_ERR_INVALID_ARGUMENT;
    if (channels * HW > KT_MAX_ITEMS / n) return KBN_ERR_UNSUPPORTED;
    return KBN_OK;
}

}  // namespace kbn

extern "C" int kbn_resize_nearest_forward(const float* in, long long in_batch_stride, float* out, long long out_batch_stride, int n,
                                          int channels, int in_height, int in_width, int out_height, int out_width,
                                          kbn_stream_t stream) {
    using namespace kbn;
    if (int rc = resize_args(in, out, in_batch_stride, out_batch_stride, n, channels, in_height, in_width, out_height, out_width)) return rc;
    const bool vec = out_width % 4 == 0 && aligned16(out) && (n == 1 || out_batch_stride % 4 == 0);
    const long long total = (long long)n * channels * out_height * (out_width / (vec ? 4 : 1));
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(resize_nearest_fwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, in, in_batch_stride, out,
                           out_batch_stride, channels, in_height, in_width, out_height, out_width, total);
    else
        hipLaunchKernelGGL(resize_nearest_fwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, in_batch_stride, out,
                           out_batch_stride, channels, in_height, in_width, out_height, out_width, total);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_resize_nearest_backward(const float* grad_out, long long grad_out_batch_stride, float* grad_in,
                                           long long grad_in_batch_stride, int n, int channels, int in_height, int in_width,
                                           int out_height, int out_width, kbn_stream_t stream) {
    using namespace kbn;
    if (int rc = resize_args(grad_out, grad_in, grad_in_batch_stride, grad_out_batch_stride, n, channels, in_height, in_width, out_height,
                             out_width))
        return rc;
    const bool vec = in_width % 4 == 0 && aligned16(grad_in) && (n == 1 || grad_in_batch_stride % 4 == 0);
    const long long total = (long long)n * channels * in_height * (in_width / (vec ? 4 : 1));
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(resize_nearest_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, grad_out, grad_out_batch_stride, grad_in,
                           grad_in_batch_stride, channels, in_height, in_width, out_height, out_width, total);
    else
        hipLaunchKernelGGL(resize_nearest_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, grad_out, grad_out_batch_stride, grad_in,
                           grad_in_batch_stride, channels, in_height, in_width, out_height, out_width, total);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_kb_xyz_backward(const float* z, long long z_batch_stride, const float* coordinates,
                                   long long coordinates_batch_stride, const float* grad_xyz, long long grad_xyz_batch_stride,
                                   float* grad_pre, long long grad_pre_batch_stride, int n, int height, int width, int apply_activation,
                                   float negative_slope, kbn_stream_t stream) {
    using namespace kbn;
    if (!z || !coordinates || !grad_xyz || !grad_pre) return KBN_ERR_INVALID_ARGUMENT;
    if (n <= 0 || height <= 0 || width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    const long long plane = (long long)height * width;
    if (plane > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    if (n > 1 && (z_batch_stride < plane || grad_pre_batch_stride < plane || coordinates_batch_stride < 3 * plane ||
                  grad_xyz_batch_stride < 3 * plane))
        return KBN_ERR_INVALID_ARGUMENT;
    if (plane > KT_MAX_ITEMS / n) return KBN_ERR_UNSUPPORTED;
    const bool strides4 = n == 1 || !((z_batch_stride | coordinates_batch_stride | grad_xyz_batch_stride | grad_pre_batch_stride) & 3);
    const bool vec = plane % 4 == 0 && strides4 && aligned16(z) && aligned16(coordinates) && aligned16(grad_xyz) && aligned16(grad_pre);
    const long long per_frame = plane / (vec ? 4 : 1), total = per_frame * n;
    const dim3 grid((unsigned)((total + 255) / 256));
    const int act = apply_activation ? 1 : 0;
    if (vec)
        hipLaunchKernelGGL(kb_xyz_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, z, z_batch_stride, coordinates,
                           coordinates_batch_stride, grad_xyz, grad_xyz_batch_stride, grad_pre, grad_pre_batch_stride, plane, per_frame,
                           total, act, negative_slope);
    else
        hipLaunchKernelGGL(kb_xyz_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, z, z_batch_stride, coordinates,
                           coordinates_batch_stride, grad_xyz, grad_xyz_batch_stride, grad_pre, grad_pre_batch_stride, plane, per_frame,
                           total, act, negative_slope);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_depth_map_backward(const float* logits, const float* depth, const float* grad_depth, float* grad_logits,
                                      long long count, float min_predict_depth, kbn_stream_t stream) {
    using namespace kbn;
    if (!logits || !depth || !grad_depth || !grad_logits) return KBN_ERR_INVALID_ARGUMENT;
    if (count <= 0 || count > KT_MAX_ITEMS || !(min_predict_depth > 0.f)) return KBN_ERR_INVALID_ARGUMENT;
    const bool vec = aligned16(logits) && aligned16(depth) && aligned16(grad_depth) && aligned16(grad_logits);
    const long long items = vec ? (count >> 2) + (count & 3) : count;
    const dim3 grid((unsigned)((items + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(depth_map_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, logits, depth, grad_depth, grad_logits,
                           count, min_predict_depth);
    else
        hipLaunchKernelGGL(depth_map_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, logits, depth, grad_depth, grad_logits,
                           count, min_predict_depth);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
