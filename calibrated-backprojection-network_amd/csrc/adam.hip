// adam.hip -- the training step's optimizer: one Adam step over a LIST of fp32 tensors (kbn_adam_step), what the reference's
// torch.optim.Adam does in src/kbnet.py:360-369, 453.  torch's _single_tensor_adam with L2 weight decay (no amsgrad, no maximize, no
// decoupled decay), per element, in fp32, in this order:
//     g' = g + wd * p                                  (skipped when wd == 0)
//     m  = m + (1 - beta1) * (g' - m)
//     v  = beta2 * v + (1 - beta2) * g' * g'
//     p  = p - step_size * m / (sqrt(v) / bc2_sqrt + eps)
// step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), 1 - beta1 and 1 - beta2 are the CALLER's fp64 numbers rounded to
// float, per tensor (t differs between tensors: a parameter without a gradient does not advance).  sqrt and the divisions are the
// correctly rounded ones (no fast-math flag on this file); a non-finite gradient element poisons its own element of p, m, v only.
//
// Launch geometry.  The pointers and scalars of up to KBN_ADAM_TABLE_CAPACITY tensors travel BY VALUE in the kernel arguments
// (72 bytes a tensor, 3456 of the 4096 bytes a launch may carry): no device-side table, no copy, no allocation, no synchronisation.
// A longer list takes ceil(count / capacity) launches.  grid = (gx, tensors of the launch), 256 threads: blockIdx.y picks the tensor
// (its record is read with scalar loads from the argument segment), blockIdx.x strides over its elements, four per thread and pass
// where p, g, m and v are all 16-byte aligned (a scalar tail of at most three elements), one per thread otherwise.
// gx = min(KBN_ADAM_MAX_BLOCKS_X, blocks that cover the launch's largest tensor once): a 2.4 M-element conv weight loops ~ 5 times in
// 512 blocks while a 64-element BatchNorm vector beside it ends after one block -- the other gx - 1 blocks of its row find nothing to
// do and leave.  One pass of the widest grid covers KBN_ADAM_PASS_ELEMENTS = 512 * 256 * 4 elements.
// No LDS, no atomics, no scratch; every element is read once (p, g, m, v) and written once (p, m, v): 28 bytes an element.
#include <math.h>

#include "kbn_common.h"

namespace kbn {

constexpr int ADAM_THREADS = 256;
static_assert((long long)KBN_ADAM_MAX_BLOCKS_X * ADAM_THREADS * 4 == KBN_ADAM_PASS_ELEMENTS, "header constants disagree");

struct AdamSlot {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long numel;
    float weight_decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps;
    int vec;   // all four pointers 16-byte aligned
};
struct AdamTable {
    AdamSlot slot[KBN_ADAM_TABLE_CAPACITY];
};
static_assert(sizeof(AdamTable) <= 3584, "the table must fit the kernel-argument segment");

template <bool DECAY>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamSlot& s) {
    if constexpr (DECAY) g = g + s.weight_decay * p;
    m = m + s.one_minus_beta1 * (g - m);
    v = s.beta2 * v + s.one_minus_beta2 * g * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p - s.step_size * m / denom;
}

template <bool DECAY>
__device__ __forceinline__ void adam_tensor(const AdamSlot& s) {
    const long long first = (long long)blockIdx.x * ADAM_THREADS + threadIdx.x;
    const long long step = (long long)gridDim.x * ADAM_THREADS;
    long long tail = 0;   // the first element of the scalar part
    if (s.vec) {
        const long long quads = s.numel >> 2;
        f32x4* p4 = reinterpret_cast<f32x4*>(s.p);
        const f32x4* g4 = reinterpret_cast<const f32x4*>(s.g);
        f32x4* m4 = reinterpret_cast<f32x4*>(s.m);
        f32x4* v4 = reinterpret_cast<f32x4*>(s.v);
        for (long long i = first; i < quads; i += step) {
            f32x4 p = p4[i], m = m4[i], v = v4[i];
            const f32x4 g = g4[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = p[k], mk = m[k], vk = v[k];
                adam_element<DECAY>(pk, g[k], mk, vk, s);
                p[k] = pk; m[k] = mk; v[k] = vk;
            }
            p4[i] = p; m4[i] = m; v4[i] = v;
        }
        tail = quads << 2;
    }
    for (long long i = tail + first; i < s.numel; i += step) {
        float p = s.p[i], m = s.m[i], v = s.v[i];
        adam_element<DECAY>(p, s.g[i], m, v, s);
        s.p[i] = p; s.m[i] = m; s.v[i] = v;
    }
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(const AdamTable table) {
    const AdamSlot& s = table.slot[blockIdx.y];
    if ((long long)blockIdx.x * ADAM_THREADS * (s.vec ? 4 : 1) >= s.numel) return;   // a short tensor beside a long one
    if (s.weight_decay != 0.f) adam_tensor<true>(s);
    else adam_tensor<false>(s);
}

}  // namespace kbn

extern "C" {

int kbn_adam_step(const kbn_adam_tensor* tensors, int count, kbn_stream_t stream) {
    using namespace kbn;
    if (!tensors || count < 1) return KBN_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < count; ++i) {
        const kbn_adam_tensor& t = tensors[i];
        if (t.numel < 0) return KBN_ERR_INVALID_ARGUMENT;
        if (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return KBN_ERR_INVALID_ARGUMENT;
    }
    AdamTable table;
    int used = 0;
    long long longest = 0;   // in thread-passes: quads of an aligned tensor, elements of another
    auto flush = [&]() {
        if (!used) return;
        const long long blocks = (longest + ADAM_THREADS - 1) / ADAM_THREADS;
        const dim3 grid((unsigned)std::min<long long>(blocks, KBN_ADAM_MAX_BLOCKS_X), (unsigned)used);
        hipLaunchKernelGGL(adam_step_kernel, grid, dim3(ADAM_THREADS), 0, (hipStream_t)stream, table);
        used = 0;
        longest = 0;
    };
    for (int i = 0; i < count; ++i) {
        const kbn_adam_tensor& t = tensors[i];
        if (t.numel == 0) continue;
        AdamSlot& s = table.slot[used++];
        s.p = t.param; s.g = t.grad; s.m = t.exp_avg; s.v = t.exp_avg_sq;
        s.numel = t.numel;
        s.weight_decay = t.weight_decay; s.one_minus_beta1 = t.one_minus_beta1; s.beta2 = t.beta2; s.one_minus_beta2 = t.one_minus_beta2;
        s.step_size = t.step_size; s.bc2_sqrt = t.bc2_sqrt; s.eps = t.eps;
        s.vec = ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) | reinterpret_cast<uintptr_t>(t.exp_avg) |
                  reinterpret_cast<uintptr_t>(t.exp_avg_sq)) & 15) == 0;
        longest = std::max(longest, s.vec ? (t.numel + 3) >> 2 : t.numel);
        if (used == KBN_ADAM_TABLE_CAPACITY) flush();
    }
    flush();
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

}  // extern "C"
