// multi_copy.hip -- dst[i][e] = src[i][e] * scale over a LIST of fp32 runs in one launch (kbn_multi_tensor_scale_copy): how
// kb.dist.GradientAverager packs every parameter's gradient, weighted by its rank's share of the global batch, into the one buffer
// the step's all-reduce runs over, and how it moves the parameters through that buffer for the broadcast.  One fp32 multiply an
// element (no fast-math flag on this file): the bits of src * scale as torch computes it, the source's own bits for scale == 1, and
// a NaN or Inf element stays in its own element.
//
// Launch geometry: adam.hip's.  The records (src, dst, numel) of up to KBN_MULTI_COPY_TABLE_CAPACITY tensors travel BY VALUE in the
// kernel arguments (32 bytes a tensor, 1536 of the 4096 bytes a launch may carry): no device-side table, no copy, no allocation, no
// synchronisation.  A longer list takes ceil(count / capacity) launches.  grid = (gx, tensors of the launch), 256 threads:
// blockIdx.y picks the tensor (its record is read with scalar loads from the argument segment), blockIdx.x strides over its
// elements, four per thread and pass where src and dst are both 16-byte aligned (a scalar tail of at most three elements), one per
// thread otherwise.  gx = min(KBN_MULTI_COPY_MAX_BLOCKS_X, blocks that cover the launch's largest tensor once): a long tensor loops
// while a short one beside it ends after one block -- the other blocks of its row find nothing to do and leave.  One pass of the
// widest grid covers KBN_MULTI_COPY_PASS_ELEMENTS = 512 * 256 * 4 elements.
// No LDS, no atomics, no scratch; every element is read once and written once: 8 bytes an element.
#include "kbn_common.h"

namespace kbn {

constexpr int MULTI_COPY_THREADS = 256;
static_assert((long long)KBN_MULTI_COPY_MAX_BLOCKS_X * MULTI_COPY_THREADS * 4 == KBN_MULTI_COPY_PASS_ELEMENTS, "header constants disagree");

struct CopySlot {
    const float* src;
    float* dst;
    long long numel;
    int vec;   // both pointers 16-byte aligned
};
struct CopyTable {
    CopySlot slot[KBN_MULTI_COPY_TABLE_CAPACITY];
};
static_assert(sizeof(CopyTable) <= 3584, "the table must fit the kernel-argument segment");

__global__ __launch_bounds__(MULTI_COPY_THREADS) void multi_tensor_scale_copy_kernel(const CopyTable table, const float scale) {
    const CopySlot& s = table.slot[blockIdx.y];
    if ((long long)blockIdx.x * MULTI_COPY_THREADS * (s.vec ? 4 : 1) >= s.numel) return;   // a short tensor beside a long one
    const long long first = (long long)blockIdx.x * MULTI_COPY_THREADS + threadIdx.x;
    const long long step = (long long)gridDim.x * MULTI_COPY_THREADS;
    long long tail = 0;   // the first element of the scalar part
    if (s.vec) {
        const long long quads = s.numel >> 2;
        const f32x4* src4 = reinterpret_cast<const f32x4*>(s.src);
        f32x4* dst4 = reinterpret_cast<f32x4*>(s.dst);
        // four passes of the stride loop at a time, their loads issued before the first store: a thread of the longest tensor's row,
        // which is still looping when the rows beside it have left, then waits for memory once per four passes
        for (long long i = first; i < quads; i += 4 * step) {
            const long long i1 = i + step, i2 = i1 + step, i3 = i2 + step;
            f32x4 a = src4[i], b = {}, c = {}, d = {};
            if (i1 < quads) b = src4[i1];
            if (i2 < quads) c = src4[i2];
            if (i3 < quads) d = src4[i3];
            dst4[i] = a * scale;
            if (i1 < quads) dst4[i1] = b * scale;
            if (i2 < quads) dst4[i2] = c * scale;
            if (i3 < quads) dst4[i3] = d * scale;
        }
        tail = quads << 2;
    }
    for (long long i = tail + first; i < s.numel; i += step) s.dst[i] = s.src[i] * scale;
}

}  // namespace kbn

extern "C" {

int kbn_multi_tensor_scale_copy(const kbn_copy_tensor* tensors, int count, float scale, kbn_stream_t stream) {
    using namespace kbn;
    if (!tensors || count < 1) return KBN_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < count; ++i) {
        const kbn_copy_tensor& t = tensors[i];
        if (t.numel < 0) return KBN_ERR_INVALID_ARGUMENT;
        if (t.numel > 0 && (!t.src || !t.dst)) return KBN_ERR_INVALID_ARGUMENT;
    }
    CopyTable table;
    int used = 0;
    long long longest = 0;   // in thread-passes: quads of an aligned tensor, elements of another
    auto flush = [&]() {
        if (!used) return;
        const long long blocks = (longest + MULTI_COPY_THREADS - 1) / MULTI_COPY_THREADS;
        const dim3 grid((unsigned)std::min<long long>(blocks, KBN_MULTI_COPY_MAX_BLOCKS_X), (unsigned)used);
        hipLaunchKernelGGL(multi_tensor_scale_copy_kernel, grid, dim3(MULTI_COPY_THREADS), 0, (hipStream_t)stream, table, scale);
        used = 0;
        longest = 0;
    };
    for (int i = 0; i < count; ++i) {
        const kbn_copy_tensor& t = tensors[i];
        if (t.numel == 0) continue;
        CopySlot& s = table.slot[used++];
        s.src = t.src; s.dst = t.dst;
        s.numel = t.numel;
        s.vec = ((reinterpret_cast<uintptr_t>(t.src) | reinterpret_cast<uintptr_t>(t.dst)) & 15) == 0;
        longest = std::max(longest, s.vec ? (t.numel + 3) >> 2 : t.numel);
        if (used == KBN_MULTI_COPY_TABLE_CAPACITY) flush();
    }
    flush();
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

}  // extern "C"
