// augment.hip -- the training step's augmentation (kbn_augment_forward): what the reference's Transforms.transform does in
// src/transforms.py:61-183 to a LIST of N x C x H x W fp32 tensors -- image normalisation, per-frame flips of every tensor, random
// removal of a fraction of the positive points of the range maps, noise on their remaining points -- with the per-frame decisions
// made by the caller (a nibble a frame: bit 0 horizontal flip, 1 vertical flip, 2 remove, 3 noise) and every random draw taken
// from Philox4x32-10 keyed by (seed, element, frame, call, purpose | map << 8), so that a host oracle computes the same bits.
// `frame` is frame_base + the index in the batch the launch was given (kbn_augment_forward_at): a rank that augments frames
// [first, first + n) of a global batch passes frame_base = first and draws what one process draws for those frames.  Addressing
// -- the source and destination frames, the flags nibble, densities[b], the workspace record -- uses the index in the batch.
//
// Two launches.
//   select_kernel   one workgroup of 1024 threads per (frame with the remove flag, range map).  The candidates are the elements
//                   > 0; each has the 64-bit value (key << 32 | source element index), all distinct.  The kernel finds the k-th
//                   smallest of them, k = trunc(fp32(density) * fp32(count)):
//                     1. one pass over the frame writes the candidates' indices to a list in the workspace and counts them (an
//                        LDS counter hands out the places); k follows from the device-resident density; k == 0 ends here;
//                     2. a radix select over the value's bytes from the top, over the LIST: a pass fills a 256-bin integer
//                        histogram in LDS (of the entries that match the prefix found so far), the first wave scans it, and the
//                        pass's bin extends the prefix.  The first pass draws the keys -- on full waves: in the frame itself 1 lane
//                        in 20 holds a KITTI point, and a wave pays Philox's 40 quarter-rate multiplies whenever one lane does --
//                        and keeps them in the list.  The loop ends as soon as the chosen bin holds exactly the candidates
//                        still wanted: with distinct keys after at most four passes (two or three at KITTI's counts); only equal
//                        keys AT the boundary go on into the index bytes, and byte 0 always ends it (the values are distinct).
//                   The threshold (key, index, k, count) goes to the frame's 16-byte workspace record; nothing comes back to the
//                   host.  A frame without the flag leaves at once.  Integer LDS atomics only; the result does not depend on the
//                   order of the list.
//   apply_kernel    one launch for all tensors: grid (x, frames, tensors), 256 threads.  Per destination element: the flipped
//                   source read, then by role the normalisation (image), the removal predicate value <= threshold and the noise
//                   (range), or nothing (validity).  Four elements a thread with 16-byte loads and stores where the row allows
//                   it (W % 4 == 0, unit element stride, 16-byte aligned pointers and strides; a horizontal flip reverses inside
//                   the vector), one element a thread otherwise.
// The tensor records (80 bytes each), the flag nibbles of up to KBN_AUGMENT_MAX_FRAMES frames and the scalars travel BY VALUE in
// the kernel arguments: no device table, no copy, no allocation, no synchronisation.  Longer lists / batches take more launches.
//
// Arithmetic (no fast-math flag on this file; every operation that a contraction could fuse is written with an explicit
// round-to-nearest intrinsic):
//   image [0, 1]   x / 255          image [-1, 1]   fsub(2 (x / 255), 1)          image [0, 255]   x
//   uniform        u = (w0 >> 8) 2^-24;  noise = fsub(u, 0.5)
//   gaussian       u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24;  noise = fmul(sqrtf(fmul(-2, logf(u1))), cosf(fmul(2 pi, u2)))
//   range          out = fmul(fadd(v, fmul(spread, noise)), v > 0 ? 1 : 0)      with v the value after removal
#include <math.h>

#include "kbn_common.h"

namespace kbn {

constexpr int AUG_THREADS = 256;
constexpr int SEL_THREADS = 1024;
constexpr int SEL_UNROLL = 8;       // 16-byte loads a thread keeps in flight while it scans a frame
constexpr int AUG_TABLE_CAPACITY = 16;       // tensors a launch carries
constexpr int AUG_TARGET_BLOCKS = 4096;      // apply: about this many workgroups a launch (256 CUs x 16)

enum { ROLE_IMAGE = KBN_AUGMENT_ROLE_IMAGE, ROLE_RANGE = KBN_AUGMENT_ROLE_RANGE, ROLE_VALIDITY = KBN_AUGMENT_ROLE_VALIDITY };
enum { FLAG_HFLIP = 1, FLAG_VFLIP = 2, FLAG_REMOVE = 4, FLAG_NOISE = 8 };

struct AugSlot {
    const float* src;
    float* dst;
    long long sn, sc, sh, sw;   // element strides of src; dst is a dense N x c x H x W tensor
    int channels, role, map_index;
    int vec;                    // the 16-byte path: see the file comment
    unsigned* thresholds;       // range maps: this map's N workspace records (4 words a frame)
    unsigned long long* candidates;   // range maps: this map's N candidate lists of c H W entries each (selection only)
};
struct AugParams {
    AugSlot slot[AUG_TABLE_CAPACITY];
    unsigned flags[KBN_AUGMENT_MAX_FRAMES / 8];   // a nibble a frame of this launch
    const float* densities;                       // N, indexed by the frame's index in the batch
    int frame0;                                   // the batch index of the launch's first frame
    unsigned frame_base;                          // the batch's first frame in the GLOBAL batch: the Philox frame word is frame_base + b
    int height, width;
    int normalization, noise_type;
    float noise_spread;
    unsigned seed_lo, seed_hi, call;
};
static_assert(sizeof(AugSlot) == 80 && sizeof(AugParams) <= 3584, "the records must fit the kernel-argument segment");

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 / cuRAND constants)
struct Philox4 { unsigned w0, w1, w2, w3; };
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}
__device__ __forceinline__ unsigned removal_key(const AugParams& p, const AugSlot& s, unsigned element, unsigned frame) {
    return philox4x32_10(element, p.frame_base + frame, p.call, 0u | ((unsigned)s.map_index << 8), p.seed_lo, p.seed_hi).w0;
}
__device__ __forceinline__ float noise_draw(const AugParams& p, const AugSlot& s, unsigned element, unsigned frame) {
    const Philox4 r = philox4x32_10(element, p.frame_base + frame, p.call, 1u | ((unsigned)s.map_index << 8), p.seed_lo, p.seed_hi);
    if (p.noise_type == KBN_AUGMENT_NOISE_UNIFORM) return __fsub_rn((float)(r.w0 >> 8) * 0x1p-24f, 0.5f);
    const float u1 = (float)((r.w0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(r.w1 >> 8) * 0x1p-24f;
    return __fmul_rn(sqrtf(__fmul_rn(-2.0f, logf(u1))), cosf(__fmul_rn(6.283185307179586f, u2)));
}
__device__ __forceinline__ unsigned frame_flags(const AugParams& p, int local_frame) {
    return (p.flags[local_frame >> 3] >> ((local_frame & 7) * 4)) & 15u;
}

// ------------------------------------------------------------------------------------------------------------ selection
// The frame's candidates (elements > 0) as a list of their element indices in `list`, in any order; returns nothing, the count is
// *total (LDS, zeroed by the caller before a barrier).  16-byte loads, SEL_UNROLL of them in flight a thread, where the slot allows.
template <bool VEC>
__device__ __forceinline__ void collect_candidates(const AugParams& p, const AugSlot& s, const float* frame, unsigned long long* list,
                                                   unsigned* total) {
    const int W = p.width, H = p.height;
    // One LDS atomic an element hands out the places: the lanes of a wave get consecutive ones, so the wave's stores fall into one
    // or two lines.  (A thread that reserved the places of all 32 elements of its trip at once wrote runs of its own, scattered
    // over the list: measured slower, 53 us instead of 46 us a KITTI frame and 174 us instead of 48 us a dense one.)
    auto visit = [&](unsigned element, float v) {
        if (v > 0.f) list[atomicAdd(total, 1u)] = element;   // at most c H W entries: the list's capacity
    };
    if constexpr (VEC) {
        const int wq = W >> 2;
        const unsigned quads = (unsigned)s.channels * H * wq;
        for (unsigned base = threadIdx.x; base < quads; base += SEL_THREADS * SEL_UNROLL) {
            f32x4 v[SEL_UNROLL];
#pragma unroll
            for (int j = 0; j < SEL_UNROLL; ++j) {
                const unsigned q = base + j * SEL_THREADS;
                const bool in = q < quads;
                const unsigned row = in ? q / wq : 0, x4 = in ? q - row * wq : 0;   // row = plane * H + y
                const unsigned plane = row / H, y = row - plane * H;
                v[j] = in ? *reinterpret_cast<const f32x4*>(frame + plane * s.sc + y * s.sh + 4ll * x4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < SEL_UNROLL; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) visit((base + j * SEL_THREADS) * 4u + i, v[j][i]);   // quad q holds elements 4 q .. 4 q + 3
        }
    } else {
        const unsigned elements = (unsigned)s.channels * H * W;
        for (unsigned base = threadIdx.x; base < elements; base += SEL_THREADS * SEL_UNROLL) {
            float v[SEL_UNROLL];
#pragma unroll
            for (int j = 0; j < SEL_UNROLL; ++j) {
                const unsigned q = base + j * SEL_THREADS;
                const bool in = q < elements;
                const unsigned row = in ? q / W : 0, x = in ? q - row * W : 0;
                const unsigned plane = row / H, y = row - plane * H;
                v[j] = in ? frame[plane * s.sc + y * s.sh + x * s.sw] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < SEL_UNROLL; ++j) visit(base + j * SEL_THREADS, v[j]);
        }
    }
}

__global__ __launch_bounds__(SEL_THREADS) void augment_select_kernel(const AugParams p) {
    __shared__ unsigned hist[256];
    __shared__ unsigned found[3];   // the pass's bin, the candidates below it, the candidates in it
    __shared__ unsigned total;
    const unsigned flags = frame_flags(p, blockIdx.x);
    if (!(flags & FLAG_REMOVE)) return;
    const AugSlot& s = p.slot[blockIdx.y];
    const unsigned b = (unsigned)p.frame0 + blockIdx.x;
    const float* frame = s.src + (long long)b * s.sn;
    unsigned* record = s.thresholds + 4ll * b;
    unsigned long long* list = s.candidates + (long long)b * ((long long)s.channels * p.height * p.width);
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (s.vec) collect_candidates<true>(p, s, frame, list, &total);
    else collect_candidates<false>(p, s, frame, list, &total);
    __syncthreads();   // the list is written by all and read by all: one workgroup, one CU, one L1
    const unsigned count = total;
    const float product = __fmul_rn(p.densities[b], (float)count);   // k from the device-resident density, the same in every thread
    unsigned k = product >= 1.f ? (product >= 4294967296.f ? count : (unsigned)product) : 0u;   // trunc; NaN and negatives give 0
    if (k > count) k = count;
    if (k == 0) {
        if (threadIdx.x == 0) { record[0] = 0; record[1] = 0; record[2] = 0; record[3] = count; }
        return;
    }
    unsigned long long prefix = 0;
    unsigned want = k;   // the rank wanted among the candidates that match the prefix (1-based)
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (unsigned i = threadIdx.x; i < count; i += SEL_THREADS) {   // entry i belongs to one thread in every pass
            unsigned long long value = list[i];
            if (shift == 56) {   // the first pass draws the keys, on full waves, and keeps them
                value |= (unsigned long long)removal_key(p, s, (unsigned)value, b) << 32;
                list[i] = value;
            } else if ((value >> (shift + 8)) != prefix) {
                continue;
            }
            atomicAdd(&hist[(unsigned)(value >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {   // the first wave: four bins a lane, an inclusive scan over the lanes
            const unsigned h0 = hist[4 * threadIdx.x], h1 = hist[4 * threadIdx.x + 1], h2 = hist[4 * threadIdx.x + 2], h3 = hist[4 * threadIdx.x + 3];
            const unsigned mine = h0 + h1 + h2 + h3;
            unsigned incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d);
                if ((int)threadIdx.x >= d) incl += up;
            }
            unsigned below = incl - mine;
            if (below < want && want <= incl) {   // exactly one lane: 1 <= want <= the candidates that match the prefix
                unsigned bin = 4 * threadIdx.x, in = h0;
                if (below + in < want) { below += in; in = h1; ++bin; }
                if (below + in < want) { below += in; in = h2; ++bin; }
                if (below + in < want) { below += in; in = h3; ++bin; }
                found[0] = bin; found[1] = below; found[2] = in;
            }
        }
        __syncthreads();
        const unsigned bin = found[0], below = found[1], in = found[2];
        prefix = (prefix << 8) | bin;
        want -= below;
        if (in == want) {   // every candidate of this bin is taken: the threshold is the largest value with this prefix
            const unsigned long long threshold = shift ? (prefix << shift) | ((1ull << shift) - 1ull) : prefix;
            if (threadIdx.x == 0) { record[0] = (unsigned)(threshold >> 32); record[1] = (unsigned)threshold; record[2] = k; record[3] = count; }
            return;
        }
        __syncthreads();   // found[] and hist[] are rewritten by the next pass
    }
}

// ---------------------------------------------------------------------------------------------------------------- apply
__device__ __forceinline__ float apply_element(const AugParams& p, const AugSlot& s, float v, unsigned element, unsigned b, unsigned flags,
                                               unsigned long long threshold) {
    if (s.role == ROLE_IMAGE) {
        if (p.normalization == KBN_AUGMENT_RANGE_0_255) return v;
        const float t = __fdiv_rn(v, 255.0f);
        return p.normalization == KBN_AUGMENT_RANGE_M1_1 ? __fsub_rn(__fmul_rn(2.0f, t), 1.0f) : t;
    }
    if (s.role == ROLE_RANGE) {
        if ((flags & FLAG_REMOVE) && v > 0.f) {
            const unsigned long long value = ((unsigned long long)removal_key(p, s, element, b) << 32) | element;
            if (value <= threshold) v = 0.f;
        }
        if (flags & FLAG_NOISE)
            v = __fmul_rn(__fadd_rn(v, __fmul_rn(p.noise_spread, noise_draw(p, s, element, b))), v > 0.f ? 1.0f : 0.0f);
    }
    return v;
}

__global__ __launch_bounds__(AUG_THREADS) void augment_apply_kernel(const AugParams p) {
    const AugSlot& s = p.slot[blockIdx.z];
    const int W = p.width, H = p.height;
    const unsigned per_frame = (unsigned)s.channels * H * W;
    const unsigned items = s.vec ? per_frame >> 2 : per_frame;
    if (blockIdx.x * (unsigned)AUG_THREADS >= items) return;   // a one-channel map beside a three-channel image
    const unsigned flags = frame_flags(p, blockIdx.y);
    const unsigned b = (unsigned)p.frame0 + blockIdx.y;
    const bool hflip = flags & FLAG_HFLIP, vflip = flags & FLAG_VFLIP;
    const float* frame = s.src + (long long)b * s.sn;
    float* out = s.dst + (long long)b * per_frame;
    unsigned long long threshold = 0;
    unsigned live = flags;
    if (s.role == ROLE_RANGE && (flags & FLAG_REMOVE)) {
        const unsigned* record = s.thresholds + 4ll * b;
        threshold = ((unsigned long long)record[0] << 32) | record[1];
        if (record[2] == 0) live &= ~(unsigned)FLAG_REMOVE;   // k == 0: nothing is removed
    }
    const unsigned first = blockIdx.x * AUG_THREADS + threadIdx.x, step = gridDim.x * AUG_THREADS;
    if (s.vec) {
        const unsigned wq = W >> 2;
        for (unsigned q = first; q < items; q += step) {
            const unsigned row = q / wq, x4 = q - row * wq;
            const unsigned plane = row / H, y = row - plane * H;
            const unsigned ys = vflip ? H - 1 - y : y, xs = hflip ? W - 4 - 4 * x4 : 4 * x4;
            const f32x4 in = *reinterpret_cast<const f32x4*>(frame + plane * s.sc + ys * s.sh + xs);
            const unsigned element = (plane * H + ys) * W + xs;   // of in[0], in the source frame
            f32x4 r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = hflip ? 3 - i : i;
                r[i] = apply_element(p, s, in[j], element + j, b, live, threshold);
            }
            *reinterpret_cast<f32x4*>(out + 4ll * q) = r;
        }
    } else {
        for (unsigned q = first; q < items; q += step) {
            const unsigned row = q / W, x = q - row * W;
            const unsigned plane = row / H, y = row - plane * H;
            const unsigned ys = vflip ? H - 1 - y : y, xs = hflip ? W - 1 - x : x;
            const float v = frame[plane * s.sc + ys * s.sh + xs * s.sw];
            out[q] = apply_element(p, s, v, (plane * H + ys) * W + xs, b, live, threshold);
        }
    }
}

}  // namespace kbn

extern "C" {

size_t kbn_augment_workspace_bytes(const kbn_augment_tensor* tensors, int count, int n, int height, int width) {
    if (!tensors || count < 1 || n < 1 || height < 1 || width < 1) return 0;
    unsigned __int128 bytes = 0;   // three ints and a count multiply past 64 bits
    for (int i = 0; i < count; ++i) {
        const kbn_augment_tensor& t = tensors[i];
        if (t.role != KBN_AUGMENT_ROLE_RANGE || t.channels < 1) continue;
        bytes += (unsigned __int128)n * (KBN_AUGMENT_WORKSPACE_RECORD_BYTES + (unsigned __int128)8 * t.channels * height * width);   // a record and a candidate list a frame
    }
    return bytes > KBN_MAX_SIZE_BYTES ? 0 : (size_t)bytes;
}

int kbn_augment_forward_at(const kbn_augment_tensor* tensors, int count, const unsigned char* flags, int n, int height, int width,
                           const float* densities, void* workspace, size_t workspace_bytes, int normalization, int noise_type,
                           float noise_spread, unsigned long long seed, unsigned call, unsigned frame_base, int stages,
                           kbn_stream_t stream) {
    using namespace kbn;
    if (!tensors || !flags || count < 1 || n < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    if ((unsigned long long)frame_base + (unsigned long long)n > 0xffffffffull) return KBN_ERR_UNSUPPORTED;   // the frame word is 32 bits
    if (normalization < KBN_AUGMENT_RANGE_0_255 || normalization > KBN_AUGMENT_RANGE_M1_1) return KBN_ERR_INVALID_ARGUMENT;
    if (noise_type < KBN_AUGMENT_NOISE_NONE || noise_type > KBN_AUGMENT_NOISE_UNIFORM) return KBN_ERR_INVALID_ARGUMENT;
    if (!(stages & (KBN_AUGMENT_STAGE_SELECT | KBN_AUGMENT_STAGE_APPLY))) return KBN_ERR_INVALID_ARGUMENT;
    bool any_remove = false, any_noise = false;
    for (int b = 0; b < n; ++b) {
        if (flags[b] > 15) return KBN_ERR_INVALID_ARGUMENT;
        any_remove |= (flags[b] & FLAG_REMOVE) != 0;
        any_noise |= (flags[b] & FLAG_NOISE) != 0;
    }
    int ranges = 0;
    for (int i = 0; i < count; ++i) {
        const kbn_augment_tensor& t = tensors[i];
        if (!t.src || !t.dst || t.channels < 1 || t.role < ROLE_IMAGE || t.role > ROLE_VALIDITY) return KBN_ERR_INVALID_ARGUMENT;
        if (t.stride_n < 0 || t.stride_c < 0 || t.stride_h < 0 || t.stride_w < 0) return KBN_ERR_INVALID_ARGUMENT;
        if ((long long)t.channels * height * width > 0x7fffffffll) return KBN_ERR_UNSUPPORTED;   // element indices are 32-bit counter words
        if (t.role == ROLE_RANGE) {
            if (t.map_index < 0 || t.map_index >= (1 << 24)) return KBN_ERR_INVALID_ARGUMENT;
            ++ranges;
        }
    }
    const bool select = ranges > 0 && any_remove;
    if (select && (!densities || !workspace)) return KBN_ERR_INVALID_ARGUMENT;
    const size_t workspace_need = select ? kbn_augment_workspace_bytes(tensors, count, n, height, width) : 0;
    if (select && (workspace_need == 0 || workspace_bytes < workspace_need)) return KBN_ERR_WORKSPACE;   // 0: no size_t holds the need
    if (select && (reinterpret_cast<uintptr_t>(workspace) & 7)) return KBN_ERR_INVALID_ARGUMENT;
    if (ranges > 0 && any_noise && noise_type == KBN_AUGMENT_NOISE_NONE) return KBN_ERR_INVALID_ARGUMENT;

    AugParams p;
    p.densities = densities;
    p.height = height; p.width = width;
    p.normalization = normalization; p.noise_type = noise_type; p.noise_spread = noise_spread;
    p.seed_lo = (unsigned)seed; p.seed_hi = (unsigned)(seed >> 32); p.call = call;
    p.frame_base = frame_base;
    // the workspace: the records of all range maps (16 bytes a frame, in the order of the range maps), then their candidate lists
    auto fill = [&](AugSlot& s, const kbn_augment_tensor& t, int range_ordinal) {
        s.src = t.src; s.dst = t.dst;
        s.sn = t.stride_n; s.sc = t.stride_c; s.sh = t.stride_h; s.sw = t.stride_w;
        s.channels = t.channels; s.role = t.role; s.map_index = t.map_index;
        s.vec = width % 4 == 0 && t.stride_w == 1 && ((t.stride_n | t.stride_c | t.stride_h) & 3) == 0 &&
                ((reinterpret_cast<uintptr_t>(t.src) | reinterpret_cast<uintptr_t>(t.dst)) & 15) == 0;
        s.thresholds = nullptr;
        s.candidates = nullptr;
        if (t.role == ROLE_RANGE && workspace) {
            s.thresholds = static_cast<unsigned*>(workspace) + 4ll * range_ordinal * n;
            long long before = 0;   // list entries of the range maps in front of this one
            for (const kbn_augment_tensor* u = tensors; u != &t; ++u)
                if (u->role == ROLE_RANGE) before += (long long)n * u->channels * height * width;
            s.candidates = reinterpret_cast<unsigned long long*>(static_cast<unsigned*>(workspace) + 4ll * ranges * n) + before;
        }
    };
    for (int frame0 = 0; frame0 < n; frame0 += KBN_AUGMENT_MAX_FRAMES) {
        const int frames = std::min(n - frame0, (int)KBN_AUGMENT_MAX_FRAMES);
        for (unsigned& word : p.flags) word = 0;
        bool chunk_remove = false;
        for (int f = 0; f < frames; ++f) {
            p.flags[f >> 3] |= (unsigned)flags[frame0 + f] << ((f & 7) * 4);
            chunk_remove |= (flags[frame0 + f] & FLAG_REMOVE) != 0;
        }
        p.frame0 = frame0;
        if ((stages & KBN_AUGMENT_STAGE_SELECT) && select && chunk_remove) {
            int used = 0, ordinal = 0;
            auto flush = [&]() {
                if (!used) return;
                hipLaunchKernelGGL(augment_select_kernel, dim3((unsigned)frames, (unsigned)used), dim3(SEL_THREADS), 0, (hipStream_t)stream, p);
                used = 0;
            };
            for (int i = 0; i < count; ++i) {
                if (tensors[i].role != ROLE_RANGE) continue;
                fill(p.slot[used++], tensors[i], ordinal++);
                if (used == AUG_TABLE_CAPACITY) flush();
            }
            flush();
        }
        if (stages & KBN_AUGMENT_STAGE_APPLY) {
            int used = 0, ordinal = 0;
            long long longest = 0;   // in thread-items: quads of a vector tensor's frame, elements of another's
            auto flush = [&]() {
                if (!used) return;
                const long long cover = (longest + AUG_THREADS - 1) / AUG_THREADS;
                const long long share = std::max<long long>(1, AUG_TARGET_BLOCKS / ((long long)frames * used));
                hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)std::min(cover, share), (unsigned)frames, (unsigned)used), dim3(AUG_THREADS),
                                   0, (hipStream_t)stream, p);
                used = 0;
                longest = 0;
            };
            for (int i = 0; i < count; ++i) {
                AugSlot& s = p.slot[used++];
                fill(s, tensors[i], ordinal);
                if (tensors[i].role == ROLE_RANGE) ++ordinal;
                const long long per_frame = (long long)s.channels * height * width;
                longest = std::max(longest, s.vec ? per_frame >> 2 : per_frame);
                if (used == AUG_TABLE_CAPACITY) flush();
            }
            flush();
        }
    }
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_augment_forward(const kbn_augment_tensor* tensors, int count, const unsigned char* flags, int n, int height, int width,
                        const float* densities, void* workspace, size_t workspace_bytes, int normalization, int noise_type,
                        float noise_spread, unsigned long long seed, unsigned call, int stages, kbn_stream_t stream) {
    return kbn_augment_forward_at(tensors, count, flags, n, height, width, densities, workspace, workspace_bytes, normalization, noise_type,
                                  noise_spread, seed, call, 0u, stages, stream);
}

}  // extern "C"
