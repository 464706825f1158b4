// pack_frames.hip -- kbn_pack_frames_forward: the device ENCODER of the packed frame store (the layout is in frame_pack.h,
// the host codec in frame_pack.hip, the device decoder in unpack_packed.hip).  A batch of equally sized frames, samples interleaved
// on the device, becomes the file images kbn_frame_encode writes, byte for byte: every b, every segment size and every table entry
// is a pure function of the samples, so nothing has to be decided in file order.
//
// Three launches a call, whatever n is (blockIdx.x carries frame and row group, blockIdx.y the plane):
//   1. sizes   a workgroup (256 threads) owns one (frame, 8-row group, plane).  16 lanes form a segment's residuals -- left row:
//              s[x] - s[x-1] from the segment's second sample on; up rows: s[y][x] - s[y-1][x]; nothing crosses a group --, zigzag
//              them and OR them over the 16 lanes: b is the bit length of the OR (that of the largest field).  Lane 0 stores b in
//              the workspace and adds the segment's bytes; a workgroup sum gives the (group, plane)'s payload length.
//   2. table   a workgroup per frame: the exclusive scan of the frame's ceil(H/8) x C lengths IS the table; it also writes the
//              32-byte header, the zero padding up to the payload and out_bytes[frame].
//   3. emit    a workgroup per (frame, group, plane) again.  Its payload offset comes from the table, its b's from the workspace;
//              a scan of the segments' bytes (kept in LDS, as in the decoder) places every segment.  The payload is assembled in an
//              LDS image, 256 segments (at most 8 KB) at a time: the image is zeroed, every lane ORs its field in at its bit position
//              with integer LDS atomics (a field of <= 16 bits touches at most two dwords; OR commutes, so the bytes do not depend
//              on the order), and the image goes to global memory.  The image is laid out at the destination's phase mod 16, so a
//              16-byte word of LDS is a 16-byte word of the file: whole words inside the range are stored as such, the ragged head
//              and tail byte by byte.  Nothing outside [0, out_bytes[i]) of a slot is written.
// Integer work; the only atomics are ORs into zeroed LDS: the same bytes on every run.  No host synchronisation, no allocation.
#include <algorithm>

#include "frame_pack.h"
#include "kbn_common.h"
#include "wg_scan.h"

namespace kbn {

constexpr int PF_THREADS = WG_THREADS;                       // wg_scan.h: the workgroup its sums, scans and flushes serve
constexpr int PF_TEAMS = PF_THREADS / fp::FP_SEG;             // segments in flight: 16 lanes each
constexpr int PF_CHUNK = 256;                                 // segments assembled per LDS image
constexpr int PF_IMAGE_BYTES = PF_CHUNK * 2 * fp::FP_SEG;     // no segment takes more than 16 samples of 16 bits: 8 KB
constexpr int PF_IMAGE_DWORDS = (PF_IMAGE_BYTES + 16) / 4 + 4;   // + the phase mod 16, + slack for a field's second dword
static_assert(PF_CHUNK % PF_TEAMS == 0, "a chunk is a whole number of team rounds");
// LDS of the emit kernel: the image (8.2 KB) and one offset of 4 bytes per segment of the group and one more, 8 x ceil(W / 16) + 1 of
// them: 32 KB at the cap -- 40.2 KB of the 64 KB a workgroup gets without opting in to more.
static_assert(sizeof(unsigned) * (fp::FP_ROWS * (KBN_PACK_FRAMES_MAX_WIDTH / fp::FP_SEG) + 1) + sizeof(unsigned) * PF_IMAGE_DWORDS + 64 <= 65536,
              "KBN_PACK_FRAMES_MAX_WIDTH must fit the LDS budget");

// the field a sample leaves behind its predictor: zigzag of the signed representative of a - pred mod 2^bits
__device__ __forceinline__ unsigned pf_field(unsigned a, unsigned pred, int bits) {
    const unsigned mask = (1u << bits) - 1u;
    const unsigned u = (a - pred) & mask;
    const int d = (u >> (bits - 1)) ? (int)u - (int)(mask + 1u) : (int)u;
    return fp::zigzag(d);
}

struct PackFramesParams {
    const void* samples;
    unsigned char* out;
    unsigned long long out_stride;
    unsigned long long* out_bytes;
    unsigned* lengths;        // workspace: n x entries payload lengths ...
    unsigned char* heads;     // ... and n x entries x (8 x segments) header bytes
    int width, height, channels;
    int groups, segments;     // ceil(height / 8), ceil(width / 16)
    unsigned start;           // of the payload in a file
};

// ---- 1. sizes ----
template <typename T>
__global__ __launch_bounds__(PF_THREADS) void pack_sizes_kernel(const PackFramesParams p) {
    __shared__ unsigned wave_total[PF_THREADS / 64];
    constexpr int bits = 8 * (int)sizeof(T);
    const int tid = (int)threadIdx.x, team = tid >> 4, j = tid & 15;
    const unsigned frame = blockIdx.x / (unsigned)p.groups;
    const int g = (int)(blockIdx.x - frame * (unsigned)p.groups);
    const int plane = (int)blockIdx.y, C = p.channels, W = p.width, S = p.segments;
    const int rows = min(fp::FP_ROWS, p.height - g * fp::FP_ROWS);
    const int nseg = rows * S;
    const size_t entry = ((size_t)frame * p.groups + g) * C + plane;
    unsigned char* head = p.heads + entry * (size_t)(fp::FP_ROWS * S);
    const size_t pitch = (size_t)W * C;
    const T* base = static_cast<const T*>(p.samples) + ((size_t)frame * p.height + (size_t)g * fp::FP_ROWS) * pitch + plane;

    unsigned bytes = 0;
    for (int e0 = 0; e0 < nseg; e0 += PF_TEAMS) {   // the same trip count in every thread: the shuffles below stay convergent
        const int e = e0 + team;
        const int r = e / S, k = e - r * S;
        const int n = min(fp::FP_SEG, W - k * fp::FP_SEG);
        unsigned z = 0;
        if (e < nseg && j < n && (r > 0 || j > 0)) {
            const T* s = base + (size_t)r * pitch + (size_t)(k * fp::FP_SEG + j) * C;
            const unsigned pred = r == 0 ? *(s - C) : *(s - pitch);
            z = pf_field(*s, pred, bits);
        }
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) z |= __shfl_xor(z, d, fp::FP_SEG);
        const int b = z ? 32 - __clz(z) : 0;
        if (e < nseg && j == 0) {
            head[e] = (unsigned char)b;
            bytes += fp::segment_bytes(n, b, bits, r == 0);
        }
    }
    const unsigned total = wg_sum(bytes, wave_total);
    if (tid == 0) p.lengths[entry] = (unsigned)nseg + total;
}

// ---- 2. header and table ----
__global__ __launch_bounds__(PF_THREADS) void pack_table_kernel(const PackFramesParams p, int bits) {
    __shared__ unsigned wave_total[PF_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const size_t frame = blockIdx.x;
    const long long entries = (long long)p.groups * p.channels;
    const unsigned* len = p.lengths + frame * (size_t)entries;
    unsigned* word = reinterpret_cast<unsigned*>(p.out + frame * p.out_stride);   // 16-byte aligned
    unsigned carry = 0;
    for (long long at = 0; at < entries; at += PF_THREADS) {
        const long long i = at + tid;
        const unsigned v = i < entries ? len[i] : 0u;
        unsigned total;
        const unsigned incl = wg_scan(v, wave_total, &total);
        if (i < entries) word[8 + i] = carry + incl - v;
        carry += total;
    }
    if (tid == 0) {
        word[0] = 0x464E424Bu; word[1] = 0x00314D52u;   // "KBNFRM1\0"
        word[2] = (unsigned)p.width; word[3] = (unsigned)p.height;
        word[4] = (unsigned)p.channels | (unsigned)bits << 16;
        word[5] = (unsigned)fp::FP_ROWS | (unsigned)fp::FP_SEG << 16;
        word[6] = carry; word[7] = 0u;                  // payload_bytes
        word[8 + entries] = carry;
        for (long long i = 8 + entries + 1; i < (long long)(p.start >> 2); ++i) word[i] = 0u;
        p.out_bytes[frame] = (unsigned long long)p.start + carry;
    }
}

// ---- 3. emit ----
template <typename T>
__global__ __launch_bounds__(PF_THREADS) void pack_emit_kernel(const PackFramesParams p) {
    extern __shared__ unsigned seg_at[];   // byte offset of every segment from the (group, plane)'s start, and the payload's length
    __shared__ __attribute__((aligned(16))) unsigned image[PF_IMAGE_DWORDS];
    __shared__ unsigned wave_total[PF_THREADS / 64];
    constexpr int bits = 8 * (int)sizeof(T);
    const int tid = (int)threadIdx.x, team = tid >> 4, j = tid & 15;
    const unsigned frame = blockIdx.x / (unsigned)p.groups;
    const int g = (int)(blockIdx.x - frame * (unsigned)p.groups);
    const int plane = (int)blockIdx.y, C = p.channels, W = p.width, S = p.segments;
    const int rows = min(fp::FP_ROWS, p.height - g * fp::FP_ROWS);
    const int nseg = rows * S;
    const size_t entry_in_frame = (size_t)g * C + plane;
    const size_t entry = (size_t)frame * p.groups * C + entry_in_frame;
    const unsigned char* head = p.heads + entry * (size_t)(fp::FP_ROWS * S);
    const size_t pitch = (size_t)W * C;
    const T* base = static_cast<const T*>(p.samples) + ((size_t)frame * p.height + (size_t)g * fp::FP_ROWS) * pitch + plane;
    unsigned char* file = p.out + (size_t)frame * p.out_stride;
    const unsigned lo = reinterpret_cast<const unsigned*>(file)[8 + entry_in_frame];   // the table kernel's
    unsigned char* dst = file + p.start + lo;
    const int last_n = W - (S - 1) * fp::FP_SEG;

    // segment offsets: every thread sums a run of consecutive segments, the partial sums are scanned (as in unpack_packed.hip)
    {
        const int per = (nseg + PF_THREADS - 1) / PF_THREADS;
        const int e0 = min(nseg, tid * per), e1 = min(nseg, e0 + per);
        unsigned sum = 0;
        int r = e0 / S, k = e0 - r * S;
        for (int e = e0; e < e1; ++e) {
            sum += fp::segment_bytes(k == S - 1 ? last_n : fp::FP_SEG, head[e], bits, r == 0);
            if (++k == S) { k = 0; ++r; }
        }
        unsigned total;
        unsigned run = (unsigned)nseg + wg_scan(sum, wave_total, &total) - sum;
        r = e0 / S; k = e0 - r * S;
        for (int e = e0; e < e1; ++e) {
            seg_at[e] = run;
            run += fp::segment_bytes(k == S - 1 ? last_n : fp::FP_SEG, head[e], bits, r == 0);
            if (++k == S) { k = 0; ++r; }
        }
        if (tid == 0) seg_at[nseg] = (unsigned)nseg + total;
        __syncthreads();
    }

    // the header bytes
    for (int c0 = 0; c0 < nseg; c0 += PF_IMAGE_BYTES) {
        const unsigned count = (unsigned)min(PF_IMAGE_BYTES, nseg - c0);
        const unsigned phase = (unsigned)(reinterpret_cast<uintptr_t>(dst + c0) & 15u);
        unsigned char* image_bytes = reinterpret_cast<unsigned char*>(image);
        for (unsigned i = tid; i < count; i += PF_THREADS) image_bytes[phase + i] = head[c0 + i];
        __syncthreads();
        wg_flush(image, phase, dst + c0, count);
        __syncthreads();
    }

    // the fields
    for (int c0 = 0; c0 < nseg; c0 += PF_CHUNK) {
        const int c1 = min(nseg, c0 + PF_CHUNK);
        const unsigned b0 = seg_at[c0], b1 = seg_at[c1];
        const unsigned phase = (unsigned)(reinterpret_cast<uintptr_t>(dst + b0) & 15u);
        const unsigned dwords = (phase + (b1 - b0) + 3u) / 4u + 1u;   // <= PF_IMAGE_DWORDS
        for (unsigned i = tid; i < dwords; i += PF_THREADS) image[i] = 0u;
        __syncthreads();
        for (int e = c0 + team; e < c1; e += PF_TEAMS) {
            const int r = e / S, k = e - r * S;
            const int n = min(fp::FP_SEG, W - k * fp::FP_SEG);
            if (j >= n) continue;
            const int b = head[e];
            const T* s = base + (size_t)r * pitch + (size_t)(k * fp::FP_SEG + j) * C;
            unsigned value, at;   // the lane's field and its bit position in the segment
            if (r == 0 && j == 0) {
                value = *s; at = 0u;   // the left row's first sample, raw
            } else {
                if (b == 0) continue;
                value = pf_field(*s, r == 0 ? *(s - C) : *(s - pitch), bits);
                at = r == 0 ? (unsigned)(bits + (j - 1) * b) : (unsigned)(j * b);
            }
            const unsigned bit = (phase + seg_at[e] - b0) * 8u + at;
            const unsigned long long v = (unsigned long long)value << (bit & 31u);
            atomicOr(&image[bit >> 5], (unsigned)v);
            if ((unsigned)(v >> 32)) atomicOr(&image[(bit >> 5) + 1u], (unsigned)(v >> 32));
        }
        __syncthreads();
        wg_flush(image, phase, dst + b0, b1 - b0);
        __syncthreads();
    }
}

// the sizes the entry points share; false for what the encoder refuses
static bool pack_frames_geometry(int width, int height, int channels, int bits, size_t* bound) {
    *bound = kbn_frame_encode_bound(width, height, channels, bits);
    return *bound != 0 && *bound <= 0xffffffffull && width <= KBN_PACK_FRAMES_MAX_WIDTH;
}

static size_t pack_frames_heads_at(int n, int height, int channels) {   // bytes of the lengths, rounded up to 16
    const size_t groups = ((size_t)height + fp::FP_ROWS - 1) / fp::FP_ROWS;
    return ((size_t)n * groups * (size_t)channels * sizeof(unsigned) + 15) & ~(size_t)15;
}

}  // namespace kbn

extern "C" size_t kbn_pack_frames_stride(int width, int height, int channels, int bits) {
    size_t bound;
    if (width < 1 || height < 1 || !kbn::pack_frames_geometry(width, height, channels, bits, &bound)) return 0;
    return (bound + 15) & ~(size_t)15;
}

extern "C" size_t kbn_pack_frames_workspace_bytes(int n, int width, int height, int channels, int bits) {
    using namespace kbn;
    size_t bound;
    if (n < 1 || width < 1 || height < 1 || !pack_frames_geometry(width, height, channels, bits, &bound)) return 0;
    const size_t groups = ((size_t)height + fp::FP_ROWS - 1) / fp::FP_ROWS, segments = ((size_t)width + fp::FP_SEG - 1) / fp::FP_SEG;
    return pack_frames_heads_at(n, height, channels) + (((size_t)n * groups * (size_t)channels * fp::FP_ROWS * segments + 15) & ~(size_t)15);
}

extern "C" int kbn_pack_frames_forward(const void* samples, int n, int width, int height, int channels, int bits, unsigned char* out,
                                       size_t out_stride, unsigned long long* out_bytes, void* workspace, size_t workspace_bytes,
                                       kbn_stream_t stream) {
    using namespace kbn;
    if (!samples || !out || !out_bytes || !workspace) return KBN_ERR_INVALID_ARGUMENT;
    if (n < 1 || width < 1 || height < 1) return KBN_ERR_INVALID_ARGUMENT;
    size_t bound;
    if (!pack_frames_geometry(width, height, channels, bits, &bound)) return KBN_ERR_UNSUPPORTED;
    const unsigned long long groups = ((unsigned long long)height + fp::FP_ROWS - 1) / fp::FP_ROWS;
    if (groups * (unsigned long long)n > 0x7fffffffull) return KBN_ERR_UNSUPPORTED;   // blockIdx.x carries (frame, group)
    if (reinterpret_cast<uintptr_t>(out) & 15) return KBN_ERR_INVALID_ARGUMENT;
    if (bits == 16 && (reinterpret_cast<uintptr_t>(samples) & 1)) return KBN_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(workspace) & 3) || (reinterpret_cast<uintptr_t>(out_bytes) & 7)) return KBN_ERR_INVALID_ARGUMENT;
    if ((out_stride & 15) || out_stride < ((bound + 15) & ~(size_t)15)) return KBN_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < kbn_pack_frames_workspace_bytes(n, width, height, channels, bits)) return KBN_ERR_WORKSPACE;

    PackFramesParams p;
    p.samples = samples; p.out = out; p.out_stride = out_stride; p.out_bytes = out_bytes;
    p.lengths = static_cast<unsigned*>(workspace);
    p.heads = static_cast<unsigned char*>(workspace) + pack_frames_heads_at(n, height, channels);
    p.width = width; p.height = height; p.channels = channels;
    p.groups = (int)groups; p.segments = (width + fp::FP_SEG - 1) / fp::FP_SEG;
    p.start = (unsigned)fp::payload_start(groups, (unsigned)channels);
    const dim3 grid((unsigned)(groups * (unsigned long long)n), (unsigned)channels), block(PF_THREADS);
    const size_t lds = sizeof(unsigned) * ((size_t)fp::FP_ROWS * p.segments + 1);
    hipStream_t s = (hipStream_t)stream;
    if (bits == 16) hipLaunchKernelGGL((pack_sizes_kernel<unsigned short>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((pack_sizes_kernel<unsigned char>), grid, block, 0, s, p);
    hipLaunchKernelGGL(pack_table_kernel, dim3((unsigned)n), block, 0, s, p, bits);
    if (bits == 16) hipLaunchKernelGGL((pack_emit_kernel<unsigned short>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((pack_emit_kernel<unsigned char>), grid, block, lds, s, p);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
