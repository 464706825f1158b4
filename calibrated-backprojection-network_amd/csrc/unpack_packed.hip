// unpack_packed.hip -- kbn_unpack_packed_frames_forward: the device decoder of the packed frame store (the layout is in
// frame_pack.h, the host codec in frame_pack.hip).  kbn_unpack_train_frames_forward's job -- the triplet split, the crop, uint8 /
// uint16 -> float32, depth / 256 -- done from the PACKED files of a batch instead of their decoded bytes, so the host only reads
// files into pinned memory and checks them (kbn_frame_check) where it used to inflate PNGs.
//
// A workgroup (256 threads) owns one (frame, row group, plane): blockIdx.z the frame -- its record travels by value in the kernel
// arguments, as in unpack_train.hip --, blockIdx.x the row group counted from the crop's first one, blockIdx.y the plane (the
// image's first min(C, 3) planes, then the depth file's one).
//   1. the group's header bytes -> every segment's byte offset, an exclusive prefix sum kept in LDS: each thread sums a run of
//      consecutive segments, the 256 partial sums are scanned with wave shuffles and four wave totals;
//   2. per wanted third and per tile of 240 output columns: the 16 segments that cover the tile are decoded by 16 lanes each, one
//      lane a column.  The group's first row ("left row") is a 16-lane inclusive scan of its differences, the rows below add their
//      difference to the value the lane holds: at most 8 serial adds.  The samples of the crop's rows go to a 4 KB LDS tile;
//   3. the tile is written out row by row: a thread converts four consecutive pixels and stores 16 bytes when width % 4 == 0 and
//      the outputs are 16-byte aligned, float by float otherwise (gray is written to all three channels).
// Integer work, no atomics, every output element written once by one thread: the same bits on every run.
//
// No address outside a file: the host entry point checks that every record lies inside its buffer and can hold its table; the
// kernel compares the file's header with the record and its table entry and prefix sum with each other before it reads a field,
// and leaves the workgroup's outputs unwritten when they disagree (files kbn_frame_check accepts always agree).  A field is read
// byte by byte, only the bytes it touches, all of them inside its segment.
#include "frame_pack.h"
#include "unpack_common.h"

namespace kbn {

constexpr int UP_THREADS = 256;
constexpr int UP_TILE = 240;                       // output columns of a tile: at most 16 segments cover them at any phase

struct UnpackPackedParams {
    kbn_packed_frame frame[KBN_UNPACK_TRAIN_MAX_FRAMES];   // of this launch
    const unsigned char* images;
    const unsigned char* depths;
    float* image0;
    float* image1;
    float* image2;
    float* depth;
    int frame0;          // the batch index of the launch's first frame
    int height, width;   // the crop
    int channels;        // of the image files
    int depth_bits;
};
static_assert(sizeof(kbn_packed_frame) == 40 && sizeof(UnpackPackedParams) <= 3584, "the records must fit the kernel-argument segment");
static_assert(UP_TILE % 4 == 0 && UP_TILE + fp::FP_SEG - 1 <= UP_THREADS, "a tile's segments must fit the workgroup");

// the `nb`-bit field (1 .. 16) at bit `at` of a segment: LSB first, only the bytes it touches
__device__ __forceinline__ unsigned read_field(const unsigned char* seg, unsigned at, int nb) {
    const unsigned char* p = seg + (at >> 3);
    const unsigned sh = at & 7u;
    const unsigned need = (sh + (unsigned)nb + 7u) >> 3;
    unsigned v = p[0];
    if (need > 1) v |= (unsigned)p[1] << 8;
    if (need > 2) v |= (unsigned)p[2] << 16;
    return (v >> sh) & ((1u << nb) - 1u);
}

template <bool VEC>
__global__ __launch_bounds__(UP_THREADS) void unpack_packed_kernel(const UnpackPackedParams p) {
    extern __shared__ unsigned seg_at[];                        // byte offset of every segment of the group, from the group's start
    __shared__ unsigned short tile[fp::FP_ROWS][UP_THREADS];    // decoded samples: [row in group][column - 16 x first segment]
    __shared__ unsigned wave_total[UP_THREADS / 64];

    const int tid = (int)threadIdx.x;
    const kbn_packed_frame& f = p.frame[blockIdx.z];
    const int W = f.raw_width / 3;
    const int y_last = f.y_start + p.height - 1;
    const int g = (f.y_start >> 3) + (int)blockIdx.x;
    if (g > (y_last >> 3)) return;   // this frame's crop spans fewer groups than the widest of the launch
    const bool is_depth = blockIdx.y + 1 == gridDim.y;
    const unsigned char* file = is_depth ? p.depths + f.depth_offset : p.images + f.image_offset;
    const unsigned file_bytes = is_depth ? f.depth_bytes : f.image_bytes;
    const int fw = is_depth ? W : f.raw_width, C = is_depth ? 1 : p.channels, bits = is_depth ? p.depth_bits : 8;
    const int plane = is_depth ? 0 : (int)blockIdx.y;
    const unsigned mask = (1u << bits) - 1u;

    // the file's header against the record (the host has made sure that header and table lie inside the file's bytes)
    const unsigned* word = reinterpret_cast<const unsigned*>(file);
    const unsigned long long start = fp::payload_start(((unsigned long long)f.height + fp::FP_ROWS - 1) / fp::FP_ROWS, (unsigned)C);
    const unsigned payload_bytes = word[6];
    bool ok = word[0] == 0x464E424Bu && word[1] == 0x00314D52u && word[2] == (unsigned)fw && word[3] == (unsigned)f.height &&
              word[4] == ((unsigned)C | (unsigned)bits << 16) && word[5] == ((unsigned)fp::FP_ROWS | (unsigned)fp::FP_SEG << 16) &&
              word[7] == 0u && start + payload_bytes == file_bytes;
    const unsigned entry = (unsigned)g * (unsigned)C + (unsigned)plane;
    const unsigned lo = word[8 + entry], hi = word[9 + entry];
    const int rows = min(fp::FP_ROWS, f.height - g * fp::FP_ROWS);
    const int S = (fw + fp::FP_SEG - 1) / fp::FP_SEG;
    const int nseg = rows * S;
    ok = ok && lo <= hi && hi <= payload_bytes && hi - lo >= (unsigned)nseg;
    if (!ok) return;
    const unsigned char* head = file + start + lo;   // nseg header bytes, then the segments
    const int last_n = fw - (S - 1) * fp::FP_SEG;

    // ---- 1. segment offsets ----
    {
        const int per = (nseg + UP_THREADS - 1) / UP_THREADS;
        const int e0 = min(nseg, tid * per), e1 = min(nseg, e0 + per);
        unsigned sum = 0;
        int r = e0 / S, k = e0 - r * S;
        for (int e = e0; e < e1; ++e) {
            sum += fp::segment_bytes(k == S - 1 ? last_n : fp::FP_SEG, min((int)head[e], bits), bits, r == 0);
            if (++k == S) { k = 0; ++r; }
        }
        unsigned incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(incl, d);
            if ((tid & 63) >= d) incl += t;
        }
        if ((tid & 63) == 63) wave_total[tid >> 6] = incl;
        __syncthreads();
        unsigned run = (unsigned)nseg + incl - sum, total = 0;
#pragma unroll
        for (int w = 0; w < UP_THREADS / 64; ++w) {
            if (w < (tid >> 6)) run += wave_total[w];
            total += wave_total[w];
        }
        r = e0 / S; k = e0 - r * S;
        for (int e = e0; e < e1; ++e) {
            seg_at[e] = run;
            run += fp::segment_bytes(k == S - 1 ? last_n : fp::FP_SEG, min((int)head[e], bits), bits, r == 0);
            if (++k == S) { k = 0; ++r; }
        }
        __syncthreads();
        if ((unsigned)nseg + total != hi - lo) return;   // the headers do not describe this payload
    }

    // ---- 2. and 3. decode and store, tile by tile ----
    const int r_first = max(0, f.y_start - g * fp::FP_ROWS), r_last = min(rows - 1, y_last - g * fp::FP_ROWS);
    const long long HW = (long long)p.height * p.width;
    const long long b = (long long)p.frame0 + blockIdx.z;
    const int slot = tid >> 4, j = tid & 15;
    const int reps = (!is_depth && C == 1) ? 3 : 1;
    for (int t = 0; t < 3; ++t) {
        float* dst = is_depth ? (t == 0 ? p.depth : nullptr) : (t == 0 ? p.image1 : t == 1 ? p.image0 : p.image2);   // by third: t-1, t, t+1
        if (!dst) continue;
        const int c0 = (is_depth ? 0 : t * W) + f.x_start;   // the crop's first column in the file
        float* out = dst + (is_depth ? b : b * 3 + (C == 1 ? 0 : plane)) * HW;
        for (int X0 = 0; X0 < p.width; X0 += UP_TILE) {
            const int tw = min(UP_TILE, p.width - X0);
            const int k_first = (c0 + X0) >> 4, k_last = (c0 + X0 + tw - 1) >> 4;
            const int k = k_first + slot;
            const bool live = k <= k_last && j < min(fp::FP_SEG, fw - k * fp::FP_SEG);
            unsigned val = 0;
            for (int r = 0; r <= r_last; ++r) {
                unsigned z = 0;
                if (live) {
                    const int e = r * S + k;
                    const int bw = min((int)head[e], bits);
                    const unsigned char* seg = head + seg_at[e];
                    if (r == 0) {
                        if (j == 0) z = read_field(seg, 0u, bits);
                        else if (bw) z = read_field(seg, (unsigned)(bits + (j - 1) * bw), bw);
                    } else if (bw) {
                        z = read_field(seg, (unsigned)(j * bw), bw);
                    }
                }
                if (r == 0) {   // the left row: raw sample in lane 0, differences in the others, an inclusive scan over the 16 lanes
                    unsigned v = j == 0 ? z : (unsigned)fp::unzigzag(z);
#pragma unroll
                    for (int d = 1; d < fp::FP_SEG; d <<= 1) {
                        const unsigned up = __shfl_up(v, d, fp::FP_SEG);
                        if (j >= d) v += up;
                    }
                    val = v & mask;
                } else {
                    val = (val + (unsigned)fp::unzigzag(z)) & mask;
                }
                if (r >= r_first) tile[r][tid] = (unsigned short)val;
            }
            __syncthreads();
            const int quads = (tw + 3) >> 2, items = (r_last - r_first + 1) * quads;
            const int phase = c0 + X0 - k_first * fp::FP_SEG;   // 0 .. 15: where the tile's first column sits in its first segment
            for (int i = tid; i < items; i += UP_THREADS) {
                const int rr = i / quads, q = i - rr * quads;
                const int r = r_first + rr;
                const unsigned short* s = &tile[r][phase + 4 * q];
                const int x = X0 + 4 * q;
                const int n_live = VEC ? 4 : min(4, p.width - x);
                f32x4 v;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const float s_f = (VEC || a < n_live) ? (float)s[a] : 0.f;
                    v[a] = is_depth ? s_f / 256.0f : s_f;
                }
                float* o = out + (long long)(g * fp::FP_ROWS + r - f.y_start) * p.width + x;
                for (int c = 0; c < reps; ++c) store_quad<VEC>(o + c * HW, v, n_live);
            }
            __syncthreads();
        }
    }
}

}  // namespace kbn

extern "C" int kbn_unpack_packed_frames_forward(const unsigned char* images, size_t image_bytes, const unsigned char* depths,
                                                size_t depth_bytes, const kbn_packed_frame* frames, int n, int height, int width,
                                                int image_channels, int depth_bits, float* image0, float* image1, float* image2,
                                                float* sparse_depth0, kbn_stream_t stream) {
    using namespace kbn;
    if (!images || !depths || !frames || !image0 || !sparse_depth0) return KBN_ERR_INVALID_ARGUMENT;
    if (n < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(depths)) & 15) return KBN_ERR_INVALID_ARGUMENT;
    const int C = image_channels;
    if ((C != 1 && C != 3 && C != 4) || (depth_bits != 8 && depth_bits != 16)) return KBN_ERR_UNSUPPORTED;
    int widest = 0;
    for (int i = 0; i < n; ++i) {   // every record before anything is launched
        const kbn_packed_frame& f = frames[i];
        if (!crop_in_frame(f.height, f.raw_width, f.y_start, f.x_start, height, width)) return KBN_ERR_INVALID_ARGUMENT;
        if (f.image_offset < 0 || f.depth_offset < 0 || (f.image_offset | f.depth_offset) & 15) return KBN_ERR_INVALID_ARGUMENT;
        const unsigned long long groups = ((unsigned long long)f.height + fp::FP_ROWS - 1) / fp::FP_ROWS;
        if (f.image_bytes < fp::payload_start(groups, (unsigned)C) || f.depth_bytes < fp::payload_start(groups, 1u))
            return KBN_ERR_INVALID_ARGUMENT;   // too short for its header and table
        if ((unsigned long long)f.image_offset + f.image_bytes > image_bytes || (unsigned long long)f.depth_offset + f.depth_bytes > depth_bytes)
            return KBN_ERR_INVALID_ARGUMENT;
        widest = std::max(widest, f.raw_width);
    }
    if (widest > KBN_UNPACK_PACKED_MAX_RAW_WIDTH) return KBN_ERR_UNSUPPORTED;   // the group's segment offsets must fit the LDS budget
    const bool vec = outputs_vectorizable(width, image0, image1, image2, sparse_depth0);
    UnpackPackedParams p;
    p.images = images; p.depths = depths;
    p.image0 = image0; p.image1 = image1; p.image2 = image2; p.depth = sparse_depth0;
    p.height = height; p.width = width; p.channels = C; p.depth_bits = depth_bits;
    for (int frame0 = 0; frame0 < n; frame0 += KBN_UNPACK_TRAIN_MAX_FRAMES) {
        const int count = std::min(n - frame0, (int)KBN_UNPACK_TRAIN_MAX_FRAMES);
        int groups = 1, segments = 1;
        for (int i = 0; i < KBN_UNPACK_TRAIN_MAX_FRAMES; ++i) {
            p.frame[i] = i < count ? frames[frame0 + i] : kbn_packed_frame{};
            if (i < count) {
                const kbn_packed_frame& f = p.frame[i];
                groups = std::max(groups, ((f.y_start + height - 1) >> 3) - (f.y_start >> 3) + 1);
                segments = std::max(segments, (f.raw_width + fp::FP_SEG - 1) / fp::FP_SEG);
            }
        }
        p.frame0 = frame0;
        const dim3 grid((unsigned)groups, (unsigned)std::min(C, 3) + 1u, (unsigned)count), block(UP_THREADS);
        const size_t lds = sizeof(unsigned) * fp::FP_ROWS * (size_t)segments;
        if (vec) hipLaunchKernelGGL((unpack_packed_kernel<true>), grid, block, lds, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((unpack_packed_kernel<false>), grid, block, lds, (hipStream_t)stream, p);
    }
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
