// unpack_sequence.hip -- the training (and inference) batch from samples that name their three frames one by one:
// kbn_unpack_sequence_frames_forward is kbn_unpack_train_frames_forward, and kbn_unpack_packed_sequence_frames_forward is
// kbn_unpack_packed_frames_forward, for frames t-1, t, t+1 that lie at three places of their own in the image buffer instead of
// side by side in one triplet (load_image_triplet, reference src/datasets.py:22-46, splits what the reference's setup scripts
// concatenated; here nothing is concatenated).  The outputs are the triplet path's, bit for bit.
//
// Decoded bytes (unpack_train.hip's thread: four consecutive output pixels of a row, of all four tensors): a frame's row is W
// pixels long, not 3 W, and each of the three sources has its own base.  The three offsets of a sample may be one offset, and
// samples may share frames: everything is read-only.
//
// Packed files (unpack_packed.hip's workgroup, unpack_packed_unit.h): blockIdx.z the sample, blockIdx.x the row group counted from
// the crop's first one, blockIdx.y the (file, plane): the planes of previous, current and next -- of current alone when image1 and
// image2 are left out -- then the depth file's one.  A unit decodes ONE output from its file, and the crop's first column is x_start
// in every file: each frame starts at segment 0, where the second and third frame of a triplet file start mid-segment unless
// W % 16 == 0.  Three coinciding offsets decode the same file three times, into three outputs.
//
// The records (kbn_sequence_frame 48 bytes, kbn_packed_sequence_frame 64) travel by value in the kernel arguments,
// KBN_UNPACK_SEQUENCE_MAX_FRAMES a launch.
#include "unpack_packed_unit.h"

namespace kbn {

constexpr int US_THREADS = 256;

struct UnpackSequenceParams {
    kbn_sequence_frame frame[KBN_UNPACK_SEQUENCE_MAX_FRAMES];   // of this launch
    const unsigned char* images;
    const unsigned char* depths;
    float* image0;
    float* image1;
    float* image2;
    float* depth;
    int frame0;          // the batch index of the launch's first sample
    int height, width;   // the crop
    unsigned quads;      // height x ceil(width / 4): the threads a sample takes
};
static_assert(sizeof(kbn_sequence_frame) == 48 && sizeof(UnpackSequenceParams) <= 3584, "the records must fit the kernel-argument segment");

template <int C, typename DepthT, bool VEC>
__global__ __launch_bounds__(US_THREADS) void unpack_sequence_kernel(const UnpackSequenceParams p) {
    const unsigned q = blockIdx.x * (unsigned)US_THREADS + threadIdx.x;
    if (q >= p.quads) return;
    const unsigned wq = (unsigned)(p.width + 3) >> 2;
    const int y = (int)(q / wq), x0 = (int)(q - (unsigned)y * wq) * 4;
    const kbn_sequence_frame& f = p.frame[blockIdx.y];
    const long long pixel = ((long long)f.y_start + y) * f.width + f.x_start + x0;   // in every frame and in the depth map
    const long long HW = (long long)p.height * p.width;
    const long long b = (long long)p.frame0 + blockIdx.y, at = (long long)y * p.width + x0;
    const int live = VEC ? 4 : min(4, p.width - x0);
    float* const out[3] = {p.image1, p.image0, p.image2};   // by frame: t-1, t, t+1
#pragma unroll
    for (int t = 0; t < 3; ++t)
        convert_store_pixels<C, VEC>(p.images + f.image_offset[t] + pixel * C, out[t] + b * 3 * HW + at, HW, live);
    convert_store_depth<DepthT, VEC>(reinterpret_cast<const DepthT*>(p.depths + f.depth_offset) + pixel, p.depth + b * HW + at, live);
}

template <int C, typename DepthT>
static void launch_unpack_sequence(const UnpackSequenceParams& p, int frames, bool vec, hipStream_t st) {
    const dim3 grid((p.quads + US_THREADS - 1) / US_THREADS, (unsigned)frames), block(US_THREADS);
    if (vec) hipLaunchKernelGGL((unpack_sequence_kernel<C, DepthT, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((unpack_sequence_kernel<C, DepthT, false>), grid, block, 0, st, p);
}

struct UnpackPackedSequenceParams {
    kbn_packed_sequence_frame frame[KBN_UNPACK_SEQUENCE_MAX_FRAMES];   // of this launch
    const unsigned char* images;
    const unsigned char* depths;
    float* image0;
    float* image1;       // null together with image2: only the current file of a sample is decoded
    float* image2;
    float* depth;
    int frame0;          // the batch index of the launch's first sample
    int height, width;   // the crop
    int channels;        // of the image files
    int depth_bits;
};
static_assert(sizeof(kbn_packed_sequence_frame) == 64 && sizeof(UnpackPackedSequenceParams) <= 3584,
              "the records must fit the kernel-argument segment");

template <bool VEC>
__global__ __launch_bounds__(UP_THREADS) void unpack_packed_sequence_kernel(const UnpackPackedSequenceParams p) {
    const kbn_packed_sequence_frame& f = p.frame[blockIdx.z];
    const int g = (f.y_start >> 3) + (int)blockIdx.x;
    if (g > ((f.y_start + p.height - 1) >> 3)) return;   // this sample's crop spans fewer groups than the widest of the launch
    const bool is_depth = blockIdx.y + 1 == gridDim.y;
    const int planes = min(p.channels, 3);
    const int which = is_depth ? 1 : p.image1 ? (int)blockIdx.y / planes : 1;   // 0 previous, 1 current, 2 next
    const int C = is_depth ? 1 : p.channels, plane = is_depth ? 0 : (int)blockIdx.y % planes;
    const long long HW = (long long)p.height * p.width;
    const long long b = (long long)p.frame0 + blockIdx.z;
    float* const dst = is_depth ? p.depth : which == 0 ? p.image1 : which == 1 ? p.image0 : p.image2;
    float* const out[3] = {dst + (is_depth ? b : b * 3 + (C == 1 ? 0 : plane)) * HW, nullptr, nullptr};
    const int c0[3] = {f.x_start, 0, 0};   // every file starts at column 0 of its frame
    unpack_packed_unit<VEC>(is_depth ? p.depths + f.depth_offset : p.images + f.image_offset[which],
                            is_depth ? f.depth_bytes : f.image_bytes[which], f.width, f.height, C, is_depth ? p.depth_bits : 8, plane,
                            g, f.y_start, p.height, p.width, out, c0, HW, (!is_depth && C == 1) ? 3 : 1, is_depth);
}

}  // namespace kbn

extern "C" int kbn_unpack_sequence_frames_forward(const unsigned char* images, size_t image_bytes, const unsigned char* depths,
                                                  size_t depth_bytes, const kbn_sequence_frame* frames, int n, int height, int width,
                                                  int image_channels, int depth_bits, float* image0, float* image1, float* image2,
                                                  float* sparse_depth0, kbn_stream_t stream) {
    using namespace kbn;
    if (!images || !depths || !frames || !image0 || !image1 || !image2 || !sparse_depth0) return KBN_ERR_INVALID_ARGUMENT;
    if (n < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    const int C = image_channels;
    if ((C != 1 && C != 3 && C != 4) || (depth_bits != 8 && depth_bits != 16)) return KBN_ERR_UNSUPPORTED;
    const long long sample = depth_bits / 8;
    for (int i = 0; i < n; ++i) {   // every record before anything is launched
        const kbn_sequence_frame& f = frames[i];
        if (!crop_in_single_frame(f.height, f.width, f.y_start, f.x_start, height, width)) return KBN_ERR_INVALID_ARGUMENT;
        const unsigned long long frame_bytes = (unsigned long long)f.height * f.width * C;
        for (int t = 0; t < 3; ++t)
            if (f.image_offset[t] < 0 || (unsigned long long)f.image_offset[t] + frame_bytes > image_bytes) return KBN_ERR_INVALID_ARGUMENT;
        if (f.depth_offset < 0 || f.depth_offset % sample != 0) return KBN_ERR_INVALID_ARGUMENT;
        if ((unsigned long long)f.depth_offset + (unsigned long long)f.height * f.width * sample > depth_bytes) return KBN_ERR_INVALID_ARGUMENT;
    }
    const long long quads = (long long)height * ((width + 3) >> 2);
    if (quads > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    const bool vec = outputs_vectorizable(width, image0, image1, image2, sparse_depth0);
    UnpackSequenceParams p;
    p.images = images; p.depths = depths;
    p.image0 = image0; p.image1 = image1; p.image2 = image2; p.depth = sparse_depth0;
    p.height = height; p.width = width; p.quads = (unsigned)quads;
    for (int frame0 = 0; frame0 < n; frame0 += KBN_UNPACK_SEQUENCE_MAX_FRAMES) {
        const int count = std::min(n - frame0, (int)KBN_UNPACK_SEQUENCE_MAX_FRAMES);
        for (int i = 0; i < KBN_UNPACK_SEQUENCE_MAX_FRAMES; ++i) p.frame[i] = i < count ? frames[frame0 + i] : kbn_sequence_frame{};
        p.frame0 = frame0;
        auto go = [&](auto depth_type) {
            using D = decltype(depth_type);
            switch (C) {
                case 1: launch_unpack_sequence<1, D>(p, count, vec, (hipStream_t)stream); break;
                case 3: launch_unpack_sequence<3, D>(p, count, vec, (hipStream_t)stream); break;
                default: launch_unpack_sequence<4, D>(p, count, vec, (hipStream_t)stream); break;
            }
        };
        if (depth_bits == 16) go((unsigned short)0);
        else go((unsigned char)0);
    }
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_unpack_packed_sequence_frames_forward(const unsigned char* images, size_t image_bytes, const unsigned char* depths,
                                                         size_t depth_bytes, const kbn_packed_sequence_frame* frames, int n, int height,
                                                         int width, int image_channels, int depth_bits, float* image0, float* image1,
                                                         float* image2, float* sparse_depth0, kbn_stream_t stream) {
    using namespace kbn;
    if (!images || !depths || !frames || !image0 || !sparse_depth0 || !image1 != !image2) return KBN_ERR_INVALID_ARGUMENT;
    if (n < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(depths)) & 15) return KBN_ERR_INVALID_ARGUMENT;
    const int C = image_channels;
    if ((C != 1 && C != 3 && C != 4) || (depth_bits != 8 && depth_bits != 16)) return KBN_ERR_UNSUPPORTED;
    int widest = 0;
    for (int i = 0; i < n; ++i) {   // every record before anything is launched
        const kbn_packed_sequence_frame& f = frames[i];
        if (!crop_in_single_frame(f.height, f.width, f.y_start, f.x_start, height, width)) return KBN_ERR_INVALID_ARGUMENT;
        const unsigned long long groups = ((unsigned long long)f.height + fp::FP_ROWS - 1) / fp::FP_ROWS;
        for (int t = 0; t < 3; ++t) {
            if (f.image_offset[t] < 0 || f.image_offset[t] & 15) return KBN_ERR_INVALID_ARGUMENT;
            if (f.image_bytes[t] < fp::payload_start(groups, (unsigned)C)) return KBN_ERR_INVALID_ARGUMENT;   // too short for its header and table
            if ((unsigned long long)f.image_offset[t] + f.image_bytes[t] > image_bytes) return KBN_ERR_INVALID_ARGUMENT;
        }
        if (f.depth_offset < 0 || f.depth_offset & 15 || f.depth_bytes < fp::payload_start(groups, 1u)) return KBN_ERR_INVALID_ARGUMENT;
        if ((unsigned long long)f.depth_offset + f.depth_bytes > depth_bytes) return KBN_ERR_INVALID_ARGUMENT;
        widest = std::max(widest, f.width);
    }
    if (widest > KBN_UNPACK_PACKED_MAX_RAW_WIDTH) return KBN_ERR_UNSUPPORTED;   // the group's segment offsets must fit the LDS budget
    const bool vec = outputs_vectorizable(width, image0, image1, image2, sparse_depth0);
    UnpackPackedSequenceParams p;
    p.images = images; p.depths = depths;
    p.image0 = image0; p.image1 = image1; p.image2 = image2; p.depth = sparse_depth0;
    p.height = height; p.width = width; p.channels = C; p.depth_bits = depth_bits;
    const unsigned units = (image1 ? 3u : 1u) * (unsigned)std::min(C, 3) + 1u;   // (file, plane) pairs of a sample, the depth plane last
    for (int frame0 = 0; frame0 < n; frame0 += KBN_UNPACK_SEQUENCE_MAX_FRAMES) {
        const int count = std::min(n - frame0, (int)KBN_UNPACK_SEQUENCE_MAX_FRAMES);
        int groups = 1, segments = 1;
        for (int i = 0; i < KBN_UNPACK_SEQUENCE_MAX_FRAMES; ++i) {
            p.frame[i] = i < count ? frames[frame0 + i] : kbn_packed_sequence_frame{};
            if (i < count) {
                const kbn_packed_sequence_frame& f = p.frame[i];
                groups = std::max(groups, ((f.y_start + height - 1) >> 3) - (f.y_start >> 3) + 1);
                segments = std::max(segments, (f.width + fp::FP_SEG - 1) / fp::FP_SEG);
            }
        }
        p.frame0 = frame0;
        const dim3 grid((unsigned)groups, units, (unsigned)count), block(UP_THREADS);
        const size_t lds = sizeof(unsigned) * fp::FP_ROWS * (size_t)segments;
        if (vec) hipLaunchKernelGGL((unpack_packed_sequence_kernel<true>), grid, block, lds, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((unpack_packed_sequence_kernel<false>), grid, block, lds, (hipStream_t)stream, p);
    }
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
