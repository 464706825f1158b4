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
//
// Steps 1 to 3 and the checks are unpack_packed_unit.h, which the decoder of one file per frame (unpack_sequence.hip) shares; the
// kernel here says which file, plane and group a workgroup owns and where the three thirds begin in the triplet's rows.
#include "unpack_packed_unit.h"

namespace kbn {

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

template <bool VEC>
__global__ __launch_bounds__(UP_THREADS) void unpack_packed_kernel(const UnpackPackedParams p) {
    const kbn_packed_frame& f = p.frame[blockIdx.z];
    const int W = f.raw_width / 3;
    const int g = (f.y_start >> 3) + (int)blockIdx.x;
    if (g > ((f.y_start + p.height - 1) >> 3)) return;   // this frame's crop spans fewer groups than the widest of the launch
    const bool is_depth = blockIdx.y + 1 == gridDim.y;
    const int C = is_depth ? 1 : p.channels, plane = is_depth ? 0 : (int)blockIdx.y;
    const long long HW = (long long)p.height * p.width;
    const long long b = (long long)p.frame0 + blockIdx.z;
    const long long at = (is_depth ? b : b * 3 + (C == 1 ? 0 : plane)) * HW;
    // by third: t-1, t, t+1; the depth map is one frame wide
    float* const out[3] = {is_depth ? p.depth + at : p.image1 ? p.image1 + at : nullptr, is_depth ? nullptr : p.image0 + at,
                           is_depth || !p.image2 ? nullptr : p.image2 + at};
    const int c0[3] = {f.x_start, W + f.x_start, 2 * W + f.x_start};   // the crop's first column in the file
    unpack_packed_unit<VEC>(is_depth ? p.depths + f.depth_offset : p.images + f.image_offset, is_depth ? f.depth_bytes : f.image_bytes,
                            is_depth ? W : f.raw_width, f.height, C, is_depth ? p.depth_bits : 8, plane, g, f.y_start, p.height,
                            p.width, out, c0, HW, (!is_depth && C == 1) ? 3 : 1, is_depth);
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
