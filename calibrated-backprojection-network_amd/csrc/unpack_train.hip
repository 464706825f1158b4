// unpack_train.hip -- device side of the TRAINING input pipeline (kbn_unpack_train_frames_forward): the decoded bytes of a batch of
// image triplets and depth maps -> what KBNetTrainingDataset.__getitem__ returns (reference src/datasets.py:199-225), batched:
//   image0 / image1 / image2   the middle (t), left (t-1) and right (t+1) third of the triplet (load_image_triplet, :22-46), cropped
//                              (random_crop's slices, :143-148), as float32 N x 3 x h x w, values 0..255 (normalize=False; gray is
//                              replicated and alpha dropped, which is what PIL's convert('RGB') does, src/data_utils.py:75)
//   sparse_depth0              the depth samples of the same crop / 256, float32 N x 1 x h x w (data_utils.load_depth,
//                              src/data_utils.py:137-141; `z[z <= 0] = 0` is a no-op on unsigned samples)
// KITTI's raw frames come in several sizes, which is why the reference crops before it batches: every frame of a launch has its
// own raw size, its own place in the two packed buffers and its own crop origin.  These records (kbn_train_frame, 32 bytes) travel BY
// VALUE in the kernel arguments, KBN_UNPACK_TRAIN_MAX_FRAMES a launch: no device table, no copy, no allocation.  A workgroup belongs
// to one frame (blockIdx.y), so its record is read with scalar loads from the argument segment.
//
// One thread per four consecutive output pixels of a row, for all four tensors: 3 x 4 C + 4 x 2 bytes in (the source starts at byte
// x_start C of a row: any alignment, so plain byte loads), 3 x 3 + 1 = 10 stores of 16 bytes out when w % 4 == 0 and the outputs are
// 16-byte aligned (a wave then writes 1 KiB of a row per instruction), float by float otherwise.  3 C + 2 bytes in and 40 bytes out a
// pixel: store bound.  Exact conversions only (uint8 / uint16 -> fp32, a division by 256).
#include "unpack_common.h"

namespace kbn {

constexpr int UT_THREADS = 256;

struct UnpackTrainParams {
    kbn_train_frame frame[KBN_UNPACK_TRAIN_MAX_FRAMES];   // of this launch
    const unsigned char* images;
    const unsigned char* depths;
    float* image0;
    float* image1;
    float* image2;
    float* depth;
    int frame0;          // the batch index of the launch's first frame
    int height, width;   // the crop
    unsigned quads;      // height x ceil(width / 4): the threads a frame takes
};
static_assert(sizeof(kbn_train_frame) == 32 && sizeof(UnpackTrainParams) <= 3584, "the records must fit the kernel-argument segment");

template <int C, typename DepthT, bool VEC>
__global__ __launch_bounds__(UT_THREADS) void unpack_train_kernel(const UnpackTrainParams p) {
    const unsigned q = blockIdx.x * (unsigned)UT_THREADS + threadIdx.x;
    if (q >= p.quads) return;
    const unsigned wq = (unsigned)(p.width + 3) >> 2;
    const int y = (int)(q / wq), x0 = (int)(q - (unsigned)y * wq) * 4;
    const kbn_train_frame& f = p.frame[blockIdx.y];
    const int W = f.raw_width / 3;
    const long long row = (long long)f.y_start + y, col = (long long)f.x_start + x0;
    const unsigned char* src = p.images + f.image_offset + (row * f.raw_width + col) * C;   // in the left third
    const DepthT* sd = reinterpret_cast<const DepthT*>(p.depths + f.depth_offset) + row * W + col;
    const long long HW = (long long)p.height * p.width;
    const long long b = (long long)p.frame0 + blockIdx.y, at = (long long)y * p.width + x0;
    const int live = VEC ? 4 : min(4, p.width - x0);
    float* const out[3] = {p.image1, p.image0, p.image2};   // by third: t-1, t, t+1
#pragma unroll
    for (int t = 0; t < 3; ++t) convert_store_pixels<C, VEC>(src + (long long)t * W * C, out[t] + b * 3 * HW + at, HW, live);
    convert_store_depth<DepthT, VEC>(sd, p.depth + b * HW + at, live);
}

template <int C, typename DepthT>
static void launch_unpack_train(const UnpackTrainParams& p, int frames, bool vec, hipStream_t st) {
    const dim3 grid((p.quads + UT_THREADS - 1) / UT_THREADS, (unsigned)frames), block(UT_THREADS);
    if (vec) hipLaunchKernelGGL((unpack_train_kernel<C, DepthT, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((unpack_train_kernel<C, DepthT, false>), grid, block, 0, st, p);
}

}  // namespace kbn

extern "C" int kbn_unpack_train_frames_forward(const unsigned char* images, size_t image_bytes, const unsigned char* depths,
                                               size_t depth_bytes, const kbn_train_frame* frames, int n, int height, int width,
                                               int image_channels, int depth_bits, float* image0, float* image1, float* image2,
                                               float* sparse_depth0, kbn_stream_t stream) {
    using namespace kbn;
    if (!images || !depths || !frames || !image0 || !image1 || !image2 || !sparse_depth0) return KBN_ERR_INVALID_ARGUMENT;
    if (n < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    const int C = image_channels;
    if ((C != 1 && C != 3 && C != 4) || (depth_bits != 8 && depth_bits != 16)) return KBN_ERR_UNSUPPORTED;
    const long long sample = depth_bits / 8;
    for (int i = 0; i < n; ++i) {   // every record before anything is launched
        const kbn_train_frame& f = frames[i];
        if (!crop_in_frame(f.height, f.raw_width, f.y_start, f.x_start, height, width)) return KBN_ERR_INVALID_ARGUMENT;
        const long long W = f.raw_width / 3;
        if (f.image_offset < 0 || f.depth_offset < 0 || f.depth_offset % sample != 0) return KBN_ERR_INVALID_ARGUMENT;
        const unsigned long long image_end = (unsigned long long)f.image_offset + (unsigned long long)f.height * f.raw_width * C;
        const unsigned long long depth_end = (unsigned long long)f.depth_offset + (unsigned long long)f.height * W * sample;
        if (image_end > image_bytes || depth_end > depth_bytes) return KBN_ERR_INVALID_ARGUMENT;
    }
    const long long quads = (long long)height * ((width + 3) >> 2);
    if (quads > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    const bool vec = outputs_vectorizable(width, image0, image1, image2, sparse_depth0);
    UnpackTrainParams p;
    p.images = images; p.depths = depths;
    p.image0 = image0; p.image1 = image1; p.image2 = image2; p.depth = sparse_depth0;
    p.height = height; p.width = width; p.quads = (unsigned)quads;
    for (int frame0 = 0; frame0 < n; frame0 += KBN_UNPACK_TRAIN_MAX_FRAMES) {
        const int count = std::min(n - frame0, (int)KBN_UNPACK_TRAIN_MAX_FRAMES);
        for (int i = 0; i < KBN_UNPACK_TRAIN_MAX_FRAMES; ++i) p.frame[i] = i < count ? frames[frame0 + i] : kbn_train_frame{};
        p.frame0 = frame0;
        auto go = [&](auto depth_type) {
            using D = decltype(depth_type);
            switch (C) {
                case 1: launch_unpack_train<1, D>(p, count, vec, (hipStream_t)stream); break;
                case 3: launch_unpack_train<3, D>(p, count, vec, (hipStream_t)stream); break;
                default: launch_unpack_train<4, D>(p, count, vec, (hipStream_t)stream); break;
            }
        };
        if (depth_bits == 16) go((unsigned short)0);
        else go((unsigned char)0);
    }
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
