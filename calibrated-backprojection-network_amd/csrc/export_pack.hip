// export_pack.hip -- device side of the output pipeline: the three float tensors run_kbnet.py --save_outputs stores for a batch
// (reference src/kbnet.py:1007-1026) -> the bytes of their PNG files' pixels, in ONE launch.
//   image    n x 3 x h x w float32 (the NORMALISED image)  ->  rgb n x h x w x 3 uint8, interleaved (what Image.fromarray reads):
//            clamp(trunc(scale * v + shift), 0, 255), NaN -> 0.  The product and the sum are each rounded to fp32 (__fmul_rn,
//            __fadd_rn: never contracted into an FMA), so NumPy's float32 arithmetic gives the same bytes.  (255, 0) on an image
//            in [0, 1] is the reference's `(255 * image).astype(np.uint8)` (:1015).
//   depth_a, depth_b  n x 1 x h x w float32  ->  n x h x w uint16 = min(trunc(z * 256), 65535), NaN and negatives -> 0
//            (kbn_depth_to_u16_forward's rule: np.uint32(z * 256.0) and PIL's clip to the PNG's 16 bits)
// Byte work, HBM bound: 20 bytes in and 7 bytes out per pixel -- the reads are three quarters of the traffic, so they are what
// is laid out for: a thread owns 4 consecutive pixels of one row and takes each source with one 16-byte load (a wave reads 1 KiB
// of each plane contiguously); it writes 12 contiguous bytes of rgb and 8 of each sample plane, neighbouring lanes neighbouring
// bytes.  Rows whose width is no multiple of 4, or pointers off a 16-byte boundary, take the same kernel with scalar loads and
// stores.  Every output byte is written exactly once and nothing outside the three outputs is touched.
#include "export_rules.h"   // rgb8, depth16
#include "kbn_common.h"

namespace kbn {

// quads = n * h * ceil(w / 4): thread q owns pixels [4 xq, 4 xq + 4) of row r = q / ceil(w / 4) of the n * h rows
template <bool VEC>
__global__ __launch_bounds__(256) void export_pack_kernel(const float* __restrict__ image, float scale, float shift,
                                                          const float* __restrict__ depth_a, const float* __restrict__ depth_b,
                                                          unsigned char* __restrict__ rgb, unsigned short* __restrict__ samples_a,
                                                          unsigned short* __restrict__ samples_b, int H, int W, long long quads) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= quads) return;
    const int wq = (W + 3) >> 2;
    const int x0 = (int)(q % wq) * 4;
    const long long r = q / wq;                       // row of the batch: frame r / H, line r % H
    const long long HW = (long long)H * W;
    const long long pix = r * W + x0;                 // first pixel in an n x h x w plane
    const long long img = (r / H) * 3 * HW + (r % H) * (long long)W + x0;
    if (VEC) {                                        // W % 4 == 0: all four pixels exist, every address below is 16-byte aligned
        if (image) {
            const f32x4 cr = *reinterpret_cast<const f32x4*>(image + img);
            const f32x4 cg = *reinterpret_cast<const f32x4*>(image + img + HW);
            const f32x4 cb = *reinterpret_cast<const f32x4*>(image + img + 2 * HW);
            unsigned b[12];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                b[3 * i] = rgb8(cr[i], scale, shift); b[3 * i + 1] = rgb8(cg[i], scale, shift); b[3 * i + 2] = rgb8(cb[i], scale, shift);
            }
            unsigned* o = reinterpret_cast<unsigned*>(rgb + pix * 3);   // 12 bytes at a multiple of 12
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
        }
        if (depth_a) {
            const f32x4 z = *reinterpret_cast<const f32x4*>(depth_a + pix);
            uint2 s;
            s.x = depth16(z[0]) | (depth16(z[1]) << 16); s.y = depth16(z[2]) | (depth16(z[3]) << 16);
            *reinterpret_cast<uint2*>(samples_a + pix) = s;
        }
        if (depth_b) {
            const f32x4 z = *reinterpret_cast<const f32x4*>(depth_b + pix);
            uint2 s;
            s.x = depth16(z[0]) | (depth16(z[1]) << 16); s.y = depth16(z[2]) | (depth16(z[3]) << 16);
            *reinterpret_cast<uint2*>(samples_b + pix) = s;
        }
    } else {
        const int count = W - x0 < 4 ? W - x0 : 4;
        for (int i = 0; i < count; ++i) {
            if (image) {
                unsigned char* o = rgb + (pix + i) * 3;
                o[0] = (unsigned char)rgb8(image[img + i], scale, shift);
                o[1] = (unsigned char)rgb8(image[img + HW + i], scale, shift);
                o[2] = (unsigned char)rgb8(image[img + 2 * HW + i], scale, shift);
            }
            if (depth_a) samples_a[pix + i] = (unsigned short)depth16(depth_a[pix + i]);
            if (depth_b) samples_b[pix + i] = (unsigned short)depth16(depth_b[pix + i]);
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace kbn

extern "C" int kbn_export_pack_forward(const float* image, float scale, float shift, const float* depth_a, const float* depth_b,
                                       unsigned char* rgb, unsigned short* samples_a, unsigned short* samples_b, int n, int height,
                                       int width, kbn_stream_t stream) {
    using namespace kbn;
    if (n < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    if ((image != nullptr) != (rgb != nullptr) || (depth_a != nullptr) != (samples_a != nullptr) ||
        (depth_b != nullptr) != (samples_b != nullptr))
        return KBN_ERR_INVALID_ARGUMENT;
    if (!image && !depth_a && !depth_b) return KBN_ERR_INVALID_ARGUMENT;
    const long long quads = (long long)n * height * ((width + 3) >> 2);
    if (quads > 0x7fffffffLL * 256LL) return KBN_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((quads + 255) / 256)), block(256);
    // a NULL pointer is aligned: an absent source does not decide the path
    const bool vec = width % 4 == 0 && aligned16(image) && aligned16(depth_a) && aligned16(depth_b) && aligned16(rgb) &&
                     aligned16(samples_a) && aligned16(samples_b);
    if (vec)
        hipLaunchKernelGGL(export_pack_kernel<true>, grid, block, 0, (hipStream_t)stream, image, scale, shift, depth_a, depth_b, rgb,
                           samples_a, samples_b, height, width, quads);
    else
        hipLaunchKernelGGL(export_pack_kernel<false>, grid, block, 0, (hipStream_t)stream, image, scale, shift, depth_a, depth_b, rgb,
                           samples_a, samples_b, height, width, quads);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
