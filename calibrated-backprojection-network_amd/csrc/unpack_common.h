// unpack_common.h -- what the record-driven unpack translation units (unpack_train.hip, unpack_packed.hip, unpack_sequence.hip) share:
// how a thread converts and stores four output pixels, and the entry points' checks that do not depend on the record's layout.
#pragma once
#include "kbn_common.h"

namespace kbn {

// four consecutive floats of an output row: one 16-byte store (VEC: `o` is 16-byte aligned), else float by float up to `live`
template <bool VEC>
__device__ __forceinline__ void store_quad(float* o, f32x4 v, int live) {
    if constexpr (VEC) {
        *reinterpret_cast<f32x4*>(o) = v;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < live) o[i] = v[i];
    }
}

// four consecutive pixels of one frame, C interleaved uint8 channels at `s`, to the three planes of an N x 3 x h x w output at `o`
// (HW apart): gray replicated, alpha dropped.  The first `live` pixels exist (all four with VEC).
template <int C, bool VEC>
__device__ __forceinline__ void convert_store_pixels(const unsigned char* s, float* o, long long HW, int live) {
    f32x4 v[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool in = VEC || i < live;
        const float c0 = in ? (float)s[i * C] : 0.f;
        v[0][i] = c0;
        v[1][i] = C >= 3 ? (in ? (float)s[i * C + 1] : 0.f) : c0;
        v[2][i] = C >= 3 ? (in ? (float)s[i * C + 2] : 0.f) : c0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) store_quad<VEC>(o + c * HW, v[c], live);
}

// four consecutive depth samples at `sd` -> sample / 256 at `od`
template <typename DepthT, bool VEC>
__device__ __forceinline__ void convert_store_depth(const DepthT* sd, float* od, int live) {
    f32x4 z;
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = (VEC || i < live) ? (float)sd[i] / 256.0f : 0.f;
    store_quad<VEC>(od, z, live);
}

// a record's raw size is that of a triplet, and the h x w crop at (y_start, x_start) lies inside each of its thirds
inline bool crop_in_frame(int height, int raw_width, int y_start, int x_start, int h, int w) {
    if (height < 1 || raw_width < 3 || raw_width % 3 != 0) return false;
    return y_start >= 0 && (long long)y_start + h <= height && x_start >= 0 && (long long)x_start + w <= raw_width / 3;
}

// the same for a record that holds a single frame's size (the sequence entry points)
inline bool crop_in_single_frame(int height, int frame_width, int y_start, int x_start, int h, int w) {
    if (height < 1 || frame_width < 1) return false;
    return y_start >= 0 && (long long)y_start + h <= height && x_start >= 0 && (long long)x_start + w <= frame_width;
}

// whether every thread may use 16-byte stores: whole quads in a row, and every output 16-byte aligned (an output left out, a null
// pointer, counts as aligned)
inline bool outputs_vectorizable(int width, const float* image0, const float* image1, const float* image2, const float* depth) {
    return width % 4 == 0 && ((reinterpret_cast<uintptr_t>(image0) | reinterpret_cast<uintptr_t>(image1) |
                               reinterpret_cast<uintptr_t>(image2) | reinterpret_cast<uintptr_t>(depth)) & 15) == 0;
}

}  // namespace kbn
