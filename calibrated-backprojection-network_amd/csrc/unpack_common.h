// unpack_common.h -- what the two record-driven unpack translation units (unpack_train.hip, unpack_packed.hip) share: how a
// thread stores four output pixels, and the entry points' checks that do not depend on the record's layout.
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

// a record's raw size is that of a triplet, and the h x w crop at (y_start, x_start) lies inside each of its thirds
inline bool crop_in_frame(int height, int raw_width, int y_start, int x_start, int h, int w) {
    if (height < 1 || raw_width < 3 || raw_width % 3 != 0) return false;
    return y_start >= 0 && (long long)y_start + h <= height && x_start >= 0 && (long long)x_start + w <= raw_width / 3;
}

// whether every thread may use 16-byte stores: whole quads in a row, and every output 16-byte aligned (an output left out, a null
// pointer, counts as aligned)
inline bool outputs_vectorizable(int width, const float* image0, const float* image1, const float* image2, const float* depth) {
    return width % 4 == 0 && ((reinterpret_cast<uintptr_t>(image0) | reinterpret_cast<uintptr_t>(image1) |
                               reinterpret_cast<uintptr_t>(image2) | reinterpret_cast<uintptr_t>(depth)) & 15) == 0;
}

}  // namespace kbn
