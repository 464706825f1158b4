// export_rules.h -- the two conversions of the output files' pixels (reference src/kbnet.py:1007-1026), stated once: export_pack.hip
// writes them into the PNG / packed files, point_cloud.hip gives a point the colour its pixel has in the image file.
#pragma once

#include <hip/hip_runtime.h>

namespace kbn {

// clamp(trunc(scale * v + shift), 0, 255), NaN -> 0.  The product and the sum are each rounded to fp32 (never contracted into an
// FMA), so NumPy's float32 arithmetic gives the same byte.
__device__ __forceinline__ unsigned rgb8(float v, float scale, float shift) {
    const float x = __fadd_rn(__fmul_rn(scale, v), shift);
    return x >= 255.0f ? 255u : (x >= 0.f ? (unsigned)x : 0u);   // NaN fails both comparisons -> 0
}
// min(trunc(z * 256), 65535), NaN and negatives -> 0
__device__ __forceinline__ unsigned depth16(float z) {
    const float v = z * 256.0f;   // exact in fp32
    return v >= 65535.0f ? 65535u : (v >= 0.f ? (unsigned)v : 0u);
}

}  // namespace kbn
