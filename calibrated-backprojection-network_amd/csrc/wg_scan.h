// wg_scan.h -- what the byte-stream writers (pack_frames.hip, point_cloud.hip) share: a 256-thread workgroup's sum and prefix sum,
// and the copy of an LDS image to global memory in whole 16-byte words.  Every thread of the workgroup makes every call (the
// functions hold __syncthreads and wave shuffles).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kbn {

constexpr int WG_THREADS = 256;

// the sum of v over the workgroup, in every thread; `wave_total` is WG_THREADS / 64 words of LDS (reusable after the call)
__device__ __forceinline__ unsigned wg_sum(unsigned v, unsigned* wave_total) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();   // earlier readers of wave_total are done
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int w = 0; w < WG_THREADS / 64; ++w) total += wave_total[w];
    return total;
}

// the inclusive prefix sum of v over the workgroup in thread order; *total receives the workgroup's sum
__device__ __forceinline__ unsigned wg_scan(unsigned v, unsigned* wave_total, unsigned* total) {
    const int tid = (int)threadIdx.x;
    unsigned incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d);
        if ((tid & 63) >= d) incl += t;
    }
    __syncthreads();
    if ((tid & 63) == 63) wave_total[tid >> 6] = incl;
    __syncthreads();
    unsigned sum = 0;
#pragma unroll
    for (int w = 0; w < WG_THREADS / 64; ++w) {
        if (w < (tid >> 6)) incl += wave_total[w];
        sum += wave_total[w];
    }
    *total = sum;
    return incl;
}

// LDS bytes [phase, phase + bytes) of `image` -> dst[0, bytes), where phase = dst mod 16: 16-byte words that lie inside the range are
// stored whole, the others byte by byte; nothing else is written
__device__ __forceinline__ void wg_flush(const unsigned* image, unsigned phase, unsigned char* dst, unsigned bytes) {
    const unsigned char* image_bytes = reinterpret_cast<const unsigned char*>(image);
    unsigned char* origin = dst - phase;   // 16-byte aligned
    const unsigned end = phase + bytes;
    for (unsigned w = threadIdx.x; w * 16u < end; w += WG_THREADS) {
        const unsigned lo = w * 16u, hi = lo + 16u;
        if (lo >= phase && hi <= end) {
            *reinterpret_cast<uint4*>(origin + lo) = *reinterpret_cast<const uint4*>(image_bytes + lo);
        } else {
            for (unsigned i = max(lo, phase); i < min(hi, end); ++i) origin[i] = image_bytes[i];
        }
    }
}

}  // namespace kbn
