// frame_pack.h -- the layout of a packed frame, version 1, shared by the host codec (frame_pack.hip) and the device
// decoder (unpack_packed.hip).  All multi-byte fields are little-endian.
//   header  32 bytes: magic "KBNFRM1\0", width u32, height u32, channels u16, bits u16, rows per group u16 (8),
//           samples per segment u16 (16), payload_bytes u64
//   table   ceil(height / 8) x channels + 1 offsets (u32, relative to the payload's start) in (group, plane) order; the last one
//           equals payload_bytes; zero padding follows so that the payload starts at a multiple of 16
//   payload per (group, plane): one header byte b per segment in (row in group, segment) order, then the segments' fields in the
//           same order, b bits each, LSB first, every segment padded with zero bits to a whole byte
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kbn {
namespace fp {

constexpr int FP_ROWS = 8;        // rows of a group
constexpr int FP_SEG = 16;        // samples of a segment
constexpr int FP_HEADER = 32;     // bytes

// bytes a segment's fields take: n samples, header byte b, sample width `bits`; a left row (the first of its group) stores its first
// sample raw and n - 1 differences to the left neighbour, an up row n differences to the row above
__host__ __device__ inline unsigned segment_bytes(int n, int b, int bits, bool left_row) {
    return (unsigned)((left_row ? bits + (n - 1) * b : n * b) + 7) >> 3;
}

// where the payload starts: header and table, padded to 16
__host__ __device__ inline unsigned long long payload_start(unsigned long long groups, unsigned channels) {
    return (FP_HEADER + 4ull * (groups * channels + 1) + 15ull) & ~15ull;
}

// residual -> field and back; d is the representative in [-2^(bits-1), 2^(bits-1) - 1] of a difference mod 2^bits
__host__ __device__ inline unsigned zigzag(int d) { return d >= 0 ? 2u * (unsigned)d : 2u * (unsigned)(-(d + 1)) + 1u; }
__host__ __device__ inline int unzigzag(unsigned z) { return (int)(z >> 1) ^ -(int)(z & 1u); }

}  // namespace fp
}  // namespace kbn
