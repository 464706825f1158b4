// point_cloud.hip -- kbn_point_cloud_forward: a batch of depth maps backprojected to the vertex records of binary PLY files.
// Frame i's slot receives, in row-major pixel order, one packed little-endian record per KEPT pixel -- float x, y, z, then uchar
// r, g, b when an image is given: 15 bytes, or 12, no padding -- and out_points[i] their number.
//   kept    d finite, d > 0, min_depth <= d <= max_depth (NaN, +-Inf, zero and negatives never)
//   point   camera_coordinate(kinv, j, x, y) * d, one __fmul_rn a component: kbn_camera_coordinates' value (camera_coordinate.h is
//           the one statement of it) times the depth, as the reference's backproject_to_camera (src/net_utils.py:1638-1667)
//   colour  export_rules.h's rgb8 of the normalised image: the bytes of the image file's pixel
// The number of records before a pixel is a prefix sum over the frame, so nothing can be placed in one pass without one workgroup
// waiting for another.  Three launches a call instead, whatever n is (as pack_frames.hip):
//   1. count  a workgroup (256 threads) owns a TILE of 1024 consecutive pixels of one frame's flattened plane, four a thread, taken
//             with one 16-byte load where the address allows it, by scalar loads otherwise (odd planes, channel slices, the ragged
//             end).  The tile's kept count goes to the workspace.
//   2. scan   a workgroup per frame turns the frame's counts into their exclusive prefix sums, in place, 256 tiles a round with a
//             carry, and writes out_points[frame].
//   3. emit   the tile's workgroup again: a pixel's rank is the tile's offset plus a workgroup scan in thread order (= pixel order).
//             The records are assembled in an LDS image (at most 15 KB) laid out at the destination's phase mod 16, so that a
//             16-byte word of LDS is a 16-byte word of the slot: whole words inside the range are stored as such, the ragged head and
//             tail byte by byte (wg_flush).  Nothing outside [0, out_points[i] * record) of a slot is written.
// No atomics at all, no inline assembly, no host synchronisation, no allocation: the bytes are a function of the arguments alone.
#include "camera_coordinate.h"
#include "export_rules.h"
#include "kbn_common.h"
#include "wg_scan.h"

namespace kbn {

constexpr int PC_PER_THREAD = 4;
constexpr int PC_TILE = WG_THREADS * PC_PER_THREAD;                 // 1024 pixels
constexpr int PC_RECORD_XYZ = 12, PC_RECORD_XYZRGB = 15;
constexpr int PC_IMAGE_DWORDS = (PC_TILE * PC_RECORD_XYZRGB + 16 + 15) / 16 * 4;   // + the phase mod 16, whole 16-byte words

struct PointCloudParams {
    const float* depth;
    long long depth_batch_stride;
    const float* image;          // NULL: no colour
    const float* kinv;
    unsigned char* out;
    unsigned long long out_stride;
    long long* out_points;
    unsigned* tiles_at;          // workspace: n x tiles kept counts, then (scan) their exclusive prefix sums
    float scale, shift, min_depth, max_depth;
    int width;
    unsigned pixels, tiles;      // height x width, ceil(pixels / PC_TILE)
};

// bit i: pixel first + i is kept.  The class test is on the bits (positive, not zero, below Inf: NaN has a larger pattern), so it
// does not depend on how comparisons treat denormals; the range test is the closed one.
__device__ __forceinline__ bool pc_kept(float d, float lo, float hi) {
    return __float_as_uint(d) - 1u < 0x7f7fffffu && d >= lo && d <= hi;
}

// the thread's four depths (0 past the plane's end) -> its mask of kept pixels
__device__ __forceinline__ unsigned pc_load(const float* __restrict__ plane, unsigned first, unsigned pixels, float lo, float hi, float d[PC_PER_THREAD]) {
    const float* at = plane + first;
    if (first + PC_PER_THREAD <= pixels && (reinterpret_cast<uintptr_t>(at) & 15) == 0) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(at);
#pragma unroll
        for (int i = 0; i < PC_PER_THREAD; ++i) d[i] = v[i];
    } else {
#pragma unroll
        for (int i = 0; i < PC_PER_THREAD; ++i) d[i] = first + i < pixels ? at[i] : 0.f;
    }
    unsigned mask = 0;
#pragma unroll
    for (int i = 0; i < PC_PER_THREAD; ++i) mask |= pc_kept(d[i], lo, hi) ? 1u << i : 0u;
    return mask;
}

// ---- 1. count ----
__global__ __launch_bounds__(WG_THREADS) void point_count_kernel(const PointCloudParams p) {
    __shared__ unsigned wave_total[WG_THREADS / 64];
    const unsigned frame = blockIdx.x / p.tiles, tile = blockIdx.x - frame * p.tiles;
    const unsigned first = tile * (unsigned)PC_TILE + threadIdx.x * (unsigned)PC_PER_THREAD;
    float d[PC_PER_THREAD];
    const unsigned mask = pc_load(p.depth + (long long)frame * p.depth_batch_stride, first, p.pixels, p.min_depth, p.max_depth, d);
    const unsigned total = wg_sum((unsigned)__popc(mask), wave_total);
    if (threadIdx.x == 0) p.tiles_at[blockIdx.x] = total;
}

// ---- 2. scan ----
__global__ __launch_bounds__(WG_THREADS) void point_scan_kernel(const PointCloudParams p) {
    __shared__ unsigned wave_total[WG_THREADS / 64];
    unsigned* at = p.tiles_at + (size_t)blockIdx.x * p.tiles;
    unsigned carry = 0;
    for (unsigned t0 = 0; t0 < p.tiles; t0 += WG_THREADS) {   // the same trip count in every thread
        const unsigned t = t0 + threadIdx.x;
        const unsigned v = t < p.tiles ? at[t] : 0u;
        unsigned total;
        const unsigned incl = wg_scan(v, wave_total, &total);
        if (t < p.tiles) at[t] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) p.out_points[blockIdx.x] = (long long)carry;
}

// ---- 3. emit ----
// 4 bytes into the LDS image at any byte offset
__device__ __forceinline__ void pc_put32(unsigned char* at, unsigned v) {
    if ((reinterpret_cast<uintptr_t>(at) & 3) == 0) {
        *reinterpret_cast<unsigned*>(at) = v;
    } else {
        at[0] = (unsigned char)v; at[1] = (unsigned char)(v >> 8); at[2] = (unsigned char)(v >> 16); at[3] = (unsigned char)(v >> 24);
    }
}

template <bool COLOUR>
__global__ __launch_bounds__(WG_THREADS) void point_emit_kernel(const PointCloudParams p) {
    constexpr unsigned RECORD = COLOUR ? PC_RECORD_XYZRGB : PC_RECORD_XYZ;
    __shared__ __attribute__((aligned(16))) unsigned image[PC_IMAGE_DWORDS];
    __shared__ unsigned wave_total[WG_THREADS / 64];
    const unsigned frame = blockIdx.x / p.tiles, tile = blockIdx.x - frame * p.tiles;
    const unsigned first = tile * (unsigned)PC_TILE + threadIdx.x * (unsigned)PC_PER_THREAD;
    float d[PC_PER_THREAD];
    const unsigned mask = pc_load(p.depth + (long long)frame * p.depth_batch_stride, first, p.pixels, p.min_depth, p.max_depth, d);
    const unsigned mine = (unsigned)__popc(mask);
    unsigned total;
    unsigned rank = wg_scan(mine, wave_total, &total) - mine;   // of the thread's first kept pixel, in the tile
    if (total == 0) return;                                     // the whole workgroup
    unsigned char* dst = p.out + (size_t)frame * p.out_stride + (size_t)p.tiles_at[blockIdx.x] * RECORD;
    const unsigned phase = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u);
    unsigned char* image_bytes = reinterpret_cast<unsigned char*>(image);

    if (mask) {
        const float* k = p.kinv + (size_t)frame * 9;
        float c[3][PC_PER_THREAD];
        if (COLOUR) {   // the normalised image's three planes, as the depth: a 16-byte load each where the address allows it
            const float* plane = p.image + (size_t)frame * 3 * p.pixels + first;
            const bool vec = first + PC_PER_THREAD <= p.pixels && (reinterpret_cast<uintptr_t>(plane) & 15) == 0 && (p.pixels & 3) == 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float* at = plane + (size_t)j * p.pixels;
                if (vec) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(at);
#pragma unroll
                    for (int i = 0; i < PC_PER_THREAD; ++i) c[j][i] = v[i];
                } else {
#pragma unroll
                    for (int i = 0; i < PC_PER_THREAD; ++i) c[j][i] = (mask >> i & 1u) ? at[i] : 0.f;
                }
            }
        }
        int y = (int)(first / (unsigned)p.width), x = (int)(first - (unsigned)y * (unsigned)p.width);
#pragma unroll
        for (int i = 0; i < PC_PER_THREAD; ++i) {
            if (mask >> i & 1u) {
                unsigned char* at = image_bytes + phase + rank * RECORD;
#pragma unroll
                for (int j = 0; j < 3; ++j) pc_put32(at + 4 * j, __float_as_uint(__fmul_rn(camera_coordinate(k, j, x, y), d[i])));
                if (COLOUR) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) at[12 + j] = (unsigned char)rgb8(c[j][i], p.scale, p.shift);
                }
                ++rank;
            }
            if (++x == p.width) { x = 0; ++y; }
        }
    }
    __syncthreads();
    wg_flush(image, phase, dst, total * RECORD);
}

// pixels and tiles of a frame; false for what the entry points refuse
static bool point_cloud_geometry(int n, int height, int width, unsigned* pixels, unsigned* tiles) {
    if (n < 1 || height < 1 || width < 1) return false;
    const long long hw = (long long)height * width;
    if (hw > 0x7fffffffLL) return false;                                   // pixel indices and ranks are 32-bit
    const long long t = (hw + PC_TILE - 1) / PC_TILE;
    if (t * n > 0x7fffffffLL) return false;                                // blockIdx.x carries (frame, tile)
    *pixels = (unsigned)hw; *tiles = (unsigned)t;
    return true;
}

}  // namespace kbn

extern "C" size_t kbn_point_cloud_workspace_bytes(int n, int height, int width) {
    unsigned pixels, tiles;
    if (!kbn::point_cloud_geometry(n, height, width, &pixels, &tiles)) return 0;
    return ((size_t)n * tiles * sizeof(unsigned) + 15) & ~(size_t)15;
}

extern "C" int kbn_point_cloud_forward(const float* depth, long long depth_batch_stride, const float* image, float scale, float shift,
                                       const float* kinv, float min_depth, float max_depth, int n, int height, int width,
                                       unsigned char* out, size_t out_stride, long long* out_points, void* workspace,
                                       size_t workspace_bytes, kbn_stream_t stream) {
    using namespace kbn;
    if (!depth || !kinv || !out || !out_points || !workspace) return KBN_ERR_INVALID_ARGUMENT;
    if (n < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    PointCloudParams p;
    if (!point_cloud_geometry(n, height, width, &p.pixels, &p.tiles)) return KBN_ERR_UNSUPPORTED;
    const size_t record = image ? PC_RECORD_XYZRGB : PC_RECORD_XYZ;
    if (out_stride < (size_t)p.pixels * record) return KBN_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(depth) & 3) || (reinterpret_cast<uintptr_t>(image) & 3) || (reinterpret_cast<uintptr_t>(kinv) & 3) ||
        (reinterpret_cast<uintptr_t>(workspace) & 3) || (reinterpret_cast<uintptr_t>(out_points) & 7))
        return KBN_ERR_INVALID_ARGUMENT;
    if (workspace_bytes < kbn_point_cloud_workspace_bytes(n, height, width)) return KBN_ERR_WORKSPACE;

    p.depth = depth; p.depth_batch_stride = depth_batch_stride; p.image = image; p.kinv = kinv;
    p.out = out; p.out_stride = out_stride; p.out_points = out_points; p.tiles_at = static_cast<unsigned*>(workspace);
    p.scale = scale; p.shift = shift; p.min_depth = min_depth; p.max_depth = max_depth; p.width = width;
    const dim3 grid(p.tiles * (unsigned)n), block(WG_THREADS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(point_count_kernel, grid, block, 0, s, p);
    hipLaunchKernelGGL(point_scan_kernel, dim3((unsigned)n), block, 0, s, p);
    if (image) hipLaunchKernelGGL(point_emit_kernel<true>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(point_emit_kernel<false>, grid, block, 0, s, p);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
