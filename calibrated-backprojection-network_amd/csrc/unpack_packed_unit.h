// unpack_packed_unit.h -- the work of one workgroup of the packed-frame device decoders (unpack_packed.hip: a triplet file,
// unpack_sequence.hip: a file per frame): one (file, row group, plane) checked, its segment offsets summed, and the crop's part of
// it decoded and stored to up to three outputs, each with a first column of its own in the file.  The steps and the discipline are
// written down at the head of unpack_packed.hip.
#pragma once
#include "frame_pack.h"
#include "unpack_common.h"

namespace kbn {

constexpr int UP_THREADS = 256;
constexpr int UP_TILE = 240;                       // output columns of a tile: at most 16 segments cover them at any phase
static_assert(UP_TILE % 4 == 0 && UP_TILE + fp::FP_SEG - 1 <= UP_THREADS, "a tile's segments must fit the workgroup");

// the `nb`-bit field (1 .. 16) at bit `at` of a segment: LSB first, only the bytes it touches
__device__ __forceinline__ unsigned read_field(const unsigned char* seg, unsigned at, int nb) {
    const unsigned char* p = seg + (at >> 3);
    const unsigned sh = at & 7u;
    const unsigned need = (sh + (unsigned)nb + 7u) >> 3;
    unsigned v = p[0];
    if (need > 1) v |= (unsigned)p[1] << 8;
    if (need > 2) v |= (unsigned)p[2] << 16;
    return (v >> sh) & ((1u << nb) - 1u);
}

// One (file, row group g, plane) of a file that the record says is fw x fheight x C samples of `bits` bits in file_bytes bytes (the
// host has made sure that header and table lie inside those bytes).  out[t] (nullptr: left out): the plane of the N x . x h x w
// output that takes the crop_h x crop_w crop whose first row is y_start and whose first column in the file is c0[t]; it is
// written `reps` times, HW floats apart (gray to all three channels); `scale_depth` divides by 256.  Every thread of the workgroup
// calls this with the same arguments.  Uses fp::FP_ROWS x ceil(fw / 16) unsigned of dynamic LDS.
template <bool VEC>
__device__ __forceinline__ void unpack_packed_unit(const unsigned char* file, unsigned file_bytes, int fw, int fheight, int C, int bits,
                                                   int plane, int g, int y_start, int crop_h, int crop_w, float* const (&out)[3],
                                                   const int (&c0s)[3], long long HW, int reps, bool scale_depth) {
    extern __shared__ unsigned seg_at[];                        // byte offset of every segment of the group, from the group's start
    __shared__ unsigned short tile[fp::FP_ROWS][UP_THREADS];    // decoded samples: [row in group][column - 16 x first segment]
    __shared__ unsigned wave_total[UP_THREADS / 64];

    const int tid = (int)threadIdx.x;
    const int y_last = y_start + crop_h - 1;
    const unsigned mask = (1u << bits) - 1u;

    // the file's header against the record
    const unsigned* word = reinterpret_cast<const unsigned*>(file);
    const unsigned long long start = fp::payload_start(((unsigned long long)fheight + fp::FP_ROWS - 1) / fp::FP_ROWS, (unsigned)C);
    const unsigned payload_bytes = word[6];
    bool ok = word[0] == 0x464E424Bu && word[1] == 0x00314D52u && word[2] == (unsigned)fw && word[3] == (unsigned)fheight &&
              word[4] == ((unsigned)C | (unsigned)bits << 16) && word[5] == ((unsigned)fp::FP_ROWS | (unsigned)fp::FP_SEG << 16) &&
              word[7] == 0u && start + payload_bytes == file_bytes;
    const unsigned entry = (unsigned)g * (unsigned)C + (unsigned)plane;
    const unsigned lo = word[8 + entry], hi = word[9 + entry];
    const int rows = min(fp::FP_ROWS, fheight - g * fp::FP_ROWS);
    const int S = (fw + fp::FP_SEG - 1) / fp::FP_SEG;
    const int nseg = rows * S;
    ok = ok && lo <= hi && hi <= payload_bytes && hi - lo >= (unsigned)nseg;
    if (!ok) return;
    const unsigned char* head = file + start + lo;   // nseg header bytes, then the segments
    const int last_n = fw - (S - 1) * fp::FP_SEG;

    // ---- 1. segment offsets ----
    {
        const int per = (nseg + UP_THREADS - 1) / UP_THREADS;
        const int e0 = min(nseg, tid * per), e1 = min(nseg, e0 + per);
        unsigned sum = 0;
        int r = e0 / S, k = e0 - r * S;
        for (int e = e0; e < e1; ++e) {
            sum += fp::segment_bytes(k == S - 1 ? last_n : fp::FP_SEG, min((int)head[e], bits), bits, r == 0);
            if (++k == S) { k = 0; ++r; }
        }
        unsigned incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(incl, d);
            if ((tid & 63) >= d) incl += t;
        }
        if ((tid & 63) == 63) wave_total[tid >> 6] = incl;
        __syncthreads();
        unsigned run = (unsigned)nseg + incl - sum, total = 0;
#pragma unroll
        for (int w = 0; w < UP_THREADS / 64; ++w) {
            if (w < (tid >> 6)) run += wave_total[w];
            total += wave_total[w];
        }
        r = e0 / S; k = e0 - r * S;
        for (int e = e0; e < e1; ++e) {
            seg_at[e] = run;
            run += fp::segment_bytes(k == S - 1 ? last_n : fp::FP_SEG, min((int)head[e], bits), bits, r == 0);
            if (++k == S) { k = 0; ++r; }
        }
        __syncthreads();
        if ((unsigned)nseg + total != hi - lo) return;   // the headers do not describe this payload
    }

    // ---- 2. and 3. decode and store, tile by tile ----
    const int r_first = max(0, y_start - g * fp::FP_ROWS), r_last = min(rows - 1, y_last - g * fp::FP_ROWS);
    const int slot = tid >> 4, j = tid & 15;
    for (int t = 0; t < 3; ++t) {
        if (!out[t]) continue;
        const int c0 = c0s[t];   // the crop's first column in the file
        for (int X0 = 0; X0 < crop_w; X0 += UP_TILE) {
            const int tw = min(UP_TILE, crop_w - X0);
            const int k_first = (c0 + X0) >> 4, k_last = (c0 + X0 + tw - 1) >> 4;
            const int k = k_first + slot;
            const bool live = k <= k_last && j < min(fp::FP_SEG, fw - k * fp::FP_SEG);
            unsigned val = 0;
            for (int r = 0; r <= r_last; ++r) {
                unsigned z = 0;
                if (live) {
                    const int e = r * S + k;
                    const int bw = min((int)head[e], bits);
                    const unsigned char* seg = head + seg_at[e];
                    if (r == 0) {
                        if (j == 0) z = read_field(seg, 0u, bits);
                        else if (bw) z = read_field(seg, (unsigned)(bits + (j - 1) * bw), bw);
                    } else if (bw) {
                        z = read_field(seg, (unsigned)(j * bw), bw);
                    }
                }
                if (r == 0) {   // the left row: raw sample in lane 0, differences in the others, an inclusive scan over the 16 lanes
                    unsigned v = j == 0 ? z : (unsigned)fp::unzigzag(z);
#pragma unroll
                    for (int d = 1; d < fp::FP_SEG; d <<= 1) {
                        const unsigned up = __shfl_up(v, d, fp::FP_SEG);
                        if (j >= d) v += up;
                    }
                    val = v & mask;
                } else {
                    val = (val + (unsigned)fp::unzigzag(z)) & mask;
                }
                if (r >= r_first) tile[r][tid] = (unsigned short)val;
            }
            __syncthreads();
            const int quads = (tw + 3) >> 2, items = (r_last - r_first + 1) * quads;
            const int phase = c0 + X0 - k_first * fp::FP_SEG;   // 0 .. 15: where the tile's first column sits in its first segment
            for (int i = tid; i < items; i += UP_THREADS) {
                const int rr = i / quads, q = i - rr * quads;
                const int r = r_first + rr;
                const unsigned short* s = &tile[r][phase + 4 * q];
                const int x = X0 + 4 * q;
                const int n_live = VEC ? 4 : min(4, crop_w - x);
                f32x4 v;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const float s_f = (VEC || a < n_live) ? (float)s[a] : 0.f;
                    v[a] = scale_depth ? s_f / 256.0f : s_f;
                }
                float* o = out[t] + (long long)(g * fp::FP_ROWS + r - y_start) * crop_w + x;
                for (int c = 0; c < reps; ++c) store_quad<VEC>(o + c * HW, v, n_live);
            }
            __syncthreads();
        }
    }
}

}  // namespace kbn
