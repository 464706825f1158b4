// upconv_split.hip -- the nearest-2x up-conv (and ConvTranspose2d(3, stride 2)) in its FOLDED form on split operands: modes 3
// and 4 of kbn_conv3x3_split_forward(_ksplit), whose argument checks and split-K reduction live in conv_split.hip.  Three
// kernels by layer width: upconv2x_split_kernel (32-filter tiles), upconv2x_split16_kernel (at most 16 filters) and
// upconv2x_split64_kernel (whole 64-filter tiles, the only one with pair tensors out and a split-K form).  The split
// arithmetic: split_common.h.
#include "split_common.h"

namespace kbn {

// ------------------------------------------------------------------------------------------------------------------
// Nearest-2x up-conv in its FOLDED form on split operands (MODE 3 of the entry point).  An output pixel (2Y+py, 2X+px)
// of conv3x3(upsample2x(x)) only sees the 2 x 2 low-resolution pixels (Y+py-1+dy, X+px-1+dx), dy, dx in {0, 1}, with
// the 3 x 3 weights summed over the taps that land on the same source pixel (rows: py 0 -> {0}, {1,2}; py 1 -> {0,1},
// {2}; columns alike): four 2 x 2 convs, one per output parity, 16 channel products per low-resolution pixel instead of
// 36 -- 2.25x fewer MFMAs than the nine-tap form (MODE 1 until round 5).  M = 32 low-resolution pixels of a row (one parity), N = 32 filters.
// Workgroup = 8 waves = 8 row groups; tile 16 x 32 low-resolution pixels (32 x 64 outputs) x 32 filters; a wave owns two
// low-resolution rows x four parities (eight accumulator blocks).  The 16 (parity, tap) weight sets of a chunk are
// visited grouped by the source offset they read, (ox = px+dx, s = py+dy): the two rows of a wave then need the A
// fragments of staged rows s and s+1 at column offset ox -- 12 fragment reads per chunk serve all 96 MFMAs; weights are
// packed in that visiting order and fetched three sets ahead.  K per output = 4 Cin: a third of the roundings of the
// unfolded form, so ONE accumulator per block keeps the accuracy of conv3x3_split_kernel's APART form (conv_split.hip).
// (UF_NT, UF_ITEMS: split_common.h)
struct UfItem { int ox, s, py, dy, px, dx; };
__host__ __device__ constexpr UfItem uf_item(int it) {
    // ox 0: (px,dx) = (0,0); ox 1: (0,1), (1,0); ox 2: (1,1).  Same for s over (py,dy).  Order: ox, s, (py,dy), (px,dx).
    int ox = it < 4 ? 0 : (it < 12 ? 1 : 2);
    int r = it - (ox == 0 ? 0 : (ox == 1 ? 4 : 12));
    const int ncol = ox == 1 ? 2 : 1;                 // (px,dx) combos of this ox
    const int rowidx = r / ncol, colidx = r % ncol;   // rowidx 0..3 over (s, (py,dy)): s0:1, s1:2, s2:1
    const int s = rowidx == 0 ? 0 : (rowidx < 3 ? 1 : 2);
    const int py = s == 0 ? 0 : (s == 2 ? 1 : rowidx - 1);
    const int px = ox == 0 ? 0 : (ox == 2 ? 1 : colidx);
    return UfItem{ox, s, py, s - py, px, ox - px};
}
// folded weight of (py, dy) x (px, dx) from the nine taps of one (filter, channel).  tr = 0: conv3x3(upsample2x(x)) -- the taps that
// land on the same low-resolution pixel are summed.  tr = 1: ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1)
// (reference src/net_utils.py:383-390) in the same four-parity form: out[2i - 1 + ky] += in[i] w[ky] gives an even output row (py 0) the one
// tap ky = 1 of row Y (dy 1), an odd one (py 1) ky = 2 of row Y (dy 0) and ky = 0 of row Y + 1 (dy 1); columns alike.  Nine of the sixteen
// folded weights are taps, seven are zero (`w9`: the weight with out_channels leading, i.e. the module's in x out x 3 x 3 weight with its first
// two axes swapped -- the host does that).
__device__ __forceinline__ void uf_taps(int p, int d, int tr, int& k0, int& k1) {
    if (tr) { k0 = p == 0 ? 1 : (d == 0 ? 2 : 0); k1 = (p == 0 && d == 0) ? 0 : k0; return; }   // (0,0): empty range
    k0 = (p == 0) ? (d == 0 ? 0 : 1) : (d == 0 ? 0 : 2);
    k1 = (p == 0) ? (d == 0 ? 0 : 2) : (d == 0 ? 1 : 2);
}
__device__ __forceinline__ float uf_fold(const float* w9, int py, int dy, int px, int dx, int tr = 0) {
    int r0, r1, c0, c1;
    uf_taps(py, dy, tr, r0, r1);
    uf_taps(px, dx, tr, c0, c1);
    float acc = 0.f;
    for (int r = r0; r <= r1; ++r) {
        float row = 0.f;
        for (int c = c0; c <= c1; ++c) row += w9[r * 3 + c];
        acc += row;
    }
    return acc;
}

__global__ void uf_scale_kernel(const float* __restrict__ w, float* __restrict__ inv_scale, int OC, int Cin, int tr) {
    const int oc = blockIdx.x;
    __shared__ float red[256];
    float m = 0.f;
    if (oc < OC)
        for (int i = threadIdx.x; i < Cin * UF_ITEMS; i += 256) {
            const int c = i / UF_ITEMS;
            const UfItem t = uf_item(i % UF_ITEMS);
            m = fmaxf(m, fabsf(uf_fold(w + ((long long)oc * Cin + c) * 9, t.py, t.dy, t.px, t.dx, tr)));
        }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int ex = SP_WEXP;
        if (red[0] > 0.f && red[0] < 3.0e38f) (void)frexpf(red[0], &ex);
        int e = SP_WEXP - ex;
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
        inv_scale[oc] = ldexpf(1.f, -e);
    }
}

// OIHW fp32 -> [n-tile][chunk][item][part][k-group][32 filters][8 channels] fp16 of the folded weights
__global__ void uf_pack_kernel(const float* __restrict__ w, const float* __restrict__ inv_scale, _Float16* __restrict__ packed,
                               int OC, int Cin, int nchunks, long long total, int tr) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    constexpr int per_item = 2 * 2 * UF_NT * 8, per_chunk = UF_ITEMS * per_item;
    int r = (int)(e % per_chunk);
    const long long q = e / per_chunk;
    const int chunk = (int)(q % nchunks), nt = (int)(q / nchunks);
    const int item = r / per_item; r -= item * per_item;
    const int part = r / (2 * UF_NT * 8); r -= part * 2 * UF_NT * 8;
    const int g = r / (UF_NT * 8); r -= g * UF_NT * 8;
    const int n = r >> 3, k = r & 7;
    const int c = chunk * SP_CK + g * 8 + k, oc = nt * UF_NT + n;
    _Float16 h = (_Float16)0.f;
    if (c < Cin && oc < OC) {
        const UfItem t = uf_item(item);
        const float ws = uf_fold(w + ((long long)oc * Cin + c) * 9, t.py, t.dy, t.px, t.dx, tr) * (1.f / inv_scale[oc]);
        const _Float16 w1 = (_Float16)ws;
        h = part == 0 ? w1 : (_Float16)(ws - (float)w1);
    }
    packed[e] = h;
}

template <int N>
__device__ __forceinline__ void uf_wait_b(f32x4 (&b)[2]) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(b[0]), "+v"(b[1]) : "n"(N));
}

// BLDS: the sixteen weight sets of a chunk (32 KiB) are copied into LDS by LDS-DMA, double buffered, like the nine taps
// of the concat convs: eight waves fetching every set straight from L1 move 256 KiB per chunk through the CU's vector
// memory pipe (42 B/clk of its 64 beside the input loads); through LDS it is 32 KiB, every global access of chunk c+1
// is issued at the start of chunk c and awaited once, late in it.
template <bool BLDS>
__global__ __launch_bounds__(SP_THREADS, 1) void upconv2x_split_kernel(const SplitConvParams p) {
    constexpr int ROWS = 18, COLS = 34, NPIX = ROWS * COLS, A_PART = 2 * NPIX * 16, A_BYTES = 2 * A_PART, PR = 3, NA_ALL = PR * 8;
    constexpr int B_ITEM = 2 * 2 * UF_NT * 16, NBL = 2, D = 3;       // bytes per weight set; loads per set; sets fetched ahead
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 6, 2), 0");   // fp16 results flush subnormals (see conv3x3_split_kernel)
    const int tid = threadIdx.x, lane = tid & 63;
    const int rg = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave = row group: low-resolution rows 2 rg, 2 rg + 1
    const int lm = lane & 31, g = lane >> 5;
    int bid = xcd_remap(blockIdx.x, p.nblocks);
    const int nt = bid % p.nTilesN;
    bid /= p.nTilesN;
    const int tx = bid % p.tilesX;
    bid /= p.tilesX;
    const int ty = bid % p.tilesY;
    const int n = bid / p.tilesY;
    const int oy0 = ty * 16, ox0 = tx * 32;                            // low-resolution tile origin
    const int H = p.H, W = p.W, sH = p.sH, sW = p.sW;
    const long long plane = (long long)sH * sW;
    const int nchunks = p.Cin / SP_CK;
    float prescale, unscale;
    sp_act_scale(p, n, prescale, unscale);

    const int kg_st = rg >> 2, t256 = tid & 255;
    int goff[PR];
#pragma unroll
    for (int u = 0; u < PR; ++u) {
        const int pix = u * 256 + t256;
        const int r = pix / COLS, c = pix - r * COLS;
        const int Y = oy0 - 1 + r, X = ox0 - 1 + c;
        goff[u] = (pix < NPIX && Y >= 0 && Y < sH && X >= 0 && X < sW) ? (Y * sW + X) * 4 : -1;
    }
    const _Float16* wp_nt = p.wp + (long long)nt * nchunks * (UF_ITEMS * B_ITEM / 2);

    float va[PR][8];
    auto load_chunk = [&](int chunk) {
        const float* base = p.src[0] + (long long)n * p.src_bstride[0] + (long long)(chunk * SP_CK + kg_st * 8) * plane;
#pragma unroll
        for (int u = 0; u < PR; ++u) {
            const unsigned voff = goff[u] < 0 ? 0u : (unsigned)goff[u];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float* sb = base + (long long)k * plane;
                asm volatile("global_load_dword %0, %1, %2" : "=v"(va[u][k]) : "v"(voff), "s"(sb) : "memory");
            }
        }
    };
    auto store_round = [&](int buf, int u) {
        unsigned char* A = smem + buf * A_BYTES + kg_st * NPIX * 16;
#pragma unroll
        for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(va[u][k]));
        const int pix = u * 256 + t256;
        if (pix < NPIX) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = goff[u] >= 0 ? va[u][k] : 0.f;
            sph8 h1, h2;
            sp_split8(v, prescale, h1, h2);
            *reinterpret_cast<sph8*>(A + pix * 16) = h1;
            *reinterpret_cast<sph8*>(A + A_PART + pix * 16) = h2;
        }
    };
    const unsigned boff = (unsigned)((g * UF_NT + lm) * 16);
    auto load_b = [&](f32x4 (&b)[2], int chunk, int item) {
        const unsigned char* base = reinterpret_cast<const unsigned char*>(wp_nt + ((long long)chunk * UF_ITEMS + item) * (B_ITEM / 2));
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned char* sb = base + t * 2 * UF_NT * 16;
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(b[t]) : "v"(boff), "s"(sb) : "memory");
        }
    };

    spf16 acc[2][2][2];   // [low-resolution row of the wave][py][px]
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a >> 2][(a >> 1) & 1][a & 1][i] = 0.f;

    const unsigned char* const aptr = smem + (g * NPIX + 2 * rg * COLS + lm) * 16;
    sph8 af[4][2];        // A fragments of staged rows 2 rg + 0..3 at the current column offset (two split terms each)
    auto load_arow = [&](int abuf, int ry, int ox) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
            af[ry][t] = *reinterpret_cast<const sph8*>(aptr + abuf + t * A_PART + (ry * COLS + ox) * 16);
    };

    if constexpr (BLDS) {
        constexpr int B_CHUNK = UF_ITEMS * B_ITEM;
        constexpr int WAIT_IT = 9;   // the set whose MFMAs follow the wait for chunk c+1's accesses (issued ahead of set 0)
        static_assert(WAIT_IT + PR < UF_ITEMS, "the staging rounds follow the wait inside the chunk");
        const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(reinterpret_cast<const float*>(smem)));
        auto stage_b = [&](int bbuf, int chunk) {
            const float* src = reinterpret_cast<const float*>(wp_nt + (long long)chunk * (B_CHUNK / 2));
            const unsigned dst = lds0 + (unsigned)(2 * A_BYTES + bbuf * B_CHUNK);
            constexpr int n4 = B_CHUNK / 16;
            static_assert(n4 % SP_THREADS == 0, "whole rounds of the workgroup");
#pragma unroll
            for (int e0 = 0; e0 < n4; e0 += SP_THREADS) {
                const int eb = e0 + rg * 64;
                lds_dma16_s(src + eb * 4, (unsigned)(lane * 16), dst + eb * 16);
            }
        };
        const unsigned char* const bptr = smem + 2 * A_BYTES + boff;
        auto body = [&](int c, auto more_tag, auto chk_tag) {
            constexpr bool MORE = decltype(more_tag)::value, CHK = decltype(chk_tag)::value;
            const int abuf = (c & 1) * A_BYTES;
            const unsigned char* B = bptr + (c & 1) * B_CHUNK;
            if (MORE) {
                stage_b((c & 1) ^ 1, c + 1);
                load_chunk(c + 1);
            }
            load_arow(abuf, 0, 0);
            load_arow(abuf, 1, 0);
            sph8 bwq[2][2];   // (w1, w2) of the current / next set
            bwq[0][0] = *reinterpret_cast<const sph8*>(B);
            bwq[0][1] = *reinterpret_cast<const sph8*>(B + 2 * UF_NT * 16);
#pragma unroll
            for (int it = 0; it < UF_ITEMS; ++it) {
                const UfItem t = uf_item(it);
                const bool first_of_group = it == 0 || uf_item(it - 1).s != t.s || uf_item(it - 1).ox != t.ox;
                if (first_of_group) {   // fetch what the NEXT group reads and this one does not hold
                    if (t.s == 0) load_arow(abuf, 2, t.ox);
                    else if (t.s == 1) load_arow(abuf, 3, t.ox);
                    else if (t.ox < 2) { load_arow(abuf, 0, t.ox + 1); load_arow(abuf, 1, t.ox + 1); }
                }
                if (it + 1 < UF_ITEMS) {
                    bwq[(it + 1) & 1][0] = *reinterpret_cast<const sph8*>(B + (it + 1) * B_ITEM);
                    bwq[(it + 1) & 1][1] = *reinterpret_cast<const sph8*>(B + (it + 1) * B_ITEM + 2 * UF_NT * 16);
                }
                sph8 bw[3];
                bw[0] = bwq[it & 1][0];
                bw[1] = bwq[it & 1][1];
                bw[2] = bw[0] * (_Float16)0.00048828125f;
                if (MORE && it == WAIT_IT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // next chunk's weights (DMA) and inputs
                __builtin_amdgcn_sched_barrier(0);
                constexpr int TA[3] = {0, 0, 1};
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb) {
                        if (CHK && oy0 + 2 * rg + mb >= sH) continue;     // low-resolution row below the map: no MFMAs (wave-uniform)
                        acc[mb][t.py][t.px] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[mb + t.s][TA[k]], bw[k], acc[mb][t.py][t.px], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
                if (MORE && it >= WAIT_IT && it - WAIT_IT < PR) store_round((c & 1) ^ 1, it - WAIT_IT);
            }
            __syncthreads();
        };
        load_chunk(0);
        stage_b(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int u = 0; u < PR; ++u) store_round(0, u);
        __syncthreads();
        auto k_loop = [&](auto chk_tag) {
            for (int c = 0; c + 1 < nchunks; ++c) body(c, std::true_type{}, chk_tag);
            body(nchunks - 1, std::false_type{}, chk_tag);
        };
        if (!KBN_SPLIT_STRAIGHT || oy0 + 16 > sH) k_loop(std::true_type{});   // tile with rows below the map (workgroup-uniform)
        else k_loop(std::false_type{});
    } else {
    f32x4 bq[4][2];       // weight sets in flight: set `it` lives in bq[it % 4]
    auto chunk_body = [&](int c, auto more_tag) {
        constexpr bool MORE = decltype(more_tag)::value;
        constexpr int NA = MORE ? NA_ALL : 0;
        const int abuf = (c & 1) * A_BYTES;
        load_arow(abuf, 0, 0);
        load_arow(abuf, 1, 0);
#pragma unroll
        for (int it = 0; it < UF_ITEMS; ++it) {
            const UfItem t = uf_item(it);
            const bool first_of_group = it == 0 || uf_item(it - 1).s != t.s || uf_item(it - 1).ox != t.ox;
            if (first_of_group) {   // fetch what the NEXT group reads and this one does not hold
                if (t.s == 0) load_arow(abuf, 2, t.ox);
                else if (t.s == 1) load_arow(abuf, 3, t.ox);
                else if (t.ox < 2) { load_arow(abuf, 0, t.ox + 1); load_arow(abuf, 1, t.ox + 1); }
            }
            f32x4 (&bc)[2] = bq[it % 4];
            if (it + D < UF_ITEMS) load_b(bq[(it + D) % 4], c, it + D);
            else if (MORE) load_b(bq[(it + D) % 4], c + 1, it + D - UF_ITEMS);
            if (it == 0 && MORE) load_chunk(c + 1);
            // outstanding, oldest first: b(it) b(it+1) b(it+2) [b(it+3) | inputs in issue order]
            if (it <= D) uf_wait_b<D * NBL + NA>(bc);
            else if (MORE || it + D < UF_ITEMS) uf_wait_b<D * NBL>(bc);
            else if (it == UF_ITEMS - 3) uf_wait_b<2 * NBL>(bc);
            else if (it == UF_ITEMS - 2) uf_wait_b<NBL>(bc);
            else uf_wait_b<0>(bc);
            sph8 bw[3];
            bw[0] = __builtin_bit_cast(sph8, bc[0]);
            bw[1] = __builtin_bit_cast(sph8, bc[1]);
            bw[2] = bw[0] * (_Float16)0.00048828125f;
            __builtin_amdgcn_sched_barrier(0);
            constexpr int TA[3] = {0, 0, 1};
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    if (oy0 + 2 * rg + mb >= sH) continue;            // low-resolution row below the map: no MFMAs (wave-uniform)
                    acc[mb][t.py][t.px] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[mb + t.s][TA[k]], bw[k], acc[mb][t.py][t.px], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
            if (MORE && it > D + 1 && it - D - 2 < PR) store_round((c & 1) ^ 1, it - D - 2);   // the wait of set D+1 covered the inputs
        }
        __syncthreads();
    };

    load_chunk(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < PR; ++u) store_round(0, u);
#pragma unroll
    for (int it = 0; it < D; ++it) load_b(bq[it], 0, it);
    __syncthreads();
    for (int c = 0; c + 1 < nchunks; ++c) chunk_body(c, std::true_type{});
    chunk_body(nchunks - 1, std::false_type{});
    }

    // ---- epilogue: acc[mb][py][px][i]: low-resolution x = 8 (i / 4) + 4 g + (i % 4), filter lm; outputs (2 Y + py, 2 x + px)
    const long long oplane = (long long)H * W;
    const int oc = nt * UF_NT + lm;
    const float inv = p.inv_scale[oc] * unscale;
    float* outc = p.out + (long long)n * p.out_bstride + (long long)oc * oplane;
    const float slope = p.act ? p.slope : 1.f;
    float amax = 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        const int Y = oy0 + 2 * rg + mb;
        if (Y >= sH || oc >= p.OC) continue;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            float* orow = outc + (long long)(2 * Y + py) * W;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int X = 2 * (ox0 + 8 * q4 + 4 * g);              // first output column of this lane's 8
                f32x4 v0, v1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a = acc[mb][py][j & 1][q4 * 4 + (j >> 1)] * inv;
                    const float b = acc[mb][py][j & 1][q4 * 4 + 2 + (j >> 1)] * inv;
                    v0[j] = a > 0.f ? a : a * slope;
                    v1[j] = b > 0.f ? b : b * slope;
                }
                if (X < W) { *reinterpret_cast<f32x4*>(orow + X) = v0; amax = sp_amax4(amax, v0); }
                if (X + 4 < W) { *reinterpret_cast<f32x4*>(orow + X + 4) = v1; amax = sp_amax4(amax, v1); }
            }
        }
    }
    if (p.out_amax) absmax_commit(p.out_amax + n, amax);
}


// ------------------------------------------------------------------------------------------------------------------
// The folded up-conv for NARROW layers (at most 16 filters, Cin % 32 == 0: deconv0's 64 -> 12 up-conv at full
// resolution, reference src/net_utils.py:484-499 with n_filters_decoder[-1] = 12): 16-filter tiles on
// v_mfma_f32_16x16x32_f16 instead of 32-filter tiles on 32x32x16 -- 12 of 16 columns live instead of 12 of 32.  Same
// arithmetic as upconv2x_split_kernel (sixteen folded 2 x 2 weight sets, three fp16 products per fp32 product, one
// accumulator per block).  M = 16 low-resolution pixels of a row, N = 16 filters, K = 32 channels per MFMA; chunk = 32
// channels.  Workgroup = 4 waves = 2 row groups x 2 column halves; tile 8 x 32 low-resolution pixels; a wave owns four
// low-resolution rows x 16 pixels x four parities (sixteen 16 x 16 accumulator blocks).  A in LDS as
// [part][k-group (4)][pixel][8 fp16]; a group of weight sets (ox, s) reads the staged rows s .. s+3 at column offset
// ox: rows stream through eight register slots (rows 2 and 3 have two: the last group of one column offset still
// reads them while the first of the next is being fetched).  Weights: [chunk][set][part][k-group][16 filters][8
// channels] fp16, one 1 KiB wave-wide load per (set, part), fetched three sets ahead.
// (U16_NT, U16_CK, uf_narrow: split_common.h)

// OIHW fp32 -> [n-tile][chunk][set][part][k-group (4)][16 filters][8 channels] fp16 of the folded weights
__global__ void uf16_pack_kernel(const float* __restrict__ w, const float* __restrict__ inv_scale, _Float16* __restrict__ packed,
                                 int OC, int Cin, int nchunks, long long total, int tr) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    constexpr int per_item = 2 * 4 * U16_NT * 8, per_chunk = UF_ITEMS * per_item;
    int r = (int)(e % per_chunk);
    const long long q = e / per_chunk;
    const int chunk = (int)(q % nchunks), nt = (int)(q / nchunks);
    const int item = r / per_item; r -= item * per_item;
    const int part = r / (4 * U16_NT * 8); r -= part * 4 * U16_NT * 8;
    const int g = r / (U16_NT * 8); r -= g * U16_NT * 8;
    const int n = r >> 3, k = r & 7;
    const int c = chunk * U16_CK + g * 8 + k, oc = nt * U16_NT + n;
    _Float16 h = (_Float16)0.f;
    if (c < Cin && oc < OC) {
        const UfItem t = uf_item(item);
        const float ws = uf_fold(w + ((long long)oc * Cin + c) * 9, t.py, t.dy, t.px, t.dx, tr) * (1.f / inv_scale[oc]);
        const _Float16 w1 = (_Float16)ws;
        h = part == 0 ? w1 : (_Float16)(ws - (float)w1);
    }
    packed[e] = h;
}

// NW = 4 waves per workgroup: tile 8 x 32, ONE staging buffer (43.5 KB) refilled from registers between two barriers, two
// workgroups per CU -- with only Cin / 32 = 2 chunks per tile the first fetch and the stores are most of a workgroup's life,
// and a second resident workgroup multiplies meanwhile: 616 us for deconv0's up-conv against 700 with 8 waves on 16 x 32
// tiles, the staged chunk double buffered (157 KB of LDS, one workgroup per CU; that form is no longer built).
// (Measured and not kept, DESIGN.md round 3: persistent workgroups, with the weights from L2 as here or resident in LDS.)
// PIN: the input is a pair tensor, staged by LDS-DMA (see upconv2x_split64_kernel); POUT: the output is written as one with
// 16 channels (two k-groups; channels past OC are zero) -- the decoder tail (csrc/tail.hip) stages it by DMA
template <int NW, bool PIN, bool POUT = false, bool ONE = false>   // ONE: h1 w1 alone (KBN_FP16_ONE_TERM, throughput only; see conv3x3_split_kernel)
__global__ __launch_bounds__(NW * 64, 2) void upconv2x_split16_kernel(const SplitConvParams p) {
    static_assert(NW == 4, "4 waves (8-row tiles)");
    constexpr int ROWS = 2 * NW, TPG = 16 * NW;                        // low-resolution rows per tile; threads per k-group in staging
    constexpr int COLS = 34, NPIX = (ROWS + 2) * COLS, KG = 4;
    // plane pitch of a k-group, padded to a multiple of 16 granules: ds_read_b128 serves lanes {0-3, 12-15, 20-27} together, i.e. the kq = 0 and
    // kq = 1 halves of an A fragment, conflict-free only when they sit 0 (mod 256 B) apart (340 granules: SQ_LDS_BANK_CONFLICT / IDX_ACTIVE 0.50)
    constexpr int NPP = (NPIX + 15) / 16 * 16;
    constexpr int A_PART = KG * NPP * 16, A_BYTES = 2 * A_PART;       // [part][k-group][pixel (pitch NPP)][8 fp16]
    constexpr int PR = (NPIX + TPG - 1) / TPG;                         // staging rounds of a quarter of the threads (one k-group each)
    // pair input: a staged chunk is 8 planes (term, k-group) x NPIX granules; wave-wide DMA id = plane * NR + round
    constexpr int NR = (NPIX + 63) / 64, NDMA = (ONE ? 1 : 2) * KG * NR, DPW = NDMA / NW;   // ONE: the h1 planes only
    static_assert(NDMA % NW == 0, "the same number of DMAs in every wave (the vmcnt arithmetic counts them)");
    constexpr int NA_ALL = PIN ? DPW : PR * 8;                         // vector-memory operations of a wave per staged chunk
    constexpr int B_ITEM = 2 * KG * U16_NT * 16, NBL = 2, D = 3;      // bytes per weight set; loads per set; sets fetched ahead
    static_assert(D * NBL + NA_ALL < 64, "vmcnt is a 6-bit counter");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 6, 2), 0");   // fp16 results flush subnormals (see conv3x3_split_kernel)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rg = wave >> 1, mblk = wave & 1;                         // low-resolution rows 4 rg .. 4 rg + 3, pixels 16 mblk .. + 15
    const int lp = lane & 15, kq = lane >> 4;
    int bid = xcd_remap(blockIdx.x, p.nblocks);
    const int nt = bid % p.nTilesN;
    bid /= p.nTilesN;
    const int tx = bid % p.tilesX;
    bid /= p.tilesX;
    const int ty = bid % p.tilesY;
    const int n = bid / p.tilesY;
    const int oy0 = ty * ROWS, ox0 = tx * 32;                            // low-resolution tile origin
    const int H = p.H, W = p.W, sH = p.sH, sW = p.sW;
    const long long plane = (long long)sH * sW;
    const int nchunks = p.Cin / U16_CK;
    float prescale, unscale;
    if constexpr (PIN) { prescale = 0.f; unscale = 1.f / p.pair_src_scale[n]; }
    else sp_act_scale(p, n, prescale, unscale);

    const int kg_st = wave / (NW / 4), t128 = tid & (TPG - 1);         // staging: NW / 4 waves per k-group
    int goff[PR];
#pragma unroll
    for (int u = 0; u < PR; ++u) {
        const int pix = u * TPG + t128;
        const int r = pix / COLS, c = pix - r * COLS;
        const int Y = oy0 - 1 + r, X = ox0 - 1 + c;
        goff[u] = (pix < NPIX && Y >= 0 && Y < sH && X >= 0 && X < sW) ? (Y * sW + X) * 4 : -1;
    }
    const unsigned char* wp_nt = reinterpret_cast<const unsigned char*>(p.wp) + (long long)nt * nchunks * (UF_ITEMS * B_ITEM);

    float va[PR][8];
    auto load_chunk = [&](int chunk) {
        const float* base = p.src[0] + (long long)n * p.src_bstride[0] + (long long)(chunk * U16_CK + kg_st * 8) * plane;
#pragma unroll
        for (int u = 0; u < PR; ++u) {
            const unsigned voff = goff[u] < 0 ? 0u : (unsigned)goff[u];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float* sb = base + (long long)k * plane;         // wave-uniform
                asm volatile("global_load_dword %0, %1, %2" : "=v"(va[u][k]) : "v"(voff), "s"(sb) : "memory");
            }
        }
    };
    auto store_round = [&](int buf, int u) {
        unsigned char* A = smem + buf * A_BYTES + kg_st * NPP * 16;
#pragma unroll
        for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(va[u][k]));
        const int pix = u * TPG + t128;
        if (pix < NPIX) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = goff[u] >= 0 ? va[u][k] : 0.f;
            sph8 h1, h2;
            sp_split8(v, prescale, h1, h2);
            *reinterpret_cast<sph8*>(A + pix * 16) = h1;
            *reinterpret_cast<sph8*>(A + A_PART + pix * 16) = h2;
        }
    };
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(reinterpret_cast<const float*>(smem)));
    unsigned dvoff[PIN ? DPW : 1];
    if constexpr (PIN) {
#pragma unroll
        for (int i = 0; i < DPW; ++i) {
            const int pix = ((wave + NW * i) % NR) * 64 + lane;
            const int r = pix / COLS, c = pix - r * COLS;
            const int Y = oy0 - 1 + r, X = ox0 - 1 + c;
            dvoff[i] = (pix < NPIX && Y >= 0 && Y < sH && X >= 0 && X < sW) ? (unsigned)(Y * sW + X) * 16u : (unsigned)(sH * sW) * 16u;
        }
    }
    const long long pplane = pair_plane_halves(sH, sW);
    auto dma_chunk = [&](int buf, int chunk) {
        const _Float16* pn = p.pair_src + (long long)n * p.pair_src_bstride + (long long)(KG * chunk) * 2 * pplane;
#pragma unroll
        for (int i = 0; i < DPW; ++i) {
            const int id = wave + NW * i, plane = id / NR, j = id - plane * NR;
            const int t = plane / KG, kgl = plane - t * KG;
            const unsigned long long mask = (j == NR - 1 && (NPIX & 63)) ? ((1ull << (NPIX & 63)) - 1) : ~0ull;
            lds_dma16_sm(reinterpret_cast<const float*>(pn + (long long)(kgl * 2 + t) * pplane), dvoff[i],
                         lds0 + (unsigned)(buf * A_BYTES + t * A_PART + (kgl * NPP + j * 64) * 16), mask);
        }
    };
    const unsigned boff = (unsigned)(lane * 16);                       // [k-group kq][filter lp][8 channels]
    auto load_b = [&](f32x4 (&b)[2], int chunk, int item) {
        const unsigned char* base = wp_nt + ((long long)chunk * UF_ITEMS + item) * B_ITEM;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned char* sb = base + t * (B_ITEM / 2);
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(b[t]) : "v"(boff), "s"(sb) : "memory");
        }
    };

    spf4 acc[4][2][2];    // [low-resolution row of the wave][py][px]
#pragma unroll
    for (int a = 0; a < 16; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[a >> 2][(a >> 1) & 1][a & 1][i] = 0.f;

    // staged row r (0..5 of the wave's six) at column offset ox lives in register slot r, rows 2 and 3 at odd ox in 6 and 7
    const unsigned char* const aptr = smem + (kq * NPP + 4 * rg * COLS + 16 * mblk + lp) * 16;
    sph8 af[8][2];
    auto slot = [](int r, int ox) constexpr { return (r == 2 || r == 3) && (ox & 1) ? r + 4 : r; };
    auto load_arow = [&](int r, int ox) {
#pragma unroll
        for (int t = 0; t < (ONE ? 1 : 2); ++t)
            af[slot(r, ox)][t] = *reinterpret_cast<const sph8*>(aptr + t * A_PART + (r * COLS + ox) * 16);
    };

    f32x4 bq[4][2];       // weight sets in flight: set `it` lives in bq[it % 4]
    auto chunk_body = [&](int c, auto more_tag, auto chk_tag) {
        constexpr bool MORE = decltype(more_tag)::value, CHK = decltype(chk_tag)::value;
        constexpr int NA = (MORE && !PIN) ? NA_ALL : 0;   // pair input: the DMA follows the chunk's barrier
#pragma unroll
        for (int r = 0; r < 4; ++r) load_arow(r, 0);
#pragma unroll
        for (int it = 0; it < UF_ITEMS; ++it) {
            const UfItem t = uf_item(it);
            const bool first_of_group = it == 0 || uf_item(it - 1).s != t.s || uf_item(it - 1).ox != t.ox;
            if (first_of_group) {   // fetch what the NEXT groups read and this one does not hold
                if (t.s == 0) load_arow(4, t.ox);
                else if (t.s == 1) load_arow(5, t.ox);
                else if (t.ox < 2) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) load_arow(r, t.ox + 1);
                }
            }
            f32x4 (&bc)[2] = bq[it % 4];
            if (it + D < UF_ITEMS) load_b(bq[(it + D) % 4], c, it + D);
            else if (MORE) load_b(bq[(it + D) % 4], c + 1, it + D - UF_ITEMS);
            if constexpr (!PIN) {
                if (it == 0 && MORE) load_chunk(c + 1);
            }
            // outstanding, oldest first: b(it) b(it+1) b(it+2) [b(it+3) | inputs in issue order]
            if (it <= D) uf_wait_b<D * NBL + NA>(bc);
            else if (MORE || it + D < UF_ITEMS) uf_wait_b<D * NBL>(bc);
            else if (it == UF_ITEMS - 3) uf_wait_b<2 * NBL>(bc);
            else if (it == UF_ITEMS - 2) uf_wait_b<NBL>(bc);
            else uf_wait_b<0>(bc);
            sph8 bw[3];
            bw[0] = __builtin_bit_cast(sph8, bc[0]);
            bw[1] = __builtin_bit_cast(sph8, bc[1]);
            bw[2] = bw[0] * (_Float16)0.00048828125f;
            __builtin_amdgcn_sched_barrier(0);
            constexpr int TA[3] = {0, 0, 1};
#pragma unroll
            for (int k = 0; k < (ONE ? 1 : 3); ++k)
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) {
                    if (CHK && oy0 + 4 * rg + mb >= sH) continue;      // low-resolution row below the map: no MFMAs (wave-uniform)
                    acc[mb][t.py][t.px] = POUT ? __builtin_amdgcn_mfma_f32_16x16x32_f16(bw[k], af[slot(mb + t.s, t.ox)][TA[k]],
                                                                                         acc[mb][t.py][t.px], 0, 0, 0)
                                               : __builtin_amdgcn_mfma_f32_16x16x32_f16(af[slot(mb + t.s, t.ox)][TA[k]], bw[k],
                                                                                         acc[mb][t.py][t.px], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        if (MORE) {              // one buffer: every wave has read its last fragment of chunk c; the inputs arrived under set D+1's wait
            if constexpr (PIN) {
                // the first weight sets of chunk c+1 (fetched above, MORE) are in flight too: vmcnt(0) covers both
                dma_chunk(0, c + 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
#pragma unroll
                for (int u = 0; u < PR; ++u) store_round(0, u);
            }
            __syncthreads();
        }
    };

    if constexpr (PIN) dma_chunk(0, 0);
    else load_chunk(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (!PIN) {
#pragma unroll
        for (int u = 0; u < PR; ++u) store_round(0, u);
    }
    __syncthreads();
    auto k_loop = [&](auto chk_tag) {
        // the first weight fetches are issued INSIDE the variant that awaits them: a register copy at the branch between an
        // asm load and its vmcnt wait would copy what the register held before the data arrived
#pragma unroll
        for (int it = 0; it < D; ++it) load_b(bq[it], 0, it);
        for (int c = 0; c + 1 < nchunks; ++c) chunk_body(c, std::true_type{}, chk_tag);
        chunk_body(nchunks - 1, std::false_type{}, chk_tag);
    };
    if (!KBN_SPLIT_STRAIGHT || oy0 + ROWS > sH) k_loop(std::true_type{});   // tile with rows below the map (workgroup-uniform)
    else k_loop(std::false_type{});

    const float slope = p.act ? p.slope : 1.f;
    if constexpr (POUT) {
        // ---- pair epilogue: acc[mb][py][px][i]: low-resolution x = 16 mblk + lp, filter 4 kq + i: a lane holds half a granule
        // (channels 4 (kq & 1) ..) of k-group kq >> 1 of the outputs (2 Y + py, 2 x + px); 8-byte stores, two lanes per granule
        const float ps_out = sp_pair_out_scale(p, n);
        const long long oph = pair_plane_halves(H, W);
        _Float16* const pn = p.pair_out + (long long)n * p.pair_out_bstride;
        if (tid == 0) p.pair_out_scale[n] = ps_out;
        if (tx == 0 && ty == 0 && wave == 0 && lane < 4)    // the zero granules of the two k-groups x two terms
            *reinterpret_cast<f32x4*>(pn + (long long)lane * oph + (long long)H * W * 8) = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 inv4 = *reinterpret_cast<const f32x4*>(p.inv_scale + 4 * kq) * unscale;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * kq + i >= p.OC) inv4[i] = 0.f;          // channels past the last filter: zeros
        const int x = ox0 + 16 * mblk + lp;
        _Float16* const k0 = pn + (long long)((kq >> 1) * 2) * oph;
        float amax = 0.f;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const int Y = oy0 + 4 * rg + mb;
            if (Y >= sH) continue;                          // wave-uniform
#pragma unroll
            for (int py = 0; py < 2; ++py) {
                f32x4 v0, v1;                               // this lane's four channels of outputs (2 x, 2 x + 1)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float a = acc[mb][py][0][i] * inv4[i], b = acc[mb][py][1][i] * inv4[i];
                    v0[i] = a > 0.f ? a : a * slope;
                    v1[i] = b > 0.f ? b : b * slope;
                }
                if (x < sW) amax = sp_amax4(sp_amax4(amax, v0), v1);
                sph4 a1, a2, b1, b2;
                sp_split4(v0 * ps_out, a1, a2);
                sp_split4(v1 * ps_out, b1, b2);
                const spu4 g1 = sp_pair_exchange16(a1, b1), g2 = sp_pair_exchange16(a2, b2);   // every lane takes part
                if (x < sW) {                               // even kq: the whole granule of pixel 2 x, odd kq: of pixel 2 x + 1
                    const long long o = ((long long)(2 * Y + py) * W + 2 * x + (kq & 1)) * 8;
                    *reinterpret_cast<spu4*>(k0 + o) = g1;
                    if constexpr (!ONE) *reinterpret_cast<spu4*>(k0 + oph + o) = g2;   // (the one-term consumer never fetches the h2 planes)
                }
            }
        }
        if (p.out_amax) absmax_commit(p.out_amax + n, amax);
        return;
    }
    // ---- epilogue: acc[mb][py][px][i]: low-resolution x = 16 mblk + 4 kq + i, filter lp; outputs (2 Y + py, 2 x + px)
    const long long oplane = (long long)H * W;
    const int oc = nt * U16_NT + lp;
    const float inv = p.inv_scale[oc] * unscale;                    // the table is padded to whole n-tiles
    float* outc = p.out + (long long)n * p.out_bstride + (long long)oc * oplane;
    const int X = 2 * (ox0 + 16 * mblk + 4 * kq);                      // first of this lane's 8 output columns
    float amax = 0.f;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const int Y = oy0 + 4 * rg + mb;
        if (Y >= sH || oc >= p.OC) continue;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            float* orow = outc + (long long)(2 * Y + py) * W;
            f32x4 v0, v1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = acc[mb][py][j & 1][j >> 1] * inv;
                const float b = acc[mb][py][j & 1][2 + (j >> 1)] * inv;
                v0[j] = a > 0.f ? a : a * slope;
                v1[j] = b > 0.f ? b : b * slope;
            }
            if (X < W) { *reinterpret_cast<f32x4*>(orow + X) = v0; amax = sp_amax4(amax, v0); }
            if (X + 4 < W) { *reinterpret_cast<f32x4*>(orow + X + 4) = v1; amax = sp_amax4(amax, v1); }
        }
    }
    if (p.out_amax) absmax_commit(p.out_amax + n, amax);
}


// ------------------------------------------------------------------------------------------------------------------
// The folded up-conv with 64-FILTER tiles (layers whose filter count fills whole 64-wide tiles: KBNet's four wide
// up-convs, 256 / 128 / 128 / 64 filters).  upconv2x_split_kernel's wave owns two low-resolution rows x one 32-filter
// block x four parities; here it owns ONE row x TWO 32-filter blocks x four parities -- the same eight accumulator
// blocks -- so a workgroup covers 8 x 32 low-resolution pixels x 64 filters: per MFMA it stages and splits 340 pixels
// instead of 612, and every input tile is staged by half as many filter tiles.  On random operands the two kernels
// take the same time (1770 vs 1768 us over the four up-convs, tools/split_bench.py); inside a KITTI forward this one is
// 3 % faster (tools/layer_profile.py: 2330 vs 2400 us for the five up-convs).  Eight-row tiles also fit the 11- and 22-row maps better.  A in LDS as before ([part][k-group]
// [pixel][8 fp16], double buffered, 43 KiB); the sixteen weight sets of a chunk are 64 KiB now, so they go through LDS
// in HALVES of eight sets (32 KiB, two buffers): the DMA of the next half flies while the current half multiplies; two
// barriers per chunk.  Weights: [n-tile][chunk][set][part][k-group][64 filters][8 channels] fp16.
// (U64_NT, uf_wide: split_common.h)

__global__ void uf64_pack_kernel(const float* __restrict__ w, const float* __restrict__ inv_scale, _Float16* __restrict__ packed,
                                 int OC, int Cin, int nchunks, long long total, int tr) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    constexpr int per_item = 2 * 2 * U64_NT * 8, per_chunk = UF_ITEMS * per_item;
    int r = (int)(e % per_chunk);
    const long long q = e / per_chunk;
    const int chunk = (int)(q % nchunks), nt = (int)(q / nchunks);
    const int item = r / per_item; r -= item * per_item;
    const int part = r / (2 * U64_NT * 8); r -= part * 2 * U64_NT * 8;
    const int g = r / (U64_NT * 8); r -= g * U64_NT * 8;
    const int n = r >> 3, k = r & 7;
    const int c = chunk * SP_CK + g * 8 + k, oc = nt * U64_NT + n;
    _Float16 h = (_Float16)0.f;
    if (c < Cin && oc < OC) {
        const UfItem t = uf_item(item);
        const float ws = uf_fold(w + ((long long)oc * Cin + c) * 9, t.py, t.dy, t.px, t.dx, tr) * (1.f / inv_scale[oc]);
        const _Float16 w1 = (_Float16)ws;
        h = part == 0 ? w1 : (_Float16)(ws - (float)w1);
    }
    packed[e] = h;
}

// PIN: the input is a pair tensor (staged by LDS-DMA, nothing to split); POUT: the output is written as one (the MFMA
// operands swap roles, so that a lane's accumulator registers run over FILTERS of one pixel: four consecutive channels
// = half a granule per store).
template <bool PIN, bool POUT, bool MIXED = false, bool ONE = false, bool KSPLIT = false>   // MIXED: p.nblocks whole tiles, then p.tp_nblocks transposed ones; ONE, KSPLIT: see conv3x3_split_kernel
__global__ __launch_bounds__(SP_THREADS, 1) void upconv2x_split64_kernel(const SplitConvParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (!MIXED || (int)blockIdx.x < p.nblocks) {
        constexpr bool TP = false;
        const int block = blockIdx.x, nblocks = p.nblocks, tilesX = p.tilesX, tilesY = p.tilesY;
#include "upconv64_split_body.inc"
    } else if constexpr (MIXED) {
        constexpr bool TP = true;
        const int block = (int)blockIdx.x - p.nblocks, nblocks = p.tp_nblocks, tilesX = 1, tilesY = p.tp_tilesY;
#include "upconv64_split_body.inc"
    }
}

// ---- host side: the pack and the launches of mode 3 / 4 (kbn_conv3x3_split_pack_weight / _forward in conv_split.hip) ----
void upconv_split_pack(const float* w, float* inv_scale, _Float16* packed, int OC, int Cin, int ocpad, long long total, int tr,
                       hipStream_t stream) {
    const dim3 grid((unsigned)((total + 255) / 256));
    hipLaunchKernelGGL(uf_scale_kernel, dim3(ocpad), dim3(256), 0, stream, w, inv_scale, OC, Cin, tr);
    if (uf_narrow(OC, Cin)) hipLaunchKernelGGL(uf16_pack_kernel, grid, dim3(256), 0, stream, w, inv_scale, packed, OC, Cin, Cin / U16_CK, total, tr);
    else if (uf_wide(OC)) hipLaunchKernelGGL(uf64_pack_kernel, grid, dim3(256), 0, stream, w, inv_scale, packed, OC, Cin, Cin / SP_CK, total, tr);
    else hipLaunchKernelGGL(uf_pack_kernel, grid, dim3(256), 0, stream, w, inv_scale, packed, OC, Cin, Cin / SP_CK, total, tr);
}

int upconv_split_launch(SplitConvParams p, hipStream_t stream) {
    const bool one_term = knob(KNOB_FP16_ONE_TERM) != 0;   // THROUGHPUT-ONLY: h1 w1 alone
    int rc;
    if (uf_narrow(p.OC, p.Cin)) {   // 8 x 32 low-resolution pixels per workgroup of 4 waves, two workgroups per CU
        p.tilesY = ceil_div(p.sH, 8);
        const long long blocks8 = (long long)p.tilesX * p.tilesY * p.N * p.nTilesN;
        if (blocks8 > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
        p.nblocks = (int)blocks8;
        constexpr size_t lds16 = 2 * 4 * ((10 * 34 + 15) / 16 * 16) * 16;
        const bool pin = p.pair_src != nullptr, pout = p.pair_out != nullptr;
        if (one_term && pin && pout)   // THROUGHPUT-ONLY: the decoder's pair chain in one-term mode (the shipped form of deconv0's up-conv)
            rc = split_launch<upconv2x_split16_kernel<4, true, true, true>>(p.nblocks, 256, lds16, stream, p);
        else if (pout) rc = pin ? split_launch<upconv2x_split16_kernel<4, true, true>>(p.nblocks, 256, lds16, stream, p)
                                : split_launch<upconv2x_split16_kernel<4, false, true>>(p.nblocks, 256, lds16, stream, p);
        else rc = pin ? split_launch<upconv2x_split16_kernel<4, true>>(p.nblocks, 256, lds16, stream, p)
                      : split_launch<upconv2x_split16_kernel<4, false>>(p.nblocks, 256, lds16, stream, p);
    } else if (uf_wide(p.OC)) {   // 8 x 32 low-resolution pixels x 64 filters per workgroup
        p.tilesX = ceil_div(p.sW, 32); p.tilesY = ceil_div(p.sH, 8);
        const long long blocks64 = (long long)p.tilesX * p.tilesY * p.N * p.nTilesN * p.ksplit;
        if (blocks64 > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
        p.nblocks = (int)blocks64;
        constexpr size_t lds64 = 2 * (2 * 2 * 10 * 34 * 16) + 2 * (8 * 2 * 2 * 64 * 16);
        if (p.ksplit > 1)   // the latency form, whole tiles only
            return split_launch<upconv2x_split64_kernel<false, false, false, false, true>>(p.nblocks, SP_THREADS, lds64, stream, p);
        // a low-resolution map whose width leaves 1-16 columns behind the whole 32-column tiles: transposed tiles (16 rows x 16
        // columns) for that column, in the same launch (KBN_DEBUG & 512: off)
        const int wrem = p.sW % 32;
        const bool tp = p.sW >= 32 && wrem >= 1 && wrem <= 16 && !(knob(KNOB_DEBUG) & 512);
        if (tp) {
            p.tilesX = p.sW / 32;
            p.nblocks = p.tilesX * p.tilesY * p.N * p.nTilesN;
            p.tp_x0 = 32 * p.tilesX;
            p.tp_tilesY = ceil_div(p.sH, 16);
            p.tp_nblocks = p.tp_tilesY * p.N * p.nTilesN;
        }
        rc = split_dispatch([&](auto PIN, auto POUT, auto TP, auto ONE) {
            return split_launch<upconv2x_split64_kernel<PIN, POUT, TP, ONE>>(p.nblocks + (tp ? p.tp_nblocks : 0), SP_THREADS, lds64, stream, p);
        }, p.pair_src != nullptr, p.pair_out != nullptr, tp, one_term);
    } else {
        // two A buffers (18 x 34 pixels x 16 channels x two fp16 terms) + two buffers of sixteen weight sets
        rc = split_launch<upconv2x_split_kernel<true>>(p.nblocks, SP_THREADS, 2 * (2 * 2 * 18 * 34 * 16) + 2 * UF_ITEMS * (2 * 2 * UF_NT * 16),
                                                       stream, p);
    }
    if (rc != KBN_OK) return rc;
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

}  // namespace kbn
