// kb1_front.hip -- the full-resolution front of the encoder's image branch in ONE kernel, on the 16-bit matrix core:
//     conv0_image = act(conv3x3(image))                                  reference src/networks.py:364-365 (net_utils.Conv2d)
//     conv_image  = act(conv3x3 s2 (conv0_image))                        reference src/net_utils.py:1348   (KB block, level 0)
//     conv_fused  = act(conv1x1 s2 (cat[conv0_image, xyz]))              reference src/net_utils.py:1352-1369
// conv0_image -- 48 channels at full resolution, 82 MB per KITTI frame -- is consumed by these two convs only, so it is
// computed per tile (+ halo) and kept in LDS: it never reaches HBM (round 2 wrote and re-read 5.3 GB of it per 32-frame
// step: conv0_image at 4.1 TB/s + the fused fp32 KB kernel, 2.45 ms of a 12.8 ms step on the fp32 pipe).  All three convs take
// their fp32 products as three fp16 MFMAs over two-term splits of both operands, like csrc/conv_split.hip:
//     a 2^k = h1 + 2^-11 h2,   w 2^e = w1 + 2^-11 w2'   ->   a w 2^(e+k) = h1 w1 + 2^-11 (h1 w2' + h2 w1)
// with fp32 accumulators for the main and the small term.  The windows follow the data inside the kernel, tile by tile: k of
// the image from max |image| over the pixels the workgroup loads; k of the on-chip conv0 output from the BOUND
// max |conv0| <= (max_f sum |w0_f|) max |image| (the true maximum is not known before the values are written; the bound
// is within a few binades of it, and a window may sit 2^16 above the data before anything is lost --
// tests/test_split_math_cpu.py).  Outputs are fp32 NCHW with their absmax slots filled, like every other conv.
//
// Tile = 8 x 16 output pixels (half resolution) of one frame per workgroup of 8 waves; v_mfma_f32_16x16x32_f16 throughout.
//   A  the (2*8+3) x (2*16+3) image pixels the tile's conv0 outputs read: loaded, split, one 16-byte granule [8 channels]
//      per pixel and split term (channels >= c_in are zero).
//   B  conv0, 16 filters at a time: D[filter][pixel], A operand = weights, B operand = pixels; K = (tap, channel): k-group =
//      tap, so a B fragment is ONE ds_read_b128 of the granule at (pixel + tap offset).  The 16 x 16 result blocks hold 4
//      consecutive CHANNELS of a pixel per lane: LeakyReLU, zero outside the image (it is the padding of the next conv),
//      split with the bound's exponent, ds_write_b64 into X [term][k-group][17 x 33 pixels, columns de-interleaved][8 ch].
//   C  conv_image (nine taps, two per MFMA: K = [16 ch of tap t | 16 ch of tap t+1]) and conv_fused (centre tap) over
//      these 16 channels: D[pixel][filter], A operand = pixels of one output row per wave (stride-2 reads of X are
//      consecutive granules thanks to the de-interleave), B operand = weights from LDS (double buffered, LDS-DMA).
//   D  after the last chunk: scales, xyz channels of conv_fused in fp32 (kbn_kb_xyz_s2_forward computes them once per block),
//      LeakyReLU, 16-byte NCHW stores (a lane holds 4 consecutive pixels of a filter), absmax.
#include <type_traits>

#include "front_common.h"

namespace kbn {

struct FrontParams {
    const float* image;
    long long image_bstride;
    const float* tab;             // scales / xyz weights (FR_TAB floats)
    const _Float16* w0;           // [chunk][2 k-steps][term][4 k-groups][16 filters][8] -- k-group = (tap row, column pair), 8 = 2 pixels x 4 channels
    const _Float16* wc;           // [chunk]{[5 k-steps][term][4 k-groups][FI filters][8] (tap pairs) | [term][2 k-groups][FI][8] (conv_fused)}
    const float* xyz;             // N x 3 x h x w or null
    long long xyz_bstride;
    float* out_image;
    long long out_image_bstride;
    float* out_fused;
    long long out_fused_bstride;
    unsigned* amax_out_image;
    unsigned* amax_out_fused;
    int N, Cin, H, W, h, w, tilesX, tilesY, ntiles;
    float slope0, slope1;
    int vec4;
    // NEXT (kbn_kb1_front_next_forward): the NEXT KB level's conv_fused in the same launch -- a 1x1 stride-2 conv over
    // cat[conv_image, xyz of that level, conv_fused] reads exactly the even pixels of this tile's two outputs (no halo)
    const float* tab2;            // [2^-e per filter FO][xyz weights FO x 3]
    const _Float16* wn;           // [k-step][term][4 k-groups][FO filters][8]: K = (conv_image channels, conv_fused channels)
    const float* xyz2;            // N x 3 x h2 x w2 (kbn_kb_xyz_s2_forward of the next level)
    long long xyz2_bstride;
    float* out2;                  // N x FO x h2 x w2
    long long out2_bstride;
    unsigned* amax_out2;
    int h2, w2, vec4_2;
    float slope2;
};

// LDS per workgroup: IN 10.5 KB + X 35.1 KB + one chunk of conv_image / conv_fused weights 33 KB = 78.6 KB: TWO workgroups
// per CU, so that one's image loads, barriers and stores hide under the other's MFMAs.
// ONE: the THROUGHPUT-ONLY one-term mode (KBN_FP16_ONE_TERM=1, BASELINE configs[2]'s 16-bit leg): every product is h1 w1 alone -- plain fp16
// operands, fp32 accumulation, a third of the MFMAs, no h2 granules written or read
template <int NC0, int NBI, bool NEXT = false, bool ONE = false>   // conv0 filters / 16, conv_image = conv_fused filters / 16; NEXT: + the next level's conv_fused
__global__ __launch_bounds__(FR_THREADS, NEXT ? 4 : 2) void kb1_front_kernel(const FrontParams p) {
    constexpr int FI = NBI * 16;
    constexpr int IN_PART = FR_NIN * 8, IN_BYTES = 2 * IN_PART;            // [term][pixel][4 channels] fp16
    constexpr int X_KG = FR_XP * 16, X_PART = 2 * X_KG, X_BYTES = 2 * X_PART;
    constexpr int WC_KQ = FI * 16, WC_PART = 4 * WC_KQ, WC_KS = 2 * WC_PART, WC_FUSED = 2 * 2 * WC_KQ, WC_CHUNK = 5 * WC_KS + WC_FUSED;
    constexpr int OFF_X = IN_BYTES, OFF_WC = OFF_X + X_BYTES;
    static_assert(OFF_WC + WC_CHUNK <= 80 * 1024, "two workgroups per CU");
    constexpr int NBLK = (FR_NB0 + 7) / 8;                                  // conv0 pixel blocks per wave: 5 (waves 4-7: 4)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 6, 2), 0");   // fp16 results flush subnormals (see conv3x3_split_kernel)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    int bid = xcd_remap(blockIdx.x, p.ntiles);
    const int tx = bid % p.tilesX;
    bid /= p.tilesX;
    const int ty = bid % p.tilesY;
    const int n = bid / p.tilesY;
    const int oy0 = ty * FR_TH, ox0 = tx * FR_TW;
    const int H = p.H, W = p.W;
    const long long plane = (long long)H * W;

    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(reinterpret_cast<const float*>(smem)));
    auto dma_wc = [&](int chunk) {   // whole-workgroup copy of one chunk's weights, 16 bytes per lane and round
        const float* src = reinterpret_cast<const float*>(p.wc + (long long)chunk * (WC_CHUNK / 2));
        constexpr int n4 = WC_CHUNK / 16;
#pragma unroll
        for (int e0 = 0; e0 < n4; e0 += FR_THREADS) {
            const int eb = e0 + wave * 64;
            if (eb + lane < n4) lds_dma16_s(src + eb * 4, (unsigned)(lane * 16), lds0 + (unsigned)(OFF_WC + eb * 16));
        }
    };
    dma_wc(0);

    // ---- A: image tile -> split entries [4 channels] per pixel (two pixels = one 16-byte K group of conv0).  The fp16
    // windows are the TILE's own: max |image| over the pixels this workgroup reads (one LDS reduction) places the image's, the
    // bound L1max0 * that maximum conv0's -- no pass over the image beforehand, and a tile never pays for a bright spot elsewhere.
    float pre_img, un_img, pre0, un0;
    {
        const float* img = p.image + (long long)n * p.image_bstride;
        ff4 raw[2];
        float tm = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int pix = u * FR_THREADS + tid;
            const int r = pix / FR_R0W, c = pix - r * FR_R0W;
            const int Y = 2 * oy0 - 2 + r, X = 2 * ox0 - 2 + c;
            const bool ok = pix < FR_NP0 && Y >= 0 && Y < H && X >= 0 && X < W;   // entries past the tile stay zero (pair reads touch one)
            const float* src = img + (long long)(ok ? Y : 0) * W + (ok ? X : 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                raw[u][j] = (ok && j < p.Cin) ? src[(long long)(j < p.Cin ? j : 0) * plane] : 0.f;
                tm = fmaxf(tm, fin_abs(raw[u][j]));
            }
        }
        tm = __uint_as_float(wave_max_bits(tm));
        float* red = reinterpret_cast<float*>(smem + OFF_X);   // X is idle until conv0 writes it (after the next barrier)
        if (lane == 0) red[wave] = tm;
        __syncthreads();
        tm = fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
        const unsigned abits = __builtin_amdgcn_readfirstlane(__float_as_uint(tm));
        fr_scales(abits, pre_img, un_img);
        fr_scales(__float_as_uint(p.tab[0] * __uint_as_float(abits)), pre0, un0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int pix = u * FR_THREADS + tid;
            if (pix < FR_NIN) {
                fh4 h1, h2;
                fr_split4(raw[u] * pre_img, h1, h2);
                *reinterpret_cast<fh4*>(smem + pix * 8) = h1;
                *reinterpret_cast<fh4*>(smem + IN_PART + pix * 8) = h2;
            }
        }
    }

    // ---- per-lane offsets, computed once per tile.  The tile decode, the window reduction, the conv0 block table / epilogue / dispatch, the
    // stride-2 offsets and the quad store are written out here AND in kb1_depth_front_kernel (csrc/kb1_depth_front.hip): as shared
    // force-inlined helpers they changed the register counts of some instantiation.  A fix to one copy belongs in the other too.
    // conv0: k-group g = 4 ks + kq = (tap row g >> 1, column pair g & 1: columns 0-1 / 2-3, the fourth carries zero weights);
    // groups 6, 7 are all zero weights: any valid address
    int goff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int g = min(4 * ks + kq, 5);
        goff[ks] = ((g >> 1) * FR_R0W + 2 * (g & 1)) * 8;
    }
    // conv0 block j (0..35) of the 17 x 33 region: j < 34: row j >> 1, columns 16 (j & 1) + l15; 34, 35: the last column (32),
    // rows l15 / 16 + l15.  Wave w takes blocks w, w + 8, .. (five for waves 0-3, four for the others).
    int inoff[NBLK], xoff[NBLK];
    unsigned inside = 0, valid = 0;
#pragma unroll
    for (int i = 0; i < NBLK; ++i) {
        const int j = wave + 8 * i;
        const int r1 = j < 34 ? (j >> 1) : (j == 34 ? l15 : 16 + l15);
        const int c1 = j < 34 ? 16 * (j & 1) + l15 : 32;
        const bool ok = r1 < FR_R1H;
        const int r1c = ok ? r1 : FR_R1H - 1;
        const int Y = 2 * oy0 - 1 + r1c, X = 2 * ox0 - 1 + c1;
        inoff[i] = (r1c * FR_R0W + c1) * 8;
        const int xi = r1c * FR_R1W + ((c1 & 1) ? (FR_R1W + 1) / 2 + (c1 >> 1) : (c1 >> 1));   // columns de-interleaved
        xoff[i] = OFF_X + (kq >> 1) * X_KG + xi * 16 + (kq & 1) * 8;
        if (ok) valid |= 1u << i;
        if (ok && Y >= 0 && Y < H && X >= 0 && X < W) inside |= 1u << i;
    }
    // a tile whose halo region lies inside the image needs no zero padding of conv0's output (workgroup-uniform)
    const bool interior = 2 * oy0 - 1 >= 0 && 2 * oy0 - 1 + FR_R1H <= H && 2 * ox0 - 1 >= 0 && 2 * ox0 - 1 + FR_R1W <= W;
    // conv_image: k-step s covers taps 2 s, 2 s + 1 (k-groups 0-1 / 2-3), k-group parity = which 8 of the chunk's 16 channels
    const int yrow = wave;   // this wave's output row of the tile
    int aoff[5], aoff_f;
    {
        const int kg = kq & 1, tsel = kq >> 1;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int tap = min(2 * s + tsel, 8);
            const int ky = tap / 3, kx = tap % 3;
            const int col = kx == 0 ? l15 : (kx == 1 ? (FR_R1W + 1) / 2 + l15 : l15 + 1);
            aoff[s] = OFF_X + (kg * FR_XP + (2 * yrow + ky) * FR_R1W + col) * 16;
        }
        aoff_f = OFF_X + (kg * FR_XP + (2 * yrow + 1) * FR_R1W + (FR_R1W + 1) / 2 + l15) * 16;
    }
    const bool row_live = oy0 + yrow < p.h;   // wave-uniform
    const int nblk = wave + 8 * (NBLK - 1) < FR_NB0 ? NBLK : NBLK - 1;   // wave-uniform

    ff4 mI[NBI], sI[NBI], mF[NBI], sF[NBI];
#pragma unroll
    for (int nb = 0; nb < NBI; ++nb) {
        mI[nb] = (ff4){0.f, 0.f, 0.f, 0.f}; sI[nb] = mI[nb]; mF[nb] = mI[nb]; sF[nb] = mI[nb];
    }
    const float* inv0 = p.tab + 4;
    const float sc0 = un_img * pre0;   // conv0's result leaves the accumulators already in the next window's scale
    __syncthreads();   // IN complete

#pragma unroll 1
    for (int c = 0; c < NC0; ++c) {
        // ---- B: conv0, filters 16 c .. 16 c + 15, over the 561 pixels of the tile's halo region
        {
            fh8 a1[2], a2[2];   // weights straight from L2 / L1: 4 KB per chunk
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                a1[ks] = *reinterpret_cast<const fh8*>(p.w0 + ((c * 2 + ks) * 2 + 0) * 512 + lane * 8);
                a2[ks] = *reinterpret_cast<const fh8*>(p.w0 + ((c * 2 + ks) * 2 + 1) * 512 + lane * 8);
            }
            ff4 sc = *reinterpret_cast<const ff4*>(inv0 + 16 * c + 4 * kq);   // 2^-e of this lane's four filters
            sc *= sc0;
            const f32x2 sc01 = {sc[0], sc[1]}, sc23 = {sc[2], sc[3]};
            auto block = [&](int i, auto border_tag) {
                constexpr bool BORDER = decltype(border_tag)::value;
                const unsigned char* inb = smem + inoff[i];
                ff4 m = (ff4){0.f, 0.f, 0.f, 0.f}, s = m;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const fh4 b1l = *reinterpret_cast<const fh4*>(inb + goff[ks]);
                    const fh4 b1h = *reinterpret_cast<const fh4*>(inb + goff[ks] + 8);
                    const fh8 b1 = __builtin_shufflevector(b1l, b1h, 0, 1, 2, 3, 4, 5, 6, 7);
                    m = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[ks], b1, m, 0, 0, 0);
                    if constexpr (!ONE) {
                        const fh4 b2l = *reinterpret_cast<const fh4*>(inb + IN_PART + goff[ks]);
                        const fh4 b2h = *reinterpret_cast<const fh4*>(inb + IN_PART + goff[ks] + 8);
                        const fh8 b2 = __builtin_shufflevector(b2l, b2h, 0, 1, 2, 3, 4, 5, 6, 7);
                        s = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[ks], b1, s, 0, 0, 0);
                        s = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[ks], b2, s, 0, 0, 0);
                    }
                }
                // (main + 2^-11 small) 2^-e 2^(k0 - k), LeakyReLU as max(t, slope t) (0 <= slope <= 1), in packed fp32
                f32x2 t01 = (f32x2){s[0], s[1]} * 0.00048828125f + (f32x2){m[0], m[1]};
                f32x2 t23 = (f32x2){s[2], s[3]} * 0.00048828125f + (f32x2){m[2], m[3]};
                t01 *= sc01; t23 *= sc23;
                const f32x2 u01 = t01 * p.slope0, u23 = t23 * p.slope0;
                ff4 v = {fmaxf(t01[0], u01[0]), fmaxf(t01[1], u01[1]), fmaxf(t23[0], u23[0]), fmaxf(t23[1], u23[1])};
                if (BORDER && !((inside >> i) & 1)) v = (ff4){0.f, 0.f, 0.f, 0.f};   // outside the image: the zero padding of conv_image
                fh4 h1, h2;
                fr_split4(v, h1, h2);
                if (!BORDER || ((valid >> i) & 1)) {
                    *reinterpret_cast<fh4*>(smem + xoff[i]) = h1;
                    if constexpr (!ONE) *reinterpret_cast<fh4*>(smem + xoff[i] + X_PART) = h2;
                }
            };
            if (interior) {
#pragma unroll
                for (int i = 0; i < NBLK - 1; ++i) block(i, std::false_type{});     // blocks 0 .. 31: whole rows of 16 pixels
                if (NBLK - 1 < nblk) block(NBLK - 1, std::true_type{});              // 32 .. 35: the last row / the last column
            } else {
#pragma unroll
                for (int i = 0; i < NBLK; ++i)
                    if (i < nblk) block(i, std::true_type{});
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this chunk's conv_image / conv_fused weights (DMA issued a stage ago)
        __syncthreads();
        // ---- C: conv_image (taps in pairs) and conv_fused (centre tap) over these 16 channels
        if (row_live) {
            const unsigned char* wcb = smem + OFF_WC + kq * WC_KQ + l15 * 16;
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const fh8 a1 = *reinterpret_cast<const fh8*>(smem + aoff[s]);
                fh8 a2 = a1;
                if constexpr (!ONE) a2 = *reinterpret_cast<const fh8*>(smem + X_PART + aoff[s]);
#pragma unroll
                for (int nb = 0; nb < NBI; ++nb) {
                    const fh8 b1 = *reinterpret_cast<const fh8*>(wcb + s * WC_KS + nb * 256);
                    mI[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, mI[nb], 0, 0, 0);
                    if constexpr (!ONE) {
                        const fh8 b2 = *reinterpret_cast<const fh8*>(wcb + s * WC_KS + WC_PART + nb * 256);
                        sI[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b2, sI[nb], 0, 0, 0);
                        sI[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, b1, sI[nb], 0, 0, 0);
                    }
                }
            }
            {   // conv_fused: K = this chunk's 16 channels at the centre tap; k-groups 2, 3 of the MFMA are zeroed on the A side
                fh8 a1 = *reinterpret_cast<const fh8*>(smem + aoff_f);
                fh8 a2 = a1;
                if constexpr (!ONE) a2 = *reinterpret_cast<const fh8*>(smem + X_PART + aoff_f);
                if (kq >= 2) { a1 = (fh8)(_Float16)0.f; a2 = a1; }
                const unsigned char* wf = smem + OFF_WC + 5 * WC_KS + (kq & 1) * WC_KQ + l15 * 16;
#pragma unroll
                for (int nb = 0; nb < NBI; ++nb) {
                    const fh8 b1 = *reinterpret_cast<const fh8*>(wf + nb * 256);
                    mF[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, mF[nb], 0, 0, 0);
                    if constexpr (!ONE) {
                        const fh8 b2 = *reinterpret_cast<const fh8*>(wf + 2 * WC_KQ + nb * 256);
                        sF[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b2, sF[nb], 0, 0, 0);
                        sF[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, b1, sF[nb], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();   // X and the weight buffer are free again
        if (c + 1 < NC0) dma_wc(c + 1);
    }

    // ---- D: a lane holds pixels x = 4 kq .. 4 kq + 3 of row yrow for filter 16 nb + l15
    const int Yo = oy0 + yrow, Xo = ox0 + 4 * kq;
    float amI = 0.f, amF = 0.f;
    f32x2 eI[NEXT ? NBI : 1], eF[NEXT ? NBI : 1];   // NEXT: this lane's two EVEN pixels (x = 4 kq, 4 kq + 2) of both outputs, zero outside the map
    if constexpr (NEXT) {
#pragma unroll
        for (int nb = 0; nb < NBI; ++nb) { eI[nb] = (f32x2){0.f, 0.f}; eF[nb] = eI[nb]; }
    }
    if (row_live && Xo < p.w) {
        const long long oplane = (long long)p.h * p.w;
        const long long pix = (long long)Yo * p.w + Xo;
        ff4 xz[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            xz[j] = (ff4){0.f, 0.f, 0.f, 0.f};
            if (p.xyz) {
                const float* xp = p.xyz + (long long)n * p.xyz_bstride + j * oplane + pix;
                if (p.vec4) {   // w % 4 == 0: the quad is inside the row (the caller checked xyz's alignment with the outputs')
                    xz[j] = *reinterpret_cast<const ff4*>(xp);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (Xo + r < p.w) xz[j][r] = xp[r];
                }
            }
        }
        const float* invI = p.tab + 4 + 64;
        const float* invF = p.tab + 4 + 128;
        const float* wx = p.tab + 4 + 192;
#pragma unroll
        for (int nb = 0; nb < NBI; ++nb) {
            const int f = nb * 16 + l15;
            const float scI = invI[f] * un0, scF = invF[f] * un0;
            const float w0x = wx[f * 3], w1x = wx[f * 3 + 1], w2x = wx[f * 3 + 2];
            ff4 vI, vF;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = __builtin_fmaf(sI[nb][r], 0.00048828125f, mI[nb][r]) * scI;
                vI[r] = a > 0.f ? a : a * p.slope1;
                float b = __builtin_fmaf(sF[nb][r], 0.00048828125f, mF[nb][r]) * scF;
                b = __builtin_fmaf(w2x, xz[2][r], __builtin_fmaf(w1x, xz[1][r], __builtin_fmaf(w0x, xz[0][r], b)));   // fixed order: the same bits in every instantiation
                vF[r] = b > 0.f ? b : b * p.slope1;
            }
            if constexpr (NEXT) {
                const bool two = Xo + 2 < p.w;
                eI[nb] = (f32x2){vI[0], two ? vI[2] : 0.f};
                eF[nb] = (f32x2){vF[0], two ? vF[2] : 0.f};
            }
            if constexpr (NEXT) {
                // the values wait in the accumulator registers: every store of this kernel is issued BEHIND stage E, whose loads would
                // otherwise queue behind these stores in the in-order vmcnt and wait for their write acknowledgements
                mI[nb] = vI; mF[nb] = vF;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (p.vec4 || Xo + r < p.w) { amI = fmaxf(amI, fin_abs(vI[r])); amF = fmaxf(amF, fin_abs(vF[r])); }
                continue;
            }
            float* oi = p.out_image + (long long)n * p.out_image_bstride + f * oplane + pix;
            float* of = p.out_fused + (long long)n * p.out_fused_bstride + f * oplane + pix;
            if (p.vec4) {
                *reinterpret_cast<ff4*>(oi) = vI;
                *reinterpret_cast<ff4*>(of) = vF;
#pragma unroll
                for (int r = 0; r < 4; ++r) { amI = fmaxf(amI, fin_abs(vI[r])); amF = fmaxf(amF, fin_abs(vF[r])); }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (Xo + r < p.w) {
                        oi[r] = vI[r]; of[r] = vF[r];
                        amI = fmaxf(amI, fin_abs(vI[r])); amF = fmaxf(amF, fin_abs(vF[r]));
                    }
            }
        }
    }
    auto store_own = [&]() {   // NEXT: phase D's stores, issued after stage E
        if (row_live && Xo < p.w) {
            const long long oplane = (long long)p.h * p.w;
            const long long pix = (long long)Yo * p.w + Xo;
#pragma unroll
            for (int nb = 0; nb < NBI; ++nb) {
                const int f = nb * 16 + l15;
                float* oi = p.out_image + (long long)n * p.out_image_bstride + f * oplane + pix;
                float* of = p.out_fused + (long long)n * p.out_fused_bstride + f * oplane + pix;
                if (p.vec4) {
                    *reinterpret_cast<ff4*>(oi) = mI[nb];
                    *reinterpret_cast<ff4*>(of) = mF[nb];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (Xo + r < p.w) { oi[r] = mI[nb][r]; of[r] = mF[nb][r]; }
                }
            }
        }
    };
    if (p.amax_out_image) absmax_commit(p.amax_out_image + n, amI);
    if (p.amax_out_fused) absmax_commit(p.amax_out_fused + n, amF);

    // ---- E (NEXT): conv_fused of the next KB level, reference src/net_utils.py:1352-1369 one level down: a 1x1 stride-2 conv over
    // cat[conv_image, xyz, conv_fused] of THIS level samples the pixels (2 y, 2 x) -- for this tile the 4 x 8 even pixels of the two
    // outputs the lanes still hold.  They become split granules G [term][k-group = channel / 8][32 pixels][8] in the (idle) X buffer,
    // window = the tile's own maximum; D[pixel][filter] over K = 2 FI channels, weights straight from L2 / L1 (36 KB, shared by every
    // tile); the three backprojection channels of the next level enter in fp32 like this level's in phase D.
    if constexpr (NEXT) {
        constexpr int FO = 2 * FI, NBK = FO / 16, KG2 = 2 * FI / 8, KS2 = KG2 / 4;
        static_assert(KG2 % 4 == 0, "whole k-steps");
        constexpr int G_PART = KG2 * 32 * 16;
        static_assert(2 * G_PART + 64 <= X_BYTES, "G overlays X");
        unsigned char* const G = smem + OFF_X;
        float* const red2 = reinterpret_cast<float*>(smem + OFF_X + 2 * G_PART);
        const bool even_row = (yrow & 1) == 0;   // wave-uniform
        float tm = 0.f;
        if (even_row) {
#pragma unroll
            for (int nb = 0; nb < NBI; ++nb)
                tm = fmaxf(fmaxf(tm, fmaxf(fin_abs(eI[nb][0]), fin_abs(eI[nb][1]))), fmaxf(fin_abs(eF[nb][0]), fin_abs(eF[nb][1])));
        }
        {
            const unsigned tb = wave_max_bits(tm);
            if (lane == 0) red2[wave] = __uint_as_float(tb);
        }
        // wave nbk < NBK owns the filter block 16 nbk .. 16 nbk + 15 for BOTH pixel blocks of the tile, so that a weight fragment is
        // fetched once per tile (the 36 KB of weights against 32 pixels are what this stage costs: every tile pulls them from L2 / L1);
        // the fragments are requested before the barriers
        static_assert(NBK <= 8, "one filter block per wave");
        const bool has_blk = wave < NBK;   // wave-uniform
        fh8 wb1[KS2], wb2[KS2];
        if (has_blk) {
            const int f = 16 * wave + l15;
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
                wb1[ks] = *reinterpret_cast<const fh8*>(p.wn + ((long long)((ks * 2 + 0) * 4 + kq) * FO + f) * 8);
                if constexpr (!ONE) wb2[ks] = *reinterpret_cast<const fh8*>(p.wn + ((long long)((ks * 2 + 1) * 4 + kq) * FO + f) * 8);
            }
        }
        __syncthreads();
        tm = fmaxf(fmaxf(fmaxf(red2[0], red2[1]), fmaxf(red2[2], red2[3])), fmaxf(fmaxf(red2[4], red2[5]), fmaxf(red2[6], red2[7])));
        float pre2, un2;
        fr_scales(__builtin_amdgcn_readfirstlane(__float_as_uint(tm)), pre2, un2);
        if (even_row) {
            const int pbase = (yrow >> 1) * 8 + 2 * kq;
#pragma unroll
            for (int nb = 0; nb < NBI; ++nb) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {   // conv_image channels first, conv_fused channels behind them (the reference's cat order)
                    const f32x2 v = (t == 0 ? eI[nb] : eF[nb]) * pre2;
                    const fh2 c1 = __builtin_convertvector(v, fh2);
                    const f32x2 f1 = {(float)c1[0], (float)c1[1]};
                    const f32x2 r = (v - f1) * 2048.f;
                    const fh2 c2 = __builtin_convertvector(r, fh2);
                    const int kg = t * (FI / 8) + 2 * nb + (l15 >> 3);
                    _Float16* g1 = reinterpret_cast<_Float16*>(G + (kg * 32 + pbase) * 16) + (l15 & 7);
                    _Float16* g2 = reinterpret_cast<_Float16*>(G + G_PART + (kg * 32 + pbase) * 16) + (l15 & 7);
                    g1[0] = c1[0]; g1[8] = c1[1];
                    if constexpr (!ONE) { g2[0] = c2[0]; g2[8] = c2[1]; }
                }
            }
        }
        __syncthreads();
        const float* inv2 = p.tab2;
        const float* wx2 = p.tab2 + FO;
        const long long plane2 = (long long)p.h2 * p.w2;
        float am2 = 0.f;
        if (has_blk) {
            const int f = 16 * wave + l15;
            ff4 m[2], sm[2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) { m[mb] = (ff4){0.f, 0.f, 0.f, 0.f}; sm[mb] = m[mb]; }
#pragma unroll
            for (int ks = 0; ks < KS2; ++ks) {
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    const fh8 a1 = *reinterpret_cast<const fh8*>(G + ((4 * ks + kq) * 32 + 16 * mb + l15) * 16);
                    m[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, wb1[ks], m[mb], 0, 0, 0);
                    if constexpr (!ONE) {
                        const fh8 a2 = *reinterpret_cast<const fh8*>(G + G_PART + ((4 * ks + kq) * 32 + 16 * mb + l15) * 16);
                        sm[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, wb2[ks], sm[mb], 0, 0, 0);
                        sm[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, wb1[ks], sm[mb], 0, 0, 0);
                    }
                }
            }
            const float sc = inv2[f] * un2;
            const float w0x = wx2[f * 3], w1x = wx2[f * 3 + 1], w2x = wx2[f * 3 + 2];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                // rows 4 kq + r of the block = pixels 16 mb + 4 kq + r of the tile's 4 x 8 even pixels: row 2 mb + (kq >> 1), columns 4 (kq & 1) + r
                const int Y2 = (oy0 >> 1) + 2 * mb + (kq >> 1), X2 = (ox0 >> 1) + 4 * (kq & 1);
                if (Y2 < p.h2 && X2 < p.w2) {
                    const long long pix2 = (long long)Y2 * p.w2 + X2;
                    const float* xp = p.xyz2 + (long long)n * p.xyz2_bstride + pix2;
                    float* op = p.out2 + (long long)n * p.out2_bstride + f * plane2 + pix2;
                    ff4 xz[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        if (p.vec4_2) {
                            xz[j] = *reinterpret_cast<const ff4*>(xp + j * plane2);
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) xz[j][r] = X2 + r < p.w2 ? xp[j * plane2 + r] : 0.f;
                        }
                    }
                    ff4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float t = __builtin_fmaf(sm[mb][r], 0.00048828125f, m[mb][r]) * sc;
                        t = __builtin_fmaf(w2x, xz[2][r], __builtin_fmaf(w1x, xz[1][r], __builtin_fmaf(w0x, xz[0][r], t)));
                        v[r] = t > 0.f ? t : t * p.slope2;
                    }
                    if (p.vec4_2) {
                        *reinterpret_cast<ff4*>(op) = v;
#pragma unroll
                        for (int r = 0; r < 4; ++r) am2 = fmaxf(am2, fin_abs(v[r]));
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (X2 + r < p.w2) { op[r] = v[r]; am2 = fmaxf(am2, fin_abs(v[r])); }
                    }
                }
            }
        }
        store_own();
        if (p.amax_out2) absmax_commit(p.amax_out2 + n, am2);
    }
}

// ---- weight packing ---------------------------------------------------------------------------------------------
// table: per-filter 2^-e (largest |w 2^e| in [2^12, 2^13)), the bound factor L1max0 = max_f sum |w0_f|, the fp32 xyz weights
__global__ void front_table_kernel(const float* __restrict__ w0, const float* __restrict__ wi, const float* __restrict__ wf,
                                   float* __restrict__ tab, int Cin, int F0, int FI) {
    __shared__ float red[256], red2[256];
    const int which = blockIdx.y, f = blockIdx.x;   // which 0: conv0, 1: conv_image, 2: conv_fused
    const int nf = which == 0 ? F0 : FI;
    const int per = which == 0 ? Cin * 9 : (which == 1 ? F0 * 9 : F0 + 3);
    const float* w = which == 0 ? w0 : (which == 1 ? wi : wf);
    float m = 0.f, l1 = 0.f;
    if (f < nf)
        for (int i = threadIdx.x; i < per; i += 256) {
            const float a = fabsf(w[(long long)f * per + i]);
            m = fmaxf(m, a);
            l1 += a;
        }
    red[threadIdx.x] = m;
    red2[threadIdx.x] = l1;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
            red2[threadIdx.x] += red2[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int ex = FR_WEXP;
        if (red[0] > 0.f && red[0] < 3.0e38f) (void)frexpf(red[0], &ex);
        int e = FR_WEXP - ex;
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
        tab[4 + 64 * which + f] = ldexpf(1.f, -e);
        if (which == 0 && f < F0) atomicMax(reinterpret_cast<unsigned*>(tab), __float_as_uint(red2[0]));   // L1max0 (non-negative floats order like their bits)
        if (which == 2 && f < FI)
            for (int j = 0; j < 3; ++j) tab[4 + 192 + f * 3 + j] = wf[(long long)f * (F0 + 3) + F0 + j];
    }
}


// conv0 panel: [chunk][k-step 2][term][k-group 4][filter 16][8]; k-group g = 4 ks + kq = (tap row g >> 1, column pair g & 1),
// slot j = (column 2 (g & 1) + (j >> 2), channel j & 3); groups >= 6, column 3, channels >= Cin: zero
__global__ void front_pack0_kernel(const float* __restrict__ w0, const float* __restrict__ tab, _Float16* __restrict__ out, int Cin, int F0,
                                   int total) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int r = e;
    const int j = r & 7; r >>= 3;
    const int m = r & 15; r >>= 4;
    const int kq = r & 3; r >>= 2;
    const int term = r & 1; r >>= 1;
    const int ks = r & 1, c = r >> 1;
    const int g = 4 * ks + kq, f = 16 * c + m;
    const int ky = g >> 1, kx = 2 * (g & 1) + (j >> 2), ch = j & 3;
    _Float16 h = (_Float16)0.f;
    if (g < 6 && kx < 3 && ch < Cin && f < F0) h = fr_term(w0[((long long)f * Cin + ch) * 9 + ky * 3 + kx] / tab[4 + f], term);
    out[e] = h;
}

// conv_image + conv_fused panel, per chunk: [k-step 5][term][k-group 4][filter FI][8]: tap 2 s + (kq >> 1) (< 9, else zero),
// channel 16 chunk + 8 (kq & 1) + j of conv_image; then [term][k-group 2][filter FI][8]: conv_fused's weights of channels
// 16 chunk + 8 kq + j
__global__ void front_packc_kernel(const float* __restrict__ wi, const float* __restrict__ wf, const float* __restrict__ tab,
                                   _Float16* __restrict__ out, int F0, int FI, int total) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int per_chunk = (5 * 2 * 4 + 2 * 2) * FI * 8;
    const int c = e / per_chunk;
    int r = e - c * per_chunk;
    _Float16 h = (_Float16)0.f;
    if (r < 5 * 2 * 4 * FI * 8) {
        const int j = r & 7; r >>= 3;
        const int f = r % FI; r /= FI;
        const int kq = r & 3; r >>= 2;
        const int term = r & 1; r >>= 1;
        const int s = r;
        const int ch = 16 * c + 8 * (kq & 1) + j, tap = 2 * s + (kq >> 1);
        if (ch < F0 && tap < 9) h = fr_term(wi[((long long)f * F0 + ch) * 9 + tap] / tab[4 + 64 + f], term);
    } else {
        r -= 5 * 2 * 4 * FI * 8;
        const int j = r & 7; r >>= 3;
        const int f = r % FI; r /= FI;
        const int kg = r & 1; r >>= 1;
        const int term = r;
        const int ch = 16 * c + 8 * kg + j;
        if (ch < F0) h = fr_term(wf[(long long)f * (F0 + 3) + ch] / tab[4 + 128 + f], term);
    }
    out[e] = h;
}

// next-level conv_fused panel (kb1_front_kernel<.., NEXT>): tab2 = [2^-e per filter FO][xyz weights FO x 3], then
// [k-step][term][k-group 4][filter FO][8]: K index 32 ks + 8 kq + j = channel c of cat[conv_image (CI), conv_fused (CF)];
// the reference's weight columns are [image CI | xyz 3 | fused CF] (src/net_utils.py:1362-1368)
__global__ void front_next_pack_kernel(const float* __restrict__ wf, float* __restrict__ tab2, _Float16* __restrict__ out, int CI, int CF, int FO,
                                       int total) {
    __shared__ float inv[128];
    const int per = CI + 3 + CF;
    for (int f = threadIdx.x; f < FO; f += blockDim.x) {
        float m = 0.f;
        for (int c = 0; c < per; ++c)
            if (c < CI || c >= CI + 3) m = fmaxf(m, fabsf(wf[(long long)f * per + c]));
        int ex = FR_WEXP;
        if (m > 0.f && m < 3.0e38f) (void)frexpf(m, &ex);
        int e = FR_WEXP - ex;
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
        inv[f] = ldexpf(1.f, -e);
        tab2[f] = inv[f];
        for (int j = 0; j < 3; ++j) tab2[FO + f * 3 + j] = wf[(long long)f * per + CI + j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        int r = e;
        const int j = r & 7; r >>= 3;
        const int f = r % FO; r /= FO;
        const int kq = r & 3; r >>= 2;
        const int term = r & 1; r >>= 1;
        const int c = 32 * r + 8 * kq + j;
        _Float16 h = (_Float16)0.f;
        if (c < CI + CF) h = fr_term(wf[(long long)f * per + (c < CI ? c : c + 3)] / inv[f], term);
        out[e] = h;
    }
}

}  // namespace kbn

extern "C" {

static bool front_shape_ok(int c_in, int f0, int fi) { return c_in >= 1 && c_in <= 4 && f0 == 48 && fi == 48; }
static size_t front_w0_halves(int f0) { return (size_t)(f0 / 16) * 2 * 2 * 64 * 8; }
static size_t front_wc_halves(int f0, int fi) { return (size_t)(f0 / 16) * (5 * 2 * 4 + 2 * 2) * fi * 8; }

size_t kbn_kb1_front_packed_weight_bytes(int image_channels, int conv0_filters, int kb_filters) {
    if (!front_shape_ok(image_channels, conv0_filters, kb_filters)) return 0;
    return (size_t)kbn::FR_TAB * 4 + 2 * (front_w0_halves(conv0_filters) + front_wc_halves(conv0_filters, kb_filters));
}

int kbn_kb1_front_pack_weight(const float* w_conv0, const float* w_conv_image, const float* w_conv_fused, void* packed,
                              int image_channels, int conv0_filters, int kb_filters, kbn_stream_t stream) {
    using namespace kbn;
    if (!w_conv0 || !w_conv_image || !w_conv_fused || !packed) return KBN_ERR_INVALID_ARGUMENT;
    if (!front_shape_ok(image_channels, conv0_filters, kb_filters)) return KBN_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    float* tab = static_cast<float*>(packed);
    if (hipMemsetAsync(tab, 0, FR_TAB * 4, st) != hipSuccess) return KBN_ERR_LAUNCH;
    hipLaunchKernelGGL(front_table_kernel, dim3(64, 3), dim3(256), 0, st, w_conv0, w_conv_image, w_conv_fused, tab, image_channels,
                       conv0_filters, kb_filters);
    _Float16* p0 = reinterpret_cast<_Float16*>(tab + FR_TAB);
    const int t0 = (int)front_w0_halves(conv0_filters);
    hipLaunchKernelGGL(front_pack0_kernel, dim3((t0 + 255) / 256), dim3(256), 0, st, w_conv0, tab, p0, image_channels, conv0_filters, t0);
    const int tc = (int)front_wc_halves(conv0_filters, kb_filters);
    hipLaunchKernelGGL(front_packc_kernel, dim3((tc + 255) / 256), dim3(256), 0, st, w_conv_image, w_conv_fused, tab, p0 + t0, conv0_filters,
                       kb_filters, tc);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_kb1_front_query(int image_channels, int conv0_filters, int kb_filters, int height, int width, float conv0_negative_slope) {
    using namespace kbn;
    if (height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    if (!front_shape_ok(image_channels, conv0_filters, kb_filters) || knob(KNOB_NO_SPLIT)) return KBN_ERR_UNSUPPORTED;
    if ((long long)height * width > 0x1fffffffLL) return KBN_ERR_UNSUPPORTED;
    if (!(conv0_negative_slope >= 0.f && conv0_negative_slope <= 1.f)) return KBN_ERR_UNSUPPORTED;   // LeakyReLU as max(t, slope t)
    return KBN_OK;
}

// ---- the next level's conv_fused inside the same launch (kb1_front_kernel<3, 3, true>) ----
static bool front_next_shape_ok(int ci, int cf, int fo) { return ci == 48 && cf == 48 && fo == 96; }
static size_t front_next_tab_floats(int fo) { return (size_t)fo * 4; }
static size_t front_next_halves(int ci, int cf, int fo) { return (size_t)((ci + cf) / 32) * 2 * 4 * fo * 8; }

size_t kbn_kb1_front_next_packed_weight_bytes(int image_channels, int fused_channels, int filters) {
    if (!front_next_shape_ok(image_channels, fused_channels, filters)) return 0;
    return front_next_tab_floats(filters) * 4 + 2 * front_next_halves(image_channels, fused_channels, filters);
}

int kbn_kb1_front_next_pack_weight(const float* w_conv_fused, void* packed, int image_channels, int fused_channels, int filters,
                                   kbn_stream_t stream) {
    using namespace kbn;
    if (!w_conv_fused || !packed) return KBN_ERR_INVALID_ARGUMENT;
    if (!front_next_shape_ok(image_channels, fused_channels, filters)) return KBN_ERR_UNSUPPORTED;
    float* tab2 = static_cast<float*>(packed);
    hipLaunchKernelGGL(front_next_pack_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, w_conv_fused, tab2,
                       reinterpret_cast<_Float16*>(tab2 + front_next_tab_floats(filters)), image_channels, fused_channels, filters,
                       (int)front_next_halves(image_channels, fused_channels, filters));
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_kb1_front_next_query(int image_channels, int conv0_filters, int kb_filters, int next_filters, int height, int width,
                             float conv0_negative_slope) {
    using namespace kbn;
    if (int rc = kbn_kb1_front_query(image_channels, conv0_filters, kb_filters, height, width, conv0_negative_slope)) return rc;
    if (!front_next_shape_ok(kb_filters, kb_filters, next_filters) || knob(KNOB_NO_FRONT_NEXT)) return KBN_ERR_UNSUPPORTED;
    return KBN_OK;
}

static int kb1_front_launch(const float* image, long long image_batch_stride, const void* packed_weight,
                            const float* xyz, long long xyz_batch_stride, float* out_image, long long out_image_batch_stride,
                            float* out_fused, long long out_fused_batch_stride, int n, int image_channels, int conv0_filters,
                            int kb_filters, int height, int width, float conv0_negative_slope, float kb_negative_slope,
                            unsigned* out_image_absmax, unsigned* out_fused_absmax, const void* packed_next, const float* xyz_next,
                            long long xyz_next_batch_stride, float* out_next, long long out_next_batch_stride, int next_filters,
                            float next_negative_slope, unsigned* out_next_absmax, kbn_stream_t stream) {
    using namespace kbn;
    if (!image || !packed_weight || !out_image || !out_fused || n < 1 || height < 1 || width < 1)
        return KBN_ERR_INVALID_ARGUMENT;
    if (int rc = kbn_kb1_front_query(image_channels, conv0_filters, kb_filters, height, width, conv0_negative_slope)) return rc;
    if (packed_next) {
        if (!xyz_next || !out_next) return KBN_ERR_INVALID_ARGUMENT;
        if (int rc = kbn_kb1_front_next_query(image_channels, conv0_filters, kb_filters, next_filters, height, width, conv0_negative_slope)) return rc;
    }
    FrontParams p{};
    p.image = image; p.image_bstride = image_batch_stride;
    p.tab = static_cast<const float*>(packed_weight);
    p.w0 = reinterpret_cast<const _Float16*>(p.tab + FR_TAB);
    p.wc = p.w0 + front_w0_halves(conv0_filters);
    p.xyz = xyz; p.xyz_bstride = xyz_batch_stride;
    p.out_image = out_image; p.out_image_bstride = out_image_batch_stride;
    p.out_fused = out_fused; p.out_fused_bstride = out_fused_batch_stride;
    p.amax_out_image = out_image_absmax; p.amax_out_fused = out_fused_absmax;
    p.N = n; p.Cin = image_channels; p.H = height; p.W = width;
    p.h = ceil_div(height, 2); p.w = ceil_div(width, 2);
    p.tilesX = ceil_div(p.w, FR_TW); p.tilesY = ceil_div(p.h, FR_TH);
    const long long tiles = (long long)p.tilesX * p.tilesY * n;
    if (tiles > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    p.ntiles = (int)tiles;
    p.slope0 = conv0_negative_slope; p.slope1 = kb_negative_slope;
    p.vec4 = !((p.w & 3) || (reinterpret_cast<uintptr_t>(out_image) & 15) || (reinterpret_cast<uintptr_t>(out_fused) & 15) ||
               (out_image_batch_stride & 3) || (out_fused_batch_stride & 3) || (reinterpret_cast<uintptr_t>(xyz) & 15) ||
               (xyz_batch_stride & 3)) ? 1 : 0;
    constexpr size_t lds = 2 * FR_NIN * 8 + 2 * 2 * FR_XP * 16 + (5 * 2 * 4 + 2 * 2) * 48 * 16;
    if (packed_next) {
        p.tab2 = static_cast<const float*>(packed_next);
        p.wn = reinterpret_cast<const _Float16*>(p.tab2 + front_next_tab_floats(next_filters));
        p.xyz2 = xyz_next; p.xyz2_bstride = xyz_next_batch_stride;
        p.out2 = out_next; p.out2_bstride = out_next_batch_stride;
        p.amax_out2 = out_next_absmax;
        p.h2 = ceil_div(p.h, 2); p.w2 = ceil_div(p.w, 2);
        p.slope2 = next_negative_slope;
        p.vec4_2 = !((p.w2 & 3) || (reinterpret_cast<uintptr_t>(out_next) & 15) || (out_next_batch_stride & 3) ||
                     (reinterpret_cast<uintptr_t>(xyz_next) & 15) || (xyz_next_batch_stride & 3)) ? 1 : 0;
    }
    const bool one_term = knob(KNOB_FP16_ONE_TERM) != 0;   // THROUGHPUT-ONLY: h1 w1 alone
    if (int rc = flag_dispatch([&](auto NEXT, auto ONE) {
            return launch_lds<kb1_front_kernel<3, 3, NEXT, ONE>, 80 * 1024>(p.ntiles, FR_THREADS, lds, (hipStream_t)stream, p);
        }, packed_next != nullptr, one_term))
        return rc;
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_kb1_front_forward(const float* image, long long image_batch_stride, const void* packed_weight,
                          const float* xyz, long long xyz_batch_stride, float* out_image, long long out_image_batch_stride,
                          float* out_fused, long long out_fused_batch_stride, int n, int image_channels, int conv0_filters,
                          int kb_filters, int height, int width, float conv0_negative_slope, float kb_negative_slope,
                          unsigned* out_image_absmax, unsigned* out_fused_absmax, kbn_stream_t stream) {
    return kb1_front_launch(image, image_batch_stride, packed_weight, xyz, xyz_batch_stride, out_image, out_image_batch_stride, out_fused,
                            out_fused_batch_stride, n, image_channels, conv0_filters, kb_filters, height, width, conv0_negative_slope,
                            kb_negative_slope, out_image_absmax, out_fused_absmax, nullptr, nullptr, 0, nullptr, 0, 0, 0.f, nullptr, stream);
}

int kbn_kb1_front_next_forward(const float* image, long long image_batch_stride, const void* packed_weight,
                               const float* xyz, long long xyz_batch_stride, float* out_image, long long out_image_batch_stride,
                               float* out_fused, long long out_fused_batch_stride, int n, int image_channels, int conv0_filters,
                               int kb_filters, int height, int width, float conv0_negative_slope, float kb_negative_slope,
                               unsigned* out_image_absmax, unsigned* out_fused_absmax, const void* packed_next, const float* xyz_next,
                               long long xyz_next_batch_stride, float* out_next_fused, long long out_next_fused_batch_stride, int next_filters,
                               float next_negative_slope, unsigned* out_next_fused_absmax, kbn_stream_t stream) {
    if (!packed_next) return KBN_ERR_INVALID_ARGUMENT;
    return kb1_front_launch(image, image_batch_stride, packed_weight, xyz, xyz_batch_stride, out_image, out_image_batch_stride, out_fused,
                            out_fused_batch_stride, n, image_channels, conv0_filters, kb_filters, height, width, conv0_negative_slope,
                            kb_negative_slope, out_image_absmax, out_fused_absmax, packed_next, xyz_next, xyz_next_batch_stride,
                            out_next_fused, out_next_fused_batch_stride, next_filters, next_negative_slope, out_next_fused_absmax, stream);
}

}  // extern "C"
