// The body of upconv2x_split64_kernel (csrc/upconv_split.hip), included once per tile form: in scope are the kernel's template
// parameters PIN / POUT, `p`, `smem`, the compile-time `TP` and the tile's `block`, `nblocks`, `tilesX`, `tilesY`.
    // TP: transposed tiles for a narrow last tile column (see conv3x3_split_kernel): 16 low-resolution rows x 16 columns, a wave's
    // 32-pixel block = rows 2 rg, 2 rg + 1 x 16 pixels, the staged region 18 x 18 pixels in a buffer sized for the 10 x 34 of the
    // whole tiles (NPIX: the layout; NPIXL: the pixels staged)
    constexpr int TH = TP ? 16 : 8, COLS = TP ? 18 : 34, NPIX = 10 * 34, NPIXL = TP ? 18 * 18 : NPIX, NB = 2;
    constexpr int A_PART = 2 * NPIX * 16, A_BYTES = 2 * A_PART, PR = (NPIX + 255) / 256;
    constexpr int B_ITEM = 2 * 2 * U64_NT * 16, HALF = UF_ITEMS / 2, B_HALF = HALF * B_ITEM;   // bytes per weight set / half chunk
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 6, 2), 0");   // fp16 results flush subnormals (see conv3x3_split_kernel)
    const int tid = threadIdx.x, lane = tid & 63;
    const int rg = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave = low-resolution row oy0 + rg (transposed: rows oy0 + 2 rg, + 1)
    const int lm = lane & 31, g = lane >> 5;
    int bid = xcd_remap(block, nblocks);
    int ks = 0;   // KSPLIT: see conv_split_body.inc
    if constexpr (KSPLIT) { ks = bid % p.ksplit; bid /= p.ksplit; }
    const int nt = bid % p.nTilesN;
    bid /= p.nTilesN;
    const int tx = bid % tilesX;
    bid /= tilesX;
    const int ty = bid % tilesY;
    const int n = bid / tilesY;
    const int oy0 = ty * TH, ox0 = TP ? p.tp_x0 : tx * 32;             // low-resolution tile origin
    const int H = p.H, W = p.W, sH = p.sH, sW = p.sW;
    const long long plane = (long long)sH * sW;
    const int nchunks = p.Cin / SP_CK;
    int c_lo = 0, c_hi = nchunks;
    if constexpr (KSPLIT) {
        static_assert(!PIN && !POUT && !TP, "the split-K form: an fp32 source in, partial fp32 sums out, whole tiles");
        const int per = (nchunks + p.ksplit - 1) / p.ksplit;
        c_lo = ks * per;
        c_hi = min(nchunks, c_lo + per);
    }
    float prescale, unscale;
    if constexpr (PIN) { prescale = 0.f; unscale = 1.f / p.pair_src_scale[n]; }
    else sp_act_scale(p, n, prescale, unscale);

    const int kg_st = rg >> 2, t256 = tid & 255;
    int goff[PR];
#pragma unroll
    for (int u = 0; u < PR; ++u) {
        const int pix = u * 256 + t256;
        const int r = pix / COLS, c = pix - r * COLS;
        const int Y = oy0 - 1 + r, X = ox0 - 1 + c;
        goff[u] = (pix < NPIXL && Y >= 0 && Y < sH && X >= 0 && X < sW) ? (Y * sW + X) * 4 : -1;
    }
    const unsigned char* wp_nt = reinterpret_cast<const unsigned char*>(p.wp) + (long long)nt * nchunks * (UF_ITEMS * B_ITEM);

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
        if (pix < NPIXL) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = goff[u] >= 0 ? va[u][k] : 0.f;
            sph8 h1, h2;
            sp_split8(v, prescale, h1, h2);
            *reinterpret_cast<sph8*>(A + pix * 16) = h1;
            if (!ONE) *reinterpret_cast<sph8*>(A + A_PART + pix * 16) = h2;
        }
    };
    // weights: half chunks (eight sets, 32 KiB) by LDS-DMA into two buffers behind the A buffers
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr(reinterpret_cast<const float*>(smem)));
    // pair input: a staged chunk is 4 planes (term, k-group) x NPIX granules; wave-wide DMA id = plane * NR + round, wave rg
    // issues ids rg, rg + 8, ..; a halo pixel outside the map reads the plane's zero granule
    constexpr int NR = (NPIXL + 63) / 64, NDMA = 4 * NR, DPW = NDMA / 8;
    static_assert(NDMA % 8 == 0, "the same number of DMAs in every wave");
    unsigned dvoff[DPW];
    if constexpr (PIN) {
#pragma unroll
        for (int i = 0; i < DPW; ++i) {
            const int pix = ((rg + 8 * i) % NR) * 64 + lane;
            const int r = pix / COLS, c = pix - r * COLS;
            const int Y = oy0 - 1 + r, X = ox0 - 1 + c;
            dvoff[i] = (pix < NPIXL && Y >= 0 && Y < sH && X >= 0 && X < sW) ? (unsigned)(Y * sW + X) * 16u : (unsigned)(sH * sW) * 16u;
        }
    }
    const long long pplane = pair_plane_halves(sH, sW);
    auto dma_chunk = [&](int buf, int chunk) {
        const _Float16* pn = p.pair_src + (long long)n * p.pair_src_bstride + (long long)(2 * chunk) * 2 * pplane;
#pragma unroll
        for (int i = 0; i < DPW; ++i) {
            const int id = rg + 8 * i, plane = id / NR, j = id - plane * NR;
            const int t = plane >> 1, kgl = plane & 1;
            if (ONE && t == 1) continue;   // wave-uniform; the h2 planes are not read (every wait of this kernel is vmcnt(0))
            const unsigned long long mask = (j == NR - 1 && (NPIXL & 63)) ? ((1ull << (NPIXL & 63)) - 1) : ~0ull;
            lds_dma16_sm(reinterpret_cast<const float*>(pn + (long long)(kgl * 2 + t) * pplane), dvoff[i],
                         lds0 + (unsigned)(buf * A_BYTES + t * A_PART + (kgl * NPIX + j * 64) * 16), mask);
        }
    };
    auto stage_half = [&](int hbuf, int chunk, int half) {
        const float* src = reinterpret_cast<const float*>(wp_nt + ((long long)chunk * UF_ITEMS + half * HALF) * B_ITEM);
        const unsigned dst = lds0 + (unsigned)(2 * A_BYTES + hbuf * B_HALF);
        constexpr int n4 = B_HALF / 16;
        static_assert(n4 % SP_THREADS == 0, "whole rounds of the workgroup");
#pragma unroll
        for (int e0 = 0; e0 < n4; e0 += SP_THREADS) {
            const int eb = e0 + rg * 64;
            lds_dma16_s(src + eb * 4, (unsigned)(lane * 16), dst + eb * 16);
        }
    };

    spf16 acc[2][2][NB];   // [py][px][32-filter block]
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a >> 2][(a >> 1) & 1][a & 1][i] = 0.f;

    const unsigned char* const aptr = TP ? smem + (g * NPIX + (2 * rg + (lm >> 4)) * COLS + (lm & 15)) * 16
                                         : smem + (g * NPIX + rg * COLS + lm) * 16;
    sph8 af[3][2];        // A fragments of staged rows rg + 0..2 at the column offset of their group (two split terms each)
    auto load_arow = [&](int abuf, int ry, int ox) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
            af[ry][t] = *reinterpret_cast<const sph8*>(aptr + abuf + t * A_PART + (ry * COLS + ox) * 16);
    };
    const unsigned char* const bptr = smem + 2 * A_BYTES + (g * U64_NT + lm) * 16;   // + part * 2 NT 16 + nb * 32 * 16
    const bool row_live = oy0 + (TP ? 2 : 1) * rg < sH;                             // wave-uniform
    constexpr int WAIT_IT = 4;   // set of the first half whose MFMAs follow the wait for the next chunk's inputs (and the second half's weights)
    static_assert(WAIT_IT + PR <= HALF, "the staging rounds sit in the first half");

    auto half_body = [&](int c, auto half_tag, auto more_tag) {
        constexpr int HF = decltype(half_tag)::value;
        constexpr bool MORE = decltype(more_tag)::value;   // a chunk c+1 exists
        const int abuf = (c & 1) * A_BYTES;
        const unsigned char* B = bptr + HF * B_HALF;
        // the other weight buffer was last read in the previous half (a barrier ago): refill it
        if (HF == 0) {
            stage_half(1, c, 1);
            if (MORE) {
                if constexpr (PIN) dma_chunk((c & 1) ^ 1, c + 1);   // the other buffer was last read a chunk (two barriers) ago
                else load_chunk(c + 1);
            }
            load_arow(abuf, 0, 0);
        } else if (MORE) {
            stage_half(0, c + 1, 0);
        }
        sph8 bwq[2][NB][2];   // (w1, w2) of the current / next set, per 32-filter block
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int t = 0; t < 2; ++t) bwq[0][nb][t] = *reinterpret_cast<const sph8*>(B + (t * 2 * U64_NT + nb * 32) * 16);
#pragma unroll
        for (int ih = 0; ih < HALF; ++ih) {
            constexpr int dummy = 0; (void)dummy;
            const int it = HF * HALF + ih;
            const UfItem t = uf_item(it);
            const bool first_of_group = it == 0 || uf_item(it - 1).s != t.s || uf_item(it - 1).ox != t.ox;
            if (first_of_group) {   // fetch the row the NEXT group reads
                if (t.s < 2) load_arow(abuf, t.s + 1, t.ox);
                else if (t.ox < 2) load_arow(abuf, 0, t.ox + 1);
            }
            if (ih + 1 < HALF) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt)
                        bwq[(ih + 1) & 1][nb][tt] = *reinterpret_cast<const sph8*>(B + (ih + 1) * B_ITEM + (tt * 2 * U64_NT + nb * 32) * 16);
            }
            sph8 bw[NB][3];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                bw[nb][0] = bwq[ih & 1][nb][0];
                bw[nb][1] = bwq[ih & 1][nb][1];
                bw[nb][2] = bw[nb][0] * (_Float16)0.00048828125f;   // w1 2^-11
            }
            if (!PIN && HF == 0 && MORE && ih == WAIT_IT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // next chunk's inputs (and this chunk's second half of weights)
            __builtin_amdgcn_sched_barrier(0);
            if (row_live) {
                constexpr int TA[3] = {0, 0, 1};
                constexpr int NTERM = ONE ? 1 : 3;   // ONE (throughput-only fp16 leg): h1 w1 alone
#pragma unroll
                for (int k = 0; k < NTERM; ++k)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        acc[t.py][t.px][nb] = POUT ? __builtin_amdgcn_mfma_f32_32x32x16_f16(bw[nb][k], af[t.s][TA[k]], acc[t.py][t.px][nb], 0, 0, 0)
                                                   : __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t.s][TA[k]], bw[nb][k], acc[t.py][t.px][nb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (!PIN && HF == 0 && MORE && ih >= WAIT_IT && ih - WAIT_IT < PR) store_round((c & 1) ^ 1, ih - WAIT_IT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the weight DMA issued at the top of the half
        __syncthreads();
    };

    if constexpr (PIN) dma_chunk(0, 0);
    else load_chunk(c_lo);
    stage_half(0, c_lo, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (!PIN) {
#pragma unroll
        for (int u = 0; u < PR; ++u) store_round(c_lo & 1, u);
    }
    __syncthreads();
    for (int c = c_lo; c + 1 < c_hi; ++c) {
        half_body(c, std::integral_constant<int, 0>{}, std::true_type{});
        half_body(c, std::integral_constant<int, 1>{}, std::true_type{});
    }
    half_body(c_hi - 1, std::integral_constant<int, 0>{}, std::false_type{});
    half_body(c_hi - 1, std::integral_constant<int, 1>{}, std::false_type{});

    const float slope = (p.act && !KSPLIT) ? p.slope : 1.f;
    float amax = 0.f;
    if constexpr (POUT) {
        // ---- pair epilogue: acc[py][px][nb][i]: low-resolution x = lm, filter nb * 32 + 8 (i / 4) + 4 g + (i % 4): a lane holds
        // channels 4 g .. 4 g + 3 of k-group (nt 64 + nb 32) / 8 + i / 4 -- half a granule -- of outputs (2 Y + py, 2 x + px)
        const float ps_out = sp_pair_out_scale(p, n);
        const long long oph = pair_plane_halves(H, W);
        _Float16* const pn = p.pair_out + (long long)n * p.pair_out_bstride;
        if (tid == 0) p.pair_out_scale[n] = ps_out;
        if (tx == 0 && ty == 0 && rg == 0 && lane < 16) {   // the zero granules of this filter tile's 8 k-groups x 2 terms
            const int kgz = nt * (U64_NT / 8) + (lane >> 1);
            if (kgz * 8 < p.OC)
                *reinterpret_cast<f32x4*>(pn + (long long)(kgz * 2 + (lane & 1)) * oph + (long long)H * W * 8) = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const int Yb = oy0 + (TP ? 2 : 1) * rg;
        if (Yb >= sH) return;   // wave-uniform
        const int Y = TP ? Yb + (lm >> 4) : Yb, x = TP ? ox0 + (lm & 15) : ox0 + lm;
        const bool live = x < sW && Y < sH;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {     // k-groups 2 qp, 2 qp + 1 of the block: after the exchange this lane stores k-group 2 qp + g whole
                const int kg0 = nt * (U64_NT / 8) + nb * 4 + 2 * qp;
                if (kg0 * 8 >= p.OC) continue;   // wave-uniform; pair outputs have whole k-groups (OC % 8 == 0)
                const f32x4 invA = *reinterpret_cast<const f32x4*>(p.inv_scale + kg0 * 8 + 4 * g) * unscale;
                const f32x4 invB = *reinterpret_cast<const f32x4*>(p.inv_scale + kg0 * 8 + 8 + 4 * g) * unscale;   // the table is padded to whole tiles
                const bool mine = (kg0 + g) * 8 < p.OC;
                _Float16* const k0 = pn + (long long)((kg0 + g) * 2) * oph;
#pragma unroll
                for (int py = 0; py < 2; ++py)
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        f32x4 va, vb;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float ta = acc[py][px][nb][qp * 8 + j] * invA[j];
                            const float tb = acc[py][px][nb][qp * 8 + 4 + j] * invB[j];
                            va[j] = ta > 0.f ? ta : ta * slope;
                            vb[j] = tb > 0.f ? tb : tb * slope;
                        }
                        if (live) amax = sp_amax4(sp_amax4(amax, va), vb);
                        sph4 a1, a2, b1, b2;
                        sp_split4(va * ps_out, a1, a2);
                        sp_split4(vb * ps_out, b1, b2);
                        const spu4 g1 = sp_pair_exchange(a1, b1), g2 = sp_pair_exchange(a2, b2);   // every lane takes part
                        if (live && mine) {
                            const long long o = ((long long)(2 * Y + py) * W + 2 * x + px) * 8;
                            *reinterpret_cast<spu4*>(k0 + o) = g1;
                            *reinterpret_cast<spu4*>(k0 + oph + o) = g2;
                        }
                    }
            }
        if (p.out_amax) absmax_commit(p.out_amax + n, amax);
        return;
    }
    // ---- epilogue: acc[py][px][nb][i]: low-resolution x = 8 (i / 4) + 4 g + (i % 4), filter nb * 32 + lm; outputs (2 Y + py, 2 x + px)
    // (transposed tiles: pixel index 8 (i / 4) + 4 g + (i % 4) of the block = row index >> 4, column index & 15)
    const long long oplane = (long long)H * W;
    const int Yb = oy0 + (TP ? 2 : 1) * rg;
    if (Yb >= sH) return;   // wave-uniform: a wave whose row(s) lie below the map stores nothing
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int oc = nt * U64_NT + nb * 32 + lm;
        const float inv = p.inv_scale[oc] * unscale;
        if (oc >= p.OC) continue;
        float* outc = p.out + (long long)n * p.out_bstride + (long long)oc * oplane + (KSPLIT ? (long long)ks * p.ks_stride : 0);
#pragma unroll
        for (int py = 0; py < 2; ++py) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int Y = TP ? Yb + (q4 >> 1) : Yb;
                if (Y >= sH) continue;
                float* orow = outc + (long long)(2 * Y + py) * W;
                const int X = TP ? 2 * (ox0 + 8 * (q4 & 1) + 4 * g) : 2 * (ox0 + 8 * q4 + 4 * g);   // first output column of this lane's 8
                f32x4 v0, v1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a = acc[py][j & 1][nb][q4 * 4 + (j >> 1)] * inv;
                    const float b = acc[py][j & 1][nb][q4 * 4 + 2 + (j >> 1)] * inv;
                    v0[j] = a > 0.f ? a : a * slope;
                    v1[j] = b > 0.f ? b : b * slope;
                }
                if (X < W) { *reinterpret_cast<f32x4*>(orow + X) = v0; amax = sp_amax4(amax, v0); }
                if (X + 4 < W) { *reinterpret_cast<f32x4*>(orow + X + 4) = v1; amax = sp_amax4(amax, v1); }
            }
        }
    }
    if (!KSPLIT && p.out_amax) absmax_commit(p.out_amax + n, amax);
