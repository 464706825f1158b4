
// conv1x1s2_split.hip -- 1x1 stride-2 conv (+ LeakyReLU) on split operands (the arithmetic: split_common.h): conv_fused of the KB block, reference src/net_utils.py:1337-1343 and
// :1366-1368 (cat[image, xyz, fused] -> Conv2d(kernel 1, stride 2)).  The tensor channels (image, fused: multiples of
// 16) go through the matrix core like the 3x3 kernels' -- one "tap", M = 32 output pixels of a row (input pixels
// (2y, 2x)), N = 32 filters, K = 16 channels -- the three backprojection channels K^-1 [x y 1]^T z, computed once per
// block by kb_xyz_s2_kernel, enter in fp32 in the epilogue (three FMAs per output).  Workgroup = 8 waves = 2 row groups
// x 4 filter groups (a wave: 4 rows x one 32-filter block), tile 8 rows x 32 pixels x 128 filters, main and small-term
// accumulators as in conv3x3_split_kernel.
// A chunk is only twelve MFMAs per wave, so the K loop is a short software pipeline: weights of chunk c+1 and inputs of
// chunk c+2 are issued at the top of chunk c (two register sets by chunk parity), the inputs of chunk c+1 are split and
// written to the other A buffer after the MFMAs of chunk c; one barrier per chunk; vmcnt waits count the loads in
// issue order (b(c) | inputs(c+1) | b(c+1) | inputs(c+2)).  Past the last chunk the fetches repeat the last chunk (never
// used) and the MFMAs are skipped: the vmcnt arithmetic is the same in every iteration and the kernel holds two copies
// of the body (seven tail variants spilled).  The loop is bound by memory latency, not by its MFMAs (a wave-private
// variant without LDS and barriers, every lane fetching its own fragment, measured 15 % slower: twice the loads).
#include "split_common.h"

namespace kbn {

template <int N, int NBX>
__device__ __forceinline__ void c1_wait_b(f32x4 (&b)[NBX][2]) {
    static_assert(NBX == 1, "one 32-filter block per wave (the 4 x 2 wave form with two was measured and removed)");
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(b[0][0]), "+v"(b[0][1]) : "n"(N));
}
template <int N>
__device__ __forceinline__ void c1_wait_a(float (&v)[8]) {
    asm volatile("s_waitcnt vmcnt(%8)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]) : "n"(N));
}

template <int RG, int NB, bool ONE = false>   // RG row groups x 8 / RG filter groups of waves; a wave: 8 / RG rows x NB 32-filter blocks (RG * NB = 4: 128 filters per tile); ONE: h1 w1 alone (throughput only)
__global__ __launch_bounds__(SP_THREADS, 1) void conv1x1s2_split_kernel(const SplitConvParams p) {
    constexpr int TH = 8, MB = TH / RG, NT = 128, NPIX = TH * SP_TW;
    static_assert(32 * NB * (8 / RG) == NT, "128 filters per workgroup");
    constexpr int A_PART = 2 * NPIX * 16, A_BYTES = 2 * A_PART;          // [part][k-group][pixel][8 fp16]
    constexpr int B_CHUNK = 2 * 2 * NT * 16;                             // bytes: [part][k-group][filter][8 fp16]
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 6, 2), 0");      // fp16 results flush subnormals (see conv3x3_split_kernel)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rg = wave % RG, fg = wave / RG;
    const int lm = lane & 31, g = lane >> 5;
    int bid = xcd_remap(blockIdx.x, p.nblocks);
    const int nt = bid % p.nTilesN;
    bid /= p.nTilesN;
    const int tx = bid % p.tilesX;
    bid /= p.tilesX;
    const int ty = bid % p.tilesY;
    const int n = bid / p.tilesY;
    const int oy0 = ty * TH, ox0 = tx * SP_TW;
    const int H = p.H, W = p.W, sH = p.sH, sW = p.sW;
    const long long plane = (long long)sH * sW;
    const int nchunks = p.Cin / SP_CK, last = nchunks - 1;
    float prescale, unscale;
    sp_act_scale(p, n, prescale, unscale);

    // staging: waves 0-3 take k-group 0 of a chunk, waves 4-7 k-group 1; one pixel per thread: output (r, c) reads input (2 r, 2 c)
    const int kg_st = wave >> 2, t256 = tid & 255;
    const int sy = 2 * (oy0 + (t256 >> 5)), sx = 2 * (ox0 + (t256 & 31));
    const int goff = (sy < sH && sx < sW) ? (sy * sW + sx) * 4 : -1;
    // a source that was written at the even pixels only (p.sub0: the stride-2 split conv's fp32 side output): same validity
    const int goff_sub = goff >= 0 ? ((sy >> 1) * W + (sx >> 1)) * 4 : -1;
    const long long plane_sub = (long long)H * W;
    const unsigned char* wp_nt = reinterpret_cast<const unsigned char*>(p.wp) + (long long)nt * nchunks * B_CHUNK;

    float va[2][8];
    auto load_chunk = [&](float (&v)[8], int chunk) {
        int c = chunk * SP_CK, s = 0;
        if (p.nsrc > 1 && c >= p.srcC[0]) { c -= p.srcC[0]; s = 1; }
        const bool sub = p.sub0 && s == 0;                 // launch- / wave-uniform
        const long long pl = sub ? plane_sub : plane;
        const float* base = p.src[s] + (long long)n * p.src_bstride[s] + (long long)(c + kg_st * 8) * pl;
        const int go = sub ? goff_sub : goff;
        const unsigned voff = go < 0 ? 0u : (unsigned)go;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float* sb = base + (long long)k * pl;   // wave-uniform
            asm volatile("global_load_dword %0, %1, %2" : "=v"(v[k]) : "v"(voff), "s"(sb) : "memory");
        }
    };
    auto store_chunk = [&](int buf, const float (&vin)[8]) {
        unsigned char* A = smem + buf * A_BYTES + kg_st * NPIX * 16;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = goff >= 0 ? vin[k] : 0.f;
        sph8 h1, h2;
        sp_split8(v, prescale, h1, h2);
        *reinterpret_cast<sph8*>(A + t256 * 16) = h1;
        *reinterpret_cast<sph8*>(A + A_PART + t256 * 16) = h2;
    };
    const unsigned boff = (unsigned)((g * NT + fg * 32 * NB + lm) * 16);
    auto load_b = [&](f32x4 (&b)[NB][2], int chunk) {
        const unsigned char* base = wp_nt + (long long)chunk * B_CHUNK;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const unsigned char* sb = base + (t * 2 * NT + nb * 32) * 16;   // wave-uniform
                asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(b[nb][t]) : "v"(boff), "s"(sb) : "memory");
            }
    };

    spf16 acc[MB][NB], lo[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc[mb][nb][i] = 0.f; lo[mb][nb][i] = 0.f; }

    const unsigned char* const aptr = smem + (g * NPIX + MB * rg * SP_TW + lm) * 16;
    f32x4 bq[2][NB][2];
    constexpr int NLB = 2 * NB, NLA = 8;   // loads per weight fetch / per input fetch
    auto body = [&](int c, auto par_tag) {   // PAR: parity of c (register sets, A buffer)
        constexpr int PAR = decltype(par_tag)::value;
        load_b(bq[PAR ^ 1], min(c + 1, last));
        load_chunk(va[PAR], min(c + 2, last));
        // outstanding, oldest first: b(c) | inputs(c+1) | b(c+1) | inputs(c+2)
        c1_wait_b<NLA + NLB + NLA>(bq[PAR]);
        if (c <= last) {
            sph8 bw[NB][2], a[MB][2];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                bw[nb][0] = __builtin_bit_cast(sph8, bq[PAR][nb][0]);
                bw[nb][1] = __builtin_bit_cast(sph8, bq[PAR][nb][1]);
            }
            const int abuf = PAR * A_BYTES;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int t = 0; t < 2; ++t) a[mb][t] = *reinterpret_cast<const sph8*>(aptr + abuf + t * A_PART + mb * SP_TW * 16);
            constexpr int TA[3] = {0, 0, 1}, TBP[3] = {0, 1, 0};   // h1 w1 | h1 (w2 2^11), h2 w1
#pragma unroll
            for (int t = 0; t < (ONE ? 1 : 3); ++t)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        spf16& d = t > 0 ? lo[mb][nb] : acc[mb][nb];
                        d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mb][TA[t]], bw[nb][TBP[t]], d, 0, 0, 0);
                    }
        }
        c1_wait_a<NLB + NLA>(va[PAR ^ 1]);   // inputs of chunk c+1 (fetched a chunk and a half ago)
        store_chunk(PAR ^ 1, va[PAR ^ 1]);
        __syncthreads();
    };

    load_chunk(va[0], 0);
    c1_wait_a<0>(va[0]);
    store_chunk(0, va[0]);
    load_b(bq[0], 0);
    load_chunk(va[1], min(1, last));
    __syncthreads();
    for (int c = 0; c < nchunks; c += 2) {
        body(c, std::integral_constant<int, 0>{});
        body(c + 1, std::integral_constant<int, 1>{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the repeated fetches of the last iterations land before their registers are reused

    // ---- epilogue: acc[mb][nb][i]: pixel x = 8 (i / 4) + 4 g + (i % 4) of row MB rg + mb, filter fg * 64 + nb * 32 + lm
    const long long oplane = (long long)H * W;
    float* outn = p.out + (long long)n * p.out_bstride;
    const float* xyzn = p.xyz ? p.xyz + (long long)n * p.xyz_bstride : nullptr;
    const float slope = p.act ? p.slope : 1.f;
    const bool vec4 = p.vec4 != 0;
    float amax = 0.f;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int oc = nt * NT + fg * 32 * NB + nb * 32 + lm;
        const float inv = p.inv_scale[oc] * unscale;               // 2^-e 2^-k; the table is padded to whole n-tiles
        if (oc >= p.OC) continue;
        float wx[3] = {0.f, 0.f, 0.f};
        if (xyzn) { wx[0] = p.wxyz[oc * 3]; wx[1] = p.wxyz[oc * 3 + 1]; wx[2] = p.wxyz[oc * 3 + 2]; }
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int Y = oy0 + MB * rg + mb;
            if (Y >= H) continue;
            float* o = outn + (long long)oc * oplane + (long long)Y * W + ox0 + 4 * g;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int X = ox0 + 8 * q4 + 4 * g;
                if (X >= W) continue;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float t = __builtin_fmaf(lo[mb][nb][q4 * 4 + j], 0.00048828125f, acc[mb][nb][q4 * 4 + j]) * inv;
                    if (xyzn && X + j < W) {
                        const float* xp = xyzn + (long long)Y * W + X + j;
                        t += wx[0] * xp[0] + wx[1] * xp[oplane] + wx[2] * xp[2 * oplane];
                    }
                    v[j] = t > 0.f ? t : t * slope;
                }
                if (vec4) {
                    *reinterpret_cast<f32x4*>(o + 8 * q4) = v;
                    amax = sp_amax4(amax, v);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (X + j < W) { o[8 * q4 + j] = v[j]; amax = fmaxf(amax, fin_abs(v[j])); }
                }
            }
        }
    }
    if (p.out_amax) absmax_commit(p.out_amax + n, amax);
}

// the KB block's backprojection at the positions its stride-2 1x1 conv reads: xyz[:, j, y, x] = (K^-1 [2x 2y 1]^T)_j z,
// z = act(proj_weight . depth[:, 2y, 2x]) (reference src/net_utils.py:1352-1359; the same expressions as the in-kernel
// synthesis of the fp32 conv kernels, conv_dma_impl.h)
__global__ void kb_xyz_s2_kernel(const float* __restrict__ depth, long long dbs, int Cd, int H, int W, const float* __restrict__ proj,
                                 const float* __restrict__ kinv, int act, float slope, float* __restrict__ xyz, long long xbs,
                                 int oh, int ow) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    if (idx >= oh * ow) return;
    const int oy = idx / ow, ox = idx - oy * ow;
    const int Y = 2 * oy, X = 2 * ox;
    const long long HW = (long long)H * W;
    const float* db = depth + (long long)n * dbs + (long long)Y * W + X;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int c = 0;
    for (; c + 3 < Cd; c += 4) {
        a0 = fmaf(proj[c], db[(long long)c * HW], a0);
        a1 = fmaf(proj[c + 1], db[(long long)(c + 1) * HW], a1);
        a2 = fmaf(proj[c + 2], db[(long long)(c + 2) * HW], a2);
        a3 = fmaf(proj[c + 3], db[(long long)(c + 3) * HW], a3);
    }
    for (; c < Cd; ++c) a0 = fmaf(proj[c], db[(long long)c * HW], a0);
    const float a = (a0 + a1) + (a2 + a3);
    const float z = act ? leaky_relu(a, slope) : a;
    const float* ki = kinv + (long long)n * 9;
    float* o = xyz + (long long)n * xbs + idx;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        o[(long long)j * oh * ow] = (fmaf(ki[j * 3 + 1], (float)Y, ki[j * 3 + 0] * (float)X) + ki[j * 3 + 2]) * z;
}

__global__ void copy_wxyz_kernel(const float* __restrict__ w, float* __restrict__ wxyz, int OC, int cin_total, int xyz_offset) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < OC * 3) wxyz[e] = w[(long long)(e / 3) * cin_total + xyz_offset + e % 3];
}

}  // namespace kbn

extern "C" {

// blob: [inv_scale: tiles x 128 floats][fp16 panel: tiles x (cin / 16) x 8 KiB][wxyz: out_channels x 3 floats, if any]
static size_t c1_panel_bytes(int out_channels, int cin) {
    return (size_t)kbn::ceil_div(out_channels, 128) * (128 * 4 + (size_t)(cin / kbn::SP_CK) * (2 * 2 * 128 * 16));
}

size_t kbn_conv1x1s2_split_packed_weight_bytes(int out_channels, int tensor_channels, int has_xyz) {
    if (out_channels < 1 || tensor_channels < 1 || (tensor_channels % kbn::SP_CK) != 0) return 0;
    if (!kbn::layer_shape_ok(out_channels, tensor_channels, 1)) return 0;
    return c1_panel_bytes(out_channels, tensor_channels) + (has_xyz ? (size_t)out_channels * 3 * 4 : 0);
}

int kbn_conv1x1s2_split_pack_weight(const float* weight, void* packed, int out_channels, int in_channels, int xyz_offset,
                                    kbn_stream_t stream) {
    using namespace kbn;
    const bool has_xyz = xyz_offset >= 0;
    const int cin = in_channels - (has_xyz ? 3 : 0);
    if (!weight || !packed || (has_xyz && xyz_offset > cin) || kbn_conv1x1s2_split_packed_weight_bytes(out_channels, cin, has_xyz) == 0)
        return KBN_ERR_INVALID_ARGUMENT;
    const int ocpad = ceil_div(out_channels, 128) * 128;
    float* inv = static_cast<float*>(packed);
    _Float16* wp = reinterpret_cast<_Float16*>(inv + ocpad);
    const long long total = (long long)((c1_panel_bytes(out_channels, cin) - (size_t)ocpad * 4) / 2);
    // per-filter exponent over ALL input channels of the filter (the three fp32 ones can only make it more cautious)
    split_pack_launch(weight, inv, wp, out_channels, in_channels, cin, 128, total, 1, has_xyz ? xyz_offset : cin, has_xyz ? 3 : 0,
                      (hipStream_t)stream);
    if (has_xyz) {
        float* wxyz = reinterpret_cast<float*>(static_cast<unsigned char*>(packed) + c1_panel_bytes(out_channels, cin));
        hipLaunchKernelGGL(copy_wxyz_kernel, dim3(ceil_div(out_channels * 3, 256)), dim3(256), 0, (hipStream_t)stream, weight, wxyz,
                           out_channels, in_channels, xyz_offset);
    }
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_conv1x1s2_split_forward(const kbn_conv_src* srcs, int n_src, const void* packed_weight, const float* xyz,
                                long long xyz_batch_stride, float* out, long long out_batch_stride, int n, int out_channels,
                                int height, int width, int act_exponent, int apply_activation, float negative_slope,
                                unsigned* out_absmax, kbn_stream_t stream) {
    using namespace kbn;
    if (act_exponent < -60 || act_exponent > 60) return KBN_ERR_INVALID_ARGUMENT;
    if (!srcs || n_src < 1 || n_src > 2 || !packed_weight || !out || n < 1 || out_channels < 1 || height < 1 || width < 1)
        return KBN_ERR_INVALID_ARGUMENT;
    if (knob(KNOB_NO_SPLIT)) return KBN_ERR_UNSUPPORTED;
    SplitConvParams p{};
    int cin = 0;
    for (int s = 0; s < n_src; ++s) {
        const kbn_conv_src& a = srcs[s];
        if (a.kind != KBN_SRC_TENSOR || !a.data || a.channels < 1 || (a.channels % SP_CK) != 0) return KBN_ERR_UNSUPPORTED;
        // with two sources, source 0 may come pre-subsampled: height x width planes holding the pixels (2y, 2x) of the tensor
        // the reference's conv reads (the fp32 side output of kbn_conv3x3_split_forward(mode 2, pair_out))
        const bool sub = s == 0 && n_src == 2 && a.src_height == height && a.src_width == width &&
                         (srcs[1].src_height != height || srcs[1].src_width != width);
        if (sub) p.sub0 = 1;
        else {
            if (!p.sH) { p.sH = a.src_height; p.sW = a.src_width; }
            if (a.src_height != p.sH || a.src_width != p.sW) return KBN_ERR_INVALID_ARGUMENT;
        }
        p.src[s] = a.data; p.src_bstride[s] = a.batch_stride; p.srcC[s] = a.channels;
        cin += a.channels;
    }
    if (ceil_div(p.sH, 2) != height || ceil_div(p.sW, 2) != width) return KBN_ERR_INVALID_ARGUMENT;
    if ((long long)p.sH * p.sW > 0x1fffffffLL) return KBN_ERR_UNSUPPORTED;
    if (n_src == 1) { p.src[1] = p.src[0]; p.src_bstride[1] = p.src_bstride[0]; p.srcC[1] = 0; }
    p.nsrc = n_src;
    // the exponent follows the data when EVERY source brings its slots; otherwise the static act_exponent serves
    if (srcs[0].absmax && (n_src == 1 || srcs[1].absmax)) { p.amax[0] = srcs[0].absmax; p.amax[1] = n_src > 1 ? srcs[1].absmax : nullptr; }
    p.out_amax = out_absmax;
    if (!layer_shape_ok(out_channels, cin, 1)) return KBN_ERR_UNSUPPORTED;   // the shapes the blob's size function answers 0 for
    p.nTilesN = ceil_div(out_channels, 128);
    p.inv_scale = static_cast<const float*>(packed_weight);
    p.wp = reinterpret_cast<const _Float16*>(p.inv_scale + p.nTilesN * 128);
    p.xyz = xyz; p.xyz_bstride = xyz_batch_stride;
    p.wxyz = xyz ? reinterpret_cast<const float*>(static_cast<const unsigned char*>(packed_weight) + c1_panel_bytes(out_channels, cin)) : nullptr;
    p.out = out; p.out_bstride = out_batch_stride;
    p.N = n; p.OC = out_channels; p.Cin = cin; p.H = height; p.W = width;
    p.tilesX = ceil_div(width, SP_TW); p.tilesY = ceil_div(height, 8);
    const long long blocks = (long long)p.tilesX * p.tilesY * n * p.nTilesN;
    if (blocks > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    p.nblocks = (int)blocks;
    p.act = apply_activation ? 1 : 0; p.slope = negative_slope;
    p.prescale = ldexpf(1.f, act_exponent); p.unscale = ldexpf(1.f, -act_exponent);
    p.vec4 = !((width & 3) || (reinterpret_cast<uintptr_t>(out) & 15) || (out_batch_stride & 3)) ? 1 : 0;
    // 2 row groups x 4 filter groups (a wave: 4 rows x one 32-filter block): every weight fragment is fetched by two waves
    // instead of four (the 4 x 2 form, measured against it, is no longer built)
    if (knob(KNOB_FP16_ONE_TERM))   // THROUGHPUT-ONLY: h1 w1 alone
        hipLaunchKernelGGL((conv1x1s2_split_kernel<2, 1, true>), dim3(p.nblocks), dim3(SP_THREADS), 2 * 2 * 2 * 256 * 16, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((conv1x1s2_split_kernel<2, 1>), dim3(p.nblocks), dim3(SP_THREADS), 2 * 2 * 2 * 256 * 16, (hipStream_t)stream, p);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_kb_xyz_s2_forward(const float* depth, long long depth_batch_stride, int depth_channels, int height, int width,
                          const float* proj_weight, const float* kinv, int apply_activation, float negative_slope, float* xyz,
                          long long xyz_batch_stride, int n, kbn_stream_t stream) {
    using namespace kbn;
    if (!depth || !proj_weight || !kinv || !xyz || n < 1 || depth_channels < 1 || height < 1 || width < 1) return KBN_ERR_INVALID_ARGUMENT;
    const int oh = ceil_div(height, 2), ow = ceil_div(width, 2);
    hipLaunchKernelGGL(kb_xyz_s2_kernel, dim3(ceil_div(oh * ow, 256), n), dim3(256), 0, (hipStream_t)stream, depth, depth_batch_stride,
                       depth_channels, height, width, proj_weight, kinv, apply_activation ? 1 : 0, negative_slope, xyz,
                       xyz_batch_stride, oh, ow);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

}  // extern "C"
