// split_common.h -- what the split-operand kernels share: fp32 products on the 16-bit matrix core (operands split in two
// fp16 terms), the launch parameters, the device helpers of the split and of the PAIR tensor format, and the launch helpers.
// The kernels: conv_split.hip (3x3 concat and stride-2 convs, split-K, absmax pass), upconv_split.hip (the folded 2x
// up-convs), conv1x1s2_split.hip (conv_fused of the KB block).
//
// gfx950 runs v_mfma_f32_*_f32 on the fp32 VECTOR datapath (157 TFLOP/s, issue shared with every other vector
// instruction: tools/probe/valu_probe.hip); the matrix core proper takes 16-bit and narrower operands (2.5 PFLOP/s dense)
// and runs beside the vector ALU (tools/probe/bf16x_probe.hip: an MFMA wave keeps 32 clk per MFMA with a v_fma wave on
// the same SIMD).  These kernels feed it fp32 operands as pairs of fp16 values:
//     activation  a 2^k    = h1 + 2^-11 h2,   h1 = fp16(a 2^k),   h2 = fp16((a 2^k - h1) 2^11)       (22+ bits of a)
//     weight      w 2^e    = w1 + w2,         w1 = fp16(w 2^e),   w2 = fp16(w 2^e - w1)              (22+ bits of w)
//     a w 2^(e+k) = h1 w1 + h1 w2 + h2 (w1 2^-11)   (+ h2 w2 2^-11, below 2^-22 |a w|, dropped)
//                 = h1 w1 + 2^-11 (h1 (w2 2^11) + h2 w1): the 3x3 kernels keep w2 scaled by 2^11 as well (normal in fp16
//                   down to |w2| = 2^-25) and sum the two small terms, both 2^11 times their share, in an accumulator of
//                   their own that enters the result once, in the epilogue -- no per-tap scaling of w1 in the K loop
// THREE fp16 MFMAs with fp32 accumulation per product, 3/16 of the fp32 MFMA's time.  The residual h2 is kept SCALED by
// 2^11 so that it sits in fp16's normal range whenever h1 does (the matrix core flushes fp16 subnormals); e is chosen
// per filter at pack time (largest |w 2^e| in [2^12, 2^13)); k (`act_exponent`) is the caller's: it places the fp16
// window on the layer's activations -- |a| 2^k up to 65504 is finite, |a| 2^k >= 2^-14 has the full 22 bits, smaller
// activations (h1 subnormal -> flushed, the mode register is set so) are carried by h2 alone with 11 bits.  There is
// no calibration and no state: every producer folds max |out| per frame into a device-side slot (kbn_conv_src.absmax,
// ops.ActStats) and the consumer derives k = 14 - floor(log2 max) per frame inside the forward (sp_act_scale below: the
// frame's maximum lands in [2^14, 2^15) of the window); a source without a slot takes the ABI default -6, which covers
// 0.0039 .. 4.2e6.  Measured against an fp64 evaluation (profiles/r02/bf16x_probe.txt, K = 576 .. 6912): rms error 0.28e-6 .. 0.9e-6
// of the output's rms, the fp32 MFMA chain (== fmaf chain) 0.44e-6 .. 1.7e-6 -- the accuracy class of the fp32 path, which
// is why these kernels sit on the parity-gated path (tests/test_hip_parity.py holds it to the same 1e-4 bar).

#pragma once
#include "conv_common.h"

#include <type_traits>

// 1: tiles without padding (no output rows below the map, no 32-filter blocks past the last filter) run a K loop whose
// MFMAs carry no tests at all; only the other tiles take the loop with a wave-uniform test in front of every MFMA (which
// puts each MFMA in a basic block of its own).  0: every tile takes the tested loop (A/B builds).
#ifndef KBN_SPLIT_STRAIGHT
#define KBN_SPLIT_STRAIGHT 1
#endif

namespace kbn {

typedef _Float16 sph8 __attribute__((ext_vector_type(8)));
typedef _Float16 sph2 __attribute__((ext_vector_type(2)));
typedef float spf16 __attribute__((ext_vector_type(16)));
typedef float spf4 __attribute__((ext_vector_type(4)));
typedef _Float16 sph4 __attribute__((ext_vector_type(4)));

constexpr int SP_TW = 32, SP_CK = 16, SP_TH = 16, SP_THREADS = 512;
constexpr int SP_WEXP = 13;                // largest |w 2^e| of a filter in [2^12, 2^13)

template <int MODE>   // conv3x3_split_kernel: 0 plain 3x3, 2 stride-2 conv
struct SpGeom {
    static constexpr bool S2 = MODE == 2;
    static constexpr int TH = S2 ? 8 : SP_TH;                            // output rows per workgroup
    static constexpr int ROWS = S2 ? 2 * TH + 1 : TH + 2;
    static constexpr int COLS = S2 ? 2 * SP_TW + 1 : SP_TW + 2, NPIX = ROWS * COLS;
    static constexpr int A_PART = 2 * NPIX * 16, A_BYTES = 2 * A_PART;   // [part][k-group][pixel][8 fp16]
    static constexpr int LDS = 2 * A_BYTES;
    static constexpr int PR = (NPIX + 255) / 256;                        // staging rounds of a 256-thread half (one k-group each)
    static constexpr int NLOADA = PR * 8;                                // vector-memory loads per chunk (inputs)
};

struct SplitConvParams {
    const float* src[2];
    long long src_bstride[2];
    int srcC[2];
    int nsrc;
    const float* inv_scale;     // per filter: 2^-e
    const _Float16* wp;         // [n-tile][chunk][tap][part][k-group][NT filters][8 channels] fp16
    float* out;
    long long out_bstride;
    int N, OC, Cin, H, W;       // output size
    int sH, sW;                 // source planes: H x W, (H/2) x (W/2) for the up-conv, the input size of a stride-2 conv
    int tilesX, tilesY, nTilesN, nblocks;
    int act;
    float slope;
    int vec4;                   // output rows are 16-byte aligned quads (width % 4 == 0, aligned base and strides)
    float prescale;             // 2^k on the activations (k = act_exponent of the launch): used when amax[0] is null
    float unscale;              // 2^-k
    const unsigned* amax[2];    // per-frame max |a| slots of the sources (kbn_common.h): k follows the data, frame by frame
    unsigned* out_amax;         // per-frame max |out| slot of the output, or null
    // producer-written split format ("pair" tensors, see below): source 0 and / or the output as fp16 pairs
    const _Float16* pair_src;   // source 0 in pair format, or null (then src[0] is an fp32 NCHW tensor)
    long long pair_src_bstride; // halves per frame
    const float* pair_src_scale;// per frame: the 2^k its producer applied
    _Float16* pair_out;         // the output in pair format, or null (then `out`)
    long long pair_out_bstride;
    float* pair_out_scale;      // per frame: the 2^k applied here (every workgroup of a frame writes the same value)
    const float* l1;            // per 16-channel chunk: max over filters of sum |w| (the table behind the packed weights)
    int tp_x0, tp_tilesY, tp_nblocks;   // conv3x3_split_mixed_kernel: first column, tile rows and workgroups of the transposed tiles
    int sub0;                   // conv1x1s2_split_kernel: source 0 holds only the pixels the conv reads (H x W planes, stride 1)
    // conv1x1s2_split_kernel: three more input channels taken in fp32 in the epilogue (the KB block's backprojection)
    const float* xyz;           // N x 3 x H x W (output size), or null
    long long xyz_bstride;
    const float* wxyz;          // out_channels x 3 fp32
    // split-K (KSPLIT kernels): workgroups per tile, elements between the partial sums' plane sets (p.out is the workspace then)
    int ksplit;
    long long ks_stride;
};

// two-term split of 8 floats: h1 = fp16(a 2^k), h2 = fp16((a 2^k - h1) 2^11)
__device__ __forceinline__ void sp_split8(const float (&v)[8], float prescale, sph8& h1, sph8& h2) {
    const float prescale_hi = prescale * 2048.f;
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const f32x2 a = {v[k], v[k + 1]};
        const sph2 c1 = __builtin_convertvector(a * prescale, sph2);
        const f32x2 f = {(float)c1[0], (float)c1[1]};
        const f32x2 hi = a * prescale_hi;
        const f32x2 r = {__builtin_fmaf(f[0], -2048.f, hi[0]), __builtin_fmaf(f[1], -2048.f, hi[1])};
        const sph2 c2 = __builtin_convertvector(r, sph2);
        h1[k] = c1[0]; h1[k + 1] = c1[1];
        h2[k] = c2[0]; h2[k + 1] = c2[1];
    }
}

// The activation exponent of frame n: with slots on the sources, k = 14 - floor(log2(max |a|)) puts the frame's largest
// activation in [2^14, 2^15) of the fp16 window (65504 is the overflow: a factor 2 to spare for the rounding of h1), so
// |a| 2^k >= 2^-14 -- 29 binades below the maximum -- keeps the full 22 bits and anything smaller is off by less than
// 2^-40 of the maximum.  An all-zero frame (or a denormal maximum) takes k = 100, Inf / NaN maxima k = -100: finite
// scales either way.  Wave-uniform: n comes from blockIdx, the loads are scalar.
__device__ __forceinline__ void sp_act_scale(const SplitConvParams& p, int n, float& prescale, float& unscale) {
    prescale = p.prescale;
    unscale = p.unscale;
    if (p.amax[0]) {   // launch-uniform
        unsigned b = p.amax[0][n];
        if (p.amax[1]) b = max(b, p.amax[1][n]);
        int k = 14 + 127 - (int)(b >> 23);
        k = k > 100 ? 100 : (k < -100 ? -100 : k);
        prescale = __uint_as_float((unsigned)(127 + k) << 23);
        unscale = __uint_as_float((unsigned)(127 - k) << 23);
    }
}
__device__ __forceinline__ float sp_amax4(float m, const f32x4& v) {
    return fmaxf(fmaxf(m, fmaxf(fin_abs(v[0]), fin_abs(v[1]))), fmaxf(fin_abs(v[2]), fin_abs(v[3])));
}

// ------------------------------------------------------------------------------------------------------------------
// PAIR tensors: the producer-written split format.  A consumer that splits its fp32 inputs itself does so once per
// (input value x halo x filter tile of the consumer) -- 2.4 to 4.8 times per value in the decoder -- on the vector ALU,
// beside the MFMAs it feeds (staging ablation in DESIGN.md: 10-13 % of the decoder kernels).  A producer that knows its
// output is only read by split-operand kernels writes the two fp16 terms itself, once, in the layout the consumers
// stage: per frame [k-group = channel / 8][term h1 | h2][H * W + 1 pixels][8 channels] fp16 -- the same 4 bytes per
// value as fp32 -- and a consumer's staging is then one 16-byte LDS-DMA per pixel, k-group and term, no vector ALU
// work and no staging registers.  The extra granule at the end of every plane is ZERO (written by the producer): the
// per-lane DMA offset of a halo pixel outside the map points there.
//   The 2^k of a pair tensor is fixed by its producer BEFORE it has seen its output: from the bound
// |out| <= sum over sources (max |a_s| of the frame, from the source's slot) x (sum over the source's 16-channel chunks
// of max over filters of sum |w|), the table `l1` behind the packed weights), placed in [2^14, 2^15) like the measured
// maxima of sp_act_scale.  The bound overshoots the true maximum by a few binades (never accumulating over layers: every
// layer starts from the MEASURED maxima of its inputs), and a window up to 2^16 too high costs nothing (the terms keep
// 22 bits down to 2^-29 of the window, tests/test_split_math_cpu.py).  Every workgroup of a frame computes the same k
// and writes it to the tensor's per-frame scale slot; consumers read it there.  With two sources in different formats
// the accumulators are rescaled by the exact power of two between the two windows when the K loop changes source.
// (pair_plane_halves: conv_common.h)

__device__ __forceinline__ float sp_scale_of_bound(float bound) {   // 2^k with bound 2^k in [2^14, 2^15); finite for 0 / Inf / NaN
    int k = 14 + 127 - (int)(__float_as_uint(bound) >> 23 & 255u);
    k = k > 100 ? 100 : (k < -100 ? -100 : k);
    return __uint_as_float((unsigned)(127 + k) << 23);
}
// the 2^k of this launch's pair output for frame n (wave-uniform: scalar loads)
__device__ __forceinline__ float sp_pair_out_scale(const SplitConvParams& p, int n) {
    const int nchunks = p.Cin / SP_CK, n0 = p.nsrc > 1 ? p.srcC[0] / SP_CK : nchunks;
    float w0 = 0.f, w1 = 0.f;
    for (int c = 0; c < n0; ++c) w0 += p.l1[c];
    for (int c = n0; c < nchunks; ++c) w1 += p.l1[c];
    float bound = __uint_as_float(p.amax[0][n]) * w0;
    if (p.nsrc > 1) bound += __uint_as_float(p.amax[1][n]) * w1;
    return sp_scale_of_bound(bound);
}
// window of ONE source from its slot (the other source of the launch is a pair tensor with a scale of its own)
__device__ __forceinline__ void sp_act_scale_of(const SplitConvParams& p, int s, int n, float& prescale, float& unscale) {
    prescale = p.prescale;
    unscale = p.unscale;
    if (p.amax[s]) {
        int k = 14 + 127 - (int)(p.amax[s][n] >> 23);
        k = k > 100 ? 100 : (k < -100 ? -100 : k);
        prescale = __uint_as_float((unsigned)(127 + k) << 23);
        unscale = __uint_as_float((unsigned)(127 - k) << 23);
    }
}
// Halves of two granules -> one whole granule per lane.  In the pair epilogues lane (pixel, g = lane >> 5) holds channels
// 4 g .. 4 g + 3 of every k-group of its 32 filters; `a` is its piece of k-group q, `b` of k-group q + 1.  One
// v_permlane32_swap per dword hands lanes 0-31 the whole granule q and lanes 32-63 the whole granule q + 1: 16-byte stores.
typedef unsigned spu2 __attribute__((ext_vector_type(2)));
typedef unsigned spu4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ spu4 sp_pair_exchange(const sph4& a, const sph4& b) {
    const spu2 A = __builtin_bit_cast(spu2, a), B = __builtin_bit_cast(spu2, b);
    const auto r0 = __builtin_amdgcn_permlane32_swap(A[0], B[0], false, false);   // {A.lo | B.lo , A.hi | B.hi} by lane half
    const auto r1 = __builtin_amdgcn_permlane32_swap(A[1], B[1], false, false);
    return (spu4){r0[0], r1[0], r0[1], r1[1]};
}
// The same between 16-lane rows r and r + 1 (the 16x16x32 epilogue: lane (pixel lp, kq) holds channels 4 (kq & 1) .. of k-group
// kq >> 1): `a` is the lane's half granule of output pixel px = 0, `b` of px = 1; rows with even kq end up with the whole
// granule of px = 0, rows with odd kq with that of px = 1 (v_permlane16_swap: odd rows of the first operand <-> even rows of
// the second).
__device__ __forceinline__ spu4 sp_pair_exchange16(const sph4& a, const sph4& b) {
    const spu2 A = __builtin_bit_cast(spu2, a), B = __builtin_bit_cast(spu2, b);
    const auto r0 = __builtin_amdgcn_permlane16_swap(A[0], B[0], false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(A[1], B[1], false, false);
    return (spu4){r0[0], r1[0], r0[1], r1[1]};
}
// two-term split of 4 floats already in window units (t = a 2^k)
__device__ __forceinline__ void sp_split4(const f32x4& t, sph4& h1, sph4& h2) {
#pragma unroll
    for (int k = 0; k < 4; k += 2) {   // two at a time: packed conversions and packed fp32 arithmetic
        const f32x2 a = {t[k], t[k + 1]};
        const sph2 c1 = __builtin_convertvector(a, sph2);
        const f32x2 f = {(float)c1[0], (float)c1[1]};
        const sph2 c2 = __builtin_convertvector((a - f) * 2048.f, sph2);   // a - f and the scaling are exact
        h1[k] = c1[0]; h1[k + 1] = c1[1];
        h2[k] = c2[0]; h2[k + 1] = c2[1];
    }
}

// Tiles of the folded up-convs (upconv_split.hip); the host side needs them for the blob layout (split_nt).
constexpr int UF_NT = 32, UF_ITEMS = 16;   // upconv2x_split_kernel: 32 filters per tile; sixteen folded 2 x 2 weight sets per channel
constexpr int U16_NT = 16, U16_CK = 32;    // upconv2x_split16_kernel: 16 filters per tile, 32 channels per chunk
constexpr int U64_NT = 64;                 // upconv2x_split64_kernel: 64 filters per tile
__host__ __device__ constexpr bool uf_narrow(int out_channels, int in_channels) {
    return out_channels <= U16_NT && (in_channels % U16_CK) == 0;
}
__host__ __device__ constexpr bool uf_wide(int out_channels) {   // whole 64-wide tiles, no more padding than 32-wide ones
    return out_channels >= U64_NT && (ceil_div(out_channels, 32) & 1) == 0;
}

// ---- host side ----------------------------------------------------------------------------------------------------
// One launch of the split-conv kernel instantiation K (launch_lds, kbn_common.h: the once-per-device flag belongs to K); its flags
// PIN, POUT, TP, ONE come from flag_dispatch
template <auto K>
int split_launch(unsigned blocks, unsigned threads, size_t lds, hipStream_t stream, const SplitConvParams& p) {
    return launch_lds<K, 160 * 1024>(blocks, threads, lds, stream, p);
}
template <class... A>
int split_dispatch(A&&... a) { return flag_dispatch(std::forward<A>(a)...); }

// Launchers shared between the translation units of the split-operand kernels.
// conv_split.hip: per-filter exponents (split_scale_kernel over `per_filter` weights of each of ceil(OC / NT) * NT filters) and
// the fp16 panel (pack_split_kernel: `total` halves, `taps` 9 or 1, channels from skip_at on shifted by `skip`) of a 3x3 or 1x1 weight
void split_pack_launch(const float* w, float* inv_scale, _Float16* packed, int OC, int per_filter, int Cin, int NT, long long total,
                       int taps, int skip_at, int skip, hipStream_t stream);
// upconv_split.hip: per-filter exponents (ocpad filters) and the folded weights of an up-conv blob (tr: ConvTranspose2d taps)
void upconv_split_pack(const float* w, float* inv_scale, _Float16* packed, int OC, int Cin, int ocpad, long long total, int tr,
                       hipStream_t stream);
// upconv_split.hip: the folded up-conv of a launch kbn_conv3x3_split_forward(_ksplit) has validated (mode 3 / 4); p.ksplit > 1:
// the 64-filter kernel's split-K form into p.out (the workspace), reduced by the caller
int upconv_split_launch(SplitConvParams p, hipStream_t stream);

}  // namespace kbn
