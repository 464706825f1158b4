// conv_split.hip -- 3x3 convs with fp32-grade results on the 16-bit matrix core (operands split in two fp16 terms: the
// arithmetic is described in split_common.h), the split-K reduction of their latency form and the per-frame absmax pass.
//
// Direct 3x3 conv (+ LeakyReLU) over one or two NCHW fp32 sources -- MODE 0: the concat convs of the decoder, reference
// src/net_utils.py:1483-1487; MODE 2: stride 2, the image convs of the KB blocks, :1348 -- as an implicit GEMM with M = 32 output
// pixels of a row, N = 32 filters, K = 16 channels per v_mfma_f32_32x32x16_f16.  (MODE 3 / 4, the folded nearest-2x up-conv and
// the transposed conv, run the kernels of upconv_split.hip behind the same entry point.)  Workgroup = 512 threads = 8 waves = RG
// row groups x 8/RG filter groups; a wave owns MB rows (m-blocks) x two 32-filter n-blocks and keeps TWO accumulators
// per block: the main term h1 w1, and the two small terms (2^-11 of it) apart, so that the main accumulator is rounded
// once per 16-channel step.  Stride 1: 8 x 1 waves, tile 16 rows x 32 pixels x 64 filters; stride 2: 4 x 2 waves, tile
// 8 x 32 x 128.  K loop over chunks of 16 channels, 9 taps each:
//   A  the (16+2) x (32+2) input pixels of the chunk (stride 2: 17 x 65, columns de-interleaved), split on the way into
//      LDS: a thread loads 8 channels of a pixel (scalar plane base + lane offset), splits them (v_cvt_pk_f16_f32,
//      v_cvt_f32_f16, v_pk_fma_f32) and writes two 16-byte words, layout [part][k-group][pixel][8 channels]: an MFMA A fragment is one
//      ds_read_b128, fetched one m-block ahead of its MFMAs.  Double buffered: the global loads of chunk c+1 are in
//      flight under the MFMAs of chunk c, their split + LDS writes are spread over the MFMA groups of the later taps.
//   B  weights pre-split at pack time, [chunk][tap][part][k-group][filter][8 channels] fp16.  MODE 0: the nine taps of
//      a chunk are copied into LDS by LDS-DMA (double buffered): every global access of chunk c+1 is issued at the
//      start of chunk c and awaited once, late in it -- no vmcnt wait between MFMAs.  MODE 2 (its input tile leaves no
//      LDS for that): every wave loads its B fragments straight from global memory, one tap ahead (the row-group waves
//      of a filter group hit the same lines in L1).
// ONE barrier per chunk.  What bounds it: the chip's power limit (the MFMAs alone: 77 % of the launch at 1.7-2.0 GHz;
// zero-filled operands run 25 % faster through the same instruction stream), then the part of the skeleton that does
// not hide under them (DESIGN.md section 4 has the ablation).
#include "split_common.h"

// A/B builds (KBN_HIPCC_FLAGS=-DKBN_SPLIT_PRIO=n): 1 s_setprio(1) around every MFMA group of the concat kernel, 2 once for
// waves 4-7.  Measured inside the forward (four concat convs, 32 KITTI frames): 4168-4312 us without, 4334-4360 with 1, 4165 with 2:
// the waves of this kernel move in lockstep, there is nothing for the arbiter to prefer.  Off.
#ifndef KBN_SPLIT_PRIO
#define KBN_SPLIT_PRIO 0
#endif

namespace kbn {

// pass 1 of the pack: per-filter exponent; inv_scale[oc] = 2^-e
__global__ void split_scale_kernel(const float* __restrict__ w, float* __restrict__ inv_scale, int OC, int per_filter) {
    const int oc = blockIdx.x;
    __shared__ float red[256];
    float m = 0.f;
    if (oc < OC)
        for (int i = threadIdx.x; i < per_filter; i += 256) m = fmaxf(m, fabsf(w[(long long)oc * per_filter + i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int ex = SP_WEXP;
        if (red[0] > 0.f && red[0] < 3.0e38f) (void)frexpf(red[0], &ex);   // red[0] = m 2^ex, m in [0.5, 1)
        int e = SP_WEXP - ex;
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
        inv_scale[oc] = ldexpf(1.f, -e);
    }
}

// pass 2: OIHW fp32 -> [n-tile][chunk][tap][part][k-group][n][8 k] fp16, zero padded
// `taps` = 9 (3x3) or 1 (1x1); channel c of the packed panel is channel c (c < skip_at) or c + skip of the weight: the
// 1x1 conv of the KB block leaves its three backprojection channels out of the panel (they are taken in fp32)
__global__ void pack_split_kernel(const float* __restrict__ w, const float* __restrict__ inv_scale, _Float16* __restrict__ packed,
                                  int OC, int Cin, int nchunks, int NT, long long total, int taps, int skip_at, int skip) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int per_chunk = taps * 2 * 2 * NT * 8;
    int r = (int)(e % per_chunk);
    const long long q = e / per_chunk;
    const int chunk = (int)(q % nchunks), nt = (int)(q / nchunks);
    const int tap = r / (2 * 2 * NT * 8); r -= tap * 2 * 2 * NT * 8;
    const int part = r / (2 * NT * 8); r -= part * 2 * NT * 8;
    const int g = r / (NT * 8); r -= g * NT * 8;
    const int n = r >> 3, k = r & 7;
    const int c = chunk * SP_CK + g * 8 + k, oc = nt * NT + n;
    _Float16 h = (_Float16)0.f;
    if (c < Cin && oc < OC) {
        const int cw = c < skip_at ? c : c + skip;
        const float ws = w[((long long)oc * (Cin + skip) + cw) * taps + tap] * (1.f / inv_scale[oc]);   // w 2^e, exact
        const _Float16 w1 = (_Float16)ws;
        h = part == 0 ? w1 : (_Float16)((ws - (float)w1) * 2048.f);   // the residual scaled by 2^11 (|.| <= 4096), like the activations'

    }
    packed[e] = h;
}

// the bound table of the pair format: l1[c] = max over filters of sum |w| over the 16 input channels of chunk c (all taps);
// one block per chunk.  For the folded up-convs the unfolded 3 x 3 weights bound the folded ones (triangle inequality).
__global__ __launch_bounds__(256) void split_l1_kernel(const float* __restrict__ w, float* __restrict__ l1, int OC, int Cin, int taps) {
    __shared__ float red[256];
    const int c = blockIdx.x;
    float m = 0.f;
    for (int oc = threadIdx.x; oc < OC; oc += 256) {
        const float* wp = w + ((long long)oc * Cin + c * SP_CK) * taps;
        float sum = 0.f;
        for (int e = 0; e < SP_CK * taps; ++e) sum += fabsf(wp[e]);
        m = fmaxf(m, sum);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + st]);
        __syncthreads();
    }
    if (threadIdx.x == 0) l1[c] = red[0];
}

// max |x| of each of n frames of `per_frame` contiguous floats (frames batch_stride apart) into slots[frame] (integer
// atomic max of the bit patterns).  HBM bound: 16-byte loads when the frames are 16-byte aligned, four in flight per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void absmax_frames_kernel(const float* __restrict__ x, long long batch_stride, long long per_frame,
                                                            unsigned* __restrict__ slots) {
    const float* xn = x + (long long)blockIdx.y * batch_stride;
    float m = 0.f;
    const long long stride = (long long)gridDim.x * 256;
    if constexpr (VEC) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(xn);
        const long long n4 = per_frame >> 2;
        long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        for (; i + 3 * stride < n4; i += 4 * stride) {
            const f32x4 a = x4[i], b = x4[i + stride], c = x4[i + 2 * stride], d = x4[i + 3 * stride];
            m = sp_amax4(sp_amax4(sp_amax4(sp_amax4(m, a), b), c), d);
        }
        for (; i < n4; i += stride) m = sp_amax4(m, x4[i]);
        for (long long t = (n4 << 2) + (long long)blockIdx.x * 256 + threadIdx.x; t < per_frame; t += stride) m = fmaxf(m, fin_abs(xn[t]));
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per_frame; i += stride) m = fmaxf(m, fin_abs(xn[i]));
    }
    absmax_commit(slots + blockIdx.y, m);
}

int absmax_frames_launch(const float* x, long long batch_stride, int n, long long per_frame, unsigned* slots, hipStream_t stream) {
    if (!x || !slots || n < 1 || per_frame < 1) return KBN_ERR_INVALID_ARGUMENT;
    const bool vec = !((reinterpret_cast<uintptr_t>(x) & 15) || (batch_stride & 3));
    const int blocks = (int)std::min<long long>(std::max(1, 2048 / n), (per_frame + 4095) / 4096);   // >= 16 floats per thread, ~2048 workgroups
    if (vec) hipLaunchKernelGGL(absmax_frames_kernel<true>, dim3(blocks, n), dim3(256), 0, stream, x, batch_stride, per_frame, slots);
    else hipLaunchKernelGGL(absmax_frames_kernel<false>, dim3(blocks, n), dim3(256), 0, stream, x, batch_stride, per_frame, slots);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

template <int N, int NBX>
__device__ __forceinline__ void sp_wait_b(f32x4 (&b)[NBX][2]) {   // vmcnt(N), tied to the registers it guards
    static_assert(NBX == 1 || NBX == 2, "one or two 32-filter blocks per wave");
    if constexpr (NBX == 2) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(b[0][0]), "+v"(b[0][1]), "+v"(b[1][0]), "+v"(b[1][1]) : "n"(N));
    else asm volatile("s_waitcnt vmcnt(%2)" : "+v"(b[0][0]), "+v"(b[0][1]) : "n"(N));
}

// RG row groups x (8 / RG) filter groups of waves; a wave owns MB = TH / RG rows (m-blocks) x two 32-filter n-blocks.
// APART: the two small terms (h1 w2, h2 w1 2^-11; 2^-11 of the sum) accumulate in their own registers, so that the main
// accumulator is rounded once per k-step instead of three times (error vs fp64 / 1.7: the level of the Winograd kernel).
// BLDS: the weights of a chunk (nine taps) are copied into LDS by LDS-DMA, double buffered like the inputs: every global
// access of chunk c+1 is issued at the start of chunk c and awaited once, in front of the barrier that ends chunk c --
// no vmcnt wait sits between MFMAs (waves retire their loads in order: with the weights fetched per tap into registers,
// the tap-2 wait also had to wait for the next chunk's inputs, +28 % on the decoder's concat convs).
// PIN0: source 0 is a pair tensor (its chunks are staged by LDS-DMA; a second, fp32 source is split here as before and the
// accumulators change window between the two); POUT: the output is written as a pair tensor (MFMA operands swapped: a
// lane's accumulator registers run over the FILTERS of one pixel).  Both: MODE 0 with the weights through LDS.
// TP (MODE 0): TRANSPOSED tiles for the last, narrow column of a map whose width leaves 1-16 columns behind the whole 32-column
// tiles (KITTI: 76 = 2 x 32 + 12, 304 = 9 x 32 + 16): 32 rows x 16 columns per workgroup, a 32-pixel MFMA block = two rows of 16
// pixels, the staged region 34 rows x 18 columns (the same 612 granules).  Half the MFMAs of the column tiles it replaces
// (22 x 76: 55 instead of 66 blocks per frame).  The transposed tiles are the LAST workgroups of the same launch
// (conv3x3_split_mixed_kernel): as a launch of their own -- 128 workgroups for deconv4's conv -- they would cost the round of
// workgroups they save.
// MIXED: the grid is p.nblocks whole tiles followed by p.tp_nblocks transposed ones: the body (conv_split_body.inc) is compiled
// twice into the kernel, once per tile form, and a workgroup takes the one its block index selects.
// ONE: the THROUGHPUT-ONLY one-term mode (KBN_FP16_ONE_TERM=1; BASELINE configs[2]'s 16-bit leg and the ablation "same skeleton, a
// third of the MFMAs"): only h1 w1 is issued -- plain fp16 operands, fp32 accumulation -- and the h2 halves of the staged tiles
// are neither fetched (pair sources, weights through LDS) nor read.  Never on the parity-gated path.
template <int MODE, int RG, bool APART, bool BLDS, int NBW = 2, bool PIN0 = false, bool POUT = false, bool MIXED = false, bool ONE = false, bool KSPLIT = false>   // NBW: 32-filter blocks per wave
__global__ __launch_bounds__(SP_THREADS, 1) void conv3x3_split_kernel(const SplitConvParams p) {
    static_assert(MODE != 1, "the nine-tap up-conv (MODE 1) is gone: the folded up-convs are in upconv_split.hip");
    static_assert(!MIXED || (MODE == 0 && BLDS), "transposed tiles: the concat kernel");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (!MIXED || (int)blockIdx.x < p.nblocks) {
        constexpr bool TP = false;
        const int block = blockIdx.x, nblocks = p.nblocks, tilesX = p.tilesX, tilesY = p.tilesY;
#include "conv_split_body.inc"
    } else if constexpr (MIXED) {
        constexpr bool TP = true;
        const int block = (int)blockIdx.x - p.nblocks, nblocks = p.tp_nblocks, tilesX = 1, tilesY = p.tp_tilesY;
#include "conv_split_body.inc"
    }
}

// Sum of the split-K partial planes (conv3x3_split_kernel / upconv2x_split64_kernel<.., KSPLIT>), in split order, + activation + the frame's max |out|:
// ws [ksplit][n][OC][H W] -> out (frames out_bstride apart).  A thread owns `kr` items of four consecutive pixels (VEC) or of one, 256
// threads apart (the launcher keeps about 512 blocks per frame, at most 8 items per thread); the block's maximum meets in LDS so that
// ONE wave per block touches the frame's slot (a commit per wave is 13 k agent-scope accesses of one address for deconv2's conv: 110 us
// of a 60 us launch).
template <bool VEC>
__global__ __launch_bounds__(256) void ksplit_reduce_kernel(const float* __restrict__ ws, long long ks_stride, int ksplit, float* __restrict__ out,
                                                            long long out_bstride, long long per_frame, float slope, unsigned* __restrict__ out_amax, int kr) {
    __shared__ float red[4];
    const int n = blockIdx.y;
    float m = 0.f;
    for (int r = 0; r < kr; ++r) {
        const long long i = (((long long)blockIdx.x * kr + r) * 256 + threadIdx.x) * (VEC ? 4 : 1);
        if (i < per_frame) {
            const float* src = ws + (long long)n * per_frame + i;
            if constexpr (VEC) {
                f32x4 a = *reinterpret_cast<const f32x4*>(src);
                for (int k = 1; k < ksplit; ++k) a += *reinterpret_cast<const f32x4*>(src + (long long)k * ks_stride);
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = a[j] > 0.f ? a[j] : a[j] * slope;
                *reinterpret_cast<f32x4*>(out + (long long)n * out_bstride + i) = a;
                m = sp_amax4(m, a);
            } else {
                float a = src[0];
                for (int k = 1; k < ksplit; ++k) a += src[(long long)k * ks_stride];
                a = a > 0.f ? a : a * slope;
                out[(long long)n * out_bstride + i] = a;
                m = fmaxf(m, fin_abs(a));
            }
        }
    }
    if (out_amax) {   // launch-uniform
        const unsigned b = wave_max_bits(m);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __uint_as_float(b);
        __syncthreads();
        absmax_commit(out_amax + n, threadIdx.x < 64 ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : 0.f);
    }
}

void split_pack_launch(const float* w, float* inv_scale, _Float16* packed, int OC, int per_filter, int Cin, int NT, long long total,
                       int taps, int skip_at, int skip, hipStream_t stream) {
    hipLaunchKernelGGL(split_scale_kernel, dim3(ceil_div(OC, NT) * NT), dim3(256), 0, stream, w, inv_scale, OC, per_filter);
    hipLaunchKernelGGL(pack_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w, inv_scale, packed, OC, Cin,
                       Cin / SP_CK, NT, total, taps, skip_at, skip);
}

}  // namespace kbn

extern "C" {

// filters per workgroup; the folded up-conv takes 16-filter tiles for narrow layers (upconv2x_split16_kernel)
static int split_nt(int mode, int out_channels, int in_channels) {
    if (mode == 3 && kbn::uf_narrow(out_channels, in_channels)) return kbn::U16_NT;
    // a function of the layer's shape ONLY: the blob layout follows it, so no run-time knob may enter here (a switch read
    // at pack time and again at launch time would let kbn_reload_env() in between walk a blob with the wrong tiling)
    if (mode == 3 && kbn::uf_wide(out_channels)) return kbn::U64_NT;
    return mode == 2 ? 128 : (mode == 3 ? kbn::UF_NT : 64);
}

size_t kbn_conv3x3_split_packed_weight_bytes(int out_channels, int in_channels, int mode) {
    using namespace kbn;
    if (mode == 4) mode = 3;   // the transposed conv runs the folded up-conv's kernels on its own folded weights: same blob layout
    if (out_channels < 1 || in_channels < 1 || (in_channels % SP_CK) != 0 || mode < 0 || mode > 3) return 0;
    if (!layer_shape_ok(out_channels, in_channels, 3)) return 0;
    const int nt = split_nt(mode, out_channels, in_channels), tiles = ceil_div(out_channels, nt);
    return (size_t)tiles * nt * 4 + (size_t)tiles * (in_channels / SP_CK) * ((mode == 3 ? UF_ITEMS : 9) * 2 * 2 * nt * 16)   // per 16 channels: [set][part][2 k-groups][nt][8] fp16
           + (size_t)(in_channels / SP_CK) * 4;                                                                                  // the bound table of the pair format (split_l1_kernel)
}

int kbn_conv3x3_split_pack_weight(const float* weight, void* packed, int out_channels, int in_channels, int mode,
                                  kbn_stream_t stream) {
    using namespace kbn;
    const size_t bytes = kbn_conv3x3_split_packed_weight_bytes(out_channels, in_channels, mode);
    if (!weight || !packed || bytes == 0) return KBN_ERR_INVALID_ARGUMENT;
    const int tr = mode == 4 ? 1 : 0;   // ConvTranspose2d taps instead of the nearest-2x fold (uf_fold)
    if (tr) mode = 3;
    const int nt = split_nt(mode, out_channels, in_channels), ocpad = ceil_div(out_channels, nt) * nt;
    float* inv = static_cast<float*>(packed);
    _Float16* wp = reinterpret_cast<_Float16*>(inv + ocpad);
    const size_t l1_bytes = (size_t)(in_channels / SP_CK) * 4;
    const long long total = (long long)((bytes - (size_t)ocpad * 4 - l1_bytes) / 2);
    hipLaunchKernelGGL(split_l1_kernel, dim3(in_channels / SP_CK), dim3(256), 0, (hipStream_t)stream, weight,
                       reinterpret_cast<float*>(static_cast<unsigned char*>(packed) + bytes - l1_bytes), out_channels, in_channels, 9);
    if (mode == 3) upconv_split_pack(weight, inv, wp, out_channels, in_channels, ocpad, total, tr, (hipStream_t)stream);
    else split_pack_launch(weight, inv, wp, out_channels, in_channels * 9, in_channels, nt, total, 9, in_channels, 0, (hipStream_t)stream);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_absmax_frames(const float* x, long long batch_stride, int n, long long per_frame, unsigned* slots, kbn_stream_t stream) {
    return kbn::absmax_frames_launch(x, batch_stride, n, per_frame, slots, (hipStream_t)stream);
}

static int conv3x3_split_impl(const kbn_conv_src* srcs, int n_src, const void* packed_weight, float* out,
                              long long out_batch_stride, int n, int out_channels, int height, int width, int mode,
                              int act_exponent, int apply_activation, float negative_slope, unsigned* out_absmax,
                              void* pair_out, long long pair_out_batch_stride, float* pair_out_scale, int ksplit, float* workspace,
                              kbn_stream_t stream) {
    using namespace kbn;
    if (act_exponent < -60 || act_exponent > 60) return KBN_ERR_INVALID_ARGUMENT;
    if (!srcs || n_src < 1 || n_src > 2 || !packed_weight || (!out && !pair_out) || n < 1 || out_channels < 1 || height < 1 || width < 1)
        return KBN_ERR_INVALID_ARGUMENT;
    if (mode == 4) mode = 3;   // ConvTranspose2d(3, stride 2, padding 1, output_padding 1): the folded kernels on a blob packed with mode 4
    if (mode < 0 || mode > 3) return KBN_ERR_INVALID_ARGUMENT;
    if (knob(KNOB_NO_SPLIT)) return KBN_ERR_UNSUPPORTED;
    const bool vec4 = pair_out || !((width & 3) || (reinterpret_cast<uintptr_t>(out) & 15) || (out_batch_stride & 3));
    if (!vec4 && (mode == 1 || mode == 3)) return KBN_ERR_UNSUPPORTED;   // the up-convs only store whole quads
    if ((mode == 1 || mode == 3) && (n_src != 1 || (height & 1) || (width & 1))) return KBN_ERR_UNSUPPORTED;
    SplitConvParams p{};
    int cin = 0;
    for (int s = 0; s < n_src; ++s) {
        const kbn_conv_src& a = srcs[s];
        const bool pair = a.kind == KBN_SRC_PAIR;
        if ((a.kind != KBN_SRC_TENSOR && !pair) || !a.data || a.channels < 1 || (a.channels % SP_CK) != 0) return KBN_ERR_UNSUPPORTED;
        if (s == 0) { p.sH = a.src_height; p.sW = a.src_width; }
        if (a.src_height != p.sH || a.src_width != p.sW) return KBN_ERR_INVALID_ARGUMENT;
        if (pair) {   // source 0 of the concat conv / the input of a folded up-conv, written by a split-operand producer
            if (s != 0 || mode == 1) return KBN_ERR_UNSUPPORTED;
            if (mode == 2 && n_src != 1) return KBN_ERR_UNSUPPORTED;
            // the concat kernel's K loop: a pair source beside an fp32 one, at least two 16-channel chunks each
            if (mode == 0 && (n_src != 2 || a.channels < 2 * SP_CK || srcs[1].kind != KBN_SRC_TENSOR || srcs[1].channels < 2 * SP_CK))
                return KBN_ERR_UNSUPPORTED;
            if (!a.scale || (reinterpret_cast<uintptr_t>(a.data) & 15) || (a.batch_stride & 7) ||
                a.batch_stride < (long long)(a.channels / 8) * 2 * pair_plane_halves(a.src_height, a.src_width))
                return KBN_ERR_INVALID_ARGUMENT;
            if ((long long)a.src_height * a.src_width >= 0x0fffffffLL) return KBN_ERR_UNSUPPORTED;   // 32-bit DMA offsets
            p.pair_src = reinterpret_cast<const _Float16*>(a.data); p.pair_src_bstride = a.batch_stride; p.pair_src_scale = a.scale;
        } else {
            p.src[s] = a.data; p.src_bstride[s] = a.batch_stride;
        }
        p.srcC[s] = a.channels;
        cin += a.channels;
    }
    if (p.pair_src && !p.src[0]) { p.src[0] = p.src[1]; p.src_bstride[0] = p.src_bstride[1]; }   // never dereferenced: the kernels stage source 0 by DMA
    const bool dims_ok = mode == 0 ? (p.sH == height && p.sW == width)
                       : mode != 2 ? (2 * p.sH == height && 2 * p.sW == width)
                                   : (ceil_div(p.sH, 2) == height && ceil_div(p.sW, 2) == width);
    if (!dims_ok) return KBN_ERR_INVALID_ARGUMENT;
    if (mode == 1) return KBN_ERR_UNSUPPORTED;   // the nine-tap up-conv form (rounds 2-5; superseded by the folded form, mode 3) is no longer built
    if ((long long)p.sH * p.sW > 0x1fffffffLL || (long long)height * width > 0x1fffffffLL) return KBN_ERR_UNSUPPORTED;
    if (n_src == 1) { p.src[1] = p.src[0]; p.src_bstride[1] = p.src_bstride[0]; p.srcC[1] = 0; }
    p.nsrc = n_src;
    // the exponent follows the data when EVERY source brings its slots; otherwise the static act_exponent serves
    if (srcs[0].absmax && (n_src == 1 || srcs[1].absmax)) { p.amax[0] = srcs[0].absmax; p.amax[1] = n_src > 1 ? srcs[1].absmax : nullptr; }
    else if (p.pair_src && n_src > 1 && srcs[1].absmax) p.amax[1] = srcs[1].absmax;   // the fp32 source beside a pair source: its own window
    p.out_amax = out_absmax;
    if (!layer_shape_ok(out_channels, cin, 3)) return KBN_ERR_UNSUPPORTED;   // the shapes the blob's size function answers 0 for
    const int ntf = split_nt(mode, out_channels, cin);
    p.nTilesN = ceil_div(out_channels, ntf);
    p.inv_scale = static_cast<const float*>(packed_weight);
    p.wp = reinterpret_cast<const _Float16*>(p.inv_scale + p.nTilesN * ntf);
    p.l1 = reinterpret_cast<const float*>(static_cast<const unsigned char*>(packed_weight) +
                                          kbn_conv3x3_split_packed_weight_bytes(out_channels, cin, mode) - (size_t)(cin / SP_CK) * 4);
    if (pair_out) {   // the output as a pair tensor: concat convs and the 64-filter folded up-convs; its 2^k needs every source's slot
        // the narrow up-conv writes 16 channels (two k-groups, zeros past out_channels): its pair tensor feeds the decoder tail
        const bool narrow = mode == 3 && uf_narrow(out_channels, cin);
        const bool kernel_ok = (mode == 0) || (mode == 3 && ntf == U64_NT && !uf_narrow(out_channels, cin)) ||
                               (mode == 2 && n_src == 1) || narrow;
        if (!kernel_ok || (!narrow && (out_channels & 7))) return KBN_ERR_UNSUPPORTED;
        const int pair_channels = narrow ? U16_NT : out_channels;
        if (!p.amax[0] || (n_src > 1 && !p.amax[1]) || !pair_out_scale || (reinterpret_cast<uintptr_t>(pair_out) & 15) ||
            (pair_out_batch_stride & 7) || pair_out_batch_stride < (long long)(pair_channels / 8) * 2 * pair_plane_halves(height, width))
            return KBN_ERR_INVALID_ARGUMENT;
        p.pair_out = static_cast<_Float16*>(pair_out); p.pair_out_bstride = pair_out_batch_stride; p.pair_out_scale = pair_out_scale;
    }
    if (p.pair_src && mode == 3 && !(ntf == U64_NT || uf_narrow(out_channels, cin))) return KBN_ERR_UNSUPPORTED;   // the 32-filter up-conv kernel splits its inputs itself
    if (p.pair_src && mode == 3 && uf_narrow(out_channels, cin) && (srcs[0].channels % U16_CK)) return KBN_ERR_UNSUPPORTED;
    p.out = out; p.out_bstride = out_batch_stride;
    p.N = n; p.OC = out_channels; p.Cin = cin; p.H = height; p.W = width;
    p.tilesX = ceil_div(width, SP_TW); p.tilesY = ceil_div(height, mode == 2 ? SpGeom<2>::TH : SpGeom<0>::TH);
    if (mode == 3) { p.tilesX = ceil_div(p.sW, 32); p.tilesY = ceil_div(p.sH, 16); }   // tiles of 16 x 32 low-resolution pixels
    const long long blocks = (long long)p.tilesX * p.tilesY * n * p.nTilesN;
    if (blocks > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    p.nblocks = (int)blocks;
    p.act = apply_activation ? 1 : 0; p.slope = negative_slope;
    p.prescale = ldexpf(1.f, act_exponent); p.unscale = ldexpf(1.f, -act_exponent);
    p.vec4 = vec4 ? 1 : 0;
    p.ksplit = 1;
    if (ksplit > 1) {
        // The latency form: a layer whose tiles cannot fill the chip (deconv4's conv on ONE KITTI frame: 24 workgroups of 48 chunks each)
        // spreads every tile's K loop over `ksplit` workgroups; partial sums go to `workspace` [ksplit][n][out_channels][height x width]
        // and ksplit_reduce_kernel adds them in split order.  Another summation order than the one-workgroup form: same 1e-4 parity,
        // other low bits -- opt-in (KBNetModel.latency_mode), never mixed with the default form inside one model.
        const bool up64 = mode == 3 && ntf == U64_NT && !uf_narrow(out_channels, cin);   // the 64-filter folded up-conv
        if ((mode != 0 && mode != 2 && !up64) || p.pair_src || pair_out || !workspace || !out || knob(KNOB_FP16_ONE_TERM)) return KBN_ERR_UNSUPPORTED;
        const int nchunks = cin / SP_CK;
        if (ksplit > nchunks || (long long)(ceil_div(nchunks, ksplit)) * (ksplit - 1) >= nchunks) return KBN_ERR_INVALID_ARGUMENT;   // an empty range
        if (blocks * ksplit > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
        const long long per_frame = (long long)out_channels * height * width;
        SplitConvParams q = p;
        q.ksplit = ksplit;
        q.out = workspace; q.out_bstride = per_frame; q.ks_stride = per_frame * n;
        q.out_amax = nullptr; q.act = 0;
        q.vec4 = !((width & 3) || (reinterpret_cast<uintptr_t>(workspace) & 15)) ? 1 : 0;
        q.nblocks = (int)(blocks * ksplit);
        int rc;
        if (up64) rc = upconv_split_launch(q, (hipStream_t)stream);
        else if (mode == 0)
            rc = split_launch<conv3x3_split_kernel<0, 8, true, true, 2, false, false, false, false, true>>(
                q.nblocks, SP_THREADS, SpGeom<0>::LDS + 2 * 9 * 2 * 2 * 64 * 16, (hipStream_t)stream, q);
        else rc = split_launch<conv3x3_split_kernel<2, 2, true, false, 1, false, false, false, false, true>>(q.nblocks, SP_THREADS, SpGeom<2>::LDS,
                                                                                                           (hipStream_t)stream, q);
        if (rc != KBN_OK) return rc;
        KBN_CHECK_LAUNCH();
        const float slope = apply_activation ? negative_slope : 1.f;
        const bool vec = !(per_frame & 3) && !(out_batch_stride & 3) && !((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 15);
        const long long items = vec ? per_frame / 4 : per_frame;
        long long kr = items / (256LL * 512);
        kr = kr < 1 ? 1 : (kr > 8 ? 8 : kr);
        const dim3 grid((unsigned)((items + 256 * kr - 1) / (256 * kr)), (unsigned)n);
        if (vec) hipLaunchKernelGGL(ksplit_reduce_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, workspace, q.ks_stride, ksplit, out, out_batch_stride, per_frame, slope, out_absmax, (int)kr);
        else hipLaunchKernelGGL(ksplit_reduce_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, workspace, q.ks_stride, ksplit, out, out_batch_stride, per_frame, slope, out_absmax, (int)kr);
        KBN_CHECK_LAUNCH();
        return KBN_OK;
    }
    // THROUGHPUT-ONLY (KBN_FP16_ONE_TERM=1): the concat convs, the 64-filter folded up-convs and the stride-2 convs issue h1 w1 alone
    const bool one_term = knob(KNOB_FP16_ONE_TERM) != 0;
    int rc;
    if (mode == 3) rc = upconv_split_launch(p, (hipStream_t)stream);
    else if (mode == 0) {
        // (a 16x16x32 form of this kernel was built and measured in round 2 -- profiles/r02/HISTORY.md: 1-7 % slower
        // inside the forward -- and removed in round 6)
        // a map whose width leaves 1-16 columns behind the whole 32-column tiles: that column goes to transposed tiles
        // (32 rows x 16 columns) at the end of the same launch, half the MFMAs of the tiles it replaces (KBN_DEBUG & 512: off)
        const int wrem = width % SP_TW;
        const bool tp = width >= SP_TW && wrem >= 1 && wrem <= 16 && !(knob(KNOB_DEBUG) & 512);
        if (tp) {
            p.tilesX = width / SP_TW;
            p.nblocks = p.tilesX * p.tilesY * n * p.nTilesN;
            p.tp_x0 = SP_TW * p.tilesX;
            p.tp_tilesY = ceil_div(height, 2 * SpGeom<0>::TH);
            p.tp_nblocks = p.tp_tilesY * n * p.nTilesN;
        }
        rc = split_dispatch([&](auto PIN, auto POUT, auto TP, auto ONE) {
            return split_launch<conv3x3_split_kernel<0, 8, true, true, 2, PIN, POUT, TP, ONE>>(
                p.nblocks + (tp ? p.tp_nblocks : 0), SP_THREADS, SpGeom<0>::LDS + 2 * 9 * 2 * 2 * 64 * 16, (hipStream_t)stream, p);
        }, p.pair_src != nullptr, p.pair_out != nullptr, tp, one_term);
    } else {
        // 2 row groups x 4 filter groups of waves (a wave: 4 rows x ONE 32-filter block): every weight fragment is fetched from
        // L2 by two waves instead of four -- half the vector-memory traffic of a chunk -- for twice the A fragment reads
        // from LDS.  Inside the forward (KB2 / KB3 / KB4 / conv5 image / conv5 depth, 32 KITTI frames): 397 / 337 / 314 /
        // 247 / 60 us against 414 / 360 / 322 / 281 / 69 with 4 x 2 waves of 2 rows x two blocks
        rc = split_dispatch([&](auto PIN, auto POUT, auto ONE) {
            return split_launch<conv3x3_split_kernel<2, 2, true, false, 1, PIN, POUT, false, ONE>>(p.nblocks, SP_THREADS, SpGeom<2>::LDS,
                                                                                                  (hipStream_t)stream, p);
        }, p.pair_src != nullptr, p.pair_out != nullptr, one_term);
    }
    if (rc != KBN_OK) return rc;
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

int kbn_conv3x3_split_forward(const kbn_conv_src* srcs, int n_src, const void* packed_weight, float* out,
                              long long out_batch_stride, int n, int out_channels, int height, int width, int mode,
                              int act_exponent, int apply_activation, float negative_slope, unsigned* out_absmax,
                              void* pair_out, long long pair_out_batch_stride, float* pair_out_scale, kbn_stream_t stream) {
    return conv3x3_split_impl(srcs, n_src, packed_weight, out, out_batch_stride, n, out_channels, height, width, mode, act_exponent,
                              apply_activation, negative_slope, out_absmax, pair_out, pair_out_batch_stride, pair_out_scale, 1, nullptr, stream);
}

int kbn_conv3x3_split_forward_ksplit(const kbn_conv_src* srcs, int n_src, const void* packed_weight, float* out,
                                     long long out_batch_stride, int n, int out_channels, int height, int width, int mode,
                                     int act_exponent, int apply_activation, float negative_slope, unsigned* out_absmax,
                                     int ksplit, float* workspace, kbn_stream_t stream) {
    if (ksplit < 1) return KBN_ERR_INVALID_ARGUMENT;
    return conv3x3_split_impl(srcs, n_src, packed_weight, out, out_batch_stride, n, out_channels, height, width, mode, act_exponent,
                              apply_activation, negative_slope, out_absmax, nullptr, 0, nullptr, ksplit, workspace, stream);
}

}  // extern "C"
