// conv_bwd_weight.hip -- the weight gradient of every conv the three trainable networks differentiate: one kernel family, one host body.
//
// conv_bwd_weight_kernel<KS, STRIDE, MB>: the gradient with respect to the OIHW weight of conv_{KS x KS, STRIDE, padding KS / 2}(cat(srcs)),
//   for (KS, STRIDE) in {(3, 1), (1, 1), (1, 2), (3, 2), (5, 2), (7, 2)}.  fp32 in and out, NO floating-point atomics.
//   M = output channels, 16 MB per workgroup;  N = (input channel, ky, kx) = the weight's flat inner index, 64 per workgroup;
//   K = every OUTPUT pixel of the batch, 32 per chunk, on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 sums).
//   A[k][m] = g[pixel, oc] (contiguous along pixels), B[k][n] = the input at the tap (zero outside by predicate).  A thread's 8
//   columns are the same in every chunk: decoded once, before the K loop.  Wave w owns columns 16 w .. 16 w + 15 times all MB row blocks.
//   grid.z workgroups SPLIT K: split z sums chunks [z cps, (z + 1) cps) into plane z of a scratch buffer and sum_splits_kernel adds
//   the planes in split order (the KSPLIT + ksplit_reduce_kernel pattern of conv_split.hip); one split writes the weight gradient
//   directly.  The split comes from the shape alone (bwd_weight_plan): the bits are a function of the arguments.
//   LDS is double-buffered with pitches = 17 mod 32: the staging stores (a lane per pixel = per row) fall on 32 distinct banks, the
//   fragment reads (16 consecutive floats per row, two rows per half-wave) collide on one bank only.
//
// conv_bwd_weight / conv_bwd_weight_scratch_bytes: what the two extern "C" pairs run behind their own case checks
//   (kbn_conv2d_s2_backward_weight in posenet_backward.hip, kbn_conv2d_backward_weight in conv_affine_backward.hip).
#include "conv_bwd_weight.h"

namespace kbn {
namespace {

constexpr int BW_BN = 64, BW_KC = 32, BW_BP = BW_BN + 17;
constexpr int BW_TARGET_WORKGROUPS = 512;   // two per CU of a 256-CU device; a constant, so that the split (and the bits) do not follow the device
constexpr int BW_MIN_CHUNKS = 4, BW_MAX_SPLITS = 1024;

__host__ __device__ inline int bw_mb(int oc) { return oc <= 16 ? 1 : (oc <= 32 ? 2 : 4); }
__host__ __device__ constexpr int bw_ap(int mb) { return mb == 1 ? 49 : 16 * mb + 17; }   // = 17 mod 32

struct BwParams {
    const float* g;
    long long gbs;
    const float* src0;
    const float* src1;
    long long bs0, bs1;
    int C0, Ctot;
    float* out;   // the weight gradient (one split) or the scratch planes
    int N, OC, H, W, OH, OW;
    int M;        // N * OH * OW
    int CK;       // Ctot k k
    int nchunks, cps;   // chunks of 32 pixels; chunks per split
};

__global__ void sum_splits_kernel(const float* __restrict__ planes, float* __restrict__ out, long long total, int splits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float s = planes[i];
    for (int z = 1; z < splits; ++z) s += planes[(long long)z * total + i];   // split order, always
    out[i] = s;
}

struct BwPlan {
    int ok, OH, OW, M, CK, nchunks, cps, splits, mb;
    unsigned ntn, ntm;
};

// `splits` <= 0: chosen here (enough workgroups for the chip, at least BW_MIN_CHUNKS chunks each); > 0: as asked, at most one per chunk
BwPlan bwd_weight_plan(int n, int oc, int cin, int ks, int stride, int h, int w, int splits) {
    BwPlan pl{};
    if (n <= 0 || oc <= 0 || cin <= 0 || h <= 0 || w <= 0 || ks <= 0 || stride <= 0) return pl;
    // the ranges of include/kbnet_hip.h, asked before any int arithmetic (ceil_div adds before it divides)
    if (oc > KBN_MAX_CHANNELS || cin > KBN_MAX_CHANNELS || ks > 7 || stride > 2 || h > KBN_MAX_MAP_SIDE || w > KBN_MAX_MAP_SIDE) return pl;
    if ((long long)h * w > 0x7fffffffLL) return pl;   // before n x OH x OW, which then fits 64 bits
    pl.OH = ceil_div(h, stride);
    pl.OW = ceil_div(w, stride);
    const long long M = (long long)n * pl.OH * pl.OW;
    const long long CK = (long long)cin * ks * ks;
    if (M > 0x7fffffffLL - BW_KC || CK > (1 << 24) || (long long)h * w > 0x7fffffffLL || (long long)oc * CK > 0x7fffffffLL) return pl;
    pl.M = (int)M;
    pl.CK = (int)CK;
    pl.nchunks = ceil_div(pl.M, BW_KC);
    pl.mb = bw_mb(oc);
    pl.ntn = (unsigned)ceil_div(pl.CK, BW_BN);
    pl.ntm = (unsigned)ceil_div(oc, 16 * pl.mb);
    if (pl.ntm > 65535u) return pl;
    if (splits <= 0) {
        const long long tiles = (long long)pl.ntn * pl.ntm;
        long long s = (BW_TARGET_WORKGROUPS + tiles - 1) / tiles;
        s = s < pl.nchunks / BW_MIN_CHUNKS ? s : pl.nchunks / BW_MIN_CHUNKS;
        splits = (int)(s < 1 ? 1 : s);
    }
    if (splits > BW_MAX_SPLITS) splits = BW_MAX_SPLITS;
    if (splits > pl.nchunks) splits = pl.nchunks;
    pl.cps = ceil_div(pl.nchunks, splits);
    pl.splits = ceil_div(pl.nchunks, pl.cps);   // no empty split
    pl.ok = 1;
    return pl;
}

// The launch that ends a split weight gradient: grad_weight = the planes of `scratch` added in split order
void sum_splits_launch(const float* scratch, float* grad_weight, long long total, int splits, hipStream_t stream) {
    hipLaunchKernelGGL(sum_splits_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, scratch, grad_weight, total,
                       splits);
}

template <int KS, int STRIDE, int MB>
__global__ __launch_bounds__(256) void conv_bwd_weight_kernel(const BwParams p) {
    constexpr int KK = KS * KS, PAD = KS / 2, BM = 16 * MB, AP = bw_ap(MB);
    constexpr int AJ = BM / 8;    // rows of A a thread stages per chunk
    __shared__ float As[2][BW_KC * AP];
    __shared__ float Bs[2][BW_KC * BW_BP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nt = blockIdx.x, mt = blockIdx.y, split = blockIdx.z;
    const int HW = p.H * p.W, OHW = p.OH * p.OW;
    const int px = tid & (BW_KC - 1), cr = tid >> 5;   // this thread's pixel of a chunk; its first row / column

    // the 8 columns (input channel, tap) this thread gathers, fixed over the K loop: c << 6 | ky << 3 | kx, or -1
    int cols[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = nt * BW_BN + cr + 8 * j;
        if (col < p.CK) {
            const int c = col / KK, t = col - c * KK;
            const int ky = t / KS, kx = t - ky * KS;
            cols[j] = (c << 6) | (ky << 3) | kx;
        } else {
            cols[j] = -1;
        }
    }

    const int c_begin = split * p.cps;
    const int c_end = min(p.nchunks, c_begin + p.cps);

    float va[AJ], vb[8];
    auto load_chunk = [&](int chunk) {
        const int m = chunk * BW_KC + px;
        const bool mvalid = m < p.M;
        int fn = 0, rem = 0, iy0 = 0, ix0 = 0;
        if (mvalid) {
            fn = m / OHW;
            rem = m - fn * OHW;
            const int oy = rem / p.OW, ox = rem - oy * p.OW;
            iy0 = STRIDE * oy - PAD;
            ix0 = STRIDE * ox - PAD;
        }
        const float* gf = p.g + (long long)fn * p.gbs + rem;
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int oc = mt * BM + cr + 8 * j;
            va[j] = (mvalid && oc < p.OC) ? gf[(long long)oc * OHW] : 0.f;
        }
        const float* f0 = p.src0 + (long long)fn * p.bs0;
        const float* f1 = p.src1 ? p.src1 + (long long)fn * p.bs1 : nullptr;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = cols[j];
            const int c = e >> 6, iy = iy0 + ((e >> 3) & 7), ix = ix0 + (e & 7);
            float v = 0.f;
            if (mvalid && e >= 0 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
                const float* plane = (c < p.C0) ? f0 + (long long)c * HW : f1 + (long long)(c - p.C0) * HW;
                v = plane[iy * p.W + ix];
            }
            vb[j] = v;
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) As[buf][px * AP + cr + 8 * j] = va[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[buf][px * BW_BP + cr + 8 * j] = vb[j];
    };

    f32x4 acc[MB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) acc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (c_begin < c_end) {
        load_chunk(c_begin);
        store_chunk(0);
    }
    __syncthreads();
    for (int chunk = c_begin; chunk < c_end; ++chunk) {
        const int buf = (chunk - c_begin) & 1;
        const bool more = chunk + 1 < c_end;
        if (more) load_chunk(chunk + 1);
        const float* Ab = As[buf] + lk * AP + li;
        const float* Bb = Bs[buf] + lk * BW_BP + wave * 16 + li;
#pragma unroll
        for (int k4 = 0; k4 < BW_KC / 4; ++k4) {
            const float b = Bb[k4 * 4 * BW_BP];
#pragma unroll
            for (int mi = 0; mi < MB; ++mi)
                acc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ab[k4 * 4 * AP + mi * 16], b, acc[mi], 0, 0, 0);
        }
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // lane (li, lk) holds output channels 4 lk + r of each row block for column li of this wave's 16
    const int col = nt * BW_BN + wave * 16 + li;
    if (col < p.CK) {
        float* o = p.out + (long long)split * p.OC * p.CK + col;
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int oc = mt * BM + mi * 16 + lk * 4 + r;
                if (oc < p.OC) o[(long long)oc * p.CK] = acc[mi][r];
            }
        }
    }
}

template <int KS, int STRIDE>
void bwd_weight_launch_mb(const BwParams& p, int mb, dim3 grid, hipStream_t stream) {
    switch (mb) {
        case 1: hipLaunchKernelGGL((conv_bwd_weight_kernel<KS, STRIDE, 1>), grid, dim3(256), 0, stream, p); break;
        case 2: hipLaunchKernelGGL((conv_bwd_weight_kernel<KS, STRIDE, 2>), grid, dim3(256), 0, stream, p); break;
        default: hipLaunchKernelGGL((conv_bwd_weight_kernel<KS, STRIDE, 4>), grid, dim3(256), 0, stream, p); break;
    }
}

}  // namespace

size_t conv_bwd_weight_scratch_bytes(int n, int out_channels, int in_channels, int kernel_size, int stride, int in_height, int in_width,
                                     int splits) {
    const BwPlan pl = bwd_weight_plan(n, out_channels, in_channels, kernel_size, stride, in_height, in_width, splits);
    if (!pl.ok || pl.splits <= 1) return 0;
    return (size_t)pl.splits * out_channels * pl.CK * sizeof(float);
}

int conv_bwd_weight(bool case_ok, const kbn_conv_src* srcs, int n_src, const float* grad_out, long long grad_out_batch_stride,
                    float* grad_weight, int n, int out_channels, int kernel_size, int stride, int in_height, int in_width, int splits,
                    float* scratch, size_t scratch_bytes, hipStream_t stream) {
    if (!srcs || !grad_out || !grad_weight) return KBN_ERR_INVALID_ARGUMENT;
    if (n_src < 1 || n_src > 2 || n <= 0 || out_channels <= 0 || in_height <= 0 || in_width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    if (!case_ok) return KBN_ERR_UNSUPPORTED;
    BwParams p{};
    int ctot = 0;
    if (int rc = check_tensor_srcs(srcs, n_src, n, in_height, in_width, &ctot)) return rc;
    if (ctot >= (1 << 24)) return KBN_ERR_UNSUPPORTED;   // the column code keeps the channel above 6 bits of tap
    const BwPlan pl = bwd_weight_plan(n, out_channels, ctot, kernel_size, stride, in_height, in_width, splits);
    if (!pl.ok) return KBN_ERR_UNSUPPORTED;
    if (grad_out_batch_stride < (long long)out_channels * pl.OH * pl.OW && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    const long long total = (long long)out_channels * pl.CK;
    if (pl.splits > 1 && (!scratch || scratch_bytes < (size_t)pl.splits * total * sizeof(float))) return KBN_ERR_INVALID_ARGUMENT;
    p.g = grad_out;
    p.gbs = grad_out_batch_stride;
    p.src0 = srcs[0].data;
    p.bs0 = srcs[0].batch_stride;
    p.C0 = srcs[0].channels;
    if (n_src == 2) { p.src1 = srcs[1].data; p.bs1 = srcs[1].batch_stride; }
    p.Ctot = ctot;
    p.out = pl.splits > 1 ? scratch : grad_weight;
    p.N = n;
    p.OC = out_channels;
    p.H = in_height;
    p.W = in_width;
    p.OH = pl.OH;
    p.OW = pl.OW;
    p.M = pl.M;
    p.CK = pl.CK;
    p.nchunks = pl.nchunks;
    p.cps = pl.cps;
    const dim3 grid(pl.ntn, pl.ntm, (unsigned)pl.splits);
    switch (10 * kernel_size + stride) {   // the six instantiations; the callers' case checks let nothing else through
        case 31: bwd_weight_launch_mb<3, 1>(p, pl.mb, grid, stream); break;
        case 11: bwd_weight_launch_mb<1, 1>(p, pl.mb, grid, stream); break;
        case 12: bwd_weight_launch_mb<1, 2>(p, pl.mb, grid, stream); break;
        case 32: bwd_weight_launch_mb<3, 2>(p, pl.mb, grid, stream); break;
        case 52: bwd_weight_launch_mb<5, 2>(p, pl.mb, grid, stream); break;
        case 72: bwd_weight_launch_mb<7, 2>(p, pl.mb, grid, stream); break;
        default: return KBN_ERR_UNSUPPORTED;
    }
    KBN_CHECK_LAUNCH();
    if (pl.splits > 1) {
        sum_splits_launch(scratch, grad_weight, total, pl.splits, stream);
        KBN_CHECK_LAUNCH();
    }
    return KBN_OK;
}

}  // namespace kbn
