// posenet.hip -- the two kernels of the pose network's eval-mode forward.
//
//   networks.PoseEncoder       reference src/networks.py:536-671    seven x (conv k x k stride 2, BatchNorm2d, LeakyReLU(0.20))
//   net_utils.Conv2d           reference src/net_utils.py:51-141    bias-free conv, padding k / 2, then norm, then activation
//   networks.PoseDecoder       reference src/networks.py:1992-2075  1 x 1 conv to 6 channels, mean over H W, x 0.01, pose_matrix
//   net_utils.pose_matrix      reference src/net_utils.py:1493-1595
//
// conv_s2_affine_kernel<KS, NB>: implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 products, as conv_igemm.hip).
//   M = every output pixel of the BATCH in one index m = (frame * OH + oy) * OW + ox: a workgroup's 128-pixel tile may
//       span rows and frames, so that the last maps (11 x 38 and below) fill workgroups with pixels of several frames;
//   N = output channels, 16 NB per workgroup (NB in {1, 2, 4} from the channel count: pose_igemm_nb, pose_igemm.h);
//   K = (input channel, ky, kx) flattened, C k k, zero-padded to a multiple of 16 -- any channel count is legal.
// 256 threads = 4 waves; wave w owns m-blocks 2 w, 2 w + 1 (16 pixels each) times all NB n-blocks.
// K loop, 16 at a time: thread t gathers pixel t % 128 at k = t / 128 + 2 j (j < 8; k is wave-uniform, so the
// (channel, tap) decode is scalar) into registers while the MFMAs of the previous chunk run, then stores them to the
// other LDS buffer: one barrier per chunk.  Taps outside the image and k >= C k k are zero by predicate: no address
// outside the planes is formed into a load.  The packed weight is [n-tile][K chunk][16][16 NB], a straight copy.
// LDS: A[2][16][144] + B[2][16][BP] floats (pitches = 16 mod 32: the k = 0 / k = 1 rows of a half-wave's ds_read_b32
// fall on disjoint 16-bank groups) = 18.4 + at most 10.2 KiB.
// Epilogue: out = leaky(acc * scale[oc] + shift[oc], slope).  `scale` stays here, it is not folded into the weights:
// the conv itself then rounds as the reference's does.
//
// pose_head_kernel: one workgroup per frame.  The mean over H W of a 1 x 1 conv is the 1 x 1 conv of the per-channel
// means: only another summation order (C h w products and sums either way), and it needs no 6-channel map.
#include "pose_igemm.h"

namespace kbn {
namespace {

constexpr int S2_KC = 16;

struct S2Params {
    const float* src0;
    const float* src1;
    long long bs0, bs1;
    int C0, Ctot;
    const float* wp;
    const float* scale;
    const float* shift;
    float* out;
    long long out_bstride;
    int N, OC, H, W, OH, OW;
    int M;        // N * OH * OW
    int K, nchunks;
    int act;
    float slope;
};

template <int KS, int NB>
__global__ __launch_bounds__(256) void conv_s2_affine_kernel(const S2Params p) {
    constexpr int KK = KS * KS, PAD = KS / 2, BN = 16 * NB, BP = pose_igemm_bp(NB);
    __shared__ float As[2][S2_KC * PI_AP];
    __shared__ float Bs[2][S2_KC * BP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int mt = blockIdx.x, nt = blockIdx.y;
    const int HW = p.H * p.W, OHW = p.OH * p.OW;

    // the pixel this thread gathers
    const int pm = tid & (PI_BM - 1);
    const int khalf = __builtin_amdgcn_readfirstlane(tid >> 7);   // 0 for waves 0, 1; 1 for waves 2, 3
    const int m = mt * PI_BM + pm;
    const bool mvalid = m < p.M;
    int fn = 0, iy0 = 0, ix0 = 0;
    if (mvalid) {
        fn = m / OHW;
        const int rem = m - fn * OHW;
        const int oy = rem / p.OW, ox = rem - oy * p.OW;
        iy0 = 2 * oy - PAD;
        ix0 = 2 * ox - PAD;
    }
    const float* f0 = p.src0 + (long long)fn * p.bs0;
    const float* f1 = p.src1 ? p.src1 + (long long)fn * p.bs1 : nullptr;
    const float* wtile = p.wp + (long long)nt * p.nchunks * (S2_KC * BN);

    float va[8];
    float vb[NB];
    auto load_chunk = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = chunk * S2_KC + khalf + 2 * j;      // wave-uniform
            const int c = k / KK, t = k - c * KK;
            const int ky = t / KS, kx = t - ky * KS;
            const int iy = iy0 + ky, ix = ix0 + kx;
            float v = 0.f;
            if (mvalid && k < p.K && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
                const float* plane = (c < p.C0) ? f0 + (long long)c * HW : f1 + (long long)(c - p.C0) * HW;
                v = plane[iy * p.W + ix];
            }
            va[j] = v;
        }
        const float* wc = wtile + (long long)chunk * (S2_KC * BN);
#pragma unroll
        for (int j = 0; j < NB; ++j) vb[j] = wc[tid + 256 * j];
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 8; ++j) As[buf][(khalf + 2 * j) * PI_AP + pm] = va[j];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int e = tid + 256 * j;
            Bs[buf][(e / BN) * BP + (e % BN)] = vb[j];
        }
    };

    f32x4 acc[2][NB];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mi][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int chunk = 0; chunk < p.nchunks; ++chunk) {
        const int buf = chunk & 1;
        const bool more = chunk + 1 < p.nchunks;
        if (more) load_chunk(chunk + 1);
        const float* Ab = As[buf] + lk * PI_AP + wave * 32 + li;
        const float* Bb = Bs[buf] + lk * BP + li;
#pragma unroll
        for (int k4 = 0; k4 < S2_KC / 4; ++k4) {
            float a[2], b[NB];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[mi] = Ab[k4 * 4 * PI_AP + mi * 16];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) b[nb] = Bb[k4 * 4 * BP + nb * 16];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[mi][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi], b[nb], acc[mi][nb], 0, 0, 0);
        }
        if (more) store_chunk(buf ^ 1);   // the other buffer: its readers passed the barrier that ended the previous iteration
        __syncthreads();
    }

    // epilogue: lane (li, lk) holds pixels 4 lk + r (r < 4) of each m-block for output channel li of each n-block
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int oc = nt * BN + nb * 16 + li;
        if (oc >= p.OC) continue;
        const float sc = p.scale[oc], sh = p.shift[oc];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int om = mt * PI_BM + (wave * 2 + mi) * 16 + lk * 4 + r;
                if (om >= p.M) continue;
                const int n = om / OHW, rem = om - n * OHW;
                float v = acc[mi][nb][r] * sc + sh;
                if (p.act) v = leaky_relu(v, p.slope);
                p.out[(long long)n * p.out_bstride + (long long)oc * OHW + rem] = v;
            }
        }
    }
}

template <int KS>
int conv_s2_affine_launch(const S2Params& p, int nb, dim3 grid, hipStream_t stream) {
    return dispatch_nb(nb, [&](auto nbc) {
        hipLaunchKernelGGL((conv_s2_affine_kernel<KS, decltype(nbc)::value>), grid, dim3(256), 0, stream, p);
        return KBN_OK;
    });
}

// ---- pose head ------------------------------------------------------------------------------------------------------
constexpr int PH_THREADS = 256;

// Written without contraction: ops.pose_matrix evaluates every product and sum of the rotation as an operation of its own.
__device__ void pose_from_dof(const float* v, float* m) {
#pragma clang fp contract(off)
    const float r0 = v[0], r1 = v[1], r2 = v[2];
    const float angle = sqrtf((r0 * r0 + r1 * r1) + r2 * r2);
    const float d = angle + 1e-7f;
    const float x = r0 / d, y = r1 / d, z = r2 / d;
    const float ca = cosf(angle), sa = sinf(angle);
    const float c = 1.f - ca;
    const float xs = x * sa, ys = y * sa, zs = z * sa;
    const float xc = x * c, yc = y * c, zc = z * c;
    const float xyc = x * yc, yzc = y * zc, zxc = z * xc;
    m[0] = x * xc + ca;  m[1] = xyc - zs;      m[2] = zxc + ys;      m[3] = v[3];
    m[4] = xyc + zs;     m[5] = y * yc + ca;   m[6] = yzc - xs;      m[7] = v[4];
    m[8] = zxc - ys;     m[9] = yzc + xs;      m[10] = z * zc + ca;  m[11] = v[5];
    m[12] = 0.f;         m[13] = 0.f;          m[14] = 0.f;          m[15] = 1.f;
}

// Steps in a FIXED order, no atomics: (1) wave w sums channels w, w + 4, ...: lane l adds pixels l, l + 64, ... in order, then
// a butterfly over the wave (the same tree in every lane); (2) thread j < 6 runs over the channels in order; (3) / (h w);
// (4) x 0.01; (5) the matrix.  A frame's pose depends on that frame's latent and the weight alone.
__global__ __launch_bounds__(PH_THREADS) void pose_head_kernel(const float* __restrict__ latent, long long bstride,
                                                               const float* __restrict__ weight, float* __restrict__ pose,
                                                               float* __restrict__ dof, int C, int HW) {
    extern __shared__ float sums[];   // C channel sums, then 6 dof
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* x = latent + (long long)n * bstride;
    for (int c = wave; c < C; c += PH_THREADS / 64) {
        const float* plane = x + (long long)c * HW;
        float s = 0.f;
        for (int i = lane; i < HW; i += 64) s += plane[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) sums[c] = s;
    }
    __syncthreads();
    float* v = sums + C;
    if (threadIdx.x < 6) {
        const float* w = weight + threadIdx.x * C;
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(w[c], sums[c], s);
        s = s / (float)HW;
        s = 0.01f * s;
        v[threadIdx.x] = s;
        if (dof) dof[n * 6 + threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m[16];
        pose_from_dof(v, m);
#pragma unroll
        for (int i = 0; i < 16; ++i) pose[n * 16 + i] = m[i];
    }
}

}  // namespace
}  // namespace kbn

using namespace kbn;

static bool s2_kernel_size_ok(int ks) { return ks == 3 || ks == 5 || ks == 7; }

extern "C" size_t kbn_conv2d_s2_affine_packed_weight_bytes(int out_channels, int in_channels, int kernel_size) {
    if (out_channels <= 0 || in_channels <= 0 || !s2_kernel_size_ok(kernel_size)) return 0;
    return pose_igemm_packed_bytes(out_channels, (long long)in_channels * kernel_size * kernel_size, S2_KC);
}

extern "C" int kbn_conv2d_s2_affine_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                                                int kernel_size, kbn_stream_t stream) {
    return pose_igemm_pack_weight(weight, packed, out_channels, in_channels, kernel_size, S2_KC,
                                  kbn_conv2d_s2_affine_packed_weight_bytes(out_channels, in_channels, kernel_size), (hipStream_t)stream);
}

extern "C" int kbn_conv2d_s2_affine_forward(const kbn_conv_src* srcs, int n_src, const float* packed_weight, const float* scale,
                                            const float* shift, float* out, long long out_batch_stride, int n, int out_channels,
                                            int kernel_size, int in_height, int in_width, int apply_activation,
                                            float negative_slope, kbn_stream_t stream) {
    if (!srcs || !packed_weight || !scale || !shift || !out) return KBN_ERR_INVALID_ARGUMENT;
    if (n_src < 1 || n_src > 2 || n <= 0 || out_channels <= 0 || in_height <= 0 || in_width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    if (!s2_kernel_size_ok(kernel_size)) return KBN_ERR_UNSUPPORTED;
    S2Params p{};
    int ctot = 0;
    if (int rc = check_tensor_srcs(srcs, n_src, n, in_height, in_width, &ctot)) return rc;
    p.src0 = srcs[0].data;
    p.bs0 = srcs[0].batch_stride;
    p.C0 = srcs[0].channels;
    if (n_src == 2) { p.src1 = srcs[1].data; p.bs1 = srcs[1].batch_stride; }
    p.Ctot = ctot;
    p.OH = ceil_div(in_height, 2);
    p.OW = ceil_div(in_width, 2);
    const long long M = (long long)n * p.OH * p.OW;
    const long long K = (long long)ctot * kernel_size * kernel_size;
    if (M > 0x7fffffffLL - PI_BM || K > (1 << 24) || (long long)in_height * in_width > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    if (out_batch_stride < (long long)out_channels * p.OH * p.OW && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    p.wp = packed_weight;
    p.scale = scale;
    p.shift = shift;
    p.out = out;
    p.out_bstride = out_batch_stride;
    p.N = n;
    p.OC = out_channels;
    p.H = in_height;
    p.W = in_width;
    p.M = (int)M;
    p.K = (int)K;
    if (pose_igemm_packed_bytes(out_channels, K, S2_KC) == 0) return KBN_ERR_UNSUPPORTED;   // no blob exists for this shape
    p.nchunks = ceil_div((int)K, S2_KC);
    p.act = apply_activation ? 1 : 0;
    p.slope = negative_slope;
    const int nb = pose_igemm_nb(out_channels);
    const unsigned ntn = (unsigned)ceil_div(out_channels, 16 * nb);
    if (ntn > 65535u) return KBN_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)ceil_div((int)M, PI_BM), ntn);
    switch (kernel_size) {
        case 3: conv_s2_affine_launch<3>(p, nb, grid, (hipStream_t)stream); break;
        case 5: conv_s2_affine_launch<5>(p, nb, grid, (hipStream_t)stream); break;
        default: conv_s2_affine_launch<7>(p, nb, grid, (hipStream_t)stream); break;
    }
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_pose_head_forward(const float* latent, long long latent_batch_stride, const float* weight, float* pose,
                                     float* dof, int n, int channels, int height, int width, kbn_stream_t stream) {
    if (!latent || !weight || !pose) return KBN_ERR_INVALID_ARGUMENT;
    if (n <= 0 || channels <= 0 || height <= 0 || width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    const long long hw = (long long)height * width;
    if (hw > (1 << 24)) return KBN_ERR_UNSUPPORTED;             // (float)HW is exact below 2^24
    if (channels > 8192) return KBN_ERR_UNSUPPORTED;            // the channel sums live in LDS
    if (latent_batch_stride < channels * hw && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(pose_head_kernel, dim3((unsigned)n), dim3(PH_THREADS), (size_t)(channels + 6) * sizeof(float),
                       (hipStream_t)stream, latent, latent_batch_stride, weight, pose, dof, channels, (int)hw);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
