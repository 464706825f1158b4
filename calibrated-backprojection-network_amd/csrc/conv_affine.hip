// conv_affine.hip -- the conv and the pool of the ResNet-18/34 pose encoders and of the pose decoder's hidden layers, eval mode.
//
//   networks.ResNetEncoder     reference src/networks.py:674-996     conv1 7 x 7 stride 2, MaxPool2d(3, 2, 1), blocks2 .. blocks5
//   net_utils.ResNetBlock      reference src/net_utils.py:572-667    act(act(bn(conv2(act(bn(conv1(x)))))) + X), X = x or a 1 x 1 projection
//   net_utils.Conv2d           reference src/net_utils.py:51-141     bias-free conv, padding k / 2, then norm, then activation
//   networks.PoseDecoder       reference src/networks.py:1992-2075   n_filters = [256, 256]: two 3 x 3 stride-2 convs before the 1 x 1
//
// conv_affine_kernel<KS, STRIDE, NB>: the implicit GEMM of posenet.hip (conv_s2_affine_kernel; that kernel is left as it is) for
// k in {1, 3, 7} at stride 1 or 2, with a residual epilogue, on v_mfma_f32_16x16x4_f32 (exact fp32 products).
//   M = every output pixel of the BATCH in one index m = (frame * OH + oy) * OW + ox, 128 per workgroup;
//   N = output channels, 16 NB per workgroup (NB in {1, 2, 4} from the channel count);
//   K = (input channel, ky, kx) flattened, C k k, zero-padded to a multiple of CA_KC -- any channel count is legal.
// 256 threads = 4 waves; wave w owns m-blocks 2 w, 2 w + 1 (16 pixels each) times all NB n-blocks.
// K loop, CA_KC = 32 at a time (posenet.hip takes 16: a barrier and a gather latency per 16 -- DESIGN 8b; 32 halves both and
// still leaves two workgroups per CU): thread t gathers pixel t % 128 at k = t / 128 + 2 j (j < 16; k is wave-uniform, so the
// (channel, tap) decode is scalar) into registers while the MFMAs of the previous chunk run, then stores them to the other LDS
// buffer: one barrier per chunk.  Taps outside the image and k >= C k k are zero by predicate: no address outside the planes is
// formed into a load.  The packed weight is [n-tile][K chunk][CA_KC][16 NB], a straight copy.
// LDS (dynamic): A[2][CA_KC][144] + B[2][CA_KC][BP] floats.  The fragments are read with ds_read_b32, whose banks are the dword
// address mod 32 and whose lanes conflict inside a half-wave only: a half-wave reads k rows lk = 0, 1 (or 2, 3) x 16 consecutive
// floats, and pitches = 16 mod 32 (144; 16, 48, 80) put the two rows on disjoint 16-bank groups.  36 + at most 20 KiB: two
// workgroups per CU.
// Epilogue: v = acc * scale[oc] + shift[oc]; act; + residual; act (the second only with a residual).  `scale` is not folded into
// the weights: the conv itself then rounds as the reference's does.
//
// maxpool3x3s2_kernel: MaxPool2d(3, stride 2, padding 1), one thread per output, torch's update rule (v > m || isnan(v)).
#include "pose_igemm.h"

namespace kbn {
namespace {

constexpr int CA_KC = 32;
constexpr int CA_MAX_LDS = pose_igemm_lds_floats(CA_KC, 4) * (int)sizeof(float);

struct CAParams {
    const float* src0;
    const float* src1;
    long long bs0, bs1;
    int C0, Ctot;
    const float* wp;
    const float* scale;
    const float* shift;
    const float* residual;
    long long res_bstride;
    float* out;
    long long out_bstride;
    int N, OC, H, W, OH, OW;
    int M;        // N * OH * OW
    int K, nchunks;
    int act;
    float slope;
};

template <int KS, int STRIDE, int NB>
__global__ __launch_bounds__(256) void conv_affine_kernel(const CAParams p) {
    constexpr int KK = KS * KS, PAD = KS / 2, BN = 16 * NB, BP = pose_igemm_bp(NB);
    constexpr int NA = CA_KC / 2;                 // gathered values per thread and chunk
    constexpr int NW = CA_KC * BN / 256;          // weights per thread and chunk
    extern __shared__ float ca_lds[];
    float* const As = ca_lds;                     // [2][CA_KC * PI_AP]
    float* const Bs = ca_lds + 2 * CA_KC * PI_AP; // [2][CA_KC * BP]

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
        iy0 = STRIDE * oy - PAD;
        ix0 = STRIDE * ox - PAD;
    }
    const float* f0 = p.src0 + (long long)fn * p.bs0;
    const float* f1 = p.src1 ? p.src1 + (long long)fn * p.bs1 : nullptr;
    const float* wtile = p.wp + (long long)nt * p.nchunks * (CA_KC * BN);

    float va[NA];
    float vb[NW];
    auto load_chunk = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int k = chunk * CA_KC + khalf + 2 * j;      // wave-uniform
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
        const float* wc = wtile + (long long)chunk * (CA_KC * BN);
#pragma unroll
        for (int j = 0; j < NW; ++j) vb[j] = wc[tid + 256 * j];
    };
    auto store_chunk = [&](int buf) {
        float* Ab = As + buf * (CA_KC * PI_AP);
        float* Bb = Bs + buf * (CA_KC * BP);
#pragma unroll
        for (int j = 0; j < NA; ++j) Ab[(khalf + 2 * j) * PI_AP + pm] = va[j];
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int e = tid + 256 * j;
            Bb[(e / BN) * BP + (e % BN)] = vb[j];
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
        const float* Ab = As + buf * (CA_KC * PI_AP) + lk * PI_AP + wave * 32 + li;
        const float* Bb = Bs + buf * (CA_KC * BP) + lk * BP + li;
#pragma unroll
        for (int k4 = 0; k4 < CA_KC / 4; ++k4) {
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
                const long long plane = (long long)oc * OHW + rem;
                float v = acc[mi][nb][r] * sc + sh;
                if (p.act) v = leaky_relu(v, p.slope);
                if (p.residual) {
                    v += p.residual[(long long)n * p.res_bstride + plane];
                    if (p.act) v = leaky_relu(v, p.slope);
                }
                p.out[(long long)n * p.out_bstride + plane] = v;
            }
        }
    }
}

template <int KS, int STRIDE>
int conv_affine_launch(const CAParams& p, int nb, dim3 grid, hipStream_t stream) {
    return dispatch_nb(nb, [&](auto nbc) {
        constexpr int NB = decltype(nbc)::value;
        constexpr auto kernel = conv_affine_kernel<KS, STRIDE, NB>;
        if (int rc = set_max_dynamic_lds(lds_once<kernel>, reinterpret_cast<const void*>(kernel), CA_MAX_LDS)) return rc;
        hipLaunchKernelGGL(kernel, grid, dim3(256), (size_t)pose_igemm_lds_floats(CA_KC, NB) * sizeof(float), stream, p);
        return (int)KBN_OK;
    });
}

template <int KS>
int conv_affine_launch_stride(const CAParams& p, int stride, int nb, dim3 grid, hipStream_t stream) {
    return stride == 1 ? conv_affine_launch<KS, 1>(p, nb, grid, stream) : conv_affine_launch<KS, 2>(p, nb, grid, stream);
}

// ---- max pool ---------------------------------------------------------------------------------------------------------
// torch's rule (aten/src/ATen/native/cpu/MaxPoolKernel.cpp, the same on the device): start at -inf, take v when v > m or v is
// NaN -- a NaN in the window wins and stays; taps outside the image are skipped, they never win.
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* __restrict__ in, long long in_bstride, float* __restrict__ out,
                                                           long long out_bstride, int C, int H, int W, int OH, int OW,
                                                           long long total) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int ox = (int)(i % OW);
        long long t = i / OW;
        const int oy = (int)(t % OH);
        t /= OH;
        const int c = (int)(t % C);
        const long long n = t / C;
        const float* plane = in + n * in_bstride + (long long)c * H * W;
        float m = -__builtin_inff();
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                const float v = plane[iy * W + ix];
                if (v > m || v != v) m = v;
            }
        }
        out[n * out_bstride + ((long long)c * OH + oy) * OW + ox] = m;
    }
}

}  // namespace
}  // namespace kbn

using namespace kbn;

static bool ca_kernel_size_ok(int ks) { return ks == 1 || ks == 3 || ks == 7; }

extern "C" size_t kbn_conv2d_affine_packed_weight_bytes(int out_channels, int in_channels, int kernel_size) {
    if (out_channels <= 0 || in_channels <= 0 || !ca_kernel_size_ok(kernel_size)) return 0;
    return pose_igemm_packed_bytes(out_channels, (long long)in_channels * kernel_size * kernel_size, CA_KC);
}

extern "C" int kbn_conv2d_affine_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                                             int kernel_size, kbn_stream_t stream) {
    return pose_igemm_pack_weight(weight, packed, out_channels, in_channels, kernel_size, CA_KC,
                                  kbn_conv2d_affine_packed_weight_bytes(out_channels, in_channels, kernel_size), (hipStream_t)stream);
}

extern "C" int kbn_conv2d_affine_forward(const kbn_conv_src* srcs, int n_src, const float* packed_weight, const float* scale,
                                         const float* shift, const float* residual, long long residual_batch_stride, float* out,
                                         long long out_batch_stride, int n, int out_channels, int kernel_size, int stride,
                                         int in_height, int in_width, int apply_activation, float negative_slope,
                                         kbn_stream_t stream) {
    if (!srcs || !packed_weight || !scale || !shift || !out) return KBN_ERR_INVALID_ARGUMENT;
    if (n_src < 1 || n_src > 2 || n <= 0 || out_channels <= 0 || in_height <= 0 || in_width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    if (!ca_kernel_size_ok(kernel_size) || (stride != 1 && stride != 2)) return KBN_ERR_UNSUPPORTED;
    CAParams p{};
    int ctot = 0;
    if (int rc = check_tensor_srcs(srcs, n_src, n, in_height, in_width, &ctot)) return rc;
    p.src0 = srcs[0].data;
    p.bs0 = srcs[0].batch_stride;
    p.C0 = srcs[0].channels;
    if (n_src == 2) { p.src1 = srcs[1].data; p.bs1 = srcs[1].batch_stride; }
    p.Ctot = ctot;
    p.OH = ceil_div(in_height, stride);
    p.OW = ceil_div(in_width, stride);
    const long long M = (long long)n * p.OH * p.OW;
    const long long K = (long long)ctot * kernel_size * kernel_size;
    if (M > 0x7fffffffLL - PI_BM || K > (1 << 24) || (long long)in_height * in_width > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    const long long frame = (long long)out_channels * p.OH * p.OW;
    if (out_batch_stride < frame && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    if (residual && residual_batch_stride < frame && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    p.wp = packed_weight;
    p.scale = scale;
    p.shift = shift;
    p.residual = residual;
    p.res_bstride = residual_batch_stride;
    p.out = out;
    p.out_bstride = out_batch_stride;
    p.N = n;
    p.OC = out_channels;
    p.H = in_height;
    p.W = in_width;
    p.M = (int)M;
    p.K = (int)K;
    if (pose_igemm_packed_bytes(out_channels, K, CA_KC) == 0) return KBN_ERR_UNSUPPORTED;   // no blob exists for this shape
    p.nchunks = ceil_div((int)K, CA_KC);
    p.act = apply_activation ? 1 : 0;
    p.slope = negative_slope;
    const int nb = pose_igemm_nb(out_channels);
    const unsigned ntn = (unsigned)ceil_div(out_channels, 16 * nb);
    if (ntn > 65535u) return KBN_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)ceil_div((int)M, PI_BM), ntn);
    int rc;
    switch (kernel_size) {
        case 1: rc = conv_affine_launch_stride<1>(p, stride, nb, grid, (hipStream_t)stream); break;
        case 3: rc = conv_affine_launch_stride<3>(p, stride, nb, grid, (hipStream_t)stream); break;
        default: rc = conv_affine_launch_stride<7>(p, stride, nb, grid, (hipStream_t)stream); break;
    }
    if (rc != KBN_OK) return rc;
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}

extern "C" int kbn_maxpool3x3s2_forward(const float* in, long long in_batch_stride, float* out, long long out_batch_stride, int n,
                                        int channels, int height, int width, kbn_stream_t stream) {
    if (!in || !out) return KBN_ERR_INVALID_ARGUMENT;
    if (n <= 0 || channels <= 0 || height <= 0 || width <= 0) return KBN_ERR_INVALID_ARGUMENT;
    if ((long long)height * width > 0x7fffffffLL) return KBN_ERR_UNSUPPORTED;
    const int oh = ceil_div(height, 2), ow = ceil_div(width, 2);
    if (in_batch_stride < (long long)channels * height * width && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    if (out_batch_stride < (long long)channels * oh * ow && n > 1) return KBN_ERR_INVALID_ARGUMENT;
    if ((long long)channels * oh * ow > 0x7fffffffffffLL / n) return KBN_ERR_UNSUPPORTED;
    const long long total = (long long)n * channels * oh * ow;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0,
                       (hipStream_t)stream, in, in_batch_stride, out, out_batch_stride, channels, height, width, oh, ow, total);
    KBN_CHECK_LAUNCH();
    return KBN_OK;
}
