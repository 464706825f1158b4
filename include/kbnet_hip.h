/*
 * kbnet_hip.h -- C ABI of the MI355X (gfx950) KBNet inference hot path.
 *
 * The reference (alexklwong/calibrated-backprojection-network) is pure Python on
 * PyTorch and has no FFI of its own; the entry points below are what a binding for
 * its hot path would call, one per reference operator.  Each declaration cites the
 * reference interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - every tensor is fp32, NCHW, W-contiguous, device (HBM) memory owned by the
 *     caller; the library allocates nothing and keeps no pointer after return;
 *   - every call only enqueues work on `stream` (a hipStream_t of the calling thread's
 *     current device) and returns: no synchronisation, no timing, no file I/O -- unless
 *     the caller has switched first-use tuning on (kbn_set_autotune, OFF by default);
 *   - return value: KBN_OK (0) or a negative kbn_status; nothing throws across the ABI;
 *   - the library is re-entrant and multi-device: its only process state is (a) one-time
 *     kernel attribute setup, done per device, (b) the debug knobs, read from the
 *     environment once at load time (kbn_reload_env re-reads them), (c) the launch-geometry
 *     cache, per device, written only while tuning is on.
 */
#ifndef KBNET_HIP_H
#define KBNET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KBN_ABI_VERSION 11

typedef void* kbn_stream_t; /* hipStream_t */

typedef enum kbn_status {
    KBN_OK = 0,
    KBN_ERR_INVALID_ARGUMENT = -1, /* null pointer, non-positive size, bad enum      */
    KBN_ERR_UNSUPPORTED = -2,      /* legal for the reference, outside kernel limits */
    KBN_ERR_WORKSPACE = -3,        /* caller-provided buffer too small               */
    KBN_ERR_LAUNCH = -4            /* HIP reported a launch error                    */
} kbn_status;

int kbn_version(void);
const char* kbn_status_string(int status);

/* Re-reads the KBN_* debug / experiment variables and KBN_TUNE_CACHE from the environment
 * (they are otherwise read once, when the library is loaded; no launch path calls getenv). */
void kbn_reload_env(void);

/* Value of a KBN_* switch AS THE LIBRARY READ IT (at load time / the last kbn_reload_env()): 0 when unset or unknown.  The
 * host mirror asks here instead of reading the environment itself, so its A/B switches (KBN_NO_SPLIT, KBN_NO_PAIR,
 * KBN_NO_PAIR_MID, KBN_NO_PAIR_ENC, KBN_NO_PAIR_TAIL, KBN_NO_OVERLAP, KBN_DEPTH_FRONT_FUSION, KBN_NO_DEPTH_FRONT_FUSION,
 * KBN_FP16_ONE_TERM, KBN_NO_FRONT_NEXT) change together with the library's.  Values are integers (atoi); a variable that is set to
 * something that is not a number ("true", "yes", "on") reads as 1, so that KBN_NO_PAIR=true still switches the path off. */
int kbn_knob(const char* name);

/* First-use tuning of launch geometry (tile / region shapes; csrc/tune.hip).  OFF by default:
 * calls launch the analytic choice or a cached one.  While ON, the first call of a problem
 * shape on a device times every candidate geometry on `stream` and waits for its own events --
 * results are bit-identical whatever is picked -- so switch it on only around a warm-up pass:
 *     kbn_set_autotune(1); <one forward per shape>; kbn_set_autotune(0);
 * Never tunes while `stream` is being captured.  KBN_AUTOTUNE=1 in the environment at load time
 * is the same switch; KBN_TUNE_CACHE=<file> preloads / records choices.  Returns the old state. */
int kbn_set_autotune(int enabled);
int kbn_get_autotune(void);

/* ------------------------------------------------------------------ S2D -------
 * networks.SparseToDensePool.forward(x)            reference src/networks.py:2168-2196
 * (pool construction :2112-2132, 1x1 convs :2138-2152, 3x3 conv :2156-2166).
 *
 *   x              N x input_channels x H x W; channel 0 is the sparse depth
 *   w_pool_convs   n_convolution pointers: [0] is n_filter x (n_min+n_max) x 1 x 1,
 *                  the others n_filter x n_filter x 1 x 1  (pool_convs.{i}.conv.weight)
 *   w_conv         n_filter x (n_filter+input_channels) x 3 x 3   (conv.conv.weight)
 *   out            N x n_filter x H x W
 *   pool sizes     odd kernel sizes > 1 (the caller drops sizes <= 1 like the
 *                  reference does); min pools ignore zeros (999 sentinel semantics)
 * Limits: n_filter <= 8, input_channels <= 2, n_min+n_max <= 8, n_convolution <= 4,
 *         pool size <= 31 and odd.
 */
int kbn_s2d_forward(const float* x, const float* const* w_pool_convs, const float* w_conv,
                    float* out, int n, int height, int width, int input_channels,
                    const int* min_pool_sizes, int n_min, const int* max_pool_sizes, int n_max,
                    int n_convolution, int n_filter, float negative_slope, kbn_stream_t stream);

/* Optional debug/parity output of the min/max pyramid alone (the tensor the
 * reference concatenates at src/networks.py:2189): N x (n_min+n_max) x H x W. */
int kbn_s2d_pyramid(const float* x_depth, long long batch_stride, float* pyramid, int n,
                    int height, int width, const int* min_pool_sizes, int n_min,
                    const int* max_pool_sizes, int n_max, kbn_stream_t stream);

/* ----------------------------------------------------------- intrinsics --------
 * KBNetEncoder.forward closures scale_intrinsics + torch.inverse
 *                                                  reference src/networks.py:328, 333-352
 * kinv[n] = inverse(K[n] (.) [[sx,1,sx],[1,sy,sy],[1,1,1]]); pass sx = sy = 1 for level 0.
 */
int kbn_intrinsics_inverse(const float* intrinsics, float* kinv, int n, float scale_x,
                           float scale_y, kbn_stream_t stream);

/* camera_coordinates closure + net_utils.meshgrid   reference src/networks.py:317-331,
 * src/net_utils.py:1601-1636.  coordinates: N x 3 x H x W = kinv . [x y 1]^T. */
int kbn_camera_coordinates(const float* kinv, float* coordinates, int n, int height, int width,
                           kbn_stream_t stream);

/* ------------------------------------------------------------- conv2d ----------
 * net_utils.Conv2d.forward (bias-free conv, padding k//2, optional LeakyReLU)
 *                                                  reference src/net_utils.py:85-93, 120-141
 * fused with the ops the reference runs around it:
 *   - torch.cat of the inputs along channels (src/net_utils.py:1351, 1366, 1483):
 *     up to KBN_MAX_SRC sources, concatenated in order;
 *   - UpConv2d's nearest interpolate (src/net_utils.py:497): KBN_RESIZE_NEAREST
 *     (only with a single tensor source);
 *   - the KB layer's coordinate / backprojection channels (src/net_utils.py:1351-1360),
 *     synthesized while the input tile is staged (source kinds below).
 */
#define KBN_MAX_SRC 3

typedef enum kbn_src_kind {
    KBN_SRC_TENSOR = 0, /* data: N x channels x src_height x src_width                     */
    KBN_SRC_COORDS = 1, /* 3 channels kinv.[x y 1]^T, kinv: N x 3 x 3 (data unused)        */
    KBN_SRC_XYZ = 2,    /* 3 channels coords * z, z = act(proj_weight . depth[:, y, x]);   */
                        /* data = depth N x aux_channels x H x W, proj_weight = aux_channels */
                        /* floats, coords from `coordinates` (N x 3 x H x W) if non-null,  */
                        /* else from kinv                                                  */
    KBN_SRC_PAIR = 3    /* a PAIR tensor (below): activations already split into two fp16 terms by  */
                        /* their producer; kbn_conv3x3_split_forward only, source 0 only            */
} kbn_src_kind;

typedef struct kbn_conv_src {
    int kind;               /* kbn_src_kind                                       */
    int channels;           /* channels this source contributes to the concat     */
    const float* data;
    long long batch_stride; /* elements between consecutive frames of `data`      */
    int src_height, src_width; /* size of `data` planes (KBN_SRC_TENSOR)          */
    int aux_channels;       /* KBN_SRC_XYZ: channels of the depth feature tensor  */
    const float* proj_weight;  /* KBN_SRC_XYZ                                     */
    const float* coordinates;  /* KBN_SRC_XYZ, optional                           */
    long long coordinates_batch_stride;
    const float* kinv;      /* KBN_SRC_COORDS / KBN_SRC_XYZ without coordinates    */
    const unsigned* absmax; /* KBN_SRC_TENSOR / KBN_SRC_PAIR, optional: the per-frame max |a| slots of this tensor
                             * (see "activation statistics" below); read by the split-operand convs only  */
    const float* scale;     /* KBN_SRC_PAIR: the per-frame 2^k its producer wrote (pair_out_scale)         */
} kbn_conv_src;

/* ------------------------------------------------ PAIR tensors (producer-written split operands) --
 * The reference passes fp32 tensors between its convs (src/net_utils.py:1483-1487: conv over cat[deconv, skip]).  Where a
 * tensor is read ONLY by split-operand convs -- the decoder's up-conv outputs and concat-conv outputs -- the producer
 * can write the two fp16 terms itself, once, instead of every consumer splitting every value it stages (2.4-4.8 times
 * per value: halos x filter tiles).  Layout per frame, C channels (C % 8 == 0), H x W pixels:
 *     [k-group = channel / 8][term: h1 | h2][H * W + 1 pixels][8 channels] fp16      (4 bytes per value, like fp32)
 * a 2^k = h1 + 2^-11 h2; the extra pixel that ends every plane is ZERO (written by the producer; a consumer's halo pixels
 * outside the map read it).  Frames are batch_stride fp16 elements apart (>= (C / 8) * 2 * (H * W + 1) * 8, a multiple
 * of 8; base 16-byte aligned).  k is chosen per frame by the producer from a bound of its output -- (max |a| of each
 * input, from the inputs' absmax slots) x (a table of weight norms kept behind the packed weights) -- and written to
 * `pair_out_scale[frame]` as the float 2^k; the consumer receives that array as kbn_conv_src.scale.  The producer still
 * folds the true max |out| into out_absmax.  kbn_conv3x3_split_forward: `pair_out` for modes 0 and 2 and for mode 3 with whole
 * 64-filter tiles (needs absmax slots on every source and out_channels % 8 == 0; mode 3 with at most 16 filters writes 16 channels, zeros past out_channels); a KBN_SRC_PAIR source 0 for mode 0
 * (beside an fp32 source 1), mode 2 (one source) and mode 3 (64-filter tiles, or at most 16 filters and channels % 32 == 0); KBN_ERR_UNSUPPORTED otherwise -- the
 * caller then keeps the tensor in fp32. */

/* ----------------------------------------------- activation statistics ("absmax slots") --
 * The split-operand convs further down represent an activation as two fp16 terms under a per-frame
 * exponent, which has to follow the magnitude of the data.  It does so on the device: a SLOT is an array of
 * n unsigned values, one per frame, holding the bit pattern of max |a| over that frame of a tensor
 * (bit patterns of non-negative floats order like the floats).  Every conv entry point takes `out_absmax`
 * (may be NULL): the kernel folds the values it stores into out_absmax[frame] with an atomic max in its epilogue
 * (several launches may fill channel slices of one tensor into one slot); the caller zeroes a slot before its first
 * producer.  A consumer is handed the slot through kbn_conv_src.absmax.  kbn_absmax_frames is the stand-alone
 * pass for tensors that come from elsewhere.  No host synchronisation, no state between calls: the result of a
 * forward is a function of its inputs and weights alone, frame by frame (the reference's convs are exactly
 * that: src/net_utils.py:120-141). */
int kbn_absmax_frames(const float* x, long long batch_stride, int n, long long per_frame, unsigned* slots,
                      kbn_stream_t stream);

#define KBN_RESIZE_NONE 0
#define KBN_RESIZE_NEAREST 1

/* ----------------------------------------------- the size functions and their argument ranges --
 * Every size_t-returning function of this header is pure host arithmetic (no launch, no device pointer followed), takes any int
 * and answers 0 for what its kernels do not support: a dimension <= 0, a kernel size, stride, mode, channel count or bit width that
 * is not one of the legal ones named beside it, or a shape past the common range below.  A caller allocates what a NONZERO answer
 * says and treats 0 as a refusal, never as "allocate nothing"; the pack and forward entry points refuse the same shapes
 * (KBN_ERR_UNSUPPORTED or KBN_ERR_INVALID_ARGUMENT).  tests/host_san/size_sweep.cpp sweeps them all over extreme arguments
 * in a sanitizer build.
 * The common range of the conv layers: 1 <= out_channels, in_channels <= KBN_MAX_CHANNELS and out_channels x in_channels x k x k
 * <= KBN_MAX_WEIGHT_ELEMENTS (1 GiB of fp32 OIHW weights); the plans behind the kernels are computed in int. */
#define KBN_MAX_CHANNELS 1048576
#define KBN_MAX_WEIGHT_ELEMENTS 268435456
/* A map side the weight-gradient scratch functions take (its pixels must also fit an int), and the largest answer any size
 * function gives: a product of the arguments past it is answered with 0, not with its low 64 bits. */
#define KBN_MAX_MAP_SIDE 16777216
#define KBN_MAX_SIZE_BYTES ((size_t)1 << 62)

/* Bytes of the packed weight blob for a conv with these dimensions (0 if unsupported).  The
 * blob layout depends on the stride the weight will be used with.  kernel_size 1 or 3, stride 1 or 2, channels in the common range. */
size_t kbn_conv2d_packed_weight_bytes(int out_channels, int in_channels, int kernel_size, int stride);

/* Re-orders an OIHW weight (out_channels x in_channels x k x k) into the MFMA
 * fragment order the kernel consumes.  `packed` must hold
 * kbn_conv2d_packed_weight_bytes(...) bytes.  Do this once per weight (and stride).  For wide
 * 3x3 stride-1 convs the blob also carries the Winograd-domain weights G g G^T behind the
 * fragment-order copy; kbn_conv2d_forward picks the kernel per launch. */
int kbn_conv2d_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                           int kernel_size, int stride, kbn_stream_t stream);

/* out[n, :, oy, ox] = act(sum_c,ky,kx W[:, c, ky, kx] * in[n, c, oy*stride+ky-pad, ox*stride+kx-pad])
 * where `in` is the channel concat of the sources, logically in_height x in_width
 * (sources are nearest-resized to that size first when resize = KBN_RESIZE_NEAREST).
 * out: frames `out_batch_stride` elements apart (lets the caller write straight into a
 * channel slice of a larger skip tensor), out_channels x ceil(in_h/stride) x ceil(in_w/stride).
 * kernel_size in {1, 3}; stride in {1, 2}.  out_absmax: n slots of max |out| per frame, or NULL. */
int kbn_conv2d_forward(const kbn_conv_src* srcs, int n_src, const float* packed_weight, float* out,
                       long long out_batch_stride, int n, int out_channels, int kernel_size,
                       int stride, int in_height, int in_width, int resize, int apply_activation,
                       float negative_slope, unsigned* out_absmax, kbn_stream_t stream);

/* --------------------------------------------- layer-by-layer form: activation, backprojection -------
 * The fused kernels are written around max(v, slope v): LeakyReLU(0.20), ReLU (slope 0) and -- with slope 1 -- no activation.
 * net_utils.activation_func also builds torch.nn.ELU() and torch.nn.Sigmoid() (reference src/net_utils.py:38-43; run_kbnet.py
 * --activation_func elu | sigmoid).  A model with one of those runs layer by layer: every conv is launched WITHOUT activation
 * (apply_activation = 0) and followed by kbn_activation_forward in place; the KB block's z = act(proj_depth . depth)
 * (:1352-1355) is then a tensor of its own and xyz = coordinates * z (:1357-1359) one kbn_scale_planes_forward.
 *   kbn_activation_forward    x: n frames of per_frame contiguous floats, batch_stride apart; kind KBN_ACT_ELU (v > 0 ? v :
 *                             expm1(v), alpha = 1) or KBN_ACT_SIGMOID (1 / (1 + exp(-v))); out_absmax (may be NULL): the per-frame
 *                             max |a| slots of the tensor (above), which receive the maxima of the ACTIVATED values -- the convs in
 *                             front of this pass are given no slot
 *   kbn_scale_planes_forward  out[n, c, y, x] = x[n, c, y, x] * z[n, 0, y, x], c < channels; dense planes, frames *_batch_stride apart */
enum { KBN_ACT_ELU = 1, KBN_ACT_SIGMOID = 2 };
int kbn_activation_forward(float* x, long long batch_stride, int n, long long per_frame, int kind, unsigned* out_absmax,
                           kbn_stream_t stream);
int kbn_scale_planes_forward(const float* x, long long x_batch_stride, const float* z, long long z_batch_stride, float* out,
                             long long out_batch_stride, int n, int channels, int height, int width, kbn_stream_t stream);

/* ------------------------------------------------------------ up-conv 2x -------
 * net_utils.UpConv2d.forward when the target size is exactly twice the input:
 * interpolate(nearest) + conv3x3 (+ activation)       reference src/net_utils.py:484-499
 * evaluated as four 2x2 convs on the low-resolution input (one per output phase) with
 * pre-summed weights: 4 instead of 9 MACs per output and input channel, no upsampled tensor;
 * maps with 16-byte aligned rows go further: with differences of neighbouring input pixels the
 * two phases of an axis share a product (o0 = -g0 (in[x]-in[x-1]) + G in[x], o1 = g2 (in[x+1]-in[x])
 * + G in[x], G = g0+g1+g2): 3 or 2.25 MACs per output and input channel (csrc/conv_up2x.hip).
 *   src   N x in_channels x src_height x src_width (frames src_batch_stride apart)
 *   out   N x out_channels x 2*src_height x 2*src_width (frames out_batch_stride apart)
 *   packed_weight from kbn_upconv2x_pack_weight (OIHW 3x3 weight in; the blob holds the 4-phase,
 *   the 3-product and, for <= 16 or a multiple of 32 filters, the 9-product weights back to back).
 * Other target sizes go through kbn_conv2d_forward(..., KBN_RESIZE_NEAREST). */
/* range: channels in the common range (kernel 3 x 3); 0 otherwise */
size_t kbn_upconv2x_packed_weight_bytes(int out_channels, int in_channels);
int kbn_upconv2x_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                             kbn_stream_t stream);
int kbn_upconv2x_forward(const float* src, long long src_batch_stride, const float* packed_weight,
                         float* out, long long out_batch_stride, int n, int in_channels,
                         int out_channels, int src_height, int src_width, int apply_activation,
                         float negative_slope, unsigned* out_absmax, kbn_stream_t stream);

/* Which algebraic form kbn_upconv2x_forward runs for a problem (diagnostics, roofline accounting):
 * info[4] = {channel products per low-resolution pixel: 16 four 2x2 phases / 12 three-product columns /
 * 9 three-product rows and columns; padded output channels; padded input channels; 0}.  The launch
 * executes 2 * n * src_height * src_width * info[0] * info[1] * info[2] FLOP on the matrix cores. */
int kbn_upconv2x_query(int n, int in_channels, int out_channels, int src_height, int src_width, int* info);

/* ------------------------------------------------------- transposed conv 2x -------
 * net_utils.TransposeConv2d.forward -- the decoder blocks' up-sampling layer with deconv_type='transpose'
 * (run_kbnet.py --deconv_type transpose; reference src/net_utils.py:350-440, DecoderBlock :1468-1469):
 * torch.nn.ConvTranspose2d(in, out, kernel_size=3, stride=2, padding=1, output_padding=1, bias=False) (+ activation),
 *     out[n, o, 2i - 1 + ky, 2j - 1 + kx] += src[n, c, i, j] w[c, o, ky, kx],    output exactly 2 src_height x 2 src_width.
 * By output parity this is four small convs on the source (1, 2, 2 and 4 taps), i.e. the four-phase form of the up-conv
 * above with nine of its sixteen phase weights taken from w and seven zero: same kernels, same blob size
 * (kbn_upconv2x_packed_weight_bytes), always the four-phase form.
 *   weight  out_channels x in_channels x 3 x 3: the module's in x out x 3 x 3 parameter with its first two axes swapped
 *           (the Python mirror does that: ops.pack_upconv2x_weight(transposed=True)). */
int kbn_deconv2x_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                             kbn_stream_t stream);
int kbn_deconv2x_forward(const float* src, long long src_batch_stride, const float* packed_weight,
                         float* out, long long out_batch_stride, int n, int in_channels,
                         int out_channels, int src_height, int src_width, int apply_activation,
                         float negative_slope, unsigned* out_absmax, kbn_stream_t stream);

/* ------------------------------- fp32-grade 3x3 convs on the 16-bit matrix core --
 * gfx950 executes fp32 MFMAs on the fp32 vector datapath (157 TFLOP/s); the matrix core proper takes
 * 16-bit operands (2.5 PFLOP/s dense).  These entry points feed it fp32 operands as pairs of fp16 values:
 * a 2^k = h1 + 2^-11 h2 (activations, split in the kernel), w 2^e = w1 + w2 (weights, split at pack time,
 * e per filter), a w = 2^-(e+k) (h1 w1 + h1 w2 + h2 (w1 2^-11)) up to 2^-22 |a w|: three fp16 MFMAs with fp32
 * accumulation per product, 3/16 of the fp32 MFMA's time, errors measured against fp64 no larger than the
 * fp32 MFMA chain's (profiles/r02/bf16x_probe.txt).  They ARE on the parity-gated path: the stride-1 3x3
 * convs of the decoder (reference src/net_utils.py:484-499 nearest-2x + conv, :1483-1487 conv over
 * cat[deconv, skip]) and the stride-2 image convs of the KB blocks run through them when the shape
 * qualifies.
 *   act_exponent  k: places the fp16 window on the activations: |a| 2^k must stay below 65504 (beyond: inf),
 *             |a| 2^k >= 2^-14 keeps the full 22 bits, smaller activations are carried by the scaled residual
 *             alone (absolute error below 2^-40 of the window's top).  USED ONLY WHEN A SOURCE HAS NO absmax SLOT:
 *             with slots on every source the kernel derives k per frame from the data, max |a| 2^k in [2^14, 2^15)
 *             (the Python mirror always provides slots; a static k is for callers that know their range: -6
 *             covers 0.0039 .. 4.2e6).  Range -60 .. 60.
 *   mode      0: 3x3 stride 1 over height x width sources; 1: nearest-2x up-conv in its nine-tap form (ONE source with
 *             (height/2) x (width/2) planes; no longer built since ABI 7: KBN_ERR_UNSUPPORTED, use mode 3); 2: 3x3 stride 2 (source planes h x w with ceil(h/2) = height,
 *             ceil(w/2) = width: the image convs of the KB blocks, reference src/net_utils.py:1348); 3: mode 1 in its folded
 *             form (four 2x2 convs on the low-resolution source, 16 instead of 36 channel products per source pixel: what the
 *             decoder runs); 4: ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1) -- deconv_type='transpose',
 *             reference src/net_utils.py:383-390 -- on mode 3's kernels (nine of the sixteen folded weights are the layer's taps,
 *             seven are zero; `weight` for kbn_conv3x3_split_pack_weight: out x in x 3 x 3, the module's parameter with its
 *             first two axes swapped); whatever this text says of mode 3 holds for mode 4
 *   srcs      1 or 2 KBN_SRC_TENSOR sources, each a multiple of 16 channels; source 0 may be a KBN_SRC_PAIR (above)
 *   pair_out  NULL, or the output as a PAIR tensor (then `out` is ignored and may be NULL), with
 *             pair_out_batch_stride (fp16 elements) and pair_out_scale (n floats).  Mode 2 with pair_out (one source): a
 *             non-NULL `out` receives, in fp32, the output pixels (2y, 2x) only, as N x out_channels x ceil(height / 2) x
 *             ceil(width / 2) -- what the next KB level's 1x1 stride-2 conv_fused reads of this tensor
 *             (kbn_conv1x1s2_split_forward takes it as a pre-subsampled source 0)
 *   packed    from kbn_conv3x3_split_pack_weight (OIHW fp32 3x3 weight in) for the SAME mode (the
 *             filter tiling of the blob depends on it)
 *   out       N x out_channels x height x width fp32, frames out_batch_stride elements apart
 * Modes 1 and 3 return KBN_ERR_UNSUPPORTED unless width % 4 == 0 and `out` is 16-byte aligned (callers fall back
 * to kbn_upconv2x_forward); modes 0 and 2 store element-wise in that case.  KBN_NO_SPLIT=1: always unsupported. */
/* range: mode 0 .. 4, in_channels % 16 == 0, channels in the common range; 0 otherwise */
size_t kbn_conv3x3_split_packed_weight_bytes(int out_channels, int in_channels, int mode);
int kbn_conv3x3_split_pack_weight(const float* weight, void* packed, int out_channels, int in_channels, int mode,
                                  kbn_stream_t stream);
int kbn_conv3x3_split_forward(const kbn_conv_src* srcs, int n_src, const void* packed_weight, float* out,
                              long long out_batch_stride, int n, int out_channels, int height, int width, int mode,
                              int act_exponent, int apply_activation, float negative_slope, unsigned* out_absmax,
                              void* pair_out, long long pair_out_batch_stride, float* pair_out_scale, kbn_stream_t stream);
/* The LATENCY form of modes 0 and 2 (round 6): the same conv (reference src/net_utils.py:1483-1487 / :1348, net_utils.Conv2d.forward
 * :120-141) for launches whose tiles cannot fill the chip -- one KITTI frame gives deconv4's conv (768 -> 256 at 22 x 76) 24 workgroups
 * of 48 K-chunks each on 256 CUs.  `ksplit` workgroups share every tile, each summing a contiguous range of the 16-channel chunks
 * into a plane set of its own in `workspace` (ksplit x n x out_channels x height x width floats, 16-byte aligned), and a second kernel
 * adds the sets in split order, applies the activation and fills out_absmax.  fp32 KBN_SRC_TENSOR sources only, no pair output.
 * The result differs from kbn_conv3x3_split_forward's in summation order (same 1e-4 bar, other low bits), so a model uses one form
 * throughout (KBNetModel.latency_mode).  ksplit = 1 is kbn_conv3x3_split_forward; 1 <= ksplit <= in_channels / 16 with no empty range
 * (ceil(chunks / ksplit) * (ksplit - 1) < chunks), else KBN_ERR_INVALID_ARGUMENT. */
int kbn_conv3x3_split_forward_ksplit(const kbn_conv_src* srcs, int n_src, const void* packed_weight, float* out,
                                     long long out_batch_stride, int n, int out_channels, int height, int width, int mode,
                                     int act_exponent, int apply_activation, float negative_slope, unsigned* out_absmax,
                                     int ksplit, float* workspace, kbn_stream_t stream);

/* conv_fused of the KB block on split operands -- reference src/net_utils.py:1337-1343 (Conv2d(in_channels_fused + 3,
 * n_filter_fused, kernel_size=1, stride=2)) applied to cat[image, xyz, fused] (:1352-1368).  The tensor channels
 * (image, fused: one or two KBN_SRC_TENSOR sources of H x W planes, channels % 16 == 0; with two sources, source 0 may
 * instead hold only the pixels the conv reads: src_height x src_width = the OUTPUT size) are taken through the 16-bit
 * matrix core like the 3x3 convs above; the three backprojection channels xyz = K^-1 [x y 1]^T z, z =
 * act(proj_depth . depth) (:1352-1359), are computed once per block at the positions a stride-2 1x1 conv reads
 * (kbn_kb_xyz_s2_forward: xyz[:, :, y, x] belongs to input pixel (2y, 2x)) and enter in fp32.
 *   weight    out_channels x in_channels fp32 (the 1x1 OIHW weight), in_channels = tensor channels (+ 3);
 *             xyz_offset = index of the first of the three xyz input channels (channels of `image`), -1: none
 *   packed    kbn_conv1x1s2_split_packed_weight_bytes(out_channels, tensor_channels, has_xyz) bytes
 *   xyz       N x 3 x height x width fp32 (output size), frames xyz_batch_stride apart; null iff packed without xyz
 *   out       N x out_channels x height x width, height = ceil(H / 2), width = ceil(W / 2) */
/* range: tensor_channels % 16 == 0, channels in the common range; 0 otherwise */
size_t kbn_conv1x1s2_split_packed_weight_bytes(int out_channels, int tensor_channels, int has_xyz);
int kbn_conv1x1s2_split_pack_weight(const float* weight, void* packed, int out_channels, int in_channels, int xyz_offset,
                                    kbn_stream_t stream);
int kbn_conv1x1s2_split_forward(const kbn_conv_src* srcs, int n_src, const void* packed_weight, const float* xyz,
                                long long xyz_batch_stride, float* out, long long out_batch_stride, int n, int out_channels,
                                int height, int width, int act_exponent, int apply_activation, float negative_slope,
                                unsigned* out_absmax, kbn_stream_t stream);
int kbn_kb_xyz_s2_forward(const float* depth, long long depth_batch_stride, int depth_channels, int height, int width,
                          const float* proj_weight, const float* kinv, int apply_activation, float negative_slope, float* xyz,
                          long long xyz_batch_stride, int n, kbn_stream_t stream);


/* Which kernel variant / tile geometry kbn_conv2d_forward picks for a problem (diagnostics,
 * profiling): info[8] = {CK, NB, MW, TWB, TH, workgroups, staged positions per thread, kernel};
 * kernel 2 = conv_dma_kernel<kernel_size, stride, CK, NB, MW, ...> (LDS-DMA staging; needs
 * W % 4 == 0, 16-byte aligned planes, no resize), 1 / 0 = conv_igemm_kernel<...> with / without
 * register prefetch, 3 = conv_wino_kernel (Winograd F(2x2,3x3) for 3x3 stride-1 convs with
 * in_channels % 16 == 0, in_channels >= 32, out_channels >= 32, every source a multiple of 8 channels and the conv_dma alignment rules;
 * then MW x TWB = tile rows x columns of a workgroup's region and TH = its pixel rows). */
int kbn_conv2d_query(int n, int out_channels, int in_channels, int kernel_size, int stride,
                     int in_height, int in_width, int resize, int* info);

/* What the LAST kbn_conv2d_forward / kbn_upconv2x_forward / kbn_deconv2x_forward of the calling thread actually launched (the two
 * queries above predict from the shape alone and assume aligned, dense tensor sources).  Written on the host at the point of
 * the successful launch; a call that failed or found no kernel leaves family 0; with first-use tuning on it is the final launch's.
 * info[KBN_CONV_ROUTE_FIELDS] = {family, kernel_size, stride, CK, NB, MW, TWB, Winograd RT, Winograd CT, LDS epilogue in effect,
 * up-conv form (9 / 3 / 4 products or phases), up-conv DMA granule in bytes (16 / 4 / 0), up-conv half-size tile, 0, 0, 0}.
 * family: 0 none, 1 conv_wino_kernel, 2 conv_dma_kernel, 3 conv_dma_kernel with generic (SYN) staging, 4 conv_igemm_kernel
 * pipelined, 5 conv_igemm_kernel not pipelined, 6 conv_up2x9_kernel, 7 conv_up2x_dma_kernel, 8 conv_up2x_kernel.  The numbers
 * are the template arguments of the kernel that ran (the up-convs report kernel 3 stride 1, the conv behind the 2x fold). */
#define KBN_CONV_ROUTE_FIELDS 16
int kbn_conv_last_route(int* info);

/* ----------------------------------------------------------- KB block ----------
 * net_utils.CalibratedBackprojectionBlock.forward(image, depth, coordinates, fused)
 *                                                  reference src/net_utils.py:1343-1371
 * conv_image (3x3 s2), conv_depth (3x3 s2 on cat[depth, coordinates]) and conv_fused (1x1 s2 on
 * cat[image, coordinates*z, fused]) with z = act(proj_depth(depth)) evaluated only where the
 * stride-2 conv samples it.  KBNet's shapes (filters_image == filters_fused in {48, 96, 192, 384},
 * aligned rows) run conv_image + conv_fused as ONE kernel over a shared image tile, with a
 * 16-filter conv_depth in the same launch (csrc/kb_pair.hip); anything else takes three
 * kbn_conv2d_forward-style launches.  Same results bit for bit either way.
 *   coordinates     N x 3 x H x W, or NULL to synthesize them from kinv (N x 3 x 3)
 *   fused           N x channels_fused x H x W or NULL (level 0)
 *   packed weights  from kbn_conv2d_pack_weight; proj_weight is the raw (1 x Cd x 1 x 1)
 *   outputs         each at ceil(H/2) x ceil(W/2), with its own batch stride
 *   *_batch_stride  elements between frames (inputs/outputs may be channel slices of a
 *                   larger NCHW tensor, e.g. the encoder's skip buffers; `coordinates`, when
 *                   given, is contiguous N x 3 x H x W)
 *   out_*_absmax    per-frame max |out| slots of the three outputs (each may be NULL; two may be the same slot)
 */
int kbn_kb_block_forward(const float* image, long long image_batch_stride, const float* depth,
                         long long depth_batch_stride, const float* coordinates, const float* kinv,
                         const float* fused, long long fused_batch_stride,
                         const float* packed_w_image, const float* packed_w_depth,
                         const float* proj_weight, const float* packed_w_fused, float* out_image,
                         long long out_image_batch_stride, float* out_depth,
                         long long out_depth_batch_stride, float* out_fused,
                         long long out_fused_batch_stride, int n, int height, int width,
                         int channels_image, int channels_depth, int channels_fused,
                         int filters_image, int filters_depth, int filters_fused,
                         float negative_slope, unsigned* out_image_absmax, unsigned* out_depth_absmax,
                         unsigned* out_fused_absmax, kbn_stream_t stream);

/* ------------------------------------------- encoder front (image branch) ------
 * conv0_image and the two convs of the level-0 KB block that read it, in ONE launch:
 *     conv0_image = act(conv3x3(image))                          reference src/networks.py:364-365
 *     conv_image  = act(conv3x3 s2 (conv0_image))                reference src/net_utils.py:1348
 *     conv_fused  = act(conv1x1 s2 (cat[conv0_image, xyz]))      reference src/net_utils.py:1352-1369 (level 0: no `fused` input)
 * conv0_image (conv0_filters channels at full resolution) is consumed by nothing else, so it is computed per tile and kept
 * on the CU: it never reaches HBM.  All three convs on split fp16 operands (see the split-operand section above; same
 * accuracy class, same parity gate); csrc/kb1_front.hip.
 *   image           N x image_channels x H x W (image_channels <= 4), frames image_batch_stride apart
 *                   (the fp16 windows of the image and of conv0's on-chip output follow the data tile by tile, inside the kernel)
 *   packed_weight   from kbn_kb1_front_pack_weight: conv0_image.conv.weight (conv0_filters x image_channels x 3 x 3),
 *                   the block's conv_image weight (kb_filters x conv0_filters x 3 x 3) and conv_fused weight
 *                   (kb_filters x (conv0_filters + 3) x 1 x 1, input order [image channels, xyz])
 *   xyz             N x 3 x ceil(H/2) x ceil(W/2) from kbn_kb_xyz_s2_forward (depth = conv0_depth's output), or NULL
 *   out_image/fused N x kb_filters x ceil(H/2) x ceil(W/2) each, with their own batch strides and absmax slots
 * KBN_ERR_UNSUPPORTED unless conv0_filters == kb_filters == 48 (KBNet's level 0 in all three presets) -- the caller then
 * runs kbn_conv2d_forward + kbn_kb_block_forward. */
/* range: image_channels 1 .. 4, both filter counts 48; 0 otherwise */
size_t kbn_kb1_front_packed_weight_bytes(int image_channels, int conv0_filters, int kb_filters);
/* KBN_OK when kbn_kb1_front_forward would take this problem, KBN_ERR_UNSUPPORTED otherwise (widths, map size, slope outside
 * [0, 1], KBN_NO_SPLIT): lets a caller decide BEFORE it launches the depth branch whose xyz output the kernel consumes. */
int kbn_kb1_front_query(int image_channels, int conv0_filters, int kb_filters, int height, int width, float conv0_negative_slope);
int kbn_kb1_front_pack_weight(const float* w_conv0, const float* w_conv_image, const float* w_conv_fused, void* packed,
                              int image_channels, int conv0_filters, int kb_filters, kbn_stream_t stream);
int kbn_kb1_front_forward(const float* image, long long image_batch_stride, const void* packed_weight, const float* xyz, long long xyz_batch_stride, float* out_image,
                          long long out_image_batch_stride, float* out_fused, long long out_fused_batch_stride, int n,
                          int image_channels, int conv0_filters, int kb_filters, int height, int width,
                          float conv0_negative_slope, float kb_negative_slope, unsigned* out_image_absmax,
                          unsigned* out_fused_absmax, kbn_stream_t stream);

/* The same launch PLUS conv_fused of the NEXT KB level (round 5):
 *     conv_fused_next = act(conv1x1 s2 (cat[conv_image, xyz_next, conv_fused]))     reference src/net_utils.py:1352-1369, the block of
 *                                                                                   level 1 (src/networks.py:401-405)
 * A 1x1 stride-2 conv reads only the pixels (2y, 2x) of its inputs -- for a tile of this kernel the 4 x 8 even pixels of the two
 * outputs its lanes still hold: no halo, no second pass over conv_image / conv_fused (as its own launch the layer is the one
 * HBM-bound conv of the network: it fetches every other ROW of 96 channels at half resolution to use every other pixel of it).
 * The even pixels are split tile by tile (window = the tile's own maximum) and multiplied on the fp16 matrix core like every other
 * split-operand conv; the three backprojection channels of the next level enter in fp32.
 *   packed_next     from kbn_kb1_front_next_pack_weight: the next block's conv_fused weight, filters x (kb_filters + 3 + kb_filters)
 *                   x 1 x 1, input order [conv_image channels, xyz, conv_fused channels]
 *   xyz_next        N x 3 x h2 x w2 (h2 = ceil(ceil(H/2)/2)): kbn_kb_xyz_s2_forward on the level-0 conv_depth output with the next
 *                   block's proj_depth weight and the level-1 inverse intrinsics
 *   out_next_fused  N x next_filters x h2 x w2, frames out_next_fused_batch_stride apart; out_next_fused_absmax its slot (or NULL)
 * KBN_ERR_UNSUPPORTED (kbn_kb1_front_next_query tells beforehand) unless kb_filters == 48 and next_filters == 96 -- KBNet's levels 0 / 1
 * in all presets -- or with KBN_NO_FRONT_NEXT=1: the caller then runs kbn_kb1_front_forward and the next block's conv_fused on its own. */
/* range: (48, 48, 96) only; 0 otherwise */
size_t kbn_kb1_front_next_packed_weight_bytes(int image_channels, int fused_channels, int filters);
int kbn_kb1_front_next_pack_weight(const float* w_conv_fused, void* packed, int image_channels, int fused_channels, int filters,
                                   kbn_stream_t stream);
int kbn_kb1_front_next_query(int image_channels, int conv0_filters, int kb_filters, int next_filters, int height, int width,
                             float conv0_negative_slope);
int kbn_kb1_front_next_forward(const float* image, long long image_batch_stride, const void* packed_weight, const float* xyz,
                               long long xyz_batch_stride, float* out_image, long long out_image_batch_stride, float* out_fused,
                               long long out_fused_batch_stride, int n, int image_channels, int conv0_filters, int kb_filters, int height,
                               int width, float conv0_negative_slope, float kb_negative_slope, unsigned* out_image_absmax,
                               unsigned* out_fused_absmax, const void* packed_next, const float* xyz_next, long long xyz_next_batch_stride,
                               float* out_next_fused, long long out_next_fused_batch_stride, int next_filters, float next_negative_slope,
                               unsigned* out_next_fused_absmax, kbn_stream_t stream);

/* The depth branch of the same front:
 *     conv0_depth = act(conv3x3(depth))                                 reference src/networks.py:366-367
 *     conv_depth  = act(conv3x3 s2 (cat[conv0_depth, coordinates]))     reference src/net_utils.py:1351
 *     xyz         = coordinates * act(proj_depth(conv0_depth))          reference src/net_utils.py:1354-1360, sampled at (2y, 2x)
 * conv0_depth stays on the CU; the tensor channels on split fp16 operands, the three coordinate channels K^-1 [x y 1]^T in fp32.
 *   depth           N x depth_channels x H x W (the S2D output, depth_channels <= 8)
 *   kinv            N x 3 x 3 inverse intrinsics of level 0 (kbn_intrinsics_inverse)
 *   packed_weight   from kbn_kb1_depth_front_pack_weight: conv0_depth.conv.weight (16 x depth_channels x 3 x 3), the block's
 *                   conv_depth weight (16 x (16 + 3) x 3 x 3, input order [depth channels, coordinates]) and proj_depth weight (16)
 *   out_depth       N x 16 x ceil(H/2) x ceil(W/2) (frames out_depth_batch_stride apart), out_depth_absmax its slot (or NULL)
 *   xyz             N x 3 x ceil(H/2) x ceil(W/2): what kbn_kb1_front_forward / kbn_conv1x1s2_split_forward take
 * KBN_ERR_UNSUPPORTED unless conv0_filters == kb_filters == 16. */
/* range: depth_channels 1 .. 8, both filter counts 16; 0 otherwise */
size_t kbn_kb1_depth_front_packed_weight_bytes(int depth_channels, int conv0_filters, int kb_filters);
int kbn_kb1_depth_front_query(int depth_channels, int conv0_filters, int kb_filters, int height, int width, float conv0_negative_slope);
int kbn_kb1_depth_front_pack_weight(const float* w_conv0, const float* w_conv_depth, const float* w_proj, void* packed,
                                    int depth_channels, int conv0_filters, int kb_filters, kbn_stream_t stream);
int kbn_kb1_depth_front_forward(const float* depth, long long depth_batch_stride, const float* kinv, const void* packed_weight,
                                float* out_depth, long long out_depth_batch_stride, float* xyz, long long xyz_batch_stride, int n,
                                int depth_channels, int conv0_filters, int kb_filters, int height, int width,
                                float conv0_negative_slope, float kb_negative_slope, int proj_activation, float proj_negative_slope,
                                unsigned* out_depth_absmax, kbn_stream_t stream);

/* The same depth branch with the S2D layer in front of it, in ONE launch (csrc/s2d_stage.h, kb1_depth_front_kernel<pool preset>):
 *     s2d         = SparseToDensePool.forward(x)                        reference src/networks.py:2168-2196, src/kbnet_model.py:161-163
 *     conv0_depth, conv_depth, xyz as above                             reference src/networks.py:366-367, src/net_utils.py:1351-1360
 * Per tile of 8 x 16 half-resolution pixels the workgroup evaluates S2D for the 19 x 35 full-resolution pixels conv0_depth reads
 * (min / max pyramid bit-exact as in kbn_s2d_forward; the 1x1 chain and the 3x3 conv on split fp16 operands) and keeps the result
 * in LDS: the N x 8 x H x W S2D tensor (13.7 MB per KITTI frame written and read back) never reaches HBM.
 *   x               N x 2 x H x W: [sparse depth, validity map] (kbn_s2d_forward's input), frames x_batch_stride apart
 *   packed_s2d      from kbn_s2d_depth_front_pack_weight: pool_convs.{0,1,2}.conv.weight (8 x n_pools | 8 | 8), conv.conv.weight (8 x 10 x 3 x 3)
 *   packed_weight   from kbn_kb1_depth_front_pack_weight (depth_channels = 8)
 *   pool lists      as kbn_s2d_forward; the kernel is compiled for the reference's shipped presets -- KITTI (min 5..13, max 15, 17), VOID / NYUv2
 *                   (min 15, 17, max 23, 27, 29), VOID training (min 15, 17, 19, max 23, 27)
 * KBN_ERR_UNSUPPORTED (kbn_s2d_depth_front_query says so beforehand) for any other pool list, input_channels != 2, n_convolution != 3,
 * n_filter != 8, slopes outside [0, 1], under KBN_NO_DEPTH_FRONT_FUSION=1 or KBN_NO_SPLIT=1, and wherever kbn_kb1_depth_front_forward
 * declines: the caller runs kbn_s2d_forward + kbn_kb1_depth_front_forward. */
/* range: n_pools 1 .. 8; 0 otherwise */
size_t kbn_s2d_depth_front_packed_weight_bytes(int n_pools);
int kbn_s2d_depth_front_pack_weight(const float* w_pool_conv0, const float* w_pool_conv1, const float* w_pool_conv2, const float* w_conv,
                                    void* packed, int n_pools, kbn_stream_t stream);
int kbn_s2d_depth_front_query(int input_channels, const int* min_pool_sizes, int n_min, const int* max_pool_sizes, int n_max,
                              int n_convolution, int n_filter, int conv0_filters, int kb_filters, int height, int width,
                              float s2d_negative_slope, float conv0_negative_slope);
int kbn_s2d_depth_front_forward(const float* x, long long x_batch_stride, const float* kinv, const void* packed_s2d, const void* packed_weight,
                                float* out_depth, long long out_depth_batch_stride, float* xyz, long long xyz_batch_stride, int n,
                                int input_channels, const int* min_pool_sizes, int n_min, const int* max_pool_sizes, int n_max,
                                int n_convolution, int n_filter, int conv0_filters, int kb_filters, int height, int width,
                                float s2d_negative_slope, float conv0_negative_slope, float kb_negative_slope, int proj_activation,
                                float proj_negative_slope, unsigned* out_depth_absmax, kbn_stream_t stream);

/* ------------------------------------------------------------ depth head -------
 * MultiScaleDecoder.output0 (3x3, linear)           reference src/networks.py:1842-1851, 1985
 * + KBNetModel.forward's sigmoid / depth mapping    reference src/kbnet_model.py:181-184
 *   depth = d_min / (sigmoid(conv3x3(x, w)) + d_min / d_max)
 * x: N x channels x H x W (channels <= 16), w: 1 x channels x 3 x 3 (raw OIHW).
 * `logits` may be NULL; when given it receives the pre-sigmoid conv output. */
int kbn_depth_head_forward(const float* x, const float* weight, float* depth, float* logits, int n,
                           int channels, int height, int width, float min_predict_depth,
                           float max_predict_depth, kbn_stream_t stream);

/* The decoder's tail in one launch: DecoderBlock deconv0's second conv (channels -> channels, 3x3,
 * optional LeakyReLU; reference src/net_utils.py:1485-1487 with no skip, src/networks.py:1966-1983)
 * + output0 + the depth mapping above; the channels-wide full-resolution tensor between the two convs
 * stays on the CU.  x: N x channels x H x W (frames x_batch_stride elements apart), w_conv: channels x
 * channels x 3 x 3 and w_out: 1 x channels x 3 x 3, both raw OIHW.  KBN_ERR_UNSUPPORTED unless channels is a
 * multiple of 4 (<= 16), width a multiple of 4 and the planes 16-byte aligned: the caller then runs
 * kbn_conv2d_forward + kbn_depth_head_forward (same results up to fp32 summation order). */
int kbn_conv_head_forward(const float* x, long long x_batch_stride, const float* w_conv, const float* w_out,
                          float* depth, float* logits, int n, int channels, int height, int width,
                          int apply_activation, float negative_slope, float min_predict_depth,
                          float max_predict_depth, kbn_stream_t stream);

/* The same tail with the channels -> channels conv on split fp16 operands (csrc/tail.hip; see the split-operand section: same
 * accuracy class, same parity gate): on the fp32 MFMAs that conv was what bound kbn_conv_head_forward.  packed_w_conv from
 * kbn_conv_tail_pack_weight (raw channels x channels x 3 x 3 weight in); w_out raw.  No alignment requirements.
 * KBN_ERR_UNSUPPORTED for channels > 12 (the caller runs kbn_conv_head_forward or the two-launch path). */
/* range: channels 1 .. 16; 0 otherwise */
size_t kbn_conv_tail_packed_weight_bytes(int channels);
int kbn_conv_tail_pack_weight(const float* w_conv, void* packed, int channels, kbn_stream_t stream);
int kbn_conv_tail_forward(const float* x, long long x_batch_stride, const void* packed_w_conv, const float* w_out, float* depth,
                          float* logits, int n, int channels, int height, int width, int apply_activation, float negative_slope,
                          float min_predict_depth, float max_predict_depth, kbn_stream_t stream);
/* The same launch with the input as a PAIR tensor of 16 channels (two k-groups; channels past `channels` zero): what
 * kbn_conv3x3_split_forward(mode 3, pair_out) writes for a layer of at most 16 filters -- deconv0's up-conv, reference
 * src/net_utils.py:484-499 -- so that the 12-channel full-resolution tensor between the up-conv and the tail is staged by
 * LDS-DMA instead of being loaded, measured and split per tile. */
int kbn_conv_tail_forward_pair(const void* x_pair, long long x_pair_batch_stride, const float* x_pair_scale, const void* packed_w_conv,
                               const float* w_out, float* depth, float* logits, int n, int channels, int height, int width,
                               int apply_activation, float negative_slope, float min_predict_depth, float max_predict_depth,
                               kbn_stream_t stream);

/* ------------------------------------------------- pre-model stage --
 * What the reference's run loop does between the host->device copy and the model call:
 *   validity = where(sparse > 0, 1, sparse)                        reference src/kbnet.py:899-902
 *   OutlierRemoval(kernel_size, threshold).remove_outliers          reference src/net_utils.py:1761-1806
 *     (k x k min filter over the depth with invalid pixels and the padding set to
 *      10 * max(sparse_depth) -- a BATCH-global maximum; a point is dropped if
 *      min < depth - threshold)
 *   image / 255, or 2 (image / 255) - 1 (image_range KBN_IMAGE_RANGE_M1_1)   reference src/transforms.py:201-208
 * image/out_image: N x image_channels x H x W (both may be NULL to skip the normalisation);
 * out_validity: the filtered validity map the model is fed; out_sparse_depth (may be NULL): the
 * filtered sparse depth.  workspace: >= 4 bytes of device memory.  kernel_size odd, <= 15. */
enum { KBN_IMAGE_RANGE_0_1 = 0, KBN_IMAGE_RANGE_M1_1 = 1 };   /* run_kbnet.py --normalized_image_range 0 1 | -1 1 (0 255: pass NULL images) */
int kbn_preprocess_forward(const float* image, const float* sparse_depth, float* out_image,
                           float* out_validity, float* out_sparse_depth, void* workspace,
                           size_t workspace_bytes, int n, int image_channels, int height, int width,
                           int kernel_size, float threshold, int image_range, kbn_stream_t stream);

/* ------------------------------------------------- on-device evaluation
 * The reference's per-sample metrics                  reference src/kbnet.py:932-950,
 *                                                     src/eval_utils.py:20-78
 * over the pixels with ground_truth_validity > 0 and min < ground_truth < max.  ADDS into
 * sums[n*5 + k] (fp64, caller zeroes): k=0 sum|1000(o-g)|, 1 sum(1000(g-o))^2,
 * 2 sum|1/(.001g) - 1/(.001o)|, 3 its square, 4 pixel count.  MAE = s0/s4 (mm),
 * RMSE = sqrt(s1/s4), iMAE = s2/s4 (1/km), iRMSE = sqrt(s3/s4).  The bounds are strict and a NaN validity or
 * ground truth counts nothing; what a masked-out pixel holds (NaN, inf) is never read into a sum.  Every per-pixel
 * term is formed in fp32 with each product and the difference rounded on its own (no FMA contraction), as numpy
 * forms it; only the sums are fp64.  A frame in which no pixel passes the mask leaves s4 = 0: the caller divides
 * 0 by 0 and reports NaN there, as the reference's np.mean over an empty selection does (ops.eval_metrics does so;
 * inference.run and validation.validate then report NaN means exactly where the reference's are NaN). */
int kbn_eval_accumulate(const float* output_depth, const float* ground_truth,
                        const float* ground_truth_validity, double* sums, int n, int height,
                        int width, float min_evaluate_depth, float max_evaluate_depth,
                        kbn_stream_t stream);

/* ------------------------------------------------- forward value of the objective ----
 * KBNetModel.compute_loss                              reference src/kbnet_model.py:188-304
 *   net_utils.backproject_to_camera / project_to_pixel  reference src/net_utils.py:1638-1704
 *     points = K^-1 [x y 1]^T z;  xy = (T p)[0:2] / ((T p)[2] + 1e-7),  T = rows 0-2 of (K | 0) pose
 *   net_utils.grid_sample (bilinear, border, align_corners)  reference src/net_utils.py:1706-1739
 *   losses.color_consistency_loss_func, structural_consistency_loss_func (ssim: AvgPool2d(3, 1),
 *     stretched back to H x W with nearest interpolation), sparse_depth_consistency_loss_func,
 *     smoothness_loss_func                              reference src/losses.py:23-158
 * in ONE image-sized launch, without an image-sized intermediate.  image0 / image1 / image2:
 * N x 3 x H x W; output_depth / sparse_depth / validity_map: N x 1 x H x W; intrinsics N x 3 x 3;
 * pose01 / pose02 N x 4 x 4 (image0 -> image1, image0 -> image2).  WRITES sums[n*8 + k] (fp64; the
 * entry zeroes them on `stream` first): k=0 sum|image01 - image0|, 1 sum|image02 - image0| (over
 * the 3 channels), 2 / 3 sum of the up-sampled 1-SSIM maps of the two pairs (3 channels), 4 sum
 * v|sparse - depth|, 5 sum v, 6 sum wx|dx depth| (H (W-1) terms), 7 sum wy|dy depth| ((H-1) W terms).
 * image01 / image02 (N x 3 x H x W): the warped neighbour frames, or both NULL.  height, width >= 3.
 * Sample positions of any value (points behind the camera, Inf, NaN) read inside the planes. */
int kbn_photometric_loss_forward(const float* image0, const float* image1, const float* image2,
                                 const float* output_depth, const float* sparse_depth,
                                 const float* validity_map, const float* intrinsics,
                                 const float* pose01, const float* pose02, double* sums,
                                 float* image01, float* image02, int n, int height, int width,
                                 kbn_stream_t stream);

/* ------------------------------------------------- gradient of the objective ----
 * torch.autograd's backward of KBNetModel.compute_loss  reference src/kbnet_model.py:188-304
 *   project_to_pixel: d = q2 + 1e-7, u = q0 / d, v = q1 / d   reference src/net_utils.py:1676-1704
 *   grid_sample (bilinear, border: no gradient for a position on or beyond the border)
 *                                                       reference src/net_utils.py:1706-1739
 *   the four terms (abs: sgn(0) = 0; clamp passes the gradient on [0, 1])   reference src/losses.py:23-158
 * with respect to what the reference trains through: output_depth and the two poses.  Inputs as
 * kbn_photometric_loss_forward; grad_sums: N x 8 fp64, the gradient of that entry's sums (column 5,
 * sum v, depends on nothing differentiable).  WRITES every element of grad_depth (N x 1 x H x W) once
 * and ADDS INTO grad_proj[(n*2 + pair)*12 + i*4 + j] (fp64; the entry zeroes the buffer on `stream`
 * first) the gradient with respect to T[i][j], T = rows 0-2 of (K | 0) pose of pair 0 (pose01) and
 * 1 (pose02): grad_pose[0:3, :] = K^T grad_T, row 3 is zero.  One launch; allocates nothing, does not
 * synchronise.  Sample positions of any value read inside the planes, as in the forward. */
int kbn_photometric_loss_backward(const float* image0, const float* image1, const float* image2,
                                  const float* output_depth, const float* sparse_depth,
                                  const float* validity_map, const float* intrinsics,
                                  const float* pose01, const float* pose02, const double* grad_sums,
                                  float* grad_depth, double* grad_proj, int n, int height, int width,
                                  kbn_stream_t stream);

/* ------------------------------------------------- pose network (eval mode) ----
 * PoseNetModel.forward                                 reference src/posenet_model.py:95-112
 *   networks.PoseEncoder                               reference src/networks.py:536-671
 *     seven net_utils.Conv2d (src/net_utils.py:51-141): bias-free conv, kernel 7, 5, 3, 3, 3, 3, 3, stride 2, padding k / 2,
 *     BatchNorm2d (eval: running statistics), LeakyReLU(0.20)
 *   networks.PoseDecoder                               reference src/networks.py:1992-2075
 *     1 x 1 conv to 6 channels, mean over H W, x 0.01, net_utils.pose_matrix (src/net_utils.py:1493-1595)
 *
 * kbn_conv2d_s2_affine_forward: out[n, o, oy, ox] = act((sum_c,ky,kx W[o, c, ky, kx] in[n, c, 2 oy + ky - k/2, 2 ox + kx - k/2])
 * * scale[o] + shift[o]), act = max(v, slope v) when apply_activation.  `in` is the channel concat of one or two
 * KBN_SRC_TENSOR sources of in_height x in_width (the two images are read in place, src/posenet_model.py:109); taps outside
 * the image are zero.  kernel_size in {3, 5, 7}; any channel counts.  scale / shift: out_channels floats each -- BatchNorm2d in
 * eval mode is scale = g / sqrt(var + eps), shift = b - mean * scale; the scale is applied to the finished sum, not folded
 * into the weights.  out: out_channels x ceil(in_h / 2) x ceil(in_w / 2) per frame, frames out_batch_stride elements apart.
 * Every output pixel is a function of its frame and the weights alone. */
/* range: kernel_size 3, 5 or 7, channels in the common range, in_channels x k x k <= 2^24; 0 otherwise */
size_t kbn_conv2d_s2_affine_packed_weight_bytes(int out_channels, int in_channels, int kernel_size);
int kbn_conv2d_s2_affine_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                                     int kernel_size, kbn_stream_t stream);
int kbn_conv2d_s2_affine_forward(const kbn_conv_src* srcs, int n_src, const float* packed_weight, const float* scale,
                                 const float* shift, float* out, long long out_batch_stride, int n, int out_channels,
                                 int kernel_size, int in_height, int in_width, int apply_activation,
                                 float negative_slope, kbn_stream_t stream);

/* PoseDecoder.forward with n_filters = [] (reference src/networks.py:2067-2075) in one launch, one workgroup per frame:
 * latent N x channels x height x width (frames latent_batch_stride elements apart), weight 6 x channels (the 1 x 1 conv) ->
 * pose N x 16 (row-major 4 x 4: rotation from the axis-angle dof[0:3], translation dof[3:6], last row 0 0 0 1) and, when
 * `dof` is not NULL, the N x 6 vector 0.01 * mean(conv(latent)) itself.  The spatial sums run in a fixed order without
 * atomics, and the mean is taken before the 6 x channels product (the conv of the mean is the mean of the conv). */
int kbn_pose_head_forward(const float* latent, long long latent_batch_stride, const float* weight, float* pose,
                          float* dof, int n, int channels, int height, int width, kbn_stream_t stream);

/* ------------------------------------------------- pose network (training: the backward of a PoseEncoder layer) ----
 * What reference src/kbnet.py:392-453 (loss.backward() through pose_model in train mode) needs of net_utils.Conv2d
 * (src/net_utils.py:51-141: bias-free conv stride 2 padding k / 2, torch.nn.BatchNorm2d, LeakyReLU) on the HIP path.  fp32 in and
 * out; the matrix products on v_mfma_f32_16x16x4_f32; no floating-point atomics: every sum has a fixed order, a call's bits are a
 * function of its arguments alone.
 *
 * kbn_conv2d_s2_backward_data (the conv of src/net_utils.py:120-126, differentiated by its input):
 *   grad_in[n, c, iy, ix] = sum_o,ky,kx W[o, c, ky, kx] grad_out[n, o, (iy + k/2 - ky) / 2, (ix + k/2 - kx) / 2] over the taps
 *   whose numerators are even and land inside the ceil(in_h / 2) x ceil(in_w / 2) output map.  The gradient of the channel concat
 *   of one or two inputs: channels [0, channels0) go to grad_in0, the next channels1 to grad_in1 (NULL and 0 for one input), frames
 *   *_batch_stride elements apart.  kernel_size in {3, 5, 7}, any channel counts.  packed_weight: the OIHW weight through
 *   kbn_conv2d_s2_backward_data_pack_weight (its own, transposed order: not the forward's blob).
 * kbn_conv2d_s2_backward_weight (the same conv, differentiated by its OIHW weight):
 *   grad_weight[o, c, ky, kx] = sum_n,oy,ox grad_out[n, o, oy, ox] in[n, c, 2 oy + ky - k/2, 2 ox + kx - k/2], `in` the concat of
 *   one or two KBN_SRC_TENSOR sources as kbn_conv2d_s2_affine_forward reads them, taps outside the image zero.  The sum over the
 *   output pixels is split over `splits` workgroups per tile (<= 0: chosen from the shape alone, not from the device), whose
 *   partial sums go to `scratch` (kbn_conv2d_s2_backward_weight_scratch_bytes(..., splits) bytes; 0 bytes, and scratch may be
 *   NULL, when one split remains) and are added in split order by a second launch.  grad_weight is plain OIHW. */
/* range: kernel_size 3, 5 or 7, channels in the common range, out_channels x k x k <= 2^24; 0 otherwise */
size_t kbn_conv2d_s2_backward_data_packed_weight_bytes(int out_channels, int in_channels, int kernel_size);
int kbn_conv2d_s2_backward_data_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                                            int kernel_size, kbn_stream_t stream);
int kbn_conv2d_s2_backward_data(const float* grad_out, long long grad_out_batch_stride, const float* packed_weight,
                                float* grad_in0, long long grad_in0_batch_stride, int channels0, float* grad_in1,
                                long long grad_in1_batch_stride, int channels1, int n, int out_channels, int kernel_size,
                                int in_height, int in_width, kbn_stream_t stream);
/* range: kernel_size 3, 5 or 7; n, sides >= 1, sides <= KBN_MAX_MAP_SIDE, height x width and n x output pixels below 2^31, channels in the common range, in_channels x k x k <= 2^24, the weight below 2^31 elements; splits <= 0 lets the library choose.  0 otherwise, and 0 when the gradient is not split (no scratch needed): kbn_conv2d_s2_backward_weight tells the two apart */
size_t kbn_conv2d_s2_backward_weight_scratch_bytes(int n, int out_channels, int in_channels, int kernel_size, int in_height,
                                                   int in_width, int splits);
int kbn_conv2d_s2_backward_weight(const kbn_conv_src* srcs, int n_src, const float* grad_out, long long grad_out_batch_stride,
                                  float* grad_weight, int n, int out_channels, int kernel_size, int in_height, int in_width,
                                  int splits, float* scratch, size_t scratch_bytes, kbn_stream_t stream);

/* torch.nn.BatchNorm2d in train mode (src/net_utils.py:103-104, 128-129) with the activation behind it (:131-141).
 * kbn_bn_stats_forward: mean[c] and the BIASED variance var[c] of x (N x channels x H x W, frames batch_stride apart) over N, H, W,
 *   two passes accumulated in fp64 (the mean, then the centred squares), rounded to fp32 once.
 * kbn_bn_act_forward: y = act(u * scale[c] + shift[c]) (one fused multiply-add), act = max(v, slope v) when apply_activation.
 *   The caller forms scale = gamma rstd and shift = beta - mean scale from the running or the batch statistics.
 * kbn_bn_act_backward: two launches.  (1) per channel, in fp64 and a fixed order: sums[c] = sum g_z (the gradient of beta) and
 *   sums[channels + c] = sum g_z xhat (the gradient of gamma), g_z = grad_y (z > 0 ? 1 : slope) with z = u * scale[c] + shift[c]
 *   formed as the forward forms it (z <= 0 takes the slope, as torch's leaky_relu at 0), xhat = (u - mean[c]) rstd[c].
 *   (2) grad_u = scale[c] (g_z - (sums[c] + xhat sums[channels + c]) / (N H W)) with batch_statistics, scale[c] g_z without (the
 *   statistics are constants then). */
int kbn_bn_stats_forward(const float* x, long long batch_stride, float* mean, float* var, int n, int channels, int height,
                         int width, kbn_stream_t stream);
int kbn_bn_act_forward(const float* u, long long u_batch_stride, const float* scale, const float* shift, float* y,
                       long long y_batch_stride, int n, int channels, int height, int width, int apply_activation,
                       float negative_slope, kbn_stream_t stream);
int kbn_bn_act_backward(const float* u, long long u_batch_stride, const float* grad_y, long long grad_y_batch_stride,
                        const float* scale, const float* shift, const float* mean, const float* rstd, double* sums,
                        float* grad_u, long long grad_u_batch_stride, int n, int channels, int height, int width,
                        int apply_activation, float negative_slope, int batch_statistics, kbn_stream_t stream);

/* The same BatchNorm2d (src/net_utils.py:103-104, 128-141) on the statistics of a batch that is spread over several ranks, in
 * place of the per-replica statistics of torch.nn.DataParallel (src/kbnet_model.py:408-415): rank r holds n_r frames,
 * c_r = n_r H W values per channel, M = sum c_r.  Between the ranks travel fp64 records that the caller gathers; every sum over
 * ranks runs in rank order, so all ranks form the same bits.
 * kbn_bn_moments_forward: record[0] = c_r, record[1 + c] = the mean of channel c over the rank's frames, record[1 + channels + c]
 *   = its sum of centred squares: kbn_bn_stats_forward's two fp64 passes, not rounded to fp32 (2 channels + 1 doubles).
 * kbn_bn_moments_merge: `records` (world x (2 channels + 1), rank order) merged pairwise from rank 0 on,
 *   d = m_B - m_A; m = m_A + d c_B / (c_A + c_B); q = q_A + q_B + d^2 c_A c_B / (c_A + c_B), then rounded to fp32 once:
 *   mean, var = q / M (normalises) and var_unbiased = q / (M - 1) (the running variance's update).
 * kbn_bn_act_backward_sums: launch (1) of kbn_bn_act_backward alone, on the merged statistics: the rank's sums (2 channels doubles).
 * kbn_bn_act_backward_sync_apply: S = sum_r (c_r / M) gathered_sums[r] in rank order (world x 2 channels; the counts c_r are
 *   gathered_records[r][0]), then grad_u = scale[c] (g_z - (S[c] + xhat S[channels + c]) / c_rank): the divisor is the rank's own
 *   count, which keeps grad_u in the units of a loss that is the mean over the rank's own frames. */
int kbn_bn_moments_forward(const float* x, long long batch_stride, double* record, int n, int channels, int height, int width,
                           kbn_stream_t stream);
int kbn_bn_moments_merge(const double* records, int world, int channels, float* mean, float* var, float* var_unbiased,
                         kbn_stream_t stream);
int kbn_bn_act_backward_sums(const float* u, long long u_batch_stride, const float* grad_y, long long grad_y_batch_stride,
                             const float* scale, const float* shift, const float* mean, const float* rstd, double* sums, int n,
                             int channels, int height, int width, int apply_activation, float negative_slope, kbn_stream_t stream);
int kbn_bn_act_backward_sync_apply(const float* u, long long u_batch_stride, const float* grad_y, long long grad_y_batch_stride,
                                   const float* scale, const float* shift, const float* mean, const float* rstd,
                                   const double* gathered_sums, const double* gathered_records, int world, int rank, float* grad_u,
                                   long long grad_u_batch_stride, int n, int channels, int height, int width, int apply_activation,
                                   float negative_slope, kbn_stream_t stream);

/* ------------------------------------------------- ResNet pose networks (eval mode) ----
 * PoseNetModel(encoder_type='resnet18' | 'resnet34')   reference src/posenet_model.py:55-87 (what src/kbnet.py:221-226 trains)
 *   networks.ResNetEncoder                             reference src/networks.py:674-996
 *     conv1 7 x 7 stride 2, MaxPool2d(3, stride 2, padding 1), blocks2 .. blocks5 of net_utils.ResNetBlock
 *   net_utils.ResNetBlock                              reference src/net_utils.py:572-667
 *     act(act(bn(conv2(act(bn(conv1(x)))))) + X), X = x, or a 1 x 1 conv of x at the block's stride when the shape differs
 *   networks.PoseDecoder, n_filters = [256, 256]       reference src/networks.py:1992-2075
 *     two 3 x 3 stride-2 convs (BatchNorm2d, activation) before the 1 x 1 conv that kbn_pose_head_forward takes
 *
 * kbn_conv2d_affine_forward: v = (sum_c,ky,kx W[o, c, ky, kx] in[n, c, s oy + ky - k/2, s ox + kx - k/2]) * scale[o] + shift[o];
 * v = act(v) when apply_activation; with `residual` (N x out_channels x OH x OW, frames residual_batch_stride elements apart,
 * or NULL) v = v + residual, and v = act(v) once more when apply_activation; act = max(v, slope v).  kernel_size in {1, 3, 7},
 * stride s in {1, 2}, padding k / 2, OH = ceil(in_h / s), OW = ceil(in_w / s); otherwise the contract of
 * kbn_conv2d_s2_affine_forward: one or two KBN_SRC_TENSOR sources, any channel counts, taps outside the image zero, scale
 * applied to the finished sum (the projection passes scale 1, shift 0), every output pixel a function of its frame and the
 * weights alone.  The packed weight is this entry's own (another K chunk than kbn_conv2d_s2_affine_pack_weight's). */
/* range: kernel_size 1, 3 or 7, channels in the common range, in_channels x k x k <= 2^24; 0 otherwise */
size_t kbn_conv2d_affine_packed_weight_bytes(int out_channels, int in_channels, int kernel_size);
int kbn_conv2d_affine_pack_weight(const float* weight, float* packed, int out_channels, int in_channels,
                                  int kernel_size, kbn_stream_t stream);
int kbn_conv2d_affine_forward(const kbn_conv_src* srcs, int n_src, const float* packed_weight, const float* scale,
                              const float* shift, const float* residual, long long residual_batch_stride, float* out,
                              long long out_batch_stride, int n, int out_channels, int kernel_size, int stride,
                              int in_height, int in_width, int apply_activation, float negative_slope,
                              kbn_stream_t stream);

/* torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (reference src/networks.py:747): in N x channels x height x width ->
 * out N x channels x ceil(height / 2) x ceil(width / 2), frames in_batch_stride / out_batch_stride elements apart.  Taps
 * outside the image never win; a NaN in the window is the result, as in torch. */
int kbn_maxpool3x3s2_forward(const float* in, long long in_batch_stride, float* out, long long out_batch_stride, int n,
                             int channels, int height, int width, kbn_stream_t stream);

/* ------------------------------------------------- ResNet pose networks (training: the backward of their layers) ----
 * What the layers above need beside the stride-2 gradients and the BatchNorm2d entries of the section before them.  fp32 in and
 * out, no floating-point atomics: a call's bits are a function of its arguments alone.  (kernel_size, stride) is one of (3, 1),
 * (1, 1), (1, 2), padding kernel_size / 2, OH = ceil(in_h / stride), OW = ceil(in_w / stride); anything else KBN_ERR_UNSUPPORTED.
 *
 * kbn_conv2d_backward_weight: grad_weight[o, c, ky, kx] = sum_n,oy,ox grad_out[n, o, oy, ox] in[n, c, s oy + ky - k/2, s ox + kx - k/2]
 *   with the sources, the split, the scratch planes and the fixed-order sum of kbn_conv2d_s2_backward_weight.
 * kbn_conv2d_backward_data: grad_in[n, c, iy, ix] = sum_o,ky,kx W[o, c, ky, kx] grad_out[n, o, (iy + k/2 - ky) / s, (ix + k/2 - kx) / s]
 *   over the taps that land on an output pixel; EVERY element of grad_in (N x in_channels x in_h x in_w, one tensor) is written.
 *   At stride 1 this is kbn_conv2d_affine_forward over grad_out with the weight transposed and its taps flipped -- what
 *   kbn_conv2d_backward_data_pack_weight writes, with the unit scale and zero shift behind it; at (1, 2) one launch of its own
 *   writes W^T grad_out to the even-even pixels and zeros to the rest (the blob is the weight itself). */
/* range: as kbn_conv2d_s2_backward_weight_scratch_bytes, with (kernel_size, stride) (3, 1), (1, 1) or (1, 2) */
size_t kbn_conv2d_backward_weight_scratch_bytes(int n, int out_channels, int in_channels, int kernel_size, int stride, int in_height,
                                                int in_width, int splits);
int kbn_conv2d_backward_weight(const kbn_conv_src* srcs, int n_src, const float* grad_out, long long grad_out_batch_stride,
                               float* grad_weight, int n, int out_channels, int kernel_size, int stride, int in_height,
                               int in_width, int splits, float* scratch, size_t scratch_bytes, kbn_stream_t stream);
/* range: (kernel_size, stride) (3, 1), (1, 1) or (1, 2), channels in the common range; 0 otherwise */
size_t kbn_conv2d_backward_data_packed_weight_bytes(int out_channels, int in_channels, int kernel_size, int stride);
int kbn_conv2d_backward_data_pack_weight(const float* weight, float* packed, int out_channels, int in_channels, int kernel_size,
                                         int stride, kbn_stream_t stream);
int kbn_conv2d_backward_data(const float* grad_out, long long grad_out_batch_stride, const float* packed_weight, float* grad_in,
                             long long grad_in_batch_stride, int n, int out_channels, int in_channels, int kernel_size, int stride,
                             int in_height, int in_width, kbn_stream_t stream);

/* The gradient of kbn_maxpool3x3s2_forward: grad_in[n, c, iy, ix] = the sum of grad_out over the windows whose FIRST maximum (the
 * forward's scan: row-major, v > m or v is NaN) is this pixel, the at most four windows taken in (oy, ox) order.  x: the forward's input. */
int kbn_maxpool3x3s2_backward(const float* x, long long x_batch_stride, const float* grad_out, long long grad_out_batch_stride,
                              float* grad_in, long long grad_in_batch_stride, int n, int channels, int height, int width,
                              kbn_stream_t stream);

/* The add that ends a ResNetBlock (src/net_utils.py:666-667) over `count` contiguous floats: y = act(a + b), act = max(v, slope v)
 * when apply_activation.  Backward: grad = grad_y where y > 0, negative_slope grad_y elsewhere (y <= 0 takes the slope, as torch's
 * leaky_relu at 0) -- the gradient of both addends; without activation a copy. */
int kbn_add_act_forward(const float* a, const float* b, float* y, long long count, int apply_activation, float negative_slope,
                        kbn_stream_t stream);
int kbn_add_act_backward(const float* y, const float* grad_y, float* grad, long long count, int apply_activation,
                         float negative_slope, kbn_stream_t stream);

/* ------------------------------------------------- depth network (training: what only KBNet's backward needs) ----
 * KBNetModel(trainable=True): the layers of the depth network one by one, each a differentiable node.  The conv gradients are the
 * entries of the two sections above; these are the three pieces only KBNet has.  fp32 in and out, no atomics, nothing cleared
 * beforehand, every output element written exactly once by the one launch: a call's bits are a function of its arguments alone.
 *
 * kbn_resize_nearest_forward: torch.nn.functional.interpolate(mode='nearest', size=(out_h, out_w)) in front of an up-conv
 *   (UpConv2d.forward, reference src/net_utils.py:484-499; DecoderBlock.forward :1453-1487) as a tensor of its own:
 *   out[n, c, Y, X] = in[n, c, idx(Y, in_h, out_h), idx(X, in_w, out_w)] with the index rule of KBN_RESIZE_NEAREST (the same device
 *   function).  in N x channels x in_h x in_w, out N x channels x out_h x out_w, dense planes, frames *_batch_stride elements apart.
 *   out_h >= in_h and out_w >= in_w; a smaller output is KBN_ERR_UNSUPPORTED.
 * kbn_resize_nearest_backward: grad_in[n, c, y, x] = the sum of grad_out[n, c, Y, X] over the destination pixels with idx(Y) = y and
 *   idx(X) = x, taken in row-major order (a gather: one thread per source pixel, or per four of a row). */
int kbn_resize_nearest_forward(const float* in, long long in_batch_stride, float* out, long long out_batch_stride, int n,
                               int channels, int in_height, int in_width, int out_height, int out_width, kbn_stream_t stream);
int kbn_resize_nearest_backward(const float* grad_out, long long grad_out_batch_stride, float* grad_in,
                                long long grad_in_batch_stride, int n, int channels, int in_height, int in_width, int out_height,
                                int out_width, kbn_stream_t stream);

/* The backprojection of a KB layer, z = act(proj_depth(depth)), xyz = coordinates * z (CalibratedBackprojectionBlock.forward,
 * reference src/net_utils.py:1352-1359), differentiated with respect to proj_depth's PRE-activation:
 *   grad_pre[n, 0, y, x] = act'(z) * sum_c coordinates[n, c, y, x] grad_xyz[n, c, y, x], c < 3; act'(z) = 1 where z > 0, negative_slope
 *   elsewhere (the branch is read from the saved OUTPUT z, as kbn_add_act_backward reads it), 1 everywhere without apply_activation.
 * z and grad_pre N x 1 x height x width, coordinates and grad_xyz N x 3 x height x width (grad_xyz usually a channel slice of
 * conv_fused's data gradient), dense planes, frames *_batch_stride elements apart. */
int kbn_kb_xyz_backward(const float* z, long long z_batch_stride, const float* coordinates, long long coordinates_batch_stride,
                        const float* grad_xyz, long long grad_xyz_batch_stride, float* grad_pre, long long grad_pre_batch_stride,
                        int n, int height, int width, int apply_activation, float negative_slope, kbn_stream_t stream);

/* The gradient of KBNetModel.forward's depth mapping depth = d_min / (sigmoid(l) + d_min / d_max) (reference
 * src/kbnet_model.py:181-184) over `count` contiguous floats: grad_logits = -grad_depth depth^2 / d_min * s (1 - s), s = sigmoid(l),
 * with s (1 - s) taken as e / (1 + e)^2, e = exp(-|l|) (no cancellation where the sigmoid saturates).  logits and depth: what the
 * forward produced (kbn_depth_head_forward with `logits`). */
int kbn_depth_map_backward(const float* logits, const float* depth, const float* grad_depth, float* grad_logits, long long count,
                           float min_predict_depth, kbn_stream_t stream);

/* ------------------------------------------------------------- the optimizer ----
 * torch.optim.Adam as the reference's training loop constructs and steps it:
 *   optimizer = torch.optim.Adam([{'params': parameters_depth_model, 'weight_decay': w_weight_decay_depth},
 *                                 {'params': parameters_pose_model, 'weight_decay': w_weight_decay_pose}], lr=learning_rate)
 *   ... optimizer.step()                                                  reference src/kbnet.py:360-369, 453
 * kbn_adam_step applies ONE Adam step (L2 weight decay; no amsgrad, no maximize, no decoupled decay) to `count` fp32 tensors, each a
 * run of `numel` contiguous floats, in place.  Per element, in fp32, in this order (torch's _single_tensor_adam):
 *   g' = grad + weight_decay * param                              (skipped when weight_decay == 0)
 *   exp_avg    = exp_avg + one_minus_beta1 * (g' - exp_avg)
 *   exp_avg_sq = beta2 * exp_avg_sq + one_minus_beta2 * g' * g'
 *   param      = param - step_size * exp_avg / (sqrt(exp_avg_sq) / bc2_sqrt + eps)
 * with step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) computed by the caller in fp64 for the tensor's own step
 * count t.  `tensors` is a HOST array, read before the call returns; the records travel to the device in the kernel arguments,
 * KBN_ADAM_TABLE_CAPACITY a launch, so the call issues ceil(records with numel > 0 / capacity) launches and nothing else: no
 * device table, no copy, no allocation, no synchronisation.  Tensors whose four pointers are 16-byte aligned are processed four
 * elements a thread; one pass of the widest grid covers KBN_ADAM_PASS_ELEMENTS elements of a tensor (longer ones loop).
 * A record with numel == 0 is skipped (its pointers may be NULL).  KBN_ERR_INVALID_ARGUMENT for a NULL table, count < 1, numel < 0 or
 * a NULL pointer in a record with numel > 0 -- checked for every record before anything is launched.  The four tensors of a record
 * must not overlap each other or another record's. */
#define KBN_ADAM_TABLE_CAPACITY 48
#define KBN_ADAM_MAX_BLOCKS_X 512
#define KBN_ADAM_PASS_ELEMENTS 524288 /* KBN_ADAM_MAX_BLOCKS_X blocks x 256 threads x 4 elements */
typedef struct kbn_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long numel;
    float weight_decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps;
} kbn_adam_tensor;
int kbn_adam_step(const kbn_adam_tensor* tensors, int count, kbn_stream_t stream);

/* ------------------------------------------------- the data-parallel step's gradient pack ----
 * The reference trains on every visible device through torch.nn.DataParallel (src/kbnet_model.py:408-415); here each GPU has its own
 * process and the ranks meet in ONE all-reduce a step over one flat buffer (kb.dist.GradientAverager).
 * kbn_multi_tensor_scale_copy fills and empties that buffer: dst[e] = src[e] * scale for `count` fp32 tensors, each a run of `numel`
 * contiguous floats, `scale` one float for the call.  One fp32 multiply an element: the bits of src * scale (the source's own bits
 * for scale == 1.0f); a NaN or Inf element stays in its own element.
 * `tensors` is a HOST array, read before the call returns; the records travel to the device in the kernel arguments,
 * KBN_MULTI_COPY_TABLE_CAPACITY a launch, so the call issues ceil(records with numel > 0 / capacity) launches and nothing else: no
 * device table, no copy, no allocation, no synchronisation.  Tensors whose two pointers are 16-byte aligned are processed four
 * elements a thread; one pass of the widest grid covers KBN_MULTI_COPY_PASS_ELEMENTS elements of a tensor (longer ones loop).
 * A record with numel == 0 is skipped (its pointers may be NULL).  KBN_ERR_INVALID_ARGUMENT for a NULL table, count < 1, numel < 0 or
 * a NULL pointer in a record with numel > 0 -- checked for every record before anything is launched.  The two tensors of a record
 * must not overlap each other or another record's dst. */
#define KBN_MULTI_COPY_TABLE_CAPACITY 48
#define KBN_MULTI_COPY_MAX_BLOCKS_X 512
#define KBN_MULTI_COPY_PASS_ELEMENTS 524288 /* KBN_MULTI_COPY_MAX_BLOCKS_X blocks x 256 threads x 4 elements */
typedef struct kbn_copy_tensor {
    const float* src;
    float* dst;
    long long numel;
} kbn_copy_tensor;
int kbn_multi_tensor_scale_copy(const kbn_copy_tensor* tensors, int count, float scale, kbn_stream_t stream);

/* ------------------------------------------------- the training step's augmentation ----
 *   [images, depths, validity] = transforms.transform(images_arr=..., range_maps_arr=..., validity_maps_arr=...,
 *                                                     random_transform_probability=...)     reference src/kbnet.py:411-422
 * kbn_augment_forward does the device part of the reference's Transforms.transform (src/transforms.py:61-183) for `count` fp32
 * tensors of n frames of channels x height x width elements: src (any non-negative element strides) is read, dst (dense) is
 * written, nothing else.  flags[n] is a HOST array, a nibble a frame, drawn by the caller: bit 0 horizontal flip, bit 1 vertical
 * flip (every tensor), bit 2 remove points, bit 3 noise (range maps only).  By role:
 *   image      normalization KBN_AUGMENT_RANGE_0_1: x / 255; _M1_1: 2 (x / 255) - 1, one rounding for the subtraction; _0_255: x
 *   range      remove: of the frame's elements > 0 (count of them, over all channels), the k = trunc(fp32(densities[b]) *
 *              fp32(count)) with the smallest (key, source element index) become 0; then noise: out = (v + spread * noise) *
 *              (v > 0 ? 1 : 0), each operation rounded on its own
 *   validity   a copy
 * Random words come from Philox4x32-10 with key = (low, high word of `seed`) and counter = (element index in the SOURCE frame,
 * frame index, `call`, purpose | map_index << 8): purpose 0 is the removal key (word 0), purpose 1 the noise -- uniform:
 * (w0 >> 8) 2^-24 - 0.5; gaussian: sqrtf(-2 logf(((w0 >> 8) + 1) 2^-24)) cosf(2 pi (w1 >> 8) 2^-24).
 * densities[n] is DEVICE memory; count and k never reach the host.  `stages`: KBN_AUGMENT_STAGE_SELECT finds each flagged frame's
 * threshold into `workspace` (kbn_augment_workspace_bytes(...) bytes, 8-byte aligned: first KBN_AUGMENT_WORKSPACE_RECORD_BYTES a
 * frame and range map, in the order of the range maps in `tensors` -- words key, index, k, count -- then a list of 8 bytes an
 * element for the candidates of each), KBN_AUGMENT_STAGE_APPLY writes the outputs and reads the thresholds; pass both for the
 * whole operation (a caller that times the stages passes them one by one, with the same arguments).  The records and flags travel
 * in the kernel arguments: launches only, no copy, no allocation, no synchronisation.  densities and workspace may be NULL when
 * no frame has bit 2 or no tensor is a range map.  KBN_ERR_INVALID_ARGUMENT for NULL pointers, zero sizes, a flag above 15, bit 3
 * with KBN_AUGMENT_NOISE_NONE; KBN_ERR_WORKSPACE for a workspace that is too small; KBN_ERR_UNSUPPORTED for a frame of 2^31
 * elements or more -- all checked before anything is launched.
 *
 * kbn_augment_forward_at is the same operation for a SHARD of a larger batch: the n frames given are frames frame_base ..
 * frame_base + n - 1 of it, and the counter's frame word is frame_base + the frame's index here.  With the same seed, call and
 * map indices, and with flags[] and densities[] the shard's slices of the larger batch's, the outputs are bit for bit the slices
 * [frame_base, frame_base + n) of what one call over the larger batch writes: the ranks of a data-parallel run draw, between
 * them, what one process draws.  Everything that addresses memory -- src, dst, flags[], densities[], the workspace -- is indexed
 * by the frame's index here, 0 .. n - 1.  KBN_ERR_UNSUPPORTED when frame_base + n exceeds 2^32 - 1 (the word is 32 bits);
 * otherwise the arguments, checks and launches of kbn_augment_forward, which is kbn_augment_forward_at with frame_base 0. */
#define KBN_AUGMENT_ROLE_IMAGE 0
#define KBN_AUGMENT_ROLE_RANGE 1
#define KBN_AUGMENT_ROLE_VALIDITY 2
#define KBN_AUGMENT_RANGE_0_255 0
#define KBN_AUGMENT_RANGE_0_1 1
#define KBN_AUGMENT_RANGE_M1_1 2
#define KBN_AUGMENT_NOISE_NONE 0
#define KBN_AUGMENT_NOISE_GAUSSIAN 1
#define KBN_AUGMENT_NOISE_UNIFORM 2
#define KBN_AUGMENT_STAGE_SELECT 1
#define KBN_AUGMENT_STAGE_APPLY 2
#define KBN_AUGMENT_MAX_FRAMES 512 /* frames whose flags one launch carries; longer batches take more launches */
#define KBN_AUGMENT_WORKSPACE_RECORD_BYTES 16
typedef struct kbn_augment_tensor {
    const float* src;
    float* dst;
    long long stride_n, stride_c, stride_h, stride_w; /* of src, in elements */
    int channels;
    int role;      /* KBN_AUGMENT_ROLE_* */
    int map_index; /* range maps: the map's index among the call's range maps (a word of the random counter) */
    int reserved;
} kbn_augment_tensor;
/* range: tensors non-NULL, count, n, height, width >= 1, a need of at most KBN_MAX_SIZE_BYTES; 0 otherwise, and 0 when no record is a
 * range map (nothing to select from).  kbn_augment_forward refuses a selection whose need is 0. */
size_t kbn_augment_workspace_bytes(const kbn_augment_tensor* tensors, int count, int n, int height, int width); /* 0 for bad arguments */
int kbn_augment_forward(const kbn_augment_tensor* tensors, int count, const unsigned char* flags, int n, int height, int width,
                        const float* densities, void* workspace, size_t workspace_bytes, int normalization, int noise_type,
                        float noise_spread, unsigned long long seed, unsigned call, int stages, kbn_stream_t stream);
int kbn_augment_forward_at(const kbn_augment_tensor* tensors, int count, const unsigned char* flags, int n, int height, int width,
                           const float* densities, void* workspace, size_t workspace_bytes, int normalization, int noise_type,
                           float noise_spread, unsigned long long seed, unsigned call, unsigned frame_base, int stages,
                           kbn_stream_t stream);

/* ------------------------------------------------- the training loop's image summaries ----
 *   depth_model.log_summary(summary_writer, tag, step, image0, image01, image02, output_depth0, ...)   reference src/kbnet.py:455-472
 * kbn_summary_panel_forward writes, in ONE launch, one finished panel of the reference's log_summary (src/kbnet_model.py:417-650):
 * the 3 x Hg x Wg fp32 tensor torchvision.utils.make_grid(torch.cat(rows, dim=2), nrow=n_display) returns, for `frames` frames
 * (the first `frames` of every source) and n_rows rows (2 .. KBN_SUMMARY_MAX_ROWS) of a left and a right height x width cell.
 *   frames > 1    panel 3 x (n_rows height + 4) x (frames (2 width + 2) + 2): make_grid's padding 2, pad_value 0; frame k's tile
 *                 at row 2, column k (2 width + 2) + 2
 *   frames == 1   panel 3 x (n_rows height) x (2 width): the tile itself, no padding
 * Every element of `panel` (dense) is written, padding and zero cells included; the sources are only read.  Cell kinds, each
 * operation rounded on its own in fp32 with IEEE division:
 *   ZERO        (right)  0                                                                           no source
 *   COPY        (left)   src[0], a 3-channel image, as it is
 *   PHOTO_ERR   (right)  inferno((((|a0 - b0| + |a1 - b1|) + |a2 - b2|) / 3) / 0.10f)                 a = src[0], b = src[1], 3 channels
 *   DEPTH       (left)   viridis(d / max_predict_depth)                                              d = src[0], 1 channel
 *   REL_ERR     (right)  inferno((v == 1 ? (|out - ref| + 1e-8f) / (ref + 1e-8f) : v) / 0.05f)       out, ref, v = src[0 .. 2], 1 channel
 * The colour lookup is matplotlib's Colormap.__call__ on float32 data: t = x * 256; t < 0 entry 0, t >= 256 entry 255, else entry
 * (int)t, NaN (0, 0, 0); the tables are matplotlib's `viridis` and `inferno` rounded to float32 (csrc/colormaps.h).
 * `rows` is a HOST array read before the call returns; the records travel in the kernel arguments (no device table, no allocation,
 * no synchronisation).  Sources may have any non-negative element strides; a cell whose sources have unit element stride, other
 * strides that are multiples of 4 and 16-byte aligned pointers is read with 16-byte loads when width % 4 == 0.
 * KBN_ERR_INVALID_ARGUMENT: NULL pointers, n_rows outside 2 .. 4, sizes < 1, a negative stride, a kind on the wrong side, a NaN
 * max_predict_depth; KBN_ERR_UNSUPPORTED: a COPY / PHOTO_ERR source that is not 3-channel, a DEPTH / REL_ERR source that is not
 * 1-channel, a panel of 2^31 elements or more -- all checked before anything is launched.
 *
 * kbn_summary_colorize_forward is the lookup alone (log_utils.colorize, reference src/log_utils.py:48-75): x, n frames of height x
 * width values at the given element strides -> out, n x 3 x height x width dense.  KBN_ERR_UNSUPPORTED for another colormap. */
#define KBN_SUMMARY_CELL_ZERO 0
#define KBN_SUMMARY_CELL_COPY 1
#define KBN_SUMMARY_CELL_PHOTO_ERR 2
#define KBN_SUMMARY_CELL_DEPTH 3
#define KBN_SUMMARY_CELL_REL_ERR 4
#define KBN_SUMMARY_COLORMAP_VIRIDIS 0
#define KBN_SUMMARY_COLORMAP_INFERNO 1
#define KBN_SUMMARY_MAX_ROWS 4
typedef struct kbn_summary_source {
    const float* data;
    long long stride_n, stride_c, stride_h, stride_w; /* in elements */
    int channels;
    int reserved;
} kbn_summary_source;
typedef struct kbn_summary_cell {
    int kind; /* KBN_SUMMARY_CELL_* */
    int reserved;
    kbn_summary_source src[3];
} kbn_summary_cell;
typedef struct kbn_summary_row {
    kbn_summary_cell left, right;
} kbn_summary_row;
int kbn_summary_panel_forward(const kbn_summary_row* rows, int n_rows, int frames, int height, int width, float max_predict_depth,
                              float* panel, kbn_stream_t stream);
int kbn_summary_colorize_forward(const float* x, long long stride_n, long long stride_h, long long stride_w, int n, int height, int width,
                                 int colormap, float* out, kbn_stream_t stream);

/* ------------------------------------------------- input pipeline ----
 * The reference reads every sample through PIL on one DataLoader worker:
 *   data_utils.load_image   Image.open(path).convert('RGB') -> float32   reference src/data_utils.py:58-85
 *   data_utils.load_depth   16-bit PNG / 256                              reference src/data_utils.py:123-152
 *   datasets.KBNetInferenceDataset.__getitem__: middle third of the image triplet
 *   (load_image_triplet), depth as 1 x H x W, intrinsics from .npy       reference src/datasets.py:22-46, 259-283
 *
 * kbn_png_info / kbn_png_decode: HOST-side PNG reader (zlib inflate + scanline filters; 8-bit
 * gray / RGB / RGBA / palette and 16-bit gray, non-interlaced) for pools of loader threads filling
 * pinned staging buffers.  `pixels` receives height x width x channels uint8 (palette expanded to
 * RGB), or height x width uint16 in host byte order for 16-bit files; *channels / *bit_depth say which.
 * KBN_ERR_UNSUPPORTED for interlaced files and other colour types / depths,
 * KBN_ERR_INVALID_ARGUMENT for damaged or truncated files and short output buffers. */
int kbn_png_info(const unsigned char* file, size_t file_bytes, int* width, int* height, int* channels,
                 int* bit_depth);
int kbn_png_decode(const unsigned char* file, size_t file_bytes, void* pixels, size_t pixels_bytes);
/* `n` files at once on `threads` host threads of the library's own (no interpreter lock involved);
 * status[i] (may be NULL) receives the per-file code, the return value is the first failure. */
int kbn_png_decode_batch(const unsigned char* const* files, const size_t* file_bytes, void* const* pixels,
                         const size_t* pixels_bytes, int n, int threads, int* status);

/* The output side -- data_utils.save_depth, reference src/data_utils.py:154-167 (np.uint32(z * 256.0) ->
 * Image.fromarray(mode='I').save(path): a 16-bit grayscale PNG, samples clipped at 65535), which run_kbnet.py --save_outputs
 * calls for the output, the filtered sparse depth and the ground truth (src/kbnet.py:1018-1026).
 *   kbn_depth_to_u16_forward   DEVICE: count depths (any shape, contiguous) -> samples = min(trunc(z * 256), 65535)
 *   kbn_png_encode_gray16      HOST: height x width samples (host byte order) -> a PNG file image in `out` (one IDAT, filter 0,
 *                              zlib `level` -1 .. 9); *out_bytes = its size.  out_capacity >= kbn_png_encode_gray16_bound(width,
 *                              height), else KBN_ERR_WORKSPACE.  Thread-safe, no GPU work: a pool of host threads writes a batch.
 * Readers (kbn_png_decode, PIL) recover the samples bit for bit; the file's bytes are not PIL's (other filters). */
int kbn_depth_to_u16_forward(const float* depth, unsigned short* samples, long long count, kbn_stream_t stream);
/* range: sides >= 1 and (1 + 2 width) x height < 2^32 (zlib counts in 32 bits); 0 otherwise */
size_t kbn_png_encode_gray16_bound(int width, int height);
int kbn_png_encode_gray16(const unsigned short* pixels, int width, int height, unsigned char* out, size_t out_capacity,
                          size_t* out_bytes, int level);

/* The whole export of a batch (src/kbnet.py:1007-1026: the normalised image as an 8-bit RGB PNG, two depth maps as 16-bit PNGs).
 *   kbn_export_pack_forward  DEVICE, ONE launch for all sources of the batch:
 *       image    n x 3 x height x width float32, dense, or NULL  ->  rgb n x height x width x 3 uint8, interleaved:
 *                clamp(trunc(scale * v + shift), 0, 255), NaN -> 0; product and sum each rounded to fp32 (no FMA), so float32 NumPy
 *                reproduces the bytes.  (255, 0) on an image in [0, 1] is the reference's (255 * image).astype(np.uint8), bit for
 *                bit; (127.5, 127.5) and (1, 0) give back the picture for the [-1, 1] and [0, 255] ranges (the reference's cast of
 *                those leaves the uint8 range: its files hold garbage there)
 *       depth_a, depth_b  n x 1 x height x width float32, dense, either or both NULL  ->  samples_a / samples_b n x height x width
 *                uint16 by kbn_depth_to_u16_forward's rule
 *     A thread owns 4 consecutive pixels of a row: 16-byte loads when width % 4 == 0 and all pointers are 16-byte aligned, scalar
 *     loads and stores otherwise.  Every output byte is written once; nothing but the n*h*w*3 / n*h*w*2 bytes is touched.
 *     KBN_ERR_INVALID_ARGUMENT, before anything is launched: an output without its source or a source without its output, nothing
 *     to do at all, n, height or width < 1.
 *   kbn_png_encode_rgb8      HOST: height x width x 3 interleaved uint8 -> a PNG file image, under kbn_png_encode_gray16's contract
 *                            (one IDAT, filter 0, level -1 .. 9, thread-safe, no GPU work; KBN_ERR_WORKSPACE when out_capacity <
 *                            kbn_png_encode_rgb8_bound(width, height)). */
int kbn_export_pack_forward(const float* image, float scale, float shift, const float* depth_a, const float* depth_b,
                            unsigned char* rgb, unsigned short* samples_a, unsigned short* samples_b, int n, int height, int width,
                            kbn_stream_t stream);
/* range: sides >= 1 and (1 + 3 width) x height < 2^32; 0 otherwise */
size_t kbn_png_encode_rgb8_bound(int width, int height);
int kbn_png_encode_rgb8(const unsigned char* pixels, int width, int height, unsigned char* out, size_t out_capacity,
                        size_t* out_bytes, int level);
/* HOST: height x width uint8 -> an 8-bit grayscale PNG, under kbn_png_encode_rgb8's contract (tools/unpack_dataset.py writes a
 * one-plane packed frame of 8 bits with it). */
/* range: sides >= 1 and (1 + width) x height < 2^32; 0 otherwise */
size_t kbn_png_encode_gray8_bound(int width, int height);
int kbn_png_encode_gray8(const unsigned char* pixels, int width, int height, unsigned char* out, size_t out_capacity,
                         size_t* out_bytes, int level);

/* Decoded pixels (device buffers) -> the tensors the reference's dataset returns:
 *   image_u8     N x height x raw_width x image_channels uint8 (1 gray, 3 RGB, 4 RGBA); columns
 *                [x_offset, x_offset + width) are taken (x_offset = width, raw_width = 3 * width for
 *                the middle image of a triplet)  ->  image N x 3 x height x width float32, values 0..255
 *                (normalize=False; gray replicated, alpha dropped = convert('RGB'))
 *   depth_raw    N x height x width uint16 (depth_bits 16) or uint8 (8)  ->  sparse_depth
 *                N x 1 x height x width float32 = value / 256
 * Either pair may be NULL.  kbn_preprocess_forward then derives the validity map, removes
 * outliers and normalises the image. */
int kbn_unpack_frames_forward(const unsigned char* image_u8, const void* depth_raw, float* image,
                              float* sparse_depth, int n, int height, int width, int raw_width,
                              int x_offset, int image_channels, int depth_bits, kbn_stream_t stream);

/* The TRAINING batch: what KBNetTrainingDataset.__getitem__ returns (reference src/datasets.py:199-225), batched, from the decoded
 * bytes of `n` image triplets and their depth maps -- the triplet split (load_image_triplet, :22-46), the crop (random_crop's
 * slices, :143-148), uint8 -> float32 and depth / 256 in ONE launch per KBN_UNPACK_TRAIN_MAX_FRAMES frames.
 *   images       a packed buffer of `image_bytes` bytes; frame i's triplet is height_i x raw_width_i x image_channels uint8
 *                (1 gray, 3 RGB, 4 RGBA; the same for all frames) at byte image_offset_i, raw_width_i = 3 x W_i
 *   depths       a packed buffer of `depth_bytes` bytes; frame i's samples are height_i x W_i uint16 (depth_bits 16, host byte
 *                order, depth_offset_i even) or uint8 (8) at byte depth_offset_i
 *   frames       a HOST array of n records, read before the call returns; they travel to the device in the kernel arguments
 *                (no device table, no copy, no allocation).  Frames may differ in size; the crop `height` x `width` is one.
 *   image0 / image1 / image2   n x 3 x height x width float32, values 0..255: the middle (t), left (t-1) and right (t+1) third
 *                of the triplet; output pixel (y, x) of frame i is raw pixel (y_start_i + y, x_start_i + x) of that third
 *                (gray replicated, alpha dropped)
 *   sparse_depth0              n x 1 x height x width float32 = sample / 256
 * A thread writes four consecutive pixels of a row of all four tensors, with 16-byte stores when width % 4 == 0 and the four
 * outputs are 16-byte aligned.  Pure data movement and exact conversions: the results are the reference's bits.
 * Checked for every record before anything is launched -- KBN_ERR_INVALID_ARGUMENT: a NULL pointer, n < 1, height or width < 1,
 * a raw width that is not 3 x W, a crop that leaves its frame (y_start < 0, y_start + height > height_i, x_start < 0,
 * x_start + width > W_i), a negative or (16-bit depth) odd offset, a frame that does not lie inside its packed buffer;
 * KBN_ERR_UNSUPPORTED: other image_channels / depth_bits, a crop of more than 2^31 - 1 four-pixel groups. */
#define KBN_UNPACK_TRAIN_MAX_FRAMES 64 /* records a launch carries (2 KB of its argument block); longer batches take more launches */
typedef struct kbn_train_frame {
    long long image_offset; /* bytes, into `images` */
    long long depth_offset; /* bytes, into `depths` */
    int height;             /* raw rows of the triplet and of the depth map */
    int raw_width;          /* raw columns of the triplet: 3 x W */
    int y_start, x_start;   /* the crop's first row and its first column inside each third */
} kbn_train_frame;
int kbn_unpack_train_frames_forward(const unsigned char* images, size_t image_bytes, const unsigned char* depths, size_t depth_bytes,
                                    const kbn_train_frame* frames, int n, int height, int width, int image_channels, int depth_bits,
                                    float* image0, float* image1, float* image2, float* sparse_depth0, kbn_stream_t stream);

/* The packed frame store: a lossless container the loaders read in place of PNG files, decoded on the DEVICE.  One file
 * holds height x width x channels samples (channels 1, 3 or 4; 8 or 16 bits), stored per plane in groups of 8 rows and segments of
 * 16 samples, every segment with a bit width of its own (version 1; the layout is written down in DESIGN 8t and csrc/frame_pack.h).
 * HOST functions, thread-safe, no GPU work:
 *   kbn_frame_info          reads the 32-byte header (file_bytes >= 32 is enough)
 *   kbn_frame_encode_bound  the capacity kbn_frame_encode needs for these sizes; 0 for sizes it refuses
 *   kbn_frame_encode        samples: height x width x channels interleaved, uint8 or (bits 16) uint16 in host byte order -> the file
 *                           image in `out`, *out_bytes its size; KBN_ERR_WORKSPACE when out_capacity < the bound
 *   kbn_frame_decode        the inverse, after kbn_frame_check; samples_bytes >= height x width x channels x bits / 8
 *   kbn_frame_check         the complete structural check: magic and version constants, sizes, payload_bytes against file_bytes,
 *                           zero padding, a table that starts at 0, is monotone and ends at payload_bytes, every header byte <= bits,
 *                           every (group, plane) payload exactly its header bytes plus the bytes of its segments.  EVERY file
 *                           passes it before its bytes reach kbn_unpack_packed_frames_forward.
 * KBN_ERR_INVALID_ARGUMENT: NULL pointers, sizes < 1, a damaged or truncated file, a short output; KBN_ERR_UNSUPPORTED: other
 * channels / bits / version constants, an image whose encoding could pass 4 GiB (the table's offsets are 32-bit). */
int kbn_frame_info(const unsigned char* file, size_t file_bytes, int* width, int* height, int* channels, int* bits);
/* range: sides >= 1, channels 1, 3 or 4, bits 8 or 16, a bound of at most KBN_MAX_SIZE_BYTES; 0 otherwise.  kbn_frame_encode itself takes frames whose bound is below 4 GiB */
size_t kbn_frame_encode_bound(int width, int height, int channels, int bits);
int kbn_frame_encode(const void* samples, int width, int height, int channels, int bits, unsigned char* out, size_t out_capacity,
                     size_t* out_bytes);
int kbn_frame_decode(const unsigned char* file, size_t file_bytes, void* samples, size_t samples_bytes);
int kbn_frame_check(const unsigned char* file, size_t file_bytes);

/* kbn_unpack_train_frames_forward from PACKED files: `images` and `depths` are device buffers that hold the packed files of the
 * batch's triplets (image_channels planes of 8 bits, raw_width_i = 3 x W_i wide) and depth maps (one plane of depth_bits, W_i wide)
 * as they are on disk, each at a 16-byte-aligned offset; both buffers are 16-byte aligned.  Outputs, crop and records as there, the
 * record also carrying the two files' sizes.  image1 and image2 may be NULL: then only the middle third is decoded (inference).
 * One launch per KBN_UNPACK_TRAIN_MAX_FRAMES frames, one workgroup per (frame, group of 8 rows that the crop touches, plane); integer
 * work, no atomics, the same bits on every run, and the bits kbn_unpack_train_frames_forward gives for the decoded samples.
 * The files must have passed kbn_frame_check on the host.  The kernel never reads outside a file: it compares header, table and
 * header bytes with the record and with each other first, and leaves the outputs of a (frame, group, plane) that disagrees unwritten.
 * Checked for every record before anything is launched -- KBN_ERR_INVALID_ARGUMENT: a NULL pointer other than image1 / image2,
 * misaligned buffers, n < 1, height or width < 1, a raw width that is not 3 x W, a crop that leaves its frame, a negative or
 * misaligned offset, a file too short for its header and table or not inside its buffer; KBN_ERR_UNSUPPORTED: other image_channels /
 * depth_bits, a raw width above KBN_UNPACK_PACKED_MAX_RAW_WIDTH (a group's segment offsets, 4 bytes each, live in LDS: 32 KB there). */
#define KBN_UNPACK_PACKED_MAX_RAW_WIDTH 16384
typedef struct kbn_packed_frame {
    long long image_offset;   /* bytes, into `images`; a multiple of 16 */
    long long depth_offset;   /* bytes, into `depths`; a multiple of 16 */
    unsigned int image_bytes; /* the packed triplet's file size */
    unsigned int depth_bytes; /* the packed depth map's file size */
    int height;               /* raw rows of the triplet and of the depth map */
    int raw_width;            /* raw columns of the triplet: 3 x W */
    int y_start, x_start;     /* the crop's first row and its first column inside each third */
} kbn_packed_frame;
int kbn_unpack_packed_frames_forward(const unsigned char* images, size_t image_bytes, const unsigned char* depths, size_t depth_bytes,
                                     const kbn_packed_frame* frames, int n, int height, int width, int image_channels, int depth_bits,
                                     float* image0, float* image1, float* image2, float* sparse_depth0, kbn_stream_t stream);

/* kbn_unpack_train_frames_forward for samples that name their three frames one by one: what load_image_triplet (reference
 * src/datasets.py:22-46) makes of the concatenation of frames t-1, t, t+1, from the three frames where each lies -- no triplet is
 * ever assembled.  Frame k of sample i (0 previous -> image1, 1 current -> image0, 2 next -> image2) is height_i x width_i x
 * image_channels uint8 at byte image_offset_i[k] of `images`; width_i is a FRAME's width W_i, the depth map's too.  The three offsets
 * of a sample may coincide (the reference's validation and testing triplets are one frame three times, setup_dataset_kitti.py:514-516)
 * and samples may share frames.  Outputs, crop (random_crop's slices, src/datasets.py:143-148), conversions and the 16-byte-store /
 * float-by-float split are kbn_unpack_train_frames_forward's; so are the bits, for the triplet np.concatenate makes of the frames.
 * One launch per KBN_UNPACK_SEQUENCE_MAX_FRAMES samples, the records by value in the kernel arguments.
 * Checked for every record before anything is launched -- KBN_ERR_INVALID_ARGUMENT: a NULL pointer, n < 1, height or width < 1, a
 * frame size < 1, a crop that leaves its frame (y_start < 0, y_start + height > height_i, x_start < 0, x_start + width > width_i),
 * a negative or (16-bit depth) odd offset, one of the three frames or the depth map not inside its buffer; KBN_ERR_UNSUPPORTED:
 * other image_channels / depth_bits, a crop of more than 2^31 - 1 four-pixel groups. */
#define KBN_UNPACK_SEQUENCE_MAX_FRAMES 48 /* records a launch of either sequence entry point carries: 48 x 64 bytes of the packed record = 3 KB of the argument block */
typedef struct kbn_sequence_frame {
    long long image_offset[3]; /* bytes, into `images`: previous, current, next */
    long long depth_offset;    /* bytes, into `depths` */
    int height;                /* rows of each frame and of the depth map */
    int width;                 /* columns of each frame and of the depth map: W */
    int y_start, x_start;      /* the crop's first row and first column in every frame */
} kbn_sequence_frame;
int kbn_unpack_sequence_frames_forward(const unsigned char* images, size_t image_bytes, const unsigned char* depths, size_t depth_bytes,
                                       const kbn_sequence_frame* frames, int n, int height, int width, int image_channels,
                                       int depth_bits, float* image0, float* image1, float* image2, float* sparse_depth0,
                                       kbn_stream_t stream);

/* kbn_unpack_packed_frames_forward for three packed files a sample: frame k of sample i is a packed file of
 * image_channels planes of 8 bits, width_i wide, image_bytes_i[k] long, at the 16-byte-aligned offset image_offset_i[k]; the depth map
 * one plane of depth_bits, width_i wide.  Offsets may coincide and be shared, as above.  image1 and image2 may be NULL: then only the
 * CURRENT file of every sample is decoded (KBNetInferenceDataset.__getitem__, reference src/datasets.py:259-283, on a sequence entry).
 * One launch per KBN_UNPACK_SEQUENCE_MAX_FRAMES samples; one workgroup per (sample, which of the three files or the depth map, group of
 * 8 rows that the crop touches, plane).  Every file starts at segment 0 of its rows, so the crop's first column sits at x_start of
 * its file, where a triplet's second and third frame start mid-segment unless W % 16 == 0.  The decoder's discipline is
 * kbn_unpack_packed_frames_forward's: the files must have passed kbn_frame_check; the kernel compares header, table and header bytes
 * with the record and with each other before it reads, leaves the outputs of a unit that disagrees unwritten, and never reads
 * outside a file.  The bits are kbn_unpack_sequence_frames_forward's for the decoded samples.
 * Checked for every record before anything is launched -- KBN_ERR_INVALID_ARGUMENT: a NULL pointer other than image1 / image2 (one
 * of the two alone is refused), misaligned buffers, n < 1, height or width < 1, a frame size < 1, a crop that leaves its frame, a
 * negative or misaligned offset, a file (all three are checked, whatever is decoded) too short for its header and table or not
 * inside its buffer; KBN_ERR_UNSUPPORTED: other image_channels / depth_bits, a width above KBN_UNPACK_PACKED_MAX_RAW_WIDTH. */
typedef struct kbn_packed_sequence_frame {
    long long image_offset[3];   /* bytes, into `images`, multiples of 16: previous, current, next */
    long long depth_offset;      /* bytes, into `depths`; a multiple of 16 */
    unsigned int image_bytes[3]; /* the three packed files' sizes */
    unsigned int depth_bytes;    /* the packed depth map's file size */
    int height;                  /* rows of each frame and of the depth map */
    int width;                   /* columns of each frame and of the depth map: W */
    int y_start, x_start;        /* the crop's first row and first column in every frame */
} kbn_packed_sequence_frame;
int kbn_unpack_packed_sequence_frames_forward(const unsigned char* images, size_t image_bytes, const unsigned char* depths,
                                              size_t depth_bytes, const kbn_packed_sequence_frame* frames, int n, int height, int width,
                                              int image_channels, int depth_bits, float* image0, float* image1, float* image2,
                                              float* sparse_depth0, kbn_stream_t stream);

/* The device ENCODER of the packed frame store (csrc/pack_frames.hip): n frames of one size -> n file images, each byte
 * for byte what kbn_frame_encode writes for the same samples (header, table, zero padding up to the payload, payload).
 *   kbn_pack_frames_stride           capacity of one frame's slot: kbn_frame_encode_bound rounded up to 16; 0 for sizes the encoder
 *                                    refuses
 *   kbn_pack_frames_workspace_bytes  device bytes a call needs (a payload length per (frame, group, plane), a byte per segment); 0
 *                                    for sizes the encoder refuses and n < 1
 *   kbn_pack_frames_forward
 *     samples    n x height x width x channels interleaved, uint8 or (bits 16) uint16 (2-byte aligned), dense, on the DEVICE -- per
 *                frame exactly what kbn_frame_encode takes on the host
 *     out        frame i's file image at out + i * out_stride (out 16-byte aligned, out_stride a multiple of 16 and >=
 *                kbn_pack_frames_stride); out_bytes[i] (8-byte aligned): its size, written by the device.  Bytes of a slot past
 *                out_bytes[i], and anything outside the slots, stay as they were.
 *     workspace  workspace_bytes >= kbn_pack_frames_workspace_bytes device bytes, 4-byte aligned; no allocation in here
 * Three launches whatever n is (sizes, table, emit), no host synchronisation, integer work: the same bytes on every run.
 * Before anything is launched -- KBN_ERR_INVALID_ARGUMENT: NULL pointers, sizes < 1, a misaligned pointer, a stride that is short
 * or not a multiple of 16; KBN_ERR_WORKSPACE: a short workspace; KBN_ERR_UNSUPPORTED: other channel counts or bit widths, an
 * encoding that could pass 4 GiB, n x ceil(height / 8) > 2^31 - 1 (the grid's first dimension), a width above
 * KBN_PACK_FRAMES_MAX_WIDTH, the samples of one plane row.  The cap is the emit kernel's LDS budget: it keeps one byte offset of 4
 * bytes for each of the 8 x ceil(width / 16) segments of a (group, plane) in LDS, 2 x width bytes = 32 KB at the cap, beside the
 * 8.2 KB image it assembles the payload in -- 40.2 KB of the 64 KB a workgroup gets without opting in to more (the decoder's
 * KBN_UNPACK_PACKED_MAX_RAW_WIDTH is the same budget). */
#define KBN_PACK_FRAMES_MAX_WIDTH 16384
/* range: kbn_frame_encode_bound's range, width <= KBN_PACK_FRAMES_MAX_WIDTH, a bound below 4 GiB; 0 otherwise */
size_t kbn_pack_frames_stride(int width, int height, int channels, int bits);
/* range: n >= 1 and kbn_pack_frames_stride's range; 0 otherwise */
size_t kbn_pack_frames_workspace_bytes(int n, int width, int height, int channels, int bits);
int kbn_pack_frames_forward(const void* samples, int n, int width, int height, int channels, int bits, unsigned char* out,
                            size_t out_stride, unsigned long long* out_bytes, void* workspace, size_t workspace_bytes,
                            kbn_stream_t stream);

/* Point clouds (csrc/point_cloud.hip): n depth maps of height x width backprojected to the vertex records of binary
 * little-endian PLY files, on the device.  Frame i's slot, out + i * out_stride, receives one packed record per KEPT pixel in
 * row-major pixel order -- float x, y, z, then uchar r, g, b when `image` is given: 15 bytes a record, 12 without, no padding --
 * and out_points[i] their number.
 *   depth       n x 1 x height x width float32, dense planes, frame i at depth + i * depth_batch_stride (elements): a channel slice
 *               of a wider tensor works; 4-byte aligned (16-byte loads where an address allows them)
 *   image       NULL, or n x 3 x height x width float32, contiguous: the NORMALISED image; a byte is kbn_export_pack_forward's rgb
 *               rule under the same scale and shift, so the colours are the image file's pixels
 *   kinv        n x 3 x 3 float32: what kbn_intrinsics_inverse(K, 1, 1) wrote
 *   kept        a pixel is kept iff its depth d is finite, d > 0, d >= min_depth and d <= max_depth: NaN, +-Inf, zero and negatives
 *               never are (0 and +Inf as the range keep every finite depth above 0)
 *   point       component j is c_j * d, ONE product rounded to fp32, where c_j is bit for bit what kbn_camera_coordinates stores
 *               for the pixel: fmaf(k[3j+1], (float)y, k[3j] * (float)x) + k[3j+2] with integer pixel coordinates
 *               (csrc/camera_coordinate.h states it for both)
 *   out         any alignment; out_stride >= height * width * record bytes.  Nothing outside [0, out_points[i] * record) of a slot
 *               is written, nothing outside the slots either.  out_points: 8-byte aligned int64, written by the device.
 *   workspace   workspace_bytes >= kbn_point_cloud_workspace_bytes(n, height, width) device bytes (4 a tile of 1024 pixels), 4-byte
 *               aligned; nothing past that size is touched; no allocation in here
 * Three launches whatever n is (count, scan, emit), no atomics, no host synchronisation: the bytes are a function of the arguments.
 * Before anything is launched -- KBN_ERR_INVALID_ARGUMENT: a NULL pointer (a NULL image alone is legal), n, height or width < 1, a
 * misaligned pointer, a short out_stride; KBN_ERR_WORKSPACE: a short workspace; KBN_ERR_UNSUPPORTED: height * width > 2^31 - 1 or
 * n x ceil(height * width / 1024) > 2^31 - 1 (the grid's first dimension). */
/* range: n, height, width >= 1 and the two products above; 0 otherwise.  Swept over extreme arguments under the sanitizers by a
 * program of its own, tests/host_san/point_cloud_size_sweep.cpp (tests/test_point_cloud_sanitizers_cpu.py), not by
 * tests/host_san/size_sweep.cpp, whose driver links a fixed list of sources and finds its functions by lines that begin
 * with the return type: hence the comment in front of this one. */
/* own sweep */ size_t kbn_point_cloud_workspace_bytes(int n, int height, int width);
int kbn_point_cloud_forward(const float* depth, long long depth_batch_stride, const float* image, float scale, float shift,
                            const float* kinv, float min_depth, float max_depth, int n, int height, int width, unsigned char* out,
                            size_t out_stride, long long* out_points, void* workspace, size_t workspace_bytes, kbn_stream_t stream);

/* TensorBoard's default histogram of an fp32 device tensor -- what SummaryWriter.add_histogram(bins='tensorflow') computes on the
 * host, np.histogram(values.astype(float), bins=edges) with min, max, sum and values.dot(values) -- in one pass (csrc/histogram.hip).
 *   x               n float32, dense, 4-byte aligned (16-byte loads from the first 16-byte boundary on)
 *   positive_edges  DEVICE: the KBN_HISTOGRAM_POSITIVE_EDGES positive edges as float64, increasing -- v = 1e-12; while v < 1e20:
 *                   append v, v *= 1.1 in float64, by repeated multiplication.  The edges are these, mirrored negative, 0 between:
 *                   E[774] = 0, E[775 + k] = P[k], E[773 - k] = -P[k]
 *   counts          KBN_HISTOGRAM_BINS int32: bin i counts the x, widened to float64, with E[i] <= x < E[i + 1]; the last bin is
 *                   closed on the right; x outside [E[0], E[1548]], NaN and +-inf are counted in no bin
 *   stats           4 float64: min, max (NaN propagates, as np.min / np.max), sum, sum of squares, all over ALL n values
 *   workspace       KBN_HISTOGRAM_WORKSPACE_BYTES device bytes, 8-byte aligned (one record a workgroup)
 * Two launches behind a memset of `counts`: integer LDS atomics, one integer global add per non-empty bin and workgroup, the float64
 * sums as per-workgroup records folded by the second launch in a fixed order -- two runs give the same bits.
 * KBN_ERR_INVALID_ARGUMENT, before anything is launched: a NULL or misaligned pointer, n < 1; KBN_ERR_WORKSPACE: a short
 * workspace; KBN_ERR_UNSUPPORTED: n > 2^31 - 1 (the counts are 32-bit). */
#define KBN_HISTOGRAM_POSITIVE_EDGES 774
#define KBN_HISTOGRAM_BINS 1548
#define KBN_HISTOGRAM_WORKSPACE_BYTES 32768
int kbn_histogram_forward(const float* x, long long n, const double* positive_edges, int* counts, double* stats, void* workspace,
                          size_t workspace_bytes, kbn_stream_t stream);

/* HOST: CRC-32C (Castagnoli) of `bytes` bytes, continued from `crc` (0 to begin): the checksum of an event file's records
 * (kb.summary.EventWriter).  kbn_crc32c("123456789", 9, 0) == 0xE3069283.  Thread-safe, no GPU work. */
unsigned int kbn_crc32c(const unsigned char* data, size_t bytes, unsigned int crc);

#ifdef __cplusplus
}
#endif
#endif /* KBNET_HIP_H */
