// Shared device/host helpers for the KBNet gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "../../include/kbnet_hip.h"

#define KBN_CHECK_LAUNCH()                                   \
    do {                                                     \
        hipError_t e__ = hipGetLastError();                  \
        if (e__ != hipSuccess) return KBN_ERR_LAUNCH;        \
    } while (0)

namespace kbn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
// HOST: the layer shapes the plan makers and size functions take (include/kbnet_hip.h states them).  ceil_div and round_up work in
// int, a + b - 1 included, and so do the plans built from them: every size function and every entry point that makes a plan asks
// this first and answers 0 / KBN_ERR_UNSUPPORTED outside it, so that no plan is ever made from a count near INT_MAX.
inline bool layer_shape_ok(int out_channels, int in_channels, int kernel_size) {
    return out_channels >= 1 && in_channels >= 1 && kernel_size >= 1 && kernel_size <= 7 && out_channels <= KBN_MAX_CHANNELS &&
           in_channels <= KBN_MAX_CHANNELS &&
           (long long)out_channels * in_channels * kernel_size * kernel_size <= (long long)KBN_MAX_WEIGHT_ELEMENTS;
}

__device__ __forceinline__ float leaky_relu(float v, float slope) { return v > 0.f ? v : v * slope; }
// |v| for the running maxima behind the fp16 windows (absmax slots, per-tile maxima): 0 for Inf and NaN
__device__ __forceinline__ float fin_abs(float v) { const float a = fabsf(v); return a < __builtin_inff() ? a : 0.f; }

// ---- per-frame activation statistics ("absmax slots") ------------------------------------------------
// A slot is one unsigned per frame: the bit pattern of max |a| over a tensor's frame (bit patterns of non-negative
// floats order like the floats).  The caller zeroes the slots; every conv kernel folds the values it stores into the
// slot of its output tensor (out_absmax) in its epilogue; the split-operand kernels read the slots of their inputs
// (kbn_conv_src.absmax) and place their fp16 window on them (sp_act_scale, conv_split.hip) -- the exponent follows the
// data of THIS forward, frame by frame, with no host round trip and no state between calls.
// `m` >= 0: this thread's maximum over the FINITE values (fin_abs: an Inf or NaN counts as 0).  A window placed on an Inf maximum
// would be 2^-100 and flush every finite value of the frame to zero; the non-finite values themselves still propagate through
// the convs (a split of Inf is Inf / NaN), as in the reference.  One atomic per wave, and only when the wave
// would raise the slot (the plain load may be stale -- then the atomic is merely redundant).
// Bit pattern of the maximum of a NON-NEGATIVE float over the wave, wave-uniform (an SGPR).  DPP butterflies inside each row of 16
// lanes (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror: max is idempotent, any covering pattern does), then the four rows
// meet through v_readlane + s_max_u32.  No LDS crossbar: __shfl_xor is ds_bpermute_b32 with a per-lane address register for every
// distance -- six registers that hipcc computes in a kernel's prologue, and in a kernel at its register limit SPILLS, so that every
// step of the reduction became scratch_load + s_waitcnt vmcnt(0), i.e. a wait for all the stores the epilogue had just issued
// (kb1_front_kernel<.., NEXT>: + 330 us per 32 KITTI frames, round 5).
// PRECONDITION: the whole wave is active at the call (EXEC = all ones).  v_readlane of an inactive lane returns whatever its register
// holds, and lanes 0 / 16 / 32 / 48 are read unconditionally.  Every call site sits in wave-convergent code (after the epilogue's loops,
// with out-of-image lanes contributing 0 instead of leaving); a caller inside divergent control flow must reduce another way.
__device__ __forceinline__ unsigned wave_max_bits(float m) {
#define KBN_DPP_MAX(ctrl) m = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), ctrl, 0xf, 0xf, true)))
    KBN_DPP_MAX(0xB1);    // quad_perm [1, 0, 3, 2]
    KBN_DPP_MAX(0x4E);    // quad_perm [2, 3, 0, 1]
    KBN_DPP_MAX(0x141);   // row_half_mirror
    KBN_DPP_MAX(0x140);   // row_mirror
#undef KBN_DPP_MAX
    const int v = __float_as_int(m);
    const unsigned a = (unsigned)__builtin_amdgcn_readlane(v, 0), b = (unsigned)__builtin_amdgcn_readlane(v, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane(v, 32), d = (unsigned)__builtin_amdgcn_readlane(v, 48);
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;   // non-negative floats order like their bit patterns
}
// x + its three quad neighbours (lanes 4 q .. 4 q + 3), in every lane of the quad: two DPP quad_perm moves instead of two ds_bpermute
__device__ __forceinline__ float quad_sum(float x) {
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));   // quad_perm [1, 0, 3, 2]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true));   // quad_perm [2, 3, 0, 1]
    return x;
}
__device__ __forceinline__ void absmax_commit(unsigned* slot, float m) {
    const unsigned b = wave_max_bits(m);
    if ((threadIdx.x & 63) == 0) {
        if (b > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, b);
    }
}
// max |x| of each of n frames of per_frame contiguous floats into slots[n] (csrc/conv_split.hip): the stand-alone pass
// for tensors whose producer did not fill a slot (inputs of a drop-in module call, outputs of the fallback kernels)
int absmax_frames_launch(const float* x, long long batch_stride, int n, long long per_frame, unsigned* slots, hipStream_t stream);

// ---- per-device one-time kernel setup -------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a property of (kernel, device): one bit per device
// ordinal of the calling thread's current device, so that a process driving several GPUs (the reference
// wraps its modules in torch.nn.DataParallel, src/kbnet_model.py:408-415) sets it on each of them.
struct DeviceOnce {
    std::atomic<unsigned long long> done[4] = {};   // 256 device ordinals
};
inline int set_max_dynamic_lds(DeviceOnce& once, const void* kernel, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return KBN_ERR_LAUNCH;
    const unsigned long long bit = 1ull << (dev & 63);
    std::atomic<unsigned long long>& word = once.done[(dev >> 6) & 3];
    if (word.load(std::memory_order_relaxed) & bit) return KBN_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return KBN_ERR_LAUNCH;   // not a stream operation: legal while a stream is being captured
    word.fetch_or(bit, std::memory_order_relaxed);
    return KBN_OK;
}
// One launch of the kernel (instantiation) K with `lds` bytes of dynamic LDS, its limit raised to MAX_LDS bytes once per device.
// The flag that records the raise is lds_once<K>: it belongs to K by construction, no call site pairs a flag with a kernel by hand
// (a wrong pairing compiles, works on the first device and fails on a second one only).  The caller checks the launch (KBN_CHECK_LAUNCH).
template <auto K>
inline DeviceOnce lds_once;
template <auto K, int MAX_LDS, class... Args>
int launch_lds(unsigned blocks, unsigned threads, size_t lds, hipStream_t stream, const Args&... args) {
    if (int rc = set_max_dynamic_lds(lds_once<K>, reinterpret_cast<const void*>(K), MAX_LDS)) return rc;
    hipLaunchKernelGGL(K, dim3(blocks), dim3(threads), lds, stream, args...);
    return KBN_OK;
}
// f(std::bool_constant<flags>...): run-time flags (in the kernel's template order) as compile-time ones.  Instantiates f for every
// combination of the flags passed; a form that lacks a flag does not pass it.
template <class F>
int flag_dispatch(F&& f) { return f(); }
template <class F, class... Flags>
int flag_dispatch(F&& f, bool flag, Flags... rest) {
    auto bind = [&](auto c) { return flag_dispatch([&](auto... more) { return f(c, more...); }, rest...); };
    return flag ? bind(std::true_type{}) : bind(std::false_type{});
}
int device_cu_count();   // abi.hip: compute units of the current device (cached per device), <= 0 on error

// ---- debug / experiment knobs ------------------------------------------------------------------------
// Read from the environment ONCE when the library is loaded (and again by kbn_reload_env(), which tests
// and the ablation tools call after changing a variable): no getenv on any launch path.
enum Knob {
    KNOB_DEBUG, KNOB_FORCE_MW, KNOB_FORCE_TWB, KNOB_EPI_LDS, KNOB_NO_WINO,
    KNOB_NO_UP2X9, KNOB_NO_UP2X3, KNOB_WINO_RT,
    KNOB_NO_KB_PAIR, KNOB_NO_KB_DEPTH_FUSION, KNOB_PAIR_CAND, KNOB_S2D_DEBUG, KNOB_AUTOTUNE,
    KNOB_NO_HEAD_FUSION, KNOB_NO_SPLIT,
    // switches of the host mirror (modules.py asks kbn_knob(): one reading of the environment for both sides)
    KNOB_NO_OVERLAP, KNOB_NO_PAIR, KNOB_NO_PAIR_MID, KNOB_NO_PAIR_ENC, KNOB_NO_PAIR_TAIL, KNOB_NO_DEPTH_FRONT_FUSION,
    KNOB_FP16_ONE_TERM, KNOB_DEPTH_FRONT_FUSION, KNOB_NO_FRONT_NEXT, KNOB_COUNT
};
struct KnobValue { int set, value; };
extern KnobValue g_knobs[KNOB_COUNT];
inline int knob(Knob k) { return g_knobs[k].value; }        // 0 when unset
inline bool knob_set(Knob k) { return g_knobs[k].set != 0; }

// XCD-aware block remap (bijective for any grid size): the dispatcher places block b on
// XCD b % 8; give every XCD one contiguous range of logical tiles so that neighbouring
// tiles (which share input halos / weight panels) hit the same 4 MiB L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblocks) {
    const int NX = 8;
    int xcd = bid % NX, idx = bid / NX;
    int q = nblocks / NX, r = nblocks % NX;
    int start = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + idx;
}

// PyTorch's nearest-neighbour source index (aten/src/ATen/native/UpSample.h
// nearest_idx): identity when sizes match, >>1 for an exact 2x, else
// min(floor(dst * (float)in/out), in-1).
__device__ __forceinline__ int nearest_src_index(int dst, int in_size, int out_size) {
    if (in_size == out_size) return dst;
    if (out_size == 2 * in_size) return dst >> 1;
    float scale = (float)in_size / (float)out_size;
    int s = (int)floorf((float)dst * scale);
    return s < in_size - 1 ? s : in_size - 1;
}

// ---- route record of the fp32 conv family (kbn_conv_last_route) ------------------------------------------
// HOST bookkeeping only: which kernel instantiation conv2d_launch / the 2x up-conv launcher last launched on the calling
// thread, written by the launcher of that instantiation right after its launch succeeded.  The entry points clear it when
// they are entered and again when they fail, so a declined or failed call reads as family 0.  Field order = kbn_conv_last_route's.
enum RouteFamily {
    ROUTE_NONE = 0, ROUTE_WINO = 1, ROUTE_DMA = 2, ROUTE_DMA_SYN = 3, ROUTE_IGEMM_PIPE = 4, ROUTE_IGEMM = 5,
    ROUTE_UP2X9 = 6, ROUTE_UP2X_DMA = 7, ROUTE_UP2X = 8
};
struct ConvRoute {
    int family, ks, stride, ck, nb, mw, twb, wino_rt, wino_ct, epi_lds, up_form, up_granule, up_half, reserved[3];
};
static_assert(sizeof(ConvRoute) == KBN_CONV_ROUTE_FIELDS * sizeof(int), "kbn_conv_last_route copies the struct as ints");
ConvRoute& conv_route();   // abi.hip: the calling thread's record
inline void route_clear() { conv_route() = ConvRoute{}; }
inline void route_conv(int family, int ks, int stride, int ck, int nb, int mw, int twb, int epi_lds) {
    ConvRoute r{};
    r.family = family; r.ks = ks; r.stride = stride; r.ck = ck; r.nb = nb; r.mw = mw; r.twb = twb; r.epi_lds = epi_lds;
    conv_route() = r;
}
inline void route_up2x(int family, int nb, int mw, int twb, int form, int granule, int half) {
    ConvRoute r{};
    r.family = family; r.ks = 3; r.stride = 1; r.ck = 8; r.nb = nb; r.mw = mw; r.twb = twb;
    r.up_form = form; r.up_granule = granule; r.up_half = half;
    conv_route() = r;
}

// conv_igemm.hip
int conv2d_launch(const kbn_conv_src* srcs, int n_src, const float* packed_weight, float* out,
                  long long out_batch_stride, int n, int out_channels, int kernel_size, int stride,
                  int in_height, int in_width, int resize, int apply_activation, float negative_slope,
                  unsigned* out_absmax, hipStream_t stream);

}  // namespace kbn
