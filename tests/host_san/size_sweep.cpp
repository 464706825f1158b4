// size_sweep -- every size_t-returning pure function of include/kbnet_hip.h over extreme arguments, in a build with
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_host_sanitizers_cpu.py builds and runs it).  Python allocates from
// these answers what the kernels then write, so an answer must be 0 (a refusal) or at least as large as the data it is for:
//   - no sanitizer report (the build aborts at the first);
//   - 0 whenever a dimension is <= 0 or a kernel size, stride, mode, channel count or bit width is not a legal one;
//   - a nonzero answer is never below a floor computed here in unsigned __int128: two bytes a weight for the packed-weight
//     functions, the raw samples for the frame and PNG bounds -- what a wrapped product would miss;
//   - one ordinary call of every function answers nonzero, so that "always 0" does not pass.
// No call here takes a pointer to GPU memory or launches anything.
// usage: size_sweep            every function
//        size_sweep --list     their names
//        size_sweep NAME...    these only (the driver runs one process a function, so that one report does not hide the next)
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include <sanitizer/common_interface_defs.h>

#include "../../include/kbnet_hip.h"

typedef unsigned __int128 u128;
typedef std::vector<int> Ints;

static const Ints WIDE = {INT_MIN, -1, 0, 1, 3, 16, 48, 384, 512, 1216, 4096, 65535, 65536, 1 << 20, 1 << 24, INT_MAX / 2, INT_MAX - 1, INT_MAX};

struct Arg {
    const char* name;
    Ints values;       // what it ranges over
    Ints legal;        // empty: any value >= 1 may be legal; else: exactly these
    bool any_sign;     // true: values <= 0 are legal too (a flag, a count that may be "choose for me")
};
static Arg dim(const char* name) { return Arg{name, WIDE, {}, false}; }
static Arg one_of(const char* name, Ints legal, int illegal) {
    Ints v = legal;
    v.push_back(illegal);
    return Arg{name, v, legal, true};      // the list decides, not the sign (mode 0 is a mode)
}
// a dimension only a few values of which are legal: the whole wide range and the legal values
static Arg dim_of(const char* name, Ints legal) {
    Ints v = WIDE;
    for (int x : legal) v.push_back(x);
    return Arg{name, v, legal, false};
}
static Arg flag(const char* name, Ints values) { return Arg{name, values, {}, true}; }

struct Function {
    const char* name;
    std::vector<Arg> args;
    std::function<size_t(const Ints&)> call;
    std::function<u128(const Ints&)> floor;
    Ints ordinary;                                            // must answer nonzero
    std::function<bool(const Ints&)> legal_together;          // optional: a combination rule (kernel size with stride)
};

static const char* g_name = "";
static Ints g_args;
static void on_death() {
    fprintf(stderr, "size_sweep: the sanitizer report above came from %s(", g_name);
    for (size_t i = 0; i < g_args.size(); ++i) fprintf(stderr, "%s%d", i ? ", " : "", g_args[i]);
    fprintf(stderr, ")\n");
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static u128 P(int a) { return (u128)(a > 0 ? a : 0); }

static int sweep(const Function& f) {
    long long calls = 0, nonzero = 0, failures = 0;
    g_name = f.name;
    auto one = [&](const Ints& v) {
        g_args = v;
        bool must_be_zero = false;
        for (size_t i = 0; i < v.size(); ++i) {
            const Arg& a = f.args[i];
            if (!a.any_sign && v[i] <= 0) must_be_zero = true;
            if (!a.legal.empty()) {
                bool in = false;
                for (int x : a.legal) in = in || x == v[i];
                if (!in) must_be_zero = true;
            }
        }
        if (f.legal_together && !f.legal_together(v)) must_be_zero = true;
        const size_t got = f.call(v);
        ++calls;
        nonzero += got != 0;
        const char* what = nullptr;
        if (must_be_zero && got != 0) what = "an illegal argument, yet a nonzero answer";
        else if (got != 0 && (u128)got < f.floor(v)) what = "a nonzero answer below the floor (a wrapped product)";
        if (what && failures++ < 5) {
            printf("FAIL %s(", f.name);
            for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
            printf(") = %zu: %s\n", got, what);
        }
    };
    double product = 1;
    for (const Arg& a : f.args) product *= (double)a.values.size();
    Ints v(f.args.size());
    if (product <= 2.5e6) {                  // the whole product
        std::vector<size_t> at(f.args.size(), 0);
        for (;;) {
            for (size_t i = 0; i < v.size(); ++i) v[i] = f.args[i].values[at[i]];
            one(v);
            size_t i = 0;
            while (i < at.size() && ++at[i] == f.args[i].values.size()) at[i++] = 0;
            if (i == at.size()) break;
        }
    } else {                                 // the corners {1, INT_MAX}^n, then a fixed random sample of the product
        for (unsigned m = 0; m < (1u << v.size()); ++m) {
            for (size_t i = 0; i < v.size(); ++i) {
                const Arg& a = f.args[i];
                v[i] = a.legal.empty() ? ((m >> i & 1) ? INT_MAX : 1) : a.legal[(m >> i & 1) ? a.legal.size() - 1 : 0];
            }
            one(v);
        }
        for (int s = 0; s < 1500000; ++s) {
            for (size_t i = 0; i < v.size(); ++i) v[i] = f.args[i].values[rnd() % f.args[i].values.size()];
            one(v);
        }
    }
    g_args = f.ordinary;
    if (f.call(f.ordinary) == 0) {
        printf("FAIL %s: an ordinary call answers 0\n", f.name);
        ++failures;
    }
    printf("%-48s %9lld calls, %8lld nonzero, %lld failures\n", f.name, calls, nonzero, failures);
    return failures != 0;
}

// ---- kbn_augment_workspace_bytes: records built on the host (no pointer in them is ever followed)
static kbn_augment_tensor record(int channels, int role) {
    kbn_augment_tensor t;
    memset(&t, 0, sizeof t);
    t.channels = channels;
    t.role = role;
    return t;
}
static const std::vector<std::vector<kbn_augment_tensor>> RECORDS = {
    {record(3, KBN_AUGMENT_ROLE_IMAGE), record(1, KBN_AUGMENT_ROLE_RANGE)},
    {record(1, KBN_AUGMENT_ROLE_RANGE), record(2, KBN_AUGMENT_ROLE_RANGE), record(1, KBN_AUGMENT_ROLE_VALIDITY)},
    {record(INT_MAX, KBN_AUGMENT_ROLE_RANGE), record(INT_MAX, KBN_AUGMENT_ROLE_RANGE), record(65536, KBN_AUGMENT_ROLE_RANGE)},
};

static std::vector<Function> functions() {
    const Ints FRAME_C = {1, 3, 4}, FRAME_BITS = {8, 16};
    auto weights = [](int oc, int cin, int ks) { return P(oc) * P(cin) * P(ks) * P(ks) * 2; };
    auto frame = [](const Ints& v) { return P(v[0]) * P(v[1]) * P(v[2]) * P(v[3]) / 8; };
    auto bw_case = [](int ks, int stride) { return (ks == 3 && stride == 1) || (ks == 1 && (stride == 1 || stride == 2)); };
    std::vector<Function> fs;
    fs.push_back({"kbn_conv2d_packed_weight_bytes", {dim("out_channels"), dim("in_channels"), one_of("kernel_size", {1, 3}, 2), one_of("stride", {1, 2}, 3)},
                  [](const Ints& v) { return kbn_conv2d_packed_weight_bytes(v[0], v[1], v[2], v[3]); },
                  [=](const Ints& v) { return weights(v[0], v[1], v[2]); }, {64, 48, 3, 1}, nullptr});
    fs.push_back({"kbn_upconv2x_packed_weight_bytes", {dim("out_channels"), dim("in_channels")},
                  [](const Ints& v) { return kbn_upconv2x_packed_weight_bytes(v[0], v[1]); },
                  [=](const Ints& v) { return weights(v[0], v[1], 3); }, {64, 48}, nullptr});
    fs.push_back({"kbn_conv3x3_split_packed_weight_bytes", {dim("out_channels"), dim("in_channels"), one_of("mode", {0, 1, 2, 3, 4}, 5)},
                  [](const Ints& v) { return kbn_conv3x3_split_packed_weight_bytes(v[0], v[1], v[2]); },
                  [=](const Ints& v) { return weights(v[0], v[1], 3); }, {96, 48, 0}, nullptr});
    fs.push_back({"kbn_conv1x1s2_split_packed_weight_bytes", {dim("out_channels"), dim("tensor_channels"), flag("has_xyz", {0, 1})},
                  [](const Ints& v) { return kbn_conv1x1s2_split_packed_weight_bytes(v[0], v[1], v[2]); },
                  [=](const Ints& v) { return weights(v[0], v[1], 1) + (v[2] ? P(v[0]) * 3 * 4 : 0); }, {96, 48, 1}, nullptr});
    fs.push_back({"kbn_kb1_front_packed_weight_bytes", {dim_of("image_channels", {1, 2, 3, 4}), dim_of("conv0_filters", {48}), dim_of("kb_filters", {48})},
                  [](const Ints& v) { return kbn_kb1_front_packed_weight_bytes(v[0], v[1], v[2]); },
                  [=](const Ints& v) { return weights(v[1], v[0], 3) + weights(v[2], v[1], 1); }, {3, 48, 48}, nullptr});
    fs.push_back({"kbn_kb1_front_next_packed_weight_bytes", {dim_of("image_channels", {48}), dim_of("fused_channels", {48}), dim_of("filters", {96})},
                  [](const Ints& v) { return kbn_kb1_front_next_packed_weight_bytes(v[0], v[1], v[2]); },
                  [=](const Ints& v) { return (P(v[0]) + P(v[1])) * P(v[2]) * 2; }, {48, 48, 96}, nullptr});
    fs.push_back({"kbn_kb1_depth_front_packed_weight_bytes", {dim_of("depth_channels", {1, 2, 3, 4, 5, 6, 7, 8}), dim_of("conv0_filters", {16}), dim_of("kb_filters", {16})},
                  [](const Ints& v) { return kbn_kb1_depth_front_packed_weight_bytes(v[0], v[1], v[2]); },
                  [=](const Ints& v) { return weights(v[1], v[0], 3) + weights(v[2], v[1], 1); }, {2, 16, 16}, nullptr});
    fs.push_back({"kbn_s2d_depth_front_packed_weight_bytes", {dim_of("n_pools", {1, 2, 3, 4, 5, 6, 7, 8})},
                  [](const Ints& v) { return kbn_s2d_depth_front_packed_weight_bytes(v[0]); }, [](const Ints&) { return (u128)1; }, {2}, nullptr});
    fs.push_back({"kbn_conv_tail_packed_weight_bytes", {dim_of("channels", {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16})},
                  [](const Ints& v) { return kbn_conv_tail_packed_weight_bytes(v[0]); },
                  [=](const Ints& v) { return weights(v[0], v[0], 3); }, {16}, nullptr});
    fs.push_back({"kbn_conv2d_s2_affine_packed_weight_bytes", {dim("out_channels"), dim("in_channels"), one_of("kernel_size", {3, 5, 7}, 4)},
                  [](const Ints& v) { return kbn_conv2d_s2_affine_packed_weight_bytes(v[0], v[1], v[2]); },
                  [=](const Ints& v) { return weights(v[0], v[1], v[2]); }, {64, 3, 7}, nullptr});
    fs.push_back({"kbn_conv2d_s2_backward_data_packed_weight_bytes", {dim("out_channels"), dim("in_channels"), one_of("kernel_size", {3, 5, 7}, 4)},
                  [](const Ints& v) { return kbn_conv2d_s2_backward_data_packed_weight_bytes(v[0], v[1], v[2]); },
                  [=](const Ints& v) { return weights(v[0], v[1], v[2]); }, {64, 16, 3}, nullptr});
    fs.push_back({"kbn_conv2d_affine_packed_weight_bytes", {dim("out_channels"), dim("in_channels"), one_of("kernel_size", {1, 3, 7}, 5)},
                  [](const Ints& v) { return kbn_conv2d_affine_packed_weight_bytes(v[0], v[1], v[2]); },
                  [=](const Ints& v) { return weights(v[0], v[1], v[2]); }, {64, 64, 3}, nullptr});
    fs.push_back({"kbn_conv2d_backward_data_packed_weight_bytes", {dim("out_channels"), dim("in_channels"), one_of("kernel_size", {1, 3}, 5), one_of("stride", {1, 2}, 3)},
                  [](const Ints& v) { return kbn_conv2d_backward_data_packed_weight_bytes(v[0], v[1], v[2], v[3]); },
                  [=](const Ints& v) { return weights(v[0], v[1], v[2]); }, {64, 64, 3, 1}, [=](const Ints& v) { return bw_case(v[2], v[3]); }});
    // the scratch of a split weight gradient: `splits` planes (at least two, or the answer is 0: no scratch) of one fp32 weight gradient
    fs.push_back({"kbn_conv2d_s2_backward_weight_scratch_bytes",
                  {dim("n"), dim("out_channels"), dim("in_channels"), one_of("kernel_size", {3, 5, 7}, 4), dim("in_height"), dim("in_width"), flag("splits", WIDE)},
                  [](const Ints& v) { return kbn_conv2d_s2_backward_weight_scratch_bytes(v[0], v[1], v[2], v[3], v[4], v[5], v[6]); },
                  [=](const Ints& v) { return 2 * 2 * weights(v[1], v[2], v[3]); }, {8, 64, 16, 3, 96, 320, 4}, nullptr});
    fs.push_back({"kbn_conv2d_backward_weight_scratch_bytes",
                  {dim("n"), dim("out_channels"), dim("in_channels"), one_of("kernel_size", {1, 3}, 5), one_of("stride", {1, 2}, 3), dim("in_height"), dim("in_width"), flag("splits", WIDE)},
                  [](const Ints& v) { return kbn_conv2d_backward_weight_scratch_bytes(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]); },
                  [=](const Ints& v) { return 2 * 2 * weights(v[1], v[2], v[3]); }, {8, 64, 16, 3, 1, 96, 320, 4}, [=](const Ints& v) { return bw_case(v[3], v[4]); }});
    // which: an index into RECORDS; count: -1, 0 or the records' number (-2 stands for it)
    fs.push_back({"kbn_augment_workspace_bytes", {flag("records", {0, 1, 2}), flag("count", {-1, 0, -2}), dim("n"), dim("height"), dim("width")},
                  [](const Ints& v) { return kbn_augment_workspace_bytes(RECORDS[v[0]].data(), v[1] == -2 ? (int)RECORDS[v[0]].size() : v[1], v[2], v[3], v[4]); },
                  [](const Ints& v) {
                      u128 need = 0;
                      for (const kbn_augment_tensor& t : RECORDS[v[0]])
                          if (t.role == KBN_AUGMENT_ROLE_RANGE) need += P(v[2]) * (KBN_AUGMENT_WORKSPACE_RECORD_BYTES + 8 * P(t.channels) * P(v[3]) * P(v[4]));
                      return need;
                  }, {0, -2, 8, 96, 320}, [](const Ints& v) { return v[1] == -2; }});
    fs.push_back({"kbn_png_encode_gray16_bound", {dim("width"), dim("height")}, [](const Ints& v) { return kbn_png_encode_gray16_bound(v[0], v[1]); },
                  [](const Ints& v) { return P(v[0]) * P(v[1]) * 2; }, {320, 96}, nullptr});
    fs.push_back({"kbn_png_encode_rgb8_bound", {dim("width"), dim("height")}, [](const Ints& v) { return kbn_png_encode_rgb8_bound(v[0], v[1]); },
                  [](const Ints& v) { return P(v[0]) * P(v[1]) * 3; }, {320, 96}, nullptr});
    fs.push_back({"kbn_png_encode_gray8_bound", {dim("width"), dim("height")}, [](const Ints& v) { return kbn_png_encode_gray8_bound(v[0], v[1]); },
                  [](const Ints& v) { return P(v[0]) * P(v[1]); }, {320, 96}, nullptr});
    fs.push_back({"kbn_frame_encode_bound", {dim("width"), dim("height"), one_of("channels", FRAME_C, 2), one_of("bits", FRAME_BITS, 12)},
                  [](const Ints& v) { return kbn_frame_encode_bound(v[0], v[1], v[2], v[3]); }, frame, {320, 96, 3, 8}, nullptr});
    fs.push_back({"kbn_pack_frames_stride", {dim("width"), dim("height"), one_of("channels", FRAME_C, 2), one_of("bits", FRAME_BITS, 12)},
                  [](const Ints& v) { return kbn_pack_frames_stride(v[0], v[1], v[2], v[3]); }, frame, {320, 96, 3, 8}, nullptr});
    // the workspace: a length of four bytes a (frame, group, plane) and a header byte a segment
    fs.push_back({"kbn_pack_frames_workspace_bytes", {dim("n"), dim("width"), dim("height"), one_of("channels", FRAME_C, 2), one_of("bits", FRAME_BITS, 12)},
                  [](const Ints& v) { return kbn_pack_frames_workspace_bytes(v[0], v[1], v[2], v[3], v[4]); },
                  [](const Ints& v) { return P(v[0]) * P(v[3]) * ((P(v[2]) + 7) / 8 * 4 + P(v[2]) * ((P(v[1]) + 15) / 16)); }, {8, 320, 96, 3, 8}, nullptr});
    return fs;
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    __sanitizer_set_death_callback(on_death);
    const std::vector<Function> fs = functions();
    if (argc == 2 && strcmp(argv[1], "--list") == 0) {
        for (const Function& f : fs) printf("%s\n", f.name);
        return 0;
    }
    int failed = 0, ran = 0;
    for (const Function& f : fs) {
        bool wanted = argc == 1;
        for (int i = 1; i < argc; ++i) wanted = wanted || strcmp(argv[i], f.name) == 0;
        if (!wanted) continue;
        failed += sweep(f);
        ++ran;
    }
    if (ran == 0) { printf("no such function\n"); return 2; }
    printf("size_sweep: %d functions, %d failed\n", ran, failed);
    return failed ? 1 : 0;
}
