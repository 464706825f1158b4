// point_cloud_size_sweep -- kbn_point_cloud_workspace_bytes over extreme arguments, in a build with AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_point_cloud_sanitizers_cpu.py builds it from this file and csrc/point_cloud.hip and runs
// it).  size_sweep.cpp's rules, for the one size function that program's driver does not link:
//   - no sanitizer report (the build aborts at the first);
//   - 0 whenever n, height or width is <= 0;
//   - a nonzero answer is never below the floor computed here in unsigned __int128: four bytes a (frame, tile of 1024 pixels);
//   - an ordinary call answers nonzero, so that "always 0" does not pass;
// and the entry point refuses, before any launch, the sizes the size function answers 0 for (its pointers are never followed).
// Nothing here takes a pointer to GPU memory or launches anything.
#include <limits.h>
#include <stdio.h>

#include "../../include/kbnet_hip.h"

typedef unsigned __int128 u128;

static const int WIDE[] = {INT_MIN, -1, 0, 1, 3, 16, 48, 384, 512, 1216, 4096, 65535, 65536, 1 << 20, 1 << 24, INT_MAX / 2, INT_MAX - 1, INT_MAX};

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    long long calls = 0, nonzero = 0, failures = 0;
    static double memory[64];      // aligned host memory to stand for the pointers: a refusal comes before any of it is read
    for (int n : WIDE)
        for (int h : WIDE)
            for (int w : WIDE) {
                const size_t got = kbn_point_cloud_workspace_bytes(n, h, w);
                ++calls;
                nonzero += got != 0;
                const char* what = nullptr;
                if ((n <= 0 || h <= 0 || w <= 0) && got != 0) what = "an illegal argument, yet a nonzero answer";
                else if (got != 0 && (u128)got < (u128)n * (((u128)h * (u128)w + 1023) / 1024) * 4) what = "a nonzero answer below the floor (a wrapped product)";
                else if (got == 0) {
                    const int status = kbn_point_cloud_forward((const float*)memory, 1, nullptr, 255.f, 0.f, (const float*)memory, 0.f, 1.f, n, h, w,
                                                               (unsigned char*)memory, (size_t)-1, (long long*)memory, memory, (size_t)-1, nullptr);
                    if (status != KBN_ERR_INVALID_ARGUMENT && status != KBN_ERR_UNSUPPORTED) what = "no workspace size, yet the entry point does not refuse";
                }
                if (what && failures++ < 5) printf("FAIL kbn_point_cloud_workspace_bytes(%d, %d, %d) = %zu: %s\n", n, h, w, got, what);
            }
    if (kbn_point_cloud_workspace_bytes(8, 352, 1216) != 8 * 418 * 4) {
        printf("FAIL kbn_point_cloud_workspace_bytes: an ordinary call does not answer 4 bytes a tile\n");
        ++failures;
    }
    printf("%-48s %9lld calls, %8lld nonzero, %lld failures\n", "kbn_point_cloud_workspace_bytes", calls, nonzero, failures);
    return failures != 0;
}
