// Rate of the grinding search kernel (csrc/stark_grind.cuh), stand-alone: the specialised candidate permutation against the
// same loop over the unmodified keccak_f1600 (LW_GRIND_PLAIN_VARIANT, defined in this build only).  One launch covers one
// window of the size the library uses for the given grinding factor; the validity limit is set so that no candidate
// passes (shift for factor 63), so every work-item runs its whole share.  Per variant and window: one warm-up launch,
// then 9 timed launches (HIP events); prints median, min, max and candidates per second of the median.
// usage: stark_grind_bench [factor ...]      (default 20 24 28)
#define LW_GRIND_PLAIN_VARIANT 1
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../lambda_elliptic_curves_amd/csrc/stark_grind.cuh"

#define CHECK(e)                                                                         \
    do {                                                                                 \
        hipError_t _e = (e);                                                             \
        if (_e != hipSuccess) {                                                          \
            fprintf(stderr, "%s: %s (line %d)\n", #e, hipGetErrorString(_e), __LINE__);  \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

template <int PLAIN>
static int run(const lw::GrindArgs &g, unsigned long long *d_best, uint32_t factor, const char *name) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const uint32_t blocks = std::min<uint32_t>((g.count + 255) / 256, lw::GRIND_MAX_BLOCKS);
    std::vector<float> ms;
    for (int rep = 0; rep < 10; rep++) {
        CHECK(hipMemset(d_best, 0xff, 8));
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((lw::grind_kernel<PLAIN>), dim3(blocks), dim3(256), 0, 0, g, d_best);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        float t;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep) ms.push_back(t);
    }
    unsigned long long best;
    CHECK(hipMemcpy(&best, d_best, 8, hipMemcpyDeviceToHost));
    std::sort(ms.begin(), ms.end());
    printf("%-11s factor %2u window 2^%-2d  median %8.4f ms  [min %8.4f .. max %8.4f]  %7.3f G candidates/s%s\n", name, factor,
           31 - __builtin_clz(g.count), ms[4], ms.front(), ms.back(), g.count / (ms[4] * 1e6), best == ~0ull ? "" : "  (a candidate passed)");
    return 0;
}

int main(int argc, char **argv) {
    std::vector<uint32_t> factors;
    for (int i = 1; i < argc; i++) factors.push_back((uint32_t)atoi(argv[i]));
    if (factors.empty()) factors = {20, 24, 28};
    uint8_t inner[32];
    for (int i = 0; i < 32; i++) inner[i] = (uint8_t)(37 * i + 11);   // any 32 bytes: the rate does not depend on them
    unsigned long long *d_best;
    CHECK(hipMalloc(&d_best, 8));
    for (uint32_t f : factors) {
        if (f < 1 || f > 63) continue;
        lw::GrindArgs g;
        lw::grind_prepare(inner, g);
        g.start = 0;
        g.count = (uint32_t)lw::grind_window(f);
        g.shift = 1;
        if (run<0>(g, d_best, f, "specialised")) return 1;
        if (run<1>(g, d_best, f, "plain")) return 1;
    }
    CHECK(hipFree(d_best));
    return 0;
}
