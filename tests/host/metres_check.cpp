// metres_check.cpp -- csrc/sfm_metres.h, the one check of a per-scene length in metres (sense_range, max_range, the radii of
// episodes and scans), without a GPU and without the HIP runtime.  Built and run by tests/test_metres_host.py; exits non-zero on
// the first failed check.
#include "sfm_metres.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

using sfm::check_metres;

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

// accepted: no message, and the square is the double product rounded once
static void accepted(float r, bool strict) {
    float sq = -1.f;
    CHECK(check_metres(3, "sense_range", r, strict, &sq).empty());
    CHECK(same_bits(sq, (float)((double)r * (double)r)));
}

// refused: the library's message, character for character, and *sq untouched
static void refused(float r, bool strict) {
    float sq = -1.f;
    const std::string why = check_metres(3, "veh_radius", r, strict, &sq);
    CHECK(why == (strict ? "scene 3: veh_radius must be finite, > 0 and <= 1e6 metres" : "scene 3: veh_radius must be finite, >= 0 and <= 1e6 metres"));
    CHECK(sq == -1.f);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float denorm = std::numeric_limits<float>::denorm_min(), over = std::nextafterf(1e6f, inf);
    CHECK(SFM_BATCH_MAX_SENSE_RANGE == 1e6f && over > 1e6f);
    for (int strict = 0; strict < 2; ++strict) {
        for (float r : {denorm, 1.0f, 1e6f, 0.3f, std::nextafterf(1e6f, 0.f)}) accepted(r, strict != 0);
        for (float r : {over, inf, -inf, -1.0f, -denorm, nan, -nan}) refused(r, strict != 0);
    }
    accepted(0.0f, false);   refused(0.0f, true);            // 0 switches a radius off; a range of 0 sees nothing
    accepted(-0.0f, false);  refused(-0.0f, true);           // -0 is 0
    float sq = -1.f;
    CHECK(check_metres(0, "r", -0.0f, false, &sq).empty() && same_bits(sq, 0.0f));       // ... and its square is +0
    CHECK(check_metres(0, "r", denorm, false, &sq).empty() && same_bits(sq, 0.0f));      // (2^-298 rounds to 0)
    CHECK(check_metres(12, "max_range", 0.0f, true, &sq) == "scene 12: max_range must be finite, > 0 and <= 1e6 metres");

    // Many lengths over (0, 1e6]: every square is the double product rounded once.  Beside it the loop counts the values whose
    // square formed in float differs.  Under IEEE 754 there is none: the product of two 24-bit significands is exact in double, so
    // both ways round the exact product once, to the same float -- "formed in double" says how the library writes it, and no float
    // argument can tell the two apart.  So the count is asserted to be 0 (a host whose float arithmetic is not IEEE single --
    // x87 excess precision, flush-to-zero -- would show here).
    long tried = 0, differ = 0;
    uint32_t lcg = 12345u;
    for (int i = 0; i < 400000; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        uint32_t bits = lcg >> 1;                            // a positive float
        float r;
        memcpy(&r, &bits, sizeof(r));
        if (!(r > 0.f) || r > 1e6f) continue;
        ++tried;
        accepted(r, true);
        volatile float f = r * r;                            // squared in float
        if (!same_bits(f, (float)((double)r * (double)r))) ++differ;
    }
    CHECK(tried > 100000 && differ == 0);
    CHECK(check_metres(0, "r", 1.0f, true, nullptr).empty() && !check_metres(0, "r", 0.0f, true, nullptr).empty());   // the check alone
    printf("metres_check ok (%ld lengths, %ld squares differ when formed in float)\n", tried, differ);
    return 0;
}
