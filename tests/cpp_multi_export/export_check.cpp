// Host-only check, built with g++ and -fsanitize=address,undefined by tests/test_multi_export_cpu.py: the
// host-and-device functions of ransac_amd/csrc/usac_pixels.hpp (the text k_multi_export runs on the device and
// usac_multi_pixel_models on the host) against a long-double restatement on random intrinsics and essential
// matrices, and the extent rule of usac_multi_export_device (usac_pack.hpp) at its edges.  No GPU, no HIP, no
// library.
//   export_check <cases>   prints "ok <cases>" or a message and exits 1
//
// The bounds come from the formats.  A pixel-model entry is ((b0 g0 + b1 g1) + b2 g2) with g = ((e0 a0 + e1 a1)
// + e2 a2) in fp64 over entries of the closed-form inverses (at most five roundings each), then one cast to
// fp32: every path from an input to the entry passes fewer than 32 fp64 roundings, each relative to a partial
// result no larger than S = sum |b| |e| |a| over the entry's 27 products, and the cast adds half an fp32 ulp of
// the entry.  So |f - f_exact| <= 2^-24 |f_exact| + 32 * 2^-53 * S, with the 64-bit-mantissa long double standing
// for exact.  The threshold is five fp32 roundings (three sums, a quotient, a square; * 0.25 is exact): a relative
// 6 * 2^-24 covers them with their second-order terms.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "usac_pack.hpp"
#include "usac_pixels.hpp"

typedef long double ld;

static int fail(const char *what, unsigned item) {
    std::printf("FAILED %s (item %u)\n", what, item);
    return 1;
}

// xorshift64*: the cases are the same on every machine
static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uniform(double lo, double hi) {
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    const uint64_t r = g_state * 0x2545f4914f6cdd1dull;
    return lo + (hi - lo) * (double)(r >> 11) * (1.0 / 9007199254740992.0);
}

static void random_k(float *k) {
    const float v[9] = {(float)uniform(300, 3000), (float)uniform(-3, 3), (float)uniform(100, 2000), 0.f,
                        (float)uniform(300, 3000), (float)uniform(100, 2000), 0.f, 0.f, 1.f};
    for (int i = 0; i < 9; i++) k[i] = v[i];
}

static void inverse_ld(const float *k, ld *inv) {
    const ld fx = k[0], s = k[1], cx = k[2], fy = k[4], cy = k[5];
    const ld v[9] = {1 / fx, -s / (fx * fy), (s * cy - cx * fy) / (fx * fy), 0, 1 / fy, -cy / fy, 0, 0, 1};
    for (int i = 0; i < 9; i++) inv[i] = v[i];
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const unsigned cases = (unsigned)std::atoi(argv[1]);
    const ld e24 = std::ldexp((ld)1, -24), e53 = std::ldexp((ld)1, -53);
    for (unsigned c = 0; c < cases; c++) {
        std::vector<float> k1(9), k2(9), e(9), f(9), packed(usac::kCalibFloats);
        random_k(k1.data());
        random_k(k2.data());
        for (int i = 0; i < 9; i++) e[i] = (float)uniform(-2, 2);
        if (!usac::pixel_k_ok(k1.data()) || !usac::pixel_k_ok(k2.data())) return fail("a good K refused", c);
        std::vector<double> a(9), b(9);
        usac::pixel_k_inverse(k1.data(), a.data());
        usac::pixel_k_inverse(k2.data(), b.data());
        ld al[9], bl[9];
        inverse_ld(k1.data(), al);
        inverse_ld(k2.data(), bl);
        for (int i = 0; i < 9; i++) {  // at most five fp64 roundings per entry, cancellation in entry 2 included
            const ld scale = i == 2 ? (std::fabs((ld)k1[1] * k1[5]) + std::fabs((ld)k1[2] * k1[4])) / ((ld)k1[0] * k1[4])
                                    : std::fabs(al[i]);
            if (std::fabs((ld)a[i] - al[i]) > 6 * e53 * scale) return fail("inverse of K", c);
        }
        usac::pixel_model(k1.data(), k2.data(), e.data(), f.data());
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                ld exact = 0, S = 0;
                for (int r = 0; r < 3; r++)
                    for (int q = 0; q < 3; q++) {
                        const ld term = bl[3 * r + i] * (ld)e[3 * r + q] * al[3 * q + j];
                        exact += term;
                        S += std::fabs(term);
                    }
                if (std::fabs((ld)f[3 * i + j] - exact) > e24 * std::fabs(exact) + 32 * e53 * S)
                    return fail("pixel model", c);
            }
        std::vector<float> inplace(e);  // E and F the same array
        usac::pixel_model(k1.data(), k2.data(), inplace.data(), inplace.data());
        for (int i = 0; i < 9; i++)
            if (inplace[i] != f[i]) return fail("pixel model in place", c);
        const float t = (float)uniform(0.5, 60);
        const float thr = usac::pixel_threshold(k1.data(), k2.data(), t);
        const ld fm = ((ld)k1[0] + k1[4] + k2[0] + k2[4]) / 4, want = (t / fm) * (t / fm);
        if (std::fabs((ld)thr - want) > 6 * e24 * want) return fail("threshold", c);
        usac::pixel_pack(k1.data(), k2.data(), packed.data());
        const float lay[12] = {k1[0], k1[1], k1[2], k1[4], k1[5], k2[0], k2[1], k2[2], k2[4], k2[5], 0.f, 0.f};
        for (int i = 0; i < 12; i++)
            if (packed[i] != lay[i]) return fail("packed intrinsics", c);
        std::vector<float> bad(k1);
        const int which = (int)(c % 6);
        bad[which == 0 ? 0 : which == 1 ? 4 : which == 2 ? 3 : which == 3 ? 6 : which == 4 ? 7 : 8] =
            which < 2 ? -1.f : which == 5 ? 2.f : 0.5f;
        if (usac::pixel_k_ok(bad.data())) return fail("a bad K accepted", c);
    }
    // the extent rule: P x n_max and P x k_max below 2^32, n_max > 0, k_max 0 = no list
    struct { uint32_t P, n_max, k_max; bool ok; } ex[] = {
        {65535u, 65537u, 0u, true},        // 2^32 - 1 cells
        {65535u, 65538u, 0u, false},       // the first width past 2^32 at the largest P
        {1u, 0xffffffffu, 0u, true},       {2u, 0x80000000u, 0u, false},  // exactly 2^32
        {2u, 0x7fffffffu, 0u, true},       {6u, 0u, 0u, false},
        {0u, 300u, 0u, false},             {6u, 300u, 300u, true},
        {65535u, 300u, 65537u, true},      {65535u, 300u, 65538u, false},
        {2u, 300u, 0x80000000u, false},    {1u, 1u, 0xffffffffu, true},
        {65535u, 65538u, 1u, false},
    };
    unsigned n = 0;
    for (const auto &q : ex) {
        if (usac::export_extent_ok(q.P, q.n_max, q.k_max) != q.ok) return fail("extent rule", n);
        n++;
    }
    std::printf("ok %u\n", cases);
    return 0;
}
