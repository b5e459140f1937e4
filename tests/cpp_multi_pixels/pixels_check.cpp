// Host-only check, built with -fsanitize=address,undefined by tests/test_multi_pixels_cpu.py: the host part of
// the pixel entries of a multi context (ransac_amd/csrc/usac_pixels.hpp -- the text
// usac_multi_create_essential_pixels, usac_multi_set_pixel_thresholds and usac_multi_pixel_models apply)
// against values the test computed with tests/helpers/multi_pixels_ref.py, every array in a heap buffer of
// exactly its size.  No GPU, no HIP, no library.
//   pixels_check <file> <P> <n_bad>   prints "ok <P> <n_bad>" or a message and exits 1
// file, float32: K1 [P x 9], K2 [P x 9], t [P], thr [P], E [P x 9], F [P x 9], bad K [n_bad x 9]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "usac_pixels.hpp"

static int fail(const char *what, unsigned p) {
    std::printf("FAILED %s (item %u)\n", what, p);
    return 1;
}

static bool same(const float *a, const float *b, size_t n) { return !std::memcmp(a, b, sizeof(float) * n); }

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const unsigned P = (unsigned)std::atoi(argv[2]), n_bad = (unsigned)std::atoi(argv[3]);
    const size_t total = (size_t)P * (9 + 9 + 1 + 1 + 9 + 9) + (size_t)n_bad * 9;
    std::vector<float> all(total);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(all.data(), sizeof(float), total, f) != total) return fail("input file", 0);
    std::fclose(f);
    const float *at = all.data();
    const std::vector<float> K1(at, at + 9 * P), K2(at + 9 * P, at + 18 * P);
    at += 18 * (size_t)P;
    const std::vector<float> t(at, at + P), thr(at + P, at + 2 * P);
    at += 2 * (size_t)P;
    const std::vector<float> E(at, at + 9 * P), F(at + 9 * P, at + 18 * P);
    at += 18 * (size_t)P;
    const std::vector<float> bad(at, at + 9 * n_bad);

    for (unsigned p = 0; p < P; p++) {
        const float *k1 = &K1[9 * p], *k2 = &K2[9 * p];
        if (!usac::pixel_k_ok(k1) || !usac::pixel_k_ok(k2)) return fail("a good K refused", p);
        const float got = usac::pixel_threshold(k1, k2, t[p]);
        if (!same(&got, &thr[p], 1)) return fail("threshold bits", p);
        std::vector<float> out(9);
        usac::pixel_model(k1, k2, &E[9 * p], out.data());
        if (!same(out.data(), &F[9 * p], 9)) return fail("pixel model bits", p);
        std::vector<float> inplace(&E[9 * p], &E[9 * p] + 9);  // E and F the same array
        usac::pixel_model(k1, k2, inplace.data(), inplace.data());
        if (!same(inplace.data(), &F[9 * p], 9)) return fail("pixel model in place", p);
        std::vector<float> packed(usac::kCalibFloats);
        usac::pixel_pack(k1, k2, packed.data());
        const float want[12] = {k1[0], k1[1], k1[2], k1[4], k1[5], k2[0], k2[1], k2[2], k2[4], k2[5], 0.f, 0.f};
        if (!same(packed.data(), want, 12)) return fail("packed intrinsics", p);
    }
    for (unsigned b = 0; b < n_bad; b++) {
        const std::vector<float> k(&bad[9 * b], &bad[9 * b] + 9);
        if (usac::pixel_k_ok(k.data())) return fail("a bad K accepted", b);
    }
    std::printf("ok %u %u\n", P, n_bad);
    return 0;
}
