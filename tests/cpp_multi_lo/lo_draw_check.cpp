// Host-only check, built with -fsanitize=address,undefined by tests/test_gpu_multi_lo_cpp.py: the host text
// of the LO draw (ransac_amd/csrc/usac_lo_draw.hpp) into heap buffers of exactly k ints, and the
// consumer's host-only part (consumer_host.hpp).  No GPU, no HIP, no library.
//   lo_draw_check <scratch file>   prints "ok <sets>" or a message and exits 1
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "consumer_host.hpp"
#include "usac_lo_draw.hpp"

static int fail(const char *what, unsigned k, unsigned top) {
    std::printf("FAILED %s (k = %u, max = %u)\n", what, k, top);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    unsigned sets = 0;
    const unsigned ks[] = {1, 2, 7, 14, 63, 64};
    const unsigned tops[] = {0, 1, 13, 14, 63, 64, 999, 16383, 0x7FFFFFFFu};
    for (unsigned k : ks)
        for (unsigned top : tops) {
            if ((unsigned long long)k > (unsigned long long)top + 1) continue;
            for (uint64_t seed = 0; seed < 3; seed++)
                for (uint64_t draw = 0; draw < 4; draw++) {
                    std::vector<int32_t> a(k), b(k);
                    usac::lo_draw(seed * 0x9E3779B97F4A7C15ull + 5, draw, k, top, a.data());
                    usac::lo_draw(seed * 0x9E3779B97F4A7C15ull + 5, draw, k, top, b.data());
                    if (a != b) return fail("not deterministic", k, top);
                    std::set<int32_t> seen;
                    for (int32_t v : a) {
                        if (v < 0 || (uint32_t)v > top) return fail("out of range", k, top);
                        seen.insert(v);
                    }
                    if (seen.size() != k) return fail("not distinct", k, top);
                    if (k == top + 1 && (*seen.begin() != 0 || *seen.rbegin() != (int32_t)top))
                        return fail("not a permutation", k, top);
                    sets++;
                }
        }
    // the consumer's host-only part: a file round trip and one problem's JSON
    std::vector<float> w(37);
    for (size_t i = 0; i < w.size(); i++) w[i] = 0.5f * (float)i;
    FILE *f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(w.data(), sizeof(float), w.size(), f) != w.size()) return fail("scratch file", 0, 0);
    std::fclose(f);
    if (consumer_host::read_file<float>(argv[1], w.size()) != w) return fail("read_file", 0, 0);
    bool threw = false;
    try {
        consumer_host::read_file<float>(argv[1], w.size() + 1);
    } catch (const std::exception &) {
        threw = true;
    }
    if (!threw) return fail("short read not reported", 0, 0);
    usac_multi_output o = usac_multi_output();
    o.best.hyp_index = ~0ull;
    o.best.inliers = -2147483647;
    for (int k = 0; k < 9; k++) o.best.model[k] = -3.4e38f;
    o.rounds = o.hypotheses = o.bound = 0xFFFFFFFFu;
    usac_multi_lo_output l = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, -1e30f};
    usac_multi_prosac_output q = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const std::string js = consumer_host::problem_json(o, l, &q);
    if (js.empty() || js[0] != '{' || js[js.size() - 1] != '}' || consumer_host::bits(1.0f) != 0x3F800000)
        return fail("problem_json", 0, 0);
    std::printf("ok %u\n", sets);
    return 0;
}
