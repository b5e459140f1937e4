// Host-only check, built with -fsanitize=address,undefined by tests/test_multi_sprt_cpu.py: the per-round
// SPRT update of multi-problem runs (ransac_amd/csrc/usac_host.hpp: SprtRounds, sprt_rounds_update -- the text
// usac_multi_run_sprt and usac_multi_sprt_update apply) over a scripted sequence of rounds, with the
// history in heap buffers of exactly the capacity given, and the consumer's host-only part
// (consumer_host.hpp).  No GPU, no HIP, no library.
//   sprt_update_check <scratch file>   prints "ok <updates> <tests designed>" or a message and exits 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "consumer_host.hpp"
#include "usac_host.hpp"

static int fail(const char *what, int est, unsigned step) {
    std::printf("FAILED %s (estimator %d, step %u)\n", what, est, step);
    return 1;
}

struct Round {
    uint32_t head_inliers, head_points;
    bool improved;
    uint32_t best_inliers, term_bound;
};

static bool same(const usac::Sprt::History &a, const usac::Sprt::History &b) {
    return !std::memcmp(&a.epsilon, &b.epsilon, sizeof(double)) && !std::memcmp(&a.delta, &b.delta, sizeof(double)) &&
           !std::memcmp(&a.A, &b.A, sizeof(double)) && a.k == b.k;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const uint32_t n = 1000, R = 64, max_iters = 4096;
    // delta only, neither, epsilon only, both, no head points, the guard twice (epsilon^ = 1, delta^ >= epsilon'),
    // a tiny epsilon^ (the denominator exit), a large one after a long history (a bound of 0), counts at the
    // integer limits
    const Round script[] = {{300, 10000, false, 0, 0},  {300, 10000, false, 0, 0},     {0, 0, true, 300, 900},
                            {900, 10000, true, 350, 800}, {0, 0, false, 0, 0},         {0, 0, true, 1000, 1},
                            {9000, 10000, false, 0, 0}, {1049, 100000, true, 20, 4000}, {5, 100000, true, 900, 4096},
                            {0xFFFFFFFFu, 0xFFFFFFFFu, true, 950, 0xFFFFFFFFu}, {1, 0xFFFFFFFFu, false, 0, 0}};
    const unsigned steps = sizeof(script) / sizeof(script[0]);
    unsigned updates = 0, designed = 0;
    for (int est = 2; est <= 3; est++) {
        const uint32_t m = est == 2 ? 4 : 7;
        for (uint32_t cap = 1; cap <= steps + 1; cap += steps) {  // a capacity of one test, and of all
            std::vector<usac::Sprt::History> hist(cap);
            uint32_t nh = 0, last = 0, bound = 0;
            usac::SprtRounds obj(est, n, m, max_iters);
            if (usac::sprt_rounds_update(est, n, m, max_iters, hist.data(), &nh, cap, &last, &bound, 0, 0, 0, false, 0, 0))
                return fail("initialisation refused", est, 0);
            if (nh != 1 || last != 0 || bound != max_iters || !same(hist[0], obj.test()) || hist[0].k != 0)
                return fail("initial state", est, 0);
            for (unsigned s = 0; s < steps; s++) {
                const Round &r = script[s];
                const uint32_t done = (s + 1) * R, before = nh;
                const int rc = usac::sprt_rounds_update(est, n, m, max_iters, hist.data(), &nh, cap, &last, &bound, done,
                                                        r.head_inliers, r.head_points, r.improved, r.best_inliers,
                                                        r.term_bound);
                const bool grew = obj.update(done, r.head_inliers, r.head_points, r.improved, r.best_inliers, r.term_bound);
                updates++;
                if (rc) {  // only a full history is refused, and it leaves the state alone
                    if (!(grew && before == cap && nh == before)) return fail("update refused", est, s);
                    break;
                }
                if (nh != before + (grew ? 1u : 0u)) return fail("history length", est, s);
                designed += grew ? 1 : 0;
                if (!same(hist[nh - 1], obj.test()) || last != obj.last_update() || bound != obj.bound())
                    return fail("the plain state and the object differ", est, s);
                const usac::Sprt::History &t = hist[nh - 1];
                if (!(0 < t.delta && t.delta < t.epsilon && t.epsilon < 1) || !(t.A >= 1)) return fail("the guard", est, s);
                if (bound > max_iters && !(r.improved && bound == r.term_bound)) return fail("bound", est, s);
                long long ksum = 0;
                for (uint32_t i = 0; i < nh; i++) ksum += hist[i].k;
                if (ksum != (long long)last || last > done) return fail("k values", est, s);
            }
        }
        // argument errors leave everything alone
        usac::Sprt::History one[1];
        uint32_t nh = 2, last = 7, bound = 9;
        if (!usac::sprt_rounds_update(est, n, m, max_iters, one, &nh, 1, &last, &bound, 64, 0, 0, false, 0, 0) ||
            !usac::sprt_rounds_update(est, n, m, max_iters, nullptr, &nh, 1, &last, &bound, 64, 0, 0, false, 0, 0) ||
            !usac::sprt_rounds_update(4, n, m, max_iters, one, &nh, 4, &last, &bound, 64, 0, 0, false, 0, 0) || nh != 2 ||
            last != 7 || bound != 9)
            return fail("argument errors", est, 0);
    }
    // the consumer's host-only part: a file round trip and one problem's JSON
    std::vector<float> w(37);
    for (size_t i = 0; i < w.size(); i++) w[i] = 0.5f * (float)i;
    FILE *f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(w.data(), sizeof(float), w.size(), f) != w.size()) return fail("scratch file", 0, 0);
    std::fclose(f);
    if (consumer_host::read_file<float>(argv[1], w.size()) != w) return fail("read_file", 0, 0);
    usac_multi_output o = usac_multi_output();
    o.best.hyp_index = ~0ull;
    o.best.inliers = -2147483647;
    for (int k = 0; k < 9; k++) o.best.model[k] = -3.4e38f;
    o.rounds = o.hypotheses = o.bound = 0xFFFFFFFFu;
    usac_multi_sprt_output sp = {-1.7e308, -1.7e308, -1.7e308, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, ~0ull};
    usac_multi_prosac_output q = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    const std::string js = consumer_host::problem_json(o, sp, &q);
    if (js.empty() || js[0] != '{' || js[js.size() - 1] != '}' || consumer_host::bits(1.0f) != 0x3F800000)
        return fail("problem_json", 0, 0);
    std::printf("ok %u %u\n", updates, designed);
    return 0;
}
