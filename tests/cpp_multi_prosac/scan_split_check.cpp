// scan_split_check.cpp -- CPU check (tests/test_multi_prosac_scan_split.py) of the device / host split
// of PROSAC's termination scan for multi-problem batches.  The kernel's part
// (kernels_multi_prosac.hip: flags -> running counts -> non_random update -> ordered candidates) is
// restated here on the host and feeds usac::ProsacTerminationCriteria::applyCandidates; bound and
// termination length are compared, call after call, with the plain scan of
// prosac_termination_criteria.hpp:148-201 (every candidate's value computed and applied in place).
// Random call sequences over n in 21..5000 and m in {4, 7}, plus the degenerate flag patterns.
// Prints "ok <calls>" or the first difference.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "usac_host.hpp"

namespace {

constexpr uint32_t kMin = 20;

struct PlainScan {
    usac::StandardTerminationCriteria std_;
    std::vector<uint32_t> growth_, non_random_, maximality_;
    uint32_t n_, term_len_;
    PlainScan(const std::vector<uint32_t> &growth, float p, uint32_t m, uint32_t n, uint32_t max_iters)
        : std_(p, m, n, max_iters), growth_(growth),
          non_random_(usac::ProsacTerminationCriteria::non_random_table(n, m)), maximality_(n, 10000), n_(n),
          term_len_(n) {}
    uint32_t scan(uint32_t hypCount, const std::vector<char> &inl, uint32_t largest) {
        uint32_t max_samples = maximality_[term_len_ - 1];
        uint32_t count = 0;
        for (uint32_t i = 0; i < kMin; i++) count += inl[i] ? 1 : 0;
        bool cur = inl[kMin], nxt = false;
        for (uint32_t i = kMin; i < n_; ++i) {
            if (i != n_ - 1) nxt = inl[i + 1];
            count += cur ? 1 : 0;
            if (non_random_[i] < count) {
                non_random_[i] = count;
                if (i == n_ - 1 || (cur && !nxt)) {
                    uint32_t samples = std_.getUpBoundIterations(count, i + 1);
                    if (i + 1 < largest) samples += hypCount - growth_[i];
                    if (samples < maximality_[i]) {
                        maximality_[i] = samples;
                        if (samples < max_samples || (samples == max_samples && i + 1 >= term_len_)) {
                            term_len_ = i + 1;
                            max_samples = samples;
                        }
                    }
                }
            }
            cur = nxt;
        }
        return max_samples;
    }
};

// The kernel's half: tiles of `tile` points, a carried count, per-point inclusive counts, the
// non_random update for i >= 20 and the (i, count) pairs of the raised points that end a run of
// inliers or are the last point, ascending i.
struct DeviceHalf {
    std::vector<uint32_t> non_random;
    uint32_t n;
    DeviceHalf(uint32_t n_, uint32_t m) : non_random(usac::ProsacTerminationCriteria::table(n_, m)), n(n_) {}
    void scan(const std::vector<char> &inl, uint32_t tile, std::vector<uint32_t> &cand) {
        cand.clear();
        uint32_t carry = 0;
        for (uint32_t t0 = 0; t0 < n; t0 += tile) {
            uint32_t in_tile = 0;
            for (uint32_t i = t0; i < std::min(n, t0 + tile); i++) {
                in_tile += inl[i] ? 1 : 0;
                const uint32_t count = carry + in_tile;
                const bool next = i + 1 < n && inl[i + 1];
                if (i >= kMin && non_random[i] < count) {
                    non_random[i] = count;
                    if (i == n - 1 || (inl[i] && !next)) {
                        cand.push_back(i);
                        cand.push_back(count);
                    }
                }
            }
            carry += in_tile;
        }
    }
};

struct Trial {
    usac::ProsacTerminationCriteria split;
    DeviceHalf dev;
    PlainScan plain;
    std::vector<uint32_t> cand;
    uint32_t n;
    Trial(const std::vector<uint32_t> &growth, float p, uint32_t m, uint32_t n_, uint32_t max_iters)
        : split(usac::ProsacTerminationCriteria::CandidatesOnly{}, growth, p, m, n_, max_iters), dev(n_, m),
          plain(growth, p, m, n_, max_iters), n(n_) {}
    bool call(uint32_t hyp, const std::vector<char> &inl, uint32_t largest, const char *what) {
        const uint32_t a = plain.scan(hyp, inl, largest);
        dev.scan(inl, 256, cand);
        if (cand.size() / 2 > n / 2 + 1) {
            printf("diff %s n %u: %zu candidates past the capacity\n", what, n, cand.size() / 2);
            return false;
        }
        const uint32_t b = split.applyCandidates(hyp, largest, cand.data(), (uint32_t)(cand.size() / 2));
        if (a != b || plain.term_len_ != split.terminationLength() || dev.non_random != plain.non_random_) {
            printf("diff %s n %u hyp %u largest %u: bound %u / %u, term_len %u / %u\n", what, n, hyp, largest, a, b,
                   plain.term_len_, split.terminationLength());
            return false;
        }
        return true;
    }
};

}  // namespace

int main(int argc, char **argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937 g(4242);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long calls = 0;
    // ---- random call sequences
    for (int t = 0; t < trials; t++) {
        const uint32_t sizes[] = {21, 22, 64, 255, 256, 257, 515, 1000};
        const uint32_t n = t < 8 ? sizes[t] : 21 + (uint32_t)(U(g) * 4980);
        const uint32_t m = (t % 2) ? 7u : 4u;
        const uint32_t max_iters = (t % 4 == 0) ? 1000u : 10000u;
        const float p = (t % 5 == 0) ? 0.99f : 0.95f;
        usac::ProsacSampler pro(t + 1, n, m);
        Trial tr(pro.growth(), p, m, n, max_iters);
        uint32_t hyp = (uint32_t)(U(g) * 20);
        const int ncalls = 1 + (int)(U(g) * 8);
        double quality = 0.2 + 0.7 * U(g);
        for (int k = 0; k < ncalls; k++) {
            std::vector<char> inl(n);
            const double front = quality * (0.5 + 0.5 * U(g)), noise = 0.05 * U(g);
            for (uint32_t i = 0; i < n; i++) inl[i] = U(g) < front * (1.0 - (double)i / n) + noise ? 1 : 0;
            const uint32_t largest = m + (uint32_t)(U(g) * (U(g) < 0.5 ? 50 : n));
            calls++;
            if (!tr.call(hyp, inl, largest, "random")) return 1;
            hyp += 1 + (uint32_t)(U(g) * 200);
            quality = std::min(0.95, quality * (1.0 + 0.3 * U(g)));
        }
    }
    // ---- the degenerate patterns, each as a first call and after an all-inlier call, then repeated
    for (uint32_t n : {21u, 22u, 256u, 257u, 515u, 100u}) {
        for (uint32_t m : {4u, 7u}) {
            usac::ProsacSampler pro(1, n, m);
            for (int pat = 0; pat < 8; pat++) {
                std::vector<char> inl(n, 0);
                switch (pat) {
                    case 0: break;                                                                // no inlier
                    case 1: std::fill(inl.begin(), inl.end(), 1); break;                          // all
                    case 2: std::fill(inl.begin(), inl.begin() + 20, 1); break;                   // below 20 only
                    case 3: inl[20] = 1; break;                                                   // one, at 20
                    case 4: for (uint32_t i = 0; i < n; i++) inl[i] = (char)(i % 2 == 0); break;  // alternating
                    case 5: for (uint32_t i = 0; i < n; i++) inl[i] = (char)(i % 2 == 1); break;  // the other phase
                    case 6: std::fill(inl.begin(), inl.begin() + n / 2, 1); inl[n - 1] = 1; break;  // last: inlier
                    default: std::fill(inl.begin(), inl.begin() + n / 2, 1); break;               // last: outlier
                }
                for (int prior = 0; prior < 2; prior++) {
                    Trial tr(pro.growth(), 0.95f, m, n, 10000);
                    if (prior) {
                        calls++;
                        if (!tr.call(3, std::vector<char>(n, 1), n, "prior")) return 1;
                    }
                    calls += 2;
                    if (!tr.call(10, inl, m + 10, "pattern")) return 1;
                    // the same flags again: nothing is raised, so no candidate, same answer
                    if (!tr.call(40, inl, n, "repeat") || !tr.cand.empty()) {
                        printf("diff repeat n %u pattern %d: %zu candidates\n", n, pat, tr.cand.size() / 2);
                        return 1;
                    }
                }
            }
        }
    }
    printf("ok %ld\n", calls);
    return 0;
}
