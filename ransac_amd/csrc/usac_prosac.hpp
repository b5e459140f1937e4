// usac_prosac.hpp -- the PROSAC sampler's subset size in closed form, shared by the host
// (usac_host.hpp, usac_api.cpp) and the device (kernels_multi.hip): one text, so the two cannot
// drift apart.
//
// ProsacSampler::generateSample (prosac_sampler.hpp:117-172) grows its subset by at most one per
// call, when hypCount > growth[subset - 1].  growth is strictly increasing from index m - 1, so
// after the call with hypCount = t the subset is
//     s(t) = min(n, m + #{ i in [m - 1, n) : growth[i] < t }),   s(0) = m,
// a bisection over the growth function instead of a per-hypothesis table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define USAC_HD __host__ __device__ __forceinline__
#else
#define USAC_HD inline
#endif

namespace usac {

constexpr uint32_t kProsacGrowthMax = 200000;  // T_N (prosac_sampler.hpp:62): later samples are uniform

// #{ i in [m - 1, n) : g[i] < x }
USAC_HD uint32_t prosac_growth_below(const uint32_t *g, uint32_t n, uint32_t m, uint32_t x) {
    uint32_t lo = m - 1, hi = n;  // g[i] < x for i in [m - 1, lo), g[i] >= x for i in [hi, n)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo - (m - 1);
}

USAC_HD uint32_t prosac_subset(const uint32_t *g, uint32_t n, uint32_t m, uint32_t t) {
    const uint32_t s = m + prosac_growth_below(g, n, m, t);
    return s < n ? s : n;
}

// s(t - 1) and s(t) from one bisection: the count grows by at most one from t - 1 to t (the
// growth values are distinct integers), and then by the next entry alone.  t >= 1.
USAC_HD void prosac_subset_pair(const uint32_t *g, uint32_t n, uint32_t m, uint32_t t, uint32_t &s_prev,
                                uint32_t &s_now) {
    const uint32_t c = prosac_growth_below(g, n, m, t - 1), next = m - 1 + c;
    const uint32_t c1 = c + ((next < n && g[next] < t) ? 1u : 0u);
    s_prev = m + c < n ? m + c : n;
    s_now = m + c1 < n ? m + c1 : n;
}

}  // namespace usac
