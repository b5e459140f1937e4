// usac_multi_sampler.hpp -- the device samplers of multi-problem batches, shared by the solve kernels
// of kernels_multi.hip (H, F) and kernels_ess.hip (E) and by k_multi_draw.
#pragma once
#include <hip/hip_runtime.h>

#include "usac_device.hpp"
#include "usac_kernels.h"
#include "usac_prosac.hpp"

namespace usac {

namespace {

__device__ __forceinline__ DevSampler uniform_sampler(uint64_t seed) {
    DevSampler ds{};
    ds.seed = seed;
    return ds;
}

// The sampler of an instantiation and the kernels' last argument under it: the growth functions
// (PROSAC; unused by the uniform sampler) or the problems' grids (NAPSAC, kernels_multi_grid.hip).
enum : int { kUniform = 0, kProsac = 1, kNapsac = 2 };
template <int SAMPLER>
struct SamplerArg {
    using type = const uint32_t *__restrict__;
};
template <>
struct SamplerArg<kNapsac> {
    using type = MultiGrid;
};

// Lane h's sample of a round.  Uniform: draw_sample over n_p.  PROSAC (usac_prosac.hpp's closed form
// over the problem's growth function g, the item's clock T and termination length L): t = T + h,
//   t > T_N        : M distinct indices of [0, n)        (the reference past its growth table)
//   s(t - 1) > L   : M distinct indices of [0, L]        (closed range, L < n; the subset is tested
//                                                          before this call's increment)
//   otherwise      : M - 1 distinct indices of [0, s(t) - 2] and point s(t) - 1
// from the (seed, global hypothesis index) stream either way: the first M - 1 draws are
// draw_unique's over the branch's range, the last one is its M-th step or the fixed point.
// NAPSAC: draw_sample's NAPSAC branch over the problem's slices of the grid CSR (block-uniform bases):
// the initial point uniform over the eligible points, M - 1 consecutive neighbours from a random
// phase, uniform samples for a problem without an eligible point -- what a usac_ctx over the
// problem's points draws after usac_set_cell_size and usac_set_device_sampler(NAPSAC).
template <int M, bool PROSAC>
__device__ __forceinline__ void stream_sample(const MultiItem &it, const uint32_t *__restrict__ g, uint32_t n,
                                              uint64_t hyp, uint32_t h, int32_t (&s)[M]) {
    if constexpr (!PROSAC) {
        draw_sample<M>(uniform_sampler(it.seed), hyp, n, s);
    } else {
        uint64_t st = it.seed ^ (hyp * 0xD1B54A32D192ED03ull);
        const uint32_t t = it.clock + h;
        uint32_t range = n, last = 0;  // last != 0: the fixed point + 1
        if (t <= kProsacGrowthMax) {
            uint32_t s_prev, s_now;
            prosac_subset_pair(g, n, (uint32_t)M, t, s_prev, s_now);
            if (s_prev > it.term_len) {
                range = it.term_len + 1;
            } else {
                range = s_now - 1;
                last = s_now;
            }
        }
        draw_unique<M - 1>(st, range, s);
        if (last) {
            s[M - 1] = (int32_t)last - 1;
        } else {  // draw_unique<M>'s last step
            int32_t v;
            bool dup;
            do {
                const uint64_t r = splitmix64(st);
                v = (int32_t)(((r >> 32) * (uint64_t)range) >> 32);
                dup = false;
#pragma unroll
                for (int j = 0; j < M - 1; j++) dup |= (s[j] == v);
            } while (dup);
            s[M - 1] = v;
        }
    }
}

template <int M, int SAMPLER>
__device__ __forceinline__ void multi_sample(const MultiItem &it, const typename SamplerArg<SAMPLER>::type &aux,
                                             uint32_t base, uint32_t n, uint64_t hyp, uint32_t h, int32_t (&s)[M]) {
    if constexpr (SAMPLER == kNapsac) {
        DevSampler ds{};
        ds.seed = it.seed;
        ds.nap_n_eligible = aux.n_eligible[it.problem];
        ds.nap_cell = aux.cell + base;
        ds.nap_rank = aux.rank + base;
        ds.nap_start = aux.start + base + it.problem;
        ds.nap_members = aux.members + base;
        ds.nap_eligible = aux.eligible + base;
        draw_sample<M>(ds, hyp, n, s);
    } else {
        stream_sample<M, SAMPLER == kProsac>(it, aux + base, n, hyp, h, s);
    }
}

}  // namespace

}  // namespace usac
