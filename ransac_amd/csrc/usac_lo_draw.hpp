// usac_lo_draw.hpp -- the sample sets of the multi-problem LO (kernels_nonmin.hip k_multi_lo), shared
// by the host (usac_api.cpp usac_lo_draw, which the tests' restatement draws through) and the device:
// one text, so the two cannot drift apart.
//
// lo_draw is UniformRandomGenerator::generateUniqueRandomSet(sample, max) with the reference's
// generator replaced by the device sampler's SplitMix64 (usac_device.hpp), as the uniform multi
// sampler replaces the glibc stream: k distinct integers of the closed range [0, max], in draw
// order, by draw_unique's rejection loop with k a run-time value.  The stream is keyed by (problem
// seed, kLoDrawTag, draw), draw = the number of sets drawn so far for the problem in the run; the
// tag keeps it apart from the hypothesis streams seed ^ (hyp * 0xD1B54A32D192ED03).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define USAC_LO_HD __host__ __device__ __forceinline__
#else
#define USAC_LO_HD inline
#endif

namespace usac {

constexpr uint32_t kLoDrawMax = 64;  // the largest lo_sample_size of the multi-problem LO
constexpr uint64_t kLoDrawTag = 0x4C4F5F44524157A5ull;

USAC_LO_HD uint64_t lo_splitmix64(uint64_t &s) {  // usac_device.hpp splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// k <= max + 1 (else the loop does not end): the callers check
USAC_LO_HD void lo_draw(uint64_t seed, uint64_t draw, uint32_t k, uint32_t max, int32_t *out) {
    uint64_t st = seed ^ kLoDrawTag ^ (draw * 0xD1B54A32D192ED03ull);
    const uint64_t range = (uint64_t)max + 1;
    for (uint32_t i = 0; i < k; i++) {
        int32_t v;
        bool dup;
        do {
            const uint64_t r = lo_splitmix64(st);
            v = (int32_t)(((r >> 32) * range) >> 32);
            dup = false;
            for (uint32_t j = 0; j < i; j++) dup |= (out[j] == v);
        } while (dup);
        out[i] = v;
    }
}

}  // namespace usac
