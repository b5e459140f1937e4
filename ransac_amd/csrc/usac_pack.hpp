// Device input of a multi context (ABI 25, usac_multi_create_device), the host-only part: the extent check
// of the padded input and the step between the two pack kernels (kernels_multi_pack.hip) -- the problems'
// kept-row counts and error flags in, their offsets or the first problem to refuse out.  No HIP call and no
// other header of the library, so a stand-alone program can include it (tests/cpp_multi_device/pack_check.cpp).
#pragma once
#include <cstdint>
#include <string>

namespace usac {

// what k_multi_pack_count reports of a problem beside its size
constexpr uint32_t kPackFlagCount = 1u;  // counts[p] < 0 or > n_max
constexpr uint32_t kPackFlagMatch = 2u;  // a match index >= n1

enum PackStatus { kPackOk = 0, kPackBadCount = 1, kPackBadMatch = 2, kPackTooFew = 3, kPackOverflow = 4 };

// P x n_max cells are indexed in 32 bits by the unpack and allocated by the caller
inline bool pack_extent_ok(uint32_t P, uint32_t n_max) {
    return P != 0 && n_max != 0 && (uint64_t)P * n_max < (1ull << 32);
}

// the outputs of usac_multi_export_device (ABI 27) under the same rule: P x n_max mask bytes and, where a list is
// asked for (k_max != 0), P x k_max entries
inline bool export_extent_ok(uint32_t P, uint32_t n_max, uint32_t k_max) {
    return pack_extent_ok(P, n_max) && (k_max == 0 || pack_extent_ok(P, k_max));
}

// The width a caller names for P x n_max output bytes (usac_multi_export_device, and usac_multi_pose_device of ABI
// 28).  ctx_n_max: the padded width of a context from device input, 0 for a context created from the host, whose
// source is the identity so that every local index below `widest` (the largest problem's size) needs a column.
enum WidthStatus { kWidthOk = 0, kWidthNotTheContexts = 1, kWidthBelowWidest = 2 };
inline uint32_t widest_problem(const uint32_t *offsets, uint32_t P) {
    uint32_t widest = 0;
    for (uint32_t p = 0; p < P; p++)
        if (offsets[p + 1] - offsets[p] > widest) widest = offsets[p + 1] - offsets[p];
    return widest;
}
inline WidthStatus output_width(uint32_t ctx_n_max, uint32_t widest, uint32_t n_max) {
    if (ctx_n_max) return n_max == ctx_n_max ? kWidthOk : kWidthNotTheContexts;
    return n_max >= widest ? kWidthOk : kWidthBelowWidest;
}
inline std::string width_message(WidthStatus st, uint32_t ctx_n_max, uint32_t widest) {
    switch (st) {
    case kWidthNotTheContexts: return "n_max must be the context's, " + std::to_string(ctx_n_max);
    case kWidthBelowWidest: return "n_max must be at least the largest problem's size, " + std::to_string(widest);
    default: return "";
    }
}

// Pose refinement (ABI 29).  The step limit both entries take, and the one device block usac_multi_refine_pose
// stages its host arrays through: P problems, n packed rows.  The doubles come first so that they are 8-byte
// aligned at any P; R and t are refined in place; the mask's n bytes come last.
constexpr uint32_t kRefineIterLimit = 100;
inline bool refine_iters_ok(uint32_t max_iters) { return max_iters <= kRefineIterLimit; }
struct RefineBlock {
    size_t cost0, cost, R, t, E, iterations, used, mask, bytes;
};
inline RefineBlock refine_block(size_t P, size_t n) {
    RefineBlock b;
    b.cost0 = 0;
    b.cost = b.cost0 + 8 * P;
    b.R = b.cost + 8 * P;
    b.t = b.R + 36 * P;
    b.E = b.t + 12 * P;
    b.iterations = b.E + 36 * P;
    b.used = b.iterations + 4 * P;
    b.mask = b.used + 4 * P;
    b.bytes = b.mask + n;
    return b;
}

// sizes[P], flags[P] -> offsets[P + 1] (offsets[0] = 0, the exclusive sum).  Returns kPackOk, or what the first
// offending problem *bad is refused for (offsets is then unspecified): a flag the kernel raised, a size above
// n_max (no count of n_max columns is), fewer kept rows than the sample size m, or a total of 2^32 rows or more.
inline PackStatus pack_offsets(const uint32_t *sizes, const uint32_t *flags, uint32_t P, uint32_t m, uint32_t n_max,
                               uint32_t *offsets, uint32_t *bad) {
    uint64_t sum = 0;
    offsets[0] = 0;
    for (uint32_t p = 0; p < P; p++) {
        *bad = p;
        if (flags[p] & kPackFlagCount) return kPackBadCount;
        if (flags[p] & kPackFlagMatch) return kPackBadMatch;
        if (sizes[p] > n_max) return kPackBadCount;
        if (sizes[p] < m) return kPackTooFew;
        sum += sizes[p];
        if (sum >= (1ull << 32)) return kPackOverflow;
        offsets[p + 1] = (uint32_t)sum;
    }
    *bad = P;
    return kPackOk;
}

// the report of a refusal, naming the problem
inline std::string pack_message(PackStatus st, uint32_t p, uint32_t size, uint32_t m) {
    const std::string who = "problem " + std::to_string(p) + ": ";
    switch (st) {
    case kPackBadCount: return who + "counts[p] is negative or above n_max";
    case kPackBadMatch: return who + "a match index is >= n1";
    case kPackTooFew:
        return who + std::to_string(size) + " kept rows, fewer than the sample size " + std::to_string(m);
    case kPackOverflow: return who + "the kept rows of the problems up to it number 2^32 or more";
    default: return "";
    }
}

}  // namespace usac
