// Device input of a multi context (ABI 25, usac_multi_create_device): the pack, an order-preserving compaction
// of padded per-problem input into the concatenated N_total x 4 rows every multi kernel reads, and the unpack,
// the scatter of a mask over the packed rows back into the padded P x n_max layout (usac_multi_padded_mask).
//
// Two passes, one 256-thread workgroup per problem each, with the host between them (DESIGN.md §8b "Device
// input"): k_multi_pack_count writes each problem's kept rows and error flags, the host takes the exclusive
// sum (usac_pack.hpp; P <= 65535 values earn no launch), k_multi_pack writes the rows and their source columns.
// Both walk n_max in blocks of 256 columns; a kept column's place is the problem's running base, plus the
// kept columns of the waves before its own (four totals through LDS), plus those of the lanes below it (the
// ballot).  Columns stay in ascending order, so quality-sorted input stays sorted for PROSAC.
//
// Rows are moved as integers, 16 or 8 bytes at a time, with no arithmetic on them: every bit arrives as it
// was, NaN payloads and negative zeros included.  Both passes are bound by the bytes they move: neighbouring
// lanes read neighbouring columns, and a wave's kept rows land in one contiguous run.
#include <hip/hip_runtime.h>

#include "usac_kernels.h"

namespace usac {

namespace {

// does column j of problem p stay, and (form b) which row of kpts1 goes with it; err gathers the problem's flags
__device__ __forceinline__ bool pack_keep(const MultiPack &a, uint32_t p, uint32_t j, uint32_t limit, uint32_t &target,
                                          uint32_t &err) {
    target = 0;
    if (j >= a.n_max) return false;
    const size_t at = (size_t)p * a.n_max + j;
    if (a.match) {
        const int32_t t = a.match[at];
        if (t < 0) return false;
        if ((uint32_t)t >= a.n1) {  // never dereferenced: the problem is refused
            err |= kPackFlagMatch;
            return false;
        }
        target = (uint32_t)t;
        return true;
    }
    if (a.valid) return a.valid[at] != 0;
    return j < limit;  // counts (the prefix form), or everything
}

// counts[p] as the number of leading columns kept: n_max without counts, 0 and a flag where it is out of range
__device__ __forceinline__ uint32_t pack_limit(const MultiPack &a, uint32_t p, uint32_t &err) {
    if (!a.counts) return a.n_max;
    const int32_t c = a.counts[p];
    if (c < 0 || (uint32_t)c > a.n_max) {
        err |= kPackFlagCount;
        return 0;
    }
    return (uint32_t)c;
}

// blocks of 256 columns over n_max; block b's columns b * 256 + 0..255 stay below 2^32 for any n_max
__device__ __forceinline__ uint32_t pack_blocks(uint32_t n_max) { return (n_max >> 8) + ((n_max & 255u) != 0u); }

}  // namespace

// sizes[p]: the kept columns of problem p; flags[p]: kPackFlag* of what the problem must be refused for
__global__ __launch_bounds__(256) void k_multi_pack_count(MultiPack a, uint32_t *__restrict__ sizes,
                                                          uint32_t *__restrict__ flags) {
    __shared__ uint32_t sh_n[4], sh_err[4];
    const uint32_t p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t err = 0, n = 0, target;
    const uint32_t limit = pack_limit(a, p, err);
    for (uint32_t b = 0; b < pack_blocks(a.n_max); b++)
        n += (uint32_t)__popcll(__ballot(pack_keep(a, p, b * 256 + threadIdx.x, limit, target, err)));
    const bool e_cnt = __ballot((err & kPackFlagCount) != 0) != 0, e_match = __ballot((err & kPackFlagMatch) != 0) != 0;
    if (lane == 0) {
        sh_n[wave] = n;
        sh_err[wave] = (e_cnt ? kPackFlagCount : 0u) | (e_match ? kPackFlagMatch : 0u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sizes[p] = (sh_n[0] + sh_n[1]) + (sh_n[2] + sh_n[3]);
        flags[p] = (sh_err[0] | sh_err[1]) | (sh_err[2] | sh_err[3]);
    }
}

// pts / src: the packed rows and their columns; offsets: the exclusive sum of the sizes k_multi_pack_count wrote.
// A problem writes inside offsets[p] .. offsets[p + 1] - 1 whatever its input holds by now.
__global__ __launch_bounds__(256) void k_multi_pack(MultiPack a, const uint32_t *__restrict__ offsets,
                                                    uint4 *__restrict__ pts, uint32_t *__restrict__ src) {
    __shared__ uint32_t sh_n[2][4];
    const uint32_t p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t out0 = offsets[p], room = offsets[p + 1] - out0;
    uint32_t err = 0, running = 0, target;
    const uint32_t limit = pack_limit(a, p, err);
    for (uint32_t b = 0, it = 0; b < pack_blocks(a.n_max); b++, it ^= 1) {
        const uint32_t j = b * 256 + threadIdx.x;
        const bool keep = pack_keep(a, p, j, limit, target, err);
        const unsigned long long bal = __ballot(keep);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        // two copies of the totals, taken in turn: a wave writes a copy again only after the barrier of the
        // block in between, which every wave reaches after it has read that copy
        if (lane == 0) sh_n[it][wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        const uint32_t t0 = sh_n[it][0], t1 = sh_n[it][1], t2 = sh_n[it][2], t3 = sh_n[it][3];
        const uint32_t before = wave == 0 ? 0u : wave == 1 ? t0 : wave == 2 ? t0 + t1 : t0 + t1 + t2;
        const uint32_t at = running + before + below;
        if (keep && at < room) {
            const size_t col = (size_t)p * a.n_max + j;
            uint4 row;
            if (a.match) {
                const uint2 q0 = a.kpts0[col], q1 = a.kpts1[(size_t)p * a.n1 + target];
                row = make_uint4(q0.x, q0.y, q1.x, q1.y);
            } else {
                row = a.rows[col];
            }
            pts[(size_t)out0 + at] = row;
            src[(size_t)out0 + at] = j;
        }
        running += (t0 + t1) + (t2 + t3);
    }
}

// out[p, src[i]] = mask[i] over the packed rows, one thread per row, its problem by bisection of offsets (as
// k_multi_calibrate); the caller has cleared out.  src[i] < n_max by construction (k_multi_pack wrote it).
__global__ __launch_bounds__(256) void k_multi_unpack_mask(const uint8_t *__restrict__ mask,
                                                           const uint32_t *__restrict__ src,
                                                           const uint32_t *__restrict__ offsets, uint32_t P,
                                                           uint32_t n_total, uint32_t n_max, uint8_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    uint32_t lo = 0, hi = P;  // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    const uint32_t j = src[i];
    if (j < n_max) out[(size_t)lo * n_max + j] = mask[i];
}

hipError_t launch_multi_pack_count(hipStream_t st, const MultiPack &a, uint32_t *sizes, uint32_t *flags) {
    if (a.P == 0 || a.P > kMultiMaxActive || a.n_max == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_multi_pack_count, dim3(a.P), dim3(256), 0, st, a, sizes, flags);
    return hipGetLastError();
}

hipError_t launch_multi_pack(hipStream_t st, const MultiPack &a, const uint32_t *offsets, float4 *pts, uint32_t *src) {
    if (a.P == 0 || a.P > kMultiMaxActive || a.n_max == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_multi_pack, dim3(a.P), dim3(256), 0, st, a, offsets, reinterpret_cast<uint4 *>(pts), src);
    return hipGetLastError();
}

hipError_t launch_multi_unpack_mask(hipStream_t st, const uint8_t *mask, const uint32_t *src, const uint32_t *offsets,
                                    uint32_t P, uint32_t n_total, uint32_t n_max, uint8_t *out) {
    if (P == 0 || n_total == 0 || n_max == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_multi_unpack_mask, dim3((n_total + 255) / 256), dim3(256), 0, st, mask, src, offsets, P, n_total,
                       n_max, out);
    return hipGetLastError();
}

}  // namespace usac
