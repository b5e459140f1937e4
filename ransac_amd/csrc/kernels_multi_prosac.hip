// kernels_multi_prosac.hip -- the device half of PROSAC's termination scan for multi-problem
// batches (DESIGN.md §8b "PROSAC").
//
// ProsacTerminationCriteria::getUpBoundIterations (prosac_termination_criteria.hpp:148-201) walks
// the quality-sorted points of a new best model once: a running inlier count, the per-point update
// non_random[i] = max(non_random[i], count_i) for i >= 20, and at each raised point that ends a run
// of inliers (or is the last point) a candidate termination length whose value takes a log.  The
// walk and the update are O(n) and run here; the candidates are O(n / 2) at most, usually a handful,
// and go to the host in order, where the log is the host libm's (as the reference's) and the ordered
// minimum search keeps its tie rule.  No log on the device.
//
// One workgroup of 256 threads per active entry, launched after the round's argmax.  A workgroup
// whose problem did not improve in this round leaves at once.  Otherwise it walks the problem's
// points in tiles of 256, point i = tile + thread:
//   flag_i    = residual(point i) < thr, the residual of usac_get_inliers / k_multi_mask (H, F or E; H^-1
//               by inv3x3 of the running model);
//   count_i   = inliers among points 0 .. i: the tiles before (a register every thread carries), the
//               waves before in this tile (their ballots' popcounts through LDS), the lanes up to
//               this one (the wave's ballot under the lane mask);
//   flag_i+1  = the next point's own residual, evaluated by this thread: no value crosses a lane,
//               wave or tile boundary, so none can be stale;
//   append    = the candidates of a tile go behind those of the tiles and waves before (the same
//               ballot / LDS scheme), so a problem's segment is in ascending i.
#include <hip/hip_runtime.h>

#include "usac_device.hpp"
#include "usac_device_e5.hpp"
#include "usac_kernels.h"

namespace usac {

namespace {

constexpr uint32_t kScanWaves = kMultiScanTile / 64;
constexpr uint32_t kProsacMinLength = 20;  // min_termination_length (prosac_termination_criteria.hpp)

template <int EST>
__device__ __forceinline__ bool scan_flag(const float4 *__restrict__ pts, uint32_t i, uint32_t n, const float *m,
                                          const float *mi, float thr) {
    if (i >= n) return false;
    const float4 p = pts[i];
    float err;
    if constexpr (EST == USAC_HOMOGRAPHY) err = homography_error(m, mi, p.x, p.y, p.z, p.w);
    else if constexpr (EST == USAC_FUNDAMENTAL) err = fundamental_error(m, p.x, p.y, p.z, p.w);
    else err = essential_error(m, p.x, p.y, p.z, p.w);
    return err < thr;
}

}  // namespace

template <int EST>
__global__ __launch_bounds__(kMultiScanTile) void k_multi_prosac_scan(
    const float4 *__restrict__ pts_all, const uint32_t *__restrict__ offsets, const MultiItem *__restrict__ items,
    const usac_record *__restrict__ running, uint64_t first_hyp, float thr_s, const float *__restrict__ thrs,
    uint32_t *__restrict__ non_random, uint32_t *__restrict__ cand, uint32_t *__restrict__ cand_n) {
    // the waves' inlier and candidate totals of the current tile: each is written before one of the
    // tile's two barriers and read after it, so the next tile's writes cannot overtake a read
    __shared__ uint32_t sh_inl[kScanWaves], sh_cand[kScanWaves];
    const uint32_t a = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t prob = items[a].problem;
    const usac_record *__restrict__ rec = running + prob;
    if (!rec->valid || rec->hyp_index < first_hyp) {  // block-uniform: no new best in this round
        if (t == 0) cand_n[a] = 0;
        return;
    }
    const float thr = thrs ? thrs[prob] : thr_s;  // per-problem thresholds: the workgroup's problem's
    const uint32_t base = offsets[prob], n = offsets[prob + 1] - base;
    const float4 *__restrict__ pts = pts_all + base;
    uint32_t *__restrict__ nr = non_random + base;
    const size_t seg = 2 * multi_cand_offset(base, prob);
    const uint32_t cap = (n >> 1) + 1;
    float m[9], mi[9] = {};
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = rec->model[k];
    if (EST == USAC_HOMOGRAPHY) inv3x3(m, mi);
    uint32_t count0 = 0, ncand = 0;  // inliers / candidates of the tiles before (block-uniform)
    for (uint32_t tile = 0; tile < n; tile += kMultiScanTile) {
        const uint32_t i = tile + t;
        const bool flag = scan_flag<EST>(pts, i, n, m, mi, thr);
        const bool next = scan_flag<EST>(pts, i + 1, n, m, mi, thr);
        const unsigned long long bal = __ballot(flag);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (lane == 0) sh_inl[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kScanWaves; w++) {
            const uint32_t v = sh_inl[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        const uint32_t count = count0 + before + below + (flag ? 1u : 0u);
        bool is_cand = false;
        if (i >= kProsacMinLength && i < n && nr[i] < count) {
            nr[i] = count;
            is_cand = i == n - 1 || (flag && !next);
        }
        const unsigned long long cbal = __ballot(is_cand);
        const uint32_t cbelow =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(cbal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cbal, 0u));
        if (lane == 0) sh_cand[wave] = (uint32_t)__popcll(cbal);
        __syncthreads();
        uint32_t cbefore = 0, ctotal = 0;
#pragma unroll
        for (uint32_t w = 0; w < kScanWaves; w++) {
            const uint32_t v = sh_cand[w];
            cbefore += w < wave ? v : 0u;
            ctotal += v;
        }
        const uint32_t pos = ncand + cbefore + cbelow;
        if (is_cand && pos < cap) {  // (pos < cap always: a candidate needs a 1 -> 0 step or the last point)
            cand[seg + 2 * (size_t)pos] = i;
            cand[seg + 2 * (size_t)pos + 1] = count;
        }
        count0 += total;
        ncand += ctotal;
    }
    if (t == 0) cand_n[a] = ncand < cap ? ncand : cap;
}

hipError_t launch_multi_prosac_scan(hipStream_t st, int estimator, const float4 *pts, const uint32_t *offsets,
                                    const MultiItem *items, uint32_t A, const usac_record *running,
                                    uint64_t first_hyp, float thr, const float *thrs, uint32_t *non_random,
                                    uint32_t *cand, uint32_t *cand_n) {
    if (A == 0) return hipErrorInvalidValue;
    if (estimator == USAC_HOMOGRAPHY)
        hipLaunchKernelGGL(k_multi_prosac_scan<USAC_HOMOGRAPHY>, dim3(A), dim3(kMultiScanTile), 0, st, pts, offsets, items, running,
                           first_hyp, thr, thrs, non_random, cand, cand_n);
    else if (estimator == USAC_FUNDAMENTAL)
        hipLaunchKernelGGL(k_multi_prosac_scan<USAC_FUNDAMENTAL>, dim3(A), dim3(kMultiScanTile), 0, st, pts, offsets, items,
                           running, first_hyp, thr, thrs, non_random, cand, cand_n);
    else if (estimator == USAC_ESSENTIAL)
        hipLaunchKernelGGL(k_multi_prosac_scan<USAC_ESSENTIAL>, dim3(A), dim3(kMultiScanTile), 0, st, pts, offsets, items,
                           running, first_hyp, thr, thrs, non_random, cand, cand_n);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace usac
