// kernels_multi.hip -- multi-problem batches (DESIGN.md "Multi-problem batches"): one launch over
// (active problem, 64-hypothesis tile) for P independent two-view problems of one estimator.
//
// Layout:
//   points   : N_total x float4, the problems' rows concatenated; offsets[P + 1], problem p owns
//              rows offsets[p] .. offsets[p + 1] - 1 (sample, hypothesis and inlier indices are
//              local to the problem);
//   items    : A x MultiItem, the launch's active list (problem id, its sampler seed and, for the
//              PROSAC sampler, the round's clock and termination length);
//   growth   : PROSAC only, N_total uint32: problem p's growth function at growth + offsets[p];
//   grid     : NAPSAC only, the problems' grid neighbours (MultiGrid, kernels_multi_grid.hip);
//   models   : per-launch SoA slab over the A * R hypotheses of the launch, hypothesis h of
//              active entry a at g = a * R + h -- H: [18][A R] (H then H^-1), F: [9][3 A R] with
//              slot 3 g + j = the j-th valid model of the sample (seven_points.cpp root order),
//              E: [9][A R], slot g = the sample's model (launch_multi_solve_e5, kernels_ess.hip);
//   counts / sums : per slot, count -1 on an empty F / E slot;
//   list / list_n : F and E, per active entry the occupied slots (spk R entries each, any order).
//
// Every per-hypothesis step is the single-problem path's device math (usac_device.hpp), so a
// problem's models, counts and sums equal those of a usac_ctx over its points bit for bit: the
// sample of (seed, global hypothesis index) by draw_sample over n_p (or, in the PROSAC
// instantiations, by stream_sample's closed-form PROSAC rule on the same stream; in the NAPSAC ones, by
// draw_sample's NAPSAC branch over the problem's grid), the thin-QR DLT with the
// row-Jacobi fall-back (or the 7-point chain), and the ONE-CHUNK score: each lane walks its
// problem's points in order, so Σ is the reference's sequential fp32 sum.  R is a multiple of
// 64: a wave never spans two problems, so the problem id, the point base and every point are
// wave-uniform (scalar loads).  No point chunking: a problem's points are walked by one wave per
// 64 hypotheses, which suits problems of up to a few thousand points.
#include <hip/hip_runtime.h>

#include "usac_device.hpp"
#include "usac_device_e5.hpp"
#include "usac_kernels.h"
#include "usac_multi_sampler.hpp"
#include "usac_prosac.hpp"

namespace usac {

namespace {

// as kernels.hip store_h: H = v / v[8] in fp64, one cast, H^-1 by inv3x3
__device__ __forceinline__ void multi_store_h(float *__restrict__ models, size_t stride, size_t g, const double *v) {
    float H[9], Hi[9];
#pragma unroll
    for (int k = 0; k < 9; k++) H[k] = (float)(v[k] / v[8]);
    inv3x3(H, Hi);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        models[(size_t)k * stride + g] = H[k];
        models[(size_t)(9 + k) * stride + g] = Hi[k];
    }
}

__device__ __forceinline__ void multi_dlt_system(const float4 *__restrict__ pts, const int32_t (&s)[4],
                                                 double (&W)[8][9]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float4 p = pts[s[i]];
        dlt_rows(p.x, p.y, p.z, p.w, W[2 * i], W[2 * i + 1]);
    }
}

}  // namespace

// ------------------------------------------------------------------------ solve (H, 4-pt)
// grid (R / 64, A).  Thin mode: dlt4_thin_qr, and the lanes it refuses solve the rebuilt system by
// row_jacobi + pick_vector in the same kernel (what k_solve_h4_jac does for k_solve_h4's list);
// nullspace mode: the row Jacobi for every lane.
template <bool NULLSPACE, int SAMPLER>
__global__ __launch_bounds__(64) void k_multi_solve_h4(const float4 *__restrict__ pts_all,
                                                       const uint32_t *__restrict__ offsets,
                                                       const MultiItem *__restrict__ items,
                                                       const int32_t *__restrict__ samples_in, uint32_t R,
                                                       uint64_t first_hyp, float *__restrict__ models,
                                                       const typename SamplerArg<SAMPLER>::type aux) {
    const uint32_t a = blockIdx.y;
    const MultiItem it = items[a];
    const uint32_t base = offsets[it.problem], n = offsets[it.problem + 1] - base;
    const float4 *__restrict__ pts = pts_all + base;
    const uint32_t h = blockIdx.x * 64 + threadIdx.x;
    const size_t g = (size_t)a * R + h, stride = (size_t)gridDim.y * R;
    int32_t s[4];
    if (samples_in) {
#pragma unroll
        for (int i = 0; i < 4; i++) s[i] = samples_in[4 * g + i];
    } else {
        multi_sample<4, SAMPLER>(it, aux, base, n, first_hyp + h, h, s);
    }
    double W[8][9];
    double v[9];
    multi_dlt_system(pts, s, W);
    if constexpr (!NULLSPACE) {
        if (dlt4_thin_qr(W, v)) {
            multi_store_h(models, stride, g, v);
            return;
        }
        multi_dlt_system(pts, s, W);
    }
    row_jacobi<8>(W);
    pick_vector<8>(W, NULLSPACE ? 1 : 0, v);
    multi_store_h(models, stride, g, v);
}

// ------------------------------------------------------------------------ solve (F, 7-pt)
// grid (R / 64, A): k_solve_f7's chain per lane, slots 3 g + j, the occupied slots appended to
// the active entry's list (wave-aggregated atomic on list_n[a], zeroed by the launcher).
template <int SAMPLER>
__global__ __launch_bounds__(64) void k_multi_solve_f7(const float4 *__restrict__ pts_all,
                                                       const uint32_t *__restrict__ offsets,
                                                       const MultiItem *__restrict__ items,
                                                       const int32_t *__restrict__ samples_in, uint32_t R,
                                                       uint64_t first_hyp, float *__restrict__ models,
                                                       int32_t *__restrict__ counts, float *__restrict__ sums,
                                                       uint32_t *__restrict__ list, uint32_t *__restrict__ list_n,
                                                       const typename SamplerArg<SAMPLER>::type aux) {
    const uint32_t a = blockIdx.y;
    const MultiItem it = items[a];
    const uint32_t base = offsets[it.problem], n = offsets[it.problem + 1] - base;
    const float4 *__restrict__ pts = pts_all + base;
    const uint32_t lane = threadIdx.x;
    const uint32_t h = blockIdx.x * 64 + lane;
    const size_t g = (size_t)a * R + h, stride = 3 * (size_t)gridDim.y * R;
    int nvalid = 0;
    {
        int32_t s[7];
        if (samples_in) {
#pragma unroll
            for (int i = 0; i < 7; i++) s[i] = samples_in[7 * g + i];
        } else {
            multi_sample<7, SAMPLER>(it, aux, base, n, first_hyp + h, h, s);
        }
        double W[7][9];
#pragma unroll
        for (int i = 0; i < 7; i++) {
            const float4 p = pts[s[i]];
            fund_row(p.x, p.y, p.z, p.w, W[i]);
        }
        double N[2][9];
        if (!qr_null<7>(W, N)) {  // a zero / non-finite column: the row-Jacobi completion
#pragma unroll
            for (int i = 0; i < 7; i++) {
                const float4 p = pts[s[i]];
                fund_row(p.x, p.y, p.z, p.w, W[i]);
            }
            row_jacobi<7>(W);
            null_complement7(W, N);
        }
        float f1[9], f2[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            f1[k] = (float)N[0][k];
            f2[k] = (float)N[1][k];
        }
        float c[4];
        fund_cubic(f1, f2, c);
        double r[3];
        const int nr = cubic_roots((double)c[0], (double)c[1], (double)c[2], (double)c[3], r);
        for (int j = 0; j < nr; j++) {
            float F[9];
            fund_from_root(f1, f2, (float)r[j], F);
            if (fund_oriented(F, pts, s)) {
                const size_t slot = 3 * g + nvalid;
#pragma unroll
                for (int k = 0; k < 9; k++) models[(size_t)k * stride + slot] = F[k];
                nvalid++;
            }
        }
        for (int j = 0; j < 3; j++) {  // an empty slot reads (-1, 0)
            counts[3 * g + j] = j < nvalid ? 0 : -1;
            sums[3 * g + j] = 0.f;
        }
    }
    uint32_t incl = (uint32_t)nvalid;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += v;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    uint32_t lbase = 0;
    if (lane == 63 && total) lbase = atomicAdd(list_n + a, total);
    lbase = __shfl(lbase, 63, 64);
    uint32_t *__restrict__ my = list + 3 * (size_t)a * R + lbase + incl - (uint32_t)nvalid;
    for (int j = 0; j < nvalid; j++) my[j] = (uint32_t)(3 * g) + (uint32_t)j;
}

// ------------------------------------------------------------------------ score
// grid (R / 64, A), one wave: lanes = the tile's hypotheses, the problem's points in order by
// scalar loads (as k_score_h<1>)
__global__ __launch_bounds__(64) void k_multi_score_h(const float4 *__restrict__ pts_all,
                                                      const uint32_t *__restrict__ offsets,
                                                      const MultiItem *__restrict__ items,
                                                      const float *__restrict__ models, uint32_t R, float thr_s,
                                                      const float *__restrict__ thrs,
                                                      int32_t *__restrict__ counts, float *__restrict__ sums) {
    const uint32_t a = blockIdx.y;
    const uint32_t prob = items[a].problem;
    const float thr = thrs ? thrs[prob] : thr_s;  // per-problem thresholds: the workgroup's problem's
    const uint32_t base = offsets[prob], n = offsets[prob + 1] - base;
    const float4 *__restrict__ pts = pts_all + base;
    const size_t g = (size_t)a * R + blockIdx.x * 64 + threadIdx.x, stride = (size_t)gridDim.y * R;
    float H[9], Hi[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        H[k] = models[(size_t)k * stride + g];
        Hi[k] = models[(size_t)(9 + k) * stride + g];
    }
    int cnt = 0;
    float sum = 0.f;
    for (uint32_t i = 0; i < n; ++i) {
        const float4 p = pts[i];
        const float err = homography_error(H, Hi, p.x, p.y, p.z, p.w);
        if (err < thr) {
            cnt++;
            sum += err;
        }
    }
    counts[g] = cnt;
    sums[g] = sum;
}

template <int EST>
__device__ __forceinline__ float multi_epipolar_error(const float *f, const float4 &p) {
    if constexpr (EST == USAC_ESSENTIAL) return essential_error(f, p.x, p.y, p.z, p.w);
    else return fundamental_error(f, p.x, p.y, p.z, p.w);
}

// grid (SPK R / 64, A), SPK = 3 (F) or 1 (E) slots per sample: lanes walk the active entry's
// occupied-slot list (as k_score_f<1, EST>); tiles past the list's end leave at once
template <int EST>
__global__ __launch_bounds__(64) void k_multi_score_f(const float4 *__restrict__ pts_all,
                                                      const uint32_t *__restrict__ offsets,
                                                      const MultiItem *__restrict__ items,
                                                      const float *__restrict__ models, uint32_t R,
                                                      const uint32_t *__restrict__ list,
                                                      const uint32_t *__restrict__ list_n, float thr_s,
                                                      const float *__restrict__ thrs,
                                                      int32_t *__restrict__ counts, float *__restrict__ sums) {
    constexpr uint32_t SPK = EST == USAC_FUNDAMENTAL ? 3 : 1;
    const uint32_t a = blockIdx.y;
    const uint32_t K = __builtin_amdgcn_readfirstlane(list_n[a]);
    const uint32_t i0 = blockIdx.x * 64;
    if (i0 >= K) return;  // block-uniform
    const uint32_t prob = items[a].problem;
    const float thr = thrs ? thrs[prob] : thr_s;  // per-problem thresholds: the workgroup's problem's
    const uint32_t base = offsets[prob], n = offsets[prob + 1] - base;
    const float4 *__restrict__ pts = pts_all + base;
    const size_t stride = SPK * (size_t)gridDim.y * R;
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t slot = list[SPK * (size_t)a * R + (i < K ? i : K - 1)];
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = models[(size_t)k * stride + slot];
    int cnt = 0;
    float sum = 0.f;
    uint32_t p = 0;
    for (; p + 4 <= n; p += 4) {
        const float4 a0 = pts[p], a1 = pts[p + 1], a2 = pts[p + 2], a3 = pts[p + 3];
        const float e0 = multi_epipolar_error<EST>(f, a0);
        const float e1 = multi_epipolar_error<EST>(f, a1);
        const float e2 = multi_epipolar_error<EST>(f, a2);
        const float e3 = multi_epipolar_error<EST>(f, a3);
        if (e0 < thr) { cnt++; sum += e0; }
        if (e1 < thr) { cnt++; sum += e1; }
        if (e2 < thr) { cnt++; sum += e2; }
        if (e3 < thr) { cnt++; sum += e3; }
    }
    for (; p < n; p++) {
        const float e = multi_epipolar_error<EST>(f, pts[p]);
        if (e < thr) { cnt++; sum += e; }
    }
    if (i < K) {
        counts[slot] = cnt;
        sums[slot] = sum;
    }
}

// ------------------------------------------------------------------------ per-problem argmax
// One workgroup per active entry: the best of its S = spk * R slots under record_better (the
// strict total order of k_argmax_part / k_argmax_final: count, then Σ, then the earlier slot;
// count < 0 never wins), the record as k_argmax_final writes it (hyp_index = first_hyp + slot /
// spk).  With `running` the record is folded into the problem's running record by the order of
// usac_merge_records (valid, count, Σ, earlier hyp_index) and out[a] receives the merged record;
// without it out[a] is the round's record.
struct MultiBest {
    int c;
    float s;
    uint32_t i;
};

__global__ __launch_bounds__(256) void k_multi_argmax(const MultiItem *__restrict__ items,
                                                      const int32_t *__restrict__ counts,
                                                      const float *__restrict__ sums,
                                                      const float *__restrict__ models, uint32_t S, int ncomp,
                                                      uint64_t first_hyp, uint32_t spk,
                                                      usac_record *__restrict__ running,
                                                      usac_record *__restrict__ out) {
    __shared__ MultiBest sh[256];
    const uint32_t a = blockIdx.x, t = threadIdx.x;
    const size_t g0 = (size_t)a * S, stride = (size_t)gridDim.x * S;
    MultiBest b{-1, 0.f, 0xFFFFFFFFu};
    for (uint32_t i = t; i < S; i += 256) {
        const int c = counts[g0 + i];
        const float s = sums[g0 + i];
        if (c >= 0 && (b.c < 0 || record_better(c, s, i, b.c, b.s, b.i))) b = MultiBest{c, s, i};
    }
    sh[t] = b;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (t < w) {
            const MultiBest o = sh[t + w];
            if (o.c >= 0 && (sh[t].c < 0 || record_better(o.c, o.s, o.i, sh[t].c, sh[t].s, sh[t].i))) sh[t] = o;
        }
        __syncthreads();
    }
    if (t == 0) {
        const MultiBest best = sh[0];
        usac_record r;
        r.valid = best.c >= 0 ? 1 : 0;
        r.inliers = best.c < 0 ? 0 : best.c;
        r.score = best.s;
        r.hyp_index = first_hyp + (best.i == 0xFFFFFFFFu ? 0 : best.i / spk);
        for (int k = 0; k < 9; k++)
            r.model[k] = (k < ncomp && r.valid) ? models[(size_t)k * stride + g0 + best.i] : 0.f;
        if (running) {
            usac_record *cur = running + items[a].problem;
            const usac_record o = *cur;
            bool better;
            if (!r.valid) better = false;
            else if (!o.valid) better = true;
            else if (r.inliers != o.inliers) better = r.inliers > o.inliers;
            else if (r.score != o.score) better = r.score > o.score;
            else better = r.hyp_index < o.hyp_index;
            if (better) *cur = r;
            else r = o;
        }
        out[a] = r;
    }
}

// ------------------------------------------------------------------------ per-point masks
// models (P x 9 row-major) -> m18 (P x 18): the model, and for H its inverse by inv3x3
__global__ __launch_bounds__(256) void k_multi_mask_prep(const float *__restrict__ models, uint32_t P, int is_h,
                                                         float *__restrict__ m18) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float m[9], mi[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = models[9 * (size_t)p + k];
    if (is_h) inv3x3(m, mi);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        m18[18 * (size_t)p + k] = m[k];
        m18[18 * (size_t)p + 9 + k] = is_h ? mi[k] : 0.f;
    }
}

// one thread per point of the concatenated array: its problem by bisection of offsets, the
// residual of usac_get_inliers under that problem's model (H, F or E), mask = err < thr (thrs given:
// that problem's, per thread -- the lanes of a wave may straddle a boundary).  PT: per-problem thresholds, a
// template parameter so that the instantiation without them is the kernel it was before they existed
template <bool PT>
__global__ __launch_bounds__(256) void k_multi_mask(const float4 *__restrict__ pts_all,
                                                    const uint32_t *__restrict__ offsets, uint32_t P,
                                                    uint32_t n_total, const float *__restrict__ m18, int est,
                                                    float thr_s, uint8_t *__restrict__ mask,
                                                    const float *__restrict__ thrs) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    uint32_t lo = 0, hi = P;  // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    float m[18];
#pragma unroll
    for (int k = 0; k < 18; k++) m[k] = m18[18 * (size_t)lo + k];
    const float4 p = pts_all[i];
    const float err = est == USAC_HOMOGRAPHY    ? homography_error(m, m + 9, p.x, p.y, p.z, p.w)
                      : est == USAC_FUNDAMENTAL ? fundamental_error(m, p.x, p.y, p.z, p.w)
                                                : essential_error(m, p.x, p.y, p.z, p.w);
    const float thr = PT ? thrs[lo] : thr_s;
    mask[i] = err < thr ? 1 : 0;
}

// ------------------------------------------------------------------------ launchers
hipError_t launch_multi_round(hipStream_t st, const MultiRound &r) {
    if (r.A == 0 || r.R == 0 || r.R % 64 || (r.growth && r.grid)) return hipErrorInvalidValue;
    const dim3 grid(r.R / 64, r.A);
    if (r.estimator == USAC_HOMOGRAPHY) {
        if (r.grid) {
            auto *solve = r.nullspace ? k_multi_solve_h4<true, kNapsac> : k_multi_solve_h4<false, kNapsac>;
            hipLaunchKernelGGL(solve, grid, dim3(64), 0, st, r.pts, r.offsets, r.items, r.samples_in, r.R, r.first_hyp,
                               r.models, *r.grid);
        } else {
            auto *solve = r.growth ? (r.nullspace ? k_multi_solve_h4<true, kProsac> : k_multi_solve_h4<false, kProsac>)
                                   : (r.nullspace ? k_multi_solve_h4<true, kUniform> : k_multi_solve_h4<false, kUniform>);
            hipLaunchKernelGGL(solve, grid, dim3(64), 0, st, r.pts, r.offsets, r.items, r.samples_in, r.R, r.first_hyp,
                               r.models, r.growth);
        }
        if (r.sprt) {
            const hipError_t e = launch_multi_sprt_score(st, r);
            if (e != hipSuccess) return e;
        } else {
            hipLaunchKernelGGL(k_multi_score_h, grid, dim3(64), 0, st, r.pts, r.offsets, r.items, r.models, r.R, r.thr,
                               r.thrs, r.counts, r.sums);
        }
        hipLaunchKernelGGL(k_multi_argmax, dim3(r.A), dim3(256), 0, st, r.items, r.counts, r.sums, r.models, r.R, 9,
                           r.first_hyp, 1u, r.running, r.out);
    } else if (r.estimator == USAC_FUNDAMENTAL) {
        hipError_t e = hipMemsetAsync(r.list_n, 0, sizeof(uint32_t) * r.A, st);
        if (e != hipSuccess) return e;
        if (r.grid) {
            hipLaunchKernelGGL(k_multi_solve_f7<kNapsac>, grid, dim3(64), 0, st, r.pts, r.offsets, r.items, r.samples_in,
                               r.R, r.first_hyp, r.models, r.counts, r.sums, r.list, r.list_n, *r.grid);
        } else {
            auto *solve = r.growth ? k_multi_solve_f7<kProsac> : k_multi_solve_f7<kUniform>;
            hipLaunchKernelGGL(solve, grid, dim3(64), 0, st, r.pts, r.offsets, r.items, r.samples_in, r.R, r.first_hyp,
                               r.models, r.counts, r.sums, r.list, r.list_n, r.growth);
        }
        if (r.sprt) {
            e = launch_multi_sprt_score(st, r);
            if (e != hipSuccess) return e;
        } else {
            hipLaunchKernelGGL(k_multi_score_f<USAC_FUNDAMENTAL>, dim3(3 * r.R / 64, r.A), dim3(64), 0, st, r.pts, r.offsets, r.items,
                               r.models, r.R, r.list, r.list_n, r.thr, r.thrs, r.counts, r.sums);
        }
        hipLaunchKernelGGL(k_multi_argmax, dim3(r.A), dim3(256), 0, st, r.items, r.counts, r.sums, r.models, 3 * r.R,
                           9, r.first_hyp, 3u, r.running, r.out);
    } else if (r.estimator == USAC_ESSENTIAL) {  // one slot per sample; no SPRT, no NAPSAC
        if (r.sprt || r.grid) return hipErrorInvalidValue;
        const hipError_t e = launch_multi_solve_e5(st, r);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_multi_score_f<USAC_ESSENTIAL>, grid, dim3(64), 0, st, r.pts, r.offsets, r.items, r.models,
                           r.R, r.list, r.list_n, r.thr, r.thrs, r.counts, r.sums);
        hipLaunchKernelGGL(k_multi_argmax, dim3(r.A), dim3(256), 0, st, r.items, r.counts, r.sums, r.models, r.R, 9,
                           r.first_hyp, 1u, r.running, r.out);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the samples alone: grid (R / 64, A), lane h of entry a writes its m indices
template <int M, int SAMPLER>
__global__ __launch_bounds__(64) void k_multi_draw(const uint32_t *__restrict__ offsets,
                                                   const MultiItem *__restrict__ items, uint32_t R,
                                                   uint64_t first_hyp, const typename SamplerArg<SAMPLER>::type aux,
                                                   int32_t *__restrict__ out) {
    const uint32_t a = blockIdx.y;
    const MultiItem it = items[a];
    const uint32_t base = offsets[it.problem], n = offsets[it.problem + 1] - base;
    const uint32_t h = blockIdx.x * 64 + threadIdx.x;
    int32_t s[M];
    multi_sample<M, SAMPLER>(it, aux, base, n, first_hyp + h, h, s);
    int32_t *__restrict__ o = out + ((size_t)a * R + h) * M;
#pragma unroll
    for (int i = 0; i < M; i++) o[i] = s[i];
}

hipError_t launch_multi_draw(hipStream_t st, int estimator, const uint32_t *offsets, const MultiItem *items, uint32_t A,
                             uint32_t R, uint64_t first_hyp, const uint32_t *growth, const MultiGrid *mg, int32_t *out) {
    if (A == 0 || R == 0 || R % 64 || (growth && mg)) return hipErrorInvalidValue;
    const dim3 grid(R / 64, A);
    if (estimator != USAC_HOMOGRAPHY && estimator != USAC_FUNDAMENTAL && estimator != USAC_ESSENTIAL)
        return hipErrorInvalidValue;
    if (mg) {
        if (estimator == USAC_ESSENTIAL) return hipErrorInvalidValue;
        auto *draw = estimator == USAC_HOMOGRAPHY ? k_multi_draw<4, kNapsac> : k_multi_draw<7, kNapsac>;
        hipLaunchKernelGGL(draw, grid, dim3(64), 0, st, offsets, items, R, first_hyp, *mg, out);
        return hipGetLastError();
    }
    auto *draw4 = growth ? k_multi_draw<4, kProsac> : k_multi_draw<4, kUniform>;
    auto *draw5 = growth ? k_multi_draw<5, kProsac> : k_multi_draw<5, kUniform>;
    auto *draw7 = growth ? k_multi_draw<7, kProsac> : k_multi_draw<7, kUniform>;
    hipLaunchKernelGGL(estimator == USAC_HOMOGRAPHY ? draw4 : estimator == USAC_ESSENTIAL ? draw5 : draw7, grid, dim3(64),
                       0, st, offsets, items, R, first_hyp, growth, out);
    return hipGetLastError();
}

hipError_t launch_multi_mask(hipStream_t st, int estimator, const float4 *pts, const uint32_t *offsets, uint32_t P,
                             uint32_t n_total, const float *models, float thr, const float *thrs, float *m18,
                             uint8_t *mask) {
    const int is_h = estimator == USAC_HOMOGRAPHY;
    hipLaunchKernelGGL(k_multi_mask_prep, dim3((P + 255) / 256), dim3(256), 0, st, models, P, is_h, m18);
    hipLaunchKernelGGL(thrs ? k_multi_mask<true> : k_multi_mask<false>, dim3((n_total + 255) / 256), dim3(256), 0, st, pts,
                       offsets, P, n_total, m18, estimator, thr, mask, thrs);
    return hipGetLastError();
}

}  // namespace usac
