// Pose refinement of a multi context's essential batches (ABI 29, usac_multi_refine_pose_device /
// usac_multi_refine_pose): for every problem a pose (R, t) refined by Levenberg-Marquardt steps on its five
// parameters over the Sampson distances of its masked rows, by the rule include/usac_gpu.h states under "Pose
// refinement (ABI 29)".  fp64 under -ffp-contract=off, division and square root correctly rounded, no other
// library function: tests/helpers/multi_refine_ref.py runs the same operations in numpy and the outputs agree bit
// for bit.
//
// One launch, one 256-thread workgroup per problem, any n_p (DESIGN.md §8b "Pose refinement").  The whole loop
// runs in the kernel.  Thread 0 owns the serial part -- the 5 x 5 solve, the trial pose, its frame (E and the five
// derivative matrices) -- and keeps all of it in LDS, so that it costs the other 255 threads no registers; behind
// a barrier every thread copies the trial frame into registers and runs the pass over its rows i = T, T + 256,
// ...: 21 fp64 accumulators, the xor butterfly over the wave, four wave totals per sum through LDS.  Behind the
// second barrier thread 0 combines them as (w0 + w1) + (w2 + w3), accepts or rejects, and solves until there is a
// new trial pose or the loop has ended.  Every branch that decides whether a barrier is reached reads LDS (go,
// skip), so it is uniform over the workgroup.  The rows are read again from L2 in every pass.
#include <hip/hip_runtime.h>

#include "usac_kernels.h"

namespace usac {

namespace {

constexpr int kSums = 21;  // H's upper triangle row by row (15), g (5), c

struct RefineShared {
    // the current pose, its frame and its sums
    double R[9], t[3], b1[3], b2[3], E[9], sums[kSums], lambda, cost0;
    // the trial pose and its frame: what the pass reads
    double tR[9], tt[3], tb1[3], tb2[3], tE[9], tD[5][9];
    double wave[4][kSums];
    // thread 0's work space: G = [e_j]x R, the Cholesky factor, the two solves
    double G[9], L[5][5], y[5], d[5];
    uint32_t count[4];
    int go, first, iterations, skip;
};

__device__ __forceinline__ bool refine_finite(float v) { return fabsf(v) < INFINITY; }

__device__ __forceinline__ bool refine_row_finite(const float4 &r) {
    return refine_finite(r.x) && refine_finite(r.y) && refine_finite(r.z) && refine_finite(r.w);
}

// H_jk of the 15 sums, j <= k
__device__ __forceinline__ int tri(int j, int k) { return j * 5 - (j * (j - 1)) / 2 + (k - j); }

__device__ void unit3(const double *v, double *out) {
    const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    out[0] = v[0] / n;
    out[1] = v[1] / n;
    out[2] = v[2] / n;
}

// out = [v]x M: column c is v x (column c of M)
__device__ void skew_times(const double *v, const double *M, double *out) {
    for (int c = 0; c < 3; c++) {
        out[c] = v[1] * M[6 + c] - v[2] * M[3 + c];
        out[3 + c] = v[2] * M[c] - v[0] * M[6 + c];
        out[6 + c] = v[0] * M[3 + c] - v[1] * M[c];
    }
}

// out = [e_j]x M, exactly
__device__ void unit_skew_times(int j, const double *M, double *out) {
    for (int c = 0; c < 3; c++) {
        const double m0 = M[c], m1 = M[3 + c], m2 = M[6 + c];
        out[c] = j == 0 ? 0.0 : j == 1 ? m2 : -m1;
        out[3 + c] = j == 0 ? -m2 : j == 1 ? 0.0 : m0;
        out[6 + c] = j == 0 ? m1 : j == 1 ? -m0 : 0.0;
    }
}

// the frame at the trial pose (tR, tt): tb1, tb2, tE, tD
__device__ void trial_frame(RefineShared &s) {
    const double *t = s.tt;
    int k = 0;
    if (fabs(t[1]) < fabs(t[k])) k = 1;
    if (fabs(t[2]) < fabs(t[k])) k = 2;
    double c[3];  // t x e_k
    c[0] = k == 0 ? 0.0 : k == 1 ? -t[2] : t[1];
    c[1] = k == 0 ? t[2] : k == 1 ? 0.0 : -t[0];
    c[2] = k == 0 ? -t[1] : k == 1 ? t[0] : 0.0;
    unit3(c, s.tb1);
    s.tb2[0] = t[1] * s.tb1[2] - t[2] * s.tb1[1];
    s.tb2[1] = t[2] * s.tb1[0] - t[0] * s.tb1[2];
    s.tb2[2] = t[0] * s.tb1[1] - t[1] * s.tb1[0];
    skew_times(t, s.tR, s.tE);
    for (int j = 0; j < 3; j++) {
        unit_skew_times(j, s.tR, s.G);
        skew_times(t, s.G, s.tD[j]);
    }
    skew_times(s.tb1, s.tR, s.tD[3]);
    skew_times(s.tb2, s.tR, s.tD[4]);
}

// (H + lambda diag H) d = -g by Cholesky, lower triangle, columns in order; false: a pivot is not > 0
__device__ bool refine_solve(RefineShared &s) {
    const double *H = s.sums, *g = s.sums + 15;
    for (int j = 0; j < 5; j++) {
        double p = H[tri(j, j)] + s.lambda * H[tri(j, j)];
        for (int k = 0; k < j; k++) p = p - s.L[j][k] * s.L[j][k];
        if (!(p > 0)) return false;
        s.L[j][j] = sqrt(p);
        for (int i = j + 1; i < 5; i++) {
            double q = H[tri(j, i)];
            for (int k = 0; k < j; k++) q = q - s.L[i][k] * s.L[j][k];
            s.L[i][j] = q / s.L[j][j];
        }
    }
    for (int i = 0; i < 5; i++) {
        double q = -g[i];
        for (int k = 0; k < i; k++) q = q - s.L[i][k] * s.y[k];
        s.y[i] = q / s.L[i][i];
    }
    for (int i = 4; i >= 0; i--) {
        double q = s.y[i];
        for (int k = i + 1; k < 5; k++) q = q - s.L[k][i] * s.d[k];
        s.d[i] = q / s.L[i][i];
    }
    return true;
}

// the trial pose from the current one and the step d: tR = Q(d0, d1, d2) R, tt = unit(t + d3 b1 + d4 b2)
__device__ void refine_update(RefineShared &s) {
    const double qx = s.d[0] * 0.5, qy = s.d[1] * 0.5, qz = s.d[2] * 0.5;
    const double w = 1.0 / sqrt(((1.0 + qx * qx) + qy * qy) + qz * qz);
    const double x = qx * w, y = qy * w, z = qz * w;
    double Q[9];
    Q[0] = 1.0 - 2.0 * (y * y + z * z);
    Q[1] = 2.0 * (x * y - w * z);
    Q[2] = 2.0 * (x * z + w * y);
    Q[3] = 2.0 * (x * y + w * z);
    Q[4] = 1.0 - 2.0 * (x * x + z * z);
    Q[5] = 2.0 * (y * z - w * x);
    Q[6] = 2.0 * (x * z - w * y);
    Q[7] = 2.0 * (y * z + w * x);
    Q[8] = 1.0 - 2.0 * (x * x + y * y);
#pragma unroll
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            s.tR[3 * r + c] = (Q[3 * r] * s.R[c] + Q[3 * r + 1] * s.R[3 + c]) + Q[3 * r + 2] * s.R[6 + c];
    double u[3];
    for (int k = 0; k < 3; k++) u[k] = (s.t[k] + s.d[3] * s.b1[k]) + s.d[4] * s.b2[k];
    unit3(u, s.tt);
}

// the trial pose, its frame and its sums become the current ones
__device__ void refine_take(RefineShared &s, const double *sums) {
    for (int k = 0; k < 9; k++) {
        s.R[k] = s.tR[k];
        s.E[k] = s.tE[k];
    }
    for (int k = 0; k < 3; k++) {
        s.t[k] = s.tt[k];
        s.b1[k] = s.tb1[k];
        s.b2[k] = s.tb2[k];
    }
    for (int k = 0; k < kSums; k++) s.sums[k] = sums[k];
}

// Solves until a trial pose stands in LDS (go = 1) or the loop has ended (go = 0)
__device__ void refine_next(RefineShared &s, uint32_t max_iters) {
    s.go = 0;
    while ((uint32_t)s.iterations < max_iters) {
        if (refine_solve(s)) {
            refine_update(s);
            trial_frame(s);
            s.go = 1;
            return;
        }
        s.lambda = 10.0 * s.lambda;  // a pivot that is not > 0: a rejected trial without a pass
        if (s.lambda > 1e8) return;
    }
}

// M x1 (three entries) and the first two entries of M^T x2
#define REFINE_MV(M, u0, u1, u2, v0, v1)                      \
    const double u0 = (M[0] * x1 + M[1] * y1) + M[2];        \
    const double u1 = (M[3] * x1 + M[4] * y1) + M[5];        \
    const double u2 = (M[6] * x1 + M[7] * y1) + M[8];        \
    const double v0 = (M[0] * x2 + M[3] * y2) + M[6];        \
    const double v1 = (M[1] * x2 + M[4] * y2) + M[7];

}  // namespace

// IDENT: packed row i of a problem is column i of its row of a padded mask (no source columns)
template <bool IDENT>
__global__ __launch_bounds__(256) void k_multi_refine(MultiRefine a) {
    __shared__ RefineShared s;
    const uint32_t p = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t base = a.offsets[p], n = a.offsets[p + 1] - base;
    const uint8_t *mrow = !a.mask ? nullptr : a.mask_packed ? a.mask + base : a.mask + (size_t)p * a.n_max;

    // whether packed row i is used: its mask byte is set and its four values are finite
    auto row_used = [&](uint32_t i, float4 &r) -> bool {
        if (mrow) {
            const uint32_t col = (a.mask_packed || IDENT) ? i : a.src[(size_t)base + i];
            if (!(a.mask_packed || IDENT) && col >= a.n_max) return false;
            if (mrow[col] == 0) return false;
        }
        r = a.pts[(size_t)base + i];
        return refine_row_finite(r);
    };

    // the start, read before anything is written (R_in / t_in may be R / t), and the number of used rows
    float R0[9], t0[3];
    if (threadIdx.x == 0) {
        for (int k = 0; k < 9; k++) R0[k] = a.R_in[9 * (size_t)p + k];
        for (int k = 0; k < 3; k++) t0[k] = a.t_in[3 * (size_t)p + k];
    }
    uint32_t cnt = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        float4 r;
        cnt += row_used(i, r) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) s.count[wave] = cnt;
    __syncthreads();
    const uint32_t used = (s.count[0] + s.count[1]) + (s.count[2] + s.count[3]);
    if (threadIdx.x == 0) {
        const int32_t status = a.pol ? a.pol[p].status : (int32_t)USAC_OK;
        bool finite = true, zero = true;
        for (int k = 0; k < 9; k++) finite = finite && refine_finite(R0[k]);
        for (int k = 0; k < 3; k++) {
            finite = finite && refine_finite(t0[k]);
            zero = zero && t0[k] == 0.0f;
        }
        const bool skip = status != (int32_t)USAC_OK || !finite || zero || used < 5;
        s.skip = skip ? 1 : 0;
        s.go = skip ? 0 : 1;
        s.first = 1;
        s.iterations = 0;
        s.lambda = 1e-3;
        if (skip) {  // the inputs' bits, E zero, costs 0, iterations -1
            if (a.R)
                for (int k = 0; k < 9; k++) a.R[9 * (size_t)p + k] = R0[k];
            if (a.t)
                for (int k = 0; k < 3; k++) a.t[3 * (size_t)p + k] = t0[k];
            if (a.E)
                for (int k = 0; k < 9; k++) a.E[9 * (size_t)p + k] = 0.0f;
            if (a.cost0) a.cost0[p] = 0.0;
            if (a.cost) a.cost[p] = 0.0;
            if (a.iterations) a.iterations[p] = -1;
            if (a.used) a.used[p] = (int32_t)used;
        } else {  // the first pass runs at the normalised start
            double tw[3];
            for (int k = 0; k < 9; k++) s.tR[k] = (double)R0[k];
            for (int k = 0; k < 3; k++) tw[k] = (double)t0[k];
            unit3(tw, s.tt);
            trial_frame(s);
        }
    }
    for (;;) {
        __syncthreads();  // thread 0's trial frame, go and skip are visible
        if (!s.go) break;
        double E[9], D[5][9];
#pragma unroll
        for (int k = 0; k < 9; k++) E[k] = s.tE[k];
#pragma unroll
        for (int j = 0; j < 5; j++)
#pragma unroll
            for (int k = 0; k < 9; k++) D[j][k] = s.tD[j][k];
        double acc[kSums];
#pragma unroll
        for (int k = 0; k < kSums; k++) acc[k] = 0.0;
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            float4 row;
            if (!row_used(i, row)) continue;
            const double x1 = (double)row.x, y1 = (double)row.y, x2 = (double)row.z, y2 = (double)row.w;
            REFINE_MV(E, a0, a1, a2, b0, b1)
            const double C = (x2 * a0 + y2 * a1) + a2;
            const double S = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
            if (!(S > 0)) continue;
            const double sq = sqrt(S), r = C / sq;
            double J[5];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                REFINE_MV(D[j], u0, u1, u2, v0, v1)
                const double num = (x2 * u0 + y2 * u1) + u2;
                const double q = ((a0 * u0 + a1 * u1) + b0 * v0) + b1 * v1;
                J[j] = num / sq - (r * q) / S;
            }
            int at = 0;
#pragma unroll
            for (int j = 0; j < 5; j++)
#pragma unroll
                for (int k = j; k < 5; k++) {
                    acc[at] = acc[at] + J[j] * J[k];
                    at++;
                }
#pragma unroll
            for (int j = 0; j < 5; j++) acc[15 + j] = acc[15 + j] + J[j] * r;
            acc[20] = acc[20] + r * r;
        }
#pragma unroll
        for (int k = 0; k < kSums; k++) {
            for (int o = 32; o > 0; o >>= 1) acc[k] = acc[k] + __shfl_xor(acc[k], o, 64);
            if (lane == 0) s.wave[wave][k] = acc[k];
        }
        __syncthreads();  // every wave's totals are in LDS; every thread has read the trial frame and go
        if (threadIdx.x == 0) {
            double sums[kSums];
#pragma unroll
            for (int k = 0; k < kSums; k++) sums[k] = (s.wave[0][k] + s.wave[1][k]) + (s.wave[2][k] + s.wave[3][k]);
            const double c_new = sums[20];
            bool stop = false;
            if (s.first) {
                s.first = 0;
                s.cost0 = c_new;
                refine_take(s, sums);
            } else {
                s.iterations += 1;
                const double c_old = s.sums[20];
                if (c_new < c_old) {  // accept; a NaN rejects
                    refine_take(s, sums);
                    const double tenth = s.lambda / 10.0;
                    s.lambda = tenth > 1e-12 ? tenth : 1e-12;
                    double dmax = 0.0;
                    for (int k = 0; k < 5; k++) dmax = fabs(s.d[k]) > dmax ? fabs(s.d[k]) : dmax;
                    stop = c_old - c_new <= 1e-12 * c_old || dmax < 1e-10;
                } else {
                    s.lambda = 10.0 * s.lambda;
                    stop = s.lambda > 1e8;
                }
            }
            if (stop) s.go = 0;
            else refine_next(s, a.max_iters);
        }
    }
    if (threadIdx.x == 0 && !s.skip) {
        if (a.R)
            for (int k = 0; k < 9; k++) a.R[9 * (size_t)p + k] = (float)s.R[k];
        if (a.t)
            for (int k = 0; k < 3; k++) a.t[3 * (size_t)p + k] = (float)s.t[k];
        if (a.E)
            for (int k = 0; k < 9; k++) a.E[9 * (size_t)p + k] = (float)s.E[k];
        if (a.cost0) a.cost0[p] = s.cost0;
        if (a.cost) a.cost[p] = s.sums[20];
        if (a.iterations) a.iterations[p] = s.iterations;
        if (a.used) a.used[p] = (int32_t)used;
    }
}

#undef REFINE_MV

hipError_t launch_multi_refine(hipStream_t st, const MultiRefine &a) {
    if (a.P == 0 || a.P > kMultiMaxActive || !a.R_in || !a.t_in || !refine_iters_ok(a.max_iters) ||
        (a.mask && !a.mask_packed && a.n_max == 0) || (a.mask_packed && a.src))
        return hipErrorInvalidValue;
    if (a.src) hipLaunchKernelGGL(k_multi_refine<false>, dim3(a.P), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_multi_refine<true>, dim3(a.P), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace usac
