// Relative pose of a multi context's essential matrices (ABI 28, usac_multi_pose_device / usac_multi_pose): for
// every problem the one of the four [R | t] of its model E that puts the most of its masked rows in front of both
// cameras, by the rule include/usac_gpu.h states under "Pose (ABI 28)".
//
// The arithmetic is the 5-point solver's cheirality test, usac_device_e5.hpp as it is: e5::svd3 and e5::projection
// (ProjectionsFromEssential), e5::in_front (TriangulatePoint as the rank-3 null vector on the first ray, and
// CalcDepth), fp64 under -ffp-contract=off.  k_e5_check runs it over the five points of a minimal sample; here it
// runs over a model's inlier set.
//
// One launch, one 256-thread workgroup per problem, any n_p (DESIGN.md §8b "Pose").  Thread 0 decomposes E and
// leaves the four projections in LDS (4 x 12 doubles); behind a barrier every thread holds them in registers.
// Pass 1 strides over the rows: four integer counters per thread, summed over the wave, four wave totals per
// candidate through LDS, and every thread derives the same choice -- integers only, so the result does not depend
// on the order of anything.  Pass 2 evaluates in_front under the chosen projection alone and sets the bytes of
// front_mask, whose row the workgroup cleared itself before the first barrier (k_multi_export's scheme: no memset
// and no second launch).
#include <hip/hip_runtime.h>

#include "usac_device_e5.hpp"
#include "usac_kernels.h"

namespace usac {

namespace {

// row[0 .. n) = 0 by all 256 threads: single bytes up to the first 16-byte boundary, 16-byte stores, a tail of
// single bytes (k_multi_export's export_fill for bytes)
__device__ __forceinline__ void pose_clear(uint8_t *row, uint32_t n) {
    uint32_t head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u;
    if (head > n) head = n;
    const uint32_t wide = (n - head) / 16u, tail0 = head + wide * 16u;  // n - tail0 < 16
    if (threadIdx.x < head) row[threadIdx.x] = 0;
    uint4 *q = reinterpret_cast<uint4 *>(row + head);
    for (uint32_t i = threadIdx.x; i < wide; i += 256) q[i] = make_uint4(0u, 0u, 0u, 0u);
    if (threadIdx.x < n - tail0) row[tail0 + threadIdx.x] = 0;
}

// A row with a non-finite value is in front of nothing (the rule, step 2).  The comparisons of in_front alone do
// not say so: with a non-finite x2 and a finite y2, n0 is NaN, `n0 >= n1` is false and the point is triangulated
// from the row of y2 as if x2 were not there.
__device__ __forceinline__ bool pose_row_finite(const float4 &r) {
    return fabsf(r.x) < INFINITY && fabsf(r.y) < INFINITY && fabsf(r.z) < INFINITY && fabsf(r.w) < INFINITY;
}

}  // namespace

// IDENT: packed row i of a problem is column i of its front_mask row (no source columns, or the packed layout)
template <bool IDENT>
__global__ __launch_bounds__(256) void k_multi_pose(MultiPose a) {
    __shared__ double sh_P[4][3][4];
    __shared__ uint32_t sh_c[4][4];  // [wave][candidate]
    const uint32_t p = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t base = a.offsets[p], n = a.offsets[p + 1] - base;
    const float *model = a.pol ? a.pol[p].model : a.models + 9 * (size_t)p;
    const int32_t status = a.pol ? a.pol[p].status : (int32_t)USAC_OK;
    // the problem's row of front_mask: n bytes at its packed rows, or n_max bytes of the padded layout
    uint8_t *mrow = !a.front_mask ? nullptr : a.packed ? a.front_mask + base : a.front_mask + (size_t)p * a.n_max;
    if (mrow) pose_clear(mrow, a.packed ? n : a.n_max);
    if (threadIdx.x == 0) {
        double E[9], U[3][3], V[3][3];
        for (int k = 0; k < 9; k++) E[k] = (double)model[k];
        e5::svd3(E, U, V);
        for (int j = 0; j < 4; j++) {
            double Pj[3][4];
            e5::projection(U, V, j, Pj);
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 4; c++) sh_P[j][r][c] = Pj[r][c];
        }
    }
    // the projections, and the cleared row, are visible to the whole workgroup
    __syncthreads();
    double P[4][3][4];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) P[j][r][c] = sh_P[j][r][c];
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        if (a.mask && a.mask[(size_t)base + i] == 0) continue;
        const float4 r = a.pts[(size_t)base + i];
        if (!pose_row_finite(r)) continue;
        const double x1 = (double)r.x, y1 = (double)r.y, x2 = (double)r.z, y2 = (double)r.w;
#pragma unroll
        for (int j = 0; j < 4; j++) cnt[j] += e5::in_front(x1, y1, x2, y2, P[j]) ? 1u : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        for (int o = 32; o > 0; o >>= 1) cnt[j] += __shfl_xor(cnt[j], o, 64);
        if (lane == 0) sh_c[wave][j] = cnt[j];
    }
    __syncthreads();
    int choice = -1;
    uint32_t best = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t t = (sh_c[0][j] + sh_c[1][j]) + (sh_c[2][j] + sh_c[3][j]);
        if (t > best) {  // the largest count, the lowest j on ties; a count of 0 chooses nothing
            best = t;
            choice = j;
        }
    }
    if (status != (int32_t)USAC_OK) {
        choice = -1;
        best = 0;
    }
    // the chosen projection by value (no dynamic register indexing)
    double Pc[3][4];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++)
            Pc[r][c] = choice == 0 ? P[0][r][c] : choice == 1 ? P[1][r][c] : choice == 2 ? P[2][r][c] : P[3][r][c];
    if (threadIdx.x == 0) {
        // P and -P are one camera; the output is the one of the two whose 3x3 block is a rotation.  The sorted
        // SVD gives det U = -1 when the sort is an odd permutation, and CalcDepth's own sign made up for it
        const double sgn = e5::det3p(Pc) > 0 ? 1.0 : -1.0;
        if (a.R)
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++)
                    a.R[9 * (size_t)p + 3 * r + c] = choice < 0 ? (r == c ? 1.0f : 0.0f) : (float)(sgn * Pc[r][c]);
        if (a.t)
            for (int r = 0; r < 3; r++) a.t[3 * (size_t)p + r] = choice < 0 ? 0.0f : (float)(sgn * Pc[r][3]);
        if (a.front) a.front[p] = (int32_t)best;
        if (a.choice) a.choice[p] = choice;
    }
    if (!mrow || choice < 0) return;  // uniform over the workgroup; the row is cleared
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        if (a.mask && a.mask[(size_t)base + i] == 0) continue;
        const float4 r = a.pts[(size_t)base + i];
        if (!pose_row_finite(r)) continue;
        if (!e5::in_front((double)r.x, (double)r.y, (double)r.z, (double)r.w, Pc)) continue;
        const uint32_t col = IDENT ? i : a.src[(size_t)base + i];
        if (IDENT || col < a.n_max) mrow[col] = 1;
    }
}

hipError_t launch_multi_pose(hipStream_t st, const MultiPose &a) {
    if (a.P == 0 || a.P > kMultiMaxActive || (a.pol == nullptr) == (a.models == nullptr) ||
        (a.front_mask && !a.packed && a.n_max == 0) || (a.packed && a.src))
        return hipErrorInvalidValue;
    if (a.src) hipLaunchKernelGGL(k_multi_pose<false>, dim3(a.P), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_multi_pose<true>, dim3(a.P), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace usac
