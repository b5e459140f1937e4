// kernels_multi_grid.hip -- grid neighbours of every problem of a multi-problem batch in one launch
// (DESIGN.md §8b "NAPSAC"): one workgroup per problem writes the CSR of usac::GridNeighbors(pts_p,
// n_p, cell_size) (usac_host.hpp) -- cell = ((int)(x1/cs), (int)(y1/cs), (int)(x2/cs), (int)(y2/cs))
// with fp32 division and truncation, cells numbered in order of first appearance, members ascending
// within a cell -- and the NAPSAC-eligible points (>= m neighbours, ascending), problem-local at the
// points' offsets:
//   cell / rank / members / eligible : N_total each, problem p's n_p values at offsets[p];
//   start                            : N_total + P, problem p's n_cells + 1 entries at offsets[p] + p;
//   n_cells / n_eligible / status    : P each.
//
// n_p is about 10^3, so there is no hash table and no atomic: the problem's cell indices sit in LDS,
// and each thread takes points i = t, t + T, ... and walks j = 0 .. n_p - 1 over them (all lanes read
// the same j: a broadcast read), which gives the point's first equal-key index, its rank (equal keys
// with j < i) and its cell's size.  A block scan over the points in index order with three counters
// (heads, the heads' cell sizes, eligible points; wave_scan3 of kernels_grid.hip) turns a head into
// its first-appearance cell number and the cell's start, and lists the eligible points; then
// members[start + rank] = i.  The result does not depend on the schedule.
//
// Past the caps (the polish's rule): a problem of more than kMultiGridMax points, or with a coordinate
// for which !(|x| / cs < 1e9f) (non-finite values included: the int cell index itself is out of
// range, ensure_grid's test), writes status = kMultiGridDefer and nothing else; the host builds it.
// The decision is workgroup-uniform.
//
// LDS (-Rpass-analysis=kernel-resource-usage): 80 304 B per workgroup -- kMultiGridMax = 4000 points x
// (16 B of cell indices + one packed (first, size) word), the scan's partials -- above the 64 KiB of
// gfx90a / gfx942 and within gfx950's 160 KiB; two workgroups share a CU (occupancy 2, 49 VGPRs, no
// scratch).  This build targets gfx950 only (ransac_amd/Makefile ARCH); the bound is checked below.
#include <hip/hip_runtime.h>

#include "usac_kernels.h"

namespace usac {

namespace {

constexpr uint32_t kT = 256;  // threads per problem
constexpr uint32_t kBlk = 4;  // points a thread carries through one walk
static_assert(kMultiGridMax <= 0xffffu, "first, size, cell number and start are packed into 16 bits each");
static_assert(kMultiGridMax * (sizeof(int4) + sizeof(uint32_t)) + 3 * 4 * sizeof(uint32_t) <= 160 * 1024,
              "k_multi_grid's LDS exceeds gfx950's 160 KiB per workgroup");

// wave-inclusive scan of three counters (64 lanes), as kernels_grid.hip's
__device__ __forceinline__ void wave_scan3(uint32_t &a, uint32_t &b, uint32_t &c) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ta = __shfl_up(a, d), tb = __shfl_up(b, d), tc = __shfl_up(c, d);
        if (lane >= d) {
            a += ta;
            b += tb;
            c += tc;
        }
    }
}

__device__ __forceinline__ bool same_cell(const int4 &a, const int4 &b) {
    return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}

}  // namespace

__global__ __launch_bounds__(256) void k_multi_grid(const float4 *__restrict__ pts_all,
                                                    const uint32_t *__restrict__ offsets, float cs, uint32_t m,
                                                    MultiGrid g) {
    __shared__ int4 key[kMultiGridMax];      // after the walk: (cell number << 16 | start) of a head, as uint32
    __shared__ uint32_t fs[kMultiGridMax];   // first equal-key index << 16 | cell size
    __shared__ uint32_t red[3][4];
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const uint32_t base = offsets[p], n = offsets[p + 1] - base;
    if (n > kMultiGridMax) {  // block-uniform
        if (t == 0) g.status[p] = kMultiGridDefer;
        return;
    }
    const float4 *__restrict__ pts = pts_all + base;
    int bad = 0;
    for (uint32_t i = t; i < n; i += kT) {
        const float4 q = pts[i];
        const float v[4] = {q.x, q.y, q.z, q.w};
        int c[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            bad |= !(fabsf(v[j]) / cs < 1.0e9f);
            c[j] = (int)(v[j] / cs);  // IEEE fp32 division, truncation (as the reference)
        }
        key[i] = make_int4(c[0], c[1], c[2], c[3]);
    }
    if (__syncthreads_or(bad)) {  // block-uniform
        if (t == 0) g.status[p] = kMultiGridDefer;
        return;
    }
    uint32_t *__restrict__ rank = g.rank + base;
    // the walk: kBlk points per thread and pass
    for (uint32_t i0 = t; i0 < n; i0 += kBlk * kT) {
        int4 k[kBlk];
        uint32_t first[kBlk], rk[kBlk], sz[kBlk];
#pragma unroll
        for (uint32_t b = 0; b < kBlk; b++) {
            const uint32_t i = i0 + b * kT;
            k[b] = key[i < n ? i : i0];
            first[b] = 0xffffffffu;
            rk[b] = sz[b] = 0;
        }
        for (uint32_t j = 0; j < n; j++) {
            const int4 kj = key[j];
#pragma unroll
            for (uint32_t b = 0; b < kBlk; b++) {
                const bool eq = same_cell(kj, k[b]);
                first[b] = eq && first[b] == 0xffffffffu ? j : first[b];
                rk[b] += eq && j < i0 + b * kT;
                sz[b] += eq;
            }
        }
#pragma unroll
        for (uint32_t b = 0; b < kBlk; b++) {
            const uint32_t i = i0 + b * kT;
            if (i < n) {
                fs[i] = first[b] << 16 | sz[b];
                rank[i] = rk[b];
            }
        }
    }
    __syncthreads();  // the keys are read no more: their memory takes the heads' (cell number, start)
    uint32_t *__restrict__ hq = reinterpret_cast<uint32_t *>(key);
    uint32_t *__restrict__ start = g.start + base + p;
    int32_t *__restrict__ eligible = g.eligible + base;
    const int lane = t & 63, w = t >> 6;
    uint32_t cq = 0, cst = 0, ce = 0;  // the earlier tiles' totals
    for (uint32_t i0 = 0; i0 < n; i0 += kT) {
        const uint32_t i = i0 + t;
        const uint32_t f = i < n ? fs[i] : 0u;
        const bool head = i < n && (f >> 16) == i;
        const uint32_t size = f & 0xffffu;
        const bool elig = i < n && size - 1 >= m;
        const uint32_t h = head, s = head ? size : 0u, e = elig;
        uint32_t ih = h, is = s, ie = e;
        wave_scan3(ih, is, ie);
        if (lane == 63) {
            red[0][w] = ih;
            red[1][w] = is;
            red[2][w] = ie;
        }
        __syncthreads();
        uint32_t q = cq + ih - h, st = cst + is - s, el = ce + ie - e;
        for (int v = 0; v < w; v++) {
            q += red[0][v];
            st += red[1][v];
            el += red[2][v];
        }
        if (head) {
            hq[i] = q << 16 | st;
            start[q] = st;
        }
        if (elig) eligible[el] = (int32_t)i;
        cq += red[0][0] + red[0][1] + red[0][2] + red[0][3];
        cst += red[1][0] + red[1][1] + red[1][2] + red[1][3];
        ce += red[2][0] + red[2][1] + red[2][2] + red[2][3];
        __syncthreads();  // red[] reused by the next tile; hq complete after the last one
    }
    if (t == 0) {
        start[cq] = n;
        g.n_cells[p] = cq;
        g.n_eligible[p] = ce;
        g.status[p] = 0;
    }
    uint32_t *__restrict__ cell = g.cell + base;
    int32_t *__restrict__ members = g.members + base;
    for (uint32_t i = t; i < n; i += kT) {
        const uint32_t h = hq[fs[i] >> 16];
        cell[i] = h >> 16;
        members[(h & 0xffffu) + rank[i]] = (int32_t)i;  // rank[i]: this thread's own store
    }
}

hipError_t launch_multi_grid(hipStream_t st, const float4 *pts, const uint32_t *offsets, uint32_t P, int cell_size,
                             uint32_t m, const MultiGrid &g) {
    if (P == 0 || cell_size <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_multi_grid, dim3(P), dim3(kT), 0, st, pts, offsets, (float)cell_size, m, g);
    return hipGetLastError();
}

}  // namespace usac
