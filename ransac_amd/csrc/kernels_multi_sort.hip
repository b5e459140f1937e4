// Device input in quality order (ABI 26, usac_multi_create_device_sorted): a stable sort of every problem's packed
// rows by the caller's score per column, better first (usac_sort_key.hpp has the rule and the key).
//
// It runs behind the two pack passes (kernels_multi_pack.hip), which are as they were: k_multi_pack has written the
// kept rows and their columns, in ascending column order, into a temporary block, and k_multi_sort, one 256-thread
// workgroup per problem, moves them into the context's own pts / src in sorted order.  A row's score is read once,
// through its column: scores[p * n_max + src[i]]; scores of columns that were not kept are never looked at.  What
// is sorted is the composite (key << 32 | i), i the row's place among the problem's packed rows: the pack keeps
// column order, so i orders as the column does, the composites are distinct -- the sort is stable whatever the
// algorithm -- and i, unlike a column read back from memory, is below the problem's row count by construction.
//
// Up to `cap` rows (kMultiSortLds = 4096, 32 KB of composites; USAC_MULTI_SORT_LDS lowers it for tests): a bitonic
// network in LDS over the next power of two, padded with all-ones composites, which no row has (its low half is a
// place below 4096).  Every loop bound and barrier depends on the padded size alone: they are workgroup-uniform.
// Above the cap: the rows are sorted `cap` at a time by the same network into runs in global memory (8 bytes per
// row, allocated only when a problem needs it), and a row's destination is its rank -- its place in its own run plus,
// by bisection, the number of smaller composites in every other run; distinct composites make the ranks a
// permutation.  That is O(n (n / cap) log cap) steps, for any n the pack accepts.
//
// Rows are moved as integers, 16 bytes at a time, and never computed with.  A problem writes only inside
// offsets[p] .. offsets[p + 1] - 1 whatever the caller's memory holds by now: the destination is a place below the
// problem's row count, the source a place the composite carried, checked against the same count, and a column that
// is not below n_max (a place the pack did not write because the input changed under it) is not dereferenced.
#include <hip/hip_runtime.h>

#include "usac_kernels.h"
#include "usac_sort_key.hpp"

namespace usac {

namespace {

constexpr uint64_t kSortPad = ~0ull;

// the composite of packed row i of problem p
__device__ __forceinline__ uint64_t sort_load(const MultiSort &a, uint32_t p, uint32_t out0, uint32_t i) {
    const uint32_t j = a.src_in[(size_t)out0 + i];
    if (j >= a.n_max) return (uint64_t)kSortKeyLast << 32 | i;
    return sort_composite(a.scores[(size_t)p * a.n_max + j], a.descending != 0, i);
}

// the smallest power of two >= x, at least 2
__device__ __forceinline__ uint32_t sort_pow2(uint32_t x) { return x <= 2 ? 2u : 1u << (32 - __clz((int)(x - 1))); }

// sh[0 .. N) ascending, N a power of two in 2..kMultiSortLds; the caller's barrier stands between its writes of sh
// and this, and the last barrier here between the network and the caller's reads
__device__ __forceinline__ void sort_tile(uint64_t *sh, uint32_t N) {
    for (uint32_t k = 2; k <= N; k <<= 1)
        for (uint32_t j = k >> 1; j != 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (N >> 1); t += 256) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint64_t x = sh[lo], y = sh[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    sh[lo] = y;
                    sh[hi] = x;
                }
            }
            __syncthreads();
        }
}

// packed row `from` of the temporary block -> row `to` of the context, both places of problem p (n rows at out0)
__device__ __forceinline__ void sort_move(const MultiSort &a, uint32_t out0, uint32_t n, uint32_t to, uint32_t from) {
    if (to >= n || from >= n) return;
    a.pts[(size_t)out0 + to] = a.rows_in[(size_t)out0 + from];
    a.src[(size_t)out0 + to] = a.src_in[(size_t)out0 + from];
}

}  // namespace

__global__ __launch_bounds__(256) void k_multi_sort(MultiSort a) {
    __shared__ uint64_t sh[kMultiSortLds];
    const uint32_t p = blockIdx.x, out0 = a.offsets[p], n = a.offsets[p + 1] - out0;
    const uint32_t L = a.cap == 0 ? 1u : a.cap < kMultiSortLds ? a.cap : kMultiSortLds;
    if (n <= L) {
        const uint32_t N = sort_pow2(n);
        for (uint32_t i = threadIdx.x; i < N; i += 256) sh[i] = i < n ? sort_load(a, p, out0, i) : kSortPad;
        __syncthreads();
        sort_tile(sh, N);
        for (uint32_t i = threadIdx.x; i < n; i += 256) sort_move(a, out0, n, i, (uint32_t)sh[i]);
        return;
    }
    // above the cap (n > L >= 1): runs of L rows, r * L < n for every run r
    const uint32_t runs = (n - 1) / L + 1;
    for (uint32_t r = 0; r < runs; r++) {
        const uint32_t s = r * L, cnt = n - s < L ? n - s : L, N = sort_pow2(cnt);
        for (uint32_t i = threadIdx.x; i < N; i += 256) sh[i] = i < cnt ? sort_load(a, p, out0, s + i) : kSortPad;
        __syncthreads();
        sort_tile(sh, N);
        for (uint32_t i = threadIdx.x; i < cnt; i += 256) a.runs[(size_t)out0 + s + i] = sh[i];
        __syncthreads();  // sh is free again; after the last run, every run is visible to the workgroup
    }
    const uint64_t *run = a.runs + out0;
    for (uint32_t e = threadIdx.x; e < n; e += 256) {
        const uint64_t c = run[e];
        const uint32_t own = e / L;
        uint32_t rank = e - own * L;
        for (uint32_t r = 0; r < runs; r++) {
            if (r == own) continue;
            const uint32_t s = r * L, cnt = n - s < L ? n - s : L;
            uint32_t lo = 0, hi = cnt;  // run[s + x] < c for x < lo, > c for x >= hi
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (run[(size_t)s + mid] < c) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        sort_move(a, out0, n, rank, (uint32_t)c);
    }
}

hipError_t launch_multi_sort(hipStream_t st, uint32_t P, const MultiSort &a) {
    if (P == 0 || P > kMultiMaxActive || a.n_max == 0 || a.cap == 0 || a.cap > kMultiSortLds) return hipErrorInvalidValue;
    if (!a.scores || !a.offsets || !a.rows_in || !a.src_in || !a.pts || !a.src) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_multi_sort, dim3(P), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace usac
