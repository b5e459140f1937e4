// Device output of a multi context (ABI 27, usac_multi_export_device): the resident result of a polishing call,
// the P results k_multi_polish wrote and its mask over the packed rows, handed over in a GPU consumer's layout
// -- models, counts and statuses as arrays, the mask scattered into P x n_max bytes, the inliers' columns as
// P x k_max entries padded with -1, the pixel-space models of an essential context with intrinsics.
//
// One launch, one 256-thread workgroup per problem (DESIGN.md §8b "Device output").  A workgroup owns its output
// rows: it writes the whole mask row to 0 and the whole list row to -1, passes a barrier, and only then scatters
// into them, so no memset and no second launch come before it.  The walk over the packed rows is k_multi_pack's
// (kernels_multi_pack.hip): blocks of 256 rows, neighbouring lanes on neighbouring rows, a set row's place in the
// list the running base, plus the set rows of the waves below (four totals through LDS, two copies taken in
// turn), plus those of the lanes below (ballot and mbcnt).  The list is in packed-row order: ascending columns on
// a context from usac_multi_create_device, quality order on one from usac_multi_create_device_sorted.
//
// Rows are moved, not computed with.  The pixel-space model is the one piece of arithmetic: usac_pixels.hpp's
// pixel_model, the text usac_multi_pixel_models runs on the host, in fp64 under -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "usac_kernels.h"
#include "usac_pixels.hpp"

namespace usac {

namespace {

// row[0 .. n) = v by all 256 threads: a head of single units up to the first 16-byte boundary, 16-byte stores,
// a tail of single units.  v16 is v repeated over 16 bytes.  Unit is uint8_t or uint32_t (row is aligned to it).
template <typename Unit>
__device__ __forceinline__ void export_fill(Unit *row, uint32_t n, Unit v, uint32_t v16) {
    constexpr uint32_t kPer = 16 / sizeof(Unit);  // units per 16-byte store
    uint32_t head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / (uint32_t)sizeof(Unit);
    if (head > n) head = n;
    const uint32_t wide = (n - head) / kPer, tail0 = head + wide * kPer;  // n - tail0 < kPer
    if (threadIdx.x < head) row[threadIdx.x] = v;
    uint4 *q = reinterpret_cast<uint4 *>(row + head);
    for (uint32_t i = threadIdx.x; i < wide; i += 256) q[i] = make_uint4(v16, v16, v16, v16);
    if (threadIdx.x < n - tail0) row[tail0 + threadIdx.x] = v;
}

}  // namespace

// IDENT: the context has no source columns, packed row i of a problem is its column i
template <bool IDENT>
__global__ __launch_bounds__(256) void k_multi_export(MultiExport a) {
    __shared__ uint32_t sh_n[2][4];
    const uint32_t p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t base = a.offsets[p], n = a.offsets[p + 1] - base;
    uint8_t *mrow = a.mask_out ? a.mask_out + (size_t)p * a.n_max : nullptr;
    int32_t *crow = a.cols ? a.cols + (size_t)p * a.k_max : nullptr;
    if (mrow) export_fill<uint8_t>(mrow, a.n_max, 0, 0u);
    if (crow) export_fill<uint32_t>(reinterpret_cast<uint32_t *>(crow), a.k_max, 0xffffffffu, 0xffffffffu);
    if (threadIdx.x == 0) {
        const usac_multi_polish_output &r = a.pol[p];
        if (a.models)
            for (int k = 0; k < 9; k++) a.models[9 * (size_t)p + k] = r.model[k];
        if (a.inliers) a.inliers[p] = r.inliers;
        if (a.status) a.status[p] = r.status;
    }
    if (a.pixel_models && threadIdx.x == 64) {  // the second wave's first lane: beside thread 0's copies
        float f[9];
        pixel_model(a.k + 9 * (size_t)p, a.k + 9 * ((size_t)a.P + p), a.pol[p].model, f);
        for (int k = 0; k < 9; k++) a.pixel_models[9 * (size_t)p + k] = f[k];
    }
    if (!mrow && !crow) return;  // uniform over the workgroup
    // the rows' clears are visible to the whole workgroup before any lane scatters into them
    __syncthreads();
    uint32_t running = 0;
    for (uint32_t b = 0, it = 0; b < (n >> 8) + ((n & 255u) != 0u); b++, it ^= 1) {
        const uint32_t i = b * 256 + threadIdx.x;
        const bool in = i < n;
        const uint8_t bit = in ? a.mask[(size_t)base + i] : (uint8_t)0;
        const uint32_t col = !in ? 0u : IDENT ? i : a.src[(size_t)base + i];
        const bool set = bit != 0 && col < a.n_max;
        if (set && mrow) mrow[col] = bit;
        if (!crow) continue;  // uniform: no barrier is skipped by a part of the workgroup
        const unsigned long long bal = __ballot(set);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        // two copies of the totals, taken in turn (k_multi_pack): a wave writes a copy again only after the
        // barrier of the block in between, which every wave reaches after it has read that copy
        if (lane == 0) sh_n[it][wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        const uint32_t t0 = sh_n[it][0], t1 = sh_n[it][1], t2 = sh_n[it][2], t3 = sh_n[it][3];
        const uint32_t before = wave == 0 ? 0u : wave == 1 ? t0 : wave == 2 ? t0 + t1 : t0 + t1 + t2;
        const uint32_t at = running + before + below;
        if (set && at < a.k_max) crow[at] = (int32_t)col;
        running += (t0 + t1) + (t2 + t3);
    }
}

hipError_t launch_multi_export(hipStream_t st, const MultiExport &a) {
    if (a.P == 0 || a.P > kMultiMaxActive || ((a.mask_out || a.cols) && a.n_max == 0) || (a.cols != nullptr) != (a.k_max != 0) ||
        (a.pixel_models && !a.k))
        return hipErrorInvalidValue;
    if (a.src) hipLaunchKernelGGL(k_multi_export<false>, dim3(a.P), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_multi_export<true>, dim3(a.P), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace usac
