// Pixel coordinates -> calibrated coordinates of an essential multi context (ABI 24,
// usac_multi_create_essential_pixels): one launch over the concatenated points, in place.
//
// The written spec (DESIGN.md §8b "Pixel coordinates"), plain fp32 in this order, no contraction, correctly
// rounded division -- a float32 numpy restatement has the same bits:
//   y = (v - cy) / fy,  x = ((u - cx) - s * y) / fx      view 1 under K1_p, view 2 under K2_p
// The kernel moves 16 B in and 16 B out per row and is bound by that: one float4 load and one float4 store
// per thread, neighbouring threads on neighbouring rows.  The problem's intrinsics are three float4 loads of
// an address that is the same for all lanes of a wave except where the wave straddles a problem boundary.
#include <hip/hip_runtime.h>

#include "usac_kernels.h"

namespace usac {

// one thread per row of the concatenated array: its problem by bisection of offsets (as k_multi_mask),
// calib: per problem kCalibFloats floats, fx s cx fy cy of view 1, the same of view 2, two of padding
__global__ __launch_bounds__(256) void k_multi_calibrate(float4 *__restrict__ pts_all,
                                                         const uint32_t *__restrict__ offsets, uint32_t P,
                                                         uint32_t n_total, const float4 *__restrict__ calib) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_total) return;
    uint32_t lo = 0, hi = P;  // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    static_assert(kCalibFloats == 12, "three float4 per problem");
    const float4 c0 = calib[3 * (size_t)lo], c1 = calib[3 * (size_t)lo + 1], c2 = calib[3 * (size_t)lo + 2];
    const float fx1 = c0.x, s1 = c0.y, cx1 = c0.z, fy1 = c0.w, cy1 = c1.x;
    const float fx2 = c1.y, s2 = c1.z, cx2 = c1.w, fy2 = c2.x, cy2 = c2.y;
    const float4 p = pts_all[i];
    float4 q;
    q.y = (p.y - cy1) / fy1;
    q.x = ((p.x - cx1) - s1 * q.y) / fx1;
    q.w = (p.w - cy2) / fy2;
    q.z = ((p.z - cx2) - s2 * q.w) / fx2;
    pts_all[i] = q;
}

hipError_t launch_multi_calibrate(hipStream_t st, float4 *pts, const uint32_t *offsets, uint32_t P, uint32_t n_total,
                                  const float *calib) {
    if (P == 0 || n_total == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_multi_calibrate, dim3((n_total + 255) / 256), dim3(256), 0, st, pts, offsets, P, n_total,
                       reinterpret_cast<const float4 *>(calib));
    return hipGetLastError();
}

}  // namespace usac
