// Pixel coordinates of an essential multi context (ABI 24): the validation of an intrinsic matrix, the
// threshold of a pixel tolerance and the pixel-space model of an essential matrix (DESIGN.md §8b "Pixel
// coordinates").  Host and device (ABI 27: k_multi_export writes the pixel-space models; the library is built
// with -ffp-contract=off, so the one text gives one result on both).  No HIP call and no other header of the
// library, so a stand-alone program built with g++ can include it (tests/cpp_multi_pixels/pixels_check.cpp,
// tests/cpp_multi_export/export_check.cpp).
//
// K is row-major k[0..8] = fx, s, cx, 0, fy, cy, 0, 0, 1.  The calibrated point of a pixel (u, v) is, in fp32
// in this order (k_multi_calibrate, kernels_multi_calib.hip):
//   y = (v - cy) / fy,  x = ((u - cx) - s * y) / fx
#pragma once
#include <cmath>
#include <cstdint>

#ifndef USAC_HD  // as usac_prosac.hpp
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define USAC_HD __host__ __device__ __forceinline__
#else
#define USAC_HD inline
#endif
#endif

namespace usac {

// what the kernel reads per problem: fx, s, cx, fy, cy of view 1, then of view 2, padded to three float4
constexpr uint32_t kCalibFloats = 12;

// an upper-triangular K with positive focal lengths, finite entries and a last row of 0 0 1
USAC_HD bool pixel_k_ok(const float *k) {
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(k[i])) return false;
    return k[0] > 0.f && k[4] > 0.f && k[3] == 0.f && k[6] == 0.f && k[7] == 0.f && k[8] == 1.f;
}

// k1, k2 (3 x 3 each) -> the kernel's kCalibFloats values of one problem
USAC_HD void pixel_pack(const float *k1, const float *k2, float *out) {
    const float *ks[2] = {k1, k2};
    for (int v = 0; v < 2; v++) {
        const float *k = ks[v];
        float *o = out + 5 * v;
        o[0] = k[0];  // fx
        o[1] = k[1];  // s
        o[2] = k[2];  // cx
        o[3] = k[4];  // fy
        o[4] = k[5];  // cy
    }
    out[10] = out[11] = 0.f;
}

// (t / f)^2 with f the mean of the four focal lengths, in fp32 in this order
USAC_HD float pixel_threshold(const float *k1, const float *k2, float t) {
    const float f = ((k1[0] + k1[4]) + (k2[0] + k2[4])) * 0.25f;
    const float r = t / f;
    return r * r;
}

// the closed-form inverse of an upper-triangular K, from its fp32 entries widened to fp64
USAC_HD void pixel_k_inverse(const float *k, double *inv) {
    const double fx = k[0], s = k[1], cx = k[2], fy = k[4], cy = k[5];
    inv[0] = 1.0 / fx;
    inv[1] = -s / (fx * fy);
    inv[2] = (s * cy - cx * fy) / (fx * fy);
    inv[3] = 0.0;
    inv[4] = 1.0 / fy;
    inv[5] = -cy / fy;
    inv[6] = 0.0;
    inv[7] = 0.0;
    inv[8] = 1.0;
}

// F = K2^-T E K1^-1 in fp64: G = E K1^-1, then F = K2^-T G, every entry a three-term sum taken left to
// right, no normalisation, one cast to fp32 at the end
USAC_HD void pixel_model(const float *k1, const float *k2, const float *e, float *f) {
    double a[9], b[9], g[9];
    pixel_k_inverse(k1, a);
    pixel_k_inverse(k2, b);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            g[3 * i + j] = ((double)e[3 * i] * a[j] + (double)e[3 * i + 1] * a[3 + j]) + (double)e[3 * i + 2] * a[6 + j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            f[3 * i + j] = (float)((b[i] * g[j] + b[3 + i] * g[3 + j]) + b[6 + i] * g[6 + j]);
}

}  // namespace usac
