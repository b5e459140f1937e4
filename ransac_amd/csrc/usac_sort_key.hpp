// Device input in quality order (ABI 26, usac_multi_create_device_sorted): the sort key of a score, shared by the
// sort kernel (kernels_multi_sort.hip) and the host (tests/cpp_multi_device_sorted/key_check.cpp holds it to the
// written rule).  No HIP call and no other header of the library.
//
// The rule, within one problem: the better score first (descending: the larger, else the smaller); equal scores,
// +0 and -0 among them, in ascending column order; +inf and -inf are ordinary numbers; a NaN of any sign or
// payload comes after every number in either direction, NaNs among themselves in ascending column order.
//
// sort_key maps the score's bits to 32 bits whose unsigned order is that rule's, sort_composite puts the column
// below them.  The composites of a problem are all distinct, so sorting them ascending is stable by construction
// and its result does not depend on the sorting algorithm.  Integer-only, as the pack: no float is compared.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define USAC_SORT_HD __host__ __device__ __forceinline__
#else
#define USAC_SORT_HD inline
#endif

namespace usac {

// what a NaN maps to, and the key part of a padding composite: no number's key in either direction (a number's
// monotone image lies in 0x007fffff (-inf) .. 0xff800000 (+inf), and so does its complement)
constexpr uint32_t kSortKeyLast = 0xffffffffu;

USAC_SORT_HD uint32_t sort_key(uint32_t bits, bool descending) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return kSortKeyLast;   // NaN
    if (bits == 0x80000000u) bits = 0;                             // -0 == +0
    const uint32_t mono = (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;  // ascending with the number
    return descending ? ~mono : mono;
}

USAC_SORT_HD uint64_t sort_composite(uint32_t bits, bool descending, uint32_t column) {
    return (uint64_t)sort_key(bits, descending) << 32 | column;
}

}  // namespace usac
