// The sort key of device input in quality order (ransac_amd/csrc/usac_sort_key.hpp, ABI 26) in a stand-alone
// program, built by tests/test_multi_device_sorted_cpu.py with -fsanitize=address,undefined:
//   key_check <cases.u32>
// cases.u32: n_cases, then per case descending, n, bits[n] (the scores of the kept columns), cols[n] (the kept
// columns, ascending) and want[n], the order numpy's lexsort gives: want[i] is the place in bits / cols of the
// row that comes i-th.  Per case the composites must be distinct, their ascending order must be want, a NaN's key
// must be the one reserved key and no number's.  Prints "ok <n_cases>" and returns 0 when everything agrees.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <numeric>
#include <vector>

#include "usac_sort_key.hpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const std::vector<uint32_t> w(reinterpret_cast<const uint32_t *>(raw.data()),
                                  reinterpret_cast<const uint32_t *>(raw.data()) + raw.size() / 4);
    size_t at = 0;
    const uint32_t n_cases = w.at(at++);
    for (uint32_t c = 0; c < n_cases; c++) {
        const bool descending = w.at(at) != 0;
        const uint32_t n = w.at(at + 1);
        at += 2;
        if (at + 3 * (size_t)n > w.size()) {
            std::printf("case %u: short file\n", c);
            return 1;
        }
        const std::vector<uint32_t> bits(w.begin() + (long)at, w.begin() + (long)(at + n));
        const std::vector<uint32_t> cols(w.begin() + (long)(at + n), w.begin() + (long)(at + 2 * (size_t)n));
        const std::vector<uint32_t> want(w.begin() + (long)(at + 2 * (size_t)n), w.begin() + (long)(at + 3 * (size_t)n));
        at += 3 * (size_t)n;
        std::vector<uint64_t> comp(n);
        for (uint32_t i = 0; i < n; i++) {
            float x;
            std::memcpy(&x, &bits[i], sizeof(x));
            const uint32_t key = usac::sort_key(bits[i], descending);
            if ((key == usac::kSortKeyLast) != (bool)std::isnan(x)) {
                std::printf("case %u: bits %08x: key %08x\n", c, bits[i], key);
                return 1;
            }
            comp[i] = usac::sort_composite(bits[i], descending, cols[i]);
            if ((uint32_t)(comp[i] >> 32) != key || (uint32_t)comp[i] != cols[i]) {
                std::printf("case %u: the composite of place %u is not key << 32 | column\n", c, i);
                return 1;
            }
        }
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return comp[a] < comp[b]; });
        for (uint32_t i = 0; i + 1 < n; i++)
            if (comp[order[i]] == comp[order[i + 1]]) {
                std::printf("case %u: two rows share the composite %016llx\n", c, (unsigned long long)comp[order[i]]);
                return 1;
            }
        if (order != want) {
            std::printf("case %u (descending %d): the order differs from the rule's\n", c, (int)descending);
            return 1;
        }
    }
    if (at != w.size()) {
        std::printf("trailing words\n");
        return 1;
    }
    std::printf("ok %u\n", n_cases);
    return 0;
}
