// The host text between the two pack kernels (ransac_amd/csrc/usac_pack.hpp, ABI 25) in a stand-alone program,
// built by tests/test_multi_device_cpu.py with -fsanitize=address,undefined:
//   pack_check <cases.u32>
// cases.u32: n_cases, then per case P, m, n_max, want_status, want_bad, sizes[P], flags[P], want_offsets[P + 1]
// (the offsets are compared on a case that is accepted).  Every vector is allocated at its exact length, so a
// read or write past P (or P + 1) values is the sanitizer's to report.  Also the extent check's boundary values.
// Prints "ok <n_cases>" and returns 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "usac_pack.hpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const std::vector<uint32_t> w(reinterpret_cast<const uint32_t *>(raw.data()),
                                  reinterpret_cast<const uint32_t *>(raw.data()) + raw.size() / 4);
    size_t at = 0;
    const uint32_t n_cases = w.at(at++);
    for (uint32_t c = 0; c < n_cases; c++) {
        const uint32_t P = w.at(at), m = w.at(at + 1), n_max = w.at(at + 2), want = w.at(at + 3), want_bad = w.at(at + 4);
        at += 5;
        const std::vector<uint32_t> sizes(w.begin() + (long)at, w.begin() + (long)(at + P));
        const std::vector<uint32_t> flags(w.begin() + (long)(at + P), w.begin() + (long)(at + 2 * (size_t)P));
        const std::vector<uint32_t> want_off(w.begin() + (long)(at + 2 * (size_t)P), w.begin() + (long)(at + 3 * (size_t)P + 1));
        at += 3 * (size_t)P + 1;
        std::vector<uint32_t> off((size_t)P + 1, 0xdeadbeefu);
        uint32_t bad = 0xdeadbeefu;
        const usac::PackStatus st = usac::pack_offsets(sizes.data(), flags.data(), P, m, n_max, off.data(), &bad);
        if ((uint32_t)st != want || bad != want_bad) {
            std::printf("case %u: status %u (want %u), bad %u (want %u)\n", c, (unsigned)st, want, bad, want_bad);
            return 1;
        }
        if (st == usac::kPackOk && off != want_off) {
            std::printf("case %u: offsets differ\n", c);
            return 1;
        }
        if (st != usac::kPackOk) {
            const std::string msg = usac::pack_message(st, bad, sizes[bad], m);
            if (msg.find("problem " + std::to_string(bad) + ":") != 0) {
                std::printf("case %u: the message does not name the problem: %s\n", c, msg.c_str());
                return 1;
            }
        }
    }
    if (at != w.size()) {
        std::printf("trailing words\n");
        return 1;
    }
    const bool ext = usac::pack_extent_ok(1, 1) && usac::pack_extent_ok(65535, 65537) && usac::pack_extent_ok(1, 0xffffffffu) &&
                     !usac::pack_extent_ok(65536, 65536) && !usac::pack_extent_ok(0, 5) && !usac::pack_extent_ok(5, 0) &&
                     !usac::pack_extent_ok(2, 0x80000000u);
    if (!ext) {
        std::printf("pack_extent_ok is wrong at a boundary\n");
        return 1;
    }
    std::printf("ok %u\n", n_cases);
    return 0;
}
