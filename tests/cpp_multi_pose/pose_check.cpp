// Host-only check, built with g++ and -fsanitize=address,undefined by tests/test_multi_pose_cpu.py: the argument
// rule usac_multi_pose_device shares with usac_multi_export_device (ransac_amd/csrc/usac_pack.hpp) -- the largest
// problem of a context from its offsets, the width a caller may name for P x n_max output bytes, the message of
// a refusal, and the extent of the pose's one P x n_max output.  No GPU, no HIP, no library.
//   pose_check   prints "ok" or a message and exits 1
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "usac_pack.hpp"

static int fail(const char *what, unsigned item) {
    std::printf("FAILED %s (item %u)\n", what, item);
    return 1;
}

int main() {
    // the largest problem: heap arrays of exactly P + 1 offsets, so that a read past the end is seen
    struct { std::vector<uint32_t> offsets; uint32_t widest; } sizes[] = {
        {{0u, 5u}, 5u},
        {{0u, 5u, 11u, 74u, 138u, 203u, 460u, 1460u, 1717u}, 1000u},
        {{0u, 1000u, 1005u}, 1000u},
        {{0u, 7u, 14u, 21u}, 7u},
        {{0u, 0xfffffff0u, 0xffffffffu}, 0xfffffff0u},
        {{0u}, 0u},  // P = 0: no problem, no read
    };
    unsigned n = 0;
    for (const auto &q : sizes) {
        const std::vector<uint32_t> heap(q.offsets);
        if (usac::widest_problem(heap.data(), (uint32_t)heap.size() - 1) != q.widest) return fail("widest problem", n);
        n++;
    }
    // the width: a context from device input (ctx_n_max != 0) takes its own alone, one from the host any width
    // from the largest problem's size up
    struct { uint32_t ctx, widest, n_max; usac::WidthStatus st; } widths[] = {
        {300u, 0u, 300u, usac::kWidthOk},
        {300u, 0u, 299u, usac::kWidthNotTheContexts},
        {300u, 0u, 301u, usac::kWidthNotTheContexts},
        {300u, 0u, 0u, usac::kWidthNotTheContexts},
        {0u, 1000u, 1000u, usac::kWidthOk},
        {0u, 1000u, 999u, usac::kWidthBelowWidest},
        {0u, 1000u, 0u, usac::kWidthBelowWidest},
        {0u, 1000u, 0xffffffffu, usac::kWidthOk},
        {0u, 0u, 0u, usac::kWidthOk},  // the extent rule refuses a width of 0, below
        {0xffffffffu, 0u, 0xffffffffu, usac::kWidthOk},
    };
    n = 0;
    for (const auto &q : widths) {
        const usac::WidthStatus st = usac::output_width(q.ctx, q.widest, q.n_max);
        if (st != q.st) return fail("width rule", n);
        const std::string msg = usac::width_message(st, q.ctx, q.widest);
        if ((st == usac::kWidthOk) != msg.empty()) return fail("a message for every refusal, and for none else", n);
        if (st == usac::kWidthNotTheContexts && msg.find(std::to_string(q.ctx)) == std::string::npos)
            return fail("the message names the context's width", n);
        if (st == usac::kWidthBelowWidest && msg.find(std::to_string(q.widest)) == std::string::npos)
            return fail("the message names the largest problem's size", n);
        n++;
    }
    // the extent of front_mask: P x n_max bytes below 2^32, n_max > 0
    struct { uint32_t P, n_max; bool ok; } ex[] = {
        {65535u, 65537u, true}, {65535u, 65538u, false}, {1u, 0xffffffffu, true}, {2u, 0x80000000u, false},
        {2u, 0x7fffffffu, true}, {8u, 0u, false},        {0u, 1000u, false},      {8u, 1000u, true},
    };
    n = 0;
    for (const auto &q : ex) {
        if (usac::pack_extent_ok(q.P, q.n_max) != q.ok) return fail("extent rule", n);
        n++;
    }
    std::printf("ok\n");
    return 0;
}
