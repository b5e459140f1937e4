// Host-only check, built with g++ and -fsanitize=address,undefined by tests/test_multi_refine_cpu.py: the argument
// logic of the pose refinement entries that needs no device (ransac_amd/csrc/usac_pack.hpp) -- the step limit both
// entries take, and the layout of the one device block usac_multi_refine_pose stages its host arrays through:
// every array inside the block, none overlapping another, the doubles 8-byte and the floats and ints 4-byte
// aligned at any P.  The layout is exercised on a heap block of exactly `bytes` bytes, so that a write past an
// array's end is seen.  No GPU, no HIP, no library.
//   refine_check   prints "ok" or a message and exits 1
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "usac_pack.hpp"

static int fail(const char *what, unsigned item) {
    std::printf("FAILED %s (item %u)\n", what, item);
    return 1;
}

int main() {
    struct { uint32_t iters; bool ok; } lim[] = {{0u, true},   {1u, true},    {10u, true},         {100u, true},
                                                 {101u, false}, {1000u, false}, {0xffffffffu, false}};
    unsigned n = 0;
    for (const auto &q : lim) {
        if (usac::refine_iters_ok(q.iters) != q.ok) return fail("step limit", n);
        n++;
    }
    struct { size_t P, rows; } cases[] = {{1, 5}, {1, 0}, {2, 11}, {3, 1000}, {7, 1463}, {8, 2461}, {11, 3}, {512, 512000}};
    n = 0;
    for (const auto &q : cases) {
        const usac::RefineBlock b = usac::refine_block(q.P, q.rows);
        struct { size_t at, bytes, align; } parts[] = {
            {b.cost0, 8 * q.P, 8}, {b.cost, 8 * q.P, 8},       {b.R, 36 * q.P, 4},    {b.t, 12 * q.P, 4},
            {b.E, 36 * q.P, 4},    {b.iterations, 4 * q.P, 4}, {b.used, 4 * q.P, 4}, {b.mask, q.rows, 1}};
        size_t total = 0;
        for (const auto &part : parts) {
            if (part.at % part.align) return fail("alignment", n);
            if (part.at + part.bytes > b.bytes) return fail("an array ends past the block", n);
            total += part.bytes;
        }
        if (total != b.bytes) return fail("the block is the sum of its arrays", n);
        // every array filled with its own tag in a block of exactly b.bytes: no tag is overwritten by another
        std::vector<uint8_t> block(b.bytes);
        unsigned tag = 1;
        for (const auto &part : parts) {
            if (part.bytes) std::memset(block.data() + part.at, (int)tag, part.bytes);
            tag++;
        }
        tag = 1;
        for (const auto &part : parts) {
            for (size_t k = 0; k < part.bytes; k++)
                if (block[part.at + k] != tag) return fail("two arrays overlap", n);
            tag++;
        }
        n++;
    }
    std::printf("ok\n");
    return 0;
}
