// The host-only part of tests/cpp_multi_lo/consumer.cpp: file reading and the JSON of one problem.
// No library call in here, so lo_draw_check.cpp runs it under the sanitizers without the device library.
#pragma once
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "usac_gpu.h"

namespace consumer_host {

template <class T>
std::vector<T> read_file(const char *path, size_t count) {
    std::vector<T> v(count);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(sizeof(T) * count));
    if ((size_t)f.gcount() != sizeof(T) * count) throw std::runtime_error(std::string("short read: ") + path);
    return v;
}

inline int32_t bits(float x) {
    int32_t b;
    std::memcpy(&b, &x, sizeof(b));
    return b;
}

// one problem as a JSON object (floats as their int32 bit patterns); q == NULL: no PROSAC keys
inline std::string problem_json(const usac_multi_output &o, const usac_multi_lo_output &l,
                                const usac_multi_prosac_output *q) {
    char buf[256];
    std::string s;
    std::snprintf(buf, sizeof(buf), "{\"hyp_index\": %llu, \"inliers\": %d, \"score\": %d, \"valid\": %d, \"model\": [",
                  (unsigned long long)o.best.hyp_index, o.best.inliers, bits(o.best.score), o.best.valid);
    s += buf;
    for (int k = 0; k < 9; k++) {
        std::snprintf(buf, sizeof(buf), "%s%d", k ? ", " : "", bits(o.best.model[k]));
        s += buf;
    }
    std::snprintf(buf, sizeof(buf), "], \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d", o.rounds,
                  o.hypotheses, o.bound, o.status);
    s += buf;
    std::snprintf(buf, sizeof(buf),
                  ", \"lo\": {\"lo_calls\": %u, \"inner_iters\": %u, \"iterative_iters\": %u, \"fits\": %u, "
                  "\"improved\": %u, \"capped\": %u, \"draws\": %u, \"threshold\": %d}",
                  l.lo_calls, l.inner_iters, l.iterative_iters, l.fits, l.improved, l.capped, l.draws, bits(l.threshold));
    s += buf;
    if (q) {
        std::snprintf(buf, sizeof(buf),
                      ", \"termination_length\": %u, \"largest_sample_size\": %u, \"clock\": %u, \"scans\": %u",
                      q->termination_length, q->largest_sample_size, q->clock, q->scans);
        s += buf;
    }
    return s + "}";
}

}  // namespace consumer_host
