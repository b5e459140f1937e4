// The host-only part of tests/cpp_multi_sprt/consumer.cpp: file reading and the JSON of one problem.
// No library call in here, so sprt_update_check.cpp runs it under the sanitizers without the device library.
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

inline long long bits(double x) {
    long long b;
    std::memcpy(&b, &x, sizeof(b));
    return b;
}

// one problem as a JSON object (floats and doubles as their integer bit patterns); q == NULL: no PROSAC keys
inline std::string problem_json(const usac_multi_output &o, const usac_multi_sprt_output &s,
                                const usac_multi_prosac_output *q) {
    char buf[320];
    std::string js;
    std::snprintf(buf, sizeof(buf), "{\"hyp_index\": %llu, \"inliers\": %d, \"score\": %d, \"valid\": %d, \"model\": [",
                  (unsigned long long)o.best.hyp_index, o.best.inliers, bits(o.best.score), o.best.valid);
    js += buf;
    for (int k = 0; k < 9; k++) {
        std::snprintf(buf, sizeof(buf), "%s%d", k ? ", " : "", bits(o.best.model[k]));
        js += buf;
    }
    std::snprintf(buf, sizeof(buf), "], \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d", o.rounds,
                  o.hypotheses, o.bound, o.status);
    js += buf;
    std::snprintf(buf, sizeof(buf),
                  ", \"sprt\": {\"epsilon\": %lld, \"delta\": %lld, \"A\": %lld, \"tests\": %u, \"accepted\": %u, "
                  "\"rejected\": %u, \"points_tested\": %llu}",
                  bits(s.epsilon), bits(s.delta), bits(s.A), s.tests, s.accepted, s.rejected,
                  (unsigned long long)s.points_tested);
    js += buf;
    if (q) {
        std::snprintf(buf, sizeof(buf),
                      ", \"termination_length\": %u, \"largest_sample_size\": %u, \"clock\": %u, \"scans\": %u",
                      q->termination_length, q->largest_sample_size, q->clock, q->scans);
        js += buf;
    }
    return js + "}";
}

}  // namespace consumer_host
