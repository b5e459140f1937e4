// A consumer of usac_gpu::MultiContext::runNapsac / gridNeighbors (include/usac_gpu.hpp), C++11, no HIP
// headers:
//   consumer abi
//   consumer run <estimator> <P> <pts.f32> <offsets.u32> <thr> <prob> <max_iters> <R> <seed> <cell_size> <lo>
// `run` prints one JSON object: per problem the result of runNapsac and of the C call
// usac_multi_run_napsac on the same context (floats as their int32 bit patterns), and the sizes of its
// grid (cells, eligible points, and a checksum of the members).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "usac_gpu.hpp"

namespace {

template <class T>
std::vector<T> read_file(const char *path, size_t count) {
    std::vector<T> v(count);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(sizeof(T) * count));
    if ((size_t)f.gcount() != sizeof(T) * count) throw std::runtime_error(std::string("short read: ") + path);
    return v;
}

int32_t bits(float x) {
    int32_t b;
    std::memcpy(&b, &x, sizeof(b));
    return b;
}

// one problem as a JSON object; l == NULL: no LO keys
std::string problem_json(const usac_multi_output &o, const usac_multi_lo_output *l) {
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
    if (l) {
        std::snprintf(buf, sizeof(buf),
                      ", \"lo\": {\"lo_calls\": %u, \"inner_iters\": %u, \"iterative_iters\": %u, \"fits\": %u, "
                      "\"improved\": %u, \"capped\": %u, \"draws\": %u, \"threshold\": %d}",
                      l->lo_calls, l->inner_iters, l->iterative_iters, l->fits, l->improved, l->capped, l->draws,
                      bits(l->threshold));
        s += buf;
    }
    return s + "}";
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            std::printf("{\"abi\": %d, \"header\": %d}\n", usac_abi_version(), USAC_ABI_VERSION);
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 13 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run est P pts offsets thr prob max_iters R seed cell_size lo\n");
            return 2;
        }
        const usac_gpu::ESTIMATOR est = (usac_gpu::ESTIMATOR)std::atoi(argv[2]);
        const uint32_t P = (uint32_t)std::atoi(argv[3]);
        const std::vector<uint32_t> offsets = read_file<uint32_t>(argv[5], (size_t)P + 1);
        const std::vector<float> pts = read_file<float>(argv[4], 4 * (size_t)offsets[P]);
        usac_gpu::Model model((float)std::atof(argv[6]), est == usac_gpu::Fundamental ? 7u : 4u,
                              (float)std::atof(argv[7]), 5, est, usac_gpu::Napsac);
        model.max_iterations = (unsigned int)std::atoi(argv[8]);
        model.batch = (uint32_t)std::atoi(argv[9]);
        model.seed = (uint32_t)std::atoi(argv[10]);
        model.setNeighborsType(usac_gpu::Grid);
        model.setCellSize(std::atoi(argv[11]));
        model.lo = (usac_gpu::LocOpt)std::atoi(argv[12]);
        model.lo_inner_iterations = 10;
        model.ResetRandomGenerator(false);
        const bool lo = model.lo != usac_gpu::NullLO;

        usac_gpu::MultiContext mc(est, pts.data(), offsets);
        const std::vector<usac_gpu::MultiContext::GridCsr> grid = mc.gridNeighbors(model.cell_size);
        const usac_gpu::MultiContext::Napsac res = mc.runNapsac(model);
        usac_params prm = model.params();
        prm.seed = model.seed;
        std::vector<usac_multi_output> out(P);
        std::vector<usac_multi_lo_output> los(P);
        mc.check(usac_multi_run_napsac(mc.get(), &prm, nullptr, out.data(), los.data(), nullptr, nullptr),
                 "usac_multi_run_napsac");

        std::printf("{\"problems\": [");
        for (unsigned int p = 0; p < mc.problems(); p++) {
            unsigned long long sum = 0;
            for (size_t i = 0; i < grid[p].members.size(); i++) sum += (unsigned long long)(i + 1) * (unsigned)grid[p].members[i];
            std::printf("%s{\"cpp\": %s, \"c\": %s, \"cells\": %u, \"eligible\": %u, \"members_sum\": %llu}", p ? ", " : "",
                        problem_json(res.run[p], lo ? &res.lo[p] : nullptr).c_str(),
                        problem_json(out[p], lo ? &los[p] : nullptr).c_str(), (unsigned)grid[p].start.size() - 1,
                        (unsigned)grid[p].eligible.size(), sum);
        }
        std::printf("]}\n");
        return 0;
    } catch (const usac_gpu::Error &e) {
        std::fprintf(stderr, "usac_gpu::Error %d: %s\n", e.code, e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
