// A consumer of usac_gpu::MultiContext::runProsac (include/usac_gpu.hpp), C++11, no HIP headers:
//   consumer abi
//   consumer run <estimator> <P> <pts.f32> <offsets.u32> <thr> <prob> <max_iters> <R> <seed>
// `run` prints one JSON object: per problem the result of runProsac and of the C call
// usac_multi_run_prosac on the same context (floats as their int32 bit patterns).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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

void print_problem(const usac_multi_output &o, const usac_multi_prosac_output &q) {
    std::printf("{\"hyp_index\": %llu, \"inliers\": %d, \"score\": %d, \"valid\": %d, \"model\": [",
                (unsigned long long)o.best.hyp_index, o.best.inliers, bits(o.best.score), o.best.valid);
    for (int k = 0; k < 9; k++) std::printf("%s%d", k ? ", " : "", bits(o.best.model[k]));
    std::printf("], \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d, \"termination_length\": %u, "
                "\"largest_sample_size\": %u, \"clock\": %u, \"scans\": %u}",
                o.rounds, o.hypotheses, o.bound, o.status, q.termination_length, q.largest_sample_size, q.clock,
                q.scans);
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            std::printf("{\"abi\": %d, \"header\": %d}\n", usac_abi_version(), USAC_ABI_VERSION);
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 11 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run est P pts offsets thr prob max_iters R seed\n");
            return 2;
        }
        const usac_gpu::ESTIMATOR est = (usac_gpu::ESTIMATOR)std::atoi(argv[2]);
        const uint32_t P = (uint32_t)std::atoi(argv[3]);
        const std::vector<uint32_t> offsets = read_file<uint32_t>(argv[5], (size_t)P + 1);
        const std::vector<float> pts = read_file<float>(argv[4], 4 * (size_t)offsets[P]);
        usac_gpu::Model model((float)std::atof(argv[6]), est == usac_gpu::Fundamental ? 7u : 4u,
                              (float)std::atof(argv[7]), 5, est, usac_gpu::Prosac);
        model.max_iterations = (unsigned int)std::atoi(argv[8]);
        model.batch = (uint32_t)std::atoi(argv[9]);
        model.seed = (uint32_t)std::atoi(argv[10]);
        model.ResetRandomGenerator(false);

        usac_gpu::MultiContext mc(est, pts.data(), offsets);
        const usac_gpu::MultiContext::Prosac res = mc.runProsac(model);
        usac_params prm = model.params();
        prm.seed = model.seed;
        std::vector<usac_multi_output> out(P);
        std::vector<usac_multi_prosac_output> pro(P);
        mc.check(usac_multi_run_prosac(mc.get(), &prm, nullptr, out.data(), pro.data(), nullptr, nullptr),
                 "usac_multi_run_prosac");

        std::printf("{\"problems\": [");
        for (unsigned int p = 0; p < mc.problems(); p++) {
            std::printf("%s{\"cpp\": ", p ? ", " : "");
            print_problem(res.run[p], res.prosac[p]);
            std::printf(", \"c\": ");
            print_problem(out[p], pro[p]);
            std::printf("}");
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
