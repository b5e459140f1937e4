// A consumer of usac_gpu::MultiContext::runPolished / polish (include/usac_gpu.hpp), C++11, no HIP
// headers:
//   consumer_multi_polish abi
//   consumer_multi_polish run <estimator> <P> <pts.f32> <offsets.u32> <thr> <prob> <max_iters> <R> <seed>
// `run` prints one JSON object: per problem the run's best record, the polished result (floats as
// their int32 bit patterns), the polished model's inliers, and polish() of the run's best models.
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

void print_record(const usac_record &r) {
    std::printf("{\"hyp_index\": %llu, \"inliers\": %d, \"score\": %d, \"valid\": %d, \"model\": [",
                (unsigned long long)r.hyp_index, r.inliers, bits(r.score), r.valid);
    for (int k = 0; k < 9; k++) std::printf("%s%d", k ? ", " : "", bits(r.model[k]));
    std::printf("]}");
}

void print_polished(const usac_multi_polish_output &o) {
    std::printf("{\"inliers\": %d, \"score\": %d, \"minimal_inliers\": %d, \"minimal_score\": %d, \"passes\": %d, "
                "\"status\": %d, \"model\": [",
                o.inliers, bits(o.score), o.minimal_inliers, bits(o.minimal_score), o.passes, o.status);
    for (int k = 0; k < 9; k++) std::printf("%s%d", k ? ", " : "", bits(o.model[k]));
    std::printf("]}");
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            std::printf("{\"abi\": %d, \"header\": %d}\n", usac_abi_version(), USAC_ABI_VERSION);
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 11 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer_multi_polish abi | run est P pts offsets thr prob max_iters R seed\n");
            return 2;
        }
        const usac_gpu::ESTIMATOR est = (usac_gpu::ESTIMATOR)std::atoi(argv[2]);
        const uint32_t P = (uint32_t)std::atoi(argv[3]);
        const std::vector<uint32_t> offsets = read_file<uint32_t>(argv[5], (size_t)P + 1);
        const std::vector<float> pts = read_file<float>(argv[4], 4 * (size_t)offsets[P]);
        usac_gpu::Model model((float)std::atof(argv[6]), est == usac_gpu::Fundamental ? 7u : 4u,
                              (float)std::atof(argv[7]), 5, est, usac_gpu::Uniform);
        model.max_iterations = (unsigned int)std::atoi(argv[8]);
        model.batch = (uint32_t)std::atoi(argv[9]);
        model.seed = (uint32_t)std::atoi(argv[10]);
        model.ResetRandomGenerator(false);

        usac_gpu::MultiContext mc(est, pts.data(), offsets);
        const usac_gpu::MultiContext::Polished res = mc.runPolished(model);
        std::vector<float> models(9 * (size_t)mc.problems());
        for (unsigned int p = 0; p < mc.problems(); p++)
            std::memcpy(&models[9 * p], res.run[p].best.model, sizeof(float) * 9);
        std::vector<std::vector<int> > inl;
        const std::vector<usac_multi_polish_output> again = mc.polish(models.data(), model.threshold, &inl);

        std::printf("{\"problems\": [");
        for (unsigned int p = 0; p < mc.problems(); p++) {
            std::printf("%s{\"best\": ", p ? ", " : "");
            print_record(res.run[p].best);
            std::printf(", \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d, \"polished\": ",
                        res.run[p].rounds, res.run[p].hypotheses, res.run[p].bound, res.run[p].status);
            print_polished(res.polished[p]);
            std::printf(", \"polish_again\": ");
            print_polished(again[p]);
            std::printf(", \"inliers\": [");
            for (size_t i = 0; i < res.inliers[p].size(); i++) std::printf("%s%d", i ? ", " : "", res.inliers[p][i]);
            std::printf("], \"inliers_again\": [");
            for (size_t i = 0; i < inl[p].size(); i++) std::printf("%s%d", i ? ", " : "", inl[p][i]);
            std::printf("]}");
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
