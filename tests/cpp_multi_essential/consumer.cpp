// A consumer of usac_gpu::MultiContext::essential (include/usac_gpu.hpp, ABI 21), C++11, no HIP headers:
//   consumer abi
//   consumer run <P> <pts.f32> <offsets.u32> <thr> <prob> <max_iters> <R> <seed>
// `run` prints one JSON object: per problem the run's record (floats as their int32 bit patterns),
// rounds, hypotheses, bound, status, the inlier count of the best model, and the first round's best;
// then whether the constructor still refuses the essential estimator.
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

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            std::printf("{\"abi\": %d, \"header\": %d}\n", usac_abi_version(), USAC_ABI_VERSION);
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 10 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run P pts offsets thr prob max_iters R seed\n");
            return 2;
        }
        const usac_gpu::ESTIMATOR est = usac_gpu::Essential;
        const uint32_t P = (uint32_t)std::atoi(argv[2]);
        const std::vector<uint32_t> offsets = read_file<uint32_t>(argv[4], (size_t)P + 1);
        const std::vector<float> pts = read_file<float>(argv[3], 4 * (size_t)offsets[P]);
        usac_gpu::Model model((float)std::atof(argv[5]), 5u, (float)std::atof(argv[6]), 5, est, usac_gpu::Uniform);
        model.max_iterations = (unsigned int)std::atoi(argv[7]);
        model.batch = (uint32_t)std::atoi(argv[8]);
        model.seed = (uint32_t)std::atoi(argv[9]);
        model.ResetRandomGenerator(false);

        int ctor_code = 0;  // the constructor keeps refusing the essential estimator
        try {
            usac_gpu::MultiContext refused(est, pts.data(), offsets);
        } catch (const usac_gpu::Error &e) {
            ctor_code = e.code;
        }
        usac_gpu::MultiContext mc = usac_gpu::MultiContext::essential(pts.data(), offsets);
        if (mc.sampleSize() != 5u || mc.modelSlots() != 1u) throw std::runtime_error("sampleSize / modelSlots");
        std::vector<uint64_t> seeds(mc.problems());
        for (unsigned int p = 0; p < mc.problems(); p++) seeds[p] = (uint64_t)model.seed + p;
        const usac_gpu::MultiContext::Round first = mc.hypothesizeScore(model.batch, seeds, 0, model.threshold);
        const std::vector<usac_multi_output> out = mc.run(model);
        std::vector<float> models(9 * (size_t)mc.problems());
        for (unsigned int p = 0; p < mc.problems(); p++) std::memcpy(&models[9 * p], out[p].best.model, sizeof(float) * 9);
        const std::vector<std::vector<int> > inl = mc.inliers(models.data(), model.threshold);

        std::printf("{\"problems\": [");
        for (unsigned int p = 0; p < mc.problems(); p++) {
            std::printf("%s{\"best\": ", p ? ", " : "");
            print_record(out[p].best);
            std::printf(", \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d, \"n_inliers\": %u, "
                        "\"first_round\": ",
                        out[p].rounds, out[p].hypotheses, out[p].bound, out[p].status, (unsigned)inl[p].size());
            print_record(first.best[p]);
            std::printf("}");
        }
        std::printf("], \"constructor_code\": %d}\n", ctor_code);
        return 0;
    } catch (const usac_gpu::Error &e) {
        std::fprintf(stderr, "usac_gpu::Error %d: %s\n", e.code, e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
