// A consumer of usac_gpu::MultiContext::set_thresholds / clear_thresholds / thresholds
// (include/usac_gpu.hpp, ABI 22), C++11, no HIP headers:
//   consumer abi
//   consumer run <est> <P> <pts.f32> <offsets.u32> <thr.f32> <scalar> <prob> <max_iters> <R> <seed>
// est 2 (homography): runLo under the P thresholds of thr.f32; est 4 (essential): run and the polish of
// its best models.  `scalar` is the model's own threshold, which the calls must not read.  `run` prints
// one JSON object: the thresholds read back, per problem the run's record (floats as their int32 bit
// patterns), rounds, hypotheses, bound, status and the LO threshold (H) or the polish (E); then whether
// thresholds() is empty after clear_thresholds() and the code a bad length raises.
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

void print_model(const float *m) {
    std::printf("[");
    for (int k = 0; k < 9; k++) std::printf("%s%d", k ? ", " : "", bits(m[k]));
    std::printf("]");
}

void print_record(const usac_record &r) {
    std::printf("{\"hyp_index\": %llu, \"inliers\": %d, \"score\": %d, \"valid\": %d, \"model\": ",
                (unsigned long long)r.hyp_index, r.inliers, bits(r.score), r.valid);
    print_model(r.model);
    std::printf("}");
}

void print_run(const usac_multi_output &o) {
    std::printf("\"best\": ");
    print_record(o.best);
    std::printf(", \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d", o.rounds, o.hypotheses, o.bound,
                o.status);
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            std::printf("{\"abi\": %d, \"header\": %d}\n", usac_abi_version(), USAC_ABI_VERSION);
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 12 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run est P pts offsets thr scalar prob max_iters R seed\n");
            return 2;
        }
        const usac_gpu::ESTIMATOR est = (usac_gpu::ESTIMATOR)std::atoi(argv[2]);
        if (est != usac_gpu::Homography && est != usac_gpu::Essential) throw std::runtime_error("est: 2 or 4");
        const bool ess = est == usac_gpu::Essential;
        const uint32_t P = (uint32_t)std::atoi(argv[3]);
        const std::vector<uint32_t> offsets = read_file<uint32_t>(argv[5], (size_t)P + 1);
        const std::vector<float> pts = read_file<float>(argv[4], 4 * (size_t)offsets[P]);
        const std::vector<float> thr = read_file<float>(argv[6], P);
        usac_gpu::Model model((float)std::atof(argv[7]), ess ? 5u : 4u, (float)std::atof(argv[8]), 5, est,
                              usac_gpu::Uniform);
        model.max_iterations = (unsigned int)std::atoi(argv[9]);
        model.batch = (uint32_t)std::atoi(argv[10]);
        model.seed = (uint32_t)std::atoi(argv[11]);
        model.ResetRandomGenerator(false);

        usac_gpu::MultiContext mc = ess ? usac_gpu::MultiContext::essential(pts.data(), offsets)
                                        : usac_gpu::MultiContext(est, pts.data(), offsets);
        if (!mc.thresholds().empty()) throw std::runtime_error("a fresh context has thresholds");
        int bad_length_code = 0;
        try {
            mc.set_thresholds(std::vector<float>(P + 1, 1.f));
        } catch (const usac_gpu::Error &e) {
            bad_length_code = e.code;
        }
        mc.set_thresholds(thr);
        const std::vector<float> back = mc.thresholds();
        std::printf("{\"thresholds\": [");
        for (size_t p = 0; p < back.size(); p++) std::printf("%s%d", p ? ", " : "", bits(back[p]));
        std::printf("], \"problems\": [");
        if (ess) {
            const std::vector<usac_multi_output> out = mc.run(model);
            std::vector<float> models(9 * (size_t)P);
            for (uint32_t p = 0; p < P; p++) std::memcpy(&models[9 * p], out[p].best.model, sizeof(float) * 9);
            std::vector<std::vector<int> > inl;
            const std::vector<usac_multi_polish_output> pol = mc.polish(models.data(), model.threshold, &inl);
            for (uint32_t p = 0; p < P; p++) {
                std::printf("%s{", p ? ", " : "");
                print_run(out[p]);
                std::printf(", \"polished\": {\"model\": ");
                print_model(pol[p].model);
                std::printf(", \"inliers\": %d, \"score\": %d, \"passes\": %d, \"status\": %d, \"n_mask\": %u}}",
                            pol[p].inliers, bits(pol[p].score), pol[p].passes, pol[p].status, (unsigned)inl[p].size());
            }
        } else {
            model.lo = usac_gpu::InItLORsc;
            model.lo_inner_iterations = 10;
            const usac_gpu::MultiContext::Lo res = mc.runLo(model);
            for (uint32_t p = 0; p < P; p++) {
                std::printf("%s{", p ? ", " : "");
                print_run(res.run[p]);
                std::printf(", \"lo_calls\": %u, \"fits\": %u, \"lo_threshold\": %d}", res.lo[p].lo_calls, res.lo[p].fits,
                            bits(res.lo[p].threshold));
            }
        }
        mc.clear_thresholds();
        std::printf("], \"cleared\": %s, \"bad_length_code\": %d}\n", mc.thresholds().empty() ? "true" : "false",
                    bad_length_code);
        return 0;
    } catch (const usac_gpu::Error &e) {
        std::fprintf(stderr, "usac_gpu::Error %d: %s\n", e.code, e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
