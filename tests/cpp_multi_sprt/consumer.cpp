// A consumer of usac_gpu::MultiContext::runSprt (include/usac_gpu.hpp), C++11, no HIP headers:
//   consumer abi
//   consumer run <estimator> <P> <pts.f32> <offsets.u32> <thr> <prob> <max_iters> <R> <seed> <sampler>
// `run` prints one JSON object: per problem the result of runSprt and of the C call usac_multi_run_sprt on
// the same context (floats and doubles as their integer bit patterns).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "consumer_host.hpp"
#include "usac_gpu.hpp"

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            std::printf("{\"abi\": %d, \"header\": %d}\n", usac_abi_version(), USAC_ABI_VERSION);
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 12 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run est P pts offsets thr prob max_iters R seed sampler\n");
            return 2;
        }
        const usac_gpu::ESTIMATOR est = (usac_gpu::ESTIMATOR)std::atoi(argv[2]);
        const uint32_t P = (uint32_t)std::atoi(argv[3]);
        const std::vector<uint32_t> offsets = consumer_host::read_file<uint32_t>(argv[5], (size_t)P + 1);
        const std::vector<float> pts = consumer_host::read_file<float>(argv[4], 4 * (size_t)offsets[P]);
        const bool prosac = std::atoi(argv[11]) == (int)usac_gpu::Prosac;
        usac_gpu::Model model((float)std::atof(argv[6]), est == usac_gpu::Fundamental ? 7u : 4u,
                              (float)std::atof(argv[7]), 5, est, prosac ? usac_gpu::Prosac : usac_gpu::Uniform);
        model.max_iterations = (unsigned int)std::atoi(argv[8]);
        model.batch = (uint32_t)std::atoi(argv[9]);
        model.seed = (uint32_t)std::atoi(argv[10]);
        model.setSprt(true);
        model.ResetRandomGenerator(false);

        usac_gpu::MultiContext mc(est, pts.data(), offsets);
        mc.setSprtPool();
        const usac_gpu::MultiContext::Sprt res = mc.runSprt(model);
        usac_params prm = model.params();
        prm.seed = model.seed;
        std::vector<usac_multi_output> out(P);
        std::vector<usac_multi_sprt_output> sp(P);
        std::vector<usac_multi_prosac_output> pro(P);
        mc.check(usac_multi_run_sprt(mc.get(), &prm, nullptr, out.data(), sp.data(), pro.data(), nullptr, nullptr),
                 "usac_multi_run_sprt");

        std::printf("{\"problems\": [");
        for (unsigned int p = 0; p < mc.problems(); p++)
            std::printf("%s{\"cpp\": %s, \"c\": %s}", p ? ", " : "",
                        consumer_host::problem_json(res.run[p], res.sprt[p], prosac ? &res.prosac[p] : nullptr).c_str(),
                        consumer_host::problem_json(out[p], sp[p], prosac ? &pro[p] : nullptr).c_str());
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
