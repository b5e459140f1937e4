// A consumer of usac_gpu::MultiContext::runLoEssential / loEssential (include/usac_gpu.hpp, ABI 23), C++11,
// no HIP headers:
//   consumer abi
//   consumer run <P> <pts.f32> <offsets.u32> <thr> <prob> <max_iters> <R> <seed> <sampler> <lo>
// `run` prints one JSON object: per problem the result of runLoEssential, of the C call
// usac_multi_run_lo_essential on the same context, and of one more loEssential() call on the run's records
// (floats as their int32 bit patterns); then the codes with which runLo() and lo() refuse the context.
// The host-only part (file reading, one problem's JSON) is tests/cpp_multi_lo/consumer_host.hpp, which
// that directory's lo_draw_check.cpp runs under the sanitizers.
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
            std::fprintf(stderr, "usage: consumer abi | run P pts offsets thr prob max_iters R seed sampler lo\n");
            return 2;
        }
        const uint32_t P = (uint32_t)std::atoi(argv[2]);
        const std::vector<uint32_t> offsets = consumer_host::read_file<uint32_t>(argv[4], (size_t)P + 1);
        const std::vector<float> pts = consumer_host::read_file<float>(argv[3], 4 * (size_t)offsets[P]);
        const bool prosac = std::atoi(argv[10]) == (int)usac_gpu::Prosac;
        usac_gpu::Model model((float)std::atof(argv[5]), 5u, (float)std::atof(argv[6]), 5, usac_gpu::Essential,
                              prosac ? usac_gpu::Prosac : usac_gpu::Uniform);
        model.max_iterations = (unsigned int)std::atoi(argv[7]);
        model.batch = (uint32_t)std::atoi(argv[8]);
        model.seed = (uint32_t)std::atoi(argv[9]);
        model.lo = (usac_gpu::LocOpt)std::atoi(argv[11]);
        model.lo_inner_iterations = 10;
        model.ResetRandomGenerator(false);

        usac_gpu::MultiContext mc = usac_gpu::MultiContext::essential(pts.data(), offsets);
        const usac_gpu::MultiContext::Lo res = mc.runLoEssential(model);
        usac_params prm = model.params();
        prm.seed = model.seed;
        std::vector<usac_multi_output> out(P);
        std::vector<usac_multi_lo_output> lo(P);
        std::vector<usac_multi_prosac_output> pro(P);
        mc.check(usac_multi_run_lo_essential(mc.get(), &prm, nullptr, out.data(), lo.data(), pro.data(), nullptr, nullptr),
                 "usac_multi_run_lo_essential");
        // one more LO call on the run's records, through the hook
        std::vector<usac_record> recs(P);
        for (uint32_t p = 0; p < P; p++) recs[p] = res.run[p].best;
        const std::vector<usac_multi_lo_output> hook = mc.loEssential(model, recs);
        // the H / F entries keep refusing the context
        int run_lo_code = 0, lo_code = 0;
        try {
            mc.runLo(model);
        } catch (const usac_gpu::Error &e) {
            run_lo_code = e.code;
        }
        try {
            std::vector<usac_record> again = recs;
            mc.lo(model, again);
        } catch (const usac_gpu::Error &e) {
            lo_code = e.code;
        }

        std::printf("{\"problems\": [");
        for (unsigned int p = 0; p < mc.problems(); p++) {
            usac_multi_output again = res.run[p];
            again.best = recs[p];
            std::printf("%s{\"cpp\": %s, \"c\": %s, \"hook\": %s}", p ? ", " : "",
                        consumer_host::problem_json(res.run[p], res.lo[p], prosac ? &res.prosac[p] : nullptr).c_str(),
                        consumer_host::problem_json(out[p], lo[p], prosac ? &pro[p] : nullptr).c_str(),
                        consumer_host::problem_json(again, hook[p], nullptr).c_str());
        }
        std::printf("], \"run_lo_code\": %d, \"lo_code\": %d}\n", run_lo_code, lo_code);
        return 0;
    } catch (const usac_gpu::Error &e) {
        std::fprintf(stderr, "usac_gpu::Error %d: %s\n", e.code, e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
