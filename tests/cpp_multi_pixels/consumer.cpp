// A consumer of usac_gpu::MultiContext::essentialPixels / setPixelThresholds / pixelModels / points
// (include/usac_gpu.hpp, ABI 24), C++11, no HIP headers:
//   consumer abi
//   consumer run <P> <px.f32> <offsets.u32> <K1.f32> <K2.f32 | -> <t_px.f32> <n_t> <prob> <max_iters> <R> <seed>
// px.f32: N_total pixel rows; K1 / K2: P x 9 intrinsics ("-": K1 for both views); t_px.f32: n_t (1 or P) pixel
// tolerances.  `run` prints one JSON object: the calibrated rows and the thresholds read back (floats as their
// int32 bit patterns), per problem runPolished's record, rounds, hypotheses, bound, status, the polish and the
// pixel-space model of the polished model; then the codes setPixelThresholds and pixelModels raise on a context
// from essential(), and the code a bad tolerance raises.
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

void print_floats(const float *m, size_t n) {
    std::printf("[");
    for (size_t k = 0; k < n; k++) std::printf("%s%d", k ? ", " : "", bits(m[k]));
    std::printf("]");
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            std::printf("{\"abi\": %d, \"header\": %d}\n", usac_abi_version(), USAC_ABI_VERSION);
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 13 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run P px offsets K1 K2|- t_px n_t prob max_iters R seed\n");
            return 2;
        }
        const uint32_t P = (uint32_t)std::atoi(argv[2]);
        const std::vector<uint32_t> offsets = read_file<uint32_t>(argv[4], (size_t)P + 1);
        const std::vector<float> px = read_file<float>(argv[3], 4 * (size_t)offsets[P]);
        const std::vector<float> K1 = read_file<float>(argv[5], 9 * (size_t)P);
        const std::vector<float> K2 = std::strcmp(argv[6], "-") ? read_file<float>(argv[6], 9 * (size_t)P) : std::vector<float>();
        const std::vector<float> t_px = read_file<float>(argv[7], (size_t)std::atoi(argv[8]));
        usac_gpu::Model model(1.f, 5u, (float)std::atof(argv[9]), 5, usac_gpu::Essential, usac_gpu::Uniform);
        model.max_iterations = (unsigned int)std::atoi(argv[10]);
        model.batch = (uint32_t)std::atoi(argv[11]);
        model.seed = (uint32_t)std::atoi(argv[12]);
        model.ResetRandomGenerator(false);

        usac_gpu::MultiContext mc = usac_gpu::MultiContext::essentialPixels(px.data(), offsets, K1, K2);
        const std::vector<float> rows = mc.points();
        int bad_code = 0;
        try {
            mc.setPixelThresholds(-1.f);
        } catch (const usac_gpu::Error &e) {
            bad_code = e.code;
        }
        if (!mc.thresholds().empty()) throw std::runtime_error("a refused tolerance left thresholds behind");
        if (t_px.size() == 1) mc.setPixelThresholds(t_px[0]);
        else mc.setPixelThresholds(t_px);
        const std::vector<float> thr = mc.thresholds();
        const usac_gpu::MultiContext::Polished res = mc.runPolished(model);  // the model's threshold is not read
        std::vector<float> E(9 * (size_t)P);
        for (uint32_t p = 0; p < P; p++) std::memcpy(&E[9 * p], res.polished[p].model, sizeof(float) * 9);
        const std::vector<float> F = mc.pixelModels(E);

        int set_code = 0, models_code = 0;  // a context from calibrated rows refuses both
        {
            usac_gpu::MultiContext plain = usac_gpu::MultiContext::essential(rows.data(), offsets);
            try {
                plain.setPixelThresholds(1.f);
            } catch (const usac_gpu::Error &e) {
                set_code = e.code;
            }
            try {
                plain.pixelModels(E);
            } catch (const usac_gpu::Error &e) {
                models_code = e.code;
            }
        }

        std::printf("{\"points\": ");
        print_floats(rows.data(), rows.size());
        std::printf(", \"thresholds\": ");
        print_floats(thr.data(), thr.size());
        std::printf(", \"problems\": [");
        for (uint32_t p = 0; p < P; p++) {
            const usac_multi_output &o = res.run[p];
            const usac_multi_polish_output &q = res.polished[p];
            std::printf("%s{\"best\": {\"hyp_index\": %llu, \"inliers\": %d, \"score\": %d, \"valid\": %d, \"model\": ",
                        p ? ", " : "", (unsigned long long)o.best.hyp_index, o.best.inliers, bits(o.best.score), o.best.valid);
            print_floats(o.best.model, 9);
            std::printf("}, \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d, \"polished\": {\"model\": ",
                        o.rounds, o.hypotheses, o.bound, o.status);
            print_floats(q.model, 9);
            std::printf(", \"inliers\": %d, \"score\": %d, \"passes\": %d, \"status\": %d, \"n_mask\": %u}, \"pixel_model\": ",
                        q.inliers, bits(q.score), q.passes, q.status, (unsigned)res.inliers[p].size());
            print_floats(&F[9 * p], 9);
            std::printf("}");
        }
        std::printf("], \"bad_tolerance_code\": %d, \"plain_set_code\": %d, \"plain_models_code\": %d}\n", bad_code, set_code,
                    models_code);
        return 0;
    } catch (const usac_gpu::Error &e) {
        std::fprintf(stderr, "usac_gpu::Error %d: %s\n", e.code, e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
