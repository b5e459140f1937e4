// A consumer of usac_gpu::MultiContext::fromDeviceSorted (include/usac_gpu.hpp, ABI 26), C++11, built with hipcc
// because it allocates the device memory it hands over:
//   consumer abi
//   consumer run <estimator> <P> <n_max> <rows.f32> <valid.u8> <scores.f32> <descending> <thr> <prob> <max_iters> <R> <seed>
// `abi` needs no GPU: the ABI numbers of the library and the header, and the size and field offsets of
// usac_multi_device_order.  rows.f32: P x n_max x 4 floats; valid.u8: P x n_max bytes; scores.f32: P x n_max floats.
// `run` uploads the three, creates the context from the device pointers in quality order and prints one JSON
// object: the packed rows (floats as their int32 bit patterns), the offsets, the source columns, per problem
// runProsac's record, rounds, hypotheses, bound, status and PROSAC state and the polish of its best model, and the
// P x n_max bytes paddedMask wrote for the polished inliers.
#include <hip/hip_runtime_api.h>

#include <cstddef>
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

template <class T>
void print_uints(const T *m, size_t n) {
    std::printf("[");
    for (size_t k = 0; k < n; k++) std::printf("%s%u", k ? ", " : "", (unsigned)m[k]);
    std::printf("]");
}

void hip_ok(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// device memory holding a copy of a host vector
template <class T>
struct Uploaded {
    T *p = nullptr;
    explicit Uploaded(const std::vector<T> &v) {
        hip_ok(hipMalloc(reinterpret_cast<void **>(&p), sizeof(T) * v.size()), "hipMalloc");
        hip_ok(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice), "hipMemcpy");
    }
    ~Uploaded() { (void)hipFree(p); }
    Uploaded(const Uploaded &) = delete;
    Uploaded &operator=(const Uploaded &) = delete;
};

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            typedef usac_multi_device_order Order;
            std::printf("{\"abi\": %d, \"header\": %d, \"sizeof\": %u, \"offsets\": {\"scores\": %u, \"descending\": %u}}\n",
                        usac_abi_version(), USAC_ABI_VERSION, (unsigned)sizeof(Order), (unsigned)offsetof(Order, scores),
                        (unsigned)offsetof(Order, descending));
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 14 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run estimator P n_max rows valid scores descending thr prob "
                                 "max_iters R seed\n");
            return 2;
        }
        const int est = std::atoi(argv[2]);
        const uint32_t P = (uint32_t)std::atoi(argv[3]), n_max = (uint32_t)std::atoi(argv[4]);
        const size_t cells = (size_t)P * n_max;
        const std::vector<float> rows = read_file<float>(argv[5], 4 * cells);
        const std::vector<uint8_t> valid = read_file<uint8_t>(argv[6], cells);
        const std::vector<float> scores = read_file<float>(argv[7], cells);
        const float thr = (float)std::atof(argv[9]);
        const unsigned int m = est == USAC_FUNDAMENTAL ? 7u : est == USAC_ESSENTIAL ? 5u : 4u;
        usac_gpu::Model model(thr, m, (float)std::atof(argv[10]), 5, (usac_gpu::ESTIMATOR)est, usac_gpu::Prosac);
        model.max_iterations = (unsigned int)std::atoi(argv[11]);
        model.batch = (uint32_t)std::atoi(argv[12]);
        model.seed = (uint32_t)std::atoi(argv[13]);
        model.ResetRandomGenerator(false);

        hip_ok(hipSetDevice(0), "hipSetDevice");
        Uploaded<float> d_rows(rows);
        Uploaded<uint8_t> d_valid(valid);
        Uploaded<float> d_scores(scores);
        Uploaded<uint8_t> d_out(std::vector<uint8_t>(cells, 0xff));  // paddedMask must clear what it does not set
        usac_multi_device_input in;
        std::memset(&in, 0, sizeof(in));
        in.P = P;
        in.n_max = n_max;
        in.rows = d_rows.p;
        in.valid = d_valid.p;
        usac_multi_device_order order;
        order.scores = d_scores.p;
        order.descending = std::atoi(argv[8]);
        usac_gpu::MultiContext mc = usac_gpu::MultiContext::fromDeviceSorted(est, in, order);
        const std::vector<float> pts = mc.points();
        const std::vector<uint32_t> &offsets = mc.offsets();
        const std::vector<uint32_t> src = mc.source();
        const usac_gpu::MultiContext::Prosac res = mc.runProsac(model);
        std::vector<float> models(9 * (size_t)P);
        for (uint32_t p = 0; p < P; p++) std::memcpy(&models[9 * (size_t)p], res.run[p].best.model, sizeof(float) * 9);
        std::vector<std::vector<int> > inliers;
        const std::vector<usac_multi_polish_output> polished = mc.polish(models.data(), thr, &inliers);
        std::vector<uint8_t> mask(offsets[P], 0);
        for (uint32_t p = 0; p < P; p++)
            for (size_t k = 0; k < inliers[p].size(); k++) mask[offsets[p] + (uint32_t)inliers[p][k]] = 1;
        mc.paddedMask(mask, d_out.p);
        std::vector<uint8_t> padded(cells);
        hip_ok(hipMemcpy(padded.data(), d_out.p, cells, hipMemcpyDeviceToHost), "hipMemcpy mask");

        std::printf("{\"n_max\": %u, \"points\": ", mc.paddedWidth());
        print_floats(pts.data(), pts.size());
        std::printf(", \"offsets\": ");
        print_uints(offsets.data(), offsets.size());
        std::printf(", \"source\": ");
        print_uints(src.data(), src.size());
        std::printf(", \"padded_mask\": ");
        print_uints(padded.data(), padded.size());
        std::printf(", \"problems\": [");
        for (uint32_t p = 0; p < P; p++) {
            const usac_multi_output &o = res.run[p];
            const usac_multi_polish_output &q = polished[p];
            const usac_multi_prosac_output &g = res.prosac[p];
            std::printf("%s{\"best\": {\"hyp_index\": %llu, \"inliers\": %d, \"score\": %d, \"valid\": %d, \"model\": ",
                        p ? ", " : "", (unsigned long long)o.best.hyp_index, o.best.inliers, bits(o.best.score), o.best.valid);
            print_floats(o.best.model, 9);
            std::printf("}, \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d, \"polished\": {\"model\": ",
                        o.rounds, o.hypotheses, o.bound, o.status);
            print_floats(q.model, 9);
            std::printf(", \"inliers\": %d, \"score\": %d, \"passes\": %d, \"status\": %d}, \"prosac\": {"
                        "\"termination_length\": %u, \"largest_sample_size\": %u, \"clock\": %u, \"scans\": %u}}",
                        q.inliers, bits(q.score), q.passes, q.status, g.termination_length, g.largest_sample_size,
                        g.clock, g.scans);
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
