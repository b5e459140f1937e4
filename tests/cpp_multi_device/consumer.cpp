// A consumer of usac_gpu::MultiContext::fromDevice / source / paddedMask (include/usac_gpu.hpp, ABI 25), C++11,
// built with hipcc because it allocates the device memory it hands over:
//   consumer abi
//   consumer run <estimator> <P> <n_max> <rows.f32> <valid.u8> <thr> <prob> <max_iters> <R> <seed>
// `abi` needs no GPU: the ABI numbers of the library and the header, and the size and field offsets of
// usac_multi_device_input.  rows.f32: P x n_max x 4 floats; valid.u8: P x n_max bytes.  `run` uploads both, creates
// the context from the device pointers and prints one JSON object: the packed rows (floats as their int32 bit
// patterns), the offsets, the source columns, per problem runPolished's record, rounds, hypotheses, bound, status
// and the polish, and the P x n_max bytes paddedMask wrote for the polished inliers.
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
            typedef usac_multi_device_input In;
            std::printf("{\"abi\": %d, \"header\": %d, \"sizeof\": %u, \"offsets\": {\"P\": %u, \"n_max\": %u, \"rows\": %u, "
                        "\"valid\": %u, \"counts\": %u, \"kpts0\": %u, \"kpts1\": %u, \"n1\": %u, \"match\": %u, \"K1\": %u, "
                        "\"K2\": %u, \"stream\": %u}}\n",
                        usac_abi_version(), USAC_ABI_VERSION, (unsigned)sizeof(In), (unsigned)offsetof(In, P),
                        (unsigned)offsetof(In, n_max), (unsigned)offsetof(In, rows), (unsigned)offsetof(In, valid),
                        (unsigned)offsetof(In, counts), (unsigned)offsetof(In, kpts0), (unsigned)offsetof(In, kpts1),
                        (unsigned)offsetof(In, n1), (unsigned)offsetof(In, match), (unsigned)offsetof(In, K1),
                        (unsigned)offsetof(In, K2), (unsigned)offsetof(In, stream));
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 12 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run estimator P n_max rows valid thr prob max_iters R seed\n");
            return 2;
        }
        const int est = std::atoi(argv[2]);
        const uint32_t P = (uint32_t)std::atoi(argv[3]), n_max = (uint32_t)std::atoi(argv[4]);
        const size_t cells = (size_t)P * n_max;
        const std::vector<float> rows = read_file<float>(argv[5], 4 * cells);
        const std::vector<uint8_t> valid = read_file<uint8_t>(argv[6], cells);
        const unsigned int m = est == USAC_FUNDAMENTAL ? 7u : est == USAC_ESSENTIAL ? 5u : 4u;
        usac_gpu::Model model((float)std::atof(argv[7]), m, (float)std::atof(argv[8]), 5, (usac_gpu::ESTIMATOR)est,
                              usac_gpu::Uniform);
        model.max_iterations = (unsigned int)std::atoi(argv[9]);
        model.batch = (uint32_t)std::atoi(argv[10]);
        model.seed = (uint32_t)std::atoi(argv[11]);
        model.ResetRandomGenerator(false);

        hip_ok(hipSetDevice(0), "hipSetDevice");
        Uploaded<float> d_rows(rows);
        Uploaded<uint8_t> d_valid(valid);
        Uploaded<uint8_t> d_out(std::vector<uint8_t>(cells, 0xff));  // paddedMask must clear what it does not set
        usac_multi_device_input in;
        std::memset(&in, 0, sizeof(in));
        in.P = P;
        in.n_max = n_max;
        in.rows = d_rows.p;
        in.valid = d_valid.p;
        usac_gpu::MultiContext mc = usac_gpu::MultiContext::fromDevice(est, in);
        const std::vector<float> pts = mc.points();
        const std::vector<uint32_t> &offsets = mc.offsets();
        const std::vector<uint32_t> src = mc.source();
        const usac_gpu::MultiContext::Polished res = mc.runPolished(model);
        std::vector<uint8_t> mask(offsets[P], 0);
        for (uint32_t p = 0; p < P; p++)
            for (size_t k = 0; k < res.inliers[p].size(); k++) mask[offsets[p] + (uint32_t)res.inliers[p][k]] = 1;
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
            const usac_multi_polish_output &q = res.polished[p];
            std::printf("%s{\"best\": {\"hyp_index\": %llu, \"inliers\": %d, \"score\": %d, \"valid\": %d, \"model\": ",
                        p ? ", " : "", (unsigned long long)o.best.hyp_index, o.best.inliers, bits(o.best.score), o.best.valid);
            print_floats(o.best.model, 9);
            std::printf("}, \"rounds\": %u, \"hypotheses\": %u, \"bound\": %u, \"status\": %d, \"polished\": {\"model\": ",
                        o.rounds, o.hypotheses, o.bound, o.status);
            print_floats(q.model, 9);
            std::printf(", \"inliers\": %d, \"score\": %d, \"passes\": %d, \"status\": %d}}", q.inliers, bits(q.score),
                        q.passes, q.status);
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
