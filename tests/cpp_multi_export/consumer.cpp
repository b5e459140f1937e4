// A consumer of usac_gpu::MultiContext::setResident / exportDevice (include/usac_gpu.hpp, ABI 27), C++11, built
// with hipcc because it allocates the device memory it hands over:
//   consumer abi
//   consumer run <P> <n_max> <rows.f32> <valid.u8> <thr> <prob> <max_iters> <R> <seed> <k_max>
// `abi` needs no GPU: the ABI numbers of the library and the header, and the size and field offsets of
// usac_multi_device_output.  `run` uploads the padded homography rows (P x n_max x 4 floats) and their keep mask
// (P x n_max bytes), creates the context from the device pointers, runs runPolished and exports its result into
// device memory filled with 0xFF bytes; then the same in resident mode.  It prints one JSON object: what the
// export wrote (floats as their int32 bit patterns), and whether the resident-mode export wrote the same bytes.
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

template <class T>
void print_ints(const T *m, size_t n) {
    std::printf("[");
    for (size_t k = 0; k < n; k++) std::printf("%s%d", k ? ", " : "", (int)m[k]);
    std::printf("]");
}

void hip_ok(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// device memory holding a copy of a host vector
template <class T>
struct Uploaded {
    T *p = nullptr;
    size_t n;
    explicit Uploaded(const std::vector<T> &v) : n(v.size()) {
        hip_ok(hipMalloc(reinterpret_cast<void **>(&p), sizeof(T) * n), "hipMalloc");
        hip_ok(hipMemcpy(p, v.data(), sizeof(T) * n, hipMemcpyHostToDevice), "hipMemcpy");
    }
    ~Uploaded() { (void)hipFree(p); }
    Uploaded(const Uploaded &) = delete;
    Uploaded &operator=(const Uploaded &) = delete;
    std::vector<T> down() const {
        std::vector<T> v(n);
        hip_ok(hipMemcpy(v.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost), "hipMemcpy down");
        return v;
    }
};

// the six outputs of one export, every byte 0xFF before it
struct Outputs {
    Uploaded<int32_t> models, inliers, status, cols;  // the models as their bit patterns
    Uploaded<uint8_t> mask;
    Outputs(uint32_t P, uint32_t n_max, uint32_t k_max)
        : models(std::vector<int32_t>(9 * (size_t)P, -1)), inliers(std::vector<int32_t>(P, -1)),
          status(std::vector<int32_t>(P, -1)), cols(std::vector<int32_t>((size_t)P * k_max, -1)),
          mask(std::vector<uint8_t>((size_t)P * n_max, 0xff)) {}
    usac_multi_device_output view(uint32_t n_max, uint32_t k_max) const {
        usac_multi_device_output o;
        std::memset(&o, 0, sizeof(o));
        o.n_max = n_max;
        o.k_max = k_max;
        o.models = reinterpret_cast<float *>(models.p);
        o.inliers = inliers.p;
        o.status = status.p;
        o.mask = mask.p;
        o.inlier_cols = cols.p;
        return o;
    }
};

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            typedef usac_multi_device_output Out;
            std::printf("{\"abi\": %d, \"header\": %d, \"sizeof\": %u, \"offsets\": {\"n_max\": %u, \"k_max\": %u, "
                        "\"models\": %u, \"pixel_models\": %u, \"inliers\": %u, \"status\": %u, \"mask\": %u, "
                        "\"inlier_cols\": %u, \"stream\": %u}}\n",
                        usac_abi_version(), USAC_ABI_VERSION, (unsigned)sizeof(Out), (unsigned)offsetof(Out, n_max),
                        (unsigned)offsetof(Out, k_max), (unsigned)offsetof(Out, models),
                        (unsigned)offsetof(Out, pixel_models), (unsigned)offsetof(Out, inliers),
                        (unsigned)offsetof(Out, status), (unsigned)offsetof(Out, mask),
                        (unsigned)offsetof(Out, inlier_cols), (unsigned)offsetof(Out, stream));
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 12 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run P n_max rows valid thr prob max_iters R seed k_max\n");
            return 2;
        }
        const uint32_t P = (uint32_t)std::atoi(argv[2]), n_max = (uint32_t)std::atoi(argv[3]);
        const uint32_t k_max = (uint32_t)std::atoi(argv[11]);
        const size_t cells = (size_t)P * n_max;
        const std::vector<float> rows = read_file<float>(argv[4], 4 * cells);
        const std::vector<uint8_t> valid = read_file<uint8_t>(argv[5], cells);
        usac_gpu::Model model((float)std::atof(argv[6]), 4u, (float)std::atof(argv[7]), 5, usac_gpu::Homography,
                              usac_gpu::Uniform);
        model.max_iterations = (unsigned int)std::atoi(argv[8]);
        model.batch = (uint32_t)std::atoi(argv[9]);
        model.seed = (uint32_t)std::atoi(argv[10]);
        model.ResetRandomGenerator(false);

        hip_ok(hipSetDevice(0), "hipSetDevice");
        Uploaded<float> d_rows(rows);
        Uploaded<uint8_t> d_valid(valid);
        usac_multi_device_input in;
        std::memset(&in, 0, sizeof(in));
        in.P = P;
        in.n_max = n_max;
        in.rows = d_rows.p;
        in.valid = d_valid.p;
        usac_gpu::MultiContext mc = usac_gpu::MultiContext::fromDevice(USAC_HOMOGRAPHY, in);
        bool refused = false;
        Outputs first(P, n_max, k_max), second(P, n_max, k_max);
        try {  // no polishing call has run yet
            mc.exportDevice(first.view(n_max, k_max));
        } catch (const usac_gpu::Error &e) {
            refused = e.code == USAC_ERR_UNSUPPORTED;
        }
        const usac_gpu::MultiContext::Polished res = mc.runPolished(model);
        mc.exportDevice(first.view(n_max, k_max));
        // resident mode: a polishing call without a host mask leaves the same result on the device
        mc.setResident(true);
        std::vector<float> starts(9 * (size_t)P);
        for (uint32_t p = 0; p < P; p++) std::memcpy(&starts[9 * (size_t)p], res.run[p].best.model, sizeof(float) * 9);
        mc.polish(starts.data(), model.threshold);
        mc.exportDevice(second.view(n_max, k_max));
        const bool same = first.models.down() == second.models.down() && first.inliers.down() == second.inliers.down() &&
                          first.status.down() == second.status.down() && first.mask.down() == second.mask.down() &&
                          first.cols.down() == second.cols.down();

        const std::vector<int32_t> models = first.models.down(), inliers = first.inliers.down(),
                                   status = first.status.down(), cols = first.cols.down();
        const std::vector<uint8_t> mask = first.mask.down();
        std::printf("{\"refused_before_a_polish\": %s, \"resident_mode_same\": %s, \"models\": ", refused ? "true" : "false",
                    same ? "true" : "false");
        print_ints(models.data(), models.size());
        std::printf(", \"inliers\": ");
        print_ints(inliers.data(), inliers.size());
        std::printf(", \"status\": ");
        print_ints(status.data(), status.size());
        std::printf(", \"mask\": ");
        print_ints(mask.data(), mask.size());
        std::printf(", \"inlier_cols\": ");
        print_ints(cols.data(), cols.size());
        std::printf(", \"host_inliers\": [");
        for (uint32_t p = 0; p < P; p++) std::printf("%s%d", p ? ", " : "", res.polished[p].inliers);
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
