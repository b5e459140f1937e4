// A consumer of usac_gpu::MultiContext::poseDevice / pose (include/usac_gpu.hpp, ABI 28), C++11, built with hipcc
// because it allocates the device memory it hands over:
//   consumer abi
//   consumer run <P> <n_max> <rows.f32> <valid.u8> <thr> <prob> <max_iters> <R> <seed>
// `abi` needs no GPU: the ABI numbers of the library and the header, and the size and field offsets of
// usac_multi_pose_output.  `run` uploads the padded calibrated rows (P x n_max x 4 floats) and their keep mask
// (P x n_max bytes), creates an essential context from the device pointers, runs runPolished and asks for the pose
// of its result in device memory filled with 0xFF bytes; then pose() from host arrays, of the polished models
// over all rows.  It prints one JSON object (floats as their int32 bit patterns).
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
void print_ints(const char *name, const T *m, size_t n, const char *end) {
    std::printf("\"%s\": [", name);
    for (size_t k = 0; k < n; k++) std::printf("%s%d", k ? ", " : "", (int)m[k]);
    std::printf("]%s", end);
}

void print_bits(const char *name, const std::vector<float> &v, const char *end) {
    std::vector<int32_t> bits(v.size());
    if (!v.empty()) std::memcpy(bits.data(), v.data(), sizeof(float) * v.size());
    print_ints(name, bits.data(), bits.size(), end);
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

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            typedef usac_multi_pose_output Out;
            std::printf("{\"abi\": %d, \"header\": %d, \"sizeof\": %u, \"offsets\": {\"n_max\": %u, \"R\": %u, \"t\": %u, "
                        "\"front\": %u, \"choice\": %u, \"front_mask\": %u, \"stream\": %u}}\n",
                        usac_abi_version(), USAC_ABI_VERSION, (unsigned)sizeof(Out), (unsigned)offsetof(Out, n_max),
                        (unsigned)offsetof(Out, R), (unsigned)offsetof(Out, t), (unsigned)offsetof(Out, front),
                        (unsigned)offsetof(Out, choice), (unsigned)offsetof(Out, front_mask),
                        (unsigned)offsetof(Out, stream));
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 11 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run P n_max rows valid thr prob max_iters R seed\n");
            return 2;
        }
        const uint32_t P = (uint32_t)std::atoi(argv[2]), n_max = (uint32_t)std::atoi(argv[3]);
        const size_t cells = (size_t)P * n_max;
        const std::vector<float> rows = read_file<float>(argv[4], 4 * cells);
        const std::vector<uint8_t> valid = read_file<uint8_t>(argv[5], cells);
        usac_gpu::Model model((float)std::atof(argv[6]), 5u, (float)std::atof(argv[7]), 5, usac_gpu::Essential,
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
        usac_gpu::MultiContext mc = usac_gpu::MultiContext::fromDevice(USAC_ESSENTIAL, in);
        Uploaded<float> d_R(std::vector<float>(9 * (size_t)P, -1.f)), d_t(std::vector<float>(3 * (size_t)P, -1.f));
        Uploaded<int32_t> d_front(std::vector<int32_t>(P, -7)), d_choice(std::vector<int32_t>(P, -7));
        Uploaded<uint8_t> d_mask(std::vector<uint8_t>(cells, 0xff));
        usac_multi_pose_output o;
        std::memset(&o, 0, sizeof(o));
        o.n_max = n_max;
        o.R = d_R.p;
        o.t = d_t.p;
        o.front = d_front.p;
        o.choice = d_choice.p;
        o.front_mask = d_mask.p;
        bool refused = false;
        try {  // no polishing call has run yet
            mc.poseDevice(o);
        } catch (const usac_gpu::Error &e) {
            refused = e.code == USAC_ERR_UNSUPPORTED;
        }
        const usac_gpu::MultiContext::Polished res = mc.runPolished(model);
        mc.poseDevice(o);
        std::vector<float> models(9 * (size_t)P);
        for (uint32_t p = 0; p < P; p++) std::memcpy(&models[9 * (size_t)p], res.polished[p].model, sizeof(float) * 9);
        const usac_gpu::MultiContext::Pose all = mc.pose(models);

        std::printf("{\"refused_before_a_polish\": %s, ", refused ? "true" : "false");
        print_bits("R", d_R.down(), ", ");
        print_bits("t", d_t.down(), ", ");
        const std::vector<int32_t> front = d_front.down(), choice = d_choice.down();
        const std::vector<uint8_t> mask = d_mask.down();
        print_ints("front", front.data(), front.size(), ", ");
        print_ints("choice", choice.data(), choice.size(), ", ");
        print_ints("front_mask", mask.data(), mask.size(), ", ");
        print_bits("models", models, ", ");
        print_bits("all_R", all.R, ", ");
        print_bits("all_t", all.t, ", ");
        print_ints("all_front", all.front.data(), all.front.size(), ", ");
        print_ints("all_choice", all.choice.data(), all.choice.size(), ", ");
        print_ints("all_front_mask", all.front_mask.data(), all.front_mask.size(), "}\n");
        return 0;
    } catch (const usac_gpu::Error &e) {
        std::fprintf(stderr, "usac_gpu::Error %d: %s\n", e.code, e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
