// A consumer of usac_gpu::MultiContext::refinePoseDevice / refinePose (include/usac_gpu.hpp, ABI 29), C++11, built
// with hipcc because it allocates the device memory it hands over:
//   consumer abi
//   consumer run <P> <n_max> <rows.f32> <valid.u8> <thr> <prob> <max_iters> <R> <seed> <refine_iters>
// `abi` needs no GPU: the ABI numbers of the library and the header, and the size and field offsets of
// usac_multi_refine_io.  `run` uploads the padded calibrated rows (P x n_max x 4 floats) and their keep mask
// (P x n_max bytes), creates an essential context from the device pointers, runs runPolished, takes the pose of
// its result with poseDevice and refines it over the pose's front mask into device memory filled with 0xFF bytes;
// then refinePose from host arrays, of the same poses over all rows.  It prints one JSON object (floats as their
// int32 bit patterns, doubles as their int64 bit patterns).
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
    for (size_t k = 0; k < n; k++) std::printf("%s%lld", k ? ", " : "", (long long)m[k]);
    std::printf("]%s", end);
}

void print_bits(const char *name, const std::vector<float> &v, const char *end) {
    std::vector<int32_t> bits(v.size());
    if (!v.empty()) std::memcpy(bits.data(), v.data(), sizeof(float) * v.size());
    print_ints(name, bits.data(), bits.size(), end);
}

void print_bits(const char *name, const std::vector<double> &v, const char *end) {
    std::vector<int64_t> bits(v.size());
    if (!v.empty()) std::memcpy(bits.data(), v.data(), sizeof(double) * v.size());
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

template <class T>
std::vector<T> filled(size_t n, unsigned char byte) {
    std::vector<T> v(n);
    if (n) std::memset(v.data(), byte, sizeof(T) * n);
    return v;
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "abi")) {
            typedef usac_multi_refine_io IO;
            std::printf("{\"abi\": %d, \"header\": %d, \"sizeof\": %u, \"offsets\": {\"n_max\": %u, \"max_iters\": %u, "
                        "\"R_in\": %u, \"t_in\": %u, \"mask_in\": %u, \"R\": %u, \"t\": %u, \"E\": %u, \"cost0\": %u, "
                        "\"cost\": %u, \"iterations\": %u, \"used\": %u, \"stream\": %u}}\n",
                        usac_abi_version(), USAC_ABI_VERSION, (unsigned)sizeof(IO), (unsigned)offsetof(IO, n_max),
                        (unsigned)offsetof(IO, max_iters), (unsigned)offsetof(IO, R_in), (unsigned)offsetof(IO, t_in),
                        (unsigned)offsetof(IO, mask_in), (unsigned)offsetof(IO, R), (unsigned)offsetof(IO, t),
                        (unsigned)offsetof(IO, E), (unsigned)offsetof(IO, cost0), (unsigned)offsetof(IO, cost),
                        (unsigned)offsetof(IO, iterations), (unsigned)offsetof(IO, used), (unsigned)offsetof(IO, stream));
            return usac_abi_version() == USAC_ABI_VERSION ? 0 : 1;
        }
        if (argc != 12 || std::strcmp(argv[1], "run")) {
            std::fprintf(stderr, "usage: consumer abi | run P n_max rows valid thr prob max_iters R seed refine_iters\n");
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
        const uint32_t refine_iters = (uint32_t)std::atoi(argv[11]);

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
        // the pose of the polished result, and the rows it counted
        Uploaded<float> d_R0(filled<float>(9 * (size_t)P, 0xff)), d_t0(filled<float>(3 * (size_t)P, 0xff));
        Uploaded<uint8_t> d_front(filled<uint8_t>(cells, 0xff));
        usac_multi_pose_output po;
        std::memset(&po, 0, sizeof(po));
        po.n_max = n_max;
        po.R = d_R0.p;
        po.t = d_t0.p;
        po.front_mask = d_front.p;
        // the refinement, into 0xFF bytes
        Uploaded<float> d_R(filled<float>(9 * (size_t)P, 0xff)), d_t(filled<float>(3 * (size_t)P, 0xff)),
            d_E(filled<float>(9 * (size_t)P, 0xff));
        Uploaded<double> d_cost0(filled<double>(P, 0xff)), d_cost(filled<double>(P, 0xff));
        Uploaded<int32_t> d_iter(filled<int32_t>(P, 0xff)), d_used(filled<int32_t>(P, 0xff));
        usac_multi_refine_io o;
        std::memset(&o, 0, sizeof(o));
        o.n_max = n_max;
        o.max_iters = refine_iters;
        o.R_in = d_R0.p;
        o.t_in = d_t0.p;
        o.mask_in = d_front.p;
        o.R = d_R.p;
        o.t = d_t.p;
        o.E = d_E.p;
        o.cost0 = d_cost0.p;
        o.cost = d_cost.p;
        o.iterations = d_iter.p;
        o.used = d_used.p;
        bool refused = false;
        try {  // no polishing call has run yet
            mc.refinePoseDevice(o);
        } catch (const usac_gpu::Error &e) {
            refused = e.code == USAC_ERR_UNSUPPORTED;
        }
        (void)mc.runPolished(model);
        mc.poseDevice(po);
        mc.refinePoseDevice(o);
        const std::vector<float> R0 = d_R0.down(), t0 = d_t0.down();
        const usac_gpu::MultiContext::Refined all = mc.refinePose(R0, t0, std::vector<uint8_t>(), refine_iters);

        std::printf("{\"refused_before_a_polish\": %s, ", refused ? "true" : "false");
        print_bits("R0", R0, ", ");
        print_bits("t0", t0, ", ");
        print_bits("R", d_R.down(), ", ");
        print_bits("t", d_t.down(), ", ");
        print_bits("E", d_E.down(), ", ");
        print_bits("cost0", d_cost0.down(), ", ");
        print_bits("cost", d_cost.down(), ", ");
        const std::vector<int32_t> iter = d_iter.down(), used = d_used.down();
        print_ints("iterations", iter.data(), iter.size(), ", ");
        print_ints("used", used.data(), used.size(), ", ");
        print_bits("all_R", all.R, ", ");
        print_bits("all_t", all.t, ", ");
        print_bits("all_E", all.E, ", ");
        print_bits("all_cost0", all.cost0, ", ");
        print_bits("all_cost", all.cost, ", ");
        print_ints("all_iterations", all.iterations.data(), all.iterations.size(), ", ");
        print_ints("all_used", all.used.data(), all.used.size(), "}\n");
        return 0;
    } catch (const usac_gpu::Error &e) {
        std::fprintf(stderr, "usac_gpu::Error %d: %s\n", e.code, e.what());
        return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
