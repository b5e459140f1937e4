// usac_api.cpp -- C-ABI (include/usac_gpu.h) over the HIP kernels, plus the batched
// Ransac::run replay.  Host code only; every model estimation and every residual runs on
// the device -- there is no CPU compute path (a context without a usable GPU fails at
// usac_create with USAC_ERR_HIP).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/usac_gpu.h"
#include "usac_host.hpp"
#include "usac_maxflow.hpp"
#include "usac_kernels.h"
#include "usac_lo_draw.hpp"

namespace {

constexpr uint32_t kDefaultBatch = 8192;
constexpr uint32_t kRampFirst = 1024;  // first batch of a run with the default batch
// the SPRT batch's whole [nw][S] word block copied with its list in one host wait up to this size
constexpr size_t kMaskWholeCopy = 512 * 1024;
constexpr uint32_t kRampFirstProsac = 32;

// Device memory of the contexts comes from a process-wide cache per device: a context is
// typically created per Ransac::run (as the reference constructs its Ransac per run), and
// hipMalloc / hipFree -- the latter synchronising the whole device -- cost milliseconds per
// context.  Blocks are kept in power-of-two size classes (>= 4 KB); a released block goes back
// to its class after its context's stream has drained (usac_destroy synchronises first), a
// block replaced by a larger one only after the device has (reserve() below), so no block is
// handed out while a kernel may still use it.  At most kPoolCap bytes per device are cached.
constexpr size_t kPoolCap = size_t(16) << 30;

struct DevPool {
    std::mutex mu;
    std::multimap<std::pair<int, size_t>, void *> free;  // (device, class bytes) -> block
    std::map<int, size_t> cached;                         // bytes held per device
    static DevPool &get() {
        static DevPool *pool = new DevPool();  // never destroyed: no hipFree after runtime teardown
        return *pool;
    }
    static size_t size_class(size_t b) {
        size_t c = 4096;
        while (c < b) c <<= 1;
        return c;
    }
    hipError_t alloc(size_t b, void **p, size_t *got) {
        const size_t c = size_class(b);
        int dev = 0;
        (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = free.find({dev, c});
            if (it != free.end()) {
                *p = it->second;
                free.erase(it);
                cached[dev] -= c;
                *got = c;
                return hipSuccess;
            }
        }
        hipError_t e = hipMalloc(p, c);
        if (e == hipSuccess) *got = c;
        return e;
    }
    void give_back(void *p, size_t c) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(mu);
            if (cached[dev] + c <= kPoolCap) {
                free.emplace(std::make_pair(dev, c), p);
                cached[dev] += c;
                return;
            }
        }
        (void)hipFree(p);
    }
};

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t b) {
        if (b <= bytes) return hipSuccess;
        if (p) {  // kernels of this context may still read the old block
            (void)hipDeviceSynchronize();
            DevPool::get().give_back(p, bytes);
        }
        p = nullptr;
        bytes = 0;
        return DevPool::get().alloc(b, &p, &bytes);
    }
    void release() {  // the owner's stream has drained (usac_destroy)
        if (p) DevPool::get().give_back(p, bytes);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

// streams and events likewise: creating / destroying them per context costs more than a run
struct StreamPool {
    std::mutex mu;
    std::multimap<int, hipStream_t> streams;
    std::multimap<int, hipEvent_t> events;
    static StreamPool &get() {
        static StreamPool *pool = new StreamPool();
        return *pool;
    }
    hipError_t stream(hipStream_t *s) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = streams.find(dev);
            if (it != streams.end()) {
                *s = it->second;
                streams.erase(it);
                return hipSuccess;
            }
        }
        return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    }
    hipError_t event(hipEvent_t *ev) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = events.find(dev);
            if (it != events.end()) {
                *ev = it->second;
                events.erase(it);
                return hipSuccess;
            }
        }
        return hipEventCreate(ev);
    }
    void give_back(hipStream_t s) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> g(mu);
        streams.emplace(dev, s);
    }
    void give_back(hipEvent_t ev) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> g(mu);
        events.emplace(dev, ev);
    }
};

// pinned host staging blocks (hipHostMalloc costs far more than a run's copies), by size class
struct PinnedPool {
    std::mutex mu;
    std::multimap<size_t, void *> free;
    static PinnedPool &get() {
        static PinnedPool *pool = new PinnedPool();
        return *pool;
    }
    void *take(size_t b, size_t *got) {
        const size_t c = DevPool::size_class(b);
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = free.find(c);
            if (it != free.end()) {
                void *p = it->second;
                free.erase(it);
                *got = c;
                return p;
            }
        }
        void *p = nullptr;
        if (hipHostMalloc(&p, c, hipHostMallocDefault) != hipSuccess) return nullptr;
        *got = c;
        return p;
    }
    void give_back(void *p, size_t c) {
        std::lock_guard<std::mutex> g(mu);
        free.emplace(c, p);
    }
};

// std::vector storage in pinned host memory (PinnedPool), for the loop's DMA sources and
// targets: a copy from / to pageable memory goes through a staging buffer and holds the host
// for the copy; these copies sit between every device step and the host replay.
template <class T>
struct PinnedAlloc {
    typedef T value_type;
    PinnedAlloc() = default;
    template <class U>
    PinnedAlloc(const PinnedAlloc<U> &) {}
    T *allocate(size_t k) {
        size_t got = 0;
        void *p = PinnedPool::get().take(sizeof(T) * (k ? k : 1), &got);
        if (!p) throw std::bad_alloc();
        return static_cast<T *>(p);
    }
    void deallocate(T *p, size_t k) { PinnedPool::get().give_back(p, DevPool::size_class(sizeof(T) * (k ? k : 1))); }
    // default-initialise (no zero fill of staging that a copy overwrites anyway); explicit
    // values as usual
    template <class U>
    void construct(U *p) noexcept {
        ::new (static_cast<void *>(p)) U;
    }
    template <class U, class... A>
    void construct(U *p, A &&...a) {
        ::new (static_cast<void *>(p)) U(std::forward<A>(a)...);
    }
    template <class U>
    bool operator==(const PinnedAlloc<U> &) const { return true; }
    template <class U>
    bool operator!=(const PinnedAlloc<U> &) const { return false; }
};
template <class T>
using pinned_vector = std::vector<T, PinnedAlloc<T>>;

// a pinned staging block (PinnedPool) that only grows
struct PinBlock {
    void *p = nullptr;
    size_t bytes = 0;
};

// at least `need` bytes in a pinned block; growing it moves it, so its users take the pointer afterwards.
// false: the allocation failed (the block is then empty)
bool pin_grow(PinBlock &b, size_t need) {
    if (need <= b.bytes) return true;
    if (b.p) PinnedPool::get().give_back(b.p, b.bytes);
    b.bytes = 0;
    b.p = PinnedPool::get().take(need, &b.bytes);
    return b.p != nullptr;
}

// the block back to the pool (usac_destroy, usac_multi_destroy: the owner's streams have drained)
void pin_release(PinBlock &b) {
    if (b.p) PinnedPool::get().give_back(b.p, b.bytes);
    b.p = nullptr;
    b.bytes = 0;
}

// Wait for a stream by polling it: the loop's host replay waits on the device dozens of
// times per run (LO stages, batches, polish), and a blocking hipStreamSynchronize adds a wake-up
// latency of ~20 us each time; polling returns within about a microsecond of completion.
hipError_t stream_wait(hipStream_t st) {
    for (uint32_t spins = 0;; spins++) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if ((spins & 1023u) == 1023u) std::this_thread::yield();
    }
}

}  // namespace

struct usac_ctx {
    int device = 0;
    int estimator = 0;
    uint32_t n = 0, cols = 0, m = 0;
    int dlt_mode = USAC_DLT_THIN;
    int chunks = 4;
    int score_variant = 0;  // 0 = guard-band fast path (+ pre-sort; multi-chunk H: the matrix-core prefilter),
                            // 1 = exact expression only, 2 = fast, no pre-sort, 3 = (tests) usac_score_models
                            // of H through the multi-chunk scorer
    hipStream_t stream = nullptr;
    DevBuf pts;
    DevBuf rec;             // fast-kernel point records (32 B / point)
    DevBuf prosac_tab;      // device PROSAC schedule: subset size per hypothesis (< T_N)
    uint32_t prosac_len = 0;  // its entries
    int dev_sampler = USAC_SAMPLER_UNIFORM;
    DevBuf tv_part;         // two-view scorer scratch: pre-sort permutation, chunk partials
    DevBuf perm;            // hypothesis pre-sort of the fast kernel (usac::presort_bytes)
    void *perm_zeroed = nullptr;  // the perm block whose region counters were zeroed
    DevBuf hf_part;         // fast-kernel partials of a point range split over workgroups
    float rec_thr = -1.f;   // threshold the record bands were built for
    float4 ext = {0, 0, 0, 0};  // dataset box: max |x1|, |y1|, |x2|, |y2| over the finite rows (fast-kernel bounds)
    float4 grid_ext = {0, 0, 0, 0};  // the same over every row, infinite coordinates included (ensure_grid)
    // the matrix-core prefilter scorer of homographies (kernels_h16.hip): dataset constants, fp16
    // point features (built on first use), per-batch rows / slacks and chunk partials; h16 = 1 when
    // usable (USAC_H16=0 turns it off: the lanes-over-hypotheses k_score_hf then scores every batch)

    int h16 = 0;
    bool h16_feat_ok = false;
    bool h16_off = false;  // k_score_hf for every batch (usac_ransac_run sets it for its loop)
    uint32_t h16_rows_for = 0;  // > 0: the solver wrote the rows of a batch of this size for h16_rows_thr
    float h16_rows_thr = 0.f;
    uint32_t h16_deferred_ch = 0;  // > 0: the last h16 batch's chunk partials await batch_argmax
    float h16_deferred_thr = 0.f;
    DevBuf h16_k, h16_feat, h16_rows, h16_fm, h16_part;  // h16_k: the dataset constants (usac::H16Consts)
    // the matrix-core prefilter scorer of essential matrices (kernels_e16.hip): the h16 dataset
    // constants, its own rho-scaled fp16 features, per-batch rows / bounds and chunk partials; e16 = 1
    // when usable (USAC_E16=0: the lanes-over-models k_score_f2 scores every throughput batch)
    int e16 = 0;
    bool h16_k_ok = false, e16_feat_ok = false;
    DevBuf e16_feat, e16_rows, e16_cm, e16_part;
    // batch buffers
    DevBuf samples, models, counts, sums, best, hostmodels, argmax_part;
    DevBuf list, list_n;    // fundamental: occupied model slots (compacted) and their number
    DevBuf h4_fb, h4_fb_n;  // homography thin DLT: QR fall-back hypotheses and two counters (zeroed once)
    DevBuf pool_idx, pool_pts, masks;  // SPRT parity path: pool order, permuted points, flag words
    // LO-RANSAC (LoRansac): W speculative inner iterations in flight -- their inlier lists
    // (W x N), LSQ sample positions (W x lo_sample_size), point counts, thresholds, models,
    // fit flags, scores, fit and scoring scratch; lo_max = the current best's inlier list
    DevBuf lo_max, lo_lists, lo_pos, lo_ns, lo_thrs, lo_slots, lo_models, lo_ok, lo_cnts, lo_sums, lo_q, lo_part,
        lo_ws, lo_scr;
    DevBuf knn_idx, knn_d2;  // KNN neighbour table (usac_knn, NAPSAC KNN)
    // grid neighbours (build_grid): CSR of the cells of size grid_cs, NAPSAC-eligible points
    // grid CSR in one block, downloaded by one copy: cell[n], rank[n], members[n], start[n + 1]
    DevBuf grid_csr, grid_elig, grid_ws;
    uint32_t *grid_cell() const { return grid_csr.as<uint32_t>(); }
    uint32_t *grid_rank() const { return grid_csr.as<uint32_t>() + n; }
    int32_t *grid_members() const { return reinterpret_cast<int32_t *>(grid_csr.as<uint32_t>() + 2 * (size_t)n); }
    uint32_t *grid_start() const { return grid_csr.as<uint32_t>() + 3 * (size_t)n; }
    int grid_cs = 0;        // cell size the grid was built for (0 = none)
    uint64_t grid_gen = 0;  // bumped at every (re)build of the device grid
    // the host copy of the grid (download_grid), reused while grid_gen is unchanged
    std::shared_ptr<const usac::GridNeighbors> grid_host;
    uint64_t grid_host_gen = ~0ull;
    int cell_size = 50;     // model.hpp:43, the device NAPSAC sampler's grid
    uint32_t grid_n_cells = 0, grid_n_elig = 0;
    DevBuf gc_err;           // graph-cut LO: residuals of the model being labelled
    DevBuf e5_ws;                      // staged 5-point solver workspace
    // throughput SPRT (usac_set_sprt): batch-fixed test on the pool-ordered points
    bool sprt_on = false;
    usac::SprtConsts sprt_k{};      // up, down, A and their logs (the reference's doubles)
    double sprt_eps = 0.0, sprt_delta = 0.0;
    DevBuf sprt_pts, sprt_tested, sprt_surv, sprt_surv_n, sprt_starts;
    uint32_t spk = 1;       // model slots per hypothesis (3 for the 7-point solver)
    // single-model / polish buffers
    DevBuf one_model, inl_idx, inl_cnt, inl_sum, inl_scratch, q, partial, ws, nm_model, nm_ok;
    PinBlock grid_pin;               // pinned words the grid build reads its two counts into
    DevBuf pol_res;                  // polish pass results (usac_kernels.h kPol*: per pass model, ok, count, sum)
    DevBuf pol_lists;                // the polish passes' inlier lists (4 x n)
    PinBlock pol_pin;                // their pinned host copy (PinnedPool)
    DevBuf nm_seq;          // normalisation scratch of the non-minimal fits (polish and LO)
    DevBuf nm_w, nm_qw;     // usac_lsq_fit with weights: the weights, the weighted points
    DevBuf lo_io;           // one LO stage's inputs (two blocks, alternating) and outputs
    // the LO stages' Σerr passes run on their own stream beside the next stage's fit
    hipStream_t lo_stream = nullptr;
    PinBlock rec_pin;  // usac_fetch_best's pinned staging (a pageable D2H copy is staged by the runtime)
    // the loop's next batch drawn and run ahead of the current batch's replay (usac_ransac_run)
    hipStream_t spec_stream = nullptr;
    hipEvent_t spec_ev = nullptr;
    // per block parity: the stage's outputs in the host block (main), its Σ (side); round end
    hipEvent_t lo_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // comm
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    DevBuf rec_send, rec_all;
    DevBuf x_send, x_recv;  // sharded-run all-gather buffers (RCCL path, device-packed)
    PinBlock x_pin;         // their pinned host copy (the replay's counts / model words)
    // batch-best exchange (usac_exchange_best_async / _wait): a dedicated stream ordered after
    // each batch by an event, a ring of in-flight all-gathers (device + pinned host records)
    hipStream_t xstream = nullptr;
    hipEvent_t xev_batch[USAC_XRING] = {}, xev_done[USAC_XRING] = {};
    DevBuf xring;
    PinBlock xring_host;    // the ring's pinned host records
    usac_record *xring_records() const { return static_cast<usac_record *>(xring_host.p); }
    // collectives on one communicator must run in one order on every rank: the two streams
    // that issue them are ordered by events -- a collective on `stream` waits for the last
    // exchange (x_last), an exchange waits for the last collective on `stream` (coll_ev)
    int x_last = -1;
    hipEvent_t coll_ev = nullptr;
    bool coll_pending = false;
    // timing
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float last_ms[3] = {0, 0, 0};
    bool batch_valid = false;  // counts / sums hold a batch's scores (usac_last_counts)
    uint32_t sprt_S = 0;       // model slots of the last batch-SPRT launch (usac_batch_sprt_info)
    bool timed_pending = false;
    bool timing_on = true;  // usac_set_timing
    std::string err;
};

namespace {

int fail(usac_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((ctx), USAC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define NCCL_TRY(ctx, expr)                                                                        \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return fail((ctx), USAC_ERR_HIP, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

// before a collective on c->stream: after every exchange issued on the exchange stream
hipError_t order_after_exchanges(usac_ctx *c) {
    if (c->xstream && c->x_last >= 0) return hipStreamWaitEvent(c->stream, c->xev_done[c->x_last], 0);
    return hipSuccess;
}
// after a collective on c->stream: later exchanges wait for it
hipError_t mark_collective(usac_ctx *c) {
    if (!c->coll_ev) return hipSuccess;
    hipError_t e = hipEventRecord(c->coll_ev, c->stream);
    if (e == hipSuccess) c->coll_pending = true;
    return e;
}

bool is_h(const usac_ctx *c) { return c->estimator == USAC_HOMOGRAPHY; }
bool is_f(const usac_ctx *c) { return c->estimator == USAC_FUNDAMENTAL; }
bool is_e(const usac_ctx *c) { return c->estimator == USAC_ESSENTIAL; }
// solvers that may return no model for a sample: occupied slots are listed (list / list_n)
bool listed(const usac_ctx *c) { return is_f(c) || is_e(c); }
bool two_view(const usac_ctx *c) { return c->cols == 4; }
int ncomp(const usac_ctx *c) { return two_view(c) ? 9 : 3; }
int ncomp_dev(const usac_ctx *c) { return is_h(c) ? 18 : ncomp(c); }

// B = hypotheses (minimal samples); every per-model buffer holds B * spk slots
int ensure_batch(usac_ctx *c, uint32_t B) {
    const size_t S = (size_t)B * c->spk;
    HIP_TRY(c, c->samples.reserve(sizeof(int32_t) * (size_t)B * c->m));
    HIP_TRY(c, c->models.reserve(sizeof(float) * S * ncomp_dev(c)));
    HIP_TRY(c, c->counts.reserve(sizeof(int32_t) * S));
    HIP_TRY(c, c->sums.reserve(sizeof(float) * S));
    HIP_TRY(c, c->best.reserve(sizeof(usac_record)));
    HIP_TRY(c, c->argmax_part.reserve(16 * (S / 2048 + 1)));
    HIP_TRY(c, c->hostmodels.reserve(sizeof(float) * 9 * S));
    if (listed(c)) {
        HIP_TRY(c, c->list.reserve(sizeof(uint32_t) * S));
        HIP_TRY(c, c->list_n.reserve(sizeof(uint32_t)));
    }
    if (is_h(c)) {
        HIP_TRY(c, c->h4_fb.reserve(sizeof(uint32_t) * (size_t)B));
        if (!c->h4_fb_n.p) {  // the kernels reset the counters after each use; a pooled block is not zero
            HIP_TRY(c, c->h4_fb_n.reserve(2 * sizeof(uint32_t)));
            HIP_TRY(c, hipMemsetAsync(c->h4_fb_n.p, 0, 2 * sizeof(uint32_t), c->stream));
        }
    }
    return USAC_OK;
}

int ensure_single(usac_ctx *c) {
    HIP_TRY(c, c->one_model.reserve(sizeof(float) * 9));
    HIP_TRY(c, c->inl_idx.reserve(sizeof(int32_t) * (size_t)std::max<uint32_t>(c->n, 1)));
    HIP_TRY(c, c->pol_lists.reserve(sizeof(int32_t) * 4 * (size_t)std::max<uint32_t>(c->n, 1)));
    // the polish's later passes fit with c->n as the bound on their device-side counts: their
    // scratch reserved here, so no growth (a device synchronise) inside a run
    HIP_TRY(c, c->nm_seq.reserve(usac::nonminimal_seq_bytes(std::max<uint32_t>(c->n, 1), 1)));
    HIP_TRY(c, c->pol_res.reserve(sizeof(float) * usac::kPolWords));
    HIP_TRY(c, c->inl_cnt.reserve(sizeof(int32_t)));
    HIP_TRY(c, c->inl_sum.reserve(sizeof(float)));
    HIP_TRY(c, c->q.reserve(sizeof(float) * 4 * (size_t)std::max<uint32_t>(c->n, 1)));
    HIP_TRY(c, c->partial.reserve(sizeof(double) * 45 * ((size_t)c->n / 64 + 2)));
    HIP_TRY(c, c->ws.reserve(sizeof(float) * 32));
    HIP_TRY(c, c->nm_model.reserve(sizeof(float) * 9));
    HIP_TRY(c, c->nm_ok.reserve(sizeof(int32_t)));
    return USAC_OK;
}

usac::DevSampler dev_sampler(const usac_ctx *c, uint64_t seed) {
    const bool prosac = c->dev_sampler == USAC_SAMPLER_PROSAC;
    usac::DevSampler ds{};
    ds.seed = seed;
    ds.prosac = prosac ? c->prosac_tab.as<uint32_t>() : nullptr;
    ds.prosac_len = prosac ? c->prosac_len : 0u;
    if (c->dev_sampler == USAC_SAMPLER_NAPSAC) {
        ds.nap_n_eligible = c->grid_n_elig;
        ds.nap_cell = c->grid_cell();
        ds.nap_rank = c->grid_rank();
        ds.nap_start = c->grid_start();
        ds.nap_members = c->grid_members();
        ds.nap_eligible = c->grid_elig.as<int32_t>();
    }
    return ds;
}

// The grid of a dataset whose cell key does not fit the device build's 63-bit packed key (more
// than 65536 cells along a dimension, or four ranges wider than 63 bits in all): built on the host
// (usac::GridNeighbors' hash map takes any key) from the device's points, then uploaded in the
// device CSR layout -- the same cells, numbering and member order as the device build.
int host_grid(usac_ctx *c, int cs) {
    const size_t n = c->n;
    std::vector<float> pts(4 * n);
    HIP_TRY(c, hipMemcpyAsync(pts.data(), c->pts.p, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    const usac::GridNeighbors g(pts.data(), c->n, cs);
    std::vector<uint32_t> csr(4 * n + 1);
    const uint32_t nc = (uint32_t)g.starts().size() - 1;
    memcpy(csr.data(), g.cells().data(), 4 * n);
    memcpy(csr.data() + n, g.ranks().data(), 4 * n);
    memcpy(csr.data() + 2 * n, g.members().data(), 4 * n);
    memcpy(csr.data() + 3 * n, g.starts().data(), 4 * ((size_t)nc + 1));
    std::vector<int32_t> elig;
    for (uint32_t i = 0; i < c->n; i++)
        if (g.count(i) >= c->m) elig.push_back((int32_t)i);
    HIP_TRY(c, hipMemcpyAsync(c->grid_csr.p, csr.data(), sizeof(uint32_t) * (3 * n + nc + 1), hipMemcpyHostToDevice,
                              c->stream));
    if (!elig.empty())
        HIP_TRY(c, hipMemcpyAsync(c->grid_elig.p, elig.data(), sizeof(int32_t) * elig.size(), hipMemcpyHostToDevice,
                                  c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    c->grid_n_cells = nc;
    c->grid_n_elig = (uint32_t)elig.size();
    c->grid_cs = cs;
    c->grid_gen++;
    return USAC_OK;
}

// NearestNeighbors::getGridNearestNeighbors (nearest_neighbors.cpp:160-202) on the device for
// cell size cs (kept until another size is asked for).  Cells are packed per dimension relative
// to the dataset box's lowest cell; a box too wide for the packed key takes host_grid instead.
int ensure_grid(usac_ctx *c, int cs) {
    if (c->grid_cs == cs) return USAC_OK;
    if (c->cols != 4) return fail(c, USAC_ERR_ARG, "grid neighbours need 4-column points (SURVEY Q17)");
    if (cs <= 0) return fail(c, USAC_ERR_ARG, "grid cell_size must be > 0");
    const float e[4] = {c->grid_ext.x, c->grid_ext.y, c->grid_ext.z, c->grid_ext.w};
    int lo[4], bits[4];
    bool packable = true;
    for (int j = 0; j < 4; j++) {
        lo[j] = bits[j] = 0;
        if (!(e[j] / (float)cs < 1.0e9f)) {  // the int cell index itself is out of range
            packable = false;
            continue;
        }
        lo[j] = (int)(-e[j] / (float)cs);
        const long long range = (long long)(int)(e[j] / (float)cs) - lo[j];
        packable &= range <= 65535;
        bits[j] = 1;  // 2^bits - 1 > range: room for the out-of-box sentinel
        while (bits[j] < 40 && (1ll << bits[j]) - 1 <= range) bits[j]++;
    }
    // each dimension keeps its range plus the out-of-box sentinel; the build's hash table keeps
    // the all-ones word as its empty slot, so the key must fit 63 bits (clamping a dimension
    // would give the sentinel a real cell's value)
    packable &= bits[0] + bits[1] + bits[2] + bits[3] <= 63;
    const size_t n = c->n;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->grid_csr.reserve(sizeof(uint32_t) * (4 * n + 1)));
    HIP_TRY(c, c->grid_elig.reserve(sizeof(int32_t) * n));
    c->grid_cs = 0;
    c->grid_gen++;
    if (!packable) return host_grid(c, cs);
    if (!pin_grow(c->grid_pin, 64)) return fail(c, USAC_ERR_HIP, "pinned host allocation failed");
    HIP_TRY(c, c->grid_ws.reserve(usac::grid_workspace_bytes(c->n)));
    c->grid_cs = 0;
    c->grid_gen++;
    HIP_TRY(c, usac::build_grid(c->stream, c->pts.as<float4>(), c->n, cs, make_int4(lo[0], lo[1], lo[2], lo[3]),
                                make_int4(bits[0], bits[1], bits[2], bits[3]), c->m, c->grid_ws.p,
                                c->grid_cell(), c->grid_rank(), c->grid_start(), c->grid_members(),
                                c->grid_elig.as<int32_t>(), static_cast<uint32_t *>(c->grid_pin.p),
                                &c->grid_n_cells, &c->grid_n_elig));
    c->grid_cs = cs;
    c->grid_gen++;
    return USAC_OK;
}

// the device grid as the host loop's GridNeighbors (bit-identical to building it on the host)
int download_grid(usac_ctx *c, int cs, std::shared_ptr<const usac::GridNeighbors> &out) {
    int rc = ensure_grid(c, cs);
    if (rc) return rc;
    if (c->grid_host && c->grid_host_gen == c->grid_gen) {  // the same device grid: its host copy
        out = c->grid_host;
        return USAC_OK;
    }
    // DMA into one pinned block, then into the host vectors (the sampler reads them at random:
    // they should be cache-warm, which DMA-written pinned memory is not)
    const size_t n = c->n, nc1 = (size_t)c->grid_n_cells + 1;
    // (a raw pooled block: a pinned_vector would zero-fill the 1.2 MB first)
    size_t got = 0;
    uint32_t *w = static_cast<uint32_t *>(PinnedPool::get().take(sizeof(uint32_t) * (3 * n + nc1), &got));
    if (!w) return fail(c, USAC_ERR_HIP, "pinned host allocation failed");
    struct Back {
        void *p;
        size_t b;
        ~Back() { PinnedPool::get().give_back(p, b); }
    } back{w, got};
    HIP_TRY(c, hipMemcpyAsync(w, c->grid_csr.p, sizeof(uint32_t) * (3 * n + nc1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    std::vector<uint32_t> cell(w, w + n), rank(w + n, w + 2 * n), start(w + 3 * n, w + 3 * n + nc1);
    std::vector<int32_t> members(reinterpret_cast<const int32_t *>(w + 2 * n), reinterpret_cast<const int32_t *>(w + 3 * n));
    out = std::make_shared<const usac::GridNeighbors>(std::move(cell), std::move(rank), std::move(start),
                                                      std::move(members));
    c->grid_host = out;
    c->grid_host_gen = c->grid_gen;
    return USAC_OK;
}

// solve (samples on device, or device RNG when samples_dev == nullptr) into c->models
hipError_t h16_init(usac_ctx *c);

// h16_thr >= 0: the batch will be scored by the matrix-core scorer (h16_scores) -- the homography
// solvers then also write its rows and slacks (usac_h16.hpp), so enqueue_score_h16 skips k_h16_rows
hipError_t enqueue_solve(usac_ctx *c, const int32_t *samples_dev, uint32_t B, uint64_t seed, uint64_t first_hyp,
                         int32_t *samples_out, float h16_thr = -1.f) {
    const usac::DevSampler ds = dev_sampler(c, seed);
    c->h16_rows_for = 0;
    if (is_e(c)) {
        hipError_t e = c->e5_ws.reserve(usac::e5_workspace_bytes(B));
        if (e != hipSuccess) return e;
        return usac::launch_solve_e5(c->stream, c->pts.as<float4>(), c->n, samples_dev, samples_out, B, ds,
                                     first_hyp, c->models.as<float>(), c->counts.as<int32_t>(),
                                     c->list.as<uint32_t>(), c->list_n.as<uint32_t>(), c->e5_ws.p);
    }
    if (is_f(c))
        return usac::launch_solve_f7(c->stream, c->pts.as<float4>(), c->n, samples_dev, samples_out, B, ds,
                                     first_hyp, c->models.as<float>(), c->counts.as<int32_t>(),
                                     c->list.as<uint32_t>(), c->list_n.as<uint32_t>());
    if (is_h(c)) {
        usac::H16Emit em{nullptr, 0.f, nullptr, nullptr};
        if (h16_thr >= 0.f) {
            hipError_t e = h16_init(c);
            if (e == hipSuccess) e = c->h16_rows.reserve((size_t)B * 96);
            if (e == hipSuccess) e = c->h16_fm.reserve(sizeof(float) * (size_t)B);
            if (e != hipSuccess) return e;
            em = usac::H16Emit{c->h16_k.as<usac::H16Consts>(), h16_thr, c->h16_rows.p, c->h16_fm.as<float>()};
        }
        const hipError_t e = usac::launch_solve_h4(c->stream, c->pts.as<float4>(), c->n, samples_dev, samples_out, B,
                                                   ds, first_hyp, c->dlt_mode == USAC_DLT_NULLSPACE,
                                                   c->models.as<float>(), c->h4_fb.as<uint32_t>(),
                                                   c->h4_fb_n.as<uint32_t>(), em.rows ? &em : nullptr);
        if (e == hipSuccess && em.rows) {
            c->h16_rows_for = B;
            c->h16_rows_thr = h16_thr;
        }
        return e;
    }
    return usac::launch_solve_line(c->stream, c->pts.as<float2>(), c->n, samples_dev, samples_out, B, ds, first_hyp,
                                   c->models.as<float>());
}

// point chunks of the matrix-core scorer for a batch of B: ~16 waves per SIMD over the launch
// (20 hypotheses per wave; USAC_H16_CHUNKS overrides), at most one 32-point block per chunk and 256
uint32_t h16_chunks(const usac_ctx *c, uint32_t B) {
    const uint32_t waves = (B + 19) / 20, nblk = (c->n + 31) / 32;
    static const int env_ch = getenv("USAC_H16_CHUNKS") ? atoi(getenv("USAC_H16_CHUNKS")) : 0;
    const uint32_t ch = env_ch > 0 ? (uint32_t)env_ch : (16384u + waves - 1) / waves;
    // at most 2^23 points per chunk: a hypothesis' fixed-point Σ partial of one chunk stays below 2^63
    // (launch_score_h16 refuses more); n <= 2^25 makes this at most 4
    const uint32_t min_ch = (nblk + (1u << 18) - 1) >> 18;
    return std::max(std::max(1u, min_ch), std::min(ch, std::min(nblk, 256u)));
}

// The matrix-core prefilter scorer (kernels_h16.hip): the point features once per context, each
// hypothesis' fp16 rows and slack per batch, then the scorer over point chunks -- enough chunks for
// ~16 waves per SIMD over the launch (20 hypotheses per wave; USAC_H16_CHUNKS overrides).
// the dataset constants and the point features, once per context (on its stream)
// the dataset constants (centres, power-of-two scales, feature maxima), shared by h16 and e16
hipError_t h16_consts_init(usac_ctx *c) {
    if (c->h16_k_ok) return hipSuccess;
    hipError_t e;
    if ((e = c->h16_k.reserve(sizeof(usac::H16Consts))) != hipSuccess) return e;
    if ((e = usac::launch_h16_consts(c->stream, c->pts.as<float4>(), c->n, c->ext, c->h16_k.as<usac::H16Consts>())) !=
        hipSuccess)
        return e;
    c->h16_k_ok = true;
    return hipSuccess;
}

hipError_t h16_init(usac_ctx *c) {
    if (c->h16_feat_ok) return hipSuccess;
    hipError_t e;
    if ((e = h16_consts_init(c)) != hipSuccess) return e;
    if ((e = c->h16_feat.reserve(usac::h16_feature_bytes(c->n))) != hipSuccess) return e;
    if ((e = usac::launch_h16_points(c->stream, c->pts.as<float4>(), c->n, c->h16_k.as<usac::H16Consts>(),
                                     c->h16_feat.p)) != hipSuccess)
        return e;
    c->h16_feat_ok = true;
    return hipSuccess;
}

// will enqueue_score(c, B, thr, chunks) take the matrix-core scorer?
bool h16_scores(const usac_ctx *c, int chunks);
// ... and should the solver write its rows (USAC_H16_FUSE=0: k_h16_rows after the solve, A/B)
float h16_solver_thr(const usac_ctx *c, int chunks, float thr) {
    static const bool fuse = !getenv("USAC_H16_FUSE") || atoi(getenv("USAC_H16_FUSE")) != 0;
    return fuse && h16_scores(c, chunks) ? thr : -1.f;
}
bool h16_scores(const usac_ctx *c, int chunks) {
    return is_h(c) && !c->sprt_on && c->h16 == 1 && !c->h16_off && (c->score_variant == 0 || c->score_variant == 3) &&
           chunks > 1;
}

// defer_finish: the chunk partials stay for the batch argmax (launch_argmax_h16, via batch_argmax)
hipError_t enqueue_score_h16(usac_ctx *c, uint32_t B, float thr, bool defer_finish) {
    hipError_t e;
    c->h16_deferred_ch = 0;
    if ((e = h16_init(c)) != hipSuccess) return e;
    const uint32_t ch = h16_chunks(c, B);
    if ((e = c->h16_part.reserve(usac::h16_part_bytes(B, (int)ch))) != hipSuccess) return e;
    const bool ready = c->h16_rows_for == B && c->h16_rows_thr == thr;  // written by the solver
    c->h16_rows_for = 0;
    if (!ready) {
        if ((e = c->h16_rows.reserve((size_t)B * 96)) != hipSuccess) return e;
        if ((e = c->h16_fm.reserve(sizeof(float) * (size_t)B)) != hipSuccess) return e;
        if ((e = usac::launch_h16_rows(c->stream, c->models.as<float>(), B, c->h16_k.as<usac::H16Consts>(), thr,
                                       c->h16_rows.p, c->h16_fm.as<float>())) != hipSuccess)
            return e;
    }
    e = usac::launch_score_h16(c->stream, c->h16_feat.p, c->pts.as<float4>(), c->n, c->h16_rows.p,
                               c->h16_fm.as<float>(), c->models.as<float>(), B, thr, (int)ch, c->h16_part.p,
                               c->counts.as<int32_t>(), c->sums.as<float>(), !defer_finish);
    if (e == hipSuccess && defer_finish) {
        c->h16_deferred_ch = ch;
        c->h16_deferred_thr = thr;
    }
    return e;
}

// The essential matrix-core prefilter scorer (kernels_e16.hip): throughput batches of listed models
// (chunks > 1: Σ re-associated, counts exact), the default score variant, USAC_E16 unset or 1
bool e16_scores(const usac_ctx *c, int chunks, float thr) {
    return is_e(c) && !c->sprt_on && c->e16 == 1 && c->score_variant == 0 && chunks > 1 && thr > 0x1p-100f &&
           thr < 0x1p100f;
}

// point chunks of the e16 scorer for kmax listed slots: ~12 waves per SIMD if every slot is
// occupied (64 models per wave), at most one 32-point block per chunk, 256 chunks, and >= 1 per
// 2^23 points (its fixed-point Σ bound)
uint32_t e16_chunks(const usac_ctx *c, uint32_t kmax) {
    const uint32_t waves = (kmax + 63) / 64, nblk = (c->n + 31) / 32;
    const uint32_t ch = (12288u + waves - 1) / waves;
    const uint32_t min_ch = (nblk + (1u << 18) - 1) >> 18;
    return std::max(std::max(1u, min_ch), std::min(ch, std::min(nblk, 256u)));
}

// list / list_n: the batch's occupied slots (nullptr: models 0 .. kmax - 1)
hipError_t enqueue_score_e16(usac_ctx *c, uint32_t kmax, float thr, const uint32_t *list, const uint32_t *list_n) {
    hipError_t e;
    if ((e = h16_consts_init(c)) != hipSuccess) return e;
    if (!c->e16_feat_ok) {
        if ((e = c->e16_feat.reserve(usac::e16_feature_bytes(c->n))) != hipSuccess) return e;
        if ((e = usac::launch_e16_points(c->stream, c->pts.as<float4>(), c->n, c->h16_k.as<usac::H16Consts>(),
                                         c->e16_feat.p)) != hipSuccess)
            return e;
        c->e16_feat_ok = true;
    }
    const uint32_t ch = e16_chunks(c, kmax);
    if ((e = c->e16_rows.reserve(usac::e16_row_bytes(kmax))) != hipSuccess) return e;
    if ((e = c->e16_cm.reserve(sizeof(float) * (size_t)kmax)) != hipSuccess) return e;
    if ((e = c->e16_part.reserve(usac::e16_part_bytes(kmax, (int)ch))) != hipSuccess) return e;
    const size_t stride = kmax;
    if ((e = usac::launch_e16_rows(c->stream, c->models.as<float>(), stride, list, list_n, kmax,
                                   c->h16_k.as<usac::H16Consts>(), thr, c->e16_rows.p, c->e16_cm.as<float>())) !=
        hipSuccess)
        return e;
    return usac::launch_score_e16(c->stream, c->e16_feat.p, c->pts.as<float4>(), c->n, c->e16_rows.p,
                                  c->e16_cm.as<float>(), c->models.as<float>(), stride, list, list_n, kmax, thr,
                                  (int)ch, c->e16_part.p, c->counts.as<int32_t>(), c->sums.as<float>());
}

// chunks == 1 is the parity configuration: per-hypothesis sums are the exact sequential
// fp32 sums of the reference.  chunks > 1 re-associates Σerr across chunks (counts exact).
hipError_t enqueue_score(usac_ctx *c, uint32_t B, float thr, int chunks, bool defer_finish = false) {
    if (c->sprt_on) {
        hipError_t e = hipMemsetAsync(c->sprt_tested.p, 0, sizeof(uint32_t), c->stream);
        if (e != hipSuccess) return e;
        const uint32_t S = B * c->spk;
        c->sprt_S = S;
        e = c->sprt_surv.reserve(usac::sprt_survivor_bytes() * (size_t)S);
        if (e != hipSuccess) return e;
        e = c->sprt_starts.reserve(sizeof(uint32_t) * (size_t)S);
        if (e != hipSuccess) return e;
        return usac::launch_score_sprt(c->stream, c->estimator, c->sprt_pts.p, c->n, c->models.as<float>(),
                                       (size_t)S, listed(c) ? c->list.as<uint32_t>() : nullptr,
                                       listed(c) ? c->list_n.as<uint32_t>() : nullptr, S, thr, c->sprt_k,
                                       c->counts.as<int32_t>(), c->sums.as<float>(), c->sprt_tested.as<uint32_t>(),
                                       c->sprt_surv.p, c->sprt_surv_n.as<uint32_t>(), c->sprt_starts.as<uint32_t>());
    }
    if ((listed(c) || is_h(c)) && c->score_variant != 1 && c->rec_thr != thr) {  // fast-kernel point records
        hipError_t e = c->rec.reserve(sizeof(float) * 32 * (((size_t)c->n + 3) / 4));
        if (e != hipSuccess) return e;
        e = usac::launch_prepare_rec(c->stream, c->pts.as<float4>(), c->n, thr, c->rec.as<float4>());
        if (e != hipSuccess) return e;
        c->rec_thr = thr;
    }
    if (listed(c)) {  // the occupied slots of the last solve
        if (c->score_variant == 1)
            return usac::launch_score_f(c->stream, c->estimator, chunks, c->pts.as<float4>(), c->n,
                                        c->models.as<float>(), (size_t)B * c->spk, c->list.as<uint32_t>(),
                                        c->list_n.as<uint32_t>(), B * c->spk, thr, c->counts.as<int32_t>(),
                                        c->sums.as<float>());
        if (e16_scores(c, chunks, thr))  // counts exact
            return enqueue_score_e16(c, B * c->spk, thr, c->list.as<uint32_t>(), c->list_n.as<uint32_t>());
        hipError_t e = c->tv_part.reserve(usac::tv_scratch_bytes(B * c->spk, chunks));
        if (e != hipSuccess) return e;
        return usac::launch_score_f2(c->stream, c->estimator, chunks, c->rec.as<float4>(), c->pts.as<float4>(), c->n,
                                     c->ext, c->models.as<float>(),
                                     (size_t)B * c->spk, c->list.as<uint32_t>(), c->list_n.as<uint32_t>(), B * c->spk,
                                     thr, c->counts.as<int32_t>(), c->sums.as<float>(), c->tv_part.p);
    }
    if (is_h(c)) {
        if (c->score_variant == 1)
            return usac::launch_score_h(c->stream, chunks, c->pts.as<float4>(), c->n, c->models.as<float>(), B, thr,
                                        c->counts.as<int32_t>(), c->sums.as<float>());
        if (h16_scores(c, chunks)) return enqueue_score_h16(c, B, thr, defer_finish);  // counts exact
        uint32_t *perm = nullptr;
        if (c->score_variant == 0) {  // 2: fast kernel without the hypothesis pre-sort (A/B)
            hipError_t e = c->perm.reserve(usac::presort_bytes(B));
            if (e != hipSuccess) return e;
            if (c->perm_zeroed != c->perm.p) {  // a new block: its region counters start at 0
                e = hipMemsetAsync(c->perm.p, 0, usac::presort_counter_bytes(), c->stream);
                if (e != hipSuccess) return e;
                c->perm_zeroed = c->perm.p;
            }
            perm = c->perm.as<uint32_t>();
        }
        // small batches over many points (the loop's batches): split each tile's points over
        // several workgroups too, so the chip holds ~8 waves per SIMD
        uint32_t ys = 1;
        if (chunks > 1) {
            const uint32_t waves = (B + 63) / 64 * (uint32_t)chunks, groups = (c->n + 3) / 4;
            while (ys < 16 && waves * ys * 2 <= 8192u && groups / ((uint32_t)chunks * ys * 2) >= 64u) ys *= 2;
        }
        if (ys > 1) {
            hipError_t e = c->hf_part.reserve(sizeof(int32_t) * 2 * (size_t)ys * B);
            if (e != hipSuccess) return e;
        }
        return usac::launch_score_hf(c->stream, chunks, chunks == 1, c->rec.as<float4>(), c->n, c->ext,
                                     c->models.as<float>(), B, thr, perm, c->counts.as<int32_t>(), c->sums.as<float>(),
                                     ys, ys > 1 ? c->hf_part.p : nullptr);
    }
    return usac::launch_score_line(c->stream, chunks, c->pts.as<float2>(), c->n, c->models.as<float>(), B, thr,
                                   c->counts.as<int32_t>(), c->sums.as<float>());
}

// point chunks for the loop's batches (counts only -- the sums the replay reads are exact,
// exact_sums): lanes-over-hypotheses kernels need ~4 waves per SIMD, and the loop's batches
// are small (<= 8192 samples, often max_iterations), so H / line split the points finer
int loop_chunks(const usac_ctx *c, uint32_t B) {
    if (listed(c)) return c->chunks;
    const uint32_t tiles = (B + 63) / 64;
    int ch = c->chunks;
    while (ch < 16 && tiles * (uint32_t)ch < 4096u) ch *= 2;
    return ch;
}

// exact single-model inliers into c->inl_idx / inl_cnt / inl_sum (device)
hipError_t enqueue_inliers(usac_ctx *c, const float *model_dev, float thr) {
    hipError_t e = c->inl_scratch.reserve(usac::inliers_scratch_bytes(c->n, 1));
    if (e != hipSuccess) return e;
    return usac::launch_inliers(c->stream, c->estimator, c->pts.p, c->n, model_dev, thr, c->inl_idx.as<int32_t>(),
                                c->inl_cnt.as<int32_t>(), c->inl_sum.as<float>(), c->inl_scratch.p);
}

// ns_dev (nullable): the fit's point count on the device, n then only a bound on it
hipError_t enqueue_nonminimal(usac_ctx *c, const int32_t *idx_dev, uint32_t n, float *model_out = nullptr,
                              int32_t *ok_out = nullptr, const float *weights_dev = nullptr,
                              const uint32_t *ns_dev = nullptr, usac::NmBatch *batch_out = nullptr) {
    hipError_t e = c->nm_seq.reserve(usac::nonminimal_seq_bytes(n, 1));
    if (e != hipSuccess) return e;
    usac::NmBatch b{};
    // batch_out: the fit stops before its finish (NmBatch::skip_finish) and the batch is handed
    // back for launch_finish_score
    b.seq = c->nm_seq.p;
    b.base = idx_dev;
    b.n1 = n;
    b.W = 1;
    b.nmax = n;
    b.ns = ns_dev;
    b.fused_any = ns_dev != nullptr;
    b.q = c->q.p;
    b.partial = c->partial.as<double>();
    b.ws = c->ws.as<float>();
    b.model_out = model_out ? model_out : c->nm_model.as<float>();
    b.ok = ok_out ? ok_out : c->nm_ok.as<int32_t>();
    if (weights_dev) {
        if ((e = c->nm_qw.reserve(sizeof(float) * 4 * (size_t)n)) != hipSuccess) return e;
        b.weights = weights_dev;
        b.qw = c->nm_qw.p;
    }
    b.skip_finish = batch_out != nullptr;
    if (batch_out) *batch_out = b;
    return usac::launch_nonminimal_batch(c->stream, c->estimator, c->pts.p, b);
}

// The ranks of a sharded run and their all-gather of host bytes: the gather callback when one
// is given, else RCCL on the context's communicator (staged through device buffers).  Every
// payload is prefixed by the sender's status word, so a rank whose local part failed still
// joins the collective and every rank then fails with the first failing rank's status.
struct Shard {
    int nranks = 1, rank = 0;
    usac_allgather_fn gather = nullptr;
    void *user = nullptr;
};

int shard_allgather(usac_ctx *c, const Shard &sh, int status, const void *send, size_t bytes,
                    std::vector<uint8_t> &recv) {
    const size_t rb = 8 + ((bytes + 7) & ~(size_t)7);  // status word padded to 8, payload
    std::vector<uint8_t> mine(rb, 0);
    memcpy(mine.data(), &status, sizeof(status));
    if (bytes) memcpy(mine.data() + 8, send, bytes);
    recv.resize(rb * (size_t)sh.nranks);
    if (sh.gather) {
        if (sh.gather(sh.user, mine.data(), rb, recv.data()) != 0)
            return fail(c, USAC_ERR_ARG, "all-gather callback failed (gather callbacks must fail on every rank)");
    } else {
        if (!c->comm) return fail(c, USAC_ERR_ARG, "sharded run without a communicator");
        HIP_TRY(c, c->x_send.reserve(rb));
        HIP_TRY(c, c->x_recv.reserve(rb * (size_t)sh.nranks));
        pinned_vector<uint8_t> st(rb * (size_t)(sh.nranks + 1));
        memcpy(st.data(), mine.data(), rb);
        HIP_TRY(c, hipMemcpyAsync(c->x_send.p, st.data(), rb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, order_after_exchanges(c));
        NCCL_TRY(c, ncclAllGather(c->x_send.p, c->x_recv.p, rb, ncclUint8, c->comm, c->stream));
        HIP_TRY(c, mark_collective(c));
        HIP_TRY(c, hipMemcpyAsync(st.data() + rb, c->x_recv.p, rb * (size_t)sh.nranks, hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, stream_wait(c->stream));
        memcpy(recv.data(), st.data() + rb, rb * (size_t)sh.nranks);
    }
    for (int r = 0; r < sh.nranks; r++) {
        int32_t st;
        memcpy(&st, recv.data() + (size_t)r * rb, sizeof(st));
        if (st != USAC_OK)
            return r == sh.rank ? st : fail(c, st, "sharded run: rank " + std::to_string(r) + " failed (status " +
                                                        std::to_string(st) + ")");
    }
    // payloads only, rank after rank (bytes each)
    for (int r = 0; r < sh.nranks; r++) memmove(recv.data() + (size_t)r * bytes, recv.data() + (size_t)r * rb + 8, bytes);
    recv.resize(bytes * (size_t)sh.nranks);
    return USAC_OK;
}

// LO-RANSAC: InnerLocalOptimization::GetModelScore (inner_local_optimization.hpp:74-133) with
// IterativeLocalOptimization (iterative_local_optimization.hpp:61-136).  lo_model's threshold
// persists across calls and compounds like the reference's; the LO mt19937 is
// seeded with seed + 1 (the reference: std::random_device).
//
// The reference runs its <= 20 inner iterations one after the other, each a chain of up to
// five dependent (least-squares fit -> scored inlier list) steps whose sequential fp32 sums
// make every step latency-bound.  Inner iteration j depends on the earlier ones only through
// (a) the best model / inlier list, which changes only when an iteration improves it,
// (b) the generator, which (unlimited variant) only the inner sample draws advance, and
// (c) the LO threshold each iteration starts from.  So all remaining iterations run at once
// as speculative chains: their samples are drawn up front under "no improvement", each starts
// from the threshold the previous one would leave after a completed iterative stage, and the
// chains advance in lockstep -- one batched fit launch, then one batched scoring launch, per
// stage (kernels_nonmin.hip / kernels_inliers.hip, W fits at once).  The host then replays
// the iterations in order with the reference's exact control flow: a chain whose start
// threshold was mis-predicted, or every chain after one that improved the best, is discarded
// and the speculation restarts there with the generator rewound to just after the last kept
// draw.  Every kept result is bit-identical to the sequential order.  The limited variant
// (InItFLORsc) draws inside the iterative stage, so it runs one chain at a time.
struct LoRansac {
    enum Phase { INNER_FIT, INNER_SCORE, ITER_FIT, ITER_SCORE, DONE };
    enum Outcome { RETURN, SKIP, FEW, ITERATED };
    struct Chain {
        float thr_start = 0.f, thr = 0.f;
        Phase phase = DONE;
        Outcome outcome = SKIP;
        int lo_cnt = 0;
        float lo_sum = 0.f;
        uint32_t it = 0, iter_count = 0;
        int32_t failed = 0, fit_pos = 0;
        float model[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        // the model and threshold that produced the chain's inlier list (its last successful
        // fit's scoring): a rank that does not own the chain rebuilds the list from them
        float list_model[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        float list_thr = 0.f;
    };

    usac_ctx *c;
    Shard sh;  // sharded run: chain w runs on rank w % nranks (unlimited variant only)
    usac::Mt19937 g;
    bool limited;
    uint32_t inner, iters, limit, mult, m, n, wmax;
    float theta, lo_thr, step;
    uint32_t inner_count = 0, iterative_count = 0;
    uint32_t rounds = 0, stages = 0, fits = 0;  // speculation rounds, device stages, fits (statistics)
    double t_enqueue = 0.0, t_poll = 0.0;          // host ms spent enqueuing stages / waiting for them (USAC_PROFILE)
    int rc = USAC_OK;
    // entry best of the current call
    int best_cnt = 0;
    float best_sum = 0.f;
    std::vector<Chain> ch;
    std::vector<usac::Mt19937> g_after;  // generator after chain w's inner draw
    // A stage's inputs (ns, thresholds, slots, LSQ positions) and outputs (models, fit flags,
    // counts, Σ) as one pinned host block mirrored by one device block, one copy each way; two
    // such pairs (and two scoring scratch areas), by stage parity, so that a pipelined round
    // can have stage k + 1 on the device while the host reads stage k.
    void *pin = nullptr;
    size_t pin_bytes = 0, in_bytes = 0, out_bytes = 0, scr_bytes = 0;
    uint32_t *hns = nullptr, *hslots = nullptr;
    int32_t *hpos = nullptr, *hcnt = nullptr, *hok = nullptr;
    float *hthr = nullptr, *hsum = nullptr, *hmod = nullptr;
    float *hmodel = nullptr;  // pinned slot of the model a round starts from (its H2D copy)
    uint32_t *dns = nullptr, *dslots = nullptr;
    int32_t *dpos = nullptr, *dcnt = nullptr, *dok = nullptr;
    float *dthr = nullptr, *dsum = nullptr, *dmod = nullptr;
    int next_par = 0;  // block parity of the next pipelined stage (alternates across rounds too)

    LoRansac(usac_ctx *ctx, const usac_params *p, const Shard &shard)
        : c(ctx),
          sh(shard),
          g(p->seed + 1u),
          limited(p->lo == USAC_LO_INITFLORSC),
          inner(p->lo_inner_iterations),
          iters(p->lo_iterative_iterations),
          limit(p->lo_sample_size),
          mult(p->lo_threshold_multiplier),
          m(ctx->m),
          n(ctx->n),
          wmax(std::max<uint32_t>(1u, p->lo == USAC_LO_INITFLORSC ? 1u : p->lo_inner_iterations)),
          theta(p->threshold),
          lo_thr(p->threshold),
          step((p->threshold * p->lo_threshold_multiplier - p->threshold) / p->lo_iterative_iterations),
          ch(wmax),
          g_after(wmax, usac::Mt19937(0)) {}
    ~LoRansac() {
        if (pin) {  // a pipelined round's unread last stage may still copy into the blocks
            (void)hipStreamSynchronize(c->stream);
            if (c->lo_stream) (void)hipStreamSynchronize(c->lo_stream);
            PinnedPool::get().give_back(pin, pin_bytes);
        }
    }

    int reserve() {
        const size_t W = wmax, N = n, L = std::max<uint32_t>(1u, limit);
        HIP_TRY(c, c->lo_max.reserve(sizeof(int32_t) * N));
        HIP_TRY(c, c->lo_lists.reserve(sizeof(int32_t) * N * W));
        in_bytes = sizeof(uint32_t) * (3 * W + W * L);
        out_bytes = sizeof(float) * 12 * W;
        HIP_TRY(c, c->lo_io.reserve(2 * (in_bytes + out_bytes)));
        pin = PinnedPool::get().take(2 * (in_bytes + out_bytes) + sizeof(float) * 16, &pin_bytes);
        if (!pin) return fail(c, USAC_ERR_HIP, "hipHostMalloc (LO staging) failed");
        hmodel = reinterpret_cast<float *>(static_cast<char *>(pin) + 2 * (in_bytes + out_bytes));
        if (!limited && !c->lo_stream) {
            HIP_TRY(c, StreamPool::get().stream(&c->lo_stream));
            for (auto &ev : c->lo_ev) HIP_TRY(c, StreamPool::get().event(&ev));
        }
        set_block(0);
        HIP_TRY(c, c->lo_q.reserve(sizeof(float) * c->cols * N * W));
        HIP_TRY(c, c->lo_part.reserve(sizeof(double) * usac::nonminimal_partial_stride(n) * W));
        HIP_TRY(c, c->nm_seq.reserve(usac::nonminimal_seq_bytes(n, (uint32_t)W)));
        HIP_TRY(c, c->lo_ws.reserve(sizeof(float) * 18 * W));
        scr_bytes = usac::inliers_scratch_bytes(n, wmax);
        HIP_TRY(c, c->lo_scr.reserve(2 * scr_bytes));
        return USAC_OK;
    }

    // the host and device blocks of parity b: inputs then outputs (layout of both)
    void set_block(int b) {
        const size_t W = wmax, L = std::max<uint32_t>(1u, limit);
        auto lay = [&](uint32_t *w, uint32_t *&ns, float *&thr, uint32_t *&slots, int32_t *&pos, float *&mod,
                       int32_t *&ok, int32_t *&cnt, float *&sum) {
            ns = w;
            thr = reinterpret_cast<float *>(w + W);
            slots = w + 2 * W;
            pos = reinterpret_cast<int32_t *>(w + 3 * W);
            mod = reinterpret_cast<float *>(w + 3 * W + W * L);
            ok = reinterpret_cast<int32_t *>(mod + 9 * W);
            cnt = ok + W;
            sum = reinterpret_cast<float *>(cnt + W);
        };
        const size_t off = (size_t)b * (in_bytes + out_bytes) / sizeof(uint32_t);
        lay(static_cast<uint32_t *>(pin) + off, hns, hthr, hslots, hpos, hmod, hok, hcnt, hsum);
        lay(c->lo_io.as<uint32_t>() + off, dns, dthr, dslots, dpos, dmod, dok, dcnt, dsum);
    }
    void *scr(int b) const { return static_cast<char *>(c->lo_scr.p) + (size_t)b * scr_bytes; }
    int poll(hipEvent_t ev) {
        for (uint32_t spins = 0;; spins++) {
            const hipError_t e = hipEventQuery(ev);
            if (e == hipSuccess) return USAC_OK;
            if (e != hipErrorNotReady) return fail(c, USAC_ERR_HIP, std::string("LO stage: ") + hipGetErrorString(e));
            if ((spins & 1023u) == 1023u) std::this_thread::yield();
        }
    }
    static bool bigger(int c1, float s1, int c2, float s2) { return c1 > c2 || (c1 == c2 && s1 > s2); }
    // chains of this rank: all of them unless the run is sharded.  The limited variant draws
    // inside its iterative stage (one chain, the generator moves), so it is never split.
    bool own(uint32_t w) const { return sh.nranks == 1 || limited || (int)(w % (uint32_t)sh.nranks) == sh.rank; }

    // the threshold an inner iteration leaves when its iterative stage runs all its steps
    float predict(float t) const {
        t = (float)mult * t;
        for (uint32_t k = 0; k < iters; k++) t -= step;
        return fabsf(t - theta) > 0.00001 ? theta : t;
    }

    // IterativeLocalOptimization loop head: decrement, the break tests, then the next fit
    void iter_head(Chain &h, uint32_t w) {
        for (;;) {
            if (h.it >= iters) return finish(h);
            h.thr -= step;
            if (h.lo_cnt <= (int)m) return finish(h);
            h.fit_pos = false;
            if (limited && h.lo_cnt > (int)limit) {  // GetScoreLimited: a random subset of lo_inliers
                usac::unique_set(g, hpos + (size_t)w * limit, limit, (uint32_t)(h.lo_cnt - 1));
                h.fit_pos = true;
            }
            h.phase = ITER_FIT;
            return;
        }
    }
    void finish(Chain &h) {
        h.failed = fabsf(h.thr - theta) > 0.00001;  // double literal, as the reference
        if (h.failed) h.thr = theta;
        h.outcome = ITERATED;
        h.phase = DONE;
    }

    // one lockstep stage: the batched fit of every chain in INNER_FIT / ITER_FIT and, in the
    // same submission, the batched scoring of the fitted models at the threshold each chain
    // scores with after its fit (inner: K * thr, iterative: the already decremented thr); the
    // scoring leaves the index list of a failed fit alone (the limited variant refits from it).
    // One host synchronisation per stage; then every chain's state machine takes the fit
    // outcome and, if the fit succeeded, the score.  (A chain in a SCORE phase only arises
    // without a fused fit -- never here -- so it is scored on its own.)
    int stage(uint32_t W, int inner_cnt) {
        bool fit = false, score = false, inner_fit = false, iter_fit = false, pos = false;
        uint32_t nmax = 0, ns = 0;
        for (uint32_t w = 0; w < W; w++) {
            const Chain &h = ch[w];
            hns[w] = 0;
            if (!own(w)) continue;
            if (h.phase == INNER_FIT || h.phase == ITER_FIT) {
                fit = true;
                bool p;
                if (h.phase == INNER_FIT) {
                    inner_fit = true;
                    p = inner_cnt > (int)limit;
                    hns[w] = p ? limit : (uint32_t)inner_cnt;
                    hthr[w] = (float)mult * h.thr;
                } else {
                    iter_fit = true;
                    p = h.fit_pos;
                    hns[w] = p ? limit : (uint32_t)h.lo_cnt;
                    hthr[w] = h.thr;
                }
                pos = pos || p;
                fits++;
                hslots[ns++] = w;
                nmax = std::max(nmax, hns[w]);
            } else if (h.phase == INNER_SCORE || h.phase == ITER_SCORE) {
                score = true;
                hslots[ns++] = w;
                hthr[w] = h.thr;
            }
        }
        // never: fit and score stages alternate, and inner fits only open a round
        if ((fit && score) || (inner_fit && iter_fit)) return fail(c, USAC_ERR_HIP, "LO chains out of lockstep");
        if (pos) {
            // the position list is per launch: a fitting chain without its own positions
            // (GetScoreLimited with lo_cnt <= limit, or an inner fit of <= limit points) fits
            // its first hns[w] list entries -- identity positions (hns[w] <= limit)
            for (uint32_t w = 0; w < W; w++) {
                const Chain &h = ch[w];
                const bool fitting = own(w) && (h.phase == INNER_FIT || h.phase == ITER_FIT);
                const bool own = h.phase == INNER_FIT ? inner_cnt > (int)limit : h.fit_pos;
                if (fitting && !own)
                    for (uint32_t i = 0; i < hns[w]; i++) hpos[(size_t)w * limit + i] = (int32_t)i;
            }
        }
        hipStream_t st = c->stream;
        HIP_TRY(c, hipMemcpyAsync(dns, hns, in_bytes, hipMemcpyHostToDevice, st));
        if (fit) {
            usac::NmBatch b{};
            b.base = inner_fit ? c->lo_max.as<int32_t>() : c->lo_lists.as<int32_t>();
            b.base_stride = inner_fit ? 0 : n;
            b.pos = pos ? dpos : nullptr;
            b.pos_stride = limit;
            b.ns = dns;
            b.W = W;
            b.nmax = nmax;
            b.q = c->lo_q.p;
            b.q_stride = n;
            b.partial = c->lo_part.as<double>();
            b.p_stride = usac::nonminimal_partial_stride(n);
            b.ws = c->lo_ws.as<float>();
            b.model_out = dmod;
            b.ok = dok;
            b.seq = c->nm_seq.p;
            HIP_TRY(c, usac::launch_nonminimal_batch(st, c->estimator, c->pts.p, b));
        }
        HIP_TRY(c, usac::launch_inliers_batch(st, c->estimator, c->pts.p, n, dmod, ns, 0.f, dthr, dslots,
                                              c->lo_lists.as<int32_t>(), n, dcnt, dsum, scr(0), fit ? dok : nullptr));
        HIP_TRY(c, hipMemcpyAsync(hmod, dmod, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, stream_wait(st));
        stages++;
        take(W, inner_cnt);
        return USAC_OK;
    }

    // the chains' state machines take a stage's outputs (host block in use: hmod, hok, hcnt,
    // hsum, hthr)
    void take(uint32_t W, int inner_cnt) {
        for (uint32_t w = 0; w < W; w++) {
            Chain &h = ch[w];
            if (!own(w)) continue;
            switch (h.phase) {
                case INNER_FIT:  // LeastSquaresFitting(lo_sample | max_inliers) -> lo_model
                    memcpy(h.model, hmod + 9 * (size_t)w, sizeof(h.model));
                    if (!hok[w]) {
                        h.outcome = inner_cnt > (int)limit ? SKIP : RETURN;
                        h.phase = DONE;
                    } else {
                        h.thr = (float)mult * h.thr;  // K * theta
                        scored_list(h, w);
                        inner_scored(h, w);
                    }
                    break;
                case INNER_SCORE:
                    inner_scored(h, w);
                    break;
                case ITER_FIT:
                    memcpy(h.model, hmod + 9 * (size_t)w, sizeof(h.model));
                    if (hok[w]) {
                        scored_list(h, w);
                        iter_scored(h, w);
                    } else if (h.fit_pos) {  // GetScoreLimited: continue
                        h.it++;
                        iter_head(h, w);
                    } else {
                        finish(h);  // break
                    }
                    break;
                case ITER_SCORE:
                    iter_scored(h, w);
                    break;
                default:
                    break;
            }
        }
    }
    // a fitted model was scored: lo_lists[w] now holds its inliers at the chain's threshold
    // (inner: K * theta, iterative: the already decremented one -- the stage's scoring threshold)
    void scored_list(Chain &h, uint32_t) {
        memcpy(h.list_model, h.model, sizeof(h.model));
        h.list_thr = h.thr;
    }
    // the inner iteration's scoring of lo_model at K * theta
    void inner_scored(Chain &h, uint32_t w) {
        h.lo_cnt = hcnt[w];
        h.lo_sum = hsum[w];
        if (h.lo_cnt <= (int)m) {
            h.outcome = FEW;
            h.phase = DONE;
        } else {
            h.it = 0;
            h.iter_count = 0;
            iter_head(h, w);
        }
    }
    // an iterative step's scoring of its fit
    void iter_scored(Chain &h, uint32_t w) {
        h.lo_cnt = hcnt[w];
        h.lo_sum = hsum[w];
        if (!limited && bigger(best_cnt, best_sum, h.lo_cnt, h.lo_sum)) {
            finish(h);  // GetScoreUnlimited: the best is bigger -> break
        } else {
            h.iter_count++;
            h.it++;
            iter_head(h, w);
        }
    }

    // ---- pipelined rounds (the unlimited variant): stage k + 1 is on the device while the
    // host reads stage k.  Everything a stage needs is known before stage k's outputs are read
    // except the point counts of its fits: each chain's threshold follows a fixed schedule
    // (K * theta_start, then one step less per iterative fit), its list is on the device, and
    // the fit's gather derives its n from stage k's outputs on the device -- zero, a no-op fit
    // and scoring that leave the chain's list alone, once the chain has certainly stopped
    // (failed fit, <= m inliers, fewer inliers than the best).  A count tie with the best
    // needs Σ to decide; the device continues such a chain, and if the host's state machine
    // (which reads every stage in order, exactly as the sequential stages did) stops it, its
    // later speculative fits are never read -- a chain stopped by the comparison never
    // improves the best, so its list is never used either.  The scoring's Σ runs on the side
    // stream beside the next stage's fit.  The stage after a round's last is usually already
    // queued: it runs for nothing, ordered before every later use of the LO buffers.
    int enqueue_pipe(uint32_t k, uint32_t W, int inner_cnt) {
        const int b = next_par;
        next_par ^= 1;
        set_block(b ^ 1);  // the previous stage's device block (the count derivation's inputs)
        const uint32_t *pns = dns;
        const int32_t *pok = dok, *pcnt = dcnt;
        const float *pthr = dthr;
        set_block(b);
        hipStream_t st = c->stream;
        const bool pos = k == 0 && inner_cnt > (int)limit;
        uint32_t nmax = 0;
        if (k == 0) {  // the round's inner fits: inputs from the host
            for (uint32_t w = 0; w < W; w++) {
                hslots[w] = w;
                hthr[w] = (float)mult * ch[w].thr_start;
                hns[w] = own(w) ? (pos ? limit : (uint32_t)inner_cnt) : 0u;
                nmax = std::max(nmax, hns[w]);
            }
            HIP_TRY(c, hipMemcpyAsync(dns, hns, in_bytes, hipMemcpyHostToDevice, st));
        }
        // iterative fits: counts and thresholds derived on the device from the previous stage
        // (by the fit's first kernel)
        const usac::LoPrep prep{pns, pok, pcnt, pthr, dns, dthr, (int32_t)m, best_cnt, k > 1 ? 1 : 0, step};
        usac::NmBatch nb{};
        nb.base = k == 0 ? c->lo_max.as<int32_t>() : c->lo_lists.as<int32_t>();
        nb.base_stride = k == 0 ? 0 : n;
        nb.pos = pos ? dpos : nullptr;
        nb.pos_stride = limit;
        nb.ns = dns;
        nb.W = W;
        nb.nmax = k == 0 ? nmax : n;  // iterative fits: n bounds the counts on the device
        nb.fused_any = k > 0;
        nb.prep = k > 0 ? &prep : nullptr;
        nb.q = c->lo_q.p;
        nb.q_stride = n;
        nb.partial = c->lo_part.as<double>();
        nb.p_stride = usac::nonminimal_partial_stride(n);
        nb.ws = c->lo_ws.as<float>();
        nb.model_out = dmod;
        nb.ok = dok;
        nb.seq = c->nm_seq.p;
        HIP_TRY(c, usac::launch_nonminimal_batch(st, c->estimator, c->pts.p, nb));
        HIP_TRY(c, usac::launch_inliers_batch(st, c->estimator, c->pts.p, n, dmod, W, 0.f, dthr, nullptr,
                                              c->lo_lists.as<int32_t>(), n, dcnt, nullptr, scr(b), dok));
        // the side stream: Σ, then every output of the stage into the host block
        HIP_TRY(c, hipEventRecord(c->lo_ev[b], st));
        HIP_TRY(c, hipStreamWaitEvent(c->lo_stream, c->lo_ev[b], 0));
        HIP_TRY(c, usac::launch_inliers_sums(c->lo_stream, n, W, nullptr, dcnt, dsum, scr(b)));
        HIP_TRY(c, hipMemcpyAsync(hmod, dmod, out_bytes, hipMemcpyDeviceToHost, c->lo_stream));
        HIP_TRY(c, hipEventRecord(c->lo_ev[2 + b], c->lo_stream));
        return USAC_OK;
    }

    int round_pipe(uint32_t W, int inner_cnt) {
        const int b0 = next_par;
        uint32_t queued = 0;  // stages 0 .. queued - 1 are on the device
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::milli>(b - a).count();
        };
        auto t0 = now();
        int r = enqueue_pipe(queued++, W, inner_cnt);
        if (!r && iters > 0) r = enqueue_pipe(queued++, W, inner_cnt);
        t_enqueue += ms(t0, now());
        for (uint32_t k = 0; !r; k++) {
            const int b = (b0 + (int)k) & 1;
            t0 = now();
            r = poll(c->lo_ev[2 + b]);
            t_poll += ms(t0, now());
            if (r) break;
            set_block(b);
            for (uint32_t w = 0; w < W; w++)
                if (own(w) && (ch[w].phase == INNER_FIT || ch[w].phase == ITER_FIT)) fits++;
            stages++;
            take(W, inner_cnt);
            bool active = false;
            for (uint32_t w = 0; w < W; w++) active |= own(w) && ch[w].phase != DONE;
            if (!active) break;
            // an active chain fits again at stage k + 1 <= iters, which is queued
            if (queued < k + 2) {
                r = fail(c, USAC_ERR_HIP, "LO pipeline out of step");
                break;
            }
            if (k + 2 <= iters && queued == k + 2) {
                t0 = now();
                r = enqueue_pipe(queued++, W, inner_cnt);
                t_enqueue += ms(t0, now());
            }
        }
        // later main-stream users of the LO scratch wait for the side stream's last Σ pass
        if (!r) {
            hipError_t e = hipEventRecord(c->lo_ev[4], c->lo_stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->lo_ev[4], 0);
            if (e != hipSuccess) r = fail(c, USAC_ERR_HIP, std::string("LO stage: ") + hipGetErrorString(e));
        } else {
            (void)hipStreamSynchronize(c->stream);
            (void)hipStreamSynchronize(c->lo_stream);
        }
        return r;
    }

    // GetModelScore(best_model, best_score): model / (cnt, sum) improved in place
    void run(float *model, int &cnt, float &sum) {
        if (cnt < 12 || rc) return;
        // quality->getInliers(best_model) -> max_inliers (device)
        memcpy(hmodel, model, sizeof(float) * 9);  // (the previous round's copy has completed)
        hipError_t e = hipMemcpyAsync(c->one_model.p, hmodel, sizeof(float) * 9, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = c->inl_scratch.reserve(usac::inliers_scratch_bytes(n, 1));
        if (e == hipSuccess)
            e = usac::launch_inliers(c->stream, c->estimator, c->pts.p, n, c->one_model.as<float>(), theta,
                                     c->lo_max.as<int32_t>(), c->inl_cnt.as<int32_t>(), c->inl_sum.as<float>(),
                                     c->inl_scratch.p);
        if (e != hipSuccess) {
            rc = fail(c, USAC_ERR_HIP, std::string("LO inliers: ") + hipGetErrorString(e));
            return;
        }
        uint32_t j0 = 0;
        while (j0 < inner && !rc) {
            // speculate iterations j0 .. j0 + W - 1 under "no improvement"
            const uint32_t W = std::min(wmax, inner - j0);
            const usac::Mt19937 g_before = g;
            best_cnt = cnt;
            best_sum = sum;
            float t = lo_thr;
            set_block(limited ? 0 : next_par);  // the round's first stage block (its LSQ positions)
            for (uint32_t w = 0; w < W; w++) {
                Chain &h = ch[w];
                h = Chain();
                h.thr_start = h.thr = t;
                h.phase = INNER_FIT;
                if (cnt > (int)limit) {
                    usac::unique_set(g, hpos + (size_t)w * limit, limit, (uint32_t)(cnt - 1));
                }
                g_after[w] = g;
                t = predict(t);
            }
            rounds++;
            int st = USAC_OK;
            if (!limited) {
                st = round_pipe(W, cnt);
            } else {
                for (;;) {
                    bool active = false;
                    for (uint32_t w = 0; w < W; w++) active |= own(w) && ch[w].phase != DONE;
                    if (!active) break;
                    if ((st = stage(W, cnt))) break;
                }
            }
            if (sh.nranks > 1 && !limited) {  // every rank's chains, one all-gather per round
                std::vector<uint8_t> all;
                if ((rc = shard_allgather(c, sh, st, ch.data(), sizeof(Chain) * W, all))) return;
                for (uint32_t w = 0; w < W; w++)
                    if (!own(w))
                        memcpy(&ch[w], all.data() + sizeof(Chain) * ((size_t)(w % (uint32_t)sh.nranks) * W + w),
                               sizeof(Chain));
            } else if ((rc = st)) {
                return;
            }
            if (limited) g_after[0] = g;  // the iterative stage's draws
            // replay in order
            bool restart = false;
            uint32_t w = 0;
            for (; w < W; w++) {
                const Chain &h = ch[w];
                if (memcmp(&h.thr_start, &lo_thr, sizeof(float)) != 0) {  // mis-predicted start
                    g = w ? g_after[w - 1] : g_before;
                    j0 += w;
                    restart = true;
                    break;
                }
                if (h.outcome == RETURN) {
                    g = g_after[w];
                    return;
                }
                if (h.outcome == SKIP) continue;
                lo_thr = h.thr;
                if (h.outcome == FEW) continue;
                iterative_count += h.iter_count;
                inner_count++;
                if (!h.failed && bigger(h.lo_cnt, h.lo_sum, cnt, sum)) {
                    memcpy(model, h.model, sizeof(h.model));
                    cnt = h.lo_cnt;
                    sum = h.lo_sum;
                    if (own(w)) {
                        e = hipMemcpyAsync(c->lo_max.p, c->lo_lists.as<int32_t>() + (size_t)w * n,
                                           sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToDevice, c->stream);
                    } else {  // another rank's chain: its list is the inliers of (list_model, list_thr)
                        memcpy(hmodel, h.list_model, sizeof(float) * 9);
                        e = hipMemcpyAsync(c->one_model.p, hmodel, sizeof(float) * 9, hipMemcpyHostToDevice, c->stream);
                        if (e == hipSuccess)
                            e = usac::launch_inliers(c->stream, c->estimator, c->pts.p, n, c->one_model.as<float>(),
                                                     h.list_thr, c->lo_max.as<int32_t>(), c->inl_cnt.as<int32_t>(),
                                                     c->inl_sum.as<float>(), c->inl_scratch.p);
                        // hmodel is reused by the next H2D copy: that copy is queued behind this one
                        if (e == hipSuccess) e = stream_wait(c->stream);
                    }
                    if (e != hipSuccess) {
                        rc = fail(c, USAC_ERR_HIP, std::string("LO inliers copy: ") + hipGetErrorString(e));
                        return;
                    }
                    g = g_after[w];
                    j0 += w + 1;
                    restart = true;
                    break;
                }
            }
            if (!restart) {
                g = g_after[W - 1];
                j0 += W;
            }
        }
    }
};

constexpr uint32_t kExactSumsMax = 64;  // models per exact_sums launch

// exact_sums' buffers at their full size, before the loop: growing a DevBuf synchronises the
// device, and under the speculation that waited for the speculative batch (plus a hipMalloc) --
// 0.47 ms a cfg5 run (USAC_PROFILE, round 4)
int reserve_exact_sums(usac_ctx *c) {
    HIP_TRY(c, c->lo_models.reserve(sizeof(float) * 9 * kExactSumsMax));
    HIP_TRY(c, c->lo_cnts.reserve(sizeof(int32_t) * kExactSumsMax));
    HIP_TRY(c, c->lo_sums.reserve(sizeof(float) * kExactSumsMax));
    HIP_TRY(c, c->lo_scr.reserve(usac::inliers_scratch_bytes(c->n, kExactSumsMax)));
    return USAC_OK;
}

// Σerr where the replay can read it.  The loop compares a model's Σ only against the running
// best with an equal count, and stores it only when the model becomes the best (Score::bigger,
// quality.hpp:22-31); both need count >= the running best count, which is at least
// max(best count at batch start, every earlier count of the batch).  So only the slots whose
// count reaches that running maximum get the reference's sequential fp32 sum -- computed
// exactly on the device, 64 models per launch (launch_inliers_batch) -- and the batch itself
// is scored by the fast multi-chunk kernel, whose counts are exact.  Other slots' sums are
// never read.  The recount doubles as a check of the fast kernel's counts.
int exact_sums(usac_ctx *c, float thr, int best_count, const int32_t *hc, const float *hmod, size_t SB, size_t S,
               float *hsum, uint32_t *n_models) {
    constexpr uint32_t kMax = kExactSumsMax;
    std::vector<uint32_t> cand;
    int run_max = best_count;
    for (size_t sl = 0; sl < S; sl++) {
        if (hc[sl] < 0) continue;
        if (hc[sl] >= run_max) {
            cand.push_back((uint32_t)sl);
            run_max = hc[sl];
        }
    }
    if (cand.empty()) return USAC_OK;
    const int nc = ncomp(c);
    pinned_vector<float> am(9 * (size_t)kMax);
    pinned_vector<int32_t> cc(kMax);
    pinned_vector<float> cs(kMax);
    HIP_TRY(c, c->lo_models.reserve(sizeof(float) * 9 * kMax));
    HIP_TRY(c, c->lo_cnts.reserve(sizeof(int32_t) * kMax));
    HIP_TRY(c, c->lo_sums.reserve(sizeof(float) * kMax));
    HIP_TRY(c, c->lo_scr.reserve(usac::inliers_scratch_bytes(c->n, kMax)));
    for (size_t k0 = 0; k0 < cand.size(); k0 += kMax) {
        const uint32_t K = (uint32_t)std::min<size_t>(kMax, cand.size() - k0);
        for (uint32_t k = 0; k < K; k++)
            for (int e = 0; e < 9; e++) am[9 * k + e] = e < nc ? hmod[(size_t)e * SB + cand[k0 + k]] : 0.f;
        HIP_TRY(c, hipMemcpyAsync(c->lo_models.p, am.data(), sizeof(float) * 9 * K, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, usac::launch_inliers_batch(c->stream, c->estimator, c->pts.p, c->n, c->lo_models.as<float>(), K, thr,
                                              nullptr, nullptr, nullptr, 0, c->lo_cnts.as<int32_t>(),
                                              c->lo_sums.as<float>(), c->lo_scr.p));
        HIP_TRY(c, hipMemcpyAsync(cc.data(), c->lo_cnts.p, sizeof(int32_t) * K, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(cs.data(), c->lo_sums.p, sizeof(float) * K, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, stream_wait(c->stream));
        for (uint32_t k = 0; k < K; k++) {
            if (cc[k] != hc[cand[k0 + k]])
                return fail(c, USAC_ERR_HIP, "score kernel count differs from the exact recount (slot " +
                                                 std::to_string(cand[k0 + k]) + ": " + std::to_string(hc[cand[k0 + k]]) +
                                                 " vs " + std::to_string(cc[k]) + ")");
            hsum[cand[k0 + k]] = cs[k];
        }
    }
    *n_models += (uint32_t)cand.size();
    return USAC_OK;
}

// Graph-cut LO: GraphCut::GetModelScore (graphcut.hpp:99-153) with GraphCut::labeling
// (graphcut.cpp:7-101).  Per labelling: the device computes every point's exact residual
// under the best model; the host turns them into the reference's energies -- unary
// exp(-(e*e) / (2 thr^2)) (float argument, double exp as the reference's unqualified exp of
// a float), pairwise terms over the KNN (device usac_knn) or grid neighbour lists, skipping
// non-submodular / NaN terms, lambda = spatial_coherence_gc as given (model.hpp:33 default 0.1;
// graphcut.hpp:43 uses it unchanged, 0 = no pairwise term) -- and runs
// the reference's BK min cut (usac_maxflow.hpp); inliers = SINK nodes.  The <=
// lo_inner_iterations least-squares fits on 7m-point subsets of the labelling's inliers do
// not depend on each other (only the comparisons with the best do), so all of them run as
// one batched fit and one batched scoring on the device, then the host replays them in
// order (a failed fit ends the round; the generator is rewound to just after its draw).
// Its mt19937 is seeded with seed + 1 (reference: std::random_device).
struct GcLo {
    usac_ctx *c;
    usac::Mt19937 g;
    uint32_t inner, m, n, limit;
    float thr, lambda, sqr_thr;
    const int32_t *knn_tab;
    uint32_t knn;
    const usac::GridNeighbors *grid;
    uint32_t gc_iters = 0, labelings = 0, stages = 0;
    int rc = USAC_OK;
    std::vector<float> err, en, hsum, hmod;
    std::vector<int32_t> inl, hpos, hcnt, hok;
    std::vector<usac::Mt19937> g_after;

    GcLo(usac_ctx *ctx, const usac_params *p, const int32_t *knn_table, uint32_t k, const usac::GridNeighbors *gr)
        : c(ctx),
          g(p->seed + 1u),
          inner(p->lo_inner_iterations),
          m(ctx->m),
          n(ctx->n),
          limit(7 * ctx->m),
          thr(p->threshold),
          lambda(p->spatial_coherence_gc),
          sqr_thr(2 * p->threshold * p->threshold),
          knn_tab(knn_table),
          knn(k),
          grid(gr),
          err(ctx->n),
          en(ctx->n),
          hsum(std::max<uint32_t>(1u, p->lo_inner_iterations)),
          hmod(9 * (size_t)std::max<uint32_t>(1u, p->lo_inner_iterations)),
          inl(ctx->n),
          hpos((size_t)7 * ctx->m * std::max<uint32_t>(1u, p->lo_inner_iterations)),
          hcnt(std::max<uint32_t>(1u, p->lo_inner_iterations)),
          hok(std::max<uint32_t>(1u, p->lo_inner_iterations)),
          g_after(std::max<uint32_t>(1u, p->lo_inner_iterations), usac::Mt19937(0)) {}

    int reserve() {
        const size_t W = std::max<uint32_t>(1u, inner);
        HIP_TRY(c, c->lo_max.reserve(sizeof(int32_t) * n));
        HIP_TRY(c, c->lo_pos.reserve(sizeof(int32_t) * hpos.size()));
        HIP_TRY(c, c->lo_models.reserve(sizeof(float) * 9 * W));
        HIP_TRY(c, c->lo_ok.reserve(sizeof(int32_t) * W));
        HIP_TRY(c, c->lo_cnts.reserve(sizeof(int32_t) * W));
        HIP_TRY(c, c->lo_sums.reserve(sizeof(float) * W));
        HIP_TRY(c, c->lo_q.reserve(sizeof(float) * c->cols * limit * W));
        HIP_TRY(c, c->lo_part.reserve(sizeof(double) * usac::nonminimal_partial_stride(limit) * W));
        HIP_TRY(c, c->nm_seq.reserve(usac::nonminimal_seq_bytes(limit, (uint32_t)W)));
        HIP_TRY(c, c->lo_ws.reserve(sizeof(float) * 18 * W));
        HIP_TRY(c, c->lo_scr.reserve(usac::inliers_scratch_bytes(n, (uint32_t)W)));
        HIP_TRY(c, c->gc_err.reserve(sizeof(float) * n));
        return USAC_OK;
    }

    static bool bigger(int c1, float s1, int c2, float s2) { return c1 > c2 || (c1 == c2 && s1 > s2); }

    // GraphCut::labeling -> number of SINK nodes, their ascending list in inl (host) and lo_max
    int labeling(const float *model) {
        HIP_TRY(c, hipMemcpyAsync(c->one_model.p, model, sizeof(float) * 9, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, usac::launch_point_errors(c->stream, c->estimator, c->pts.p, n, c->one_model.as<float>(),
                                             c->gc_err.as<float>()));
        HIP_TRY(c, hipMemcpyAsync(err.data(), c->gc_err.p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, stream_wait(c->stream));
        for (uint32_t i = 0; i < n; i++) {
            const float d = err[i];
            en[i] = (float)std::exp((double)(-(d * d) / sqr_thr));
        }
        usac::BkGraph G((int)n, knn_tab ? (size_t)knn * n : (size_t)n);
        for (uint32_t i = 0; i < n; i++) G.add_node();
        for (uint32_t i = 0; i < n; i++) G.add_term1((int)i, en[i], 0.f);
        const float e01 = 1.f, e10 = 1.f;
        for (uint32_t i = 0; i < n; i++) {
            const float energy1 = en[i];
            const uint32_t cnt = knn_tab ? knn : grid->count(i);
            for (uint32_t k = 0; k < cnt; k++) {
                const int32_t j = knn_tab ? knn_tab[(size_t)knn * i + k] : grid->at(i, k);
                if (j == (int32_t)i || j < 0) continue;
                const float energy2 = en[j];
                const float e00 = (energy1 + energy2) / 2;
                const float e11 = 1 - e00;
                if (e00 + e11 > e01 + e10 || std::isnan(e00)) continue;
                G.add_term2((int)i, j, e00 * lambda, e01 * lambda, e10 * lambda, e11 * lambda);
            }
        }
        G.maxflow();
        int L = 0;
        for (uint32_t i = 0; i < n; i++)
            if (G.is_sink((int)i)) inl[L++] = (int32_t)i;
        if (L > 0)
            HIP_TRY(c, hipMemcpyAsync(c->lo_max.p, inl.data(), sizeof(int32_t) * L, hipMemcpyHostToDevice, c->stream));
        labelings++;
        return L;
    }

    void run(float *model, int &cnt, float &sum) {
        bool updated = true;
        while (updated && !rc) {
            updated = false;
            const int L = labeling(model);
            if (L < 0) {
                rc = L;
                return;
            }
            if (L <= (int)m) break;
            const bool sampled = (uint32_t)L > limit;
            const uint32_t W = std::min<uint32_t>(inner, sampled ? inner : 1u);
            if (W == 0) break;
            for (uint32_t w = 0; w < W; w++) {
                if (sampled) usac::unique_set(g, hpos.data() + (size_t)w * limit, limit, (uint32_t)(L - 1));
                g_after[w] = g;
            }
            if ((rc = fit_and_score(W, sampled ? limit : (uint32_t)L, sampled))) return;
            uint32_t w = 0;
            for (; w < W; w++) {
                if (!hok[w]) break;  // EstimateModelNonMinimalSample failed: end of this round
                if (bigger(hcnt[w], hsum[w], cnt, sum)) {
                    updated = true;
                    cnt = hcnt[w];
                    sum = hsum[w];
                    memcpy(model, hmod.data() + 9 * (size_t)w, sizeof(float) * 9);
                }
                gc_iters++;
            }
            g = g_after[w < W ? w : W - 1];
        }
    }

    // W least-squares fits (sampled positions into lo_max, or all npts of it) and their
    // (count, sequential sum) at the model threshold
    int fit_and_score(uint32_t W, uint32_t npts, bool sampled) {
        hipStream_t st = c->stream;
        if (sampled)
            HIP_TRY(c, hipMemcpyAsync(c->lo_pos.p, hpos.data(), sizeof(int32_t) * (size_t)W * limit,
                                      hipMemcpyHostToDevice, st));
        usac::NmBatch b{};
        b.base = c->lo_max.as<int32_t>();
        b.base_stride = 0;
        b.pos = sampled ? c->lo_pos.as<int32_t>() : nullptr;
        b.pos_stride = limit;
        b.n1 = npts;
        b.W = W;
        b.nmax = npts;
        b.q = c->lo_q.p;
        b.q_stride = limit;
        b.partial = c->lo_part.as<double>();
        b.p_stride = usac::nonminimal_partial_stride(limit);
        b.ws = c->lo_ws.as<float>();
        b.model_out = c->lo_models.as<float>();
        b.ok = c->lo_ok.as<int32_t>();
        b.seq = c->nm_seq.p;
        HIP_TRY(c, usac::launch_nonminimal_batch(st, c->estimator, c->pts.p, b));
        HIP_TRY(c, usac::launch_inliers_batch(st, c->estimator, c->pts.p, n, c->lo_models.as<float>(), W, thr, nullptr,
                                              nullptr, nullptr, 0, c->lo_cnts.as<int32_t>(), c->lo_sums.as<float>(),
                                              c->lo_scr.p));
        HIP_TRY(c, hipMemcpyAsync(hmod.data(), c->lo_models.p, sizeof(float) * 9 * W, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(hok.data(), c->lo_ok.p, sizeof(int32_t) * W, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(hcnt.data(), c->lo_cnts.p, sizeof(int32_t) * W, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(hsum.data(), c->lo_sums.p, sizeof(float) * W, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, stream_wait(st));
        stages++;
        return USAC_OK;
    }
};

// model.hpp:40 max_hypothesis_test_before_sprt (usac_params, ABI 12; 0 = the default 20)
static int max_before_sprt(const usac_params *p) {
    return p->max_hypothesis_test_before_sprt ? (int)p->max_hypothesis_test_before_sprt : 20;
}

bool rec_better(const usac_record &a, const usac_record &b) {
    if (!a.valid) return false;
    if (!b.valid) return true;
    if (a.inliers != b.inliers) return a.inliers > b.inliers;
    if (a.score != b.score) return a.score > b.score;
    return a.hyp_index < b.hyp_index;
}

}  // namespace

extern "C" {

int usac_abi_version(void) { return USAC_ABI_VERSION; }

int usac_create(usac_ctx **out, int device, int estimator, const float *pts, uint32_t n, uint32_t cols) {
    if (!out) return USAC_ERR_ARG;
    *out = nullptr;
    if (estimator != USAC_LINE2D && estimator != USAC_HOMOGRAPHY && estimator != USAC_FUNDAMENTAL &&
        estimator != USAC_ESSENTIAL)
        return USAC_ERR_UNSUPPORTED;
    if ((estimator == USAC_LINE2D) != (cols == 2) || (cols != 2 && cols != 4)) return USAC_ERR_ARG;
    if (n == 0 || !pts) return USAC_ERR_ARG;
    usac_ctx *c = new usac_ctx();
    c->device = device;
    c->estimator = estimator;
    c->n = n;
    c->cols = cols;
    c->m = estimator == USAC_LINE2D ? 2 : estimator == USAC_FUNDAMENTAL ? 7 : estimator == USAC_ESSENTIAL ? 5 : 4;
    c->spk = estimator == USAC_FUNDAMENTAL ? 3 : 1;
    // two-view scoring: a batch yields few models (about 0.4-1.3 per sample) and the few with
    // many inliers are much slower to score, so their point ranges are cut finer
    if (estimator == USAC_FUNDAMENTAL || estimator == USAC_ESSENTIAL) c->chunks = 96;
    int rc = USAC_OK;
    do {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { rc = fail(c, USAC_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e)); break; }
        e = StreamPool::get().stream(&c->stream);
        if (e != hipSuccess) { rc = fail(c, USAC_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); break; }
        for (auto &ev : c->ev) {
            e = StreamPool::get().event(&ev);
            if (e != hipSuccess) break;
        }
        if (e != hipSuccess) { rc = fail(c, USAC_ERR_HIP, "hipEventCreate failed"); break; }
        e = c->pts.reserve(sizeof(float) * (size_t)n * cols);
        if (e != hipSuccess) { rc = fail(c, USAC_ERR_HIP, "hipMalloc points failed"); break; }
        e = hipMemcpy(c->pts.p, pts, sizeof(float) * (size_t)n * cols, hipMemcpyHostToDevice);
        if (cols == 4) {
            // The dataset box of the score kernels' error bounds: over the rows whose four coordinates are
            // finite.  A row with a NaN or an infinite coordinate is never an inlier of the reference and
            // needs no bound (DESIGN.md "Guard band"); one infinite coordinate in the box would switch off
            // stage A and both matrix-core prefilters for the whole set.  The grid's box keeps every
            // coordinate that compares (NaN does not): an infinite one sends it to the host build.
            float mx[4] = {0, 0, 0, 0}, ga[4] = {0, 0, 0, 0};
            for (uint32_t i = 0; i < n; i++) {
                float v[4];
                bool fin = true;
                for (int k = 0; k < 4; k++) {
                    v[k] = fabsf(pts[4 * (size_t)i + k]);
                    if (v[k] > ga[k]) ga[k] = v[k];
                    fin = fin && std::isfinite(v[k]);
                }
                if (fin)
                    for (int k = 0; k < 4; k++)
                        if (v[k] > mx[k]) mx[k] = v[k];
            }
            c->ext = make_float4(mx[0], mx[1], mx[2], mx[3]);
            c->grid_ext = make_float4(ga[0], ga[1], ga[2], ga[3]);
            const char *h16env = getenv("USAC_H16");
            c->h16 = !h16env || atoi(h16env) != 0 ? 1 : 0;
            const char *e16env = getenv("USAC_E16");  // USAC_E16=0: k_score_f2 for every essential batch
            c->e16 = !e16env || atoi(e16env) != 0 ? 1 : 0;
        }
        if (e != hipSuccess) { rc = fail(c, USAC_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e)); break; }
    } while (0);
    if (rc != USAC_OK) {
        // keep the message reachable for the caller through a static copy
        static thread_local std::string last;
        last = c->err;
        usac_destroy(c);
        fprintf(stderr, "usac_create: %s\n", last.c_str());
        return rc;
    }
    *out = c;
    return USAC_OK;
}

void usac_destroy(usac_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);  // the pools are per device
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->xstream) (void)hipStreamSynchronize(c->xstream);
    if (c->lo_stream) (void)hipStreamSynchronize(c->lo_stream);
    if (c->spec_stream) (void)hipStreamSynchronize(c->spec_stream);
    if (c->comm) ncclCommDestroy(c->comm);
    for (PinBlock *b : {&c->pol_pin, &c->x_pin, &c->xring_host, &c->rec_pin, &c->grid_pin}) pin_release(*b);
    for (int k = 0; k < USAC_XRING; k++) {
        if (c->xev_batch[k]) StreamPool::get().give_back(c->xev_batch[k]);
        if (c->xev_done[k]) StreamPool::get().give_back(c->xev_done[k]);
    }
    if (c->xstream) StreamPool::get().give_back(c->xstream);
    if (c->coll_ev) StreamPool::get().give_back(c->coll_ev);
    for (auto &ev : c->lo_ev)
        if (ev) StreamPool::get().give_back(ev);
    if (c->lo_stream) StreamPool::get().give_back(c->lo_stream);
    if (c->spec_ev) StreamPool::get().give_back(c->spec_ev);
    if (c->spec_stream) StreamPool::get().give_back(c->spec_stream);
    for (DevBuf *b : {&c->pts, &c->rec, &c->perm, &c->samples, &c->models, &c->counts, &c->sums, &c->best, &c->hostmodels,
                      &c->argmax_part, &c->list, &c->list_n, &c->h4_fb, &c->h4_fb_n, &c->pool_idx, &c->pool_pts, &c->masks, &c->sprt_pts,
                      &c->sprt_tested, &c->sprt_surv, &c->sprt_surv_n, &c->sprt_starts, &c->inl_scratch, &c->e5_ws, &c->one_model,
                      &c->h16_k, &c->h16_feat, &c->h16_rows, &c->h16_fm, &c->h16_part, &c->e16_feat, &c->e16_rows, &c->e16_cm, &c->e16_part,
                      &c->inl_idx, &c->pol_lists, &c->pol_res, &c->inl_cnt, &c->inl_sum, &c->q, &c->partial, &c->ws, &c->nm_model, &c->nm_ok, &c->nm_seq, &c->nm_w, &c->nm_qw, &c->lo_io,
                      &c->rec_send, &c->rec_all, &c->tv_part, &c->hf_part, &c->prosac_tab, &c->lo_max, &c->lo_lists, &c->lo_pos,
                      &c->lo_ns, &c->lo_thrs, &c->lo_slots, &c->lo_models, &c->lo_ok, &c->lo_cnts, &c->lo_sums,
                      &c->lo_q, &c->lo_part, &c->lo_ws, &c->lo_scr, &c->knn_idx, &c->knn_d2, &c->gc_err, &c->grid_csr,
                      &c->grid_elig, &c->grid_ws, &c->x_send,
                      &c->x_recv, &c->xring})
        b->release();
    for (auto &ev : c->ev)
        if (ev) StreamPool::get().give_back(ev);
    if (c->stream) StreamPool::get().give_back(c->stream);
    delete c;
}

const char *usac_last_error(const usac_ctx *c) { return c ? c->err.c_str() : "null context"; }

int usac_set_dlt_mode(usac_ctx *c, int mode) {
    if (!c || (mode != USAC_DLT_THIN && mode != USAC_DLT_NULLSPACE)) return USAC_ERR_ARG;
    c->dlt_mode = mode;
    return USAC_OK;
}

int usac_set_score_chunks(usac_ctx *c, int chunks) {
    if (!c) return USAC_ERR_ARG;
    const bool ok = listed(c) ? (chunks >= 1 && chunks <= 128)
                              : (chunks == 1 || chunks == 2 || chunks == 4 || chunks == 8 || chunks == 16);
    if (!ok) return USAC_ERR_ARG;
    c->chunks = chunks;
    return USAC_OK;
}

int usac_set_score_variant(usac_ctx *c, int variant) {
    if (!c || variant < 0 || variant > 3) return USAC_ERR_ARG;
    c->score_variant = variant;
    return USAC_OK;
}

uint32_t usac_sample_size(const usac_ctx *c) { return c ? c->m : 0; }
uint32_t usac_num_points(const usac_ctx *c) { return c ? c->n : 0; }

int usac_estimate_models(usac_ctx *c, const int32_t *samples, uint32_t B, float *models, int32_t *n_models) {
    if (!c || !samples || !models || B == 0) return USAC_ERR_ARG;
    for (uint64_t i = 0; i < (uint64_t)B * c->m; i++)
        if (samples[i] < 0 || (uint32_t)samples[i] >= c->n) return fail(c, USAC_ERR_ARG, "sample index out of range");
    int rc = ensure_batch(c, B);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->samples.p, samples, sizeof(int32_t) * (size_t)B * c->m, hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, enqueue_solve(c, c->samples.as<int32_t>(), B, 0, 0, nullptr));
    const size_t S = (size_t)B * c->spk;
    std::vector<float> soa((size_t)ncomp(c) * S);
    std::vector<int32_t> slot_cnt(S, 0);
    HIP_TRY(c, hipMemcpyAsync(soa.data(), c->models.p, sizeof(float) * soa.size(), hipMemcpyDeviceToHost, c->stream));
    if (listed(c))
        HIP_TRY(c, hipMemcpyAsync(slot_cnt.data(), c->counts.p, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    const int nc = ncomp(c);
    for (size_t sl = 0; sl < S; sl++) {
        const bool ok = slot_cnt[sl] >= 0;
        for (int k = 0; k < 9; k++) models[9 * sl + k] = (k < nc && ok) ? soa[(size_t)k * S + sl] : 0.f;
    }
    if (n_models)
        for (uint32_t h = 0; h < B; h++) {
            int32_t k = 0;
            for (uint32_t j = 0; j < c->spk; j++) k += slot_cnt[(size_t)h * c->spk + j] >= 0;
            n_models[h] = k;
        }
    return USAC_OK;
}

int usac_score_models(usac_ctx *c, const float *models, uint32_t nm, float thr, int32_t *counts, float *sums) {
    if (!c || !models || !counts || nm == 0) return USAC_ERR_ARG;
    int rc = ensure_batch(c, nm);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // Quality::getNumberInliers never runs the SPRT (quality.hpp:60-101): the throughput SPRT of
    // usac_set_sprt applies to the hypothesize_* batches only, so it is off for this call.
    struct SprtOff {
        usac_ctx *c;
        bool saved;
        ~SprtOff() { c->sprt_on = saved; }
    } sprt_off{c, c->sprt_on};
    c->sprt_on = false;
    HIP_TRY(c, hipMemcpyAsync(c->hostmodels.p, models, sizeof(float) * 9 * (size_t)nm, hipMemcpyHostToDevice, c->stream));
    if (listed(c)) {
        HIP_TRY(c, usac::launch_prepare_f(c->stream, c->hostmodels.as<float>(), nm, c->models.as<float>()));
        if (c->score_variant == 1) {
            HIP_TRY(c, usac::launch_score_f(c->stream, c->estimator, 1, c->pts.as<float4>(), c->n,
                                            c->models.as<float>(), nm, nullptr, nullptr, nm, thr,
                                            c->counts.as<int32_t>(), c->sums.as<float>()));
        } else if (c->score_variant == 3 && is_e(c) && c->e16 == 1 && thr > 0x1p-100f && thr < 0x1p100f) {
            // variant 3 (tests): the matrix-core throughput scorer -- counts exact, Σ within its bound
            HIP_TRY(c, enqueue_score_e16(c, nm, thr, nullptr, nullptr));
        } else {  // the fast two-view kernel, one chunk: exact sequential sums
            if (c->rec_thr != thr) {
                HIP_TRY(c, c->rec.reserve(sizeof(float) * 32 * (((size_t)c->n + 3) / 4)));
                HIP_TRY(c, usac::launch_prepare_rec(c->stream, c->pts.as<float4>(), c->n, thr, c->rec.as<float4>()));
                c->rec_thr = thr;
            }
            HIP_TRY(c, c->tv_part.reserve(usac::tv_scratch_bytes(nm, 1)));
            HIP_TRY(c, usac::launch_score_f2(c->stream, c->estimator, 1, c->rec.as<float4>(), c->pts.as<float4>(),
                                             c->n, c->ext, c->models.as<float>(), nm, nullptr, nullptr, nm, thr,
                                             c->counts.as<int32_t>(), c->sums.as<float>(), c->tv_part.p));
        }
    } else {
        if (is_h(c))
            HIP_TRY(c, usac::launch_prepare_h(c->stream, c->hostmodels.as<float>(), nm, c->models.as<float>()));
        else
            HIP_TRY(c, usac::launch_prepare_line(c->stream, c->hostmodels.as<float>(), nm, c->models.as<float>()));
        // variant 3 (tests): the throughput scorer on the given models -- counts exact, Σ within its bound
        HIP_TRY(c, enqueue_score(c, nm, thr, c->score_variant == 3 ? std::max(c->chunks, 2) : 1));
    }
    HIP_TRY(c, hipMemcpyAsync(counts, c->counts.p, sizeof(int32_t) * nm, hipMemcpyDeviceToHost, c->stream));
    if (sums) HIP_TRY(c, hipMemcpyAsync(sums, c->sums.p, sizeof(float) * nm, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_get_inliers(usac_ctx *c, const float *model, float thr, int32_t *idx, uint32_t *n, float *sum) {
    if (!c || !model) return USAC_ERR_ARG;
    int rc = ensure_single(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->one_model.p, model, sizeof(float) * 9, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, enqueue_inliers(c, c->one_model.as<float>(), thr));
    int32_t cnt = 0;
    float s = 0.f;
    HIP_TRY(c, hipMemcpyAsync(&cnt, c->inl_cnt.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&s, c->inl_sum.p, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    if (idx && cnt > 0)
        HIP_TRY(c, hipMemcpy(idx, c->inl_idx.p, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost));
    if (n) *n = (uint32_t)cnt;
    if (sum) *sum = s;
    return USAC_OK;
}

float usac_bk_label(int n, const float *unary, int m, const int32_t *ei, const int32_t *ej, const float *e00,
                    const float *e01, const float *e10, const float *e11, int32_t *sink_out) {
    usac::BkGraph G(n, (size_t)m);
    for (int i = 0; i < n; i++) G.add_node();
    for (int i = 0; i < n; i++) G.add_term1(i, unary[i], 0.f);
    for (int k = 0; k < m; k++) G.add_term2(ei[k], ej[k], e00[k], e01[k], e10[k], e11[k]);
    const float f = G.maxflow();
    for (int i = 0; i < n; i++) sink_out[i] = G.is_sink(i) ? 1 : 0;
    return f;
}

int usac_knn(usac_ctx *c, uint32_t k, int32_t *idx, float *d2) {
    if (!c || !idx || k == 0 || k > usac::kKnnMax) return USAC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nk = (size_t)c->n * k;
    HIP_TRY(c, c->knn_idx.reserve(sizeof(int32_t) * nk));
    if (d2) HIP_TRY(c, c->knn_d2.reserve(sizeof(float) * nk));
    HIP_TRY(c, usac::launch_knn(c->stream, c->pts.as<float>(), c->n, c->cols, k, c->knn_idx.as<int32_t>(),
                                d2 ? c->knn_d2.as<float>() : nullptr));
    HIP_TRY(c, hipMemcpyAsync(idx, c->knn_idx.p, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, c->stream));
    if (d2) HIP_TRY(c, hipMemcpyAsync(d2, c->knn_d2.p, sizeof(float) * nk, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_nonminimal(usac_ctx *c, const int32_t *idx, uint32_t n, float *model) {
    return usac_lsq_fit(c, idx, n, nullptr, model);
}

int usac_lsq_fit(usac_ctx *c, const int32_t *idx, uint32_t n, const float *weights, float *model) {
    if (!c || !idx || !model) return USAC_ERR_ARG;
    if (n == 0) return fail(c, USAC_ERR_ARG, "empty sample");
    if (weights && c->estimator != USAC_HOMOGRAPHY && c->estimator != USAC_FUNDAMENTAL)
        return fail(c, USAC_ERR_UNSUPPORTED, "weighted non-minimal fit: homography / fundamental only "
                                             "(the other estimators inherit estimator.hpp:26's NOT IMPLEMENTED)");
    for (uint32_t i = 0; i < n; i++)
        if (idx[i] < 0 || (uint32_t)idx[i] >= c->n) return fail(c, USAC_ERR_ARG, "index out of range");
    int rc = ensure_single(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->inl_idx.reserve(sizeof(int32_t) * std::max<size_t>(n, c->n)));
    HIP_TRY(c, c->q.reserve(sizeof(float) * 4 * (size_t)n));
    HIP_TRY(c, c->partial.reserve(sizeof(double) * 45 * ((size_t)n / 64 + 2)));
    HIP_TRY(c, hipMemcpyAsync(c->inl_idx.p, idx, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    if (weights) {
        HIP_TRY(c, c->nm_w.reserve(sizeof(float) * (size_t)c->n));
        HIP_TRY(c, hipMemcpyAsync(c->nm_w.p, weights, sizeof(float) * c->n, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, enqueue_nonminimal(c, c->inl_idx.as<int32_t>(), n, nullptr, nullptr,
                                  weights ? c->nm_w.as<float>() : nullptr));
    int32_t ok = 0;
    HIP_TRY(c, hipMemcpyAsync(model, c->nm_model.p, sizeof(float) * 9, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&ok, c->nm_ok.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return ok ? USAC_OK : fail(c, USAC_ERR_NO_MODEL, "non-minimal estimation failed");
}

// USAC_H16_DEFER=0: the h16 scorer's own finish kernel, then the plain argmax (A/B)
bool h16_defer() {
    static const bool on = !getenv("USAC_H16_DEFER") || atoi(getenv("USAC_H16_DEFER")) != 0;
    return on;
}

// the batch argmax (record of the batch) -- over the h16 scorer's chunk partials when it deferred
// its finish (one launch fewer), else over counts / sums
hipError_t batch_argmax(usac_ctx *c, uint32_t S, uint64_t first_hyp) {
    if (c->h16_deferred_ch) {
        const uint32_t ch = c->h16_deferred_ch;
        c->h16_deferred_ch = 0;
        return usac::launch_argmax_h16(c->stream, c->h16_part.p, S, (int)ch, c->h16_deferred_thr,
                                       c->counts.as<int32_t>(), c->sums.as<float>(), c->models.as<float>(), ncomp(c),
                                       first_hyp, c->spk, c->argmax_part.p, c->best.as<usac_record>());
    }
    return usac::launch_argmax(c->stream, c->counts.as<int32_t>(), c->sums.as<float>(), S, c->models.as<float>(),
                               ncomp(c), first_hyp, c->spk, c->argmax_part.p, c->best.as<usac_record>());
}

int usac_hypothesize_score(usac_ctx *c, const int32_t *samples, uint32_t B, uint64_t seed, uint64_t first_hyp,
                           float thr, int32_t *counts, float *sums, usac_record *best) {
    if (!c || B == 0) return USAC_ERR_ARG;
    if (samples)
        for (uint64_t i = 0; i < (uint64_t)B * c->m; i++)
            if (samples[i] < 0 || (uint32_t)samples[i] >= c->n) return fail(c, USAC_ERR_ARG, "sample index out of range");
    int rc = ensure_batch(c, B);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (samples)
        HIP_TRY(c, hipMemcpyAsync(c->samples.p, samples, sizeof(int32_t) * (size_t)B * c->m, hipMemcpyHostToDevice,
                                  c->stream));
    // per-hypothesis outputs requested -> exact sequential sums (one chunk)
    const int chunks = (counts || sums) ? 1 : c->chunks;
    HIP_TRY(c, enqueue_solve(c, samples ? c->samples.as<int32_t>() : nullptr, B, seed, first_hyp,
                             samples ? nullptr : c->samples.as<int32_t>(), h16_solver_thr(c, chunks, thr)));
    HIP_TRY(c, enqueue_score(c, B, thr, chunks, h16_defer()));
    c->batch_valid = true;
    const uint32_t S = B * c->spk;
    HIP_TRY(c, batch_argmax(c, S, first_hyp));
    if (counts) HIP_TRY(c, hipMemcpyAsync(counts, c->counts.p, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
    if (sums) HIP_TRY(c, hipMemcpyAsync(sums, c->sums.p, sizeof(float) * S, hipMemcpyDeviceToHost, c->stream));
    if (best) HIP_TRY(c, hipMemcpyAsync(best, c->best.p, sizeof(usac_record), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_hypothesize_async(usac_ctx *c, uint32_t B, uint64_t seed, uint64_t first_hyp, float thr) {
    if (!c || B == 0) return USAC_ERR_ARG;
    int rc = ensure_batch(c, B);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const bool tm = c->timing_on;
    if (tm) HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(c, enqueue_solve(c, nullptr, B, seed, first_hyp, nullptr, h16_solver_thr(c, c->chunks, thr)));
    if (tm) HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(c, enqueue_score(c, B, thr, c->chunks, h16_defer()));
    c->batch_valid = true;
    if (tm) HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
    HIP_TRY(c, batch_argmax(c, B * c->spk, first_hyp));
    if (tm) HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
    c->timed_pending = tm;
    return USAC_OK;
}

int usac_selftest_rpoly(usac_ctx *c, const double *coeffs, uint32_t B, double *roots, int32_t *nroots) {
    if (!c || !coeffs || !roots || !nroots || B == 0) return USAC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf dc, dr, dn, ws;
    struct Rel {
        DevBuf *b[4];
        ~Rel() {
            (void)hipDeviceSynchronize();
            for (DevBuf *x : b) x->release();
        }
    } rel{{&dc, &dr, &dn, &ws}};
    HIP_TRY(c, dc.reserve(sizeof(double) * 11 * (size_t)B));
    HIP_TRY(c, dr.reserve(sizeof(double) * 10 * (size_t)B));
    HIP_TRY(c, dn.reserve(sizeof(int32_t) * (size_t)B));
    HIP_TRY(c, ws.reserve(usac::e5_workspace_bytes(B)));
    HIP_TRY(c, hipMemcpyAsync(dc.p, coeffs, sizeof(double) * 11 * (size_t)B, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, usac::launch_e5_roots_selftest(c->stream, dc.as<double>(), B, dr.as<double>(), dn.as<int32_t>(), ws.p));
    std::vector<double> r(10 * (size_t)B);
    HIP_TRY(c, hipMemcpyAsync(r.data(), dr.p, sizeof(double) * 10 * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(nroots, dn.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    for (uint32_t h = 0; h < B; h++)  // device layout [r B + h] -> row h
        for (int k = 0; k < 10; k++) roots[10 * (size_t)h + k] = k < nroots[h] ? r[(size_t)k * B + h] : 0.0;
    return USAC_OK;
}

int usac_selftest_logexp(usac_ctx *c, const double *x, uint32_t n, double *log_out, double *exp_out) {
    if (!c || !x || !log_out || !exp_out || n == 0) return USAC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf dx, dl, de;
    struct Rel {
        DevBuf *b[3];
        ~Rel() {
            (void)hipDeviceSynchronize();
            for (DevBuf *y : b) y->release();
        }
    } rel{{&dx, &dl, &de}};
    HIP_TRY(c, dx.reserve(sizeof(double) * n));
    HIP_TRY(c, dl.reserve(sizeof(double) * n));
    HIP_TRY(c, de.reserve(sizeof(double) * n));
    HIP_TRY(c, hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, usac::launch_jt_logexp_selftest(c->stream, dx.as<double>(), n, dl.as<double>(), de.as<double>()));
    HIP_TRY(c, hipMemcpyAsync(log_out, dl.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(exp_out, de.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_last_counts(usac_ctx *c, int32_t *counts, float *sums, uint32_t n) {
    if (!c || !counts || n == 0) return USAC_ERR_ARG;
    if (!c->batch_valid) return fail(c, USAC_ERR_ARG, "no batch since the last usac_ransac_run");
    if ((size_t)n * sizeof(int32_t) > c->counts.bytes) return fail(c, USAC_ERR_ARG, "more slots than the last batch");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(counts, c->counts.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    if (sums) HIP_TRY(c, hipMemcpyAsync(sums, c->sums.p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_fetch_best(usac_ctx *c, usac_record *best) {
    if (!c || !best) return USAC_ERR_ARG;
    if (!pin_grow(c->rec_pin, sizeof(usac_record)))
        return fail(c, USAC_ERR_HIP, "pinned host allocation failed");
    HIP_TRY(c, hipMemcpyAsync(c->rec_pin.p, c->best.p, sizeof(usac_record), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    memcpy(best, c->rec_pin.p, sizeof(usac_record));
    return USAC_OK;
}

int usac_sync(usac_ctx *c) {
    if (!c) return USAC_ERR_ARG;
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_set_timing(usac_ctx *c, int on) {
    if (!c) return USAC_ERR_ARG;
    c->timing_on = on != 0;
    return USAC_OK;
}

int usac_last_timings(usac_ctx *c, float *ms3) {
    if (!c || !ms3) return USAC_ERR_ARG;
    if (c->timed_pending) {
        HIP_TRY(c, hipEventSynchronize(c->ev[3]));
        HIP_TRY(c, hipEventElapsedTime(&c->last_ms[0], c->ev[0], c->ev[3]));
        HIP_TRY(c, hipEventElapsedTime(&c->last_ms[1], c->ev[1], c->ev[2]));
        HIP_TRY(c, hipEventElapsedTime(&c->last_ms[2], c->ev[0], c->ev[1]));
        c->timed_pending = false;
    }
    memcpy(ms3, c->last_ms, sizeof(c->last_ms));
    return USAC_OK;
}

uint32_t usac_std_termination(uint32_t inliers, uint32_t points_size, uint32_t sample_size, float desired_prob,
                              uint32_t max_iterations) {
    usac::StandardTerminationCriteria t(desired_prob, sample_size, points_size, max_iterations);
    return t.getUpBoundIterations(inliers);
}

int usac_uniform_samples(uint32_t seed, uint32_t n_points, uint32_t m, uint32_t count, int32_t *out) {
    if (!out || n_points == 0 || m == 0) return USAC_ERR_ARG;
    usac::UniformSampler s(seed, n_points, m);
    for (uint32_t i = 0; i < count; i++) s.generateSample(out + (size_t)i * m);
    return USAC_OK;
}

int usac_set_device_sampler(usac_ctx *c, int sampler) {
    if (!c || (sampler != USAC_SAMPLER_UNIFORM && sampler != USAC_SAMPLER_PROSAC && sampler != USAC_SAMPLER_NAPSAC))
        return USAC_ERR_ARG;
    if (sampler == USAC_SAMPLER_NAPSAC) {
        const int rc = ensure_grid(c, c->cell_size);
        if (rc) return rc;
    }
    if (sampler == USAC_SAMPLER_PROSAC) {
        if (c->n < c->m) return fail(c, USAC_ERR_ARG, "PROSAC needs n >= sample size");
        // the subset sequence of ProsacSampler::generateSample with termination_length = n
        usac::ProsacSampler ps(1, c->n, c->m);
        const uint32_t T = usac::ProsacSampler::kGrowthMax;
        std::vector<int32_t> smp(c->m);
        std::vector<uint32_t> tab(T);
        for (uint32_t h = 0; h < T; h++) {
            ps.generateSample(smp.data(), c->n);
            tab[h] = ps.subset();
        }
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->prosac_tab.reserve(sizeof(uint32_t) * T));
        HIP_TRY(c, hipMemcpy(c->prosac_tab.p, tab.data(), sizeof(uint32_t) * T, hipMemcpyHostToDevice));
        c->prosac_len = T;
    }
    c->dev_sampler = sampler;
    return USAC_OK;
}

int usac_set_cell_size(usac_ctx *c, int cell_size) {
    if (!c || cell_size <= 0) return USAC_ERR_ARG;
    c->cell_size = cell_size;
    return c->dev_sampler == USAC_SAMPLER_NAPSAC ? ensure_grid(c, cell_size) : USAC_OK;
}

int usac_grid_neighbors(usac_ctx *c, int cell_size, uint32_t *n_cells, uint32_t *cell, uint32_t *rank, uint32_t *start,
                        int32_t *members, int32_t *eligible, uint32_t *n_eligible) {
    if (!c) return USAC_ERR_ARG;
    int rc = ensure_grid(c, cell_size);
    if (rc) return rc;
    const size_t n = c->n;
    if (n_cells) *n_cells = c->grid_n_cells;
    if (n_eligible) *n_eligible = c->grid_n_elig;
    if (cell) HIP_TRY(c, hipMemcpyAsync(cell, c->grid_cell(), 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (rank) HIP_TRY(c, hipMemcpyAsync(rank, c->grid_rank(), 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (start)
        HIP_TRY(c, hipMemcpyAsync(start, c->grid_start(), 4 * ((size_t)c->grid_n_cells + 1), hipMemcpyDeviceToHost,
                                  c->stream));
    if (members) HIP_TRY(c, hipMemcpyAsync(members, c->grid_members(), 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (eligible && c->grid_n_elig)
        HIP_TRY(c, hipMemcpyAsync(eligible, c->grid_elig.p, 4 * (size_t)c->grid_n_elig, hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_draw_samples(usac_ctx *c, uint32_t B, uint64_t seed, uint64_t first_hyp, int32_t *out) {
    if (!c || !out || B == 0) return USAC_ERR_ARG;
    int rc = ensure_batch(c, B);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, usac::launch_draw_samples(c->stream, (int)c->m, c->n, B, dev_sampler(c, seed), first_hyp,
                                         c->samples.as<int32_t>()));
    HIP_TRY(c, hipMemcpyAsync(out, c->samples.p, sizeof(int32_t) * (size_t)B * c->m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_set_sprt(usac_ctx *c, int enable, uint32_t seed, double epsilon, double delta) {
    if (!c) return USAC_ERR_ARG;
    if (!enable) {
        c->sprt_on = false;
        return USAC_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    usac::GlibcRandom g(seed);
    usac::Sprt sp(g, c->estimator, c->n, c->m, 10000);
    const double eps = epsilon > 0 ? epsilon : sp.epsilon0(), del = delta > 0 ? delta : sp.delta0();
    if (!(eps < 1.0) || !(del < 1.0)) return fail(c, USAC_ERR_ARG, "SPRT: epsilon and delta must be in (0, 1)");
    // the reference's constants (sprt.hpp:219-224: lambda * (delta / epsilon), lambda * ((1 - delta) /
    // (1 - epsilon)), compared with A), and their logs for the certified decisions (kernels_sprt.hip)
    c->sprt_eps = eps;
    c->sprt_delta = del;
    c->sprt_k.up = del / eps;
    c->sprt_k.down = (1 - del) / (1 - eps);
    c->sprt_k.A = sp.thresholdA(eps, del);
    c->sprt_k.lu = log(c->sprt_k.up);
    c->sprt_k.ld = log(c->sprt_k.down);
    c->sprt_k.lA = log(c->sprt_k.A);
    // test hooks: a wider margin / a lower climb limit sends more walks down the sequential path
    const char *em = getenv("USAC_SPRT_CERT_MARGIN"), *ec = getenv("USAC_SPRT_CERT_CLIMB");
    c->sprt_k.margin = em ? atof(em) : 1e-7;
    c->sprt_k.climb = ec ? atof(ec) : 700.0;
    if (!(c->sprt_k.margin >= 1e-7) || !(c->sprt_k.climb > 0) || c->sprt_k.climb > 700.0)
        return fail(c, USAC_ERR_ARG, "SPRT certificate: margin >= 1e-7 and 0 < climb <= 700");
    {  // the certificate's error budget at this n (kernels_sprt.hip): never a margin below it
        const double L = std::max(std::max(fabs(c->sprt_k.lu), fabs(c->sprt_k.ld)), 1.0);
        const double nn = (double)c->n, per = std::ceil(std::max(nn - 64.0, 0.0) / 256.0) + 64.0;
        const double budget = 2.0 * nn * L * 0x1p-51 + per * per * L * 0x1p-53 + fabs(c->sprt_k.lA) * 0x1p-53;
        c->sprt_k.margin = std::max(c->sprt_k.margin, 8.0 * budget);
    }
    HIP_TRY(c, c->pool_idx.reserve(sizeof(uint32_t) * c->n));
    HIP_TRY(c, c->sprt_pts.reserve(sizeof(float) * c->cols * (size_t)c->n));
    HIP_TRY(c, c->sprt_tested.reserve(sizeof(uint32_t)));
    HIP_TRY(c, c->sprt_surv_n.reserve(sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpyAsync(c->pool_idx.p, sp.pool().data(), sizeof(uint32_t) * c->n, hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, usac::launch_gather_points(c->stream, c->pts.p, c->cols, c->pool_idx.as<uint32_t>(), c->n,
                                          c->sprt_pts.p));
    HIP_TRY(c, hipMemsetAsync(c->sprt_tested.p, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    c->sprt_on = true;
    return USAC_OK;
}

int usac_batch_sprt_info(usac_ctx *c, double *eps_delta_A, uint32_t *starts, uint32_t n) {
    if (!c) return USAC_ERR_ARG;
    if (!c->sprt_on) return fail(c, USAC_ERR_ARG, "SPRT not enabled");
    if (eps_delta_A) {
        eps_delta_A[0] = c->sprt_eps;
        eps_delta_A[1] = c->sprt_delta;
        eps_delta_A[2] = c->sprt_k.A;
    }
    if (starts && n) {
        if (!c->batch_valid || n > c->sprt_S) return fail(c, USAC_ERR_ARG, "no SPRT batch of that many slots");
        HIP_TRY(c, hipMemcpyAsync(starts, c->sprt_starts.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
        uint32_t ln = 0;
        if (listed(c)) HIP_TRY(c, hipMemcpyAsync(&ln, c->list_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, stream_wait(c->stream));
        if (listed(c)) {  // k_sprt_head writes the listed (occupied) slots only: the others get UINT32_MAX
            std::vector<uint32_t> lst(ln);
            if (ln) {
                HIP_TRY(c, hipMemcpyAsync(lst.data(), c->list.p, sizeof(uint32_t) * ln, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, stream_wait(c->stream));
            }
            std::vector<char> occ(n, 0);
            for (uint32_t k = 0; k < ln; k++)
                if (lst[k] < n) occ[lst[k]] = 1;
            for (uint32_t i = 0; i < n; i++)
                if (!occ[i]) starts[i] = UINT32_MAX;
        }
    }
    return USAC_OK;
}

int usac_sprt_tested(usac_ctx *c, uint64_t *points_tested) {
    if (!c || !points_tested) return USAC_ERR_ARG;
    if (!c->sprt_on) return fail(c, USAC_ERR_ARG, "SPRT not enabled");
    uint32_t t = 0;
    HIP_TRY(c, hipMemcpyAsync(&t, c->sprt_tested.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    *points_tested = t;
    return USAC_OK;
}

int usac_prosac_samples(uint32_t seed, uint32_t n_points, uint32_t m, uint32_t count, uint32_t termination_length,
                        int32_t *out) {
    if (!out || m < 2 || n_points < m || termination_length == 0 || count > usac::ProsacSampler::kGrowthMax)
        return USAC_ERR_ARG;
    usac::ProsacSampler s(seed, n_points, m);
    for (uint32_t i = 0; i < count; i++) s.generateSample(out + (size_t)i * m, termination_length);
    return USAC_OK;
}

int usac_sprt_pool(uint32_t seed, int estimator, uint32_t n_points, uint32_t m, uint32_t *pool, double *A0) {
    if (!pool || n_points == 0) return USAC_ERR_ARG;
    usac::GlibcRandom g(seed);
    usac::Sprt s(g, estimator, n_points, m, 10000);
    memcpy(pool, s.pool().data(), sizeof(uint32_t) * n_points);
    if (A0) *A0 = s.thresholdA0();
    return USAC_OK;
}

// Ransac::run (ransac.cpp:14-238): Uniform (glibc stream) or PROSAC sampler, optional SPRT,
// no LO.  Samples are drawn on the host in loop order and shipped in batches; the device
// solves every sample of a batch and either scores every model exactly (count, sequential
// Σerr) or, with SPRT, produces every model's inlier flags in SPRT-pool order; the host
// then replays the sequential loop over the batch -- SPRT walk, Score::bigger, termination
// update at each new best (standard, or PROSAC's scan of the best model's device inlier
// list), `while (iters < max_iters)` with the reference's SPRT double counting.
// This reproduces the reference's iteration sequence exactly because the loop state
// changes only at those points.  PROSAC samples depend on
// termination_length, which a best update can change: a batch is speculative, and when a
// change would alter a later sample of the batch the rest of the batch is dropped and the
// sampler is rewound to just after the current sample.  Then the <= 4-pass non-minimal
// polish on the device.
// One batch of a sharded run: rank r solves and scores slots of samples [r P, r P + P) (P =
// ceil(B / nranks); the last slices may be short or empty), packs its status word, counts and
// model words (int32 / fp32, padded to P x spk slots, counts -1 on padding) and all-gathers
// them; every rank unpacks all slices into hc / hmod exactly as the unsharded batch leaves
// them.  A rank whose local part failed still joins the all-gather with its error as status,
// and every rank then fails with the first failing rank's status: no rank is left blocked in
// a collective its peers never enter.  The RCCL path packs on the device (no host staging on
// the way out) and brings the gathered words back with one copy into pinned memory; a gather
// callback (e.g. gloo) receives host buffers.
static int sharded_batch(usac_ctx *c, const int32_t *hs, uint32_t B, uint32_t iters, float thr, int nranks, int rank,
                         usac_allgather_fn gather, void *user, std::vector<uint8_t> &xbuf, int32_t *hc, float *hmod,
                         size_t SB, bool sprt, uint32_t *hmask) {
    const uint32_t m = c->m, spk = c->spk;
    const int nc = ncomp(c);
    const uint32_t P = (B + (uint32_t)nranks - 1) / (uint32_t)nranks;
    const uint32_t lo = std::min<uint32_t>(B, (uint32_t)rank * P);
    const uint32_t Bs = std::min<uint32_t>(B, lo + P) - lo;
    const size_t Ps = (size_t)P * spk, Ss = (size_t)Bs * spk;
    // SPRT: every slot's pool-order inlier words follow the models ([nw][Ps], row = slot)
    const size_t nw = sprt ? (c->n + 31) / 32 : 0, moff = 1 + (1 + (size_t)nc) * Ps;
    const size_t words = moff + nw * Ps, bytes = 4 * words;
    auto pool_mask = [&](uint32_t *out) -> hipError_t {
        return usac::launch_pool_mask(c->stream, c->estimator, c->pool_pts.p, c->n, c->models.as<float>(), Ss, nullptr,
                                      nullptr, (uint32_t)Ss, thr, out, (uint32_t)Ps);
    };
    // the local part: its first error becomes this rank's status (the message stays in c->err)
    auto local = [&]() -> int {
        if (!Bs) return USAC_OK;
        HIP_TRY(c, hipMemcpyAsync(c->samples.p, hs + (size_t)lo * m, sizeof(int32_t) * (size_t)Bs * m,
                                  hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, enqueue_solve(c, c->samples.as<int32_t>(), Bs, 0, (uint64_t)iters + lo, nullptr));
        if (!sprt) HIP_TRY(c, enqueue_score(c, Bs, thr, loop_chunks(c, Bs)));
        return USAC_OK;
    };
    const int status = local();
    const std::string local_err = c->err;
    const uint8_t *recv = nullptr;
    if (gather) {
        xbuf.resize(bytes * (1 + (size_t)nranks));
        int32_t *send = reinterpret_cast<int32_t *>(xbuf.data());
        std::fill(send + 1, send + 1 + Ps, -1);
        std::fill(send + 1 + Ps, send + words, 0);
        send[0] = status;
        if (status == USAC_OK && Bs) {
            HIP_TRY(c, hipMemcpyAsync(send + 1, c->counts.p, sizeof(int32_t) * Ss, hipMemcpyDeviceToHost, c->stream));
            for (int k = 0; k < nc; k++)
                HIP_TRY(c, hipMemcpyAsync(send + 1 + (1 + (size_t)k) * Ps, c->models.as<float>() + (size_t)k * Ss,
                                          sizeof(float) * Ss, hipMemcpyDeviceToHost, c->stream));
            if (sprt) {
                HIP_TRY(c, pool_mask(c->masks.as<uint32_t>()));
                HIP_TRY(c, hipMemcpyAsync(send + moff, c->masks.p, sizeof(uint32_t) * nw * Ps, hipMemcpyDeviceToHost,
                                          c->stream));
            }
            HIP_TRY(c, stream_wait(c->stream));
        }
        if (gather(user, send, bytes, xbuf.data() + bytes) != 0)
            return fail(c, USAC_ERR_ARG, "all-gather callback failed (gather callbacks must fail on every rank)");
        recv = xbuf.data() + bytes;
    } else {
        HIP_TRY(c, c->x_send.reserve(bytes));
        HIP_TRY(c, c->x_recv.reserve(bytes * (size_t)nranks));
        if (!pin_grow(c->x_pin, bytes * (size_t)nranks)) return fail(c, USAC_ERR_HIP, "pinned host allocation failed");
        HIP_TRY(c, usac::launch_pack_slice(c->stream, c->counts.as<int32_t>(), c->models.as<float>(),
                                           status == USAC_OK ? (uint32_t)Ss : 0u, (uint32_t)Ps, nc, status,
                                           c->x_send.as<int32_t>()));
        if (sprt && status == USAC_OK && Bs) HIP_TRY(c, pool_mask(c->x_send.as<uint32_t>() + moff));
        HIP_TRY(c, order_after_exchanges(c));
        NCCL_TRY(c, ncclAllGather(c->x_send.p, c->x_recv.p, bytes, ncclUint8, c->comm, c->stream));
        HIP_TRY(c, mark_collective(c));
        HIP_TRY(c, hipMemcpyAsync(c->x_pin.p, c->x_recv.p, bytes * (size_t)nranks, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, stream_wait(c->stream));
        recv = static_cast<const uint8_t *>(c->x_pin.p);
    }
    for (int r = 0; r < nranks; r++) {
        const int32_t st = *reinterpret_cast<const int32_t *>(recv + (size_t)r * bytes);
        if (st != USAC_OK)
            return fail(c, st, r == rank ? local_err : "sharded run: rank " + std::to_string(r) + " failed (status " +
                                                           std::to_string(st) + ")");
    }
    for (int r = 0; r < nranks; r++) {
        const uint32_t lr = std::min<uint32_t>(B, (uint32_t)r * P);
        const size_t Sr = (size_t)(std::min<uint32_t>(B, lr + P) - lr) * spk;
        const int32_t *rc_ = reinterpret_cast<const int32_t *>(recv + (size_t)r * bytes) + 1;
        memcpy(hc + (size_t)lr * spk, rc_, sizeof(int32_t) * Sr);
        for (int k = 0; k < nc; k++)
            memcpy(hmod + (size_t)k * SB + (size_t)lr * spk, rc_ + (1 + (size_t)k) * Ps, sizeof(float) * Sr);
        // mask rows = slots of the whole batch: hmask[w * S + slot]
        for (size_t w = 0; w < nw; w++)
            memcpy(hmask + w * (size_t)B * spk + (size_t)lr * spk, rc_ + (moff - 1) + w * Ps, sizeof(uint32_t) * Sr);
    }
    // without a slot list a model's count is never -1 (ransac_run_impl's unsharded SPRT path)
    if (sprt && !listed(c)) std::fill(hc, hc + (size_t)B * spk, 0);
    return USAC_OK;
}

namespace {

// The state of one Ransac::run and its stages, in the order ransac_run_impl calls them.  The members are
// declared in the order the run builds them, so they are destroyed in the reverse of it: the pinned
// staging vectors before lo (whose destructor drains the LO streams), lo before the samplers' generator.
// Guards: the destructor body -- which runs before any member goes -- waits for a speculative batch
// still copying into hs2 / hc2 / hmod2; the two guards that put c->h16_off, c->dlt_mode and c->sprt_on
// back are locals of ransac_run_impl, declared before the RansacRun, so they act after it on every exit.
struct RansacRun {
    usac_ctx *const c;
    const usac_params *const prm;
    const int nranks, rank;
    const usac_allgather_fn gather;
    void *const gather_user;
    usac_run_output *const out;
    int32_t *const inliers_out;
    usac_record *const records;
    const uint32_t rec_cap;

    // the parameter checks' flags
    bool prosac = false, napsac = false, knn_mode = false, use_lo = false, use_gc = false, gc_knn = false;

    std::chrono::steady_clock::time_point t0;
    // wall-time split of the run, printed to stderr when USAC_PROFILE is set
    enum { T_SETUP, T_DRAW, T_DEVICE, T_SUMS, T_REPLAY, T_LO, T_POLISH, T_N };
    double tsplit[T_N] = {0, 0, 0, 0, 0, 0, 0};
    double t_verify = 0.0, t_drawonly = 0.0;  // USAC_PROFILE detail: host SPRT walks, sample draws
    std::chrono::steady_clock::time_point tmark;
    // sub-split of the setup (USAC_PROFILE): buffers, neighbours, LO / GC reservations
    double tsub[3] = {0, 0, 0};

    const uint32_t batch;
    const uint32_t n, m, spk;
    const float thr;

    usac::GlibcRandom grng;
    std::unique_ptr<usac::UniformSampler> uni;
    std::unique_ptr<usac::ProsacSampler> pro;
    std::unique_ptr<usac::ProsacTerminationCriteria> pterm;
    std::shared_ptr<const usac::GridNeighbors> grid;
    std::unique_ptr<usac::NapsacSampler> nap;
    std::unique_ptr<usac::NapsacKnnSampler> napk;
    std::vector<int32_t> knn_tab;
    std::unique_ptr<LoRansac> lo;
    std::unique_ptr<GcLo> gc;
    usac::StandardTerminationCriteria term;
    std::unique_ptr<usac::Sprt> sprt;
    const int max_before;
    const uint32_t nw;
    bool defer_pool = false;

    const size_t SB;            // slot stride of the host copies
    std::vector<uint8_t> xbuf;  // sharded runs: all-gather send + receive buffers
    pinned_vector<int32_t> hs, hc;
    std::vector<int32_t> slot_row;
    std::vector<float> hsum;
    pinned_vector<float> hmod;
    pinned_vector<uint32_t> hlist;  // the SPRT batch's occupied-slot list, its count at [SB]
    pinned_vector<uint32_t> hmask;  // words, PoolTail
    std::vector<uint32_t> subset_at, largest_at;
    std::vector<int32_t> last_sample;
    bool spec_ok = false;
    pinned_vector<int32_t> hs2, hc2;
    pinned_vector<float> hmod2;
    std::vector<int32_t> spec_last;
    bool spec = false;          // a speculative batch is on the spec stream
    uint32_t spec_B = 0;        // its size
    uint32_t sampler_keep = 0;  // > 0: roll the sampler back and redraw this many samples
    pinned_vector<int32_t> inl_list;
    usac::Score best;
    float best_model[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t iters = 0, max_iters;
    int32_t nrec = 0;
    // exact inliers of a model on the device -> (cnt, s) and c->inl_idx
    int32_t cnt = 0;
    float s = 0.f;
    bool mask_list = false, mask_check = false;
    std::vector<uint64_t> pt_bits;
    uint32_t cap = 0;

    // this batch
    uint32_t B = 0;
    bool have = false;  // this batch's device results are already on the host (speculation)
    size_t spec_hst = 0;
    std::unique_ptr<usac::ProsacSampler> snapshot;
    uint32_t gen_term = 0;
    size_t S = 0;
    size_t hst = 0;            // host stride of hmod's components this batch
    uint32_t rows = 0;
    uint32_t mask_stride = 0;  // host row stride of hmask (SPRT)

    // the polish: its passes, and what it leaves for emit() -- best_model's own inlier list on the device
    static constexpr int kPasses = 4;
    int32_t *cur = nullptr;
    int32_t cur_cnt = 0;

    RansacRun(usac_ctx *c_, const usac_params *prm_, int nranks_, int rank_, usac_allgather_fn gather_, void *gather_user_,
              usac_run_output *out_, int32_t *inliers_out_, usac_record *records_, uint32_t rec_cap_)
        : c(c_),
          prm(prm_),
          nranks(nranks_),
          rank(rank_),
          gather(gather_),
          gather_user(gather_user_),
          out(out_),
          inliers_out(inliers_out_),
          records(records_),
          rec_cap(rec_cap_),
          batch(prm->batch ? prm->batch : (prm->sprt ? 1024u : kDefaultBatch)),
          n(c->n),
          m(c->m),
          spk(c->spk),
          thr(prm->threshold),
          grng(prm->seed),
          term(prm->desired_prob, m, n, prm->max_iterations),
          max_before(max_before_sprt(prm)),
          nw((n + 31) / 32),
          SB((size_t)batch * spk),
          max_iters(prm->max_iterations) {}
    // every exit waits for a speculative batch still copying into hs2 / hc2 / hmod2
    ~RansacRun() {
        if (spec) (void)hipStreamSynchronize(c->spec_stream);
    }

    void lap(int k) {
        const auto t = std::chrono::steady_clock::now();
        tsplit[k] += std::chrono::duration<double, std::milli>(t - tmark).count();
        tmark = t;
    }
    void sub(int k) {
        const auto t = std::chrono::steady_clock::now();
        tsub[k] = std::chrono::duration<double, std::milli>(t - tmark).count();
    }
    void sampler_mark() {
        if (nap) nap->mark();
        else uni->mark();
    }
    void sampler_commit() {
        if (nap) nap->commit();
        else uni->commit();
    }
    void sampler_rollback() {
        if (nap) nap->rollback();
        else uni->rollback();
    }

    int check_params();
    int begin();
    int pool_upload();
    int construct();
    int host_buffers();
    int score_inliers(const float *model_host, int32_t *list_pin = nullptr);
    int32_t mask_inliers(const uint32_t *row, size_t stride, int32_t *list);
    void draw_into(int32_t *buf, uint32_t count, usac::ProsacSampler *pro_, uint32_t term_len);
    void settle_sampler();
    hipError_t spec_wait();
    int take_speculation();
    void draw();
    int one_rank_batch();
    int device_batch();
    int speculate_next();
    int sums();
    int replay();
    void lo_counters();
    int finish();
    void polish_replay(int k0, int k1, const float *hres, int32_t *const *lists, int &prev, bool &stop);
    int polish_fused_profile(int k_first);
    int polish_pass(int k, float *dres, int32_t *dres_i, int32_t *const *lists, bool finish_score);
    int polish();
    int emit();
};

// 1. Parameter checks.  Reads prm and the context's shape; leaves the sampler / LO flags, and c->h16_off
// set for the loop.
int RansacRun::check_params() {
    // The loop scores homographies with k_score_hf, not the matrix-core scorer: its batches are
    // small (the ramp; h16's per-batch rows + finish launches cost more than they save: cfg5 3.30 ms
    // per run with k_score_hf, 3.8-3.9 with h16).  USAC_LOOP_H16=1 lets the loop use it (tests: the
    // round-5 miscount beside the speculative h16 batch was packed-fp32 VALU corruption beside MFMA
    // waves, gone since the library issues no packed fp32 instruction -- usac_pk.hpp).
    const bool loop_h16 = getenv("USAC_LOOP_H16") && atoi(getenv("USAC_LOOP_H16")) != 0;
    c->h16_off = !loop_h16;
    if (nranks > 1 && !gather && (!c->comm || c->nranks != nranks || c->rank != rank))
        return fail(c, USAC_ERR_ARG, "sharded run without a gather callback needs usac_comm_init(nranks, rank)");
    prosac = prm->sampler == USAC_SAMPLER_PROSAC;
    napsac = prm->sampler == USAC_SAMPLER_NAPSAC;
    if (!prosac && !napsac && prm->sampler != USAC_SAMPLER_UNIFORM && prm->sampler != 0)
        return fail(c, USAC_ERR_UNSUPPORTED, "sampler not supported (Uniform, Napsac, Prosac)");
    knn_mode = napsac && prm->neighbors != USAC_NEIGHBORS_GRID;  // ransac.hpp:62-78
    if (napsac && !knn_mode && c->cols != 4)
        return fail(c, USAC_ERR_ARG, "NAPSAC grid neighbours need 4-column points (SURVEY Q17)");
    if (napsac && !knn_mode && prm->cell_size <= 0) return fail(c, USAC_ERR_ARG, "NAPSAC cell_size must be > 0");
    if (knn_mode && (prm->knn == 0 || prm->knn > usac::kKnnMax || prm->knn + 1 < c->m))
        return fail(c, USAC_ERR_ARG, "NAPSAC KNN: k_nearest_neighbors must be in [sample_size - 1, 32] "
                                     "(napsac_sampler.hpp:48)");
    use_lo = prm->lo == USAC_LO_INITLORSC || prm->lo == USAC_LO_INITFLORSC;
    use_gc = prm->lo == USAC_LO_GC;
    if (prm->lo != USAC_LO_NONE && !use_lo && !use_gc)
        return fail(c, USAC_ERR_UNSUPPORTED, "LO: InItLORsc / InItFLORsc / GC only");
    if (use_gc && napsac)  // ransac.hpp:62-78 gives the neighbours to the sampler only: GC's are unset
        return fail(c, USAC_ERR_UNSUPPORTED, "NAPSAC + GC: the reference leaves the graph cut without neighbours");
    gc_knn = use_gc && prm->neighbors != USAC_NEIGHBORS_GRID;
    if (use_gc && !gc_knn && (c->cols != 4 || prm->cell_size <= 0))
        return fail(c, USAC_ERR_ARG, "GC grid neighbours need 4-column points and cell_size > 0");
    if (gc_knn && (prm->knn == 0 || prm->knn > usac::kKnnMax))
        return fail(c, USAC_ERR_ARG, "GC KNN: k_nearest_neighbors must be in [1, 32]");
    if (use_lo && (prm->lo_sample_size == 0 || prm->lo_iterative_iterations == 0))
        return fail(c, USAC_ERR_ARG, "LO parameters must be > 0");
    if (prosac && c->n <= 20) return fail(c, USAC_ERR_ARG, "PROSAC needs > 20 points (prosac_termination_criteria.hpp:158-163)");
    if (prosac && prm->max_iterations > usac::ProsacSampler::kGrowthMax)
        return fail(c, USAC_ERR_ARG, "PROSAC max_iterations > 200000 (reference draws outside the point range)");
    return USAC_OK;
}

// The context for the run: its device, the batch and single-model buffers, the run's DLT mode, the batch
// SPRT off.  Leaves t0 / tmark started.
int RansacRun::begin() {
    t0 = std::chrono::steady_clock::now();
    tmark = std::chrono::steady_clock::now();
    HIP_TRY(c, hipSetDevice(c->device));
    c->batch_valid = false;  // the run's batches, LO and polish reuse the batch buffers
    int rc = ensure_batch(c, batch);
    if (rc) return rc;
    rc = ensure_single(c);
    if (rc) return rc;
    sub(0);
    c->dlt_mode = prm->dlt_mode;
    c->sprt_on = false;  // the replay verifies exactly; the batch test is off
    return USAC_OK;
}

// the SPRT pool shuffled (n glibc draws) and the pool-ordered points on the device
int RansacRun::pool_upload() {
    sprt->shuffle_pool();
    HIP_TRY(c, hipMemcpyAsync(c->pool_idx.p, sprt->pool().data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, usac::launch_gather_points(c->stream, c->pts.p, c->cols, c->pool_idx.as<uint32_t>(), n,
                                          c->pool_pts.p));
    return USAC_OK;
}

// 2. Construction, in the reference's order.  Reads the flags; leaves the sampler, the termination
// criteria, the neighbours, lo / gc (reserved), the exact-sum buffers, sprt and its pool.
int RansacRun::construct() {
    int rc;
    // Ransac ctor order (ransac.hpp:41-93): sampler, termination criteria, then SPRT -- the
    // SPRT pool shuffle draws n values of the glibc stream before the Uniform sampler's first.
    if (prosac) {
        pro.reset(new usac::ProsacSampler(prm->seed, n, m));
        pterm.reset(new usac::ProsacTerminationCriteria(pro->growth(), prm->desired_prob, m, n, prm->max_iterations));
    } else if (knn_mode) {  // NearestNeighbors::getNearestNeighbors_nanoflann on the device
        knn_tab.resize((size_t)n * prm->knn);
        if ((rc = usac_knn(c, prm->knn, knn_tab.data(), nullptr))) return rc;
        napk.reset(new usac::NapsacKnnSampler(grng, knn_tab.data(), n, m, prm->knn));
    } else if (napsac) {  // getGridNearestNeighbors on the device (kernels_grid.hip)
        if ((rc = download_grid(c, prm->cell_size, grid))) return rc;
        nap.reset(new usac::NapsacSampler(grng, *grid, n, m));
    } else {
        uni.reset(new usac::UniformSampler(grng, n, m));
    }
    sub(1);
    if (use_lo) {
        Shard shard;
        shard.nranks = nranks;
        shard.rank = rank;
        shard.gather = gather;
        shard.user = gather_user;
        lo.reset(new LoRansac(c, prm, shard));
        if ((rc = lo->reserve())) return rc;
    }
    if (use_gc) {  // Ransac ctor neighbours for the graph cut (ransac.hpp:60-78)
        if (gc_knn) {
            knn_tab.resize((size_t)n * prm->knn);
            if ((rc = usac_knn(c, prm->knn, knn_tab.data(), nullptr))) return rc;
        } else if ((rc = download_grid(c, prm->cell_size, grid))) {
            return rc;
        }
        gc.reset(new GcLo(c, prm, gc_knn ? knn_tab.data() : nullptr, prm->knn, grid.get()));
        if ((rc = gc->reserve())) return rc;
    }
    if (!prm->sprt && (rc = reserve_exact_sums(c))) return rc;
    sub(2);
    // PROSAC + SPRT on one rank: the pool shuffle (n glibc draws, the sampler has its own
    // generator) runs after the first batch's solve is enqueued, overlapping it (pool_upload)
    defer_pool = prm->sprt && prosac && nranks == 1 && !getenv("USAC_NO_DEFER_POOL");
    if (prm->sprt) {
        sprt.reset(new usac::Sprt(grng, c->estimator, n, m, prm->max_iterations, max_before_sprt(prm), defer_pool));
        HIP_TRY(c, c->pool_idx.reserve(sizeof(uint32_t) * n));
        HIP_TRY(c, c->pool_pts.reserve(sizeof(float) * c->cols * (size_t)n));
        // the words [nw][rows], then the batch's PoolTail (2 S + 1 + ncomp S words)
        HIP_TRY(c, c->masks.reserve(sizeof(uint32_t) * ((size_t)nw + 2 + (size_t)ncomp(c)) * batch * spk + 4));
        if (!defer_pool && (rc = pool_upload())) return rc;
    }
    return USAC_OK;
}

// 3. Host buffers and speculation state.  Reads batch, the samplers and sprt; leaves the pinned host copies
// sized for a whole batch, spec_ok with its stream, event and reservations, the polish result block and
// its pinned copy, mask_list / mask_check, and the first batch's cap.
int RansacRun::host_buffers() {
    hs.assign((size_t)batch * m, 0);
    hc.resize(SB);
    slot_row.resize(SB);
    hsum.resize(SB);
    hmod.resize((size_t)ncomp(c) * SB);
    hlist.resize(SB + 1);
    hmask.resize(sprt ? ((size_t)nw + 2 + (size_t)ncomp(c)) * SB + 4 : 0);
    subset_at.resize(batch);
    largest_at.resize(batch);
    last_sample.assign(m, 0);
    // Speculation: the next batch is drawn and solved / scored on its own stream while the
    // current batch is replayed (its LO fits run meanwhile).  Its size assumes the replay
    // leaves max_iterations alone; a smaller actual batch takes the prefix of its results (the
    // same samples, the same kernels per hypothesis), and the sampler's extra draws are undone
    // (journal rollback, then a redraw of the kept prefix) before the sampler is used again.
    // Uniform / NAPSAC-grid without SPRT on one rank only (PROSAC's draws depend on the replay).
    spec_ok = !prosac && !prm->sprt && nranks == 1 && !napk && (nap || uni) && !getenv("USAC_NO_SPECULATION");
    hs2.resize(spec_ok ? (size_t)batch * m : 0);
    hc2.resize(spec_ok ? SB : 0);
    hmod2.resize(spec_ok ? (size_t)ncomp(c) * SB : 0);
    spec_last.assign(m, 0);
    if (spec_ok) {
        if (!c->spec_stream) HIP_TRY(c, StreamPool::get().stream(&c->spec_stream));
        if (!c->spec_ev) HIP_TRY(c, StreamPool::get().event(&c->spec_ev));
        // every buffer a batch of `batch` samples grows into, now: a reserve() that grows a
        // block synchronises the device, which must not happen under the speculation
        HIP_TRY(c, c->perm.reserve(usac::presort_bytes(batch)));
        HIP_TRY(c, c->hf_part.reserve(sizeof(int32_t) * 2 * 16 * (size_t)batch));
        if (listed(c)) HIP_TRY(c, c->tv_part.reserve(usac::tv_scratch_bytes(batch * c->spk, c->chunks)));
        if (is_e(c)) HIP_TRY(c, c->e5_ws.reserve(usac::e5_workspace_bytes(batch)));
    }
    inl_list.resize(prosac ? n : 0);

    // (count, sum) of a host model through one pinned D2H (polish result block, slots 12-13)
    HIP_TRY(c, c->pol_res.reserve(sizeof(float) * usac::kPolWords));
    if (!pin_grow(c->pol_pin, sizeof(float) * usac::kPolWords))
        return fail(c, USAC_ERR_HIP, "pinned host allocation failed");

    // PROSAC + SPRT: a new best's inlier list (getUpBoundIterationsSorted's input) decoded from its
    // pool-order mask row on the host instead of a device getInliers round trip per update.  An
    // accepted model's row covers every point (Sprt::verify counts the rest of the pool for a
    // model it keeps), and k_pool_mask evaluates the same residual (no contraction: Makefile) on
    // copies of the same points with the same model words -- except H, whose mask uses the
    // solver's H^-1 where getInliers inverts on the device.  USAC_CHECK_MASK_LIST=1 compares both.
    mask_list = prosac && sprt && c->estimator != USAC_HOMOGRAPHY && !getenv("USAC_DEVICE_INLIERS");
    mask_check = mask_list && getenv("USAC_CHECK_MASK_LIST");
    pt_bits.assign(mask_list ? ((size_t)n + 63) / 64 : 0, 0);

    lap(T_SETUP);
    // with the library's default batch the batches ramp up (1024, 2048, ...): the termination
    // bound drops once the loop has a good model, and a smaller first batch draws, solves and
    // scores fewer hypotheses the run never reaches (the replay is exact for any partition)
    // PROSAC on quality-sorted points finds its model within a few dozen samples and its
    // termination bound then drops to about as many (cfg3: ~9 iterations a run), so its ramp
    // starts at 32
    cap = prm->batch ? batch : std::min<uint32_t>(batch, prosac ? kRampFirstProsac : kRampFirst);
    return USAC_OK;
}

// exact (count, sum) of a host model -> (cnt, s), its inliers in c->inl_idx.
// list_pin (nullable): the whole n-word inlier list copied in the same submission (its
// first cnt words are the list) -- one host wait instead of a second, synchronous copy
int RansacRun::score_inliers(const float *model_host, int32_t *list_pin) {
    float *dres = c->pol_res.as<float>();
    HIP_TRY(c, hipMemcpyAsync(c->one_model.p, model_host, sizeof(float) * 9, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, c->inl_scratch.reserve(usac::inliers_scratch_bytes(c->n, 1)));
    HIP_TRY(c, usac::launch_inliers_batch(c->stream, c->estimator, c->pts.p, c->n, c->one_model.as<float>(), 1, thr,
                                          nullptr, nullptr, c->inl_idx.as<int32_t>(), 0,
                                          reinterpret_cast<int32_t *>(dres + 12), dres + 13, c->inl_scratch.p));
    HIP_TRY(c, hipMemcpyAsync(static_cast<float *>(c->pol_pin.p) + 12, dres + 12, sizeof(float) * 2,
                              hipMemcpyDeviceToHost, c->stream));
    if (list_pin)
        HIP_TRY(c, hipMemcpyAsync(list_pin, c->inl_idx.p, sizeof(int32_t) * (size_t)c->n, hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    memcpy(&cnt, static_cast<const float *>(c->pol_pin.p) + 12, sizeof(int32_t));
    memcpy(&s, static_cast<const float *>(c->pol_pin.p) + 13, sizeof(float));
    return USAC_OK;
}

// the inlier list of a pool-order mask row, ascending (PROSAC + SPRT, mask_list)
int32_t RansacRun::mask_inliers(const uint32_t *row, size_t stride, int32_t *list) {
    std::fill(pt_bits.begin(), pt_bits.end(), 0);
    const uint32_t *pool = sprt->pool().data();
    for (uint32_t w = 0; w < nw; w++)
        for (uint32_t bits = row[(size_t)w * stride]; bits; bits &= bits - 1) {
            const uint32_t p = pool[32 * w + (uint32_t)__builtin_ctz(bits)];
            pt_bits[p >> 6] |= 1ull << (p & 63);
        }
    int32_t k = 0;
    for (size_t w = 0; w < pt_bits.size(); w++)
        for (uint64_t bits = pt_bits[w]; bits; bits &= bits - 1)
            list[k++] = (int32_t)(64 * w + (uint32_t)__builtin_ctzll(bits));
    return k;
}

// draws count samples into buf (the reference's sample array reuse for NAPSAC: a sample the
// sampler leaves (partly) unwritten keeps the previous sample's entries)
void RansacRun::draw_into(int32_t *buf, uint32_t count, usac::ProsacSampler *pro_, uint32_t term_len) {
    for (uint32_t j = 0; j < count; j++) {
        int32_t *smp = buf + (size_t)j * m;
        if (pro_) {
            subset_at[j] = pro_->subset();
            pro_->generateSample(smp, term_len);
            largest_at[j] = pro_->largest();
        } else if (napk) {
            napk->generateSample(smp);
        } else if (napsac) {
            if (j > 0) memcpy(smp, smp - m, sizeof(int32_t) * m);
            else memcpy(smp, last_sample.data(), sizeof(int32_t) * m);
            nap->generateSample(smp);
            if (j + 1 == count) memcpy(last_sample.data(), smp, sizeof(int32_t) * m);
        } else {
            uni->generateSample(smp);
        }
    }
}

// the sampler exactly after the batches consumed so far (undo a speculation's extra draws)
void RansacRun::settle_sampler() {
    if (!sampler_keep) return;
    sampler_rollback();
    last_sample = spec_last;
    draw_into(hs2.data(), sampler_keep, nullptr, n);  // hs2 is free again: the kept batch moved to hs
    sampler_keep = 0;
}

hipError_t RansacRun::spec_wait() {
    for (uint32_t spins = 0;; spins++) {
        const hipError_t e = hipEventQuery(c->spec_ev);
        if (e != hipErrorNotReady) return e;
        if ((spins & 1023u) == 1023u) std::this_thread::yield();
    }
}

// 4. The batch's size, and the batch drawn ahead taken (its first B samples are this batch: have) or dropped.
// Reads spec / spec_B; leaves B, cap, have, spec_hst, the sampler marks and the spec_* counters.
int RansacRun::take_speculation() {
    B = std::min(std::min(batch, max_iters - iters), cap);
    if (!prm->batch) cap = std::min<uint32_t>(batch, 2 * cap);
    have = false;  // this batch's device results are already on the host (speculation)
    spec_hst = 0;
    if (spec) {
        spec = false;
        HIP_TRY(c, spec_wait());
        if (B <= spec_B) {  // its first B samples are this batch
            std::swap(hs, hs2);
            std::swap(hc, hc2);
            std::swap(hmod, hmod2);
            spec_hst = (size_t)spec_B * spk;
            have = true;
            if (B < spec_B) {
                sampler_keep = B;  // undone lazily, before the next draw
                out->spec_rollbacks++;
                out->spec_wasted += spec_B - B;
            } else {
                sampler_commit();
            }
        } else {  // (max_iterations grew) the speculation is dropped
            out->spec_wasted += spec_B;
            sampler_rollback();
            last_sample = spec_last;
        }
    }
    return USAC_OK;
}

// 5. Draw.  Reads have; leaves B samples in hs (PROSAC: gen_term, the sampler's snapshot, subset_at / largest_at).
void RansacRun::draw() {
    // ---- draw the batch (speculatively for PROSAC)
    snapshot.reset();
    gen_term = prosac ? pterm->terminationLength() : n;
    if (!have) {
        settle_sampler();
        const auto td0 = std::chrono::steady_clock::now();
        if (prosac) snapshot.reset(new usac::ProsacSampler(*pro));
        draw_into(hs.data(), B, prosac ? pro.get() : nullptr, gen_term);
        t_drawonly += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td0).count();
    }
    lap(T_DRAW);
}

// 6a. The one-rank device batch: solve, then the scorer's counts or (SPRT) the pool-order words, and the
// download ladder (PoolTail / whole copy / rows only).  Reads hs, B, S; leaves hc, hmod (stride hst), and
// with SPRT hlist, hmask, rows, mask_stride.
int RansacRun::one_rank_batch() {
    int rc;
    HIP_TRY(c, hipMemcpyAsync(c->samples.p, hs.data(), sizeof(int32_t) * (size_t)B * m, hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, enqueue_solve(c, c->samples.as<int32_t>(), B, 0, iters, nullptr));
    const size_t mstride = (size_t)B * spk;
    // listed SPRT batches: the slot counts, list and models ride behind the words (PoolTail)
    const bool tailed = sprt && listed(c) && !getenv("USAC_NO_POOL_TAIL");
    const size_t tail_off = (size_t)nw * S, tail_words = (2 + (size_t)ncomp(c)) * S + 1;
    if (sprt && !sprt->pool_ready() && (rc = pool_upload())) return rc;  // deferred: behind the solve
    if (sprt) {
        const usac::PoolTail tail{reinterpret_cast<const uint32_t *>(c->counts.p), c->list_n.as<uint32_t>(),
                                  c->list.as<uint32_t>(), c->models.as<uint32_t>(), (uint32_t)S,
                                  (uint32_t)(ncomp(c) * S), c->masks.as<uint32_t>() + tail_off};
        HIP_TRY(c, usac::launch_pool_mask(c->stream, c->estimator, c->pool_pts.p, n, c->models.as<float>(), mstride,
                                          listed(c) ? c->list.as<uint32_t>() : nullptr,
                                          listed(c) ? c->list_n.as<uint32_t>() : nullptr, (uint32_t)S, thr,
                                          c->masks.as<uint32_t>(), listed(c) ? 0u : (uint32_t)S,
                                          tailed ? &tail : nullptr));
    } else {  // exact counts from the fast multi-chunk scorer; exact sums below, where needed
        HIP_TRY(c, enqueue_score(c, B, thr, loop_chunks(c, B)));
        HIP_TRY(c, hipMemcpyAsync(hc.data(), c->counts.p, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
    }
    // the device's component-major [ncomp][S] block in one copy (host stride S this batch:
    // every copy costs a fixed overhead, 18 per-component copies of a ramp batch cost more
    // than the batch's kernels)
    hst = S;
    if (!tailed)
        HIP_TRY(c, hipMemcpyAsync(hmod.data(), c->models.p, sizeof(float) * S * ncomp(c), hipMemcpyDeviceToHost,
                                  c->stream));
    const uint32_t *htail = nullptr;  // the batch's PoolTail on the host
    auto untail = [&]() {
        memcpy(hc.data(), htail, sizeof(int32_t) * S);
        hlist[SB] = htail[S];
        memcpy(hlist.data(), htail + S + 1, sizeof(uint32_t) * S);
        memcpy(hmod.data(), htail + 2 * S + 1, sizeof(float) * S * ncomp(c));
    };
    if (tailed) {
        // small batches (the PROSAC ramp's first ones, where a cfg3 run ends): words and tail in
        // one copy, one host wait; larger ones: the tail first, then only the rows' words (the
        // words are packed [nw][rows] on the device: k_pool_mask, row stride 0)
        const bool whole = (size_t)nw * S * sizeof(uint32_t) <= kMaskWholeCopy;
        if (whole) {
            HIP_TRY(c, hipMemcpyAsync(hmask.data(), c->masks.p, sizeof(uint32_t) * (tail_off + tail_words),
                                      hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, stream_wait(c->stream));
            htail = hmask.data() + tail_off;
            untail();
        } else {
            HIP_TRY(c, hipMemcpyAsync(hmask.data() + (size_t)nw * SB, c->masks.as<uint32_t>() + tail_off,
                                      sizeof(uint32_t) * tail_words, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, stream_wait(c->stream));
            htail = hmask.data() + (size_t)nw * SB;
            untail();
            rows = hlist[SB];
            if (rows) HIP_TRY(c, hipMemcpyAsync(hmask.data(), c->masks.p, sizeof(uint32_t) * (size_t)rows * nw,
                                                hipMemcpyDeviceToHost, c->stream));
        }
    } else if (sprt) {
        // listed: the occupied rows' words packed [nw][rows] on the device (k_pool_mask, row
        // stride 0).  Small batches (the PROSAC ramp's first ones, where a cfg3 run ends): the
        // whole block with the list in the same submission -- one host wait; larger ones: the
        // list count first, then only the rows' words (a plain copy: hipMemcpy2DAsync's first
        // call in a process cost ~7 ms, round 5)
        const bool whole = !listed(c) || (size_t)nw * S * sizeof(uint32_t) <= kMaskWholeCopy;
        if (listed(c)) {  // occupied slots -> mask rows
            HIP_TRY(c, hipMemcpyAsync(hc.data(), c->counts.p, sizeof(int32_t) * S, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(hlist.data() + SB, c->list_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost,
                                      c->stream));
            if (whole) {
                HIP_TRY(c, hipMemcpyAsync(hlist.data(), c->list.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost,
                                          c->stream));
            } else {
                HIP_TRY(c, stream_wait(c->stream));
                rows = hlist[SB];
                if (rows) HIP_TRY(c, hipMemcpyAsync(hlist.data(), c->list.p, sizeof(uint32_t) * rows,
                                                    hipMemcpyDeviceToHost, c->stream));
            }
        } else {
            std::fill(hc.begin(), hc.begin() + S, 0);
        }
        if (whole) {
            mask_stride = (uint32_t)S;  // listed: the row count, below
            HIP_TRY(c, hipMemcpyAsync(hmask.data(), c->masks.p, sizeof(uint32_t) * S * nw, hipMemcpyDeviceToHost,
                                      c->stream));
        } else if (rows) {
            HIP_TRY(c, hipMemcpyAsync(hmask.data(), c->masks.p, sizeof(uint32_t) * (size_t)rows * nw,
                                      hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(c, stream_wait(c->stream));
    if (sprt && listed(c)) mask_stride = rows = hlist[SB];
    return USAC_OK;
}

// 6. Device batch: already here (speculation), sharded, or one rank.  Leaves S, hst, rows, mask_stride,
// the host arrays and slot_row.
int RansacRun::device_batch() {
    int rc;
    // ---- device: solve, then exact scores or pool-order flags
    S = (size_t)B * spk;
    hst = SB;  // host stride of hmod's components this batch
    rows = (uint32_t)S;
    mask_stride = (uint32_t)S;  // host row stride of hmask (SPRT)
    if (have) {
        hst = spec_hst;
    } else if (nranks > 1) {  // this rank's slice, then the all-gather of every slice's counts and models
        if ((rc = sharded_batch(c, hs.data(), B, iters, thr, nranks, rank, gather, gather_user, xbuf, hc.data(),
                                hmod.data(), SB, sprt != nullptr, hmask.data())))
            return rc;
    } else if ((rc = one_rank_batch())) {
        return rc;
    }
    if (sprt) {
        if (listed(c) && nranks == 1) {
            std::fill(slot_row.begin(), slot_row.begin() + S, -1);
            for (uint32_t r = 0; r < rows; r++) slot_row[hlist[r]] = (int32_t)r;
        } else {
            for (size_t sl = 0; sl < S; sl++) slot_row[sl] = (int32_t)sl;
        }
    }
    return USAC_OK;
}

// 7. Speculate the next batch on the spec stream.  Reads hc, best, max_iters; leaves spec, spec_B, hs2 /
// hc2 / hmod2 in flight.
int RansacRun::speculate_next() {
    // ---- speculation: the next batch, as if the replay leaves max_iterations alone -- unless
    // this batch certainly ends the run: the replay leaves max_iters <= the termination bound
    // of its final best, whose count is at least every count of this batch (Score::bigger
    // orders by count first; LO only adds inliers) and the bound does not grow with the count
    bool spec_next = spec_ok && iters + B < max_iters;
    if (spec_next) {
        int maxc = best.inlier_number;
        for (size_t sl = 0; sl < S; sl++) maxc = std::max(maxc, hc[sl]);
        spec_next = term.getUpBoundIterations((uint32_t)maxc) > iters + B;
    }
    if (spec_next) {
        settle_sampler();
        const uint32_t B2 = std::min(std::min(batch, max_iters - (iters + B)), cap);
        sampler_mark();
        spec_last = last_sample;
        draw_into(hs2.data(), B2, nullptr, n);
        const size_t S2 = (size_t)B2 * spk;
        std::swap(c->stream, c->spec_stream);  // the launchers enqueue on c->stream
        hipError_t e = hipMemcpyAsync(c->samples.p, hs2.data(), sizeof(int32_t) * (size_t)B2 * m,
                                      hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = enqueue_solve(c, c->samples.as<int32_t>(), B2, 0, iters + B, nullptr);
        if (e == hipSuccess) e = enqueue_score(c, B2, thr, loop_chunks(c, B2));
        if (e == hipSuccess)
            e = hipMemcpyAsync(hc2.data(), c->counts.p, sizeof(int32_t) * S2, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(hmod2.data(), c->models.p, sizeof(float) * S2 * ncomp(c), hipMemcpyDeviceToHost,
                               c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->spec_ev, c->stream);
        std::swap(c->stream, c->spec_stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->spec_stream);
            return fail(c, USAC_ERR_HIP, std::string("speculative batch: ") + hipGetErrorString(e));
        }
        spec = true;
        spec_B = B2;
        out->spec_batches++;
    }
    lap(T_DEVICE);
    return USAC_OK;
}

// Exact sums of the slots the replay can read.  Reads hc, hmod; leaves hsum.
int RansacRun::sums() {
    int rc;
    if (!sprt && (rc = exact_sums(c, thr, best.inlier_number, hc.data(), hmod.data(), hst, S, hsum.data(),
                                  &out->sum_models)))
        return rc;
    lap(T_SUMS);
    out->batches++;
    return USAC_OK;
}

// 8. Sequential replay of the batch, the PROSAC rewind included.  Reads the host arrays; leaves best,
// best_model, iters, max_iters, the records and the run counters.
int RansacRun::replay() {
    int rc;
    // ---- sequential replay
    uint32_t j = 0;
    bool rewind = false;
    for (; j < B && iters < max_iters; j++) {
        for (uint32_t q = 0; q < spk; q++) {
            const size_t sl = (size_t)j * spk + q;
            if (hc[sl] < 0) break;  // empty slot: the sample has no more models
            usac::Score cur;
            int32_t r = 0;
            if (sprt) {
                r = slot_row[sl];
                const auto tv0 = std::chrono::steady_clock::now();
                const bool good = sprt->verify(hmask.data() + r, (int)iters, (uint32_t)best.inlier_number,
                                               cur.inlier_number, cur.score, mask_stride);
                t_verify += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tv0).count();
                if (!good) {
                    out->sprt_rejected++;
                    if ((int)iters >= max_before) {  // max_hypothesis_test_before_sprt (model.hpp:40), Q9
                        iters++;
                        continue;
                    }
                }
            } else {
                cur.inlier_number = hc[sl];
                cur.score = hsum[sl];
            }
            if (!cur.bigger(best)) continue;
            float model[9];
            for (int k = 0; k < 9; k++) model[k] = k < ncomp(c) ? hmod[(size_t)k * hst + sl] : 0.f;
            if (lo) {  // ransac.cpp:110-112, before the best is replaced
                lap(T_REPLAY);
                lo->run(model, cur.inlier_number, cur.score);
                if (lo->rc) return lo->rc;
                lap(T_LO);
            }
            if (gc) {
                lap(T_REPLAY);
                gc->run(model, cur.inlier_number, cur.score);
                if (gc->rc) return gc->rc;
                lap(T_LO);
            }
            best = cur;
            memcpy(best_model, model, sizeof(best_model));
            if (prosac && mask_list) {
                cnt = mask_inliers(hmask.data() + r, mask_stride, inl_list.data());
                if (mask_check) {
                    std::vector<int32_t> dl(n);
                    const int32_t mc = cnt;
                    if ((rc = score_inliers(best_model, dl.data()))) return rc;
                    const std::vector<int32_t> tmp(inl_list.data(), inl_list.data() + mc);
                    if (cnt != mc || cnt != cur.inlier_number ||
                        !std::equal(tmp.begin(), tmp.end(), dl.begin()))
                        return fail(c, USAC_ERR_HIP, "mask-decoded inlier list differs from getInliers");
                    cnt = mc;
                }
                max_iters = pterm->getUpBoundIterationsSorted(iters, inl_list.data(), (uint32_t)cnt, largest_at[j]);
            } else if (prosac) {
                if ((rc = score_inliers(best_model, inl_list.data()))) return rc;
                // (the list is ascending: the compaction keeps point order)
                max_iters = pterm->getUpBoundIterationsSorted(iters, inl_list.data(), (uint32_t)cnt, largest_at[j]);
            } else {
                max_iters = term.getUpBoundIterations((uint32_t)best.inlier_number);
            }
            if (sprt) max_iters = std::min(max_iters, sprt->getUpperBoundIterations(best.inlier_number));
            if (records && (uint32_t)nrec < rec_cap) {
                usac_record &rr = records[nrec];
                rr.hyp_index = iters;
                rr.inliers = cur.inlier_number;
                rr.score = cur.score;
                memcpy(rr.model, best_model, sizeof(best_model));
                rr.valid = 1;
            }
            nrec++;
        }
        iters++;
        if (prosac && pterm->terminationLength() != gen_term && j + 1 < B) {
            // would the NEXT sample be drawn differently (prosac_sampler.hpp: a subset above the
            // termination length takes the uniform draw)?  The subsets only grow and the length
            // only shrinks, so the batch's samples stay valid up to the first one that would --
            // the replay goes on through them (the run often ends there) and rewinds at it
            const uint32_t tl = pterm->terminationLength();
            rewind = (subset_at[j + 1] > gen_term) || (subset_at[j + 1] > tl);
            if (rewind) break;
        }
    }
    if (rewind) {  // sampler state just after sample j: replay the first j + 1 draws
        pro = std::move(snapshot);
        std::vector<int32_t> tmp(m);
        for (uint32_t k = 0; k <= j; k++) pro->generateSample(tmp.data(), gen_term);
        out->rollbacks++;
    }
    return USAC_OK;
}

void RansacRun::lo_counters() {
    out->lo_inner_iters = lo ? lo->inner_count : gc ? gc->gc_iters : 0;
    out->lo_iterative_iters = lo ? lo->iterative_count : gc ? gc->labelings : 0;
    out->lo_rounds = lo ? lo->rounds : gc ? gc->labelings : 0;
    out->lo_stages = lo ? lo->stages : gc ? gc->stages : 0;
    out->lo_fits = lo ? lo->fits : 0;
}

// 9. Finish: the loop's out fields, no-model exit, the forced graph cut.  Reads best / best_model; may raise them.
int RansacRun::finish() {
    if (spec) out->spec_wasted += spec_B;  // the run ended before the batch drawn ahead
    out->iters = iters;
    out->n_records = nrec;
    out->sprt_histories = sprt ? (int32_t)sprt->histories() : 0;
    out->prosac_term_len = prosac ? pterm->terminationLength() : n;
    lo_counters();
    memcpy(out->minimal_model, best_model, sizeof(best_model));
    out->minimal_inliers = best.inlier_number;
    if (best.inlier_number == 0) {
        memcpy(out->model, best_model, sizeof(best_model));
        return fail(c, USAC_ERR_NO_MODEL, "best score is 0 (ransac.cpp:143-147)");
    }
    if (gc && gc->gc_iters == 0) {  // "Graph Cut lo was set, but did not run, run it" (ransac.cpp:149-153)
        lap(T_REPLAY);
        gc->run(best_model, best.inlier_number, best.score);
        if (gc->rc) return gc->rc;
        lap(T_LO);
        lo_counters();
        memcpy(out->minimal_model, best_model, sizeof(best_model));
        out->minimal_inliers = best.inlier_number;
    }

    lap(T_REPLAY);
    return USAC_OK;
}

// ransac.cpp:170-200 on the results of passes k0 .. k1 - 1 (pol_pin)
void RansacRun::polish_replay(int k0, int k1, const float *hres, int32_t *const *lists, int &prev, bool &stop) {
    int32_t ok = 0;
    for (int k = k0; k < k1; k++) {
        const float *r = hres + usac::kPolPass * k;
        memcpy(&ok, r + 9, sizeof(int32_t));
        memcpy(&cnt, r + 10, sizeof(int32_t));
        memcpy(&s, r + 11, sizeof(float));
        if (!ok || (double)((float)cnt / (float)best.inlier_number) < 0.8 || cnt <= prev) {
            stop = true;
            break;
        }
        prev = cnt;
        best.inlier_number = cnt;
        best.score = s;
        memcpy(best_model, r, sizeof(best_model));
        cur = lists[k + 1];
        cur_cnt = cnt;
        out->polish_passes++;
    }
}

// the fused polish's phases (us): getInliers, then per pass gather, means,
// distance terms, distances, A^T A, finish, score, Σerr
int RansacRun::polish_fused_profile(int k_first) {
    uint64_t st[64] = {0};
    HIP_TRY(c, hipMemcpy(st, c->partial.p, sizeof(st), hipMemcpyDeviceToHost));
    fprintf(stderr, "polish_fused us: init %.1f %.1f |", (st[1] - st[0]) * 0.01, (st[2] - st[1]) * 0.01);
    uint64_t last = st[2];
    for (int k = 0; k < k_first; k++) {
        for (int i = 0; i < 8; i++) {
            const uint64_t v = st[3 + 8 * k + i];
            fprintf(stderr, " %.1f", v >= last ? (v - last) * 0.01 : -1.0);
            if (v >= last) last = v;
        }
        fprintf(stderr, " |");
    }
    fprintf(stderr, " walked segments: 4ch %llu 2ch %llu 1ch %llu\n", (unsigned long long)st[44],
            (unsigned long long)st[42], (unsigned long long)st[41]);
    return USAC_OK;
}

// pass k of the multi-launch polish enqueued: the fit of list k, its scoring into list k + 1
int RansacRun::polish_pass(int k, float *dres, int32_t *dres_i, int32_t *const *lists, bool finish_score) {
    float *pres = dres + usac::kPolPass * k;
    int32_t *dok = dres_i + usac::kPolPass * k + 9;
    // the pass's finish, scoring and acceptance in one workgroup (k_finish_score) when the
    // points fit its LDS and the fit takes the multi-launch path
    const uint32_t nfit = k == 0 ? (uint32_t)best.inlier_number : c->n;
    const bool fs = finish_score && nfit > usac::kSmallFitMax;
    usac::NmBatch nb{};
    if (k == 0)
        HIP_TRY(c, enqueue_nonminimal(c, lists[0], nfit, pres, dok, nullptr, nullptr, fs ? &nb : nullptr));
    else  // the count pass k - 1's acceptance left on the device; c->n bounds it
        HIP_TRY(c, enqueue_nonminimal(c, lists[k], nfit, pres, dok, nullptr,
                                      reinterpret_cast<const uint32_t *>(dres_i + usac::kPolNs + k),
                                      fs ? &nb : nullptr));
    if (fs) {
        HIP_TRY(c, usac::launch_finish_score(c->stream, c->estimator, nb, c->pts.p, c->n, thr, lists[k + 1],
                                             dok + 1, pres + 11, dres_i, k + 1 < kPasses ? k : -1,
                                             best.inlier_number));
        return USAC_OK;
    }
    HIP_TRY(c, usac::launch_inliers_batch(c->stream, c->estimator, c->pts.p, c->n, pres, 1, thr, nullptr,
                                          nullptr, lists[k + 1], 0, dok + 1, pres + 11, c->inl_scratch.p, dok));
    if (k + 1 < kPasses) HIP_TRY(c, usac::launch_polish_prep(c->stream, dres_i, k, best.inlier_number));
    return USAC_OK;
}

// 10. Polish.  Reads best / best_model; leaves them polished, cur / cur_cnt (best_model's own inlier list on
// the device) and out->polish_passes.
int RansacRun::polish() {
    int rc;
    // ---- polish (ransac.cpp:157-207) on the device, the passes submitted in groups: pass k
    // fits the list pass k - 1 scored (the initial getInliers(best_model) list for pass 0) and
    // scores the fitted model from device memory into list k + 1 (compaction gated on the fit's
    // ok); between passes k_polish_prep takes the host's acceptance decision on the device and
    // hands pass k + 1 its point count, or 0 after a rejection (a no-op pass).  All results land
    // in one device block (usac_kernels.h kPol*) copied with one D2H per group; the host replays the
    // reference's loop on them and stops at the first rejection, so `cur` ends as best_model's
    // own inlier list (the same kernels, model and threshold as the final getInliers would use).
    HIP_TRY(c, c->pol_res.reserve(sizeof(float) * usac::kPolWords));
    HIP_TRY(c, c->pol_lists.reserve(sizeof(int32_t) * 4 * (size_t)std::max<uint32_t>(c->n, 1)));
    HIP_TRY(c, c->inl_scratch.reserve(usac::inliers_scratch_bytes(c->n, 1)));
    if (!pin_grow(c->pol_pin, sizeof(float) * usac::kPolWords))
        return fail(c, USAC_ERR_HIP, "pinned host allocation failed");
    float *dres = c->pol_res.as<float>();
    int32_t *dres_i = c->pol_res.as<int32_t>();
    const float *hres = static_cast<const float *>(c->pol_pin.p);
    int32_t *lists[5] = {c->inl_idx.as<int32_t>(), c->pol_lists.as<int32_t>(), nullptr, nullptr, nullptr};
    for (int k = 2; k < 5; k++) lists[k] = lists[1] + (size_t)(k - 1) * std::max<uint32_t>(c->n, 1);
    HIP_TRY(c, hipMemcpyAsync(c->one_model.p, best_model, sizeof(float) * 9, hipMemcpyHostToDevice, c->stream));
    // USAC_POLISH_FUSED=1: the whole polish in one workgroup (k_polish_fused) when the best
    // model's list and the point set fit its LDS -- one launch instead of ~56, bit-identical, but
    // not faster on cfg3 exact (0.30-0.33 vs 0.28 ms: the sequential sums' 64-candidate
    // speculation needs more than one CU's issue rate), so off by default
    // (USAC_POLISH_FUSED_MAX: a lower list bound, which makes the tests resume passes the
    // multi-launch way)
    const char *fe = getenv("USAC_POLISH_FUSED"), *fm = getenv("USAC_POLISH_FUSED_MAX");
    const uint32_t fit_max = fm ? std::min<uint32_t>((uint32_t)atoi(fm), usac::kPolFitMax) : usac::kPolFitMax;
    const bool fused = fe && atoi(fe) != 0 && c->estimator != USAC_LINE2D && c->n <= usac::kPolPtsMax &&
                       (uint32_t)best.inlier_number <= fit_max;
    const bool pol_prof = fused && getenv("USAC_PROFILE");
    if (pol_prof) {
        HIP_TRY(c, c->partial.reserve(sizeof(uint64_t) * 64));
        HIP_TRY(c, hipMemsetAsync(c->partial.p, 0, sizeof(uint64_t) * 64, c->stream));
    }
    if (fused)
        HIP_TRY(c, usac::launch_polish_fused(c->stream, c->estimator, c->pts.p, c->n, c->one_model.as<float>(), thr,
                                             best.inlier_number, usac::PolLists{{lists[0], lists[1], lists[2], lists[3],
                                                                                 lists[4]}},
                                             dres_i, fit_max, pol_prof ? c->partial.as<uint64_t>() : nullptr));
    else
        HIP_TRY(c, usac::launch_inliers_batch(c->stream, c->estimator, c->pts.p, c->n, c->one_model.as<float>(), 1,
                                              thr, nullptr, nullptr, lists[0], 0, dres_i + 12, dres + 13,
                                              c->inl_scratch.p));  // quality->getInliers(best_model)
    // passes go out in groups of G (USAC_POLISH_GROUP): a group is one submission and one host
    // wait; the next group is submitted only while every pass so far was accepted.  Default: all
    // four at once for a best model of <= 8192 inliers (cfg3 exact: 1.15 vs 1.20-1.28 ms per run
    // with groups of 2), two above (cfg5's 17 k-inlier fits: a rejected pass's no-op successors
    // cost 0.1 ms; profiles/r4c/ab_polish.txt, profiles/r5/polish_ab.txt)
    const int kGroup = [&] {
        const char *g = getenv("USAC_POLISH_GROUP");
        const int v = g ? atoi(g) : best.inlier_number <= 8192 ? 4 : 2;
        return v < 1 ? 1 : v > kPasses ? kPasses : v;
    }();
    cur = lists[0];
    cur_cnt = 0;
    int prev = 0;
    bool stop = false;
    int k_first = 0;  // the first pass for the multi-launch path
    const bool finish_score = c->estimator != USAC_LINE2D && c->n <= usac::kPolPtsMax;
    if (fused) {
        HIP_TRY(c, hipMemcpyAsync(c->pol_pin.p, dres, sizeof(float) * usac::kPolWords, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, stream_wait(c->stream));
        memcpy(&cur_cnt, hres + 12, sizeof(int32_t));
        memcpy(&k_first, hres + usac::kPolStop, sizeof(int32_t));
        if (k_first < 0 || k_first > kPasses) return fail(c, USAC_ERR_HIP, "fused polish: bad pass count");
        polish_replay(0, k_first, hres, lists, prev, stop);
        if (pol_prof && (rc = polish_fused_profile(k_first))) return rc;
    }
    for (int k0 = k_first; k0 < kPasses && !stop; k0 += kGroup) {
        const int k1 = std::min(k0 + kGroup, kPasses);
        for (int k = k0; k < k1; k++)
            if ((rc = polish_pass(k, dres, dres_i, lists, finish_score))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->pol_pin.p, dres, sizeof(float) * usac::kPolPass * k1, hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, stream_wait(c->stream));
        if (k0 == 0) memcpy(&cur_cnt, hres + 12, sizeof(int32_t));
        polish_replay(k0, k1, hres, lists, prev, stop);
    }
    return USAC_OK;
}

// 11. The USAC_PROFILE line, the inlier list and the last out fields.
int RansacRun::emit() {
    const auto t1 = std::chrono::steady_clock::now();
    lap(T_POLISH);
    if (getenv("USAC_PROFILE"))
        fprintf(stderr,
                "usac_ransac_run ms: setup %.3f draw %.3f device %.3f sums %.3f replay %.3f lo %.3f polish %.3f "
                "(lo rounds %u stages %u enqueue %.3f poll %.3f; setup: buffers %.3f neighbours %.3f "
                "lo/gc %.3f; sprt walks %.3f, draws %.3f; iters %u batches %u)\n",
                tsplit[T_SETUP], tsplit[T_DRAW], tsplit[T_DEVICE], tsplit[T_SUMS], tsplit[T_REPLAY], tsplit[T_LO],
                tsplit[T_POLISH], lo ? lo->rounds : gc ? gc->labelings : 0u, lo ? lo->stages : gc ? gc->stages : 0u,
                lo ? lo->t_enqueue : 0.0, lo ? lo->t_poll : 0.0, tsub[0],
                tsub[1] - tsub[0], tsub[2] - tsub[1], t_verify, t_drawonly, iters, (uint32_t)out->batches);
    // ransac.cpp:214 getInliers(best_model): `cur` already is that list (see above)
    cnt = cur_cnt;
    if (inliers_out && cnt > 0) {  // DMA into pinned memory, then into the caller's buffer
        pinned_vector<int32_t> stage((size_t)cnt);
        HIP_TRY(c, hipMemcpyAsync(stage.data(), cur, sizeof(int32_t) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, stream_wait(c->stream));
        memcpy(inliers_out, stage.data(), sizeof(int32_t) * (size_t)cnt);
    }
    memcpy(out->model, best_model, sizeof(best_model));
    out->inliers = best.inlier_number;
    out->time_us = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
    return USAC_OK;
}

}  // namespace

// Ransac::run with each batch's hypotheses sharded over nranks: every rank
// draws the same host sample stream, solves and scores only its contiguous slice of the
// batch, and the slices' per-slot counts and models are all-gathered (gather(), or RCCL on
// the context's communicator when gather is null); the replay -- records, termination, LO,
// polish -- then runs on the merged batch identically on every rank (ransac.cpp:58-139 order).
static int ransac_run_impl(usac_ctx *c, const usac_params *prm, int nranks, int rank, usac_allgather_fn gather,
                           void *gather_user, usac_run_output *out, int32_t *inliers_out, usac_record *records,
                           uint32_t rec_cap) {
    if (!c || !prm || !out || nranks < 1 || rank < 0 || rank >= nranks) return USAC_ERR_ARG;
    memset(out, 0, sizeof(*out));
    // what the run changes in the context goes back on every exit, after the run's state is gone
    struct H16Off {
        usac_ctx *c;
        bool saved;
        ~H16Off() { c->h16_off = saved; }
    } h16_off{c, c->h16_off};
    struct Restore {
        usac_ctx *c;
        int mode;
        bool sprt;
        ~Restore() {
            c->dlt_mode = mode;
            c->sprt_on = sprt;
        }
    } restore{c, c->dlt_mode, c->sprt_on};
    RansacRun r(c, prm, nranks, rank, gather, gather_user, out, inliers_out, records, rec_cap);
    int rc;
    if ((rc = r.check_params())) return rc;
    if ((rc = r.begin())) return rc;
    if ((rc = r.construct())) return rc;
    if ((rc = r.host_buffers())) return rc;
    while (r.iters < r.max_iters) {
        if ((rc = r.take_speculation())) return rc;
        r.draw();
        if ((rc = r.device_batch())) return rc;
        if ((rc = r.speculate_next())) return rc;
        if ((rc = r.sums())) return rc;
        if ((rc = r.replay())) return rc;
    }
    if ((rc = r.finish())) return rc;
    if ((rc = r.polish())) return rc;
    return r.emit();
}

int usac_ransac_run(usac_ctx *c, const usac_params *prm, usac_run_output *out, int32_t *inliers_out,
                    usac_record *records, uint32_t rec_cap) {
    return ransac_run_impl(c, prm, 1, 0, nullptr, nullptr, out, inliers_out, records, rec_cap);
}

int usac_ransac_run_sharded(usac_ctx *c, const usac_params *prm, int nranks, int rank, usac_allgather_fn gather,
                            void *gather_user, usac_run_output *out, int32_t *inliers_out, usac_record *records,
                            uint32_t rec_cap) {
    return ransac_run_impl(c, prm, nranks, rank, gather, gather_user, out, inliers_out, records, rec_cap);
}

// ---------------------------------------------------------------- multi-GPU
int usac_comm_unique_id(uint8_t *id128) {
    if (!id128) return USAC_ERR_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return USAC_ERR_HIP;
    memcpy(id128, &id, sizeof(id) < 128 ? sizeof(id) : 128);
    return USAC_OK;
}

int usac_comm_init(usac_ctx *c, int nranks, int rank, const uint8_t *id128) {
    if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return USAC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id) < 128 ? sizeof(id) : 128);
    NCCL_TRY(c, ncclCommInitRank(&c->comm, nranks, id, rank));
    if (!c->coll_ev) HIP_TRY(c, StreamPool::get().event(&c->coll_ev));
    c->nranks = nranks;
    c->rank = rank;
    HIP_TRY(c, c->rec_send.reserve(sizeof(usac_record)));
    HIP_TRY(c, c->rec_all.reserve(sizeof(usac_record) * (size_t)nranks));
    return USAC_OK;
}

int usac_comm_count(usac_ctx *c, int *nranks, int *rank, int *device) {
    if (!c || !nranks || !rank || !device) return USAC_ERR_ARG;
    if (!c->comm) return fail(c, USAC_ERR_ARG, "usac_comm_init not called");
    NCCL_TRY(c, ncclCommCount(c->comm, nranks));
    NCCL_TRY(c, ncclCommUserRank(c->comm, rank));
    NCCL_TRY(c, ncclCommCuDevice(c->comm, device));
    return USAC_OK;
}

int usac_exchange_best_async(usac_ctx *c, usac_ctx *batch, uint32_t slot) {
    if (!c || !batch || slot >= USAC_XRING) return USAC_ERR_ARG;
    if (!c->comm) return fail(c, USAC_ERR_ARG, "usac_comm_init not called");
    if (batch->device != c->device) return fail(c, USAC_ERR_ARG, "exchange: batch context on another device");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->xstream) {
        HIP_TRY(c, StreamPool::get().stream(&c->xstream));
        for (int k = 0; k < USAC_XRING; k++) {
            HIP_TRY(c, StreamPool::get().event(&c->xev_batch[k]));
            HIP_TRY(c, StreamPool::get().event(&c->xev_done[k]));
        }
        HIP_TRY(c, c->xring.reserve(sizeof(usac_record) * (size_t)USAC_XRING * (size_t)(c->nranks + 1)));
        if (!pin_grow(c->xring_host, sizeof(usac_record) * (size_t)USAC_XRING * (size_t)c->nranks))
            return fail(c, USAC_ERR_HIP, "pinned host allocation failed");
    }
    // the batch's argmax record is copied into the ring's send slot on the batch stream (the
    // batch's next use of that stream overwrites its record); the exchange stream waits for
    // that copy only (neither stream waits for the other's later work)
    usac_record *dsend = c->xring.as<usac_record>() + (size_t)USAC_XRING * c->nranks + slot;
    usac_record *dall = c->xring.as<usac_record>() + (size_t)slot * c->nranks;
    HIP_TRY(c, hipMemcpyAsync(dsend, batch->best.p, sizeof(usac_record), hipMemcpyDeviceToDevice, batch->stream));
    HIP_TRY(c, hipEventRecord(c->xev_batch[slot], batch->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->xstream, c->xev_batch[slot], 0));
    if (c->coll_pending) {  // after the last collective issued on c->stream
        HIP_TRY(c, hipStreamWaitEvent(c->xstream, c->coll_ev, 0));
        c->coll_pending = false;
    }
    NCCL_TRY(c, ncclAllGather(dsend, dall, sizeof(usac_record), ncclUint8, c->comm, c->xstream));
    HIP_TRY(c, hipMemcpyAsync(c->xring_records() + (size_t)slot * c->nranks, dall, sizeof(usac_record) * (size_t)c->nranks,
                              hipMemcpyDeviceToHost, c->xstream));
    HIP_TRY(c, hipEventRecord(c->xev_done[slot], c->xstream));
    c->x_last = (int)slot;
    return USAC_OK;
}

int usac_exchange_best_wait(usac_ctx *c, uint32_t slot, usac_record *all) {
    if (!c || !all || slot >= USAC_XRING || !c->xstream) return USAC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    for (uint32_t spins = 0;; spins++) {  // poll (as stream_wait): returns within ~1 us
        const hipError_t e = hipEventQuery(c->xev_done[slot]);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) return fail(c, USAC_ERR_HIP, std::string("exchange: ") + hipGetErrorString(e));
        if ((spins & 1023u) == 1023u) std::this_thread::yield();
    }
    memcpy(all, c->xring_records() + (size_t)slot * c->nranks, sizeof(usac_record) * (size_t)c->nranks);
    return USAC_OK;
}

int usac_allgather_records(usac_ctx *c, const usac_record *local, usac_record *all) {
    if (!c || !local || !all) return USAC_ERR_ARG;
    if (!c->comm) return fail(c, USAC_ERR_ARG, "usac_comm_init not called");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->rec_send.p, local, sizeof(usac_record), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, order_after_exchanges(c));
    NCCL_TRY(c, ncclAllGather(c->rec_send.p, c->rec_all.p, sizeof(usac_record), ncclUint8, c->comm, c->stream));
    HIP_TRY(c, mark_collective(c));
    HIP_TRY(c, hipMemcpyAsync(all, c->rec_all.p, sizeof(usac_record) * (size_t)c->nranks, hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    return USAC_OK;
}

int usac_merge_records(const usac_record *recs, uint32_t n, usac_record *best) {
    if (!recs || !best || n == 0) return USAC_ERR_ARG;
    usac_record b = recs[0];
    for (uint32_t i = 1; i < n; i++)
        if (rec_better(recs[i], b)) b = recs[i];
    *best = b;
    return USAC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- stateful plugins (ABI 11)
// The reference's per-call plugin surface: handles that keep each plugin's state
// between calls, so a caller that keeps its own Ransac::run loop swaps plugin by plugin.  The
// state machines are usac_host.hpp's (the same ones ransac_run_impl replays with); every inlier
// test, least-squares fit and neighbour build runs on the context's device.

struct usac_random {
    usac::GlibcRandom g;
    explicit usac_random(uint32_t seed) : g(seed) {}
};

struct usac_sampler {
    usac_ctx *c = nullptr;
    int kind = USAC_SAMPLER_UNIFORM;
    uint32_t n = 0, m = 0;
    std::unique_ptr<usac::UniformSampler> uni;
    std::unique_ptr<usac::ProsacSampler> pro;
    std::shared_ptr<const usac::GridNeighbors> grid;
    std::unique_ptr<usac::NapsacSampler> nap;
    std::vector<int32_t> knn_tab;
    std::unique_ptr<usac::NapsacKnnSampler> napk;
    usac_termination *term = nullptr;  // the linked ProsacTerminationCriteria (PROSAC)
    uint64_t drawn = 0;
    std::vector<int32_t> last;  // generate_batch: the reference's reused sample array
};

struct usac_termination {
    usac_ctx *c = nullptr;
    float thr = 0.f;
    usac::StandardTerminationCriteria std_;
    std::unique_ptr<usac::ProsacTerminationCriteria> pro;
    usac_sampler *sampler = nullptr;
    std::vector<int32_t> inl;
    usac_termination(usac_ctx *ctx, const usac_params *p)
        : c(ctx), thr(p->threshold), std_(p->desired_prob, ctx->m, ctx->n, p->max_iterations) {}
};

struct usac_sprt {
    usac_ctx *c = nullptr;
    float thr = 0.f;
    uint32_t nw = 0;
    std::unique_ptr<usac::Sprt> s;
    DevBuf pool_idx, pool_pts, masks;
    std::vector<uint32_t> hmask;  // the current batch's words [nw][rows]
    uint32_t rows = 0;
    std::vector<int32_t> row_of;  // batch slot -> row (-1: empty slot)
    uint32_t batch_B = 0, batch_slots = 0;
    uint32_t rejected = 0;
    int max_before = 20;  // usac_params::max_hypothesis_test_before_sprt
    ~usac_sprt() {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        pool_idx.release();
        pool_pts.release();
        masks.release();
    }
};

struct usac_lo {
    usac_ctx *c = nullptr;
    std::unique_ptr<LoRansac> lo;
    std::unique_ptr<GcLo> gc;
    std::vector<int32_t> knn_tab;
    std::shared_ptr<const usac::GridNeighbors> grid;
};

namespace {

// host models (K x 9, line: first 3 of each row) into the context's device model layout (H: H
// and H^-1, [18][K]; F / E: [9][K]; line [3][K]), the layout the solve kernels leave
int upload_models(usac_ctx *c, const float *models, uint32_t K) {
    int rc = ensure_batch(c, K);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->hostmodels.p, models, sizeof(float) * 9 * (size_t)K, hipMemcpyHostToDevice,
                              c->stream));
    if (listed(c)) HIP_TRY(c, usac::launch_prepare_f(c->stream, c->hostmodels.as<float>(), K, c->models.as<float>()));
    else if (is_h(c)) HIP_TRY(c, usac::launch_prepare_h(c->stream, c->hostmodels.as<float>(), K, c->models.as<float>()));
    else HIP_TRY(c, usac::launch_prepare_line(c->stream, c->hostmodels.as<float>(), K, c->models.as<float>()));
    return USAC_OK;
}

// pool-order inlier words of K host models into s->hmask ([nw][K], row = model)
int sprt_masks(usac_sprt *s, const float *models, uint32_t K) {
    usac_ctx *c = s->c;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = upload_models(c, models, K);
    if (rc) return rc;
    HIP_TRY(c, s->masks.reserve(sizeof(uint32_t) * s->nw * (size_t)K));
    HIP_TRY(c, usac::launch_pool_mask(c->stream, c->estimator, s->pool_pts.p, c->n, c->models.as<float>(), K, nullptr,
                                      nullptr, K, s->thr, s->masks.as<uint32_t>(), K));
    s->hmask.resize((size_t)s->nw * K);
    HIP_TRY(c, hipMemcpyAsync(s->hmask.data(), s->masks.p, sizeof(uint32_t) * s->nw * (size_t)K, hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, stream_wait(c->stream));
    s->rows = K;
    return USAC_OK;
}

// the host walk of row r (sprt.hpp:191-317)
bool sprt_walk(usac_sprt *s, uint32_t r, int32_t current_hypothese, uint32_t maximum_score, int &count, float &score) {
    const bool good = s->s->verify(s->hmask.data() + r, current_hypothese, maximum_score, count, score, s->rows);
    if (!good) s->rejected++;
    return good;
}

}  // namespace

extern "C" {

int usac_random_create(uint32_t seed, usac_random **out) {
    if (!out) return USAC_ERR_ARG;
    *out = new usac_random(seed);
    return USAC_OK;
}

uint32_t usac_random_next(usac_random *rng) { return rng ? rng->g.next() : 0u; }

void usac_random_destroy(usac_random *rng) { delete rng; }

int usac_sampler_create(usac_ctx *c, const usac_params *p, usac_random *rng, usac_sampler **out) {
    if (!c || !p || !out) return USAC_ERR_ARG;
    *out = nullptr;
    const int kind = p->sampler == 0 ? USAC_SAMPLER_UNIFORM : p->sampler;
    if (kind != USAC_SAMPLER_UNIFORM && kind != USAC_SAMPLER_PROSAC && kind != USAC_SAMPLER_NAPSAC)
        return fail(c, USAC_ERR_UNSUPPORTED, "sampler: Uniform, Napsac or Prosac");
    if (kind != USAC_SAMPLER_PROSAC && !rng) return fail(c, USAC_ERR_ARG, "sampler: Uniform / NAPSAC draw from a usac_random");
    std::unique_ptr<usac_sampler> s(new usac_sampler());
    s->c = c;
    s->kind = kind;
    s->n = c->n;
    s->m = c->m;
    s->last.assign(c->m, 0);
    if (kind == USAC_SAMPLER_PROSAC) {
        if (c->n < c->m || c->m < 2) return fail(c, USAC_ERR_ARG, "PROSAC needs n >= sample size");
        s->pro.reset(new usac::ProsacSampler(p->seed, c->n, c->m));
    } else if (kind == USAC_SAMPLER_NAPSAC) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (p->neighbors == USAC_NEIGHBORS_GRID) {
            if (c->cols != 4) return fail(c, USAC_ERR_ARG, "NAPSAC grid neighbours need 4-column points (SURVEY Q17)");
            if (p->cell_size <= 0) return fail(c, USAC_ERR_ARG, "NAPSAC cell_size must be > 0");
            int rc = download_grid(c, p->cell_size, s->grid);
            if (rc) return rc;
            s->nap.reset(new usac::NapsacSampler(rng->g, *s->grid, c->n, c->m));
        } else {
            if (p->knn == 0 || p->knn > usac::kKnnMax || p->knn + 1 < c->m)
                return fail(c, USAC_ERR_ARG, "NAPSAC KNN: k_nearest_neighbors must be in [sample_size - 1, 32]");
            s->knn_tab.resize((size_t)c->n * p->knn);
            int rc = usac_knn(c, p->knn, s->knn_tab.data(), nullptr);
            if (rc) return rc;
            s->napk.reset(new usac::NapsacKnnSampler(rng->g, s->knn_tab.data(), c->n, c->m, p->knn));
        }
    } else {
        s->uni.reset(new usac::UniformSampler(rng->g, c->n, c->m));
    }
    *out = s.release();
    return USAC_OK;
}

int usac_sampler_generate(usac_sampler *s, int32_t *sample) {
    if (!s || !sample) return USAC_ERR_ARG;
    if (s->pro) {
        if (s->drawn >= usac::ProsacSampler::kGrowthMax)
            return fail(s->c, USAC_ERR_UNSUPPORTED, "PROSAC: more than T_N = 200000 samples (the reference then "
                                                    "draws outside the point range)");
        s->pro->generateSample(sample, s->term && s->term->pro ? s->term->pro->terminationLength() : s->n);
    } else if (s->nap) {
        s->nap->generateSample(sample);
    } else if (s->napk) {
        s->napk->generateSample(sample);
    } else {
        s->uni->generateSample(sample);
    }
    s->drawn++;
    return USAC_OK;
}

int usac_sampler_generate_batch(usac_sampler *s, uint32_t count, int32_t *samples) {
    if (!s || (!samples && count)) return USAC_ERR_ARG;
    for (uint32_t j = 0; j < count; j++) {
        int32_t *smp = samples + (size_t)j * s->m;
        memcpy(smp, s->last.data(), sizeof(int32_t) * s->m);
        int rc = usac_sampler_generate(s, smp);
        if (rc) return rc;
        memcpy(s->last.data(), smp, sizeof(int32_t) * s->m);
    }
    return USAC_OK;
}

int usac_sampler_state(const usac_sampler *s, uint64_t *drawn, uint32_t *subset_size, uint32_t *largest) {
    if (!s) return USAC_ERR_ARG;
    if (drawn) *drawn = s->drawn;
    if (subset_size) *subset_size = s->pro ? s->pro->subset() : s->n;
    if (largest) *largest = s->pro ? s->pro->largest() : s->n;
    return USAC_OK;
}

void usac_sampler_destroy(usac_sampler *s) {
    if (!s) return;
    if (s->term) s->term->sampler = nullptr;
    delete s;
}

int usac_termination_create(usac_ctx *c, const usac_params *p, usac_sampler *prosac, usac_termination **out) {
    if (!c || !p || !out) return USAC_ERR_ARG;
    *out = nullptr;
    if (prosac && (!prosac->pro || prosac->c != c))
        return fail(c, USAC_ERR_ARG, "termination: the linked sampler must be a PROSAC sampler of this context");
    if (prosac && prosac->term) return fail(c, USAC_ERR_ARG, "termination: the sampler is linked already");
    if (prosac && c->n <= 20)
        return fail(c, USAC_ERR_ARG, "PROSAC termination needs > 20 points (prosac_termination_criteria.hpp:158-163)");
    std::unique_ptr<usac_termination> t(new usac_termination(c, p));
    if (prosac) {
        t->pro.reset(new usac::ProsacTerminationCriteria(prosac->pro->growth(), p->desired_prob, c->m, c->n,
                                                         p->max_iterations));
        t->sampler = prosac;
        prosac->term = t.get();
        t->inl.resize(c->n);
    }
    *out = t.release();
    return USAC_OK;
}

uint32_t usac_termination_bound(const usac_termination *t, uint32_t inlier_size, uint32_t points_size) {
    if (!t) return 0;
    return t->std_.getUpBoundIterations(inlier_size, points_size ? points_size : t->c->n);
}

int usac_prosac_termination(usac_termination *t, uint32_t hyp_count, const float *model, uint32_t *max_iters,
                            uint32_t *termination_length) {
    if (!t || !model || !max_iters) return USAC_ERR_ARG;
    usac_ctx *c = t->c;
    if (!t->pro) return fail(c, USAC_ERR_ARG, "not a PROSAC termination criteria");
    if (!t->sampler) return fail(c, USAC_ERR_ARG, "PROSAC termination: its sampler was destroyed");
    uint32_t n = 0;
    int rc = usac_get_inliers(c, model, t->thr, t->inl.data(), &n, nullptr);
    if (rc) return rc;
    *max_iters = t->pro->getUpBoundIterationsSorted(hyp_count, t->inl.data(), n, t->sampler->pro->largest());
    if (termination_length) *termination_length = t->pro->terminationLength();
    return USAC_OK;
}

void usac_termination_destroy(usac_termination *t) {
    if (!t) return;
    if (t->sampler) t->sampler->term = nullptr;
    delete t;
}

int usac_sprt_create(usac_ctx *c, const usac_params *p, usac_random *rng, usac_sprt **out) {
    if (!c || !p || !rng || !out) return USAC_ERR_ARG;
    *out = nullptr;
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<usac_sprt> s(new usac_sprt());
    s->c = c;
    s->thr = p->threshold;
    s->nw = (c->n + 31) / 32;
    s->max_before = max_before_sprt(p);
    s->s.reset(new usac::Sprt(rng->g, c->estimator, c->n, c->m, p->max_iterations, s->max_before));
    HIP_TRY(c, s->pool_idx.reserve(sizeof(uint32_t) * c->n));
    HIP_TRY(c, s->pool_pts.reserve(sizeof(float) * c->cols * (size_t)c->n));
    HIP_TRY(c, hipMemcpyAsync(s->pool_idx.p, s->s->pool().data(), sizeof(uint32_t) * c->n, hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, usac::launch_gather_points(c->stream, c->pts.p, c->cols, s->pool_idx.as<uint32_t>(), c->n,
                                          s->pool_pts.p));
    HIP_TRY(c, stream_wait(c->stream));
    *out = s.release();
    return USAC_OK;
}

int usac_sprt_verify(usac_sprt *s, const float *model, int32_t current_hypothese, uint32_t maximum_score,
                     int32_t *good, int32_t *count, float *score) {
    if (!s || !model || !good || !count || !score) return USAC_ERR_ARG;
    float m9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    memcpy(m9, model, sizeof(float) * (size_t)ncomp(s->c));
    s->batch_B = 0;  // a batch replay's words are gone
    int rc = sprt_masks(s, m9, 1);
    if (rc) return rc;
    int cnt = *count;
    float sc = *score;
    *good = sprt_walk(s, 0, current_hypothese, maximum_score, cnt, sc) ? 1 : 0;
    *count = cnt;
    *score = sc;
    return USAC_OK;
}

uint32_t usac_sprt_upper_bound(const usac_sprt *s, uint32_t inlier_size) {
    return s ? s->s->getUpperBoundIterations((int)inlier_size) : 0u;
}

int usac_sprt_stats(const usac_sprt *s, uint32_t *histories, uint32_t *rejected) {
    if (!s) return USAC_ERR_ARG;
    if (histories) *histories = (uint32_t)s->s->histories();
    if (rejected) *rejected = s->rejected;
    return USAC_OK;
}

int usac_sprt_replay(usac_sprt *s, const float *models, const int32_t *n_models, uint32_t B, usac_sprt_state *st) {
    if (!s || !models || !n_models || !st) return USAC_ERR_ARG;
    usac_ctx *c = s->c;
    const uint32_t S = c->spk;
    if (st->sample > B || (st->sample < B && st->slot > S)) return fail(c, USAC_ERR_ARG, "sprt_replay: cursor out of range");
    st->found = 0;
    st->rejected = 0;
    if (st->sample == 0 && st->slot == 0) {  // a new batch: every model's pool-order inlier words
        std::vector<float> list;
        s->row_of.assign((size_t)B * S, -1);
        uint32_t K = 0;
        for (uint32_t b = 0; b < B; b++) {
            if (n_models[b] < 0 || (uint32_t)n_models[b] > S) return fail(c, USAC_ERR_ARG, "sprt_replay: n_models out of range");
            for (uint32_t q = 0; q < (uint32_t)n_models[b]; q++) {
                s->row_of[(size_t)b * S + q] = (int32_t)K++;
                list.insert(list.end(), models + ((size_t)b * S + q) * 9, models + ((size_t)b * S + q + 1) * 9);
            }
        }
        if (K) {
            int rc = sprt_masks(s, list.data(), K);
            if (rc) return rc;
        }
        s->batch_B = B;
    } else if (s->batch_B != B) {
        return fail(c, USAC_ERR_ARG, "sprt_replay: a batch resumes with the models it started with");
    }
    const uint32_t rej0 = s->rejected;
    uint32_t b = st->sample, q = st->slot;
    while (b < B) {
        if (q == 0 && st->iters >= st->max_iters) break;  // while (iters < max_iters)
        for (; q < (uint32_t)n_models[b]; q++) {
            int cnt = 0;
            float sc = 0.f;
            const bool good = sprt_walk(s, (uint32_t)s->row_of[(size_t)b * S + q], (int)st->iters,
                                        (uint32_t)st->best_inliers, cnt, sc);
            if (!good && (int)st->iters >= s->max_before) {  // max_hypothesis_test_before_sprt (model.hpp:40), Q9
                st->iters++;
                continue;
            }
            usac::Score cur, best;
            cur.inlier_number = cnt;
            cur.score = sc;
            best.inlier_number = st->best_inliers;
            best.score = st->best_score;
            if (cur.bigger(best)) {
                st->found = 1;
                st->inliers = cnt;
                st->score = sc;
                st->found_sample = b;
                st->found_slot = q;
                st->sample = b;
                st->slot = q + 1;
                st->rejected = s->rejected - rej0;
                return USAC_OK;
            }
        }
        st->iters++;
        b++;
        q = 0;
    }
    st->sample = b;
    st->slot = 0;
    st->rejected = s->rejected - rej0;
    return USAC_OK;
}

void usac_sprt_destroy(usac_sprt *s) { delete s; }

int usac_lo_create(usac_ctx *c, const usac_params *p, usac_lo **out) {
    if (!c || !p || !out) return USAC_ERR_ARG;
    *out = nullptr;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_single(c);
    if (rc) return rc;
    std::unique_ptr<usac_lo> h(new usac_lo());
    h->c = c;
    if (p->lo == USAC_LO_INITLORSC || p->lo == USAC_LO_INITFLORSC) {
        if (p->lo_sample_size == 0 || p->lo_iterative_iterations == 0)
            return fail(c, USAC_ERR_ARG, "LO parameters must be > 0");
        h->lo.reset(new LoRansac(c, p, Shard()));
        if ((rc = h->lo->reserve())) return rc;
    } else if (p->lo == USAC_LO_GC) {
        const bool knn = p->neighbors != USAC_NEIGHBORS_GRID;
        if (knn) {
            if (p->knn == 0 || p->knn > usac::kKnnMax) return fail(c, USAC_ERR_ARG, "GC KNN: k_nearest_neighbors must be in [1, 32]");
            h->knn_tab.resize((size_t)c->n * p->knn);
            if ((rc = usac_knn(c, p->knn, h->knn_tab.data(), nullptr))) return rc;
        } else {
            if (c->cols != 4 || p->cell_size <= 0)
                return fail(c, USAC_ERR_ARG, "GC grid neighbours need 4-column points and cell_size > 0");
            if ((rc = download_grid(c, p->cell_size, h->grid))) return rc;
        }
        h->gc.reset(new GcLo(c, p, knn ? h->knn_tab.data() : nullptr, p->knn, h->grid.get()));
        if ((rc = h->gc->reserve())) return rc;
    } else {
        return fail(c, USAC_ERR_UNSUPPORTED, "LO: InItLORsc / InItFLORsc / GC only");
    }
    *out = h.release();
    return USAC_OK;
}

int usac_lo_get_model_score(usac_lo *h, float *model, int32_t *inliers, float *score) {
    if (!h || !model || !inliers || !score) return USAC_ERR_ARG;
    HIP_TRY(h->c, hipSetDevice(h->c->device));
    int cnt = *inliers;
    float sum = *score;
    if (h->lo) {
        h->lo->run(model, cnt, sum);
        if (h->lo->rc) return h->lo->rc;
    } else {
        h->gc->run(model, cnt, sum);
        if (h->gc->rc) return h->gc->rc;
    }
    *inliers = cnt;
    *score = sum;
    return USAC_OK;
}

int usac_lo_iters(const usac_lo *h, uint32_t *inner, uint32_t *iterative) {
    if (!h) return USAC_ERR_ARG;
    if (inner) *inner = h->lo ? h->lo->inner_count : h->gc->gc_iters;
    if (iterative) *iterative = h->lo ? h->lo->iterative_count : h->gc->labelings;
    return USAC_OK;
}

void usac_lo_destroy(usac_lo *h) {
    if (!h) return;
    (void)hipSetDevice(h->c->device);
    (void)hipStreamSynchronize(h->c->stream);
    delete h;
}

}  // extern "C"

// ---------------------------------------------------------------- multi-problem batches (ABI 15 .. 20)
// P independent two-view problems in one context (kernels_multi.hip): the usac_hypothesize_score
// round over (active problem, hypothesis tile), and a batch-granular RANSAC whose host loop only
// reads the active problems' records once per round, evaluates the standard termination criterion
// and uploads the compacted active list.  One stream; every buffer is sized once per call, for
// (active problems) x R, none inside the round loop.  There is one such loop, multi_run_driver, with
// four options read from the params; usac_multi_run, _run_polished, _run_prosac, _run_lo, _run_sprt and
// _run_napsac check their arguments and call it:
//   PROSAC (ABI 17): the PROSAC sampler in closed form (usac_prosac.hpp) and PROSAC's termination scan,
//     split between k_multi_prosac_scan, which stores its candidates into pinned host memory, and
//     ProsacTerminationCriteria::applyCandidates;
//   LO (ABI 18): k_multi_lo (kernels_nonmin.hip) between the round's merge and the scan / the record copy;
//     on an essential context through usac_multi_run_lo_essential alone (ABI 23);
//   SPRT (ABI 19): the round's score launch replaced by SPRT verification (kernels_multi_sprt.hip), one
//     test per problem and round, re-designed on the host between rounds (usac::SprtRounds) from the
//     statistics that come down with the records.  LO and SPRT do not combine;
//   NAPSAC (ABI 20): the solve kernels' NAPSAC instantiation over the problems' grid neighbours, built for
//     all problems in one launch (kernels_multi_grid.hip) and kept for the cell size; the standard
//     termination criterion; with LO, not with SPRT.

struct usac_multi {
    int device = 0;
    int estimator = 0;
    uint32_t P = 0, m = 0, spk = 1, n_total = 0;
    hipStream_t stream = nullptr;
    std::vector<uint32_t> offsets;  // host copy, P + 1
    DevBuf pts, offs, items, samples, models, counts, sums, list, list_n, out, running, mmodels, m18, mask;
    DevBuf pol_lists, pol_out;  // the polish: two inlier lists per problem (2 x N_total), P results
    DevBuf lo_state;            // LO (ABI 18): per problem the threshold, the draw counter, the counters
    bool lo_state_set = false;  // usac_multi_lo: the state of an earlier call is there to continue
    PinBlock pin;               // pinned staging: the active list up, the records down
    PinBlock pol_pin;           // pinned staging of the polish: P results and the mask down
    // PROSAC (built at the first PROSAC call): the problems' growth functions and pristine non-random
    // minima (N_total values each, the points' offsets), the working copy the scan kernel raises, the
    // pinned block it stores candidates and their numbers into, and the per-problem host halves
    DevBuf growth, non_random0, non_random;
    std::vector<std::shared_ptr<const std::vector<uint32_t>>> growth_host;  // per problem, shared by shape
    PinBlock pro_pin;  // (N_total / 2 + P) candidate pairs, then P numbers
    std::vector<std::unique_ptr<usac::ProsacTerminationCriteria>> pterm;
    // SPRT (ABI 19): the pool-ordered copy of the points and its index (usac_multi_sprt_setup), per
    // launch the active entries' tests (their statistics sit behind the records in `out`), the survivor
    // list and its counter, the slots' starts (the hook only); pinned staging of the tests up and of
    // the records and statistics down
    DevBuf sprt_pts, sprt_idx, sprt_consts, sprt_surv, sprt_surv_n, sprt_starts;
    bool sprt_ready = false, sprt_tail = false;
    PinBlock sprt_pin;
    // NAPSAC (ABI 20): the problems' grid neighbours for cell size grid_cs (0 = none), one block in
    // usac::MultiGrid's layout (multi_grid_args), and the host copy of [status | n_cells | n_eligible]
    DevBuf grid;
    int grid_cs = 0;
    std::vector<uint32_t> grid_counts;  // 3 P
    // Essential (ABI 21): the 5-point pipeline's workspace and the cap on a solve slice's samples
    // (kMultiE5Slice, lowered by USAC_MULTI_E5_SLICE at creation)
    DevBuf e5_ws;
    uint32_t e5_slice = usac::kMultiE5Slice;
    // Per-problem thresholds (ABI 22): empty = none, every call uses its scalar; else P values, their
    // device copy, and per LO call the iterative steps (θ_p mult - θ_p) / iterations of the call's params
    std::vector<float> thr_host;
    DevBuf thrs, lo_steps;
    uint32_t lo_steps_mult = 0, lo_steps_iters = 0;  // what lo_steps was computed for (iters 0: nothing)
    // Pixel coordinates (ABI 24): a context created from pixels keeps its problems' intrinsics (P x 9 each; k2 =
    // k1 where the caller gave one K) for the pixel thresholds and the pixel-space models; else both are empty
    std::vector<float> k1, k2;
    // Device input (ABI 25): a context from usac_multi_create_device keeps the padded width of its input and, per
    // packed row, the column it came from (N_total values on the device); else n_max is 0 and src is empty
    uint32_t n_max = 0;
    DevBuf src;
    // Device output (ABI 27): resident_valid says that pol_out and mask hold the complete result of the last
    // polishing call; resident_end names what ended that otherwise (nullptr: no polishing call has run).
    // resident_on: polishing calls compute the device mask without a host mask (usac_multi_set_resident).
    // kdev: the intrinsics of a context that has them, P x 9 of view 1 then of view 2, at the first export
    bool resident_on = false, resident_valid = false;
    const char *resident_end = nullptr;
    DevBuf kdev;
    // Pose (ABI 28): usac_multi_pose's own block -- the caller's models and mask up, the outputs down
    DevBuf pose_buf;
    // Pose refinement (ABI 29): usac_multi_refine_pose's own block -- the caller's poses and mask up, the outputs down
    DevBuf refine_buf;
    std::string err;
};

namespace {

int fail(usac_multi *mc, int code, const std::string &msg) {
    if (mc) mc->err = msg;
    return code;
}

// the resident result (ABI 27) ends: by, the call that wrote over it or left it incomplete
void multi_resident_end(usac_multi *mc, const char *by) {
    mc->resident_valid = false;
    mc->resident_end = by;
}

bool multi_round_ok(uint32_t R) { return R >= 64 && R <= 8192 && R % 64 == 0; }

bool multi_is_e(const usac_multi *mc) { return mc->estimator == USAC_ESSENTIAL; }

// what an essential context does not offer: refused before any device call
int multi_no_essential(usac_multi *mc, const char *who) {
    if (!multi_is_e(mc)) return USAC_OK;
    return fail(mc, USAC_ERR_UNSUPPORTED, std::string(who) + ": not for the essential estimator (multi-problem batches "
                                                              "of essential matrices have no SPRT or NAPSAC, and LO through "
                                                              "usac_multi_lo_essential / usac_multi_run_lo_essential)");
}

// the entries of an essential context alone (ABI 23): `other` is the H / F entry with the same contract
int multi_only_essential(usac_multi *mc, const char *who, const char *other) {
    if (multi_is_e(mc)) return USAC_OK;
    return fail(mc, USAC_ERR_UNSUPPORTED, std::string(who) + ": for the essential estimator only (homography and "
                                                              "fundamental contexts: " + other + ")");
}

// device buffers and pinned staging for a round of A active problems x R hypotheses
int multi_ensure(usac_multi *mc, uint32_t A, uint32_t R, bool host_samples) {
    const size_t G = (size_t)A * R, S = G * mc->spk;
    HIP_TRY(mc, mc->items.reserve(sizeof(usac::MultiItem) * (size_t)A));
    if (host_samples) HIP_TRY(mc, mc->samples.reserve(sizeof(int32_t) * G * mc->m));
    HIP_TRY(mc, mc->models.reserve(sizeof(float) * S * (mc->estimator == USAC_HOMOGRAPHY ? 18 : 9)));
    HIP_TRY(mc, mc->counts.reserve(sizeof(int32_t) * S));
    HIP_TRY(mc, mc->sums.reserve(sizeof(float) * S));
    HIP_TRY(mc, mc->out.reserve(sizeof(usac_record) * (size_t)A));
    if (mc->estimator != USAC_HOMOGRAPHY) {
        HIP_TRY(mc, mc->list.reserve(sizeof(uint32_t) * S));
        HIP_TRY(mc, mc->list_n.reserve(sizeof(uint32_t) * (size_t)A));
    }
    if (multi_is_e(mc))
        HIP_TRY(mc, mc->e5_ws.reserve(usac::multi_e5_workspace_bytes(A, R, usac::multi_e5_slice_samples(mc->e5_slice, R))));
    if (!pin_grow(mc->pin, (sizeof(usac::MultiItem) + sizeof(usac_record)) * (size_t)A))
        return fail(mc, USAC_ERR_HIP, "hipHostMalloc failed");
    return USAC_OK;
}

usac::MultiItem *multi_items_pin(usac_multi *mc) { return static_cast<usac::MultiItem *>(mc->pin.p); }
usac_record *multi_records_pin(usac_multi *mc, uint32_t A_cap) {
    return reinterpret_cast<usac_record *>(multi_items_pin(mc) + A_cap);
}

// the device thresholds of a context that has them set (else null: the call's scalar), and problem p's on the host
const float *multi_thrs(const usac_multi *mc) { return mc->thr_host.empty() ? nullptr : mc->thrs.as<float>(); }
float multi_thr_of(const usac_multi *mc, uint32_t p, float scalar) { return mc->thr_host.empty() ? scalar : mc->thr_host[p]; }

usac::MultiRound multi_round(usac_multi *mc, uint32_t A, uint32_t R, uint64_t first_hyp, float thr, int dlt_mode) {
    usac::MultiRound r{};
    r.estimator = mc->estimator;
    r.nullspace = dlt_mode == USAC_DLT_NULLSPACE;
    r.pts = mc->pts.as<float4>();
    r.offsets = mc->offs.as<uint32_t>();
    r.items = mc->items.as<usac::MultiItem>();
    r.A = A;
    r.R = R;
    r.first_hyp = first_hyp;
    r.thr = thr;
    r.thrs = multi_thrs(mc);
    r.models = mc->models.as<float>();
    r.counts = mc->counts.as<int32_t>();
    r.sums = mc->sums.as<float>();
    r.list = mc->list.as<uint32_t>();
    r.list_n = mc->list_n.as<uint32_t>();
    r.out = mc->out.as<usac_record>();
    r.e5_ws = mc->e5_ws.p;
    r.e5_slice = usac::multi_e5_slice_samples(mc->e5_slice, R);
    return r;
}

// The polish of one problem past k_multi_polish's caps: the loop of ransac.cpp:157-214 over
// usac_get_inliers / usac_nonminimal of a temporary single context on the problem's points (the
// multi-launch kernels, any n and any list size; the same bits as the fused workgroup where both
// apply).  mask_p (nullable): the problem's n_p mask bytes.
int multi_polish_single(usac_multi *mc, uint32_t p, const float *start, float thr, usac_multi_polish_output *o,
                        uint8_t *mask_p) {
    const uint32_t base = mc->offsets[p], n = mc->offsets[p + 1] - base;
    std::vector<float> pts(4 * (size_t)n);
    HIP_TRY(mc, hipMemcpy(pts.data(), mc->pts.as<float>() + 4 * (size_t)base, sizeof(float) * 4 * (size_t)n,
                          hipMemcpyDeviceToHost));
    usac_ctx *c = nullptr;
    int rc = usac_create(&c, mc->device, mc->estimator, pts.data(), n, 4);
    if (rc) return fail(mc, rc, "usac_multi_polish: no single context for a problem past the fused caps");
    std::vector<int32_t> cur(n), nxt(n);
    uint32_t c0 = 0, cnt = 0;
    float s0 = 0.f, s = 0.f;
    auto done = [&](int code, const char *what) {
        if (code) fail(mc, code, std::string("usac_multi_polish: ") + what + ": " + usac_last_error(c));
        usac_destroy(c);
        return code;
    };
    if ((rc = usac_get_inliers(c, start, thr, cur.data(), &c0, &s0))) return done(rc, "get_inliers");
    *o = usac_multi_polish_output{};
    memcpy(o->model, start, sizeof(o->model));
    o->inliers = o->minimal_inliers = (int32_t)c0;
    o->score = o->minimal_score = s0;
    o->status = c0 > 0 ? USAC_OK : USAC_ERR_NO_MODEL;
    int32_t prev = 0;
    for (int k = 0; k < 4 && c0 > 0; k++) {
        float nm[9];
        rc = usac_nonminimal(c, cur.data(), (uint32_t)o->inliers, nm);
        if (rc == USAC_ERR_NO_MODEL) break;
        if (rc) return done(rc, "nonminimal");
        if ((rc = usac_get_inliers(c, nm, thr, nxt.data(), &cnt, &s))) return done(rc, "get_inliers");
        if ((double)((float)(int32_t)cnt / (float)o->inliers) < 0.8 || (int32_t)cnt <= prev) break;
        prev = o->inliers = (int32_t)cnt;
        o->score = s;
        memcpy(o->model, nm, sizeof(nm));
        o->passes++;
        cur.swap(nxt);
    }
    if (mask_p) {
        memset(mask_p, 0, n);
        for (int32_t i = 0; i < o->inliers; i++) mask_p[cur[i]] = 1;
    }
    return done(USAC_OK, "");
}

// usac_multi_polish on start models already on the device (dmodels + p * stride floats); hstart:
// the same models on the host (+ p * hstride floats), read only for the problems the kernel defers
int multi_polish_device(usac_multi *mc, const float *dmodels, uint32_t stride, const float *hstart, size_t hstride,
                        float thr, usac_multi_polish_output *out, uint8_t *mask) {
    const uint32_t P = mc->P;
    // the device mask: for the caller's host mask, or (resident mode, ABI 27) to stay where it is
    const bool dmask = mask || mc->resident_on;
    multi_resident_end(mc, "a polishing call that failed");  // until this one has finished
    HIP_TRY(mc, mc->pol_lists.reserve(sizeof(int32_t) * 2 * (size_t)mc->n_total));
    HIP_TRY(mc, mc->pol_out.reserve(sizeof(usac_multi_polish_output) * (size_t)P));
    if (dmask) HIP_TRY(mc, mc->mask.reserve(mc->n_total));
    HIP_TRY(mc, usac::launch_multi_polish(mc->stream, mc->estimator, mc->pts.as<float4>(), mc->offs.as<uint32_t>(), P,
                                          mc->n_total, dmodels, stride, thr, multi_thrs(mc), mc->pol_lists.as<int32_t>(),
                                          mc->pol_out.as<usac_multi_polish_output>(),
                                          dmask ? mc->mask.as<uint8_t>() : nullptr));
    // results and mask come down through pinned staging, then into the caller's (pageable) buffers
    const size_t out_bytes = sizeof(usac_multi_polish_output) * (size_t)P, need = out_bytes + (mask ? mc->n_total : 0);
    if (!pin_grow(mc->pol_pin, need)) return fail(mc, USAC_ERR_HIP, "hipHostMalloc failed");
    uint8_t *stage = static_cast<uint8_t *>(mc->pol_pin.p);
    HIP_TRY(mc, hipMemcpyAsync(stage, mc->pol_out.p, out_bytes, hipMemcpyDeviceToHost, mc->stream));
    if (mask) HIP_TRY(mc, hipMemcpyAsync(stage + out_bytes, mc->mask.p, mc->n_total, hipMemcpyDeviceToHost, mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    memcpy(out, stage, out_bytes);
    if (mask) memcpy(mask, stage + out_bytes, mc->n_total);
    std::vector<uint8_t> tmp;  // resident mode without a host mask: a deferred problem's mask bytes
    for (uint32_t p = 0; p < P; p++) {
        if (out[p].status != usac::kMultiPolishDefer) continue;
        const uint32_t base = mc->offsets[p], n = mc->offsets[p + 1] - base;
        uint8_t *mask_p = mask ? mask + base : nullptr;
        if (!mask && dmask) {
            tmp.resize(n);
            mask_p = tmp.data();
        }
        const int rc = multi_polish_single(mc, p, hstart + (size_t)p * hstride, multi_thr_of(mc, p, thr), out + p, mask_p);
        if (rc) return rc;
        if (!dmask) continue;
        // the resident result is complete (ABI 27): what the host path computed goes back to the device
        HIP_TRY(mc, hipMemcpy(mc->pol_out.as<usac_multi_polish_output>() + p, out + p, sizeof(usac_multi_polish_output),
                              hipMemcpyHostToDevice));
        HIP_TRY(mc, hipMemcpy(mc->mask.as<uint8_t>() + base, mask_p, n, hipMemcpyHostToDevice));
    }
    if (dmask) mc->resident_valid = true;
    else multi_resident_end(mc, "a polishing call that computed no mask (a NULL mask with resident mode off)");
    return USAC_OK;
}

// ---- PROSAC for multi-problem batches (ABI 17)
uint32_t *multi_cand_pin(usac_multi *mc) { return static_cast<uint32_t *>(mc->pro_pin.p); }
uint32_t *multi_cand_n_pin(usac_multi *mc) {
    return multi_cand_pin(mc) + 2 * usac::multi_cand_capacity(mc->n_total, mc->P);
}

// once per context: the device growth functions and non-random minima, the pinned candidate block
int multi_prosac_ensure(usac_multi *mc) {
    if (!mc->growth_host.empty()) return USAC_OK;
    const size_t bytes = sizeof(uint32_t) * (size_t)mc->n_total;
    std::vector<uint32_t> g(mc->n_total), nr(mc->n_total);
    std::vector<std::shared_ptr<const std::vector<uint32_t>>> tabs(mc->P);
    for (uint32_t p = 0; p < mc->P; p++) {
        const uint32_t base = mc->offsets[p], n = mc->offsets[p + 1] - base;
        tabs[p] = usac::ProsacSampler::growth_table(n, mc->m);
        std::copy(tabs[p]->begin(), tabs[p]->end(), g.begin() + base);
        const std::vector<uint32_t> t = usac::ProsacTerminationCriteria::table(n, mc->m);
        std::copy(t.begin(), t.end(), nr.begin() + base);
    }
    HIP_TRY(mc, mc->growth.reserve(bytes));
    HIP_TRY(mc, mc->non_random0.reserve(bytes));
    HIP_TRY(mc, mc->non_random.reserve(bytes));
    HIP_TRY(mc, hipMemcpy(mc->growth.p, g.data(), bytes, hipMemcpyHostToDevice));
    HIP_TRY(mc, hipMemcpy(mc->non_random0.p, nr.data(), bytes, hipMemcpyHostToDevice));
    if (!pin_grow(mc->pro_pin, sizeof(uint32_t) * (2 * usac::multi_cand_capacity(mc->n_total, mc->P) + mc->P)))
        return fail(mc, USAC_ERR_HIP, "hipHostMalloc failed");
    mc->growth_host.swap(tabs);
    return USAC_OK;
}

// the start of a run: every problem's termination state fresh, the device minima pristine
int multi_prosac_reset(usac_multi *mc, const usac_params *prm) {
    mc->pterm.resize(mc->P);
    for (uint32_t p = 0; p < mc->P; p++)
        mc->pterm[p].reset(new usac::ProsacTerminationCriteria(usac::ProsacTerminationCriteria::CandidatesOnly{},
                                                               *mc->growth_host[p], prm->desired_prob, mc->m,
                                                               mc->offsets[p + 1] - mc->offsets[p],
                                                               prm->max_iterations));
    HIP_TRY(mc, hipMemcpyAsync(mc->non_random.p, mc->non_random0.p, sizeof(uint32_t) * (size_t)mc->n_total,
                               hipMemcpyDeviceToDevice, mc->stream));
    return USAC_OK;
}

hipError_t multi_launch_scan(usac_multi *mc, uint32_t A, uint64_t first_hyp, float thr) {
    return usac::launch_multi_prosac_scan(mc->stream, mc->estimator, mc->pts.as<float4>(), mc->offs.as<uint32_t>(),
                                          mc->items.as<usac::MultiItem>(), A, mc->running.as<usac_record>(),
                                          first_hyp, thr, multi_thrs(mc), mc->non_random.as<uint32_t>(), multi_cand_pin(mc),
                                          multi_cand_n_pin(mc));
}

// the host half of problem p's scan: the candidates active entry a's workgroup left
uint32_t multi_apply_candidates(usac_multi *mc, uint32_t a, uint32_t p, uint32_t hyp_count, uint32_t largest) {
    const uint32_t *cand = multi_cand_pin(mc) + 2 * usac::multi_cand_offset(mc->offsets[p], p);
    return mc->pterm[p]->applyCandidates(hyp_count, largest, cand, multi_cand_n_pin(mc)[a]);
}

// ---- LO-RANSAC for multi-problem batches (ABI 18)
// the checks of usac_multi_lo / usac_multi_run_lo that precede any device call
int multi_lo_check(usac_multi *mc, const usac_params *prm, const char *who) {
    if (prm->lo == USAC_LO_GC || prm->sprt)
        return fail(mc, USAC_ERR_UNSUPPORTED, std::string(who) + ": no graph-cut LO, no SPRT");
    if (prm->lo != USAC_LO_INITLORSC && prm->lo != USAC_LO_INITFLORSC)
        return fail(mc, USAC_ERR_ARG, std::string(who) + ": params->lo must be USAC_LO_INITLORSC or USAC_LO_INITFLORSC");
    if (prm->lo_sample_size == 0 || prm->lo_sample_size > usac::kLoDrawMax)
        return fail(mc, USAC_ERR_ARG, std::string(who) + ": lo_sample_size in 1..64");
    if (prm->lo_iterative_iterations == 0) return fail(mc, USAC_ERR_ARG, std::string(who) + ": lo_iterative_iterations >= 1");
    return USAC_OK;
}

// the LO buffers, and at the start of a run (reset) every problem's state fresh: threshold θ, counters 0
int multi_lo_ensure(usac_multi *mc, const usac_params *prm, bool reset) {
    const uint32_t P = mc->P;
    HIP_TRY(mc, mc->pol_lists.reserve(sizeof(int32_t) * 2 * (size_t)mc->n_total));
    HIP_TRY(mc, mc->lo_state.reserve(sizeof(usac_multi_lo_output) * (size_t)P));
    if (reset || !mc->lo_state_set) {
        std::vector<usac_multi_lo_output> init(P, usac_multi_lo_output{});
        for (uint32_t p = 0; p < P; p++) init[p].threshold = multi_thr_of(mc, p, prm->threshold);
        HIP_TRY(mc, hipMemcpy(mc->lo_state.p, init.data(), sizeof(usac_multi_lo_output) * (size_t)P, hipMemcpyHostToDevice));
        mc->lo_state_set = true;
    }
    // the call's iterative steps: multi_lo_args' expression with θ_p for θ; uploaded when the thresholds or
    // the two parameters they depend on changed
    if (!mc->thr_host.empty() && (mc->lo_steps_mult != prm->lo_threshold_multiplier ||
                                  mc->lo_steps_iters != prm->lo_iterative_iterations)) {
        std::vector<float> steps(P);
        for (uint32_t p = 0; p < P; p++) {
            const float t = mc->thr_host[p];
            steps[p] = (t * prm->lo_threshold_multiplier - t) / prm->lo_iterative_iterations;
        }
        HIP_TRY(mc, mc->lo_steps.reserve(sizeof(float) * (size_t)P));
        HIP_TRY(mc, hipMemcpy(mc->lo_steps.p, steps.data(), sizeof(float) * (size_t)P, hipMemcpyHostToDevice));
        mc->lo_steps_mult = prm->lo_threshold_multiplier;
        mc->lo_steps_iters = prm->lo_iterative_iterations;
    }
    return USAC_OK;
}

// threshold arithmetic as LoRansac's (above): the same fp32 expressions
usac::MultiLo multi_lo_args(usac_multi *mc, const usac_params *prm, uint64_t first_hyp, bool force) {
    usac::MultiLo lo{};
    lo.items = mc->items.as<usac::MultiItem>();
    lo.running = mc->running.as<usac_record>();
    lo.out = mc->out.as<usac_record>();
    lo.first_hyp = first_hyp;
    lo.force = force ? 1 : 0;
    lo.limited = prm->lo == USAC_LO_INITFLORSC ? 1 : 0;
    lo.thr = prm->threshold;
    lo.mult = (float)prm->lo_threshold_multiplier;
    lo.step = (prm->threshold * prm->lo_threshold_multiplier - prm->threshold) / prm->lo_iterative_iterations;
    lo.thrs = multi_thrs(mc);
    lo.steps = lo.thrs ? mc->lo_steps.as<float>() : nullptr;  // uploaded by multi_lo_ensure
    lo.inner = prm->lo_inner_iterations;
    lo.iters = prm->lo_iterative_iterations;
    lo.limit = prm->lo_sample_size;
    lo.lists = mc->pol_lists.as<int32_t>();
    lo.n_total = mc->n_total;
    lo.state = mc->lo_state.as<usac_multi_lo_output>();
    return lo;
}

int multi_lo_fetch(usac_multi *mc, usac_multi_lo_output *lo) {
    if (lo) HIP_TRY(mc, hipMemcpy(lo, mc->lo_state.p, sizeof(usac_multi_lo_output) * (size_t)mc->P, hipMemcpyDeviceToHost));
    return USAC_OK;
}

// usac_multi_lo / usac_multi_lo_essential after their own checks: one LO call on recs, every record a new best
int multi_lo_hook(usac_multi *mc, const usac_params *prm, int reset, const uint64_t *seeds, usac_record *recs,
                  usac_multi_lo_output *lo, const char *who) {
    int rc = multi_lo_check(mc, prm, who);
    if (rc) return rc;
    const uint32_t P = mc->P;
    HIP_TRY(mc, hipSetDevice(mc->device));
    if ((rc = multi_ensure(mc, P, 64, false)) || (rc = multi_lo_ensure(mc, prm, reset != 0))) return rc;
    usac::MultiItem *items = multi_items_pin(mc);
    for (uint32_t p = 0; p < P; p++) items[p] = usac::MultiItem{p, 0u, seeds ? seeds[p] : (uint64_t)prm->seed + p, 0u, 0u};
    HIP_TRY(mc, hipMemcpyAsync(mc->items.p, items, sizeof(usac::MultiItem) * (size_t)P, hipMemcpyHostToDevice, mc->stream));
    HIP_TRY(mc, hipMemcpyAsync(mc->running.p, recs, sizeof(usac_record) * (size_t)P, hipMemcpyHostToDevice, mc->stream));
    HIP_TRY(mc, usac::launch_multi_lo(mc->stream, mc->estimator, mc->pts.as<float4>(), mc->offs.as<uint32_t>(), P,
                                      multi_lo_args(mc, prm, 0, true)));
    HIP_TRY(mc, hipMemcpyAsync(recs, mc->running.p, sizeof(usac_record) * (size_t)P, hipMemcpyDeviceToHost, mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    return multi_lo_fetch(mc, lo);
}

// ---- SPRT for multi-problem batches (ABI 19)
// the certificate's margin and climb limit with their test overrides, as usac_set_sprt reads them
bool multi_sprt_cert(double &margin, double &climb) {
    const char *em = getenv("USAC_SPRT_CERT_MARGIN"), *ec = getenv("USAC_SPRT_CERT_CLIMB");
    margin = em ? atof(em) : 1e-7;
    climb = ec ? atof(ec) : 700.0;
    return margin >= 1e-7 && climb > 0 && climb <= 700.0;
}

// usac_set_sprt's constants of the test (eps, del, A) for a problem of n points: the reference's doubles,
// their logs, and the certificate's margin raised to its error budget at this n
usac::SprtConsts multi_sprt_consts(double eps, double del, double A, uint32_t n, double margin, double climb) {
    usac::SprtConsts k{};
    k.up = del / eps;
    k.down = (1 - del) / (1 - eps);
    k.A = A;
    k.lu = log(k.up);
    k.ld = log(k.down);
    k.lA = log(k.A);
    k.margin = margin;
    k.climb = climb;
    const double L = std::max(std::max(fabs(k.lu), fabs(k.ld)), 1.0);
    const double nn = (double)n, per = std::ceil(std::max(nn - 64.0, 0.0) / 256.0) + 64.0;
    const double budget = 2.0 * nn * L * 0x1p-51 + per * per * L * 0x1p-53 + fabs(k.lA) * 0x1p-53;
    k.margin = std::max(k.margin, 8.0 * budget);
    return k;
}

// the pools on the host, the pool-ordered copy of the points on the device (k_gather's rule)
int multi_sprt_setup(usac_multi *mc, const uint32_t *pool_seeds) {
    std::vector<uint32_t> idx(mc->n_total);
    bool tail = false;
    for (uint32_t p = 0; p < mc->P; p++) {
        const uint32_t base = mc->offsets[p], n = mc->offsets[p + 1] - base;
        usac::GlibcRandom g(pool_seeds ? pool_seeds[p] : p + 1);
        const usac::Sprt sp(g, mc->estimator, n, mc->m, 10000);
        const std::vector<uint32_t> &pool = sp.pool();
        for (uint32_t i = 0; i < n; i++) idx[base + i] = base + pool[i];
        tail = tail || n > 64;
    }
    mc->sprt_ready = false;
    HIP_TRY(mc, mc->sprt_idx.reserve(sizeof(uint32_t) * (size_t)mc->n_total));
    HIP_TRY(mc, mc->sprt_pts.reserve(sizeof(float) * 4 * (size_t)mc->n_total));
    HIP_TRY(mc, mc->sprt_surv_n.reserve(sizeof(uint32_t)));
    HIP_TRY(mc, hipMemcpyAsync(mc->sprt_idx.p, idx.data(), sizeof(uint32_t) * (size_t)mc->n_total, hipMemcpyHostToDevice,
                               mc->stream));
    HIP_TRY(mc, usac::launch_gather_points(mc->stream, mc->pts.p, 4, mc->sprt_idx.as<uint32_t>(), mc->n_total,
                                           mc->sprt_pts.p));
    HIP_TRY(mc, stream_wait(mc->stream));
    mc->sprt_ready = true;
    mc->sprt_tail = tail;
    return USAC_OK;
}

// The SPRT buffers of a launch of up to A entries x R hypotheses (after multi_ensure): the tests, the
// survivor list, the starts if asked for; the statistics sit behind the records in mc->out, so that both
// come down in one copy; pinned staging: A tests up, then A records and A statistics down.
int multi_sprt_ensure(usac_multi *mc, uint32_t A, uint32_t R, bool starts) {
    if (!mc->sprt_ready) {
        const int rc = multi_sprt_setup(mc, nullptr);
        if (rc) return rc;
    }
    const size_t S = (size_t)A * R * mc->spk;
    HIP_TRY(mc, mc->sprt_consts.reserve(sizeof(usac::SprtConsts) * (size_t)A));
    HIP_TRY(mc, mc->out.reserve((sizeof(usac_record) + sizeof(usac_multi_sprt_stats)) * (size_t)A));
    HIP_TRY(mc, mc->sprt_surv.reserve(usac::multi_sprt_survivor_bytes() * S));
    if (starts) HIP_TRY(mc, mc->sprt_starts.reserve(sizeof(uint32_t) * S));
    if (!pin_grow(mc->sprt_pin,
                  (sizeof(usac::SprtConsts) + sizeof(usac_record) + sizeof(usac_multi_sprt_stats)) * (size_t)A))
        return fail(mc, USAC_ERR_HIP, "hipHostMalloc failed");
    return USAC_OK;
}
static_assert(sizeof(usac_record) % 8 == 0 && sizeof(usac::SprtConsts) % 8 == 0 && sizeof(usac_multi_sprt_stats) == 32,
              "the records, then the statistics, 8-byte aligned");

usac::SprtConsts *multi_sprt_consts_pin(usac_multi *mc) { return static_cast<usac::SprtConsts *>(mc->sprt_pin.p); }
// the down area behind A_cap tests: the launch's A records, then its A statistics
usac_record *multi_sprt_down_pin(usac_multi *mc, uint32_t A_cap) {
    return reinterpret_cast<usac_record *>(multi_sprt_consts_pin(mc) + A_cap);
}

// a launch of A entries: the device statistics behind the A records of mc->out
usac::MultiSprt multi_sprt_args(usac_multi *mc, uint32_t A, bool starts) {
    usac::MultiSprt s{};
    s.pool_pts = mc->sprt_pts.as<float4>();
    s.consts = mc->sprt_consts.as<usac::SprtConsts>();
    s.stats = reinterpret_cast<usac_multi_sprt_stats *>(mc->out.as<usac_record>() + A);
    s.surv = mc->sprt_surv.p;
    s.surv_n = mc->sprt_surv_n.as<uint32_t>();
    s.starts = starts ? mc->sprt_starts.as<uint32_t>() : nullptr;
    s.tail = mc->sprt_tail ? 1 : 0;
    return s;
}

// ---- NAPSAC for multi-problem batches (ABI 20)
// mc->grid in usac::MultiGrid's layout: cell, rank, members, eligible (n_total each), start (n_total + P),
// then status, n_cells, n_eligible (P each, contiguous: one copy brings them down)
usac::MultiGrid multi_grid_args(usac_multi *mc) {
    const size_t N = mc->n_total, P = mc->P;
    uint32_t *w = mc->grid.as<uint32_t>();
    usac::MultiGrid g{};
    g.cell = w;
    g.rank = w + N;
    g.members = reinterpret_cast<int32_t *>(w + 2 * N);
    g.eligible = reinterpret_cast<int32_t *>(w + 3 * N);
    g.start = w + 4 * N;
    g.status = w + 5 * N + P;
    g.n_cells = g.status + P;
    g.n_eligible = g.n_cells + P;
    return g;
}

// The grid of one problem past k_multi_grid's caps: usac::GridNeighbors over its points (any n_p, any
// coordinate), uploaded into the problem's slices in the device layout (as host_grid does)
int multi_grid_single(usac_multi *mc, const usac::MultiGrid &g, uint32_t p, int cs) {
    const uint32_t base = mc->offsets[p], n = mc->offsets[p + 1] - base;
    std::vector<float> pts(4 * (size_t)n);
    HIP_TRY(mc, hipMemcpy(pts.data(), mc->pts.as<float>() + 4 * (size_t)base, sizeof(float) * 4 * (size_t)n,
                          hipMemcpyDeviceToHost));
    const usac::GridNeighbors h(pts.data(), n, cs);
    const uint32_t nc = (uint32_t)h.starts().size() - 1;
    std::vector<int32_t> elig;
    for (uint32_t i = 0; i < n; i++)
        if (h.count(i) >= mc->m) elig.push_back((int32_t)i);
    HIP_TRY(mc, hipMemcpy(g.cell + base, h.cells().data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(mc, hipMemcpy(g.rank + base, h.ranks().data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(mc, hipMemcpy(g.members + base, h.members().data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(mc, hipMemcpy(g.start + base + p, h.starts().data(), 4 * ((size_t)nc + 1), hipMemcpyHostToDevice));
    if (!elig.empty()) HIP_TRY(mc, hipMemcpy(g.eligible + base, elig.data(), 4 * elig.size(), hipMemcpyHostToDevice));
    uint32_t *cnt = mc->grid_counts.data();
    cnt[mc->P + p] = nc;
    cnt[2 * (size_t)mc->P + p] = (uint32_t)elig.size();
    HIP_TRY(mc, hipMemcpy(g.n_cells + p, &cnt[mc->P + p], 4, hipMemcpyHostToDevice));
    HIP_TRY(mc, hipMemcpy(g.n_eligible + p, &cnt[2 * (size_t)mc->P + p], 4, hipMemcpyHostToDevice));
    return USAC_OK;
}

// the problems' grid neighbours for cell size cs, kept until another size is asked for: one launch, one
// copy of the counts down, then the problems the kernel deferred on the host
int multi_grid_ensure(usac_multi *mc, int cs) {
    if (cs <= 0) return fail(mc, USAC_ERR_ARG, "grid cell_size must be > 0");
    if (mc->grid_cs == cs) return USAC_OK;
    const size_t N = mc->n_total, P = mc->P;
    HIP_TRY(mc, hipSetDevice(mc->device));
    HIP_TRY(mc, mc->grid.reserve(sizeof(uint32_t) * (5 * N + 4 * P)));
    if (!pin_grow(mc->pin, sizeof(uint32_t) * 3 * P)) return fail(mc, USAC_ERR_HIP, "hipHostMalloc failed");
    mc->grid_cs = 0;
    const usac::MultiGrid g = multi_grid_args(mc);
    HIP_TRY(mc, usac::launch_multi_grid(mc->stream, mc->pts.as<float4>(), mc->offs.as<uint32_t>(), mc->P, cs, mc->m, g));
    HIP_TRY(mc, hipMemcpyAsync(mc->pin.p, g.status, sizeof(uint32_t) * 3 * P, hipMemcpyDeviceToHost, mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    const uint32_t *down = static_cast<const uint32_t *>(mc->pin.p);
    mc->grid_counts.assign(down, down + 3 * P);
    for (uint32_t p = 0; p < mc->P; p++)
        if (mc->grid_counts[p] == usac::kMultiGridDefer) {
            const int rc = multi_grid_single(mc, g, p, cs);
            if (rc) return rc;
        }
    mc->grid_cs = cs;
    return USAC_OK;
}

// ---- the round hooks (usac_multi_hypothesize_score, its SPRT variant, usac_multi_draw_samples)
// problems == NULL: all P problems in order, else the n_problems listed; A: the number of entries
int multi_listed(usac_multi *mc, const uint32_t *problems, uint32_t n_problems, uint32_t &A) {
    if (!problems && n_problems != 0 && n_problems != mc->P)
        return fail(mc, USAC_ERR_ARG, "problems == NULL means all problems: n_problems must be P or 0");
    A = problems ? n_problems : mc->P;
    if (A == 0 || A > usac::kMultiMaxActive) return fail(mc, USAC_ERR_ARG, "n_problems out of range");
    return USAC_OK;
}

// entry by entry, in this order: the problem index, the caller's own check own(a, p) (0: fine), and the
// entry's R x m sample indices if samples are given
template <class Own>
int multi_check_entries(usac_multi *mc, const uint32_t *problems, uint32_t A, const int32_t *samples, uint32_t R,
                        Own own) {
    for (uint32_t a = 0; a < A; a++) {
        const uint32_t p = problems ? problems[a] : a;
        if (p >= mc->P) return fail(mc, USAC_ERR_ARG, "problem index out of range");
        const int rc = own(a, p);
        if (rc) return rc;
        if (!samples) continue;
        const uint32_t n = mc->offsets[p + 1] - mc->offsets[p];
        const int32_t *s = samples + (size_t)a * R * mc->m;
        for (size_t i = 0; i < (size_t)R * mc->m; i++)
            if (s[i] < 0 || (uint32_t)s[i] >= n) return fail(mc, USAC_ERR_ARG, "sample index out of range");
    }
    return USAC_OK;
}

// the score hooks' checks that precede the per-entry ones
int multi_hook_args(usac_multi *mc, const uint32_t *problems, uint32_t n_problems, const int32_t *samples, uint32_t R,
                    const uint64_t *seeds, int dlt_mode, uint32_t &A) {
    if (!multi_round_ok(R)) return fail(mc, USAC_ERR_ARG, "R must be a multiple of 64 in 64..8192");
    if (!multi_is_e(mc) && dlt_mode != USAC_DLT_THIN && dlt_mode != USAC_DLT_NULLSPACE)
        return fail(mc, USAC_ERR_ARG, "dlt_mode");
    const int rc = multi_listed(mc, problems, n_problems, A);
    if (rc) return rc;
    if (!samples && !seeds) return fail(mc, USAC_ERR_ARG, "seeds are required with the device sampler");
    return USAC_OK;
}

// the score hooks' uploads (after multi_ensure): the entries' items, the host samples if given
int multi_hook_upload(usac_multi *mc, const uint32_t *problems, uint32_t A, const int32_t *samples, uint32_t R,
                      const uint64_t *seeds) {
    usac::MultiItem *items = multi_items_pin(mc);
    for (uint32_t a = 0; a < A; a++) items[a] = usac::MultiItem{problems ? problems[a] : a, 0u, seeds ? seeds[a] : 0ull};
    HIP_TRY(mc, hipMemcpyAsync(mc->items.p, items, sizeof(usac::MultiItem) * (size_t)A, hipMemcpyHostToDevice,
                               mc->stream));
    if (samples)
        HIP_TRY(mc, hipMemcpyAsync(mc->samples.p, samples, sizeof(int32_t) * (size_t)A * R * mc->m, hipMemcpyHostToDevice,
                                   mc->stream));
    return USAC_OK;
}

// the score hooks' results down (each nullable); the caller waits for the stream
int multi_hook_down(usac_multi *mc, uint32_t A, uint32_t R, int32_t *counts, float *sums, usac_record *best) {
    const size_t S = (size_t)A * R * mc->spk;
    if (counts) HIP_TRY(mc, hipMemcpyAsync(counts, mc->counts.p, sizeof(int32_t) * S, hipMemcpyDeviceToHost, mc->stream));
    if (sums) HIP_TRY(mc, hipMemcpyAsync(sums, mc->sums.p, sizeof(float) * S, hipMemcpyDeviceToHost, mc->stream));
    if (best)
        HIP_TRY(mc, hipMemcpyAsync(best, mc->out.p, sizeof(usac_record) * (size_t)A, hipMemcpyDeviceToHost, mc->stream));
    return USAC_OK;
}

// ---- the batch-granular run: one loop, three options
// what a run fills besides usac_multi_output (each nullable): the LO counters, PROSAC's final state, the
// SPRT totals (each only with its option), the polish of the final records and its inlier mask
struct MultiRunOutputs {
    usac_multi_lo_output *lo = nullptr;
    usac_multi_prosac_output *pro = nullptr;
    usac_multi_sprt_output *sprt = nullptr;
    usac_multi_polish_output *pol = nullptr;
    uint8_t *mask = nullptr;
};

// PROSAC's end of a round of R hypotheses from `first` for active entry a: item `it` is what the round
// sampled under, rec its record after the round; largest (the sampler's largest_sample_size), bound (the
// last scan's) and scans are the problem's own.  A new record was scanned by the kernel: its candidates are
// applied.  Returns the next round's termination length and clock.
struct ProsacNext {
    uint32_t term_len, clock;
};
ProsacNext multi_prosac_round_end(usac_multi *mc, uint32_t a, const usac::MultiItem &it, const usac_record &rec,
                                  uint64_t first, uint32_t R, uint32_t &largest, uint32_t &bound, uint32_t &scans) {
    const uint32_t p = it.problem, n = mc->offsets[p + 1] - mc->offsets[p];
    const uint32_t *g = mc->growth_host[p]->data();
    // the round's sampler: PROSAC lanes [0, n_prosac), drawn under (clock, term_len) of its start
    const uint32_t n_prosac = usac::prosac_round_lanes(g, n, it.clock, it.term_len, R);
    uint32_t L = it.term_len;
    if (rec.valid && rec.hyp_index >= first) {
        const uint32_t j = (uint32_t)(rec.hyp_index - first);
        const uint32_t at = usac::prosac_largest_at(g, n, mc->m, it.clock, n_prosac, largest, j);
        bound = multi_apply_candidates(mc, a, p, (uint32_t)rec.hyp_index, at);
        L = mc->pterm[p]->terminationLength();
        scans++;
    }
    largest = usac::prosac_largest_at(g, n, mc->m, it.clock, n_prosac, largest, R - 1);
    return ProsacNext{L, it.clock + n_prosac};
}

// The run behind usac_multi_run, _run_polished, _run_prosac, _run_lo, _run_sprt and _run_napsac, which have
// checked that the params ask for what they offer: prosac (the sampler and its termination), napsac (the
// sampler over the problems' grids, built before the loop), lo (k_multi_lo after every round) and sprt
// (verification instead of scoring; not with lo or napsac) are read from prm.  Per round:
// the active list (with sprt: and the entries' tests) up, the round, LO, the PROSAC scan, one copy of
// the records (with sprt: and the statistics behind them) down, one wait; then per entry the bound, and
// the entry is finished or kept.  Every check comes before the first change of the context's state.
// lo_essential: the caller is usac_multi_run_lo_essential, the one entry that runs LO on an essential context.
int multi_run_driver(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out,
                     const MultiRunOutputs &outs, bool lo_essential = false) {
    const bool prosac = prm->sampler == USAC_SAMPLER_PROSAC, sprt = prm->sprt != 0;
    const bool napsac = prm->sampler == USAC_SAMPLER_NAPSAC;
    const bool lo = prm->lo == USAC_LO_INITLORSC || prm->lo == USAC_LO_INITFLORSC;
    if (lo && sprt) return fail(mc, USAC_ERR_UNSUPPORTED, "no LO with SPRT");
    if (napsac && (sprt || prm->cell_size <= 0)) return fail(mc, USAC_ERR_ARG, "NAPSAC: cell_size > 0, no SPRT");
    const uint32_t R = prm->batch ? prm->batch : 256u;
    if (!multi_round_ok(R)) return fail(mc, USAC_ERR_ARG, "batch must be a multiple of 64 in 64..8192");
    if (!multi_is_e(mc) && prm->dlt_mode != USAC_DLT_THIN && prm->dlt_mode != USAC_DLT_NULLSPACE)
        return fail(mc, USAC_ERR_ARG, "dlt_mode");
    if (multi_is_e(mc) && ((lo && !lo_essential) || sprt || napsac))
        return fail(mc, USAC_ERR_UNSUPPORTED, "the essential estimator: uniform or PROSAC sampler, no SPRT, LO through "
                                              "usac_multi_run_lo_essential");
    const uint32_t P = mc->P, m = mc->m;
    if (prosac)
        for (uint32_t p = 0; p < P; p++)
            if (mc->offsets[p + 1] - mc->offsets[p] <= 20)
                return fail(mc, USAC_ERR_ARG, "PROSAC needs > 20 points per problem (prosac_termination_criteria.hpp:158-163)");
    double margin = 0, climb = 0;
    if (sprt && !multi_sprt_cert(margin, climb))
        return fail(mc, USAC_ERR_ARG, "SPRT certificate: margin >= 1e-7 and 0 < climb <= 700");
    HIP_TRY(mc, hipSetDevice(mc->device));
    // a polishing run has passed its checks: the resident result (ABI 27) is this run's from here on
    if (outs.pol) multi_resident_end(mc, "a polishing call that failed");
    // the buffers; a run starts with fresh LO and PROSAC state
    int rc = napsac ? multi_grid_ensure(mc, prm->cell_size) : USAC_OK;
    const usac::MultiGrid mg = napsac ? multi_grid_args(mc) : usac::MultiGrid{};
    if (!rc) rc = multi_ensure(mc, P, R, false);
    if (!rc && lo) rc = multi_lo_ensure(mc, prm, true);
    if (!rc && sprt) rc = multi_sprt_ensure(mc, P, R, false);
    if (!rc && prosac && !(rc = multi_prosac_ensure(mc))) rc = multi_prosac_reset(mc, prm);
    if (rc) return rc;
    // every problem's running record starts invalid (all zero), as a round without a model leaves it
    HIP_TRY(mc, hipMemsetAsync(mc->running.p, 0, sizeof(usac_record) * (size_t)P, mc->stream));
    usac::MultiItem *items = multi_items_pin(mc);
    // with sprt the records and, behind them, the statistics come down in one copy, into their own staging
    usac::SprtConsts *kc = sprt ? multi_sprt_consts_pin(mc) : nullptr;
    usac_record *recs = sprt ? multi_sprt_down_pin(mc, P) : multi_records_pin(mc, P);
    const size_t down = sizeof(usac_record) + (sprt ? sizeof(usac_multi_sprt_stats) : 0);
    // PROSAC, per problem: the sampler's largest_sample_size, the last scan's bound, the scans
    std::vector<uint32_t> largest(prosac ? P : 0, m), pbound(prosac ? P : 0, prm->max_iterations), scans(prosac ? P : 0, 0);
    // SPRT, per problem: the test history and the bound, the run's totals
    std::vector<usac::SprtRounds> tests;
    tests.reserve(sprt ? P : 0);
    std::vector<usac_multi_sprt_output> tot(sprt ? P : 0, usac_multi_sprt_output{});
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t seed = seeds ? seeds[p] : (uint64_t)prm->seed + p;
        const uint32_t n = mc->offsets[p + 1] - mc->offsets[p];
        items[p] = prosac ? usac::MultiItem{p, 1u, seed, n, 0u} : usac::MultiItem{p, 0u, seed, 0u, 0u};
        out[p] = usac_multi_output{};
        if (!sprt) continue;
        tests.emplace_back(mc->estimator, n, m, prm->max_iterations);
        tests.back().reserve_tests((size_t)prm->max_iterations / R + 2);  // at most one test per round
    }
    const usac::StandardTerminationCriteria term(prm->desired_prob, m, 0, prm->max_iterations);
    uint32_t A = P;
    for (uint32_t round = 0; A > 0; round++) {
        const uint64_t first = (uint64_t)round * R, done = first + R;
        HIP_TRY(mc, hipMemcpyAsync(mc->items.p, items, sizeof(usac::MultiItem) * (size_t)A, hipMemcpyHostToDevice,
                                   mc->stream));
        usac::MultiRound r = multi_round(mc, A, R, first, prm->threshold, prm->dlt_mode);
        r.running = mc->running.as<usac_record>();
        if (prosac) r.growth = mc->growth.as<uint32_t>();
        if (napsac) r.grid = &mg;
        const usac::MultiSprt ms = sprt ? multi_sprt_args(mc, A, false) : usac::MultiSprt{};
        if (sprt) {  // every active problem's current test
            for (uint32_t a = 0; a < A; a++) {
                const uint32_t p = items[a].problem;
                const usac::Sprt::History &t = tests[p].test();
                kc[a] = multi_sprt_consts(t.epsilon, t.delta, t.A, mc->offsets[p + 1] - mc->offsets[p], margin, climb);
            }
            HIP_TRY(mc, hipMemcpyAsync(mc->sprt_consts.p, kc, sizeof(usac::SprtConsts) * (size_t)A, hipMemcpyHostToDevice,
                                       mc->stream));
            r.sprt = &ms;
        }
        HIP_TRY(mc, usac::launch_multi_round(mc->stream, r));
        // LO of the round's new bests; the scan and the record copy see the LO'd records
        if (lo)
            HIP_TRY(mc, usac::launch_multi_lo(mc->stream, mc->estimator, mc->pts.as<float4>(), mc->offs.as<uint32_t>(), A,
                                              multi_lo_args(mc, prm, first, false)));
        if (prosac) HIP_TRY(mc, multi_launch_scan(mc, A, first, prm->threshold));
        HIP_TRY(mc, hipMemcpyAsync(recs, mc->out.p, down * (size_t)A, hipMemcpyDeviceToHost, mc->stream));
        HIP_TRY(mc, stream_wait(mc->stream));
        const usac_multi_sprt_stats *stats = reinterpret_cast<const usac_multi_sprt_stats *>(recs + A);  // with sprt
        uint32_t keep = 0;
        for (uint32_t a = 0; a < A; a++) {
            const usac::MultiItem it = items[a];
            const uint32_t p = it.problem, n = mc->offsets[p + 1] - mc->offsets[p];
            ProsacNext nx{0u, 0u};
            if (prosac) nx = multi_prosac_round_end(mc, a, it, recs[a], first, R, largest[p], pbound[p], scans[p]);
            uint32_t bnd = prosac ? pbound[p] : term.getUpBoundIterations((uint32_t)recs[a].inliers, n);
            if (sprt) {  // the sampler's bound counts in a round that improved the record only (SprtRounds::update)
                usac_multi_sprt_output &so = tot[p];
                so.accepted += stats[a].accepted;
                so.rejected += stats[a].rejected_head + stats[a].rejected_tail;
                so.points_tested += stats[a].points_tested;
                tests[p].update((uint32_t)done, stats[a].head_inliers, stats[a].head_points,
                                recs[a].valid && recs[a].hyp_index >= first, (uint32_t)recs[a].inliers, bnd);
                bnd = tests[p].bound();
            }
            if (done >= std::min(prm->max_iterations, bnd)) {
                usac_multi_output &o = out[p];
                o.best = recs[a];
                o.hypotheses = (uint32_t)done;
                o.rounds = round + 1;
                o.bound = bnd;
                o.status = recs[a].inliers > 0 ? USAC_OK : USAC_ERR_NO_MODEL;
                if (prosac && outs.pro) outs.pro[p] = usac_multi_prosac_output{nx.term_len, largest[p], nx.clock, scans[p]};
            } else {
                items[keep++] = prosac ? usac::MultiItem{p, nx.clock, it.seed, nx.term_len, 0u} : it;
            }
        }
        A = keep;
    }
    if (lo && (rc = multi_lo_fetch(mc, outs.lo))) return rc;
    if (sprt && outs.sprt)
        for (uint32_t p = 0; p < P; p++) {
            const usac::Sprt::History &t = tests[p].test();
            tot[p].epsilon = t.epsilon;
            tot[p].delta = t.delta;
            tot[p].A = t.A;
            tot[p].tests = (uint32_t)tests[p].histories();
            outs.sprt[p] = tot[p];
        }
    if (!outs.pol) return USAC_OK;
    // the run's final records are the device's running records (a problem without a model: all
    // zero, which the polish reports as USAC_ERR_NO_MODEL): their model fields are the start models
    static_assert(offsetof(usac_record, model) % sizeof(float) == 0 && sizeof(usac_record) % sizeof(float) == 0,
                  "usac_record's model as a strided float array");
    static_assert(offsetof(usac_multi_output, best) % sizeof(float) == 0 && sizeof(usac_multi_output) % sizeof(float) == 0,
                  "usac_multi_output's model as a strided float array");
    return multi_polish_device(mc, mc->running.as<float>() + offsetof(usac_record, model) / sizeof(float),
                               sizeof(usac_record) / sizeof(float), out[0].best.model,
                               sizeof(usac_multi_output) / sizeof(float), prm->threshold, outs.pol, outs.mask);
}

uint32_t multi_sample_size(int estimator) {
    return estimator == USAC_FUNDAMENTAL ? 7 : estimator == USAC_ESSENTIAL ? 5 : 4;
}

// a context of P problems without points yet; no device call
usac_multi *multi_new(int device, int estimator, uint32_t P) {
    usac_multi *mc = new usac_multi();
    mc->device = device;
    mc->estimator = estimator;
    mc->P = P;
    mc->m = multi_sample_size(estimator);
    mc->spk = estimator == USAC_FUNDAMENTAL ? 3 : 1;
    if (const char *es = getenv("USAC_MULTI_E5_SLICE")) {  // tests: a lower cap on the 5-point solve's slices
        const long v = atol(es);
        if (v > 0 && v < (long)usac::kMultiE5Slice) mc->e5_slice = (uint32_t)v;
    }
    return mc;
}

// usac_multi_create / usac_multi_create_essential after their own checks (out is not NULL): the
// arguments, before any device call, then the context
int multi_create(usac_multi **out, int device, int estimator, const float *pts, const uint32_t *offsets, uint32_t P) {
    const uint32_t m = multi_sample_size(estimator);
    if (P == 0 || P > usac::kMultiMaxActive || !pts || !offsets || offsets[0] != 0) return USAC_ERR_ARG;
    for (uint32_t p = 0; p < P; p++)
        if (offsets[p + 1] < offsets[p] || offsets[p + 1] - offsets[p] < m) return USAC_ERR_ARG;
    usac_multi *mc = multi_new(device, estimator, P);
    mc->n_total = offsets[P];
    mc->offsets.assign(offsets, offsets + P + 1);
    hipError_t e = hipSetDevice(device);
    const char *what = "hipSetDevice";
    if (e == hipSuccess) {
        e = StreamPool::get().stream(&mc->stream);
        what = "hipStreamCreate";
    }
    if (e == hipSuccess) {
        e = mc->pts.reserve(sizeof(float) * 4 * (size_t)mc->n_total);
        what = "hipMalloc points";
    }
    if (e == hipSuccess) e = mc->offs.reserve(sizeof(uint32_t) * ((size_t)P + 1));
    if (e == hipSuccess) e = mc->running.reserve(sizeof(usac_record) * (size_t)P);
    if (e == hipSuccess) {
        e = hipMemcpy(mc->pts.p, pts, sizeof(float) * 4 * (size_t)mc->n_total, hipMemcpyHostToDevice);
        what = "hipMemcpy";
    }
    if (e == hipSuccess) e = hipMemcpy(mc->offs.p, offsets, sizeof(uint32_t) * ((size_t)P + 1), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        fprintf(stderr, "usac_multi_create: %s: %s\n", what, hipGetErrorString(e));
        usac_multi_destroy(mc);
        return USAC_ERR_HIP;
    }
    *out = mc;
    return USAC_OK;
}

// usac_multi_run with or without the polish (usac_multi_run_polished)
int multi_run_uniform(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out,
                      usac_multi_polish_output *pol, uint8_t *mask) {
    if (prm->sprt || prm->lo != USAC_LO_NONE || prm->sampler != USAC_SAMPLER_UNIFORM)
        return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_run: uniform sampler only, no SPRT, no LO (LO: usac_multi_run_lo)");
    return multi_run_driver(mc, prm, seeds, out, MultiRunOutputs{nullptr, nullptr, nullptr, pol, mask});
}

// ---- device input (ABI 25)
// what usac_multi_create_device refused its input for, kept for usac_multi_last_error(NULL): the context that
// would hold the message does not survive the refusal
thread_local std::string g_create_device_err;
thread_local const char *g_create_device_entry = "usac_multi_create_device";  // the entry that reports

int create_device_fail(int code, const std::string &msg) {
    g_create_device_err = std::string(g_create_device_entry) + ": " + msg;
    fprintf(stderr, "%s\n", g_create_device_err.c_str());
    return code;
}

// the caller's pointer `name` must be device memory of `device` with room for `bytes` and aligned to `align`;
// else the reason.  No launch has read it yet.  The extent is checked where the runtime knows the allocation.
std::string device_pointer_problem(const void *ptr, const char *name, int device, size_t bytes, size_t align) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // the sticky error of a pointer the runtime does not know
        return std::string(name) + " is not device memory (" + hipGetErrorString(e) + ")";
    }
    if (at.type != hipMemoryTypeDevice) return std::string(name) + " is not device memory";
    if (at.device != device)
        return std::string(name) + " is memory of device " + std::to_string(at.device) + ", not " + std::to_string(device);
    if (reinterpret_cast<uintptr_t>(ptr) % align)
        return std::string(name) + " is not aligned to " + std::to_string(align) + " bytes";
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ptr)) == hipSuccess) {
        const size_t used = (size_t)(static_cast<const char *>(ptr) - static_cast<const char *>(base));
        if (used > size || size - used < bytes)
            return std::string(name) + " has room for " + std::to_string(size - used) + " bytes, " + std::to_string(bytes) +
                   " are needed";
    } else {
        (void)hipGetLastError();
    }
    return "";
}

// the width of P x n_max output bytes (usac_multi_export_device, usac_multi_pose_device): usac_pack.hpp's rule
int multi_width_check(usac_multi *mc, const char *who, uint32_t n_max) {
    const uint32_t widest = mc->n_max ? 0u : usac::widest_problem(mc->offsets.data(), mc->P);
    const usac::WidthStatus st = usac::output_width(mc->n_max, widest, n_max);
    if (st == usac::kWidthOk) return USAC_OK;
    return fail(mc, USAC_ERR_ARG, std::string(who) + usac::width_message(st, mc->n_max, widest));
}

// the entries that read the resident result (ABI 27): refused, with what ended it, when there is none
int multi_resident_check(usac_multi *mc, const char *who) {
    if (mc->resident_valid) return USAC_OK;
    return fail(mc, USAC_ERR_UNSUPPORTED,
                std::string(who) + (mc->resident_end ? std::string("the result of the last polishing call is no longer "
                                                                   "resident: ended by ") + mc->resident_end
                                                     : std::string("no polishing call has run on this context")));
}

// the pose entries (ABI 28) decompose an essential matrix: refused on any other context before a device call
int multi_pose_only_essential(usac_multi *mc, const char *who) {
    if (multi_is_e(mc)) return USAC_OK;
    return fail(mc, USAC_ERR_UNSUPPORTED, std::string(who) + "for the essential estimator only (a homography or a "
                                                             "fundamental matrix has no four [R | t] to choose from)");
}

}  // namespace

extern "C" {

int usac_prosac_schedule(uint32_t n, uint32_t m, uint32_t clock, uint32_t term_len, uint32_t R, uint32_t *subset,
                         uint32_t *clock_next, uint32_t *largest) {
    if (m < 2 || n < m || clock < 1 || clock > (1u << 30) || term_len < m || term_len > n || R > (1u << 20))
        return USAC_ERR_ARG;
    const auto tab = usac::ProsacSampler::growth_table(n, m);
    const uint32_t *g = tab->data();
    if (subset)
        for (uint32_t j = 0; j < R; j++) {  // the branch rule of the device sampler, lane by lane
            const uint32_t t = clock + j;
            uint32_t s_prev, s_now;
            if (t > usac::kProsacGrowthMax) {
                subset[j] = UINT32_MAX;
                continue;
            }
            usac::prosac_subset_pair(g, n, m, t, s_prev, s_now);
            subset[j] = s_prev > term_len ? 0u : s_now;
        }
    const uint32_t n_prosac = usac::prosac_round_lanes(g, n, clock, term_len, R);
    if (clock_next) *clock_next = clock + n_prosac;
    if (largest) *largest = usac::prosac_largest_at(g, n, m, clock, n_prosac, *largest, R ? R - 1 : 0);
    return USAC_OK;
}

int usac_multi_create(usac_multi **out, int device, int estimator, const float *pts, const uint32_t *offsets,
                      uint32_t P) {
    if (!out) return USAC_ERR_ARG;
    *out = nullptr;
    if (estimator != USAC_HOMOGRAPHY && estimator != USAC_FUNDAMENTAL) return USAC_ERR_UNSUPPORTED;
    return multi_create(out, device, estimator, pts, offsets, P);
}

int usac_multi_create_essential(usac_multi **out, int device, const float *pts, const uint32_t *offsets, uint32_t P) {
    if (!out) return USAC_ERR_ARG;
    *out = nullptr;
    return multi_create(out, device, USAC_ESSENTIAL, pts, offsets, P);
}

int usac_multi_create_essential_pixels(usac_multi **out, int device, const float *pts_px, const uint32_t *offsets,
                                       uint32_t P, const float *K1, const float *K2) {
    if (!out) return USAC_ERR_ARG;
    *out = nullptr;
    if (!K1 || P == 0 || P > usac::kMultiMaxActive) return USAC_ERR_ARG;
    if (!K2) K2 = K1;
    for (uint32_t p = 0; p < P; p++)
        if (!usac::pixel_k_ok(K1 + 9 * (size_t)p) || !usac::pixel_k_ok(K2 + 9 * (size_t)p)) return USAC_ERR_ARG;
    usac_multi *mc = nullptr;
    const int rc = multi_create(&mc, device, USAC_ESSENTIAL, pts_px, offsets, P);
    if (rc) return rc;
    mc->k1.assign(K1, K1 + 9 * (size_t)P);
    mc->k2.assign(K2, K2 + 9 * (size_t)P);
    // the rows in place: the problems' intrinsics up, one launch, and the call returns when it has finished
    std::vector<float> calib(usac::kCalibFloats * (size_t)P);
    for (uint32_t p = 0; p < P; p++)
        usac::pixel_pack(K1 + 9 * (size_t)p, K2 + 9 * (size_t)p, calib.data() + usac::kCalibFloats * (size_t)p);
    DevBuf dcal;
    hipError_t e = dcal.reserve(sizeof(float) * calib.size());
    const char *what = "hipMalloc intrinsics";
    if (e == hipSuccess) {
        e = hipMemcpy(dcal.p, calib.data(), sizeof(float) * calib.size(), hipMemcpyHostToDevice);
        what = "hipMemcpy intrinsics";
    }
    if (e == hipSuccess) {
        e = usac::launch_multi_calibrate(mc->stream, mc->pts.as<float4>(), mc->offs.as<uint32_t>(), P, mc->n_total,
                                         static_cast<const float *>(dcal.p));
        what = "k_multi_calibrate";
    }
    if (e == hipSuccess) e = hipStreamSynchronize(mc->stream);
    dcal.release();
    if (e != hipSuccess) {
        fprintf(stderr, "usac_multi_create_essential_pixels: %s: %s\n", what, hipGetErrorString(e));
        usac_multi_destroy(mc);
        return USAC_ERR_HIP;
    }
    *out = mc;
    return USAC_OK;
}

// usac_multi_create_device (sorted false, order ignored) and usac_multi_create_device_sorted (ABI 26: order and its
// scores are needed), reporting under the entry's name
static int multi_create_device(const char *entry, usac_multi **out, int device, int estimator, const usac_multi_device_input *in,
                               bool sorted, const usac_multi_device_order *order) {
    if (!out) return USAC_ERR_ARG;
    *out = nullptr;
    g_create_device_err.clear();
    g_create_device_entry = entry;
    if (!in) return create_device_fail(USAC_ERR_ARG, "NULL input");
    if (estimator != USAC_HOMOGRAPHY && estimator != USAC_FUNDAMENTAL && estimator != USAC_ESSENTIAL)
        return create_device_fail(USAC_ERR_UNSUPPORTED, "homography, fundamental or essential estimator only");
    const uint32_t P = in->P, n_max = in->n_max;
    if (P == 0 || P > usac::kMultiMaxActive) return create_device_fail(USAC_ERR_ARG, "P must be in 1..65535");
    if (!usac::pack_extent_ok(P, n_max)) return create_device_fail(USAC_ERR_ARG, "n_max must be > 0 and P * n_max < 2^32");
    const bool form_a = in->rows || in->valid || in->counts, form_b = in->kpts0 || in->kpts1 || in->match || in->n1;
    if (form_a == form_b)
        return create_device_fail(USAC_ERR_ARG, "give rows (form a) or kpts0 / kpts1 / match (form b), one of them");
    if (form_a && !in->rows) return create_device_fail(USAC_ERR_ARG, "valid or counts without rows");
    if (in->valid && in->counts) return create_device_fail(USAC_ERR_ARG, "valid and counts are alternatives");
    if (form_b && (!in->kpts0 || !in->kpts1 || !in->match || in->n1 == 0))
        return create_device_fail(USAC_ERR_ARG, "form b needs kpts0, kpts1, match and n1 > 0");
    if (form_b && (uint64_t)P * in->n1 >= (1ull << 32)) return create_device_fail(USAC_ERR_ARG, "P * n1 must be < 2^32");
    if ((in->K1 || in->K2) && estimator != USAC_ESSENTIAL)
        return create_device_fail(USAC_ERR_ARG, "K1 / K2 are for the essential estimator");
    if (in->K2 && !in->K1) return create_device_fail(USAC_ERR_ARG, "K2 without K1");
    const float *K1 = in->K1, *K2 = in->K2 ? in->K2 : in->K1;
    if (K1)
        for (uint32_t p = 0; p < P; p++)
            if (!usac::pixel_k_ok(K1 + 9 * (size_t)p) || !usac::pixel_k_ok(K2 + 9 * (size_t)p))
                return create_device_fail(USAC_ERR_ARG, "problem " + std::to_string(p) + ": K must be finite and upper "
                                                        "triangular with fx, fy > 0 and a last row of 0 0 1");
    if (sorted && (!order || !order->scores)) return create_device_fail(USAC_ERR_ARG, "NULL order or scores");
    const float *scores = sorted ? order->scores : nullptr;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return create_device_fail(USAC_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    // a host pointer must never reach a kernel: every pointer the kernels will read, before any launch
    const size_t cells = (size_t)P * n_max;
    struct { const void *p; const char *name; size_t bytes, align; } ptrs[] = {
        {in->rows, "rows", cells * 16, 16},           {in->valid, "valid", cells, 1},
        {in->counts, "counts", (size_t)P * 4, 4},     {in->kpts0, "kpts0", cells * 8, 8},
        {in->kpts1, "kpts1", (size_t)P * in->n1 * 8, 8}, {in->match, "match", cells * 4, 4},
        {scores, "scores", cells * 4, 4}};
    for (const auto &q : ptrs) {
        if (!q.p) continue;
        const std::string why = device_pointer_problem(q.p, q.name, device, q.bytes, q.align);
        if (!why.empty()) return create_device_fail(USAC_ERR_ARG, why);
    }
    usac::MultiPack pk{};
    pk.P = P;
    pk.n_max = n_max;
    pk.n1 = in->n1;
    pk.rows = reinterpret_cast<const uint4 *>(in->rows);
    pk.valid = in->valid;
    pk.counts = in->counts;
    pk.kpts0 = reinterpret_cast<const uint2 *>(in->kpts0);
    pk.kpts1 = reinterpret_cast<const uint2 *>(in->kpts1);
    pk.match = in->match;
    // every kernel that reads the caller's memory runs on the caller's stream, behind the producer's work
    hipStream_t cs = static_cast<hipStream_t>(in->stream);
    usac_multi *mc = multi_new(device, estimator, P);
    mc->n_max = n_max;
    DevBuf dcount, dcal;  // the counting pass's 2 P values; the intrinsics
    DevBuf dtmp, druns;   // with scores: the pack's rows and columns before the sort; the sort's runs past its cap
    PinBlock pin;
    std::string msg;
    const char *what = "hipStreamCreate";
    auto done = [&](int code) {
        dcount.release();
        dcal.release();
        dtmp.release();
        druns.release();
        if (pin.p) PinnedPool::get().give_back(pin.p, pin.bytes);
        if (code == USAC_OK) {
            *out = mc;
            return code;
        }
        usac_multi_destroy(mc);
        return create_device_fail(code, msg);
    };
    e = StreamPool::get().stream(&mc->stream);
    if (e == hipSuccess) {
        e = dcount.reserve(sizeof(uint32_t) * 2 * (size_t)P);
        what = "hipMalloc counts";
    }
    if (e == hipSuccess && !(pin.p = PinnedPool::get().take(sizeof(uint32_t) * 2 * (size_t)P, &pin.bytes))) {
        msg = "hipHostMalloc failed";
        return done(USAC_ERR_HIP);
    }
    uint32_t *sizes = static_cast<uint32_t *>(pin.p);
    if (e == hipSuccess) {
        e = usac::launch_multi_pack_count(cs, pk, dcount.as<uint32_t>(), dcount.as<uint32_t>() + P);
        what = "k_multi_pack_count";
    }
    if (e == hipSuccess) {
        e = hipMemcpyAsync(sizes, dcount.p, sizeof(uint32_t) * 2 * (size_t)P, hipMemcpyDeviceToHost, cs);
        what = "hipMemcpy counts";
    }
    if (e == hipSuccess) e = stream_wait(cs);
    if (e == hipSuccess) {
        mc->offsets.assign((size_t)P + 1, 0u);
        uint32_t bad = 0;
        const usac::PackStatus st = usac::pack_offsets(sizes, sizes + P, P, mc->m, n_max, mc->offsets.data(), &bad);
        if (st != usac::kPackOk) {
            msg = usac::pack_message(st, bad, sizes[bad], mc->m);
            return done(USAC_ERR_ARG);
        }
        mc->n_total = mc->offsets[P];
        e = mc->pts.reserve(sizeof(float) * 4 * (size_t)mc->n_total);
        what = "hipMalloc points";
    }
    if (e == hipSuccess) e = mc->src.reserve(sizeof(uint32_t) * (size_t)mc->n_total);
    if (e == hipSuccess) e = mc->offs.reserve(sizeof(uint32_t) * ((size_t)P + 1));
    if (e == hipSuccess) e = mc->running.reserve(sizeof(usac_record) * (size_t)P);
    if (e == hipSuccess) {
        e = hipMemcpyAsync(mc->offs.p, mc->offsets.data(), sizeof(uint32_t) * ((size_t)P + 1), hipMemcpyHostToDevice, cs);
        what = "hipMemcpy offsets";
    }
    if (e == hipSuccess && !scores) {
        e = usac::launch_multi_pack(cs, pk, mc->offs.as<uint32_t>(), mc->pts.as<float4>(), mc->src.as<uint32_t>());
        what = "k_multi_pack";
    }
    if (e == hipSuccess && scores) {
        // the pack as it is, into a temporary block of N_total x (16 + 4) bytes; the sort moves every row from it
        // to its place in quality order (kernels_multi_sort.hip), on the same stream
        usac::MultiSort so{};
        so.cap = usac::kMultiSortLds;
        if (const char *es = getenv("USAC_MULTI_SORT_LDS")) {  // tests: a lower cap on the rows sorted in LDS at once
            const long v = atol(es);
            if (v > 0 && v < (long)usac::kMultiSortLds) so.cap = (uint32_t)v;
        }
        const size_t n_total = mc->n_total;
        e = dtmp.reserve((sizeof(float) * 4 + sizeof(uint32_t)) * n_total);
        what = "hipMalloc the rows before the sort";
        if (e == hipSuccess && *std::max_element(sizes, sizes + P) > so.cap) e = druns.reserve(sizeof(uint64_t) * n_total);
        float4 *rows_in = dtmp.as<float4>();
        uint32_t *src_in = reinterpret_cast<uint32_t *>(rows_in + n_total);
        if (e == hipSuccess) {
            e = usac::launch_multi_pack(cs, pk, mc->offs.as<uint32_t>(), rows_in, src_in);
            what = "k_multi_pack";
        }
        if (e == hipSuccess) {
            so.scores = reinterpret_cast<const uint32_t *>(scores);
            so.n_max = n_max;
            so.descending = order->descending != 0;
            so.offsets = mc->offs.as<uint32_t>();
            so.rows_in = reinterpret_cast<const uint4 *>(rows_in);
            so.src_in = src_in;
            so.pts = reinterpret_cast<uint4 *>(mc->pts.as<float4>());
            so.src = mc->src.as<uint32_t>();
            so.runs = druns.as<uint64_t>();
            e = usac::launch_multi_sort(cs, P, so);
            what = "k_multi_sort";
        }
    }
    std::vector<float> calib;
    if (e == hipSuccess && K1) {  // pixels -> calibrated rows, as usac_multi_create_essential_pixels, behind the pack
        mc->k1.assign(K1, K1 + 9 * (size_t)P);
        mc->k2.assign(K2, K2 + 9 * (size_t)P);
        calib.resize(usac::kCalibFloats * (size_t)P);
        for (uint32_t p = 0; p < P; p++)
            usac::pixel_pack(K1 + 9 * (size_t)p, K2 + 9 * (size_t)p, calib.data() + usac::kCalibFloats * (size_t)p);
        e = dcal.reserve(sizeof(float) * calib.size());
        what = "hipMalloc intrinsics";
        if (e == hipSuccess) {
            e = hipMemcpyAsync(dcal.p, calib.data(), sizeof(float) * calib.size(), hipMemcpyHostToDevice, cs);
            what = "hipMemcpy intrinsics";
        }
        if (e == hipSuccess) {
            e = usac::launch_multi_calibrate(cs, mc->pts.as<float4>(), mc->offs.as<uint32_t>(), P, mc->n_total,
                                             static_cast<const float *>(dcal.p));
            what = "k_multi_calibrate";
        }
    }
    // the context holds its own copy from here on: the caller may overwrite or free its tensors
    if (e == hipSuccess) {
        e = stream_wait(cs);
        what = "the caller's stream";
    }
    if (e != hipSuccess) {
        msg = std::string(what) + ": " + hipGetErrorString(e);
        return done(USAC_ERR_HIP);
    }
    return done(USAC_OK);
}

int usac_multi_create_device(usac_multi **out, int device, int estimator, const usac_multi_device_input *in) {
    return multi_create_device("usac_multi_create_device", out, device, estimator, in, false, nullptr);
}

int usac_multi_create_device_sorted(usac_multi **out, int device, int estimator, const usac_multi_device_input *in,
                                    const usac_multi_device_order *order) {
    return multi_create_device("usac_multi_create_device_sorted", out, device, estimator, in, true, order);
}

int usac_multi_get_offsets(const usac_multi *mc, uint32_t *offsets) {
    if (!mc || !offsets) return USAC_ERR_ARG;
    std::copy(mc->offsets.begin(), mc->offsets.end(), offsets);
    return USAC_OK;
}

int usac_multi_get_source(usac_multi *mc, uint32_t *src) {
    if (!mc) return USAC_ERR_ARG;
    if (mc->n_max == 0)
        return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_get_source: the context was not created from device input "
                                              "(usac_multi_create_device)");
    if (!src) return fail(mc, USAC_ERR_ARG, "usac_multi_get_source: NULL argument");
    HIP_TRY(mc, hipSetDevice(mc->device));
    HIP_TRY(mc, hipMemcpy(src, mc->src.p, sizeof(uint32_t) * (size_t)mc->n_total, hipMemcpyDeviceToHost));
    return USAC_OK;
}

int usac_multi_padded_mask(usac_multi *mc, const uint8_t *mask, uint8_t *d_out, void *stream) {
    if (!mc) return USAC_ERR_ARG;
    if (mc->n_max == 0)
        return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_padded_mask: the context was not created from device input "
                                              "(usac_multi_create_device)");
    if (!mask || !d_out) return fail(mc, USAC_ERR_ARG, "usac_multi_padded_mask: NULL argument");
    HIP_TRY(mc, hipSetDevice(mc->device));
    const size_t cells = (size_t)mc->P * mc->n_max;
    const std::string why = device_pointer_problem(d_out, "d_out", mc->device, cells, 1);
    if (!why.empty()) return fail(mc, USAC_ERR_ARG, "usac_multi_padded_mask: " + why);
    hipStream_t cs = static_cast<hipStream_t>(stream);
    // every call of this context has waited for its stream: mc->mask is free to stage the upload
    multi_resident_end(mc, "usac_multi_padded_mask (its upload staged a host mask in the mask buffer)");
    HIP_TRY(mc, mc->mask.reserve(mc->n_total));
    HIP_TRY(mc, hipMemcpyAsync(mc->mask.p, mask, mc->n_total, hipMemcpyHostToDevice, cs));
    HIP_TRY(mc, hipMemsetAsync(d_out, 0, cells, cs));
    HIP_TRY(mc, usac::launch_multi_unpack_mask(cs, mc->mask.as<uint8_t>(), mc->src.as<uint32_t>(), mc->offs.as<uint32_t>(),
                                               mc->P, mc->n_total, mc->n_max, d_out));
    HIP_TRY(mc, stream_wait(cs));
    return USAC_OK;
}

// ---- device output (ABI 27)
int usac_multi_set_resident(usac_multi *mc, int on) {
    if (!mc) return USAC_ERR_ARG;
    mc->resident_on = on != 0;
    return USAC_OK;
}

int usac_multi_export_device(usac_multi *mc, const usac_multi_device_output *o) {
    const char *who = "usac_multi_export_device: ";
    if (!mc) return USAC_ERR_ARG;
    if (!o) return fail(mc, USAC_ERR_ARG, std::string(who) + "NULL output");
    if (!o->models && !o->pixel_models && !o->inliers && !o->status && !o->mask && !o->inlier_cols)
        return fail(mc, USAC_ERR_ARG, std::string(who) + "every output pointer is NULL");
    const uint32_t P = mc->P;
    int rc = multi_width_check(mc, who, o->n_max);
    if (rc) return rc;
    if ((o->inlier_cols != nullptr) != (o->k_max != 0))
        return fail(mc, USAC_ERR_ARG, std::string(who) + "k_max > 0 goes with inlier_cols, and 0 with a NULL inlier_cols");
    if (!usac::export_extent_ok(P, o->n_max, o->k_max))
        return fail(mc, USAC_ERR_ARG, std::string(who) + "n_max must be > 0, P * n_max and P * k_max < 2^32");
    rc = multi_resident_check(mc, who);
    if (rc) return rc;
    if (o->pixel_models && mc->k1.empty())
        return fail(mc, USAC_ERR_UNSUPPORTED, std::string(who) + "pixel_models: the context was not created with intrinsics "
                                                  "(usac_multi_create_essential_pixels, usac_multi_create_device with K1)");
    HIP_TRY(mc, hipSetDevice(mc->device));
    // a host pointer must never reach the kernel: every pointer it will write, before the launch
    const size_t cells = (size_t)P * o->n_max;
    struct { const void *p; const char *name; size_t bytes, align; } ptrs[] = {
        {o->models, "models", (size_t)P * 36, 4},   {o->pixel_models, "pixel_models", (size_t)P * 36, 4},
        {o->inliers, "inliers", (size_t)P * 4, 4},  {o->status, "status", (size_t)P * 4, 4},
        {o->mask, "mask", cells, 1},                {o->inlier_cols, "inlier_cols", (size_t)P * o->k_max * 4, 4}};
    for (const auto &q : ptrs) {
        if (!q.p) continue;
        const std::string why = device_pointer_problem(q.p, q.name, mc->device, q.bytes, q.align);
        if (!why.empty()) return fail(mc, USAC_ERR_ARG, std::string(who) + why);
    }
    if (o->pixel_models && !mc->kdev.p) {  // once: the intrinsics the context kept on the host
        const size_t half = sizeof(float) * 9 * (size_t)P;
        HIP_TRY(mc, mc->kdev.reserve(2 * half));
        hipError_t e = hipMemcpy(mc->kdev.p, mc->k1.data(), half, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(static_cast<char *>(mc->kdev.p) + half, mc->k2.data(), half, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            mc->kdev.release();
            HIP_TRY(mc, e);
        }
    }
    usac::MultiExport a{};
    a.pol = mc->pol_out.as<usac_multi_polish_output>();
    a.mask = mc->mask.as<uint8_t>();
    a.src = mc->n_max ? mc->src.as<uint32_t>() : nullptr;
    a.offsets = mc->offs.as<uint32_t>();
    a.k = mc->kdev.as<float>();
    a.P = P;
    a.n_max = o->n_max;
    a.k_max = o->k_max;
    a.models = o->models;
    a.pixel_models = o->pixel_models;
    a.inliers = o->inliers;
    a.status = o->status;
    a.mask_out = o->mask;
    a.cols = o->inlier_cols;
    // every call of this context has waited for its streams: the resident buffers are at rest, and stay so
    hipStream_t cs = static_cast<hipStream_t>(o->stream);
    HIP_TRY(mc, usac::launch_multi_export(cs, a));
    HIP_TRY(mc, stream_wait(cs));
    return USAC_OK;
}

// ---- pose (ABI 28)
int usac_multi_pose_device(usac_multi *mc, const usac_multi_pose_output *o) {
    const char *who = "usac_multi_pose_device: ";
    if (!mc) return USAC_ERR_ARG;
    int rc = multi_pose_only_essential(mc, who);
    if (rc) return rc;
    if (!o) return fail(mc, USAC_ERR_ARG, std::string(who) + "NULL output");
    if (!o->R && !o->t && !o->front && !o->choice && !o->front_mask)
        return fail(mc, USAC_ERR_ARG, std::string(who) + "every output pointer is NULL");
    const uint32_t P = mc->P;
    rc = multi_width_check(mc, who, o->n_max);
    if (rc) return rc;
    if (!usac::pack_extent_ok(P, o->n_max))
        return fail(mc, USAC_ERR_ARG, std::string(who) + "n_max must be > 0, P * n_max < 2^32");
    rc = multi_resident_check(mc, who);
    if (rc) return rc;
    HIP_TRY(mc, hipSetDevice(mc->device));
    // a host pointer must never reach the kernel: every pointer it will write, before the launch
    struct { const void *p; const char *name; size_t bytes, align; } ptrs[] = {
        {o->R, "R", (size_t)P * 36, 4},         {o->t, "t", (size_t)P * 12, 4},
        {o->front, "front", (size_t)P * 4, 4},  {o->choice, "choice", (size_t)P * 4, 4},
        {o->front_mask, "front_mask", (size_t)P * o->n_max, 1}};
    for (const auto &q : ptrs) {
        if (!q.p) continue;
        const std::string why = device_pointer_problem(q.p, q.name, mc->device, q.bytes, q.align);
        if (!why.empty()) return fail(mc, USAC_ERR_ARG, std::string(who) + why);
    }
    usac::MultiPose a{};
    a.pts = mc->pts.as<float4>();
    a.offsets = mc->offs.as<uint32_t>();
    a.pol = mc->pol_out.as<usac_multi_polish_output>();
    a.mask = mc->mask.as<uint8_t>();
    a.src = mc->n_max ? mc->src.as<uint32_t>() : nullptr;
    a.P = P;
    a.n_max = o->n_max;
    a.R = o->R;
    a.t = o->t;
    a.front = o->front;
    a.choice = o->choice;
    a.front_mask = o->front_mask;
    // every call of this context has waited for its streams: the resident buffers are at rest, and are only read
    hipStream_t cs = static_cast<hipStream_t>(o->stream);
    HIP_TRY(mc, usac::launch_multi_pose(cs, a));
    HIP_TRY(mc, stream_wait(cs));
    return USAC_OK;
}

int usac_multi_pose(usac_multi *mc, const float *E, const uint8_t *mask, float *R, float *t, int32_t *front,
                    int32_t *choice, uint8_t *front_mask) {
    const char *who = "usac_multi_pose: ";
    if (!mc) return USAC_ERR_ARG;
    const int rc = multi_pose_only_essential(mc, who);
    if (rc) return rc;
    if (!E) return fail(mc, USAC_ERR_ARG, std::string(who) + "NULL models");
    if (!R && !t && !front && !choice && !front_mask)
        return fail(mc, USAC_ERR_ARG, std::string(who) + "every output pointer is NULL");
    HIP_TRY(mc, hipSetDevice(mc->device));
    // one block of the call's own: [E | R | t | front | choice] of P problems, then the mask and the front mask
    // over the packed rows; the resident buffers (pol_out, mask) are not touched
    const size_t P = mc->P, n = mc->n_total;
    const size_t at_R = 36 * P, at_t = at_R + 36 * P, at_front = at_t + 12 * P, at_choice = at_front + 4 * P,
                 at_mask = at_choice + 4 * P, at_fm = at_mask + n;
    HIP_TRY(mc, mc->pose_buf.reserve(at_fm + n));
    char *d = mc->pose_buf.as<char>();
    HIP_TRY(mc, hipMemcpyAsync(d, E, 36 * P, hipMemcpyHostToDevice, mc->stream));
    if (mask) HIP_TRY(mc, hipMemcpyAsync(d + at_mask, mask, n, hipMemcpyHostToDevice, mc->stream));
    usac::MultiPose a{};
    a.pts = mc->pts.as<float4>();
    a.offsets = mc->offs.as<uint32_t>();
    a.models = reinterpret_cast<const float *>(d);
    a.mask = mask ? reinterpret_cast<const uint8_t *>(d + at_mask) : nullptr;
    a.P = mc->P;
    a.packed = true;
    a.R = R ? reinterpret_cast<float *>(d + at_R) : nullptr;
    a.t = t ? reinterpret_cast<float *>(d + at_t) : nullptr;
    a.front = front ? reinterpret_cast<int32_t *>(d + at_front) : nullptr;
    a.choice = choice ? reinterpret_cast<int32_t *>(d + at_choice) : nullptr;
    a.front_mask = front_mask ? reinterpret_cast<uint8_t *>(d + at_fm) : nullptr;
    HIP_TRY(mc, usac::launch_multi_pose(mc->stream, a));
    if (R) HIP_TRY(mc, hipMemcpyAsync(R, d + at_R, 36 * P, hipMemcpyDeviceToHost, mc->stream));
    if (t) HIP_TRY(mc, hipMemcpyAsync(t, d + at_t, 12 * P, hipMemcpyDeviceToHost, mc->stream));
    if (front) HIP_TRY(mc, hipMemcpyAsync(front, d + at_front, 4 * P, hipMemcpyDeviceToHost, mc->stream));
    if (choice) HIP_TRY(mc, hipMemcpyAsync(choice, d + at_choice, 4 * P, hipMemcpyDeviceToHost, mc->stream));
    if (front_mask) HIP_TRY(mc, hipMemcpyAsync(front_mask, d + at_fm, n, hipMemcpyDeviceToHost, mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    return USAC_OK;
}

// ---- pose refinement (ABI 29)
int usac_multi_refine_pose_device(usac_multi *mc, const usac_multi_refine_io *o) {
    const char *who = "usac_multi_refine_pose_device: ";
    if (!mc) return USAC_ERR_ARG;
    int rc = multi_pose_only_essential(mc, who);
    if (rc) return rc;
    if (!o) return fail(mc, USAC_ERR_ARG, std::string(who) + "NULL arguments");
    if (!o->R_in || !o->t_in) return fail(mc, USAC_ERR_ARG, std::string(who) + "NULL R_in or t_in");
    if (!usac::refine_iters_ok(o->max_iters))
        return fail(mc, USAC_ERR_ARG, std::string(who) + "max_iters must be 0..100");
    if (!o->R && !o->t && !o->E && !o->cost0 && !o->cost && !o->iterations && !o->used)
        return fail(mc, USAC_ERR_ARG, std::string(who) + "every output pointer is NULL");
    const uint32_t P = mc->P;
    rc = multi_width_check(mc, who, o->n_max);
    if (rc) return rc;
    if (!usac::pack_extent_ok(P, o->n_max))
        return fail(mc, USAC_ERR_ARG, std::string(who) + "n_max must be > 0, P * n_max < 2^32");
    rc = multi_resident_check(mc, who);
    if (rc) return rc;
    HIP_TRY(mc, hipSetDevice(mc->device));
    // a host pointer must never reach the kernel: every pointer it will read or write, before the launch
    struct { const void *p; const char *name; size_t bytes, align; } ptrs[] = {
        {o->R_in, "R_in", (size_t)P * 36, 4},   {o->t_in, "t_in", (size_t)P * 12, 4},
        {o->mask_in, "mask_in", (size_t)P * o->n_max, 1},
        {o->R, "R", (size_t)P * 36, 4},         {o->t, "t", (size_t)P * 12, 4},
        {o->E, "E", (size_t)P * 36, 4},         {o->cost0, "cost0", (size_t)P * 8, 8},
        {o->cost, "cost", (size_t)P * 8, 8},    {o->iterations, "iterations", (size_t)P * 4, 4},
        {o->used, "used", (size_t)P * 4, 4}};
    for (const auto &q : ptrs) {
        if (!q.p) continue;
        const std::string why = device_pointer_problem(q.p, q.name, mc->device, q.bytes, q.align);
        if (!why.empty()) return fail(mc, USAC_ERR_ARG, std::string(who) + why);
    }
    usac::MultiRefine a{};
    a.pts = mc->pts.as<float4>();
    a.offsets = mc->offs.as<uint32_t>();
    a.pol = mc->pol_out.as<usac_multi_polish_output>();
    a.R_in = o->R_in;
    a.t_in = o->t_in;
    // the caller's mask is padded, a row's byte at its source column; the resident one lies over the packed rows
    a.mask = o->mask_in ? o->mask_in : mc->mask.as<uint8_t>();
    a.mask_packed = o->mask_in == nullptr;
    a.src = (o->mask_in && mc->n_max) ? mc->src.as<uint32_t>() : nullptr;
    a.P = P;
    a.n_max = o->n_max;
    a.max_iters = o->max_iters;
    a.R = o->R;
    a.t = o->t;
    a.E = o->E;
    a.cost0 = o->cost0;
    a.cost = o->cost;
    a.iterations = o->iterations;
    a.used = o->used;
    // every call of this context has waited for its streams: the resident buffers are at rest, and are only read
    hipStream_t cs = static_cast<hipStream_t>(o->stream);
    HIP_TRY(mc, usac::launch_multi_refine(cs, a));
    HIP_TRY(mc, stream_wait(cs));
    return USAC_OK;
}

int usac_multi_refine_pose(usac_multi *mc, const float *R, const float *t, const uint8_t *mask, uint32_t max_iters,
                           float *R_out, float *t_out, float *E_out, double *cost0, double *cost, int32_t *iterations,
                           int32_t *used) {
    const char *who = "usac_multi_refine_pose: ";
    if (!mc) return USAC_ERR_ARG;
    const int rc = multi_pose_only_essential(mc, who);
    if (rc) return rc;
    if (!R || !t) return fail(mc, USAC_ERR_ARG, std::string(who) + "NULL R or t");
    if (!usac::refine_iters_ok(max_iters)) return fail(mc, USAC_ERR_ARG, std::string(who) + "max_iters must be 0..100");
    if (!R_out && !t_out && !E_out && !cost0 && !cost && !iterations && !used)
        return fail(mc, USAC_ERR_ARG, std::string(who) + "every output pointer is NULL");
    HIP_TRY(mc, hipSetDevice(mc->device));
    // one block of the call's own (usac_pack.hpp's refine_block): the poses are refined in place in it, the
    // resident buffers are not touched
    const size_t P = mc->P, n = mc->n_total;
    const usac::RefineBlock blk = usac::refine_block(P, n);
    const size_t at_cost0 = blk.cost0, at_cost = blk.cost, at_R = blk.R, at_t = blk.t, at_E = blk.E, at_iter = blk.iterations,
                 at_used = blk.used, at_mask = blk.mask;
    HIP_TRY(mc, mc->refine_buf.reserve(blk.bytes));
    char *d = mc->refine_buf.as<char>();
    HIP_TRY(mc, hipMemcpyAsync(d + at_R, R, 36 * P, hipMemcpyHostToDevice, mc->stream));
    HIP_TRY(mc, hipMemcpyAsync(d + at_t, t, 12 * P, hipMemcpyHostToDevice, mc->stream));
    if (mask) HIP_TRY(mc, hipMemcpyAsync(d + at_mask, mask, n, hipMemcpyHostToDevice, mc->stream));
    usac::MultiRefine a{};
    a.pts = mc->pts.as<float4>();
    a.offsets = mc->offs.as<uint32_t>();
    a.R_in = reinterpret_cast<const float *>(d + at_R);
    a.t_in = reinterpret_cast<const float *>(d + at_t);
    a.mask = mask ? reinterpret_cast<const uint8_t *>(d + at_mask) : nullptr;
    a.mask_packed = true;
    a.P = mc->P;
    a.max_iters = max_iters;
    a.R = reinterpret_cast<float *>(d + at_R);
    a.t = reinterpret_cast<float *>(d + at_t);
    a.E = E_out ? reinterpret_cast<float *>(d + at_E) : nullptr;
    a.cost0 = cost0 ? reinterpret_cast<double *>(d + at_cost0) : nullptr;
    a.cost = cost ? reinterpret_cast<double *>(d + at_cost) : nullptr;
    a.iterations = iterations ? reinterpret_cast<int32_t *>(d + at_iter) : nullptr;
    a.used = used ? reinterpret_cast<int32_t *>(d + at_used) : nullptr;
    HIP_TRY(mc, usac::launch_multi_refine(mc->stream, a));
    if (R_out) HIP_TRY(mc, hipMemcpyAsync(R_out, d + at_R, 36 * P, hipMemcpyDeviceToHost, mc->stream));
    if (t_out) HIP_TRY(mc, hipMemcpyAsync(t_out, d + at_t, 12 * P, hipMemcpyDeviceToHost, mc->stream));
    if (E_out) HIP_TRY(mc, hipMemcpyAsync(E_out, d + at_E, 36 * P, hipMemcpyDeviceToHost, mc->stream));
    if (cost0) HIP_TRY(mc, hipMemcpyAsync(cost0, d + at_cost0, 8 * P, hipMemcpyDeviceToHost, mc->stream));
    if (cost) HIP_TRY(mc, hipMemcpyAsync(cost, d + at_cost, 8 * P, hipMemcpyDeviceToHost, mc->stream));
    if (iterations) HIP_TRY(mc, hipMemcpyAsync(iterations, d + at_iter, 4 * P, hipMemcpyDeviceToHost, mc->stream));
    if (used) HIP_TRY(mc, hipMemcpyAsync(used, d + at_used, 4 * P, hipMemcpyDeviceToHost, mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    return USAC_OK;
}

void usac_multi_destroy(usac_multi *mc) {
    if (!mc) return;
    (void)hipSetDevice(mc->device);
    if (mc->stream) (void)hipStreamSynchronize(mc->stream);
    for (PinBlock *b : {&mc->pin, &mc->pol_pin, &mc->pro_pin, &mc->sprt_pin}) pin_release(*b);
    for (DevBuf *b : {&mc->growth, &mc->non_random0, &mc->non_random, &mc->grid}) b->release();
    for (DevBuf *b : {&mc->sprt_pts, &mc->sprt_idx, &mc->sprt_consts, &mc->sprt_surv, &mc->sprt_surv_n, &mc->sprt_starts})
        b->release();
    for (DevBuf *b : {&mc->pts, &mc->offs, &mc->items, &mc->samples, &mc->models, &mc->counts, &mc->sums, &mc->list,
                      &mc->list_n, &mc->out, &mc->running, &mc->mmodels, &mc->m18, &mc->mask, &mc->pol_lists,
                      &mc->pol_out, &mc->lo_state, &mc->e5_ws, &mc->thrs, &mc->lo_steps, &mc->src, &mc->kdev,
                      &mc->pose_buf, &mc->refine_buf})
        b->release();
    if (mc->stream) StreamPool::get().give_back(mc->stream);
    delete mc;
}

const char *usac_multi_last_error(const usac_multi *mc) {
    if (mc) return mc->err.c_str();
    // no context: what this thread's last usac_multi_create_device refused its input for, if it did
    return g_create_device_err.empty() ? "null context" : g_create_device_err.c_str();
}
uint32_t usac_multi_num_problems(const usac_multi *mc) { return mc ? mc->P : 0; }

// ---- per-problem thresholds (ABI 22)
int usac_multi_set_thresholds(usac_multi *mc, const float *thr) {
    if (!mc) return USAC_ERR_ARG;
    if (!thr) {
        mc->thr_host.clear();
        mc->lo_steps_iters = 0;
        return USAC_OK;
    }
    for (uint32_t p = 0; p < mc->P; p++)
        if (!(thr[p] > 0.f) || !std::isfinite(thr[p]))
            return fail(mc, USAC_ERR_ARG, "usac_multi_set_thresholds: problem " + std::to_string(p) +
                                              ": the threshold must be finite and > 0");
    // every call waits for its stream before it returns: no launch of this context reads the old values now
    HIP_TRY(mc, hipSetDevice(mc->device));
    HIP_TRY(mc, mc->thrs.reserve(sizeof(float) * (size_t)mc->P));
    HIP_TRY(mc, hipMemcpy(mc->thrs.p, thr, sizeof(float) * (size_t)mc->P, hipMemcpyHostToDevice));
    mc->thr_host.assign(thr, thr + mc->P);
    mc->lo_steps_iters = 0;  // the LO steps follow the thresholds
    return USAC_OK;
}

int usac_multi_get_thresholds(const usac_multi *mc, float *out) {
    if (!mc) return USAC_ERR_ARG;
    if (mc->thr_host.empty()) return 0;
    if (out) std::copy(mc->thr_host.begin(), mc->thr_host.end(), out);
    return 1;
}

// ---- pixel coordinates (ABI 24)
int usac_multi_set_pixel_thresholds(usac_multi *mc, const float *t_px, uint32_t n) {
    if (!mc) return USAC_ERR_ARG;
    if (mc->k1.empty())
        return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_set_pixel_thresholds: the context was not created from pixel "
                                              "coordinates (usac_multi_create_essential_pixels)");
    if (!t_px || (n != 1 && n != mc->P))
        return fail(mc, USAC_ERR_ARG, "usac_multi_set_pixel_thresholds: one tolerance, or one per problem");
    std::vector<float> thr(mc->P);
    for (uint32_t p = 0; p < mc->P; p++) {
        const float t = t_px[n == 1 ? 0 : p];
        if (!(t > 0.f) || !std::isfinite(t))
            return fail(mc, USAC_ERR_ARG, "usac_multi_set_pixel_thresholds: problem " + std::to_string(p) +
                                              ": the tolerance must be finite and > 0");
        thr[p] = usac::pixel_threshold(mc->k1.data() + 9 * (size_t)p, mc->k2.data() + 9 * (size_t)p, t);
    }
    return usac_multi_set_thresholds(mc, thr.data());  // refuses a threshold that is not finite and > 0
}

int usac_multi_pixel_models(usac_multi *mc, const float *E, float *F) {
    if (!mc) return USAC_ERR_ARG;
    if (mc->k1.empty())
        return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_pixel_models: the context was not created from pixel "
                                              "coordinates (usac_multi_create_essential_pixels)");
    if (!E || !F) return fail(mc, USAC_ERR_ARG, "usac_multi_pixel_models: NULL argument");
    for (uint32_t p = 0; p < mc->P; p++)
        usac::pixel_model(mc->k1.data() + 9 * (size_t)p, mc->k2.data() + 9 * (size_t)p, E + 9 * (size_t)p, F + 9 * (size_t)p);
    return USAC_OK;
}

int usac_multi_get_points(usac_multi *mc, float *out) {
    if (!mc) return USAC_ERR_ARG;
    if (!out) return fail(mc, USAC_ERR_ARG, "usac_multi_get_points: NULL argument");
    // every call waits for its stream before it returns: nothing of this context is in flight
    HIP_TRY(mc, hipSetDevice(mc->device));
    HIP_TRY(mc, hipMemcpy(out, mc->pts.p, sizeof(float) * 4 * (size_t)mc->n_total, hipMemcpyDeviceToHost));
    return USAC_OK;
}

int usac_multi_hypothesize_score(usac_multi *mc, const uint32_t *problems, uint32_t n_problems,
                                 const int32_t *samples, uint32_t R, const uint64_t *seeds, uint64_t first_hyp,
                                 float thr, int dlt_mode, int32_t *counts, float *sums, usac_record *best) {
    if (!mc) return USAC_ERR_ARG;
    uint32_t A = 0;
    int rc = multi_hook_args(mc, problems, n_problems, samples, R, seeds, dlt_mode, A);
    if (rc || (rc = multi_check_entries(mc, problems, A, samples, R, [](uint32_t, uint32_t) -> int { return USAC_OK; })))
        return rc;
    HIP_TRY(mc, hipSetDevice(mc->device));
    if ((rc = multi_ensure(mc, A, R, samples != nullptr)) || (rc = multi_hook_upload(mc, problems, A, samples, R, seeds)))
        return rc;
    usac::MultiRound r = multi_round(mc, A, R, first_hyp, thr, dlt_mode);
    r.samples_in = samples ? mc->samples.as<int32_t>() : nullptr;
    HIP_TRY(mc, usac::launch_multi_round(mc->stream, r));
    if ((rc = multi_hook_down(mc, A, R, counts, sums, best))) return rc;
    HIP_TRY(mc, stream_wait(mc->stream));
    return USAC_OK;
}

int usac_multi_run(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out) {
    if (!mc || !prm || !out) return USAC_ERR_ARG;
    return multi_run_uniform(mc, prm, seeds, out, nullptr, nullptr);
}

int usac_multi_inliers(usac_multi *mc, const float *models, float thr, uint8_t *mask, int32_t *counts) {
    if (!mc || !models || (!mask && !counts)) return USAC_ERR_ARG;
    HIP_TRY(mc, hipSetDevice(mc->device));
    HIP_TRY(mc, mc->mmodels.reserve(sizeof(float) * 9 * (size_t)mc->P));
    HIP_TRY(mc, mc->m18.reserve(sizeof(float) * 18 * (size_t)mc->P));
    multi_resident_end(mc, "usac_multi_inliers (it wrote another mask into the mask buffer)");
    HIP_TRY(mc, mc->mask.reserve(mc->n_total));
    HIP_TRY(mc, hipMemcpyAsync(mc->mmodels.p, models, sizeof(float) * 9 * (size_t)mc->P, hipMemcpyHostToDevice,
                               mc->stream));
    HIP_TRY(mc, usac::launch_multi_mask(mc->stream, mc->estimator, mc->pts.as<float4>(), mc->offs.as<uint32_t>(), mc->P,
                                        mc->n_total, mc->mmodels.as<float>(), thr, multi_thrs(mc), mc->m18.as<float>(),
                                        mc->mask.as<uint8_t>()));
    std::vector<uint8_t> tmp;
    if (!mask) {
        tmp.resize(mc->n_total);
        mask = tmp.data();
    }
    HIP_TRY(mc, hipMemcpyAsync(mask, mc->mask.p, mc->n_total, hipMemcpyDeviceToHost, mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    if (counts)
        for (uint32_t p = 0; p < mc->P; p++) {
            int32_t c = 0;
            for (uint32_t i = mc->offsets[p]; i < mc->offsets[p + 1]; i++) c += mask[i];
            counts[p] = c;
        }
    return USAC_OK;
}

int usac_multi_polish(usac_multi *mc, const float *models, float thr, usac_multi_polish_output *out, uint8_t *mask) {
    if (!mc || !models || !out) return USAC_ERR_ARG;
    HIP_TRY(mc, hipSetDevice(mc->device));
    HIP_TRY(mc, mc->mmodels.reserve(sizeof(float) * 9 * (size_t)mc->P));
    HIP_TRY(mc, hipMemcpyAsync(mc->mmodels.p, models, sizeof(float) * 9 * (size_t)mc->P, hipMemcpyHostToDevice,
                               mc->stream));
    return multi_polish_device(mc, mc->mmodels.as<float>(), 9, models, 9, thr, out, mask);
}

int usac_multi_run_polished(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out,
                            usac_multi_polish_output *pol, uint8_t *mask) {
    if (!mc || !prm || !out || !pol) return USAC_ERR_ARG;
    return multi_run_uniform(mc, prm, seeds, out, pol, mask);  // the run, then the polish of its final records
}

// ---- PROSAC (ABI 17)
int usac_multi_draw_samples(usac_multi *mc, const uint32_t *problems, uint32_t n_problems, uint32_t R,
                            const uint64_t *seeds, uint64_t first_hyp, const uint32_t *clock, const uint32_t *term_len,
                            int32_t *out) {
    if (!mc) return USAC_ERR_ARG;
    if (!seeds || !out || (clock && !term_len)) return fail(mc, USAC_ERR_ARG, "seeds, out and (with clock) term_len");
    if (!multi_round_ok(R)) return fail(mc, USAC_ERR_ARG, "R must be a multiple of 64 in 64..8192");
    uint32_t A = 0;
    int rc = multi_listed(mc, problems, n_problems, A);
    if (rc) return rc;
    for (uint32_t a = 0; a < A; a++) {
        const uint32_t p = problems ? problems[a] : a;
        if (p >= mc->P) return fail(mc, USAC_ERR_ARG, "problem index out of range");
        if (!clock) continue;
        const uint32_t n = mc->offsets[p + 1] - mc->offsets[p];
        if (clock[a] < 1 || clock[a] > (1u << 30) || term_len[a] < mc->m || term_len[a] > n)
            return fail(mc, USAC_ERR_ARG, "clock >= 1 and sample size <= term_len <= n_p");
    }
    HIP_TRY(mc, hipSetDevice(mc->device));
    if ((rc = multi_ensure(mc, A, R, true))) return rc;
    if (clock && (rc = multi_prosac_ensure(mc))) return rc;
    usac::MultiItem *items = multi_items_pin(mc);
    for (uint32_t a = 0; a < A; a++)
        items[a] = usac::MultiItem{problems ? problems[a] : a, clock ? clock[a] : 0u, seeds[a],
                                   clock ? term_len[a] : 0u, 0u};
    HIP_TRY(mc, hipMemcpyAsync(mc->items.p, items, sizeof(usac::MultiItem) * (size_t)A, hipMemcpyHostToDevice,
                               mc->stream));
    HIP_TRY(mc, usac::launch_multi_draw(mc->stream, mc->estimator, mc->offs.as<uint32_t>(),
                                        mc->items.as<usac::MultiItem>(), A, R, first_hyp,
                                        clock ? mc->growth.as<uint32_t>() : nullptr, nullptr, mc->samples.as<int32_t>()));
    HIP_TRY(mc, hipMemcpyAsync(out, mc->samples.p, sizeof(int32_t) * (size_t)A * R * mc->m, hipMemcpyDeviceToHost,
                               mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    return USAC_OK;
}

int usac_multi_prosac_scan(usac_multi *mc, const usac_params *prm, int reset, const float *models,
                           const uint32_t *hyp_count, const uint32_t *largest, uint32_t *bound, uint32_t *term_len,
                           uint32_t *n_cand, uint32_t *cand) {
    if (!mc || !prm || !models || !hyp_count || !largest || !bound || !term_len) return USAC_ERR_ARG;
    const uint32_t P = mc->P;
    for (uint32_t p = 0; p < P; p++)
        if (mc->offsets[p + 1] - mc->offsets[p] <= 20) return fail(mc, USAC_ERR_ARG, "PROSAC needs > 20 points per problem");
    HIP_TRY(mc, hipSetDevice(mc->device));
    int rc = multi_ensure(mc, P, 64, false);
    if (rc || (rc = multi_prosac_ensure(mc))) return rc;
    if ((reset || mc->pterm.size() != P) && (rc = multi_prosac_reset(mc, prm))) return rc;
    std::vector<usac_record> recs(P);
    usac::MultiItem *items = multi_items_pin(mc);
    for (uint32_t p = 0; p < P; p++) {
        recs[p] = usac_record{};
        recs[p].hyp_index = hyp_count[p];
        recs[p].valid = 1;
        memcpy(recs[p].model, models + 9 * (size_t)p, sizeof(recs[p].model));
        items[p] = usac::MultiItem{p, 0u, 0ull, 0u, 0u};
    }
    HIP_TRY(mc, hipMemcpyAsync(mc->items.p, items, sizeof(usac::MultiItem) * (size_t)P, hipMemcpyHostToDevice, mc->stream));
    HIP_TRY(mc, hipMemcpyAsync(mc->running.p, recs.data(), sizeof(usac_record) * (size_t)P, hipMemcpyHostToDevice,
                               mc->stream));
    HIP_TRY(mc, multi_launch_scan(mc, P, 0, prm->threshold));
    HIP_TRY(mc, stream_wait(mc->stream));
    for (uint32_t p = 0; p < P; p++) {
        bound[p] = multi_apply_candidates(mc, p, p, hyp_count[p], largest[p]);
        term_len[p] = mc->pterm[p]->terminationLength();
        if (n_cand) n_cand[p] = multi_cand_n_pin(mc)[p];
    }
    if (cand) memcpy(cand, multi_cand_pin(mc), sizeof(uint32_t) * 2 * usac::multi_cand_capacity(mc->n_total, P));
    return USAC_OK;
}

int usac_multi_run_prosac(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out,
                          usac_multi_prosac_output *pro, usac_multi_polish_output *pol, uint8_t *mask) {
    if (!mc || !prm || !out) return USAC_ERR_ARG;
    if (prm->sprt || prm->lo != USAC_LO_NONE)
        return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_run_prosac: no SPRT, no LO (LO: usac_multi_run_lo)");
    if (prm->sampler != USAC_SAMPLER_PROSAC) return fail(mc, USAC_ERR_ARG, "usac_multi_run_prosac: the PROSAC sampler");
    return multi_run_driver(mc, prm, seeds, out, MultiRunOutputs{nullptr, pro, nullptr, pol, mask});
}

// ---- LO-RANSAC (ABI 18)
int usac_lo_draw(uint64_t seed, uint64_t draw, uint32_t k, uint32_t max, int32_t *out) {
    if (!out || k < 1 || k > usac::kLoDrawMax || max > 0x7FFFFFFFu || k > max + 1) return USAC_ERR_ARG;
    usac::lo_draw(seed, draw, k, max, out);
    return USAC_OK;
}

int usac_multi_lo(usac_multi *mc, const usac_params *prm, int reset, const uint64_t *seeds, usac_record *recs,
                  usac_multi_lo_output *lo) {
    if (!mc || !prm || !recs) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_lo")) return no;
    return multi_lo_hook(mc, prm, reset, seeds, recs, lo, "usac_multi_lo");
}

int usac_multi_lo_essential(usac_multi *mc, const usac_params *prm, int reset, const uint64_t *seeds, usac_record *recs,
                            usac_multi_lo_output *lo) {
    if (!mc || !prm || !recs) return USAC_ERR_ARG;
    if (const int no = multi_only_essential(mc, "usac_multi_lo_essential", "usac_multi_lo")) return no;
    return multi_lo_hook(mc, prm, reset, seeds, recs, lo, "usac_multi_lo_essential");
}

int usac_multi_run_lo(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out,
                      usac_multi_lo_output *lo, usac_multi_prosac_output *pro, usac_multi_polish_output *pol,
                      uint8_t *mask) {
    if (!mc || !prm || !out) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_run_lo")) return no;
    int rc = multi_lo_check(mc, prm, "usac_multi_run_lo");
    if (rc) return rc;
    if (prm->sampler != USAC_SAMPLER_UNIFORM && prm->sampler != USAC_SAMPLER_PROSAC)
        return fail(mc, USAC_ERR_ARG, "usac_multi_run_lo: the uniform or the PROSAC sampler");
    return multi_run_driver(mc, prm, seeds, out, MultiRunOutputs{lo, pro, nullptr, pol, mask});
}

int usac_multi_run_lo_essential(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out,
                                usac_multi_lo_output *lo, usac_multi_prosac_output *pro, usac_multi_polish_output *pol,
                                uint8_t *mask) {
    if (!mc || !prm || !out) return USAC_ERR_ARG;
    if (const int no = multi_only_essential(mc, "usac_multi_run_lo_essential", "usac_multi_run_lo")) return no;
    int rc = multi_lo_check(mc, prm, "usac_multi_run_lo_essential");
    if (rc) return rc;
    if (prm->sampler != USAC_SAMPLER_UNIFORM && prm->sampler != USAC_SAMPLER_PROSAC)
        return fail(mc, USAC_ERR_ARG, "usac_multi_run_lo_essential: the uniform or the PROSAC sampler");
    return multi_run_driver(mc, prm, seeds, out, MultiRunOutputs{lo, pro, nullptr, pol, mask}, true);
}

// ---- SPRT (ABI 19)
int usac_multi_sprt_update(int estimator, uint32_t n_points, uint32_t m, uint32_t max_iterations,
                           usac_multi_sprt_test *hist, uint32_t *n_hist, uint32_t cap, uint32_t *last_update,
                           uint32_t *bound, uint32_t done, uint32_t head_inliers, uint32_t head_points, int improved,
                           uint32_t best_inliers, uint32_t term_bound) {
    static_assert(USAC_HOMOGRAPHY == 2 && USAC_FUNDAMENTAL == 3, "usac_host.hpp's estimator numbers");
    if (!hist || !n_hist || cap == 0 || *n_hist > cap) return USAC_ERR_ARG;
    // the state as usac_host.hpp keeps it (sprt_rounds_update: the text the run applies), and back
    std::vector<usac::Sprt::History> h(cap);
    for (uint32_t i = 0; i < *n_hist; i++) h[i] = usac::Sprt::History{hist[i].epsilon, hist[i].delta, hist[i].A, hist[i].k};
    uint32_t nh = *n_hist;
    if (usac::sprt_rounds_update(estimator, n_points, m, max_iterations, h.data(), &nh, cap, last_update, bound, done,
                                 head_inliers, head_points, improved != 0, best_inliers, term_bound))
        return USAC_ERR_ARG;
    for (uint32_t i = *n_hist; i < nh; i++) hist[i] = usac_multi_sprt_test{h[i].epsilon, h[i].delta, h[i].A, h[i].k, 0};
    *n_hist = nh;
    return USAC_OK;
}

int usac_multi_sprt_setup(usac_multi *mc, const uint32_t *pool_seeds) {
    if (!mc) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_sprt_setup")) return no;
    HIP_TRY(mc, hipSetDevice(mc->device));
    return multi_sprt_setup(mc, pool_seeds);
}

int usac_multi_hypothesize_score_sprt(usac_multi *mc, const uint32_t *problems, uint32_t n_problems,
                                      const int32_t *samples, uint32_t R, const uint64_t *seeds, uint64_t first_hyp,
                                      float thr, int dlt_mode, const double *eps_delta, int32_t *counts, float *sums,
                                      usac_record *best, usac_multi_sprt_stats *stats, uint32_t *starts) {
    if (!mc) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_hypothesize_score_sprt")) return no;
    uint32_t A = 0;
    int rc = multi_hook_args(mc, problems, n_problems, samples, R, seeds, dlt_mode, A);
    if (rc) return rc;
    double margin, climb;
    if (!multi_sprt_cert(margin, climb)) return fail(mc, USAC_ERR_ARG, "SPRT certificate: margin >= 1e-7 and 0 < climb <= 700");
    rc = multi_check_entries(mc, problems, A, samples, R, [&](uint32_t a, uint32_t) -> int {
        if (!eps_delta) return USAC_OK;
        const double e = eps_delta[2 * a], d = eps_delta[2 * a + 1];
        if ((e != 0 && !(e > 0 && e < 1)) || (d != 0 && !(d > 0 && d < 1)))
            return fail(mc, USAC_ERR_ARG, "SPRT: epsilon and delta must be in (0, 1)");
        return USAC_OK;
    });
    if (rc) return rc;
    // the tests, before any device call (delta < epsilon with the defaults filled in)
    std::vector<usac::SprtConsts> kc(A);
    for (uint32_t a = 0; a < A; a++) {
        const uint32_t p = problems ? problems[a] : a, n = mc->offsets[p + 1] - mc->offsets[p];
        const usac::SprtRounds st(mc->estimator, n, mc->m, 10000);
        const double e = eps_delta && eps_delta[2 * a] != 0 ? eps_delta[2 * a] : st.test().epsilon;
        const double d = eps_delta && eps_delta[2 * a + 1] != 0 ? eps_delta[2 * a + 1] : st.test().delta;
        if (!(d < e)) return fail(mc, USAC_ERR_ARG, "SPRT: delta must be below epsilon");
        kc[a] = multi_sprt_consts(e, d, st.thresholdA(e, d), n, margin, climb);
    }
    HIP_TRY(mc, hipSetDevice(mc->device));
    if ((rc = multi_ensure(mc, A, R, samples != nullptr)) || (rc = multi_sprt_ensure(mc, A, R, starts != nullptr)) ||
        (rc = multi_hook_upload(mc, problems, A, samples, R, seeds)))
        return rc;
    memcpy(multi_sprt_consts_pin(mc), kc.data(), sizeof(usac::SprtConsts) * (size_t)A);
    HIP_TRY(mc, hipMemcpyAsync(mc->sprt_consts.p, multi_sprt_consts_pin(mc), sizeof(usac::SprtConsts) * (size_t)A,
                               hipMemcpyHostToDevice, mc->stream));
    usac::MultiRound r = multi_round(mc, A, R, first_hyp, thr, dlt_mode);
    r.samples_in = samples ? mc->samples.as<int32_t>() : nullptr;
    const usac::MultiSprt ms = multi_sprt_args(mc, A, starts != nullptr);
    r.sprt = &ms;
    HIP_TRY(mc, usac::launch_multi_round(mc->stream, r));
    if ((rc = multi_hook_down(mc, A, R, counts, sums, best))) return rc;
    if (stats)
        HIP_TRY(mc, hipMemcpyAsync(stats, ms.stats, sizeof(usac_multi_sprt_stats) * (size_t)A, hipMemcpyDeviceToHost,
                                   mc->stream));
    if (starts)
        HIP_TRY(mc, hipMemcpyAsync(starts, mc->sprt_starts.p, sizeof(uint32_t) * (size_t)A * R * mc->spk, hipMemcpyDeviceToHost,
                                   mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    return USAC_OK;
}

int usac_multi_run_sprt(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out,
                        usac_multi_sprt_output *sprt, usac_multi_prosac_output *pro, usac_multi_polish_output *pol,
                        uint8_t *mask) {
    if (!mc || !prm || !out) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_run_sprt")) return no;
    if (prm->lo != USAC_LO_NONE)
        return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_run_sprt: no LO with SPRT (LO: usac_multi_run_lo)");
    if (!prm->sprt) return fail(mc, USAC_ERR_ARG, "usac_multi_run_sprt: params->sprt must be set");
    if (prm->sampler != USAC_SAMPLER_UNIFORM && prm->sampler != USAC_SAMPLER_PROSAC)
        return fail(mc, USAC_ERR_ARG, "usac_multi_run_sprt: the uniform or the PROSAC sampler");
    return multi_run_driver(mc, prm, seeds, out, MultiRunOutputs{nullptr, pro, sprt, pol, mask});
}

// ---- NAPSAC (ABI 20)
int usac_multi_grid(usac_multi *mc, int cell_size, uint32_t *n_cells, uint32_t *cell, uint32_t *rank, uint32_t *start,
                    int32_t *members, int32_t *eligible, uint32_t *n_eligible) {
    if (!mc) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_grid")) return no;
    const int rc = multi_grid_ensure(mc, cell_size);
    if (rc) return rc;
    const size_t N = mc->n_total, P = mc->P;
    const usac::MultiGrid g = multi_grid_args(mc);
    if (n_cells) memcpy(n_cells, mc->grid_counts.data() + P, sizeof(uint32_t) * P);
    if (n_eligible) memcpy(n_eligible, mc->grid_counts.data() + 2 * P, sizeof(uint32_t) * P);
    if (cell) HIP_TRY(mc, hipMemcpyAsync(cell, g.cell, 4 * N, hipMemcpyDeviceToHost, mc->stream));
    if (rank) HIP_TRY(mc, hipMemcpyAsync(rank, g.rank, 4 * N, hipMemcpyDeviceToHost, mc->stream));
    if (start) HIP_TRY(mc, hipMemcpyAsync(start, g.start, 4 * (N + P), hipMemcpyDeviceToHost, mc->stream));
    if (members) HIP_TRY(mc, hipMemcpyAsync(members, g.members, 4 * N, hipMemcpyDeviceToHost, mc->stream));
    if (eligible) HIP_TRY(mc, hipMemcpyAsync(eligible, g.eligible, 4 * N, hipMemcpyDeviceToHost, mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    return USAC_OK;
}

int usac_multi_draw_samples_napsac(usac_multi *mc, const uint32_t *problems, uint32_t n_problems, uint32_t R,
                                   const uint64_t *seeds, uint64_t first_hyp, int cell_size, int32_t *out) {
    if (!mc) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_draw_samples_napsac")) return no;
    if (!seeds || !out) return fail(mc, USAC_ERR_ARG, "seeds and out");
    if (cell_size <= 0) return fail(mc, USAC_ERR_ARG, "grid cell_size must be > 0");
    if (!multi_round_ok(R)) return fail(mc, USAC_ERR_ARG, "R must be a multiple of 64 in 64..8192");
    uint32_t A = 0;
    int rc = multi_listed(mc, problems, n_problems, A);
    if (rc || (rc = multi_check_entries(mc, problems, A, nullptr, R, [](uint32_t, uint32_t) -> int { return USAC_OK; })))
        return rc;
    HIP_TRY(mc, hipSetDevice(mc->device));
    if ((rc = multi_grid_ensure(mc, cell_size)) || (rc = multi_ensure(mc, A, R, true)) ||
        (rc = multi_hook_upload(mc, problems, A, nullptr, R, seeds)))
        return rc;
    const usac::MultiGrid mg = multi_grid_args(mc);
    HIP_TRY(mc, usac::launch_multi_draw(mc->stream, mc->estimator, mc->offs.as<uint32_t>(),
                                        mc->items.as<usac::MultiItem>(), A, R, first_hyp, nullptr, &mg,
                                        mc->samples.as<int32_t>()));
    HIP_TRY(mc, hipMemcpyAsync(out, mc->samples.p, sizeof(int32_t) * (size_t)A * R * mc->m, hipMemcpyDeviceToHost,
                               mc->stream));
    HIP_TRY(mc, stream_wait(mc->stream));
    return USAC_OK;
}

int usac_multi_hypothesize_score_napsac(usac_multi *mc, const uint32_t *problems, uint32_t n_problems, uint32_t R,
                                        const uint64_t *seeds, uint64_t first_hyp, float thr, int dlt_mode,
                                        int cell_size, int32_t *counts, float *sums, usac_record *best) {
    if (!mc) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_hypothesize_score_napsac")) return no;
    if (cell_size <= 0) return fail(mc, USAC_ERR_ARG, "grid cell_size must be > 0");
    uint32_t A = 0;
    int rc = multi_hook_args(mc, problems, n_problems, nullptr, R, seeds, dlt_mode, A);
    if (rc || (rc = multi_check_entries(mc, problems, A, nullptr, R, [](uint32_t, uint32_t) -> int { return USAC_OK; })))
        return rc;
    HIP_TRY(mc, hipSetDevice(mc->device));
    if ((rc = multi_grid_ensure(mc, cell_size)) || (rc = multi_ensure(mc, A, R, false)) ||
        (rc = multi_hook_upload(mc, problems, A, nullptr, R, seeds)))
        return rc;
    const usac::MultiGrid mg = multi_grid_args(mc);
    usac::MultiRound r = multi_round(mc, A, R, first_hyp, thr, dlt_mode);
    r.grid = &mg;
    HIP_TRY(mc, usac::launch_multi_round(mc->stream, r));
    if ((rc = multi_hook_down(mc, A, R, counts, sums, best))) return rc;
    HIP_TRY(mc, stream_wait(mc->stream));
    return USAC_OK;
}

int usac_multi_run_napsac(usac_multi *mc, const usac_params *prm, const uint64_t *seeds, usac_multi_output *out,
                          usac_multi_lo_output *lo, usac_multi_polish_output *pol, uint8_t *mask) {
    if (!mc || !prm || !out) return USAC_ERR_ARG;
    if (const int no = multi_no_essential(mc, "usac_multi_run_napsac")) return no;
    if (prm->sampler != USAC_SAMPLER_NAPSAC) return fail(mc, USAC_ERR_ARG, "usac_multi_run_napsac: the NAPSAC sampler");
    if (prm->neighbors != USAC_NEIGHBORS_GRID)
        return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_run_napsac: grid neighbours only (no KNN NAPSAC)");
    if (prm->cell_size <= 0) return fail(mc, USAC_ERR_ARG, "usac_multi_run_napsac: cell_size must be > 0");
    if (prm->sprt) return fail(mc, USAC_ERR_UNSUPPORTED, "usac_multi_run_napsac: no SPRT with NAPSAC");
    if (prm->lo != USAC_LO_NONE) {
        const int rc = multi_lo_check(mc, prm, "usac_multi_run_napsac");
        if (rc) return rc;
    }
    return multi_run_driver(mc, prm, seeds, out, MultiRunOutputs{prm->lo != USAC_LO_NONE ? lo : nullptr, nullptr, nullptr, pol, mask});
}

}  // extern "C"
