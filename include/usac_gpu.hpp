/*
 * usac_gpu.hpp -- C++ plugin layer over the C-ABI (usac_gpu.h), header-only, C++11.
 *
 * Mirrors the reference's plugin surface so that its callers read the same:
 *   usac_gpu::Model          usac/model.hpp:10-139 (fields, enums, setters; the cv::Mat
 *                            descriptor becomes 9 floats -- 3 for the line)
 *   usac_gpu::Score          usac/quality/quality.hpp:16-37 (bigger, copyFrom)
 *   usac_gpu::GpuEstimator   usac/estimator/estimator.hpp:14-41 (EstimateModel,
 *                            EstimateModelNonMinimalSample, LeastSquaresFitting,
 *                            SampleNumber) -- plus the batched EstimateModels
 *   usac_gpu::GpuQuality     usac/quality/quality.hpp:40-147 (init, getNumberInliers,
 *                            getInliers, static getInliers) -- plus the batched scoreModels
 *   usac_gpu::RansacOutput   usac/ransac/ransac_output.hpp:11-99 (getters)
 *   usac_gpu::Ransac         usac/ransac/ransac.hpp:18-117 + ransac.cpp:14-238 (Ransac(model,
 *                            points); run(); getRansacOutput()), the loop on the device
 *                            (usac_ransac_run), or hypothesis-sharded over ranks (runSharded)
 *   usac_gpu::Context        one usac_ctx (device, HIP stream, resident points)
 *   usac_gpu::RandomGenerator  the global glibc random() stream the samplers / SPRT share
 *   usac_gpu::Sampler        usac/sampler/sampler.hpp:11-35 (Uniform / Prosac / Napsac)
 *   usac_gpu::TerminationCriteria, ProsacTerminationCriteria
 *                            termination_criteria.hpp:16-17, prosac_termination_criteria.hpp:44-201
 *   usac_gpu::SPRT           usac/sprt.hpp:89-491 (verifyModelAndGetModelScore,
 *                            getUpperBoundIterations; replay = usac_sprt_replay)
 *   usac_gpu::LocalOptimization  local_optimization.hpp:19 (InItLORsc / InItFLORsc / GC)
 *
 * Errors: the C-ABI's negative status codes become usac_gpu::Error (code + usac_last_error);
 * USAC_ERR_NO_MODEL (-111) is the reference's exit(111) of ransac.cpp:143-147.
 * No CPU fallback: Context throws when no GPU is usable.
 */
#ifndef USAC_GPU_HPP
#define USAC_GPU_HPP

#include <array>
#include <cstdint>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "usac_gpu.h"

namespace usac_gpu {

// usac/model.hpp:10-13 (same numeric values as the C-ABI's USAC_* enums)
enum ESTIMATOR { NullE, Line2d, Homography, Fundamental, Essential };
enum SAMPLER { NullS, Uniform, ProgressiveNAPSAC, Napsac, Prosac, Evsac, ProsacNapsac };
enum NeighborsSearch { NullN, Nanoflann, Grid };
enum LocOpt { NullLO, InItLORsc, InItFLORsc, GC, IRLS };

class Error : public std::runtime_error {
public:
    int code;
    Error(int code_, const std::string &what) : std::runtime_error(what), code(code_) {}
};

// usac/quality/quality.hpp:16-37
class Score {
public:
    int inlier_number = 0;
    float score = 0;
    bool bigger(const Score *const score2) const { return bigger(*score2); }
    bool bigger(const Score &score2) const {
        if (inlier_number > score2.inlier_number) return true;
        if (inlier_number == score2.inlier_number) return score > score2.score;
        return false;
    }
    void copyFrom(const Score *const s) {
        score = s->score;
        inlier_number = s->inlier_number;
    }
};

typedef std::array<float, 9> Descriptor;

// usac/model.hpp:15-139
class Model {
public:
    float threshold = 2;
    float desired_prob = 0.95f;
    unsigned int sample_size = 0;
    unsigned int min_iterations = 20;
    unsigned int max_iterations = 10000;
    unsigned int k_nearest_neighbors = 5;
    LocOpt lo = NullLO;
    unsigned int lo_sample_size = 14;
    unsigned int lo_iterative_iterations = 4;
    unsigned int lo_inner_iterations = 20;
    unsigned int lo_threshold_multiplier = 10;
    float spatial_coherence_gc = 0.1f;
    ESTIMATOR estimator = NullE;
    SAMPLER sampler = NullS;
    bool sprt = false;
    unsigned int max_hypothesis_test_before_sprt = 20;
    NeighborsSearch neighborsType = NullN;
    int cell_size = 50;
    bool reset_random_generator = true;
    // device-side knobs (no reference counterpart)
    uint32_t seed = 1;          // srandom(seed) when reset_random_generator is false
    int dlt_mode = USAC_DLT_THIN;
    uint32_t batch = 0;         // hypotheses per device batch (0 = library default)
    int device = 0;

    Model(float threshold_, unsigned int sample_number_, float desired_prob_, unsigned int knn, ESTIMATOR estimator_,
          SAMPLER sampler_)
        : threshold(threshold_), desired_prob(desired_prob_), sample_size(sample_number_),
          k_nearest_neighbors(knn), estimator(estimator_), sampler(sampler_) {}
    explicit Model(const Model *const m) { *this = *m; }

    void ResetRandomGenerator(bool reset) { reset_random_generator = reset; }
    void setNeighborsType(NeighborsSearch t) { neighborsType = t; }
    void setCellSize(int c) { cell_size = c; }
    void setSprt(bool s) { sprt = s; }
    void setLOParametres(unsigned int lo_iterative_iters, unsigned int lo_inner_iters, unsigned int lo_thresh_mult) {
        lo_iterative_iterations = lo_iterative_iters;
        lo_inner_iterations = lo_inner_iters;
        lo_threshold_multiplier = lo_thresh_mult;
    }
    void setThreshold(float t) { threshold = t; }
    void setSampleNumber(float n) { sample_size = (unsigned int)n; }
    void setDesiredProbability(float p) { desired_prob = p; }
    void setKNearestNeighbors(int k) { k_nearest_neighbors = (unsigned int)k; }
    void setDescriptor(const float *d) { std::memcpy(descriptor.data(), d, sizeof(float) * descriptorSize()); }
    const Descriptor &returnDescriptor() const { return descriptor; }
    unsigned int descriptorSize() const { return estimator == Line2d ? 3u : 9u; }

    usac_params params() const {
        usac_params p;
        std::memset(&p, 0, sizeof(p));
        p.threshold = threshold;
        p.desired_prob = desired_prob;
        p.max_iterations = max_iterations;
        p.seed = reset_random_generator ? (uint32_t)std::random_device{}() : seed;  // ransac.cpp srand(time)
        p.dlt_mode = dlt_mode;
        p.batch = batch;
        p.sampler = (int32_t)sampler;
        p.sprt = sprt ? 1 : 0;
        p.lo = (int32_t)lo;
        p.lo_sample_size = lo_sample_size;
        p.lo_iterative_iterations = lo_iterative_iterations;
        p.lo_inner_iterations = lo_inner_iterations;
        p.lo_threshold_multiplier = lo_threshold_multiplier;
        p.cell_size = cell_size;
        p.neighbors = (int32_t)neighborsType;
        p.knn = k_nearest_neighbors;
        p.spatial_coherence_gc = spatial_coherence_gc;
        p.max_hypothesis_test_before_sprt = max_hypothesis_test_before_sprt;
        return p;
    }

private:
    Descriptor descriptor = {{0, 0, 0, 0, 0, 0, 0, 0, 0}};
};

// One device context: points resident in HBM, one HIP stream.  Not copyable.
class Context {
public:
    Context(ESTIMATOR est, const float *points, unsigned int points_size, int device = 0) : est_(est) {
        const int rc = usac_create(&ctx_, device, (int)est, points, points_size, est == Line2d ? 2u : 4u);
        if (rc != USAC_OK) {
            const std::string msg = ctx_ ? usac_last_error(ctx_) : "usac_create failed";
            if (ctx_) usac_destroy(ctx_);
            ctx_ = nullptr;
            throw Error(rc, msg);
        }
    }
    ~Context() {
        if (ctx_) usac_destroy(ctx_);
    }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;

    usac_ctx *get() const { return ctx_; }
    ESTIMATOR estimator() const { return est_; }
    unsigned int pointsSize() const { return usac_num_points(ctx_); }
    unsigned int sampleSize() const { return usac_sample_size(ctx_); }
    // model slots per minimal sample (the 7-point solver returns up to 3 F)
    unsigned int modelSlots() const { return est_ == Fundamental ? 3u : 1u; }
    void check(int rc, const char *what) const {
        if (rc != USAC_OK) throw Error(rc, std::string(what) + ": " + usac_last_error(ctx_));
    }

private:
    usac_ctx *ctx_ = nullptr;
    ESTIMATOR est_;
};

// usac/estimator/estimator.hpp:14-41 on the device
class GpuEstimator {
public:
    explicit GpuEstimator(Context &ctx) : ctx_(ctx) {}
    virtual ~GpuEstimator() = default;

    // minimal model estimation: appends the sample's valid models, returns their number
    unsigned int EstimateModel(const int *const sample, std::vector<Descriptor> &models) {
        const unsigned int S = ctx_.modelSlots();
        std::vector<float> out(9 * S, 0.f);
        int32_t nm = 0;
        ctx_.check(usac_estimate_models(ctx_.get(), sample, 1, out.data(), &nm), "EstimateModel");
        for (int j = 0; j < nm; j++) {
            Descriptor d;
            std::memcpy(d.data(), &out[9 * j], sizeof(float) * 9);
            models.push_back(d);
        }
        return (unsigned int)nm;
    }
    // batched: samples B x m -> models B x slots x 9, n_models[B]
    void EstimateModels(const int *const samples, unsigned int B, float *models, int *n_models) {
        ctx_.check(usac_estimate_models(ctx_.get(), samples, B, models, n_models), "EstimateModels");
    }
    bool EstimateModelNonMinimalSample(const int *const sample, unsigned int sample_size, Descriptor &model) {
        const int rc = usac_nonminimal(ctx_.get(), sample, sample_size, model.data());
        if (rc == USAC_ERR_NO_MODEL) return false;
        ctx_.check(rc, "EstimateModelNonMinimalSample");
        return true;
    }
    // the weighted overload (estimator.hpp:26): weights[point index], homography / fundamental
    bool EstimateModelNonMinimalSample(const int *const sample, unsigned int sample_size, const float *const weights,
                                       Descriptor &model) {
        const int rc = usac_lsq_fit(ctx_.get(), sample, sample_size, weights, model.data());
        if (rc == USAC_ERR_NO_MODEL) return false;
        ctx_.check(rc, "EstimateModelNonMinimalSample(weights)");
        return true;
    }
    bool LeastSquaresFitting(const int *const sample, unsigned int sample_size, Descriptor &model) {
        return EstimateModelNonMinimalSample(sample, sample_size, model);
    }
    int SampleNumber() const { return (int)ctx_.sampleSize(); }
    Context &context() { return ctx_; }

private:
    Context &ctx_;
};

// usac/quality/quality.hpp:40-147 on the device: counts exact, Σerr the reference's
// sequential fp32 sum (quality.hpp:89-96), inliers ascending.
class GpuQuality {
protected:
    unsigned int points_size = 0;
    float threshold = 0;
    GpuEstimator *estimator = nullptr;
    bool isinit = false;

public:
    bool isInit() const { return isinit; }
    void init(unsigned int points_size_, float threshold_, GpuEstimator *estimator_) {
        points_size = points_size_;
        threshold = threshold_;
        estimator = estimator_;
        isinit = true;
    }
    // `parallel` is accepted for signature parity; the device path is always parallel
    void getNumberInliers(Score *score, const float *model, float thr = 0, bool get_inliers = false,
                          int *inliers = nullptr, bool /*parallel*/ = false) {
        if (thr == 0) thr = threshold;
        float m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        std::memcpy(m, model, sizeof(float) * modelFloats());
        Context &c = estimator->context();
        if (get_inliers) {
            uint32_t n = 0;
            c.check(usac_get_inliers(c.get(), m, thr, inliers, &n, &score->score), "getNumberInliers");
            score->inlier_number = (int)n;
        } else {
            c.check(usac_score_models(c.get(), m, 1, thr, &score->inlier_number, &score->score), "getNumberInliers");
        }
    }
    void getNumberInliers(Score *score, const Descriptor &model, float thr = 0, bool get_inliers = false,
                          int *inliers = nullptr) {
        getNumberInliers(score, model.data(), thr, get_inliers, inliers);
    }
    // batched getNumberInliers over n models (n x 9 floats)
    void scoreModels(const float *models, unsigned int n, float thr, int *counts, float *sums) {
        Context &c = estimator->context();
        c.check(usac_score_models(c.get(), models, n, thr == 0 ? threshold : thr, counts, sums), "scoreModels");
    }
    void getInliers(const float *model, int *inliers) {
        Score s;
        getNumberInliers(&s, model, threshold, true, inliers);
    }
    static void getInliers(GpuEstimator *est, const Descriptor &model, float thr, unsigned int points_size,
                           std::vector<int> &inliers) {
        inliers.assign(points_size, 0);
        uint32_t n = 0;
        float sum = 0;
        Context &c = est->context();
        c.check(usac_get_inliers(c.get(), model.data(), thr, inliers.data(), &n, &sum), "getInliers");
        inliers.resize(n);
    }

private:
    unsigned int modelFloats() const { return estimator->context().estimator() == Line2d ? 3u : 9u; }
};

// ---- the stateful plugins (usac_gpu.h ABI 11): what a caller keeping its own loop swaps in ----

// The reference's global glibc random() stream (srand(seed)): UniformSampler / NapsacSampler draw
// from it and the SPRT ctor shuffles its pool with it (uniform_sampler.hpp:22-54, sprt.hpp:93-104).
class RandomGenerator {
public:
    explicit RandomGenerator(uint32_t seed) {
        if (usac_random_create(seed, &h_) != USAC_OK) throw Error(USAC_ERR_ARG, "usac_random_create");
    }
    ~RandomGenerator() { usac_random_destroy(h_); }
    RandomGenerator(const RandomGenerator &) = delete;
    RandomGenerator &operator=(const RandomGenerator &) = delete;
    uint32_t next() { return usac_random_next(h_); }
    usac_random *get() const { return h_; }

private:
    usac_random *h_ = nullptr;
};

// usac/sampler/sampler.hpp:11-35, built as initSampler builds it for model.sampler: UniformSampler
// (persistent pool on rng), ProsacSampler (mt19937 seeded with model.seed), NapsacSampler (grid or KNN
// neighbours built on the device, on rng)
class Sampler {
public:
    Sampler(Context &ctx, const Model &model, RandomGenerator *rng) : ctx_(ctx) {
        const usac_params p = model.params();
        ctx_.check(usac_sampler_create(ctx_.get(), &p, rng ? rng->get() : nullptr, &h_), "Sampler");
    }
    virtual ~Sampler() { usac_sampler_destroy(h_); }
    Sampler(const Sampler &) = delete;
    Sampler &operator=(const Sampler &) = delete;
    void generateSample(int *sample) { ctx_.check(usac_sampler_generate(h_, sample), "generateSample"); }
    // count samples in a row (count x m; each row starts from the previous one, as the reused array)
    void generateSamples(unsigned int count, int *samples) {
        ctx_.check(usac_sampler_generate_batch(h_, count, samples), "generateSamples");
    }
    unsigned int getNumberOfIterations() const {
        uint64_t d = 0;
        usac_sampler_state(h_, &d, nullptr, nullptr);
        return (unsigned int)d;
    }
    bool isInit() const { return h_ != nullptr; }
    usac_sampler *get() const { return h_; }

private:
    Context &ctx_;
    usac_sampler *h_ = nullptr;
};

// usac/termination_criteria/termination_criteria.hpp:16-17 (StandardTerminationCriteria)
class TerminationCriteria {
public:
    TerminationCriteria(Context &ctx, const Model &model, Sampler *prosac_sampler = nullptr) : ctx_(ctx) {
        const usac_params p = model.params();
        ctx_.check(usac_termination_create(ctx_.get(), &p, prosac_sampler ? prosac_sampler->get() : nullptr, &h_),
                   "TerminationCriteria");
    }
    virtual ~TerminationCriteria() { usac_termination_destroy(h_); }
    TerminationCriteria(const TerminationCriteria &) = delete;
    TerminationCriteria &operator=(const TerminationCriteria &) = delete;
    unsigned int getUpBoundIterations(unsigned int inlier_size) { return usac_termination_bound(h_, inlier_size, 0); }
    unsigned int getUpBoundIterations(unsigned int inlier_size, unsigned int points_size) {
        return usac_termination_bound(h_, inlier_size, points_size);
    }

protected:
    Context &ctx_;
    usac_termination *h_ = nullptr;
};

// usac/termination_criteria/prosac_termination_criteria.hpp:44-201, linked to its PROSAC sampler
class ProsacTerminationCriteria : public TerminationCriteria {
public:
    ProsacTerminationCriteria(Context &ctx, const Model &model, Sampler &prosac_sampler)
        : TerminationCriteria(ctx, model, &prosac_sampler), termination_length(ctx.pointsSize()) {}
    using TerminationCriteria::getUpBoundIterations;
    // getUpBoundIterations(hypCount, model): the model's inliers over the quality-sorted points
    unsigned int getUpBoundIterations(unsigned int hypCount, const Descriptor &model) {
        uint32_t max_samples = 0;
        ctx_.check(usac_prosac_termination(h_, hypCount, model.data(), &max_samples, &termination_length),
                   "ProsacTerminationCriteria::getUpBoundIterations");
        return max_samples;
    }
    unsigned int *getStoppingLength() { return &termination_length; }

private:
    unsigned int termination_length;
};

// usac/sprt.hpp:89-491
class SPRT {
public:
    SPRT(Context &ctx, const Model &model, RandomGenerator &rng) : ctx_(ctx) {
        const usac_params p = model.params();
        ctx_.check(usac_sprt_create(ctx_.get(), &p, rng.get(), &h_), "SPRT");
    }
    ~SPRT() { usac_sprt_destroy(h_); }
    SPRT(const SPRT &) = delete;
    SPRT &operator=(const SPRT &) = delete;
    // verifyModelAndGetModelScore(model, current_hypothese, maximum_score, score) (sprt.hpp:191-317)
    bool verifyModelAndGetModelScore(const Descriptor &model, int current_hypothese, unsigned int maximum_score,
                                     Score *score) {
        int32_t good = 0;
        ctx_.check(usac_sprt_verify(h_, model.data(), current_hypothese, maximum_score, &good, &score->inlier_number,
                                    &score->score),
                   "SPRT::verifyModelAndGetModelScore");
        return good != 0;
    }
    unsigned int getUpperBoundIterations(int inlier_size) { return usac_sprt_upper_bound(h_, (uint32_t)inlier_size); }
    // the batch form of the loop body (usac_sprt_replay): models B x slots x 9, n_models[B]
    bool replay(const float *models, const int *n_models, unsigned int B, usac_sprt_state &state) {
        ctx_.check(usac_sprt_replay(h_, models, n_models, B, &state), "SPRT::replay");
        return state.found != 0;
    }
    unsigned int histories() const {
        uint32_t h = 0;
        usac_sprt_stats(h_, &h, nullptr);
        return h;
    }

private:
    Context &ctx_;
    usac_sprt *h_ = nullptr;
};

// usac/local_optimization/local_optimization.hpp:19, built as initLocalOptimization builds it for
// model.lo (InItLORsc / InItFLORsc: inner + iterative LO-RANSAC; GC: graph cut)
class LocalOptimization {
public:
    LocalOptimization(Context &ctx, const Model &model) : ctx_(ctx) {
        const usac_params p = model.params();
        ctx_.check(usac_lo_create(ctx_.get(), &p, &h_), "LocalOptimization");
    }
    ~LocalOptimization() { usac_lo_destroy(h_); }
    LocalOptimization(const LocalOptimization &) = delete;
    LocalOptimization &operator=(const LocalOptimization &) = delete;
    void GetModelScore(Model *best_model, Score *best_score) {
        Descriptor d = best_model->returnDescriptor();
        ctx_.check(usac_lo_get_model_score(h_, d.data(), &best_score->inlier_number, &best_score->score),
                   "LocalOptimization::GetModelScore");
        best_model->setDescriptor(d.data());
    }
    // (lo_inner_iters, lo_iterative_iters) -- GC: (gc_iterations, labellings)
    void iters(unsigned int &inner, unsigned int &iterative) const {
        uint32_t a = 0, b = 0;
        usac_lo_iters(h_, &a, &b);
        inner = a;
        iterative = b;
    }

private:
    Context &ctx_;
    usac_lo *h_ = nullptr;
};

// usac/ransac/ransac_output.hpp:11-99
class RansacOutput {
public:
    RansacOutput(const Model &model_, const usac_run_output &raw_, std::vector<int> inliers_,
                 std::vector<usac_record> records_)
        : model(model_), raw(raw_), inliers(std::move(inliers_)), records(std::move(records_)) {
        model.setDescriptor(raw.model);
        const bool gc = model_.lo == GC;
        lo_inner_iters = gc ? 0u : raw.lo_inner_iters;
        lo_iterative_iters = gc ? 0u : raw.lo_iterative_iters;
        gc_iters = gc ? raw.lo_inner_iters : 0u;
    }
    std::vector<int> getInliers() const { return inliers; }
    long getTimeMicroSeconds() const { return (long)raw.time_us; }
    unsigned int getNumberOfInliers() const { return (unsigned int)raw.inliers; }
    unsigned int getNumberOfMainIterations() const { return raw.iters; }
    unsigned int getLOIters() const { return lo_inner_iters + lo_iterative_iters + gc_iters; }
    unsigned int getLOInnerIters() const { return lo_inner_iters; }
    unsigned int getLOIterativeIters() const { return lo_iterative_iters; }
    unsigned int getGCIters() const { return gc_iters; }
    const Model *getModel() const { return &model; }
    // beyond the reference: the C-ABI's counters and the best-score updates in loop order
    const usac_run_output &getRaw() const { return raw; }
    const std::vector<usac_record> &getRecords() const { return records; }

private:
    Model model;
    usac_run_output raw;
    std::vector<int> inliers;
    std::vector<usac_record> records;
    unsigned int lo_inner_iters, lo_iterative_iters, gc_iters;
};

// usac/ransac/ransac.hpp:18-117: Ransac(model, points); run(); getRansacOutput().
class Ransac {
public:
    Ransac(Model *model_, const float *points, unsigned int points_size_)
        : model(model_), points_size(points_size_),
          own_(new Context(model_->estimator, points, points_size_, model_->device)), ctx(own_) {}
    // run on an existing context over the same points (e.g. the one holding the RCCL communicator)
    Ransac(Model *model_, Context &ctx_) : model(model_), points_size(ctx_.pointsSize()), ctx(&ctx_) {}
    ~Ransac() {
        delete out_;
        delete own_;
    }
    Ransac(const Ransac &) = delete;
    Ransac &operator=(const Ransac &) = delete;

    void run(uint32_t rec_cap = 4096) { runImpl(1, 0, nullptr, nullptr, false, rec_cap); }
    // hypothesis-sharded (usac_ransac_run_sharded): gather == nullptr -> RCCL on the context's
    // communicator (usac_comm_init); every rank's output equals run()'s
    void runSharded(int nranks, int rank, usac_allgather_fn gather, void *user, uint32_t rec_cap = 4096) {
        runImpl(nranks, rank, gather, user, true, rec_cap);
    }
    RansacOutput *getRansacOutput() { return out_; }
    Context &context() { return *ctx; }

private:
    void runImpl(int nranks, int rank, usac_allgather_fn gather, void *user, bool sharded, uint32_t rec_cap) {
        usac_params p = model->params();
        usac_run_output raw;
        std::memset(&raw, 0, sizeof(raw));
        std::vector<int> inl(points_size);
        std::vector<usac_record> recs(rec_cap);
        const int rc = sharded ? usac_ransac_run_sharded(ctx->get(), &p, nranks, rank, gather, user, &raw, inl.data(),
                                                         recs.data(), rec_cap)
                               : usac_ransac_run(ctx->get(), &p, &raw, inl.data(), recs.data(), rec_cap);
        ctx->check(rc, "Ransac::run");
        inl.resize((size_t)raw.inliers);
        recs.resize(raw.n_records < (int32_t)rec_cap ? (size_t)raw.n_records : rec_cap);
        delete out_;
        out_ = new RansacOutput(*model, raw, std::move(inl), std::move(recs));
    }

    Model *model;
    unsigned int points_size;
    Context *own_ = nullptr;
    Context *ctx;
    RansacOutput *out_ = nullptr;
};

// P independent two-view problems of one estimator (Homography / Fundamental, or Essential through
// MultiContext::essential, or MultiContext::essentialPixels from pixel coordinates) run together (usac_multi_*, ABI 15): points concatenated, offsets[P + 1]; sample, hypothesis and inlier indices
// are local to each problem, and every per-problem result equals a Context over that problem's
// points bit for bit.  Not copyable.
class MultiContext {
public:
    // one problem's round outputs: counts / sums of R * modelSlots() slots, and the round's best
    struct Round {
        std::vector<int32_t> counts;
        std::vector<float> sums;
        std::vector<usac_record> best;
    };

    MultiContext(ESTIMATOR est, const float *points, const std::vector<uint32_t> &offsets, int device = 0)
        : est_(est), offsets_(offsets) {
        const uint32_t P = offsets.empty() ? 0u : (uint32_t)(offsets.size() - 1);
        const int rc = usac_multi_create(&mc_, device, (int)est, points, offsets.data(), P);
        if (rc != USAC_OK) throw Error(rc, "usac_multi_create failed");
    }
    // P essential-matrix problems (usac_multi_create_essential, ABI 21): points are calibrated
    // coordinates (K^-1 x), 5-point samples, one model slot per sample.  The constructor keeps
    // refusing Essential.  No LO, SPRT or NAPSAC: those members throw USAC_ERR_UNSUPPORTED.
    static MultiContext essential(const float *points, const std::vector<uint32_t> &offsets, int device = 0) {
        MultiContext mc(offsets);
        const uint32_t P = offsets.empty() ? 0u : (uint32_t)(offsets.size() - 1);
        const int rc = usac_multi_create_essential(&mc.mc_, device, points, offsets.data(), P);
        if (rc != USAC_OK) throw Error(rc, "usac_multi_create_essential failed");
        return mc;
    }
    // essential() from pixel coordinates (usac_multi_create_essential_pixels, ABI 24): rows (u1, v1, u2, v2) in
    // pixels, K1 / K2: P x 9 row-major intrinsics fx s cx 0 fy cy 0 0 1 of view 1 / view 2 (K2 empty: K1 for
    // both).  The device converts the rows in place -- y = (v - cy) / fy, x = ((u - cx) - s * y) / fx in fp32 --
    // and every member then works as on essential() over those rows (points() returns them).
    static MultiContext essentialPixels(const float *points_px, const std::vector<uint32_t> &offsets,
                                        const std::vector<float> &K1, const std::vector<float> &K2 = std::vector<float>(),
                                        int device = 0) {
        MultiContext mc(offsets);
        const uint32_t P = offsets.empty() ? 0u : (uint32_t)(offsets.size() - 1);
        if (K1.size() != 9 * (size_t)P || (!K2.empty() && K2.size() != 9 * (size_t)P))
            throw Error(USAC_ERR_ARG, "essentialPixels: P x 9 intrinsics per view");
        const int rc = usac_multi_create_essential_pixels(&mc.mc_, device, points_px, offsets.data(), P, K1.data(),
                                                          K2.empty() ? nullptr : K2.data());
        if (rc != USAC_OK) throw Error(rc, "usac_multi_create_essential_pixels failed");
        return mc;
    }
    // P problems from padded device memory (usac_multi_create_device, ABI 25): in holds device pointers of
    // `device` in one of its two forms (rows with valid / counts, or kpts0 / kpts1 / match), K1 / K2 on the host
    // (Essential only) and the stream (a hipStream_t as void *) that orders the producer's writes.  The device
    // packs the kept rows in ascending column order; every member then works as on a context over them
    // (offsets() and points() return what it holds).  Throws with the library's message, which names the
    // argument or the first problem it refuses.
    static MultiContext fromDevice(int estimator, const usac_multi_device_input &in, int device = 0) {
        MultiContext mc((std::vector<uint32_t>()));
        mc.est_ = (ESTIMATOR)estimator;
        const int rc = usac_multi_create_device(&mc.mc_, device, estimator, &in);
        if (rc != USAC_OK) throw Error(rc, usac_multi_last_error(nullptr));
        mc.offsets_.resize((size_t)in.P + 1);
        mc.n_max_ = in.n_max;
        mc.check(usac_multi_get_offsets(mc.mc_, mc.offsets_.data()), "MultiContext::fromDevice");
        return mc;
    }
    // fromDevice with every problem's kept rows sorted by a score per column, the better first
    // (usac_multi_create_device_sorted, ABI 26; the rule: usac_gpu.h): order.scores is P x n_max fp32 of device
    // memory, read on in.stream.  What runProsac expects of its input.  Ownership as fromDevice's: the context
    // holds its own copy when the call returns; source() then returns the sorted order.
    static MultiContext fromDeviceSorted(int estimator, const usac_multi_device_input &in,
                                         const usac_multi_device_order &order, int device = 0) {
        MultiContext mc((std::vector<uint32_t>()));
        mc.est_ = (ESTIMATOR)estimator;
        const int rc = usac_multi_create_device_sorted(&mc.mc_, device, estimator, &in, &order);
        if (rc != USAC_OK) throw Error(rc, usac_multi_last_error(nullptr));
        mc.offsets_.resize((size_t)in.P + 1);
        mc.n_max_ = in.n_max;
        mc.check(usac_multi_get_offsets(mc.mc_, mc.offsets_.data()), "MultiContext::fromDeviceSorted");
        return mc;
    }
    ~MultiContext() {
        if (mc_) usac_multi_destroy(mc_);
    }
    MultiContext(const MultiContext &) = delete;
    MultiContext &operator=(const MultiContext &) = delete;
    MultiContext(MultiContext &&o) : mc_(o.mc_), est_(o.est_), offsets_(std::move(o.offsets_)), n_max_(o.n_max_) {
        o.mc_ = nullptr;
    }

    usac_multi *get() const { return mc_; }
    unsigned int problems() const { return usac_multi_num_problems(mc_); }
    unsigned int sampleSize() const { return est_ == Fundamental ? 7u : est_ == Essential ? 5u : 4u; }
    unsigned int modelSlots() const { return est_ == Fundamental ? 3u : 1u; }
    unsigned int pointsSize(unsigned int p) const { return offsets_[p + 1] - offsets_[p]; }
    void check(int rc, const char *what) const {
        if (rc != USAC_OK) throw Error(rc, std::string(what) + ": " + usac_multi_last_error(mc_));
    }

    // usac_multi_set_thresholds (ABI 22): one inlier threshold per problem, in the units of its own
    // coordinates.  While set, every member below that takes a threshold (thr, or the model's) uses
    // problem p's value and ignores its own; they persist until clear_thresholds().  Throws
    // USAC_ERR_ARG (nothing changed) for a wrong length or a value that is not finite and > 0.
    void set_thresholds(const std::vector<float> &thr) const {
        if (thr.size() != problems()) throw Error(USAC_ERR_ARG, "set_thresholds: one threshold per problem");
        check(usac_multi_set_thresholds(mc_, thr.data()), "MultiContext::set_thresholds");
    }
    void clear_thresholds() const { check(usac_multi_set_thresholds(mc_, nullptr), "MultiContext::clear_thresholds"); }
    // the thresholds in effect; empty: none
    std::vector<float> thresholds() const {
        std::vector<float> out(problems());
        const int rc = usac_multi_get_thresholds(mc_, out.data());
        if (rc < 0) check(rc, "MultiContext::thresholds");
        if (rc == 0) out.clear();
        return out;
    }

    // usac_multi_set_pixel_thresholds (ABI 24, a context from essentialPixels): one pixel tolerance for all
    // problems or one each; problem p's threshold becomes (t / f_p)^2, f_p the mean of its four focal lengths,
    // installed as by set_thresholds (thresholds() shows the values).  Throws USAC_ERR_ARG (nothing changed) for
    // a wrong length or a tolerance that is not finite and > 0, USAC_ERR_UNSUPPORTED on any other context.
    void setPixelThresholds(const std::vector<float> &t_px) const {
        check(usac_multi_set_pixel_thresholds(mc_, t_px.data(), (uint32_t)t_px.size()), "MultiContext::setPixelThresholds");
    }
    void setPixelThresholds(float t_px) const { setPixelThresholds(std::vector<float>(1, t_px)); }
    // usac_multi_pixel_models (ABI 24, a context from essentialPixels): E, P x 9 -> F_p = K2_p^-T E_p K1_p^-1,
    // fp64 on the host, not normalised
    std::vector<float> pixelModels(const std::vector<float> &E) const {
        if (E.size() != 9 * (size_t)problems()) throw Error(USAC_ERR_ARG, "pixelModels: P x 9 values");
        std::vector<float> F(E.size());
        check(usac_multi_pixel_models(mc_, E.data(), F.data()), "MultiContext::pixelModels");
        return F;
    }
    // usac_multi_get_points (ABI 24): the N_total x 4 rows resident on the device
    std::vector<float> points() const {
        std::vector<float> out(4 * (size_t)(offsets_.empty() ? 0u : offsets_.back()));
        check(usac_multi_get_points(mc_, out.data()), "MultiContext::points");
        return out;
    }

    // the context's offsets[P + 1], and the padded width of a context from fromDevice (else 0)
    const std::vector<uint32_t> &offsets() const { return offsets_; }
    unsigned int paddedWidth() const { return n_max_; }
    // usac_multi_get_source (ABI 25, a context from fromDevice / fromDeviceSorted): per packed row the column of
    // the padded input it came from, ascending within a problem (fromDeviceSorted: in quality order).  Throws
    // USAC_ERR_UNSUPPORTED on any other context.
    std::vector<uint32_t> source() const {
        std::vector<uint32_t> out(offsets_.empty() ? 0u : offsets_.back());
        check(usac_multi_get_source(mc_, out.empty() ? nullptr : out.data()), "MultiContext::source");
        return out;
    }
    // usac_multi_padded_mask (ABI 25, a context from fromDevice): mask, N_total bytes as inliers / polish / a
    // polished run wrote them, scattered into d_out, P x paddedWidth() bytes of device memory, zero wherever no
    // packed row came from; enqueued on stream (a hipStream_t as void *) and waited for
    void paddedMask(const std::vector<uint8_t> &mask, uint8_t *d_out, void *stream = nullptr) const {
        if (mask.size() != (offsets_.empty() ? 0u : offsets_.back()))
            throw Error(USAC_ERR_ARG, "paddedMask: N_total mask bytes");
        check(usac_multi_padded_mask(mc_, mask.data(), d_out, stream), "MultiContext::paddedMask");
    }
    // usac_multi_set_resident (ABI 27): while on, a polishing call given no host mask still leaves its mask on
    // the device for exportDevice, and nothing N_total-sized comes down
    void setResident(bool on) const { check(usac_multi_set_resident(mc_, on ? 1 : 0), "MultiContext::setResident"); }
    // usac_multi_export_device (ABI 27): the result of the last polishing call (polish, runPolished, ...) written
    // into the device memory o names -- models, counts, statuses, the P x n_max mask, the inliers' columns padded
    // with -1, pixel-space models -- by one launch on o.stream, which the call waits for.  Every pointer of o is
    // nullable; o.n_max is paddedWidth() on a context from fromDevice, any width >= the largest problem on one
    // from the host (columns are then local indices).  Throws USAC_ERR_UNSUPPORTED when no polishing call's
    // result is resident any more (the message names what ended it), USAC_ERR_ARG for a pointer that is not
    // device memory of the context's device, misaligned or too short.
    void exportDevice(const usac_multi_device_output &o) const {
        check(usac_multi_export_device(mc_, &o), "MultiContext::exportDevice");
    }
    // usac_multi_pose_device (ABI 28, an essential context): the relative pose of every problem's polished model
    // -- of the four [R | t] of E the one with the most inliers in front of both cameras -- written into the
    // device memory o names by one launch on o.stream, which the call waits for: R (P x 9, row-major), t (P x 3,
    // |t| = 1), the count in front, the choice (0..3, -1: none) and the P x n_max mask of the rows counted.
    // Every pointer of o is nullable; o.n_max as exportDevice's.  It reads the resident result of the last
    // polishing call and leaves it as it is; it throws what exportDevice throws, and USAC_ERR_UNSUPPORTED on a
    // homography or fundamental context.
    void poseDevice(const usac_multi_pose_output &o) const {
        check(usac_multi_pose_device(mc_, &o), "MultiContext::poseDevice");
    }
    // usac_multi_pose (ABI 28): the same choice for the caller's own models (P x 9) and mask (N_total bytes over
    // the packed rows; empty: every row), into host vectors; front_mask is N_total bytes in packed-row order
    struct Pose {
        std::vector<float> R, t;
        std::vector<int32_t> front, choice;
        std::vector<uint8_t> front_mask;
    };
    Pose pose(const std::vector<float> &E, const std::vector<uint8_t> &mask = std::vector<uint8_t>()) const {
        const size_t P = offsets_.empty() ? 0u : offsets_.size() - 1, n = offsets_.empty() ? 0u : offsets_.back();
        if (E.size() != 9 * P) throw Error(USAC_ERR_ARG, "pose: P x 9 model values");
        if (!mask.empty() && mask.size() != n) throw Error(USAC_ERR_ARG, "pose: N_total mask bytes, or none");
        Pose r;
        r.R.resize(9 * P);
        r.t.resize(3 * P);
        r.front.resize(P);
        r.choice.resize(P);
        r.front_mask.resize(n);
        check(usac_multi_pose(mc_, E.data(), mask.empty() ? nullptr : mask.data(), r.R.data(), r.t.data(), r.front.data(),
                              r.choice.data(), r.front_mask.data()), "MultiContext::pose");
        return r;
    }
    // usac_multi_refine_pose_device (ABI 29, an essential context): the poses o.R_in (P x 9) and o.t_in (P x 3) in
    // device memory refined by up to o.max_iters (0..100) Levenberg-Marquardt trial steps over the Sampson
    // distances of the rows o.mask_in marks (P x n_max bytes at source columns, poseDevice's front_mask; NULL: the
    // resident inlier mask), by one launch on o.stream, which the call waits for: R, t, E = [t]x R, the cost at the
    // start and at the output (doubles), the trial steps evaluated (-1: the problem was skipped) and the rows used.
    // Every output pointer of o is nullable; o.R may be o.R_in and o.t may be o.t_in.  It reads the resident result
    // of the last polishing call and leaves it as it is; it throws what poseDevice throws.
    void refinePoseDevice(const usac_multi_refine_io &o) const {
        check(usac_multi_refine_pose_device(mc_, &o), "MultiContext::refinePoseDevice");
    }
    // usac_multi_refine_pose (ABI 29): the same refinement of the caller's own poses (R P x 9, t P x 3) over the
    // mask (N_total bytes over the packed rows; empty: every row), into host vectors
    struct Refined {
        std::vector<float> R, t, E;
        std::vector<double> cost0, cost;
        std::vector<int32_t> iterations, used;
    };
    Refined refinePose(const std::vector<float> &R, const std::vector<float> &t,
                       const std::vector<uint8_t> &mask = std::vector<uint8_t>(), uint32_t max_iters = 10) const {
        const size_t P = offsets_.empty() ? 0u : offsets_.size() - 1, n = offsets_.empty() ? 0u : offsets_.back();
        if (R.size() != 9 * P || t.size() != 3 * P) throw Error(USAC_ERR_ARG, "refinePose: P x 9 and P x 3 pose values");
        if (!mask.empty() && mask.size() != n) throw Error(USAC_ERR_ARG, "refinePose: N_total mask bytes, or none");
        Refined r;
        r.R.resize(9 * P);
        r.t.resize(3 * P);
        r.E.resize(9 * P);
        r.cost0.resize(P);
        r.cost.resize(P);
        r.iterations.resize(P);
        r.used.resize(P);
        check(usac_multi_refine_pose(mc_, R.data(), t.data(), mask.empty() ? nullptr : mask.data(), max_iters, r.R.data(),
                                     r.t.data(), r.E.data(), r.cost0.data(), r.cost.data(), r.iterations.data(),
                                     r.used.data()), "MultiContext::refinePose");
        return r;
    }

    // one round of R hypotheses (a multiple of 64 in 64..8192) for the listed problems (empty: all,
    // in order), device sampler keyed by seeds[i] for problems[i]; with per_hypothesis the counts
    // and sums of every slot come back too
    Round hypothesizeScore(uint32_t R, const std::vector<uint64_t> &seeds, uint64_t first_hyp, float thr,
                           const std::vector<uint32_t> &active = std::vector<uint32_t>(),
                           int dlt_mode = USAC_DLT_THIN, bool per_hypothesis = true) const {
        const uint32_t A = active.empty() ? problems() : (uint32_t)active.size();
        if (seeds.size() != A) throw Error(USAC_ERR_ARG, "hypothesizeScore: one seed per listed problem");
        Round out;
        out.best.resize(A);
        if (per_hypothesis) {
            out.counts.resize((size_t)A * R * modelSlots());
            out.sums.resize(out.counts.size());
        }
        check(usac_multi_hypothesize_score(mc_, active.empty() ? nullptr : active.data(), A, nullptr, R, seeds.data(),
                                           first_hyp, thr, dlt_mode, per_hypothesis ? out.counts.data() : nullptr,
                                           per_hypothesis ? out.sums.data() : nullptr, out.best.data()),
              "MultiContext::hypothesizeScore");
        return out;
    }

    // usac_multi_run: batch-granular RANSAC with the standard termination criterion (uniform device
    // sampler; no SPRT / LO; the polish: runPolished); seeds empty: model.seed + p
    std::vector<usac_multi_output> run(const Model &model, const std::vector<uint64_t> &seeds = std::vector<uint64_t>()) const {
        usac_params p = model.params();
        p.seed = model.seed;
        if (!seeds.empty() && seeds.size() != problems()) throw Error(USAC_ERR_ARG, "run: one seed per problem");
        std::vector<usac_multi_output> out(problems());
        check(usac_multi_run(mc_, &p, seeds.empty() ? nullptr : seeds.data(), out.data()), "MultiContext::run");
        return out;
    }

    // ascending inlier indices (local to each problem) of each problem's model (P x 9 floats)
    std::vector<std::vector<int> > inliers(const float *models, float thr) const {
        const unsigned int P = problems();
        std::vector<uint8_t> mask(offsets_[P]);
        check(usac_multi_inliers(mc_, models, thr, mask.data(), nullptr), "MultiContext::inliers");
        std::vector<std::vector<int> > out(P);
        for (unsigned int p = 0; p < P; p++)
            for (uint32_t i = offsets_[p]; i < offsets_[p + 1]; i++)
                if (mask[i]) out[p].push_back((int)(i - offsets_[p]));
        return out;
    }

    // usac_multi_polish: the non-minimal polish of ransac.cpp:157-214 for every problem from its start
    // model (P x 9 floats), one workgroup per problem; inliers (nullable): the final getInliers of
    // each polished model, ascending indices local to the problem
    std::vector<usac_multi_polish_output> polish(const float *models, float thr,
                                                 std::vector<std::vector<int> > *inliers = nullptr) const {
        const unsigned int P = problems();
        std::vector<usac_multi_polish_output> out(P);
        std::vector<uint8_t> mask(inliers ? offsets_[P] : 0u);
        check(usac_multi_polish(mc_, models, thr, out.data(), inliers ? mask.data() : nullptr), "MultiContext::polish");
        if (inliers) splitMask(mask, inliers);
        return out;
    }

    // one problem's result of runPolished: run()'s output and polish()'s of its best model
    struct Polished {
        std::vector<usac_multi_output> run;
        std::vector<usac_multi_polish_output> polished;
        std::vector<std::vector<int> > inliers;
    };

    // usac_multi_run_polished: run(), then the polish of every best model at the model's threshold
    // (the records stay on the device in between)
    Polished runPolished(const Model &model, const std::vector<uint64_t> &seeds = std::vector<uint64_t>()) const {
        usac_params p = model.params();
        p.seed = model.seed;
        const unsigned int P = problems();
        if (!seeds.empty() && seeds.size() != P) throw Error(USAC_ERR_ARG, "runPolished: one seed per problem");
        Polished out;
        out.run.resize(P);
        out.polished.resize(P);
        std::vector<uint8_t> mask(offsets_[P]);
        check(usac_multi_run_polished(mc_, &p, seeds.empty() ? nullptr : seeds.data(), out.run.data(),
                                      out.polished.data(), mask.data()),
              "MultiContext::runPolished");
        splitMask(mask, &out.inliers);
        return out;
    }

    // one problem's result of runProsac: run()'s output and the PROSAC state at its end
    struct Prosac {
        std::vector<usac_multi_output> run;
        std::vector<usac_multi_prosac_output> prosac;
    };

    // usac_multi_run_prosac: run() with the PROSAC sampler and PROSAC's termination criterion per
    // problem (model.sampler = Prosac; every point set sorted by descending quality, n_p > 20)
    Prosac runProsac(const Model &model, const std::vector<uint64_t> &seeds = std::vector<uint64_t>()) const {
        usac_params p = model.params();
        p.seed = model.seed;
        const unsigned int P = problems();
        if (!seeds.empty() && seeds.size() != P) throw Error(USAC_ERR_ARG, "runProsac: one seed per problem");
        Prosac out;
        out.run.resize(P);
        out.prosac.resize(P);
        check(usac_multi_run_prosac(mc_, &p, seeds.empty() ? nullptr : seeds.data(), out.run.data(), out.prosac.data(),
                                    nullptr, nullptr),
              "MultiContext::runProsac");
        return out;
    }

    // usac_multi_lo: one LO call (inner + iterative LO-RANSAC, model.lo = InItLORsc / InItFLORsc) for
    // every problem, records[p] (in / out) taken as a new best; the LO threshold, the draw counter and
    // the counters persist from call to call unless reset.  Returns the P LO states after the call.
    std::vector<usac_multi_lo_output> lo(const Model &model, std::vector<usac_record> &records,
                                         const std::vector<uint64_t> &seeds = std::vector<uint64_t>(),
                                         bool reset = true) const {
        usac_params p = model.params();
        p.seed = model.seed;
        const unsigned int P = problems();
        if (records.size() != P) throw Error(USAC_ERR_ARG, "lo: one record per problem");
        if (!seeds.empty() && seeds.size() != P) throw Error(USAC_ERR_ARG, "lo: one seed per problem");
        std::vector<usac_multi_lo_output> out(P);
        check(usac_multi_lo(mc_, &p, reset ? 1 : 0, seeds.empty() ? nullptr : seeds.data(), records.data(), out.data()),
              "MultiContext::lo");
        return out;
    }

    // one problem's result of runLo: run()'s output, the LO counters and, with the PROSAC sampler,
    // the PROSAC state at the end (empty otherwise)
    struct Lo {
        std::vector<usac_multi_output> run;
        std::vector<usac_multi_lo_output> lo;
        std::vector<usac_multi_prosac_output> prosac;
    };

    // usac_multi_run_lo: run() (model.sampler = Uniform) or runProsac() (Prosac) with LO-RANSAC of every
    // round's new bests on the device (model.lo = InItLORsc / InItFLORsc, lo_sample_size <= 64)
    Lo runLo(const Model &model, const std::vector<uint64_t> &seeds = std::vector<uint64_t>()) const {
        usac_params p = model.params();
        p.seed = model.seed;
        const unsigned int P = problems();
        if (!seeds.empty() && seeds.size() != P) throw Error(USAC_ERR_ARG, "runLo: one seed per problem");
        Lo out;
        out.run.resize(P);
        out.lo.resize(P);
        if (p.sampler == USAC_SAMPLER_PROSAC) out.prosac.resize(P);
        check(usac_multi_run_lo(mc_, &p, seeds.empty() ? nullptr : seeds.data(), out.run.data(), out.lo.data(),
                                out.prosac.empty() ? nullptr : out.prosac.data(), nullptr, nullptr),
              "MultiContext::runLo");
        return out;
    }

    // usac_multi_lo_essential / usac_multi_run_lo_essential (ABI 23): lo() and runLo() on a context from
    // essential(), where those two keep refusing; sample size 5, the 8-point non-minimal fit
    std::vector<usac_multi_lo_output> loEssential(const Model &model, std::vector<usac_record> &records,
                                                  const std::vector<uint64_t> &seeds = std::vector<uint64_t>(),
                                                  bool reset = true) const {
        usac_params p = model.params();
        p.seed = model.seed;
        const unsigned int P = problems();
        if (records.size() != P) throw Error(USAC_ERR_ARG, "loEssential: one record per problem");
        if (!seeds.empty() && seeds.size() != P) throw Error(USAC_ERR_ARG, "loEssential: one seed per problem");
        std::vector<usac_multi_lo_output> out(P);
        check(usac_multi_lo_essential(mc_, &p, reset ? 1 : 0, seeds.empty() ? nullptr : seeds.data(), records.data(),
                                      out.data()),
              "MultiContext::loEssential");
        return out;
    }

    Lo runLoEssential(const Model &model, const std::vector<uint64_t> &seeds = std::vector<uint64_t>()) const {
        usac_params p = model.params();
        p.seed = model.seed;
        const unsigned int P = problems();
        if (!seeds.empty() && seeds.size() != P) throw Error(USAC_ERR_ARG, "runLoEssential: one seed per problem");
        Lo out;
        out.run.resize(P);
        out.lo.resize(P);
        if (p.sampler == USAC_SAMPLER_PROSAC) out.prosac.resize(P);
        check(usac_multi_run_lo_essential(mc_, &p, seeds.empty() ? nullptr : seeds.data(), out.run.data(), out.lo.data(),
                                          out.prosac.empty() ? nullptr : out.prosac.data(), nullptr, nullptr),
              "MultiContext::runLoEssential");
        return out;
    }

    // usac_multi_sprt_setup: the problems' SPRT pools (the reference's shuffle after srandom(seeds[p]),
    // default p + 1) and the pool-ordered copy of the points on the device; once per context
    void setSprtPool(const std::vector<uint32_t> &seeds = std::vector<uint32_t>()) const {
        if (!seeds.empty() && seeds.size() != problems()) throw Error(USAC_ERR_ARG, "setSprtPool: one seed per problem");
        check(usac_multi_sprt_setup(mc_, seeds.empty() ? nullptr : seeds.data()), "MultiContext::setSprtPool");
    }

    // one problem's result of runSprt: run()'s output, the SPRT state at the end and, with the PROSAC
    // sampler, the PROSAC state (empty otherwise)
    struct Sprt {
        std::vector<usac_multi_output> run;
        std::vector<usac_multi_sprt_output> sprt;
        std::vector<usac_multi_prosac_output> prosac;
    };

    // usac_multi_run_sprt: run() (model.sampler = Uniform) or runProsac() (Prosac) with SPRT verification of
    // every slot on the device, one test per problem and round (model.sprt set, model.lo = NullLO)
    Sprt runSprt(const Model &model, const std::vector<uint64_t> &seeds = std::vector<uint64_t>()) const {
        usac_params p = model.params();
        p.seed = model.seed;
        const unsigned int P = problems();
        if (!seeds.empty() && seeds.size() != P) throw Error(USAC_ERR_ARG, "runSprt: one seed per problem");
        Sprt out;
        out.run.resize(P);
        out.sprt.resize(P);
        if (p.sampler == USAC_SAMPLER_PROSAC) out.prosac.resize(P);
        check(usac_multi_run_sprt(mc_, &p, seeds.empty() ? nullptr : seeds.data(), out.run.data(), out.sprt.data(),
                                  out.prosac.empty() ? nullptr : out.prosac.data(), nullptr, nullptr),
              "MultiContext::runSprt");
        return out;
    }

    // one problem's grid neighbours: the CSR of Context's grid neighbours over its points (cells in order of
    // first appearance, members ascending) and the points with >= sampleSize() neighbours; local indices
    struct GridCsr {
        std::vector<uint32_t> cell, rank, start;
        std::vector<int32_t> members, eligible;
    };

    // usac_multi_grid: every problem's grid neighbours for cell_size, built in one launch and kept in the
    // context until another size is asked for
    std::vector<GridCsr> gridNeighbors(int cell_size) const {
        const unsigned int P = problems();
        const size_t N = offsets_[P];
        std::vector<uint32_t> nc(P), ne(P), cell(N), rank(N), start(N + P);
        std::vector<int32_t> members(N), eligible(N);
        check(usac_multi_grid(mc_, cell_size, nc.data(), cell.data(), rank.data(), start.data(), members.data(),
                              eligible.data(), ne.data()),
              "MultiContext::gridNeighbors");
        std::vector<GridCsr> out(P);
        for (unsigned int p = 0; p < P; p++) {
            const size_t a = offsets_[p], b = offsets_[p + 1];
            out[p].cell.assign(cell.begin() + a, cell.begin() + b);
            out[p].rank.assign(rank.begin() + a, rank.begin() + b);
            out[p].start.assign(start.begin() + a + p, start.begin() + a + p + nc[p] + 1);
            out[p].members.assign(members.begin() + a, members.begin() + b);
            out[p].eligible.assign(eligible.begin() + a, eligible.begin() + a + ne[p]);
        }
        return out;
    }

    // one problem's result of runNapsac: run()'s output and, with LO, the LO counters (empty otherwise)
    struct Napsac {
        std::vector<usac_multi_output> run;
        std::vector<usac_multi_lo_output> lo;
    };

    // usac_multi_run_napsac: run() with the grid NAPSAC sampler per problem (model.sampler = Napsac,
    // model.neighborsType = Grid, model.cell_size) and, with model.lo = InItLORsc / InItFLORsc, runLo()'s LO
    Napsac runNapsac(const Model &model, const std::vector<uint64_t> &seeds = std::vector<uint64_t>()) const {
        usac_params p = model.params();
        p.seed = model.seed;
        const unsigned int P = problems();
        if (!seeds.empty() && seeds.size() != P) throw Error(USAC_ERR_ARG, "runNapsac: one seed per problem");
        Napsac out;
        out.run.resize(P);
        if (p.lo != USAC_LO_NONE) out.lo.resize(P);
        check(usac_multi_run_napsac(mc_, &p, seeds.empty() ? nullptr : seeds.data(), out.run.data(),
                                    out.lo.empty() ? nullptr : out.lo.data(), nullptr, nullptr),
              "MultiContext::runNapsac");
        return out;
    }

private:
    void splitMask(const std::vector<uint8_t> &mask, std::vector<std::vector<int> > *out) const {
        const unsigned int P = problems();
        out->assign(P, std::vector<int>());
        for (unsigned int p = 0; p < P; p++)
            for (uint32_t i = offsets_[p]; i < offsets_[p + 1]; i++)
                if (mask[i]) (*out)[p].push_back((int)(i - offsets_[p]));
    }

    explicit MultiContext(const std::vector<uint32_t> &offsets) : est_(Essential), offsets_(offsets) {}  // essential()

    usac_multi *mc_ = nullptr;
    ESTIMATOR est_;
    std::vector<uint32_t> offsets_;
    uint32_t n_max_ = 0;
};

}  // namespace usac_gpu

#endif  // USAC_GPU_HPP
