/*
 * usac_gpu.h -- C-ABI of the MI355X-native USAC hypothesize-and-verify engine
 * (libransac_amd.so).  Plain pointers and sizes, opaque handles, int status
 * (0 = ok, < 0 = error, message via usac_last_error), never exit().
 *
 * Each entry point replaces one reference interface (MathsionYang/Ransac paths):
 *
 *   usac_create / usac_destroy     Ransac(Model*, cv::InputArray) estimator+quality init
 *                                  (usac/ransac/ransac.hpp:41-93, init.cpp:3-20)
 *   usac_estimate_models           Estimator::EstimateModel, batched
 *                                  (usac/estimator/estimator.hpp:19; homography
 *                                  homography_estimator.hpp:47-56 -> dlt.cpp:7-52;
 *                                  fundamental fundamental_estimator.hpp:48-63 ->
 *                                  seven_points.cpp:49-156;
 *                                  line2d line2d_estimator.hpp:36-54)
 *   usac_score_models              Quality::getNumberInliers(score, model), batched over
 *                                  models (usac/quality/quality.hpp:60-101)
 *   usac_get_inliers               Quality::getNumberInliers(..., get_inliers=true, inliers)
 *                                  / Quality::getInliers (quality.hpp:80-87, 108-121)
 *   usac_nonminimal / usac_lsq_fit Estimator::EstimateModelNonMinimalSample (weighted: estimator.hpp:26)
 *                                  (estimator.hpp:21; normalized_dlt.cpp:7-23;
 *                                  eight_points.cpp:4-100;
 *                                  line2d_estimator.hpp:59-107)
 *   usac_hypothesize_score         Sampler::generateSample + Estimator::EstimateModel +
 *                                  Quality::getNumberInliers + Score::bigger, fused over a
 *                                  batch (the body of ransac.cpp:58-139)
 *   usac_std_termination           StandardTerminationCriteria::getUpBoundIterations
 *                                  (standard_termination_criteria.hpp:52-62)
 *   usac_set_sprt / usac_sprt_tested  SPRT::verifyModelAndGetModelScore as a batch test
 *                                  (sprt.hpp:191-317, 332-355)
 *   usac_prosac_samples            ProsacSampler::generateSample (prosac_sampler.hpp:117-172)
 *   usac_set_device_sampler        Sampler choice of the throughput batches (Uniform / PROSAC
 *   usac_draw_samples              schedule, prosac_sampler.hpp:62-172 / NAPSAC grid,
 *   usac_set_cell_size             napsac_sampler.hpp:100-138) and its samples
 *   usac_grid_neighbors            NearestNeighbors::getGridNearestNeighbors
 *                                  (nearest_neighbors.cpp:160-202) built on the device
 *   usac_sprt_pool                 SPRT ctor pool + A0 (sprt.hpp:89-175)
 *   usac_ransac_run                Ransac::run + RansacOutput (ransac.cpp:14-238,
 *                                  ransac_output.hpp:29-97), Uniform sampler
 *   usac_ransac_run_sharded        Ransac::run with hypothesis-sharded batches
 *   usac_comm_*                    new: one RCCL all-gather of best records per batch
 *   usac_random / usac_sampler /   the per-call plugin state (ABI 11): the glibc random() stream,
 *   usac_termination / usac_sprt / Sampler::generateSample (sampler.hpp:11-35), TerminationCriteria
 *   usac_lo                        (termination_criteria.hpp:16-17, prosac_termination_criteria.hpp:
 *                                  148-201), SPRT (sprt.hpp:191-393, + the batch replay
 *                                  usac_sprt_replay), LocalOptimization::GetModelScore
 *                                  (local_optimization.hpp:19)
 *   usac_multi_*                   new (ABI 15): P independent two-view problems per launch -- the
 *                                  usac_hypothesize_score round and a batch-granular RANSAC with the
 *                                  standard termination criterion over a ragged set of point sets;
 *                                  ABI 16: usac_multi_polish / usac_multi_run_polished, the non-minimal
 *                                  polish and final getInliers of ransac.cpp:157-214 for every
 *                                  problem in one launch (one workgroup per problem);
 *                                  ABI 17: usac_multi_run_prosac, the PROSAC sampler and PROSAC's
 *                                  termination criterion per problem (the sampler in closed form on the
 *                                  device, the termination scan split between a kernel and the host),
 *                                  with usac_prosac_schedule / usac_multi_draw_samples /
 *                                  usac_multi_prosac_scan exposing its parts;
 *                                  ABI 18: usac_multi_run_lo, inner + iterative LO-RANSAC of every
 *                                  round's new bests in one launch (one workgroup per problem), with
 *                                  usac_lo_draw / usac_multi_lo exposing its parts;
 *                                  ABI 19: usac_multi_run_sprt, SPRT verification of every slot on the
 *                                  device with one test per problem and round, with usac_multi_sprt_setup /
 *                                  usac_multi_hypothesize_score_sprt / usac_multi_sprt_update exposing its parts;
 *                                  ABI 20: usac_multi_run_napsac, the grid NAPSAC sampler per problem over
 *                                  grid neighbours built for all problems in one launch (one workgroup per
 *                                  problem), optionally with LO and the polish, with usac_multi_grid /
 *                                  usac_multi_draw_samples_napsac / usac_multi_hypothesize_score_napsac
 *                                  exposing its parts;
 *                                  ABI 21: usac_multi_create_essential, multi contexts of essential-matrix
 *                                  problems (5-point solver): rounds, runs, masks, the polish and PROSAC;
 *                                  ABI 22: usac_multi_set_thresholds / usac_multi_get_thresholds, one inlier
 *                                  threshold per problem of a multi context in place of the calls' scalar;
 *                                  ABI 23: usac_multi_lo_essential / usac_multi_run_lo_essential, LO-RANSAC
 *                                  on multi contexts of essential-matrix problems (8-point non-minimal fit);
 *                                  ABI 24: usac_multi_create_essential_pixels, an essential multi context from
 *                                  pixel coordinates and per-pair intrinsics (converted on the device), with
 *                                  usac_multi_set_pixel_thresholds, usac_multi_pixel_models and
 *                                  usac_multi_get_points;
 *                                  ABI 25: usac_multi_create_device, a multi context from padded device memory
 *                                  (rows with a validity mask or counts, or keypoints with a match index),
 *                                  packed on the device, with usac_multi_get_offsets, usac_multi_get_source
 *                                  and usac_multi_padded_mask, a host mask scattered into P x n_max device bytes;
 *                                  ABI 26: usac_multi_create_device_sorted, the same context with every problem's
 *                                  kept rows sorted on the device by a score per column, the better first, so
 *                                  that usac_multi_run_prosac runs on a matcher's output as it is;
 *                                  ABI 27: usac_multi_export_device, the result of the last polishing call --
 *                                  models, counts, the padded mask, the inliers' columns, pixel-space models --
 *                                  written into device memory on the caller's stream, and usac_multi_set_resident,
 *                                  polishing calls that bring no mask to the host;
 *                                  ABI 28: usac_multi_pose_device and usac_multi_pose, the rotation and translation
 *                                  direction of an essential context's models, chosen on the device by a vote of
 *                                  the inliers over the four decompositions;
 *                                  ABI 29: usac_multi_refine_pose_device and usac_multi_refine_pose, a pose (R, t)
 *                                  refined on the device by Levenberg-Marquardt steps on its five parameters over
 *                                  the inliers' Sampson distances
 *
 * Threading: a context is bound to one device and one HIP stream and is not
 * thread-safe (one host thread / process per GPU).  Calls are synchronous with respect
 * to their outputs unless named *_async.
 */
#ifndef USAC_GPU_H
#define USAC_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USAC_ABI_VERSION 29

/* = enum ESTIMATOR (usac/model.hpp:10) */
enum { USAC_LINE2D = 1, USAC_HOMOGRAPHY = 2, USAC_FUNDAMENTAL = 3, USAC_ESSENTIAL = 4 };
/* = enum SAMPLER (usac/model.hpp:11): Uniform, Napsac (grid neighbours), Prosac */
enum { USAC_SAMPLER_UNIFORM = 1, USAC_SAMPLER_NAPSAC = 3, USAC_SAMPLER_PROSAC = 4 };
/* = enum LocOpt (usac/model.hpp:13): inner + iterative LO-RANSAC (unlimited / limited), graph-cut
 * LO (graphcut.hpp) */
enum { USAC_LO_NONE = 0, USAC_LO_INITLORSC = 1, USAC_LO_INITFLORSC = 2, USAC_LO_GC = 3 };
/* = enum NeighborsSearch (usac/model.hpp:12): the Ransac ctor (ransac.hpp:60-78) builds Grid
 * neighbours for Grid and nanoflann KNN for any other value (NullN included) */
enum { USAC_NEIGHBORS_NULL = 0, USAC_NEIGHBORS_NANOFLANN = 1, USAC_NEIGHBORS_GRID = 2 };
/* 4-pt DLT: THIN = reference semantics (vt.row(7) of the thin 8x9 SVD, dlt.cpp:43-48);
 * NULLSPACE = true null vector. */
enum { USAC_DLT_THIN = 0, USAC_DLT_NULLSPACE = 1 };

enum {
    USAC_OK = 0,
    USAC_ERR_ARG = -1,
    USAC_ERR_HIP = -2,
    USAC_ERR_UNSUPPORTED = -3,
    USAC_ERR_NO_MODEL = -111 /* best score 0, ransac.cpp:143-147 (reference exit(111)) */
};

typedef struct usac_ctx usac_ctx;

/* A hypothesis record: Score {inlier_number, score} (quality.hpp:16-37) of model
 * `model` produced by hypothesis `hyp_index` (global sample index). */
typedef struct usac_record {
    uint64_t hyp_index;
    int32_t inliers;
    float score;
    float model[9];
    int32_t valid;
} usac_record;

/* Model (usac/model.hpp:15-45) fields the loop reads. */
typedef struct usac_params {
    float threshold;            /* model.hpp:17 (default 2) */
    float desired_prob;         /* model.hpp:18 (0.95) */
    uint32_t max_iterations;    /* model.hpp:22 (10000) */
    uint32_t seed;              /* glibc srandom(seed): ResetRandomGenerator(false) semantics;
                                   also seeds PROSAC's mt19937 (the reference uses random_device) */
    int32_t dlt_mode;           /* USAC_DLT_* */
    uint32_t batch;             /* hypotheses per device batch (0 = default: 1024, 2048, ... up to 8192; SPRT 1024) */
    int32_t sampler;            /* USAC_SAMPLER_UNIFORM | _NAPSAC (grid) | _PROSAC (points sorted by quality) */
    int32_t sprt;               /* Model::setSprt (model.hpp:104): SPRT verification, sprt.hpp */
    int32_t lo;                 /* USAC_LO_* (model.hpp:26) */
    uint32_t lo_sample_size;          /* model.hpp:27 (14) */
    uint32_t lo_iterative_iterations; /* model.hpp:28 (4) */
    uint32_t lo_inner_iterations;     /* model.hpp:29 (20) */
    uint32_t lo_threshold_multiplier; /* model.hpp:30 (10) */
    int32_t cell_size;                /* model.hpp:43 (50): NAPSAC grid cell */
    int32_t neighbors;                /* USAC_NEIGHBORS_* (model.hpp:42): NAPSAC Grid or KNN */
    uint32_t knn;                     /* model.hpp:23 k_nearest_neighbors (NAPSAC KNN / GC, 1..32) */
    float spatial_coherence_gc;       /* model.hpp:33 (0.1): GC pairwise weight, used as given
                                         (graphcut.hpp:43; 0 = no pairwise term) */
    uint32_t max_hypothesis_test_before_sprt; /* model.hpp:40 (20; ABI 12): a rejected model still counts
                                         as an iteration from this iteration on (ransac.cpp:81-83), and the
                                         SPRT's adaptive history starts then (sprt.hpp:243); 0 = 20 */
} usac_params;

/* RansacOutput getters (ransac_output.hpp:57-97) */
typedef struct usac_run_output {
    float model[9];
    int32_t inliers;            /* getNumberOfInliers */
    uint32_t iters;             /* getNumberOfMainIterations */
    int64_t time_us;            /* getTimeMicroSeconds (loop + polish, as ransac.cpp:15,209) */
    int32_t n_records;          /* best-score updates in the main loop */
    int32_t polish_passes;
    float minimal_model[9];     /* best model before the non-minimal polish */
    int32_t minimal_inliers;
    uint32_t batches;           /* device batches launched */
    int32_t sprt_rejected;      /* models rejected by SPRT */
    int32_t sprt_histories;     /* SPRT tests designed (sprt_histories.size()) */
    uint32_t prosac_term_len;   /* final PROSAC termination_length (n without PROSAC) */
    uint32_t rollbacks;         /* PROSAC speculative batches cut short by a termination_length change */
    uint32_t lo_inner_iters;    /* getLOIters (ransac_output.hpp): inner LO iterations (GC: gc_iterations) */
    uint32_t lo_iterative_iters; /* iterative LO iterations (GC: labellings) */
    uint32_t lo_rounds;         /* LO speculation rounds (batches of inner iterations run at once) */
    uint32_t lo_stages;         /* LO device stages (one batched fit or one batched scoring each) */
    uint32_t sum_models;        /* models whose exact sequential Σerr the replay needed */
    uint32_t lo_fits;           /* LO least-squares fits this rank ran (a sharded run splits the
                                   inner-iteration chains: the ranks' counts add up to the 1-rank run's) */
    uint32_t spec_batches;      /* batches drawn and solved ahead of the replay (speculation) */
    uint32_t spec_rollbacks;    /* of those, cut short by a smaller termination bound (sampler rolled back) */
    uint32_t spec_wasted;       /* hypotheses solved and scored ahead that the run never reached */
} usac_run_output;

/* ---- lifetime ----------------------------------------------------------------- */
/* pts: n rows of `cols` floats (2: line [x y]; 4: two-view [x1 y1 x2 y2]), host memory,
 * copied to the device at create (the caller may free it). */
int usac_create(usac_ctx **out, int device, int estimator, const float *pts, uint32_t n, uint32_t cols);
void usac_destroy(usac_ctx *ctx);
const char *usac_last_error(const usac_ctx *ctx);
int usac_abi_version(void);
int usac_set_dlt_mode(usac_ctx *ctx, int mode);
uint32_t usac_sample_size(const usac_ctx *ctx);
uint32_t usac_num_points(const usac_ctx *ctx);

/* ---- plugin operators ----------------------------------------------------------- */
/* samples: B x m int32 (host) -> models: B x S x 9 floats, n_models[B] valid models per
 * sample, S = model slots per sample (3 for USAC_FUNDAMENTAL -- SevenPointsAlgorithm returns
 * <= 3 F that pass the oriented constraint, fundamental_estimator.hpp:48-63 -- else 1);
 * empty slots are zero-filled. */
int usac_estimate_models(usac_ctx *ctx, const int32_t *samples, uint32_t B, float *models, int32_t *n_models);
/* models: n_models x 9 floats (host); counts/sums (host, sums nullable).  Counts are
 * exact; sums are the sequential fp32 sums of quality.hpp:89-96. */
int usac_score_models(usac_ctx *ctx, const float *models, uint32_t n_models, float thr, int32_t *counts,
                      float *sums);
/* One model: ascending inlier indices (idx capacity >= n points), count and sum. */
int usac_get_inliers(usac_ctx *ctx, const float *model, float thr, int32_t *idx, uint32_t *n, float *sum);
/* The graph-cut LO's min cut, host side (usac_maxflow.hpp; gco-v3.0 energy.h + maxflow.inl
 * semantics): n nodes with add_term1(i, unary[i], 0), add_term2(ei[k], ej[k], e00[k], e01[k],
 * e10[k], e11[k]) in order, BK max-flow; sink_out[i] = 1 iff what_segment(i) == SINK.
 * Returns the flow.  No device work (exposed for parity tests against the gco sources). */
float usac_bk_label(int n, const float *unary, int m, const int32_t *ei, const int32_t *ej, const float *e00,
                    const float *e01, const float *e10, const float *e11, int32_t *sink_out);
/* NearestNeighbors::getNearestNeighbors_nanoflann (nearest_neighbors.cpp:69-128) on the
 * device: the k nearest neighbours of every point (1 <= k <= 32; idx n x k, d2 n x k
 * squared distances, nullable) by nanoflann's float L2 distance, the point itself excluded,
 * ascending distance, equal distances by ascending index; -1 / +inf where n - 1 < k. */
int usac_knn(usac_ctx *ctx, uint32_t k, int32_t *idx, float *d2);
/* Non-minimal least squares on the listed points; returns USAC_OK and writes model. */
int usac_nonminimal(usac_ctx *ctx, const int32_t *idx, uint32_t n, float *model);
/* Estimator::EstimateModelNonMinimalSample with optional weights (estimator.hpp:21,26):
 * weights == NULL is usac_nonminimal; otherwise weights[i] belongs to point i of the context
 * (n_points floats, indexed by point index as the reference's weights[sample[i]]) and the fit
 * is the weighted overload -- homography: weighted NormalizedDLT (normalized_dlt.cpp:25-36),
 * fundamental: weighted EightPointsAlgorithm (eight_points.cpp:176-228), both through the
 * weighted GetNormalizingTransformation (normalizing_transformation.cpp:117-166).  Line and
 * essential estimators have no weighted overload (USAC_ERR_UNSUPPORTED). */
int usac_lsq_fit(usac_ctx *ctx, const int32_t *idx, uint32_t n, const float *weights, float *model);

/* Fused batch: samples (B x m host int32) or NULL => device xorshift sampler keyed by
 * (seed, first_hyp + i).  Per-model counts/sums (host, nullable, B x S entries: slot
 * b*S + j = j-th valid model of sample b, count -1 on an empty slot) and the batch best
 * under Score::bigger with the earliest (sample, slot) on exact ties (best, nullable;
 * best->hyp_index = first_hyp + sample). */
int usac_hypothesize_score(usac_ctx *ctx, const int32_t *samples, uint32_t B, uint64_t seed, uint64_t first_hyp,
                           float thr, int32_t *counts, float *sums, usac_record *best);
/* Asynchronous device-sampled batch for throughput runs: enqueues sample+solve+score+
 * argmax on the context stream; usac_fetch_best waits and returns the batch best. */
int usac_hypothesize_async(usac_ctx *ctx, uint32_t B, uint64_t seed, uint64_t first_hyp, float thr);
int usac_fetch_best(usac_ctx *ctx, usac_record *best);
/* Per-slot counts / sums (sums nullable) of the last batch as the score kernel left them (the
 * throughput kernels' chunked sums included): n <= B x slots.  Waits for the stream.  For tests.
 * USAC_ERR_ARG after a usac_ransac_run until the next batch (the run's buffers are not a batch's). */
int usac_last_counts(usac_ctx *ctx, int32_t *counts, float *sums, uint32_t n);
int usac_sync(usac_ctx *ctx);
/* Device time of the last async batch's kernels, measured with HIP events on the
 * context stream: [0] whole batch, [1] score kernel, [2] solve kernel (ms). */
int usac_last_timings(usac_ctx *ctx, float *ms3);
/* ABI 14: on = 0 stops usac_hypothesize_async recording those HIP events on this context (four
 * event records of host time per batch; usac_last_timings then keeps returning the last timed
 * batch's values); on = 1 (the default) records them again. */
int usac_set_timing(usac_ctx *ctx, int on);
/* Score-kernel split factor (point chunks per hypothesis tile, 1 = exact sequential sums):
 * 1, 2, 4, 8, 16; any of 1..128 for the fundamental / essential estimators (their chunks are
 * separate workgroups, combined in chunk order; default 96). */
int usac_set_score_chunks(usac_ctx *ctx, int chunks);
/* Homography score kernel: 0 = guard-band fast path with the hypothesis pre-sort (default; multi-
 * chunk batches -- the throughput and loop batches -- go through the matrix-core prefilter scorer
 * unless USAC_H16=0), 1 = exact reference expression for every pair, 2 = fast path without the
 * pre-sort, 3 = as 0, and usac_score_models also scores through the multi-chunk scorer (tests: exact
 * counts, Σ within its bound).  Every variant gives the same counts. */
int usac_set_score_variant(usac_ctx *ctx, int variant);

/* Throughput SPRT (sprt.hpp:191-317 as a batch test): with enable != 0 every later
 * batch (usac_hypothesize_score / _async) verifies each model by the SPRT with fixed
 * (epsilon, delta) -- <= 0 selects the reference's initial values for the estimator
 * (sprt.hpp:106-150) -- and threshold A = estimateThresholdA(epsilon, delta), over the
 * SPRT pool of srandom(seed) (sprt.hpp:93-104), each model from a pool position of its own
 * (usac_batch_sprt_info) instead of the rolling index, without the history updates.  Each
 * decision equals the reference's fp64 lambda product walk with those constants from that
 * position (certified in log space from exact counts, the sequential product where the
 * certificate fails; kernels_sprt.hip).  Rejected models get count -1; accepted ones count =
 * inliers over all points, score = (float)count (sprt.hpp:276-281).  usac_ransac_run always
 * replays the exact sequential SPRT (rolling index, history) instead. */
int usac_set_sprt(usac_ctx *ctx, int enable, uint32_t seed, double epsilon, double delta);
/* pool points the SPRT tested in the last batch (the scoring work actually done) */
int usac_sprt_tested(usac_ctx *ctx, uint64_t *points_tested);
/* The batch test's constants -- eps_delta_A[3] = epsilon, delta, A (nullable) -- and the first pool
 * position each model slot of the last batch was tested from (starts, n slots, nullable; slots of
 * the fundamental solver 3 per sample; n <= the last batch's slots; a slot the solver left empty
 * reads UINT32_MAX).  Every decision equals the reference's fp64 product walk (sprt.hpp:209-234)
 * with these constants from that position.  For tests. */
int usac_batch_sprt_info(usac_ctx *ctx, double *eps_delta_A, uint32_t *starts, uint32_t n);
/* Sampler of the throughput batches' device stream (usac_hypothesize_score with samples ==
 * NULL, usac_hypothesize_async): USAC_SAMPLER_UNIFORM (default), USAC_SAMPLER_NAPSAC (grid
 * neighbours of usac_set_cell_size's cell, default 50, built on the device: the initial point
 * uniform over the points with >= m neighbours, then m - 1 consecutive entries of its
 * neighbour list from a random phase -- napsac_sampler.hpp:100-138, whose cursor persists
 * across samples; uniform samples when no point qualifies; 4-column points) or
 * USAC_SAMPLER_PROSAC --
 * hypothesis h (the global index first_hyp + b) uses the reference's PROSAC subset schedule
 * (growth function prosac_sampler.hpp:62-114, termination_length = n; points must be sorted
 * by quality): the subset's last point plus m - 1 distinct points before it, for
 * h < T_N = 200000, uniform afterwards (prosac_sampler.hpp:117-172).  The random draws are
 * the device SplitMix64 stream, not the host mt19937 (usac_ransac_run keeps that one). */
int usac_set_device_sampler(usac_ctx *ctx, int sampler);
/* Grid cell size of the device NAPSAC sampler (model.hpp:43, default 50). */
int usac_set_cell_size(usac_ctx *ctx, int cell_size);
/* NearestNeighbors::getGridNearestNeighbors (nearest_neighbors.cpp:160-202) on the device:
 * cell ((int)(x1/cs), (int)(y1/cs), (int)(x2/cs), (int)(y2/cs)), fp32 division.  CSR (every
 * output nullable, host memory): cell[n] (cells numbered in order of first appearance),
 * rank[n] (position in the cell), start[n_cells + 1], members[n] (cells in order, ascending
 * index) -- point i's neighbours are its cell's members except itself, ascending -- and
 * eligible[n_eligible] = the points with >= sample-size neighbours (NAPSAC, Q18), ascending.
 * usac_ransac_run's NAPSAC / graph-cut grids are this one. */
int usac_grid_neighbors(usac_ctx *ctx, int cell_size, uint32_t *n_cells, uint32_t *cell, uint32_t *rank,
                        uint32_t *start, int32_t *members, int32_t *eligible, uint32_t *n_eligible);
/* The device stream's samples for hypotheses first_hyp .. first_hyp + B - 1 (B x m int32,
 * host memory): what the solve kernels draw.  For tests. */
int usac_draw_samples(usac_ctx *ctx, uint32_t B, uint64_t seed, uint64_t first_hyp, int32_t *out);

/* ---- loop --------------------------------------------------------------------- */
uint32_t usac_std_termination(uint32_t inliers, uint32_t points_size, uint32_t sample_size, float desired_prob,
                              uint32_t max_iterations);
/* Ransac::run (ransac.cpp:14-238) with the Uniform (glibc random() stream), NAPSAC (grid or
 * KNN neighbours, napsac_sampler.hpp), graph-cut LO (graphcut.hpp; KNN or grid neighbours;
 * not with NAPSAC, whose combination the reference leaves undefined) or PROSAC (prosac_sampler.hpp + prosac_termination_criteria.hpp)
 * sampler, optional SPRT (sprt.hpp; pool shuffle from the same glibc stream), optional
 * inner + iterative LO-RANSAC (inner_local_optimization.hpp, iterative_local_optimization.hpp;
 * its mt19937 seeded with seed + 1).  inliers_out (capacity n,
 * nullable): final inliers ascending.  records (nullable, capacity rec_cap): best-score
 * updates in loop order (hyp_index = iteration, SPRT double counting included). */
int usac_ransac_run(usac_ctx *ctx, const usac_params *params, usac_run_output *out, int32_t *inliers_out,
                    usac_record *records, uint32_t rec_cap);
/* All-gather of host bytes across the ranks of a sharded run: every rank passes `bytes` bytes at
 * `send`; `recv` (nranks x bytes) receives them in rank order.  Returns 0 on success. */
typedef int (*usac_allgather_fn)(void *user, const void *send, size_t bytes, void *recv);
/* Ransac::run with every batch's hypotheses sharded over nranks processes / GPUs:
 * each rank draws the same host sample stream (same params, same seed), solves and scores its
 * contiguous slice of the batch, and the slices' counts and models are all-gathered -- through
 * `gather` when non-null (e.g. a torch.distributed gloo group), else RCCL on the communicator of
 * usac_comm_init(ctx, nranks, rank, id).  Termination, LO, graph cut and polish are then replayed
 * on the merged batch identically on every rank, so every rank's output equals usac_ransac_run's.
 * With SPRT each rank also computes its slice's pool-order inlier words (the words the sequential
 * SPRT walk reads, sprt.hpp:191-317), all-gathered with the models; every rank replays the walk.
 * A rank that fails joins the all-gather with its status and every rank fails with it; a gather
 * callback must therefore fail (return non-zero) on every rank or on none. */
int usac_ransac_run_sharded(usac_ctx *ctx, const usac_params *params, int nranks, int rank, usac_allgather_fn gather,
                            void *gather_user, usac_run_output *out, int32_t *inliers_out, usac_record *records,
                            uint32_t rec_cap);
/* Host glibc-compatible UniformSampler stream (uniform_sampler.hpp:42-54): count x m
 * samples after srandom(seed).  Exposed for parity tests. */
int usac_uniform_samples(uint32_t seed, uint32_t n_points, uint32_t m, uint32_t count, int32_t *out);
/* Host ProsacSampler stream (prosac_sampler.hpp:117-172), mt19937 seeded with `seed`,
 * termination_length held at `termination_length`: count x m samples.  For parity tests. */
int usac_prosac_samples(uint32_t seed, uint32_t n_points, uint32_t m, uint32_t count, uint32_t termination_length,
                        int32_t *out);
/* SPRT random pool after srandom(seed) (sprt.hpp:89-104; n_points glibc draws) and the
 * first test's threshold A (sprt.hpp:332-355) for `estimator`.  For parity tests. */
int usac_sprt_pool(uint32_t seed, int estimator, uint32_t n_points, uint32_t m, uint32_t *pool, double *A0);

/* ---- stateful plugins: the reference's per-call surface (ABI 11) ----------------------
 * Handles that keep the reference's plugin state between calls, so a caller that keeps its
 * own Ransac::run loop (ransac.cpp:58-139) swaps each plugin for the device one:
 *   usac_random       the global glibc random() stream after srandom(seed) -- UniformSampler and
 *                     NapsacSampler draw from it, the SPRT ctor shuffles its pool with it
 *                     (uniform_sampler.hpp:22-54, array_random_generator.hpp:21-49, sprt.hpp:93-104)
 *   usac_sampler      Sampler::generateSample (sampler.hpp:11-35): Uniform (persistent pool),
 *                     PROSAC (growth function, termination length), NAPSAC (grid / KNN neighbours
 *                     built on the context's device)
 *   usac_termination  TerminationCriteria::getUpBoundIterations (termination_criteria.hpp:16-17) and
 *                     ProsacTerminationCriteria::getUpBoundIterations(hypCount, model)
 *                     (prosac_termination_criteria.hpp:148-201)
 *   usac_sprt         SPRT::verifyModelAndGetModelScore (sprt.hpp:191-317), getUpperBoundIterations
 *                     (sprt.hpp:371-393) and the batch replay of the loop body with SPRT
 *   usac_lo           LocalOptimization::GetModelScore (local_optimization.hpp:19): inner + iterative
 *                     LO-RANSAC or graph-cut LO
 * A handle created on a context uses that context's device, stream and buffers: it must be
 * destroyed before the context, and -- like the reference's plugins -- is not thread-safe.
 * Handles drawing from a usac_random keep a pointer to it (destroy them first). */
typedef struct usac_random usac_random;
typedef struct usac_sampler usac_sampler;
typedef struct usac_termination usac_termination;
typedef struct usac_sprt usac_sprt;
typedef struct usac_lo usac_lo;

int usac_random_create(uint32_t seed, usac_random **out);
uint32_t usac_random_next(usac_random *rng); /* random() */
void usac_random_destroy(usac_random *rng);

/* initSampler (ransac/init.cpp) for params->sampler:
 *   USAC_SAMPLER_UNIFORM  UniformSampler on rng: m draws without replacement from a persistent
 *                         pool, idx = random() % max, refilled when max reaches 0 (Q5)
 *   USAC_SAMPLER_PROSAC   ProsacSampler, its mt19937 seeded with params->seed (the reference:
 *                         std::random_device); points sorted by quality; sampling is limited to the
 *                         termination length of the PROSAC termination criteria created on it
 *                         (usac_termination_create), n before that (prosac_sampler.hpp:117-172)
 *   USAC_SAMPLER_NAPSAC   NapsacSampler on rng with grid neighbours (params->neighbors ==
 *                         USAC_NEIGHBORS_GRID, cell params->cell_size; 4-column points) or KNN
 *                         (params->knn), both built on ctx's device (napsac_sampler.hpp:40-158)
 * rng: required for Uniform / NAPSAC, ignored for PROSAC. */
int usac_sampler_create(usac_ctx *ctx, const usac_params *params, usac_random *rng, usac_sampler **out);
/* generateSample(sample): m indices into `sample`.  NAPSAC rewrites only sample[0] once it has
 * turned uniform (as the reference), so pass the same array every call, as the loop does. */
int usac_sampler_generate(usac_sampler *s, int32_t *sample);
/* count successive generateSample calls into samples (count x m; each row starts as a copy of
 * the previous one, the reference's reused sample array) */
int usac_sampler_generate_batch(usac_sampler *s, uint32_t count, int32_t *samples);
/* samples drawn so far; PROSAC: subset_size and largest_sample_size (else n, n) -- nullable */
int usac_sampler_state(const usac_sampler *s, uint64_t *drawn, uint32_t *subset_size, uint32_t *largest_sample_size);
void usac_sampler_destroy(usac_sampler *s);

/* initTerminationCriteria: StandardTerminationCriteria (params->desired_prob, ->max_iterations;
 * m and n from ctx), or -- prosac != NULL, a USAC_SAMPLER_PROSAC sampler -- ProsacTerminationCriteria
 * linked to it both ways as in the reference (the sampler reads its termination length, it reads
 * the sampler's growth function and largest sample size; prosac_termination_criteria.hpp:44-119). */
int usac_termination_create(usac_ctx *ctx, const usac_params *params, usac_sampler *prosac, usac_termination **out);
/* getUpBoundIterations(inlier_size) / (inlier_size, points_size) (standard_termination_criteria.hpp:
 * 52-74); points_size 0 = the context's n */
uint32_t usac_termination_bound(const usac_termination *t, uint32_t inlier_size, uint32_t points_size);
/* ProsacTerminationCriteria::getUpBoundIterations(hypCount, model): the model's inlier flags at
 * params->threshold over the quality-sorted points from the device, the non-randomness /
 * maximality scan on the host.  *max_iters = the new bound, *termination_length (nullable) = the
 * updated termination length (the linked sampler uses it from its next sample on). */
int usac_prosac_termination(usac_termination *t, uint32_t hyp_count, const float *model, uint32_t *max_iters,
                            uint32_t *termination_length);
void usac_termination_destroy(usac_termination *t);

/* SPRT ctor (sprt.hpp:89-175): the random pool from n draws of rng (the Ransac ctor creates it after
 * the sampler, before the sampler's first draw), the reference's initial epsilon / delta / t_M / m_S
 * for ctx's estimator; params->threshold, ->max_iterations, ->max_hypothesis_test_before_sprt. */
int usac_sprt_create(usac_ctx *ctx, const usac_params *params, usac_random *rng, usac_sprt **out);
/* verifyModelAndGetModelScore(model, current_hypothese, maximum_score, score), one model (9 floats;
 * line: 3): the model's inlier flags in pool order from the device, the reference's fp64 lambda walk
 * over the rolling pool index on the host.  *good = the decision; *count / *score written as the
 * reference writes them (accepted: inliers, (float)inliers; rejected while current_hypothese <
 * params->max_hypothesis_test_before_sprt (default 20): the full count; otherwise left untouched). */
int usac_sprt_verify(usac_sprt *s, const float *model, int32_t current_hypothese, uint32_t maximum_score,
                     int32_t *good, int32_t *count, float *score);
/* getUpperBoundIterations(inlier_size) (sprt.hpp:371-393) */
uint32_t usac_sprt_upper_bound(const usac_sprt *s, uint32_t inlier_size);
/* tests designed so far (sprt_histories.size()) and models rejected by this handle */
int usac_sprt_stats(const usac_sprt *s, uint32_t *histories, uint32_t *rejected);

/* The loop body of ransac.cpp:58-139 with SPRT over a batch of minimal samples (SURVEY §8(b)
 * usac_sprt_replay).  State in / out: */
typedef struct usac_sprt_state {
    uint32_t iters;        /* in/out: the loop's iteration counter (ransac.cpp:55) */
    uint32_t max_iters;    /* in: the bound in force (`while (iters < max_iters)`) */
    int32_t best_inliers;  /* in: best_score->inlier_number */
    float best_score;      /* in: best_score->score */
    uint32_t sample;       /* in/out cursor: the next sample of the batch ... */
    uint32_t slot;         /* ... and model slot to verify; (0, 0) starts a new batch */
    int32_t found;         /* out: 1 = stopped after a model bigger than the best (Score::bigger) */
    int32_t inliers;       /* out: that model's score (the caller updates its best, runs LO and */
    float score;           /*      the termination, sets max_iters / best_* and calls again) */
    uint32_t found_sample, found_slot;
    uint32_t rejected;     /* out: models rejected during this call */
} usac_sprt_state;
/* models: B x slots x 9 floats and n_models[B] (usac_estimate_models' layout; slots = 3 for the
 * 7-point solver, else 1).  From the cursor, in loop order: verify(model, iters, best_inliers); a
 * rejected model at iters >= max_hypothesis_test_before_sprt (the handle's params, default 20) counts an
 * iteration and is skipped (Q9); every other model is
 * compared with the best; after each sample iters++; before each sample `iters < max_iters` is
 * checked.  Returns with found = 1 at the first model bigger than the best (the cursor then points
 * past it), or found = 0 when the batch is exhausted (sample == B) or the loop bound is reached
 * (iters >= max_iters).  The batch's inlier words are computed on the device when the cursor is at
 * (0, 0); later calls for the same batch must pass the same models. */
int usac_sprt_replay(usac_sprt *s, const float *models, const int32_t *n_models, uint32_t B, usac_sprt_state *st);
void usac_sprt_destroy(usac_sprt *s);

/* initLocalOptimization for params->lo: USAC_LO_INITLORSC / _INITFLORSC (InnerLocalOptimization with
 * IterativeLocalOptimization, unlimited / limited; inner_local_optimization.hpp:40-133,
 * iterative_local_optimization.hpp:28-136; its mt19937 seeded with params->seed + 1) or USAC_LO_GC
 * (GraphCut, graphcut.hpp:99-153, KNN or grid neighbours built on ctx's device; params->neighbors,
 * ->knn, ->cell_size, ->spatial_coherence_gc).  The LO threshold persists across calls (Q11). */
int usac_lo_create(usac_ctx *ctx, const usac_params *params, usac_lo **out);
/* GetModelScore(best_model, best_score): model (9 floats), inliers and score improved in place */
int usac_lo_get_model_score(usac_lo *lo, float *model, int32_t *inliers, float *score);
/* lo_inner_iters / lo_iterative_iters (InnerLocalOptimization), or gc_iterations / labellings (GC) */
int usac_lo_iters(const usac_lo *lo, uint32_t *inner, uint32_t *iterative);
void usac_lo_destroy(usac_lo *lo);

/* ---- multi-GPU (RCCL over xGMI) --------------------------------------------------- */
/* 128-byte RCCL unique id (rank 0 creates, everyone receives it out of band). */
int usac_comm_unique_id(uint8_t *id128);
int usac_comm_init(usac_ctx *ctx, int nranks, int rank, const uint8_t *id128);
/* What RCCL itself reports for ctx's communicator (ABI 12): ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice -- a multi-GPU bench line states the rank count RCCL saw, not the one asked for. */
int usac_comm_count(usac_ctx *ctx, int *nranks, int *rank, int *device);
/* All-gather of one usac_record per rank on the context stream: all[nranks]. */
int usac_allgather_records(usac_ctx *ctx, const usac_record *local, usac_record *all);
/* The per-batch best exchange of the throughput pipeline, off the compute streams: the record
 * usac_hypothesize_async(batch) leaves on the device is all-gathered over ctx's communicator
 * on ctx's own exchange stream, ordered after `batch`'s stream by an event (neither stream
 * waits for the other's later work; no host staging), then copied to pinned host memory.
 * `slot` (< USAC_XRING) names the exchange in a ring; usac_exchange_best_wait(slot) returns
 * the nranks records (rank order) and frees the slot: at most USAC_XRING exchanges may be
 * outstanding.  Every rank must issue the exchanges -- and the context's other collectives
 * (usac_allgather_records, sharded runs on its communicator) -- in the same order; the two kinds
 * may be mixed: a collective on the context stream waits for the exchanges issued before it, an
 * exchange for the context-stream collectives issued before it (events, no host wait).
 * batch may be ctx itself or another context on the same device. */
#define USAC_XRING 8
int usac_exchange_best_async(usac_ctx *ctx, usac_ctx *batch, uint32_t slot);
int usac_exchange_best_wait(usac_ctx *ctx, uint32_t slot, usac_record *all);
/* Merge n records by Score::bigger, earliest hyp_index on exact ties. */
int usac_merge_records(const usac_record *recs, uint32_t n, usac_record *best);

/* ---- multi-problem batches (ABI 15; polish: ABI 16; PROSAC: ABI 17, below) ----------------------------
 * A multi context holds P independent two-view problems of one estimator (USAC_HOMOGRAPHY or
 * USAC_FUNDAMENTAL; the essential matrix through usac_multi_create_essential, ABI 21; line:
 * USAC_ERR_UNSUPPORTED) and runs them together: one launch
 * whose grid covers (problem, 64-hypothesis tile).  Points are one concatenated N_total x 4 fp32
 * array and offsets[P + 1] with offsets[0] = 0: problem p owns rows offsets[p] .. offsets[p + 1] - 1,
 * n_p >= the sample size.  Sample, hypothesis and inlier indices are local to the problem.
 *
 * Per problem every result equals the single-context path bit for bit: problem p with seed s and
 * global hypothesis index h draws the sample a usac_ctx over its points draws (device uniform sampler
 * keyed by (s, h) over n_p), the solvers are the same (H: thin QR with the row-Jacobi fall-back,
 * honouring dlt_mode; F: up to 3 slots, oriented filter, compaction order), and scoring is the
 * one-chunk exact form: exact counts, the sequential fp32 sum in point order, count -1 (sum 0) on an
 * empty F slot -- what usac_hypothesize_score returns when per-hypothesis outputs are requested.
 *
 * A problem's points are walked by one wave per 64 hypotheses, without point chunking: any n_p is
 * correct, but the design targets n_p up to a few thousand (many small problems fill the device,
 * one large problem does not).  P <= 65535.  One device, one HIP stream, not thread-safe. */
typedef struct usac_multi usac_multi;

/* One problem's result of usac_multi_run. */
typedef struct usac_multi_output {
    usac_record best;     /* the run's best under usac_merge_records' order */
    uint32_t hypotheses;  /* hypotheses evaluated: rounds x R */
    uint32_t rounds;
    uint32_t bound;       /* usac_std_termination(best.inliers, n_p, m, desired_prob, max_iterations) */
    int32_t status;       /* USAC_OK, or USAC_ERR_NO_MODEL when the best count is 0 */
} usac_multi_output;

/* USAC_ERR_ARG for P == 0 or P > 65535, offsets[0] != 0, non-monotonic offsets or any n_p < m, and
 * USAC_ERR_UNSUPPORTED for the line and essential estimators -- all before any device call.  A multi
 * context of essential-matrix problems comes from usac_multi_create_essential. */
int usac_multi_create(usac_multi **out, int device, int estimator, const float *pts, const uint32_t *offsets,
                      uint32_t P);
/* usac_multi_create for the essential matrix (ABI 21): the points are calibrated coordinates (K^-1 x), as
 * usac_create's for USAC_ESSENTIAL; m = 5, one slot per sample (S = 1; count -1, sum 0 on a sample without
 * a model).  USAC_ERR_ARG as usac_multi_create's (P == 0 or > 65535, offsets, any n_p < 5, NULL pointers)
 * -- before any device call.
 * Per problem every result equals a usac_ctx of USAC_ESSENTIAL over its points bit for bit: the 5-point
 * solver keeps the reference's candidate (rpoly's order) and scoring is the one-chunk exact form.
 * On such a context work: usac_multi_hypothesize_score (dlt_mode is ignored), usac_multi_run,
 * usac_multi_inliers, usac_multi_polish, usac_multi_run_polished, usac_multi_draw_samples,
 * usac_multi_run_prosac and usac_multi_prosac_scan, with the contracts they have for H / F.
 * USAC_ERR_UNSUPPORTED, before any device call: usac_multi_lo, usac_multi_run_lo, usac_multi_sprt_setup,
 * usac_multi_hypothesize_score_sprt, usac_multi_run_sprt, usac_multi_grid,
 * usac_multi_draw_samples_napsac, usac_multi_hypothesize_score_napsac and usac_multi_run_napsac.
 * LO-RANSAC on such a context has entries of its own (ABI 23): usac_multi_lo_essential and
 * usac_multi_run_lo_essential.
 * The solve's workspace is ~1.2 KB per sample; a round of more than 131 072 samples is solved in slices
 * of whole problems (USAC_MULTI_E5_SLICE in the environment at creation lowers the cap, for tests);
 * the results do not depend on the slice.
 * A caller with pixel coordinates and intrinsics uses usac_multi_create_essential_pixels (ABI 24). */
int usac_multi_create_essential(usac_multi **out, int device, const float *pts, const uint32_t *offsets, uint32_t P);
/* usac_multi_create_essential from pixel coordinates (ABI 24).  pts_px: N_total rows (u1, v1, u2, v2) in
 * pixels; K1, K2: P x 9 fp32, problem p's intrinsics of view 1 and view 2, row-major
 * k[0..8] = fx, s, cx, 0, fy, cy, 0, 0, 1; K2 == NULL: both views use K1.  The rows are converted on the
 * device, in place, in fp32 in this order (no contraction, correctly rounded division):
 *   y = (v - cy) / fy,  x = ((u - cx) - s * y) / fx      view 1 under K1_p, view 2 under K2_p
 * and the context keeps (x1, y1, x2, y2) alone, not the pixels.  The result is an essential multi context
 * over those rows: every call behaves as on usac_multi_create_essential over them, bit for bit.
 * USAC_ERR_ARG, before any device call: everything usac_multi_create_essential refuses, a NULL K1, and any
 * K with a non-finite entry, fx <= 0, fy <= 0, k[3], k[6] or k[7] != 0, or k[8] != 1. */
int usac_multi_create_essential_pixels(usac_multi **out, int device, const float *pts_px, const uint32_t *offsets,
                                       uint32_t P, const float *K1, const float *K2);
/* Per-problem thresholds from pixel tolerances, on a context from usac_multi_create_essential_pixels (ABI 24).
 * t_px: n tolerances in pixels, n == 1 (one for all problems) or n == P.  Problem p's threshold is, in fp32,
 *   f_p = ((fx1 + fy1) + (fx2 + fy2)) * 0.25f,  r = t / f_p,  thr_p = r * r
 * computed on the host and installed as by usac_multi_set_thresholds: usac_multi_get_thresholds returns the
 * values, usac_multi_set_thresholds(mc, NULL) clears them, and every contract of ABI 22 holds.
 * The value is compared with the essential residual as it is, the mean of the two point-to-epipolar-line
 * distances in calibrated units (EssentialEstimator::GetError, not squared): thr_p admits t^2 / f_p pixels of
 * it, so t = 45 at f = 1000 gives the 0.002 that 2 pixels of distance are (Pixel coordinates).
 * USAC_ERR_ARG, with nothing changed: a NULL mc or t_px, n other than 1 or P, a tolerance that is not finite
 * and > 0, or a thr_p that is not finite and > 0.  USAC_ERR_UNSUPPORTED on a context not created from pixels. */
int usac_multi_set_pixel_thresholds(usac_multi *mc, const float *t_px, uint32_t n);
/* The pixel-space models of a context from usac_multi_create_essential_pixels (ABI 24): E, F: P x 9,
 * F_p = K2_p^-T E_p K1_p^-1 in fp64 on the host (P x 9 values earn no launch).  The inverse of K is the closed
 * form 1/fx, -s/(fx fy), (s cy - cx fy)/(fx fy); 0, 1/fy, -cy/fy; 0, 0, 1 from the fp32 entries widened to
 * fp64; G = E K1^-1, then F = K2^-T G, every entry a three-term sum taken left to right; no normalisation,
 * one cast to fp32 at the end.  E and F may be the same array.
 * USAC_ERR_ARG for a NULL argument, USAC_ERR_UNSUPPORTED on a context not created from pixels. */
int usac_multi_pixel_models(usac_multi *mc, const float *E, float *F);
/* The context's resident points (ABI 24): out holds N_total x 4 floats, the rows every kernel of the context
 * reads, by a device-to-host copy -- on a context from usac_multi_create_essential_pixels the calibrated rows
 * the conversion wrote.  Any multi context.  USAC_ERR_ARG for a NULL argument. */
int usac_multi_get_points(usac_multi *mc, float *out);
/* Device input (ABI 25): P problems as padded device memory of `device`, n_max columns each, in one of two forms.
 * Form a, rows: rows is P x n_max x 4 fp32, contiguous and 16-byte aligned, with valid (P x n_max bytes, nonzero
 * keeps the row) or counts (P int32, the first counts[p] rows of problem p are kept) or neither (all rows are
 * kept).  Form b, matches: kpts0 is P x n_max x 2 fp32, kpts1 P x n1 x 2 fp32, match P x n_max int32; column j is
 * kept when match[p, j] >= 0 and its row is (kpts0[p, j], kpts1[p, match[p, j]]); two columns may share a target.
 * The pointers of the form not used are NULL (and n1 is 0 in form a). */
typedef struct usac_multi_device_input {
    uint32_t P, n_max;
    const float *rows; const uint8_t *valid; const int32_t *counts;      /* form a */
    const float *kpts0, *kpts1; uint32_t n1; const int32_t *match;       /* form b */
    const float *K1, *K2;  /* HOST, P x 9 each, essential only: pixels -> calibrated as ABI 24; NULL: rows are used as they are */
    void *stream;          /* the hipStream_t that orders the producer's writes; NULL: the null stream */
} usac_multi_device_input;
/* A multi context of USAC_HOMOGRAPHY, USAC_FUNDAMENTAL or USAC_ESSENTIAL problems (line: USAC_ERR_UNSUPPORTED)
 * from device input.  The device packs every problem's kept rows, in ascending column order, into the concatenated
 * N_total x 4 rows and offsets[P + 1] all multi contexts hold, and keeps per packed row the column it came from.
 * Rows are moved, not computed with: every bit arrives as it was.  With K1 (K2 == NULL: K1 for both views) the
 * packed rows are then converted as by usac_multi_create_essential_pixels, and usac_multi_set_pixel_thresholds /
 * usac_multi_pixel_models work.  The result is an ordinary multi context: every usac_multi_* call works on it,
 * and per problem it equals, bit for bit, a context created from the host over the kept rows.
 * Every kernel that reads the caller's memory is enqueued on in->stream, behind the work that produced it, and
 * the call waits for that stream: when it returns the context holds its own copy.
 * USAC_ERR_ARG before any device call: a NULL out or in, P == 0 or > 65535, n_max == 0, P * n_max >= 2^32, both
 * forms or neither, valid together with counts, form b with n1 == 0 or a NULL among its three pointers, K1 or K2
 * with an estimator other than USAC_ESSENTIAL, K2 without K1, a K usac_multi_create_essential_pixels refuses.
 * USAC_ERR_ARG before any launch: a pointer that is not device memory of `device` (hipPointerGetAttributes), is
 * misaligned, or whose allocation is too short.  USAC_ERR_ARG after the counting pass, with nothing kept: a
 * problem with fewer kept rows than the sample size, counts[p] < 0 or > n_max, a match index >= n1 (it is never
 * dereferenced).  *out is NULL after any failure; the reason, naming the argument or the first offending
 * problem, goes to stderr and is what usac_multi_last_error(NULL) returns to the calling thread until its next
 * usac_multi_create_device. */
int usac_multi_create_device(usac_multi **out, int device, int estimator, const usac_multi_device_input *in);
/* The context's offsets (ABI 25): offsets[P + 1], host.  Any multi context; what a caller of
 * usac_multi_create_device sizes its arrays by (N_total = offsets[P]).  USAC_ERR_ARG for a NULL argument. */
int usac_multi_get_offsets(const usac_multi *mc, uint32_t *offsets);
/* Device input in quality order (ABI 26): usac_multi_create_device with the kept columns of every problem sorted
 * by a score per column before anything else sees them -- what usac_multi_run_prosac expects of its input, from
 * a matcher that emits matches in keypoint order and a score per keypoint.  scores[p, j] is the quality of column j
 * of problem p: P x n_max fp32 of device memory of `device`, 4-byte aligned, checked as every pointer of `in` and
 * read on in->stream.  The order within problem p:
 *   - the better score first: the larger with descending != 0 (a confidence), the smaller with 0 (a distance);
 *   - equal scores in ascending column order; +0 and -0 are equal;
 *   - +inf and -inf are ordinary numbers;
 *   - a NaN, whatever its sign or payload, after every number in either direction, in ascending column order;
 *   - scores of columns that are not kept are never looked at.
 * In numpy, for the kept columns cols (ascending) and k = scores[p, cols]:
 *   nan = isnan(k); k2 = where(nan, 0, k); order = lexsort((cols, -k2 if descending else k2, nan)).
 * The sort is stable and deterministic.  Rows are moved, not computed with; with K1 / K2 the conversion runs
 * after the sort, on the sorted rows. */
typedef struct usac_multi_device_order {
    const float *scores;   /* DEVICE, P x n_max fp32: the quality of column j of problem p */
    int descending;        /* nonzero: larger is better; 0: smaller is better */
} usac_multi_device_order;
/* usac_multi_create_device over `in`, the kept rows of every problem in the order above.  Everything
 * usac_multi_create_device refuses is refused here with the same code at the same stage; also USAC_ERR_ARG before
 * any device call for a NULL order or order->scores, and before any launch for scores that are not device memory
 * of `device`, misaligned, or an allocation too short.  The result is an ordinary device-input context:
 * usac_multi_get_offsets, usac_multi_get_source (the sorted order) and usac_multi_padded_mask work on it, and per
 * problem it equals, bit for bit, a context created from the host over the kept rows in that order.
 * usac_multi_run_prosac keeps refusing problems of 20 points or fewer.  A refusal is reported as
 * usac_multi_create_device's, under this entry's name. */
int usac_multi_create_device_sorted(usac_multi **out, int device, int estimator, const usac_multi_device_input *in,
                                    const usac_multi_device_order *order);
/* The column of every packed row (ABI 25): src[N_total], host; row offsets[p] + i of the context is column
 * src[offsets[p] + i] of problem p's padded input: ascending within a problem on a context from
 * usac_multi_create_device, in quality order (ABI 26) on one from usac_multi_create_device_sorted.
 * USAC_ERR_UNSUPPORTED on a context created from the host, USAC_ERR_ARG for a NULL argument. */
int usac_multi_get_source(usac_multi *mc, uint32_t *src);
/* A mask over the packed rows back in the padded layout (ABI 25).  mask: HOST, N_total bytes, what
 * usac_multi_inliers, usac_multi_polish or a polished run wrote; d_out: P x n_max bytes of device memory of the
 * context's device (checked as usac_multi_create_device's pointers).  out[p, src[i]] = mask[i], every other cell
 * 0.  The upload, the memset and the scatter are enqueued on `stream` (a hipStream_t; NULL: the null stream) and
 * the call waits for it.  Stateless: it scatters the host mask it is given, whichever call wrote it, and its
 * upload ends the context's resident result; usac_multi_export_device (ABI 27) is the alternative that writes
 * the last polishing call's mask from the device, with nothing N_total-sized crossing.  USAC_ERR_UNSUPPORTED on
 * a context not created by usac_multi_create_device, USAC_ERR_ARG for a NULL mc, mask or d_out. */
int usac_multi_padded_mask(usac_multi *mc, const uint8_t *mask, uint8_t *d_out, void *stream);
/* Device output (ABI 27).  A multi context remembers that its device buffers hold the complete result of its
 * last polishing call: usac_multi_polish, usac_multi_run_polished, or usac_multi_run_prosac, _run_lo,
 * _run_lo_essential, _run_sprt or _run_napsac with a non-NULL pol.  Complete includes the problems the polish
 * defers to its host path (more than 16 384 points, or a list to fit above 4 096): their results and mask bytes
 * are written back to the device, so the resident bytes equal what the caller received.  The result stops being
 * valid through usac_multi_inliers and usac_multi_padded_mask (both write the mask buffer), through a polishing
 * call that computed no mask (mask == NULL with resident mode off), and through a polishing call that failed
 * after it passed its argument checks (a call refused for its arguments changes nothing).
 * usac_multi_set_resident: resident mode, off at creation.  While on, a polishing call whose mask argument is
 * NULL still computes the device mask (a deferred problem's on the host, uploaded) and copies no mask to the
 * host: nothing N_total-sized crosses.  While off every call behaves as before ABI 27.  Returns USAC_OK, or
 * USAC_ERR_ARG for a NULL mc. */
int usac_multi_set_resident(usac_multi *mc, int on);
typedef struct usac_multi_device_output {
    uint32_t n_max;        /* columns per problem of mask */
    uint32_t k_max;        /* entries per problem of inlier_cols; 0 with a NULL inlier_cols */
    float   *models;       /* DEVICE, P x 9: the polished model (usac_multi_polish_output.model) */
    float   *pixel_models; /* DEVICE, P x 9: F_p = K2_p^-T E_p K1_p^-1, contexts with intrinsics only */
    int32_t *inliers;      /* DEVICE, P: the polished model's inlier count, never truncated */
    int32_t *status;       /* DEVICE, P: usac_multi_polish_output.status */
    uint8_t *mask;         /* DEVICE, P x n_max bytes of 0 / 1 */
    int32_t *inlier_cols;  /* DEVICE, P x k_max: the inliers' columns, -1 behind the last */
    void    *stream;       /* hipStream_t the writes are enqueued on; NULL: the null stream */
} usac_multi_device_output;
/* The resident result of the last polishing call, written into the caller's device memory by one launch on
 * o->stream (one workgroup per problem, no memset before it); the call waits for that stream.  Every pointer is
 * nullable, not all of them.
 *   mask[p, src[offsets[p] + i]] = the resident mask byte of packed row offsets[p] + i, every other cell of row p
 *     0: what usac_multi_padded_mask writes from the host mask.
 *   inlier_cols[p, :]: the columns src[offsets[p] + i] of problem p's inlier rows in packed-row order -- ascending
 *     columns on a context from usac_multi_create_device, quality order on one from
 *     usac_multi_create_device_sorted.  The first min(inliers[p], k_max) are written, every later entry is -1;
 *     inliers[p] stays the full count, so a truncation shows.
 *   A context created from the host has no src: its source is the identity, a column is an index local to the
 *     problem, and n_max may be any value >= max n_p.  A context from device input demands its own n_max.
 *   pixel_models: the bits usac_multi_pixel_models returns for the exported models (fp64, the closed-form
 *     inverse of K, G = E K1^-1 then F = K2^-T G, three-term sums left to right, one cast to fp32), on a context
 *     with intrinsics (usac_multi_create_essential_pixels, usac_multi_create_device with K1).  The intrinsics go
 *     to the device once, at the first export that asks for them.
 *   A problem with USAC_ERR_NO_MODEL exports its start model, a count of 0, a zero mask row and a row of -1: the
 *     resident bytes.
 * USAC_ERR_ARG before any device call: a NULL mc or o, every pointer NULL, n_max == 0 or not the context's (from
 * the host: below max n_p), k_max == 0 with inlier_cols or k_max != 0 without, P * n_max or P * k_max >= 2^32.
 * USAC_ERR_UNSUPPORTED before any device call: no valid resident result (the message names the call that ended
 * it, or says that no polishing call has run); pixel_models on a context without intrinsics.  USAC_ERR_ARG before
 * any launch, nothing written: a pointer that is not device memory of the context's device, is misaligned (4
 * bytes for the float and int arrays), or whose allocation is too short.  The reason is what
 * usac_multi_last_error returns. */
int usac_multi_export_device(usac_multi *mc, const usac_multi_device_output *o);
/* Pose (ABI 28): the rotation and translation direction of an essential context's models, chosen on the device.
 * The rule, for problem p with its model E (9 fp32 values, widened to fp64), its calibrated rows (x1 y1 x2 y2,
 * widened likewise) and a 0 / 1 mask over them:
 *   1. U, V = the 3x3 SVD of E by row Jacobi with accumulated rotations, singular values descending, v3 = v1 x v2;
 *      P_j = [R | t] for j = 0..3 are the four projections of ProjectionsFromEssential (five_points.cpp:336-371):
 *      R = U W V^T for j = 0, 1 and U W^T V^T for j = 2, 3, W = [0 -1 0; 1 0 0; 0 0 1]; t = +u3 for even j, -u3
 *      for odd j.  The convention is the reference's: P_ref = [I | 0], so x2 ~ R x1 + t.  All fp64, no
 *      contraction, correctly rounded division and square root, in the operation order of the 5-point solver's
 *      cheirality test: the very text that test runs.
 *   2. count_j = the number of rows with a set mask byte that are in front of both cameras under P_j: the point
 *      triangulated as the null vector on the first ray (TriangulatePoint) has CalcDepth > 0 for P_ref and for
 *      P_j.  A row with a non-finite value is in front of nothing: it is skipped before the test.  (The
 *      comparisons alone would not say so: the triangulation takes the row of x2 or the row of y2, whichever has
 *      the larger norm, and a non-finite x2 beside a finite y2 loses that comparison and leaves a finite point.)
 *   3. choice = the j with the largest count_j, the lowest j on ties; -1 when the largest count is 0 or the
 *      problem's status is not USAC_OK (USAC_ERR_NO_MODEL in the resident result).
 *   4. s = +1 if the determinant of P_choice's 3x3 block (CalcDepth's cofactor expansion along the first row) is
 *      > 0, else -1.  R = s times that block (row-major) and t = s times the fourth column, each cast once to
 *      fp32; front = count_choice; front_mask = 1 exactly on the rows counted in count_choice.  With choice =
 *      -1: R the identity, t zero, front 0, the mask row zero.
 * det R = +1: U's columns are the rows of a product of plane rotations taken in the order of the sorted singular
 * values, so det U is the sign of that permutation -- +1 or -1 --, V's third column is the cross product of its
 * first two (det V = +1) and det W = 1.  P and -P are one camera, CalcDepth already multiplies by the sign of the
 * determinant so that the counts do not depend on it, and s picks the one of the two whose block is a rotation.
 * |t| = 1; the scale of the translation is not observable.
 * One launch, one workgroup per problem, any n_p: nothing is deferred to the host, the counts are integers and
 * the result does not depend on the order of anything. */
typedef struct usac_multi_pose_output {
    uint32_t n_max;      /* columns per problem of front_mask, as usac_multi_device_output.n_max */
    float   *R;          /* DEVICE, P x 9, row-major */
    float   *t;          /* DEVICE, P x 3 */
    int32_t *front;      /* DEVICE, P: count_choice */
    int32_t *choice;     /* DEVICE, P: 0..3, or -1 */
    uint8_t *front_mask; /* DEVICE, P x n_max bytes of 0 / 1, a row's byte at its source column */
    void    *stream;     /* hipStream_t the launch is enqueued on; NULL: the null stream */
} usac_multi_pose_output;
/* The rule above over the resident result of the last polishing call (usac_multi_export_device says what is
 * resident and what ends it): E and the status of problem p are its polished result's, the mask is the resident
 * inlier mask.  One launch on o->stream, which the call waits for; the workgroup clears its own front_mask row,
 * no memset comes first.  Every pointer is nullable, not all of them.  The call reads the resident result and
 * leaves it as it is.  USAC_ERR_UNSUPPORTED before any device call on a homography or fundamental context, and
 * when no result is resident (usac_multi_export_device's message); USAC_ERR_ARG before any device call for a NULL
 * mc or o, every pointer NULL, or an n_max usac_multi_export_device would refuse; USAC_ERR_ARG before any launch,
 * nothing written, for a pointer that is not device memory of the context's device, is misaligned or too short. */
int usac_multi_pose_device(usac_multi *mc, const usac_multi_pose_output *o);
/* The same kernel from host arrays, for models of the caller's own: E P x 9; mask N_total bytes over the packed
 * rows, NULL: every row; every status counts as USAC_OK.  R P x 9, t P x 3, front P, choice P and front_mask
 * (N_total bytes in packed-row order, like every host mask) are host arrays, each nullable, not all of them.
 * The call uses buffers of its own: the resident result stays as it is.  USAC_ERR_UNSUPPORTED before any device
 * call on a homography or fundamental context, USAC_ERR_ARG for a NULL mc or E or when every output is NULL. */
int usac_multi_pose(usac_multi *mc, const float *E, const uint8_t *mask, float *R, float *t, int32_t *front,
                    int32_t *choice, uint8_t *front_mask);
/* Pose refinement (ABI 29): a pose (R, t) of an essential context's problem refined on the device, a few
 * Levenberg-Marquardt steps on its five parameters over the Sampson distances of the masked rows.  All arithmetic
 * is fp64, no contraction, correctly rounded division and square root and no other library function (DESIGN.md
 * §4); every expression below is evaluated as it is bracketed, left to right otherwise.
 * Inputs, for problem p: a start R0 (9 fp32, row-major) and t0 (3 fp32), widened to fp64; its calibrated rows
 * (x1 y1 x2 y2, fp32, widened); a 0 / 1 mask over the rows; a status.  A row is USED when its mask byte is set and
 * its four values are finite.  The problem is SKIPPED when its status is not USAC_OK, a value of R0 or t0 is not
 * finite, t0 is the zero vector, or fewer than 5 rows are used: R and t are then the inputs' bits, E is zero, cost0
 * and cost are 0, iterations is -1, used is the number of used rows.  (usac_multi_pose_device's choice = -1 output,
 * R the identity and t zero, is skipped by this without a special case.)
 *   Helpers.  unit(v) = v / sqrt((v0 v0 + v1 v1) + v2 v2), one division per entry.  u x v = (u1 v2 - u2 v1,
 *     u2 v0 - u0 v2, u0 v1 - u1 v0).  [v]x M is the matrix whose column c is v x (column c of M).  [e_j]x M is
 *     exact: rows (0, -M2, M1) for j = 0, (M2, 0, -M0) for j = 1, (-M1, M0, 0) for j = 2, M0..M2 the rows of M.
 *   Start.  t = unit(t0); R = R0 as given.  R is not re-orthonormalised: an fp32 rotation has det R - 1 of about
 *     2e-8, and left multiplication by exact rotations keeps it there.
 *   Frame at (R, t).  k = the lowest index of the smallest |t_k|; c = t x e_k written out -- (0, t2, -t1), (-t2, 0,
 *     t0) or (t1, -t0, 0) --; b1 = unit(c), b2 = t x b1.  E = [t]x R.  D_j = [t]x ([e_j]x R) for j = 0, 1, 2 (a
 *     left perturbation of R), D_3 = [b1]x R, D_4 = [b2]x R.
 *   Per used row.  For a matrix M: M x1 has the entries (M_r0 x1 + M_r1 y1) + M_r2, and (M^T x2)_c = (M_0c x2 +
 *     M_1c y2) + M_2c.  a = E x1; b = the first two entries of E^T x2; C = (x2 a0 + y2 a1) + a2; S = ((a0 a0 +
 *     a1 a1) + b0 b0) + b1 b1.  A row whose S is not > 0 contributes nothing in that pass.  s = sqrt(S), r = C / s:
 *     the signed Sampson distance (the standard one, not EssentialEstimator::GetError, which the inlier test uses;
 *     the mask is an input and is never re-evaluated).  For j = 0..4, with u = D_j x1 and v = the first two
 *     entries of D_j^T x2: num = (x2 u0 + y2 u1) + u2, q = ((a0 u0 + a1 u1) + b0 v0) + b1 v1 and
 *     J_j = num / s - (r q) / S, the full derivative, the denominator's included.
 *   One pass gives 21 sums over the contributing rows: H_jk = sum J_j J_k for j <= k (H is symmetric), g_j = sum
 *     J_j r, c = sum r r.  The order of summation is part of the rule: thread T of 256 adds its rows i = T, T +
 *     256, ... in ascending order into an accumulator that starts at +0; the 64 lane values of a wave are combined
 *     by the xor butterfly with offsets 32, 16, 8, 4, 2, 1 (v = v[:32] + v[32:], then v[:16] + v[16:], ...); the
 *     four wave totals as (w0 + w1) + (w2 + w3).  No atomics.
 *   Loop.  lambda = 1e-3.  The first pass, at the start pose, gives (H, g, c) and cost0 = c; iterations = 0.  While
 *     iterations < max_iters:
 *       Solve (H + lambda diag H) d = -g: A_jj = H_jj + lambda H_jj, the rest of A is H; Cholesky A = L L^T by
 *       columns j = 0..4: p = A_jj - L_j0 L_j0 - ... (k ascending), a pivot p that is not > 0 REJECTS without a
 *       pass; L_jj = sqrt(p), L_ij = (A_ij - L_i0 L_j0 - ...) / L_jj for i > j.  y_i = (-g_i - L_i0 y_0 - ...) /
 *       L_ii for i = 0..4, then d_i = (y_i - L_(i+1)i d_(i+1) - ...) / L_ii (k ascending) for i = 4..0.
 *       Trial pose: q = (d0 / 2, d1 / 2, d2 / 2) (a multiplication by 0.5), w = 1 / sqrt(((1 + qx qx) + qy qy) +
 *       qz qz), x = qx w, y = qy w, z = qz w, Q = [1 - 2 (y y + z z), 2 (x y - w z), 2 (x z + w y); 2 (x y + w z),
 *       1 - 2 (x x + z z), 2 (y z - w x); 2 (x z - w y), 2 (y z + w x), 1 - 2 (x x + y y)]; R'_rc = (Q_r0 R_0c +
 *       Q_r1 R_1c) + Q_r2 R_2c; t' = unit((t_k + d3 b1_k) + d4 b2_k).
 *       One pass at (R', t'), with the frame rebuilt there, gives (H', g', c'); iterations += 1.
 *       ACCEPT if c' < c (a NaN c' rejects): the primed values and their frame become the current ones, lambda =
 *       max(lambda / 10, 1e-12); stop if c - c' <= 1e-12 c or max |d_j| < 1e-10, c the old cost.
 *       REJECT otherwise: lambda = 10 lambda, stop if lambda > 1e8; the kept (H, g) are solved again, no pass is
 *       repeated.
 *     So a call runs iterations + 1 passes; a rejection by the pivot runs none and is bounded by lambda alone.
 *     With max_iters = 0 the outputs are the normalised start, cost = cost0 and iterations = 0.
 *   Outputs.  R and t, each cast once to fp32; E, the nine entries of [t]x R in fp64 cast once (a model
 *     usac_multi_inliers or usac_multi_pose takes); cost0 and cost, fp64, cost <= cost0 by construction; iterations
 *     and used, int32.
 * On 5 or 6 noisy rows a 5-parameter fit follows the noise, as any does: the cost falls, the pose need not improve.
 * One launch, one 256-thread workgroup per problem, any n_p, the whole loop inside the kernel. */
typedef struct usac_multi_refine_io {
    uint32_t n_max;        /* columns per problem of mask_in, as usac_multi_device_output.n_max */
    uint32_t max_iters;    /* 0..100 trial steps; 10 is the documented default */
    const float   *R_in;   /* DEVICE, P x 9, row-major: the start rotations */
    const float   *t_in;   /* DEVICE, P x 3: the start translations, any non-zero length */
    const uint8_t *mask_in;/* DEVICE, P x n_max bytes of 0 / 1, a row's byte at its source column (front_mask of
                            * usac_multi_pose_output); NULL: the resident inlier mask */
    float   *R;            /* DEVICE, P x 9; may be R_in */
    float   *t;            /* DEVICE, P x 3; may be t_in */
    float   *E;            /* DEVICE, P x 9: [t]x R */
    double  *cost0;        /* DEVICE, P doubles, 8-byte aligned: the cost at the start */
    double  *cost;         /* DEVICE, P doubles, 8-byte aligned: the cost at the output */
    int32_t *iterations;   /* DEVICE, P: the trial poses evaluated, -1: skipped */
    int32_t *used;         /* DEVICE, P: the used rows */
    void    *stream;       /* hipStream_t the launch is enqueued on; NULL: the null stream */
} usac_multi_refine_io;
/* The rule above for every problem of an essential context, the status of problem p being that of the resident
 * result of the last polishing call (usac_multi_export_device says what is resident and what ends it), the mask
 * mask_in or, with NULL, the resident inlier mask.  One launch on o->stream, which the call waits for.  The inputs
 * R_in and t_in may be the very pointers R and t: a workgroup reads its problem's start before it writes anything.
 * Every output pointer is nullable, not all of them.  The call reads the resident result and leaves it as it is.
 * USAC_ERR_UNSUPPORTED before any device call on a homography or fundamental context, and when no result is
 * resident; USAC_ERR_ARG before any device call for a NULL mc, o, R_in or t_in, max_iters > 100, every output
 * NULL, or an n_max usac_multi_export_device would refuse; USAC_ERR_ARG before any launch, nothing written, for a
 * pointer that is not device memory of the context's device, is misaligned or too short. */
int usac_multi_refine_pose_device(usac_multi *mc, const usac_multi_refine_io *o);
/* The same kernel from host arrays: R P x 9, t P x 3; mask N_total bytes over the packed rows, NULL: every row;
 * every status counts as USAC_OK.  R_out P x 9, t_out P x 3, E_out P x 9, cost0 P, cost P, iterations P and used P
 * are host arrays, each nullable, not all of them; R_out may be R and t_out may be t.  The call uses buffers of its
 * own: the resident result stays as it is.  USAC_ERR_UNSUPPORTED before any device call on a homography or
 * fundamental context, USAC_ERR_ARG for a NULL mc, R or t, max_iters > 100 or when every output is NULL. */
int usac_multi_refine_pose(usac_multi *mc, const float *R, const float *t, const uint8_t *mask, uint32_t max_iters,
                           float *R_out, float *t_out, float *E_out, double *cost0, double *cost, int32_t *iterations,
                           int32_t *used);
void usac_multi_destroy(usac_multi *mc);
/* The message of the context's last failed call; mc == NULL: "null context", or see usac_multi_create_device. */
const char *usac_multi_last_error(const usac_multi *mc);
uint32_t usac_multi_num_problems(const usac_multi *mc);
/* Per-problem thresholds (ABI 22).  thr: P finite values > 0, problem p's inlier threshold in the units of
 * its own coordinates (E: the squared Sampson distance in calibrated coordinates, so (t_px / f)^2 for a
 * pixel tolerance t_px and focal length f); NULL clears them.  While they are set, every usac_multi_*
 * call that reads a threshold -- the rounds, the runs, usac_multi_inliers, usac_multi_polish (its host
 * path for a problem past the caps included), usac_multi_prosac_scan, usac_multi_lo -- uses thr[p] for
 * problem p, whatever its place in an active list, and does not read its scalar (the thr argument or
 * params->threshold); the LO threshold of problem p starts at thr[p], returns to thr[p] and steps by
 * (thr[p] * lo_threshold_multiplier - thr[p]) / lo_iterative_iterations.  They are state of the context: they persist from call to call
 * until cleared, and after a clear every call behaves as before ABI 22.  usac_multi_lo's persistent
 * state is not touched: reset it after changing the thresholds.
 * USAC_ERR_ARG for a NULL mc, or a value that is not finite and > 0 (the context and the thresholds set
 * before stay as they were; usac_multi_last_error names the first bad problem). */
int usac_multi_set_thresholds(usac_multi *mc, const float *thr);
/* Returns 1 and fills out[P] if thresholds are set, 0 (out untouched) if not, USAC_ERR_ARG on a NULL mc. */
int usac_multi_get_thresholds(const usac_multi *mc, float *out);
/* One round.  problems: the active list, n_problems problem ids in any order (NULL: all P in order,
 * n_problems = P or 0).  samples: host n_problems x R x m indices local to each problem (out of
 * range: USAC_ERR_ARG), or NULL for the device sampler with seeds[i] for problems[i].  R: a multiple
 * of 64 in 64..8192 (a wave never spans two problems).  counts / sums (nullable): n_problems x R x S,
 * S = 3 for the fundamental solver, else 1 (essential: count -1 on a sample without a model).  best (nullable): n_problems records, each the round's
 * best of its problem under Score::bigger with the earliest (sample, slot) on exact ties,
 * hyp_index = first_hyp + sample.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and thr is not read. */
int usac_multi_hypothesize_score(usac_multi *mc, const uint32_t *problems, uint32_t n_problems,
                                 const int32_t *samples, uint32_t R, const uint64_t *seeds, uint64_t first_hyp,
                                 float thr, int dlt_mode, int32_t *counts, float *sums, usac_record *best);
/* Batch-granular RANSAC with the standard termination criterion, all problems together: in round
 * r = 0, 1, ... every still-active problem evaluates hypotheses [r R, (r + 1) R) (device sampler,
 * seeds[p]; seeds == NULL: params->seed + p), its running best is merged by usac_merge_records'
 * order, bound_p = usac_std_termination(best.inliers, n_p, m, desired_prob, max_iterations), and the
 * problem is finished once (r + 1) R >= min(max_iterations, bound_p).  The clamp to max_iterations is
 * a deviation from ransac.cpp, which lets the bound exceed it: a batch call must stay bounded.  A run
 * evaluates at least as many hypotheses as the bound asks for, so the confidence guarantee holds.
 * This is NOT the glibc-stream Ransac::run (usac_ransac_run): no NAPSAC, SPRT is usac_multi_run_sprt's, PROSAC is
 * usac_multi_run_prosac's and LO is usac_multi_run_lo's -- params->sprt, ->lo or a sampler other than USAC_SAMPLER_UNIFORM return
 * USAC_ERR_UNSUPPORTED here -- and it stops at the best minimal model; usac_multi_run_polished adds
 * the run's non-minimal polish.
 * Reads threshold, desired_prob, max_iterations, dlt_mode, seed and batch (= R, 0 = 256).
 * out: P results.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and params->threshold is not read. */
int usac_multi_run(usac_multi *mc, const usac_params *params, const uint64_t *seeds, usac_multi_output *out);
/* Per-point inlier flags of each problem's model (models P x 9, mask N_total bytes of 0 / 1, counts
 * P, nullable) from the residual of usac_get_inliers; for H, H^-1 is the device inv3x3 of the given H.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and thr is not read. */
int usac_multi_inliers(usac_multi *mc, const float *models, float thr, uint8_t *mask, int32_t *counts);

/* One problem's result of usac_multi_polish (ABI 16). */
typedef struct usac_multi_polish_output {
    float   model[9];          /* best model after the polish (= the start model when no pass is accepted) */
    int32_t inliers;  float score;                  /* its count and sequential Σ at thr */
    int32_t minimal_inliers; float minimal_score;   /* the start model's */
    int32_t passes;            /* accepted passes, 0..4 */
    int32_t status;            /* USAC_OK, or USAC_ERR_NO_MODEL when the start model has no inlier */
} usac_multi_polish_output;

/* The end of Ransac::run (ransac.cpp:157-214) for every problem, from its start model (models: P x 9):
 * getInliers(start) gives the list and its count c0; then up to four passes, each a non-minimal fit
 * (usac_nonminimal) on the first `best` entries of the current list and a getInliers of the fitted
 * model -- stopped by a failed fit, by (float)c / (float)best < 0.8 or by c <= the last accepted
 * count, otherwise the fitted model, its count, Σ and list are accepted -- and the final getInliers
 * of the accepted model.  c0 = 0: status USAC_ERR_NO_MODEL, the start model returned, no fit.  Every
 * value has the bits the same loop over usac_get_inliers / usac_nonminimal of a usac_ctx over the
 * problem's points gives.  One launch, one workgroup per problem, for n_p <= 16384 and lists to fit of
 * <= 4096 points; a problem past either cap is polished through a temporary single context over its
 * points (same result, a host loop for that problem only).
 * out: P results.  mask (nullable): N_total bytes of 0 / 1, the final getInliers of out[p].model.
 * NULL mc, models or out: USAC_ERR_ARG before any device call.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and thr is not read. */
int usac_multi_polish(usac_multi *mc, const float *models, float thr,
                      usac_multi_polish_output *out, uint8_t *mask);

/* usac_multi_run, then the polish of every problem's best model at params->threshold without the
 * records leaving the device in between; out as usac_multi_run writes it (unchanged), pol / mask as
 * usac_multi_polish (a problem without a model: USAC_ERR_NO_MODEL in both).  The remaining deviations
 * from Ransac::run are usac_multi_run's: no NAPSAC (PROSAC: usac_multi_run_prosac, LO:
 * usac_multi_run_lo, SPRT: usac_multi_run_sprt), batch-granular termination.
 * NULL mc, params, out or pol: USAC_ERR_ARG before any device call.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and params->threshold is not read. */
int usac_multi_run_polished(usac_multi *mc, const usac_params *params, const uint64_t *seeds,
                            usac_multi_output *out, usac_multi_polish_output *pol, uint8_t *mask);

/* ---- multi-problem batches: PROSAC (ABI 17) ---------------------------------------------------------
 * The sampler in closed form.  With g = the reference's growth function of (n, m) (prosac_sampler.hpp:
 * 62-114), ProsacSampler::generateSample's subset after the call with hypCount = t is
 *     s(t) = min(n, m + #{ i in [m - 1, n) : g[i] < t }),  s(0) = m,
 * so the sampler is a pure function of two integers per problem, both fixed for a round: the clock T
 * (the sampler's hypCount, from 1) and the termination length L (from n_p).  Lane j of a round has
 * t = T + j and draws, from the (seed, global hypothesis index) stream of the uniform device sampler,
 *     t > 200000    : m distinct indices of [0, n_p)             (clock does not advance)
 *     s(t - 1) > L  : m distinct indices of the closed [0, L]    (clock does not advance; L < n_p)
 *     otherwise     : m - 1 distinct indices of [0, s(t) - 2] and point s(t) - 1  (a PROSAC lane)
 * The PROSAC lanes are a prefix of the round; after it T += their number, and largest_sample_size =
 * max(previous, s(T_old + n_prosac - 1)).
 *
 * usac_prosac_schedule: that rule for one problem and one round, on the host (no context, no device).
 * subset (nullable, R): s(t) of a PROSAC lane, 0 = uniform over [0, term_len], UINT32_MAX = uniform
 * over n.  largest (nullable): in = the previous value, out = the updated one.  USAC_ERR_ARG unless
 * 2 <= m <= term_len <= n and clock >= 1. */
int usac_prosac_schedule(uint32_t n, uint32_t m, uint32_t clock, uint32_t term_len, uint32_t R, uint32_t *subset,
                         uint32_t *clock_next, uint32_t *largest);
/* For tests: the samples the solve kernels of a round draw (the same device function), n_problems x R x
 * m indices local to each problem.  clock == NULL: the uniform sampler of usac_multi_hypothesize_score;
 * else the PROSAC sampler with clock[i] / term_len[i] for problems[i] (m <= term_len <= n_p).  problems,
 * R, seeds, first_hyp as usac_multi_hypothesize_score. */
int usac_multi_draw_samples(usac_multi *mc, const uint32_t *problems, uint32_t n_problems, uint32_t R,
                            const uint64_t *seeds, uint64_t first_hyp, const uint32_t *clock, const uint32_t *term_len,
                            int32_t *out);

/* One problem's PROSAC state at the end of usac_multi_run_prosac. */
typedef struct usac_multi_prosac_output {
    uint32_t termination_length;   /* ProsacTerminationCriteria's, n_p if no scan moved it */
    uint32_t largest_sample_size;  /* the sampler's */
    uint32_t clock;                /* the sampler's hypCount at the end */
    uint32_t scans;                /* rounds whose new best was scanned */
} usac_multi_prosac_output;

/* usac_multi_run with the PROSAC sampler and PROSAC's termination criterion (prosac_termination_
 * criteria.hpp:148-201) per problem.  Every problem's points are assumed sorted by descending quality
 * (not checked).  Per problem T = 1, L = n_p, largest = m, bound = max_iterations.  In round r every
 * active problem evaluates hypotheses [r R, (r + 1) R) drawn under its (T, L), and its running best is
 * merged as in usac_multi_run.  If the running best improved in the round, the device walks the
 * problem's points under the new best (inlier flags by the residual of usac_get_inliers, the running
 * count, non_random[i] = max(old, count_i) for i >= 20) and hands the host the raised points that end a
 * run of inliers, in order; the host evaluates them as the reference does (its libm's log, the
 * maximality samples, the minimum with its tie rule) with hypCount = best.hyp_index (0-based, as
 * usac_ransac_run passes it; uint32 wrap-around in hypCount - growth[i] kept) and largest_sample_size
 * at that hypothesis, which gives the new bound and L.  Then T and largest advance, and the problem is
 * finished once (r + 1) R >= min(max_iterations, bound).
 * Deviations from Ransac::run with PROSAC: batch granularity, two ways -- only a round's final best is
 * scanned (the reference scans every new best), and L changes only between rounds (the reference's next
 * sample already sees it); the clamp to max_iterations; the device random stream (the reference draws
 * from std::mt19937).  No NAPSAC; LO: usac_multi_run_lo, SPRT: usac_multi_run_sprt.
 * USAC_ERR_UNSUPPORTED for params->sprt or ->lo; USAC_ERR_ARG for a sampler other than
 * USAC_SAMPLER_PROSAC, any n_p <= 20 (the reference reads point 20), a bad batch or dlt_mode, NULL mc,
 * params or out -- all before any device call.
 * out: P results as usac_multi_run's (bound: the last scan's, max_iterations if none ran).  pro
 * (nullable): P states.  pol (nullable): the polish of usac_multi_run_polished from the device's running
 * records, with mask (nullable, read only with pol).
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and params->threshold is not read. */
int usac_multi_run_prosac(usac_multi *mc, const usac_params *params, const uint64_t *seeds, usac_multi_output *out,
                          usac_multi_prosac_output *pro, usac_multi_polish_output *pol, uint8_t *mask);
/* For tests: one termination scan of every problem, models (P x 9) taken as new bests found at
 * hypothesis hyp_count[p] with largest_sample_size largest[p], at params->threshold.  The termination
 * state persists in the context from call to call; reset != 0 (and any usac_multi_run_prosac) starts
 * it afresh from params->desired_prob and ->max_iterations.  bound / term_len: P values after the
 * scan.  n_cand (nullable): P candidate numbers; cand (nullable): N_total / 2 + P pairs (i, count),
 * problem p's from pair offsets[p] / 2 + p, ascending i.  Every n_p > 20.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and params->threshold is not read. */
int usac_multi_prosac_scan(usac_multi *mc, const usac_params *params, int reset, const float *models,
                           const uint32_t *hyp_count, const uint32_t *largest, uint32_t *bound, uint32_t *term_len,
                           uint32_t *n_cand, uint32_t *cand);

/* ---- multi-problem batches: LO-RANSAC (ABI 18) -------------------------------------------------------
 * The sample sets of the LO: k distinct integers of the closed range [0, max], in draw order --
 * UniformRandomGenerator::generateUniqueRandomSet(sample, max) with the reference's generator replaced
 * by the device sampler's SplitMix64 stream keyed by (seed, a fixed LO tag, draw), draw = the number of
 * sets drawn so far for the problem in the run.  The device draws through the same text.  No context,
 * no device.  USAC_ERR_ARG unless 1 <= k <= 64, k <= max + 1 and max < 2^31. */
int usac_lo_draw(uint64_t seed, uint64_t draw, uint32_t k, uint32_t max, int32_t *out);

/* One problem's LO state: the counters of a run (or since the last reset of usac_multi_lo). */
typedef struct usac_multi_lo_output {
    uint32_t lo_calls, inner_iters, iterative_iters, fits, improved, capped, draws;
    float threshold;  /* the LO threshold as the last call left it */
} usac_multi_lo_output;
/* lo_calls: LO calls on a new best (those that return at once for < 12 inliers included);
 * inner_iters / iterative_iters: the reference's "only for test" counters at their positions;
 * fits: non-minimal fits; improved: inner iterations whose model became the best; capped: calls ended
 * by the caps rule; draws: sets drawn. */

/* One LO call -- InnerLocalOptimization::GetModelScore (inner_local_optimization.hpp:74-133) with
 * IterativeLocalOptimization::GetScoreUnlimited / GetScoreLimited (iterative_local_optimization.hpp:
 * 61-136), params->lo = USAC_LO_INITLORSC / USAC_LO_INITFLORSC -- for every problem at once, one
 * workgroup per problem, every exit taken on the device.  recs[p] (in / out) is taken as a new best:
 * its model, and (inliers, score) as best_score; a record that is not valid or has < 12 inliers comes
 * back unchanged.  The list of the model's inliers is its getInliers at params->threshold, and the list's
 * own length stands for best_score's count wherever the reference sizes a sample by it (equal for a
 * record that holds its model's count).  Fits are usac_nonminimal's, scores usac_get_inliers' (count and
 * sequential Σ), comparisons Score::bigger's; on an improvement model, inliers and score change, hyp_index
 * and valid stay.  The LO threshold, the draw counter and the counters are per-problem state that
 * persists in the context from call to call (the threshold compounds as the reference's does); reset
 * != 0 (and any usac_multi_run_lo) starts them afresh.  seeds (nullable): P draw seeds, NULL =
 * params->seed + p.  lo (nullable): P states after the call.
 * The caps rule, a deviation: a problem of n_p > 16384 points, or an iterative-stage list to fit of
 * > 4096 points, ends that LO call there -- the best so far is kept, the threshold goes back to
 * params->threshold, capped is incremented.
 * Reads of params: threshold, seed, lo, sprt, lo_sample_size, lo_inner_iterations,
 * lo_iterative_iterations and lo_threshold_multiplier -- not sampler, batch, dlt_mode, desired_prob or
 * max_iterations.  USAC_ERR_UNSUPPORTED for USAC_LO_GC or params->sprt; USAC_ERR_ARG for USAC_LO_NONE,
 * lo_sample_size 0 or > 64, lo_iterative_iterations 0, NULL mc, params or recs -- all before any device
 * call.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and params->threshold is not read. */
int usac_multi_lo(usac_multi *mc, const usac_params *params, int reset, const uint64_t *seeds,
                  usac_record *recs, usac_multi_lo_output *lo);

/* usac_multi_run (params->sampler = USAC_SAMPLER_UNIFORM) or usac_multi_run_prosac (USAC_SAMPLER_PROSAC)
 * with LO-RANSAC: in every round, after the merge, each problem whose running best improved in the round
 * gets one LO call as usac_multi_lo's on the device, before the PROSAC scan (which therefore sees the
 * LO'd model: ransac.cpp:110-128) and before the records come down -- so the termination bound comes
 * from the LO'd count.  The LO'd record keeps the hyp_index of the minimal model it started from (later
 * merges, the "improved in this round" test and PROSAC's hypCount read it).
 * Deviations from Ransac::run: only a round's final best is optimised (the reference optimises every new
 * best); the LO draws come from the device stream (usac_lo_draw); the caps rule of usac_multi_lo; and
 * those of usac_multi_run / usac_multi_run_prosac.  No NAPSAC; SPRT (without LO): usac_multi_run_sprt.
 * USAC_ERR_UNSUPPORTED for USAC_LO_GC or params->sprt; USAC_ERR_ARG for USAC_LO_NONE, lo_sample_size 0
 * or > 64, lo_iterative_iterations 0, USAC_SAMPLER_NAPSAC, a bad batch or dlt_mode, NULL mc, params or
 * out, and with PROSAC any n_p <= 20 -- all before any device call.
 * out / pol / mask as usac_multi_run_prosac's; lo (nullable): P LO states; pro (nullable) is written
 * only with PROSAC.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and params->threshold is not read. */
int usac_multi_run_lo(usac_multi *mc, const usac_params *params, const uint64_t *seeds, usac_multi_output *out,
                      usac_multi_lo_output *lo, usac_multi_prosac_output *pro, usac_multi_polish_output *pol,
                      uint8_t *mask);

/* LO-RANSAC on a multi context of essential-matrix problems (usac_multi_create_essential; ABI 23).
 * usac_multi_lo_essential is usac_multi_lo and usac_multi_run_lo_essential is usac_multi_run_lo, each with
 * its contract word for word -- the params read, the error codes before any device call, the uniform or
 * the PROSAC sampler (PROSAC: every n_p > 20), the per-problem state, the caps rule, out / lo / pro / pol /
 * mask, per-problem thresholds -- on an essential context: the sample size every `<= m` test of the
 * reference reads is 5, a non-minimal sample is fitted by the 8-point algorithm
 * (essential_estimator.hpp:64-74: usac_nonminimal's fit on a usac_ctx of USAC_ESSENTIAL) and scored by the
 * squared Sampson distance in calibrated coordinates.  dlt_mode is ignored.  The 5-point solve of a round
 * is sliced as without LO (usac_multi_create_essential); the results do not depend on the slice.
 * They are entries of their own because usac_multi_lo / usac_multi_run_lo keep returning
 * USAC_ERR_UNSUPPORTED on an essential context.  On a homography or fundamental context these two return
 * USAC_ERR_UNSUPPORTED and name usac_multi_lo / usac_multi_run_lo.  No SPRT, no NAPSAC. */
int usac_multi_lo_essential(usac_multi *mc, const usac_params *params, int reset, const uint64_t *seeds,
                            usac_record *recs, usac_multi_lo_output *lo);
int usac_multi_run_lo_essential(usac_multi *mc, const usac_params *params, const uint64_t *seeds,
                                usac_multi_output *out, usac_multi_lo_output *lo, usac_multi_prosac_output *pro,
                                usac_multi_polish_output *pol, uint8_t *mask);

/* ---- multi-problem batches: SPRT verification (ABI 19) ----------------------------------------------
 * A batch-granular SPRT: every problem has its own test (epsilon, delta, A), fixed for a round of R
 * hypotheses; every slot of the round is verified on the device by usac_set_sprt's throughput test --
 * the reference's fp64 lambda walk (sprt.hpp:209-234) over the problem's pool-ordered points from the
 * slot tile's start (tile * 7919) mod n_p, the first 64 pool points by a wave per tile, the rest by a
 * workgroup per survivor.  A rejected slot reads count -1, sum 0 (never a best); an accepted one reads
 * its inliers over all n_p points and sum = (float)count (sprt.hpp:276-281).  Problem p's pool is the
 * reference's shuffle after srandom(pool_seed_p) (usac_sprt_pool).
 *
 * One problem's statistics of a round. */
typedef struct usac_multi_sprt_stats {
    uint32_t accepted;        /* slots accepted */
    uint32_t rejected_head;   /* slots rejected within the first min(n_p, 64) pool points' launch */
    uint32_t rejected_tail;   /* slots rejected past them */
    uint32_t head_inliers;    /* over the rejected_head slots: inliers seen up to the rejecting point */
    uint32_t head_points;     /* over the same slots: points tested up to it */
    uint32_t pad;
    uint64_t points_tested;   /* point tests done (a tail rejection counts to the end of its chunk) */
} usac_multi_sprt_stats;

/* One entry of a problem's test history (the reference's SPRT_history). */
typedef struct usac_multi_sprt_test {
    double epsilon, delta, A;
    int32_t k;                /* hypotheses evaluated under the previous test */
    int32_t pad;
} usac_multi_sprt_test;

/* One problem's SPRT state at the end of usac_multi_run_sprt. */
typedef struct usac_multi_sprt_output {
    double epsilon, delta, A; /* the last test */
    uint32_t tests;           /* tests designed, the first one included */
    uint32_t accepted;        /* slots accepted, over the run */
    uint32_t rejected;        /* slots rejected, over the run */
    uint32_t pad;
    uint64_t points_tested;   /* over the run */
} usac_multi_sprt_output;

/* Builds the problems' pools on the host (pool_seeds: P seeds, NULL: p + 1) and the pool-ordered copy
 * of the points on the device; once per context, a later call replaces both.  The SPRT entry points
 * below call it with the default seeds if it was never called. */
int usac_multi_sprt_setup(usac_multi *mc, const uint32_t *pool_seeds);

/* usac_multi_hypothesize_score with SPRT verification in place of the scoring.  eps_delta (nullable):
 * n_problems x 2 doubles, (epsilon, delta) of problems[i]'s test; a 0 stands for the estimator's
 * default (H: 0.1, 0.01; F: 0.2, 0.05); A = estimateThresholdA(epsilon, delta).  counts / sums / best as
 * usac_multi_hypothesize_score's, over the verified slots; stats (nullable): n_problems entries;
 * starts (nullable): n_problems x R x S first pool positions, UINT32_MAX on an empty F slot.
 * USAC_ERR_ARG also for an epsilon or delta outside (0, 1) or delta >= epsilon -- before any device
 * call.  The certificate's margin and climb limit are usac_set_sprt's, its budget taken at each
 * problem's n_p, with the same USAC_SPRT_CERT_MARGIN / USAC_SPRT_CERT_CLIMB test overrides.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and thr is not read. */
int usac_multi_hypothesize_score_sprt(usac_multi *mc, const uint32_t *problems, uint32_t n_problems,
                                      const int32_t *samples, uint32_t R, const uint64_t *seeds, uint64_t first_hyp,
                                      float thr, int dlt_mode, const double *eps_delta, int32_t *counts, float *sums,
                                      usac_record *best, usac_multi_sprt_stats *stats, uint32_t *starts);

/* The per-round update of one problem's test, on the host (no context, no device) -- the function
 * usac_multi_run_sprt applies after every round.  State: hist[0 .. *n_hist) (capacity cap), *last_update,
 * *bound.  *n_hist == 0 initialises it as the reference's constructor does (sprt.hpp:114-170: the
 * estimator's epsilon_0, delta_0, A_0 = estimateThresholdA, k = 0; last_update 0; bound =
 * max_iterations) before anything else; done == 0 then returns.  Otherwise, after a round that ends at
 * `done` hypotheses, with (epsilon, delta) the current (last) test:
 *   1. head_points > 0: d = (float)head_inliers / (float)head_points; new_delta = d > 0 &&
 *      fabs(delta - d) / delta > 0.05 (sprt.hpp:298, over the round's head rejections);
 *   2. improved != 0 (the running record improved in the round): e = (double)((float)best_inliers /
 *      (float)n_points) (sprt.hpp:270);
 *   3. with e' / d' the new values where set, else the current ones: if either is set and 0 < d' < e' <
 *      1, the test {e', d', estimateThresholdA(e', d'), k = done - *last_update} is appended and
 *      *last_update = done.  The guard is a deviation from the reference, which would design a test with
 *      epsilon = 1 or delta >= epsilon;
 *   4. improved: *bound = min(term_bound, getUpperBoundIterations(best_inliers)) (sprt.hpp:371-393 over the
 *      history, ransac.cpp:126-132), term_bound being the caller's termination bound for that count.
 * Returns USAC_OK, or USAC_ERR_ARG for a NULL pointer, an estimator other than homography / fundamental,
 * n_points < m, *n_hist > cap, or a test to append with *n_hist == cap. */
int usac_multi_sprt_update(int estimator, uint32_t n_points, uint32_t m, uint32_t max_iterations,
                           usac_multi_sprt_test *hist, uint32_t *n_hist, uint32_t cap, uint32_t *last_update,
                           uint32_t *bound, uint32_t done, uint32_t head_inliers, uint32_t head_points, int improved,
                           uint32_t best_inliers, uint32_t term_bound);

/* usac_multi_run (params->sampler = USAC_SAMPLER_UNIFORM) or usac_multi_run_prosac (USAC_SAMPLER_PROSAC)
 * with SPRT verification: per round the active list and its tests go up, the round runs solve, SPRT
 * head + tail, argmax / merge and (PROSAC) the scan, the records and statistics come down in one copy,
 * and the host applies usac_multi_sprt_update to every active problem with term_bound =
 * usac_std_termination(best.inliers, ...) or the PROSAC scan's bound.  A problem is finished once
 * (r + 1) R >= min(max_iterations, bound_p).
 * Deviations from Ransac::run with SPRT: batch granularity (one test per problem and round, at most one
 * re-design per round); delta^ averaged over the round's head rejections; max_hypothesis_test_before_sprt
 * is not applied (a rejected model is never a best, as in usac_set_sprt's mode); the starts are per slot
 * tile instead of the rolling pool index; the guard of usac_multi_sprt_update; and those of usac_multi_run /
 * usac_multi_run_prosac.  No NAPSAC; LO with SPRT would mix sum scores with count scores and is left out.
 * USAC_ERR_ARG for params->sprt == 0, USAC_SAMPLER_NAPSAC, a bad batch or dlt_mode, NULL mc, params or
 * out, and with PROSAC any n_p <= 20; USAC_ERR_UNSUPPORTED for params->lo != USAC_LO_NONE -- all before
 * any device call.
 * out / pro / pol / mask as usac_multi_run_prosac's (pro is written only with PROSAC; the polish reads
 * only the record's model); sprt (nullable): P states.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and params->threshold is not read. */
int usac_multi_run_sprt(usac_multi *mc, const usac_params *params, const uint64_t *seeds, usac_multi_output *out,
                        usac_multi_sprt_output *sprt, usac_multi_prosac_output *pro, usac_multi_polish_output *pol,
                        uint8_t *mask);

/* ---- NAPSAC for multi-problem batches (ABI 20) ---------------------------------------- */
/* usac_grid_neighbors for every problem: the CSR of NearestNeighbors::getGridNearestNeighbors over each
 * problem's points for cell_size (> 0), built in one launch (one workgroup per problem; a problem of more
 * than 4000 points, or with a coordinate x for which !(|x| / cell_size < 1e9), is built on the host --
 * the same CSR) and kept in the context until another size is asked for.  Indices are local to each
 * problem and the arrays are problem-local at the points' offsets: cell, rank, members, eligible (points
 * with >= m neighbours, ascending; n_eligible[p] of them): N_total values each, problem p's at
 * offsets[p]; start: N_total + P values, problem p's n_cells[p] + 1 entries at offsets[p] + p.  Values
 * past a problem's n_eligible / n_cells + 1 entries are unspecified.  Every output is nullable. */
int usac_multi_grid(usac_multi *mc, int cell_size, uint32_t *n_cells, uint32_t *cell, uint32_t *rank,
                    uint32_t *start, int32_t *members, int32_t *eligible, uint32_t *n_eligible);

/* usac_multi_draw_samples with the NAPSAC device sampler over the grid of cell_size: for each listed
 * problem what a usac_ctx over its points draws after usac_set_cell_size(cell_size) and
 * usac_set_device_sampler(USAC_SAMPLER_NAPSAC) -- the initial point uniform over the eligible points,
 * m - 1 consecutive grid neighbours from a random phase; uniform samples for a problem without an
 * eligible point.  out: n_problems x R x m indices local to each problem. */
int usac_multi_draw_samples_napsac(usac_multi *mc, const uint32_t *problems, uint32_t n_problems, uint32_t R,
                                   const uint64_t *seeds, uint64_t first_hyp, int cell_size, int32_t *out);

/* usac_multi_hypothesize_score with that sampler (seeds required; no host samples).
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and thr is not read. */
int usac_multi_hypothesize_score_napsac(usac_multi *mc, const uint32_t *problems, uint32_t n_problems, uint32_t R,
                                        const uint64_t *seeds, uint64_t first_hyp, float thr, int dlt_mode,
                                        int cell_size, int32_t *counts, float *sums, usac_record *best);

/* usac_multi_run with the NAPSAC sampler (params->sampler = USAC_SAMPLER_NAPSAC, ->neighbors =
 * USAC_NEIGHBORS_GRID, ->cell_size > 0) and the standard termination criterion, optionally with LO
 * (params->lo = USAC_LO_INITLORSC / _INITFLORSC, as usac_multi_run_lo: the LO draws do not depend on the
 * main sampler) and the polish.  Deviations from the glibc-stream Ransac::run with NAPSAC: the device
 * stream's random phase in place of the reference's persistent per-point cursor (as the single context's
 * throughput sampler), batch-granular termination, and those of usac_multi_run / usac_multi_run_lo.
 * USAC_ERR_ARG for another sampler, cell_size <= 0, a bad batch or dlt_mode, the LO parameters
 * usac_multi_run_lo refuses, NULL mc, params or out; USAC_ERR_UNSUPPORTED for ->neighbors other than
 * USAC_NEIGHBORS_GRID (KNN NAPSAC is not built), params->sprt, USAC_LO_GC -- all before any device call
 * (the grid build included).  out / pol / mask as usac_multi_run_prosac's; lo (nullable): P LO states,
 * written only with LO.
 * While usac_multi_set_thresholds is in effect (ABI 22) problem p uses its own threshold and params->threshold is not read. */
int usac_multi_run_napsac(usac_multi *mc, const usac_params *params, const uint64_t *seeds, usac_multi_output *out,
                          usac_multi_lo_output *lo, usac_multi_polish_output *pol, uint8_t *mask);

/* ---- self-test hooks (ABI 13) ------------------------------------------------------- */
/* The essential 5-point solver's root step alone (five_points.cpp:139-157: rpoly_ak1's real zeros
 * in its order, usac_rpoly.hpp) on B host polynomials of 11 ascending coefficients each: roots
 * (B x 10 doubles, row h = polynomial h's real zeros in order) and their numbers.  Its correctly
 * rounded log / exp (rpoly.cpp:82,98) on n host arguments.  Device: the context's; no other state. */
int usac_selftest_rpoly(usac_ctx *ctx, const double *coeffs, uint32_t B, double *roots, int32_t *nroots);
int usac_selftest_logexp(usac_ctx *ctx, const double *x, uint32_t n, double *log_out, double *exp_out);

#ifdef __cplusplus
}
#endif
#endif
