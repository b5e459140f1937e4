"""ransac_amd -- MI355X-native USAC hypothesize-and-verify engine.

Python host mirror of the reference's plugin surface (MathsionYang/Ransac ``usac/``):
``Model`` (usac/model.hpp), ``Ransac`` + ``RansacOutput`` (usac/ransac/ransac.hpp,
ransac_output.hpp), ``Score`` (usac/quality/quality.hpp), and the operator level
``Context`` (Estimator::EstimateModel, Quality::getNumberInliers, ... batched).  All
compute goes through the C-ABI of ``libransac_amd.so`` (include/usac_gpu.h) into the HIP
kernels; there is no Python or CPU compute fallback -- if the library or a GPU is
missing, the calls raise.
"""
import ctypes
import enum
import os
import subprocess

import numpy as np

__all__ = ["ESTIMATOR", "SAMPLER", "LocOpt", "NeighborsSearch", "DLT", "Model", "Ransac", "RansacOutput", "Score", "Context", "Record",
           "RandomGenerator", "Sampler", "TerminationCriteria", "SPRT", "LocalOptimization", "SprtState", "MultiContext",
           "build", "lib", "std_termination", "uniform_samples", "prosac_samples", "sprt_pool", "lo_draw", "UsacError"]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RANSAC_AMD_LIB") or os.path.join(_HERE, "libransac_amd.so")  # override: A/B builds


class ESTIMATOR(enum.IntEnum):  # usac/model.hpp:10
    NullE = 0
    Line2d = 1
    Homography = 2
    Fundamental = 3
    Essential = 4


class SAMPLER(enum.IntEnum):  # usac/model.hpp:11
    NullS = 0
    Uniform = 1
    ProgressiveNAPSAC = 2
    Napsac = 3
    Prosac = 4
    Evsac = 5
    ProsacNapsac = 6


class LocOpt(enum.IntEnum):  # usac/model.hpp:13 (IRLS is out of scope: debug prints only)
    NullLO = 0
    InItLORsc = 1
    InItFLORsc = 2
    GC = 3


class NeighborsSearch(enum.IntEnum):  # usac/model.hpp:12 (NullN / Nanoflann = KNN on the device)
    NullN = 0
    Nanoflann = 1
    Grid = 2


class DLT(enum.IntEnum):
    THIN = 0        # reference semantics: vt.row(7) of the thin 8x9 SVD (dlt.cpp:43-48)
    NULLSPACE = 1   # true null vector


class UsacError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("usac error %d: %s" % (code, msg))
        self.code = code


class Record(ctypes.Structure):
    _fields_ = [("hyp_index", ctypes.c_uint64), ("inliers", ctypes.c_int32), ("score", ctypes.c_float),
                ("model", ctypes.c_float * 9), ("valid", ctypes.c_int32)]

    def as_dict(self):
        return {"hyp_index": int(self.hyp_index), "inliers": int(self.inliers), "score": float(self.score),
                "model": np.array(self.model[:], dtype=np.float32), "valid": bool(self.valid)}


class _Params(ctypes.Structure):
    _fields_ = [("threshold", ctypes.c_float), ("desired_prob", ctypes.c_float), ("max_iterations", ctypes.c_uint32),
                ("seed", ctypes.c_uint32), ("dlt_mode", ctypes.c_int32), ("batch", ctypes.c_uint32),
                ("sampler", ctypes.c_int32), ("sprt", ctypes.c_int32), ("lo", ctypes.c_int32),
                ("lo_sample_size", ctypes.c_uint32), ("lo_iterative_iterations", ctypes.c_uint32),
                ("lo_inner_iterations", ctypes.c_uint32), ("lo_threshold_multiplier", ctypes.c_uint32),
                ("cell_size", ctypes.c_int32), ("neighbors", ctypes.c_int32), ("knn", ctypes.c_uint32),
                ("spatial_coherence_gc", ctypes.c_float), ("max_hypothesis_test_before_sprt", ctypes.c_uint32)]


class SprtState(ctypes.Structure):
    """usac_sprt_state (include/usac_gpu.h): the loop state in / out of usac_sprt_replay."""
    _fields_ = [("iters", ctypes.c_uint32), ("max_iters", ctypes.c_uint32), ("best_inliers", ctypes.c_int32),
                ("best_score", ctypes.c_float), ("sample", ctypes.c_uint32), ("slot", ctypes.c_uint32),
                ("found", ctypes.c_int32), ("inliers", ctypes.c_int32), ("score", ctypes.c_float),
                ("found_sample", ctypes.c_uint32), ("found_slot", ctypes.c_uint32), ("rejected", ctypes.c_uint32)]


class _RunOutput(ctypes.Structure):
    _fields_ = [("model", ctypes.c_float * 9), ("inliers", ctypes.c_int32), ("iters", ctypes.c_uint32),
                ("time_us", ctypes.c_int64), ("n_records", ctypes.c_int32), ("polish_passes", ctypes.c_int32),
                ("minimal_model", ctypes.c_float * 9), ("minimal_inliers", ctypes.c_int32),
                ("batches", ctypes.c_uint32), ("sprt_rejected", ctypes.c_int32), ("sprt_histories", ctypes.c_int32),
                ("prosac_term_len", ctypes.c_uint32), ("rollbacks", ctypes.c_uint32),
                ("lo_inner_iters", ctypes.c_uint32), ("lo_iterative_iters", ctypes.c_uint32),
                ("lo_rounds", ctypes.c_uint32), ("lo_stages", ctypes.c_uint32), ("sum_models", ctypes.c_uint32),
                ("lo_fits", ctypes.c_uint32), ("spec_batches", ctypes.c_uint32), ("spec_rollbacks", ctypes.c_uint32),
                ("spec_wasted", ctypes.c_uint32)]


class _MultiOutput(ctypes.Structure):
    """usac_multi_output (include/usac_gpu.h): one problem's result of usac_multi_run."""
    _fields_ = [("best", Record), ("hypotheses", ctypes.c_uint32), ("rounds", ctypes.c_uint32),
                ("bound", ctypes.c_uint32), ("status", ctypes.c_int32)]


class _MultiPolishOutput(ctypes.Structure):
    """usac_multi_polish_output (include/usac_gpu.h): one problem's result of usac_multi_polish."""
    _fields_ = [("model", ctypes.c_float * 9), ("inliers", ctypes.c_int32), ("score", ctypes.c_float),
                ("minimal_inliers", ctypes.c_int32), ("minimal_score", ctypes.c_float), ("passes", ctypes.c_int32),
                ("status", ctypes.c_int32)]

    DTYPE = np.dtype([("model", np.float32, (9,)), ("inliers", np.int32), ("score", np.float32),
                      ("minimal_inliers", np.int32), ("minimal_score", np.float32), ("passes", np.int32),
                      ("status", np.int32)])

    @classmethod
    def as_dicts(cls, arr):
        """a ctypes array of results -> a list of dicts (model: float32[9], score / minimal_score:
        np.float32, the rest ints), through one numpy view instead of a field read per value"""
        a = np.frombuffer(arr, dtype=cls.DTYPE).copy()
        models, score, mscore = np.ascontiguousarray(a["model"]), a["score"], a["minimal_score"]
        cols = [a[k].tolist() for k in ("inliers", "minimal_inliers", "passes", "status")]
        return [{"model": models[p], "inliers": cols[0][p], "score": score[p], "minimal_inliers": cols[1][p],
                 "minimal_score": mscore[p], "passes": cols[2][p], "status": cols[3][p]}
                for p in range(len(a))]


class _MultiProsacOutput(ctypes.Structure):
    """usac_multi_prosac_output (include/usac_gpu.h): one problem's PROSAC state after usac_multi_run_prosac."""
    _fields_ = [("termination_length", ctypes.c_uint32), ("largest_sample_size", ctypes.c_uint32),
                ("clock", ctypes.c_uint32), ("scans", ctypes.c_uint32)]


class _MultiLoOutput(ctypes.Structure):
    """usac_multi_lo_output (include/usac_gpu.h): one problem's LO counters and threshold."""
    _fields_ = [("lo_calls", ctypes.c_uint32), ("inner_iters", ctypes.c_uint32), ("iterative_iters", ctypes.c_uint32),
                ("fits", ctypes.c_uint32), ("improved", ctypes.c_uint32), ("capped", ctypes.c_uint32),
                ("draws", ctypes.c_uint32), ("threshold", ctypes.c_float)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_[:-1]}
        d["threshold"] = np.float32(self.threshold)
        return d


class _MultiSprtStats(ctypes.Structure):
    """usac_multi_sprt_stats (include/usac_gpu.h): one problem's SPRT statistics of a round."""
    _fields_ = [("accepted", ctypes.c_uint32), ("rejected_head", ctypes.c_uint32), ("rejected_tail", ctypes.c_uint32),
                ("head_inliers", ctypes.c_uint32), ("head_points", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("points_tested", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class _MultiSprtTest(ctypes.Structure):
    """usac_multi_sprt_test (include/usac_gpu.h): one entry of a problem's SPRT test history."""
    _fields_ = [("epsilon", ctypes.c_double), ("delta", ctypes.c_double), ("A", ctypes.c_double),
                ("k", ctypes.c_int32), ("pad", ctypes.c_int32)]


class _MultiSprtOutput(ctypes.Structure):
    """usac_multi_sprt_output (include/usac_gpu.h): one problem's SPRT state after usac_multi_run_sprt."""
    _fields_ = [("epsilon", ctypes.c_double), ("delta", ctypes.c_double), ("A", ctypes.c_double),
                ("tests", ctypes.c_uint32), ("accepted", ctypes.c_uint32), ("rejected", ctypes.c_uint32),
                ("pad", ctypes.c_uint32), ("points_tested", ctypes.c_uint64)]

    def as_dict(self):
        return {"epsilon": float(self.epsilon), "delta": float(self.delta), "A": float(self.A), "tests": int(self.tests),
                "accepted": int(self.accepted), "rejected": int(self.rejected), "points_tested": int(self.points_tested)}


class _MultiDeviceInput(ctypes.Structure):
    """usac_multi_device_input (ABI 25): the device pointers as integers, K1 / K2 on the host"""
    _fields_ = [("P", ctypes.c_uint32), ("n_max", ctypes.c_uint32), ("rows", ctypes.c_void_p),
                ("valid", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("kpts0", ctypes.c_void_p),
                ("kpts1", ctypes.c_void_p), ("n1", ctypes.c_uint32), ("match", ctypes.c_void_p),
                ("K1", ctypes.POINTER(ctypes.c_float)), ("K2", ctypes.POINTER(ctypes.c_float)),
                ("stream", ctypes.c_void_p)]


class _MultiDeviceOrder(ctypes.Structure):
    """usac_multi_device_order (ABI 26): the scores' device pointer as an integer, and the direction"""
    _fields_ = [("scores", ctypes.c_void_p), ("descending", ctypes.c_int)]


class _MultiDeviceOutput(ctypes.Structure):
    """usac_multi_device_output (ABI 27): the widths, the output device pointers as integers, the stream"""
    _fields_ = [("n_max", ctypes.c_uint32), ("k_max", ctypes.c_uint32), ("models", ctypes.c_void_p),
                ("pixel_models", ctypes.c_void_p), ("inliers", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("inlier_cols", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


class _MultiPoseOutput(ctypes.Structure):
    """usac_multi_pose_output (ABI 28): the mask's width, the output device pointers as integers, the stream"""
    _fields_ = [("n_max", ctypes.c_uint32), ("R", ctypes.c_void_p), ("t", ctypes.c_void_p),
                ("front", ctypes.c_void_p), ("choice", ctypes.c_void_p), ("front_mask", ctypes.c_void_p),
                ("stream", ctypes.c_void_p)]


class _MultiRefineIO(ctypes.Structure):
    """usac_multi_refine_io (ABI 29): the mask's width, the step limit, the input and output device pointers as
    integers, the stream"""
    _fields_ = [("n_max", ctypes.c_uint32), ("max_iters", ctypes.c_uint32), ("R_in", ctypes.c_void_p),
                ("t_in", ctypes.c_void_p), ("mask_in", ctypes.c_void_p), ("R", ctypes.c_void_p), ("t", ctypes.c_void_p),
                ("E", ctypes.c_void_p), ("cost0", ctypes.c_void_p), ("cost", ctypes.c_void_p),
                ("iterations", ctypes.c_void_p), ("used", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


# every symbol include/usac_gpu.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "usac_create", "usac_destroy", "usac_last_error", "usac_abi_version", "usac_set_dlt_mode", "usac_sample_size",
    "usac_num_points", "usac_estimate_models", "usac_score_models", "usac_get_inliers", "usac_knn", "usac_bk_label",
    "usac_nonminimal", "usac_lsq_fit",
    "usac_hypothesize_score", "usac_hypothesize_async", "usac_fetch_best", "usac_sync", "usac_last_timings",
    "usac_set_score_chunks", "usac_set_score_variant", "usac_last_counts", "usac_std_termination", "usac_ransac_run", "usac_ransac_run_sharded", "usac_uniform_samples",
    "usac_prosac_samples", "usac_sprt_pool", "usac_set_sprt", "usac_sprt_tested", "usac_set_device_sampler",
    "usac_draw_samples", "usac_set_cell_size", "usac_grid_neighbors",
    "usac_comm_unique_id", "usac_comm_init", "usac_comm_count", "usac_allgather_records", "usac_merge_records",
    "usac_exchange_best_async", "usac_exchange_best_wait",
    "usac_random_create", "usac_random_next", "usac_random_destroy", "usac_sampler_create", "usac_sampler_generate",
    "usac_sampler_generate_batch", "usac_sampler_state", "usac_sampler_destroy", "usac_termination_create",
    "usac_termination_bound", "usac_prosac_termination", "usac_termination_destroy", "usac_sprt_create",
    "usac_sprt_verify", "usac_sprt_upper_bound", "usac_sprt_stats", "usac_sprt_replay", "usac_sprt_destroy",
    "usac_lo_create", "usac_lo_get_model_score", "usac_lo_iters", "usac_lo_destroy", "usac_batch_sprt_info",
    "usac_selftest_rpoly", "usac_selftest_logexp", "usac_set_timing",
    "usac_multi_create", "usac_multi_destroy", "usac_multi_last_error", "usac_multi_num_problems",
    "usac_multi_hypothesize_score", "usac_multi_run", "usac_multi_inliers", "usac_multi_polish",
    "usac_multi_run_polished",
    "usac_prosac_schedule", "usac_multi_draw_samples", "usac_multi_run_prosac", "usac_multi_prosac_scan",
    "usac_lo_draw", "usac_multi_lo", "usac_multi_run_lo",
    "usac_multi_sprt_setup", "usac_multi_hypothesize_score_sprt", "usac_multi_sprt_update", "usac_multi_run_sprt",
    "usac_multi_grid", "usac_multi_draw_samples_napsac", "usac_multi_hypothesize_score_napsac", "usac_multi_run_napsac",
    "usac_multi_create_essential",
    "usac_multi_set_thresholds", "usac_multi_get_thresholds",
    "usac_multi_lo_essential", "usac_multi_run_lo_essential",
    "usac_multi_create_essential_pixels", "usac_multi_set_pixel_thresholds", "usac_multi_pixel_models",
    "usac_multi_get_points",
    "usac_multi_create_device", "usac_multi_get_offsets", "usac_multi_get_source", "usac_multi_padded_mask",
    "usac_multi_create_device_sorted",
    "usac_multi_set_resident", "usac_multi_export_device",
    "usac_multi_pose_device", "usac_multi_pose",
    "usac_multi_refine_pose_device", "usac_multi_refine_pose",
]


def build(jobs=8):
    """Compile libransac_amd.so for gfx950 in-tree (hipcc via ransac_amd/Makefile)."""
    subprocess.run(["make", "-s", "-C", _HERE, "-j%d" % jobs], check=True)


_lib = None
_P = ctypes.POINTER
_vp = ctypes.c_void_p


def lib():
    """Load libransac_amd.so (raises if it is missing: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("ransac_amd: %s is missing -- run ransac_amd.build() (hipcc, gfx950)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    f32p, i32p, u32p, u8p = _P(ctypes.c_float), _P(ctypes.c_int32), _P(ctypes.c_uint32), _P(ctypes.c_uint8)
    f64p = _P(ctypes.c_double)
    sig = {
        "usac_create": (ctypes.c_int, [_P(_vp), ctypes.c_int, ctypes.c_int, f32p, ctypes.c_uint32, ctypes.c_uint32]),
        "usac_destroy": (None, [_vp]),
        "usac_last_error": (ctypes.c_char_p, [_vp]),
        "usac_abi_version": (ctypes.c_int, []),
        "usac_set_dlt_mode": (ctypes.c_int, [_vp, ctypes.c_int]),
        "usac_set_score_chunks": (ctypes.c_int, [_vp, ctypes.c_int]),
        "usac_set_score_variant": (ctypes.c_int, [_vp, ctypes.c_int]),
        "usac_last_counts": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float),
                                            ctypes.c_uint32]),
        "usac_sample_size": (ctypes.c_uint32, [_vp]),
        "usac_num_points": (ctypes.c_uint32, [_vp]),
        "usac_estimate_models": (ctypes.c_int, [_vp, i32p, ctypes.c_uint32, f32p, i32p]),
        "usac_score_models": (ctypes.c_int, [_vp, f32p, ctypes.c_uint32, ctypes.c_float, i32p, f32p]),
        "usac_get_inliers": (ctypes.c_int, [_vp, f32p, ctypes.c_float, i32p, u32p, f32p]),
        "usac_knn": (ctypes.c_int, [_vp, ctypes.c_uint32, i32p, f32p]),
        "usac_bk_label": (ctypes.c_float, [ctypes.c_int, f32p, ctypes.c_int, i32p, i32p, f32p, f32p, f32p, f32p, i32p]),
        "usac_nonminimal": (ctypes.c_int, [_vp, i32p, ctypes.c_uint32, f32p]),
        "usac_lsq_fit": (ctypes.c_int, [_vp, i32p, ctypes.c_uint32, f32p, f32p]),
        "usac_hypothesize_score": (ctypes.c_int, [_vp, i32p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_float, i32p, f32p, _P(Record)]),
        "usac_hypothesize_async": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_float]),
        "usac_fetch_best": (ctypes.c_int, [_vp, _P(Record)]),
        "usac_sync": (ctypes.c_int, [_vp]),
        "usac_last_timings": (ctypes.c_int, [_vp, f32p]),
        "usac_set_timing": (ctypes.c_int, [_vp, ctypes.c_int]),
        "usac_std_termination": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_float, ctypes.c_uint32]),
        "usac_ransac_run": (ctypes.c_int, [_vp, _P(_Params), _P(_RunOutput), i32p, _P(Record), ctypes.c_uint32]),
        "usac_ransac_run_sharded": (ctypes.c_int, [_vp, _P(_Params), ctypes.c_int, ctypes.c_int, _vp, _vp,
                                                   _P(_RunOutput), i32p, _P(Record), ctypes.c_uint32]),
        "usac_uniform_samples": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                i32p]),
        "usac_prosac_samples": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, i32p]),
        "usac_sprt_pool": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, u32p,
                                          _P(ctypes.c_double)]),
        "usac_set_sprt": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_uint32, ctypes.c_double, ctypes.c_double]),
        "usac_set_device_sampler": (ctypes.c_int, [_vp, ctypes.c_int]),
        "usac_draw_samples": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, _vp]),
        "usac_set_cell_size": (ctypes.c_int, [_vp, ctypes.c_int]),
        "usac_grid_neighbors": (ctypes.c_int, [_vp, ctypes.c_int, u32p, u32p, u32p, u32p, i32p, i32p, u32p]),
        "usac_sprt_tested": (ctypes.c_int, [_vp, _P(ctypes.c_uint64)]),
        "usac_batch_sprt_info": (ctypes.c_int, [_vp, _P(ctypes.c_double), u32p, ctypes.c_uint32]),
        "usac_comm_unique_id": (ctypes.c_int, [u8p]),
        "usac_comm_init": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, u8p]),
        "usac_comm_count": (ctypes.c_int, [_vp, i32p, i32p, i32p]),
        "usac_allgather_records": (ctypes.c_int, [_vp, _P(Record), _P(Record)]),
        "usac_exchange_best_async": (ctypes.c_int, [_vp, _vp, ctypes.c_uint32]),
        "usac_exchange_best_wait": (ctypes.c_int, [_vp, ctypes.c_uint32, _P(Record)]),
        "usac_merge_records": (ctypes.c_int, [_P(Record), ctypes.c_uint32, _P(Record)]),
        "usac_random_create": (ctypes.c_int, [ctypes.c_uint32, _P(_vp)]),
        "usac_random_next": (ctypes.c_uint32, [_vp]),
        "usac_random_destroy": (None, [_vp]),
        "usac_sampler_create": (ctypes.c_int, [_vp, _P(_Params), _vp, _P(_vp)]),
        "usac_sampler_generate": (ctypes.c_int, [_vp, i32p]),
        "usac_sampler_generate_batch": (ctypes.c_int, [_vp, ctypes.c_uint32, i32p]),
        "usac_sampler_state": (ctypes.c_int, [_vp, _P(ctypes.c_uint64), u32p, u32p]),
        "usac_sampler_destroy": (None, [_vp]),
        "usac_termination_create": (ctypes.c_int, [_vp, _P(_Params), _vp, _P(_vp)]),
        "usac_termination_bound": (ctypes.c_uint32, [_vp, ctypes.c_uint32, ctypes.c_uint32]),
        "usac_prosac_termination": (ctypes.c_int, [_vp, ctypes.c_uint32, f32p, u32p, u32p]),
        "usac_termination_destroy": (None, [_vp]),
        "usac_sprt_create": (ctypes.c_int, [_vp, _P(_Params), _vp, _P(_vp)]),
        "usac_sprt_verify": (ctypes.c_int, [_vp, f32p, ctypes.c_int32, ctypes.c_uint32, i32p, i32p, f32p]),
        "usac_sprt_upper_bound": (ctypes.c_uint32, [_vp, ctypes.c_uint32]),
        "usac_sprt_stats": (ctypes.c_int, [_vp, u32p, u32p]),
        "usac_sprt_replay": (ctypes.c_int, [_vp, f32p, i32p, ctypes.c_uint32, _P(SprtState)]),
        "usac_sprt_destroy": (None, [_vp]),
        "usac_lo_create": (ctypes.c_int, [_vp, _P(_Params), _P(_vp)]),
        "usac_lo_get_model_score": (ctypes.c_int, [_vp, f32p, i32p, f32p]),
        "usac_lo_iters": (ctypes.c_int, [_vp, u32p, u32p]),
        "usac_lo_destroy": (None, [_vp]),
        "usac_multi_create": (ctypes.c_int, [_P(_vp), ctypes.c_int, ctypes.c_int, f32p, u32p, ctypes.c_uint32]),
        "usac_multi_create_essential": (ctypes.c_int, [_P(_vp), ctypes.c_int, f32p, u32p, ctypes.c_uint32]),
        "usac_multi_create_essential_pixels": (ctypes.c_int, [_P(_vp), ctypes.c_int, f32p, u32p, ctypes.c_uint32, f32p,
                                                              f32p]),
        "usac_multi_set_pixel_thresholds": (ctypes.c_int, [_vp, f32p, ctypes.c_uint32]),
        "usac_multi_pixel_models": (ctypes.c_int, [_vp, f32p, f32p]),
        "usac_multi_get_points": (ctypes.c_int, [_vp, f32p]),
        "usac_multi_create_device": (ctypes.c_int, [_P(_vp), ctypes.c_int, ctypes.c_int, _P(_MultiDeviceInput)]),
        "usac_multi_create_device_sorted": (ctypes.c_int, [_P(_vp), ctypes.c_int, ctypes.c_int, _P(_MultiDeviceInput),
                                                           _P(_MultiDeviceOrder)]),
        "usac_multi_get_offsets": (ctypes.c_int, [_vp, u32p]),
        "usac_multi_get_source": (ctypes.c_int, [_vp, u32p]),
        "usac_multi_padded_mask": (ctypes.c_int, [_vp, u8p, _vp, _vp]),
        "usac_multi_set_resident": (ctypes.c_int, [_vp, ctypes.c_int]),
        "usac_multi_export_device": (ctypes.c_int, [_vp, _P(_MultiDeviceOutput)]),
        "usac_multi_pose_device": (ctypes.c_int, [_vp, _P(_MultiPoseOutput)]),
        "usac_multi_pose": (ctypes.c_int, [_vp, f32p, u8p, f32p, f32p, i32p, i32p, u8p]),
        "usac_multi_refine_pose_device": (ctypes.c_int, [_vp, _P(_MultiRefineIO)]),
        "usac_multi_refine_pose": (ctypes.c_int, [_vp, f32p, f32p, u8p, ctypes.c_uint32, f32p, f32p, f32p, f64p, f64p,
                                                  i32p, i32p]),
        "usac_multi_destroy": (None, [_vp]),
        "usac_multi_last_error": (ctypes.c_char_p, [_vp]),
        "usac_multi_num_problems": (ctypes.c_uint32, [_vp]),
        "usac_multi_set_thresholds": (ctypes.c_int, [_vp, f32p]),
        "usac_multi_get_thresholds": (ctypes.c_int, [_vp, f32p]),
        "usac_multi_hypothesize_score": (ctypes.c_int, [_vp, u32p, ctypes.c_uint32, i32p, ctypes.c_uint32,
                                                        _P(ctypes.c_uint64), ctypes.c_uint64, ctypes.c_float,
                                                        ctypes.c_int, i32p, f32p, _P(Record)]),
        "usac_multi_run": (ctypes.c_int, [_vp, _P(_Params), _P(ctypes.c_uint64), _P(_MultiOutput)]),
        "usac_multi_inliers": (ctypes.c_int, [_vp, f32p, ctypes.c_float, u8p, i32p]),
        "usac_multi_polish": (ctypes.c_int, [_vp, f32p, ctypes.c_float, _P(_MultiPolishOutput), u8p]),
        "usac_multi_run_polished": (ctypes.c_int, [_vp, _P(_Params), _P(ctypes.c_uint64), _P(_MultiOutput),
                                                   _P(_MultiPolishOutput), u8p]),
        "usac_prosac_schedule": (ctypes.c_int, [ctypes.c_uint32] * 5 + [u32p, u32p, u32p]),
        "usac_multi_draw_samples": (ctypes.c_int, [_vp, u32p, ctypes.c_uint32, ctypes.c_uint32, _P(ctypes.c_uint64),
                                                   ctypes.c_uint64, u32p, u32p, i32p]),
        "usac_multi_run_prosac": (ctypes.c_int, [_vp, _P(_Params), _P(ctypes.c_uint64), _P(_MultiOutput),
                                                 _P(_MultiProsacOutput), _P(_MultiPolishOutput), u8p]),
        "usac_multi_prosac_scan": (ctypes.c_int, [_vp, _P(_Params), ctypes.c_int, f32p, u32p, u32p, u32p, u32p, u32p,
                                                  u32p]),
        "usac_lo_draw": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, i32p]),
        "usac_multi_lo": (ctypes.c_int, [_vp, _P(_Params), ctypes.c_int, _P(ctypes.c_uint64), _P(Record),
                                         _P(_MultiLoOutput)]),
        "usac_multi_run_lo": (ctypes.c_int, [_vp, _P(_Params), _P(ctypes.c_uint64), _P(_MultiOutput),
                                             _P(_MultiLoOutput), _P(_MultiProsacOutput), _P(_MultiPolishOutput), u8p]),
        "usac_multi_lo_essential": (ctypes.c_int, [_vp, _P(_Params), ctypes.c_int, _P(ctypes.c_uint64), _P(Record),
                                                   _P(_MultiLoOutput)]),
        "usac_multi_run_lo_essential": (ctypes.c_int, [_vp, _P(_Params), _P(ctypes.c_uint64), _P(_MultiOutput),
                                                       _P(_MultiLoOutput), _P(_MultiProsacOutput),
                                                       _P(_MultiPolishOutput), u8p]),
        "usac_multi_sprt_setup": (ctypes.c_int, [_vp, u32p]),
        "usac_multi_hypothesize_score_sprt": (ctypes.c_int, [_vp, u32p, ctypes.c_uint32, i32p, ctypes.c_uint32,
                                                             _P(ctypes.c_uint64), ctypes.c_uint64, ctypes.c_float,
                                                             ctypes.c_int, _P(ctypes.c_double), i32p, f32p, _P(Record),
                                                             _P(_MultiSprtStats), u32p]),
        "usac_multi_sprt_update": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_uint32] * 3 + [_P(_MultiSprtTest), u32p,
                                                  ctypes.c_uint32, u32p, u32p] + [ctypes.c_uint32] * 3 +
                                   [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]),
        "usac_multi_run_sprt": (ctypes.c_int, [_vp, _P(_Params), _P(ctypes.c_uint64), _P(_MultiOutput),
                                               _P(_MultiSprtOutput), _P(_MultiProsacOutput), _P(_MultiPolishOutput), u8p]),
        "usac_multi_grid": (ctypes.c_int, [_vp, ctypes.c_int, u32p, u32p, u32p, u32p, i32p, i32p, u32p]),
        "usac_multi_draw_samples_napsac": (ctypes.c_int, [_vp, u32p, ctypes.c_uint32, ctypes.c_uint32,
                                                          _P(ctypes.c_uint64), ctypes.c_uint64, ctypes.c_int, i32p]),
        "usac_multi_hypothesize_score_napsac": (ctypes.c_int, [_vp, u32p, ctypes.c_uint32, ctypes.c_uint32,
                                                               _P(ctypes.c_uint64), ctypes.c_uint64, ctypes.c_float,
                                                               ctypes.c_int, ctypes.c_int, i32p, f32p, _P(Record)]),
        "usac_multi_run_napsac": (ctypes.c_int, [_vp, _P(_Params), _P(ctypes.c_uint64), _P(_MultiOutput),
                                                 _P(_MultiLoOutput), _P(_MultiPolishOutput), u8p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _ptr(a, t):
    return a.ctypes.data_as(_P(t)) if a is not None else None


class _DevArray:
    """A device array as the library takes it: the pointer, the shape, a dtype code (f4, i4, i8, u1, b1) and
    the object that owns the memory.  A torch tensor (data_ptr()) or anything with __cuda_array_interface__;
    TypeError for host memory, ValueError for a layout that is not C-contiguous."""

    _TORCH = {"torch.float32": "f4", "torch.float64": "f8", "torch.int32": "i4", "torch.int64": "i8", "torch.uint8": "u1",
              "torch.bool": "b1"}

    def __init__(self, obj, name):
        self.obj, self.name = obj, name
        self.torch = False
        self.device = None
        if isinstance(obj, np.ndarray) or isinstance(obj, (list, tuple)):
            raise TypeError("%s: a device array is needed, got host memory (%s)" % (name, type(obj).__name__))
        if hasattr(obj, "data_ptr") and hasattr(obj, "is_contiguous"):
            if not getattr(obj, "is_cuda", False):
                raise TypeError("%s: a device tensor is needed, got one on %s" % (name, getattr(obj, "device", "the host")))
            self.torch = True
            self.device = obj.device.index
            self.shape = tuple(int(d) for d in obj.shape)
            self.kind = self._TORCH.get(str(obj.dtype), str(obj.dtype))
            if not obj.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
            self.ptr = int(obj.data_ptr())
        elif hasattr(obj, "__cuda_array_interface__"):
            d = obj.__cuda_array_interface__
            self.shape = tuple(int(v) for v in d["shape"])
            self.kind = d["typestr"][1:]
            if d.get("strides") is not None:
                want, step = [], int(self.kind[1:])
                for n in reversed(self.shape):
                    want.insert(0, step)
                    step *= n
                if tuple(d["strides"]) != tuple(want):
                    raise ValueError("%s must be contiguous" % name)
            self.ptr = int(d["data"][0])
        else:
            raise TypeError("%s: a device array is needed (data_ptr() or __cuda_array_interface__), got %s"
                            % (name, type(obj).__name__))

    def need(self, shape, kinds):
        """ValueError unless the shape (None: any extent) and one of the dtype codes fit"""
        ok = len(self.shape) == len(shape) and all(w is None or w == h for w, h in zip(shape, self.shape))
        if not ok:
            raise ValueError("%s must be %s, got %s" % (self.name, " x ".join("*" if w is None else str(w) for w in shape),
                                                        " x ".join(map(str, self.shape))))
        if self.kind not in kinds:
            raise ValueError("%s must be of dtype %s, got %s" % (self.name, " or ".join(kinds), self.kind))
        return self


def bk_label(unary, ei, ej, e00, e01, e10, e11):
    """The graph-cut LO's host min cut (usac_bk_label): add_term1(i, unary[i], 0), add_term2 per
    pair, BK max-flow -> (sink mask, flow).  No device work."""
    a = [np.ascontiguousarray(unary, np.float32), np.ascontiguousarray(ei, np.int32), np.ascontiguousarray(ej, np.int32)]
    a += [np.ascontiguousarray(x, np.float32) for x in (e00, e01, e10, e11)]
    out = np.zeros(len(a[0]), np.int32)
    f = lib().usac_bk_label(len(a[0]), _ptr(a[0], ctypes.c_float), len(a[1]), _ptr(a[1], ctypes.c_int32),
                            _ptr(a[2], ctypes.c_int32), _ptr(a[3], ctypes.c_float), _ptr(a[4], ctypes.c_float),
                            _ptr(a[5], ctypes.c_float), _ptr(a[6], ctypes.c_float), _ptr(out, ctypes.c_int32))
    return out.astype(bool), f


def std_termination(inliers, points_size, sample_size, desired_prob, max_iterations=10000):
    """StandardTerminationCriteria::getUpBoundIterations (standard_termination_criteria.hpp:52-62)."""
    return int(lib().usac_std_termination(inliers, points_size, sample_size, ctypes.c_float(desired_prob),
                                          max_iterations))


def prosac_samples(seed, n_points, m, count, termination_length=None):
    """Host ProsacSampler stream (mt19937 seeded with `seed`), count x m int32."""
    out = np.zeros((count, m), dtype=np.int32)
    tl = n_points if termination_length is None else termination_length
    rc = lib().usac_prosac_samples(seed, n_points, m, count, tl, _ptr(out, ctypes.c_int32))
    if rc:
        raise UsacError(rc, "usac_prosac_samples")
    return out


UNIFORM_OVER_N = 0xFFFFFFFF  # prosac_schedule: a lane past T_N = 200000


def prosac_schedule(n, m, clock, term_len, R, largest=None):
    """usac_prosac_schedule: one round of the multi-problem PROSAC sampler for one problem, on the host.
    Returns (subset uint32[R], clock_next, largest): subset[j] = s(t) of a PROSAC lane, 0 for a lane
    drawn uniformly from [0, term_len], UNIFORM_OVER_N for one drawn uniformly from all n points;
    largest = the sampler's largest_sample_size after the round (in: its value before, default m)."""
    sub = np.zeros(R, dtype=np.uint32)
    nxt = ctypes.c_uint32(0)
    lg = ctypes.c_uint32(m if largest is None else largest)
    rc = lib().usac_prosac_schedule(n, m, clock, term_len, R, _ptr(sub, ctypes.c_uint32), ctypes.byref(nxt),
                                    ctypes.byref(lg))
    if rc:
        raise UsacError(rc, "usac_prosac_schedule")
    return sub, int(nxt.value), int(lg.value)


def lo_draw(seed, draw, k, max):
    """usac_lo_draw: the draw-th sample set of the multi-problem LO under `seed` -- k distinct integers of
    the closed range [0, max], in draw order (int32[k]).  On the host; the device draws through the same text."""
    out = np.zeros(int(k) if 0 < int(k) <= 64 else 1, dtype=np.int32)  # (a bad k: the C call refuses it)
    rc = lib().usac_lo_draw(int(seed), int(draw), int(k), int(max), _ptr(out, ctypes.c_int32))
    if rc:
        raise UsacError(rc, "usac_lo_draw")
    return out


class MultiSprtState:
    """One problem's SPRT state of a multi-problem run, advanced by usac_multi_sprt_update -- the host
    function usac_multi_run_sprt applies after every round (no context, no device).  history: a list of
    (epsilon, delta, A, k); last_update; bound (max_iterations until a round improves the record)."""

    def __init__(self, estimator, n_points, m, max_iterations, cap=256):
        self.estimator, self.n, self.m, self.max_iterations = int(estimator), int(n_points), int(m), int(max_iterations)
        self._hist = (_MultiSprtTest * cap)()
        self._n = ctypes.c_uint32(0)
        self._last = ctypes.c_uint32(0)
        self._bound = ctypes.c_uint32(0)
        self._call(0, 0, 0, False, 0, 0)

    def _call(self, done, head_inliers, head_points, improved, best_inliers, term_bound):
        rc = lib().usac_multi_sprt_update(self.estimator, self.n, self.m, self.max_iterations, self._hist,
                                          ctypes.byref(self._n), len(self._hist), ctypes.byref(self._last),
                                          ctypes.byref(self._bound), int(done), int(head_inliers), int(head_points),
                                          1 if improved else 0, int(best_inliers), int(term_bound))
        if rc:
            raise UsacError(rc, "usac_multi_sprt_update")

    def update(self, done, head_inliers, head_points, improved, best_inliers=0, term_bound=0):
        """the update after a round that ends at `done` hypotheses; True when a new test was designed"""
        before = self._n.value
        self._call(done, head_inliers, head_points, improved, best_inliers, term_bound)
        return self._n.value > before

    @property
    def history(self):
        return [(h.epsilon, h.delta, h.A, int(h.k)) for h in self._hist[:self._n.value]]

    @property
    def test(self):
        h = self._hist[self._n.value - 1]
        return h.epsilon, h.delta, h.A

    @property
    def last_update(self):
        return int(self._last.value)

    @property
    def bound(self):
        return int(self._bound.value)


def multi_sprt_update(state, done, head_inliers, head_points, improved, best_inliers=0, term_bound=0):
    """usac_multi_sprt_update on a MultiSprtState (see MultiSprtState.update)."""
    return state.update(done, head_inliers, head_points, improved, best_inliers, term_bound)


def sprt_pool(seed, estimator, n_points, m):
    """SPRT random pool after srandom(seed) and the first threshold A."""
    pool = np.zeros(n_points, dtype=np.uint32)
    A = ctypes.c_double(0)
    rc = lib().usac_sprt_pool(seed, int(estimator), n_points, m, _ptr(pool, ctypes.c_uint32), ctypes.byref(A))
    if rc:
        raise UsacError(rc, "usac_sprt_pool")
    return pool, A.value


def uniform_samples(seed, n_points, m, count):
    """UniformSampler stream after srandom(seed) (uniform_sampler.hpp:42-54): count x m int32."""
    out = np.zeros((count, m), dtype=np.int32)
    rc = lib().usac_uniform_samples(seed, n_points, m, count, _ptr(out, ctypes.c_int32))
    if rc:
        raise UsacError(rc, "usac_uniform_samples")
    return out


class Context:
    """One device + estimator + resident correspondence set (operator-level API)."""

    def __init__(self, estimator, points, device=0):
        L = lib()
        self.points = np.ascontiguousarray(points, dtype=np.float32)
        if self.points.ndim != 2:
            raise ValueError("points must be N x cols")
        self.estimator = ESTIMATOR(estimator)
        self.n, self.cols = self.points.shape
        h = _vp()
        rc = L.usac_create(ctypes.byref(h), device, int(self.estimator), _ptr(self.points, ctypes.c_float), self.n,
                           self.cols)
        if rc != 0:
            raise UsacError(rc, "usac_create(device=%d, estimator=%s, n=%d, cols=%d) failed (no usable GPU?)"
                            % (device, self.estimator.name, self.n, self.cols))
        self._h = h
        self.m = int(L.usac_sample_size(h))
        # model slots per minimal sample: the 7-point solver returns up to 3 models
        self.spk = 3 if self.estimator == ESTIMATOR.Fundamental else 1

    def close(self):
        if getattr(self, "_h", None):
            lib().usac_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            msg = lib().usac_last_error(self._h)
            raise UsacError(rc, "%s: %s" % (what, msg.decode() if msg else ""))

    def set_dlt_mode(self, mode):
        self._check(lib().usac_set_dlt_mode(self._h, int(mode)), "set_dlt_mode")

    def set_score_chunks(self, chunks):
        self._check(lib().usac_set_score_chunks(self._h, int(chunks)), "set_score_chunks")

    def selftest_rpoly(self, coeffs):
        """The device's 5-point root step alone (usac_selftest_rpoly) on polynomials of 11 ascending
        coefficients -> (roots B x 10, numbers of real zeros), rpoly's order."""
        a = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1, 11)
        r = np.zeros((a.shape[0], 10), np.float64)
        n = np.zeros(a.shape[0], np.int32)
        self._check(lib().usac_selftest_rpoly(self._h, _ptr(a, ctypes.c_double), a.shape[0], _ptr(r, ctypes.c_double),
                                              _ptr(n, ctypes.c_int32)), "selftest_rpoly")
        return r, n

    def selftest_logexp(self, x):
        """The root step's correctly rounded log / exp on the device (usac_selftest_logexp)."""
        v = np.ascontiguousarray(x, dtype=np.float64)
        lg = np.zeros_like(v)
        ex = np.zeros_like(v)
        self._check(lib().usac_selftest_logexp(self._h, _ptr(v, ctypes.c_double), len(v), _ptr(lg, ctypes.c_double),
                                               _ptr(ex, ctypes.c_double)), "selftest_logexp")
        return lg, ex

    def last_counts(self, n):
        """Per-slot (counts, sums) of the last batch as the score kernel left them."""
        c = np.zeros(n, dtype=np.int32)
        sm = np.zeros(n, dtype=np.float32)
        self._check(lib().usac_last_counts(self._h, _ptr(c, ctypes.c_int32), _ptr(sm, ctypes.c_float), n),
                    "last_counts")
        return c, sm

    def set_score_variant(self, variant):
        """0 = guard-band fast path (default), 1 = exact reference expression for every pair."""
        self._check(lib().usac_set_score_variant(self._h, int(variant)), "set_score_variant")

    def estimate_models(self, samples):
        """Estimator::EstimateModel over a batch of minimal samples -> (models, n_models):
        models is B x 9, or B x 3 x 9 for the fundamental 7-point solver (valid models first,
        zero-filled)."""
        s = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, self.m)
        B = s.shape[0]
        models = np.zeros((B, self.spk, 9), dtype=np.float32)
        nm = np.zeros(B, dtype=np.int32)
        self._check(lib().usac_estimate_models(self._h, _ptr(s, ctypes.c_int32), B, _ptr(models, ctypes.c_float),
                                               _ptr(nm, ctypes.c_int32)), "estimate_models")
        return (models[:, 0] if self.spk == 1 else models), nm

    def score_models(self, models, thr):
        """Quality::getNumberInliers for each model -> (counts, sums)."""
        m = np.ascontiguousarray(models, dtype=np.float32)
        if m.ndim == 1:
            m = m.reshape(1, -1)
        full = np.zeros((m.shape[0], 9), dtype=np.float32)
        full[:, : m.shape[1]] = m
        c = np.zeros(full.shape[0], dtype=np.int32)
        s = np.zeros(full.shape[0], dtype=np.float32)
        self._check(lib().usac_score_models(self._h, _ptr(full, ctypes.c_float), full.shape[0], ctypes.c_float(thr),
                                            _ptr(c, ctypes.c_int32), _ptr(s, ctypes.c_float)), "score_models")
        return c, s

    def knn(self, k, distances=True):
        """NearestNeighbors::getNearestNeighbors_nanoflann (nearest_neighbors.cpp:69-128) on the
        device -> (idx n x k int32, d2 n x k float32 or None): self excluded, ascending squared
        distance, equal distances by ascending index, -1 / inf where n - 1 < k."""
        idx = np.zeros((self.n, int(k)), dtype=np.int32)
        d2 = np.zeros((self.n, int(k)), dtype=np.float32) if distances else None
        self._check(lib().usac_knn(self._h, int(k), _ptr(idx, ctypes.c_int32),
                                   _ptr(d2, ctypes.c_float) if distances else None), "knn")
        return idx, d2

    def get_inliers(self, model, thr):
        """Quality::getNumberInliers(get_inliers=true) -> (count, sum, ascending indices)."""
        full = np.zeros(9, dtype=np.float32)
        mm = np.asarray(model, dtype=np.float32).reshape(-1)
        full[: mm.size] = mm
        idx = np.zeros(self.n, dtype=np.int32)
        n = ctypes.c_uint32(0)
        s = ctypes.c_float(0)
        self._check(lib().usac_get_inliers(self._h, _ptr(full, ctypes.c_float), ctypes.c_float(thr),
                                           _ptr(idx, ctypes.c_int32), ctypes.byref(n), ctypes.byref(s)),
                    "get_inliers")
        return n.value, s.value, idx[: n.value].copy()

    def nonminimal(self, idx):
        """Estimator::EstimateModelNonMinimalSample on the listed points."""
        i = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.zeros(9, dtype=np.float32)
        self._check(lib().usac_nonminimal(self._h, _ptr(i, ctypes.c_int32), i.size, _ptr(out, ctypes.c_float)),
                    "nonminimal")
        return out

    def lsq_fit(self, idx, weights=None):
        """usac_lsq_fit: EstimateModelNonMinimalSample(sample, n[, weights], model) -- weights (one
        float per point of the context, by point index) select the weighted overload
        (estimator.hpp:26; homography and fundamental)."""
        i = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.zeros(9, dtype=np.float32)
        wp = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.size != self.n:
                raise ValueError("weights: one per point (%d), got %d" % (self.n, w.size))
            wp = _ptr(w, ctypes.c_float)
        self._check(lib().usac_lsq_fit(self._h, _ptr(i, ctypes.c_int32), i.size, wp, _ptr(out, ctypes.c_float)),
                    "lsq_fit")
        return out

    def hypothesize_score(self, B=None, samples=None, seed=0, first_hyp=0, thr=2.0, per_hypothesis=True):
        """Fused sample + solve + score (+ batch best).  samples=None -> device sampler.
        Per-model outputs have B * spk entries (slot 3b + j = j-th valid model of sample b
        for the fundamental solver; count -1 marks an empty slot)."""
        L = lib()
        if samples is not None:
            s = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, self.m)
            B = s.shape[0]
        else:
            s = None
        c = np.zeros(B * self.spk, dtype=np.int32) if per_hypothesis else None
        sm = np.zeros(B * self.spk, dtype=np.float32) if per_hypothesis else None
        best = Record()
        self._check(L.usac_hypothesize_score(self._h, _ptr(s, ctypes.c_int32), B, seed, first_hyp,
                                             ctypes.c_float(thr), _ptr(c, ctypes.c_int32), _ptr(sm, ctypes.c_float),
                                             ctypes.byref(best)), "hypothesize_score")
        return c, sm, best.as_dict()

    def set_sprt(self, enable, seed=1, epsilon=0.0, delta=0.0):
        """Batch SPRT verification for the throughput entry points (reference defaults when
        epsilon / delta are 0)."""
        self._check(lib().usac_set_sprt(self._h, 1 if enable else 0, seed, epsilon, delta), "set_sprt")

    def set_device_sampler(self, sampler):
        """Sampler of the throughput batches' device stream: SAMPLER.Uniform, SAMPLER.Prosac
        (the reference's PROSAC subset schedule; points sorted by quality) or SAMPLER.Napsac
        (grid neighbours built on the device, cell size of set_cell_size)."""
        self._check(lib().usac_set_device_sampler(self._h, int(sampler)), "set_device_sampler")

    def set_cell_size(self, cell_size):
        """Grid cell of the device NAPSAC sampler (model.hpp:43, default 50)."""
        self._check(lib().usac_set_cell_size(self._h, int(cell_size)), "set_cell_size")

    def grid_neighbors(self, cell_size):
        """NearestNeighbors::getGridNearestNeighbors on the device -> dict of the CSR: cell, rank,
        start (n_cells + 1), members, and eligible (points with >= m neighbours)."""
        n = self.n
        nc, ne = ctypes.c_uint32(0), ctypes.c_uint32(0)
        cell = np.zeros(n, dtype=np.uint32)
        rank = np.zeros(n, dtype=np.uint32)
        start = np.zeros(n + 1, dtype=np.uint32)
        members = np.zeros(n, dtype=np.int32)
        elig = np.zeros(n, dtype=np.int32)
        u32 = ctypes.c_uint32
        self._check(lib().usac_grid_neighbors(self._h, int(cell_size), ctypes.byref(nc), _ptr(cell, u32),
                                              _ptr(rank, u32), _ptr(start, u32), _ptr(members, ctypes.c_int32),
                                              _ptr(elig, ctypes.c_int32), ctypes.byref(ne)), "grid_neighbors")
        return {"cell": cell, "rank": rank, "start": start[: nc.value + 1].copy(), "members": members,
                "eligible": elig[: ne.value].copy()}

    def draw_samples(self, B, seed, first_hyp=0):
        """The device stream's samples for hypotheses first_hyp .. first_hyp + B - 1 (B x m)."""
        out = np.zeros((B, self.m), dtype=np.int32)
        self._check(lib().usac_draw_samples(self._h, B, seed, first_hyp, out.ctypes.data_as(ctypes.c_void_p)),
                    "draw_samples")
        return out

    def batch_sprt_info(self, n_slots=0):
        """The batch SPRT's (epsilon, delta, A) and each slot's first pool position in the last batch."""
        eda = np.zeros(3, dtype=np.float64)
        st = np.zeros(max(n_slots, 1), dtype=np.uint32)
        self._check(lib().usac_batch_sprt_info(self._h, _ptr(eda, ctypes.c_double),
                                               _ptr(st, ctypes.c_uint32) if n_slots else None, n_slots),
                    "batch_sprt_info")
        return tuple(float(x) for x in eda), st[:n_slots]

    def sprt_tested(self):
        t = ctypes.c_uint64(0)
        self._check(lib().usac_sprt_tested(self._h, ctypes.byref(t)), "sprt_tested")
        return int(t.value)

    def hypothesize_async(self, B, seed, first_hyp, thr):
        self._check(lib().usac_hypothesize_async(self._h, B, seed, first_hyp, ctypes.c_float(thr)),
                    "hypothesize_async")

    def fetch_best(self):
        r = Record()
        self._check(lib().usac_fetch_best(self._h, ctypes.byref(r)), "fetch_best")
        return r

    def sync(self):
        self._check(lib().usac_sync(self._h), "sync")

    def set_timing(self, on):
        """usac_set_timing (ABI 14): record the batches' HIP events (default) or not."""
        self._check(lib().usac_set_timing(self._h, 1 if on else 0), "set_timing")

    def last_timings(self):
        ms = np.zeros(3, dtype=np.float32)
        self._check(lib().usac_last_timings(self._h, _ptr(ms, ctypes.c_float)), "last_timings")
        return {"batch_ms": float(ms[0]), "score_ms": float(ms[1]), "solve_ms": float(ms[2])}

    # ---- multi-GPU
    @staticmethod
    def comm_unique_id():
        buf = (ctypes.c_uint8 * 128)()
        rc = lib().usac_comm_unique_id(buf)
        if rc:
            raise UsacError(rc, "usac_comm_unique_id")
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        self._check(lib().usac_comm_init(self._h, nranks, rank, buf), "comm_init")
        self.nranks = nranks

    def comm_count(self):
        """(nranks, rank, device) as RCCL reports them for this context's communicator."""
        v = np.zeros(3, dtype=np.int32)
        p = [v[i:].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) for i in range(3)]
        self._check(lib().usac_comm_count(self._h, *p), "comm_count")
        return int(v[0]), int(v[1]), int(v[2])

    def allgather_record(self, rec):
        allr = (Record * self.nranks)()
        self._check(lib().usac_allgather_records(self._h, ctypes.byref(rec), allr), "allgather_records")
        return list(allr)

    XRING = 8  # USAC_XRING

    def exchange_best_async(self, batch_ctx, slot):
        """All-gather the batch best that hypothesize_async left on batch_ctx (same device) over
        this context's communicator, on its exchange stream, after batch_ctx's stream (no host
        staging, no wait on any compute stream); slot < XRING names it for exchange_best_wait."""
        self._check(lib().usac_exchange_best_async(self._h, batch_ctx._h, slot), "exchange_best_async")

    def exchange_best_wait(self, slot):
        allr = (Record * self.nranks)()
        self._check(lib().usac_exchange_best_wait(self._h, slot, allr), "exchange_best_wait")
        return list(allr)


class MultiContext:
    """P independent two-view problems of one estimator on one device, run together
    (include/usac_gpu.h usac_multi_*): point_sets is a list of n_p x 4 arrays, stored as one
    concatenated array plus offsets.  Sample, hypothesis and inlier indices are local to each problem,
    and every per-problem result equals a Context over that problem's points bit for bit.

    MultiContext(estimator, point_sets) takes Homography or Fundamental.  Essential-matrix problems
    come from MultiContext.essential(point_sets): calibrated coordinates (K^-1 x), 5-point samples, one
    slot per sample (count -1 on a sample without a model).  On such a context hypothesize_score,
    run (with and without polish), inliers, polish, draw_samples, run_prosac and prosac_scan work as
    for H / F; the LO, SPRT and NAPSAC methods raise UsacError(-3).

    MultiContext.essential_pixels(point_sets, K1, K2) is the same context from pixel coordinates and
    per-pair intrinsics: the device converts the rows, `points` holds the calibrated rows it wrote, and
    set_pixel_thresholds / pixel_models speak pixels on the way in and out.

    MultiContext.from_padded(estimator, rows, valid / counts) and MultiContext.from_matches(estimator, kpts0,
    kpts1, matches) take padded device tensors (usac_multi_create_device): the device packs the kept rows, nothing
    comes down at creation (`points` is None, resident_points() fetches the rows), `n_max` is the padded width and
    `source_index` the column of every packed row.  Such a context has inlier_lists = False: a polished run keeps
    its host mask as `last_mask` and returns no index lists, and padded_mask() hands the mask back as a
    (P, n_max) device tensor.  With scores=(P, n_max) float32 device tensor (usac_multi_create_device_sorted) the
    device also sorts every problem's kept rows by score, the better first and ties in column order: the input
    run_prosac expects, from a matcher's output as it is.  `sorted_by_score` is then True, `source_index` is in
    that order, and padded_mask() still lands every bit on its column.

    export_device() (usac_multi_export_device) hands the result of the last polishing call over as device tensors
    -- models, counts, the padded mask, the inliers' columns -- without a trip through the host, on any multi
    context; with keep_on_device = True the polishing calls bring no mask down in the first place."""

    inlier_lists = True  # False: polish(with_inliers=True) and the polished runs return no index lists
    last_mask = None     # the N_total host mask bytes of the last call that computed inliers
    n_max = None         # the padded width of a context from device input
    sorted_by_score = False  # True: from_padded / from_matches with scores, the rows are in quality order
    _keep_on_device = False  # keep_on_device: polishing calls leave their mask on the device (export_device)
    device = 0

    def __init__(self, estimator, point_sets, device=0):
        self._create(ESTIMATOR(estimator), point_sets, device, False)

    @classmethod
    def essential(cls, point_sets, device=0):
        """usac_multi_create_essential: a multi context of essential-matrix problems (the constructor
        keeps refusing ESTIMATOR.Essential)."""
        self = cls.__new__(cls)
        self._create(ESTIMATOR.Essential, point_sets, device, True)
        return self

    @staticmethod
    def _intrinsics(K, P, name):
        """one 3 x 3 matrix (for all problems) or P of them -> P x 9 float32"""
        K = np.asarray(K, dtype=np.float32)
        if K.shape == (3, 3):
            K = np.broadcast_to(K, (P, 3, 3))
        if K.shape != (P, 3, 3):
            raise ValueError("%s must be 3 x 3 or P x 3 x 3 (P = %d), got %s" % (name, P, K.shape))
        return np.ascontiguousarray(K.reshape(P, 9))

    @classmethod
    def essential_pixels(cls, point_sets, K1, K2=None, device=0):
        """usac_multi_create_essential_pixels: essential-matrix problems from pixel rows (u1, v1, u2, v2) and
        intrinsics K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]] -- K1 for view 1, K2 for view 2 (None: K1), each one
        3 x 3 matrix for all problems or P x 3 x 3.  The device converts the rows in place in fp32,
        y = (v - cy) / fy, x = ((u - cx) - s * y) / fx, and `points` is read back from it: the calibrated rows
        every other method works on.  UsacError(-1) for a K that is not finite, upper triangular with
        fx, fy > 0 and a last row of 0 0 1."""
        self = cls.__new__(cls)
        P = len(point_sets)
        k1 = cls._intrinsics(K1, P, "K1")
        k2 = None if K2 is None else cls._intrinsics(K2, P, "K2")
        self._create(ESTIMATOR.Essential, point_sets, device, True, k1, k2)
        return self

    def _create(self, estimator, point_sets, device, essential, k1=None, k2=None):
        L = lib()
        self.estimator = estimator
        self._h = None
        sets = [np.ascontiguousarray(p, dtype=np.float32) for p in point_sets]
        for p in sets:
            if p.ndim != 2 or p.shape[1] != 4:
                raise ValueError("every point set must be n x 4")
        self.P = len(sets)
        self.sizes = np.array([len(p) for p in sets], dtype=np.int64)
        self.offsets = np.zeros(self.P + 1, dtype=np.uint32)
        self.offsets[1:] = np.cumsum(self.sizes)
        self.points = np.concatenate(sets, axis=0) if sets else np.zeros((0, 4), np.float32)
        self.points = np.ascontiguousarray(self.points, dtype=np.float32)
        self.dlt_mode = DLT.THIN
        h = _vp()
        if k1 is not None:
            name = "usac_multi_create_essential_pixels"
            rc = L.usac_multi_create_essential_pixels(ctypes.byref(h), device, _ptr(self.points, ctypes.c_float),
                                                      _ptr(self.offsets, ctypes.c_uint32), self.P,
                                                      _ptr(k1, ctypes.c_float),
                                                      None if k2 is None else _ptr(k2, ctypes.c_float))
        elif essential:
            name = "usac_multi_create_essential"
            rc = L.usac_multi_create_essential(ctypes.byref(h), device, _ptr(self.points, ctypes.c_float),
                                               _ptr(self.offsets, ctypes.c_uint32), self.P)
        else:
            name = "usac_multi_create"
            rc = L.usac_multi_create(ctypes.byref(h), device, int(self.estimator), _ptr(self.points, ctypes.c_float),
                                     _ptr(self.offsets, ctypes.c_uint32), self.P)
        if rc != 0:
            raise UsacError(rc, "%s(device=%d, estimator=%s, P=%d) failed (bad arguments, or no "
                                "usable GPU)" % (name, device, self.estimator.name, self.P))
        self._h = h
        self.m = {ESTIMATOR.Fundamental: 7, ESTIMATOR.Essential: 5}.get(self.estimator, 4)
        self.spk = 3 if self.estimator == ESTIMATOR.Fundamental else 1
        if k1 is not None:  # the rows the device wrote replace the pixels
            self.points = self.resident_points()

    @classmethod
    def from_padded(cls, estimator, rows, valid=None, counts=None, K1=None, K2=None, stream=None, device=None,
                    scores=None, descending=True):
        """usac_multi_create_device, form a: rows is a (P, n_max, 4) float32 device tensor, with valid (P, n_max)
        bool or uint8, nonzero keeps the row, or counts (P,) int32, the first counts[p] rows are kept, or neither
        (all rows are kept).  estimator: Homography, Fundamental or Essential; K1 / K2 (Essential only, host, as
        essential_pixels') convert the kept pixel rows on the device.  stream: the stream handle that orders the
        writes of the tensors (default: torch's current stream for torch tensors, else 0); the call waits for it.
        TypeError for host arrays, ValueError for a wrong shape, dtype or a non-contiguous layout, UsacError(-1)
        naming the problem that keeps fewer rows than the sample size or has a count outside 0..n_max.
        scores (usac_multi_create_device_sorted): a (P, n_max) float32 device tensor, the quality of every column;
        the kept rows of a problem are then sorted on the device, the better score first (descending: the larger,
        else the smaller), equal scores (+0 and -0 are) in column order, NaNs last in column order; scores of
        columns that are not kept are not looked at.  None: column order, as without the argument."""
        r = _DevArray(rows, "rows").need((None, None, 4), ("f4",))
        P, n_max = r.shape[0], r.shape[1]
        v = None if valid is None else _DevArray(valid, "valid").need((P, n_max), ("b1", "u1"))
        c = None if counts is None else _DevArray(counts, "counts").need((P,), ("i4",))
        if v is not None and c is not None:
            raise ValueError("valid and counts are alternatives")
        s = None if scores is None else _DevArray(scores, "scores").need((P, n_max), ("f4",))
        inp = _MultiDeviceInput(P=P, n_max=n_max, rows=r.ptr, valid=v and v.ptr, counts=c and c.ptr)
        return cls._from_device(estimator, inp, [r, v, c, s], K1, K2, stream, device, s, descending)

    @classmethod
    def from_matches(cls, estimator, kpts0, kpts1, matches, K1=None, K2=None, stream=None, device=None,
                     scores=None, descending=True):
        """usac_multi_create_device, form b: kpts0 (P, n0, 2) and kpts1 (P, n1, 2) float32 device tensors and
        matches (P, n0) int32 (int64 is cast on the device): keypoint j of view 1 is kept when matches[p, j] >= 0,
        its row is (kpts0[p, j], kpts1[p, matches[p, j]]); n_max is n0.  Otherwise as from_padded; UsacError(-1)
        also for a match index >= n1, which is never dereferenced.  scores: (P, n0) float32, a matcher's score
        per keypoint of view 1, as from_padded's."""
        a = _DevArray(kpts0, "kpts0").need((None, None, 2), ("f4",))
        P, n0 = a.shape[0], a.shape[1]
        b = _DevArray(kpts1, "kpts1").need((P, None, 2), ("f4",))
        m = _DevArray(matches, "matches").need((P, n0), ("i4", "i8"))
        s = None if scores is None else _DevArray(scores, "scores").need((P, n0), ("f4",))
        if m.kind == "i8":
            if not m.torch:
                raise ValueError("matches must be of dtype i4, got i8")
            import torch

            # the cast runs on torch's current stream; a caller's other stream waits for it through the host
            m = _DevArray(matches.to(torch.int32), "matches")
            cur = torch.cuda.current_stream(matches.device)
            if stream is not None and int(stream) != cur.cuda_stream:
                cur.synchronize()
        inp = _MultiDeviceInput(P=P, n_max=n0, kpts0=a.ptr, kpts1=b.ptr, n1=b.shape[1], match=m.ptr)
        return cls._from_device(estimator, inp, [a, b, m, s], K1, K2, stream, device, s, descending)

    @classmethod
    def _from_device(cls, estimator, inp, arrays, K1, K2, stream, device, scores=None, descending=True):
        arrays = [a for a in arrays if a is not None]
        self = cls.__new__(cls)
        self._h = None
        self.estimator = ESTIMATOR(estimator)
        if device is None:
            device = next((a.device for a in arrays if a.device is not None), 0)
        if stream is None:
            stream = 0
            if arrays[0].torch:
                import torch

                stream = torch.cuda.current_stream(arrays[0].obj.device).cuda_stream
        P = int(inp.P)
        if K2 is not None and K1 is None:
            raise ValueError("K2 without K1")
        k1 = None if K1 is None else cls._intrinsics(K1, P, "K1")
        k2 = None if K2 is None else cls._intrinsics(K2, P, "K2")
        inp.K1 = _ptr(k1, ctypes.c_float)
        inp.K2 = _ptr(k2, ctypes.c_float)
        inp.stream = int(stream) or None
        L = lib()
        h = _vp()
        if scores is None:
            rc = L.usac_multi_create_device(ctypes.byref(h), int(device), int(self.estimator), ctypes.byref(inp))
        else:
            order = _MultiDeviceOrder(scores=scores.ptr, descending=1 if descending else 0)
            rc = L.usac_multi_create_device_sorted(ctypes.byref(h), int(device), int(self.estimator), ctypes.byref(inp),
                                                   ctypes.byref(order))
        if rc != 0:
            msg = L.usac_multi_last_error(None)
            raise UsacError(rc, msg.decode() if msg else "usac_multi_create_device failed")
        self._h = h
        self.device = int(device)
        self.P, self.n_max = P, int(inp.n_max)
        self.offsets = np.zeros(P + 1, dtype=np.uint32)
        self._check(L.usac_multi_get_offsets(self._h, _ptr(self.offsets, ctypes.c_uint32)), "multi_get_offsets")
        self.sizes = np.diff(self.offsets.astype(np.int64))
        self.points = None  # nothing comes down at creation: resident_points()
        self.dlt_mode = DLT.THIN
        self.m = {ESTIMATOR.Fundamental: 7, ESTIMATOR.Essential: 5}.get(self.estimator, 4)
        self.spk = 3 if self.estimator == ESTIMATOR.Fundamental else 1
        self.inlier_lists = False
        self.sorted_by_score = scores is not None
        self._source = None
        return self

    @property
    def source_index(self):
        """usac_multi_get_source (a context from device input): per packed row the column of the padded input it
        came from, a uint32 array of N_total values, ascending within a problem (sorted_by_score: in quality
        order); fetched at first use."""
        if getattr(self, "_source", None) is None:
            src = np.zeros(int(self.offsets[-1]), dtype=np.uint32)
            self._check(lib().usac_multi_get_source(self._h, _ptr(src, ctypes.c_uint32)), "multi_get_source")
            self._source = src
        return self._source

    def padded_mask(self, mask=None, out=None, stream=None):
        """usac_multi_padded_mask (a context from device input): the N_total mask bytes of a call that computed
        inliers (None: last_mask, the last such call's) scattered into a (P, n_max) device array, zero wherever no
        packed row came from.  out: a (P, n_max) uint8 device tensor to write (it is returned); None: a fresh
        torch tensor, returned as a torch.bool view.  stream as from_padded's; the call waits for it."""
        if self.n_max is None:
            raise UsacError(-3, "padded_mask: the context was not created from device input")
        mask = self.last_mask if mask is None else mask
        if mask is None:
            raise ValueError("padded_mask: no mask given and no call has computed one yet")
        mask = np.ascontiguousarray(mask, dtype=np.uint8).ravel()
        if mask.size != int(self.offsets[-1]):
            raise ValueError("padded_mask: N_total = %d mask bytes, got %d" % (int(self.offsets[-1]), mask.size))
        fresh = out is None
        if fresh:
            import torch

            out = torch.empty((self.P, self.n_max), dtype=torch.uint8, device="cuda:%d" % self.device)
        o = _DevArray(out, "out").need((self.P, self.n_max), ("u1", "b1"))
        if stream is None:
            stream = 0
            if o.torch:
                import torch

                stream = torch.cuda.current_stream(out.device).cuda_stream
        self._check(lib().usac_multi_padded_mask(self._h, _ptr(mask, ctypes.c_uint8), o.ptr, int(stream) or None),
                    "multi_padded_mask")
        if fresh:
            import torch

            return out.view(torch.bool)
        return out

    @property
    def keep_on_device(self):
        """usac_multi_set_resident: while True, polish() and the polished runs bring no mask to the host -- the
        mask stays on the device for export_device(), `last_mask` is not set and no index lists are built."""
        return self._keep_on_device

    @keep_on_device.setter
    def keep_on_device(self, on):
        self._check(lib().usac_multi_set_resident(self._h, 1 if on else 0), "multi_set_resident")
        self._keep_on_device = bool(on)

    def export_device(self, mask=True, inlier_cols=None, pixel_models=False, n_max=None, out=None, stream=None):
        """usac_multi_export_device: the result of the last polishing call (polish, or a run with polish=True) as
        tensors on the context's device, written by one launch: "models" (P, 3, 3) float32, "inliers" (P,) int32
        (the full counts), "status" (P,) int32, and, as asked for, "mask" (P, n_max) bool, "inlier_cols" (P, k)
        int32 with inlier_cols=k (the inliers' columns in packed-row order, the first k of them, -1 behind the
        last) and "pixel_models" (P, 3, 3) float32 (a context with intrinsics).  n_max: the context's padded width
        (the default, and the only value a context from device input takes); on a context from the host any
        width >= the largest problem, default that size, and columns are local indices.  out: a dict of caller
        tensors under the same keys, written instead of fresh ones and returned as they are (mask: uint8 or
        bool).  stream: as padded_mask's; the call waits for it.  UsacError(-3) when no polishing call's result
        is resident (the message says what ended it), or for pixel_models without intrinsics."""
        P = self.P
        out = dict(out or {})
        unknown = set(out) - {"models", "inliers", "status", "mask", "inlier_cols", "pixel_models"}
        if unknown:
            raise ValueError("export_device: unknown outputs %s" % sorted(unknown))
        if n_max is None:
            n_max = self.n_max if self.n_max is not None else int(self.sizes.max())
        n_max = int(n_max)
        k_max = None if inlier_cols is None else int(inlier_cols)
        if k_max is None and "inlier_cols" in out:
            k_max = _DevArray(out["inlier_cols"], "inlier_cols").need((P, None), ("i4",)).shape[1]
        want = {"models": ((P, 3, 3), ("f4",)), "inliers": ((P,), ("i4",)), "status": ((P,), ("i4",))}
        if mask or "mask" in out:
            want["mask"] = ((P, n_max), ("u1", "b1"))
        if k_max is not None:
            want["inlier_cols"] = ((P, k_max), ("i4",))
        if pixel_models or "pixel_models" in out:
            want["pixel_models"] = ((P, 3, 3), ("f4",))
        res, arrays = {}, {}
        for key, (shape, kinds) in want.items():
            fresh = key not in out
            if fresh:
                import torch

                dt = {"f4": torch.float32, "i4": torch.int32, "u1": torch.uint8}[kinds[0]]
                out[key] = torch.empty(shape, dtype=dt, device="cuda:%d" % self.device)
            arrays[key] = _DevArray(out[key], key).need(shape, kinds)
            res[key] = out[key].view(torch.bool) if fresh and key == "mask" else out[key]
        if stream is None:
            stream = 0
            first = next(iter(arrays.values()))
            if first.torch:
                import torch

                stream = torch.cuda.current_stream(first.obj.device).cuda_stream
        o = _MultiDeviceOutput(n_max=n_max, k_max=k_max or 0, stream=int(stream) or None,
                               **{key: a.ptr for key, a in arrays.items()})
        self._check(lib().usac_multi_export_device(self._h, ctypes.byref(o)), "multi_export_device")
        return res

    def export_pose(self, front_mask=False, n_max=None, out=None, stream=None):
        """usac_multi_pose_device (an essential context): the relative pose of every problem's polished model,
        chosen on the device from the result of the last polishing call -- of the four [R | t] of E the one that
        puts the most inliers in front of both cameras (x2 ~ R x1 + t, |t| = 1, det R = +1).  Tensors on the
        context's device, written by one launch: "R" (P, 3, 3) float32, "t" (P, 3) float32, "front" (P,) int32
        (the inliers in front), "choice" (P,) int32 (0..3; -1: no inlier in front of any candidate, or a problem
        without a model -- R is then the identity and t zero) and, with front_mask=True, "front_mask" (P, n_max)
        bool.  n_max, out and stream: as export_device's.  The resident result stays as it is."""
        P = self.P
        out = dict(out or {})
        unknown = set(out) - {"R", "t", "front", "choice", "front_mask"}
        if unknown:
            raise ValueError("export_pose: unknown outputs %s" % sorted(unknown))
        if n_max is None:
            n_max = self.n_max if self.n_max is not None else int(self.sizes.max())
        n_max = int(n_max)
        want = {"R": ((P, 3, 3), ("f4",)), "t": ((P, 3), ("f4",)), "front": ((P,), ("i4",)), "choice": ((P,), ("i4",))}
        if front_mask or "front_mask" in out:
            want["front_mask"] = ((P, n_max), ("u1", "b1"))
        res, arrays = {}, {}
        for key, (shape, kinds) in want.items():
            fresh = key not in out
            if fresh:
                import torch

                dt = {"f4": torch.float32, "i4": torch.int32, "u1": torch.uint8}[kinds[0]]
                out[key] = torch.empty(shape, dtype=dt, device="cuda:%d" % self.device)
            arrays[key] = _DevArray(out[key], key).need(shape, kinds)
            res[key] = out[key].view(torch.bool) if fresh and key == "front_mask" else out[key]
        if stream is None:
            stream = 0
            first = next(iter(arrays.values()))
            if first.torch:
                import torch

                stream = torch.cuda.current_stream(first.obj.device).cuda_stream
        o = _MultiPoseOutput(n_max=n_max, stream=int(stream) or None, **{key: a.ptr for key, a in arrays.items()})
        self._check(lib().usac_multi_pose_device(self._h, ctypes.byref(o)), "multi_pose_device")
        return res

    def pose(self, E, mask=None):
        """usac_multi_pose: the same choice for models of the caller's own.  E: (P, 3, 3) or (P, 9) float32; mask:
        N_total bytes over the packed rows (None: every row).  Returns a dict of numpy arrays: "R" (P, 3, 3), "t"
        (P, 3), "front" (P,), "choice" (P,) and "front_mask" (N_total,) uint8 in packed-row order."""
        P, n = self.P, int(self.offsets[-1])
        m = np.ascontiguousarray(E, dtype=np.float32).reshape(P, 9)
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
            if mask.size != n:
                raise ValueError("pose: mask must have N_total = %d bytes" % n)
        R = np.zeros((P, 3, 3), dtype=np.float32)
        t = np.zeros((P, 3), dtype=np.float32)
        front = np.zeros(P, dtype=np.int32)
        choice = np.zeros(P, dtype=np.int32)
        fm = np.zeros(n, dtype=np.uint8)
        self._check(lib().usac_multi_pose(self._h, _ptr(m, ctypes.c_float), _ptr(mask, ctypes.c_uint8),
                                          _ptr(R, ctypes.c_float), _ptr(t, ctypes.c_float), _ptr(front, ctypes.c_int32),
                                          _ptr(choice, ctypes.c_int32), _ptr(fm, ctypes.c_uint8)), "multi_pose")
        return {"R": R, "t": t, "front": front, "choice": choice, "front_mask": fm}

    def refine_pose(self, R, t, mask=None, max_iters=10, n_max=None, out=None, stream=None):
        """usac_multi_refine_pose_device (an essential context): the poses R (P, 3, 3) and t (P, 3), float32 device
        tensors such as export_pose's, refined on the device by up to max_iters Levenberg-Marquardt trial steps on
        the five pose parameters over the Sampson distances of the masked rows (include/usac_gpu.h "Pose
        refinement").  mask: a (P, n_max) bool or uint8 device tensor with a row's byte at its source column, such
        as export_pose's "front_mask"; None: the resident inlier mask.  The status of a problem is the resident
        result's.  Tensors on the context's device, written by one launch: "R" (P, 3, 3), "t" (P, 3) and "E"
        (P, 3, 3) float32 (E = [t]x R), "cost0" and "cost" (P,) float64 (cost <= cost0), "iterations" (P,) int32
        (-1: the problem was skipped and R, t are the inputs) and "used" (P,) int32.  out may name R and t
        themselves as outputs: the refinement is then in place.  n_max, out and stream: as export_device's.  The
        resident result stays as it is."""
        import torch

        P = self.P
        out = dict(out or {})
        spec = {"R": ((P, 3, 3), "f4"), "t": ((P, 3), "f4"), "E": ((P, 3, 3), "f4"), "cost0": ((P,), "f8"),
                "cost": ((P,), "f8"), "iterations": ((P,), "i4"), "used": ((P,), "i4")}
        unknown = set(out) - set(spec)
        if unknown:
            raise ValueError("refine_pose: unknown outputs %s" % sorted(unknown))
        if n_max is None:
            n_max = self.n_max if self.n_max is not None else int(self.sizes.max())
        n_max = int(n_max)
        max_iters = int(max_iters)
        if not 0 <= max_iters <= 100:
            raise ValueError("refine_pose: max_iters must be 0..100")
        ins = {"R_in": _DevArray(R, "R").need((P, 3, 3), ("f4",)), "t_in": _DevArray(t, "t").need((P, 3), ("f4",))}
        if mask is not None:
            ins["mask_in"] = _DevArray(mask, "mask").need((P, n_max), ("u1", "b1"))
        arrays = {}
        for key, (shape, kind) in spec.items():
            if key not in out:
                dt = {"f4": torch.float32, "f8": torch.float64, "i4": torch.int32}[kind]
                out[key] = torch.empty(shape, dtype=dt, device="cuda:%d" % self.device)
            arrays[key] = _DevArray(out[key], key).need(shape, (kind,))
        res = {key: out[key] for key in spec}
        if stream is None:
            stream = 0
            first = ins["R_in"]
            if first.torch:
                stream = torch.cuda.current_stream(first.obj.device).cuda_stream
        o = _MultiRefineIO(n_max=n_max, max_iters=max_iters, stream=int(stream) or None,
                           **{key: a.ptr for key, a in list(ins.items()) + list(arrays.items())})
        self._check(lib().usac_multi_refine_pose_device(self._h, ctypes.byref(o)), "multi_refine_pose_device")
        return res

    def refine(self, R, t, mask=None, max_iters=10):
        """usac_multi_refine_pose: the same refinement from numpy arrays.  R: (P, 3, 3) or (P, 9) float32, t: (P, 3);
        mask: N_total bytes over the packed rows (None: every row); every status counts as OK.  Returns a dict of
        numpy arrays: "R" (P, 3, 3), "t" (P, 3), "E" (P, 3, 3) float32, "cost0", "cost" (P,) float64, "iterations"
        and "used" (P,) int32."""
        P, n = self.P, int(self.offsets[-1])
        R = np.ascontiguousarray(R, dtype=np.float32).reshape(P, 9)
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(P, 3)
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
            if mask.size != n:
                raise ValueError("refine: mask must have N_total = %d bytes" % n)
        max_iters = int(max_iters)
        if not 0 <= max_iters <= 100:
            raise ValueError("refine: max_iters must be 0..100")
        Ro = np.zeros((P, 3, 3), dtype=np.float32)
        to = np.zeros((P, 3), dtype=np.float32)
        E = np.zeros((P, 3, 3), dtype=np.float32)
        cost0 = np.zeros(P, dtype=np.float64)
        cost = np.zeros(P, dtype=np.float64)
        iterations = np.zeros(P, dtype=np.int32)
        used = np.zeros(P, dtype=np.int32)
        self._check(lib().usac_multi_refine_pose(
            self._h, _ptr(R, ctypes.c_float), _ptr(t, ctypes.c_float), _ptr(mask, ctypes.c_uint8), max_iters,
            _ptr(Ro, ctypes.c_float), _ptr(to, ctypes.c_float), _ptr(E, ctypes.c_float), _ptr(cost0, ctypes.c_double),
            _ptr(cost, ctypes.c_double), _ptr(iterations, ctypes.c_int32), _ptr(used, ctypes.c_int32)), "multi_refine_pose")
        return {"R": Ro, "t": to, "E": E, "cost0": cost0, "cost": cost, "iterations": iterations, "used": used}

    def resident_points(self):
        """usac_multi_get_points: the N_total x 4 rows resident on the device (a copy)."""
        out = np.zeros((int(self.offsets[-1]), 4), dtype=np.float32)
        self._check(lib().usac_multi_get_points(self._h, _ptr(out, ctypes.c_float)), "multi_get_points")
        return out

    def set_pixel_thresholds(self, t):
        """usac_multi_set_pixel_thresholds (a context from essential_pixels): a pixel tolerance for all
        problems, or P of them; problem p's threshold becomes (t / f_p)^2 with f_p the mean of its four focal
        lengths, in fp32, installed as by set_thresholds (`thresholds` shows the values, set_thresholds(None)
        clears them).  The essential residual it is compared with is a distance in calibrated units, not a
        squared one, so (t / f)^2 admits t^2 / f pixels of it: 45 px at f = 1000 give 0.002.  UsacError(-1),
        nothing changed, for a wrong length or a tolerance that is not finite and > 0; UsacError(-3) on a
        context not created from pixels."""
        t = np.ascontiguousarray(t, dtype=np.float32).ravel()
        self._check(lib().usac_multi_set_pixel_thresholds(self._h, _ptr(t, ctypes.c_float), t.size),
                    "multi_set_pixel_thresholds")

    def pixel_models(self, E):
        """usac_multi_pixel_models (a context from essential_pixels): E, P x 3 x 3 or P x 9 essential matrices ->
        F_p = K2_p^-T E_p K1_p^-1 in the same shape, computed in fp64 on the host, not normalised."""
        E = np.ascontiguousarray(E, dtype=np.float32)
        if E.size != 9 * self.P:
            raise ValueError("pixel_models: P x 9 values (P = %d), got %s" % (self.P, E.shape))
        F = np.zeros_like(E)
        self._check(lib().usac_multi_pixel_models(self._h, _ptr(E, ctypes.c_float), _ptr(F, ctypes.c_float)),
                    "multi_pixel_models")
        return F

    def close(self):
        if getattr(self, "_h", None):
            lib().usac_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            msg = lib().usac_multi_last_error(self._h)
            raise UsacError(rc, "%s: %s" % (what, msg.decode() if msg else ""))

    def set_dlt_mode(self, mode):
        self.dlt_mode = DLT(mode)

    def set_thresholds(self, thr):
        """usac_multi_set_thresholds: one inlier threshold per problem (P finite values > 0, in the
        units of each problem's own coordinates), or None to clear them.  While set, every method
        that takes a threshold -- thr, or the model's -- uses problem p's value for problem p (whatever
        its place in `problems`) and ignores its own; they persist like set_dlt_mode.  UsacError(-1),
        nothing changed, for a wrong length or a value that is not finite and > 0."""
        if thr is None:
            self._check(lib().usac_multi_set_thresholds(self._h, None), "multi_set_thresholds")
            return
        t = np.ascontiguousarray(thr, dtype=np.float32).ravel()
        if t.size != self.P:
            raise UsacError(-1, "set_thresholds: one threshold per problem (%d), got %d" % (self.P, t.size))
        self._check(lib().usac_multi_set_thresholds(self._h, _ptr(t, ctypes.c_float)), "multi_set_thresholds")

    @property
    def thresholds(self):
        """The per-problem thresholds in effect (a float32 array of P values), or None."""
        out = np.zeros(self.P, dtype=np.float32)
        rc = lib().usac_multi_get_thresholds(self._h, _ptr(out, ctypes.c_float))
        if rc < 0:
            self._check(rc, "multi_get_thresholds")
        return out if rc == 1 else None

    def hypothesize_score(self, R, seeds=None, first_hyp=0, thr=2.0, problems=None, samples=None,
                          per_hypothesis=True):
        """One round of R hypotheses (a multiple of 64 in 64..8192) for the listed problems (None:
        all, in order): seeds[i] keys the device sampler of problems[i]; samples (A x R x m, indices
        local to each problem) replace it.  Returns (counts A x R*spk, sums, list of A best-record
        dicts); counts and sums are None without per_hypothesis."""
        A = self.P if problems is None else len(problems)
        pr = None if problems is None else np.ascontiguousarray(problems, dtype=np.uint32)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd is not None and sd.size != A:
            raise ValueError("seeds: one per listed problem (%d), got %d" % (A, sd.size))
        sm = None
        if samples is not None:
            sm = np.ascontiguousarray(samples, dtype=np.int32)
            if sm.size != A * R * self.m:
                raise ValueError("samples must be %d x %d x %d" % (A, R, self.m))
        c = np.zeros((A, R * self.spk), dtype=np.int32) if per_hypothesis else None
        s = np.zeros((A, R * self.spk), dtype=np.float32) if per_hypothesis else None
        best = (Record * max(A, 1))()
        self._check(lib().usac_multi_hypothesize_score(
            self._h, _ptr(pr, ctypes.c_uint32), A, _ptr(sm, ctypes.c_int32), R, _ptr(sd, ctypes.c_uint64), first_hyp,
            ctypes.c_float(thr), int(self.dlt_mode), _ptr(c, ctypes.c_int32), _ptr(s, ctypes.c_float), best),
            "multi_hypothesize_score")
        return c, s, [best[i].as_dict() for i in range(A)]

    def _split_mask(self, mask):
        """N_total mask bytes -> per problem the ascending local indices of its set bytes"""
        o = self.offsets.astype(np.int64)
        idx = np.flatnonzero(mask.view(np.bool_))  # the bytes are 0 / 1; nonzero is far faster on bool
        cuts = np.searchsorted(idx, o)
        local = (idx - np.repeat(o[:-1], np.diff(cuts))).astype(np.int32)
        c = cuts.tolist()
        return [local[c[p]:c[p + 1]] for p in range(self.P)]

    def polish(self, models, thr, with_inliers=False):
        """usac_multi_polish: the non-minimal polish of ransac.cpp:157-214 for every problem from its
        start model (P x 9), one workgroup per problem.  Returns a list of P dicts: model, inliers,
        score, minimal_inliers, minimal_score (the start model's), passes, status (-111 when the
        start model has no inlier) -- and, with_inliers, "inlier_idx": the final getInliers of the
        model, ascending indices local to the problem."""
        m = np.ascontiguousarray(models, dtype=np.float32).reshape(self.P, 9)
        out = (_MultiPolishOutput * self.P)()
        with_inliers = with_inliers and not self._keep_on_device  # keep_on_device: the mask stays on the device
        mask = np.zeros(int(self.offsets[-1]), dtype=np.uint8) if with_inliers else None
        self._check(lib().usac_multi_polish(self._h, _ptr(m, ctypes.c_float), ctypes.c_float(thr), out,
                                            _ptr(mask, ctypes.c_uint8)), "multi_polish")
        res = _MultiPolishOutput.as_dicts(out)
        if with_inliers:
            self.last_mask = mask
        if with_inliers and self.inlier_lists:
            for r, idx in zip(res, self._split_mask(mask)):
                r["inlier_idx"] = idx
        return res

    def _run_params(self, model_or_params):
        if isinstance(model_or_params, _Params):
            return model_or_params
        p = _params(model_or_params)
        p.seed = model_or_params.seed  # the default seeds are seed + p, never a random one
        return p

    def _run(self, name, model_or_params, seeds, polish, own=None, prosac=None):
        """What the run methods share: usac_multi_<name>(handle, params, seeds, out[, own's array]
        [, PROSAC's array][, polish results, mask]) and its list of P result dicts.  own: (key,
        structure[, wanted]) of the method's own per-problem output (not wanted: NULL is passed).  prosac: the call takes PROSAC's array, and
        its keys are returned "always" or under the PROSAC "sampler" only.  The polish arguments go to
        every function but usac_multi_run."""
        p = self._run_params(model_or_params)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd is not None and sd.size != self.P:
            raise ValueError("seeds: one per problem (%d), got %d" % (self.P, sd.size))
        out = (_MultiOutput * self.P)()
        ex = (own[1] * self.P)() if own and (len(own) < 3 or own[2]) else None  # own[2] False: a NULL argument
        pro = (_MultiProsacOutput * self.P)() if prosac else None
        pol = (_MultiPolishOutput * self.P)() if polish else None
        host_mask = polish and not self._keep_on_device  # keep_on_device: the mask stays on the device
        mask = np.zeros(int(self.offsets[-1]), dtype=np.uint8) if host_mask else None
        args = ([ex] if own else []) + ([pro] if prosac else [])
        if name != "run":
            args += [pol, _ptr(mask, ctypes.c_uint8)]
        self._check(getattr(lib(), "usac_multi_" + name)(self._h, ctypes.byref(p), _ptr(sd, ctypes.c_uint64), out, *args),
                    "multi_" + name)
        res = [{"best": o.best.as_dict(), "hypotheses": int(o.hypotheses), "rounds": int(o.rounds),
                "bound": int(o.bound), "status": int(o.status)} for o in out]
        if ex is not None:
            for r, q in zip(res, ex):
                r[own[0]] = q.as_dict()
        if prosac == "always" or (prosac and p.sampler == int(SAMPLER.Prosac)):
            for r, q in zip(res, pro):
                r.update(termination_length=int(q.termination_length), largest_sample_size=int(q.largest_sample_size),
                         clock=int(q.clock), scans=int(q.scans))
        if polish:
            if host_mask:
                self.last_mask = mask
            for r, po in zip(res, _MultiPolishOutput.as_dicts(pol)):
                r["polished"] = po
        if host_mask and self.inlier_lists:
            for r, idx in zip(res, self._split_mask(mask)):
                r["inliers"] = idx
        return res

    def run(self, model_or_params, seeds=None, polish=False):
        """usac_multi_run: batch-granular RANSAC with the standard termination criterion over all
        problems (uniform device sampler; no SPRT; LO: run_lo).  model_or_params: a Model or a
        usac_params structure; seeds default to model.seed + p.  Returns a list of P dicts: best
        (record dict), hypotheses, rounds, bound, status.  polish=True (usac_multi_run_polished)
        adds the non-minimal polish of every best model at the run's threshold: each dict gains
        "polished" (polish()'s dict) and "inliers" (the polished model's inliers, ascending local
        indices)."""
        return self._run("run_polished" if polish else "run", model_or_params, seeds, polish)

    def draw_samples(self, R, seeds, first_hyp=0, problems=None, clock=None, term_len=None):
        """usac_multi_draw_samples (for tests): the samples a round's solve kernels draw, A x R x m local
        indices.  clock=None: the uniform sampler; else the PROSAC sampler with clock[i] (its hypCount
        at the round's first lane) and term_len[i] (default n_p) for the i-th listed problem."""
        A = self.P if problems is None else len(problems)
        pr = None if problems is None else np.ascontiguousarray(problems, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd.size != A:
            raise ValueError("seeds: one per listed problem (%d), got %d" % (A, sd.size))
        ck = tl = None
        if clock is not None:
            ck = np.ascontiguousarray(clock, dtype=np.uint32)
            ids = np.arange(self.P) if problems is None else np.asarray(problems, dtype=np.int64)
            tl = np.ascontiguousarray(self.sizes[ids] if term_len is None else term_len, dtype=np.uint32)
            if ck.size != A or tl.size != A:
                raise ValueError("clock / term_len: one per listed problem (%d)" % A)
        out = np.zeros((A, R, self.m), dtype=np.int32)
        self._check(lib().usac_multi_draw_samples(self._h, _ptr(pr, ctypes.c_uint32), A, R, _ptr(sd, ctypes.c_uint64),
                                                  first_hyp, _ptr(ck, ctypes.c_uint32), _ptr(tl, ctypes.c_uint32),
                                                  _ptr(out, ctypes.c_int32)), "multi_draw_samples")
        return out

    def run_prosac(self, model_or_params, seeds=None, polish=False):
        """usac_multi_run_prosac: run() with the PROSAC sampler and PROSAC's termination criterion per
        problem; every point set sorted by descending quality.  Returns run()'s dicts plus
        termination_length, largest_sample_size, clock (the sampler's hypCount at the end) and scans;
        polish=True adds "polished" and "inliers" as run() does."""
        return self._run("run_prosac", model_or_params, seeds, polish, prosac="always")

    def prosac_scan(self, model_or_params, models, hyp_count, largest, reset=False):
        """usac_multi_prosac_scan (for tests): one PROSAC termination scan of every problem with models
        (P x 9) as new bests at hypothesis hyp_count[p] and largest_sample_size largest[p]; the state
        persists between calls, reset=True starts it afresh.  Returns (bound uint32[P], term_len
        uint32[P], candidates: per problem a k x 2 array of (i, count), ascending i)."""
        p = self._run_params(model_or_params)
        m = np.ascontiguousarray(models, dtype=np.float32).reshape(self.P, 9)
        hc = np.ascontiguousarray(hyp_count, dtype=np.uint32)
        lg = np.ascontiguousarray(largest, dtype=np.uint32)
        if hc.size != self.P or lg.size != self.P:
            raise ValueError("hyp_count / largest: one per problem (%d)" % self.P)
        bound, tl, nc = (np.zeros(self.P, dtype=np.uint32) for _ in range(3))
        cand = np.zeros((int(self.offsets[-1]) // 2 + self.P, 2), dtype=np.uint32)
        u32 = ctypes.c_uint32
        self._check(lib().usac_multi_prosac_scan(self._h, ctypes.byref(p), 1 if reset else 0, _ptr(m, ctypes.c_float),
                                                 _ptr(hc, u32), _ptr(lg, u32), _ptr(bound, u32), _ptr(tl, u32),
                                                 _ptr(nc, u32), _ptr(cand, u32)), "multi_prosac_scan")
        segs = [cand[int(o) // 2 + q:int(o) // 2 + q + int(nc[q])].copy() for q, o in enumerate(self.offsets[:-1])]
        return bound, tl, segs

    def lo(self, model_or_params, records, seeds=None, reset=True, _entry="multi_lo"):
        """usac_multi_lo: one LO call (inner + iterative LO-RANSAC, model.lo = InItLORsc / InItFLORsc) for
        every problem, records[p] (a Record or a record dict) taken as a new best.  The LO threshold, the
        draw counter and the counters persist between calls unless reset.  Returns (list of P record
        dicts, list of P dicts: lo_calls, inner_iters, iterative_iters, fits, improved, capped, draws,
        threshold)."""
        p = self._run_params(model_or_params)
        if len(records) != self.P:
            raise ValueError("records: one per problem (%d), got %d" % (self.P, len(records)))
        recs = (Record * self.P)()
        for i, r in enumerate(records):
            if isinstance(r, Record):
                recs[i] = r
            else:
                recs[i] = Record(int(r["hyp_index"]), int(r["inliers"]), float(r["score"]),
                                 (ctypes.c_float * 9)(*np.asarray(r["model"], dtype=np.float32).tolist()),
                                 int(r["valid"]))
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd is not None and sd.size != self.P:
            raise ValueError("seeds: one per problem (%d), got %d" % (self.P, sd.size))
        lo = (_MultiLoOutput * self.P)()
        self._check(getattr(lib(), "usac_" + _entry)(self._h, ctypes.byref(p), 1 if reset else 0, _ptr(sd, ctypes.c_uint64),
                                                     recs, lo), _entry)
        return [r.as_dict() for r in recs], [q.as_dict() for q in lo]

    def lo_essential(self, model_or_params, records, seeds=None, reset=True):
        """usac_multi_lo_essential: lo() on a context of essential-matrix problems (MultiContext.essential),
        where lo() itself keeps refusing: sample size 5, the 8-point non-minimal fit, the squared Sampson
        distance in calibrated coordinates.  Returns what lo() returns."""
        return self.lo(model_or_params, records, seeds, reset, _entry="multi_lo_essential")

    def run_lo(self, model_or_params, seeds=None, polish=False):
        """usac_multi_run_lo: run() (model.sampler Uniform) or run_prosac() (Prosac) with LO-RANSAC of every
        round's new bests on the device (model.lo = InItLORsc / InItFLORsc).  Returns run()'s dicts plus
        "lo" (the problem's LO counters and threshold); with PROSAC also run_prosac()'s keys; polish=True
        adds "polished" and "inliers" as run() does."""
        return self._run("run_lo", model_or_params, seeds, polish, own=("lo", _MultiLoOutput), prosac="sampler")

    def run_lo_essential(self, model_or_params, seeds=None, polish=False):
        """usac_multi_run_lo_essential: run_lo() on a context of essential-matrix problems
        (MultiContext.essential), where run_lo() itself keeps refusing.  Returns what run_lo() returns."""
        return self._run("run_lo_essential", model_or_params, seeds, polish, own=("lo", _MultiLoOutput), prosac="sampler")

    def set_sprt_pool(self, seeds=None):
        """usac_multi_sprt_setup: the problems' SPRT pools (the reference's shuffle after srandom(seeds[p]),
        default p + 1 -- what Context.set_sprt(seed=seeds[p]) uses) and the pool-ordered copy of the
        points on the device.  Once per context; the SPRT calls below do it with the default seeds
        if it was never called."""
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
        if sd is not None and sd.size != self.P:
            raise ValueError("seeds: one per problem (%d), got %d" % (self.P, sd.size))
        self._check(lib().usac_multi_sprt_setup(self._h, _ptr(sd, ctypes.c_uint32)), "multi_sprt_setup")

    def hypothesize_score_sprt(self, R, seeds=None, first_hyp=0, thr=2.0, problems=None, samples=None,
                               eps_delta=None):
        """usac_multi_hypothesize_score_sprt: hypothesize_score() with every slot verified by its problem's
        SPRT (eps_delta: A x 2 doubles, a 0 = the estimator's default) instead of scored.  Returns
        (counts A x R*spk [-1: rejected or empty], sums [(float)count], list of A best-record dicts,
        list of A statistics dicts, starts A x R*spk uint32 [0xFFFFFFFF: an empty F slot])."""
        A = self.P if problems is None else len(problems)
        pr = None if problems is None else np.ascontiguousarray(problems, dtype=np.uint32)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd is not None and sd.size != A:
            raise ValueError("seeds: one per listed problem (%d), got %d" % (A, sd.size))
        sm = None
        if samples is not None:
            sm = np.ascontiguousarray(samples, dtype=np.int32)
            if sm.size != A * R * self.m:
                raise ValueError("samples must be %d x %d x %d" % (A, R, self.m))
        ed = None
        if eps_delta is not None:
            ed = np.ascontiguousarray(eps_delta, dtype=np.float64)
            if ed.size != 2 * A:
                raise ValueError("eps_delta must be %d x 2" % A)
        c = np.zeros((A, R * self.spk), dtype=np.int32)
        s = np.zeros((A, R * self.spk), dtype=np.float32)
        st = np.zeros((A, R * self.spk), dtype=np.uint32)
        best = (Record * max(A, 1))()
        stats = (_MultiSprtStats * max(A, 1))()
        self._check(lib().usac_multi_hypothesize_score_sprt(
            self._h, _ptr(pr, ctypes.c_uint32), A, _ptr(sm, ctypes.c_int32), R, _ptr(sd, ctypes.c_uint64), first_hyp,
            ctypes.c_float(thr), int(self.dlt_mode), _ptr(ed, ctypes.c_double), _ptr(c, ctypes.c_int32),
            _ptr(s, ctypes.c_float), best, stats, _ptr(st, ctypes.c_uint32)), "multi_hypothesize_score_sprt")
        return c, s, [best[i].as_dict() for i in range(A)], [stats[i].as_dict() for i in range(A)], st

    def run_sprt(self, model_or_params, seeds=None, polish=False):
        """usac_multi_run_sprt: run() (model.sampler Uniform) or run_prosac() (Prosac) with SPRT verification
        of every slot on the device (model.sprt set, no LO), one test per problem and round.  Returns run()'s
        dicts plus "sprt" (epsilon, delta, A of the last test, tests designed, accepted, rejected,
        points_tested); with PROSAC also run_prosac()'s keys; polish=True adds "polished" and "inliers"
        as run() does."""
        return self._run("run_sprt", model_or_params, seeds, polish, own=("sprt", _MultiSprtOutput), prosac="sampler")

    def grid_neighbors(self, cell_size):
        """usac_multi_grid: Context.grid_neighbors for every problem, built in one launch and kept for
        cell_size -> a list of P dicts of the problem's CSR: cell, rank, start (n_cells + 1), members, and
        eligible (points with >= m neighbours); indices local to the problem."""
        N, P = int(self.offsets[-1]), self.P
        nc, ne = np.zeros(P, dtype=np.uint32), np.zeros(P, dtype=np.uint32)
        cell, rank = np.zeros(N, dtype=np.uint32), np.zeros(N, dtype=np.uint32)
        start = np.zeros(N + P, dtype=np.uint32)
        members, elig = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        u32, i32 = ctypes.c_uint32, ctypes.c_int32
        self._check(lib().usac_multi_grid(self._h, int(cell_size), _ptr(nc, u32), _ptr(cell, u32), _ptr(rank, u32),
                                          _ptr(start, u32), _ptr(members, i32), _ptr(elig, i32), _ptr(ne, u32)),
                    "multi_grid")
        out = []
        for p in range(P):
            a, b = int(self.offsets[p]), int(self.offsets[p + 1])
            out.append({"cell": cell[a:b].copy(), "rank": rank[a:b].copy(),
                        "start": start[a + p:a + p + int(nc[p]) + 1].copy(), "members": members[a:b].copy(),
                        "eligible": elig[a:a + int(ne[p])].copy()})
        return out

    def draw_samples_napsac(self, R, seeds, cell_size, first_hyp=0, problems=None):
        """usac_multi_draw_samples_napsac (for tests): the samples a NAPSAC round's solve kernels draw over
        the grid of cell_size, A x R x m local indices -- per problem Context.draw_samples after
        set_cell_size(cell_size) and set_device_sampler(SAMPLER.Napsac)."""
        A = self.P if problems is None else len(problems)
        pr = None if problems is None else np.ascontiguousarray(problems, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd.size != A:
            raise ValueError("seeds: one per listed problem (%d), got %d" % (A, sd.size))
        out = np.zeros((A, R, self.m), dtype=np.int32)
        self._check(lib().usac_multi_draw_samples_napsac(self._h, _ptr(pr, ctypes.c_uint32), A, R,
                                                         _ptr(sd, ctypes.c_uint64), first_hyp, int(cell_size),
                                                         _ptr(out, ctypes.c_int32)), "multi_draw_samples_napsac")
        return out

    def hypothesize_score_napsac(self, R, seeds, cell_size, first_hyp=0, thr=2.0, problems=None, per_hypothesis=True):
        """usac_multi_hypothesize_score_napsac: hypothesize_score() with the NAPSAC device sampler over the
        grid of cell_size (seeds required).  Returns what hypothesize_score() returns."""
        A = self.P if problems is None else len(problems)
        pr = None if problems is None else np.ascontiguousarray(problems, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd.size != A:
            raise ValueError("seeds: one per listed problem (%d), got %d" % (A, sd.size))
        c = np.zeros((A, R * self.spk), dtype=np.int32) if per_hypothesis else None
        s = np.zeros((A, R * self.spk), dtype=np.float32) if per_hypothesis else None
        best = (Record * max(A, 1))()
        self._check(lib().usac_multi_hypothesize_score_napsac(
            self._h, _ptr(pr, ctypes.c_uint32), A, R, _ptr(sd, ctypes.c_uint64), first_hyp, ctypes.c_float(thr),
            int(self.dlt_mode), int(cell_size), _ptr(c, ctypes.c_int32), _ptr(s, ctypes.c_float), best),
            "multi_hypothesize_score_napsac")
        return c, s, [best[i].as_dict() for i in range(A)]

    def run_napsac(self, model_or_params, seeds=None, polish=False):
        """usac_multi_run_napsac: run() with the grid NAPSAC sampler per problem (model.sampler Napsac,
        neighbours Grid, model.cell_size) and the standard termination criterion; model.lo = InItLORsc /
        InItFLORsc adds run_lo()'s LO.  Returns run()'s dicts, plus "lo" when the model asks for LO;
        polish=True adds "polished" and "inliers" as run() does."""
        p = self._run_params(model_or_params)
        return self._run("run_napsac", p, seeds, polish, own=("lo", _MultiLoOutput, p.lo != int(LocOpt.NullLO)))

    def inliers(self, models, thr):
        """Ascending inlier indices (local to each problem) of each problem's model (P x 9), by the
        residual of Context.get_inliers: a list of P int32 arrays."""
        m = np.ascontiguousarray(models, dtype=np.float32).reshape(self.P, 9)
        mask = np.zeros(int(self.offsets[-1]), dtype=np.uint8)
        cnt = np.zeros(self.P, dtype=np.int32)
        self._check(lib().usac_multi_inliers(self._h, _ptr(m, ctypes.c_float), ctypes.c_float(thr),
                                             _ptr(mask, ctypes.c_uint8), _ptr(cnt, ctypes.c_int32)), "multi_inliers")
        self.last_mask = mask
        return self._split_mask(mask)


def record_better(a, b):
    """usac_merge_records' order in Python (usac_api.cpp rec_better): a valid record beats an invalid
    one, then more inliers, then the larger Σ score (Score::bigger), then the earlier hypothesis."""
    if not a.valid:
        return False
    if not b.valid:
        return True
    if a.inliers != b.inliers:
        return a.inliers > b.inliers
    if a.score != b.score:
        return a.score > b.score
    return a.hyp_index < b.hyp_index


def merge_records(records):
    """Score::bigger over records, earliest hyp_index on exact ties."""
    arr = (Record * len(records))(*records)
    out = Record()
    rc = lib().usac_merge_records(arr, len(records), ctypes.byref(out))
    if rc:
        raise UsacError(rc, "usac_merge_records")
    return out


# --------------------------------------------------------------------------- plugin API
class Score:
    """usac/quality/quality.hpp:16-37"""

    def __init__(self, inlier_number=0, score=0.0):
        self.inlier_number = int(inlier_number)
        self.score = float(np.float32(score))

    def bigger(self, other):
        if self.inlier_number > other.inlier_number:
            return True
        if self.inlier_number == other.inlier_number:
            return self.score > other.score
        return False


class Model:
    """usac/model.hpp:15-139 (fields and setters the ported loop reads)."""

    def __init__(self, threshold, sample_number, desired_prob, knn, estimator, sampler):
        self.threshold = float(threshold)
        self.sample_size = int(sample_number)
        self.desired_prob = float(desired_prob)
        self.k_nearest_neighbors = int(knn)
        self.estimator = ESTIMATOR(estimator)
        self.sampler = SAMPLER(sampler)
        self.max_iterations = 10000
        self.min_iterations = 20
        self.reset_random_generator = True
        self.sprt = False
        self.lo = 0
        self.seed = 0
        self.dlt_mode = DLT.THIN
        self.batch = 0
        self.device = 0
        self.lo = LocOpt.NullLO
        self.lo_sample_size = 14
        self.lo_iterative_iterations = 4
        self.lo_inner_iterations = 20
        self.lo_threshold_multiplier = 10
        self.cell_size = 50
        self.neighborsType = NeighborsSearch.NullN
        self.spatial_coherence_gc = 0.1
        self.max_hypothesis_test_before_sprt = 20  # model.hpp:40

    def ResetRandomGenerator(self, reset):
        self.reset_random_generator = bool(reset)

    def setSeed(self, seed):
        """Seed of the glibc sampler stream (srandom(seed)); replaces srand(time(NULL))."""
        self.seed = int(seed)

    def setThreshold(self, thr):
        self.threshold = float(thr)

    def setDesiredProbability(self, p):
        self.desired_prob = float(p)

    def setSprt(self, sprt):
        self.sprt = bool(sprt)

    def setLOParametres(self, lo_iterative_iters, lo_inner_iters, lo_thresh_mult):
        self.lo_iterative_iterations = int(lo_iterative_iters)
        self.lo_inner_iterations = int(lo_inner_iters)
        self.lo_threshold_multiplier = int(lo_thresh_mult)

    def setCellSize(self, cell_size):
        self.cell_size = int(cell_size)

    def setNeighborsType(self, t):
        self.neighborsType = NeighborsSearch(t)

    def setDLTMode(self, mode):
        self.dlt_mode = DLT(mode)


class RansacOutput:
    """usac/ransac/ransac_output.hpp:11-99 getters."""

    def __init__(self, model, inliers, time_us, n_inliers, iters, raw, lo_iters=0):
        self._model = model
        self._inliers = inliers
        self._time = time_us
        self._n = n_inliers
        self._iters = iters
        self.raw = raw
        self._lo = lo_iters

    def getModel(self):
        return self._model

    def getInliers(self):
        return self._inliers

    def getTimeMicroSeconds(self):
        return self._time

    def getNumberOfInliers(self):
        return self._n

    def getNumberOfMainIterations(self):
        return self._iters

    def getLOIters(self):
        return self._lo


def _params(m):
    """usac_params of a Model (the fields the device loop and the plugins read)."""
    seed = m.seed
    if m.reset_random_generator and seed == 0:
        seed = int.from_bytes(os.urandom(4), "little") or 1
    return _Params(m.threshold, m.desired_prob, m.max_iterations, seed, int(m.dlt_mode), m.batch, int(m.sampler),
                   1 if m.sprt else 0, int(m.lo), m.lo_sample_size, m.lo_iterative_iterations,
                   m.lo_inner_iterations, m.lo_threshold_multiplier, m.cell_size, int(m.neighborsType),
                   m.k_nearest_neighbors, m.spatial_coherence_gc, m.max_hypothesis_test_before_sprt)


# usac_allgather_fn (include/usac_gpu.h)
_ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class Ransac:
    """usac/ransac/ransac.hpp:41-115 -- Ransac(model, points); run(); getRansacOutput()."""

    def __init__(self, model, points, ctx=None):
        """ctx: an existing Context over the same points to run on (e.g. the one holding the RCCL
        communicator of a sharded run); by default a new one."""
        if model.sampler not in (SAMPLER.Uniform, SAMPLER.Prosac, SAMPLER.Napsac):
            raise NotImplementedError("sampler %s is not supported (Uniform, Napsac, Prosac)" % model.sampler.name)
        if int(model.lo) not in (0, 1, 2, 3):
            raise NotImplementedError("LO %r is not supported (InItLORsc, InItFLORsc, GC)" % model.lo)
        self.model = model
        self.ctx = ctx if ctx is not None else Context(model.estimator, points, device=model.device)
        self._out = None
        self.records = []

    def run(self, rec_cap=4096, shard=None):
        """shard = (nranks, rank, gather): hypothesis-sharded batches (usac_ransac_run_sharded);
        gather(bytes) -> list of nranks bytes objects in rank order (e.g. a gloo all_gather), or
        gather = "rccl" for the communicator set up with Context.comm_init."""
        L = lib()
        p = _params(self.model)
        out = _RunOutput()
        inl = np.empty(self.ctx.n, dtype=np.int32)
        # the record array is the run's largest host allocation (rec_cap x 56 B, zero-filled): one
        # per Context and capacity, reused (the records are copied out below)
        cache = self.ctx.__dict__.setdefault("_rec_bufs", {})
        recs = cache.get(rec_cap)
        if recs is None:
            recs = cache[rec_cap] = (Record * rec_cap)()
        if shard is None:
            rc = L.usac_ransac_run(self.ctx._h, ctypes.byref(p), ctypes.byref(out), _ptr(inl, ctypes.c_int32), recs,
                                   rec_cap)
        else:
            nranks, rank, gather = shard
            cb = None
            if gather != "rccl":
                def _cb(user, send, nbytes, recv):
                    try:
                        parts = gather(ctypes.string_at(send, nbytes))
                        buf = b"".join(parts)
                        if len(parts) != nranks or len(buf) != nranks * nbytes:
                            return -1
                        ctypes.memmove(recv, buf, len(buf))
                        return 0
                    except Exception:  # reported as a failed all-gather (usac_last_error)
                        return -1
                cb = _ALLGATHER_FN(_cb)
            rc = L.usac_ransac_run_sharded(self.ctx._h, ctypes.byref(p), int(nranks), int(rank),
                                           ctypes.cast(cb, _vp) if cb is not None else None, None,
                                           ctypes.byref(out), _ptr(inl, ctypes.c_int32), recs, rec_cap)
        if rc == -111:
            raise UsacError(rc, "best score is 0 (ransac.cpp:143-147)")
        self.ctx._check(rc, "ransac_run")
        k = min(out.n_records, rec_cap)
        self.records = [(int(recs[i].hyp_index), int(recs[i].inliers), float(recs[i].score)) for i in range(k)]
        raw = {"minimal_model": np.array(out.minimal_model[:], dtype=np.float32),
               "minimal_inliers": out.minimal_inliers, "polish_passes": out.polish_passes,
               "n_records": out.n_records, "batches": out.batches, "sprt_rejected": out.sprt_rejected,
               "sprt_histories": out.sprt_histories, "prosac_term_len": out.prosac_term_len,
               "rollbacks": out.rollbacks, "lo_iterative_iters": out.lo_iterative_iters,
               "lo_rounds": out.lo_rounds, "lo_stages": out.lo_stages, "sum_models": out.sum_models,
               "lo_fits": out.lo_fits, "spec_batches": out.spec_batches, "spec_rollbacks": out.spec_rollbacks,
               "spec_wasted": out.spec_wasted}
        self._out = RansacOutput(np.array(out.model[:], dtype=np.float32), inl[: out.inliers].copy(), out.time_us,
                                 out.inliers, out.iters, raw, out.lo_inner_iters)

    def getRansacOutput(self):
        return self._out


# --------------------------------------------------------------------------- stateful plugins
# The reference's per-call plugin surface (include/usac_gpu.h, ABI 11): a caller that keeps its own
# Ransac::run loop (ransac.cpp:58-139) swaps plugin by plugin.  Every handle created on a Context
# must be closed before it (close(), or garbage collection in creation-reverse order).
class _Handle:
    _destroy = None

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            getattr(lib(), self._destroy)(h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class RandomGenerator(_Handle):
    """The reference's global glibc random() stream after srandom(seed) (usac_random)."""
    _destroy = "usac_random_destroy"

    def __init__(self, seed):
        h = _vp()
        rc = lib().usac_random_create(int(seed), ctypes.byref(h))
        if rc:
            raise UsacError(rc, "usac_random_create")
        self._h = h

    def next(self):
        return int(lib().usac_random_next(self._h))


class Sampler(_Handle):
    """Sampler::generateSample (sampler.hpp:11-35) as initSampler builds it for model.sampler: Uniform
    (persistent pool on rng), Prosac (own mt19937 seeded with model.seed), Napsac (grid or KNN
    neighbours built on the device, on rng)."""
    _destroy = "usac_sampler_destroy"

    def __init__(self, ctx, model, rng=None):
        h = _vp()
        self.ctx, self.rng = ctx, rng  # kept alive while the handle draws from them
        self._p = _params(model)
        ctx._check(lib().usac_sampler_create(ctx._h, ctypes.byref(self._p), rng._h if rng is not None else None,
                                             ctypes.byref(h)), "sampler_create")
        self._h = h
        self.m = ctx.m
        self._sample = np.zeros(self.m, dtype=np.int32)  # the loop's reused `int sample[m]`

    def generateSample(self):
        self.ctx._check(lib().usac_sampler_generate(self._h, _ptr(self._sample, ctypes.c_int32)), "generateSample")
        return self._sample.copy()

    def generateSamples(self, count):
        out = np.zeros((int(count), self.m), dtype=np.int32)
        self.ctx._check(lib().usac_sampler_generate_batch(self._h, int(count), _ptr(out, ctypes.c_int32)),
                        "generateSamples")
        return out

    def state(self):
        d, sub, lg = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self.ctx._check(lib().usac_sampler_state(self._h, ctypes.byref(d), ctypes.byref(sub), ctypes.byref(lg)),
                        "sampler_state")
        return {"drawn": int(d.value), "subset_size": int(sub.value), "largest_sample_size": int(lg.value)}


class TerminationCriteria(_Handle):
    """StandardTerminationCriteria, or ProsacTerminationCriteria when built on a Prosac Sampler
    (linked both ways as in the reference)."""
    _destroy = "usac_termination_destroy"

    def __init__(self, ctx, model, prosac_sampler=None):
        h = _vp()
        self.ctx, self.sampler = ctx, prosac_sampler
        self._p = _params(model)
        ctx._check(lib().usac_termination_create(ctx._h, ctypes.byref(self._p),
                                                 prosac_sampler._h if prosac_sampler is not None else None,
                                                 ctypes.byref(h)), "termination_create")
        self._h = h
        self.termination_length = ctx.n

    def getUpBoundIterations(self, a, b=None):
        """(inlier_size[, points_size]) -> standard bound; (hypCount, model array) -> PROSAC's
        getUpBoundIterations(hypCount, model) (prosac_termination_criteria.hpp:148-201)."""
        if b is None or np.ndim(b) == 0:
            return int(lib().usac_termination_bound(self._h, int(a), int(b or 0)))
        m = np.zeros(9, dtype=np.float32)
        mm = np.asarray(b, dtype=np.float32).reshape(-1)
        m[: mm.size] = mm
        mi, tl = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self.ctx._check(lib().usac_prosac_termination(self._h, int(a), _ptr(m, ctypes.c_float), ctypes.byref(mi),
                                                      ctypes.byref(tl)), "prosac_termination")
        self.termination_length = int(tl.value)
        return int(mi.value)


class SPRT(_Handle):
    """SPRT (sprt.hpp:89-491): pool shuffled from rng at construction, verifyModelAndGetModelScore,
    getUpperBoundIterations, and the batch replay of the loop body (usac_sprt_replay)."""
    _destroy = "usac_sprt_destroy"

    def __init__(self, ctx, model, rng):
        h = _vp()
        self.ctx, self.rng = ctx, rng
        self._p = _params(model)
        ctx._check(lib().usac_sprt_create(ctx._h, ctypes.byref(self._p), rng._h, ctypes.byref(h)), "sprt_create")
        self._h = h

    def verifyModelAndGetModelScore(self, model, current_hypothese, maximum_score, score):
        m = np.zeros(9, dtype=np.float32)
        mm = np.asarray(model, dtype=np.float32).reshape(-1)
        m[: mm.size] = mm
        good = ctypes.c_int32(0)
        cnt = ctypes.c_int32(score.inlier_number)
        sc = ctypes.c_float(score.score)
        self.ctx._check(lib().usac_sprt_verify(self._h, _ptr(m, ctypes.c_float), int(current_hypothese),
                                               int(maximum_score), ctypes.byref(good), ctypes.byref(cnt),
                                               ctypes.byref(sc)), "sprt_verify")
        score.inlier_number, score.score = int(cnt.value), float(sc.value)
        return bool(good.value)

    def getUpperBoundIterations(self, inlier_size):
        return int(lib().usac_sprt_upper_bound(self._h, int(inlier_size)))

    def stats(self):
        h, r = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self.ctx._check(lib().usac_sprt_stats(self._h, ctypes.byref(h), ctypes.byref(r)), "sprt_stats")
        return {"histories": int(h.value), "rejected": int(r.value)}

    def replay(self, models, n_models, state):
        """usac_sprt_replay over a batch (models B x slots x 9, n_models[B]); `state` a SprtState,
        updated in place; returns state.found."""
        m = np.ascontiguousarray(models, dtype=np.float32)
        nm = np.ascontiguousarray(n_models, dtype=np.int32)
        self.ctx._check(lib().usac_sprt_replay(self._h, _ptr(m, ctypes.c_float), _ptr(nm, ctypes.c_int32), len(nm),
                                               ctypes.byref(state)), "sprt_replay")
        return bool(state.found)


class LocalOptimization(_Handle):
    """LocalOptimization::GetModelScore (local_optimization.hpp:19) as initLocalOptimization builds it
    for model.lo: InItLORsc / InItFLORsc (inner + iterative LO-RANSAC) or GC (graph cut)."""
    _destroy = "usac_lo_destroy"

    def __init__(self, ctx, model):
        h = _vp()
        self.ctx = ctx
        self._p = _params(model)
        ctx._check(lib().usac_lo_create(ctx._h, ctypes.byref(self._p), ctypes.byref(h)), "lo_create")
        self._h = h

    def GetModelScore(self, best_model, best_score):
        """best_model: float32 array of 9 (line: 3) improved in place; best_score: a Score."""
        m = np.zeros(9, dtype=np.float32)
        m[: best_model.size] = best_model.reshape(-1)
        cnt = ctypes.c_int32(best_score.inlier_number)
        sc = ctypes.c_float(best_score.score)
        self.ctx._check(lib().usac_lo_get_model_score(self._h, _ptr(m, ctypes.c_float), ctypes.byref(cnt),
                                                      ctypes.byref(sc)), "lo_get_model_score")
        best_model.reshape(-1)[:] = m[: best_model.size]
        best_score.inlier_number, best_score.score = int(cnt.value), float(sc.value)

    def iters(self):
        a, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self.ctx._check(lib().usac_lo_iters(self._h, ctypes.byref(a), ctypes.byref(b)), "lo_iters")
        return int(a.value), int(b.value)
