"""The yardstick of the multi-problem LO tests: the control flow of k_multi_lo -- InnerLocalOptimization::
GetModelScore (inner_local_optimization.hpp:74-133) with GetScoreUnlimited / GetScoreLimited
(iterative_local_optimization.hpp:61-136), the caps rule included -- restated over the CPU oracle's
quality / nonminimal, with the sample sets of usac.lo_draw.  Everything here runs on the CPU."""
import numpy as np

from tests.helpers import multi_polish_ref as pref

THR = pref.THR
FIT_MAX, PTS_MAX = 4096, 16384  # kPolFitMax, kPolPtsMax
COUNTERS = ("lo_calls", "inner_iters", "iterative_iters", "fits", "improved", "capped", "draws")
# the hook tests' problems: 11 is below the LO floor, 13 and 14 are fit-all at the default sample size
# 14, 15 is the first sampled size; problem 8 is a copy of problem 5 (the 333-point set)
SIZES = [11, 13, 14, 15, 64, 333, 1000]
DUP = (7, 5)
DATA_SEEDS = {"H": [50, 51, 52, 53, 54, 55, 56], "F": [60, 61, 62, 63, 64, 65, 66]}
RATIOS = [1.0, 1.0, 1.0, 1.0, 0.8, 0.5, 0.4]
START_SEED, START_COUNT = 70, 64
DRAW_SEEDS = [901, 902, 903, 904, 905, 906, 907, 906]


class LoParams:
    """the LO fields of usac_params, and the fp32 threshold step of LoRansac (usac_api.cpp)"""

    def __init__(self, thr=THR, limited=False, sample_size=14, inner=10, iters=4, mult=10, m=4):
        self.thr, self.limited, self.limit, self.inner, self.iters, self.m = np.float32(thr), limited, sample_size, inner, iters, m
        self.mult = np.float32(mult)
        self.step = np.float32((self.thr * self.mult - self.thr) / np.float32(iters))


def from_model(model, m):
    from ransac_amd import LocOpt
    return LoParams(model.threshold, model.lo == LocOpt.InItFLORsc, model.lo_sample_size, model.lo_inner_iterations,
                    model.lo_iterative_iterations, model.lo_threshold_multiplier, m)


def make_model(usac, kind, limited=False, sampler=None, thr=THR, iters=4, inner=10, sample_size=14):
    """the tests' Model: LoParams' defaults"""
    est = usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental
    model = usac.Model(thr, 4 if kind == "H" else 7, 0.95, 5, est, sampler or usac.SAMPLER.Uniform)
    model.lo = usac.LocOpt.InItFLORsc if limited else usac.LocOpt.InItLORsc
    model.lo_sample_size = sample_size
    model.setLOParametres(iters, inner, 10)
    model.seed = 100
    return model


# the run tests' problems as (n, inlier ratio, data seed), every n_p > 20 (PROSAC runs on them too).  The
# last one of each kind is poor in inliers: with the tests' seeds its record improves in more than one
# round under both samplers (measured on the device; the tests assert it)
RUN_SETS = {"H": [(64, 0.8, 54), (333, 0.5, 55), (1000, 0.4, 56), (333, 0.35, 58)],
            "F": [(64, 0.8, 64), (333, 0.5, 65), (1000, 0.4, 66), (1000, 0.35, 59)]}


def run_sets(kind):
    return [pref.make_set(kind, n, r, s) for n, r, s in RUN_SETS[kind]]


def fresh_state(prm):
    st = {k: 0 for k in COUNTERS}
    st["threshold"] = np.float32(prm.thr)
    return st


def bigger(c1, s1, c2, s2):
    """Score::bigger: count, then Σ"""
    return c1 > c2 or (c1 == c2 and s1 > s2)


def sets(kind):
    out = [pref.make_set(kind, n, r, s) for n, r, s in zip(SIZES, RATIOS, DATA_SEEDS[kind])]
    out.append(out[DUP[1]].copy())
    return out


CAP_N = 4200  # > kPolFitMax


def cap_problem(oracle):
    """(points, start record): 4200 correspondences of one homography with 0.3 px noise, all of them inliers
    of the start model (that homography), so the iterative stage's first list to fit is past kPolFitMax"""
    rng = np.random.default_rng(77)
    x1 = rng.uniform(0, 1000, size=(CAP_N, 2))
    H = np.array([[0.98, 0.03, 12.0], [-0.02, 1.01, -7.0], [1e-5, -2e-5, 1.0]])
    q = np.concatenate([x1, np.ones((CAP_N, 1))], 1) @ H.T
    x2 = q[:, :2] / q[:, 2:] + rng.normal(0, 0.3, size=(CAP_N, 2))
    pts = np.concatenate([x1, x2], 1).astype(np.float32)
    model = (H / H[2, 2]).astype(np.float32).reshape(9)
    c, s = pref.estimator(oracle, "H", pts).quality(model, THR)
    return pts, {"hyp_index": 3, "inliers": int(c), "score": np.float32(s), "model": model, "valid": True}


def few_problem(oracle, kind):
    """(points, start record): 16 copies of one correspondence among 24 random ones, the start model exact
    on the copies.  Every LO sample is 14 identical points, whose fit is all NaN and has no inlier: the
    `<= sample_size` continue, ten times, each leaving the threshold multiplied."""
    rng = np.random.default_rng(3 if kind == "H" else 4)
    x1, x2 = rng.uniform(0, 1000, size=(40, 2)), rng.uniform(0, 1000, size=(40, 2))
    x1[:16], x2[:16] = [100, 200], [105, 203]
    pts = np.concatenate([x1, x2], 1).astype(np.float32)
    if kind == "H":
        model = np.array([1, 0, 5, 0, 1, 3, 0, 0, 1], np.float32)
    else:  # [t]x of the translation (5, 3, 0), scaled as the fits scale theirs
        model = (np.array([0, 0, 3, 0, 0, -5, -3, 5, 0]) / 5.0).astype(np.float32)
    c, s = pref.estimator(oracle, kind, pts).quality(model, THR)
    return pts, {"hyp_index": 1, "inliers": int(c), "score": np.float32(s), "model": model, "valid": True}


def start_record(oracle, kind, pts, seed, count=START_COUNT, est=None, hyp_index=5, thr=THR):
    """multi_polish_ref.start_model as a record dict: its own count and Σ at thr"""
    est = est or pref.estimator(oracle, kind, pts)
    model = pref.start_model(oracle, kind, pts, seed, count, est)
    c, s = est.quality(model, thr)
    return {"hyp_index": hyp_index, "inliers": int(c), "score": np.float32(s), "model": model, "valid": bool(model.any())}


def lo_ref(usac, est, rec, st, seed, prm, fit_max=FIT_MAX, pts_max=PTS_MAX, force=True, first_hyp=0):
    """One LO call on record dict `rec` with state `st` (both left alone).  Returns (record, state,
    tally): tally counts the branches taken."""
    rec = dict(rec, model=np.asarray(rec["model"], np.float32).copy(), score=np.float32(rec["score"]))
    st = dict(st)
    tally = {k: 0 for k in ("skipped", "below12", "fit_all", "sampled", "fit_failed", "few", "stage_done", "stage_break",
                            "stage_draw", "improved", "capped")}
    if not rec["valid"] or not (force or rec["hyp_index"] >= first_hyp):
        tally["skipped"] += 1
        return rec, st, tally
    st["lo_calls"] += 1
    if rec["inliers"] < 12:
        tally["below12"] += 1
        return rec, st, tally
    thr = np.float32(st["threshold"])
    theta = prm.thr

    def capped():
        st["capped"] += 1
        st["threshold"] = theta
        tally["capped"] += 1
        return rec, st, tally

    def draw(lst):
        d = usac.lo_draw(seed, st["draws"], prm.limit, len(lst) - 1)
        st["draws"] += 1
        return lst[d]

    def fit(idx):
        st["fits"] += 1
        return est.nonminimal(idx)

    if est.n > pts_max:
        return capped()
    best_cnt, best_sum = rec["inliers"], np.float32(rec["score"])
    _, _, max_inl = est.quality(rec["model"], float(theta), with_inliers=True)
    for _ in range(prm.inner):
        if len(max_inl) > prm.limit:
            tally["sampled"] += 1
            lo_model = fit(draw(max_inl))
            if lo_model is None:
                tally["fit_failed"] += 1
                continue
        else:
            tally["fit_all"] += 1
            lo_model = fit(max_inl)
            if lo_model is None:
                tally["fit_failed"] += 1
                break
        thr = np.float32(prm.mult * thr)
        lo_cnt, lo_sum, lo_inl = est.quality(lo_model, float(thr), with_inliers=True)
        lo_sum = np.float32(lo_sum)
        if lo_cnt <= prm.m:
            tally["few"] += 1
            continue
        broke = False
        k = 0
        while k < prm.iters:
            thr = np.float32(thr - prm.step)
            if lo_cnt <= prm.m:
                break
            if prm.limited and lo_cnt > prm.limit:
                tally["stage_draw"] += 1
                nm = fit(draw(lo_inl))
                if nm is None:
                    tally["fit_failed"] += 1
                    k += 1
                    continue
            else:
                if lo_cnt > fit_max:
                    return capped()
                nm = fit(lo_inl)
                if nm is None:
                    tally["fit_failed"] += 1
                    break
            lo_model = nm
            lo_cnt, lo_sum, lo_inl = est.quality(lo_model, float(thr), with_inliers=True)
            lo_sum = np.float32(lo_sum)
            if not prm.limited and bigger(best_cnt, best_sum, lo_cnt, lo_sum):
                broke = True
                break
            st["iterative_iters"] += 1
            k += 1
        fail = float(np.abs(np.float32(thr - theta))) > 0.00001
        if fail:
            thr = theta
        tally["stage_break" if broke else "stage_done"] += 1
        if not fail and bigger(lo_cnt, lo_sum, best_cnt, best_sum):
            best_cnt, best_sum, max_inl = lo_cnt, lo_sum, lo_inl
            rec["model"], rec["inliers"], rec["score"] = np.asarray(lo_model, np.float32), int(lo_cnt), lo_sum
            st["improved"] += 1
            tally["improved"] += 1
        st["inner_iters"] += 1
    st["threshold"] = np.float32(thr)
    return rec, st, tally


def assert_same_record(got, want, what=""):
    for key in ("hyp_index", "inliers", "valid"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert pref.bits(got["score"]) == pref.bits(want["score"]), (what, got["score"], want["score"])
    np.testing.assert_array_equal(pref.bits(got["model"]), pref.bits(want["model"]), err_msg=str(what))


def assert_same_state(got, want, what=""):
    for key in COUNTERS:
        assert got[key] == want[key], (what, key, got, want)
    assert pref.bits(got["threshold"]) == pref.bits(want["threshold"]), (what, got["threshold"], want["threshold"])
