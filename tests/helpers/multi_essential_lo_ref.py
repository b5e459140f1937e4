"""The inputs of the essential LO tests (usac_multi_lo_essential, usac_multi_run_lo_essential; ABI 23): the
point sets in calibrated coordinates, their start records and the degenerate and capped problems.  The
yardstick itself is tests/helpers/multi_lo_ref.py's lo_ref, as it is, over oracle.Estimator(ESSENTIAL):
sample size 5, the 8-point non-minimal fit, the squared Sampson distance.  Everything here runs on the CPU."""
import numpy as np

from ransac_amd import synthetic
from tests.helpers import multi_lo_ref as ref

THR = 0.002
M = 5
# multi_lo_ref's sizes: 11 is below the LO floor, 13 and 14 are fit-all at the default sample size 14, 15 is
# the first sampled size; problem 7 is a copy of problem 5 (the 333-point set) with its seeds
SIZES, RATIOS, DUP = ref.SIZES, ref.RATIOS, ref.DUP
DATA_SEEDS = [70, 71, 72, 73, 74, 75, 76]
START_SEED, START_COUNT = 170, 64
DRAW_SEEDS = ref.DRAW_SEEDS
CAP_N, CAP_SEED, CAP_START = 4200, 77, 177  # n > kPolFitMax, all of one motion
# the run tests' problems as (n, inlier ratio, data seed), quality-sorted (PROSAC runs on them too), every
# n_p > 20; the last one is poor in inliers: with the tests' seeds its record improves in more than one
# round under the uniform sampler (measured on the device; the tests assert it).  Under PROSAC every run
# over quality-sorted sets ends in its first round, so PROSAC's rounds with LO are tested on UNSORTED: the
# poor problem in generation order, where PROSAC starts no better than the uniform sampler
RUN_SETS = [(64, 0.8, 74), (333, 0.5, 75), (1000, 0.4, 76), (333, 0.3, 86)]
UNSORTED = (333, 0.35, 80)


def make_set(n, ratio, seed, prosac_order=False):
    return synthetic.fundamental_points(n=n, inlier_ratio=ratio, seed=seed, noise=0.5, normalized=True,
                                        prosac_order=prosac_order)[0]


def sets():
    out = [make_set(n, r, s) for n, r, s in zip(SIZES, RATIOS, DATA_SEEDS)]
    out.append(out[DUP[1]].copy())
    return out


def run_sets():
    return [make_set(n, r, s, prosac_order=True) for n, r, s in RUN_SETS]


def estimator(oracle, pts):
    return oracle.Estimator(oracle.ESSENTIAL, pts)


def make_model(usac, limited=False, sampler=None, thr=THR, iters=4, inner=10, sample_size=14):
    """multi_lo_ref.make_model for the essential estimator: LoParams' defaults"""
    model = usac.Model(thr, M, 0.95, 5, usac.ESTIMATOR.Essential, sampler or usac.SAMPLER.Uniform)
    model.lo = usac.LocOpt.InItFLORsc if limited else usac.LocOpt.InItLORsc
    model.lo_sample_size = sample_size
    model.setLOParametres(iters, inner, 10)
    model.seed = 100
    return model


def start_record(oracle, pts, seed, est=None, thr=THR, hyp_index=5, count=START_COUNT):
    """The best minimal model of `count` oracle samples by count, then Σ, then the earlier index, as a
    record dict with its own count and Σ at thr; not valid when no sample gives a model."""
    est = est or estimator(oracle, pts)
    models, nm = est.estimate_batch(oracle.uniform_samples(seed, len(pts), M, count))
    c, s = est.score_models(models, thr)
    have = [i for i in range(len(nm)) if nm[i]]
    if not have:
        return {"hyp_index": hyp_index, "inliers": 0, "score": np.float32(0), "model": np.zeros(9, np.float32), "valid": False}
    best = min(have, key=lambda i: (-int(c[i]), -float(s[i]), i))
    model = np.asarray(models[best], np.float32).copy()
    cnt, sm = est.quality(model, thr)
    return {"hyp_index": hyp_index, "inliers": int(cnt), "score": np.float32(sm), "model": model, "valid": True}


def hook_problems(oracle, thr=THR):
    """(point sets, oracle estimators, start records, draw seeds) of the hook tests: sets() with the copy
    starting where its original does"""
    pts = sets()
    ests = [estimator(oracle, p) for p in pts]
    recs = [start_record(oracle, p, START_SEED + i, est=e, thr=thr) for i, (p, e) in enumerate(zip(pts, ests))]
    recs[DUP[0]] = dict(recs[DUP[1]])
    return pts, ests, recs, list(DRAW_SEEDS)


def cap_problem(oracle):
    """(points, start record): 4200 correspondences of one motion, 3914 of them inliers of the start model at
    θ; the first inner fit's list at 10 θ, the iterative stage's first list to fit, is past kPolFitMax"""
    pts = make_set(CAP_N, 1.0, CAP_SEED)
    return pts, start_record(oracle, pts, CAP_START, hyp_index=3)


def few_problem(oracle):
    """(points, start record): 16 copies of one correspondence among 24 random ones, the start model ([t]x of
    the translation (5, 3, 0)) exact on the copies.  An LO sample of 14 identical points fits a model with
    no more than 5 inliers: the `<= m` continue, which leaves the threshold multiplied."""
    rng = np.random.default_rng(5)
    x1, x2 = rng.uniform(-0.5, 0.5, size=(40, 2)), rng.uniform(-0.5, 0.5, size=(40, 2))
    x1[:16], x2[:16] = [0.1, 0.2], [0.105, 0.203]
    pts = np.concatenate([x1, x2], 1).astype(np.float32)
    model = (np.array([0, 0, 3, 0, 0, -5, -3, 5, 0]) / 5.0).astype(np.float32)
    c, s = estimator(oracle, pts).quality(model, THR)
    return pts, {"hyp_index": 1, "inliers": int(c), "score": np.float32(s), "model": model, "valid": True}


def ref_calls(usac, ests, recs, seeds, prm, calls):
    """`calls` LO calls in a row per problem on the restatement: per call the list of (record, state, tally)"""
    out = []
    cur = [(dict(r), ref.fresh_state(prm), None) for r in recs]
    for _ in range(calls):
        cur = [ref.lo_ref(usac, e, r, st, sd, prm) for e, (r, st, _), sd in zip(ests, cur, seeds)]
        out.append(cur)
    return out
