#!/usr/bin/env python
"""Multi-problem batches against a loop over single contexts, same box, same process, same inputs.

  python tools/bench_multi.py --pairs 512 --points 1000 --round 256 --estimator homography

--estimator essential takes calibrated pairs (synthetic.fundamental_points(normalized=True), threshold
0.002) through MultiContext.essential; (b) is then the loop over Context(Essential) objects.  It offers
the plain run, --polish, --sampler prosac and --lo (through MultiContext.run_lo_essential); no --sprt and
no --sampler napsac.

(a) MultiContext.run: batch-granular RANSAC over all pairs, one launch chain per round.
(b) the same schedule -- per pair, rounds of R hypotheses until min(max_iterations, standard bound)
    is reached -- as a loop over one Context per pair with hypothesize_score(per_hypothesis=False),
    the fastest existing way.  The contexts are created outside the timed window.

Both are warmed up, then alternated for --reps repetitions each; a repetition is timed with a host
clock around work that ends in a device synchronise (both calls return after their last copy).
The per-pair best inlier counts of (a) and (b) must agree.  Prints one JSON line (and writes it to
--out): median and spread (max - min) of each, and the ratio of the medians.  The baseline is (b)
in the same job, never (a) itself; (a) counts as faster only beyond the larger of the two spreads.

--polish times the run with its non-minimal polish instead: MultiContext.run(polish=True), the multi
run alone (what the polish adds), and loop (b) followed per pair by the polish restated with
get_inliers + nonminimal.  The per-pair minimal and polished inlier counts must agree.

--sampler prosac compares the two multi runs instead: every pair's points are sorted by the PROSAC
quality of synthetic.fundamental_points(prosac_order=True) (the homography sets too), and
MultiContext.run_prosac is alternated with MultiContext.run (uniform sampler) on those same inputs;
with --polish both runs include the polish.  Reported for both: median ms and spread, rounds per pair,
the rounds of the longest pair (= the launch chains of the run) and ms per such round, total
hypotheses, mean best (and polished) inlier counts.  No loop over single contexts in this mode.

--lo lorsc|florsc compares the LO run with the run without it: MultiContext.run_lo (inner + iterative
LO-RANSAC of every round's new bests on the device) is alternated with MultiContext.run -- or, with
--sampler prosac, with MultiContext.run_prosac -- on the same inputs; with --polish both include the
polish.  Reported for both: the --sampler prosac mode's figures; for the LO run also the mean LO calls,
fits, improvements and capped calls per pair.  No loop over single contexts in this mode.

--sprt compares the SPRT run with the run without it: MultiContext.run_sprt is alternated with
MultiContext.run -- or, with --sampler prosac, with MultiContext.run_prosac -- on the same inputs; with
--polish both include the polish.  Reported for both: rounds, hypotheses, mean best inliers; for the SPRT
run also the point tests done over slots x n_p, the tests designed per pair and the accepted / rejected
slots; and, separately, the one-time cost of set_sprt_pool, which is not part of a run.

--sampler napsac [--cell-size N] [--cluster HW] compares the NAPSAC run with the uniform run:
MultiContext.run_napsac (grid NAPSAC per pair over the cells of size N) is alternated with MultiContext.run
on the same pairs; with --lo both runs include LO (run_napsac with the LO model against run_lo), with
--polish both include the polish.  --cluster HW draws the homography pairs from
synthetic.homography_points(..., cluster=(500, 500, HW)): the inliers sit in a box of half-width HW of
the first image, so that cells hold inliers.  Reported for both: median ms and spread, rounds per pair,
hypotheses, mean best inliers; for the NAPSAC run also the share of pairs without an eligible point
(they draw uniform samples) and the mean eligible share; and, apart from the runs, the grid build of all
pairs (usac_multi_grid with no output, after a build for another size), which a run pays once per cell
size.  No loop over single contexts in this mode.

--per-problem-thr compares the run with per-problem thresholds (MultiContext.set_thresholds, all P of them
equal to the scalar) with the same run without them: the plain run, or with --lo / --sprt / --sampler
prosac|napsac / --polish the run those flags select, alternated on the same context (the thresholds are
set and cleared outside the timed window).  The two results must be equal bit for bit (exit status 1
otherwise); the difference of the two medians is the cost of the indexed path.  No loop over single
contexts in this mode.

--estimator essential --pixels times the creation of an essential multi context from pixel coordinates: the
pairs are pixel correspondences under per-pair intrinsics whose focal lengths differ, and
MultiContext.essential_pixels + set_pixel_thresholds (upload, the conversion kernel, the read-back of the rows
into `points`) is alternated with the caller's path without them -- a float32 numpy conversion of every set
by the same formulas, MultiContext.essential, set_thresholds with (t_px / f)^2 computed per pair.  Reported
for both: min / median / max ms over the repetitions, the numpy conversion's share of the second, and the C
entry alone (usac_multi_create_essential_pixels + usac_multi_destroy, no read-back).  The two contexts'
run(polish=True) results must be equal bit for bit (exit status 1 otherwise).  The contexts are closed
outside the timed windows.

--device-input goes from padded torch device tensors to the polished inliers as a (pairs, n_max) bool device
tensor: the host round trip against MultiContext.from_padded + run(polish=True) + padded_mask.  With --scores the
input is a matcher's: the quality-sorted pairs of --sampler prosac with their columns permuted and a score per
column that falls with the original rank.  Three pipelines are alternated: from_padded(scores=...) + run_prosac +
padded_mask; from_padded + run + padded_mask; and torch.sort(stable=True) + gather + from_padded + run_prosac +
padded_mask + the inverse permutation of the mask.  The first and the third must return equal masks and models
(exit status 1 otherwise); the creation with and without scores is also timed alone.

--device-output (with --device-input, with or without --scores) times the way out instead: creation, the polished
run (run, or run_prosac with --scores), padded_mask() and an upload of the polished models as a (pairs, 3, 3) tensor
against creation, keep_on_device = True, the same run and export_device(inlier_cols=n_max), alternated; then
export_device alone against padded_mask() alone on one context.  The two masks and the two model tensors must be
equal (exit status 1 otherwise).

--pose (with --estimator essential --device-input --device-output) goes one step further, to a pose per pair: both
pipelines create their context from padded pixel rows with from_padded(K1=K), set keep_on_device, run(polish=True) and
export_device(); one adds export_pose(front_mask=True), the other brings models and mask to the host, decomposes and
votes per pair in numpy and uploads R, t and the front mask.  Alternated; export_pose is also timed alone.  On every
pair whose host vote has a unique winner the two rotations must agree (exit status 1 otherwise); the share of such
pairs is reported.

--refine (with --pose) measures the pose refinement behind that: the pipeline ending in export_pose(front_mask=True)
against the same pipeline plus refine_pose(R, t, front_mask), alternated in one process; refine_pose is also timed
alone.  The median rotation and translation-direction errors of both poses against the pose the pairs were
generated with are reported.  There is no threshold; exit status 1 only if a cost rose.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ransac_amd as usac  # noqa: E402
from ransac_amd import synthetic  # noqa: E402


def make_pairs(estimator, pairs, points, ratio, quality_sorted=False, cluster=None):
    if estimator == "essential":  # calibrated coordinates (K^-1 x), cfg4's generator
        return [synthetic.fundamental_points(n=points, inlier_ratio=ratio, seed=1000 + p, prosac_order=quality_sorted,
                                             normalized=True)[0] for p in range(pairs)]
    if cluster is not None:
        return [synthetic.homography_points(n=points, inlier_ratio=ratio, seed=1000 + p, cluster=(500, 500, cluster))[0]
                for p in range(pairs)]
    if quality_sorted:
        if estimator == "homography":
            sets = []
            for p in range(pairs):
                pts, _, inl = synthetic.homography_points(n=points, inlier_ratio=ratio, seed=1000 + p)
                sets.append(synthetic.quality_sort(pts, inl, 5000 + p)[0])
            return sets
        return [synthetic.fundamental_points(n=points, inlier_ratio=ratio, seed=1000 + p, prosac_order=True)[0]
                for p in range(pairs)]
    if estimator == "homography":
        return [synthetic.homography_points(n=points, inlier_ratio=ratio, seed=1000 + p)[0] for p in range(pairs)]
    return [synthetic.fundamental_points(n=points, inlier_ratio=ratio, seed=1000 + p, prosac_order=False)[0]
            for p in range(pairs)]


def loop_run(ctxs, m, seeds, R, thr, prob, max_iters):
    """method (b): usac_multi_run's schedule, one pair at a time"""
    best = []
    for ctx, seed in zip(ctxs, seeds):
        inl, r = 0, 0
        while True:
            rec = ctx.hypothesize_score(B=R, seed=seed, first_hyp=r * R, thr=thr, per_hypothesis=False)[2]
            if rec["valid"] and rec["inliers"] > inl:
                inl = rec["inliers"]
            r += 1
            if r * R >= min(max_iters, usac.std_termination(inl, ctx.n, m, prob, max_iters)):
                break
        best.append((inl, r))
    return best


def loop_run_polished(ctxs, m, seeds, R, thr, prob, max_iters):
    """method (b) with --polish: the schedule of loop_run keeping each pair's best record
    (usac_merge_records' order), then the polish of ransac.cpp:157-214 restated per context with
    get_inliers + nonminimal -- the only way to polish a batch of pairs without usac_multi_polish"""
    out = []
    for ctx, seed in zip(ctxs, seeds):
        best, r = None, 0
        while True:
            rec = ctx.hypothesize_score(B=R, seed=seed, first_hyp=r * R, thr=thr, per_hypothesis=False)[2]
            if rec["valid"] and (best is None or (rec["inliers"], rec["score"]) > (best["inliers"], best["score"])):
                best = rec
            r += 1
            inl = best["inliers"] if best else 0
            if r * R >= min(max_iters, usac.std_termination(inl, ctx.n, m, prob, max_iters)):
                break
        polished = 0
        if best is not None:
            c0, _, idx = ctx.get_inliers(best["model"], thr)
            polished, prev = c0, 0
            for _ in range(4 if c0 else 0):
                try:
                    nm = ctx.nonminimal(idx[:polished])
                except usac.UsacError:
                    break
                c, _, idx2 = ctx.get_inliers(nm, thr)
                if np.float32(c) / np.float32(polished) < 0.8 or c <= prev:
                    break
                prev = polished = c
                idx = idx2
        out.append((inl, r, polished))
    return out


def main_polish(a, mc, ctxs, model, seeds, thr, prob):
    """--polish: (a) MultiContext.run(polish=True), (a0) MultiContext.run alone, (b) the loop over
    contexts with the restated polish; alternated, host-timed, medians and spreads as in main()"""
    def run_a():
        return [(r["best"]["inliers"], r["rounds"], r["polished"]["inliers"], r["polished"]["passes"])
                for r in mc.run(model, polish=True)]

    def run_a0():
        return mc.run(model)

    def run_b():
        return loop_run_polished(ctxs, mc.m, seeds, a.R, thr, prob, a.max_iterations)

    for _ in range(a.warmup):
        ra, _, rb = run_a(), run_a0(), run_b()
    ta, ta0, tb = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ra = run_a()
        t1 = time.perf_counter()
        run_a0()
        t2 = time.perf_counter()
        rb = run_b()
        t3 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        ta0.append((t2 - t1) * 1e3)
        tb.append((t3 - t2) * 1e3)
    agree = [(x[0], x[2]) for x in ra] == [(x[0], x[2]) for x in rb]
    # the C entry points alone (no Python result lists): run + polish with the mask, the run, and
    # the polish of the run's best models with and without the mask
    L, P = usac.lib(), mc.P
    prm = usac._params(model)
    prm.seed = model.seed
    out, pol = (usac._MultiOutput * P)(), (usac._MultiPolishOutput * P)()
    mask = np.zeros(int(mc.offsets[-1]), dtype=np.uint8)
    maskp = mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    L.usac_multi_run(mc._h, ctypes.byref(prm), None, out)
    best = np.ascontiguousarray([o.best.model[:] for o in out], dtype=np.float32)
    bestp = best.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    calls = {"lib_run_polished_ms": lambda: L.usac_multi_run_polished(mc._h, ctypes.byref(prm), None, out, pol, maskp),
             "lib_run_ms": lambda: L.usac_multi_run(mc._h, ctypes.byref(prm), None, out),
             "lib_polish_ms": lambda: L.usac_multi_polish(mc._h, bestp, ctypes.c_float(thr), pol, maskp),
             "lib_polish_nomask_ms": lambda: L.usac_multi_polish(mc._h, bestp, ctypes.c_float(thr), pol, None)}
    lib_ms = {}
    for name, call in calls.items():
        ts = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            rc = call()
            ts.append((time.perf_counter() - t0) * 1e3)
            if rc != 0:
                raise RuntimeError("%s failed: %d" % (name, rc))
        lib_ms[name] = round(statistics.median(ts[a.warmup:]), 3)
    ma, ma0, mb = statistics.median(ta), statistics.median(ta0), statistics.median(tb)
    sa, sa0, sb = max(ta) - min(ta), max(ta0) - min(ta0), max(tb) - min(tb)
    line = {"bench": "multi_polish", "estimator": a.estimator, "pairs": a.pairs, "points": a.points, "round": a.R,
            "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "dlt": a.dlt, "reps": a.reps,
            "multi_polished_ms": round(ma, 3), "multi_polished_spread_ms": round(sa, 3),
            "multi_run_ms": round(ma0, 3), "multi_run_spread_ms": round(sa0, 3),
            "polish_adds_ms": round(ma - ma0, 3),
            "loop_polished_ms": round(mb, 3), "loop_polished_spread_ms": round(sb, 3),
            "ratio_loop_over_multi": round(mb / ma, 2),
            "multi_faster_beyond_spread": bool(mb - ma > max(sa, sb)),
            "mean_minimal_inliers": round(float(np.mean([x[0] for x in ra])), 2),
            "mean_polished_inliers": round(float(np.mean([x[2] for x in ra])), 2),
            "mean_passes": round(float(np.mean([x[3] for x in ra])), 2),
            "inliers_agree": bool(agree)}
    line.update(lib_ms)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    mc.close()
    for c in ctxs:
        c.close()
    return 0 if agree else 1


def main_prosac(a, mc, model, est):
    """--sampler prosac: MultiContext.run_prosac against MultiContext.run on the same quality-sorted
    inputs, alternated, host-timed, medians and spreads as in main()"""
    pmodel = usac.Model(model.threshold, mc.m, model.desired_prob, 5, est, usac.SAMPLER.Prosac)
    pmodel.max_iterations, pmodel.batch, pmodel.seed = model.max_iterations, model.batch, model.seed
    pmodel.setDLTMode(model.dlt_mode)

    def summary(res, ms):
        rounds = [r["rounds"] for r in res]
        d = {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
             "mean_rounds": round(float(np.mean(rounds)), 2), "launch_rounds": int(max(rounds)),
             "ms_per_launch_round": round(statistics.median(ms) / max(rounds), 3),
             "hypotheses": int(sum(r["hypotheses"] for r in res)),
             "mean_best_inliers": round(float(np.mean([r["best"]["inliers"] for r in res])), 2)}
        if a.polish:
            d["mean_polished_inliers"] = round(float(np.mean([r["polished"]["inliers"] for r in res])), 2)
        return d

    for _ in range(a.warmup):
        rp, ru = mc.run_prosac(pmodel, polish=a.polish), mc.run(model, polish=a.polish)
    tp, tu = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rp = mc.run_prosac(pmodel, polish=a.polish)
        t1 = time.perf_counter()
        ru = mc.run(model, polish=a.polish)
        t2 = time.perf_counter()
        tp.append((t1 - t0) * 1e3)
        tu.append((t2 - t1) * 1e3)
    line = {"bench": "multi_prosac", "estimator": a.estimator, "pairs": a.pairs, "points": a.points, "round": a.R,
            "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "dlt": a.dlt, "reps": a.reps,
            "polish": bool(a.polish), "prosac": summary(rp, tp), "uniform": summary(ru, tu),
            "mean_scans": round(float(np.mean([r["scans"] for r in rp])), 2),
            "mean_termination_length": round(float(np.mean([r["termination_length"] for r in rp])), 1)}
    line["ratio_uniform_over_prosac"] = round(line["uniform"]["ms"] / line["prosac"]["ms"], 2)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    mc.close()
    return 0


def main_lo(a, mc, model, est):
    """--lo: MultiContext.run_lo (--estimator essential: run_lo_essential) against the same run without LO (run, or run_prosac with --sampler
    prosac) on the same inputs, alternated, host-timed, medians and spreads as in main()"""
    prosac = a.sampler == "prosac"
    base = usac.Model(model.threshold, mc.m, model.desired_prob, 5, est,
                      usac.SAMPLER.Prosac if prosac else usac.SAMPLER.Uniform)
    base.max_iterations, base.batch, base.seed = model.max_iterations, model.batch, model.seed
    base.setDLTMode(model.dlt_mode)
    lmodel = usac.Model(model.threshold, mc.m, model.desired_prob, 5, est, base.sampler)
    lmodel.max_iterations, lmodel.batch, lmodel.seed = model.max_iterations, model.batch, model.seed
    lmodel.setDLTMode(model.dlt_mode)
    lmodel.lo = usac.LocOpt.InItLORsc if a.lo == "lorsc" else usac.LocOpt.InItFLORsc
    run_base = mc.run_prosac if prosac else mc.run
    run_lo = mc.run_lo_essential if a.estimator == "essential" else mc.run_lo

    def summary(res, ms):
        rounds = [r["rounds"] for r in res]
        d = {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
             "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
             "mean_rounds": round(float(np.mean(rounds)), 2), "launch_rounds": int(max(rounds)),
             "hypotheses": int(sum(r["hypotheses"] for r in res)),
             "mean_best_inliers": round(float(np.mean([r["best"]["inliers"] for r in res])), 2)}
        if a.polish:
            d["mean_polished_inliers"] = round(float(np.mean([r["polished"]["inliers"] for r in res])), 2)
        return d

    for _ in range(a.warmup):
        rl, rb = run_lo(lmodel, polish=a.polish), run_base(base, polish=a.polish)
    tl, tb = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rl = run_lo(lmodel, polish=a.polish)
        t1 = time.perf_counter()
        rb = run_base(base, polish=a.polish)
        t2 = time.perf_counter()
        tl.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    line = {"bench": "multi_lo", "lo": a.lo, "sampler": a.sampler, "estimator": a.estimator, "pairs": a.pairs,
            "points": a.points, "round": a.R, "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio,
            "dlt": a.dlt, "reps": a.reps, "polish": bool(a.polish), "with_lo": summary(rl, tl),
            "without_lo": summary(rb, tb)}
    for key in ("lo_calls", "fits", "improved", "capped", "inner_iters", "iterative_iters"):
        line["with_lo"]["mean_" + key] = round(float(np.mean([r["lo"][key] for r in rl])), 3)
    line["ratio_lo_over_without"] = round(line["with_lo"]["ms"] / line["without_lo"]["ms"], 2)
    line["lo_faster_beyond_spread"] = bool(line["without_lo"]["ms"] - line["with_lo"]["ms"] >
                                           max(line["with_lo"]["spread_ms"], line["without_lo"]["spread_ms"]))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    mc.close()
    return 0


def main_sprt(a, mc, model, est):
    """--sprt: MultiContext.run_sprt against the same run without SPRT (run, or run_prosac with --sampler
    prosac) on the same inputs, alternated, host-timed, medians and spreads as in main().  The pools and the
    pool-ordered copy (set_sprt_pool: one host shuffle per pair plus the gather) are built once, outside
    the runs, and timed separately."""
    prosac = a.sampler == "prosac"
    base = usac.Model(model.threshold, mc.m, model.desired_prob, 5, est,
                      usac.SAMPLER.Prosac if prosac else usac.SAMPLER.Uniform)
    base.max_iterations, base.batch, base.seed = model.max_iterations, model.batch, model.seed
    base.setDLTMode(model.dlt_mode)
    smodel = usac.Model(model.threshold, mc.m, model.desired_prob, 5, est, base.sampler)
    smodel.max_iterations, smodel.batch, smodel.seed = model.max_iterations, model.batch, model.seed
    smodel.setDLTMode(model.dlt_mode)
    smodel.setSprt(True)
    run_base = mc.run_prosac if prosac else mc.run

    def summary(res, ms):
        rounds = [r["rounds"] for r in res]
        d = {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
             "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
             "mean_rounds": round(float(np.mean(rounds)), 2), "launch_rounds": int(max(rounds)),
             "hypotheses": int(sum(r["hypotheses"] for r in res)),
             "mean_best_inliers": round(float(np.mean([r["best"]["inliers"] for r in res])), 2)}
        if a.polish:
            d["mean_polished_inliers"] = round(float(np.mean([r["polished"]["inliers"] for r in res])), 2)
        return d

    t0 = time.perf_counter()
    mc.set_sprt_pool()
    setup_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(a.warmup):
        rs, rb = mc.run_sprt(smodel, polish=a.polish), run_base(base, polish=a.polish)
    ts, tb = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rs = mc.run_sprt(smodel, polish=a.polish)
        t1 = time.perf_counter()
        rb = run_base(base, polish=a.polish)
        t2 = time.perf_counter()
        ts.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    line = {"bench": "multi_sprt", "sampler": a.sampler, "estimator": a.estimator, "pairs": a.pairs,
            "points": a.points, "round": a.R, "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio,
            "dlt": a.dlt, "reps": a.reps, "polish": bool(a.polish), "set_sprt_pool_ms": round(setup_ms, 3),
            "with_sprt": summary(rs, ts), "without_sprt": summary(rb, tb)}
    # slots x n_p of the SPRT run: every hypothesis slot (F: 3 per hypothesis, empty ones included)
    slots_points = sum(r["hypotheses"] * mc.spk * int(n) for r, n in zip(rs, mc.sizes))
    w = line["with_sprt"]
    w["points_tested_share"] = round(sum(r["sprt"]["points_tested"] for r in rs) / slots_points, 5)
    w["mean_tests_designed"] = round(float(np.mean([r["sprt"]["tests"] for r in rs])), 2)
    w["accepted"] = int(sum(r["sprt"]["accepted"] for r in rs))
    w["rejected"] = int(sum(r["sprt"]["rejected"] for r in rs))
    line["ratio_sprt_over_without"] = round(w["ms"] / line["without_sprt"]["ms"], 2)
    line["differs_beyond_spread"] = bool(abs(line["without_sprt"]["ms"] - w["ms"]) >
                                         max(w["spread_ms"], line["without_sprt"]["spread_ms"]))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    mc.close()
    return 0


def main_napsac(a, mc, model, est):
    """--sampler napsac: MultiContext.run_napsac against the uniform run (run, or run_lo with --lo) on the
    same inputs, alternated, host-timed, medians and spreads as in main(); the grid build timed apart"""
    nmodel = usac.Model(model.threshold, mc.m, model.desired_prob, 5, est, usac.SAMPLER.Napsac)
    nmodel.max_iterations, nmodel.batch, nmodel.seed = model.max_iterations, model.batch, model.seed
    nmodel.setDLTMode(model.dlt_mode)
    nmodel.setNeighborsType(usac.NeighborsSearch.Grid)
    nmodel.setCellSize(a.cell_size)
    if a.lo:
        nmodel.lo = model.lo = usac.LocOpt.InItLORsc if a.lo == "lorsc" else usac.LocOpt.InItFLORsc
    run_base = mc.run_lo if a.lo else mc.run

    def summary(res, ms):
        rounds = [r["rounds"] for r in res]
        d = {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
             "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
             "mean_rounds": round(float(np.mean(rounds)), 2), "launch_rounds": int(max(rounds)),
             "hypotheses": int(sum(r["hypotheses"] for r in res)),
             "mean_best_inliers": round(float(np.mean([r["best"]["inliers"] for r in res])), 2)}
        if a.polish:
            d["mean_polished_inliers"] = round(float(np.mean([r["polished"]["inliers"] for r in res])), 2)
        return d

    # the grid build of all pairs, apart from the runs: each timed build follows one for another size
    L, build = usac.lib(), []
    for _ in range(a.warmup + a.reps):
        if L.usac_multi_grid(mc._h, a.cell_size + 1, None, None, None, None, None, None, None) != 0:
            raise RuntimeError("usac_multi_grid failed")
        t0 = time.perf_counter()
        rc = L.usac_multi_grid(mc._h, a.cell_size, None, None, None, None, None, None, None)
        build.append((time.perf_counter() - t0) * 1e3)
        if rc != 0:
            raise RuntimeError("usac_multi_grid failed")
    build = build[a.warmup:]
    elig = np.array([len(g["eligible"]) for g in mc.grid_neighbors(a.cell_size)])
    for _ in range(a.warmup):
        rn, ru = mc.run_napsac(nmodel, polish=a.polish), run_base(model, polish=a.polish)
    tn, tu = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rn = mc.run_napsac(nmodel, polish=a.polish)
        t1 = time.perf_counter()
        ru = run_base(model, polish=a.polish)
        t2 = time.perf_counter()
        tn.append((t1 - t0) * 1e3)
        tu.append((t2 - t1) * 1e3)
    line = {"bench": "multi_napsac", "estimator": a.estimator, "pairs": a.pairs, "points": a.points, "round": a.R,
            "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "dlt": a.dlt, "reps": a.reps,
            "polish": bool(a.polish), "lo": a.lo, "cell_size": a.cell_size, "cluster": a.cluster,
            "grid_build_ms": round(statistics.median(build), 3), "grid_build_spread_ms": round(max(build) - min(build), 3),
            "napsac": summary(rn, tn), "uniform": summary(ru, tu)}
    line["napsac"]["share_no_eligible_point"] = round(float(np.mean(elig == 0)), 4)
    line["napsac"]["mean_eligible_share"] = round(float(np.mean(elig / mc.sizes)), 4)
    line["ratio_napsac_over_uniform"] = round(line["napsac"]["ms"] / line["uniform"]["ms"], 2)
    line["napsac_faster_beyond_spread"] = bool(line["uniform"]["ms"] - line["napsac"]["ms"] >
                                               max(line["napsac"]["spread_ms"], line["uniform"]["spread_ms"]))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    mc.close()
    return 0


def same_bits(x, y):
    """equal without tolerance: floats and float arrays by bit pattern"""
    if isinstance(x, dict):
        return list(x) == list(y) and all(same_bits(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(same_bits(u, v) for u, v in zip(x, y))
    if isinstance(x, np.ndarray):
        return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    if isinstance(x, float):
        return np.float64(x).tobytes() == np.float64(y).tobytes()
    return x == y


def main_thresholds(a, mc, model, est):
    """--per-problem-thr: the selected run with P thresholds equal to the scalar against the same run
    without them, alternated, host-timed, medians and spreads as in main()"""
    S = usac.SAMPLER
    sampler = {"uniform": S.Uniform, "prosac": S.Prosac, "napsac": S.Napsac}[a.sampler]
    rmodel = usac.Model(model.threshold, mc.m, model.desired_prob, 5, est, sampler)
    rmodel.max_iterations, rmodel.batch, rmodel.seed = model.max_iterations, model.batch, model.seed
    rmodel.setDLTMode(model.dlt_mode)
    if a.sampler == "napsac":
        rmodel.setNeighborsType(usac.NeighborsSearch.Grid)
        rmodel.setCellSize(a.cell_size)
    if a.lo:
        rmodel.lo = usac.LocOpt.InItLORsc if a.lo == "lorsc" else usac.LocOpt.InItFLORsc
    rmodel.setSprt(a.sprt)
    if a.sprt:
        mc.set_sprt_pool()
    run_lo = mc.run_lo_essential if a.estimator == "essential" else mc.run_lo
    call = (mc.run_napsac if a.sampler == "napsac" else mc.run_sprt if a.sprt else run_lo if a.lo
            else mc.run_prosac if a.sampler == "prosac" else mc.run)
    thrs = [model.threshold] * mc.P

    def run(per_problem):
        mc.set_thresholds(thrs if per_problem else None)
        t0 = time.perf_counter()
        res = call(rmodel, polish=a.polish)
        return res, (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        run(True), run(False)
    tp, ts, equal = [], [], True
    for _ in range(a.reps):
        rp, ms_p = run(True)
        rs, ms_s = run(False)
        tp.append(ms_p)
        ts.append(ms_s)
        equal = equal and same_bits(rp, rs)

    def summary(ms):
        return {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3),
                "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    line = {"bench": "multi_thresholds", "run": call.__name__, "estimator": a.estimator, "pairs": a.pairs,
            "points": a.points, "round": a.R, "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio,
            "dlt": a.dlt, "reps": a.reps, "polish": bool(a.polish), "lo": a.lo, "sprt": bool(a.sprt),
            "sampler": a.sampler, "per_problem": summary(tp), "scalar": summary(ts),
            "launch_rounds": int(max(r["rounds"] for r in rs)),
            "hypotheses": int(sum(r["hypotheses"] for r in rs)),
            "mean_best_inliers": round(float(np.mean([r["best"]["inliers"] for r in rs])), 2),
            "results_bit_equal": bool(equal)}
    line["indexed_path_ms"] = round(line["per_problem"]["ms"] - line["scalar"]["ms"], 3)
    line["differs_beyond_spread"] = bool(abs(line["indexed_path_ms"]) >
                                         max(line["per_problem"]["spread_ms"], line["scalar"]["spread_ms"]))
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    mc.close()
    return 0 if equal else 1


def pixel_pairs(pairs, points, ratio):
    """(pixel sets, K P x 3 x 3): the calibrated pairs of make_pairs seen through cameras whose focal lengths run
    from 800 to 1600 px over the pairs and whose principal points differ"""
    cal = make_pairs("essential", pairs, points, ratio)
    K = np.zeros((pairs, 3, 3), dtype=np.float32)
    sets = []
    for p, x in enumerate(cal):
        f = np.float32(800.0 + 800.0 * p / max(pairs - 1, 1))
        cx, cy = np.float32(640.0 + (p % 7)), np.float32(360.0 + (p % 5))
        K[p] = [[f, 0, cx], [0, f, cy], [0, 0, 1]]
        sets.append(np.ascontiguousarray(x * f + np.array([cx, cy, cx, cy], dtype=np.float32), dtype=np.float32))
    return sets, K


def numpy_calibrate(sets, K):
    """what a caller does today: every set to calibrated coordinates in float32, by the library's formulas"""
    out = []
    for px, k in zip(sets, K):
        fx, sk, cx, fy, cy = k[0, 0], k[0, 1], k[0, 2], k[1, 1], k[1, 2]
        y1 = (px[:, 1] - cy) / fy
        y2 = (px[:, 3] - cy) / fy
        out.append(np.stack([((px[:, 0] - cx) - sk * y1) / fx, y1, ((px[:, 2] - cx) - sk * y2) / fx, y2], axis=1))
    return out


def main_pixels(a, model):
    """--pixels: creation from pixel coordinates on the device against the numpy conversion + creation from
    calibrated rows, alternated, host-timed"""
    # (t / f)^2 against the mean epipolar distance in calibrated units: 45 px give 0.0032 .. 0.0008 over the focal
    # lengths, around the 0.002 of the other essential modes
    t_px = np.float32(45.0)
    sets, K = pixel_pairs(a.pairs, a.points, a.inlier_ratio)
    L = usac.lib()
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)

    def create_pixels():
        t0 = time.perf_counter()
        mc = usac.MultiContext.essential_pixels(sets, K)
        mc.set_pixel_thresholds(t_px)
        return mc, (time.perf_counter() - t0) * 1e3

    def create_numpy():
        t0 = time.perf_counter()
        rows = numpy_calibrate(sets, K)
        t1 = time.perf_counter()
        mc = usac.MultiContext.essential(rows)
        f = ((K[:, 0, 0] + K[:, 1, 1]) + (K[:, 0, 0] + K[:, 1, 1])) * np.float32(0.25)
        r = t_px / f
        mc.set_thresholds(r * r)
        t2 = time.perf_counter()
        return mc, (t2 - t0) * 1e3, (t1 - t0) * 1e3

    flat = np.ascontiguousarray(np.concatenate(sets, axis=0), dtype=np.float32)
    offs = np.zeros(a.pairs + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(x) for x in sets])
    k9 = np.ascontiguousarray(K.reshape(a.pairs, 9))

    def create_c():
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = L.usac_multi_create_essential_pixels(ctypes.byref(h), 0, flat.ctypes.data_as(f32p), offs.ctypes.data_as(u32p),
                                                  a.pairs, k9.ctypes.data_as(f32p), None)
        ms = (time.perf_counter() - t0) * 1e3
        if rc != 0:
            raise usac.UsacError(rc, "usac_multi_create_essential_pixels")
        L.usac_multi_destroy(h)
        return ms

    for _ in range(a.warmup):
        create_pixels()[0].close()
        create_numpy()[0].close()
        create_c()
    tp, tn, tconv, tc = [], [], [], []
    for _ in range(a.reps):
        mc, ms = create_pixels()
        mc.close()
        tp.append(ms)
        mc, ms, conv = create_numpy()
        mc.close()
        tn.append(ms)
        tconv.append(conv)
        tc.append(create_c())

    mp, _ = create_pixels()
    mn, _, _ = create_numpy()
    rows_equal = mp.points.tobytes() == mn.points.tobytes()
    thr_equal = mp.thresholds.tobytes() == mn.thresholds.tobytes()
    rp, rn = mp.run(model, polish=True), mn.run(model, polish=True)
    equal = same_bits(rp, rn)
    mp.close()
    mn.close()

    def summary(ms):
        return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}

    line = {"bench": "multi_pixels", "estimator": a.estimator, "pairs": a.pairs, "points": a.points, "round": a.R,
            "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "reps": a.reps, "t_px": float(t_px),
            "focal_lengths": [float(K[0, 0, 0]), float(K[-1, 0, 0])],
            "from_pixels": summary(tp), "numpy_then_create": summary(tn), "numpy_conversion_alone": summary(tconv),
            "c_entry_alone": summary(tc),
            "ratio_numpy_path_over_pixels": round(statistics.median(tn) / statistics.median(tp), 2),
            "rows_bit_equal": bool(rows_equal), "thresholds_bit_equal": bool(thr_equal),
            "run_polished_bit_equal": bool(equal),
            "mean_best_inliers": round(float(np.mean([r["best"]["inliers"] for r in rp])), 2),
            "mean_polished_inliers": round(float(np.mean([r["polished"]["inliers"] for r in rp])), 2)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0 if equal and rows_equal and thr_equal else 1


def device_output(a, n_max, create, run, scores):
    """--device-output (inside --device-input, with or without --scores): the results of a polished run as device
    tensors, two ways, alternated, host-timed, each ending synchronised.  A, before ABI 27: run(polish=True),
    padded_mask() and an upload of the polished models as a (P, 3, 3) tensor.  B: keep_on_device = True, the same
    run, export_device(inlier_cols=n_max) -- nothing N_total-sized crosses in either direction, and the inliers'
    columns come with it.  Both create and close their context.  Then export_device alone against padded_mask()
    alone on one context.  create() -> a context from the padded device tensors, run(mc) -> its polished run."""
    import torch

    dev = torch.device("cuda:0")

    def pipe_a():
        mc = create()
        res = run(mc)
        mask = mc.padded_mask()
        models = torch.from_numpy(np.stack([r["polished"]["model"] for r in res]).reshape(-1, 3, 3)).to(dev)
        torch.cuda.synchronize()
        mc.close()
        return mask, models, res

    def pipe_b():
        mc = create()
        mc.keep_on_device = True
        res = run(mc)
        out = mc.export_device(inlier_cols=n_max)  # waits for its stream
        mc.close()
        return out, res

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        pipe_a()
        pipe_b()
    ta, tb, tmask, texp, texp_mask = [], [], [], [], []
    for _ in range(a.reps):
        (mask_a, models_a, res_a), ms = timed(pipe_a)
        ta.append(ms)
        (out_b, res_b), ms = timed(pipe_b)
        tb.append(ms)
        mc = create()
        run(mc)
        _, ms = timed(lambda: mc.export_device(inlier_cols=n_max))
        texp.append(ms)
        _, ms = timed(mc.export_device)  # the mask, the models, counts and statuses: what A delivers
        texp_mask.append(ms)
        _, ms = timed(mc.padded_mask)    # last: its upload ends the resident result
        tmask.append(ms)
        mc.close()
    masks_equal = bool(torch.equal(mask_a, out_b["mask"]))
    models_equal = bool(torch.equal(models_a.view(torch.int32), out_b["models"].view(torch.int32)))
    counts = out_b["inliers"].cpu().numpy()
    cols = out_b["inlier_cols"].cpu().numpy()
    lists_fit = bool((counts == [r["polished"]["inliers"] for r in res_a]).all() and
                     ((cols >= 0).sum(1) == np.minimum(counts, n_max)).all())
    dicts_equal = same_bits([r["polished"] for r in res_a], [r["polished"] for r in res_b])

    def summary(ms):
        return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}

    ma, mb = statistics.median(ta), statistics.median(tb)
    line = {"bench": "multi_export", "estimator": a.estimator, "scores": bool(scores), "pairs": a.pairs,
            "points": a.points, "n_max": n_max, "round": a.R, "max_iterations": a.max_iterations,
            "inlier_ratio": a.inlier_ratio, "dlt": a.dlt, "reps": a.reps,
            "pipeline_a_padded_mask_and_model_upload": summary(ta), "pipeline_b_resident_export": summary(tb),
            "b_median_minus_a_median_ms": round(mb - ma, 3), "b_median_not_above_a_max": bool(mb <= max(ta)),
            "b_median_below_a_median": bool(mb < ma),
            "export_device_with_columns_alone": summary(texp), "export_device_mask_and_models_alone": summary(texp_mask),
            "padded_mask_alone": summary(tmask),
            "masks_equal": masks_equal, "model_tensors_bit_equal": models_equal, "polished_dicts_bit_equal": bool(dicts_equal),
            "counts_and_columns_fit": lists_fit,
            "mean_polished_inliers": round(float(np.mean([r["polished"]["inliers"] for r in res_b])), 2)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0 if masks_equal and models_equal and dicts_equal and lists_fit else 1


def numpy_pose(E, rows, mask):
    """what a caller does today with one pair's E (3 x 3), calibrated rows (n x 4, float64) and inlier mask: numpy's
    SVD, the four (R, t), a vote of the inliers by the depths of the midpoint-free linear triangulation.
    Returns (R, t, the counts of the four candidates, the chosen candidate's front flags over the n rows)."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    idx = np.flatnonzero(mask)
    x1 = np.c_[rows[idx, :2], np.ones(len(idx))]
    x2 = np.c_[rows[idx, 2:], np.ones(len(idx))]
    cands, fronts = [], []
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (U[:, 2], -U[:, 2]):
            a = np.cross(x2, x1 @ R.T)       # z1 (x2 x R x1) = -(x2 x t)
            b = np.cross(x2, np.broadcast_to(t, x2.shape))
            with np.errstate(all="ignore"):
                z1 = -(a * b).sum(1) / (a * a).sum(1)
            z2 = z1 * (x1 @ R[2]) + t[2]
            cands.append((R, t))
            fronts.append((z1 > 0) & (z2 > 0))
    counts = np.array([int(f.sum()) for f in fronts])
    best = int(np.argmax(counts))
    flags = np.zeros(len(rows), dtype=bool)
    flags[idx] = fronts[best]
    return cands[best][0], cands[best][1], counts, flags


def main_pose(a, model):
    """--pose (with --estimator essential --device-input --device-output): from a polished essential run to a pose
    per pair on the device, two ways, alternated, host-timed, each ending synchronised.  Both create their context
    with from_padded(K1=K) from padded pixel rows, set keep_on_device, run(polish=True) and export_device().  A adds
    export_pose(front_mask=True).  B adds what a caller does without it: models and mask to the host, a numpy loop
    over the pairs (numpy_pose), and an upload of R, t and the front mask; the calibrated rows it needs are on the
    host already, converted outside the timing.  A's choice must give B's rotation on every pair whose vote in B
    has a unique winner."""
    import torch

    t_px = np.float32(45.0)
    sets, K = pixel_pairs(a.pairs, a.points, a.inlier_ratio)
    P, n = len(sets), a.points
    n_max = n + n // 4
    rng = np.random.default_rng(17)
    rows = np.zeros((P, n_max, 4), dtype=np.float32)
    valid = np.zeros((P, n_max), dtype=bool)
    for p, pts in enumerate(sets):
        cols = np.sort(rng.permutation(n_max)[:len(pts)])
        rows[p, cols] = pts
        valid[p, cols] = True
    dev = torch.device("cuda:0")
    rows_t, valid_t = torch.from_numpy(rows).to(dev), torch.from_numpy(valid).to(dev)
    torch.cuda.synchronize()
    cal = np.stack(numpy_calibrate(list(rows), K)).astype(np.float64)  # B's host copy of the calibrated rows

    def shared():
        mc = usac.MultiContext.from_padded(usac.ESTIMATOR.Essential, rows_t, valid=valid_t, K1=K)
        mc.set_pixel_thresholds(t_px)
        mc.keep_on_device = True
        mc.run(model, polish=True)
        return mc, mc.export_device()

    def pipe_a():
        mc, exp = shared()
        pose = mc.export_pose(front_mask=True)  # waits for its stream
        mc.close()
        return exp, pose

    def pipe_b():
        mc, exp = shared()
        models = exp["models"].cpu().numpy().astype(np.float64)
        mask = exp["mask"].cpu().numpy()
        R = np.zeros((P, 3, 3), dtype=np.float32)
        t = np.zeros((P, 3), dtype=np.float32)
        front = np.zeros((P, n_max), dtype=bool)
        counts = np.zeros((P, 4), dtype=np.int64)
        for p in range(P):
            R[p], t[p], counts[p], front[p] = numpy_pose(models[p], cal[p], mask[p])
        up = {"R": torch.from_numpy(R).to(dev), "t": torch.from_numpy(t).to(dev), "front_mask": torch.from_numpy(front).to(dev)}
        torch.cuda.synchronize()
        mc.close()
        return exp, up, counts

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        pipe_a()
        pipe_b()
    ta, tb, tpose, tpose_nomask = [], [], [], []
    for _ in range(a.reps):
        (exp_a, pose_a), ms = timed(pipe_a)
        ta.append(ms)
        (exp_b, up_b, counts_b), ms = timed(pipe_b)
        tb.append(ms)
        mc, _ = shared()
        _, ms = timed(lambda: mc.export_pose(front_mask=True))
        tpose.append(ms)
        _, ms = timed(mc.export_pose)
        tpose_nomask.append(ms)
        mc.close()
    models_equal = bool(torch.equal(exp_a["models"].view(torch.int32), exp_b["models"].view(torch.int32)))
    top = np.sort(counts_b, axis=1)
    unique = (top[:, -1] > top[:, -2]) & (top[:, -1] > 0)
    Ra, Rb = pose_a["R"].cpu().numpy().astype(np.float64), up_b["R"].cpu().numpy().astype(np.float64)
    ta_, tb_ = pose_a["t"].cpu().numpy().astype(np.float64), up_b["t"].cpu().numpy().astype(np.float64)
    choice = pose_a["choice"].cpu().numpy()
    r_err = np.abs(Ra - Rb).reshape(P, -1).max(1)
    t_err = np.abs(ta_ - tb_).max(1)
    # the rotation decides: the two triangulations differ (B's is not the rule's), and on a poor model whose
    # inliers split almost evenly between +t and -t their votes may pick opposite signs of t for one R
    agree = (choice >= 0) & (r_err < 1e-4)
    rotations_agree = bool(agree[unique].all())
    translations_agree = int((agree & (t_err < 1e-4))[unique].sum())
    front_a = pose_a["front"].cpu().numpy()

    def summary(ms):
        return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}

    ma, mb = statistics.median(ta), statistics.median(tb)
    line = {"bench": "multi_pose", "estimator": a.estimator, "pairs": a.pairs, "points": a.points, "n_max": n_max,
            "round": a.R, "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "reps": a.reps,
            "pipeline_a_export_pose": summary(ta), "pipeline_b_host_decomposition": summary(tb),
            "a_median_minus_b_median_ms": round(ma - mb, 3), "b_median_over_a_median": round(mb / ma, 3),
            "export_pose_with_front_mask_alone": summary(tpose), "export_pose_without_front_mask_alone": summary(tpose_nomask),
            "model_tensors_bit_equal": models_equal, "pairs_with_a_unique_vote": int(unique.sum()),
            "share_of_pairs_checked": round(float(unique.mean()), 4), "rotations_agree_on_checked_pairs": rotations_agree,
            "max_rotation_difference_on_checked_pairs": float(r_err[unique].max()) if unique.any() else None,
            "checked_pairs_with_the_same_translation_too": translations_agree,
            "pairs_with_a_choice": int((choice >= 0).sum()), "mean_front": round(float(front_a.mean()), 2),
            "front_counts_equal_on_checked_pairs": bool((front_a[unique] == top[unique, -1]).all())}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0 if models_equal and rotations_agree and unique.any() else 1


def pose_errors(R, t):
    """per pair the rotation angle between R and the generator's rotation and the angle between t and the
    generator's translation direction, in degrees (every pair of make_pairs has the pose of two_view_geometry)"""
    _, R_gt, t_gt, _, _ = synthetic.two_view_geometry()
    t_gt = t_gt / np.linalg.norm(t_gt)
    R, t = R.astype(np.float64), t.astype(np.float64)
    tr = np.einsum("pij,ij->p", R, R_gt)
    rot = np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))
    nt = np.linalg.norm(t, axis=1)
    with np.errstate(all="ignore"):
        tra = np.degrees(np.arccos(np.clip((t @ t_gt) / nt, -1.0, 1.0)))
    return rot, tra


def main_refine(a, model):
    """--pose --refine: the pipeline of main_pose that ends in export_pose(front_mask=True) (A), and the same plus
    refine_pose(R, t, front_mask) (R), alternated, host-timed, each ending synchronised; refine_pose alone on one
    context.  Quality: the errors of both poses against the generator's."""
    import torch

    t_px = np.float32(45.0)
    sets, K = pixel_pairs(a.pairs, a.points, a.inlier_ratio)
    P, n = len(sets), a.points
    n_max = n + n // 4
    rng = np.random.default_rng(17)
    rows = np.zeros((P, n_max, 4), dtype=np.float32)
    valid = np.zeros((P, n_max), dtype=bool)
    for p, pts in enumerate(sets):
        cols = np.sort(rng.permutation(n_max)[:len(pts)])
        rows[p, cols] = pts
        valid[p, cols] = True
    dev = torch.device("cuda:0")
    rows_t, valid_t = torch.from_numpy(rows).to(dev), torch.from_numpy(valid).to(dev)
    torch.cuda.synchronize()

    def shared():
        mc = usac.MultiContext.from_padded(usac.ESTIMATOR.Essential, rows_t, valid=valid_t, K1=K)
        mc.set_pixel_thresholds(t_px)
        mc.keep_on_device = True
        mc.run(model, polish=True)
        mc.export_device()
        return mc, mc.export_pose(front_mask=True)  # waits for its stream

    def pipe_a():
        mc, pose = shared()
        mc.close()
        return pose

    def pipe_r():
        mc, pose = shared()
        ref = mc.refine_pose(pose["R"], pose["t"], pose["front_mask"], max_iters=a.refine_iters)  # waits for its stream
        mc.close()
        return pose, ref

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        pipe_a()
        pipe_r()
    ta, tr, talone = [], [], []
    for _ in range(a.reps):
        pose_a, ms = timed(pipe_a)
        ta.append(ms)
        (pose_r, ref), ms = timed(pipe_r)
        tr.append(ms)
        mc, pose = shared()
        _, ms = timed(lambda: mc.refine_pose(pose["R"], pose["t"], pose["front_mask"], max_iters=a.refine_iters))
        talone.append(ms)
        mc.close()
    same_start = bool(torch.equal(pose_a["R"].view(torch.int32), pose_r["R"].view(torch.int32)))
    choice = pose_r["choice"].cpu().numpy()
    it = ref["iterations"].cpu().numpy()
    cost0, cost = ref["cost0"].cpu().numpy(), ref["cost"].cpu().numpy()
    done = it >= 0
    rot0, tra0 = pose_errors(pose_r["R"].cpu().numpy()[done], pose_r["t"].cpu().numpy()[done])
    rot1, tra1 = pose_errors(ref["R"].cpu().numpy()[done], ref["t"].cpu().numpy()[done])
    never_rose = bool((cost <= cost0).all())

    def summary(ms):
        return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}

    def med(v):
        return round(float(np.median(v)), 4) if len(v) else None

    line = {"bench": "multi_refine", "estimator": a.estimator, "pairs": a.pairs, "points": a.points, "n_max": n_max,
            "round": a.R, "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "reps": a.reps,
            "refine_max_iters": a.refine_iters,
            "pipeline_a_export_pose": summary(ta), "pipeline_r_export_pose_refine_pose": summary(tr),
            "r_median_minus_a_median_ms": round(statistics.median(tr) - statistics.median(ta), 3),
            "refine_pose_alone": summary(talone), "same_start_in_both_pipelines": same_start,
            "pairs_with_a_choice": int((choice >= 0).sum()), "pairs_refined": int(done.sum()),
            "mean_used_rows": round(float(ref["used"].cpu().numpy()[done].mean()), 2) if done.any() else None,
            "iterations_min_median_max": [int(it[done].min()), float(np.median(it[done])), int(it[done].max())] if done.any() else None,
            "median_rotation_error_deg": {"export_pose": med(rot0), "refine_pose": med(rot1)},
            "median_translation_error_deg": {"export_pose": med(tra0), "refine_pose": med(tra1)},
            "pairs_whose_rotation_error_fell": int((rot1 < rot0).sum()),
            "pairs_whose_translation_error_fell": int((tra1 < tra0).sum()),
            "median_cost_ratio": med(cost[done] / cost0[done]), "cost_never_rose": never_rose}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0 if never_rose and done.any() else 1


def main_device(a, model, est, sets):
    """--device-input: from padded device tensors to the polished inliers as a (P, n_max) bool tensor on the device,
    what a caller does today (pipeline A: down to numpy, ragged sets, MultiContext, run, mask built in numpy, up
    again) against from_padded + run + padded_mask (pipeline B), alternated, host-timed; both end synchronised"""
    import torch

    P, n = len(sets), a.points
    n_max = n + n // 4  # a matcher's padded width: a fifth of the columns hold no match
    rng = np.random.default_rng(17)
    rows = np.zeros((P, n_max, 4), dtype=np.float32)
    valid = np.zeros((P, n_max), dtype=bool)
    for p, pts in enumerate(sets):
        cols = np.sort(rng.permutation(n_max)[:len(pts)])  # the pair's order survives
        rows[p, cols] = pts
        valid[p, cols] = True
    dev = torch.device("cuda:0")
    rows_t, valid_t = torch.from_numpy(rows).to(dev), torch.from_numpy(valid).to(dev)
    torch.cuda.synchronize()
    essential = est == usac.ESTIMATOR.Essential

    def create_a():
        r, v = rows_t.cpu().numpy(), valid_t.cpu().numpy()
        host_sets = [r[p][v[p]] for p in range(P)]
        return (usac.MultiContext.essential(host_sets) if essential else usac.MultiContext(est, host_sets)), v

    def create_b():
        return usac.MultiContext.from_padded(est, rows_t, valid=valid_t)

    if a.device_output:
        return device_output(a, n_max, create_b, lambda mc: mc.run(model, polish=True), False)

    def pipe_a():
        mc, v = create_a()
        res = mc.run(model, polish=True)
        pad = np.zeros((P, n_max), dtype=bool)
        for p, r in enumerate(res):
            pad[p, np.flatnonzero(v[p])[r["inliers"]]] = True
        out = torch.from_numpy(pad).to(dev)
        torch.cuda.synchronize()
        mc.close()
        return out, res

    def pipe_b():
        mc = create_b()
        res = mc.run(model, polish=True)
        out = mc.padded_mask()
        mc.close()
        return out, res

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        pipe_a()
        pipe_b()
    ta, tb, tca, tcb, trun, tmask = [], [], [], [], [], []
    for _ in range(a.reps):
        (mask_a, res_a), ms = timed(pipe_a)
        ta.append(ms)
        (mask_b, res_b), ms = timed(pipe_b)
        tb.append(ms)
        (mc, _), ms = timed(create_a)
        tca.append(ms)
        mc.close()
        mc, ms = timed(create_b)
        tcb.append(ms)
        _, ms = timed(lambda: mc.run(model, polish=True))
        trun.append(ms)
        _, ms = timed(mc.padded_mask)
        tmask.append(ms)
        mc.close()
    masks_equal = bool(torch.equal(mask_a, mask_b))
    models_equal = same_bits([r["polished"] for r in res_a], [r["polished"] for r in res_b]) and \
        same_bits([r["best"] for r in res_a], [r["best"] for r in res_b])

    def summary(ms):
        return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}

    line = {"bench": "multi_device", "estimator": a.estimator, "pairs": P, "points": n, "n_max": n_max, "round": a.R,
            "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "dlt": a.dlt, "reps": a.reps,
            "pipeline_a_host_round_trip": summary(ta), "pipeline_b_device_input": summary(tb),
            "ratio_a_over_b": round(statistics.median(ta) / statistics.median(tb), 2),
            "creation_a_numpy_sets_and_constructor": summary(tca), "creation_b_from_padded": summary(tcb),
            "run_polished_alone_on_b": summary(trun), "padded_mask_alone": summary(tmask),
            "masks_equal": masks_equal, "polished_models_bit_equal": bool(models_equal),
            "mean_polished_inliers": round(float(np.mean([r["polished"]["inliers"] for r in res_b])), 2),
            "mask_cells_set": int(mask_b.sum().item())}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0 if masks_equal and models_equal else 1


def main_device_sorted(a, model, est, sets):
    """--device-input --scores: a matcher's output -- matches in keypoint order and a score per keypoint -- as padded
    device tensors in, the polished inliers as a (P, n_max) bool device tensor out, three ways, alternated,
    host-timed, each ending synchronised.  S: from_padded(scores=...) + run_prosac + padded_mask.  U: from_padded +
    run (uniform sampler) + padded_mask, the best without the scores.  T: torch.sort(stable=True) + gather +
    from_padded + run_prosac + padded_mask + the inverse permutation of the mask, the caller's own reordering.
    sets are quality-sorted pairs; every pair's columns are permuted and column j scores 1 - rank / n."""
    import torch

    P, n = len(sets), a.points
    n_max = n + n // 4
    rng = np.random.default_rng(17)
    rows = np.zeros((P, n_max, 4), dtype=np.float32)
    valid = np.zeros((P, n_max), dtype=bool)
    scores = np.zeros((P, n_max), dtype=np.float32)
    for p, pts in enumerate(sets):
        cols = rng.permutation(n_max)[:len(pts)]  # rank i sits in column cols[i]: unsorted, with gaps
        rows[p, cols] = pts
        valid[p, cols] = True
        scores[p, cols] = (1.0 - np.arange(len(pts)) / len(pts)).astype(np.float32)
    dev = torch.device("cuda:0")
    rows_t, valid_t, scores_t = (torch.from_numpy(x).to(dev) for x in (rows, valid, scores))
    torch.cuda.synchronize()
    pmodel = usac.Model(model.threshold, model.sample_size, model.desired_prob, 5, est, usac.SAMPLER.Prosac)
    pmodel.max_iterations, pmodel.batch, pmodel.seed = model.max_iterations, model.batch, model.seed
    pmodel.setDLTMode(model.dlt_mode)

    if a.device_output:
        return device_output(a, n_max, lambda: usac.MultiContext.from_padded(est, rows_t, valid=valid_t, scores=scores_t),
                             lambda mc: mc.run_prosac(pmodel, polish=True), True)

    def pipe_s():
        mc = usac.MultiContext.from_padded(est, rows_t, valid=valid_t, scores=scores_t)
        res = mc.run_prosac(pmodel, polish=True)
        out = mc.padded_mask()
        mc.close()
        return out, res

    def pipe_u():
        mc = usac.MultiContext.from_padded(est, rows_t, valid=valid_t)
        res = mc.run(model, polish=True)
        out = mc.padded_mask()
        mc.close()
        return out, res

    def pipe_t():
        key = torch.where(valid_t, scores_t, torch.full_like(scores_t, float("-inf")))
        perm = torch.sort(key, dim=1, descending=True, stable=True).indices
        rows_s = torch.gather(rows_t, 1, perm[:, :, None].expand(-1, -1, 4)).contiguous()
        valid_s = torch.gather(valid_t, 1, perm)
        mc = usac.MultiContext.from_padded(est, rows_s, valid=valid_s)
        res = mc.run_prosac(pmodel, polish=True)
        sorted_mask = mc.padded_mask()
        out = torch.zeros_like(sorted_mask).scatter_(1, perm, sorted_mask)
        torch.cuda.synchronize()
        mc.close()
        return out, res

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        pipe_s(), pipe_u(), pipe_t()
    ts, tu, tt, tcs, tcu = [], [], [], [], []
    for _ in range(a.reps):
        (mask_s, res_s), ms = timed(pipe_s)
        ts.append(ms)
        (mask_u, res_u), ms = timed(pipe_u)
        tu.append(ms)
        (mask_t, res_t), ms = timed(pipe_t)
        tt.append(ms)
        mc, ms = timed(lambda: usac.MultiContext.from_padded(est, rows_t, valid=valid_t, scores=scores_t))
        tcs.append(ms)
        mc.close()
        mc, ms = timed(lambda: usac.MultiContext.from_padded(est, rows_t, valid=valid_t))
        tcu.append(ms)
        mc.close()
    masks_equal = bool(torch.equal(mask_s, mask_t))
    models_equal = same_bits([r["polished"] for r in res_s], [r["polished"] for r in res_t]) and \
        same_bits([r["best"] for r in res_s], [r["best"] for r in res_t])

    def summary(ms):
        return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3)}

    def outcome(res):
        return {"mean_rounds": round(float(np.mean([r["rounds"] for r in res])), 2),
                "mean_best_inliers": round(float(np.mean([r["best"]["inliers"] for r in res])), 2),
                "mean_polished_inliers": round(float(np.mean([r["polished"]["inliers"] for r in res])), 2)}

    line = {"bench": "multi_sorted", "estimator": a.estimator, "pairs": P, "points": n, "n_max": n_max, "round": a.R,
            "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "dlt": a.dlt, "reps": a.reps,
            "pipeline_s_scores_prosac": summary(ts), "pipeline_u_uniform": summary(tu),
            "pipeline_t_torch_sort_prosac": summary(tt),
            "ratio_u_over_s": round(statistics.median(tu) / statistics.median(ts), 2),
            "ratio_t_over_s": round(statistics.median(tt) / statistics.median(ts), 2),
            "creation_with_scores": summary(tcs), "creation_without_scores": summary(tcu),
            "s": outcome(res_s), "u": outcome(res_u),
            "masks_equal_s_t": masks_equal, "polished_models_bit_equal_s_t": bool(models_equal)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    return 0 if masks_equal and models_equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--round", type=int, default=256, dest="R")
    ap.add_argument("--estimator", choices=["homography", "fundamental", "essential"], default="homography",
                    help="essential: MultiContext.essential over calibrated pairs, threshold 0.002; the plain run, "
                         "--polish, --sampler prosac and --lo (MultiContext.run_lo_essential)")
    ap.add_argument("--inlier-ratio", type=float, default=0.3)
    ap.add_argument("--max-iterations", type=int, default=2048)
    ap.add_argument("--dlt", choices=["thin", "nullspace"], default="nullspace")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--polish", action="store_true",
                    help="time run + non-minimal polish: MultiContext.run(polish=True) against the multi run "
                         "alone and against the loop over contexts with the polish restated per context")
    ap.add_argument("--sampler", choices=["uniform", "prosac", "napsac"], default="uniform",
                    help="prosac: quality-sorted inputs, MultiContext.run_prosac against the uniform multi run; "
                         "napsac: MultiContext.run_napsac against the uniform multi run")
    ap.add_argument("--cell-size", type=int, default=50, help="--sampler napsac: the grid cell")
    ap.add_argument("--cluster", type=float, default=None, metavar="HW",
                    help="homography pairs whose inliers sit in the box (500 +- HW)^2 of the first image")
    ap.add_argument("--lo", choices=["lorsc", "florsc"], default=None,
                    help="MultiContext.run_lo (inner + iterative LO-RANSAC, unlimited / limited) against the same "
                         "run without LO; with --sampler prosac both use the PROSAC sampler")
    ap.add_argument("--sprt", action="store_true",
                    help="MultiContext.run_sprt (SPRT verification of every slot, one test per pair and round) against "
                         "the same run without SPRT; with --sampler prosac both use the PROSAC sampler")
    ap.add_argument("--per-problem-thr", action="store_true",
                    help="the selected multi run with P per-problem thresholds equal to the scalar "
                         "(MultiContext.set_thresholds) against the same run without them: bit-equal results, and the "
                         "cost of the indexed path")
    ap.add_argument("--pixels", action="store_true",
                    help="--estimator essential: creation from pixel coordinates (MultiContext.essential_pixels + "
                         "set_pixel_thresholds) against the numpy conversion + MultiContext.essential + set_thresholds; "
                         "the two contexts' polished runs must be bit-equal")
    ap.add_argument("--device-input", action="store_true",
                    help="padded torch device tensors in, the polished inliers as a (pairs, n_max) bool device tensor "
                         "out: the host round trip (numpy sets, MultiContext, run, numpy mask, upload) against "
                         "MultiContext.from_padded + run(polish=True) + padded_mask; masks and models must be equal")
    ap.add_argument("--scores", action="store_true",
                    help="--device-input: unsorted columns with a score each (a matcher's output); from_padded(scores=) + "
                         "run_prosac against from_padded + run and against torch.sort + gather + from_padded + run_prosac "
                         "+ the inverse permutation; the first and the last must return equal masks and models")
    ap.add_argument("--device-output", action="store_true",
                    help="--device-input, with or without --scores: the polished run's results as device tensors; run + "
                         "padded_mask + an upload of the polished models against keep_on_device + the same run + "
                         "export_device(inlier_cols=n_max); masks and model tensors must be equal")
    ap.add_argument("--pose", action="store_true",
                    help="--estimator essential --device-input --device-output: from_padded(K1=K) + keep_on_device + "
                         "run(polish=True) + export_device, then export_pose(front_mask=True) against models and mask to "
                         "the host, a numpy decomposition and vote per pair, and an upload of R, t and the front mask")
    ap.add_argument("--refine", action="store_true",
                    help="--pose: the pipeline ending in export_pose(front_mask=True) against the same pipeline plus "
                         "refine_pose(R, t, front_mask); the errors of both poses against the generator's")
    ap.add_argument("--refine-iters", type=int, default=10, help="--refine: max_iters of refine_pose (0..100)")
    a = ap.parse_args()
    if a.refine and not a.pose:
        ap.error("--refine goes with --pose")
    if a.pose and not (a.device_input and a.device_output and a.estimator == "essential" and not a.scores):
        ap.error("--pose goes with --estimator essential --device-input --device-output")
    if a.scores and not a.device_input:
        ap.error("--scores goes with --device-input")
    if a.device_output and not a.device_input:
        ap.error("--device-output goes with --device-input")
    if a.device_input and (a.pixels or a.sprt or a.lo or a.per_problem_thr or a.sampler != "uniform" or a.polish):
        ap.error("--device-input goes with --estimator alone")
    if a.pixels and (a.estimator != "essential" or a.sprt or a.lo or a.per_problem_thr or a.sampler != "uniform"):
        ap.error("--pixels goes with --estimator essential alone")
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.sprt and a.lo:
        ap.error("--sprt and --lo do not combine (usac_multi_run_sprt runs without LO)")
    if a.sampler == "napsac" and a.sprt:
        ap.error("--sampler napsac does not combine with --sprt (usac_multi_run_napsac runs without SPRT)")
    if a.cluster is not None and a.estimator != "homography":
        ap.error("--cluster applies to homography pairs")

    essential = a.estimator == "essential"
    if essential and (a.sprt or a.sampler == "napsac"):
        ap.error("--estimator essential: the plain run, --polish, --sampler prosac and --lo (no SPRT or NAPSAC)")
    est = {"homography": usac.ESTIMATOR.Homography, "fundamental": usac.ESTIMATOR.Fundamental,
           "essential": usac.ESTIMATOR.Essential}[a.estimator]
    thr, prob = (0.002 if essential else 2.0), 0.95
    sets = make_pairs(a.estimator, a.pairs, a.points, a.inlier_ratio, quality_sorted=a.sampler == "prosac" or a.scores,
                      cluster=a.cluster)
    model = usac.Model(thr, {"homography": 4, "fundamental": 7, "essential": 5}[a.estimator], prob, 5, est,
                       usac.SAMPLER.Uniform)
    model.max_iterations, model.batch, model.seed = a.max_iterations, a.R, 1
    model.setDLTMode(usac.DLT.NULLSPACE if a.dlt == "nullspace" else usac.DLT.THIN)
    seeds = [model.seed + p for p in range(a.pairs)]
    if a.pixels:
        return main_pixels(a, model)
    if a.pose and a.refine:
        return main_refine(a, model)
    if a.pose:
        return main_pose(a, model)
    if a.device_input and a.scores:
        return main_device_sorted(a, model, est, sets)
    if a.device_input:
        return main_device(a, model, est, sets)

    mc = usac.MultiContext.essential(sets) if essential else usac.MultiContext(est, sets)
    if a.per_problem_thr:
        return main_thresholds(a, mc, model, est)
    if a.sampler == "napsac":
        return main_napsac(a, mc, model, est)
    if a.sprt:
        return main_sprt(a, mc, model, est)
    if a.lo:
        return main_lo(a, mc, model, est)
    if a.sampler == "prosac":
        return main_prosac(a, mc, model, est)
    ctxs = [usac.Context(est, p) for p in sets]
    for c in ctxs:
        if not essential:
            c.set_dlt_mode(model.dlt_mode)
        c.set_timing(False)

    def run_a():
        return [(r["best"]["inliers"], r["rounds"]) for r in mc.run(model)]

    def run_b():
        return loop_run(ctxs, mc.m, seeds, a.R, thr, prob, a.max_iterations)

    if a.polish:
        return main_polish(a, mc, ctxs, model, seeds, thr, prob)

    for _ in range(a.warmup):
        ra, rb = run_a(), run_b()
    ta, tb = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ra = run_a()
        t1 = time.perf_counter()
        rb = run_b()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    agree = [x[0] for x in ra] == [x[0] for x in rb]
    ma, mb = statistics.median(ta), statistics.median(tb)
    sa, sb = max(ta) - min(ta), max(tb) - min(tb)
    line = {"bench": "multi", "estimator": a.estimator, "pairs": a.pairs, "points": a.points, "round": a.R,
            "max_iterations": a.max_iterations, "inlier_ratio": a.inlier_ratio, "dlt": a.dlt, "reps": a.reps,
            "multi_ms": round(ma, 3), "multi_spread_ms": round(sa, 3), "loop_ms": round(mb, 3),
            "loop_spread_ms": round(sb, 3), "ratio_loop_over_multi": round(mb / ma, 2),
            "multi_faster_beyond_spread": bool(mb - ma > max(sa, sb)),
            "hypotheses": int(sum(x[1] for x in ra)) * a.R, "mean_rounds": round(float(np.mean([x[1] for x in ra])), 2),
            "mean_best_inliers": round(float(np.mean([x[0] for x in ra])), 2),
            "best_inliers_agree": bool(agree)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    mc.close()
    for c in ctxs:
        c.close()
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
