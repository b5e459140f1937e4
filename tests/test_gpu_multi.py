"""Multi-problem batches (usac_multi_*, MultiContext): P ragged point sets per launch.  Every
per-problem output is compared bit for bit with the single-problem path (Context over that
problem's points) and with the CPU oracle: a round's per-hypothesis counts, sums and best record,
the batch-granular run against its loop restated over single contexts, and the inlier masks."""
import ctypes

import numpy as np
import pytest

from ransac_amd import synthetic

pytestmark = pytest.mark.gpu

THR = 2.0
SIZES = {"H": [4, 64, 65, 333, 1000], "F": [7, 64, 65, 333, 1000]}
RATIOS = [0.9, 0.3, 0.3, 0.0, 0.3]
DATA_SEEDS = {"H": [20, 21, 22, 23, 24], "F": [22, 31, 32, 33, 34]}
DUP = (5, 3)                       # problem 5 is a copy of problem 3 (the 333-point set)
SEEDS = [11, 12, 13, 14, 15, 14]   # sampler seeds: the copy shares its original's


def _sets(kind):
    out = []
    for n, ratio, seed in zip(SIZES[kind], RATIOS, DATA_SEEDS[kind]):
        if kind == "H":
            out.append(synthetic.homography_points(n=n, inlier_ratio=ratio, seed=seed)[0])
        else:
            out.append(synthetic.fundamental_points(n=n, inlier_ratio=ratio, seed=seed, prosac_order=False)[0])
    out.append(out[DUP[1]].copy())
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_record(a, b):
    assert a["hyp_index"] == b["hyp_index"] and a["inliers"] == b["inliers"] and a["valid"] == b["valid"]
    assert _bits(a["score"]) == _bits(b["score"])
    np.testing.assert_array_equal(_bits(a["model"]), _bits(b["model"]))


def _same_scores(c, s, rc, rs):
    """counts equal; sums equal bit for bit on the occupied slots and 0 on the empty ones (the
    single context leaves an empty slot's sum unwritten)."""
    np.testing.assert_array_equal(c, rc)
    ok = rc >= 0
    np.testing.assert_array_equal(_bits(s)[ok], _bits(rs)[ok])
    assert (s[~ok] == 0).all()


@pytest.fixture(scope="module")
def problems(usac):
    """kind -> (point sets, MultiContext, the single contexts)"""
    made = {}
    for kind, est in (("H", usac.ESTIMATOR.Homography), ("F", usac.ESTIMATOR.Fundamental)):
        sets = _sets(kind)
        made[kind] = (sets, usac.MultiContext(est, sets), [usac.Context(est, p) for p in sets])
    yield made
    for _, mc, singles in made.values():
        mc.close()
        for c in singles:
            c.close()


# ------------------------------------------------------------------ 1. round == single context
@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_round_equals_single_context(usac, problems, kind, dlt, R):
    sets, mc, singles = problems[kind]
    mc.set_dlt_mode(dlt)
    try:
        for f in (0, 3 * R):
            c, s, best = mc.hypothesize_score(R, SEEDS, first_hyp=f, thr=THR)
            assert c.shape == (len(sets), R * mc.spk)
            for p, ctx in enumerate(singles):
                ctx.set_dlt_mode(dlt)
                rc, rs, rbest = ctx.hypothesize_score(B=R, seed=SEEDS[p], first_hyp=f, thr=THR, per_hypothesis=True)
                ctx.set_dlt_mode(0)
                _same_scores(c[p], s[p], rc, rs)
                _same_record(best[p], rbest)
    finally:
        mc.set_dlt_mode(0)


# ------------------------------------------------------------------ 2. round == oracle
@pytest.mark.parametrize("kind", ["H", "F"])
def test_round_equals_oracle(usac, oracle, problems, kind):
    sets, mc, singles = problems[kind]
    R, f = 128, 64
    c, s, _ = mc.hypothesize_score(R, SEEDS, first_hyp=f, thr=THR)
    for p, ctx in enumerate(singles):
        samples = ctx.draw_samples(R, SEEDS[p], first_hyp=f)
        est = oracle.Estimator(oracle.HOMOGRAPHY if kind == "H" else oracle.FUNDAMENTAL, sets[p])
        om, nm = est.estimate_batch(samples)
        oc, osum = est.score_models(om, THR)
        if kind == "F":
            empty = (np.arange(3)[None, :] >= nm[:, None]).reshape(-1)
            oc = np.where(empty, -1, oc)
        _same_scores(c[p], s[p], oc, osum)


# ------------------------------------------------------------------ 3. active list
@pytest.mark.parametrize("kind", ["H", "F"])
def test_active_list_and_duplicate_problem(usac, problems, kind):
    _, mc, _ = problems[kind]
    R = 64
    c, s, best = mc.hypothesize_score(R, SEEDS, first_hyp=R, thr=THR)
    act = [4, 0, 2]
    ca, sa, ba = mc.hypothesize_score(R, [SEEDS[p] for p in act], first_hyp=R, thr=THR, problems=act)
    assert ca.shape == (3, R * mc.spk)
    for i, p in enumerate(act):
        np.testing.assert_array_equal(ca[i], c[p])
        np.testing.assert_array_equal(_bits(sa[i]), _bits(s[p]))
        _same_record(ba[i], best[p])
    # the copy of the 333-point set: same seed, same output; another seed, another output
    d, o = DUP
    np.testing.assert_array_equal(c[d], c[o])
    np.testing.assert_array_equal(_bits(s[d]), _bits(s[o]))
    _same_record(best[d], best[o])
    c2, s2, _ = mc.hypothesize_score(R, [SEEDS[o], SEEDS[o] + 1], first_hyp=R, thr=THR, problems=[o, d])
    np.testing.assert_array_equal(c2[0], c[o])
    assert (c2[1] != c2[0]).any() or (_bits(s2[1]) != _bits(s2[0])).any()
    # per_hypothesis=False returns the records alone
    cn, sn, bn = mc.hypothesize_score(R, SEEDS, first_hyp=R, thr=THR, per_hypothesis=False)
    assert cn is None and sn is None
    for p in range(mc.P):
        _same_record(bn[p], best[p])


# ------------------------------------------------------------------ 4. host samples, fall-backs
def test_host_samples_and_dlt_fallbacks(usac, oracle):
    sets = _sets("H")
    big = sets[4] = sets[4].copy()
    big[17] = 0.0
    big[18] = 0.0
    big[19] = [np.inf, 1.0, 2.0, 3.0]
    R = 128
    samples = [oracle.uniform_samples(40 + p, len(pts), 4, R) for p, pts in enumerate(sets)]
    # the degenerate rows of test_dlt4_qr_fallbacks_bit_exact: repeated points (rank-deficient rows),
    # all-zero points (a zero column norm), a non-finite point
    samples[4][:64] = [[5, 5, 9, 13], [17, 18, 17, 18], [17, 18, 20, 21], [19, 1, 2, 3]] * 16
    samples[4][64:, 1] = samples[4][64:, 0]
    H = usac.ESTIMATOR.Homography
    with usac.MultiContext(H, sets) as mc:
        c, s, best = mc.hypothesize_score(R, thr=THR, samples=np.stack(samples))
        for p, pts in enumerate(sets):
            est = oracle.Estimator(oracle.HOMOGRAPHY, pts)
            om, _ = est.estimate_batch(samples[p])
            oc, osum = est.score_models(om, THR)
            _same_scores(c[p], s[p], oc, osum)
            with usac.Context(H, pts) as ctx:
                rc, rs, rbest = ctx.hypothesize_score(samples=samples[p], thr=THR)
            _same_scores(c[p], s[p], rc, rs)
            _same_record(best[p], rbest)
            order = sorted(range(R), key=lambda i: (-oc[i], -osum[i], i))
            assert best[p]["hyp_index"] == order[0]
            np.testing.assert_array_equal(_bits(best[p]["model"]), _bits(om[order[0]]))
        bad = np.stack(samples)
        bad[1, 5, 2] = len(sets[1])  # one past problem 1's last point (a valid index of problem 4)
        with pytest.raises(usac.UsacError) as e:
            mc.hypothesize_score(R, thr=THR, samples=bad)
        assert e.value.code == -1
        for R_bad in (0, 32, 96, 8192 + 64):
            with pytest.raises(usac.UsacError) as e:
                mc.hypothesize_score(R_bad, SEEDS, thr=THR)
            assert e.value.code == -1


# ------------------------------------------------------------------ 5. run
def _record(usac, d):
    return usac.Record(d["hyp_index"], d["inliers"], d["score"], (ctypes.c_float * 9)(*d["model"].tolist()), int(d["valid"]))


def _restated_run(usac, ctx, m, seed, R, max_iters, prob, dlt):
    """usac_multi_run's loop for one problem, over a single context."""
    ctx.set_dlt_mode(dlt)
    best, r = None, 0
    while True:
        rec = _record(usac, ctx.hypothesize_score(B=R, seed=seed, first_hyp=r * R, thr=THR, per_hypothesis=True)[2])
        best = rec if best is None else usac.merge_records([best, rec])
        bound = usac.std_termination(best.inliers, ctx.n, m, prob, max_iters)
        r += 1
        if r * R >= min(max_iters, bound):
            break
    ctx.set_dlt_mode(0)
    return {"best": best.as_dict(), "rounds": r, "hypotheses": r * R, "bound": bound,
            "status": 0 if best.inliers > 0 else -111}


RUN_R, RUN_MAX, RUN_PROB = 64, 512, 0.95


def _run_model(usac, kind, dlt):
    est = usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental
    model = usac.Model(THR, 4 if kind == "H" else 7, RUN_PROB, 5, est, usac.SAMPLER.Uniform)
    model.max_iterations = RUN_MAX
    model.batch = RUN_R
    model.seed = 100
    model.setDLTMode(dlt)
    return model


@pytest.fixture(scope="module")
def runs(usac, problems):
    """(kind, dlt) -> (usac_multi_run's outputs, the restated loop's) with the default seeds"""
    out = {}
    for kind, dlt in (("H", 0), ("H", 1), ("F", 0)):
        _, mc, singles = problems[kind]
        model = _run_model(usac, kind, dlt)
        ref = [_restated_run(usac, ctx, mc.m, model.seed + p, RUN_R, RUN_MAX, RUN_PROB, dlt)
               for p, ctx in enumerate(singles)]
        out[kind, dlt] = (mc.run(model), ref)
    return out


@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_run_equals_restated_loop(usac, problems, runs, kind, dlt):
    got, ref = runs[kind, dlt]
    # the inputs make the active list shrink: the 0.9-ratio problem ends after one round, the
    # problem without inliers runs to max_iterations (its bound is clamped to 512)
    assert ref[0]["rounds"] == 1
    assert ref[3]["rounds"] == RUN_MAX // RUN_R and ref[3]["bound"] >= RUN_MAX
    for p in range(len(ref)):
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert got[p][key] == ref[p][key], (p, key, got[p], ref[p])
        _same_record(got[p]["best"], ref[p]["best"])
    # explicit seeds: the same run
    _, mc, _ = problems[kind]
    model = _run_model(usac, kind, dlt)
    again = mc.run(model, seeds=[model.seed + p for p in range(mc.P)])
    for p in range(mc.P):
        assert again[p]["rounds"] == got[p]["rounds"]
        _same_record(again[p]["best"], got[p]["best"])


def test_run_rejects_what_it_does_not_do(usac, problems):
    _, mc, _ = problems["H"]
    for change in ("sprt", "lo", "sampler", "batch"):
        model = _run_model(usac, "H", 0)
        if change == "sprt":
            model.setSprt(True)
        elif change == "lo":
            model.lo = usac.LocOpt.InItLORsc
        elif change == "sampler":
            model.sampler = usac.SAMPLER.Prosac
        else:
            model.batch = 100
        with pytest.raises(usac.UsacError) as e:
            mc.run(model)
        assert e.value.code == (-1 if change == "batch" else -3)


# ------------------------------------------------------------------ 6. inliers
@pytest.mark.parametrize("kind,dlt", [("H", 1), ("F", 0)])
def test_inliers_equal_single_context(usac, problems, runs, kind, dlt):
    _, mc, singles = problems[kind]
    models = np.stack([r["best"]["model"] for r in runs[kind, dlt][0]])
    got = mc.inliers(models, THR)
    assert len(got) == mc.P
    total = 0
    for p, ctx in enumerate(singles):
        n, _, idx = ctx.get_inliers(models[p], THR)
        assert len(got[p]) == n
        np.testing.assert_array_equal(got[p], idx)
        total += n
    assert total > 0
