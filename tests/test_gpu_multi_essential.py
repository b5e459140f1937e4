"""Multi contexts of essential-matrix problems (usac_multi_create_essential, MultiContext.essential,
ABI 21).  Every per-problem output is compared bit for bit -- counts, the int32 views of sums and
models, indices -- with the single-problem path (Context(Essential) over the problem's points) and
with the CPU oracle: a round, the active list, host samples, the solve's slicing, the samplers, the
run, the masks, the polish, the PROSAC run and the refusals."""
import ctypes
import os

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import multi_polish_ref as polref
from tests.helpers import prosac_ref as ref

pytestmark = pytest.mark.gpu

THR = 0.002
# the smallest shapes that reach n_p = m, one point past a wave, a problem without structure and a
# 4-way unrolled walk with a remainder
SIZES = [5, 8, 64, 65, 333, 1000]
RATIOS = [1.0, 0.9, 0.5, 0.3, 0.0, 0.5]
DATA_SEEDS = [40, 42, 41, 43, 44, 45]
DUP = (6, 4)                           # problem 6 is a copy of problem 4 (the 333-point set)
SEEDS = [11, 12, 13, 14, 15, 16, 15]   # sampler seeds: the copy shares its original's
M = 5


def _sets(prosac_order=False, sizes=SIZES):
    out = []
    for n, ratio, seed in zip(SIZES, RATIOS, DATA_SEEDS):
        if n in sizes:
            out.append(synthetic.fundamental_points(n=n, inlier_ratio=ratio, seed=seed, noise=0.5, normalized=True,
                                                    prosac_order=prosac_order)[0])
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
    """(point sets, the essential MultiContext, the single contexts)"""
    sets = _sets()
    sets.append(sets[DUP[1]].copy())
    E = usac.ESTIMATOR.Essential
    mc = usac.MultiContext.essential(sets)
    singles = [usac.Context(E, p) for p in sets]
    yield sets, mc, singles
    mc.close()
    for c in singles:
        c.close()


@pytest.fixture(scope="module")
def single_rounds(problems):
    """(R, first_hyp) -> per problem the single context's (counts, sums, best) of that round"""
    _, _, singles = problems
    cache = {}

    def get(R, f):
        if (R, f) not in cache:
            cache[R, f] = [ctx.hypothesize_score(B=R, seed=SEEDS[p], first_hyp=f, thr=THR, per_hypothesis=True)
                           for p, ctx in enumerate(singles)]
        return cache[R, f]

    return get


def _assert_round(mc_out, want):
    c, s, best = mc_out
    for p, (rc, rs, rbest) in enumerate(want):
        _same_scores(c[p], s[p], rc, rs)
        _same_record(best[p], rbest)


# ------------------------------------------------------------------ 1. round == single context
@pytest.mark.parametrize("R", [64, 128])
def test_round_equals_single_context(usac, problems, single_rounds, R):
    sets, mc, _ = problems
    assert mc.m == M and mc.spk == 1 and mc.estimator == usac.ESTIMATOR.Essential
    occupied = 0
    for f in (0, 3 * R):
        out = mc.hypothesize_score(R, SEEDS, first_hyp=f, thr=THR)
        assert out[0].shape == (len(sets), R)
        _assert_round(out, single_rounds(R, f))
        occupied += int((out[0] >= 0).sum())
    assert occupied > 0


# ------------------------------------------------------------------ 2. round == oracle
def test_round_equals_oracle(usac, oracle, problems):
    sets, mc, singles = problems
    R, f = 128, 64
    c, s, _ = mc.hypothesize_score(R, SEEDS, first_hyp=f, thr=THR)
    occupied = several = 0
    for p, ctx in enumerate(singles[:len(SIZES)]):
        samples = ctx.draw_samples(R, SEEDS[p], first_hyp=f)
        est = oracle.Estimator(oracle.ESSENTIAL, sets[p])
        om, nm = est.estimate_batch(samples)
        oc, osum = est.score_models(om, THR)
        oc = np.where(nm == 0, -1, oc)
        _same_scores(c[p], s[p], oc, osum)
        occupied += int((nm > 0).sum())
        several += sum(1 for smp in samples if int(est.e5_candidates(smp)[1].sum()) > 1)
    # the comparison is not vacuous: models exist, and the candidate order decides many of them
    assert occupied >= 300, occupied
    assert several >= 100, several


# ------------------------------------------------------------------ 3. active list
def test_active_list_and_duplicate_problem(usac, problems):
    _, mc, _ = problems
    R = 64
    c, s, best = mc.hypothesize_score(R, SEEDS, first_hyp=R, thr=THR)
    act = [5, 0, 2]
    ca, sa, ba = mc.hypothesize_score(R, [SEEDS[p] for p in act], first_hyp=R, thr=THR, problems=act)
    assert ca.shape == (3, R)
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


# ------------------------------------------------------------------ 4. host samples
def test_host_samples_and_degenerate_samples(usac, oracle):
    sets = _sets()
    big = sets[5] = sets[5].copy()
    big[17:22, 2] = big[17, 2]                   # five points that share one coordinate
    big[30] = [np.inf, 0.1, 0.2, 0.3]            # a non-finite point: no Householder norm
    R = 128
    samples = [oracle.uniform_samples(40 + p, len(pts), M, R) for p, pts in enumerate(sets)]
    samples[5][:4] = [[17, 18, 19, 20, 21], [30, 1, 2, 3, 4], [7, 7, 9, 11, 13], [21, 20, 19, 18, 17]]
    E = usac.ESTIMATOR.Essential
    with usac.MultiContext.essential(sets) as mc:
        c, s, best = mc.hypothesize_score(R, thr=THR, samples=np.stack(samples))
        for p, pts in enumerate(sets):
            est = oracle.Estimator(oracle.ESSENTIAL, pts)
            om, nm = est.estimate_batch(samples[p])
            oc, osum = est.score_models(om, THR)
            oc = np.where(nm == 0, -1, oc)
            _same_scores(c[p], s[p], oc, osum)
            with usac.Context(E, pts) as ctx:
                rc, rs, rbest = ctx.hypothesize_score(samples=samples[p], thr=THR)
            _same_scores(c[p], s[p], rc, rs)
            _same_record(best[p], rbest)
            order = sorted((i for i in range(R) if nm[i]), key=lambda i: (-oc[i], -osum[i], i))
            if order:
                assert best[p]["hyp_index"] == order[0]
                np.testing.assert_array_equal(_bits(best[p]["model"]), _bits(om[order[0]]))
            else:
                assert not best[p]["valid"]
        bad = np.stack(samples)
        bad[1, 5, 2] = len(sets[1])  # one past problem 1's last point (a valid index of problem 5)
        with pytest.raises(usac.UsacError) as e:
            mc.hypothesize_score(R, thr=THR, samples=bad)
        assert e.value.code == -1


# ------------------------------------------------------------------ 5. slicing
@pytest.mark.parametrize("cap", [128, 200, 300])
def test_results_do_not_depend_on_the_solve_slice(usac, problems, single_rounds, cap):
    """7 entries x 128 samples: cap 128 and 200 (rounded down to whole entries) solve one entry per
    slice, 300 two per slice with a last slice of one"""
    sets, _, _ = problems
    R = 128
    old = os.environ.get("USAC_MULTI_E5_SLICE")
    os.environ["USAC_MULTI_E5_SLICE"] = str(cap)
    try:
        mc = usac.MultiContext.essential(sets)
    finally:
        if old is None:
            del os.environ["USAC_MULTI_E5_SLICE"]
        else:
            os.environ["USAC_MULTI_E5_SLICE"] = old
    with mc:
        for f in (0, 3 * R):
            _assert_round(mc.hypothesize_score(R, SEEDS, first_hyp=f, thr=THR), single_rounds(R, f))


# ------------------------------------------------------------------ 6. samplers
def test_draw_samples(usac, problems):
    _, mc, singles = problems
    R = 64
    for f in (0, 3 * R):
        got = mc.draw_samples(R, SEEDS, first_hyp=f)
        assert got.shape == (mc.P, R, M)
        for p, ctx in enumerate(singles):
            np.testing.assert_array_equal(got[p], ctx.draw_samples(R, SEEDS[p], first_hyp=f))
    # the PROSAC sampler: usac_prosac_schedule and the restated rule (tests/helpers/prosac_ref.py)
    cases = []  # (problem, clock, term_len, first_hyp)
    for p, L in ((4, 100), (5, 400), (3, 30)):
        n = int(mc.sizes[p])
        g = ref.growth_table(n, M)
        t_max = g[L - 1] + 1  # the last clock value whose lane is a PROSAC lane
        assert t_max > 20
        cases.append((p, t_max - 20, L, 128))    # 21 PROSAC lanes, then frozen over [0, L]
        cases.append((p, t_max + 1, L, 64))      # frozen throughout
        cases.append((p, ref.T_N - 5, n, 0))     # 6 PROSAC lanes, then uniform over n
        cases.append((p, 1, n, 0))               # the start of a run
    for p, clock, L, f in cases:
        n = int(mc.sizes[p])
        sub, _, _ = usac.prosac_schedule(n, M, clock, L, R)
        got = mc.draw_samples(R, [SEEDS[p]], first_hyp=f, problems=[p], clock=[clock], term_len=[L])[0]
        np.testing.assert_array_equal(got, ref.multi_prosac_samples(SEEDS[p], f, R, n, M, clock, L))
        assert (got >= 0).all() and (got < n).all()
        assert all(len(set(row)) == M for row in got.tolist())
        pro = (sub != 0) & (sub != usac.UNIFORM_OVER_N)
        np.testing.assert_array_equal(got[pro][:, M - 1], sub[pro].astype(np.int64) - 1)
    for bad in ({"clock": [0]}, {"clock": [1], "term_len": [M - 1]}, {"clock": [1], "term_len": [334]}):
        with pytest.raises(usac.UsacError) as e:
            mc.draw_samples(R, [1], problems=[4], **bad)
        assert e.value.code == -1


# ------------------------------------------------------------------ 7. run
def _record(usac, d):
    return usac.Record(d["hyp_index"], d["inliers"], d["score"], (ctypes.c_float * 9)(*d["model"].tolist()), int(d["valid"]))


def _restated_run(usac, ctx, m, seed, R, max_iters, prob):
    """usac_multi_run's loop for one problem, over a single context."""
    best, r = None, 0
    while True:
        rec = _record(usac, ctx.hypothesize_score(B=R, seed=seed, first_hyp=r * R, thr=THR, per_hypothesis=True)[2])
        best = rec if best is None else usac.merge_records([best, rec])
        bound = usac.std_termination(best.inliers, ctx.n, m, prob, max_iters)
        r += 1
        if r * R >= min(max_iters, bound):
            break
    return {"best": best.as_dict(), "rounds": r, "hypotheses": r * R, "bound": bound,
            "status": 0 if best.inliers > 0 else -111}


RUN_R, RUN_MAX, RUN_PROB = 64, 2048, 0.95


def _run_model(usac, sampler=None, R=RUN_R):
    model = usac.Model(THR, M, RUN_PROB, 5, usac.ESTIMATOR.Essential, sampler or usac.SAMPLER.Uniform)
    model.max_iterations = RUN_MAX
    model.batch = R
    model.seed = 100
    return model


@pytest.fixture(scope="module")
def runs(usac, problems):
    """(usac_multi_run's outputs, the restated loop's) with the default seeds"""
    _, mc, singles = problems
    model = _run_model(usac)
    want = [_restated_run(usac, ctx, M, model.seed + p, RUN_R, RUN_MAX, RUN_PROB) for p, ctx in enumerate(singles)]
    return mc.run(model), want


def test_run_equals_restated_loop(usac, problems, runs):
    got, want = runs
    # the 5-point all-inlier problem ends after one round with bound 0
    assert want[0]["rounds"] == 1 and want[0]["bound"] == 0 and want[0]["best"]["inliers"] == 5
    assert any(w["rounds"] > 1 for w in want)
    for p in range(len(want)):
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert got[p][key] == want[p][key], (p, key, got[p], want[p])
        _same_record(got[p]["best"], want[p]["best"])
        assert (got[p]["status"] == -111) == (want[p]["best"]["inliers"] == 0)
    # explicit seeds: the same run
    _, mc, _ = problems
    model = _run_model(usac)
    again = mc.run(model, seeds=[model.seed + p for p in range(mc.P)])
    for p in range(mc.P):
        assert again[p]["rounds"] == got[p]["rounds"]
        _same_record(again[p]["best"], got[p]["best"])


# ------------------------------------------------------------------ 8. inliers
def test_inliers_equal_single_context(usac, problems, runs):
    _, mc, singles = problems
    models = np.stack([r["best"]["model"] for r in runs[0]])
    got = mc.inliers(models, THR)
    assert len(got) == mc.P
    total = 0
    for p, ctx in enumerate(singles):
        n, _, idx = ctx.get_inliers(models[p], THR)
        assert len(got[p]) == n
        np.testing.assert_array_equal(got[p], idx)
        total += n
    assert total > 0


# ------------------------------------------------------------------ 9. polish
class _SingleEstimator:
    """tests/helpers/multi_polish_ref.py's estimator interface over a single context: the loop
    get_inliers / nonminimal of ransac.cpp:157-214 runs on Context(Essential)"""

    def __init__(self, usac, ctx):
        self.usac, self.ctx = usac, ctx

    def quality(self, model, thr, with_inliers=False):
        c, s, idx = self.ctx.get_inliers(model, thr)
        return (c, s, idx) if with_inliers else (c, s)

    def nonminimal(self, idx):
        try:
            return self.ctx.nonminimal(idx)
        except self.usac.UsacError as e:
            if e.code != -111:
                raise
            return None


def test_polish_equals_single_context_loop(usac, problems, runs):
    _, mc, singles = problems
    got_run = runs[0]
    models = np.stack([r["best"]["model"] for r in got_run])
    want = [polref.polish_ref(_SingleEstimator(usac, ctx), models[p], THR) for p, ctx in enumerate(singles)]
    got = mc.polish(models, THR, with_inliers=True)
    for p in range(mc.P):
        polref.assert_same_polish(got[p], want[p], p)
    # the 5- and 8-point problems refit lists below 8 points
    assert 0 < want[0]["sizes"][0] < 8 and 0 < want[1]["sizes"][0] <= 8
    assert any(w["passes"] > 0 for w in want)
    # run(polish=True): the same run, then the polish of its best models and their masks
    pol = mc.run(_run_model(usac), polish=True)
    for p in range(mc.P):
        _same_record(pol[p]["best"], got_run[p]["best"])
        polref.assert_same_polish(pol[p]["polished"], want[p], p)
        np.testing.assert_array_equal(pol[p]["inliers"], want[p]["inlier_idx"])


# ------------------------------------------------------------------ 10. PROSAC run
def _restated_prosac_run(usac, mc, ctx, p, seed, R):
    """usac_multi_run_prosac's loop for problem p: the multi context only draws the samples"""
    n, m = ctx.n, mc.m
    scan = ref.PlainScan(n, m, lambda c, pts: usac.std_termination(c, pts, m, RUN_PROB, RUN_MAX))
    T, L, largest, bound, best, r, scans = 1, n, m, RUN_MAX, None, 0, 0
    while True:
        first = r * R
        samples = mc.draw_samples(R, [seed], first_hyp=first, problems=[p], clock=[T], term_len=[L])[0]
        d = ctx.hypothesize_score(samples=samples, thr=THR)[2]
        d["hyp_index"] += first
        rec = _record(usac, d)
        best = rec if best is None else usac.merge_records([best, rec])
        sub, T_next, largest_next = usac.prosac_schedule(n, m, T, L, R, largest)
        k = T_next - T  # PROSAC lanes
        if best.valid and best.hyp_index >= first:  # a new best: scan it
            j = best.hyp_index - first
            at = max(largest, int(sub[min(j, k - 1)])) if k else largest
            cnt, _, idx = ctx.get_inliers(np.array(best.model[:], dtype=np.float32), THR)
            flags = np.zeros(n, dtype=bool)
            flags[idx] = True
            bound, _ = scan.scan(best.hyp_index, flags, at)
            L = scan.term_len
            scans += 1
        T, largest = T_next, largest_next
        r += 1
        if r * R >= min(RUN_MAX, bound):
            break
    return {"best": best.as_dict(), "rounds": r, "hypotheses": r * R, "bound": bound,
            "status": 0 if best.inliers > 0 else -111, "termination_length": L, "largest_sample_size": largest,
            "clock": T, "scans": scans}


def test_run_prosac_equals_restated_loop(usac):
    sets = _sets(prosac_order=True, sizes=[64, 65, 333, 1000])
    E = usac.ESTIMATOR.Essential
    R = 64
    model = _run_model(usac, usac.SAMPLER.Prosac, R)
    with usac.MultiContext.essential(sets) as mc:
        got = mc.run_prosac(model)
        for p, pts in enumerate(sets):
            with usac.Context(E, pts) as ctx:
                want = _restated_prosac_run(usac, mc, ctx, p, model.seed + p, R)
            for key in ("rounds", "hypotheses", "bound", "status", "termination_length", "largest_sample_size", "clock",
                        "scans"):
                assert got[p][key] == want[key], (p, key, got[p], want)
            _same_record(got[p]["best"], want["best"])
        assert any(g["scans"] > 0 for g in got)
        # pol / mask: the same run, then the polish of its best models
        pol = mc.run_prosac(model, polish=True)
        wantp = mc.polish(np.stack([r["best"]["model"] for r in got]), THR, with_inliers=True)
        for p in range(mc.P):
            _same_record(pol[p]["best"], got[p]["best"])
            polref.assert_same_polish(pol[p]["polished"], wantp[p], p)
            np.testing.assert_array_equal(pol[p]["inliers"], wantp[p]["inlier_idx"])
        with pytest.raises(usac.UsacError) as e:
            mc.run(model)                      # usac_multi_run still refuses a PROSAC model
        assert e.value.code == -3
    with usac.MultiContext.essential([sets[3], sets[3][:20]]) as small:  # n_p = 20
        with pytest.raises(usac.UsacError) as e:
            small.run_prosac(model)
        assert e.value.code == -1


# ------------------------------------------------------------------ 11. refusals
def test_refusals_name_the_essential_estimator(usac, problems):
    _, mc, _ = problems
    lo = _run_model(usac)
    lo.lo = usac.LocOpt.InItLORsc
    sprt = _run_model(usac)
    sprt.setSprt(True)
    nap = _run_model(usac, usac.SAMPLER.Napsac)
    nap.setCellSize(50)
    recs = [usac.Record() for _ in range(mc.P)]
    calls = [lambda: mc.run_lo(lo), lambda: mc.lo(lo, recs), lambda: mc.run_sprt(sprt),
             lambda: mc.hypothesize_score_sprt(64, SEEDS, thr=THR), lambda: mc.set_sprt_pool(),
             lambda: mc.grid_neighbors(50), lambda: mc.run_napsac(nap),
             lambda: mc.draw_samples_napsac(64, SEEDS, 50), lambda: mc.hypothesize_score_napsac(64, SEEDS, 50, thr=THR)]
    for call in calls:
        with pytest.raises(usac.UsacError) as e:
            call()
        assert e.value.code == -3
        assert b"essential" in usac.lib().usac_multi_last_error(mc._h)
    # and usac_multi_run refuses what it refuses for H / F
    for model in (lo, sprt, nap):
        with pytest.raises(usac.UsacError) as e:
            mc.run(model)
        assert e.value.code == -3
