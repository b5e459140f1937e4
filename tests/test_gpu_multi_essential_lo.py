"""LO-RANSAC on multi contexts of essential-matrix problems (usac_multi_lo_essential,
usac_multi_run_lo_essential; ABI 23) on the device: the LO kernel through its hook against the restatement
over the CPU oracle (tests/helpers/multi_lo_ref.py's lo_ref over the oracle's essential estimator) and
against the single-context LocalOptimization, the caps rule, the run against its loop restated over single
contexts, the solve's slicing, per-problem thresholds and the refusals -- all without any tolerance."""
import ctypes
import os

import numpy as np
import pytest

from tests.helpers import multi_essential_lo_ref as eref
from tests.helpers import multi_lo_ref as ref
from tests.helpers import multi_polish_ref as pref
from tests.helpers import prosac_ref

pytestmark = pytest.mark.gpu

THR, M = eref.THR, eref.M


@pytest.fixture(scope="module")
def hook(usac, oracle):
    """(point sets, the essential MultiContext, oracle estimators, start records, draw seeds): the sizes of
    multi_lo_ref.SIZES with the copy of the 333-point set, which shares its original's start and seed"""
    sets, ests, recs, seeds = eref.hook_problems(oracle)
    mc = usac.MultiContext.essential(sets)
    yield sets, mc, ests, recs, seeds
    mc.close()


def _assert_calls(got, want, what):
    """a lo_essential result (records, states) against one call of eref.ref_calls"""
    for p, (rec, st, _) in enumerate(want):
        ref.assert_same_record(got[0][p], rec, (what, p))
        ref.assert_same_state(got[1][p], st, (what, p))


# ------------------------------------------------------------------ 1. the hook == the restatement
@pytest.mark.parametrize("limited", [False, True])
def test_hook_equals_restatement(usac, hook, limited):
    sets, mc, ests, recs, seeds = hook
    model = eref.make_model(usac, limited)
    prm = ref.from_model(model, M)
    want = eref.ref_calls(usac, ests, recs, seeds, prm, 2)
    got1 = mc.lo_essential(model, recs, seeds=seeds, reset=True)
    got2 = mc.lo_essential(model, got1[0], seeds=seeds, reset=False)  # continues the draw counter and the threshold
    got3 = mc.lo_essential(model, recs, seeds=seeds, reset=True)      # repeats the first
    _assert_calls(got1, want[0], (limited, 1))
    _assert_calls(got2, want[1], (limited, 2))
    for p in range(mc.P):
        what = (limited, p, len(sets[p]))
        ref.assert_same_record(got3[0][p], got1[0][p], what)
        ref.assert_same_state(got3[1][p], got1[1][p], what)
        # the invariant: no record is worse than its input; below the floor it comes back as it went in
        assert not ref.bigger(recs[p]["inliers"], recs[p]["score"], got1[0][p]["inliers"], got1[0][p]["score"]), what
        assert got1[0][p]["hyp_index"] == recs[p]["hyp_index"]
        if recs[p]["inliers"] < 12:
            ref.assert_same_record(got1[0][p], recs[p], what)
            assert got1[1][p]["fits"] == 0 and got1[1][p]["lo_calls"] == 1
    d, o = eref.DUP
    ref.assert_same_record(got1[0][d], got1[0][o])
    ref.assert_same_state(got2[1][d], got2[1][o])
    st1, st2 = got1[1], got2[1]
    assert any(s["draws"] > 0 for s in st1) and any(a["draws"] > b["draws"] > 0 for a, b in zip(st2, st1))
    assert any(r["inliers"] < 12 for r in recs)
    assert any(g["inliers"] > 2 * r["inliers"] for g, r in zip(got1[0], recs))


# ------------------------------------------------------------------ 2. the hook, remaining cases
def test_hook_degenerate_set_takes_the_sample_size_continue(usac, oracle):
    """14 copies of one correspondence: in some inner iterations the fitted model has <= 5 inliers (the
    `<= m` continue reads the essential sample size: with 7 or 4 the counters differ)"""
    pts, rec = eref.few_problem(oracle)
    model = eref.make_model(usac)
    prm = ref.from_model(model, M)
    want_rec, want_st, tally = ref.lo_ref(usac, eref.estimator(oracle, pts), rec, ref.fresh_state(prm), 909, prm)
    assert rec["inliers"] == 16 and 0 < tally["few"] < prm.inner
    with usac.MultiContext.essential([pts]) as mc:
        got, st = mc.lo_essential(model, [rec], seeds=[909])
    ref.assert_same_record(got[0], want_rec)
    ref.assert_same_state(st[0], want_st)
    assert st[0]["inner_iters"] == prm.inner - tally["few"] and st[0]["draws"] == prm.inner


def test_hook_threshold_with_inexact_steps(usac, oracle, hook):
    """θ = 0.0017, three iterative steps: a completed stage leaves the threshold within 1e-5 of θ but not at
    its bits, and the next call starts from there"""
    sets, mc, ests, _, seeds = hook
    model = eref.make_model(usac, thr=0.0017, iters=3)
    prm = ref.from_model(model, M)
    recs = [eref.start_record(oracle, p, eref.START_SEED + i, est=e, thr=0.0017) for i, (p, e) in enumerate(zip(sets, ests))]
    recs[eref.DUP[0]] = dict(recs[eref.DUP[1]])
    want = eref.ref_calls(usac, ests, recs, seeds, prm, 2)
    got1 = mc.lo_essential(model, recs, seeds=seeds, reset=True)
    got2 = mc.lo_essential(model, got1[0], seeds=seeds, reset=False)
    _assert_calls(got1, want[0], 1)
    _assert_calls(got2, want[1], 2)
    t = got1[1][5]["threshold"]
    assert pref.bits(t) != pref.bits(np.float32(0.0017)) and abs(float(t) - 0.0017) < 1e-5


def test_hook_leaves_invalid_and_small_records_alone(usac, hook):
    sets, mc, ests, recs, seeds = hook
    model = eref.make_model(usac)
    given = [dict(r) for r in recs]
    given[4] = dict(recs[4], valid=False)                                   # not valid: no LO call
    given[5] = dict(recs[5], inliers=11)                                    # below the 12-inlier floor
    got, st = mc.lo_essential(model, given, seeds=seeds)
    for p in (4, 5):
        ref.assert_same_record(got[p], given[p], p)
        assert st[p]["fits"] == 0 and st[p]["draws"] == 0
    assert st[4]["lo_calls"] == 0 and st[5]["lo_calls"] == 1
    want = eref.ref_calls(usac, ests, given, seeds, ref.from_model(model, M), 1)
    _assert_calls((got, st), want[0], "given")


# ------------------------------------------------------------------ 3. the caps rule
def test_hook_caps(usac, oracle, hook):
    all_sets, _, all_ests, all_recs, _ = hook
    pts, rec = eref.cap_problem(oracle)
    sets = [all_sets[4], pts, all_sets[5]]
    ests = [all_ests[4], eref.estimator(oracle, pts), all_ests[5]]
    recs = [all_recs[4], rec, all_recs[5]]
    seeds = [31, 32, 33]
    model = eref.make_model(usac)
    want = eref.ref_calls(usac, ests, recs, seeds, ref.from_model(model, M), 1)[0]
    with usac.MultiContext.essential(sets) as mc:
        got, st = mc.lo_essential(model, recs, seeds=seeds)
    _assert_calls((got, st), want, "caps")
    assert st[1]["capped"] == 1 and st[1]["fits"] == 1 and st[1]["inner_iters"] == 0
    assert st[0]["capped"] == st[2]["capped"] == 0
    assert pref.bits(st[1]["threshold"]) == pref.bits(np.float32(THR))
    ref.assert_same_record(got[1], rec)
    # the neighbours are what they are without the capped problem in the launch
    with usac.MultiContext.essential([sets[0], sets[2]]) as mc:
        alone, st_alone = mc.lo_essential(model, [recs[0], recs[2]], seeds=[31, 33])
    for a, p in enumerate((0, 2)):
        ref.assert_same_record(alone[a], got[p])
        ref.assert_same_state(st_alone[a], st[p])


# ------------------------------------------------------------------ 4. pinned to the single-context LO
def test_hook_equals_single_context_lo_without_draws(usac, hook):
    """lo_sample_size >= n_p: no inner iteration draws, so the unlimited variant is the single context's
    LocalOptimization.GetModelScore on the same points and start record"""
    sets, mc, _, recs, seeds = hook
    model = eref.make_model(usac, sample_size=64)
    got, st = mc.lo_essential(model, recs, seeds=seeds, reset=True)
    checked = 0
    for p, pts in enumerate(sets):
        if len(pts) > 64 or recs[p]["inliers"] < 12:
            continue
        with usac.Context(usac.ESTIMATOR.Essential, pts) as ctx:
            lo = usac.LocalOptimization(ctx, model)
            m = np.array(recs[p]["model"], dtype=np.float32)
            sc = usac.Score(recs[p]["inliers"], recs[p]["score"])
            lo.GetModelScore(m, sc)
            inner, iterative = lo.iters()
            lo.close()
        what = (p, len(pts))
        np.testing.assert_array_equal(pref.bits(got[p]["model"]), pref.bits(m), err_msg=str(what))
        assert got[p]["inliers"] == sc.inlier_number, what
        assert pref.bits(got[p]["score"]) == pref.bits(np.float32(sc.score)), what
        assert (st[p]["inner_iters"], st[p]["iterative_iters"]) == (inner, iterative), what
        assert st[p]["draws"] == 0
        checked += 1
    assert checked >= 2


# ------------------------------------------------------------------ 5. run_lo_essential == its restated loop
RUN_MAX, R = 1024, 64


def _run_model(usac, sampler=None, limited=False, thr=THR):
    model = eref.make_model(usac, limited, sampler=sampler, thr=thr)
    model.max_iterations = RUN_MAX
    model.batch = R
    return model


def _record(usac, d):
    return usac.Record(d["hyp_index"], d["inliers"], float(d["score"]), (ctypes.c_float * 9)(*np.asarray(d["model"]).tolist()),
                       int(d["valid"]))


def _restated_run(usac, mc, ctx, est, p, seed, prm, prosac):
    """usac_multi_run_lo_essential's loop for problem p over a single context (the multi context only draws
    the samples), with the LO restatement at each improving round"""
    n, m, thr = ctx.n, mc.m, float(prm.thr)
    scan = prosac_ref.PlainScan(n, m, lambda c, pts: usac.std_termination(c, pts, m, 0.95, RUN_MAX))
    T, L, largest, bound, best, r, scans = 1, n, m, RUN_MAX, None, 0, 0
    st = ref.fresh_state(prm)
    while True:
        first = r * R
        if prosac:
            samples = mc.draw_samples(R, [seed], first_hyp=first, problems=[p], clock=[T], term_len=[L])[0]
        else:
            samples = mc.draw_samples(R, [seed], first_hyp=first, problems=[p])[0]
        d = ctx.hypothesize_score(samples=samples, thr=thr)[2]
        d["hyp_index"] += first
        rec = _record(usac, d)
        best = rec if best is None else usac.merge_records([best, rec])
        new = bool(best.valid) and best.hyp_index >= first
        if new:
            lo_rec, st, _ = ref.lo_ref(usac, est, best.as_dict(), st, seed, prm)
            best = _record(usac, lo_rec)
        if prosac:
            sub, T_next, largest_next = usac.prosac_schedule(n, m, T, L, R, largest)
            k = T_next - T
            if new:
                j = best.hyp_index - first
                at = max(largest, int(sub[min(j, k - 1)])) if k else largest
                _, _, idx = ctx.get_inliers(np.array(best.model[:], dtype=np.float32), thr)
                flags = np.zeros(n, dtype=bool)
                flags[idx] = True
                bound, _ = scan.scan(best.hyp_index, flags, at)
                L = scan.term_len
                scans += 1
            T, largest = T_next, largest_next
        else:
            bound = usac.std_termination(best.inliers, n, m, 0.95, RUN_MAX)
        r += 1
        if r * R >= min(RUN_MAX, bound):
            break
    out = {"best": best.as_dict(), "rounds": r, "hypotheses": r * R, "bound": bound,
           "status": 0 if best.inliers > 0 else -111, "lo": st}
    if prosac:
        out.update(termination_length=L, largest_sample_size=largest, clock=T, scans=scans)
    return out


RUN_KEYS = ["rounds", "hypotheses", "bound", "status"]
PROSAC_KEYS = ["termination_length", "largest_sample_size", "clock", "scans"]


def _assert_run(got, want, keys, what):
    for key in keys:
        assert got[key] == want[key], (what, key, got, want)
    ref.assert_same_record(got["best"], want["best"], what)
    ref.assert_same_state(got["lo"], want["lo"], what)


@pytest.fixture(scope="module")
def run_problems(usac, oracle):
    """(quality-sorted point sets, the essential MultiContext, single contexts, oracle estimators)"""
    sets = eref.run_sets()
    mc = usac.MultiContext.essential(sets)
    singles = [usac.Context(usac.ESTIMATOR.Essential, p) for p in sets]
    yield sets, mc, singles, [eref.estimator(oracle, p) for p in sets]
    mc.close()
    for c in singles:
        c.close()


@pytest.fixture(scope="module")
def uniform_run(usac, run_problems):
    """the unlimited run with the uniform sampler, which the slicing and thresholds tests compare with"""
    _, mc, _, _ = run_problems
    return mc.run_lo_essential(_run_model(usac), polish=True)


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("sampler", ["uniform", "prosac"])
def test_run_equals_restated_loop(usac, run_problems, sampler, limited):
    sets, mc, singles, ests = run_problems
    prosac = sampler == "prosac"
    model = _run_model(usac, usac.SAMPLER.Prosac if prosac else usac.SAMPLER.Uniform, limited)
    prm = ref.from_model(model, M)
    got = mc.run_lo_essential(model, polish=True)
    for p, ctx in enumerate(singles):
        want = _restated_run(usac, mc, ctx, ests[p], p, model.seed + p, prm, prosac)
        _assert_run(got[p], want, RUN_KEYS + (PROSAC_KEYS if prosac else []), (sampler, limited, p))
    assert ("scans" in got[0]) == prosac
    # the inputs exercise the loop: the LO improved on a minimal model and, under the uniform sampler, the
    # poor problem's record improved in more than one round (an LO call each).  PROSAC over quality-sorted
    # sets ends every run here in its first round, after its scan of the LO'd model; its later rounds are
    # test_run_prosac_over_an_unsorted_set's
    assert any(g["lo"]["improved"] > 0 for g in got) and all(g["lo"]["lo_calls"] >= 1 for g in got)
    if prosac:
        assert all(g["scans"] >= 1 for g in got)
    else:
        assert got[3]["lo"]["lo_calls"] > 1 and got[3]["rounds"] > 1
        assert limited or got[3]["lo"]["inner_iters"] > prm.inner  # the inner iterations of more than one call
    # polish=True: mc.polish of the LO'd models
    pol = mc.polish(np.stack([g["best"]["model"] for g in got]), THR, with_inliers=True)
    for p in range(mc.P):
        pref.assert_same_polish(got[p]["polished"], pol[p], p)
        np.testing.assert_array_equal(got[p]["inliers"], pol[p]["inlier_idx"])
    again = mc.run_lo_essential(model)
    for p in range(mc.P):
        _assert_run(again[p], got[p], RUN_KEYS, p)


@pytest.mark.parametrize("limited", [False, True])
def test_run_prosac_over_an_unsorted_set(usac, oracle, limited):
    """the poor problem in generation order: PROSAC needs several rounds, the record improves in two of them,
    and each LO'd record is scanned before the next round's sampler state is taken from it"""
    pts = eref.make_set(*eref.UNSORTED)
    model = _run_model(usac, usac.SAMPLER.Prosac, limited)
    prm = ref.from_model(model, M)
    with usac.MultiContext.essential([pts]) as mc, usac.Context(usac.ESTIMATOR.Essential, pts) as ctx:
        got = mc.run_lo_essential(model)[0]
        want = _restated_run(usac, mc, ctx, eref.estimator(oracle, pts), 0, model.seed, prm, True)
    _assert_run(got, want, RUN_KEYS + PROSAC_KEYS, limited)
    assert got["rounds"] > 1 and got["lo"]["lo_calls"] > 1 and got["scans"] > 1
    assert got["lo"]["inner_iters"] > prm.inner and got["lo"]["improved"] > 0


# ------------------------------------------------------------------ 6. the solve's slicing
def test_run_does_not_depend_on_the_solve_slice(usac, run_problems, uniform_run):
    """4 entries x 64 samples under a cap of 64: one entry per slice, LO after the round's last slice"""
    sets, _, _, _ = run_problems
    old = os.environ.get("USAC_MULTI_E5_SLICE")
    os.environ["USAC_MULTI_E5_SLICE"] = str(R)
    try:
        mc = usac.MultiContext.essential(sets)
    finally:
        if old is None:
            del os.environ["USAC_MULTI_E5_SLICE"]
        else:
            os.environ["USAC_MULTI_E5_SLICE"] = old
    with mc:
        got = mc.run_lo_essential(_run_model(usac))
    for p in range(len(sets)):
        _assert_run(got[p], uniform_run[p], RUN_KEYS, p)


# ------------------------------------------------------------------ 7. per-problem thresholds
def test_equal_thresholds_are_the_scalar_call(usac, hook, run_problems, uniform_run):
    sets, mc, _, recs, seeds = hook
    model = eref.make_model(usac)
    want = mc.lo_essential(model, recs, seeds=seeds)
    far = eref.make_model(usac, thr=0.007)  # the scalar is not read while thresholds are set
    mc.set_thresholds([THR] * mc.P)
    try:
        got = mc.lo_essential(far, recs, seeds=seeds)
    finally:
        mc.set_thresholds(None)
    for p in range(mc.P):
        ref.assert_same_record(got[0][p], want[0][p], p)
        ref.assert_same_state(got[1][p], want[1][p], p)
    _, rmc, _, _ = run_problems
    rmc.set_thresholds([THR] * rmc.P)
    try:
        run = rmc.run_lo_essential(_run_model(usac, thr=0.007), polish=True)
    finally:
        rmc.set_thresholds(None)
    for p in range(rmc.P):
        _assert_run(run[p], uniform_run[p], RUN_KEYS, p)
        pref.assert_same_polish(run[p]["polished"], uniform_run[p]["polished"], p)


def test_distinct_thresholds_equal_one_problem_contexts(usac, oracle, run_problems):
    """problem p under θ_p equals a one-problem context at the scalar θ_p with p's seed: the hook (θ_p and
    its own iterative step) and the run"""
    sets, mc, _, ests = run_problems
    thrs = [THR * f for f in (1, 0.5, 2, 1.5)]
    seeds = [41, 42, 43, 44]
    recs = [eref.start_record(oracle, pts, eref.START_SEED + 20 + p, est=ests[p], thr=thrs[p]) for p, pts in enumerate(sets)]
    assert sum(r["inliers"] >= 12 for r in recs) >= 2
    far = 0.007
    mc.set_thresholds(thrs)
    try:
        hook_got = mc.lo_essential(eref.make_model(usac, thr=far), recs, seeds=seeds)
        run_got = mc.run_lo_essential(_run_model(usac, thr=far), seeds=seeds)
    finally:
        mc.set_thresholds(None)
    improved = 0
    for p, pts in enumerate(sets):
        with usac.MultiContext.essential([pts]) as one:
            h = one.lo_essential(eref.make_model(usac, thr=thrs[p]), [recs[p]], seeds=[seeds[p]])
            r = one.run_lo_essential(_run_model(usac, thr=thrs[p]), seeds=[seeds[p]])
        ref.assert_same_record(hook_got[0][p], h[0][0], p)
        ref.assert_same_state(hook_got[1][p], h[1][0], p)
        _assert_run(run_got[p], r[0], RUN_KEYS, p)
        improved += h[1][0]["improved"]
    assert improved > 0
    assert len({int(pref.bits(s["threshold"]).ravel()[0]) for s in hook_got[1]}) > 1


# ------------------------------------------------------------------ 8. refusals and leftovers
def test_refusals(usac, hook, run_problems, uniform_run):
    sets, mc, _, _ = run_problems
    none = [{"hyp_index": 0, "inliers": 0, "score": 0.0, "model": np.zeros(9), "valid": 0}] * mc.P

    def code(change):
        model = _run_model(usac)
        change(model)
        with pytest.raises(usac.UsacError) as e:
            mc.run_lo_essential(model)
        with pytest.raises(usac.UsacError) as e2:
            mc.lo_essential(model, none)
        return e.value.code, e2.value.code

    assert code(lambda m: setattr(m, "lo", usac.LocOpt.NullLO)) == (-1, -1)
    assert code(lambda m: setattr(m, "lo", usac.LocOpt.GC)) == (-3, -3)
    assert code(lambda m: m.setSprt(True)) == (-3, -3)
    assert code(lambda m: setattr(m, "lo_sample_size", 65)) == (-1, -1)
    assert code(lambda m: setattr(m, "lo_sample_size", 0)) == (-1, -1)
    assert code(lambda m: setattr(m, "lo_iterative_iterations", 0)) == (-1, -1)
    for change in (lambda m: setattr(m, "sampler", usac.SAMPLER.Napsac), lambda m: setattr(m, "batch", 100)):
        model = _run_model(usac)
        change(model)
        with pytest.raises(usac.UsacError) as e:
            mc.run_lo_essential(model)
        assert e.value.code == -1
    with usac.MultiContext.essential([sets[2], sets[2][:20]]) as small:  # n_p = 20
        with pytest.raises(usac.UsacError) as e:
            small.run_lo_essential(_run_model(usac, usac.SAMPLER.Prosac))
        assert e.value.code == -1
        assert len(small.run_lo_essential(_run_model(usac))) == 2
    # a refused call changed nothing: the same run as before
    got = mc.run_lo_essential(_run_model(usac))
    for p in range(mc.P):
        _assert_run(got[p], uniform_run[p], RUN_KEYS, p)
    # the runs without LO still refuse an LO model, and the H / F entries still refuse the essential context
    lo_model = _run_model(usac)
    for call in (lambda: mc.run(lo_model), lambda: mc.run_prosac(_run_model(usac, usac.SAMPLER.Prosac)),
                 lambda: mc.run_lo(lo_model), lambda: mc.lo(lo_model, none)):
        with pytest.raises(usac.UsacError) as e:
            call()
        assert e.value.code == -3
    assert b"essential" in usac.lib().usac_multi_last_error(mc._h)
    # on a homography context the new entries refuse and name the entry to use
    hsets = [ref.sets("H")[4]]
    hmodel = ref.make_model(usac, "H")
    with usac.MultiContext(usac.ESTIMATOR.Homography, hsets) as hmc:
        with pytest.raises(usac.UsacError) as e:
            hmc.run_lo_essential(hmodel)
        assert e.value.code == -3 and b"usac_multi_run_lo" in usac.lib().usac_multi_last_error(hmc._h)
        with pytest.raises(usac.UsacError) as e:
            hmc.lo_essential(hmodel, none[:1])
        assert e.value.code == -3 and b"usac_multi_lo" in usac.lib().usac_multi_last_error(hmc._h)
        assert len(hmc.run_lo(hmodel)) == 1
