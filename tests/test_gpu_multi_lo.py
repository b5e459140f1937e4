"""Multi-problem LO-RANSAC (usac_multi_lo, usac_multi_run_lo; ABI 18) on the device: the LO kernel
through its hook against the restatement over the CPU oracle (tests/helpers/multi_lo_ref.py) and
against the single-context LocalOptimization, the caps rule, and the run against its loop restated
over single contexts -- all without any tolerance."""
import ctypes

import numpy as np
import pytest

from tests.helpers import multi_lo_ref as ref
from tests.helpers import multi_polish_ref as pref
from tests.helpers import prosac_ref

pytestmark = pytest.mark.gpu

THR = ref.THR
M = {"H": 4, "F": 7}


def _est(usac, kind):
    return usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental


def _oracle_est(oracle, kind, pts, dlt):
    if kind == "H":
        return oracle.Estimator(oracle.HOMOGRAPHY, pts, dlt)
    return oracle.Estimator(oracle.FUNDAMENTAL, pts)


@pytest.fixture(scope="module")
def hook(usac, oracle):
    """(kind, dlt) -> (point sets, MultiContext, oracle estimators, start records, draw seeds): the sizes
    of multi_lo_ref.SIZES with the copy, then the degenerate problem"""
    made = {}
    for kind, dlt in (("H", 0), ("H", 1), ("F", 0)):
        sets = ref.sets(kind)
        ests = [_oracle_est(oracle, kind, p, dlt) for p in sets]
        recs = [ref.start_record(oracle, kind, p, ref.START_SEED + i, est=e) for i, (p, e) in enumerate(zip(sets, ests))]
        recs[ref.DUP[0]] = dict(recs[ref.DUP[1]])  # the copy starts where its original does
        fp, frec = ref.few_problem(oracle, kind)
        sets.append(fp)
        ests.append(_oracle_est(oracle, kind, fp, dlt))
        recs.append(frec)
        made[kind, dlt] = (sets, usac.MultiContext(_est(usac, kind), sets), ests, recs, ref.DRAW_SEEDS + [909])
    yield made
    for v in made.values():
        v[1].close()


def _ref_calls(usac, ests, recs, seeds, prm, calls):
    """`calls` LO calls in a row per problem on the restatement: per call the lists of records and states"""
    out = []
    cur = [(dict(r), ref.fresh_state(prm)) for r in recs]
    for _ in range(calls):
        cur = [ref.lo_ref(usac, e, r, st, sd, prm)[:2] for e, (r, st), sd in zip(ests, cur, seeds)]
        out.append(cur)
    return out


# ------------------------------------------------------------------ 1. the hook == the restatement
@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_hook_equals_restatement(usac, hook, kind, dlt, limited):
    sets, mc, ests, recs, seeds = hook[kind, dlt]
    model = ref.make_model(usac, kind, limited)
    prm = ref.from_model(model, M[kind])
    want = _ref_calls(usac, ests, recs, seeds, prm, 2)
    got1, st1 = mc.lo(model, recs, seeds=seeds, reset=True)
    got2, st2 = mc.lo(model, got1, seeds=seeds, reset=False)   # continues the draw counter and the threshold
    got3, st3 = mc.lo(model, recs, seeds=seeds, reset=True)    # repeats the first
    for p in range(mc.P):
        what = (kind, dlt, limited, p, len(sets[p]))
        ref.assert_same_record(got1[p], want[0][p][0], what)
        ref.assert_same_state(st1[p], want[0][p][1], what)
        ref.assert_same_record(got2[p], want[1][p][0], what)
        ref.assert_same_state(st2[p], want[1][p][1], what)
        ref.assert_same_record(got3[p], got1[p], what)
        ref.assert_same_state(st3[p], st1[p], what)
        # the invariant: no record is worse than its input; below the floor it comes back as it went in
        assert not ref.bigger(recs[p]["inliers"], recs[p]["score"], got1[p]["inliers"], got1[p]["score"]), what
        assert got1[p]["hyp_index"] == recs[p]["hyp_index"]
        if recs[p]["inliers"] < 12:
            ref.assert_same_record(got1[p], recs[p], what)
            assert st1[p]["fits"] == 0 and st1[p]["lo_calls"] == 1
    d, o = ref.DUP
    ref.assert_same_record(got1[d], got1[o])
    ref.assert_same_state(st2[d], st2[o])
    assert any(s["draws"] > 0 for s in st1) and any(a["draws"] > b["draws"] > 0 for a, b in zip(st2, st1))
    assert any(g["inliers"] > r["inliers"] for g, r in zip(got1, recs))
    # the degenerate problem: ten `<= sample_size` continues, the threshold left compounded
    few = st1[-1]
    assert few["inner_iters"] == 0 and few["fits"] == prm.inner and float(few["threshold"]) > 1e9


def test_hook_threshold_with_inexact_steps(usac, oracle, hook):
    """θ = 1.7, three iterative steps: a completed stage leaves the threshold within 1e-5 of θ but not at
    its bits, and the next call starts from there"""
    sets, mc, ests, _, seeds = hook["H", 1]
    model = ref.make_model(usac, "H", False, thr=1.7, iters=3)
    prm = ref.from_model(model, 4)
    recs = [ref.start_record(oracle, "H", p, ref.START_SEED + i, est=e, thr=1.7) for i, (p, e) in enumerate(zip(sets[:-1], ests))]
    recs.append(ref.few_problem(oracle, "H")[1])
    want = _ref_calls(usac, ests, recs, seeds, prm, 2)
    got1, st1 = mc.lo(model, recs, seeds=seeds, reset=True)
    got2, st2 = mc.lo(model, got1, seeds=seeds, reset=False)
    for p in range(mc.P):
        ref.assert_same_record(got1[p], want[0][p][0], p)
        ref.assert_same_state(st1[p], want[0][p][1], p)
        ref.assert_same_record(got2[p], want[1][p][0], p)
        ref.assert_same_state(st2[p], want[1][p][1], p)
    assert any(pref.bits(s["threshold"]) != pref.bits(np.float32(1.7)) and abs(float(s["threshold"]) - 1.7) < 1e-5 for s in st1)


# ------------------------------------------------------------------ 2. pinned to the single-context LO
@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_hook_equals_single_context_lo_without_draws(usac, hook, kind, dlt):
    """lo_sample_size >= n_p: no inner iteration draws, so the unlimited variant is the single context's
    LocalOptimization.GetModelScore on the same points and start record"""
    sets, mc, _, recs, seeds = hook[kind, dlt]
    model = ref.make_model(usac, kind, False, sample_size=64)
    got, st = mc.lo(model, recs, seeds=seeds, reset=True)
    checked = 0
    for p, pts in enumerate(sets):
        if len(pts) > 64 or recs[p]["inliers"] < 12:
            continue
        with usac.Context(_est(usac, kind), pts) as ctx:
            lo = usac.LocalOptimization(ctx, model)
            m = np.array(recs[p]["model"], dtype=np.float32)
            sc = usac.Score(recs[p]["inliers"], recs[p]["score"])
            lo.GetModelScore(m, sc)
            inner, iterative = lo.iters()
            lo.close()
        what = (kind, dlt, p, len(pts))
        np.testing.assert_array_equal(pref.bits(got[p]["model"]), pref.bits(m), err_msg=str(what))
        assert got[p]["inliers"] == sc.inlier_number, what
        assert pref.bits(got[p]["score"]) == pref.bits(np.float32(sc.score)), what
        assert (st[p]["inner_iters"], st[p]["iterative_iters"]) == (inner, iterative), what
        assert st[p]["draws"] == 0
        checked += 1
    assert checked >= 2


# ------------------------------------------------------------------ 3. the caps rule
def test_hook_caps(usac, oracle):
    pts, rec = ref.cap_problem(oracle)
    others = ref.sets("H")[4:6]
    sets = [others[0], pts, others[1]]
    ests = [pref.estimator(oracle, "H", p) for p in sets]
    recs = [ref.start_record(oracle, "H", sets[0], 74, est=ests[0]), rec, ref.start_record(oracle, "H", sets[2], 75, est=ests[2])]
    seeds = [31, 32, 33]
    model = ref.make_model(usac, "H", False)
    prm = ref.from_model(model, 4)
    want = _ref_calls(usac, ests, recs, seeds, prm, 1)[0]
    with usac.MultiContext(usac.ESTIMATOR.Homography, sets) as mc:
        got, st = mc.lo(model, recs, seeds=seeds)
        for p in range(3):
            ref.assert_same_record(got[p], want[p][0], p)
            ref.assert_same_state(st[p], want[p][1], p)
        assert st[1]["capped"] == 1 and st[0]["capped"] == st[2]["capped"] == 0
        ref.assert_same_record(got[1], rec)
    # the neighbours are what they are without the capped problem in the launch
    with usac.MultiContext(usac.ESTIMATOR.Homography, [sets[0], sets[2]]) as mc:
        alone, st_alone = mc.lo(model, [recs[0], recs[2]], seeds=[31, 33])
        for a, p in enumerate((0, 2)):
            ref.assert_same_record(alone[a], got[p])
            ref.assert_same_state(st_alone[a], st[p])


# ------------------------------------------------------------------ 4. run_lo == its restated loop
RUN_MAX, R = 512, 64


def _run_model(usac, kind, dlt, sampler, limited=False):
    model = ref.make_model(usac, kind, limited, sampler=sampler)
    model.max_iterations = RUN_MAX
    model.batch = R
    model.setDLTMode(dlt)
    return model


def _record(usac, d):
    return usac.Record(d["hyp_index"], d["inliers"], float(d["score"]), (ctypes.c_float * 9)(*np.asarray(d["model"]).tolist()),
                       int(d["valid"]))


def _restated_run(usac, mc, ctx, est, p, seed, dlt, prm, prosac):
    """usac_multi_run_lo's loop for problem p over a single context (the multi context only draws the
    samples), with the LO restatement at each improving round"""
    n, m = ctx.n, mc.m
    ctx.set_dlt_mode(dlt)
    scan = prosac_ref.PlainScan(n, m, lambda c, pts: usac.std_termination(c, pts, m, 0.95, RUN_MAX))
    T, L, largest, bound, best, r, scans = 1, n, m, RUN_MAX, None, 0, 0
    st = ref.fresh_state(prm)
    while True:
        first = r * R
        if prosac:
            samples = mc.draw_samples(R, [seed], first_hyp=first, problems=[p], clock=[T], term_len=[L])[0]
        else:
            samples = mc.draw_samples(R, [seed], first_hyp=first, problems=[p])[0]
        d = ctx.hypothesize_score(samples=samples, thr=THR)[2]
        d["hyp_index"] += first
        rec = _record(usac, d)
        best = rec if best is None else usac.merge_records([best, rec])
        new = bool(best.valid) and best.hyp_index >= first
        if new:
            lo_rec, st, _ = ref.lo_ref(usac, est, best.as_dict(), st, seed, prm)
            lo_rec["score"] = np.float32(lo_rec["score"])
            best = _record(usac, lo_rec)
        if prosac:
            sub, T_next, largest_next = usac.prosac_schedule(n, m, T, L, R, largest)
            k = T_next - T
            if new:
                j = best.hyp_index - first
                at = max(largest, int(sub[min(j, k - 1)])) if k else largest
                _, _, idx = ctx.get_inliers(np.array(best.model[:], dtype=np.float32), THR)
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
    ctx.set_dlt_mode(0)
    out = {"best": best.as_dict(), "rounds": r, "hypotheses": r * R, "bound": bound,
           "status": 0 if best.inliers > 0 else -111, "lo": st}
    if prosac:
        out.update(termination_length=L, largest_sample_size=largest, clock=T, scans=scans)
    return out


@pytest.fixture(scope="module")
def run_problems(usac, oracle):
    made = {}
    for kind in ("H", "F"):
        sets = ref.run_sets(kind)
        made[kind] = (sets, usac.MultiContext(_est(usac, kind), sets), [usac.Context(_est(usac, kind), p) for p in sets],
                      [pref.estimator(oracle, kind, p) for p in sets])
    yield made
    for _, mc, singles, _ in made.values():
        mc.close()
        for c in singles:
            c.close()


@pytest.mark.parametrize("sampler", ["uniform", "prosac"])
@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_run_equals_restated_loop(usac, run_problems, kind, dlt, sampler):
    sets, mc, singles, ests = run_problems[kind]
    prosac = sampler == "prosac"
    model = _run_model(usac, kind, dlt, usac.SAMPLER.Prosac if prosac else usac.SAMPLER.Uniform)
    prm = ref.from_model(model, M[kind])
    got = mc.run_lo(model, polish=True)
    keys = ["rounds", "hypotheses", "bound", "status"] + (["termination_length", "largest_sample_size", "clock", "scans"] if prosac else [])
    for p, ctx in enumerate(singles):
        want = _restated_run(usac, mc, ctx, ests[p], p, model.seed + p, dlt, prm, prosac)
        for key in keys:
            assert got[p][key] == want[key], (p, key, got[p], want)
        ref.assert_same_record(got[p]["best"], want["best"], p)
        ref.assert_same_state(got[p]["lo"], want["lo"], p)
    assert ("scans" in got[0]) == prosac
    # the inputs exercise the loop: some problem's record improved in more than one round (an LO call
    # each), the LO improved on a minimal model, and -- F, whose LO'd models later minimal models still
    # beat -- some problem went through the inner iterations of more than one call
    assert any(g["lo"]["lo_calls"] > 1 for g in got) and any(g["lo"]["improved"] > 0 for g in got)
    assert any(g["rounds"] > 1 for g in got)
    assert kind == "H" or any(g["lo"]["inner_iters"] > prm.inner for g in got)
    # polish=True: mc.polish of the LO'd models
    pol = mc.polish(np.stack([g["best"]["model"] for g in got]), THR, with_inliers=True)
    for p in range(mc.P):
        pref.assert_same_polish(got[p]["polished"], pol[p], p)
        np.testing.assert_array_equal(got[p]["inliers"], pol[p]["inlier_idx"])
    again = mc.run_lo(model)
    for p in range(mc.P):
        ref.assert_same_record(again[p]["best"], got[p]["best"], p)
        ref.assert_same_state(again[p]["lo"], got[p]["lo"], p)


def test_run_limited_variant(usac, run_problems):
    sets, mc, singles, ests = run_problems["F"]
    model = _run_model(usac, "F", 0, usac.SAMPLER.Uniform, limited=True)
    prm = ref.from_model(model, 7)
    got = mc.run_lo(model)
    for p, ctx in enumerate(singles):
        want = _restated_run(usac, mc, ctx, ests[p], p, model.seed + p, 0, prm, False)
        ref.assert_same_record(got[p]["best"], want["best"], p)
        ref.assert_same_state(got[p]["lo"], want["lo"], p)
        assert got[p]["rounds"] == want["rounds"]


# ------------------------------------------------------------------ 5. error codes
def test_run_lo_error_codes(usac, run_problems):
    sets, mc, _, _ = run_problems["H"]

    def code(change, sampler=None):
        model = _run_model(usac, "H", 0, sampler or usac.SAMPLER.Uniform)
        change(model)
        with pytest.raises(usac.UsacError) as e:
            mc.run_lo(model)
        with pytest.raises(usac.UsacError) as e2:
            mc.lo(model, [{"hyp_index": 0, "inliers": 0, "score": 0.0, "model": np.zeros(9), "valid": 0}] * mc.P)
        return e.value.code, e2.value.code

    assert code(lambda m: setattr(m, "lo", usac.LocOpt.NullLO)) == (-1, -1)
    assert code(lambda m: setattr(m, "lo", usac.LocOpt.GC)) == (-3, -3)
    assert code(lambda m: m.setSprt(True)) == (-3, -3)
    assert code(lambda m: setattr(m, "lo_sample_size", 65)) == (-1, -1)
    assert code(lambda m: setattr(m, "lo_sample_size", 0)) == (-1, -1)
    assert code(lambda m: setattr(m, "lo_iterative_iterations", 0)) == (-1, -1)
    for change in (lambda m: setattr(m, "sampler", usac.SAMPLER.Napsac), lambda m: setattr(m, "batch", 100)):
        model = _run_model(usac, "H", 0, usac.SAMPLER.Uniform)
        change(model)
        with pytest.raises(usac.UsacError) as e:
            mc.run_lo(model)
        assert e.value.code == -1
    with usac.MultiContext(usac.ESTIMATOR.Homography, [sets[2], sets[2][:20]]) as small:  # n_p = 20
        with pytest.raises(usac.UsacError) as e:
            small.run_lo(_run_model(usac, "H", 0, usac.SAMPLER.Prosac))
        assert e.value.code == -1
        assert len(small.run_lo(_run_model(usac, "H", 0, usac.SAMPLER.Uniform))) == 2
    # the runs without LO still refuse an LO model, and point to the new entry
    for call, sampler in ((mc.run, usac.SAMPLER.Uniform), (mc.run_prosac, usac.SAMPLER.Prosac)):
        with pytest.raises(usac.UsacError) as e:
            call(_run_model(usac, "H", 0, sampler))
        assert e.value.code == -3
