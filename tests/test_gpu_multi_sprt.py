"""Multi-problem SPRT (usac_multi_hypothesize_score_sprt, usac_multi_run_sprt; ABI 19) on the device: the
round hook bit for bit against the single context's throughput SPRT (H) and against the reference's walk
by the CPU oracle (H and F, with the certificate's test overrides), its statistics, the work it saves,
and the run against its loop restated in Python over the hook and the Python update rule
(tests/helpers/multi_sprt_ref.py) -- all without any tolerance."""
import ctypes

import numpy as np
import pytest

from tests.helpers import multi_polish_ref as pref
from tests.helpers import multi_sprt_ref as ref
from tests.helpers import prosac_ref

pytestmark = pytest.mark.gpu

THR = ref.THR
M = ref.M
SEEDS = [21, 22, 23, 24, 25, 26, 24]  # sampler seeds: the copy shares its original's
EMPTY = 0xFFFFFFFF


def _est(usac, kind):
    return usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_record(a, b, what=""):
    assert a["hyp_index"] == b["hyp_index"] and a["inliers"] == b["inliers"] and a["valid"] == b["valid"], (what, a, b)
    assert _bits(a["score"]) == _bits(b["score"]), what
    np.testing.assert_array_equal(_bits(a["model"]), _bits(b["model"]), err_msg=str(what))


@pytest.fixture(scope="module")
def hook(usac, oracle):
    """kind -> (point sets, inlier masks, MultiContext with the pools of ref.POOL_SEEDS, the pools)"""
    made = {}
    for kind in ("H", "F"):
        sets, inl = ref.sets(kind)
        mc = usac.MultiContext(_est(usac, kind), sets)
        mc.set_sprt_pool(ref.POOL_SEEDS)
        pools = [oracle.sprt_pool(s, ref.oracle_kind(oracle, kind), len(p), M[kind])[0] for s, p in zip(ref.POOL_SEEDS, sets)]
        made[kind] = (sets, inl, mc, pools)
    yield made
    for v in made.values():
        v[2].close()


LANES = 29  # every 29th lane from lane 3 takes a sample of known inliers


def _samples(oracle, kind, mc, sets, inl, R, problems, first_hyp=0):
    """the device sampler's samples of the listed problems, a few lanes of every tile replaced by good samples
    of known inliers (where the problem has enough): models that survive the head and reach the tail"""
    s = mc.draw_samples(R, [SEEDS[p] for p in problems], first_hyp=first_hyp, problems=problems)
    rng = np.random.default_rng(1234 + R)
    for a, p in enumerate(problems):
        lanes = list(range(3, R, LANES))
        good = ref.inlier_samples(oracle, kind, sets[p], inl[p], len(lanes), rng)
        if good is not None:
            s[a, lanes] = good
    return s


# ------------------------------------------------------------------ 1. H: the single context, bit for bit
@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("dlt", [0, 1])
def test_h_hook_equals_single_context(usac, oracle, hook, dlt, R):
    sets, inl, mc, _ = hook["H"]
    problems = [5, 2, 6, 0, 3, 1]  # a shuffled partial list (the 321-point set stays out)
    first = 3 * R
    samples = _samples(oracle, "H", mc, sets, inl, R, problems, first)
    ed = [ref.EPS_DELTA["H"][p] for p in problems]
    mc.set_dlt_mode(dlt)
    try:
        c, s, best, stats, starts = mc.hypothesize_score_sprt(R, first_hyp=first, thr=THR, problems=problems,
                                                              samples=samples, eps_delta=ed)
    finally:
        mc.set_dlt_mode(0)
    survivors = 0
    for a, p in enumerate(problems):
        with usac.Context(usac.ESTIMATOR.Homography, sets[p]) as ctx:
            ctx.set_dlt_mode(dlt)
            ctx.set_sprt(True, seed=ref.POOL_SEEDS[p], epsilon=ed[a][0], delta=ed[a][1])
            wc, ws, wbest = ctx.hypothesize_score(samples=samples[a], first_hyp=first, thr=THR)
            (e, d, A), wstarts = ctx.batch_sprt_info(R)
        what = (dlt, R, p, len(sets[p]))
        np.testing.assert_array_equal(c[a], wc, err_msg=str(what))
        np.testing.assert_array_equal(_bits(s[a]), _bits(ws), err_msg=str(what))
        np.testing.assert_array_equal(starts[a], wstarts, err_msg=str(what))
        _same_record(best[a], wbest, what)
        assert ref.bits64([e, d, A]) == ref.bits64(ref.design("H", *ed[a])), what
        assert stats[a]["accepted"] == int((wc >= 0).sum()), what
        assert stats[a]["rejected_head"] + stats[a]["rejected_tail"] == int((wc < 0).sum()), what
        if len(sets[p]) > 64:
            survivors += int((wc >= 0).sum())
    assert survivors > 0
    assert len({int(x) for x in starts[0]}) == R // 64  # one start per tile


# ------------------------------------------------------------------ 2. H and F: the reference's walk
def _oracle_models(oracle, kind, pts, samples, dlt):
    """-> (models of the occupied slots, occupied [R * spk])"""
    okind = ref.oracle_kind(oracle, kind)
    est = oracle.Estimator(okind, pts, dlt) if kind == "H" else oracle.Estimator(okind, pts)
    om, onm = est.estimate_batch(samples)
    if kind == "H":
        return est, np.asarray(om, np.float32).reshape(-1, 9), np.ones(len(samples), bool)
    occ = (np.arange(3)[None, :] < onm[:, None]).reshape(-1)
    return est, np.asarray(om, np.float32).reshape(-1, 9)[occ], occ


def _check_round(usac, oracle, hook, kind, R, dlt, with_stats):
    sets, inl, mc, pools = hook[kind]
    problems = [4, 6, 1, 5, 0, 3, 2]
    samples = _samples(oracle, kind, mc, sets, inl, R, problems)
    ed = [ref.EPS_DELTA[kind][p] for p in problems]
    mc.set_dlt_mode(dlt)
    try:
        out = mc.hypothesize_score_sprt(R, thr=THR, problems=problems, samples=samples, eps_delta=ed)
        again = mc.hypothesize_score_sprt(R, thr=THR, problems=problems, samples=samples, eps_delta=ed)
        plain = mc.hypothesize_score(R, thr=THR, problems=problems, samples=samples)[0]
    finally:
        mc.set_dlt_mode(0)
    c, s, best, stats, starts = out
    # two identical calls give identical outputs (F's solve waves append their list in any order: not read)
    np.testing.assert_array_equal(c, again[0])
    np.testing.assert_array_equal(_bits(s), _bits(again[1]))
    np.testing.assert_array_equal(starts, again[4])
    assert stats == again[3]
    for a in range(len(problems)):
        _same_record(best[a], again[2][a])
    tail_accepts = 0
    for a, p in enumerate(problems):
        n, what = len(sets[p]), (kind, R, dlt, p, len(sets[p]))
        est, models, occ = _oracle_models(oracle, kind, sets[p], samples[a], dlt)
        test = ref.design(kind, *ed[a])
        assert (c[a][~occ] == -1).all() and (s[a][~occ] == 0).all() and (starts[a][~occ] == EMPTY).all(), what
        assert (starts[a][occ] == (np.flatnonzero(occ) // 64 * 7919) % n).all(), what
        if with_stats:
            good, cnt, tested, seen = ref.walk(oracle, est, pools[p], models, starts[a][occ], test)
        else:
            good, cnt, tested = oracle.sprt_fixed_batch(est, pools[p], THR, models, starts[a][occ], *test)
        np.testing.assert_array_equal(c[a][occ], cnt, err_msg=str(what))
        np.testing.assert_array_equal(s[a][occ], np.where(good, cnt, 0).astype(np.float32), err_msg=str(what))
        # an accepted slot's count is the plain scorer's
        np.testing.assert_array_equal(c[a][occ][good], plain[a][occ][good], err_msg=str(what))
        # the round's best: the largest accepted count, the earliest slot on ties (sums = counts)
        if good.any():
            top = int(np.flatnonzero(c[a] == c[a].max())[0])
            assert best[a]["valid"] == 1 and best[a]["inliers"] == int(c[a].max()) and best[a]["hyp_index"] == top // mc.spk
        else:
            assert best[a]["valid"] == 0
        if with_stats:
            want = ref.round_stats(good, tested, seen, n)
            got = stats[a]
            assert got["accepted"] == want["accepted"], what
            assert got["rejected_head"] + got["rejected_tail"] == want["rejected"], what
            assert got["rejected_head"] == want["rejected_head"], what
            assert (got["head_inliers"], got["head_points"]) == (want["head_inliers"], want["head_points"]), what
            # the work done: the head's share exactly, a tail rejection up to its chunk's end
            per = -(-max(n - 64, 0) // 256)
            lo = int(tested.sum())
            hi = lo + int(((~good) & (tested > 64)).sum()) * max(per - 1, 0)
            assert lo <= got["points_tested"] <= hi, (what, lo, got["points_tested"], hi)
        if n > 64:
            tail_accepts += int(good.sum())
    assert tail_accepts > 0  # survivors exist and pass the tail
    return c


@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_hook_equals_reference_walk_and_statistics(usac, oracle, hook, kind, dlt, R):
    _check_round(usac, oracle, hook, kind, R, dlt, True)


@pytest.mark.parametrize("kind", ["H", "F"])
@pytest.mark.parametrize("env", [("USAC_SPRT_CERT_MARGIN", "1e9"), ("USAC_SPRT_CERT_CLIMB", "3")])
def test_hook_decisions_do_not_depend_on_the_certificate(usac, oracle, hook, monkeypatch, kind, env):
    """a margin no walk clears / a climb limit most walks reach: every decision by the sequential fall-back"""
    base = _check_round(usac, oracle, hook, kind, 128, 0, False)
    monkeypatch.setenv(*env)
    np.testing.assert_array_equal(_check_round(usac, oracle, hook, kind, 128, 0, False), base)


def test_hook_argument_errors(usac, hook):
    _, _, mc, _ = hook["H"]
    for ed in ([(1.0, 0.01)], [(0.1, -0.5)], [(0.1, 0.1)], [(0.05, 0.06)], [(0, 0.2)], [(1.5, 0)]):
        with pytest.raises(usac.UsacError) as e:
            mc.hypothesize_score_sprt(64, seeds=[1], problems=[2], eps_delta=ed)
        assert e.value.code == -1, ed
    with pytest.raises(usac.UsacError) as e:
        mc.hypothesize_score_sprt(100, seeds=[1], problems=[2])
    assert e.value.code == -1


# ------------------------------------------------------------------ 3. the work saved
def _work_samples(usac, oracle, pts, inl, R):
    """host uniform samples (seed 77), four lanes replaced by good samples of known inliers"""
    samples = usac.uniform_samples(77, len(pts), 4, R)
    samples[[3, 40, 70, 101]] = ref.inlier_samples(oracle, "H", pts, inl, 4, np.random.default_rng(99))
    return samples


def test_work_saved_on_the_1000_point_problem(usac, oracle, hook):
    """The 1000-point, 30 %-inlier homography problem under 128 host samples, four of them good ones: the
    reference's own walk reads 0.0285 of slots x n_p there (evaluated on the CPU below: two models are
    accepted after all 1000 points, the others rejected within 13 to 24 pool points); the device must stay
    below twice that."""
    sets, inl, mc, pools = hook["H"]
    p, R = 5, 128
    n = len(sets[p])
    samples = _work_samples(usac, oracle, sets[p], inl[p], R)
    est, models, occ = _oracle_models(oracle, "H", sets[p], samples, 0)
    test = ref.design("H", *ref.EPS_DELTA["H"][p])
    starts = (np.arange(R) // 64 * 7919) % n
    _, _, tested = oracle.sprt_fixed_batch(est, pools[p], THR, models, starts, *test)
    share = float(tested.sum()) / (R * n)
    print("oracle share of slots x n_p: %.4f" % share)
    assert share < 0.25
    _, _, _, stats, _ = mc.hypothesize_score_sprt(R, thr=THR, problems=[p], samples=samples[None],
                                                  eps_delta=[ref.EPS_DELTA["H"][p]])
    got = stats[0]["points_tested"] / (R * n)
    print("device share: %.4f" % got)
    assert got < 2 * share


# ------------------------------------------------------------------ 4. run_sprt == its restated loop
RUN_MAX, RUN_R, RUN_PROB = 512, 64, 0.95


def _run_model(usac, kind, dlt, sampler):
    model = usac.Model(THR, M[kind], RUN_PROB, 5, _est(usac, kind), sampler)
    model.max_iterations = RUN_MAX
    model.batch = RUN_R
    model.seed = 300
    model.setSprt(True)
    model.setDLTMode(dlt)
    return model


def _record(usac, d):
    return usac.Record(d["hyp_index"], d["inliers"], float(d["score"]), (ctypes.c_float * 9)(*np.asarray(d["model"]).tolist()),
                       int(d["valid"]))


def _restated_run(usac, mc, ctx, kind, p, seed, prosac):
    """usac_multi_run_sprt's loop for problem p over the round hook, the Python update rule and (PROSAC) the
    plain scan; mc's dlt mode is the run's"""
    n, m, R = int(mc.sizes[p]), mc.m, RUN_R
    std = lambda c, pts: usac.std_termination(c, pts, m, RUN_PROB, RUN_MAX)
    scan = prosac_ref.PlainScan(n, m, std) if prosac else None
    st = ref.RefState(kind, n, RUN_MAX)
    T, L, largest, pbound, best, r, scans = 1, n, m, RUN_MAX, None, 0, 0
    tot = {"accepted": 0, "rejected": 0, "points_tested": 0}
    while True:
        first = r * R
        if prosac:
            samples = mc.draw_samples(R, [seed], first_hyp=first, problems=[p], clock=[T], term_len=[L])
        else:
            samples = mc.draw_samples(R, [seed], first_hyp=first, problems=[p])
        e, d, _ = st.test
        _, _, recs, stats, _ = mc.hypothesize_score_sprt(R, first_hyp=first, thr=THR, problems=[p], samples=samples,
                                                         eps_delta=[(e, d)])
        rec = _record(usac, recs[0])
        best = rec if best is None else usac.merge_records([best, rec])
        new = bool(best.valid) and best.hyp_index >= first
        tb = 0
        if prosac:
            sub, T_next, largest_next = usac.prosac_schedule(n, m, T, L, R, largest)
            k = T_next - T
            if new:
                j = best.hyp_index - first
                at = max(largest, int(sub[min(j, k - 1)])) if k else largest
                _, _, idx = ctx.get_inliers(np.array(best.model[:], dtype=np.float32), THR)
                flags = np.zeros(n, dtype=bool)
                flags[idx] = True
                pbound, _ = scan.scan(best.hyp_index, flags, at)
                L = scan.term_len
                scans += 1
            T, largest = T_next, largest_next
            tb = pbound
        elif new:
            tb = std(best.inliers, n)
        tot["accepted"] += stats[0]["accepted"]
        tot["rejected"] += stats[0]["rejected_head"] + stats[0]["rejected_tail"]
        tot["points_tested"] += stats[0]["points_tested"]
        r += 1
        st.update(r * R, stats[0]["head_inliers"], stats[0]["head_points"], new, best.inliers, tb)
        if r * R >= min(RUN_MAX, st.bound):
            break
    out = {"best": best.as_dict(), "rounds": r, "hypotheses": r * R, "bound": st.bound,
           "status": 0 if best.inliers > 0 else -111, "test": st.test, "tests": len(st.history), "totals": tot}
    if prosac:
        out.update(termination_length=L, largest_sample_size=largest, clock=T, scans=scans)
    return out


@pytest.fixture(scope="module")
def run_problems(usac):
    made = {}
    for kind in ("H", "F"):
        sets, _ = ref.sets(kind, sort=True, with_m=False)
        made[kind] = (sets, usac.MultiContext(_est(usac, kind), sets), [usac.Context(_est(usac, kind), p) for p in sets])
    yield made
    for _, mc, singles in made.values():
        mc.close()
        for c in singles:
            c.close()


@pytest.mark.parametrize("sampler", ["uniform", "prosac"])
@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_run_equals_restated_loop(usac, run_problems, kind, dlt, sampler):
    sets, mc, singles = run_problems[kind]
    prosac = sampler == "prosac"
    model = _run_model(usac, kind, dlt, usac.SAMPLER.Prosac if prosac else usac.SAMPLER.Uniform)
    got = mc.run_sprt(model, polish=True)
    keys = ["rounds", "hypotheses", "bound", "status"] + (["termination_length", "largest_sample_size", "clock", "scans"] if prosac else [])
    mc.set_dlt_mode(dlt)
    try:
        for p, ctx in enumerate(singles):
            want = _restated_run(usac, mc, ctx, kind, p, model.seed + p, prosac)
            for key in keys:
                assert got[p][key] == want[key], (p, key, got[p], want)
            _same_record(got[p]["best"], want["best"], p)
            sp = got[p]["sprt"]
            assert ref.bits64([sp["epsilon"], sp["delta"], sp["A"]]) == ref.bits64(want["test"]), (p, sp, want["test"])
            assert sp["tests"] == want["tests"], p
            assert {k: sp[k] for k in want["totals"]} == want["totals"], p
    finally:
        mc.set_dlt_mode(0)
    assert ("scans" in got[0]) == prosac
    # the inputs exercise the loop: more than one round, a re-designed test, an early stop
    assert any(g["rounds"] > 1 for g in got) and any(g["sprt"]["tests"] > 1 for g in got)
    assert any(g["hypotheses"] < RUN_MAX for g in got)
    # every final record's count is the inlier count of its model
    models = np.stack([g["best"]["model"] for g in got])
    for p, idx in enumerate(mc.inliers(models, THR)):
        if got[p]["best"]["valid"]:
            assert len(idx) == got[p]["best"]["inliers"], p
            assert _bits(got[p]["best"]["score"]) == _bits(np.float32(len(idx))), p
    # polish=True: mc.polish of the same models
    pol = mc.polish(models, THR, with_inliers=True)
    for p in range(mc.P):
        pref.assert_same_polish(got[p]["polished"], pol[p], p)
        np.testing.assert_array_equal(got[p]["inliers"], pol[p]["inlier_idx"])
    again = mc.run_sprt(model)
    for p in range(mc.P):
        _same_record(again[p]["best"], got[p]["best"], p)
        assert again[p]["sprt"] == got[p]["sprt"] and again[p]["rounds"] == got[p]["rounds"]


def test_run_sprt_error_codes(usac, run_problems):
    sets, mc, _ = run_problems["H"]

    def code(change, sampler=None):
        model = _run_model(usac, "H", 0, sampler or usac.SAMPLER.Uniform)
        change(model)
        with pytest.raises(usac.UsacError) as e:
            mc.run_sprt(model)
        return e.value.code

    assert code(lambda m: m.setSprt(False)) == -1
    assert code(lambda m: setattr(m, "lo", usac.LocOpt.InItLORsc)) == -3
    assert code(lambda m: setattr(m, "lo", usac.LocOpt.GC)) == -3
    assert code(lambda m: setattr(m, "sampler", usac.SAMPLER.Napsac)) == -1
    assert code(lambda m: setattr(m, "batch", 100)) == -1
    assert code(lambda m: setattr(m, "dlt_mode", 7)) == -1
    with usac.MultiContext(usac.ESTIMATOR.Homography, [sets[2], sets[2][:20]]) as small:  # n_p = 20
        with pytest.raises(usac.UsacError) as e:
            small.run_sprt(_run_model(usac, "H", 0, usac.SAMPLER.Prosac))
        assert e.value.code == -1
        assert len(small.run_sprt(_run_model(usac, "H", 0, usac.SAMPLER.Uniform))) == 2
    # the runs without SPRT still refuse an SPRT model
    for call, sampler in ((mc.run, usac.SAMPLER.Uniform), (mc.run_prosac, usac.SAMPLER.Prosac)):
        with pytest.raises(usac.UsacError) as e:
            call(_run_model(usac, "H", 0, sampler))
        assert e.value.code == -3
