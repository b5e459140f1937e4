"""Per-problem thresholds of a multi context (usac_multi_set_thresholds, ABI 22).  The yardstick is the
code that exists without them: problem p's result in the P-problem context under thresholds t must
equal, bit for bit, the result for the same points at the scalar threshold t_p -- a Context over the
problem's points for a round's counts, sums and masks, a one-problem MultiContext with the same seed
(and SPRT pool seed) for the runs and the hooks.  The scalar every call passes while thresholds are set
is a value no problem has, so a kernel that still read it would give other counts.

Figures printed by the tests (pytest -s): none are tolerances; every comparison is exact."""
import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import multi_lo_ref as lo_ref
from tests.helpers.same_bits import same as _same

pytestmark = pytest.mark.gpu

R, MAX_IT, PROB = 64, 512, 0.95
M = {"H": 4, "F": 7, "E": 5}
# the sizes of the other multi tests (n_p = m, 21, 64, 65, 333, 1000) and, last, a copy of the 333-point
# problem under another threshold
RATIOS = [0.9, 0.5, 0.3, 0.3, 0.5, 0.3]
DATA_SEEDS = {"H": [20, 21, 22, 23, 24, 25], "F": [22, 31, 32, 33, 34, 35], "E": [22, 31, 32, 33, 34, 35]}
DUP = (6, 4)
SEEDS = [11, 12, 13, 14, 15, 16, 15]     # sampler seeds: the copy shares its original's
POOLS = [3, 4, 5, 6, 7, 8, 7]            # SPRT pool seeds, likewise
DRAWS = [901, 902, 903, 904, 905, 906, 905]
_T = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0]  # pairwise distinct
THRS = {"H": _T, "F": _T, "E": [t / 1000 for t in _T]}
SCALAR = {"H": 7.0, "F": 7.0, "E": 0.007}  # what the calls pass while thresholds are set: no problem's value
CELL = {"H": 50, "F": 400}
PARTIAL = [6, 2, 0]                        # a shuffled partial active list: entry a is not problem a


def _sizes(kind):
    return [M[kind], 21, 64, 65, 333, 1000]


def _make(kind, n, ratio, seed, **kw):
    if kind == "H":
        return synthetic.homography_points(n=n, inlier_ratio=ratio, seed=seed, **kw)[0]
    return synthetic.fundamental_points(n=n, inlier_ratio=ratio, seed=seed, prosac_order=False,
                                        normalized=(kind == "E"), **kw)[0]


def _sets(kind):
    out = [_make(kind, n, r, s) for n, r, s in zip(_sizes(kind), RATIOS, DATA_SEEDS[kind])]
    out.append(out[DUP[1]].copy())
    return out


def _est(usac, kind):
    return {"H": usac.ESTIMATOR.Homography, "F": usac.ESTIMATOR.Fundamental, "E": usac.ESTIMATOR.Essential}[kind]


def _multi(usac, kind, sets):
    return usac.MultiContext.essential(sets) if kind == "E" else usac.MultiContext(_est(usac, kind), sets)


def _oracle_est(oracle, kind, pts, dlt=0):
    if kind == "H":
        return oracle.Estimator(oracle.HOMOGRAPHY, pts, oracle.DLT_NULLSPACE if dlt else oracle.DLT_THIN)
    return oracle.Estimator(oracle.FUNDAMENTAL if kind == "F" else oracle.ESSENTIAL, pts)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_scores(c, s, rc, rs, what):
    np.testing.assert_array_equal(c, rc, err_msg=str(what))
    ok = rc >= 0
    np.testing.assert_array_equal(_bits(s)[ok], _bits(rs)[ok], err_msg=str(what))


class World:
    """one kind's point sets, the P-problem context, and per problem a Context and a one-problem MultiContext"""

    def __init__(self, usac, kind, sets):
        self.kind, self.sets, self.P = kind, sets, len(sets)
        self.mc = _multi(usac, kind, sets)
        self.singles = [usac.Context(_est(usac, kind), p) for p in sets]
        self.ones = [_multi(usac, kind, [p]) for p in sets]

    def close(self):
        for c in [self.mc] + self.singles + self.ones:
            c.close()


@pytest.fixture(scope="module")
def worlds(usac):
    """kind -> (all problems, the problems of more than 20 points: PROSAC runs on those)"""
    made = {}
    for kind in ("H", "F", "E"):
        sets = _sets(kind)
        made[kind] = (World(usac, kind, sets), World(usac, kind, sets[1:]))
    yield made
    for pair in made.values():
        for w in pair:
            w.close()


class thresholds:
    """set for the block, cleared after it"""

    def __init__(self, mc, thr):
        self.mc, self.thr = mc, thr

    def __enter__(self):
        self.mc.set_thresholds(self.thr)

    def __exit__(self, *a):
        self.mc.set_thresholds(None)
        self.mc.set_dlt_mode(0)


def test_set_get_clear(usac, worlds):
    mc = worlds["H"][0].mc
    assert mc.thresholds is None
    mc.set_thresholds(THRS["H"])
    got = mc.thresholds
    assert got.dtype == np.float32 and (got == np.asarray(THRS["H"], np.float32)).all()
    mc.set_thresholds(None)
    assert mc.thresholds is None
    for bad in ([1.0] * 6, [1.0] * 8, []):
        with pytest.raises(usac.UsacError) as e:
            mc.set_thresholds(bad)
        assert e.value.code == -1
    assert mc.thresholds is None


# ------------------------------------------------------------------ 1. a round
# R = 128: two workgroups per problem in the scorers, each of which loads its problem's threshold
@pytest.mark.parametrize("host", [True, False], ids=["host_samples", "device_sampler"])
@pytest.mark.parametrize("kind,dlt,R", [("H", 0, 64), ("H", 1, 64), ("F", 0, 64), ("E", 0, 64),
                                        ("H", 0, 128), ("F", 0, 128), ("E", 0, 128)])
def test_round_equals_single_context_and_oracle(usac, oracle, worlds, kind, dlt, R, host):
    w = worlds[kind][0]
    T, f = THRS[kind], R
    ests = [_oracle_est(oracle, kind, p, dlt) for p in w.sets]
    for c in w.singles:
        c.set_dlt_mode(dlt)
    try:
        with thresholds(w.mc, T):
            w.mc.set_dlt_mode(dlt)
            for active in (None, PARTIAL):
                ids = list(range(w.P)) if active is None else active
                if host:
                    samples = [oracle.uniform_samples(40 + p, len(w.sets[p]), M[kind], R) for p in ids]
                else:
                    samples = [w.singles[p].draw_samples(R, SEEDS[p], first_hyp=f) for p in ids]
                c, s, best = w.mc.hypothesize_score(R, None if host else [SEEDS[p] for p in ids], first_hyp=f,
                                                    thr=SCALAR[kind], problems=active,
                                                    samples=np.concatenate(samples) if host else None)
                counts = {}
                for a, p in enumerate(ids):
                    rc, rs, rbest = w.singles[p].hypothesize_score(B=R, samples=samples[a] if host else None,
                                                                   seed=SEEDS[p], first_hyp=f, thr=T[p])
                    _same_scores(c[a], s[a], rc, rs, (kind, dlt, host, active, p))
                    _same(best[a], rbest, (kind, dlt, host, active, p))
                    counts[p] = c[a]
                    if best[a]["valid"]:  # the oracle's quality of the best model at t_p
                        oc, osum = ests[p].quality(best[a]["model"], T[p])
                        assert (oc, _bits(osum)) == (best[a]["inliers"], _bits(best[a]["score"])), (kind, p)
                # the copy and its original: the same models, and the two thresholds tell them apart -- first on
                # the CPU (the precondition: a threshold indexed wrongly cannot pass unseen), then on the device
                d, o = DUP
                a_o = ids.index(o) if o in ids else None
                if a_o is not None and d in ids:
                    om, nm = ests[o].estimate_batch(samples[a_o])
                    om = om.reshape(-1, 9)
                    differ = int((ests[o].score_models(om, T[o])[0] != ests[o].score_models(om, T[d])[0]).sum())
                    print("%s dlt %d: %d of %d slots count differently at %g and %g" % (kind, dlt, differ, len(om), T[o], T[d]))
                    assert differ > 0
                    assert (counts[o] != counts[d]).any()
    finally:
        for c in w.singles:
            c.set_dlt_mode(0)


@pytest.mark.parametrize("kind,dlt,R", [("H", 0, 64), ("H", 1, 64), ("F", 0, 64), ("H", 0, 128), ("F", 0, 128)])
def test_sprt_round_equals_one_problem_context(usac, worlds, kind, dlt, R):
    w = worlds[kind][0]
    T = THRS[kind]
    w.mc.set_sprt_pool(POOLS)
    for p, one in enumerate(w.ones):
        one.set_sprt_pool([POOLS[p]])
        one.set_dlt_mode(dlt)
    try:
        with thresholds(w.mc, T):
            w.mc.set_dlt_mode(dlt)
            for active in (None, PARTIAL):
                ids = list(range(w.P)) if active is None else active
                got = w.mc.hypothesize_score_sprt(R, [SEEDS[p] for p in ids], first_hyp=R, thr=SCALAR[kind], problems=active)
                for a, p in enumerate(ids):
                    want = w.ones[p].hypothesize_score_sprt(R, [SEEDS[p]], first_hyp=R, thr=T[p])
                    _same([g[a] for g in got], [x[0] for x in want], (kind, dlt, active, p))
            full = w.mc.hypothesize_score_sprt(R, SEEDS, first_hyp=R, thr=SCALAR[kind])
        # not vacuous: without the thresholds the same call, at the scalar it passes, verifies differently (a
        # rejected slot reads -1 under any threshold, so the statistics count too)
        w.mc.set_dlt_mode(dlt)
        plain = w.mc.hypothesize_score_sprt(R, SEEDS, first_hyp=R, thr=SCALAR[kind])
        assert (full[0] != plain[0]).any() or full[3] != plain[3]
    finally:
        w.mc.set_dlt_mode(0)
        for one in w.ones:
            one.set_dlt_mode(0)


@pytest.mark.parametrize("kind", ["H", "F"])
def test_napsac_round_equals_one_problem_context(usac, worlds, kind):
    w = worlds[kind][0]
    T, cs = THRS[kind], CELL[kind]
    with thresholds(w.mc, T):
        for active in (None, PARTIAL):
            ids = list(range(w.P)) if active is None else active
            got = w.mc.hypothesize_score_napsac(R, [SEEDS[p] for p in ids], cs, first_hyp=R, thr=SCALAR[kind], problems=active)
            for a, p in enumerate(ids):
                want = w.ones[p].hypothesize_score_napsac(R, [SEEDS[p]], cs, first_hyp=R, thr=T[p])
                _same([g[a] for g in got], [x[0] for x in want], (kind, active, p))


# ------------------------------------------------------------------ 2. masks and polish
PTS_MAX = 16384  # kPolPtsMax: a larger problem is polished through a temporary single context on the host


def _round_models(mc, kind, seeds, thr):
    """every problem's best model of one round (the identity-like fallback where a problem has none)"""
    best = mc.hypothesize_score(R, seeds, first_hyp=0, thr=thr, per_hypothesis=False)[2]
    return np.stack([np.asarray(b["model"], np.float32) if b["valid"] else np.eye(3, dtype=np.float32).ravel() for b in best]), best


@pytest.mark.parametrize("kind", ["H", "F", "E"])
def test_masks_and_polish_equal_single_problem(usac, worlds, kind):
    # the usual problems and one of kPolPtsMax + 1 points, which the workgroup defers to the host
    sets = _sets(kind) + [_make(kind, PTS_MAX + 1, 0.5, 77)]
    T = THRS[kind] + [THRS[kind][1] * 1.25]
    seeds = SEEDS + [21]
    with _multi(usac, kind, sets) as mc:
        mc.set_thresholds(T)
        models, _ = _round_models(mc, kind, seeds, SCALAR[kind])
        inl = mc.inliers(models, SCALAR[kind])
        pol = mc.polish(models, SCALAR[kind], with_inliers=True)
        for p, pts in enumerate(sets):
            with usac.Context(_est(usac, kind), pts) as ctx:
                n, _, idx = ctx.get_inliers(models[p], T[p])
            assert n == len(inl[p])
            np.testing.assert_array_equal(inl[p], idx, err_msg=str((kind, p)))
            with _multi(usac, kind, [pts]) as one:
                want = one.polish(models[p:p + 1], T[p], with_inliers=True)[0]
            _same(pol[p], want, (kind, "polish", p))
        assert pol[-1]["status"] == 0 and pol[-1]["inliers"] > 0
        # not vacuous: at the scalar the big problem's mask is another one
        mc.set_thresholds(None)
        assert len(mc.inliers(models, SCALAR[kind])[-1]) != len(inl[-1])


# ------------------------------------------------------------------ 3. the runs
def _model(usac, kind, thr, sampler=None, lo=None, sprt=False, napsac=False):
    S = usac.SAMPLER
    sampler = S.Napsac if napsac else (sampler or S.Uniform)
    if lo is not None:
        model = lo_ref.make_model(usac, kind, limited=(lo == usac.LocOpt.InItFLORsc), sampler=sampler, thr=thr)
    else:
        model = usac.Model(thr, M[kind], PROB, 5, _est(usac, kind), sampler)
    if napsac:
        model.setNeighborsType(usac.NeighborsSearch.Grid)
        model.setCellSize(CELL[kind])
    model.max_iterations, model.batch, model.seed = MAX_IT, R, 300
    model.setSprt(sprt)
    return model


def _run_cases(usac, kind):
    """name -> (needs every n_p > 20, the call on a context for a threshold)"""
    S, L = usac.SAMPLER, usac.LocOpt
    cases = {
        "run": (False, lambda c, t, sd: c.run(_model(usac, kind, t), seeds=sd)),
        "run_polished": (False, lambda c, t, sd: c.run(_model(usac, kind, t), seeds=sd, polish=True)),
        "run_prosac": (True, lambda c, t, sd: c.run_prosac(_model(usac, kind, t, S.Prosac), seeds=sd, polish=True)),
    }
    if kind == "E":
        return cases
    for lo in (L.InItLORsc, L.InItFLORsc):
        cases["run_lo_%s_uniform" % lo.name] = (
            False, lambda c, t, sd, lo=lo: c.run_lo(_model(usac, kind, t, lo=lo), seeds=sd, polish=True))
        cases["run_lo_%s_prosac" % lo.name] = (
            True, lambda c, t, sd, lo=lo: c.run_lo(_model(usac, kind, t, S.Prosac, lo=lo), seeds=sd))
    cases["run_sprt"] = (False, lambda c, t, sd: c.run_sprt(_model(usac, kind, t, sprt=True), seeds=sd, polish=True))
    cases["run_sprt_prosac"] = (True, lambda c, t, sd: c.run_sprt(_model(usac, kind, t, S.Prosac, sprt=True), seeds=sd))
    cases["run_napsac"] = (False, lambda c, t, sd: c.run_napsac(_model(usac, kind, t, napsac=True), seeds=sd, polish=True))
    cases["run_napsac_lo"] = (
        False, lambda c, t, sd: c.run_napsac(_model(usac, kind, t, napsac=True, lo=L.InItLORsc), seeds=sd))
    return cases


RUN_NAMES = {"E": ["run", "run_polished", "run_prosac"]}
RUN_NAMES["H"] = RUN_NAMES["F"] = RUN_NAMES["E"] + [
    "run_lo_InItLORsc_uniform", "run_lo_InItLORsc_prosac", "run_lo_InItFLORsc_uniform", "run_lo_InItFLORsc_prosac",
    "run_sprt", "run_sprt_prosac", "run_napsac", "run_napsac_lo"]


@pytest.mark.parametrize("kind,name", [(k, n) for k in ("H", "F", "E") for n in RUN_NAMES[k]])
def test_run_equals_one_problem_runs(usac, worlds, kind, name):
    tail, call = _run_cases(usac, kind)[name]
    w = worlds[kind][1 if tail else 0]
    off = 1 if tail else 0
    T, seeds, pools = THRS[kind][off:], SEEDS[off:], POOLS[off:]
    if "sprt" in name:
        w.mc.set_sprt_pool(pools)
        for p, one in enumerate(w.ones):
            one.set_sprt_pool([pools[p]])
    with thresholds(w.mc, T):
        got = call(w.mc, SCALAR[kind], seeds)
        again = call(w.mc, SCALAR[kind], seeds)
    assert len(got) == w.P
    _same(again, got, (kind, name, "second call"))
    for p, one in enumerate(w.ones):
        want = call(one, T[p], [seeds[p]])[0]
        _same(got[p], want, (kind, name, p))
    # the copy and its original ran the same hypotheses under two thresholds
    d, o = DUP[0] - off, DUP[1] - off
    assert got[d]["best"]["inliers"] != got[o]["best"]["inliers"] or "sprt" in name
    assert sum(g["best"]["inliers"] for g in got) > 0
    if "lo" in name:
        assert any(g["lo"]["lo_calls"] > 0 for g in got)


# ------------------------------------------------------------------ 4. the LO cap
def test_lo_cap_returns_to_the_problems_threshold(usac, worlds):
    kind = "H"
    # about 4500 inliers at 0.3 px noise: the iterative stage's first list to fit is past kPolFitMax = 4096
    big = synthetic.homography_points(n=5000, inlier_ratio=0.9, seed=78, noise=0.3)[0]
    sets = _sets(kind)[3:5] + [big]
    T, seeds = [1.5, 2.5, 3.0], [13, 14, 31]
    lo = usac.LocOpt.InItLORsc
    with _multi(usac, kind, sets) as mc:
        mc.set_thresholds(T)
        got = mc.run_lo(_model(usac, kind, SCALAR[kind], lo=lo), seeds=seeds)
        for p, pts in enumerate(sets):
            with _multi(usac, kind, [pts]) as one:
                want = one.run_lo(_model(usac, kind, T[p], lo=lo), seeds=[seeds[p]])[0]
            _same(got[p], want, (kind, "cap", p))
    st = got[2]["lo"]
    print("LO cap: capped %d, lo_calls %d, threshold %r" % (st["capped"], st["lo_calls"], st["threshold"]))
    assert st["capped"] >= 1
    assert _bits(st["threshold"]) == _bits(np.float32(T[2])) != _bits(np.float32(SCALAR[kind]))


# ------------------------------------------------------------------ 5. the hooks
@pytest.mark.parametrize("kind", ["H", "F", "E"])
def test_prosac_scan_hook(usac, worlds, kind):
    w = worlds[kind][1]
    T, seeds = THRS[kind][1:], SEEDS[1:]
    S = usac.SAMPLER
    with thresholds(w.mc, T):
        models, _ = _round_models(w.mc, kind, seeds, SCALAR[kind])
        hc, lg = [R] * w.P, [M[kind]] * w.P
        bound, tl, segs = w.mc.prosac_scan(_model(usac, kind, SCALAR[kind], S.Prosac), models, hc, lg, reset=True)
    for p, one in enumerate(w.ones):
        b1, t1, s1 = one.prosac_scan(_model(usac, kind, T[p], S.Prosac), models[p:p + 1], hc[:1], lg[:1], reset=True)
        assert (bound[p], tl[p]) == (b1[0], t1[0]), (kind, p)
        np.testing.assert_array_equal(segs[p], s1[0], err_msg=str((kind, p)))
    d, o = DUP[0] - 1, DUP[1] - 1
    assert len(segs[d]) != len(segs[o]) or (segs[d] != segs[o]).any()


@pytest.mark.parametrize("kind", ["H", "F"])
@pytest.mark.parametrize("limited", [False, True])
def test_lo_hook_compounds_per_problem(usac, worlds, kind, limited):
    w = worlds[kind][0]
    T = THRS[kind]
    lo = usac.LocOpt.InItFLORsc if limited else usac.LocOpt.InItLORsc
    with thresholds(w.mc, T):
        _, recs = _round_models(w.mc, kind, SEEDS, SCALAR[kind])  # counts and Σ at t_p
        m = _model(usac, kind, SCALAR[kind], lo=lo)
        r1, s1 = w.mc.lo(m, recs, seeds=DRAWS, reset=True)
        r2, s2 = w.mc.lo(m, r1, seeds=DRAWS, reset=False)
    for p, one in enumerate(w.ones):
        mp = _model(usac, kind, T[p], lo=lo)
        q1, t1 = one.lo(mp, [recs[p]], seeds=[DRAWS[p]], reset=True)
        q2, t2 = one.lo(mp, q1, seeds=[DRAWS[p]], reset=False)
        _same([r1[p], s1[p], r2[p], s2[p]], [q1[0], t1[0], q2[0], t2[0]], (kind, limited, p))
    assert sum(s["fits"] for s in s2) > 0
    assert len({_bits(s["threshold"]).item() for s in s2}) > 1  # the problems' LO thresholds differ


# ------------------------------------------------------------------ 6. equal thresholds
def _everything(usac, w, kind, thr):
    """every entry point that reads a threshold, at the scalar thr"""
    mc, S, L = w.mc, usac.SAMPLER, usac.LocOpt
    seeds = SEEDS[1:]
    out = {"round": mc.hypothesize_score(R, seeds, first_hyp=R, thr=thr)}
    models, recs = _round_models(mc, kind, seeds, thr)
    out["inliers"] = mc.inliers(models, thr)
    out["polish"] = mc.polish(models, thr, with_inliers=True)
    out["run"] = mc.run(_model(usac, kind, thr), polish=True)
    out["run_prosac"] = mc.run_prosac(_model(usac, kind, thr, S.Prosac))
    out["scan"] = mc.prosac_scan(_model(usac, kind, thr, S.Prosac), models, [R] * w.P, [M[kind]] * w.P, reset=True)
    if kind == "E":
        return out
    out["round_sprt"] = mc.hypothesize_score_sprt(R, seeds, first_hyp=R, thr=thr)
    out["round_napsac"] = mc.hypothesize_score_napsac(R, seeds, CELL[kind], first_hyp=R, thr=thr)
    out["lo"] = mc.lo(_model(usac, kind, thr, lo=L.InItLORsc), recs, seeds=DRAWS[1:], reset=True)
    out["run_lo"] = mc.run_lo(_model(usac, kind, thr, S.Prosac, lo=L.InItFLORsc), polish=True)
    out["run_sprt"] = mc.run_sprt(_model(usac, kind, thr, sprt=True))
    out["run_napsac"] = mc.run_napsac(_model(usac, kind, thr, napsac=True, lo=L.InItLORsc))
    return out


@pytest.mark.parametrize("kind", ["H", "F", "E"])
def test_equal_thresholds_change_nothing(usac, worlds, kind):
    w = worlds[kind][1]
    thr = THRS[kind][3]
    assert w.mc.thresholds is None
    before = _everything(usac, w, kind, thr)
    w.mc.set_thresholds([thr] * w.P)
    try:
        assert (w.mc.thresholds == np.full(w.P, thr, np.float32)).all()
        _same(_everything(usac, w, kind, thr), before, (kind, "equal thresholds"))
        _same(_everything(usac, w, kind, SCALAR[kind]), before, (kind, "equal thresholds, another scalar"))
    finally:
        w.mc.set_thresholds(None)
    assert w.mc.thresholds is None
    _same(_everything(usac, w, kind, thr), before, (kind, "after the clear"))


# ------------------------------------------------------------------ 7. errors
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_bad_threshold_is_refused_and_changes_nothing(usac, worlds, bad):
    w = worlds["H"][0]
    model = _model(usac, "H", SCALAR["H"])
    with thresholds(w.mc, THRS["H"]):
        before = w.mc.run(model, polish=True)
        for pos in (0, 3, w.P - 1):
            t = list(THRS["H"])
            t[pos] = bad
            with pytest.raises(usac.UsacError) as e:
                w.mc.set_thresholds(t)
            assert e.value.code == -1
            assert "problem %d" % pos in str(e.value), str(e.value)
            assert (w.mc.thresholds == np.asarray(THRS["H"], np.float32)).all()
        _same(w.mc.run(model, polish=True), before, "after the refusals")
    # with nothing set before, nothing is set after
    with pytest.raises(usac.UsacError):
        w.mc.set_thresholds([bad] * w.P)
    assert w.mc.thresholds is None


def test_essential_refusals_are_unchanged(usac, worlds):
    w = worlds["E"][0]
    L = usac.LocOpt
    E = usac.ESTIMATOR.Essential

    def em(**kw):
        model = usac.Model(SCALAR["E"], 5, PROB, 5, E, kw.pop("sampler", usac.SAMPLER.Uniform))
        model.max_iterations, model.batch, model.seed = MAX_IT, R, 300
        for k, v in kw.items():
            setattr(model, k, v)
        return model

    napsac = em(sampler=usac.SAMPLER.Napsac, neighborsType=usac.NeighborsSearch.Grid)
    _, recs = _round_models(w.mc, "E", SEEDS, THRS["E"][3])
    with thresholds(w.mc, THRS["E"]):
        for call in (lambda: w.mc.run_lo(em(lo=L.InItLORsc)), lambda: w.mc.run_sprt(em(sprt=True)),
                     lambda: w.mc.run_napsac(napsac), lambda: w.mc.lo(em(lo=L.InItLORsc), recs),
                     lambda: w.mc.hypothesize_score_sprt(R, SEEDS, thr=SCALAR["E"]),
                     lambda: w.mc.hypothesize_score_napsac(R, SEEDS, 50, thr=SCALAR["E"])):
            with pytest.raises(usac.UsacError) as e:
                call()
            assert e.value.code == -3
        assert (w.mc.thresholds == np.asarray(THRS["E"], np.float32)).all()
