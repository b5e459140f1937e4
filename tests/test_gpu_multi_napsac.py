"""NAPSAC for multi-problem batches (usac_multi_grid, usac_multi_draw_samples_napsac,
usac_multi_hypothesize_score_napsac, usac_multi_run_napsac; ABI 20).  Every per-problem output is
compared bit for bit with the single-problem path: the grid CSR with Context.grid_neighbors and the
numpy restatement of the host GridNeighbors, the samples and a round with a Context under the NAPSAC
device sampler, the run with its loop restated over single contexts (with LO: over the multi context's
own hooks), and the run's place among the other runs of the shared round driver."""
import ctypes

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import multi_lo_ref as lo_ref
from tests.helpers import multi_polish_ref as pref
from tests.helpers.grid_ref import grid_csr
from tests.test_gpu_multi_driver import _outputs, _same

pytestmark = pytest.mark.gpu

THR = 2.0
M = {"H": 4, "F": 7}
SIZES = {"H": [4, 64, 65, 333, 1000], "F": [7, 64, 65, 333, 1000]}
RATIOS = [0.9, 0.3, 0.3, 0.0, 0.3]
DATA_SEEDS = {"H": [20, 21, 22, 23, 24], "F": [22, 31, 32, 33, 34]}
CELL = {"H": 50, "F": 400}
# points with >= m grid neighbours (numpy cell count): problems that draw NAPSAC samples, problems
# that fall back to uniform ones, and n_p = m
ELIGIBLE = {"H": [0, 0, 6, 0, 287], "F": [0, 8, 0, 151, 844]}
DUP = (5, 3)                       # problem 5 is a copy of problem 3 (the 333-point set)
SEEDS = [11, 12, 13, 14, 15, 14]   # sampler seeds: the copy shares its original's
GRID_MAX = 4000                    # kMultiGridMax: a larger problem's grid is built on the host


def _est(usac, kind):
    return usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental


def _sets(kind):
    out = []
    for n, ratio, seed in zip(SIZES[kind], RATIOS, DATA_SEEDS[kind]):
        if kind == "H":
            out.append(synthetic.homography_points(n=n, inlier_ratio=ratio, seed=seed, cluster=(500, 500, 40))[0])
        else:
            out.append(synthetic.fundamental_points(n=n, inlier_ratio=ratio, seed=seed, prosac_order=False)[0])
    out.append(out[DUP[1]].copy())
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_record(a, b, what=""):
    assert a["hyp_index"] == b["hyp_index"] and a["inliers"] == b["inliers"] and a["valid"] == b["valid"], (what, a, b)
    assert _bits(a["score"]) == _bits(b["score"]), (what, a, b)
    np.testing.assert_array_equal(_bits(a["model"]), _bits(b["model"]), err_msg=str(what))


def _same_scores(c, s, rc, rs):
    np.testing.assert_array_equal(c, rc)
    ok = rc >= 0
    np.testing.assert_array_equal(_bits(s)[ok], _bits(rs)[ok])
    assert (s[~ok] == 0).all()


def _same_grid(got, want, what):
    for k in ("cell", "rank", "start", "members", "eligible"):
        assert got[k].dtype == want[k].dtype, (what, k)
        np.testing.assert_array_equal(got[k], want[k], err_msg=str((what, k)))


def _single_grid(usac, kind, pts, cs):
    with usac.Context(_est(usac, kind), pts) as ctx:
        return ctx.grid_neighbors(cs)


@pytest.fixture(scope="module")
def problems(usac):
    """kind -> (point sets, MultiContext, the single contexts under the NAPSAC device sampler)"""
    made = {}
    for kind in ("H", "F"):
        sets = _sets(kind)
        singles = [usac.Context(_est(usac, kind), p) for p in sets]
        for c in singles:
            c.set_cell_size(CELL[kind])
            c.set_device_sampler(usac.SAMPLER.Napsac)
        made[kind] = (sets, usac.MultiContext(_est(usac, kind), sets), singles)
    yield made
    for _, mc, singles in made.values():
        mc.close()
        for c in singles:
            c.close()


def test_point_sets_cover_napsac_and_uniform_problems():
    for kind in ("H", "F"):
        got = [len(grid_csr(p, CELL[kind], M[kind])["eligible"]) for p in _sets(kind)]
        assert got == ELIGIBLE[kind] + [ELIGIBLE[kind][DUP[1]]], kind


# ------------------------------------------------------------------ 1. grid == single context == host CSR
@pytest.mark.parametrize("kind,sizes", [("H", (50, 7, 50)), ("F", (400, 400))])
def test_grid_equals_single_context_and_host_csr(usac, kind, sizes):
    sets = _sets(kind)
    with usac.MultiContext(_est(usac, kind), sets) as mc:
        seen = {}
        for cs in sizes:
            g = mc.grid_neighbors(cs)
            assert len(g) == len(sets)
            for p, pts in enumerate(sets):
                _same_grid(g[p], _single_grid(usac, kind, pts, cs), (kind, cs, p, "single"))
                _same_grid(g[p], grid_csr(pts, cs, M[kind]), (kind, cs, p, "host"))
            if cs in seen:  # asked again (at once, or after another size was built in between)
                _same(g, seen[cs], (kind, cs, "again"))
            seen[cs] = g
            if cs == CELL[kind]:
                assert [len(q["eligible"]) for q in g] == ELIGIBLE[kind] + [ELIGIBLE[kind][DUP[1]]]
        if len(seen) > 1:  # another size gave another grid
            a, b = (seen[cs] for cs in sorted(seen))
            assert any(len(x["start"]) != len(y["start"]) for x, y in zip(a, b))


# ------------------------------------------------------------------ 2. caps and deferral
def test_grid_past_the_caps_takes_the_host_path(usac):
    sets = _sets("H")
    rng = np.random.default_rng(5)
    big = rng.uniform(0, 300, (GRID_MAX + 1, 4)).astype(np.float32)   # cells are shared
    inf = sets[2].copy()
    inf[7] = [np.inf, 1.0, 2.0, 3.0]
    far = sets[2].copy()
    far[11, 2] = 1e12
    mixed = [sets[2], big, sets[1], inf, sets[4], far, sets[2]]
    cs = CELL["H"]
    with usac.MultiContext(usac.ESTIMATOR.Homography, mixed) as mc:
        g = mc.grid_neighbors(cs)
    for p, pts in enumerate(mixed):
        # the single context builds the non-finite and the far set with usac::GridNeighbors on the host
        _same_grid(g[p], _single_grid(usac, "H", pts, cs), (p, "single"))
        if p not in (3, 5):
            _same_grid(g[p], grid_csr(pts, cs, 4), (p, "host"))
    assert len(g[1]["eligible"]) > 0 and len(g[1]["start"]) - 1 < len(big)
    assert [len(g[p]["eligible"]) for p in (0, 2, 4, 6)] == [6, 0, 287, 6]


# ------------------------------------------------------------------ 3. samples
@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("kind", ["H", "F"])
def test_samples_equal_single_context(usac, problems, kind, R):
    sets, mc, singles = problems[kind]
    cs, m = CELL[kind], M[kind]
    grid = mc.grid_neighbors(cs)
    act = [4, 0, 2, 5, 3, 1, 4]  # another order, problem 4 twice
    seeds = [SEEDS[p] for p in act[:-1]] + [99]
    for f in (0, 3 * R):
        got = mc.draw_samples_napsac(R, seeds, cs, first_hyp=f, problems=act)
        assert got.shape == (len(act), R, m)
        uni = mc.draw_samples(R, seeds, first_hyp=f, problems=act)
        for a, p in enumerate(act):
            np.testing.assert_array_equal(got[a], singles[p].draw_samples(R, seeds[a], first_hyp=f), err_msg=str((a, p)))
            s = np.sort(got[a], axis=1)
            assert (s[:, 1:] != s[:, :-1]).all() and s.min() >= 0 and s.max() < len(sets[p])
            if len(grid[p]["eligible"]) == 0:
                np.testing.assert_array_equal(got[a], uni[a])
            else:
                cells = grid[p]["cell"][got[a]]
                assert (cells == cells[:, :1]).all()
                assert np.isin(got[a][:, 0], grid[p]["eligible"]).all()
                assert (got[a] != uni[a]).any()
        assert (got[0] != got[-1]).any()  # the duplicate entry under another seed
    # all problems in order, the default list
    full = mc.draw_samples_napsac(R, SEEDS, cs)
    for p, ctx in enumerate(singles):
        np.testing.assert_array_equal(full[p], ctx.draw_samples(R, SEEDS[p]))


# ------------------------------------------------------------------ 4. round
@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_round_equals_single_context(usac, problems, kind, dlt, R):
    sets, mc, singles = problems[kind]
    mc.set_dlt_mode(dlt)
    try:
        for f in (0, 3 * R):
            c, s, best = mc.hypothesize_score_napsac(R, SEEDS, CELL[kind], first_hyp=f, thr=THR)
            assert c.shape == (len(sets), R * mc.spk)
            for p, ctx in enumerate(singles):
                ctx.set_dlt_mode(dlt)
                rc, rs, rbest = ctx.hypothesize_score(B=R, seed=SEEDS[p], first_hyp=f, thr=THR, per_hypothesis=True)
                ctx.set_dlt_mode(0)
                _same_scores(c[p], s[p], rc, rs)
                _same_record(best[p], rbest, (kind, dlt, R, f, p))
        # an active list, records alone
        act = [4, 2]
        _, _, ba = mc.hypothesize_score_napsac(R, [SEEDS[p] for p in act], CELL[kind], first_hyp=3 * R, thr=THR,
                                               problems=act, per_hypothesis=False)
        for a, p in enumerate(act):
            _same_record(ba[a], best[p], (kind, "active", p))
    finally:
        mc.set_dlt_mode(0)


# ------------------------------------------------------------------ 5. run
RUN_R, RUN_MAX, RUN_PROB = 64, 512, 0.95


def _record(usac, d):
    return usac.Record(d["hyp_index"], d["inliers"], d["score"], (ctypes.c_float * 9)(*np.asarray(d["model"]).tolist()),
                       int(d["valid"]))


def _run_model(usac, kind, dlt=0, lo=None):
    model = usac.Model(THR, M[kind], RUN_PROB, 5, _est(usac, kind), usac.SAMPLER.Napsac)
    model.setNeighborsType(usac.NeighborsSearch.Grid)
    model.setCellSize(CELL[kind])
    model.max_iterations, model.batch, model.seed = RUN_MAX, RUN_R, 100
    model.setDLTMode(dlt)
    if lo is not None:
        model.lo = lo
        model.lo_sample_size = 14
        model.setLOParametres(4, 10, 10)
    return model


def _restated_run(usac, ctx, m, seed, dlt):
    """usac_multi_run_napsac's loop for one problem, over a single context under the NAPSAC device sampler"""
    ctx.set_dlt_mode(dlt)
    best, r = None, 0
    while True:
        rec = _record(usac, ctx.hypothesize_score(B=RUN_R, seed=seed, first_hyp=r * RUN_R, thr=THR, per_hypothesis=True)[2])
        best = rec if best is None else usac.merge_records([best, rec])
        bound = usac.std_termination(best.inliers, ctx.n, m, RUN_PROB, RUN_MAX)
        r += 1
        if r * RUN_R >= min(RUN_MAX, bound):
            break
    ctx.set_dlt_mode(0)
    return {"best": best.as_dict(), "rounds": r, "hypotheses": r * RUN_R, "bound": bound,
            "status": 0 if best.inliers > 0 else -111}


@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_run_equals_restated_loop(usac, problems, kind, dlt):
    _, mc, singles = problems[kind]
    model = _run_model(usac, kind, dlt)
    got = mc.run_napsac(model, polish=True)
    assert "lo" not in got[0]
    for p, ctx in enumerate(singles):
        want = _restated_run(usac, ctx, mc.m, model.seed + p, dlt)
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert got[p][key] == want[key], (p, key, got[p], want)
        _same_record(got[p]["best"], want["best"], (kind, dlt, p))
    assert any(g["rounds"] > 1 for g in got) and any(g["rounds"] < RUN_MAX // RUN_R for g in got)
    # polish=True: mc.polish of the run's best models
    pol = mc.polish(np.stack([g["best"]["model"] for g in got]), THR, with_inliers=True)
    for p in range(mc.P):
        pref.assert_same_polish(got[p]["polished"], pol[p], p)
        np.testing.assert_array_equal(got[p]["inliers"], pol[p]["inlier_idx"])
    # explicit seeds, no polish: the same run
    again = mc.run_napsac(model, seeds=[model.seed + p for p in range(mc.P)])
    assert "polished" not in again[0]
    for p in range(mc.P):
        assert again[p]["rounds"] == got[p]["rounds"]
        _same_record(again[p]["best"], got[p]["best"], p)


def _restated_lo_run(usac, mc, model, cs):
    """usac_multi_run_napsac with LO, round by round over the context's own hooks: the NAPSAC samples, their
    round, the merge, one LO call on the round's new bests (the others go in invalid: skipped), the bound"""
    P, m = mc.P, mc.m
    nothing = {"hyp_index": 0, "inliers": 0, "score": 0.0, "model": np.zeros(9, np.float32), "valid": 0}
    best, out, states = [None] * P, [None] * P, None
    active, r = list(range(P)), 0
    while active:
        first = r * RUN_R
        seeds = [model.seed + p for p in active]
        samples = mc.draw_samples_napsac(RUN_R, seeds, cs, first_hyp=first, problems=active)
        _, _, recs = mc.hypothesize_score(RUN_R, first_hyp=first, thr=THR, problems=active, samples=samples,
                                          per_hypothesis=False)
        new = []
        for a, p in enumerate(active):
            rec = _record(usac, recs[a])
            best[p] = rec if best[p] is None else usac.merge_records([best[p], rec])
            if best[p].valid and best[p].hyp_index >= first:
                new.append(p)
        lo_recs, states = mc.lo(model, [best[p] if p in new else nothing for p in range(P)], reset=(r == 0))
        for p in new:
            best[p] = _record(usac, lo_recs[p])
        r += 1
        keep = []
        for p in active:
            bound = usac.std_termination(best[p].inliers, int(mc.sizes[p]), m, RUN_PROB, RUN_MAX)
            if r * RUN_R >= min(RUN_MAX, bound):
                out[p] = {"best": best[p].as_dict(), "rounds": r, "hypotheses": r * RUN_R, "bound": bound,
                          "status": 0 if best[p].inliers > 0 else -111}
            else:
                keep.append(p)
        active = keep
    for p in range(P):
        out[p]["lo"] = states[p]
    return out


@pytest.mark.parametrize("kind", ["H", "F"])
def test_run_with_lo_equals_restated_loop_over_the_hooks(usac, problems, kind):
    _, mc, _ = problems[kind]
    model = _run_model(usac, kind, lo=usac.LocOpt.InItLORsc)
    got = mc.run_napsac(model)
    want = _restated_lo_run(usac, mc, model, CELL[kind])
    for p in range(mc.P):
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert got[p][key] == want[p][key], (p, key, got[p], want[p])
        lo_ref.assert_same_record(got[p]["best"], want[p]["best"], p)
        lo_ref.assert_same_state(got[p]["lo"], want[p]["lo"], p)
    assert any(g["lo"]["lo_calls"] > 0 for g in got)


# ------------------------------------------------------------------ 6. driver state
def _driver_model(usac, kind, sampler, lo=False, sprt=False):
    if sampler == usac.SAMPLER.Napsac:
        model = _run_model(usac, kind, lo=usac.LocOpt.InItLORsc if lo else None)
    elif lo:
        model = lo_ref.make_model(usac, kind, sampler=sampler)
    else:
        model = usac.Model(THR, M[kind], RUN_PROB, 5, _est(usac, kind), sampler)
    model.max_iterations, model.batch, model.seed = RUN_MAX, RUN_R, 300
    model.setSprt(sprt)
    return model


@pytest.mark.parametrize("kind", ["H", "F"])
def test_interleaved_runs_equal_fresh_contexts(usac, kind):
    sets = _sets(kind)[1:]  # every n_p > 20: PROSAC runs on them too
    est, S = _est(usac, kind), usac.SAMPLER

    def fresh(call):
        with usac.MultiContext(est, sets) as other:
            return call(other)

    runs = [
        lambda c: c.run_napsac(_driver_model(usac, kind, S.Napsac)),
        lambda c: c.run(_driver_model(usac, kind, S.Uniform)),
        lambda c: c.run_napsac(_driver_model(usac, kind, S.Napsac, lo=True), polish=True),
        lambda c: c.run_prosac(_driver_model(usac, kind, S.Prosac)),
        lambda c: c.run_napsac(_driver_model(usac, kind, S.Napsac)),
        lambda c: c.run_lo(_driver_model(usac, kind, S.Uniform, lo=True)),
        lambda c: c.run_sprt(_driver_model(usac, kind, S.Uniform, sprt=True)),
        lambda c: c.run_napsac(_driver_model(usac, kind, S.Napsac, lo=True)),
        lambda c: c.run(_driver_model(usac, kind, S.Uniform), polish=True),
    ]
    with usac.MultiContext(est, sets) as mc:
        got = []
        for step, call in enumerate(runs):
            got.append(call(mc))
            assert len(got[-1]) == len(sets)
            _same(got[-1], fresh(call), (kind, "step", step))
            if step == 3:  # another cell size in between: the next NAPSAC run rebuilds its grid
                mc.grid_neighbors(CELL[kind] + 3)
    assert "lo" in got[2][0] and "polished" in got[2][0] and "lo" not in got[0][0]
    assert any(g["lo"]["lo_calls"] > 0 for g in got[2]) and any(g["lo"]["lo_calls"] > 0 for g in got[7])
    _same(got[0], got[4], (kind, "the run again"))


@pytest.mark.parametrize("lo", [False, True])
def test_null_outputs(usac, lo):
    sets = _sets("H")
    L, P = usac.lib(), len(sets)
    n_total = sum(len(s) for s in sets)
    model = _run_model(usac, "H", lo=usac.LocOpt.InItLORsc if lo else None)
    prm = usac._params(model)
    prm.seed = model.seed
    with usac.MultiContext(usac.ESTIMATOR.Homography, sets) as mc:
        full, bare = (usac._MultiOutput * P)(), (usac._MultiOutput * P)()
        mask = np.zeros(n_total, dtype=np.uint8)
        rc = L.usac_multi_run_napsac(mc._h, ctypes.byref(prm), None, full, (usac._MultiLoOutput * P)(),
                                     (usac._MultiPolishOutput * P)(), mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        assert rc == 0
        assert L.usac_multi_run_napsac(mc._h, ctypes.byref(prm), None, bare, None, None, None) == 0
        _same(_outputs(bare), _outputs(full), lo)
        assert any(o.rounds > 1 for o in full) and all(o.hypotheses > 0 for o in full)
        # the grid call with every output NULL builds (or keeps) the grid and returns
        assert L.usac_multi_grid(mc._h, CELL["H"], None, None, None, None, None, None, None) == 0


# ------------------------------------------------------------------ 7. error codes
def test_run_napsac_error_codes_leave_the_context_alone(usac):
    sets = _sets("H")
    good = _run_model(usac, "H")
    with usac.MultiContext(usac.ESTIMATOR.Homography, sets) as other:
        want = other.run_napsac(good)
    changes = [
        (lambda m: setattr(m, "sampler", usac.SAMPLER.Uniform), -1),
        (lambda m: setattr(m, "sampler", usac.SAMPLER.Prosac), -1),
        (lambda m: m.setNeighborsType(usac.NeighborsSearch.Nanoflann), -3),
        (lambda m: m.setCellSize(0), -1),
        (lambda m: m.setSprt(True), -3),
        (lambda m: setattr(m, "lo", usac.LocOpt.GC), -3),
        (lambda m: setattr(m, "batch", 100), -1),
    ]
    with usac.MultiContext(usac.ESTIMATOR.Homography, sets) as mc:
        for change, code in changes:
            model = _run_model(usac, "H")
            change(model)
            with pytest.raises(usac.UsacError) as e:
                mc.run_napsac(model)
            assert e.value.code == code, (code, str(e.value))
            _same(mc.run_napsac(good), want, ("after the refused run", code))
        # the hooks: a bad cell size, a bad R, seeds missing
        for call in (lambda: mc.draw_samples_napsac(64, SEEDS, 0), lambda: mc.draw_samples_napsac(96, SEEDS, 50),
                     lambda: mc.hypothesize_score_napsac(64, SEEDS, -5), lambda: mc.grid_neighbors(0)):
            with pytest.raises(usac.UsacError) as e:
                call()
            assert e.value.code == -1
        # the other runs keep refusing the NAPSAC sampler with their codes
        for call, code in ((mc.run, -3), (mc.run_prosac, -1), (mc.run_lo, -1), (mc.run_sprt, -1)):
            model = _run_model(usac, "H")
            if call == mc.run_lo:
                model.lo = usac.LocOpt.InItLORsc
            if call == mc.run_sprt:
                model.setSprt(True)
            with pytest.raises(usac.UsacError) as e:
                call(model)
            assert e.value.code == code, call
        _same(mc.run_napsac(good), want, "after the hooks")
