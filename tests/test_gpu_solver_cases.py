"""Solver parity on degenerate samples and across dataset geometries: the minimal solvers (4-point DLT in
both modes, 7-point, 5-point), their multi-problem copies, the non-minimal fits (normalised DLT, 8-point
algorithm, the weighted overloads) and the multi-problem polish, on the tables of
tests/helpers/solver_cases.py, against the CPU oracle on the same fp32 inputs.

Every comparison is exact (solver_cases.assert_same_floats): equal bit patterns, -0 is not +0, a NaN
where the oracle has one (payload and sign free), equal model counts per sample; nothing is skipped,
filtered or retried.  tests/test_solver_cases_cpu.py shows from the oracle's path counters that the
tables reach the branches they are here for (the 7- and 5-point null-space fall-backs with models, every
arm of cubic_roots, F[8] = 0, the second epipole, the trace / converged / slow exits of the eigen spec),
and that each comparison below fails on a wrong expectation."""
import numpy as np
import pytest

from tests.helpers import multi_polish_ref as ref
from tests.helpers import solver_cases as S

pytestmark = pytest.mark.gpu


def _est(usac, kind):
    return {"H": usac.ESTIMATOR.Homography, "F": usac.ESTIMATOR.Fundamental, "E": usac.ESTIMATOR.Essential}[kind]


def _solver_params(rows):
    return [(kind, dlt, name) for kind in S.KINDS for dlt in ((0, 1) if kind == "H" else (0,)) for name in rows(kind)]


def _check_minimal(usac, oracle, kind, dlt, pts, samples, what):
    want, want_nm = oracle.Estimator(S.okind(oracle, kind), pts, dlt).estimate_batch(samples)
    with usac.Context(_est(usac, kind), pts) as ctx:
        if kind == "H":
            ctx.set_dlt_mode(dlt)
        # twice on one context: the fall-back lists carry their counters from call to call
        for call in (1, 2):
            got, got_nm = ctx.estimate_models(samples)
            S.assert_same_models(kind, got, got_nm, want, want_nm, what + (call,))


# ------------------------------------------------------------------ 1. minimal solvers
@pytest.mark.parametrize("kind,dlt,name", _solver_params(lambda kind: S.GEOMETRY_ROWS[kind]))
def test_minimal_solvers_on_geometry_rows(usac, oracle, kind, dlt, name):
    pts, _, _, samples = S.geometry_row(oracle, kind, name)
    _check_minimal(usac, oracle, kind, dlt, pts, samples, (kind, dlt, name))


@pytest.mark.parametrize("kind,dlt,name", _solver_params(S.sample_table_names))
def test_minimal_solvers_on_sample_tables(usac, oracle, kind, dlt, name):
    pts, samples = S.sample_table(oracle, kind, name)
    _check_minimal(usac, oracle, kind, dlt, pts, samples, (kind, dlt, name))


# ------------------------------------------------------------------ 2. multi kernels
# six problems from the tables (i)-(iv); the first two are fall-back tables (H: repeated points make the
# 4-point DLT's QR refuse)
MULTI_TABLES = ("rep_one", "all_equal", "same_view", "lattice", "scale_1e-10", "nan_rows")


@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0), ("E", 0)])
def test_multi_round_on_degenerate_tables(usac, oracle, kind, dlt):
    tables = [S.sample_table(oracle, kind, name) for name in MULTI_TABLES]
    sets = [pts for pts, _ in tables]
    samples = np.stack([smp for _, smp in tables])
    thr = S.THR[kind]
    want = [S.round_expectation(oracle, kind, pts, smp, thr, dlt) for pts, smp in tables]
    # from the oracle: the fall-back tables' rounds have occupied slots, and some round has an empty one
    assert all(w["occupied"].any() for w in want[:2])
    if kind != "H":
        assert any(not w["occupied"].all() for w in want)
    mc = usac.MultiContext.essential(sets) if kind == "E" else usac.MultiContext(_est(usac, kind), sets)
    with mc:
        mc.set_dlt_mode(dlt)
        for call in (1, 2):
            c, s, best = mc.hypothesize_score(S.NS, thr=thr, samples=samples)
            for p, name in enumerate(MULTI_TABLES):
                S.assert_same_round(c[p], s[p], best[p], want[p], (kind, dlt, name, call))


# ------------------------------------------------------------------ 3. non-minimal fits
def _fit(usac, ctx, idx, weights=None):
    try:
        return ctx.nonminimal(idx) if weights is None else ctx.lsq_fit(idx, weights)
    except usac.UsacError as e:
        return e.code


def _contexts(usac, kind):
    """one context per point set (the tables share their sets)"""
    made = {}

    def get(pts):
        if id(pts) not in made:
            made[id(pts)] = usac.Context(_est(usac, kind), pts)
        return made[id(pts)]

    return made, get


@pytest.mark.parametrize("kind", S.KINDS)
def test_nonminimal_fits_on_degenerate_lists(usac, oracle, kind):
    made, get = _contexts(usac, kind)
    failures = []
    try:
        for name, pts, idx in S.fit_cases(kind):
            want = S.fit_expectation(oracle, kind, pts, idx)
            got = _fit(usac, get(pts), idx)
            try:
                S.assert_same_fit(got, want, (kind, name))
            except AssertionError as e:
                failures.append(str(e))
    finally:
        for ctx in made.values():
            ctx.close()
    assert not failures, "%d of %d fits differ:\n%s" % (len(failures), len(S.fit_cases(kind)), "\n".join(failures))


@pytest.mark.parametrize("kind", ["H", "F"])
def test_weighted_fits_on_degenerate_weights(usac, oracle, kind):
    made, get = _contexts(usac, kind)
    failures = []
    try:
        for name, pts, idx, w in S.weight_cases(kind):
            want = S.fit_expectation(oracle, kind, pts, idx, w)
            got = _fit(usac, get(pts), idx, w)
            try:
                S.assert_same_fit(got, want, (kind, name))
            except AssertionError as e:
                failures.append(str(e))
    finally:
        for ctx in made.values():
            ctx.close()
    assert not failures, "%d of %d fits differ:\n%s" % (len(failures), len(S.weight_cases(kind)), "\n".join(failures))


# ------------------------------------------------------------------ 4. polish
@pytest.mark.parametrize("kind", ["H", "F"])
def test_polish_on_degenerate_sets(usac, oracle, kind):
    clean_pts, clean_model = S.base(kind)[:2]
    sets, models, names = [], [], []
    for name, pts, start in S.polish_cases(kind):  # each degenerate set next to a clean one
        sets += [pts, clean_pts]
        models += [start, clean_model]
        names += [name, "clean"]
    models = np.stack(models)
    refs = [ref.polish_ref(ref.estimator(oracle, kind, pts), m, ref.THR) for pts, m in zip(sets, models)]
    # from the reference's dicts: every degenerate set's fit ran and was accepted at least once
    for name, r in zip(names, refs):
        assert r["status"] == 0 and (name == "clean" or r["passes"] >= 1), (name, r["stop"])
    with usac.MultiContext(_est(usac, kind), sets) as mc:
        got = mc.polish(models, ref.THR, with_inliers=True)
    assert len(got) == len(sets) == 12
    for name, g, r in zip(names, got, refs):
        ref.assert_same_polish(g, r, (kind, name))
        S.assert_same_floats(g["model"], r["model"], (kind, name))
