"""Preconditions of tests/test_gpu_solver_cases.py, on the CPU oracle alone: the tables of
tests/helpers/solver_cases.py reach the solver branches they exist for.  The counts come from the
oracle's path counters (oracle.trace_reset / trace_get), which change no result.

Eigen spec exits (usac_oracle.c eig_min_invit).  The fit tables reach "trace", "converged" and "slow".
The other three were looked for and stay unreached from point sets, so no GPU test depends on them:

  Cholesky pivot, nn   the normal matrix is a sum of squares of rows of normalised fp32 points: its
                       rounding error is ~1e-16 of the trace, the shift is 1e-12 of it, and the entries
                       stay within fp32's range, so no pivot goes <= 0 and no solve overflows.  Tried, for
                       H and F with lists of 100 and 300: the whole set and view 1 alone times 10^e,
                       one far point 10^e, and uniform weights 10^e, e = -45 .. 38: only the trace exit
                       (e <= -26 or so, and non-finite), "converged" and "slow" occur.  Both exits are
                       reached below with matrices given directly to the spec (indefinite; denormal),
                       which the device offers no entry for;
  30 steps             unreachable: from the third step on every step must shrink d by 4 or leave as
                       "slow", d <= 2 for unit vectors, and 2 * 4^-22 < 1e-13, so a run ends as
                       "converged" or "slow" by step 25.
"""
import numpy as np
import pytest

from tests.helpers import solver_cases as S

FLOOR = 32  # of 256 samples


def _okind(oracle, kind):
    return {"H": oracle.HOMOGRAPHY, "F": oracle.FUNDAMENTAL, "E": oracle.ESSENTIAL}[kind]


def _per_sample(oracle, kind, name):
    """the path counters of every sample of a table, one dict per sample, and the models per sample"""
    pts, samples = S.sample_table(oracle, kind, name)
    est = oracle.Estimator(_okind(oracle, kind), pts)
    traces, nm = [], []
    for s in samples:
        oracle.trace_reset()
        nm.append(len(est.estimate(s)))
        traces.append(oracle.trace_get())
    return traces, np.array(nm)


def _reached(traces, *fields):
    return sum(any(t[f] for f in fields) for t in traces)


@pytest.fixture(scope="module")
def f_tables(oracle):
    return {name: _per_sample(oracle, "F", name) for name in S.sample_table_names("F")}


# ------------------------------------------------------------------ counters change nothing
def test_counters_are_thread_local_and_inert(oracle):
    import threading
    pts, samples = S.sample_table(oracle, "F", "rep_one")
    est = oracle.Estimator(oracle.FUNDAMENTAL, pts)
    oracle.trace_reset()
    m0, n0 = est.estimate_batch(samples)
    t0 = oracle.trace_get()
    assert t0["f7_fallback"] > 0 and t0["eig_exit"] == -1
    seen = {}

    def other():
        seen["before"] = oracle.trace_get()
        seen["models"] = est.estimate_batch(samples)
        seen["after"] = oracle.trace_get()

    th = threading.Thread(target=other)
    th.start()
    th.join()
    assert oracle.trace_get() == t0                      # another thread's solves are not counted here
    assert seen["before"]["f7_fallback"] == 0
    assert seen["after"]["f7_fallback"] == t0["f7_fallback"]
    S.assert_same_floats(seen["models"][0], m0)          # and the counting run gives the same models
    np.testing.assert_array_equal(seen["models"][1], n0)
    oracle.trace_reset()
    assert not any(v for k, v in oracle.trace_get().items() if k != "eig_exit")


# ------------------------------------------------------------------ 7-point branches
@pytest.mark.parametrize("name,fields", [
    ("rep_one", ("f7_fallback",)), ("rep_m3", ("f7_fallback",)), ("all_equal", ("f7_fallback",)),
    ("same_view", ("cubic_c0_0", "cubic_c0_1", "cubic_c0_2")),
    ("scale_1e-20", ("f8_zero",)), ("scale_1e-10", ("f8_zero",))])
def test_seven_point_tables_reach_their_branch(f_tables, name, fields):
    traces, nm = f_tables[name]
    k = _reached(traces, *fields)
    print(name, fields, "reached on", k, "of", len(traces), "samples; models per sample", np.bincount(nm, minlength=4))
    assert len(traces) == S.NS and k >= FLOOR
    if fields == ("f7_fallback",):
        # the fall-back yields models here (test_nan_rows' fall-back samples end with none)
        assert sum(1 for t, n in zip(traces, nm) if t["f7_fallback"] and n) >= FLOOR


def test_seven_point_models_per_sample_and_cubic_arms(f_tables):
    nm = np.concatenate([v[1] for v in f_tables.values()])
    hist = np.bincount(nm, minlength=4)
    print("F tables, samples with 0, 1, 2, 3 models:", hist)
    assert len(hist) == 4 and (hist > 0).all()
    total = {f: sum(t[f] for tr, _ in f_tables.values() for t in tr) for f in S_FIELDS}
    print("F tables, path counters:", total)
    # every arm of cubic_roots occurs, and the second epipole -- but for the two arms that need an exact
    # tie: c0 == 0 with one root (a linear equation or a double root) and the general arm with two roots
    # (a critical value of exactly 0; geometry row "wide" has four such samples)
    for f in ("cubic_c0_0", "cubic_c0_2", "cubic_d_le0", "cubic_gen_1", "cubic_gen_3", "f8_zero", "epipole2"):
        assert total[f] >= 1, f


S_FIELDS = ("f7_fallback", "cubic_c0_0", "cubic_c0_1", "cubic_c0_2", "cubic_d_le0", "cubic_gen_1", "cubic_gen_2",
            "cubic_gen_3", "f8_zero", "epipole2")


def test_five_point_tables_reach_the_fallback(oracle):
    for name in S.FALLBACK_TABLES + ("nan_rows",):
        traces, nm = _per_sample(oracle, "E", name)
        k = _reached(traces, "e5_fallback")
        with_model = sum(1 for t, n in zip(traces, nm) if t["e5_fallback"] and n)
        print("E", name, "fall-back on", k, "samples,", with_model, "of them with a model")
        assert k >= FLOOR
        if name != "nan_rows":
            assert with_model >= FLOOR


# ------------------------------------------------------------------ eigen spec exits
def _fit_exits(oracle, kind):
    out = {}
    est = {}
    for name, pts, idx in S.fit_cases(kind):
        e = est.setdefault(id(pts), oracle.Estimator(_okind(oracle, kind), pts))
        oracle.trace_reset()
        e.nonminimal(idx)
        t = oracle.trace_get()
        out[name] = (t["eig_exit"], t["eig_steps"])
    if kind != "E":
        for name, pts, idx, w in S.weight_cases(kind):
            e = est.setdefault(id(pts), oracle.Estimator(_okind(oracle, kind), pts))
            oracle.trace_reset()
            e.nonminimal_weighted(idx, w)
            t = oracle.trace_get()
            out["w_" + name] = (t["eig_exit"], t["eig_steps"])
    return out


@pytest.mark.parametrize("kind", S.KINDS)
def test_fit_tables_reach_the_eigen_exits(oracle, kind):
    exits = _fit_exits(oracle, kind)
    names = oracle.EIG_EXITS
    by_exit = {}
    for name, (code, steps) in exits.items():
        by_exit.setdefault("thin" if code < 0 else names[code], []).append((name, steps))
    print(kind, {k: len(v) for k, v in by_exit.items()})
    print(kind, "converged step counts:", sorted({s for _, s in by_exit["converged"]}))
    assert {"trace", "converged", "slow"} <= set(by_exit)
    assert not {"cholesky", "nn", "steps"} & set(by_exit)       # see the docstring
    assert {n for n, _ in by_exit["thin"]} == {"three", "minimal"}  # <= 8 rows: the row Jacobi, no eigen call
    if kind != "E":
        slowest = max(by_exit["converged"], key=lambda v: v[1])
        print(kind, "slowest converged fit:", slowest)
        assert slowest[1] >= 9 and exits["w_three_100"][0] == names.index("converged") and exits["w_three_100"][1] >= 9
    # both sides of the one-workgroup fit, and the superblock list
    for n in S.FIT_SIZES:
        assert exits["inliers_%d" % n][0] == names.index("converged")
        assert exits["first_rows_%d" % n][0] == names.index("slow")
        assert exits["zeros_%d" % n][0] == names.index("trace")
    assert exits["super_%d" % S.N_SUPER][0] == names.index("converged")


def test_cholesky_and_nn_exits_from_matrices(oracle):
    """the two exits no point set reaches, on the oracle's spec alone"""
    indefinite = np.diag([1.0] * 8 + [-0.5])
    oracle.trace_reset()
    v, ok = oracle.sym_eig_min(indefinite)
    assert not ok and oracle.trace_get()["eig_exit"] == oracle.EIG_EXITS.index("cholesky")
    np.testing.assert_array_equal(np.abs(v), np.eye(9)[8])  # the Jacobi fall-back's answer
    denormal = np.eye(9) * 1e-310
    oracle.trace_reset()
    _, ok = oracle.sym_eig_min(denormal)
    t = oracle.trace_get()
    assert not ok and (t["eig_exit"], t["eig_steps"]) == (oracle.EIG_EXITS.index("nn"), 1)


# ------------------------------------------------------------------ geometry rows
@pytest.mark.parametrize("kind", S.KINDS)
def test_geometry_rows_give_models(oracle, kind):
    for name in S.GEOMETRY_ROWS[kind]:
        pts, _, _, samples = S.geometry_row(oracle, kind, name)
        assert samples.shape == (S.NS, S.M[kind]) and samples.min() >= 0 and samples.max() < len(pts) <= 1500
        models, nm = oracle.Estimator(_okind(oracle, kind), pts).estimate_batch(samples)
        with_model = int((nm > 0).sum())
        finite = int((np.isfinite(models.reshape(S.NS, -1)).all(1) & (nm > 0)).sum())
        print(kind, name, "samples with a model:", with_model, "with finite models only:", finite)
        if name in S.GEOMETRY_EMPTY:
            # empty on purpose: the two-view solvers return nothing, the DLT its one model, not finite
            assert finite == 0 and with_model == (S.NS if kind == "H" else 0)
        else:
            assert with_model >= 16


# ------------------------------------------------------------------ the helper itself
def test_tables_are_deterministic_and_read_only(oracle):
    for kind in S.KINDS:
        names = S.sample_table_names(kind)
        assert len(names) == len(set(names))
        for name in names:
            pts, samples = S.sample_table(oracle, kind, name)
            assert pts.shape == (S.N_SET, 4) and pts.dtype == np.float32 and not pts.flags.writeable
            assert samples.shape == (S.NS, S.M[kind]) and samples.dtype == np.int32 and not samples.flags.writeable
            assert samples.min() >= 0 and samples.max() < S.N_SET
            p2, s2 = S.sample_table(oracle, kind, name)
            S.assert_same_floats(p2, pts)
            np.testing.assert_array_equal(s2, samples)
        for name, pts, idx in S.fit_cases(kind):
            assert not idx.flags.writeable and idx.min() >= 0 and idx.max() < len(pts) <= 1500
        assert max(len(idx) for _, _, idx in S.fit_cases(kind)) == S.N_SUPER
    rows, cols = S.spoiled_rows("F")
    assert len(rows) == 60 and np.isnan(S.changed_sets("F")["nan_rows"][rows, cols]).all()
    assert np.isposinf(S.changed_sets("F")["inf_rows"]).sum() == 60


def test_assert_same_floats_is_exact():
    a = np.array([0.0, 1.0, np.nan, np.inf], np.float32)
    S.assert_same_floats(a, a.copy())
    S.assert_same_floats(np.array([-np.nan], np.float32), np.array([np.nan], np.float32))  # payload and sign free
    for bad in (np.array([-0.0, 1.0, np.nan, np.inf], np.float32),                     # -0 is not +0
                np.array([0.0, np.nextafter(np.float32(1), np.float32(2)), np.nan, np.inf], np.float32),
                np.array([0.0, 1.0, 0.0, np.inf], np.float32),                         # a number where a NaN belongs
                np.array([0.0, np.nan, np.nan, np.inf], np.float32),                   # a NaN where a number belongs
                np.array([0.0, 1.0, np.nan, -np.inf], np.float32)):
        with pytest.raises(AssertionError):
            S.assert_same_floats(bad, a)


# ------------------------------------------------------------------ the GPU file's comparisons can fail
def test_comparisons_reject_wrong_expectations(oracle):
    """Each comparison of tests/test_gpu_solver_cases.py, fed the oracle's own output as the result and a
    deliberately wrong expectation, fails (and passes on the right one)."""
    from tests.helpers import multi_polish_ref as ref
    # 1. minimal solvers: the fall-back samples' models swapped with their neighbours'
    for kind, name in (("F", "rep_one"), ("E", "all_equal"), ("H", "nan_rows")):
        pts, samples = S.sample_table(oracle, kind, name)
        models, nm = oracle.Estimator(_okind(oracle, kind), pts).estimate_batch(samples)
        S.assert_same_models(kind, models.copy(), nm.copy(), models, nm)
        traces, _ = _per_sample(oracle, kind, name)
        rows = [i for i, t in enumerate(traces) if (t["f7_fallback"] or t["e5_fallback"]) and nm[i]] if kind != "H" \
            else [i for i in range(S.NS) if not np.isfinite(models[i]).all()]
        assert rows
        wrong = models.copy()
        for i in rows:
            wrong[i] = models[(i + 1) % S.NS]
        with pytest.raises(AssertionError):
            S.assert_same_models(kind, models, nm, wrong, nm)
        wrong_nm = nm.copy()
        wrong_nm[rows[0]] += 1
        with pytest.raises(AssertionError):
            S.assert_same_models(kind, models, nm, models, wrong_nm)
    # 2. a round: a count off by one, a sum one ulp off, an empty slot filled, another best
    pts, samples = S.sample_table(oracle, "F", "rep_one")
    w = S.round_expectation(oracle, "F", pts, samples, S.THR["F"])
    b = int(w["best"])
    best = {"valid": True, "hyp_index": b // 3, "inliers": int(w["counts"][b]), "score": float(w["sums"][b]),
            "model": w["models"][b].copy()}
    S.assert_same_round(w["counts"].copy(), w["sums"].copy(), best, w)
    live, empty = np.flatnonzero(w["occupied"]), np.flatnonzero(~w["occupied"])
    assert len(live) and len(empty) and w["counts"][b] > 0
    for field, slot, value in (("counts", live[0], w["counts"][live[0]] + 1), ("counts", empty[0], 0),
                               ("sums", b, np.nextafter(w["sums"][b], np.float32(np.inf)))):
        wrong = dict(w, **{field: w[field].copy()})
        wrong[field][slot] = value
        with pytest.raises(AssertionError):
            S.assert_same_round(w["counts"], w["sums"], best, wrong)
    other = int(live[live != b][0])
    with pytest.raises(AssertionError):
        S.assert_same_round(w["counts"], w["sums"], best, dict(w, best=other))
    with pytest.raises(AssertionError):
        S.assert_same_round(w["counts"], w["sums"], best, dict(w, best=None))
    # 3. fits: another list's model, a model where none is expected and the reverse
    cases = {name: (pts, idx) for name, pts, idx in S.fit_cases("H")}
    a = S.fit_expectation(oracle, "H", *cases["inliers_100"])
    c = S.fit_expectation(oracle, "H", *cases["inliers_300"])
    S.assert_same_fit(a.copy(), a)
    S.assert_same_fit(-111, None)
    for got, want in ((a, c), (a, None), (-111, a), (-1, None)):
        with pytest.raises(AssertionError):
            S.assert_same_fit(got, want)
    nan_fit = S.fit_expectation(oracle, "H", *cases["zeros_100"])
    assert np.isnan(nan_fit).any()
    with pytest.raises(AssertionError):
        S.assert_same_fit(a, nan_fit)
    # 4. polish: one pass fewer, another model
    name, pts, start = S.polish_cases("F")[0]
    r = ref.polish_ref(ref.estimator(oracle, "F", pts), start, ref.THR)
    ref.assert_same_polish(dict(r), r)
    with pytest.raises(AssertionError):
        ref.assert_same_polish(dict(r), dict(r, passes=r["passes"] - 1))
    with pytest.raises(AssertionError):
        ref.assert_same_polish(dict(r), dict(r, model=np.asarray(start, np.float32)))


@pytest.mark.parametrize("kind", ["H", "F"])
def test_polish_cases_run_a_degenerate_fit(oracle, kind):
    from tests.helpers import multi_polish_ref as ref
    for name, pts, start in S.polish_cases(kind):
        oracle.trace_reset()
        r = ref.polish_ref(ref.estimator(oracle, kind, pts), start, ref.THR)
        print(kind, name, "lists fitted", r["sizes"], "passes", r["passes"], "stop", r["stop"],
              "last eigen exit", oracle.EIG_EXITS[oracle.trace_get()["eig_exit"]])
        assert r["passes"] >= 1 and r["status"] == 0 and len(pts) <= 1500
