"""The multi-problem polish (MultiContext.polish / run(polish=True); usac_multi_polish,
usac_multi_run_polished): one workgroup per problem runs the non-minimal polish and the final
getInliers of ransac.cpp:157-214.  Every output is compared bit for bit with the reference's polish
restated over the CPU oracle (tests/helpers/multi_polish_ref.py, pinned against oracle.ransac_run by
tests/test_multi_polish_cpu.py) and with the same loop over a single Context's get_inliers /
nonminimal.  Start models are the oracle's, from host samples, so every expected value is computed
on the CPU.

The resume case of test_past_the_caps (a first list <= 4096, a later one above) comes from a seed
search with the oracle: one host sample with seed 4 (H, lists 1099, 2821, 4094, 4618) and seed 18
(F, lists 2150, 3710, 4837, 5356) on the 6000-point sets."""
import numpy as np
import pytest

from tests.helpers import multi_polish_ref as ref

pytestmark = pytest.mark.gpu

THR = ref.THR
KINDS = ["H", "F"]


def _est(usac, kind):
    return usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental


# ------------------------------------------------------------------ 1. every way the loop ends
@pytest.fixture(scope="module")
def branch(usac, oracle):
    """kind -> (sets, MultiContext, per start set: (start models, polish_ref's dicts))"""
    made = {}
    for kind in KINDS:
        sets = ref.branch_sets(kind)
        ests = [ref.estimator(oracle, kind, pts) for pts in sets]
        starts = []
        for count, base in ref.STARTS:
            models = np.stack([ref.start_model(oracle, kind, pts, base + p, count, ests[p])
                               for p, pts in enumerate(sets)])
            starts.append((models, [ref.polish_ref(ests[p], models[p], THR) for p in range(len(sets))]))
        made[kind] = (sets, usac.MultiContext(_est(usac, kind), sets), starts)
    yield made
    for _, mc, _ in made.values():
        mc.close()


def test_inputs_reach_every_stop_reason(branch):
    """from the oracle's values alone: the sets and start models below exercise every exit of the loop"""
    seen = {r["stop"] for kind in KINDS for _, refs in branch[kind][2] for r in refs}
    assert {("ratio", 0), ("no_gain", 1), ("no_gain", 2), ("no_gain", 3), ("four", 4), ("no_model", 0)} <= seen
    h, f = branch["H"][2], branch["F"][2]
    assert (h[0][1][4]["minimal_inliers"], h[0][1][4]["inliers"]) == (35, 230)
    assert (f[0][1][4]["minimal_inliers"], f[0][1][4]["inliers"]) == (47, 53)
    assert f[1][1][3]["status"] == -111
    # the under-determined lists (4 and 7 points) and the set without inliers stop at the ratio
    assert h[0][1][0]["stop"] == f[0][1][0]["stop"] == h[0][1][3]["stop"] == ("ratio", 0)


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_polish_equals_oracle(branch, kind, start):
    sets, mc, starts = branch[kind]
    models, refs = starts[start]
    got = mc.polish(models, THR, with_inliers=True)
    assert len(got) == len(sets)
    for p, (g, r) in enumerate(zip(got, refs)):
        ref.assert_same_polish(g, r, (kind, start, p))
    # without the mask: the same results
    for p, (g, r) in enumerate(zip(mc.polish(models, THR), refs)):
        assert "inlier_idx" not in g
        ref.assert_same_polish(g, r, (kind, start, p))


# ------------------------------------------------------------------ 2. degenerate fits, no model
@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_fit_and_zero_model(usac, oracle, kind):
    same = np.tile(np.array([10, 20, 10, 20], np.float32), (50, 1))
    other = ref.make_set(kind, 65, 0.3, 22 if kind == "H" else 32)
    start = np.eye(3, dtype=np.float32).reshape(-1) if kind == "H" else np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)
    zero = np.zeros(9, np.float32)
    with usac.MultiContext(_est(usac, kind), [same, other, same]) as mc:
        got = mc.polish(np.stack([start, zero, zero]), THR, with_inliers=True)
    g = got[0]
    assert g["passes"] == 0 and g["inliers"] == 50 and g["minimal_inliers"] == 50 and g["status"] == 0
    np.testing.assert_array_equal(ref.bits(g["model"]), ref.bits(start))
    np.testing.assert_array_equal(g["inlier_idx"], np.arange(50))
    ref.assert_same_polish(g, ref.polish_ref(ref.estimator(oracle, kind, same), start, THR), (kind, "same"))
    for p in (1, 2):
        g = got[p]
        assert g["status"] == -111 and g["inliers"] == 0 and g["minimal_inliers"] == 0 and g["passes"] == 0
        assert g["score"] == 0 and g["minimal_score"] == 0 and len(g["inlier_idx"]) == 0
        np.testing.assert_array_equal(ref.bits(g["model"]), ref.bits(zero))


# ------------------------------------------------------------------ 3. past the caps
CAPS = {"H": (27, 26, 4), "F": (37, 36, 18)}  # data seeds of the 6000 / 17000-point sets, the resume seed


@pytest.mark.parametrize("kind", KINDS)
def test_past_the_caps(usac, oracle, kind):
    """a list above 4096 from the start, one that grows past it mid-polish, and a set above 16384
    points, next to small problems in the same context"""
    s6, s17, resume_seed = CAPS[kind]
    big, huge = ref.make_set(kind, 6000, 0.9, s6), ref.make_set(kind, 17000, 0.5, s17)
    small = ref.make_set(kind, 333, 0.3, 23 if kind == "H" else 33)
    sets = [big, small, huge, big, small]
    ests = [ref.estimator(oracle, kind, pts) for pts in sets]
    models = np.stack([ref.start_model(oracle, kind, big, 47, 256, ests[0]),
                       ref.start_model(oracle, kind, small, 48, 256, ests[1]),
                       ref.start_model(oracle, kind, huge, 46, 256, ests[2]),
                       ref.start_model(oracle, kind, big, resume_seed, 1, ests[3]),
                       ref.start_model(oracle, kind, small, 49, 256, ests[4])])
    refs = [ref.polish_ref(ests[p], models[p], THR) for p in range(len(sets))]
    assert refs[0]["minimal_inliers"] == (4421 if kind == "H" else 5011)
    assert (refs[2]["minimal_inliers"], refs[2]["inliers"], refs[2]["passes"]) == \
        ((6158, 7506, 4) if kind == "H" else (5301, 7562, 4))
    assert refs[3]["sizes"][0] <= 4096 < max(refs[3]["sizes"])
    assert max(refs[1]["sizes"] + refs[4]["sizes"]) <= 4096
    with usac.MultiContext(_est(usac, kind), sets) as mc:
        got = mc.polish(models, THR, with_inliers=True)
    for p, (g, r) in enumerate(zip(got, refs)):
        ref.assert_same_polish(g, r, (kind, p))


# ------------------------------------------------------------------ 4. the single-context device path
def _polish_single(usac, ctx, model, thr):
    """polish_ref's loop over Context.get_inliers / Context.nonminimal"""
    c0, s0, idx = ctx.get_inliers(model, thr)
    best, bm, bs, prev, passes = c0, np.asarray(model, np.float32), s0, 0, 0
    for _ in range(4 if c0 else 0):
        try:
            nm = ctx.nonminimal(idx[:best])
        except usac.UsacError as e:
            assert e.code == -111
            break
        c, s, idx2 = ctx.get_inliers(nm, thr)
        if np.float32(c) / np.float32(best) < 0.8 or c <= prev:
            break
        prev = best = c
        bm, bs, idx = nm, s, idx2
        passes += 1
    return {"passes": passes, "model": bm, "inliers": best, "score": np.float32(bs), "minimal_inliers": c0,
            "minimal_score": np.float32(s0), "status": 0 if c0 else -111,
            "inlier_idx": ctx.get_inliers(bm, thr)[2]}


@pytest.mark.parametrize("kind", KINDS)
def test_polish_equals_single_context(usac, branch, kind):
    sets, mc, starts = branch[kind]
    got = [mc.polish(models, THR, with_inliers=True) for models, _ in starts]
    for p, pts in enumerate(sets):
        with usac.Context(_est(usac, kind), pts) as ctx:
            for start, (models, _) in enumerate(starts):
                ref.assert_same_polish(got[start][p], _polish_single(usac, ctx, models[p], THR), (kind, start, p))


# ------------------------------------------------------------------ 5. run(polish=True)
def _check_run_polished_past_the_caps(usac, kind, dlt):
    """a run whose polish fits a list above 4096 (an 8000-point set with 90 % inliers, second in the
    context): the polished result is the oracle's restated polish of the run's best model"""
    from oracle import oracle as O
    sets = [ref.make_set(kind, 333, 0.3, 23 if kind == "H" else 33), ref.make_set(kind, 8000, 0.9, CAPS[kind][0])]
    model = usac.Model(THR, 4 if kind == "H" else 7, 0.95, 5, _est(usac, kind), usac.SAMPLER.Uniform)
    model.max_iterations, model.batch, model.seed = 512, 256, 100  # 256 hypotheses, as CAPS' start models
    model.setDLTMode(dlt)
    with usac.MultiContext(_est(usac, kind), sets) as mc:
        got = mc.run(model, polish=True)
    for p, pts in enumerate(sets):
        r = ref.polish_ref(ref.estimator(O, kind, pts), got[p]["best"]["model"], THR)
        ref.assert_same_polish(got[p]["polished"], r, (kind, "run past the caps", p))
        np.testing.assert_array_equal(got[p]["inliers"], r["inlier_idx"])
        if p == 1:  # from the oracle's values: a list above the cap was fitted
            assert max(r["sizes"]) > 4096


@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_run_polished(usac, branch, kind, dlt):
    sets = branch[kind][0]
    sets = sets + [sets[3].copy()]               # problem 6 is a copy of problem 3 ...
    seeds = [100, 101, 102, 103, 104, 105, 103]  # ... with its sampler seed
    model = usac.Model(THR, 4 if kind == "H" else 7, 0.95, 5, _est(usac, kind), usac.SAMPLER.Uniform)
    model.max_iterations, model.batch, model.seed = 512, 64, 100
    model.setDLTMode(dlt)
    with usac.MultiContext(_est(usac, kind), sets) as mc:
        plain = mc.run(model, seeds=seeds)
        got = mc.run(model, seeds=seeds, polish=True)
        best = np.stack([r["best"]["model"] for r in plain])
        again = mc.polish(best, THR, with_inliers=True)
        inl = mc.inliers(np.stack([g["polished"]["model"] for g in got]), THR)
    assert all("polished" not in r and "inliers" not in r for r in plain)
    for p, (a, g) in enumerate(zip(plain, got)):
        for key in ("hypotheses", "rounds", "bound", "status"):
            assert a[key] == g[key], (p, key)
        for key in ("hyp_index", "inliers", "valid"):
            assert a["best"][key] == g["best"][key], (p, key)
        assert ref.bits(a["best"]["score"]) == ref.bits(g["best"]["score"])
        np.testing.assert_array_equal(ref.bits(a["best"]["model"]), ref.bits(g["best"]["model"]))
        ref.assert_same_polish(g["polished"], again[p], (kind, p))
        np.testing.assert_array_equal(g["inliers"], again[p]["inlier_idx"])
        np.testing.assert_array_equal(g["inliers"], inl[p])
        assert g["polished"]["minimal_inliers"] == a["best"]["inliers"]
        assert g["polished"]["status"] == a["status"]
    ref.assert_same_polish(got[6]["polished"], got[3]["polished"], (kind, "copy"))
    _check_run_polished_past_the_caps(usac, kind, dlt)
    np.testing.assert_array_equal(got[6]["inliers"], got[3]["inliers"])
    assert sum(g["polished"]["passes"] for g in got) > 0
    assert any(g["polished"]["inliers"] > g["best"]["inliers"] for g in got)
