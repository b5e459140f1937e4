"""Multi-problem PROSAC (usac_multi_run_prosac, ABI 17) on the device: the sampler against the single
context's PROSAC stream and a numpy restatement, the termination-scan kernel on crafted flag
patterns against the Python plain scan, the run against its loop restated over single contexts, and
the run's properties and argument errors."""
import ctypes

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import prosac_ref as ref

pytestmark = pytest.mark.gpu

THR = 2.0
SIZES = [21, 64, 65, 333, 1000]
RATIOS = [0.9, 0.3, 0.3, 0.0, 0.3]
DATA_SEEDS = {"H": [20, 21, 22, 23, 24], "F": [22, 31, 32, 33, 34]}
DUP = (5, 3)                       # problem 5 is a copy of problem 3 (the 333-point set)
SEEDS = [11, 12, 13, 14, 15, 14]   # sampler seeds: the copy shares its original's
M = {"H": 4, "F": 7}


def _sets(kind):
    """quality-sorted point sets (fundamental_points' recipe, applied to the homography sets as well)"""
    out = []
    for n, ratio, seed in zip(SIZES, RATIOS, DATA_SEEDS[kind]):
        if kind == "H":
            pts, _, inl = synthetic.homography_points(n=n, inlier_ratio=ratio, seed=seed)
            out.append(synthetic.quality_sort(pts, inl, seed + 1000)[0])
        else:
            out.append(synthetic.fundamental_points(n=n, inlier_ratio=ratio, seed=seed, prosac_order=True)[0])
    out.append(out[DUP[1]].copy())
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_record(a, b):
    assert a["hyp_index"] == b["hyp_index"] and a["inliers"] == b["inliers"] and a["valid"] == b["valid"]
    assert _bits(a["score"]) == _bits(b["score"])
    np.testing.assert_array_equal(_bits(a["model"]), _bits(b["model"]))


def _est(usac, kind):
    return usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental


@pytest.fixture(scope="module")
def problems(usac):
    """kind -> (point sets, MultiContext, the single contexts)"""
    made = {}
    for kind in ("H", "F"):
        sets = _sets(kind)
        made[kind] = (sets, usac.MultiContext(_est(usac, kind), sets), [usac.Context(_est(usac, kind), p) for p in sets])
    yield made
    for _, mc, singles in made.values():
        mc.close()
        for c in singles:
            c.close()


# ------------------------------------------------------------------ 1. samples, L = n
@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("kind", ["H", "F"])
def test_samples_equal_single_context_prosac_stream(usac, problems, kind, R):
    _, mc, singles = problems[kind]
    for f in (0, 3 * R):
        got = mc.draw_samples(R, SEEDS, first_hyp=f, clock=[1 + f] * mc.P)
        uni = mc.draw_samples(R, SEEDS, first_hyp=f)
        assert got.shape == uni.shape == (mc.P, R, mc.m)
        for p, ctx in enumerate(singles):
            ctx.set_device_sampler(usac.SAMPLER.Prosac)
            want = ctx.draw_samples(R, SEEDS[p], first_hyp=f)
            ctx.set_device_sampler(usac.SAMPLER.Uniform)
            np.testing.assert_array_equal(got[p], want)
            np.testing.assert_array_equal(uni[p], ctx.draw_samples(R, SEEDS[p], first_hyp=f))
            if ctx.n > 64:
                assert (got[p] != uni[p]).any()


# ------------------------------------------------------------------ 2. samples, L < n
@pytest.mark.parametrize("kind", ["H", "F"])
def test_samples_with_a_termination_length(usac, problems, kind):
    _, mc, _ = problems[kind]
    R, m = 64, mc.m
    cases = []  # (problem, clock, term_len, first_hyp)
    for p, L in ((3, 100), (4, 400), (2, 30)):
        n = int(mc.sizes[p])
        g = ref.growth_table(n, m)
        t_max = g[L - 1] + 1  # the last clock value whose lane is a PROSAC lane
        assert t_max > 20
        cases.append((p, t_max - 20, L, 128))    # 21 PROSAC lanes, then frozen over [0, L]
        cases.append((p, t_max + 1, L, 64))      # frozen throughout
        cases.append((p, ref.T_N - 5, n, 0))     # 6 PROSAC lanes, then uniform over n
        cases.append((p, ref.T_N + 1, L, 192))   # past the growth table: uniform over n whatever L
    for p, clock, L, f in cases:
        n = int(mc.sizes[p])
        sub, _, _ = usac.prosac_schedule(n, m, clock, L, R)
        got = mc.draw_samples(R, [SEEDS[p]], first_hyp=f, problems=[p], clock=[clock], term_len=[L])[0]
        want = ref.multi_prosac_samples(SEEDS[p], f, R, n, m, clock, L)
        np.testing.assert_array_equal(got, want)
        assert (got >= 0).all() and (got < n).all()
        assert all(len(set(row)) == m for row in got.tolist())
        frozen = sub == 0
        assert (got[frozen] <= L).all()
        pro = (sub != 0) & (sub != usac.UNIFORM_OVER_N)
        np.testing.assert_array_equal(got[pro][:, m - 1], sub[pro].astype(np.int64) - 1)
    # the first case of every problem froze in the middle of the round
    sub = usac.prosac_schedule(333, m, ref.growth_table(333, m)[99] + 1 - 20, 100, R)[0]
    assert (sub[:21] != 0).all() and (sub[21:] == 0).all()
    # several problems with their own clocks in one launch
    act, clocks, lens = [4, 2, 3], [500, 7, 90], [400, 65, 333]
    got = mc.draw_samples(R, [SEEDS[p] for p in act], first_hyp=64, problems=act, clock=clocks, term_len=lens)
    for i, p in enumerate(act):
        want = ref.multi_prosac_samples(SEEDS[p], 64, R, int(mc.sizes[p]), m, clocks[i], lens[i])
        np.testing.assert_array_equal(got[i], want)
    for bad in ({"clock": [0]}, {"clock": [1], "term_len": [m - 1]}, {"clock": [1], "term_len": [334]}):
        with pytest.raises(usac.UsacError) as e:
            mc.draw_samples(R, [1], problems=[3], **bad)
        assert e.value.code == -1


# ------------------------------------------------------------------ 3. the scan kernel alone
TILE = 256
SCAN_SIZES = [21, 22, TILE, TILE + 1, 2 * TILE + 3, 100]
PATTERNS = ["none", "all", "below20", "only20", "alternating", "alternating1", "last_in", "last_out"]
STRONG, WEAK, OUT = 0.0, 1.5, 100.0   # x2 - x1: an inlier of both calls, of the first call only, of neither
SCAN_MAX = 5000


def _pattern(name, n):
    """x offsets of n points: the inliers of the identity at THR are the points with |offset| < THR"""
    off = np.full(n, OUT)
    i = np.arange(n)
    if name == "all":
        off[:] = STRONG
    elif name == "below20":
        off[:20] = STRONG
    elif name == "only20":
        off[20] = STRONG
    elif name == "alternating":
        off[i % 2 == 0] = STRONG
    elif name == "alternating1":
        off[i % 2 == 1] = STRONG
    elif name in ("last_in", "last_out"):
        off[: n // 2] = STRONG
        off[n - 1] = STRONG if name == "last_in" else OUT
    off[(off == STRONG) & (i % 3 == 1)] = WEAK  # the second call (shifted model) loses every third inlier
    return off


def _crafted():
    """(point sets, per problem and call the x shift of its model, the expected flags)"""
    rng = np.random.default_rng(5)
    sets, shifts, flags = [], [], []

    def add(off, call_shifts):
        n = len(off)
        x1 = rng.integers(0, 1000, size=(n, 2)).astype(np.float32)
        sets.append(np.concatenate([x1, x1 + np.stack([off, np.zeros(n)], 1).astype(np.float32)], 1))
        shifts.append(call_shifts)
        flags.append([np.abs(off - s) < THR for s in call_shifts])

    for n in SCAN_SIZES:
        for name in PATTERNS:
            add(_pattern(name, n), (0.0, -1.0))  # second call: the STRONG points alone, a subset
    # the tie rule (tests/helpers/prosac_ref.py PlainScan.ties): with max_iterations = 5000 the first
    # call's only candidate (79, 11) has the clamped value 5000 and sets the length 80; the second
    # call's candidates (76, 11), (95, 12), (99, 12) all have that same value -- the first lies below the
    # length and must not move it, the other two lie above and must
    off = np.full(100, OUT)
    off[:10] = 1.25
    off[79] = 0.0
    off[[76, 95]] = 2.5
    add(off, (0.0, 2.5))
    return sets, shifts, flags


def _shift_model(dx):
    return np.array([1, 0, dx, 0, 1, 0, 0, 0, 1], dtype=np.float32)


def test_scan_kernel_on_crafted_flags(usac):
    sets, shifts, flags = _crafted()
    H, m = usac.ESTIMATOR.Homography, 4
    model = usac.Model(THR, m, 0.95, 5, H, usac.SAMPLER.Prosac)
    model.max_iterations = SCAN_MAX
    P = len(sets)
    plain = [ref.PlainScan(len(s), m, lambda c, pts: usac.std_termination(c, pts, m, 0.95, SCAN_MAX)) for s in sets]
    with usac.MultiContext(H, sets) as mc:
        n_cands = []
        for call in range(2):
            models = np.stack([_shift_model(shifts[p][call]) for p in range(P)])
            # the growth term of a candidate (i + 1 < largest, with uint32 wrap-around below growth[i])
            # on every other problem
            hyp = np.array([5 + 40 * call + p for p in range(P)], dtype=np.uint32)
            largest = np.array([len(sets[p]) if p % 2 else m + 10 * call for p in range(P)], dtype=np.uint32)
            bound, tl, cands = mc.prosac_scan(model, models, hyp, largest, reset=call == 0)
            inl = mc.inliers(models, THR)
            for p in range(P):
                n = len(sets[p])
                f = np.zeros(n, dtype=bool)
                f[inl[p]] = True
                np.testing.assert_array_equal(f, flags[p][call], err_msg="problem %d call %d" % (p, call))
                want_bound, want_cands = plain[p].scan(int(hyp[p]), f, int(largest[p]))
                assert cands[p].tolist() == [list(c) for c in want_cands], (p, call)
                assert (int(bound[p]), int(tl[p])) == (want_bound, plain[p].term_len), (p, call)
            n_cands.append([len(c) for c in cands])
        # the alternating pattern fills its segment: one candidate per raised inlier from point 20 on
        k = SCAN_SIZES.index(2 * TILE + 3) * len(PATTERNS) + PATTERNS.index("alternating")
        assert n_cands[0][k] == len(range(20, 2 * TILE + 3, 2))
        # a subset of the first call's inliers raises nothing
        assert sum(n_cands[1][:-1]) == 0 and sum(n_cands[0][:-1]) > 0
        assert n_cands[0][-1] == 1 and n_cands[1][-1] == 3 and plain[-1].ties == 3
        assert plain[-1].term_len == 100
        # reset: the first call again gives the first call's answer
        models = np.stack([_shift_model(shifts[p][0]) for p in range(P)])
        hyp = np.array([5 + p for p in range(P)], dtype=np.uint32)
        largest = np.array([len(sets[p]) if p % 2 else m for p in range(P)], dtype=np.uint32)
        _, _, again = mc.prosac_scan(model, models, hyp, largest, reset=True)
        assert [len(c) for c in again] == n_cands[0]


# ------------------------------------------------------------------ 4. run == its restated loop
RUN_MAX, RUN_PROB = 512, 0.95


def _run_model(usac, kind, dlt, R):
    model = usac.Model(THR, M[kind], RUN_PROB, 5, _est(usac, kind), usac.SAMPLER.Prosac)
    model.max_iterations = RUN_MAX
    model.batch = R
    model.seed = 100
    model.setDLTMode(dlt)
    return model


def _record(usac, d):
    return usac.Record(d["hyp_index"], d["inliers"], d["score"], (ctypes.c_float * 9)(*d["model"].tolist()), int(d["valid"]))


def _restated_run(usac, mc, ctx, p, seed, R, dlt):
    """usac_multi_run_prosac's loop for problem p: the multi context only draws the samples"""
    n, m = ctx.n, mc.m
    ctx.set_dlt_mode(dlt)
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
    ctx.set_dlt_mode(0)
    return {"best": best.as_dict(), "rounds": r, "hypotheses": r * R, "bound": bound,
            "status": 0 if best.inliers > 0 else -111, "termination_length": L, "largest_sample_size": largest,
            "clock": T, "scans": scans}


@pytest.fixture(scope="module")
def runs(usac, problems):
    return {}


def _run(usac, problems, runs, kind, dlt, R):
    if (kind, dlt, R) not in runs:
        _, mc, _ = problems[kind]
        runs[kind, dlt, R] = mc.run_prosac(_run_model(usac, kind, dlt, R))
    return runs[kind, dlt, R]


@pytest.mark.parametrize("R", [64, 256])
@pytest.mark.parametrize("kind,dlt", [("H", 0), ("H", 1), ("F", 0)])
def test_run_equals_restated_loop(usac, problems, runs, kind, dlt, R):
    _, mc, singles = problems[kind]
    got = _run(usac, problems, runs, kind, dlt, R)
    model = _run_model(usac, kind, dlt, R)
    for p, ctx in enumerate(singles):
        want = _restated_run(usac, mc, ctx, p, model.seed + p, R, dlt)
        for key in ("rounds", "hypotheses", "bound", "status", "termination_length", "largest_sample_size", "clock",
                    "scans"):
            assert got[p][key] == want[key], (p, key, got[p], want)
        _same_record(got[p]["best"], want["best"])
    # the inputs exercise the loop: a scan moved some termination length, and some problem ran on after
    # its first round
    assert any(g["termination_length"] < n for g, n in zip(got, mc.sizes))
    assert any(g["scans"] > 0 for g in got) and (R > 64 or any(g["rounds"] > 1 for g in got))


# ------------------------------------------------------------------ 5. run properties
@pytest.mark.parametrize("kind", ["H", "F"])
def test_run_properties(usac, problems, runs, kind):
    _, mc, _ = problems[kind]
    R = 64
    got = _run(usac, problems, runs, kind, 0, R)
    d, o = DUP
    model = _run_model(usac, kind, 0, R)
    seeds = [model.seed + p for p in range(mc.P)]
    again = mc.run_prosac(model, seeds=seeds)           # explicit seeds equal to seed + p: the default run
    seeds[d] = seeds[o]
    twin = mc.run_prosac(model, seeds=seeds)            # the copy with its original's seed: the same output
    keys = [k for k in got[0] if k != "best"]
    for p in range(mc.P):
        assert [again[p][k] for k in keys] == [got[p][k] for k in keys]
        _same_record(again[p]["best"], got[p]["best"])
    assert [twin[d][k] for k in keys] == [twin[o][k] for k in keys]
    _same_record(twin[d]["best"], twin[o]["best"])
    # polish=True: the same run, then mc.polish of its best models
    pol = mc.run_prosac(model, polish=True)
    want = mc.polish(np.stack([r["best"]["model"] for r in got]), THR, with_inliers=True)
    for p in range(mc.P):
        _same_record(pol[p]["best"], got[p]["best"])
        for key in ("inliers", "minimal_inliers", "passes", "status"):
            assert pol[p]["polished"][key] == want[p][key], (p, key)
        np.testing.assert_array_equal(_bits(pol[p]["polished"]["model"]), _bits(want[p]["model"]))
        assert _bits(pol[p]["polished"]["score"]) == _bits(want[p]["score"])
        np.testing.assert_array_equal(pol[p]["inliers"], want[p]["inlier_idx"])


def test_run_argument_errors(usac, problems):
    sets, mc, _ = problems["H"]
    model = _run_model(usac, "H", 0, 64)
    with pytest.raises(usac.UsacError) as e:
        mc.run(model)                      # usac_multi_run still refuses a PROSAC model
    assert e.value.code == -3
    for change, code in (("sprt", -3), ("lo", -3), ("sampler", -1), ("batch", -1)):
        model = _run_model(usac, "H", 0, 64)
        if change == "sprt":
            model.setSprt(True)
        elif change == "lo":
            model.lo = usac.LocOpt.InItLORsc
        elif change == "sampler":
            model.sampler = usac.SAMPLER.Uniform
        else:
            model.batch = 100
        with pytest.raises(usac.UsacError) as e:
            mc.run_prosac(model)
        assert e.value.code == code, change
    with usac.MultiContext(usac.ESTIMATOR.Homography, [sets[4], sets[4][:20]]) as small:  # n_p = 20
        with pytest.raises(usac.UsacError) as e:
            small.run_prosac(_run_model(usac, "H", 0, 64))
        assert e.value.code == -1
