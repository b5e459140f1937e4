"""Multi contexts from padded device tensors in quality order (MultiContext.from_padded / from_matches with
scores, usac_multi_create_device_sorted; ABI 26).  The yardstick is numpy on the host: the written rule
(tests/helpers/multi_sorted_ref.py) gives per problem the kept columns in sorted order, sets[p] =
rows[p][cols[order]], fed to the constructors that take host arrays.  A context from device input with scores must
hold the bits of np.concatenate(sets), their offsets and cols[order] as its source columns, and every call on it
must return what the same call returns on the host-built context.  Every comparison is exact (floats by bit
pattern), so there is no tolerance to choose.

The shapes are the smallest at which the sort can go wrong.  `seven`: n_max = 300, kept counts m, 21, 64, 65, 256,
257, 300 -- below, at and above a wave and the 256 threads of the workgroup, the two smallest problems with every
kept row in the last block of 256 columns.  `one`: P = 1.  `pow2`: n_max = 512 with 127, 128 and 129 kept rows, one
below, at and one above the padded size of the sorting network.  With USAC_MULTI_SORT_LDS=64 the problems of more
than 64 rows leave the network in LDS for the sort by runs and ranks (65: a run of one row; 256: four full runs;
257 and 300: a short last run), and 64 stays; 100 makes the runs no power of two.  Which path a problem takes is
decided by its row count and the cap alone (kernels_multi_sort.hip), so what the tests see of it is that the
result does not change.  Without the override: 4 096 rows, the cap, and 4 097, which must take the second path, and
9 000 (three runs).

The layout tests move rows of arbitrary bit patterns.  The whole-context tests use synthetic pairs whose columns
were permuted, with a score that falls with the original rank: the sort restores the order PROSAC expects."""
import numpy as np
import pytest

from tests.helpers import multi_essential_lo_ref as eref
from tests.helpers import multi_lo_ref as lref
from tests.helpers import multi_pixels_ref as pref
from tests.helpers import multi_sorted_ref as sref
from tests.helpers.same_bits import same as _same

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

R, MAX_IT, PROB = 64, 256, 0.95
KINDS = ("H", "F", "E")
M = {"H": 4, "F": 7, "E": 5}
THR = {"H": 2.0, "F": 2.0, "E": eref.THR}
N1 = 200
PATTERNS = ("distinct", "equal", "sorted", "reversed", "four", "zeros", "infs", "nans", "all_nan", "garbage")
BIG = (21, 64, 65, 256, 257, 300)  # the problems PROSAC accepts (more than 20 rows)


def _est(usac, kind):
    return {"H": usac.ESTIMATOR.Homography, "F": usac.ESTIMATOR.Fundamental, "E": usac.ESTIMATOR.Essential}[kind]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _valid(shape, rng):
    """the (P, n_max) keep mask of the named fixture"""
    if shape == "seven":
        valid = np.zeros((7, 300), dtype=bool)
        for p, k in enumerate((4,) + BIG):
            lo = 256 if p < 2 else 0  # the two smallest: every kept row in the last block of 256 columns
            valid[p, lo + rng.permutation(300 - lo)[:k]] = True
        return valid
    if shape == "one":
        return rng.random((1, 300)) < 0.5
    assert shape == "pow2"
    valid = np.zeros((3, 512), dtype=bool)
    for p, k in enumerate((127, 128, 129)):
        valid[p, rng.permutation(512)[:k]] = True
    return valid


def _scores(pattern, valid, rng):
    """(P, n_max) float32 scores of the named pattern; `garbage` differs from `four` in the columns not kept alone"""
    P, n = valid.shape
    if pattern == "distinct":
        return np.stack([rng.permutation(n) for _ in range(P)]).astype(np.float32) - np.float32(n // 2)
    if pattern == "equal":
        return np.full((P, n), 0.75, dtype=np.float32)
    if pattern in ("sorted", "reversed"):
        s = np.tile(np.arange(n, dtype=np.float32), (P, 1))
        return s if pattern == "sorted" else -s
    if pattern in ("four", "garbage"):
        s = np.random.default_rng(4).choice(np.array([0.25, 0.5, -1.0, 7.0], np.float32), size=(P, n))
        if pattern == "garbage":
            junk = rng.integers(0, 1 << 32, size=(P, n), dtype=np.uint64).astype(np.uint32)
            junk[:, ::3] = rng.choice(sref.NAN_BITS, size=junk[:, ::3].shape)
            s = np.where(valid, s, junk.view(np.float32))
        return np.ascontiguousarray(s, dtype=np.float32)
    if pattern == "zeros":
        return rng.choice(np.array([0x00000000, 0x80000000], np.uint32), size=(P, n)).view(np.float32)
    if pattern == "infs":
        s = rng.normal(0, 2, size=(P, n)).astype(np.float32)
        s[rng.random((P, n)) < 0.2] = np.inf
        s[rng.random((P, n)) < 0.2] = -np.inf
        return s
    if pattern == "nans":
        s = rng.choice(np.array([-3.0, -0.0, 0.0, 1.5, 2.0, np.inf], np.float32), size=(P, n)).view(np.uint32).copy()
        at = rng.random((P, n)) < 0.4
        s[at] = rng.choice(sref.NAN_BITS, size=int(at.sum()))
        return s.view(np.float32)
    assert pattern == "all_nan"
    return rng.choice(sref.NAN_BITS, size=(P, n)).view(np.float32)


def _form_a(how, valid, rng):
    """rows of arbitrary bits, and valid as form a with `how` keeps it (counts: the same sizes as prefixes)"""
    P, n = valid.shape
    rows = rng.integers(-2**31, 2**31, size=(P, n, 4), dtype=np.int64).astype(np.int32).view(np.float32)
    if how == "counts":
        valid = np.arange(n)[None, :] < valid.sum(1)[:, None]
    elif how == "all":
        valid = np.ones_like(valid)
    return rows, valid


def _create(usac, est, how, rows, valid, **kw):
    MC = usac.MultiContext
    if how == "counts":
        return MC.from_padded(est, _dev(rows), counts=_dev(valid.sum(1).astype(np.int32)), **kw)
    if how == "all":
        return MC.from_padded(est, _dev(rows), **kw)
    return MC.from_padded(est, _dev(rows), valid=_dev(valid), **kw)


def _check_layout(mc, sets, cols, what):
    """offsets, source columns and the rows' bits of a context against the yardstick's"""
    sizes = np.array([len(c) for c in cols], dtype=np.int64)
    off = np.zeros(len(cols) + 1, dtype=np.uint32)
    off[1:] = np.cumsum(sizes)
    assert mc.sorted_by_score is True and mc.inlier_lists is False and mc.points is None
    _same(mc.offsets, off, (what, "offsets"))
    src = mc.source_index
    assert src.dtype == np.uint32
    for p, c in enumerate(cols):
        _same(src[off[p]:off[p + 1]], c, (what, "source", p))
    _same(mc.resident_points().view(np.int32), np.concatenate(sets, axis=0).view(np.int32), (what, "rows"))


def _all_patterns(usac, how, rows, valid, seed, patterns=PATTERNS):
    """every score pattern in both directions on one input: layout, determinism, and what `equal` and `garbage` promise"""
    est = usac.ESTIMATOR.Homography
    rng = np.random.default_rng(seed)
    with _create(usac, est, how, rows, valid) as plain:
        assert plain.sorted_by_score is False
        plain_src, plain_rows = plain.source_index.copy(), plain.resident_points()
    four = {}
    for pattern in patterns:
        scores = _scores(pattern, valid, rng)
        d_scores = _dev(scores)
        for descending in (True, False):
            what = (how, pattern, descending)
            cols = sref.sorted_columns(scores, valid, descending)
            sets = [r[c] for r, c in zip(rows, cols)]
            with _create(usac, est, how, rows, valid, scores=d_scores, descending=descending) as mc, \
                    _create(usac, est, how, rows, valid, scores=d_scores, descending=descending) as again:
                _check_layout(mc, sets, cols, what)
                _same(again.source_index, mc.source_index, (what, "two creations"))
                if pattern in ("equal", "all_nan"):  # nothing to order by: the plain creation's result
                    _same(mc.source_index, plain_src, (what, "column order"))
                    _same(mc.resident_points().view(np.int32), plain_rows.view(np.int32), (what, "plain rows"))
                if pattern == "four":
                    four[descending] = mc.source_index.copy()
                if pattern == "garbage" and descending in four:
                    _same(mc.source_index, four[descending], (what, "columns not kept were looked at"))


@pytest.mark.parametrize("how", ["valid", "counts", "all"])
@pytest.mark.parametrize("shape", ["seven", "one", "pow2"])
def test_layout_form_a(usac, shape, how):
    rng = np.random.default_rng(31)
    rows, valid = _form_a(how, _valid(shape, rng), rng)
    _all_patterns(usac, how, rows, valid, 32)


def _matches(rng, n0=300, sizes=(7, 21, 150, 257)):
    """form b over keypoints of arbitrary bits: negatives, columns that share a target, and the index n1 - 1"""
    P = len(sizes)
    kpts0 = rng.integers(-2**31, 2**31, size=(P, n0, 2), dtype=np.int64).astype(np.int32).view(np.float32)
    kpts1 = rng.integers(-2**31, 2**31, size=(P, N1, 2), dtype=np.int64).astype(np.int32).view(np.float32)
    match = np.full((P, n0), -1, dtype=np.int32)
    for p, k in enumerate(sizes):
        cols = np.sort(rng.permutation(n0)[:k])
        match[p, cols] = rng.integers(0, N1 - 1, size=k)  # with replacement: shared targets
    kept = np.flatnonzero(match[2] >= 0)
    match[2, kept[0]] = N1 - 1
    match[2, kept[5]] = match[2, kept[9]] = match[2, kept[4]]
    match[3, match[3] == -1] = -7  # any negative means no match
    return kpts0, kpts1, match


def test_layout_form_b(usac):
    rng = np.random.default_rng(33)
    kpts0, kpts1, match = _matches(rng)
    valid = match >= 0
    assert (match[2] == N1 - 1).sum() == 1 and (np.bincount(match[2][valid[2]]) >= 3).any()
    est = usac.ESTIMATOR.Fundamental
    args = (_dev(kpts0), _dev(kpts1), _dev(match))
    for pattern in PATTERNS:
        scores = _scores(pattern, valid, rng)
        for descending in (True, False):
            cols = sref.sorted_columns(scores, valid, descending)
            sets = [np.concatenate([a[c], b[m[c]]], axis=1) for a, b, m, c in zip(kpts0, kpts1, match, cols)]
            with usac.MultiContext.from_matches(est, *args, scores=_dev(scores), descending=descending) as mc, \
                    usac.MultiContext.from_matches(est, *args, scores=_dev(scores), descending=descending) as again:
                _check_layout(mc, sets, cols, ("matches", pattern, descending))
                _same(again.source_index, mc.source_index, "two creations")
    with usac.MultiContext.from_matches(est, args[0], args[1], _dev(match.astype(np.int64)), scores=_dev(scores)) as mc:
        _check_layout(mc, [np.concatenate([a[c], b[m[c]]], axis=1) for a, b, m, c in
                           zip(kpts0, kpts1, match, sref.sorted_columns(scores, valid, True))],
                      sref.sorted_columns(scores, valid, True), "int64 matches")


@pytest.mark.parametrize("cap", [64, 100])
def test_lowered_cap_changes_nothing(usac, monkeypatch, cap):
    """read at each creation: 65, 256, 257 and 300 rows are sorted by runs and ranks, 4, 21 and 64 in one network"""
    monkeypatch.setenv("USAC_MULTI_SORT_LDS", str(cap))
    rng = np.random.default_rng(35)
    rows, valid = _form_a("valid", _valid("seven", rng), rng)
    _all_patterns(usac, "valid", rows, valid, 36)
    rows, valid = _form_a("valid", _valid("pow2", rng), rng)
    _all_patterns(usac, "valid", rows, valid, 37, patterns=("distinct", "four", "nans"))


def test_an_override_may_only_lower_the_cap(usac, monkeypatch):
    rng = np.random.default_rng(38)
    rows, valid = _form_a("valid", _valid("seven", rng), rng)
    for value in ("0", "-5", "100000", "junk"):
        monkeypatch.setenv("USAC_MULTI_SORT_LDS", value)
        _all_patterns(usac, "valid", rows, valid, 39, patterns=("distinct", "four"))


@pytest.mark.parametrize("kept", [4096, 4097, 9000])
def test_at_and_above_the_real_cap(usac, kept):
    rng = np.random.default_rng(40)
    valid = np.zeros((1, 9100), dtype=bool)
    valid[0, rng.permutation(9100)[:kept]] = True
    rows, valid = _form_a("valid", valid, rng)
    _all_patterns(usac, "valid", rows, valid, 41, patterns=("distinct", "four", "nans", "reversed"))


# ---- whole-context equality with the host-built context over the sorted sets

def _scene(kind, n, ratio, seed):
    from tests import test_gpu_multi_device as dev
    return dev._scene(kind, n, ratio, seed)


class World:
    """quality-sorted pairs with their columns permuted and a score falling with the original rank; a context from
    the device tensors with scores, the yardstick's sorted sets and a context built from them on the host"""

    def __init__(self, usac, kind, descending):
        rng = np.random.default_rng(50)
        ratios = [0.9, 0.8, 0.7, 0.6, 0.5, 0.5]
        P, n = len(BIG), 300
        self.kind, self.P, self.n_max = kind, P, n
        self.rows = np.zeros((P, n, 4), dtype=np.float32)
        self.scores = np.zeros((P, n), dtype=np.float32)
        self.valid = np.zeros((P, n), dtype=bool)
        for p, k in enumerate(BIG):
            perm = rng.permutation(n)
            self.rows[p, perm] = _scene(kind, n, ratios[p], 300 + p)
            quality = (1.0 - np.arange(n) / n).astype(np.float32)
            quality[5:9] = quality[5]  # a tie run: column order decides
            self.scores[p, perm] = quality if descending else -quality
            self.valid[p, perm[np.sort(rng.permutation(n)[:k])]] = True
        self.cols = sref.sorted_columns(self.scores, self.valid, descending)
        self.sets = [np.ascontiguousarray(r[c]) for r, c in zip(self.rows, self.cols)]
        est = _est(usac, kind)
        self.mc = usac.MultiContext.from_padded(est, _dev(self.rows), valid=_dev(self.valid), scores=_dev(self.scores),
                                                descending=descending)
        self.plain = usac.MultiContext.essential(self.sets) if kind == "E" else usac.MultiContext(est, self.sets)
        self.seeds = [11 + p for p in range(P)]

    def close(self):
        self.mc.close()
        self.plain.close()

    def scatter(self, mask):
        """the numpy way back: out[p, src[i]] = mask[i]"""
        out = np.zeros((self.P, self.n_max), dtype=bool)
        o = self.plain.offsets.astype(np.int64)
        for p, c in enumerate(self.cols):
            out[p, c] = mask[o[p]:o[p + 1]] != 0
        return out


@pytest.fixture(scope="module", params=[(k, d) for k in KINDS for d in (True, False)], ids=lambda v: "%s-%s" % v)
def world(usac, request):
    w = World(usac, *request.param)
    yield w
    w.close()


def _model(usac, kind, sampler):
    m = usac.Model(THR[kind], M[kind], PROB, 5, _est(usac, kind), sampler)
    m.max_iterations, m.batch, m.seed = MAX_IT, R, 100
    return m


def _assert_run(w, call):
    want, got = call(w.plain), call(w.mc)
    _same(got, [{k: v for k, v in r.items() if k != "inliers"} for r in want], "run")
    _same(w.mc.last_mask, w.plain.last_mask, "the host mask")
    mask = w.mc.padded_mask()
    assert mask.dtype == torch.bool and tuple(mask.shape) == (w.P, w.n_max) and mask.is_cuda
    host = mask.cpu().numpy()
    assert not host[~w.valid].any(), "a column that was not kept is set"
    np.testing.assert_array_equal(host, w.scatter(w.plain.last_mask))
    by_lists = np.zeros_like(host)
    for p, r in enumerate(want):
        by_lists[p, w.cols[p][r["inliers"]]] = True
    np.testing.assert_array_equal(host, by_lists)
    return want


def test_context_equals_host_built_over_sorted_sets(usac, world):
    w = world
    _same(w.mc.resident_points(), np.concatenate(w.sets), "rows")
    _same(w.mc.offsets, w.plain.offsets, "offsets")
    _same(w.mc.source_index, np.concatenate(w.cols), "source")
    _same(w.mc.hypothesize_score(R, seeds=w.seeds, thr=THR[w.kind]),
          w.plain.hypothesize_score(R, seeds=w.seeds, thr=THR[w.kind]), "round")


def test_prosac_run_and_the_way_back(usac, world):
    w = world
    model = _model(usac, w.kind, usac.SAMPLER.Prosac)
    want = _assert_run(w, lambda mc: mc.run_prosac(model, polish=True))
    assert all("termination_length" in r and "polished" in r for r in want)
    assert max(r["polished"]["inliers"] for r in want) > 20


@pytest.mark.parametrize("descending", [True, False])
def test_lo_run_with_the_prosac_sampler(usac, descending):
    model = lref.make_model(usac, "H", sampler=usac.SAMPLER.Prosac, thr=THR["H"])
    model.max_iterations, model.batch = MAX_IT, R
    w = World(usac, "H", descending)
    try:
        _assert_run(w, lambda mc: mc.run_lo(model, polish=True))
    finally:
        w.close()


def test_prosac_still_refuses_small_problems(usac):
    rng = np.random.default_rng(52)
    rows, valid = _form_a("valid", _valid("seven", rng), rng)  # problems of 4 and 21 rows: the first is too small
    scores = _scores("distinct", valid, rng)
    model = _model(usac, "H", usac.SAMPLER.Prosac)
    with _create(usac, usac.ESTIMATOR.Homography, "valid", rows, valid, scores=_dev(scores)) as mc:
        with pytest.raises(usac.UsacError) as e:
            mc.run_prosac(model)
        assert e.value.code == -1


@pytest.mark.parametrize("descending", [True, False])
def test_pixels_are_calibrated_after_the_sort(usac, descending):
    K1, K2 = pref.intrinsics()
    px = np.stack(pref.pixel_sets([300] * 6, K1, K2))
    rng = np.random.default_rng(53)
    valid = np.zeros((6, 300), dtype=bool)
    scores = np.zeros((6, 300), dtype=np.float32)
    for p, k in enumerate(BIG):
        perm = rng.permutation(300)
        px[p] = px[p][np.argsort(perm)]  # row i of the quality-sorted pair goes to column perm[i]
        scores[p, perm] = (np.arange(300) if not descending else -np.arange(300)).astype(np.float32)
        valid[p, rng.permutation(300)[:k]] = True
    cols = sref.sorted_columns(scores, valid, descending)
    sets = [np.ascontiguousarray(r[c]) for r, c in zip(px, cols)]
    model = _model(usac, "E", usac.SAMPLER.Prosac)
    with usac.MultiContext.from_padded(usac.ESTIMATOR.Essential, _dev(px), valid=_dev(valid), K1=K1, K2=K2,
                                       scores=_dev(scores), descending=descending) as mc, \
            usac.MultiContext.essential_pixels(sets, K1, K2) as plain:
        _same(mc.resident_points(), plain.points, "calibrated rows")
        _same(mc.resident_points(), np.concatenate(pref.calibrated_sets(sets, K1, K2)), "the restatement's rows")
        _same(mc.source_index, np.concatenate(cols), "source")
        tols = [30.0, 35.0, 40.0, 45.0, 50.0, 55.0]
        mc.set_pixel_thresholds(tols)
        plain.set_pixel_thresholds(tols)
        got, want = mc.run_prosac(model, polish=True), plain.run_prosac(model, polish=True)
        _same(got, [{k: v for k, v in r.items() if k != "inliers"} for r in want], "polished PROSAC run")
        E = np.stack([r["polished"]["model"] for r in want])
        _same(mc.pixel_models(E), plain.pixel_models(E), "pixel models")


def test_the_producers_stream_orders_the_scores(usac):
    """the scores are written by a kernel on a side stream, behind work that keeps it busy, and the context is created
    with that stream without a synchronisation in between: the sort must see what that kernel wrote"""
    rng = np.random.default_rng(54)
    rows, valid = _form_a("valid", _valid("seven", rng), rng)
    want = _scores("distinct", valid, rng)
    cols = sref.sorted_columns(want, valid, True)
    d_rows, d_valid, src_scores = _dev(rows), _dev(valid), _dev(want)
    scores = torch.full_like(src_scores, float("nan"))
    busy = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = (busy @ busy).clamp_(0, 1)
        torch.mul(src_scores, 1.0, out=scores)  # finite scores: x * 1 has x's bits
    mc = usac.MultiContext.from_padded(usac.ESTIMATOR.Homography, d_rows, valid=d_valid, scores=scores,
                                       stream=s.cuda_stream)
    try:
        _check_layout(mc, [r[c] for r, c in zip(rows, cols)], cols, "stream")
    finally:
        mc.close()
        torch.cuda.synchronize()


def test_refusals_with_scores(usac):
    est = usac.ESTIMATOR.Fundamental
    rng = np.random.default_rng(55)
    rows, valid = _form_a("valid", _valid("seven", rng), rng)
    scores = _dev(_scores("distinct", valid, rng))
    with pytest.raises(usac.UsacError) as e:  # problem 0 keeps 4 rows, fewer than 7: the pack's refusal, as without scores
        _create(usac, est, "valid", rows, valid, scores=scores)
    assert e.value.code == -1 and "problem 0:" in str(e.value) and "usac_multi_create_device_sorted" in str(e.value)

    class Odd:  # device memory, but not aligned to a float: refused before any launch
        __cuda_array_interface__ = {"shape": valid.shape, "typestr": "<f4", "data": (scores.data_ptr() + 2, False),
                                    "version": 3, "strides": None}

    with pytest.raises(usac.UsacError) as e:
        _create(usac, usac.ESTIMATOR.Homography, "valid", rows, valid, scores=Odd())
    assert e.value.code == -1 and "scores" in str(e.value) and "aligned" in str(e.value)
    with _create(usac, usac.ESTIMATOR.Homography, "valid", rows, valid, scores=scores) as mc:  # and the next one succeeds
        assert mc.sorted_by_score
