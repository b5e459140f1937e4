"""Multi contexts from padded device tensors (MultiContext.from_padded / from_matches / padded_mask,
usac_multi_create_device; ABI 25).  The yardstick is numpy on the host: sets[p] = rows[p][valid[p]], fed to the
constructors that take host arrays.  A context from device input must hold the bits of np.concatenate(sets), the
offsets and the source columns of the kept rows, and every call on it must return what the same call returns on
the host-built context, problem by problem.  Every comparison is exact (floats by bit pattern).

The fixtures are the smallest at which the compaction can go wrong.  `six`: n_max = 300, a multiple of neither
the wave (64) nor the 256-column block, kept counts m, 64, 65, 256, 257, 300 -- the smallest legal problem first
with all its rows in the last block, a count that crosses a wave and one that crosses a block, one problem kept
whole, the kept columns drawn by a seeded generator.  `edges`: n_max = 512, one problem keeps the first block, one
the second, one every second column.  `one`: P = 1.  `counts`: six's sizes in the prefix form.  `all_valid`:
neither valid nor counts.  `matches`: form b with n0 = 300, n1 = 200, negatives, columns that share a target, and
the index n1 - 1.

PROSAC needs more than 20 points per problem: on a fixture with a smaller problem run_prosac is refused with -1
on both contexts alike (asserted), and its results are compared on the fixture without that problem."""
import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import multi_essential_lo_ref as eref
from tests.helpers import multi_lo_ref as lref
from tests.helpers import multi_pixels_ref as pref
from tests.helpers.same_bits import same as _same

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

R, MAX_IT, PROB = 64, 256, 0.95
KINDS = ("H", "F", "E")
M = {"H": 4, "F": 7, "E": 5}
THR = {"H": 2.0, "F": 2.0, "E": eref.THR}
RATIOS = [0.9, 0.8, 0.7, 0.6, 0.5, 0.5]
N0, N1 = 300, 200
NAMES = ("six", "edges", "one", "counts", "all_valid", "matches")


def _est(usac, kind):
    return {"H": usac.ESTIMATOR.Homography, "F": usac.ESTIMATOR.Fundamental, "E": usac.ESTIMATOR.Essential}[kind]


def _scene(kind, n, ratio, seed):
    """n correspondences of one synthetic pair, sorted by quality (PROSAC runs on them)"""
    if kind == "H":
        return synthetic.homography_points(n=n, inlier_ratio=ratio, seed=seed)[0].astype(np.float32)
    if kind == "F":
        return synthetic.fundamental_points(n=n, inlier_ratio=ratio, seed=seed, prosac_order=True)[0].astype(np.float32)
    return eref.make_set(n, ratio, seed, prosac_order=True).astype(np.float32)


def _padded(kind, P, n_max, seed0):
    return np.stack([_scene(kind, n_max, RATIOS[p % 6], seed0 + p) for p in range(P)])


def _six_sizes(kind):
    return [M[kind], 64, 65, 256, 257, 300]


def _case(name, kind):
    """name -> dict(rows | kpts0, kpts1, match; valid; how), numpy on the host; valid is the keep mask"""
    rng = np.random.default_rng(7)
    if name in ("six", "counts"):
        rows = _padded(kind, 6, 300, 200)
        valid = np.zeros((6, 300), dtype=bool)
        for p, k in enumerate(_six_sizes(kind)):
            if name == "counts":
                valid[p, :k] = True
            elif p == 0:  # the smallest problem: all its rows in the last block of 256 columns
                valid[p, 256 + rng.permutation(300 - 256)[:k]] = True
            else:
                valid[p, rng.permutation(300)[:k]] = True
        return dict(rows=rows, valid=valid, how="counts" if name == "counts" else "valid")
    if name == "edges":
        valid = np.zeros((3, 512), dtype=bool)
        valid[0, :256] = True
        valid[1, 256:] = True
        valid[2, ::2] = True
        return dict(rows=_padded(kind, 3, 512, 210), valid=valid, how="valid")
    if name == "one":
        return dict(rows=_padded(kind, 1, 300, 220), valid=rng.random((1, 300)) < 0.5, how="valid")
    if name == "all_valid":
        return dict(rows=_padded(kind, 3, 300, 230), valid=np.ones((3, 300), dtype=bool), how="all")
    assert name == "matches"
    scene = _padded(kind, 3, N0, 240)
    kpts0 = np.ascontiguousarray(scene[:, :, :2])
    kpts1 = rng.normal(500, 200, size=(3, N1, 2)).astype(np.float32)  # unmatched keypoints of view 2
    match = np.full((3, N0), -1, dtype=np.int32)
    for p, k in enumerate([M[kind], 150, 190]):
        cols = np.sort(rng.permutation(N0)[:k])
        tgt = rng.permutation(N1 - 1)[:k]
        if p == 1:
            tgt[0] = N1 - 1                    # the last keypoint of view 2
            tgt[5], tgt[9] = tgt[4], tgt[4]    # three columns on one target
        match[p, cols] = tgt
        kpts1[p, tgt] = scene[p, cols, 2:]     # a shared target keeps its last column's point
    match[2, match[2] == -1] = -7              # any negative means no match
    assert (match[1] == N1 - 1).sum() == 1 and (np.bincount(match[1][match[1] >= 0]) == 3).any()
    return dict(kpts0=kpts0, kpts1=kpts1, match=match, valid=match >= 0, how="matches")


def _sets(case):
    """the yardstick: per problem the kept rows, in column order"""
    if case["how"] == "matches":
        out = []
        for k0, k1, mt in zip(case["kpts0"], case["kpts1"], case["match"]):
            keep = mt >= 0
            out.append(np.ascontiguousarray(np.concatenate([k0[keep], k1[mt[keep]]], axis=1)))
        return out
    return [np.ascontiguousarray(r[v]) for r, v in zip(case["rows"], case["valid"])]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _from_device(usac, kind, case, **kw):
    est = _est(usac, kind)
    if case["how"] == "matches":
        return usac.MultiContext.from_matches(est, _dev(case["kpts0"]), _dev(case["kpts1"]), _dev(case["match"]), **kw)
    if case["how"] == "counts":
        return usac.MultiContext.from_padded(est, _dev(case["rows"]), counts=_dev(case["valid"].sum(1).astype(np.int32)), **kw)
    if case["how"] == "all":
        return usac.MultiContext.from_padded(est, _dev(case["rows"]), **kw)
    return usac.MultiContext.from_padded(est, _dev(case["rows"]), valid=_dev(case["valid"]), **kw)


def _from_host(usac, kind, sets):
    return usac.MultiContext.essential(sets) if kind == "E" else usac.MultiContext(_est(usac, kind), sets)


class World:
    """a context from device tensors, the yardstick's sets and a context built from them on the host"""

    def __init__(self, usac, kind, case):
        self.kind, self.case = kind, case
        self.valid = case["valid"]
        self.P, self.n_max = self.valid.shape
        self.sets = _sets(case)
        self.mc = _from_device(usac, kind, case)
        self.plain = _from_host(usac, kind, self.sets)
        self.seeds = [11 + p for p in range(self.P)]

    def close(self):
        self.mc.close()
        self.plain.close()

    def scatter(self, lists):
        """per-problem local index lists -> the (P, n_max) mask they mean"""
        out = np.zeros((self.P, self.n_max), dtype=bool)
        for p, idx in enumerate(lists):
            out[p, np.flatnonzero(self.valid[p])[idx]] = True
        return out


@pytest.fixture(scope="module", params=[(n, k) for n in NAMES for k in KINDS], ids=lambda v: "%s-%s" % v)
def world(usac, request):
    name, kind = request.param
    w = World(usac, kind, _case(name, kind))
    yield w
    w.close()


def _model(usac, kind, sampler=None):
    m = usac.Model(THR[kind], M[kind], PROB, 5, _est(usac, kind), sampler or usac.SAMPLER.Uniform)
    m.max_iterations, m.batch, m.seed = MAX_IT, R, 100
    return m


def _lo_model(usac, kind):
    m = eref.make_model(usac) if kind == "E" else lref.make_model(usac, kind, thr=THR[kind])
    m.max_iterations, m.batch = MAX_IT, R
    return m


def test_layout_rows_and_source(usac, world):
    w = world
    sizes = [len(s) for s in w.sets]
    assert w.mc.P == w.P and w.mc.n_max == w.n_max and w.mc.points is None and w.mc.inlier_lists is False
    assert w.mc.offsets.dtype == np.uint32
    _same(w.mc.offsets, w.plain.offsets, "offsets")
    assert (w.mc.sizes == sizes).all() and (w.plain.sizes == sizes).all()
    _same(w.mc.resident_points(), np.concatenate(w.sets, axis=0), "rows")
    src = w.mc.source_index
    assert src.dtype == np.uint32 and src is w.mc.source_index
    o = w.mc.offsets.astype(np.int64)
    for p in range(w.P):
        _same(src[o[p]:o[p + 1]], np.flatnonzero(w.valid[p]).astype(np.uint32), ("source", p))


def test_round_equals_host_built_context(usac, world):
    w = world
    got = w.mc.hypothesize_score(R, seeds=w.seeds, thr=THR[w.kind])
    want = w.plain.hypothesize_score(R, seeds=w.seeds, thr=THR[w.kind])
    _same(got, want, "round")


def _outcome(call):
    try:
        return ("ok", call())
    except Exception as e:  # a refusal counts as an outcome: both contexts must refuse alike
        return ("refused", type(e).__name__, getattr(e, "code", None))


def _assert_run(w, call):
    """call(context) -> run dicts: equal but for the index lists, and the padded mask is their scatter"""
    want = _outcome(lambda: call(w.plain))
    got = _outcome(lambda: call(w.mc))
    assert got[0] == want[0], (got, want)
    if want[0] == "refused":
        assert got == want
        return False
    lists = [r["inliers"] for r in want[1]]
    _same(got[1], [{k: v for k, v in r.items() if k != "inliers"} for r in want[1]], "run")
    mask = w.mc.padded_mask()
    assert mask.dtype == torch.bool and tuple(mask.shape) == (w.P, w.n_max) and mask.is_cuda
    host = mask.cpu().numpy()
    assert not host[~w.valid].any(), "a column that was not kept is set"
    np.testing.assert_array_equal(host, w.scatter(lists))
    _same(w.mc.last_mask, w.plain.last_mask, "the host mask")
    return True


def test_polished_run(usac, world):
    assert _assert_run(world, lambda mc: mc.run(_model(usac, world.kind), polish=True))
    plain = world.mc.run(_model(usac, world.kind))  # without the polish nothing changes
    _same(plain, world.plain.run(_model(usac, world.kind)), "run")


def test_prosac_run(usac, world):
    w = world
    model = _model(usac, w.kind, usac.SAMPLER.Prosac)
    ran = _assert_run(w, lambda mc: mc.run_prosac(model, polish=True))
    small = [len(s) <= 20 for s in w.sets]
    assert ran == (not any(small))
    if ran:
        return
    case = {k: (v[~np.array(small)] if isinstance(v, np.ndarray) else v) for k, v in w.case.items()}
    tail = World(usac, w.kind, case)
    try:
        assert _assert_run(tail, lambda mc: mc.run_prosac(model, polish=True))
    finally:
        tail.close()


def test_lo_run(usac, world):
    w = world
    model = _lo_model(usac, w.kind)
    _assert_run(w, lambda mc: (mc.run_lo_essential if w.kind == "E" else mc.run_lo)(model, polish=True))


def test_padded_mask_of_a_given_mask_into_a_given_tensor(usac, world):
    w = world
    models = np.stack([r["best"]["model"] for r in w.plain.run(_model(usac, w.kind))])
    lists = w.plain.inliers(models, THR[w.kind])
    _same(w.mc.inliers(models, THR[w.kind]), lists, "inliers() keeps returning lists")
    out = torch.full((w.P, w.n_max), 255, dtype=torch.uint8, device="cuda")
    back = w.mc.padded_mask(w.plain.last_mask, out=out)
    assert back is out
    np.testing.assert_array_equal(out.cpu().numpy(), w.scatter(lists).astype(np.uint8))
    res = w.mc.polish(models, THR[w.kind], with_inliers=True)
    want = w.plain.polish(models, THR[w.kind], with_inliers=True)
    _same(res, [{k: v for k, v in r.items() if k != "inlier_idx"} for r in want], "polish")
    np.testing.assert_array_equal(w.mc.padded_mask().cpu().numpy(), w.scatter([r["inlier_idx"] for r in want]))


def test_every_bit_arrives(usac):
    """rows of arbitrary bit patterns: NaNs with payloads, infinities, denormals and negative zeros are moved"""
    rng = np.random.default_rng(3)
    bits = rng.integers(-2**31, 2**31, size=(2, 300, 4), dtype=np.int64).astype(np.int32)
    bits[0, :4] = [[0x7fc00001, -0x7fffffff - 1, 0x7f800001, -1], [0x7f800000, 1, -0x00800000, 0]] * 2
    rows = bits.view(np.float32)
    valid = rng.random((2, 300)) < 0.6
    valid[0, :4] = True
    with usac.MultiContext.from_padded(usac.ESTIMATOR.Homography, _dev(rows), valid=_dev(valid.astype(np.uint8))) as mc:
        got = mc.resident_points()
    np.testing.assert_array_equal(got.view(np.int32), np.concatenate([b[v] for b, v in zip(bits, valid)]))
    kp0, kp1 = np.ascontiguousarray(rows[:, :, :2]), np.ascontiguousarray(rows[:, :200, 2:])
    match = np.where(valid, rng.integers(0, 200, size=(2, 300)), -1)  # int64: cast on the device
    with usac.MultiContext.from_matches(usac.ESTIMATOR.Fundamental, _dev(kp0), _dev(kp1), _dev(match)) as mc:
        got = mc.resident_points()
    want = np.concatenate([np.concatenate([a[v], b[m[v]]], axis=1) for a, b, m, v in zip(kp0, kp1, match, valid)])
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


def test_pixels_with_intrinsics_equal_essential_pixels(usac):
    K1, K2 = pref.intrinsics()
    px = np.stack(pref.pixel_sets([300] * 6, K1, K2))
    rng = np.random.default_rng(5)
    valid = np.zeros((6, 300), dtype=bool)
    for p, k in enumerate(_six_sizes("E")):
        valid[p, np.sort(rng.permutation(300)[:k])] = True
    sets = [np.ascontiguousarray(r[v]) for r, v in zip(px, valid)]
    tols = [30.0, 35.0, 40.0, 45.0, 50.0, 55.0]
    model = _model(usac, "E")
    with usac.MultiContext.from_padded(usac.ESTIMATOR.Essential, _dev(px), valid=_dev(valid), K1=K1, K2=K2) as mc, \
            usac.MultiContext.essential_pixels(sets, K1, K2) as plain:
        _same(mc.resident_points(), plain.points, "calibrated rows")
        _same(mc.resident_points(), np.concatenate(pref.calibrated_sets(sets, K1, K2)), "the restatement's rows")
        mc.set_pixel_thresholds(tols)
        plain.set_pixel_thresholds(tols)
        _same(mc.thresholds, plain.thresholds, "thresholds")
        got, want = mc.run(model, polish=True), plain.run(model, polish=True)
        _same(got, [{k: v for k, v in r.items() if k != "inliers"} for r in want], "polished run")
        E = np.stack([r["polished"]["model"] for r in want])
        _same(mc.pixel_models(E), plain.pixel_models(E), "pixel models")
        assert max(r["polished"]["inliers"] for r in got) > 20
    with usac.MultiContext.from_padded(usac.ESTIMATOR.Essential, _dev(px), valid=_dev(valid), K1=K1[1]) as mc, \
            usac.MultiContext.essential_pixels(sets, K1[1]) as plain:  # one matrix for all problems and both views
        _same(mc.resident_points(), plain.points, "calibrated rows, one K")
    with usac.MultiContext.from_padded(usac.ESTIMATOR.Essential, _dev(px), valid=_dev(valid)) as mc:
        with pytest.raises(usac.UsacError) as e:
            mc.set_pixel_thresholds(tols)
        assert e.value.code == -3


def test_the_producers_stream_orders_the_pack(usac):
    """the tensors are written by kernels on a side stream, behind work that keeps it busy, and the context is created
    under that stream without a synchronisation in between: the pack must see what those kernels wrote"""
    case = _case("six", "H")
    src_rows, src_valid = _dev(case["rows"]), _dev(case["valid"].astype(np.uint8))
    rows, valid = torch.zeros_like(src_rows), torch.zeros_like(src_valid)
    busy = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = (busy @ busy).clamp_(0, 1)
        torch.mul(src_rows, 1.0, out=rows)  # finite rows: x * 1 has x's bits
        torch.add(src_valid, 0, out=valid)
        mc = usac.MultiContext.from_padded(usac.ESTIMATOR.Homography, rows, valid=valid)
    try:
        _same(mc.resident_points(), np.concatenate(_sets(case)), "rows")
    finally:
        mc.close()
        torch.cuda.synchronize()


def test_refusals_after_the_counting_pass(usac):
    kind = "F"
    est = _est(usac, kind)
    case = _case("six", kind)
    rows, valid = _dev(case["rows"]), case["valid"].copy()
    short = valid.copy()
    short[2, np.flatnonzero(short[2])[M[kind] - 1:]] = False  # m - 1 rows left in problem 2
    with pytest.raises(usac.UsacError) as e:
        usac.MultiContext.from_padded(est, rows, valid=_dev(short))
    assert e.value.code == -1 and "problem 2:" in str(e.value) and "%d kept rows" % (M[kind] - 1) in str(e.value)
    counts = valid.sum(1).astype(np.int32)
    for bad, where in ((300 + 1, 1), (-1, 4)):
        c = counts.copy()
        c[where] = bad
        with pytest.raises(usac.UsacError) as e:
            usac.MultiContext.from_padded(est, rows, counts=_dev(c))
        assert e.value.code == -1 and "problem %d:" % where in str(e.value), str(e.value)
    mcase = _case("matches", kind)
    match = mcase["match"].copy()
    match[1, np.flatnonzero(match[1] >= 0)[3]] = N1  # one past the last keypoint of view 2: never dereferenced
    with pytest.raises(usac.UsacError) as e:
        usac.MultiContext.from_matches(est, _dev(mcase["kpts0"]), _dev(mcase["kpts1"]), _dev(match))
    assert e.value.code == -1 and "problem 1:" in str(e.value) and "n1" in str(e.value)
    with usac.MultiContext.from_padded(est, rows, valid=_dev(valid)) as mc:  # and the next creation succeeds
        _same(mc.resident_points(), np.concatenate(_sets(case)), "rows after the refusals")
    with usac.MultiContext(est, _sets(case)) as plain:  # a context from the host has no source columns
        with pytest.raises(usac.UsacError) as e:
            plain.padded_mask(np.zeros(int(plain.offsets[-1]), np.uint8))
        assert e.value.code == -3
        src = np.zeros(int(plain.offsets[-1]), dtype=np.uint32)
        import ctypes
        assert usac.lib().usac_multi_get_source(plain._h, src.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == -3
