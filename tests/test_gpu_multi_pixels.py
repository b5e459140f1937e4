"""Essential multi contexts from pixel coordinates (usac_multi_create_essential_pixels,
usac_multi_set_pixel_thresholds, usac_multi_pixel_models, usac_multi_get_points; ABI 24).  The yardstick is
the written spec restated in numpy (tests/helpers/multi_pixels_ref.py): the rows k_multi_calibrate leaves on
the device, the thresholds and the pixel-space models must have its bits, and every call on the context must
return what the same call returns on MultiContext.essential over the restatement's rows with set_thresholds
over the restatement's thresholds.  Every comparison is exact.

The fixture: n_p = 5, 64, 65, 256, 257, 300 (N_total = 947, no multiple of the workgroup; the smallest legal
problem first; every boundary inside a workgroup and inside a wave), K per problem, one with skew, one with
fx != fy, K2 != K1 on half of them; the same with K2 = None; a layout of the same N_total whose boundaries lie
exactly on workgroup edges (rows 256 and 512) under one K for all problems; and P = 1.  The pixel sets are
synthetic.fundamental_points(normalized=False) with its noise, seen through the problem's own cameras.

PROSAC needs more than 20 points per problem, so run_prosac on the fixture itself is refused with -1 on both
contexts alike (asserted); its results are compared on the fixture without the 5-point problem."""
import numpy as np
import pytest

from tests.helpers import multi_essential_lo_ref as eref
from tests.helpers import multi_pixels_ref as ref
from tests.helpers.same_bits import same as _same

pytestmark = pytest.mark.gpu

R, MAX_IT, PROB = 64, 256, 0.95
# pixel tolerances, pairwise distinct.  The spec's threshold (t / f)^2 is compared with the residual of
# EssentialEstimator::GetError, the mean of the two point-to-epipolar-line distances in calibrated units (not
# squared): at f = 1000, 45 px give 0.002, the threshold of the other essential tests (2 px of distance), and
# the six values give 0.9 .. 3 px, so the runs find the scene's inliers under its 0.5 px noise
TOLS = [30.0, 35.0, 40.0, 45.0, 50.0, 55.0]
SCALAR = 0.007                           # what the calls pass while thresholds are set: no problem's value
SEEDS = [11, 12, 13, 14, 15, 16]


def _case(name):
    """name -> (pixel sets, K1, K2) as essential_pixels takes them"""
    K1, K2 = ref.intrinsics()
    if name == "six":
        return ref.pixel_sets(ref.SIZES, K1, K2), K1, K2
    if name == "six_k2_none":
        return ref.pixel_sets(ref.SIZES, K1), K1, None
    if name == "edges_one_k":  # one 3 x 3 matrix (with skew) for all problems
        return ref.pixel_sets(ref.EDGE_SIZES, K1[1]), K1[1], None
    assert name == "one"       # P = 1, two 3 x 3 matrices
    return [ref.pixel_sets(ref.SIZES, K1[1], K2[1])[5]], K1[1], K2[1]


class World:
    """a context from pixels, the restatement's rows and a context over them"""

    def __init__(self, usac, sets, K1, K2):
        self.sets, self.K1, self.K2, self.P = sets, K1, K2, len(sets)
        self.rows = ref.calibrated_sets(sets, K1, K2)
        self.mc = usac.MultiContext.essential_pixels(sets, K1, K2)
        self.plain = usac.MultiContext.essential(self.rows)
        self.tols = TOLS[:self.P]
        self.thr = ref.thresholds(self.tols, K1, K2, P=self.P)

    def arm(self):
        self.mc.set_pixel_thresholds(self.tols)
        self.plain.set_thresholds(self.thr)

    def close(self):
        self.mc.close()
        self.plain.close()


@pytest.fixture(scope="module", params=["six", "six_k2_none", "edges_one_k", "one"])
def world(usac, request):
    w = World(usac, *_case(request.param))
    yield w
    w.close()


@pytest.fixture(scope="module")
def tail_world(usac):
    """the fixture without its 5-point problem: PROSAC runs on it"""
    sets, K1, K2 = _case("six")
    w = World(usac, sets[1:], K1[1:], K2[1:])
    yield w
    w.close()


def _model(usac, sampler=None):
    m = usac.Model(SCALAR, 5, PROB, 5, usac.ESTIMATOR.Essential, sampler or usac.SAMPLER.Uniform)
    m.max_iterations, m.batch, m.seed = MAX_IT, R, 100
    return m


def _lo_model(usac, sampler=None):
    m = eref.make_model(usac, sampler=sampler, thr=SCALAR)
    m.max_iterations, m.batch = MAX_IT, R
    return m


def test_points_are_the_restatement_rows(usac, world):
    w = world
    want = np.concatenate(w.rows, axis=0)
    assert w.mc.points.dtype == np.float32 and w.mc.points.shape == (int(w.mc.offsets[-1]), 4)
    o = w.mc.offsets.astype(np.int64)
    for p in range(w.P):  # the first and the last row of every problem, by name
        _same(w.mc.points[o[p]], want[o[p]], ("first row", p))
        _same(w.mc.points[o[p + 1] - 1], want[o[p + 1] - 1], ("last row", p))
    _same(w.mc.points, want, "points")
    _same(w.mc.resident_points(), want, "resident points, read again")
    # usac_multi_get_points on any multi context: the rows it was given
    _same(w.plain.resident_points(), want, "a context from calibrated rows")
    assert (w.mc.sizes == [len(s) for s in w.sets]).all()


def test_get_points_on_a_homography_context(usac):
    from ransac_amd import synthetic
    sets = [synthetic.homography_points(n=n, inlier_ratio=0.5, seed=60 + n)[0] for n in (4, 257)]
    with usac.MultiContext(usac.ESTIMATOR.Homography, sets) as mc:
        _same(mc.resident_points(), np.concatenate(sets, axis=0), "H rows")


def test_pixel_thresholds(usac, world):
    w = world
    w.mc.set_thresholds(None)
    assert w.mc.thresholds is None
    w.mc.set_pixel_thresholds(1.5)
    _same(w.mc.thresholds, ref.thresholds(1.5, w.K1, w.K2, P=w.P), "one tolerance")
    w.mc.set_pixel_thresholds(w.tols)
    _same(w.mc.thresholds, w.thr, "a tolerance per problem")
    if w.P > 1:
        assert len(set(w.thr.tolist())) == w.P
    # a bad tolerance: -1, and the thresholds stay; 1e-30 px gives (1e-33)^2 = 0 in fp32
    bad = [0.0, -1.5, float("nan"), float("inf"), 1e-30, [1.5] * (w.P + 1), []]
    if w.P > 1:
        bad += [w.tols[:-1] + [-1.0], w.tols[:-1] + [float("nan")]]
    if w.P > 2:
        bad.append([1.5, 1.5])
    for t in bad:
        with pytest.raises(usac.UsacError) as e:
            w.mc.set_pixel_thresholds(t)
        assert e.value.code == -1, t
        _same(w.mc.thresholds, w.thr, ("after the bad tolerance", t))
    # cleared, the calls' scalar counts again, as on the other context
    w.mc.set_thresholds(None)
    assert w.mc.thresholds is None
    w.plain.set_thresholds(None)
    seeds = SEEDS[:w.P]
    got = w.mc.hypothesize_score(R, seeds=seeds, thr=float(w.thr[0]))
    want = w.plain.hypothesize_score(R, seeds=seeds, thr=float(w.thr[0]))
    _same(got, want, "a round at a scalar threshold after the clear")
    # and a failure on a context without thresholds leaves it without them
    with pytest.raises(usac.UsacError) as e:
        w.mc.set_pixel_thresholds(-1.0)
    assert e.value.code == -1 and w.mc.thresholds is None


def test_round_equals_context_over_the_rows(usac, world):
    w = world
    w.arm()
    seeds = SEEDS[:w.P]
    got = w.mc.hypothesize_score(R, seeds=seeds, first_hyp=128, thr=SCALAR)
    want = w.plain.hypothesize_score(R, seeds=seeds, first_hyp=128, thr=SCALAR)
    _same(got, want, "hypothesize_score")
    assert (got[0] >= 0).any()
    if w.P > 2:  # a shuffled partial active list
        pr = [w.P - 1, 2, 0]
        _same(w.mc.hypothesize_score(R, seeds=seeds[:3], thr=SCALAR, problems=pr),
              w.plain.hypothesize_score(R, seeds=seeds[:3], thr=SCALAR, problems=pr), "partial active list")


def test_run_polished_equals_context_over_the_rows(usac, world):
    w = world
    w.arm()
    got = w.mc.run(_model(usac), polish=True)
    want = w.plain.run(_model(usac), polish=True)
    _same(got, want, "run(polish=True)")
    print("best inliers:", [r["best"]["inliers"] for r in got], "polished:", [r["polished"]["inliers"] for r in got],
          "rounds:", [r["rounds"] for r in got])
    assert max(r["best"]["inliers"] for r in got) > 20  # the runs found the scene, not empty records alike
    # the pixel-space models of the polished models, in both shapes, and of arbitrary matrices
    E = np.stack([r["polished"]["model"] for r in got])
    _same(w.mc.pixel_models(E), ref.pixel_models(E, w.K1, w.K2), "pixel_models P x 9")
    E3 = np.random.default_rng(3).normal(size=(w.P, 3, 3)).astype(np.float32)
    F3 = w.mc.pixel_models(E3)
    assert F3.shape == (w.P, 3, 3)
    _same(F3, ref.pixel_models(E3, w.K1, w.K2), "pixel_models P x 3 x 3")
    with pytest.raises(ValueError):
        w.mc.pixel_models(E3[:, :2])


def test_run_lo_essential_equals_context_over_the_rows(usac, world):
    w = world
    w.arm()
    got = w.mc.run_lo_essential(_lo_model(usac), polish=True)
    want = w.plain.run_lo_essential(_lo_model(usac), polish=True)
    _same(got, want, "run_lo_essential(polish=True)")
    assert all("lo" in r and "polished" in r for r in got)
    print("lo calls:", [r["lo"]["lo_calls"] for r in got], "improved:", [r["lo"]["improved"] for r in got])


def test_run_prosac_equals_context_over_the_rows(usac, world, tail_world):
    w = world
    w.arm()
    model = _model(usac, usac.SAMPLER.Prosac)
    if min(len(s) for s in w.sets) <= 20:  # refused alike: PROSAC needs more than 20 points per problem
        for mc in (w.mc, w.plain):
            with pytest.raises(usac.UsacError) as e:
                mc.run_prosac(model)
            assert e.value.code == -1
        if w.K2 is None:
            return  # the fixture without its 5-point problem is run once, under K2 != K1
        w = tail_world
        w.arm()
    got = w.mc.run_prosac(model, polish=True)
    want = w.plain.run_prosac(model, polish=True)
    _same(got, want, "run_prosac(polish=True)")
    assert all("termination_length" in r and "scans" in r for r in got)
    # with LO on top (ABI 23), the PROSAC branch of the same entry
    lo = _lo_model(usac, usac.SAMPLER.Prosac)
    _same(w.mc.run_lo_essential(lo), w.plain.run_lo_essential(lo), "run_lo_essential under PROSAC")


def test_contexts_not_from_pixels_refuse(usac, world):
    from ransac_amd import synthetic
    w = world
    E = np.zeros((w.P, 9), dtype=np.float32)
    w.plain.set_thresholds(w.thr)
    for call in (lambda: w.plain.set_pixel_thresholds(1.5), lambda: w.plain.pixel_models(E)):
        with pytest.raises(usac.UsacError) as e:
            call()
        assert e.value.code == -3
    _same(w.plain.thresholds, w.thr, "the refusal leaves the thresholds alone")
    with usac.MultiContext(usac.ESTIMATOR.Homography, [synthetic.homography_points(n=40, seed=5)[0]]) as h:
        for call in (lambda: h.set_pixel_thresholds(1.5), lambda: h.pixel_models(np.zeros(9, np.float32))):
            with pytest.raises(usac.UsacError) as e:
                call()
            assert e.value.code == -3
        assert h.thresholds is None


def test_a_bad_k_is_refused_on_the_device_machine_too(usac):
    sets, K1, _ = _case("six")
    bad = K1.copy()
    bad[4, 0, 0] = 0.0
    with pytest.raises(usac.UsacError) as e:
        usac.MultiContext.essential_pixels(sets, bad)
    assert e.value.code == -1
    with pytest.raises(usac.UsacError) as e:
        usac.MultiContext.essential_pixels(sets, K1, bad)
    assert e.value.code == -1
