"""The guard-band scorers against the CPU oracle across dataset geometries (tests/helpers/geometry.py).

k_score_hf (packed stage A + per-point band), k_score_h16 (fp16 MFMA prefilter: box centres,
power-of-two scales, feature maxima, slack F_m), k_score_e16 (hi + lo fp16 MFMA prefilter) and
k_score_f2 (division-free two-view stage A) prove their rejections from constants of the point set.
Each table row moves those constants -- centres far from zero, scales far from 2^10, features in the
fp16 subnormal range, a zero extent, an empty box, NaN or infinite rows beside a live prefilter,
coordinates whose squares leave the fp32 range -- and the counts must still be the oracle's on the
same fp32 inputs: for the adversarial model family around the row's ground truth at three
thresholds, and for the base model at thresholds placed exactly on pair errors and on the next
float.  tests/test_scorer_geometry_inputs.py checks that the oracle has something to count on
every row."""
import functools

import numpy as np
import pytest

from tests.helpers import geometry as G

pytestmark = pytest.mark.gpu

B_HYP, SEED = 2048, 17


@pytest.fixture(autouse=True)
def prefilters_on(monkeypatch):
    """both matrix-core scorers are the default (read at context creation); pinned on here"""
    monkeypatch.setenv("USAC_H16", "1")
    monkeypatch.setenv("USAC_E16", "1")


def _thresholds(thr):
    return (thr, 0.25 * thr, 3.5 * thr)


@functools.lru_cache(maxsize=None)
def _reference(kind, name, normalized=None):
    """The oracle's answers for one row, computed once and shared by the row's tests (read only):
    points, base model, thr, models, {thr: (counts, sums)}, [(thr on a pair error, count)]."""
    from oracle import oracle as O

    if kind == "H":
        pts, base, thr = G.h_row(name)
        models = G.h_models(base, np.random.default_rng(3))
        est = O.Estimator(O.HOMOGRAPHY, pts)
    else:
        pts, base, thr = G.tv_row(name, normalized)
        models = G.e_models(base, np.random.default_rng(3))
        est = O.Estimator(O.ESSENTIAL if kind == "E" else O.FUNDAMENTAL, pts)
    scored = {t: est.score_models(models, t) for t in _thresholds(thr)}
    on_errors = [(t, int(est.score_models(base[None], t)[0][0])) for t in G.thresholds_on_errors(est.errors(base))]
    for a in (pts, base, models):
        a.setflags(write=False)
    return pts, base, thr, models, scored, on_errors


def _check_on_errors(ctx, base, on_errors):
    for t, oc in on_errors:
        gc, _ = ctx.score_models(base[None], t)
        assert gc[0] == oc, t


def _same_bits(a, b):
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------ homography
@pytest.mark.parametrize("name", G.H_ROWS)
def test_h_score_hf(usac, name):
    """k_score_hf, one chunk: counts and the sequential Σ equal the oracle's
    (test_gpu_parity.py::test_score_gt_models_real_scenes' assertions, per model)."""
    pts, base, thr, models, scored, on_errors = _reference("H", name)
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        for t, (oc, os_) in scored.items():
            gc, gs = ctx.score_models(models, t)
            np.testing.assert_array_equal(gc, oc, err_msg=str(t))
            np.testing.assert_array_equal(gs, os_, err_msg=str(t))  # float equality (NaN = NaN)
        _check_on_errors(ctx, base, on_errors)


@pytest.mark.parametrize("name", G.H_ROWS)
def test_h_score_h16(usac, name):
    """k_h16_rows + k_score_h16 (variant 3, four chunks): counts equal, Σ within the throughput bound."""
    pts, base, thr, models, scored, on_errors = _reference("H", name)
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(4)
        for t, (oc, os_) in scored.items():
            gc, gs = ctx.score_models(models, t)
            np.testing.assert_array_equal(gc, oc, err_msg=str(t))
            fin = np.isfinite(os_)
            err = np.abs(gs[fin].astype(np.float64) - os_[fin])
            assert (err <= G.h16_sum_bound(os_[fin], oc[fin], pts, t)).all(), t
        _check_on_errors(ctx, base, on_errors)


@pytest.mark.parametrize("name", G.H_ROWS)
def test_h_score_hf_throughput(usac, monkeypatch, name):
    """k_score_hf in throughput mode (USAC_H16=0, variant 3, four chunks): stage B decides the inliers
    too (no exact re-evaluation of them), the path that shares stage B with the h16 drains: counts
    equal, Σ within the same throughput bound."""
    monkeypatch.setenv("USAC_H16", "0")
    pts, base, thr, models, scored, on_errors = _reference("H", name)
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(4)
        for t, (oc, os_) in scored.items():
            gc, gs = ctx.score_models(models, t)
            np.testing.assert_array_equal(gc, oc, err_msg=str(t))
            fin = np.isfinite(os_)
            err = np.abs(gs[fin].astype(np.float64) - os_[fin])
            assert (err <= G.h16_sum_bound(os_[fin], oc[fin], pts, t)).all(), t
        _check_on_errors(ctx, base, on_errors)


@pytest.mark.parametrize("name", G.H_ROWS)
def test_h_hypothesize_h16(usac, name):
    """A device batch at eight chunks -- the solver's epilogue writes the h16 rows, a second writer of the
    same bound -- against the exact-expression kernel (variant 1) on the same seed."""
    pts, _, thr, _, _, _ = _reference("H", name)
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(1)
        ce, se, be = ctx.hypothesize_score(B=B_HYP, seed=SEED, first_hyp=0, thr=thr)
        ctx.set_score_variant(0)
        ctx.set_score_chunks(8)
        ctx.hypothesize_async(B_HYP, SEED, 0, thr)
        rec = ctx.fetch_best()
        cf, sf = ctx.last_counts(B_HYP)
    np.testing.assert_array_equal(cf, ce)
    fin = np.isfinite(se)
    err = np.abs(sf[fin].astype(np.float64) - se[fin].astype(np.float64))
    assert (err <= G.h16_sum_bound(se[fin], ce[fin], pts, thr)).all()
    assert rec.inliers == be["inliers"]
    # The reference's minimal solver (and so the device's) loses the model on several rows: the best of
    # these 2048 samples keeps 157 points on base and 149 on huge, 48-54 on offset / pow2_-40 / nan_only /
    # inf_only, under 10 on centred / unit / mixed / pow2_40 and none on pow2_62 and pow2_-70.  There the
    # comparison is of small counts; test_h_score_h16 carries those rows with the ground-truth family.
    if name in ("base", "huge", "far_all", "far_x1", "far_x2"):
        assert ce.max() >= 100


# ------------------------------------------------------------------------------------ two-view
_TV = [(n, k) for k in (True, False) for n in G.TV_ROWS]
_TV_IDS = ["%s-%s" % (n, "normalised" if k else "pixel") for n, k in _TV]


@pytest.mark.parametrize("kind", ["E", "F"])
@pytest.mark.parametrize("name,normalized", _TV, ids=_TV_IDS)
def test_two_view_score_f2(usac, kind, name, normalized):
    """k_score_f2, one chunk: counts equal, Σ bit-equal (tests/test_gpu_twoview_fast.py's assertions)."""
    pts, base, thr, models, scored, on_errors = _reference(kind, name, normalized)
    est_id = usac.ESTIMATOR.Essential if kind == "E" else usac.ESTIMATOR.Fundamental
    with usac.Context(est_id, pts) as ctx:
        for t, (oc, os_) in scored.items():
            gc, gs = ctx.score_models(models, t)
            np.testing.assert_array_equal(gc, oc, err_msg=str(t))
            _same_bits(gs, os_)
        _check_on_errors(ctx, base, on_errors)


@pytest.mark.parametrize("name,normalized", _TV, ids=_TV_IDS)
def test_e_score_e16(usac, name, normalized):
    """k_e16_rows + k_score_e16 (variant 3, four chunks): counts equal, Σ within the throughput bound."""
    pts, base, thr, models, scored, on_errors = _reference("E", name, normalized)
    with usac.Context(usac.ESTIMATOR.Essential, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(4)
        for t, (oc, os_) in scored.items():
            gc, gs = ctx.score_models(models, t)
            np.testing.assert_array_equal(gc, oc, err_msg=str(t))
            fin = np.isfinite(os_) & (oc > 0)
            err = np.abs(gs[fin].astype(np.float64) - os_[fin])
            assert (err <= G.e16_sum_bound(os_[fin], oc[fin], t)).all(), t
        _check_on_errors(ctx, base, on_errors)


@pytest.mark.parametrize("name,normalized", _TV, ids=_TV_IDS)
def test_e_hypothesize_e16(usac, name, normalized):
    """A device batch at eight chunks (k_score_e16 on the solver's listed slots) against the
    exact-expression kernel (variant 1) on the same seed, on the occupied slots."""
    pts, _, thr, _, _, _ = _reference("E", name, normalized)
    with usac.Context(usac.ESTIMATOR.Essential, pts) as ctx:
        ctx.set_score_variant(1)
        ce, se, be = ctx.hypothesize_score(B=B_HYP, seed=SEED, first_hyp=0, thr=thr)
        ctx.set_score_variant(0)
        ctx.set_score_chunks(8)
        ctx.hypothesize_async(B_HYP, SEED, 0, thr)
        rec = ctx.fetch_best()
        cf, sf = ctx.last_counts(B_HYP)
    occ = ce >= 0
    np.testing.assert_array_equal(cf[occ], ce[occ])
    assert (cf[~occ] < 0).all()
    fin = occ & np.isfinite(se)
    err = np.abs(sf[fin].astype(np.float64) - se[fin].astype(np.float64))
    assert (err <= G.e16_sum_bound(se[fin], ce[fin], thr)).all()
    if occ.any():
        assert rec.inliers == be["inliers"]
    if name not in ("all_nan", "identical", "x1_const"):
        assert occ.any()
