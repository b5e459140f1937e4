"""Preconditions of tests/test_gpu_scorer_geometry.py, on the CPU oracle alone: every geometry row
(tests/helpers/geometry.py) gives the oracle something to count, so that a GPU pass on it means
something -- live rows, pair errors near the thresholds, the power-of-two ladder's exact
invariance, and the rows that a non-finite coordinate takes out of the count."""
import numpy as np
import pytest

from tests.helpers import geometry as G

H_LIVE = {"base": 400, "centred": 400, "offset": 398, "unit": 400, "huge": 400, "aniso": 450, "mixed": 428,
          "far_all": 399, "far_x1": 399, "far_x2": 399, "identical": 40, "pow2_-70": 400, "pow2_-40": 400,
          "pow2_40": 400, "pow2_62": 400, "nan_only": 386, "inf_only": 386}


def _near(errs, thr):
    return int((np.abs(errs.astype(np.float64) - thr) < 0.05 * thr).sum())


@pytest.mark.parametrize("name", G.H_ROWS)
def test_homography_rows_are_live(oracle, name):
    pts, base, thr = G.h_row(name)
    assert pts.dtype == np.float32 and base.dtype == np.float32 and len(pts) <= 1500
    assert len(G.h_models(base, np.random.default_rng(0))) <= 270
    est = oracle.Estimator(oracle.HOMOGRAPHY, pts)
    c, _ = est.quality(base, thr)
    print(name, "kept by the base model:", c)
    if name == "all_nan":
        assert c == 0
    elif name == "x1_const":
        assert c >= 1 and np.ptp(pts[:, 0]) == 0 and len(pts) == 200
    elif name == "identical":
        assert c == 40 == len(pts) and (np.ptp(pts, axis=0) == 0).all()
    elif name == "pow2_-75":  # the reference's own squares are denormal here: the oracle's word stands
        assert 0 < c < 400
    else:
        assert c >= 100
    if name in H_LIVE:
        assert c == H_LIVE[name]
    if name in G.H_AFFINE:
        # pair errors within 5 % of a threshold the GPU test scores at.  aniso's own thr = 20 keeps all
        # 450 inliers with nothing near it (measured 0): its quarter threshold carries the near pairs (25)
        errs = est.errors(base)
        near = max(_near(errs, t) for t in ((thr, 0.25 * thr) if name == "aniso" else (thr,)))
        print(name, "errors within 5 % of thr:", near)
        assert near >= 10


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("name", G.TV_ROWS)
def test_two_view_rows_are_live(oracle, name, normalized):
    pts, base, thr = G.tv_row(name, normalized)
    assert len(pts) <= 1500 and len(G.e_models(base, np.random.default_rng(0))) <= 270
    c, _ = oracle.Estimator(oracle.ESSENTIAL, pts).quality(base, thr)
    print(name, normalized, "kept by the base model:", c)
    if name == "all_nan":
        assert c == 0
    elif name == "x1_const":
        assert c >= 1 and np.ptp(pts[:, 0]) == 0
    elif name == "identical":
        assert c == 40
    else:
        assert c >= 100
        if name in G.TV_AFFINE[normalized]:
            lo, hi = (453, 464) if normalized else (392, 457)
            assert lo <= c <= hi


def test_ladder_invariance(oracle):
    """Scaling by a power of two is exact: the oracle's counts of the base model and 20 perturbations
    are those of the unscaled set for k = -70 .. 62 (Σ scales exactly too while no square goes
    denormal).  At k = -75 the reference's own squares are denormal and the counts differ: that row's
    expectation is whatever the oracle says."""
    pts, Hgt = G.h_base()
    sel = [0] + [40 * j + i for j in range(4) for i in range(1, 6)]

    def scored(k):
        p, m = G.pow2_h(pts, Hgt, k)
        models = G.h_models(m, np.random.default_rng(11))[sel]
        return oracle.Estimator(oracle.HOMOGRAPHY, p).score_models(models, float(np.float32(2.0) * np.float32(2.0) ** np.float32(k)))

    c0, s0 = scored(0)
    assert c0[0] == H_LIVE["base"] and len(c0) == 21 and len(set(c0.tolist())) > 5
    bp, bm, bthr = G.h_row("base")
    assert oracle.Estimator(oracle.HOMOGRAPHY, bp).quality(bm, bthr)[0] == c0[0]
    for k in (-70, -40, 40, 62):
        c, s = scored(k)
        np.testing.assert_array_equal(c, c0)
        if k != -70:
            np.testing.assert_array_equal(s, s0 * np.float32(2.0) ** np.float32(k))
    c, _ = scored(-75)
    assert c[0] == 379 and (c != c0).any()


@pytest.mark.parametrize("kind", ["H", "En", "Ep", "Fn", "Fp"])
def test_nonfinite_rows_left_out(oracle, kind):
    """nan_only / inf_only spoil the same 40 rows: the oracle leaves out exactly those of them that the
    base set counted, the box of nan_only stays finite, and inf_only counts what nan_only counts."""
    if kind == "H":
        okind, row, pinned = oracle.HOMOGRAPHY, G.h_row, 14
    else:
        okind = oracle.ESSENTIAL if kind[0] == "E" else oracle.FUNDAMENTAL
        row = lambda name: G.tv_row(name, kind[1] == "n")  # noqa: E731
        pinned = {"En": 9, "Ep": 6, "Fn": 13, "Fp": 9}[kind]
    pts, base, thr = row("base")
    bad = G.bad_rows(len(pts))
    live = oracle.Estimator(okind, pts).errors(base) < thr
    left_out = int(live[bad].sum())
    for name in ("nan_only", "inf_only"):
        p, b, t = row(name)
        np.testing.assert_array_equal(b, base)
        assert t == thr
        spoiled = ~np.isfinite(p).all(1)
        assert spoiled.sum() == 40 and spoiled[bad].all()
        if name == "nan_only":
            assert not np.isinf(p).any() and np.isfinite(np.nanmax(np.abs(p)))
        else:
            assert not np.isnan(p).any() and np.isinf(p).sum() == 40
        c, _ = oracle.Estimator(okind, p).quality(b, t)
        assert c == int(live.sum()) - left_out
    assert left_out == pinned
