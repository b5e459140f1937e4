"""The matrix-core homography scorer (kernels_h16.hip) with its prefilter slack at the fp16 rounding
bound (usac_h16.hpp h16_rows_of): a pair the tighter prefilter drops must be one the exact
stage would have rejected, so counts equal the CPU oracle's exactly and Σ stays within the throughput
bound of test_gpu_h16.py (|Σ| c 2^-23 + c (2^-22 Mp + 2^-18 thr)).

Shapes: 33 points (a partial second block), 65 (two blocks and one point), 2 048 (several point chunks);
81 models per call (one full workgroup of four 20-hypothesis waves plus a wave with one hypothesis).
Models: the ground truth and 40 perturbations of it from 2^-4 down to one ulp; 40 four-point DLT models
of all-inlier, mixed and all-outlier samples; the ground truth with one of its rows scaled by 2^±k,
k = 2 .. 26, so the rows' common scale 2^e and the small coefficients sweep the fp16 range, subnormal
and flushed ones included.  Thresholds: the usual three, and for eight models of each kind their own pair
errors at 24 ranks spread over the sorted errors with the next float above each."""
import numpy as np
import pytest

from ransac_amd import synthetic

pytestmark = pytest.mark.gpu

SIZES = (33, 65, 2048)
KINDS = ("perturbed", "dlt", "scaled")


def _bound(sums_ref, counts, pts, thr):
    c = np.maximum(counts, 0).astype(np.float64)
    mp = float(np.abs(pts[np.isfinite(pts).all(1)].astype(np.float64)).sum(1).max())
    return np.abs(sums_ref.astype(np.float64)) * c * 2.0 ** -23 + c * (2.0 ** -22 * mp + 2.0 ** -18 * thr)


def _perturbed(base, rng):
    out = []
    for i in range(38):  # relative size 2^-4 .. 2^-22, two of each
        k = 4 + i // 2
        out.append(base * (np.float32(1) + np.float32(2.0 ** -k) * rng.uniform(-1, 1, 9).astype(np.float32)))
    out.append(np.nextafter(base, np.float32(np.inf)))   # one ulp, every coefficient
    out.append(np.nextafter(base, np.float32(-np.inf)))
    return out


def _dlt(oracle, pts, inl, rng):
    i_in, i_out = np.flatnonzero(inl), np.flatnonzero(~inl)
    samples = [rng.choice(i_in, 4, replace=False) for _ in range(14)]
    samples += [np.concatenate([rng.choice(i_in, 2, replace=False), rng.choice(i_out, 2, replace=False)])
                for _ in range(13)]
    samples += [rng.choice(i_out, 4, replace=False) for _ in range(13)]
    est = oracle.Estimator(oracle.HOMOGRAPHY, pts, oracle.DLT_THIN)
    models, _ = est.estimate_batch(np.stack(samples).astype(np.int32))
    return list(models.astype(np.float32))


def _scaled(base):
    out = [base, base * np.float32(2.0 ** 40), base * np.float32(2.0 ** -40)]
    for r in range(3):
        for k in range(2, 27, 2):
            for s in (k, -k):
                m = base.copy()
                m[3 * r:3 * r + 3] *= np.float32(2.0 ** s)
                out.append(m)
    return out


_CASES = {}


def _case(oracle, n):
    """points, oracle estimator and the two 81-model batches of one size (built once, never changed)"""
    if n not in _CASES:
        pts, Hgt, inl = synthetic.homography_points(n=n, inlier_ratio=0.3, seed=11)
        rng = np.random.default_rng(100 + n)
        base = (Hgt / Hgt[2, 2]).reshape(9).astype(np.float32)
        a = np.stack([base] + _perturbed(base, rng) + _dlt(oracle, pts, inl, rng)).astype(np.float32)
        b = np.stack(_scaled(base)).astype(np.float32)
        assert a.shape == b.shape == (81, 9)
        a.setflags(write=False)
        b.setflags(write=False)
        _CASES[n] = (pts, oracle.Estimator(oracle.HOMOGRAPHY, pts), {"perturbed": a, "dlt": a, "scaled": b})
    return _CASES[n]


def _check(ctx, est, pts, models, thr, what):
    gc, gs = ctx.score_models(models, thr)
    oc, os_ = est.score_models(models, thr)
    np.testing.assert_array_equal(gc, oc, err_msg="%s, thr %r" % (what, thr))
    fin = np.isfinite(os_)
    err = np.abs(gs[fin].astype(np.float64) - os_[fin])
    assert (err <= _bound(os_[fin], oc[fin], pts, thr)).all(), "%s, thr %r: sums" % (what, thr)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("batch", ["perturbed", "scaled"])
def test_h16_slack_counts_equal_oracle(usac, oracle, n, batch):
    pts, est, sets = _case(oracle, n)
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(4)
        for thr in (2.0, 0.5, 7.3):
            _check(ctx, est, pts, sets[batch], thr, "%s batch, %d points" % (batch, n))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_h16_slack_thresholds_on_pair_errors(usac, oracle, n, kind):
    """a threshold exactly on a pair's error excludes the pair, the next float includes it: for eight
    models of the kind, at 24 ranks of their sorted errors, the whole 81-model batch scored each time"""
    pts, est, sets = _case(oracle, n)
    models = sets[kind]
    first = {"perturbed": 1, "dlt": 41, "scaled": 3}[kind]
    span = {"perturbed": 40, "dlt": 40, "scaled": 78}[kind]
    chosen = [first + (i * span) // 8 for i in range(8)]
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(4)
        for m in chosen:
            errs = est.errors(models[m])
            errs = np.sort(errs[np.isfinite(errs) & (errs > 0)])
            assert len(errs) >= 24, "model %d has too few finite pair errors" % m
            for e in errs[np.linspace(0, len(errs) - 1, 24).astype(int)]:
                for thr in (float(e), float(np.nextafter(np.float32(e), np.float32(np.inf)))):
                    _check(ctx, est, pts, models, thr, "%s model %d, %d points" % (kind, m, n))
