"""The kept-pair queue of the matrix-core homography scorer (kernels_h16.hip k_score_h16): the
per-wave LDS ring, its drains and the drains' direct model fetch, on inputs where every pair is
kept (all-inlier point sets scored by copies of H_gt: each 32-point block appends 64 entries per
hypothesis pair of halves and the ring wraps), where only some waves ever drain, and where
non-finite models send every pair to the exact stage.  Counts equal the CPU oracle's; Σ within the
throughput bound of test_gpu_h16.py.

set_score_chunks takes 1, 2, 4, 8 or 16 for a homography context (any value > 1 selects the
multi-chunk scorer under score variant 3); the scorer's own number of point chunks is the library's
(one 32-point block per chunk on the small sets here, 13 blocks per chunk on the 100 001-point set)."""
import functools

import numpy as np
import pytest

from ransac_amd import synthetic

THR = 2.0
# 20 hypotheses per wave, 80 per workgroup; 61 and 141: only the last wave's first hypothesis exists
BATCHES = (1, 19, 20, 21, 61, 79, 80, 81, 141)


def _bound(sums_ref, counts, pts, thr):
    c = np.maximum(counts, 0).astype(np.float64)
    mp = float(np.abs(pts[np.isfinite(pts).all(1)].astype(np.float64)).sum(1).max())
    return np.abs(sums_ref.astype(np.float64)) * c * 2.0 ** -23 + c * (2.0 ** -22 * mp + 2.0 ** -18 * thr)


@functools.lru_cache(maxsize=None)
def _all_inlier_case(n):
    """(points, H_gt as 9 floats, the oracle's (count, Σ) of H_gt): every point an exact inlier."""
    from oracle import oracle as O

    pts, Hgt, _ = synthetic.homography_points(n, inlier_ratio=1.0, noise=0.0)
    h = np.ascontiguousarray(Hgt, np.float32).reshape(9)
    oc, os_ = O.Estimator(O.HOMOGRAPHY, pts).score_models(h[None], THR)
    for a in (pts, h, oc, os_):
        a.setflags(write=False)
    return pts, h, oc, os_


@functools.lru_cache(maxsize=None)
def _mixed_case():
    """81 models over 2049 points (30 % inliers): hypotheses 0, 20, 40 and 80 are H_gt, the rest random."""
    from oracle import oracle as O

    pts, Hgt, _ = synthetic.homography_points(2049, inlier_ratio=0.3)
    models = np.random.default_rng(11).standard_normal((81, 9)).astype(np.float32)
    models[[0, 20, 40, 80]] = np.asarray(Hgt, np.float32).reshape(9)
    oc, os_ = O.Estimator(O.HOMOGRAPHY, pts).score_models(models, THR)
    for a in (pts, models, oc, os_):
        a.setflags(write=False)
    return pts, models, oc, os_


@functools.lru_cache(maxsize=None)
def _nonfinite_case():
    """21 models over 65 all-inlier points: NaN, inf and zero models among copies of H_gt and random ones."""
    from oracle import oracle as O

    pts, Hgt, _ = synthetic.homography_points(65, inlier_ratio=1.0, noise=0.0)
    h = np.asarray(Hgt, np.float32).reshape(9)
    models = np.random.default_rng(12).standard_normal((21, 9)).astype(np.float32)
    models[[0, 7, 20]] = h
    models[1] = np.nan
    models[2] = np.inf
    models[3] = 0.0
    models[4] = h
    models[4, 4] = np.nan
    models[5] = h
    models[5, 8] = -np.inf
    models[19] = np.nan
    oc, os_ = O.Estimator(O.HOMOGRAPHY, pts).score_models(models, THR)
    for a in (pts, models, oc, os_):
        a.setflags(write=False)
    return pts, models, oc, os_


def test_queue_inputs_on_the_oracle():
    """The inputs do what the GPU cases rely on (no GPU): H_gt counts every point of the all-inlier
    sets, and the mixed / non-finite batches hold both full and empty hypotheses."""
    for n in (33, 65, 2049, 4096, 100001):
        _, _, oc, os_ = _all_inlier_case(n)
        assert oc[0] == n and np.isfinite(os_[0])
    _, _, oc, _ = _mixed_case()
    # 615 inliers with sigma = 1 noise per coordinate: most of them within 2 px of H_gt
    assert (oc[[0, 20, 40, 80]] >= 400).all() and (np.delete(oc, [0, 20, 40, 80]) < 100).all()
    _, models, oc, _ = _nonfinite_case()
    assert (oc[[0, 7, 20]] == 65).all() and (oc[[1, 2, 3, 4, 5, 19]] == 0).all()


def _check(ctx, pts, models, oc, os_):
    gc, gs = ctx.score_models(models, THR)
    print("counts gpu", gc[:4], "oracle", oc[:4])
    np.testing.assert_array_equal(gc, oc)
    fin = np.isfinite(os_)
    err = np.abs(gs[fin].astype(np.float64) - os_[fin])
    bound = _bound(os_[fin], oc[fin], pts, THR)
    print("max |Σ err| / bound", float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0)
    assert (err <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [2, 8, 16])
@pytest.mark.parametrize("n", [33, 2049, 4096])
def test_every_pair_kept(usac, n, chunks):
    """Every (hypothesis, point) pair is kept: each wave appends 64 entries per mask and drains its
    ring ten times per 32-point block; partial waves and workgroups at every batch size."""
    pts, h, oc1, os1 = _all_inlier_case(n)
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(chunks)
        for B in BATCHES:
            _check(ctx, pts, np.tile(h, (B, 1)), np.repeat(oc1, B), np.repeat(os1, B))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [21, 81])
def test_ring_wraps(usac, B):
    """100 001 points: the library's 256 point chunks hold 13 blocks each, so a wave appends 8 320
    entries to its 1 024-entry ring -- eight wraps, with drains between the appends of one block."""
    pts, h, oc1, os1 = _all_inlier_case(100001)
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(8)
        _check(ctx, pts, np.tile(h, (B, 1)), np.repeat(oc1, B), np.repeat(os1, B))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [2, 8, 16])
def test_mixed_waves(usac, chunks):
    """Waves whose first hypothesis alone keeps pairs beside waves that drain rarely or never
    (random models): the drains fetch their models straight from the batch's table."""
    pts, models, oc, os_ = _mixed_case()
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(chunks)
        _check(ctx, pts, models, oc, os_)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [2, 8, 16])
def test_nonfinite_models(usac, chunks):
    """NaN / inf / zero models (F = +inf: every pair of theirs goes to the exact stage) among exact ones."""
    pts, models, oc, os_ = _nonfinite_case()
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(chunks)
        _check(ctx, pts, models, oc, os_)
