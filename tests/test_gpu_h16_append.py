"""The kept-pair append of the matrix-core homography scorer (kernels_h16.hip k_score_h16) on inputs
whose kept pairs are known exactly: ballot masks with a single kept lane (most non-empty masks of a
real batch; a one-lane store at the wave-uniform ring tail was tried for them and measured slower,
DESIGN.md §6 -- these cases hold for either form) beside masks of several lanes and dense ones,
with the two blocks of a loop trip taking different paths.

Point sets: the noise-free all-inlier generator with (x2, y2) of every point but a chosen index
set moved by at least 100 px, so H_gt keeps exactly the chosen pairs and the oracle's count of
H_gt is the size of the set.  A mask is 64 lanes = hypotheses (10 a + j, 10 a + 5 + j) x 32 points,
so a batch of H_gt copies puts two lanes into a mask wherever a block has one inlier; with H_gt in
one lane half only ("lo": slots 0-4 of each ten, "hi": slots 5-9) and a model that keeps nothing
(H_gt moved by 10^5 px) in the other, every such mask has one lane: lanes 0 / 31 ("lo", inliers
at block positions 0 / 31) and 32 / 63 ("hi").

The library chooses the scorer's point chunks itself (small batches: up to 256 chunks, one to five
32-point blocks per wave on the sets here), so the in-process cases exercise the appends block by
block; the streams that need many blocks in one wave (single and multi-lane appends interleaved,
the count passing 64 on a single append with the drain after it; more than 1024 single appends,
so the ring index wraps on them) run once more in a child process with USAC_H16_CHUNKS=1 (the
knob is read once per process).

Counts equal the CPU oracle's; Σ within the bound of test_gpu_h16_queue.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ransac_amd import synthetic  # noqa: E402

THR = 2.0
BATCHES = (1, 20, 21, 80, 81)
PATTERNS = ("lo", "hi", "all")


def _bound(sums_ref, counts, pts, thr):
    """test_gpu_h16_queue.py's Σ bound"""
    c = np.maximum(counts, 0).astype(np.float64)
    mp = float(np.abs(pts[np.isfinite(pts).all(1)].astype(np.float64)).sum(1).max())
    return np.abs(sums_ref.astype(np.float64)) * c * 2.0 ** -23 + c * (2.0 ** -22 * mp + 2.0 ** -18 * thr)


def _one_per_block(n):
    """one inlier per 32-point block: position 0 of the even blocks, 31 of the odd ones"""
    idx = [32 * b + (31 if b & 1 else 0) for b in range((n + 31) // 32)]
    return np.array([i for i in idx if i < n])


def _one_and_five(n):
    """even blocks hold one inlier (position 0 or 31 in turn), odd blocks five (0, 7, 15, 16, 31)"""
    idx = []
    for b in range((n + 31) // 32):
        idx += [32 * b + p for p in ((0, 7, 15, 16, 31) if b & 1 else ((31,) if b & 2 else (0,)))]
    return np.array([i for i in idx if i < n])


SETS = {"one": _one_per_block, "one_five": _one_and_five}


@functools.lru_cache(maxsize=None)
def _case(n, kind):
    """(points, [H_gt, the keep-nothing model] as 2 x 9 floats, the oracle's counts and Σ of the two,
    the chosen index set)"""
    from oracle import oracle as O

    pts, Hgt, _ = synthetic.homography_points(n, inlier_ratio=1.0, noise=0.0)
    pts = pts.copy()
    chosen = SETS[kind](n)
    out = np.ones(n, bool)
    out[chosen] = False
    # 100 px and more, by a per-point amount (no second homography fits the moved points)
    k = np.arange(n, dtype=np.float32)
    pts[out, 2] += 100.0 + 7.0 * (k[out] % 13)
    pts[out, 3] -= 100.0 + 5.0 * (k[out] % 17)
    h = np.ascontiguousarray(Hgt, np.float32).reshape(9)
    far = h.copy()
    far[2] += 1e5
    two = np.stack([h, far])
    oc, os_ = O.Estimator(O.HOMOGRAPHY, pts).score_models(two, THR)
    for a in (pts, two, oc, os_, chosen):
        a.setflags(write=False)
    return pts, two, oc, os_, chosen


def _select(B, pattern):
    """model index per hypothesis: 0 = H_gt, 1 = the keep-nothing model"""
    half = (np.arange(B) % 10) >= 5
    return {"lo": half, "hi": ~half, "all": np.zeros(B, bool)}[pattern].astype(np.intp)


@functools.lru_cache(maxsize=None)
def _mixed_case(n, kind):
    """41 models on a point set above: H_gt at 0, 7, 25 and 40, a NaN model at 12 (F = +inf: all its
    masks are dense), random models elsewhere."""
    from oracle import oracle as O

    pts, two, _, _, _ = _case(n, kind)
    models = np.random.default_rng(21).standard_normal((41, 9)).astype(np.float32)
    models[[0, 7, 25, 40]] = two[0]
    models[12] = np.nan
    oc, os_ = O.Estimator(O.HOMOGRAPHY, pts).score_models(models, THR)
    for a in (models, oc, os_):
        a.setflags(write=False)
    return pts, models, oc, os_


def test_append_inputs_on_the_oracle():
    """The inputs do what the GPU cases rely on (no GPU): H_gt counts exactly the chosen pairs, the
    keep-nothing model none, and the mixed batch holds full, empty and NaN hypotheses."""
    for n, kind in ((65, "one"), (2049, "one"), (4096, "one_five"), (40001, "one")):
        _, _, oc, os_, chosen = _case(n, kind)
        assert oc[0] == len(chosen) and oc[1] == 0 and np.isfinite(os_[0])
    assert len(_case(65, "one")[4]) == 3 and len(_case(40001, "one")[4]) == 1251
    assert len(_case(4096, "one_five")[4]) == 64 * 6
    for n, kind in ((2049, "one"), (4096, "one_five")):
        _, _, oc, _ = _mixed_case(n, kind)
        assert (oc[[0, 7, 25, 40]] == len(_case(n, kind)[4])).all() and oc[12] == 0
        assert (np.delete(oc, [0, 7, 25, 40]) < 8).all()


def _check(ctx, pts, models, oc, os_):
    gc, gs = ctx.score_models(models, THR)
    print("counts gpu", gc[:6], "oracle", oc[:6])
    np.testing.assert_array_equal(gc, oc)
    fin = np.isfinite(os_)
    err = np.abs(gs[fin].astype(np.float64) - os_[fin])
    bound = _bound(os_[fin], oc[fin], pts, THR)
    print("max |Σ err| / bound", float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0)
    assert (err <= bound).all()


def _check_patterns(ctx, n, kind, batches):
    pts, two, oc2, os2, _ = _case(n, kind)
    for B in batches:
        for pattern in PATTERNS:
            sel = _select(B, pattern)
            _check(ctx, pts, two[sel], oc2[sel], os2[sel])


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [2, 8])
@pytest.mark.parametrize("n", [65, 2049])
def test_single_lane_appends(usac, n, chunks):
    """One inlier per block at positions 0 / 31: with H_gt in one lane half every append is a
    one-lane mask (lanes 0, 31, 32, 63); full copies give two-lane masks; partial waves and
    workgroups at every batch size; 65 points: three blocks, so a trip's second block is missing."""
    pts = _case(n, "one")[0]
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(chunks)
        _check_patterns(ctx, n, "one", BATCHES)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [2, 8])
def test_single_and_multi_lane_interleave(usac, chunks):
    """4096 points, 21 hypotheses, blocks of one and five inliers in turn."""
    pts = _case(4096, "one_five")[0]
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(chunks)
        _check_patterns(ctx, 4096, "one_five", (21,))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [2, 8])
def test_many_single_appends(usac, chunks):
    """40 001 points, one inlier per block, 21 hypotheses."""
    pts = _case(40001, "one")[0]
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(chunks)
        _check_patterns(ctx, 40001, "one", (21,))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [2, 8])
@pytest.mark.parametrize("n,kind", [(2049, "one"), (4096, "one_five")])
def test_mixed_batch(usac, n, kind, chunks):
    """H_gt copies, random models and a NaN model (dense masks) in one batch."""
    pts, models, oc, os_ = _mixed_case(n, kind)
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_variant(3)
        ctx.set_score_chunks(chunks)
        _check(ctx, pts, models, oc, os_)


def _long_streams():
    """Run by the child process (one point chunk: a wave walks every block of the set)."""
    import ransac_amd as usac

    for n, kind in ((4096, "one_five"), (40001, "one")):
        pts = _case(n, kind)[0]
        for chunks in (2, 8):
            with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
                ctx.set_score_variant(3)
                ctx.set_score_chunks(chunks)
                _check_patterns(ctx, n, kind, (21,))
                if n == 4096:
                    _check(ctx, *_mixed_case(n, kind))
    print("long streams ok")


@pytest.mark.gpu
def test_long_streams_in_one_wave():
    """One point chunk (USAC_H16_CHUNKS=1 in a child process).  4096 points, "lo" / "hi": a wave
    appends 10 single entries on an even block and 10 masks of five lanes on an odd one, so its
    count passes 64 on the fifth single append of the third block and the drain follows it;
    40 001 points: 12 510 single appends per wave into the 1024-entry ring, twelve wraps."""
    env = dict(os.environ, USAC_H16_CHUNKS="1")
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "long streams ok" in r.stdout


if __name__ == "__main__":
    _long_streams()
