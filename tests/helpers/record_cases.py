"""The inputs of the batch-record tests, shared by tests/test_batch_record_cpu.py (which asserts the
properties that keep the GPU tests from being vacuous) and tests/test_gpu_batch_record.py.

unique_best(kind): 1 000 points and a base batch of host samples whose exact counts have exactly one
slot at the maximum.  count_tie(kind, n): an all-inlier set of n = 16 or 33 points and a base batch in
which many slots tie at count == n.  `oracle` is the oracle module (the fixture's value)."""
import numpy as np

from ransac_amd import synthetic

KINDS = ("H", "F", "E", "L")
THR = {"H": 2.0, "F": 2.0, "E": 0.002, "L": 10.0}
M = {"H": 4, "F": 7, "E": 5, "L": 2}
SPK = {"H": 1, "F": 3, "E": 1, "L": 1}
UNIQUE_ROWS = {"H": 4352, "F": 2048, "E": 1024, "L": 4352}
UNIQUE_SEEDS = {"H": (21, 41), "F": (31, 41), "E": (31, 41), "L": (22, 42)}  # (data, samples)
TIE_ROWS = {"H": 2304, "F": 1024, "E": 1024, "L": 1024}


def okind(oracle, kind):
    return {"H": oracle.HOMOGRAPHY, "F": oracle.FUNDAMENTAL, "E": oracle.ESSENTIAL, "L": oracle.LINE2D}[kind]


def estimator(usac, kind):
    E = usac.ESTIMATOR
    return {"H": E.Homography, "F": E.Fundamental, "E": E.Essential, "L": E.Line2d}[kind]


def unique_best(oracle, kind):
    """-> (points 1000 x cols, samples rows x m, thr)"""
    ds, ss = UNIQUE_SEEDS[kind]
    if kind == "H":
        pts = synthetic.homography_points(n=1000, inlier_ratio=0.3, seed=ds)[0]
    elif kind == "L":
        pts = synthetic.line_points(n=1000, inlier_ratio=0.3, seed=ds)[0]
    else:
        pts = synthetic.fundamental_points(n=1000, inlier_ratio=0.5, seed=ds, prosac_order=False,
                                           normalized=kind == "E")[0]
    return pts, oracle.uniform_samples(ss, len(pts), M[kind], UNIQUE_ROWS[kind]), THR[kind]


def count_tie(oracle, kind, n):
    """-> (points n x cols, samples rows x m, thr): every point an inlier of the ground truth"""
    if kind == "H":
        pts = synthetic.homography_points(n=n, inlier_ratio=1.0, seed=5, noise=0.3)[0]
    elif kind == "L":
        pts = synthetic.line_points(n=n, inlier_ratio=1.0, seed=5, noise=0.3)[0]
    else:
        pts = synthetic.fundamental_points(n=n, inlier_ratio=1.0, seed=5, noise=0.2, prosac_order=False,
                                           normalized=kind == "E")[0]
    return pts, oracle.uniform_samples(7, len(pts), M[kind], TIE_ROWS[kind]), THR[kind]


def degenerate(oracle, kind):
    """F / E -> (points, thr, degenerate rows (2 x m), a healthy row): unique_best's 1 000 points of which
    m share a coordinate and one is non-finite; the rows sample those, the healthy row is the base
    batch's best"""
    pts, base, thr = unique_best(oracle, kind)
    c, s, _ = oracle_scores(oracle, kind, pts, base, thr)
    m = M[kind]
    pts = pts.copy()
    pts[17:17 + m, 2] = pts[17, 2]
    pts[30] = [np.inf, 0.1, 0.2, 0.3]
    bad = np.array([list(range(17, 17 + m)), [30] + list(range(1, m))], np.int32)
    return pts, thr, bad, base[int(np.argmax(c)) // SPK[kind]].copy()


def oracle_scores(oracle, kind, pts, samples, thr):
    """The oracle's per-slot (counts, sums, models S x 9): slot spk * b + j = the j-th model of sample
    b, count -1 for a slot without a model."""
    est = oracle.Estimator(okind(oracle, kind), pts)
    models, nm = est.estimate_batch(samples)
    spk = SPK[kind]
    models = np.ascontiguousarray(models.reshape(len(samples) * spk, 9))
    c, s = est.score_models(models, thr)
    occupied = (np.arange(spk)[None, :] < nm[:, None]).reshape(-1)
    return np.where(occupied, c, -1).astype(np.int32), np.where(occupied, s, 0).astype(np.float32), models


def top(counts, sums):
    """(slots at the maximum count, the maximum, the runner-up's count)"""
    mx = int(counts.max())
    tied = np.flatnonzero(counts == mx)
    rest = counts[counts < mx]
    return tied, mx, (int(rest.max()) if len(rest) else None)
