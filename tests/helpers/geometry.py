"""Dataset geometries for the guard-band scorers' parity tests (numpy only).

The scorers k_score_hf, k_score_h16, k_score_e16 and k_score_f2 prove their rejections from
constants of the point set (the box of |coordinates|, the box centres, power-of-two scales, feature
maxima).  The tables below move a base point set through axis-aligned affine maps of each image,
and the ground-truth model with it, so that those constants change while the oracle's task stays
the same: centres far from zero, scales far from 2^10, features in the fp16 subnormal range, a
zero extent, an empty box, coordinates whose squares leave the fp32 range.

A transform is A = (sx, sy, tx, ty): x' = sx x + tx, y' = sy y + ty.  Points are computed in fp64 and
rounded once to fp32; models are normalised by their largest entry and rounded to fp32 (the
power-of-two ladder keeps the model's scale: its scaling is exact).
"""
import numpy as np

from ransac_amd import synthetic

IDENT = (1.0, 1.0, 0.0, 0.0)


def affine(A):
    sx, sy, tx, ty = A
    return np.array([[sx, 0.0, tx], [0.0, sy, ty], [0.0, 0.0, 1.0]], np.float64)


def transform(pts, A1, A2):
    """Image 1 by A1, image 2 by A2; fp64, rounded once to fp32."""
    p = np.asarray(pts, np.float64)
    out = np.empty_like(p)
    out[:, 0] = A1[0] * p[:, 0] + A1[2]
    out[:, 1] = A1[1] * p[:, 1] + A1[3]
    out[:, 2] = A2[0] * p[:, 2] + A2[2]
    out[:, 3] = A2[1] * p[:, 3] + A2[3]
    return np.ascontiguousarray(out, dtype=np.float32)


def _normalised(M):
    return (M / np.abs(M).max()).reshape(9).astype(np.float32)


def transform_h(H, A1, A2):
    """H' = A2 H A1^-1 (x2' ~ H' x1'), largest entry 1."""
    return _normalised(affine(A2) @ np.asarray(H, np.float64).reshape(3, 3) @ np.linalg.inv(affine(A1)))


def transform_f(M, A1, A2):
    """F' = E' = A2^-T M A1^-1 (x2'^T M' x1' = x2^T M x1), largest entry 1."""
    return _normalised(np.linalg.inv(affine(A2)).T @ np.asarray(M, np.float64).reshape(3, 3) @ np.linalg.inv(affine(A1)))


def pow2_h(pts, H, k):
    """The ladder: points times 2^k (exact), h2 and h5 times 2^k, h6 and h7 times 2^-k, no renormalisation."""
    base = (np.asarray(H, np.float64) / np.asarray(H, np.float64)[2, 2]).reshape(9).astype(np.float32)
    s = np.float32(2.0) ** np.float32(k)
    m = base.copy()
    m[[2, 5]] *= s
    m[[6, 7]] /= s
    return np.ascontiguousarray(np.asarray(pts, np.float32) * s), m


# ------------------------------------------------------------------------------------ model families
def _common_models(base, rng):
    models = [base]
    for scale in (1e-6, 1e-4, 1e-2, 1.0):
        models += [base * (1 + scale * rng.standard_normal(9).astype(np.float32)) for _ in range(40)]
    models += [rng.standard_normal(9).astype(np.float32) * 10 ** rng.uniform(-20, 20) for _ in range(100)]
    return models


def _quiet(fn):
    """the families multiply up to inf on purpose (1e30 times a ladder model)"""
    def wrapped(base, rng):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return fn(base, rng)
    wrapped.__doc__ = fn.__doc__
    return wrapped


@_quiet
def h_models(base, rng):
    """tests/test_gpu_h16.py::_adversarial_models around `base` (9 floats): 1 + 160 + 100 + 7 models."""
    base = np.asarray(base, np.float32)
    models = _common_models(base, rng)
    tiny = base.copy()
    tiny[6:] = [1e-30, -1e-30, 1e-38]
    singular = np.array([1, 2, 3, 2, 4, 6, 1e-3, 2e-3, 3e-3], np.float32)
    models += [tiny, base * np.float32(1e30), base * np.float32(1e-30), np.full(9, np.nan, np.float32),
               np.full(9, np.inf, np.float32), np.zeros(9, np.float32), singular]
    return np.stack(models).astype(np.float32)


@_quiet
def e_models(base, rng):
    """tests/test_gpu_e16.py::_adversarial_models around `base`: 1 + 160 + 100 + 9 models."""
    base = np.asarray(base, np.float32)
    models = _common_models(base, rng)
    rank1 = np.outer([1.0, 2.0, -1.0], [0.5, -1.0, 2.0]).reshape(9).astype(np.float32)
    models += [base * np.float32(1e30), base * np.float32(1e-30), base * np.float32(1e19), np.full(9, np.nan, np.float32),
               np.full(9, np.inf, np.float32), np.zeros(9, np.float32), rank1,
               np.array([0, 0, 0, 0, 0, 0, 0, 0, 1], np.float32), np.array([0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32)]
    return np.stack(models).astype(np.float32)


# ------------------------------------------------------------------------------------ Σ bounds
def _finite_rows(pts):
    return pts[np.isfinite(pts).all(1)]


def h16_sum_bound(sums_ref, counts, pts, thr):
    """tests/test_gpu_h16.py::_bound: |Σ| c 2^-23 + c (2^-22 Mp + 2^-18 thr), Mp over the finite rows
    (0 for a set without one: its counts are 0)."""
    c = np.maximum(counts, 0).astype(np.float64)
    fin = _finite_rows(pts)
    mp = float(np.abs(fin.astype(np.float64)).sum(1).max()) if len(fin) else 0.0
    return np.abs(sums_ref.astype(np.float64)) * c * 2.0 ** -23 + c * (2.0 ** -22 * mp + 2.0 ** -18 * thr)


def e16_sum_bound(sums_ref, counts, thr):
    """tests/test_gpu_e16.py::_bound: |Σ| c 2^-23 + c thr 2^-18."""
    c = np.maximum(counts, 0).astype(np.float64)
    return np.abs(sums_ref.astype(np.float64)) * c * 2.0 ** -23 + c * thr * 2.0 ** -18


# ------------------------------------------------------------------------------------ box stress
_BAD_COLS = (0, 3, 1, 2)  # ten rows each: the column that is made non-finite


def bad_rows(n, seed=7):
    """The 40 rows that nan_only / inf_only spoil (the same rows in both)."""
    return np.random.default_rng(seed).choice(n, 40, replace=False)


def _spoil(pts, values):
    out = pts.copy()
    bad = bad_rows(len(pts))
    for j, (col, v) in enumerate(zip(_BAD_COLS, values)):
        out[bad[10 * j: 10 * j + 10], col] = v
    return out


def _box_rows(pts, live, fars):
    """Box-stress variants of a base set; `live` = a row the base model keeps; fars: name -> far row."""
    rows = {}
    for name, far in fars.items():
        p = pts.copy()
        p[live] = far
        rows[name] = p
    x1c = pts[:200].copy()
    keep = live if live < 200 else 0
    x1c[:, 0] = x1c[keep, 0]
    rows["x1_const"] = x1c
    rows["identical"] = np.repeat(pts[live: live + 1], 40, axis=0)
    rows["all_nan"] = np.full((33, 4), np.nan, np.float32)
    rows["nan_only"] = _spoil(pts, (np.nan, np.nan, np.nan, np.nan))
    rows["inf_only"] = _spoil(pts, (np.inf, np.inf, -np.inf, -np.inf))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in rows.items()}


# ------------------------------------------------------------------------------------ homography table
H_AFFINE = {  # name: (A1, A2, thr)
    "base": (IDENT, IDENT, 2.0),
    "centred": ((1, 1, -500, -500), (1, 1, -500, -500), 2.0),
    "offset": ((1, 1, 1e5, -3e4), (1, 1, -7e4, 2e5), 2.0),
    "unit": ((1e-3, 1e-3, 0, 0), (1e-3, 1e-3, 0, 0), 2e-3),
    "huge": ((1e4, 1e4, 0, 0), (1e4, 1e4, 0, 0), 2e4),
    "aniso": ((4, 1 / 256, 0, 0), (1 / 256, 8, 0, 0), 20.0),
    "mixed": ((1e-2, 1e-2, 3, 3), (50, 50, -2e4, 1e4), 60.0),
}
H_POW2 = (-75, -70, -40, 40, 62)
H_FAR = {
    "far_all": (3e6, -2e6, 1e6, 5e6),
    "far_x1": (3e6, -2e6, 400, 300),
    "far_x2": (100, 200, -4e7, 9e6),
}
H_BOX = tuple(H_FAR) + ("x1_const", "identical", "all_nan", "nan_only", "inf_only")
H_ROWS = tuple(H_AFFINE) + tuple("pow2_%d" % k for k in H_POW2) + H_BOX


def h_base():
    pts, Hgt, _ = synthetic.homography_points(n=1500, inlier_ratio=0.3, seed=4)
    return pts, Hgt


def _h_live_row(pts, Hgt):
    """the first row the fp64 symmetric transfer error of the ground truth puts well inside thr = 2"""
    H = np.asarray(Hgt, np.float64)
    p1 = np.c_[pts[:, :2].astype(np.float64), np.ones(len(pts))]
    q = p1 @ H.T
    d = np.hypot(q[:, 0] / q[:, 2] - pts[:, 2], q[:, 1] / q[:, 2] - pts[:, 3])
    return int(np.flatnonzero(d < 0.5)[0])


def h_row(name):
    """-> (points N x 4 fp32, base model (9,) fp32, thr)"""
    pts, Hgt = h_base()
    if name in H_AFFINE:
        A1, A2, thr = H_AFFINE[name]
        return transform(pts, A1, A2), transform_h(Hgt, A1, A2), thr
    if name.startswith("pow2_"):
        k = int(name[5:])
        p, m = pow2_h(pts, Hgt, k)
        return p, m, float(np.float32(2.0) * np.float32(2.0) ** np.float32(k))
    return _box_rows(pts, _h_live_row(pts, Hgt), H_FAR)[name], transform_h(Hgt, IDENT, IDENT), 2.0


# ------------------------------------------------------------------------------------ two-view table
# name: (A1, A2, thr factor) per coordinate kind; thr follows the transform's largest scale
TV_AFFINE = {
    True: {  # normalised coordinates, thr 0.002
        "base": (IDENT, IDENT, 1.0),
        "offset": ((1, 1, 3, -2), (1, 1, -5, 1), 1.0),
    },
    False: {  # pixel coordinates, thr 1
        "base": (IDENT, IDENT, 1.0),
        "offset": ((1, 1, 2000, -3000), (1, 1, -5000, 1000), 1.0),
    },
}
for _k in (True, False):
    TV_AFFINE[_k]["narrow"] = ((1e-2, 1e-2, 0, 0), (1e-2, 1e-2, 0, 0), 1e-2)
    TV_AFFINE[_k]["wide"] = ((40, 40, 0, 0), (40, 40, 0, 0), 40.0)
    TV_AFFINE[_k]["aniso"] = ((8, 1 / 8, 0, 0), (1 / 8, 8, 0, 0), 8.0)
TV_THR = {True: 0.002, False: 1.0}
TV_FAR = {True: {"far": (300.0, -200.0, 100.0, 500.0)}, False: {"far": (3e6, -2e6, 1e6, 5e6)}}
TV_BOX = ("far", "x1_const", "identical", "all_nan", "nan_only", "inf_only")
TV_ROWS = ("base", "offset", "narrow", "wide", "aniso") + TV_BOX


def tv_base(normalized):
    pts, M, _ = synthetic.fundamental_points(n=1500, inlier_ratio=0.3, seed=4, normalized=normalized)
    return pts, M


def _tv_live_row(pts, M, thr):
    """the first row whose fp64 epipolar residual of the ground truth is well inside thr"""
    F = np.asarray(M, np.float64)
    p1 = np.c_[pts[:, :2].astype(np.float64), np.ones(len(pts))]
    p2 = np.c_[pts[:, 2:].astype(np.float64), np.ones(len(pts))]
    l2 = p1 @ F.T
    l1 = p2 @ F
    r = np.abs((p2 * l2).sum(1))
    d = 0.5 * (r / np.hypot(l2[:, 0], l2[:, 1]) + r / np.hypot(l1[:, 0], l1[:, 1]))
    return int(np.flatnonzero(d < 0.25 * thr)[0])


def tv_row(name, normalized):
    """-> (points N x 4 fp32, base model (9,) fp32, thr)"""
    pts, M = tv_base(normalized)
    thr = TV_THR[normalized]
    if name in TV_AFFINE[normalized]:
        A1, A2, f = TV_AFFINE[normalized][name]
        return transform(pts, A1, A2), transform_f(M, A1, A2), thr * f
    return _box_rows(pts, _tv_live_row(pts, M, thr), TV_FAR[normalized])[name], transform_f(M, IDENT, IDENT), thr


def thresholds_on_errors(errs, count=12):
    """`count` thresholds placed exactly on pair errors (spread over the sorted finite positive ones),
    each followed by the next float up."""
    e = np.sort(errs[np.isfinite(errs) & (errs > 0)])
    out = []
    for v in e[:: max(1, len(e) // count)][:count]:
        out += [float(v), float(np.nextafter(np.float32(v), np.float32(np.inf)))]
    return out
