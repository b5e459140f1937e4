"""Degenerate inputs for the solvers' parity tests (numpy only; every array returned is read-only).

The scorers have tests/helpers/geometry.py; this is the same for the code that produces the models: the
4-point DLT, the 7-point and 5-point minimal solvers, and the non-minimal fits behind every polish and
LO pass (normalised DLT, 8-point algorithm, the weighted overloads).  Three families:

  geometry rows   geometry.H_ROWS / TV_ROWS (F: pixel rows, E: calibrated rows) with 256 samples of the
                  oracle's UniformSampler over the row's own size;
  sample tables   256 samples each over a 600-point set per estimator: (i) repeated indices, (ii)
                  changed point sets, (iii) power-of-ten scales, (iv) non-finite rows;
  fit tables      index lists of 100 and 300 (either side of the one-workgroup fit of <= 256 points) on
                  the point sets of (ii)-(iv) and degenerate lists on the clean set, one list of 4100
                  (five superblocks of the normal-matrix sum), and weight vectors for the weighted fits.

Which branches they reach is asserted from the CPU oracle's path counters by
tests/test_solver_cases_cpu.py; tests/test_gpu_solver_cases.py compares the device with the oracle on
all of them, bit for bit.

`oracle` arguments are the oracle.oracle module (the sampler stream comes from it)."""
import functools

import numpy as np

from ransac_amd import synthetic
from tests.helpers import geometry as G

KINDS = ("H", "F", "E")
M = {"H": 4, "F": 7, "E": 5}
THR = {"H": 2.0, "F": 2.0, "E": 0.002}
NS = 256      # samples per row / table
N_SET = 600   # points of a table's set, half of them inliers
SCALES = {"H": ("1e-30", "1e-20", "1e-10", "1e10", "1e18", "1e30"),
          "F": ("1e-30", "1e-20", "1e-10", "1e10", "1e18", "1e30"),
          "E": ("1e-30", "1e-10", "1e3", "1e10", "1e30")}
FIT_SIZES = (100, 300)
N_SUPER = 4100
FALLBACK_TABLES = ("rep_one", "rep_m3", "all_equal")  # (i): the tables that exist for the null-space fall-back


def _ro(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.flags.writeable = False
    return a


def unit(kind):
    """one pixel in the set's coordinates: calibrated rows are pixels / 1000 (synthetic's K)"""
    return 1e-3 if kind == "E" else 1.0


# ------------------------------------------------------------------------------------ base sets
@functools.lru_cache(maxsize=None)
def base(kind):
    """-> (points 600 x 4, ground-truth model (9,), inlier indices (300,), outlier indices (300,))"""
    if kind == "H":
        pts, model, inl = synthetic.homography_points(n=N_SET, inlier_ratio=0.5, seed=3)
    else:
        pts, model, inl = synthetic.fundamental_points(n=N_SET, inlier_ratio=0.5, seed=3, prosac_order=False,
                                                       normalized=kind == "E")
    return (_ro(pts, np.float32), _ro(model.reshape(9), np.float32), _ro(np.flatnonzero(inl), np.int32),
            _ro(np.flatnonzero(~inl), np.int32))


@functools.lru_cache(maxsize=None)
def planar(kind):
    """a planar scene for the two-view solvers: synthetic.homography_points, all inliers -> (points, F)
    with F = [e]x H, e = (1, 0, 0): one of the fundamental matrices a plane leaves free"""
    pts, H, _ = synthetic.homography_points(n=N_SET, inlier_ratio=1.0, seed=3)
    p = pts.astype(np.float64)
    Hd = np.asarray(H, np.float64).reshape(3, 3)
    if kind == "E":  # calibrated rows of synthetic's camera
        K = synthetic.two_view_geometry()[0]
        p = (p - 500.0) / 1000.0
        Hd = np.linalg.inv(K) @ Hd @ K
    F = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) @ Hd
    return _ro(p, np.float32), _ro((F / np.abs(F).max()).reshape(9), np.float32)


def _scaled(pts, s):
    with np.errstate(over="ignore", under="ignore"):
        return _ro(pts.astype(np.float64) * float(s), np.float32)


def spoiled_rows(kind):
    """the fifth of the inlier rows that nan_rows / inf_rows spoil, and each one's column"""
    inl = base(kind)[2]
    rows = inl[::5]
    return rows, np.arange(len(rows)) % 4


@functools.lru_cache(maxsize=None)
def changed_sets(kind):
    """name -> points: the sets of (ii), (iii) and (iv), all with the base set's row order (its inlier
    indices name the same rows; `planar` and `zeros` have no outliers)"""
    pts = base(kind)[0]
    u = unit(kind)
    p64 = pts.astype(np.float64)
    out = {}

    def put(name, a):
        out[name] = _ro(a, np.float32)

    a = p64.copy()
    a[:, 2:] = a[:, :2]
    put("same_view", a)
    a[:, 2] += 30 * u
    a[:, 3] -= 20 * u
    put("shifted", a)
    a = p64.copy()
    a[:, 1] = 0.5 * a[:, 0] + 100 * u
    put("line1", a)
    a[:, 3] = -0.25 * a[:, 2] + 700 * u
    put("lines", a)
    a = p64.copy()
    a[:, 0] = a[0, 0]
    put("const_coord", a)
    if kind != "H":
        put("planar", planar(kind)[0])
    put("lattice", np.round(p64 / (64 * u)) * (64 * u))
    put("zeros", np.zeros_like(p64))
    for s in SCALES[kind]:
        out["scale_" + s] = _scaled(pts, s)
    rows, cols = spoiled_rows(kind)
    for name, v in (("nan_rows", np.nan), ("inf_rows", np.inf)):
        a = pts.copy()
        a[rows, cols] = v
        put(name, a)
    return out


# ------------------------------------------------------------------------------------ samples
def geometry_row(oracle, kind, name):
    """-> (points, base model, thr, samples 256 x m): a geometry row and the UniformSampler's samples over
    its own size (identical: 40 points, all_nan: 33, x1_const: 200).  Seed 111: random 5-point samples of
    the calibrated row "wide" pass cheirality on about one sample in twenty (8 .. 18 of 256 over the seeds
    100 .. 111), and tests/test_solver_cases_cpu.py asks every live row for 16 samples with a model."""
    pts, model, thr = G.h_row(name) if kind == "H" else G.tv_row(name, kind == "E")
    samples = oracle.uniform_samples(111, len(pts), M[kind], NS)
    return _ro(pts), _ro(model), thr, _ro(samples)


GEOMETRY_ROWS = {"H": G.H_ROWS, "F": G.TV_ROWS, "E": G.TV_ROWS}
# rows that are empty on purpose: no sample of theirs gives the two-view solvers a model (H's DLT always
# returns its one model, finite or not)
GEOMETRY_EMPTY = ("all_nan",)


def inlier_samples(oracle, kind, seed=6):
    """256 samples of m distinct inlier rows of the base set (the UniformSampler's stream over the 300
    inliers, mapped to their rows).  Seed 6: of the seeds 1..12 the one whose F samples store F[8] = 0 most
    often at scale 1e-10 (42 of 256; the seeds give 28..42 and tests/test_solver_cases_cpu.py asks for 32)."""
    inl = base(kind)[2]
    return inl[oracle.uniform_samples(seed, len(inl), M[kind], NS)]


def sample_table_names(kind):
    return ("rep_one", "rep_m3", "all_equal", "reverse") + tuple(changed_sets(kind))


def sample_table(oracle, kind, name):
    """-> (points, samples 256 x m).  (i) on the base set: rep_one = the first index twice, rep_m3 = the
    first index in the first m - 3 places (H: m - 3 = 1, the plain sample), all_equal, reverse = 128
    samples each followed by its reverse; every other name is a set of changed_sets with the inlier
    samples."""
    m = M[kind]
    s = inlier_samples(oracle, kind).copy()
    if name == "rep_one":
        s[:, 1] = s[:, 0]
    elif name == "rep_m3":
        s[:, : m - 3] = s[:, :1]
    elif name == "all_equal":
        s[:, :] = s[:, :1]
    elif name == "reverse":
        s[1::2] = s[0::2, ::-1]
    else:
        return changed_sets(kind)[name], _ro(s, np.int32)
    return base(kind)[0], _ro(s, np.int32)


# ------------------------------------------------------------------------------------ fits
def _lists_on_clean(kind, n):
    _, _, inl, outl = base(kind)
    return {
        "one_point": np.repeat(inl[:1], n),
        "two_points": np.resize(inl[:2], n),
        "four_points": np.resize(inl[:4], n),
        "eight_points": np.resize(inl[:8], n),
        "inliers": inl[:n],
        "outliers": outl[:n],
        "first_rows": np.arange(n, dtype=np.int32),  # contaminated: half of the rows are outliers
    }


@functools.lru_cache(maxsize=None)
def fit_cases(kind):
    """[(name, points, index list)]: E's fit is the 8-point algorithm on its calibrated rows"""
    pts, _, inl, _ = base(kind)
    cases = []
    for n in FIT_SIZES:
        for name, p in changed_sets(kind).items():
            cases.append(("%s_%d" % (name, n), p, inl[:n]))
        for name, idx in _lists_on_clean(kind, n).items():
            cases.append(("%s_%d" % (name, n), pts, idx))
    cases.append(("three", pts, inl[:3]))
    cases.append(("minimal", pts, inl[: M[kind]]))
    cases.append(("super_%d" % N_SUPER, pts, np.resize(inl, N_SUPER)))
    return [(name, p, _ro(idx, np.int32)) for name, p, idx in cases]


@functools.lru_cache(maxsize=None)
def weight_cases(kind):
    """[(name, points, index list, weights (600,))] for lsq_fit / nonminimal_weighted (H and F)"""
    pts, _, inl, _ = base(kind)
    rng = np.random.default_rng(5)
    cases = []
    for n in FIT_SIZES:
        idx = inl[:n]
        w = {"zero": np.zeros(N_SET), "three": np.zeros(N_SET), "all_1e30": np.full(N_SET, 1e30),
             "denormal": np.full(N_SET, np.float32(1.4e-45))}
        w["three"][idx[[0, n // 2, n - 1]]] = (1.0, 0.5, 2.0)
        for name in ("one_nan", "one_negative", "half_negative"):
            w[name] = rng.uniform(0.5, 1.5, N_SET)
        w["one_nan"][idx[5]] = np.nan
        w["one_negative"][idx[5]] *= -1
        w["half_negative"][idx[::2]] *= -1
        for name, v in w.items():
            cases.append(("%s_%d" % (name, n), pts, _ro(idx, np.int32), _ro(v, np.float32)))
    return cases


# ------------------------------------------------------------------------------------ comparison
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_floats(got, want, what=""):
    """Exact equality of two fp32 arrays: the same bit pattern everywhere (so -0 is not +0), except that
    where `want` holds a NaN `got` must hold a NaN too, of any payload and sign (x86 and the GPU produce
    different default NaNs)."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~wn & (bits(got) != bits(want)))
    if bad.any():
        where = np.argwhere(bad)
        first = tuple(where[0])
        raise AssertionError("%s: %d of %d floats differ, first at %s: got %r (0x%08x), want %r (0x%08x)" % (
            what, len(where), bad.size, first, got[first], bits(got)[first], want[first], bits(want)[first]))


# ------------------------------------------------------------------------------------ polish
IDENTITY = _ro(np.eye(3).reshape(9), np.float32)
SKEW_X = _ro([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)  # [e_x]x: x^T F x = 0 for every x


@functools.lru_cache(maxsize=None)
def polish_cases(kind):
    """[(name, points, start model)] for the multi-problem polish (H, F; thr 2): six degenerate sets whose
    fit runs inside the polish.  Start models: the set's ground truth where it has one -- the identity /
    any skew matrix for same_view, the translation / [t]x for shifted, [e]x H for the planar scene, the
    base model for nan_rows (H) and the repeated points (H) -- otherwise the identity (H) or [e_x]x (F);
    at scale 1e-10 and 1e-20 every finite model keeps every row."""
    pts, gt, inl, _ = base(kind)
    sets = changed_sets(kind)
    if kind == "H":
        cases = [("same_view", sets["same_view"], IDENTITY),
                 ("shifted", sets["shifted"], [1, 0, 30, 0, 1, -20, 0, 0, 1]),
                 ("scale_1e-20", sets["scale_1e-20"], IDENTITY),
                 ("scale_1e-10", sets["scale_1e-10"], IDENTITY),
                 ("four_points", np.resize(pts[inl[:4]], (60, 4)), gt),
                 ("nan_rows", sets["nan_rows"], gt)]
    else:
        cases = [("same_view", sets["same_view"], SKEW_X),
                 ("shifted", sets["shifted"], [0, 0, -20, 0, 0, -30, 20, 30, 0]),
                 ("planar", sets["planar"], planar(kind)[1]),
                 ("scale_1e-10", sets["scale_1e-10"], SKEW_X),
                 ("one_point", np.repeat(pts[inl[:1]], 50, axis=0), SKEW_X),
                 ("nan_rows", sets["nan_rows"], SKEW_X)]
    return [(name, _ro(p, np.float32), _ro(m, np.float32)) for name, p, m in cases]


# ------------------------------------------------------------------------------------ expectations
def okind(oracle, kind):
    return {"H": oracle.HOMOGRAPHY, "F": oracle.FUNDAMENTAL, "E": oracle.ESSENTIAL}[kind]


def assert_same_models(kind, got, got_nm, want, want_nm, what=""):
    """estimate_models against estimate_batch: the model count of every sample, and every float of every
    slot -- H: one model per sample; F: three slots per sample, the valid models first and zeros behind
    them on both sides; E: one slot per sample, defined on both sides only where the sample has a model."""
    np.testing.assert_array_equal(got_nm, want_nm, err_msg="%s: models per sample" % (what,))
    if kind == "E":
        keep = np.asarray(want_nm) == 1
        assert_same_floats(np.asarray(got)[keep], np.asarray(want)[keep], what)
    else:
        assert_same_floats(got, want, what)


def round_expectation(oracle, kind, pts, samples, thr, dlt_mode=0):
    """What a round over `samples` must return, from the oracle alone: per slot (spk per sample: 3 for F)
    the count (-1 on an empty slot), the sequential sum (0 on an empty slot) and the model, and `best`, the
    first slot under (count, sum, earlier slot) among the occupied ones (None without one)."""
    est = oracle.Estimator(okind(oracle, kind), pts, dlt_mode)
    models, nm = est.estimate_batch(samples)
    spk = 3 if kind == "F" else 1
    models = np.ascontiguousarray(models.reshape(len(samples) * spk, 9))
    occupied = (np.arange(spk)[None, :] < nm[:, None]).reshape(-1)
    counts = np.full(len(models), -1, np.int32)
    sums = np.zeros(len(models), np.float32)
    if occupied.any():
        counts[occupied], sums[occupied] = est.score_models(models[occupied], thr)
    slots = np.flatnonzero(occupied)
    best = min(slots, key=lambda i: (-int(counts[i]), -float(sums[i]), i)) if len(slots) else None
    return {"counts": counts, "sums": sums, "models": models, "occupied": occupied, "best": best, "spk": spk}


def assert_same_round(counts, sums, best, want, what=""):
    """a round's per-slot counts, sums and best record against round_expectation's"""
    np.testing.assert_array_equal(counts, want["counts"], err_msg="%s: counts" % (what,))
    assert_same_floats(sums, want["sums"], "%s: sums" % (what,))
    if want["best"] is None:
        assert not best["valid"], what
        return
    b = want["best"]
    assert best["valid"], what
    assert best["hyp_index"] == b // want["spk"], (what, best["hyp_index"], b)
    assert best["inliers"] == want["counts"][b], (what, best["inliers"], want["counts"][b])
    assert_same_floats(np.float32(best["score"]).reshape(1), want["sums"][b: b + 1], "%s: best score" % (what,))
    assert_same_floats(best["model"], want["models"][b], "%s: best model" % (what,))


def fit_expectation(oracle, kind, pts, idx, weights=None, est=None):
    """the oracle's non-minimal fit (None: no model)"""
    est = est or oracle.Estimator(okind(oracle, kind), pts)
    return est.nonminimal(idx) if weights is None else est.nonminimal_weighted(idx, weights)


def assert_same_fit(got, want, what=""):
    """got: the device's model, or the UsacError code it raised"""
    if want is None:
        assert isinstance(got, int) and got == -111, (what, got)
    else:
        assert not isinstance(got, int), (what, "raised", got)
        assert_same_floats(got, want, what)
