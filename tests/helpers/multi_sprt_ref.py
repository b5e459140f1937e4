"""The yardstick of the multi-problem SPRT tests (usac_multi_run_sprt, ABI 19): the per-round update rule
of include/usac_gpu.h (usac_multi_sprt_update) restated in Python over the C library's libm, the tests'
point sets, and the round's statistics restated over the CPU oracle's walk.  Everything here runs on the
CPU."""
import ctypes
import math

import numpy as np

from ransac_amd import synthetic

THR = 2.0
M = {"H": 4, "F": 7}
EST_ID = {"H": 2, "F": 3}
# sprt.hpp:114-170: epsilon_0, delta_0, t_M, m_S
DEFAULTS = {"H": (0.1, 0.01, 200.0, 1.0), "F": (0.2, 0.05, 200.0, 2.48)}
HEAD = 64


# ---- libm as C++ sees it: math.* is the platform's libm, with C's answers where Python raises
def _log(x):
    if x != x or x < 0:
        return math.nan
    if x == 0:
        return -math.inf
    return math.log(x)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _pow(a, b):
    try:
        return math.pow(a, b)
    except OverflowError:
        return math.inf
    except ValueError:
        return math.nan


def _div(a, b):
    if b == 0:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def threshold_A(kind, epsilon, delta):
    """estimateThresholdA (sprt.hpp:332-355)"""
    _, _, t_M, m_S = DEFAULTS[kind]
    C = (1 - delta) * _log(_div(1 - delta, 1 - epsilon)) + delta * _log(_div(delta, epsilon))
    K = (t_M * C) / m_S + 1
    prev = An = K
    for _ in range(10):
        An = K + _log(prev)
        if abs(An - prev) < 1.5e-8:
            break
        prev = An
    return An


def exponent_h(epsilon, epsilon_new, delta):
    """computeExponentH (sprt.hpp:442-491)"""
    a = _log(_div(delta, epsilon))
    b = _log(_div(1 - delta, 1 - epsilon))
    x0 = _div(_log(_div(1, 1 - epsilon_new)), b)
    v0 = epsilon_new * _exp(x0 * a)
    x1 = _div(_log(_div(1 - 2 * v0, 1 - epsilon_new)), b)
    v1 = epsilon_new * _exp(x1 * a) + (1 - epsilon_new) * _exp(x1 * b)
    h = x0 - _div(x0 - x1, 1 + v0 - v1) * v0
    return 0.0 if h != h else h


class RefState:
    """One problem's SPRT state: history [epsilon, delta, A, k], last_update, bound.  `taken` collects the
    branches the updates went through."""

    def __init__(self, kind, n, max_iterations):
        self.kind, self.n, self.m, self.max_iterations = kind, n, M[kind], max_iterations
        e0, d0, _, _ = DEFAULTS[kind]
        self.history = [(e0, d0, threshold_A(kind, e0, d0), 0)]
        self.last_update = 0
        self.bound = max_iterations
        self.taken = set()

    @property
    def test(self):
        return self.history[-1][:3]

    def upper_bound(self, inliers):
        """getUpperBoundIterations (sprt.hpp:371-393)"""
        epsilon = inliers / self.n
        P_g = _pow(epsilon, self.m)
        log_eta = 0.0
        for e, d, A, k in self.history[:-1]:
            h = exponent_h(e, epsilon, d)
            log_eta += _log(1 - P_g * (1 - _pow(A, -h))) * k
        num = _log(0.05) - log_eta
        if num >= 0:
            self.taken.add("numerator>=0")
            return 0
        den = _log(1 - P_g * (1 - _div(1, self.history[-1][2])))
        if den != den or abs(den) < 0.00001:
            self.taken.add("denominator")
            return self.max_iterations
        return min(int(num / den), self.max_iterations)

    def update(self, done, head_inliers, head_points, improved, best_inliers=0, term_bound=0):
        epsilon, delta, _ = self.test
        eps_new, delta_new, new_delta = epsilon, delta, False
        if head_points > 0:
            dest = float(np.float32(head_inliers) / np.float32(head_points))
            new_delta = dest > 0 and abs(delta - dest) / delta > 0.05
            if new_delta:
                delta_new = dest
        else:
            self.taken.add("no_head_points")
        if improved:
            eps_new = float(np.float32(best_inliers) / np.float32(self.n))
        designed = False
        if improved or new_delta:
            if 0 < delta_new < eps_new < 1:
                self.history.append((eps_new, delta_new, threshold_A(self.kind, eps_new, delta_new), done - self.last_update))
                self.last_update = done
                designed = True
                self.taken.add(("both" if improved else "delta") if new_delta else "epsilon")
            else:
                self.taken.add("guard")
        else:
            self.taken.add("neither")
        if improved:
            self.bound = min(term_bound, self.upper_bound(best_inliers))
        return designed


def bits64(x):
    return np.array(x, dtype=np.float64).view(np.int64).tolist()


def assert_same_state(got, want, what=""):
    """got: a ransac_amd.MultiSprtState, want: a RefState -- without tolerance"""
    g, w = got.history, want.history
    assert len(g) == len(w), (what, g, w)
    for a, b in zip(g, w):
        assert bits64(a[:3]) == bits64(b[:3]) and a[3] == b[3], (what, a, b)
    assert (got.last_update, got.bound) == (want.last_update, want.bound), (what, got.bound, want.bound)


# ---- the GPU tests' problems
SIZES = {"H": [4, 21, 64, 65, 321, 1000], "F": [7, 21, 64, 65, 321, 1000]}
RATIOS = [0.9, 0.9, 0.3, 0.3, 0.0, 0.3]           # tests/test_gpu_multi_prosac.py's, 0.9 for the m-point set
DATA_SEEDS = {"H": [70, 71, 72, 73, 74, 75], "F": [80, 81, 82, 83, 84, 85]}
DUP = (6, 3)                                      # problem 6 is a copy of problem 3 (the 65-point set)
POOL_SEEDS = [11, 12, 13, 14, 15, 16, 14]         # the copy shares its original's pool
# a test per problem: the defaults, and others on both sides of them
EPS_DELTA = {"H": [(0, 0), (0.5, 0.02), (0.2, 0.01), (0.1, 0.03), (0.15, 0.012), (0.3, 0.008), (0.1, 0.03)],
             "F": [(0, 0), (0.5, 0.1), (0.25, 0.05), (0.2, 0.08), (0.3, 0.04), (0.3, 0.06), (0.2, 0.08)]}


def sets(kind, sort=False, with_m=True):
    """-> (point sets, inlier masks); sort: by descending quality (the PROSAC runs); with_m: the m-point set"""
    pts, inl = [], []
    for n, ratio, seed in zip(SIZES[kind], RATIOS, DATA_SEEDS[kind]):
        if n == M[kind] and not with_m:
            continue
        if kind == "H":
            p, _, i = synthetic.homography_points(n=n, inlier_ratio=ratio, seed=seed)
            if sort:
                p, i = synthetic.quality_sort(p, i, seed + 1000)
        else:
            p, _, i = synthetic.fundamental_points(n=n, inlier_ratio=ratio, seed=seed, prosac_order=sort)
        pts.append(np.ascontiguousarray(p, dtype=np.float32))
        inl.append(np.asarray(i, dtype=bool))
    d = DUP[1] - (0 if with_m else 1)
    pts.append(pts[d].copy())
    inl.append(inl[d].copy())
    return pts, inl


def inlier_samples(oracle, kind, pts, inl, count, rng, tries=48):
    """`count` minimal samples of known inliers whose models explain the set best (of `tries` random ones, by
    the oracle's count): models that survive the SPRT's head and pass its tail.  None without enough inliers."""
    good = np.flatnonzero(inl)
    m = M[kind]
    if len(good) < m:
        return None
    cand = np.stack([rng.choice(good, size=m, replace=False) for _ in range(tries)]).astype(np.int32)
    est = oracle.Estimator(oracle_kind(oracle, kind), pts)
    models, nm = est.estimate_batch(cand)
    c, _ = est.score_models(np.asarray(models, np.float32).reshape(-1, 9), THR)
    c = c.reshape(tries, -1)
    if kind == "F":
        c = np.where(np.arange(3)[None, :] < nm[:, None], c, -1)
    order = np.argsort(-c.max(axis=1), kind="stable")
    return cand[order[:count]]


def design(kind, e, d):
    """(epsilon, delta, A) of an eps_delta entry (a 0: the estimator's default)"""
    e = e if e else DEFAULTS[kind][0]
    d = d if d else DEFAULTS[kind][1]
    return e, d, threshold_A(kind, e, d)


def oracle_kind(oracle, kind):
    return oracle.HOMOGRAPHY if kind == "H" else oracle.FUNDAMENTAL


def walk(oracle, est, pool, models, starts, test, thr=THR):
    """the reference's walk of every model from its start -> (good, count [-1: rejected], tested, inliers
    seen up to the rejecting point [0 for an accepted model])"""
    good, cnt, tested = oracle.sprt_fixed_batch(est, pool, thr, models, starts, *test)
    L = oracle.lib()
    L.orc_est_error.restype = ctypes.c_float
    L.orc_est_error.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    L.orc_est_set_model.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    n = len(pool)
    seen = np.zeros(len(good), dtype=np.int64)
    models = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 9)
    for k in np.flatnonzero(~good):
        if tested[k] > HEAD:
            continue  # (only the head's rejections are summed)
        L.orc_est_set_model(est._h, models[k].ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        seen[k] = sum(1 for t in range(int(tested[k])) if L.orc_est_error(est._h, int(pool[(int(starts[k]) + t) % n])) < thr)
    return good, cnt, tested, seen


def round_stats(good, tested, seen, n):
    """the device's per-entry statistics from the walk (a rejection is the head's when it falls within the
    first min(n, 64) points)"""
    head = min(n, HEAD)
    rej_head = (~good) & (tested <= head)
    return {"accepted": int(good.sum()), "rejected": int((~good).sum()), "rejected_head": int(rej_head.sum()),
            "head_inliers": int(seen[rej_head].sum()), "head_points": int(tested[rej_head].sum())}
