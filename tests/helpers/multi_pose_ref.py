"""Pose of a multi context's essential matrices (usac_multi_pose_device / usac_multi_pose, ABI 28): the rule of
include/usac_gpu.h "Pose" restated in numpy.  Every value is an IEEE double and every operation one correctly
rounded fp64 operation, in the order of the oracle's row_jacobi_small, projections, triangulate and calc_depth
(oracle/usac_oracle.c) -- which is the order of e5::svd3, e5::projection and e5::in_front on the device -- so the
results can be compared bit for bit.  The decomposition runs on numpy float64 scalars (no exception on a division
by zero, NaN compares false); the cheirality test runs the same scalar expression over all rows of a problem at
once, elementwise: numpy's multiply, add, divide and sqrt are separate correctly rounded operations, never fused.
Nothing here calls into anything compiled."""
import numpy as np

F = np.float64
PAIRS = ((1, 2), (0, 2), (0, 1))  # the tournament order of three rows (tournament_pairs(3))
WM = ((F(0), F(-1), F(0)), (F(1), F(0), F(0)), (F(0), F(0), F(1)))
PREF = ((F(1), F(0), F(0), F(0)), (F(0), F(1), F(0), F(0)), (F(0), F(0), F(1), F(0)))
USAC_OK = 0


def _dot(a, b, n):
    s = F(0)
    for k in range(n):
        s = s + a[k] * b[k]
    return s


def jacobi3(B, J):
    """row_jacobi_small on three rows of three columns, J accumulates the rotations (both changed in place).  A
    comparison with a NaN rotates, as on the device (`!(g g <= eps a b)`)."""
    for _ in range(30):
        rotated = False
        nrm = [_dot(B[i], B[i], 3) for i in range(3)]
        for p, q in PAIRS:
            a, b = nrm[p], nrm[q]
            g = _dot(B[p], B[q], 3)
            if g * g <= F(1e-28) * (a * b):
                continue
            rotated = True
            d, g2 = b - a, F(2) * g
            t = g2 / (np.abs(d) + np.sqrt(d * d + g2 * g2))
            if d < 0:
                t = -t
            c = F(1) / np.sqrt(F(1) + t * t)
            s = c * t
            for M in (B, J):
                for k in range(3):
                    mp, mq = M[p][k], M[q][k]
                    M[p][k] = c * mp - s * mq
                    M[q][k] = s * mp + c * mq
            nrm[p] = a - t * g
            nrm[q] = b + t * g
        if not rotated:
            break


def svd3(E):
    """U, V (columns) of E (9 doubles): projections() up to the cross product"""
    B = [[F(E[3 * i + k]) for k in range(3)] for i in range(3)]
    J = [[F(1) if i == k else F(0) for k in range(3)] for i in range(3)]
    jacobi3(B, J)
    sg = [np.sqrt(_dot(B[i], B[i], 3)) for i in range(3)]
    o = [0, 1, 2]
    for i in range(3):
        for j in range(i + 1, 3):
            if sg[o[j]] > sg[o[i]]:
                o[i], o[j] = o[j], o[i]
    U = [[J[o[k]][r] for k in range(3)] for r in range(3)]
    V = [[B[o[k]][r] / sg[o[k]] if k < 2 else F(0) for k in range(3)] for r in range(3)]
    V[0][2] = V[1][0] * V[2][1] - V[2][0] * V[1][1]
    V[1][2] = V[2][0] * V[0][1] - V[0][0] * V[2][1]
    V[2][2] = V[0][0] * V[1][1] - V[1][0] * V[0][1]
    return U, V


def projection(U, V, j):
    """P_j = [R | t] as 3 rows of 4 doubles: R = U W V^T (j = 0, 1) or U W^T V^T (j = 2, 3), t = +u3 / -u3"""
    w, sgn = j >> 1, j & 1
    T = [[_dot(U[r], [WM[k][c] if w == 0 else WM[c][k] for k in range(3)], 3) for c in range(3)] for r in range(3)]
    P = []
    for r in range(3):
        row = [_dot(T[r], V[c], 3) for c in range(3)]
        row.append(U[r][2] if sgn == 0 else -U[r][2])
        P.append(row)
    return P


def projections(E):
    """the four P_j of E: 9 values in any shape, widened to float64"""
    E = np.asarray(E, dtype=F).reshape(9)
    with np.errstate(all="ignore"):
        U, V = svd3(E)
        return [projection(U, V, j) for j in range(4)]


def det3(P):
    return (P[0][0] * (P[1][1] * P[2][2] - P[1][2] * P[2][1]) - P[0][1] * (P[1][0] * P[2][2] - P[1][2] * P[2][0]) +
            P[0][2] * (P[1][0] * P[2][1] - P[1][1] * P[2][0]))


def calc_depth(X, P):
    """CalcDepth; X: four arrays (or scalars)"""
    w = F(0)
    for k in range(4):
        w = w + P[2][k] * X[k]
    det = det3(P)
    a, b, c = P[0][2], P[1][2], P[2][2]
    m3 = np.sqrt(a * a + b * b + c * c)
    sign = F(1) if det > 0 else F(-1)
    return (w / X[3]) * (sign / m3)


def in_front(x1, y1, x2, y2, P):
    """triangulate() + the two CalcDepth tests, elementwise over float64 arrays x1, y1, x2, y2 -> bool array"""
    x1, y1, x2, y2 = (np.asarray(v, dtype=F) for v in (x1, y1, x2, y2))
    with np.errstate(all="ignore"):
        b = []
        for r, u in ((0, x2), (1, y2)):
            row = [u * P[2][c] - P[r][c] for c in range(4)]
            b.append((row[0] * x1 + row[1] * y1 + row[2], row[3]))
        n0 = b[0][0] * b[0][0] + b[0][1] * b[0][1]
        n1 = b[1][0] * b[1][0] + b[1][1] * b[1][1]
        first = n0 >= n1
        sc = np.where(first, b[0][1], b[1][1])
        w = np.where(first, -b[0][0], -b[1][0])
        X = (x1 * sc, y1 * sc, sc, w)
        return (calc_depth(X, PREF) > 0) & (calc_depth(X, P) > 0)


def pose(E, rows, mask=None, status=USAC_OK):
    """The rule for one problem.  E: 9 fp32 values; rows: (n, 4) fp32 calibrated x1 y1 x2 y2; mask: n bytes or None
    (every row).  Returns a dict: R (3, 3) / t (3,) fp32, R64 / t64 the doubles before the cast, front, choice,
    front_mask (n,) uint8 and counts (4,), the rows in front per candidate."""
    E = np.asarray(E, dtype=np.float32).reshape(9).astype(F)
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4).astype(F)
    n = len(rows)
    set_ = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).reshape(n) != 0
    # a row with a non-finite value is in front of nothing.  in_front alone does not say so: a non-finite x2 beside
    # a finite y2 makes n0 NaN, `n0 >= n1` false, and the point is triangulated from y2's row
    set_ = set_ & np.isfinite(rows).all(1)
    Ps = projections(E)
    fronts = [in_front(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], P) & set_ for P in Ps]
    counts = np.array([int(f.sum()) for f in fronts], dtype=np.int64)
    choice = -1
    if status == USAC_OK and counts.max(initial=0) > 0:
        choice = int(np.argmax(counts))  # the first of the largest
    if choice < 0:
        R64, t64 = np.eye(3), np.zeros(3)
        front_mask = np.zeros(n, dtype=np.uint8)
    else:
        P = np.array(Ps[choice], dtype=F)
        if not det3(Ps[choice]) > 0:  # -P is the same camera: the one of the two whose block is a rotation
            P = F(-1) * P
        R64, t64 = P[:, :3].copy(), P[:, 3].copy()
        front_mask = fronts[choice].astype(np.uint8)
    return {"R": R64.astype(np.float32), "t": t64.astype(np.float32), "R64": R64, "t64": t64,
            "front": int(counts[choice]) if choice >= 0 else 0, "choice": choice, "front_mask": front_mask,
            "counts": counts}


def pose_batch(models, points, offsets, mask=None, status=None):
    """The rule for every problem of a context: what MultiContext.pose returns (front_mask in packed-row order)"""
    o = np.asarray(offsets, dtype=np.int64)
    P = len(o) - 1
    models = np.asarray(models, dtype=np.float32).reshape(P, 9)
    out = {"R": np.zeros((P, 3, 3), np.float32), "t": np.zeros((P, 3), np.float32), "front": np.zeros(P, np.int32),
           "choice": np.zeros(P, np.int32), "front_mask": np.zeros(int(o[-1]), np.uint8)}
    for p in range(P):
        r = pose(models[p], points[o[p]:o[p + 1]], None if mask is None else np.asarray(mask)[o[p]:o[p + 1]],
                 USAC_OK if status is None else int(status[p]))
        out["R"][p], out["t"][p], out["front"][p], out["choice"][p] = r["R"], r["t"], r["front"], r["choice"]
        out["front_mask"][o[p]:o[p + 1]] = r["front_mask"]
    return out
