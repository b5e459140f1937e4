"""Pose refinement of a multi context's essential batches (usac_multi_refine_pose_device / usac_multi_refine_pose,
ABI 29): the rule of include/usac_gpu.h "Pose refinement" restated in numpy.  Every value is an IEEE double and
every operation one correctly rounded fp64 operation in the order the header fixes, so the results can be compared
bit for bit with the kernel's.  The 3 x 3 algebra, the 5 x 5 solve and the pose update run on numpy float64 scalars;
the per-row expressions run the same scalar expression over all rows of a problem at once, elementwise (numpy's
multiply, add, divide and sqrt are separate correctly rounded operations, never fused).  The sums are spelt out:
thread tau of 256 adds its rows tau, tau + 256, ... in ascending order, the 64 lanes of a wave fold by halves
(offsets 32, 16, 8, 4, 2, 1) and the four wave totals combine as (w0 + w1) + (w2 + w3).  Nothing here calls into
anything compiled."""
import numpy as np

F = np.float64
USAC_OK = 0
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = F(1e-3), F(1e-12), F(1e8)
COST_TOL, STEP_TOL = F(1e-12), F(1e-10)
PAIRS = [(j, k) for j in range(5) for k in range(j, 5)]  # the upper triangle of H, row by row


def normalized(v):
    n = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return [v[0] / n, v[1] / n, v[2] / n]


def cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def skew_times(v, M):
    """[v]x M: column c is v x (column c of M)"""
    return [[v[1] * M[2][c] - v[2] * M[1][c] for c in range(3)],
            [v[2] * M[0][c] - v[0] * M[2][c] for c in range(3)],
            [v[0] * M[1][c] - v[1] * M[0][c] for c in range(3)]]


def unit_skew_times(j, M):
    """[e_j]x M, exactly: rows of M moved and negated"""
    z = [F(0), F(0), F(0)]
    if j == 0:
        return [z, [-M[2][c] for c in range(3)], [M[1][c] for c in range(3)]]
    if j == 1:
        return [[M[2][c] for c in range(3)], z, [-M[0][c] for c in range(3)]]
    return [[-M[1][c] for c in range(3)], [M[0][c] for c in range(3)], z]


def basis(t):
    """b1, b2: the tangent basis of the unit vector t"""
    k = 0
    for i in (1, 2):
        if np.abs(t[i]) < np.abs(t[k]):
            k = i
    c = ([F(0), t[2], -t[1]], [-t[2], F(0), t[0]], [t[1], -t[0], F(0)])[k]  # t x e_k
    b1 = normalized(c)
    return b1, cross(t, b1)


def frame(R, t):
    """E = [t]x R and the five derivative matrices at (R, t), with the basis they were built from"""
    b1, b2 = basis(t)
    E = skew_times(t, R)
    D = [skew_times(t, unit_skew_times(j, R)) for j in range(3)] + [skew_times(b1, R), skew_times(b2, R)]
    return E, D, b1, b2


def residuals(E, D, rows, used):
    """r (n,), J (5, n) and the rows that contribute (used, and S > 0), elementwise over the rows"""
    x1, y1, x2, y2 = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]

    def mv(M):  # M x1 (three rows) and the first two entries of M^T x2
        u = [(M[r][0] * x1 + M[r][1] * y1) + M[r][2] for r in range(3)]
        v = [(M[0][c] * x2 + M[1][c] * y2) + M[2][c] for c in range(2)]
        return u, v

    a, b = mv(E)
    C = (x2 * a[0] + y2 * a[1]) + a[2]
    S = ((a[0] * a[0] + a[1] * a[1]) + b[0] * b[0]) + b[1] * b[1]
    ok = used & (S > 0)
    s = np.sqrt(S)
    r = C / s
    J = []
    for j in range(5):
        u, v = mv(D[j])
        num = (x2 * u[0] + y2 * u[1]) + u[2]
        q = ((a[0] * u[0] + a[1] * u[1]) + b[0] * v[0]) + b[1] * v[1]
        J.append(num / s - (r * q) / S)
    return r, J, ok


def block_sum(v, ok):
    """the workgroup's sum of v over the rows with ok set: strided per-thread sums, the butterfly, the four waves"""
    n = len(v)
    strides = (n + 255) // 256
    vals = np.zeros(strides * 256, dtype=F)
    keep = np.zeros(strides * 256, dtype=bool)
    vals[:n], keep[:n] = v, ok
    acc = np.zeros(256, dtype=F)
    for s in range(strides):
        lo = 256 * s
        acc = np.where(keep[lo:lo + 256], acc + vals[lo:lo + 256], acc)
    w = []
    for wave in range(4):
        x = acc[64 * wave:64 * wave + 64]
        for half in (32, 16, 8, 4, 2, 1):
            x = x[:half] + x[half:]
        w.append(x[0])
    return (w[0] + w[1]) + (w[2] + w[3])


def one_pass(R, t, rows, used):
    """the 21 sums at (R, t): H (5 x 5, symmetric, from its upper triangle), g (5), c; and the frame"""
    with np.errstate(all="ignore"):
        E, D, b1, b2 = frame(R, t)
        r, J, ok = residuals(E, D, rows, used)
        H = [[F(0)] * 5 for _ in range(5)]
        for j, k in PAIRS:
            H[j][k] = H[k][j] = block_sum(J[j] * J[k], ok)
        g = [block_sum(J[j] * r, ok) for j in range(5)]
        c = block_sum(r * r, ok)
    return {"H": H, "g": g, "c": c, "E": E, "b1": b1, "b2": b2, "R": R, "t": t}


def solve(H, g, lam):
    """(H + lam diag H) delta = -g by Cholesky (lower triangle, columns in order); None: a pivot is not > 0"""
    with np.errstate(all="ignore"):
        A = [[H[i][j] for j in range(5)] for i in range(5)]
        for j in range(5):
            A[j][j] = H[j][j] + lam * H[j][j]
        L = [[F(0)] * 5 for _ in range(5)]
        for j in range(5):
            s = A[j][j]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            if not s > 0:
                return None
            L[j][j] = np.sqrt(s)
            for i in range(j + 1, 5):
                s = A[i][j]
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                L[i][j] = s / L[j][j]
        y = [F(0)] * 5
        for i in range(5):
            s = -g[i]
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s / L[i][i]
        d = [F(0)] * 5
        for i in (4, 3, 2, 1, 0):
            s = y[i]
            for k in range(i + 1, 5):
                s = s - L[k][i] * d[k]
            d[i] = s / L[i][i]
    return d


def update(R, t, b1, b2, d):
    """the trial pose: R' = Q(d0, d1, d2) R, t' = (t + d3 b1 + d4 b2) normalised"""
    with np.errstate(all="ignore"):
        qx, qy, qz = d[0] * F(0.5), d[1] * F(0.5), d[2] * F(0.5)
        inv = F(1) / np.sqrt(((F(1) + qx * qx) + qy * qy) + qz * qz)
        w, x, y, z = inv, qx * inv, qy * inv, qz * inv
        Q = [[F(1) - F(2) * (y * y + z * z), F(2) * (x * y - w * z), F(2) * (x * z + w * y)],
             [F(2) * (x * y + w * z), F(1) - F(2) * (x * x + z * z), F(2) * (y * z - w * x)],
             [F(2) * (x * z - w * y), F(2) * (y * z + w * x), F(1) - F(2) * (x * x + y * y)]]
        Rn = [[(Q[r][0] * R[0][c] + Q[r][1] * R[1][c]) + Q[r][2] * R[2][c] for c in range(3)] for r in range(3)]
        tn = normalized([(t[k] + d[3] * b1[k]) + d[4] * b2[k] for k in range(3)])
    return Rn, tn


def used_rows(rows, mask=None):
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    set_ = np.ones(len(rows), dtype=bool) if mask is None else np.asarray(mask).reshape(len(rows)) != 0
    return set_ & np.isfinite(rows).all(1)


def refine(R0, t0, rows, mask=None, max_iters=10, status=USAC_OK):
    """The rule for one problem.  R0: 9 fp32 values, t0: 3; rows: (n, 4) fp32 calibrated x1 y1 x2 y2; mask: n bytes
    or None (every row).  Returns a dict: R (3, 3) / t (3,) / E (3, 3) fp32, R64 / t64 the doubles before the cast,
    cost0 / cost float64, iterations, used, and what the outputs do not show: lambdas, the damping of every solve in
    order; pivots, the solves that a pivot rejected without a pass; stop, the test that ended the loop ("cost":
    c - c' <= 1e-12 c, "step": max |d_j| < 1e-10, "lambda": lambda > 1e8, "max_iters"; "skipped")."""
    R32 = np.asarray(R0, dtype=np.float32).reshape(3, 3)
    t32 = np.asarray(t0, dtype=np.float32).reshape(3)
    rows32 = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    used = used_rows(rows32, mask)
    n_used = int(used.sum())
    start_ok = bool(np.isfinite(R32).all() and np.isfinite(t32).all() and (t32 != 0).any())
    if status != USAC_OK or not start_ok or n_used < 5:
        return {"R": R32.copy(), "t": t32.copy(), "E": np.zeros((3, 3), np.float32), "R64": R32.astype(F),
                "t64": t32.astype(F), "cost0": F(0), "cost": F(0), "iterations": -1, "used": n_used, "lambdas": [], "pivots": 0,
                "stop": "skipped"}
    rows64 = rows32.astype(F)
    rows64[~used] = 0  # never read: a row that is not used contributes nothing
    R = [[F(R32[r, c]) for c in range(3)] for r in range(3)]
    t = normalized([F(v) for v in t32])
    cur = one_pass(R, t, rows64, used)
    cost0 = cur["c"]
    lam, iterations, lambdas, pivots, stop = LAMBDA0, 0, [], 0, "max_iters"
    while iterations < max_iters:
        lambdas.append(lam)
        d = solve(cur["H"], cur["g"], lam)
        accepted = False
        if d is not None:
            Rn, tn = update(cur["R"], cur["t"], cur["b1"], cur["b2"], d)
            new = one_pass(Rn, tn, rows64, used)
            iterations += 1
            accepted = bool(new["c"] < cur["c"])
        else:
            pivots += 1
        if accepted:
            old = cur["c"]
            cur = new
            lam = max(lam / F(10), LAMBDA_MIN)
            if old - cur["c"] <= COST_TOL * old:
                stop = "cost"
                break
            if max(np.abs(v) for v in d) < STEP_TOL:
                stop = "step"
                break
        else:
            lam = F(10) * lam
            if lam > LAMBDA_MAX:
                stop = "lambda"
                break
    R64, t64, E64 = np.array(cur["R"], dtype=F), np.array(cur["t"], dtype=F), np.array(cur["E"], dtype=F)
    return {"R": R64.astype(np.float32), "t": t64.astype(np.float32), "E": E64.astype(np.float32), "R64": R64,
            "t64": t64, "cost0": cost0, "cost": cur["c"], "iterations": iterations, "used": n_used, "lambdas": lambdas,
            "pivots": pivots, "stop": stop}


KEYS = ("R", "t", "E", "cost0", "cost", "iterations", "used")


def refine_batch(R, t, points, offsets, mask=None, max_iters=10, status=None):
    """The rule for every problem of a context: what MultiContext.refine returns (mask over the packed rows)"""
    o = np.asarray(offsets, dtype=np.int64)
    P = len(o) - 1
    R = np.asarray(R, dtype=np.float32).reshape(P, 9)
    t = np.asarray(t, dtype=np.float32).reshape(P, 3)
    out = {"R": np.zeros((P, 3, 3), np.float32), "t": np.zeros((P, 3), np.float32), "E": np.zeros((P, 3, 3), np.float32),
           "cost0": np.zeros(P, F), "cost": np.zeros(P, F), "iterations": np.zeros(P, np.int32),
           "used": np.zeros(P, np.int32)}
    for p in range(P):
        r = refine(R[p], t[p], points[o[p]:o[p + 1]], None if mask is None else np.asarray(mask)[o[p]:o[p + 1]],
                   max_iters, USAC_OK if status is None else int(status[p]))
        for key in KEYS:
            out[key][p] = r[key]
    return out
