"""Keep-mask statistics of the matrix-core homography scorer (kernels_h16.hip k_score_h16) on the
CPU: how many (hypothesis, point) pairs the fp16 tile keeps, and how they fall into the kernel's
ballot masks -- the figures that size the kept-pair append and the drains.

numpy only, no GPU.  Points: synthetic.homography_points (cfg2: 10 000 points, 30 % inliers).
Hypotheses: 4-point DLT models of random minimal samples (fp64 null vector, rounded to fp32), or with
--models a batch as the library solved it (B x 9 float32: Context.estimate_models of
Context.draw_samples) -- the two differ: the fp64 models pass through their sample points, the library's
fp32 thin-DLT models of ill-conditioned samples do not, and keep about 2.4x fewer pairs.
The statistics are printed for three slacks: the 2^-10 fp16 roundings the bound charged before, the
round-to-nearest constants of h16_rows_of (USAC_H16_ROW_ROUND, USAC_H16_FEAT_ROUND), and F_m = 0.
Rows and slack: a float32 mirror of usac_h16.hpp h16_rows_of / usac_hscore.hpp stage_a_bounds and
of k_h16_consts / k_h16_points (the same expressions in the same order; the exact slack, not an
approximation of it).  The tile: the fp16 rows times the fp16 features summed in fp64 and rounded
to fp32 (the MFMA accumulates in fp32: a different rounding of the last bit of a few sums), the
keep test |ex| <= R and |ey| <= R, R = |zr| + F in fp32 as the kernel writes it.

Layout: a wave owns 20 consecutive hypotheses and one point chunk; one iteration = one 32-point
block; one mask = 64 lanes = hypotheses (10 a + j, 10 a + 5 + j) x the block's 32 points, ten
masks per iteration.

  python3 tools/h16_mask_stats.py [--seed 1] [--hyps 2000] [--points 10000] [--chunks 5] [--models FILE.npy]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ransac_amd import synthetic  # noqa: E402

f32 = np.float32
K_BAND_MP = f32(2.0 ** -18)
K_BAND_T = f32(2.0 ** -15)
UP18 = f32(1.0 + 2.0 ** -18)
UP20 = f32(1.0 + 2.0 ** -20)


def pow2_at_least(v):
    return float(np.ldexp(1.0, int(np.floor(np.log2(v))) + 1)) if v > 0 else 1.0


def dataset_consts(pts):
    """k_h16_consts: centres (fp32 numbers), power-of-two scales, fmax of the nine features."""
    p = pts[np.isfinite(pts).all(1)].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    cc = (0.5 * (lo + hi)).astype(np.float32).astype(np.float64)
    half = np.maximum(hi - cc, cc - lo)
    s1, s2 = pow2_at_least(max(half[0], half[1])), pow2_at_least(max(half[2], half[3]))
    f = features64(p, cc, s1, s2)
    fmax = np.nextafter((np.abs(f).max(0) * (1.0 + 2.0 ** -40)).astype(np.float32), f32(np.inf))
    ext = np.abs(pts[np.isfinite(pts).all(1)]).max(0).astype(np.float32)
    return cc, s1, s2, fmax, ext


def features64(p, cc, s1, s2):
    u, v = (p[:, 0] - cc[0]) / s1, (p[:, 1] - cc[1]) / s1
    pp, q = (p[:, 2] - cc[2]) / s2, (p[:, 3] - cc[3]) / s2
    return np.stack([u, v, np.ones_like(u), pp * u, pp * v, pp, q * u, q * v, q], 1)


ROW_ROUND, FEAT_ROUND = f32(2.0 ** -11), f32(2.0 ** -11 * (1.0 + 2.0 ** -12))  # usac_h16.hpp USAC_H16_*_ROUND
SLACKS = {  # name -> (row rounding, feature rounding) charged per fp16 value; None: F_m = 0, the unreachable floor
    "2^-10 (the bound before)": (f32(2.0 ** -10), f32(2.0 ** -10)),
    "round to nearest (h16_rows_of)": (ROW_ROUND, FEAT_ROUND),
    "F_m = 0 (floor)": None,
}


def rows_and_slack(H, cc, s1, s2, fmax, ext, thr, row_round=ROW_ROUND, feat_round=FEAT_ROUND):
    """h16_rows_of for every row of H (B x 9 fp32): fp16 rows (B x 3 x 9) and the slack F_m (B)."""
    H = H.astype(np.float32)
    aH = np.abs(H)
    T = f32(2.0) * f32(thr)
    # stage_a_bounds
    s20 = f32(2.0 ** -20)
    kx = aH[:, 0] * ext[0] + aH[:, 1] * ext[1] + aH[:, 2]
    ky = aH[:, 3] * ext[0] + aH[:, 4] * ext[1] + aH[:, 5]
    kz = aH[:, 6] * ext[0] + aH[:, 7] * ext[1] + aH[:, 8]
    dx, dy, dz = s20 * kx, s20 * ky, s20 * kz
    E = ((ext[2] * dz + dx) + (ext[3] * dz + dy)) * UP18
    band_max = K_BAND_MP * (((ext[0] + ext[1]) + (ext[2] + ext[3])) * UP20) + K_BAND_T * T
    trm = (T + band_max) * UP18
    F = (trm * dz + E) * UP20
    # h16_rows_of
    cx1, cy1, cx2, cy2 = (f32(c) for c in cc)
    s1, s2 = f32(s1), f32(s2)
    P = np.zeros((len(H), 3, 3), np.float32)
    aP = np.zeros_like(P)
    for r in range(3):
        a0, a1 = H[:, 3 * r] * cx1, H[:, 3 * r + 1] * cy1
        P[:, r, 0] = H[:, 3 * r] * s1
        P[:, r, 1] = H[:, 3 * r + 1] * s1
        P[:, r, 2] = (a0 + a1) + H[:, 3 * r + 2]
        aP[:, r, 0] = np.abs(P[:, r, 0])
        aP[:, r, 1] = np.abs(P[:, r, 1])
        aP[:, r, 2] = (np.abs(a0) + np.abs(a1)) + aH[:, 3 * r + 2]
    trmi = trm * f32(1.0 + 2.0 ** -10)
    g = np.zeros((len(H), 3, 9), np.float32)
    a = np.zeros_like(g)
    for c in range(3):
        g[:, 0, c] = cx2 * P[:, 2, c] - P[:, 0, c]
        a[:, 0, c] = abs(cx2) * aP[:, 2, c] + aP[:, 0, c]
        g[:, 0, 3 + c] = s2 * P[:, 2, c]
        a[:, 0, 3 + c] = s2 * aP[:, 2, c]
        g[:, 1, c] = cy2 * P[:, 2, c] - P[:, 1, c]
        a[:, 1, c] = abs(cy2) * aP[:, 2, c] + aP[:, 1, c]
        g[:, 1, 6 + c] = s2 * P[:, 2, c]
        a[:, 1, 6 + c] = s2 * aP[:, 2, c]
        g[:, 2, c] = trmi * P[:, 2, c]
        a[:, 2, c] = trmi * aP[:, 2, c]
    mx = np.abs(g).reshape(len(H), -1).max(1)
    fin = np.isfinite(a).all((1, 2)) & np.isfinite(F) & (mx > 2.0 ** -100) & (mx < 2.0 ** 100)
    e = -np.frexp(np.where(fin, mx, f32(1.0)))[1]  # max |g| 2^e in [0.5, 1)
    gh = np.ldexp(g, e[:, None, None]).astype(np.float32)
    gt = gh.astype(np.float16)
    agt = np.abs(gt.astype(np.float32))
    fk = fmax.astype(np.float32)[None, None, :]
    ae = np.ldexp(a, e[:, None, None]).astype(np.float32)
    term = agt * (feat_round * fk + f32(2.0 ** -25)) + \
        fk * (row_round * np.abs(gh) + f32(2.0 ** -25) + f32(2.0 ** -21) * ae) + \
        f32(2.0 ** -19) * agt * (fk + f32(2.0 ** -24))
    D = np.full((len(H), 3), f32(2.0 ** -100), np.float32)
    for c in range(9):  # the device's summation order
        D = D + term[:, :, c]
    D = D * UP18
    sc = np.ldexp(f32(1.0), e).astype(np.float32)
    dxf = s20 * (aH[:, 0] * ext[0] + aH[:, 1] * ext[1] + aH[:, 2])
    dyf = s20 * (aH[:, 3] * ext[0] + aH[:, 4] * ext[1] + aH[:, 5])
    ex_fma, ey_fma = ext[2] * dz + dxf, ext[3] * dz + dyf
    Fm = (F * sc + np.maximum(D[:, 0] + ex_fma * sc, D[:, 1] + ey_fma * sc) + trmi * dz * sc + D[:, 2]) * UP18
    Fm = np.where(fin & np.isfinite(Fm), Fm, f32(np.inf)).astype(np.float32)
    gt[~fin] = 0
    return gt, Fm


def dlt_models(pts, B, rng):
    """B 4-point DLT homographies of random minimal samples: the null vector of the 8 x 9 system."""
    n = len(pts)
    idx = np.stack([rng.choice(n, 4, replace=False) for _ in range(B)])
    p = pts[idx].astype(np.float64)  # B x 4 x 4
    x1, y1, x2, y2 = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    z, o = np.zeros_like(x1), np.ones_like(x1)
    r1 = np.stack([-x1, -y1, -o, z, z, z, x2 * x1, x2 * y1, x2], -1)
    r2 = np.stack([z, z, z, -x1, -y1, -o, y2 * x1, y2 * y1, y2], -1)
    A = np.concatenate([r1, r2], 1)
    h = np.linalg.svd(A)[2][:, -1, :]
    h = h / np.abs(h).max(1, keepdims=True)
    return h.astype(np.float32)


def mask_lanes(acc, Fm, nblk):
    """kept lanes of every ballot mask: (wave, block, mask) for hypotheses x padded points of acc (3 x B x P)"""
    B = acc.shape[1]
    with np.errstate(invalid="ignore"):
        R = np.abs(acc[2]) + Fm[:, None]
        keep = (np.abs(acc[0]) <= R) & (np.abs(acc[1]) <= R)  # B x points
    # mask (wave w, block b, tile a, j): hypotheses 20 w + 10 a + j and + 5, the block's 32 points
    k = keep.reshape(B // 20, 2, 2, 5, nblk, 32)  # wave, a, half, j, block, point
    lanes = k.sum((2, 5))  # wave, a, j, block: kept lanes of the mask
    return lanes.transpose(0, 3, 1, 2).reshape(B // 20, nblk, 10)  # wave, block, mask


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--hyps", type=int, default=2000)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--inlier-ratio", type=float, default=0.3)
    ap.add_argument("--threshold", type=float, default=2.0)
    ap.add_argument("--chunks", type=int, default=5, help="point chunks (the library's choice at cfg2: 5)")
    ap.add_argument("--models", metavar="FILE.npy", default=None,
                    help="hypotheses from a file (B x 9 float32, e.g. a batch as the library solved it: "
                         "Context.estimate_models(Context.draw_samples(...))) instead of random DLT models; "
                         "--hyps then takes the file's first rows")
    args = ap.parse_args()
    pts, _, _ = synthetic.homography_points(n=args.points, inlier_ratio=args.inlier_ratio, seed=args.seed)
    cc, s1, s2, fmax, ext = dataset_consts(pts)
    if args.models:
        H = np.load(args.models).astype(np.float32).reshape(-1, 9)
        B = min(len(H), args.hyps) // 20 * 20
        H, source = H[:B], "the first %d models of %s" % (B, args.models)
    else:
        B = (args.hyps + 19) // 20 * 20
        H, source = dlt_models(pts, B, np.random.default_rng(args.seed)), "random 4-point DLT models"
    feat = features64(pts.astype(np.float64), cc, s1, s2).astype(np.float32).astype(np.float16)
    n = len(pts)
    nblk = (n + 31) // 32
    fpad = np.full((nblk * 32, 9), np.nan)
    fpad[:n] = feat.astype(np.float64)  # padding points: NaN features, never kept
    per = (nblk + args.chunks - 1) // args.chunks
    print("h16 keep-mask statistics: seed %d, %d hypotheses (%d waves; %s), %d points (%d blocks), thr %g, "
          "%d point chunks of %d blocks" % (args.seed, B, B // 20, source, n, nblk, args.threshold, args.chunks, per))
    lanes = {name: [] for name in SLACKS}
    slack = {name: [] for name in SLACKS}
    for at in range(0, B, 2000):  # 100 waves at a time: the tile of 2 000 x 10 000 pairs is 0.5 GB in fp64
        Hc = H[at:at + 2000]
        rows, _ = rows_and_slack(Hc, cc, s1, s2, fmax, ext, args.threshold)
        acc = np.einsum("hrk,pk->rhp", rows.astype(np.float64), fpad).astype(np.float32)
        for name, rounds in SLACKS.items():
            Fm = rows_and_slack(Hc, cc, s1, s2, fmax, ext, args.threshold, *rounds)[1] if rounds else \
                np.zeros(len(Hc), np.float32)
            slack[name].append(Fm)
            lanes[name].append(mask_lanes(acc, Fm, nblk))
    for name in SLACKS:
        ln, Fm = np.concatenate(lanes[name]), np.concatenate(slack[name])
        nonempty = ln > 0
        pairs = int(ln.sum())
        iters = ln.shape[0] * ln.shape[1]
        print("\nslack: %s -- float32 mirror of h16_rows_of (exact form); F_m median %.4g, non-finite hypotheses %d"
              % (name, float(np.median(Fm[np.isfinite(Fm)])), int((~np.isfinite(Fm)).sum())))
        print("keep rate                                   %.4f %%  (%d of %d pairs)"
              % (100.0 * pairs / (B * n), pairs, B * n))
        print("non-empty masks per iteration (of ten)      %.3f" % (nonempty.sum() / iters))
        print("iterations with a non-empty mask            %.1f %%" % (100.0 * nonempty.any(2).mean()))
        print("one-lane share of non-empty masks           %.1f %%" % (100.0 * (ln == 1).sum() / nonempty.sum()))
        print("kept pairs in one-lane masks                %.1f %%" % (100.0 * (ln == 1).sum() / pairs))
        print("kept pairs in masks of 8 or more lanes      %.1f %%" % (100.0 * ln[ln >= 8].sum() / pairs))
        print("kept pairs per wave (one chunk of %d)        %.1f" % (args.chunks, pairs / (ln.shape[0] * args.chunks)))
        print("non-empty masks per wave (one chunk of %d)   %.1f" % (args.chunks, nonempty.sum() / (ln.shape[0] * args.chunks)))
        hist = np.bincount(np.minimum(ln[nonempty], 9), minlength=10)[1:]
        print("non-empty masks by kept lanes 1..8, 9+      " + " ".join("%d" % c for c in hist))


if __name__ == "__main__":
    main()
