/*
 * usac_oracle.c -- CPU ORACLE (test infrastructure only; see usac_oracle.h header).
 *
 * Plain-C restatement of the reference hot path.  Build: oracle/Makefile
 * (gcc -O2 -ffp-contract=off, no -march: x86-64 SSE2 scalar fp32/fp64, no FMA,
 * matching the reference's CMake build which sets no optimisation/arch flags,
 * CMakeLists.txt:102-107).
 *
 * Floating-point conventions restated from the reference's C++ (g++/libstdc++):
 *  - unqualified sqrt()/log() on float arguments resolve to the C library's
 *    double overloads (only <cmath> is included, usac/precomp.hpp:12; no
 *    `using namespace std`), so e.g. homography_estimator.hpp:97-98 sums two
 *    double square roots before rounding to float;
 *  - every fp32 expression is evaluated left to right, one rounding per operation.
 */
#define _DEFAULT_SOURCE
#include "usac_oracle.h"

/* The LSQ fits' A^T A order (the spec shared with kernels_nonmin.hip kAtaBlock): 16-point
 * blocks, 64 blocks per superblock.  Round 4 session 2 shortened the block from 64 points: the
 * device runs one lane per (block, entry group), so the block length is its dependent chain. */
#define ORC_ATA_BLOCK 16u
#define ORC_ATA_SUPER (64u * ORC_ATA_BLOCK)

#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ glibc stream */
/* The reference draws with glibc random() (uniform_sampler.hpp:83) and seeds with
 * srand() (uniform_sampler.hpp:24); glibc's rand/srand share random()'s state. */
void orc_srandom(unsigned int seed) { srandom(seed); }
long orc_random(void) { return random(); }
void orc_random_n(long *out, int n) {
    for (int i = 0; i < n; i++) out[i] = random();
}

/* ------------------------------------------------------------ UniformSampler */
struct orc_uniform {
    unsigned int *pool;
    int max;
    unsigned int points_size, sample_size;
};

/* uniform_sampler.hpp:32-39 setPointsSize */
orc_uniform *orc_uniform_new(unsigned int points_size, unsigned int sample_size) {
    orc_uniform *s = (orc_uniform *)calloc(1, sizeof(*s));
    s->pool = (unsigned int *)malloc(sizeof(unsigned int) * (points_size ? points_size : 1));
    for (unsigned int i = 0; i < points_size; i++) s->pool[i] = i;
    s->max = (int)points_size;
    s->points_size = points_size;
    s->sample_size = sample_size;
    return s;
}
void orc_uniform_free(orc_uniform *s) {
    if (!s) return;
    free(s->pool);
    free(s);
}
/* uniform_sampler.hpp:42-54 generateSample: persistent pool; `max` refills to N when it
 * reaches 0, also in the middle of a sample. */
void orc_uniform_sample(orc_uniform *s, int *sample) {
    for (unsigned int i = 0; i < s->sample_size; i++) {
        if (s->max == 0) s->max = (int)s->points_size;
        unsigned int idx = (unsigned int)random() % (unsigned int)s->max;
        unsigned int v = s->pool[idx];
        s->max--;
        s->pool[idx] = s->pool[s->max];
        s->pool[s->max] = v;
        sample[i] = (int)v;
    }
}
void orc_uniform_samples(orc_uniform *s, int *out, int count) {
    for (int c = 0; c < count; c++) orc_uniform_sample(s, out + (size_t)c * s->sample_size);
}

/* ------------------------------------------------------------ small linear algebra */

/* cv::Mat::inv() on a CV_32F 3x3 (DECOMP_LU closed form of cv::invert): determinant and
 * cofactors from exact float*float products in fp64, scaled by 1/det in fp64, cast to
 * float once.  Singular (det == 0) => zero matrix, returns 0.  Used by
 * homography_estimator.hpp:35 (setModelParameters), normalized_dlt.cpp:18 (T2.inv()). */
int orc_inv3x3(const float *m, float *dst) {
#define M_(r, c) ((double)m[3 * (r) + (c)])
    double d = M_(0, 0) * (M_(1, 1) * M_(2, 2) - M_(1, 2) * M_(2, 1)) -
               M_(0, 1) * (M_(1, 0) * M_(2, 2) - M_(1, 2) * M_(2, 0)) +
               M_(0, 2) * (M_(1, 0) * M_(2, 1) - M_(1, 1) * M_(2, 0));
    if (d == 0.0) {
        for (int i = 0; i < 9; i++) dst[i] = 0.f;
        return 0;
    }
    d = 1.0 / d;
    double t[9];
    t[0] = (M_(1, 1) * M_(2, 2) - M_(1, 2) * M_(2, 1)) * d;
    t[1] = (M_(0, 2) * M_(2, 1) - M_(0, 1) * M_(2, 2)) * d;
    t[2] = (M_(0, 1) * M_(1, 2) - M_(0, 2) * M_(1, 1)) * d;
    t[3] = (M_(1, 2) * M_(2, 0) - M_(1, 0) * M_(2, 2)) * d;
    t[4] = (M_(0, 0) * M_(2, 2) - M_(0, 2) * M_(2, 0)) * d;
    t[5] = (M_(0, 2) * M_(1, 0) - M_(0, 0) * M_(1, 2)) * d;
    t[6] = (M_(1, 0) * M_(2, 1) - M_(1, 1) * M_(2, 0)) * d;
    t[7] = (M_(0, 1) * M_(2, 0) - M_(0, 0) * M_(2, 1)) * d;
    t[8] = (M_(0, 0) * M_(1, 1) - M_(0, 1) * M_(1, 0)) * d;
#undef M_
    for (int i = 0; i < 9; i++) dst[i] = (float)t[i];
    return 1;
}

/* Path counters (usac_oracle.h orc_trace_*): thread-local, write-only for the solvers -- no
 * result depends on them. */
static __thread int g_trace[ORC_TRACE_N];
void orc_trace_reset(void) {
    memset(g_trace, 0, sizeof(g_trace));
    g_trace[ORC_TRACE_EIG_EXIT] = -1;
}
void orc_trace_get(int *out) { memcpy(out, g_trace, sizeof(g_trace)); }
static int eig_exit(int code, int steps) {
    g_trace[ORC_TRACE_EIG_EXIT] = code;
    g_trace[ORC_TRACE_EIG_STEPS] = steps;
    return code == ORC_EIG_CONVERGED;
}

/* One-sided (Hestenes) Jacobi on the ROWS of an r x 9 matrix, r <= 9, fp64.
 * Restates the row space part of cv::SVD::compute (thin, default flags) used by
 * dlt.cpp:43 / dlt.cpp:92: after convergence the rows are mutually orthogonal,
 * row_i = sigma_i * v_i^T, so the thin vt's last row (smallest sigma) is the row of
 * smallest norm.  Fixed algorithm (shared by the GPU kernel's spec):
 *   sweeps s < 30; pairs in round-robin (tournament) order -- circle method over rows
 *   0..r-1 (odd r gets a bye slot), R-1 rounds of disjoint pairs, each pair as (min, max);
 *   row norms n_i = sum_k W[i][k]^2 (k = 0..8 in order) recomputed at each sweep start;
 *   per pair: a = n_p, b = n_q, g = sum_k W[p][k] W[q][k]; skip when g*g <= 1e-28*(a*b);
 *   d = b - a, g2 = 2g, r = sqrt(d^2 + g2^2), u = |d| + r, inv = 1/sqrt(2 r u),
 *   c = u inv, s = g2 inv (negated when d < 0), t = s (2 r inv) -- the classical
 *   t = sign(zeta)/(|zeta| + sqrt(1+zeta^2)), zeta = d/2g, c = 1/sqrt(1+t^2), s = c t with
 *   one division instead of two ((c, s) = (u, g2)/|(u, g2)|, |(u, g2)|^2 = 2 r u);
 *   row_p <- c*row_p - s*row_q; row_q <- s*row_p + c*row_q;
 *   n_p <- a - t*g, n_q <- b + t*g;  stop after a sweep with no rotation.
 * Round 3: the sums of products and the rotations are fused (fma(), one rounding, =
 * v_fma_f64 on the device): the norms and g are fma chains over k = 0..8, row_p =
 * fma(c, wp, -(s wq)), row_q = fma(s, wp, c wq), r = sqrt(fma(d, d, g2 g2)). */
#define ORC_JAC_SWEEPS 30
#define ORC_JAC_EPS2 1e-28 /* skip when g^2 <= 1e-28 a b  (|g| <= 1e-14 sqrt(a b)) */
static int tournament_pairs(int r, int pairs[][2]) {
    int m = (r % 2) ? r + 1 : r; /* bye slot for odd r */
    int arr[10], np = 0;
    for (int i = 0; i < m; i++) arr[i] = i;
    for (int round = 0; round < m - 1; round++) {
        for (int i = 0; i < m / 2; i++) {
            int p = arr[i], q = arr[m - 1 - i];
            if (p >= r || q >= r) continue;
            pairs[np][0] = p < q ? p : q;
            pairs[np][1] = p < q ? q : p;
            np++;
        }
        int last = arr[m - 1];
        for (int i = m - 1; i > 1; i--) arr[i] = arr[i - 1];
        arr[1] = last;
    }
    return np;
}

static void row_jacobi(double W[][9], int r) {
    int pairs[45][2];
    int np = tournament_pairs(r, pairs);
    for (int sweep = 0; sweep < ORC_JAC_SWEEPS; sweep++) {
        int rotated = 0;
        /* row norms recomputed once per sweep, updated exactly-in-theory within it:
         * a' = a - t g, b' = b + t g */
        double nrm[9];
        for (int i = 0; i < r; i++) {
            double a = 0.0;
            for (int k = 0; k < 9; k++) a = fma(W[i][k], W[i][k], a);
            nrm[i] = a;
        }
        for (int pi = 0; pi < np; pi++) {
            const int p = pairs[pi][0], q = pairs[pi][1];
            const double a = nrm[p], b = nrm[q];
            double g = 0.0;
            for (int k = 0; k < 9; k++) g = fma(W[p][k], W[q][k], g);
            if (g * g <= ORC_JAC_EPS2 * (a * b)) continue;
            rotated = 1;
            const double d = b - a, g2 = 2.0 * g;
            const double rr = sqrt(fma(d, d, g2 * g2));
            const double u = fabs(d) + rr, r2 = 2.0 * rr;
            const double inv = 1.0 / sqrt(r2 * u);
            const double c = u * inv;
            double s = g2 * inv;
            if (d < 0.0) s = -s;
            const double t = s * (r2 * inv);
            for (int k = 0; k < 9; k++) {
                double wp = W[p][k], wq = W[q][k];
                W[p][k] = fma(c, wp, -(s * wq));
                W[q][k] = fma(s, wp, c * wq);
            }
            nrm[p] = a - t * g;
            nrm[q] = b + t * g;
        }
        if (!rotated) break;
    }
}

/* From converged orthogonal rows pick the model vector:
 *  thin      -> row of smallest squared norm (first on ties) = vt.row(vt.rows-1)
 *  nullspace -> unit vector orthogonal to every non-zero row (two Gram-Schmidt passes
 *               starting from the least-represented coordinate axis).
 * Writes h (9 doubles, unnormalised). */
static void pick_vector(double W[][9], int r, int mode, double *h) {
    double n2[9];
    for (int i = 0; i < r; i++) {
        double a = 0.0;
        for (int k = 0; k < 9; k++) a += W[i][k] * W[i][k];
        n2[i] = a;
    }
    if (mode == ORC_DLT_THIN) {
        int best = 0;
        for (int i = 1; i < r; i++)
            if (n2[i] < n2[best]) best = i;
        for (int k = 0; k < 9; k++) h[k] = W[best][k];
        return;
    }
    double U[9][9];
    int nu = 0;
    for (int i = 0; i < r; i++) {
        if (n2[i] > 0.0) {
            double inv = 1.0 / sqrt(n2[i]);
            for (int k = 0; k < 9; k++) U[nu][k] = W[i][k] * inv;
            nu++;
        }
    }
    int ks = 0;
    double bestc = 0.0;
    for (int k = 0; k < 9; k++) {
        double c = 0.0;
        for (int i = 0; i < nu; i++) c += U[i][k] * U[i][k];
        if (k == 0 || c < bestc) {
            bestc = c;
            ks = k;
        }
    }
    for (int k = 0; k < 9; k++) h[k] = (k == ks) ? 1.0 : 0.0;
    for (int pass = 0; pass < 2; pass++) {
        for (int i = 0; i < nu; i++) {
            double d = 0.0;
            for (int k = 0; k < 9; k++) d += U[i][k] * h[k];
            for (int k = 0; k < 9; k++) h[k] -= d * U[i][k];
        }
    }
}

/* Two-sided Jacobi eigen-decomposition of a symmetric 9x9 (fp64), round-robin ("parallel")
 * ordering: a sweep is 9 rounds of 4 disjoint (p, q) planes (the circle schedule over 10
 * indices, the 10th a dummy).  Per round: every plane's rotation from the matrix at the start
 * of the round (planes with a zero off-diagonal are skipped), then all column updates, then
 * all row updates, then V's columns -- the disjoint planes make each element's update
 * unambiguous, so the device runs the four planes of a round at once (kernels_nonmin.hip).
 * Stops when the off-diagonal mass is <= 1e-30 of the diagonal's.  Returns the eigenvector
 * of the smallest eigenvalue in v.  Restates cv::SVD::compute's last vt row for a tall
 * (2n > 9) DLT system via the normal matrix (dlt.cpp:92-98, eight_points.cpp:38-44); the
 * rotation order is this build's spec (OpenCV's is unpinned). */
static const signed char kJacobiRounds[9][4][2] = {
    {{1, 8}, {2, 7}, {3, 6}, {4, 5}}, {{0, 8}, {1, 6}, {2, 5}, {3, 4}}, {{0, 7}, {1, 4}, {2, 3}, {6, 8}},
    {{0, 6}, {1, 2}, {4, 8}, {5, 7}}, {{0, 5}, {2, 8}, {3, 7}, {4, 6}}, {{0, 4}, {1, 7}, {2, 6}, {3, 5}},
    {{0, 3}, {1, 5}, {2, 4}, {7, 8}}, {{0, 2}, {1, 3}, {5, 8}, {6, 7}}, {{0, 1}, {3, 8}, {4, 7}, {5, 6}}};

static void sym_eig_min_jacobi(double A[9][9], double *v) {
    double V[9][9];
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 50; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 9; p++) {
            diag += A[p][p] * A[p][p];
            for (int q = p + 1; q < 9; q++) off += A[p][q] * A[p][q];
        }
        if (off <= 1e-30 * diag || off == 0.0) break;
        for (int r = 0; r < 9; r++) {
            double cs[4][2];
            int on[4];
            for (int k = 0; k < 4; k++) {
                const int p = kJacobiRounds[r][k][0], q = kJacobiRounds[r][k][1];
                const double apq = A[p][q];
                on[k] = apq != 0.0;
                if (!on[k]) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                cs[k][0] = c;
                cs[k][1] = s;
            }
            for (int k = 0; k < 4; k++) { /* columns */
                if (!on[k]) continue;
                const int p = kJacobiRounds[r][k][0], q = kJacobiRounds[r][k][1];
                const double c = cs[k][0], s = cs[k][1];
                for (int i = 0; i < 9; i++) {
                    const double aip = A[i][p], aiq = A[i][q];
                    A[i][p] = c * aip - s * aiq;
                    A[i][q] = s * aip + c * aiq;
                }
            }
            for (int k = 0; k < 4; k++) { /* rows */
                if (!on[k]) continue;
                const int p = kJacobiRounds[r][k][0], q = kJacobiRounds[r][k][1];
                const double c = cs[k][0], s = cs[k][1];
                for (int j = 0; j < 9; j++) {
                    const double apj = A[p][j], aqj = A[q][j];
                    A[p][j] = c * apj - s * aqj;
                    A[q][j] = s * apj + c * aqj;
                }
            }
            for (int k = 0; k < 4; k++) { /* V columns */
                if (!on[k]) continue;
                const int p = kJacobiRounds[r][k][0], q = kJacobiRounds[r][k][1];
                const double c = cs[k][0], s = cs[k][1];
                for (int i = 0; i < 9; i++) {
                    const double vip = V[i][p], viq = V[i][q];
                    V[i][p] = c * vip - s * viq;
                    V[i][q] = s * vip + c * viq;
                }
            }
        }
    }
    int m = 0;
    for (int i = 1; i < 9; i++)
        if (A[i][i] < A[m][m]) m = i;
    for (int k = 0; k < 9; k++) v[k] = V[k][m];
}

/* Smallest-eigenvalue eigenvector of the symmetric 9x9 normal matrix (the LSQ fits'
 * cv::SVD of a tall system, see sym_eig_min_jacobi): inverse iteration on A + mu I, with the
 * two-sided Jacobi above as the fall-back.  Spec (identical on the device, kernels_nonmin.hip):
 *   tr = sum of the diagonal (k = 0..8 in order); not (tr > 0) or not finite -> fall back;
 *   mu = tr * 1e-12; Cholesky L of A + mu I column by column: d = (A[j][j] + mu) - L[j][0]^2 -
 *   ... - L[j][j-1]^2 (left to right), not (d > 0) -> fall back, L[j][j] = sqrt(d),
 *   inv[j] = 1 / L[j][j], L[i][j] = (A[i][j] - L[i][0] L[j][0] - ...) * inv[j];
 *   x = (1/3, ..., 1/3); up to 30 times: L y = x (y[i] = (x[i] - L[i][0] y[0] - ...) * inv[i]),
 *   L^T z = y (i = 8..0, z[i] = (y[i] - L[i+1][i] z[i+1] - ... - L[8][i] z[8]) * inv[i]),
 *   nn = sum z[k]^2 (not (nn > 0) or not finite -> fall back), r = 1 / sqrt(nn), x' = z * r,
 *   d = max |x' - x| (first of equal maxima irrelevant), x = x'; d <= 1e-13 -> done (v = x);
 *   from the third step on, d > d_prev / 4 (slow: the two smallest eigenvalues are close, as
 *   for an outlier-contaminated algebraic fit) -> fall back; 30 steps -> fall back.
 * Converges in 5-7 steps on inlier sets (eigenvalue ratio ~1e-4); the fall-back keeps the
 * old spec for degenerate systems.  The eigenvector is defined up to sign: inverse iteration
 * from x keeps the sign with x . v > 0, the Jacobi the sign its rotations leave. */
static int eig_min_invit(double A[9][9], double *v) {
    double tr = 0.0;
    for (int k = 0; k < 9; k++) tr += A[k][k];
    if (!(tr > 0.0) || !isfinite(tr)) return eig_exit(ORC_EIG_TRACE, 0);
    const double mu = tr * 1e-12;
    double L[9][9], inv[9];
    for (int j = 0; j < 9; j++) {
        double d = A[j][j] + mu;
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
        if (!(d > 0.0)) return eig_exit(ORC_EIG_CHOLESKY, 0);
        L[j][j] = sqrt(d);
        inv[j] = 1.0 / L[j][j];
        for (int i = j + 1; i < 9; i++) {
            double s = A[i][j];
            for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
            L[i][j] = s * inv[j];
        }
    }
    double x[9], dprev = 0.0;
    for (int k = 0; k < 9; k++) x[k] = 1.0 / 3.0;
    for (int it = 0; it < 30; it++) {
        double y[9], z[9];
        for (int i = 0; i < 9; i++) {
            double s = x[i];
            for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
            y[i] = s * inv[i];
        }
        for (int i = 8; i >= 0; i--) {
            double s = y[i];
            for (int k = i + 1; k < 9; k++) s -= L[k][i] * z[k];
            z[i] = s * inv[i];
        }
        double nn = 0.0;
        for (int k = 0; k < 9; k++) nn += z[k] * z[k];
        if (!(nn > 0.0) || !isfinite(nn)) return eig_exit(ORC_EIG_NN, it + 1);
        const double r = 1.0 / sqrt(nn);
        double d = 0.0;
        for (int k = 0; k < 9; k++) {
            const double xn = z[k] * r;
            const double e = fabs(xn - x[k]);
            if (e > d) d = e;
            x[k] = xn;
        }
        if (d <= 1e-13) {
            for (int k = 0; k < 9; k++) v[k] = x[k];
            return eig_exit(ORC_EIG_CONVERGED, it + 1);
        }
        if (it >= 2 && d > 0.25 * dprev) return eig_exit(ORC_EIG_SLOW, it + 1);
        dprev = d;
    }
    return eig_exit(ORC_EIG_STEPS, 30);
}

static void sym_eig_min(double A[9][9], double *v) {
    if (!eig_min_invit(A, v)) sym_eig_min_jacobi(A, v);
}

/* test hook: the 9x9 eigen spec (returns 1 when inverse iteration converged, 0 = Jacobi) */
int orc_sym_eig_min(const double *A81, double *v) {
    double A[9][9];
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) A[i][j] = A81[9 * i + j];
    const int ok = eig_min_invit(A, v);
    if (!ok) sym_eig_min_jacobi(A, v);
    return ok;
}

/* ------------------------------------------------------------ estimators */
struct orc_est {
    int kind;
    const float *pts;
    unsigned int n;
    int dlt_mode;
    /* cached model parameters (setModelParameters) */
    float a, b, c;        /* line2d_estimator.hpp:162-164 */
    float h[9], hi[9];    /* homography_estimator.hpp:33-45 */
    float f[9];           /* fundamental_estimator.hpp:36-46 */
};

orc_est *orc_est_new(int kind, const float *points, unsigned int n, int dlt_mode) {
    if (kind != ORC_LINE2D && kind != ORC_HOMOGRAPHY && kind != ORC_FUNDAMENTAL && kind != ORC_ESSENTIAL) return NULL;
    orc_est *e = (orc_est *)calloc(1, sizeof(*e));
    e->kind = kind;
    e->pts = points;
    e->n = n;
    e->dlt_mode = dlt_mode;
    return e;
}
void orc_est_free(orc_est *e) { free(e); }
int orc_est_sample_size(const orc_est *e) {
    return e->kind == ORC_LINE2D ? 2 : e->kind == ORC_FUNDAMENTAL ? 7 : e->kind == ORC_ESSENTIAL ? 5 : 4;
}
static int orc_est_cols(const orc_est *e) { return e->kind == ORC_LINE2D ? 2 : 4; }
int orc_est_max_models(const orc_est *e) { return e->kind == ORC_FUNDAMENTAL ? 3 : 1; }

/* DLt::DLT4p (usac/estimator/dlt/dlt.cpp:7-52): rows of A built in fp32 exactly as
 * dlt.cpp:24-41, SVD restated by row_jacobi; H = v / v[8] rounded once to float. */
static int dlt_rows_solve(double W[][9], int r, int mode, float *H) {
    double v[9];
    row_jacobi(W, r);
    pick_vector(W, r, mode, v);
    for (int k = 0; k < 9; k++) H[k] = (float)(v[k] / v[8]);
    return 1;
}

static void dlt_fill_rows(float x1, float y1, float x2, float y2, double *r0, double *r1) {
    float a[9] = {-x1, -y1, -1.f, 0.f, 0.f, 0.f, x2 * x1, x2 * y1, x2};
    float b[9] = {0.f, 0.f, 0.f, -x1, -y1, -1.f, y2 * x1, y2 * y1, y2};
    for (int k = 0; k < 9; k++) {
        r0[k] = (double)a[k];
        r1[k] = (double)b[k];
    }
}

/* Thin-row spec of the 4-pt DLT (round 3; the device's k_solve_h4, usac_device.hpp dlt4_thin_qr):
 * the row of vt wanted by dlt.cpp:48 is v8, the right singular vector of the smallest of A's
 * eight singular values.  With the Householder QR of A^T = Q R (Q 9x8, R 8x8 upper),
 * A = R^T Q^T and v8 = Q w8, w8 the eigenvector of the smallest eigenvalue of R R^T.  w8 is found
 * by two-vector subspace inverse iteration with a Rayleigh-Ritz step (R R^T never formed: two
 * triangular solves per vector; the Ritz vector converges at the rate sigma_8^2 / sigma_6^2, so a
 * close sigma_7 does not slow it -- NAPSAC's neighbourhood samples have sigma_8 / sigma_7 up to
 * 0.9).  All fp64, fma() = one rounding:
 *   QR, column j = row j of W (k = j..8): s2 = fma chain of W[j][k]^2, sig = sqrt(s2)
 *     (sig not finite and > 0 -> fall back); x0 = W[j][j]; alpha_j = x0 >= 0 ? -sig : sig;
 *     beta_j = 1/(sig (sig + |x0|)); W[j][j] = x0 - alpha_j (the reflector is W[j][j..8]);
 *     rows i = j+1..7: f = beta_j * (fma chain of W[j][k] W[i][k]), W[i][k] = fma(-f, W[j][k], W[i][k]);
 *     then R[j][j] = alpha_j, R[j][i] = W[i][j] (i > j); rd_j = 1/alpha_j.
 *   back(q): y_k = (fma chain q_k - R[k][i] y_i, i = k+1..7) * rd_k, k = 7..0   (R y = q)
 *   fwd(u):  y_k = (fma chain u_k - R[i][k] y_i, i = 0..k-1) * rd_k, k = 0..7   (R^T y = u)
 *   q1 = e_7, q2 = e_6, w0 = 0; at most ORC_QR_ITERS steps:
 *     y1 = back(q1), y2 = back(q2); a = y1.y1, b = y1.y2, d = y2.y2 (fma chains, k = 0..7);
 *     h = (a - d) * 0.5, r = sqrt(fma(h, h, b b)); (c1, c2) = h >= 0 ? (h + r, b) : (b, r - h)
 *     (the larger eigenvalue's eigenvector of [[a, b], [b, d]]); nn = sqrt(fma(c1, c1, c2 c2))
 *     (not finite and > 0 -> fall back), c1 *= 1/nn, c2 *= 1/nn;
 *     w_k = fma(c1, q1_k, c2 q2_k); dt = w.w0; e_k = |w_k - (dt < 0 ? -w0_k : w0_k)|;
 *     w0 = w; stop when max_k e_k <= 1e-13 (compare-select in k order);
 *     u1_k = fma(c1, y1_k, c2 y2_k), u2_k = fma(c1, y2_k, -(c2 y1_k)); z1 = fwd(u1), z2 = fwd(u2);
 *     Gram-Schmidt: q1 = z1 * (1/sqrt(z1.z1)); p = q1.z2, z2_k = fma(-p, q1_k, z2_k),
 *     q2 = z2 * (1/sqrt(z2.z2))  (either norm not finite and > 0 -> fall back);
 *   no stop -> fall back;  v = H_0 (H_1 (... H_7 [w0; 0])), H_j x = x - beta_j (v_j . x) v_j
 *   (fma chains over k = j..8).
 * Fall-back (degenerate / non-finite systems; none of 32768 cfg2 samples, 6e-5 of NAPSAC's):
 * row_jacobi + pick_vector on the same rows, the pre-round-3 spec.  4 - 5 steps on average;
 * H agrees with LAPACK's vt[7] as the Jacobi did (tests/test_reference_statistics.py). */
#define ORC_QR_ITERS 32
static void qr_back(double W[8][9], const double *rd, const double *q, double *y) {
    for (int k = 7; k >= 0; k--) {
        double t = q[k];
        for (int i = k + 1; i < 8; i++) t = fma(-W[i][k], y[i], t);
        y[k] = t * rd[k];
    }
}
static void qr_fwd(double W[8][9], const double *rd, const double *u, double *y) {
    for (int k = 0; k < 8; k++) {
        double t = u[k];
        for (int i = 0; i < k; i++) t = fma(-W[k][i], y[i], t);
        y[k] = t * rd[k];
    }
}
static double dot8(const double *x, const double *y) {
    double t = 0.0;
    for (int k = 0; k < 8; k++) t = fma(x[k], y[k], t);
    return t;
}
static int pos_finite(double x) { return x > 0.0 && x < INFINITY; }

static int dlt4_thin_qr(const double A[8][9], double *v) {
    double W[8][9], be[8], rd[8];
    memcpy(W, A, sizeof(W));
    for (int j = 0; j < 8; j++) {
        double s2 = 0.0;
        for (int k = j; k < 9; k++) s2 = fma(W[j][k], W[j][k], s2);
        const double sig = sqrt(s2);
        if (!pos_finite(sig)) return 0;
        const double x0 = W[j][j];
        const double alpha = x0 >= 0.0 ? -sig : sig;
        be[j] = 1.0 / (sig * (sig + fabs(x0)));
        W[j][j] = x0 - alpha;
        for (int i = j + 1; i < 8; i++) {
            double s = 0.0;
            for (int k = j; k < 9; k++) s = fma(W[j][k], W[i][k], s);
            const double f = be[j] * s;
            for (int k = j; k < 9; k++) W[i][k] = fma(-f, W[j][k], W[i][k]);
        }
        rd[j] = 1.0 / alpha;
    }
    double q1[8] = {0, 0, 0, 0, 0, 0, 0, 1.0}, q2[8] = {0, 0, 0, 0, 0, 0, 1.0, 0}, w0[8] = {0};
    double y1[8], y2[8], u1[8], u2[8];
    int conv = 0;
    for (int it = 0; it < ORC_QR_ITERS && !conv; it++) {
        qr_back(W, rd, q1, y1);
        qr_back(W, rd, q2, y2);
        const double a = dot8(y1, y1), b = dot8(y1, y2), d = dot8(y2, y2);
        const double h = (a - d) * 0.5, r = sqrt(fma(h, h, b * b));
        double c1 = h >= 0.0 ? h + r : b, c2 = h >= 0.0 ? b : r - h;
        const double nn = sqrt(fma(c1, c1, c2 * c2));
        if (!pos_finite(nn)) return 0;
        const double inn = 1.0 / nn;
        c1 = c1 * inn;
        c2 = c2 * inn;
        double w[8];
        for (int k = 0; k < 8; k++) w[k] = fma(c1, q1[k], c2 * q2[k]);
        const double dt = dot8(w, w0);
        double dmax = 0.0;
        for (int k = 0; k < 8; k++) {
            const double ek = fabs(w[k] - (dt < 0.0 ? -w0[k] : w0[k]));
            if (ek > dmax) dmax = ek;
            w0[k] = w[k];
        }
        if (dmax <= 1e-13) {
            conv = 1;
            break;
        }
        for (int k = 0; k < 8; k++) {
            u1[k] = fma(c1, y1[k], c2 * y2[k]);
            u2[k] = fma(c1, y2[k], -(c2 * y1[k]));
        }
        qr_fwd(W, rd, u1, y1);
        qr_fwd(W, rd, u2, y2);
        const double n1 = dot8(y1, y1);
        if (!pos_finite(n1)) return 0;
        const double i1 = 1.0 / sqrt(n1);
        for (int k = 0; k < 8; k++) q1[k] = y1[k] * i1;
        const double p = dot8(q1, y2);
        for (int k = 0; k < 8; k++) y2[k] = fma(-p, q1[k], y2[k]);
        const double n2 = dot8(y2, y2);
        if (!pos_finite(n2)) return 0;
        const double i2 = 1.0 / sqrt(n2);
        for (int k = 0; k < 8; k++) q2[k] = y2[k] * i2;
    }
    if (!conv) return 0;
    double x[9];
    for (int k = 0; k < 8; k++) x[k] = w0[k];
    x[8] = 0.0;
    for (int j = 7; j >= 0; j--) {
        double s = 0.0;
        for (int k = j; k < 9; k++) s = fma(W[j][k], x[k], s);
        const double f = be[j] * s;
        for (int k = j; k < 9; k++) x[k] = fma(-f, W[j][k], x[k]);
    }
    for (int k = 0; k < 9; k++) v[k] = x[k];
    return 1;
}

static int homography_dlt4(const orc_est *e, const int *sample, float *H) {
    double W[8][9];
    for (int i = 0; i < 4; i++) {
        const float *p = e->pts + 4 * (size_t)sample[i];
        dlt_fill_rows(p[0], p[1], p[2], p[3], W[2 * i], W[2 * i + 1]);
    }
    if (e->dlt_mode == ORC_DLT_THIN) {
        double v[9];
        if (dlt4_thin_qr((const double(*)[9])W, v)) {
            for (int k = 0; k < 9; k++) H[k] = (float)(v[k] / v[8]);
            return 1;
        }
    }
    return dlt_rows_solve(W, 8, e->dlt_mode, H);
}

/* GetNormalizingTransformation (normalizing_transformation.cpp:7-113): fp32 sums in
 * sample order; the distance accumulation adds a double sqrt into a float (:45-46);
 * scale = M_SQRT2 / (avg / n) in double, rounded to float (:50-51).
 * With weights (weights[point index], the weighted overload :117-166): the sums run over the
 * weighted coordinates w*x, and the distances are those of the weighted points from the origin
 * (not from the mean, :130-141); the transform is then applied to the unweighted points. */
static void normalizing_transform(const float *pts, const int *sample, unsigned int n, const float *weights,
                                  float *T1, float *T2, float *norm /* n x 4 */) {
    float m1x = 0, m1y = 0, m2x = 0, m2y = 0;
    float d1 = 0, d2 = 0;
    if (weights) {
        for (unsigned int i = 0; i < n; i++) {
            const float *p = pts + 4 * (size_t)sample[i];
            const float w = weights[sample[i]];
            const float x1 = w * p[0], y1 = w * p[1], x2 = w * p[2], y2 = w * p[3];
            m1x += x1;
            m1y += y1;
            m2x += x2;
            m2y += y2;
            d1 = (float)((double)d1 + sqrt((double)(x1 * x1 + y1 * y1)));
            d2 = (float)((double)d2 + sqrt((double)(x2 * x2 + y2 * y2)));
        }
        m1x /= (float)n;
        m1y /= (float)n;
        m2x /= (float)n;
        m2y /= (float)n;
    } else {
        for (unsigned int i = 0; i < n; i++) {
            const float *p = pts + 4 * (size_t)sample[i];
            m1x += p[0];
            m1y += p[1];
            m2x += p[2];
            m2y += p[3];
        }
        m1x /= (float)n;
        m1y /= (float)n;
        m2x /= (float)n;
        m2y /= (float)n;
        for (unsigned int i = 0; i < n; i++) {
            const float *p = pts + 4 * (size_t)sample[i];
            float x1m = p[0] - m1x, y1m = p[1] - m1y, x2m = p[2] - m2x, y2m = p[3] - m2y;
            d1 = (float)((double)d1 + sqrt((double)(x1m * x1m + y1m * y1m)));
            d2 = (float)((double)d2 + sqrt((double)(x2m * x2m + y2m * y2m)));
        }
    }
    float s1 = (float)(M_SQRT2 / (double)(d1 / (float)n));
    float s2 = (float)(M_SQRT2 / (double)(d2 / (float)n));
    float t1[9] = {s1, 0.f, -m1x * s1, 0.f, s1, -m1y * s1, 0.f, 0.f, 1.f};
    float t2[9] = {s2, 0.f, -m2x * s2, 0.f, s2, -m2y * s2, 0.f, 0.f, 1.f};
    memcpy(T1, t1, sizeof(t1));
    memcpy(T2, t2, sizeof(t2));
    for (unsigned int i = 0; i < n; i++) {
        const float *p = pts + 4 * (size_t)sample[i];
        norm[4 * i + 0] = T1[0] * p[0] + T1[2];
        norm[4 * i + 1] = T1[4] * p[1] + T1[5];
        norm[4 * i + 2] = T2[0] * p[2] + T2[2];
        norm[4 * i + 3] = T2[4] * p[3] + T2[5];
    }
}

/* DLt::NormalizedDLT (normalized_dlt.cpp:7-23): DLT (dlt.cpp:55-101) on the normalised
 * points, then H = T2^-1 * H * T1, H /= H33.  2n <= 8 rows keep the thin-SVD semantics
 * (SURVEY Q2); 2n >= 10 rows take the smallest right singular vector via the fp64
 * normal matrix. */
static int homography_normalized_dlt(const orc_est *e, const int *sample, unsigned int n, const float *weights,
                                     float *H) {
    if (n == 0) return 0;
    float T1[9], T2[9], T2i[9];
    float *norm = (float *)malloc(sizeof(float) * 4 * n);
    normalizing_transform(e->pts, sample, n, weights, T1, T2, norm);
    double v[9];
    if (2 * n <= 9) {
        double W[9][9];
        for (unsigned int i = 0; i < n; i++)
            dlt_fill_rows(norm[4 * i], norm[4 * i + 1], norm[4 * i + 2], norm[4 * i + 3], W[2 * i], W[2 * i + 1]);
        row_jacobi(W, (int)(2 * n));
        pick_vector(W, (int)(2 * n), ORC_DLT_THIN, v);
    } else {
        /* A^T A summation order (no reference order exists -- OpenCV's SVD hides it):
         * ORC_ATA_BLOCK-point blocks summed in point order, 64 blocks (a superblock) summed in
         * block order into a superblock partial, superblock partials summed in order. */
        double AtA[9][9];
        memset(AtA, 0, sizeof(AtA));
        for (unsigned int s0 = 0; s0 < n; s0 += ORC_ATA_SUPER) {
            double SP[9][9];
            memset(SP, 0, sizeof(SP));
            unsigned int s1 = s0 + ORC_ATA_SUPER < n ? s0 + ORC_ATA_SUPER : n;
            for (unsigned int b0 = s0; b0 < s1; b0 += ORC_ATA_BLOCK) {
                double P[9][9];
                memset(P, 0, sizeof(P));
                unsigned int b1 = b0 + ORC_ATA_BLOCK < n ? b0 + ORC_ATA_BLOCK : n;
                for (unsigned int i = b0; i < b1; i++) {
                    double r0[9], r1[9];
                    dlt_fill_rows(norm[4 * i], norm[4 * i + 1], norm[4 * i + 2], norm[4 * i + 3], r0, r1);
                    for (int j = 0; j < 9; j++)
                        for (int k = j; k < 9; k++) P[j][k] += r0[j] * r0[k] + r1[j] * r1[k];
                }
                for (int j = 0; j < 9; j++)
                    for (int k = j; k < 9; k++) SP[j][k] += P[j][k];
            }
            for (int j = 0; j < 9; j++)
                for (int k = j; k < 9; k++) AtA[j][k] += SP[j][k];
        }
        for (int j = 0; j < 9; j++)
            for (int k = 0; k < j; k++) AtA[j][k] = AtA[k][j];
        sym_eig_min(AtA, v);
    }
    free(norm);
    orc_inv3x3(T2, T2i);
    /* H = T2i * Hn * T1 in fp64 */
    double Hn[9], tmp[9], Hd[9];
    for (int k = 0; k < 9; k++) Hn[k] = v[k];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += Hn[3 * r + k] * (double)T1[3 * k + c];
            tmp[3 * r + c] = s;
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)T2i[3 * r + k] * tmp[3 * k + c];
            Hd[3 * r + c] = s;
        }
    for (int k = 0; k < 9; k++) H[k] = (float)(Hd[k] / Hd[8]);
    return 1;
}

/* Line2DEstimator::EstimateModel (line2d_estimator.hpp:36-54) */
static int line2d_estimate(const orc_est *e, const int *sample, float *m) {
    const float *p1 = e->pts + 2 * (size_t)sample[0];
    const float *p2 = e->pts + 2 * (size_t)sample[1];
    float a = p1[1] - p2[1];
    float b = p2[0] - p1[0];
    float mag = (float)sqrt((double)(a * a + b * b));
    a /= mag;
    b /= mag;
    float c = (p1[0] * p2[1] - p2[0] * p1[1]) / mag;
    m[0] = a;
    m[1] = b;
    m[2] = c;
    for (int k = 3; k < 9; k++) m[k] = 0.f;
    return 1;
}

/* Line2DEstimator::EstimateModelNonMinimalSample (line2d_estimator.hpp:59-107): PCA
 * with fp32 moments (sum_xy initialised to 0: SURVEY Q12), cv::eigen of the 2x2
 * covariance restated in closed form (fp64); the line normal is the eigenvector of the
 * smaller eigenvalue (sign is irrelevant to |ax+by+c|). */
static int line2d_nonminimal(const orc_est *e, const int *sample, unsigned int n, float *m) {
    if (n == 0) return 0;
    float sx = 0, sy = 0, sxy = 0, sx2 = 0, sy2 = 0;
    for (unsigned int i = 0; i < n; i++) {
        const float *p = e->pts + 2 * (size_t)sample[i];
        float x = p[0], y = p[1];
        sx += x;
        sy += y;
        sxy += x * y;
        sx2 += x * x;
        sy2 += y * y;
    }
    float fn = (float)n;
    float mx = sx / fn, my = sy / fn;
    float c00 = sx2 - 2.f * sx * mx + fn * mx * mx;
    float c01 = sxy - sx * my - sy * mx + fn * mx * my;
    float c11 = sy2 - 2.f * sy * my + fn * my * my;
    double p = c00, q = c11, r = c01;
    double half = 0.5 * (p - q);
    double rad = sqrt(half * half + r * r);
    double lmin = 0.5 * (p + q) - rad;
    double vx, vy;
    if (r == 0.0) {
        if (p <= q) { vx = 1.0; vy = 0.0; } else { vx = 0.0; vy = 1.0; }
    } else if (fabs(lmin - p) > fabs(lmin - q)) {
        vx = r; vy = lmin - p;
    } else {
        vx = lmin - q; vy = r;
    }
    double nrm = sqrt(vx * vx + vy * vy);
    float a = (float)(vx / nrm), b = (float)(vy / nrm);
    m[0] = a;
    m[1] = b;
    m[2] = -a * mx - b * my;
    for (int k = 3; k < 9; k++) m[k] = 0.f;
    return 1;
}

/* ------------------------------------------------------------ fundamental */

/* Orthonormal complement of the converged Jacobi rows (the FULL_UV null-space rows of
 * cv::SVDecomp, seven_points.cpp:88-90): rows normalised (zero rows skipped); for each
 * complement vector j: start axis = argmin_k (sum_i U[i][k]^2 + sum_{l<j} N[l][k]^2) (first
 * minimum), two Gram-Schmidt passes against U then N[0..j-1], normalise (x_k / |x|). */
static void null_complement(double W[][9], int r, int count, double N[][9]) {
    double U[9][9];
    int nu = 0;
    for (int i = 0; i < r; i++) {
        double a = 0.0;
        for (int k = 0; k < 9; k++) a += W[i][k] * W[i][k];
        if (a > 0.0) {
            double inv = 1.0 / sqrt(a);
            for (int k = 0; k < 9; k++) U[nu][k] = W[i][k] * inv;
            nu++;
        }
    }
    for (int j = 0; j < count; j++) {
        int ks = 0;
        double bestc = 0.0;
        for (int k = 0; k < 9; k++) {
            double c = 0.0;
            for (int i = 0; i < nu; i++) c += U[i][k] * U[i][k];
            for (int l = 0; l < j; l++) c += N[l][k] * N[l][k];
            if (k == 0 || c < bestc) {
                bestc = c;
                ks = k;
            }
        }
        double x[9];
        for (int k = 0; k < 9; k++) x[k] = (k == ks) ? 1.0 : 0.0;
        for (int pass = 0; pass < 2; pass++) {
            for (int i = 0; i < nu; i++) {
                double d = 0.0;
                for (int k = 0; k < 9; k++) d += U[i][k] * x[k];
                for (int k = 0; k < 9; k++) x[k] -= d * U[i][k];
            }
            for (int l = 0; l < j; l++) {
                double d = 0.0;
                for (int k = 0; k < 9; k++) d += N[l][k] * x[k];
                for (int k = 0; k < 9; k++) x[k] -= d * N[l][k];
            }
        }
        double nrm = 0.0;
        for (int k = 0; k < 9; k++) nrm += x[k] * x[k];
        nrm = sqrt(nrm);
        for (int k = 0; k < 9; k++) N[j][k] = x[k] / nrm;
    }
}

/* Null-space basis of an r x 9 system (r < 9) in the same completion order, by Householder QR
 * (round 3; the device's qr_null<R>, shared by the 7-pt F and 5-pt E solvers): QR of W^T as in
 * dlt4_thin_qr (s2 = fma chain, sig = sqrt(s2) -- not finite and > 0 -> return 0 and the caller
 * falls back to row_jacobi + null_complement --, alpha, beta, reflector in W[j][j..8], rows
 * i = j+1..r-1 updated by fma); null columns q_m = H_0 (... H_{r-1} e_{r+m}), m = 0..8-r
 * (fma chains over k = j..8); then for vector j: c_k = (fma chain over l < j of N[l][k]^2) -
 * (fma chain over m of q_m[k]^2) -- the row space's share of axis k minus 1, plus the earlier
 * vectors' --, start axis ks = first argmin; x_k = fma chain over m of q_m[ks] q_m[k] (the
 * projection of e_ks onto the null space); two passes of d = fma chain N[l].x,
 * x_k = fma(-d, N[l][k], x_k) over l < j; N[j][k] = x_k / sqrt(fma chain of x_k^2).
 * In exact arithmetic this is null_complement's result (the projector onto the row space and
 * its diagonal do not depend on the basis that spans it); the QR replaces the ~8-sweep row
 * Jacobi (k_solve_f7 0.10 ms -> see DESIGN.md). */
static int qr_null(double W[][9], int r, double N[][9]) {
    const int C = 9 - r;
    double be[9], Q[9][9];
    for (int j = 0; j < r; j++) {
        double s2 = 0.0;
        for (int k = j; k < 9; k++) s2 = fma(W[j][k], W[j][k], s2);
        const double sig = sqrt(s2);
        if (!pos_finite(sig)) return 0;
        const double x0 = W[j][j];
        const double alpha = x0 >= 0.0 ? -sig : sig;
        be[j] = 1.0 / (sig * (sig + fabs(x0)));
        W[j][j] = x0 - alpha;
        for (int i = j + 1; i < r; i++) {
            double s = 0.0;
            for (int k = j; k < 9; k++) s = fma(W[j][k], W[i][k], s);
            const double f = be[j] * s;
            for (int k = j; k < 9; k++) W[i][k] = fma(-f, W[j][k], W[i][k]);
        }
    }
    for (int m = 0; m < C; m++) {
        for (int k = 0; k < 9; k++) Q[m][k] = k == r + m ? 1.0 : 0.0;
        for (int j = r - 1; j >= 0; j--) {
            double s = 0.0;
            for (int k = j; k < 9; k++) s = fma(W[j][k], Q[m][k], s);
            const double f = be[j] * s;
            for (int k = j; k < 9; k++) Q[m][k] = fma(-f, W[j][k], Q[m][k]);
        }
    }
    for (int j = 0; j < C; j++) {
        int ks = 0;
        double best = 0.0;
        for (int k = 0; k < 9; k++) {
            double t = 0.0, u = 0.0;
            for (int m = 0; m < C; m++) t = fma(Q[m][k], Q[m][k], t);
            for (int l = 0; l < j; l++) u = fma(N[l][k], N[l][k], u);
            const double c = u - t;
            if (k == 0 || c < best) {
                best = c;
                ks = k;
            }
        }
        double x[9];
        for (int k = 0; k < 9; k++) {
            double t = 0.0;
            for (int m = 0; m < C; m++) t = fma(Q[m][ks], Q[m][k], t);
            x[k] = t;
        }
        for (int pass = 0; pass < 2; pass++) {
            for (int l = 0; l < j; l++) {
                double d = 0.0;
                for (int k = 0; k < 9; k++) d = fma(N[l][k], x[k], d);
                for (int k = 0; k < 9; k++) x[k] = fma(-d, N[l][k], x[k]);
            }
        }
        double nrm = 0.0;
        for (int k = 0; k < 9; k++) nrm = fma(x[k], x[k], nrm);
        nrm = sqrt(nrm);
        for (int k = 0; k < 9; k++) N[j][k] = x[k] / nrm;
    }
    return 1;
}

/* Real roots of c0 x^3 + c1 x^2 + c2 x + c3, ascending -- restates the contract of
 * cv::solveCubic (seven_points.cpp:131) with IEEE basic operations only (OpenCV's
 * closed form uses acos/cos/pow, which are not correctly rounded; this spec is shared
 * bit-for-bit with the device).  Monic form a, b, c; Cauchy bound R = 1 + max(|a|,|b|,|c|);
 * critical points from a^2 - 3b; each sign-changing bracket refined by bisection
 * (midpoint 0.5*(lo+hi), stop when it equals an end, <= 200 steps). */
static double cubic_eval(double a, double b, double c, double x) { return ((x + a) * x + b) * x + c; }

static double cubic_bisect(double a, double b, double c, double lo, double hi) {
    double flo = cubic_eval(a, b, c, lo);
    for (int it = 0; it < 200; it++) {
        double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        double fm = cubic_eval(a, b, c, mid);
        if (fm == 0.0) return mid;
        if ((fm < 0.0) == (flo < 0.0)) {
            lo = mid;
            flo = fm;
        } else {
            hi = mid;
        }
    }
    return 0.5 * (lo + hi);
}

static int cubic_roots(double c0, double c1, double c2, double c3, double *r) {
    if (c0 == 0.0) {
        if (c1 == 0.0) {
            if (c2 == 0.0) return g_trace[ORC_TRACE_CUBIC_C0_0]++, 0;
            r[0] = -c3 / c2;
            return g_trace[ORC_TRACE_CUBIC_C0_1]++, 1;
        }
        double D = c2 * c2 - 4.0 * c1 * c3;
        if (D < 0.0) return g_trace[ORC_TRACE_CUBIC_C0_0]++, 0;
        if (D == 0.0) {
            r[0] = -c2 / (2.0 * c1);
            return g_trace[ORC_TRACE_CUBIC_C0_1]++, 1;
        }
        double s = sqrt(D);
        double q = -0.5 * (c2 + (c2 >= 0.0 ? s : -s));
        double x1 = q / c1, x2 = c3 / q;
        r[0] = x1 < x2 ? x1 : x2;
        r[1] = x1 < x2 ? x2 : x1;
        return g_trace[ORC_TRACE_CUBIC_C0_2]++, 2;
    }
    const double a = c1 / c0, b = c2 / c0, c = c3 / c0;
    double R = fabs(a);
    if (fabs(b) > R) R = fabs(b);
    if (fabs(c) > R) R = fabs(c);
    R = R + 1.0;
    const double D = a * a - 3.0 * b;
    int n = 0;
    if (!(D > 0.0)) {
        r[n++] = cubic_bisect(a, b, c, -R, R);
        g_trace[ORC_TRACE_CUBIC_D_LE0]++;
        return n;
    }
    const double s = sqrt(D);
    const double m1 = (-a - s) / 3.0, m2 = (-a + s) / 3.0;
    const double v1 = cubic_eval(a, b, c, m1), v2 = cubic_eval(a, b, c, m2);
    if (v1 >= 0.0) r[n++] = cubic_bisect(a, b, c, -R, m1);
    if (v1 > 0.0 && v2 < 0.0) r[n++] = cubic_bisect(a, b, c, m1, m2);
    if (v2 <= 0.0) r[n++] = cubic_bisect(a, b, c, m2, R);
    if (n >= 1 && n <= 3) g_trace[ORC_TRACE_CUBIC_GEN_1 + n - 1]++;
    return n;
}

/* FundamentalEstimator oriented constraint (fundamental_estimator.hpp:189-231), fp32:
 * epipole = row0 x row2 (row1 x row2 when all |e_i| <= 1.9984e-15), then the sign of
 * (F0 x2 + F3 y2 + F6)(e1 - e2 y1) must agree over the 7 sample points. */
static int fund_is_valid(const float *pts, const float *F, const int *sample) {
    float e0 = F[1] * F[8] - F[2] * F[7];
    float e1 = F[2] * F[6] - F[0] * F[8];
    float e2 = F[0] * F[7] - F[1] * F[6];
    if (!((e0 > 1.9984e-15 || e0 < -1.9984e-15) || (e1 > 1.9984e-15 || e1 < -1.9984e-15) ||
          (e2 > 1.9984e-15 || e2 < -1.9984e-15))) {
        g_trace[ORC_TRACE_EPIPOLE2]++;
        e0 = F[4] * F[8] - F[5] * F[7];
        e1 = F[5] * F[6] - F[3] * F[8];
        e2 = F[3] * F[7] - F[4] * F[6];
    }
    float sig1 = 0.f;
    for (int i = 0; i < 7; i++) {
        const float *p = pts + 4 * (size_t)sample[i];
        float s1 = F[0] * p[2] + F[3] * p[3] + F[6];
        float s2 = e1 - e2 * p[1];
        float sig = s1 * s2;
        if (i == 0) sig1 = sig;
        else if (sig1 * sig < 0) return 0;
    }
    return 1;
}

/* FundamentalSolver::SevenPointsAlgorithm (seven_points.cpp:49-156) + the validity filter
 * of FundamentalEstimator::EstimateModel (fundamental_estimator.hpp:48-63): 7x9 fp32
 * rows, fp64 null basis by qr_null (f1, f2 = the two null rows, cast to float; row Jacobi +
 * null complement when it falls back),
 * fp32 cubic coefficients exactly as :98-128, roots (cubic_roots) cast to float, fp32
 * F assembly with F33 normalisation (:138-154); valid models kept in root order. */
static int fundamental_7pt(const orc_est *e, const int *sample, float *models) {
    double W[7][9];
    for (int i = 0; i < 7; i++) {
        const float *p = e->pts + 4 * (size_t)sample[i];
        float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
        float row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.f};
        for (int k = 0; k < 9; k++) W[i][k] = (double)row[k];
    }
    double N[2][9], W0[7][9];
    memcpy(W0, W, sizeof(W0));
    if (!qr_null(W, 7, N)) {
        g_trace[ORC_TRACE_F7_FALLBACK]++;
        row_jacobi(W0, 7);
        null_complement(W0, 7, 2, N);
    }
    float f1[9], f2[9];
    for (int k = 0; k < 9; k++) {
        f1[k] = (float)N[0][k];
        f2[k] = (float)N[1][k];
    }
    for (int i = 0; i < 9; i++) f1[i] -= f2[i];
    float t0 = f2[4] * f2[8] - f2[5] * f2[7];
    float t1 = f2[3] * f2[8] - f2[5] * f2[6];
    float t2 = f2[3] * f2[7] - f2[4] * f2[6];
    float c[4];
    c[3] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
    c[2] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
           f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) - f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
           f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
           f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
    t0 = f1[4] * f1[8] - f1[5] * f1[7];
    t1 = f1[3] * f1[8] - f1[5] * f1[6];
    t2 = f1[3] * f1[7] - f1[4] * f1[6];
    c[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
           f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) - f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
           f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
           f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
    c[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
    double rd[3];
    int nroots = cubic_roots((double)c[0], (double)c[1], (double)c[2], (double)c[3], rd);
    int valid = 0;
    for (int k = 0; k < nroots; k++) {
        float r = (float)rd[k];
        float F[9];
        float lambda = r, mu = 1.f;
        float s = f1[8] * r + f2[8];
        if ((double)fabsf(s) > DBL_EPSILON) {
            mu = 1.f / s;
            lambda *= mu;
            F[8] = 1.f;
        } else {
            F[8] = 0.f;
            g_trace[ORC_TRACE_F8_ZERO]++;
        }
        for (int i = 0; i < 8; i++) F[i] = f1[i] * lambda + f2[i] * mu;
        if (fund_is_valid(e->pts, F, sample)) {
            memcpy(models + 9 * valid, F, sizeof(F));
            valid++;
        }
    }
    return valid;
}

/* FundamentalSolver::EightPointsAlgorithm (eight_points.cpp:4-100): normalising transform,
 * n x 9 rows in fp32; thin last row for n <= 8, fp64 normal-matrix smallest
 * eigenvector otherwise (blocked order as the DLT); F = T2^T F T1 (fp64), F /= F33 when
 * |F33| > FLT_EPSILON (:76-99). */
/* Rank-2 variant of the 8-point polish: the block eight_points.cpp:58-68 keeps commented out
 * (SVD of F, smallest singular value zeroed, F = U S V^T).  The reference's published kusvod2
 * statistics (results/kusvod2/ CSVs) and its stored GT F models (exactly rank 2)
 * come from a revision that ran it; tests/test_reference_statistics.py switches it on to pin
 * the 7-point / Sampson / graph-cut path against those CSVs.  Off by default (current code). */
static int g_f8_rank2 = 0;
void orc_set_f8_rank2(int on) { g_f8_rank2 = on; }

static void row_jacobi_small(double W[][4], int r, int cols, double J[][4]);

/* F = J^T B after the row Jacobi (B = J F, orthogonal rows): zero the smallest-norm row of B,
 * i.e. the smallest singular value, and rebuild (fp64). */
static void rank2_project(double v[9]) {
    double B[4][4], J[4][4];
    memset(B, 0, sizeof(B));
    memset(J, 0, sizeof(J));
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) B[i][k] = v[3 * i + k];
        J[i][i] = 1.0;
    }
    row_jacobi_small(B, 3, 3, J);
    int mi = 0;
    double nmin = 0.0;
    for (int i = 0; i < 3; i++) {
        double a = 0.0;
        for (int k = 0; k < 3; k++) a += B[i][k] * B[i][k];
        if (i == 0 || a < nmin) {
            nmin = a;
            mi = i;
        }
    }
    for (int k = 0; k < 3; k++) B[mi][k] = 0.0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double a = 0.0;
            for (int i = 0; i < 3; i++) a += J[i][r] * B[i][c];
            v[3 * r + c] = a;
        }
}

static int fundamental_8pt(const orc_est *e, const int *sample, unsigned int n, const float *weights, float *F) {
    if (n == 0) return 0;
    float T1[9], T2[9];
    float *norm = (float *)malloc(sizeof(float) * 4 * n);
    normalizing_transform(e->pts, sample, n, weights, T1, T2, norm);
    double v[9];
    if (n <= 8) {
        double W[9][9];
        for (unsigned int i = 0; i < n; i++) {
            float x1 = norm[4 * i], y1 = norm[4 * i + 1], x2 = norm[4 * i + 2], y2 = norm[4 * i + 3];
            float row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.f};
            for (int k = 0; k < 9; k++) W[i][k] = (double)row[k];
        }
        row_jacobi(W, (int)n);
        pick_vector(W, (int)n, ORC_DLT_THIN, v);
    } else {
        double AtA[9][9]; /* blocks / superblocks as homography_normalized_dlt */
        memset(AtA, 0, sizeof(AtA));
        for (unsigned int s0 = 0; s0 < n; s0 += ORC_ATA_SUPER) {
            double SP[9][9];
            memset(SP, 0, sizeof(SP));
            unsigned int s1 = s0 + ORC_ATA_SUPER < n ? s0 + ORC_ATA_SUPER : n;
            for (unsigned int b0 = s0; b0 < s1; b0 += ORC_ATA_BLOCK) {
                double P[9][9];
                memset(P, 0, sizeof(P));
                unsigned int b1 = b0 + ORC_ATA_BLOCK < n ? b0 + ORC_ATA_BLOCK : n;
                for (unsigned int i = b0; i < b1; i++) {
                    float x1 = norm[4 * i], y1 = norm[4 * i + 1], x2 = norm[4 * i + 2], y2 = norm[4 * i + 3];
                    float row[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.f};
                    double rd[9];
                    for (int k = 0; k < 9; k++) rd[k] = (double)row[k];
                    for (int j = 0; j < 9; j++)
                        for (int k = j; k < 9; k++) P[j][k] += rd[j] * rd[k];
                }
                for (int j = 0; j < 9; j++)
                    for (int k = j; k < 9; k++) SP[j][k] += P[j][k];
            }
            for (int j = 0; j < 9; j++)
                for (int k = j; k < 9; k++) AtA[j][k] += SP[j][k];
        }
        for (int j = 0; j < 9; j++)
            for (int k = 0; k < j; k++) AtA[j][k] = AtA[k][j];
        sym_eig_min(AtA, v);
    }
    free(norm);
    if (g_f8_rank2) rank2_project(v);
    /* T2^T = [s2 0 0; 0 s2 0; t2_13 t2_23 1] */
    double T2t[9] = {T2[0], 0.0, 0.0, 0.0, T2[4], 0.0, T2[2], T2[5], 1.0};
    double tmp[9], Fd[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += v[3 * r + k] * (double)T1[3 * k + c];
            tmp[3 * r + c] = s;
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += T2t[3 * r + k] * tmp[3 * k + c];
            Fd[3 * r + c] = s;
        }
    if (fabs(Fd[8]) > (double)FLT_EPSILON) {
        for (int k = 0; k < 9; k++) F[k] = (float)(Fd[k] / Fd[8]);
    } else {
        for (int k = 0; k < 9; k++) F[k] = (float)Fd[k];
    }
    return 1;
}

/* FundamentalEstimator::GetError (fundamental_estimator.hpp:101-134): Sampson error, fp32,
 * left-to-right sums, one IEEE division (threshold in px^2). */
static inline float fundamental_error(const orc_est *e, unsigned int pidx) {
    const float *p = e->pts + 4 * (size_t)pidx;
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    const float *f = e->f;
    float Fx = f[0] * x1 + f[1] * y1 + f[2];
    float Fy = f[3] * x1 + f[4] * y1 + f[5];
    float Gx = f[0] * x2 + f[3] * y2 + f[6];
    float Gy = f[1] * x2 + f[4] * y2 + f[7];
    float s = x2 * Fx + y2 * Fy + f[6] * x1 + f[7] * y1 + f[8];
    return (s * s) / (Fx * Fx + Fy * Fy + Gx * Gx + Gy * Gy);
}

/* ------------------------------------------------------------ essential (5-pt) */
/* EssentialSolver::FivePoints / Solve5PointEssential (five_points.cpp:13-274), restated
 * with IEEE basic operations only so that the device follows it bit for bit (OpenCV's
 * SVD, determinant, inv and rpoly are not reproducible here -- parity vs the reference is
 * end-to-end tolerance):
 *   1. 5 rows [x1x2, x2y1, x2, x1y2, y1y2, y2, x1, y1, 1] in fp64 (:45-59); row Jacobi +
 *      null complement -> basis N0..N3 (vt rows 5..8 of the FULL_UV SVD, :65-104);
 *   2. E(x,y,z) = x N0 + y N1 + z N2 + N3 and its ten cubic constraints -- the nine
 *      entries of 2 E E^T E - tr(E E^T) E (row-major) and det E -- as the 10 x 10 matrix
 *      M(z) over the monomials [x^3, y^3, x^2y, xy^2, x^2, y^2, xy, x, y, 1] (mblock.hpp);
 *   3. det M(z) at z = -5..5 (LU, partial pivoting), Newton divided differences ->
 *      degree-10 coefficients (:113-136 interpolates at the same nodes);
 *   4. real roots, ascending: derivative-recursion isolation (Gauss-Lucas: every
 *      derivative's roots lie inside the root bound) + safeguarded Newton (:139-158);
 *   5. per root: null vector of M(z) by elimination with partial pivoting (v9 = 1):
 *      x = v7, y = v8 (:180-187); E assembled as :190-200;
 *   6. cheirality (:202-262): 3x3 SVD (row Jacobi with accumulated rotations), the four
 *      projections, linear triangulation (the rank-3 DLT null vector on the first ray,
 *      see triangulate()), CalcDepth; the
 *      first root whose E puts all five points in front of both cameras is returned. */

/* row Jacobi on r rows of `cols` (<= 4) columns, the round-1 row_jacobi rules (unfused
 * products, t and c by two divisions); J (nullable,
 * r x r) accumulates the rotations applied to the rows */
static void row_jacobi_small(double W[][4], int r, int cols, double J[][4]) {
    int pairs[6][2];
    int np = tournament_pairs(r, pairs);
    for (int sweep = 0; sweep < ORC_JAC_SWEEPS; sweep++) {
        int rotated = 0;
        double nrm[4];
        for (int i = 0; i < r; i++) {
            double a = 0.0;
            for (int k = 0; k < cols; k++) a += W[i][k] * W[i][k];
            nrm[i] = a;
        }
        for (int pi = 0; pi < np; pi++) {
            const int p = pairs[pi][0], q = pairs[pi][1];
            const double a = nrm[p], b = nrm[q];
            double g = 0.0;
            for (int k = 0; k < cols; k++) g += W[p][k] * W[q][k];
            if (g * g <= ORC_JAC_EPS2 * (a * b)) continue;
            rotated = 1;
            const double d = b - a, g2 = 2.0 * g;
            double t = g2 / (fabs(d) + sqrt(d * d + g2 * g2));
            if (d < 0.0) t = -t;
            const double c = 1.0 / sqrt(1.0 + t * t);
            const double sn = c * t;
            for (int k = 0; k < cols; k++) {
                double wp = W[p][k], wq = W[q][k];
                W[p][k] = c * wp - sn * wq;
                W[q][k] = sn * wp + c * wq;
            }
            if (J) {
                for (int k = 0; k < r; k++) {
                    double jp = J[p][k], jq = J[q][k];
                    J[p][k] = c * jp - sn * jq;
                    J[q][k] = sn * jp + c * jq;
                }
            }
            nrm[p] = a - t * g;
            nrm[q] = b + t * g;
        }
        if (!rotated) break;
    }
}

/* ----- bivariate cubic algebra over [x^3, y^3, x^2y, xy^2, x^2, y^2, xy, x, y, 1] */
typedef struct { double a, b, c; } lin3;         /* a x + b y + c */
typedef struct { double x2, y2, xy, x, y, k; } quad3;

static quad3 q_mul(lin3 u, lin3 v) {
    quad3 q;
    q.x2 = u.a * v.a;
    q.y2 = u.b * v.b;
    q.xy = u.a * v.b + u.b * v.a;
    q.x = u.a * v.c + u.c * v.a;
    q.y = u.b * v.c + u.c * v.b;
    q.k = u.c * v.c;
    return q;
}
static quad3 q_add(quad3 p, quad3 q) {
    quad3 r = {p.x2 + q.x2, p.y2 + q.y2, p.xy + q.xy, p.x + q.x, p.y + q.y, p.k + q.k};
    return r;
}
static quad3 q_sub(quad3 p, quad3 q) {
    quad3 r = {p.x2 - q.x2, p.y2 - q.y2, p.xy - q.xy, p.x - q.x, p.y - q.y, p.k - q.k};
    return r;
}
/* cubic = Q * L into c[10] */
static void c_mul(quad3 q, lin3 l, double *c) {
    c[0] = q.x2 * l.a;
    c[1] = q.y2 * l.b;
    c[2] = q.x2 * l.b + q.xy * l.a;
    c[3] = q.y2 * l.a + q.xy * l.b;
    c[4] = q.x2 * l.c + q.x * l.a;
    c[5] = q.y2 * l.c + q.y * l.b;
    c[6] = q.xy * l.c + q.x * l.b + q.y * l.a;
    c[7] = q.x * l.c + q.k * l.a;
    c[8] = q.y * l.c + q.k * l.b;
    c[9] = q.k * l.c;
}

/* M(z): rows 0..8 = 2 (E E^T E)_ij - tr(E E^T) E_ij (row-major), row 9 = det E */
static void e5_matrix(const double N[4][9], double z, double M[10][10]) {
    lin3 E[9];
    for (int k = 0; k < 9; k++) {
        E[k].a = N[0][k];
        E[k].b = N[1][k];
        E[k].c = z * N[2][k] + N[3][k];
    }
    quad3 EEt[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            quad3 acc = q_mul(E[3 * i], E[3 * j]);
            acc = q_add(acc, q_mul(E[3 * i + 1], E[3 * j + 1]));
            acc = q_add(acc, q_mul(E[3 * i + 2], E[3 * j + 2]));
            EEt[i][j] = acc;
        }
    quad3 tr = q_add(q_add(EEt[0][0], EEt[1][1]), EEt[2][2]);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double t0[10], t1[10], t2[10], tt[10];
            c_mul(EEt[i][0], E[j], t0);
            c_mul(EEt[i][1], E[3 + j], t1);
            c_mul(EEt[i][2], E[6 + j], t2);
            c_mul(tr, E[3 * i + j], tt);
            for (int m = 0; m < 10; m++) M[3 * i + j][m] = 2.0 * (t0[m] + t1[m] + t2[m]) - tt[m];
        }
    {
        double d0[10], d1[10], d2[10];
        c_mul(q_sub(q_mul(E[4], E[8]), q_mul(E[5], E[7])), E[0], d0);
        c_mul(q_sub(q_mul(E[3], E[8]), q_mul(E[5], E[6])), E[1], d1);
        c_mul(q_sub(q_mul(E[3], E[7]), q_mul(E[4], E[6])), E[2], d2);
        for (int m = 0; m < 10; m++) M[9][m] = d0[m] - d1[m] + d2[m];
    }
}

/* e5_matrix exported for the pin against the reference's own mblock.hpp (oracle/mblock_ref.cpp,
 * tests/test_oracle_essential.py): N = 4 x 9 null basis, M = 10 x 10 row-major */
void orc_e5_matrix(const double *N, double z, double *M) {
    double Nb[4][9], Mb[10][10];
    for (int i = 0; i < 4; i++)
        for (int k = 0; k < 9; k++) Nb[i][k] = N[9 * i + k];
    e5_matrix((const double(*)[9])Nb, z, Mb);
    for (int r = 0; r < 10; r++)
        for (int c = 0; c < 10; c++) M[10 * r + c] = Mb[r][c];
}

/* determinant by LU with partial pivoting (first maximal |pivot|) */
static double det10(double A[10][10]) {
    double det = 1.0;
    for (int k = 0; k < 10; k++) {
        int p = k;
        double best = fabs(A[k][k]);
        for (int i = k + 1; i < 10; i++)
            if (fabs(A[i][k]) > best) {
                best = fabs(A[i][k]);
                p = i;
            }
        if (A[p][k] == 0.0) return 0.0;
        if (p != k) {
            for (int j = 0; j < 10; j++) {
                double t = A[k][j];
                A[k][j] = A[p][j];
                A[p][j] = t;
            }
            det = -det;
        }
        for (int i = k + 1; i < 10; i++) {
            const double f = A[i][k] / A[k][k];
            for (int j = k + 1; j < 10; j++) A[i][j] -= f * A[k][j];
        }
    }
    for (int k = 0; k < 10; k++) det *= A[k][k];
    return det;
}

/* null vector of M(z) with v9 = 1 by elimination over columns 0..8; returns 0 if singular */
static int null10(double A[10][10], double *v) {
    for (int k = 0; k < 9; k++) {
        int p = k;
        double best = fabs(A[k][k]);
        for (int i = k + 1; i < 10; i++)
            if (fabs(A[i][k]) > best) {
                best = fabs(A[i][k]);
                p = i;
            }
        if (A[p][k] == 0.0) return 0;
        if (p != k)
            for (int j = 0; j < 10; j++) {
                double t = A[k][j];
                A[k][j] = A[p][j];
                A[p][j] = t;
            }
        for (int i = k + 1; i < 10; i++) {
            const double f = A[i][k] / A[k][k];
            for (int j = k + 1; j < 10; j++) A[i][j] -= f * A[k][j];
        }
    }
    v[9] = 1.0;
    for (int k = 8; k >= 0; k--) {
        double sum = A[k][9];
        for (int j = k + 1; j < 9; j++) sum += A[k][j] * v[j];
        v[k] = -sum / A[k][k];
    }
    return 1;
}

/* Horner with fused multiply-adds (fma: one IEEE rounding, as v_fma_f64 on the device) */
static double poly_eval(const double *c, int deg, double x) {
    double r = c[deg];
    for (int i = deg - 1; i >= 0; i--) r = fma(r, x, c[i]);
    return r;
}

/* Root refinement inside a sign-changing bracket (monotone there): safeguarded Newton in the
 * manner of rtsafe, started at the secant (regula falsi) point of the bracket -- a Newton
 * step when it stays strictly inside the bracket and at least halves the previous step
 * (|2f| <= |dxold f'|), else bisection; the bracket is tightened at every evaluation.  Stops
 * on an exact zero, a Newton step below 2^-50 |x| (the root to a few ulp; its end point is
 * taken when inside the bracket), an unsplittable bracket, or 200 evaluations.  p and p' by one fused Horner pass. */
static void poly_eval2(const double *c, int deg, double x, double *f, double *df) {
    double v = c[deg], d = 0.0;
    for (int j = deg - 1; j >= 0; j--) {
        d = fma(d, x, v);
        v = fma(v, x, c[j]);
    }
    *f = v;
    *df = d;
}

static double poly_refine(const double *c, int deg, double lo, double hi, double flo, double fhi) {
    double x = lo - flo * ((hi - lo) / (fhi - flo));
    if (!(x > lo && x < hi)) x = 0.5 * (lo + hi);
    double dxold = hi - lo, dx = dxold, f, df;
    poly_eval2(c, deg, x, &f, &df);
    for (int it = 0; it < 200; it++) {
        if (f == 0.0) return x;
        if ((f < 0.0) == (flo < 0.0)) {
            lo = x;
            flo = f;
        } else {
            hi = x;
        }
        const double step = f / df;
        const double xn = x - step;
        const int inside = xn > lo && xn < hi;
        if (xn == x || fabs(step) <= 0x1p-50 * fabs(x)) return inside ? xn : x;
        const int newton = inside && !(fabs(2.0 * f) > fabs(dxold * df));
        dxold = dx;
        if (newton) {
            dx = step;
            x = xn;
        } else {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) return mid;
            dx = mid - x;
            x = mid;
        }
        poly_eval2(c, deg, x, &f, &df);
    }
    return x;
}

/* root bound with IEEE operations only: the smallest r = 2^k (k >= 0) with
 * |a_n| r > sum_i |a_i| r^(i-n+1) (then no root has |z| >= r) */
static double root_bound(const double *a, int n) {
    double r = 1.0;
    const double an = fabs(a[n]);
    for (int it = 0; it < 2100; it++) {
        double t = fabs(a[0]);
        for (int i = 1; i < n; i++) t = t / r + fabs(a[i]);
        if (an * r > t) break;
        r = r * 2.0;
    }
    return r;
}

/* real roots of a[0] + a[1] z + ... + a[n] z^n, ascending (<= n): the solver's candidate values */
static int asc_real_roots(const double *a_in, int n, double *roots) {
    while (n > 0 && a_in[n] == 0.0) n--;
    if (n == 0) return 0;
    const double R = root_bound(a_in, n);
    /* level g works on the derivative of order n-g (degree g) and leaves exactly g points,
     * ascending: the root of each sign-changing interval, or the interval's left end as a
     * filler where it has none (fillers only split monotone intervals further, and keep the
     * per-level counts fixed) */
    double crit[10], next[10];
    int found[10] = {0};
    for (int g = 1; g <= n; g++) {
        const int d = n - g;
        double c[11];
        for (int j = 0; j <= g; j++) {
            double f = 1.0;
            for (int m = j + d; m > j; m--) f *= (double)m;
            c[j] = a_in[j + d] * f;
        }
        double lo = -R, flo = poly_eval(c, g, lo);
        for (int k = 0; k < g; k++) {
            const double hi = k < g - 1 ? crit[k] : R;
            const double fhi = poly_eval(c, g, hi);
            if (hi > lo && ((flo < 0.0) != (fhi < 0.0))) {
                next[k] = poly_refine(c, g, lo, hi, flo, fhi);
                found[k] = 1;
            } else {
                next[k] = lo;
                found[k] = 0;
            }
            lo = hi;
            flo = fhi;
        }
        for (int k = 0; k < g; k++) crit[k] = next[k];
    }
    int nr = 0;
    for (int k = 0; k < n; k++)
        if (found[k]) roots[nr++] = crit[k];
    return nr;
}


/* ---- 5-pt root step: the reference's Jenkins-Traub zeros, in the order it finds them.
 * Solve5PointEssential hands det M(z)'s coefficients to rpoly_ak1 (five_points.cpp:139-157;
 * usac/estimator/essential/rpoly.cpp:7-750, the akiti.ca C++ rendering of Jenkins & Traub's
 * RPOLY, ACM TOMS 493) and keeps the zeros whose imaginary part is exactly 0 in the order rpoly
 * deflates them; the first of those whose E passes cheirality is the model (:239-273).  So the
 * order is part of the result, and it is only reproducible by running the same iteration: it is
 * restated here operation for operation (same expression shapes, no FMA contraction,
 * correctly rounded division / sqrt).  rpoly's only library calls besides sqrt are log / exp in
 * its scaling factor and root bound (rpoly.cpp:82,98): glibc's are not correctly rounded
 * (measured here: exp differs from the correctly rounded value on ~7e-4 of arguments, log on
 * ~5e-6), so the restatement uses one portable correctly rounded pair (double-double series,
 * jt_log / jt_exp) that the device repeats bit for bit; where glibc's last bit differs, the bound
 * `bnd` -- only the start of the fixed shifts -- differs in its last bits and the zeros agree to
 * rounding (tests/test_oracle_essential.py pins the order and values against oracle/_ref's
 * compiled rpoly.cpp).  Safety caps the reference lacks: non-finite coefficients give no zeros
 * (the reference's bounded loops all fail on NaN, rpoly.cpp:214-220), and the bound's chop /
 * Newton loops stop after 2100 / 500 trips (they converge in a few dozen for any finite input). */
typedef struct {
    double hi, lo;
} jt_dd;

static jt_dd jt_sum(double a, double b) { /* exact a + b */
    const double s = a + b, bb = s - a;
    const jt_dd r = {s, (a - (s - bb)) + (b - bb)};
    return r;
}
static jt_dd jt_qsum(double a, double b) { /* exact a + b for |a| >= |b| */
    const double s = a + b;
    const jt_dd r = {s, b - (s - a)};
    return r;
}
static jt_dd jt_dadd(jt_dd x, jt_dd y) {
    jt_dd s = jt_sum(x.hi, y.hi);
    const jt_dd t = jt_sum(x.lo, y.lo);
    s.lo += t.hi;
    s = jt_qsum(s.hi, s.lo);
    s.lo += t.lo;
    return jt_qsum(s.hi, s.lo);
}
static jt_dd jt_dmul(jt_dd x, jt_dd y) {
    const double p = x.hi * y.hi;
    double e = fma(x.hi, y.hi, -p);
    e += x.hi * y.lo + x.lo * y.hi;
    return jt_qsum(p, e);
}
static jt_dd jt_inv(double k) { /* 1 / k as a double-double (k a small integer) */
    const double h = 1.0 / k;
    const jt_dd r = {h, fma(-h, k, 1.0) / k};
    return r;
}
static const jt_dd JT_LN2 = {0x1.62e42fefa39efp-1, 0x1.abc9e3b39803fp-56};

/* log x correctly rounded (x > 0 finite): x = m 2^e, m in [sqrt(1/2), sqrt 2), log m = 2 atanh s,
 * s = (m - 1) / (m + 1), the series in double-double (terms below 2^-60 in double) */
static double jt_log(double x) {
    if (!(x > 0.0) || isinf(x)) return x == 0.0 ? -INFINITY : (x > 0.0 ? x : NAN);
    int e;
    double m = frexp(x, &e);
    if (m < 0x1.6a09e667f3bcdp-1) {
        m *= 2.0;
        e--;
    }
    const double f = m - 1.0; /* exact */
    const jt_dd den = jt_sum(2.0, f);
    const double sh = f / den.hi;
    const double r = fma(-sh, den.hi, f) - sh * den.lo;
    const jt_dd s = jt_qsum(sh, r / den.hi);
    const jt_dd t = jt_dmul(s, s);
    double tail = 0.0;
    for (int k = 24; k >= 11; k--) tail = tail * t.hi + 1.0 / (double)(2 * k + 1);
    jt_dd P = {tail, 0.0};
    for (int k = 10; k >= 1; k--) P = jt_dadd(jt_dmul(P, t), jt_inv((double)(2 * k + 1)));
    const jt_dd one = {1.0, 0.0};
    P = jt_dadd(jt_dmul(P, t), one);
    jt_dd lm = jt_dmul(s, P);
    lm.hi *= 2.0;
    lm.lo *= 2.0;
    const jt_dd ed = {(double)e, 0.0};
    const jt_dd res = jt_dadd(jt_dmul(ed, JT_LN2), lm);
    return res.hi + res.lo;
}

/* exp y correctly rounded: y = k ln2 + r, |r| <= ln2 / 2, the Taylor series in double-double */
static double jt_exp(double y) {
    if (y != y) return y;
    if (y > 709.79) return INFINITY;
    if (y < -745.2) return 0.0;
    const double k = nearbyint(y / JT_LN2.hi);
    const jt_dd yk = {y, 0.0}, mk = {-k, 0.0};
    const jt_dd r = jt_dadd(yk, jt_dmul(mk, JT_LN2));
    double fact = 1.0, tail = 0.0;
    double inv[28];
    for (int n = 1; n < 28; n++) {
        fact *= (double)n;
        inv[n] = 1.0 / fact;
    }
    for (int n = 27; n >= 14; n--) tail = tail * r.hi + inv[n];
    jt_dd P = {tail, 0.0};
    fact = 1.0;
    for (int n = 1; n < 14; n++) fact *= (double)n;
    for (int n = 13; n >= 1; n--) { /* 1 / n! as a double-double: n! < 2^53 is exact */
        const jt_dd c = jt_inv(fact);
        P = jt_dadd(jt_dmul(P, r), c);
        fact /= (double)n;
    }
    const jt_dd one = {1.0, 0.0};
    P = jt_dadd(jt_dmul(P, r), one);
    return ldexp(P.hi + P.lo, (int)k);
}

/* the iteration's shared scalars: rpoly passes them between its routines by pointer */
typedef struct {
    int N, NN; /* degree and coefficient count of p (highest power first) */
    double p[11], K[11], qp[11], qk[11];
    double a, b, c, d, e, f, g, h, a1, a3, a7;
} jt_state;

/* QuadSD_ak1 (rpoly.cpp:378-394): q = src / (z^2 + u z + v); the last two running values -> *ra, *rb */
static void jt_divide(int nn, double u, double v, const double *src, double *q, double *ra, double *rb) {
    double bb = src[0], aa = src[1] - bb * u;
    q[0] = bb;
    q[1] = aa;
    for (int i = 2; i < nn; i++) {
        const double t = src[i] - (aa * u + bb * v);
        q[i] = t;
        bb = aa;
        aa = t;
    }
    *ra = aa;
    *rb = bb;
}

/* calcSC_ak1 (rpoly.cpp:396-435): 3 = the quadratic almost divides K; 2 / 1 = scaled by d / c */
static int jt_scalars(jt_state *s, double u, double v) {
    const int N = s->N;
    jt_divide(N, u, v, s->K, s->qk, &s->c, &s->d);
    if (fabs(s->c) <= 100.0 * DBL_EPSILON * fabs(s->K[N - 1]) && fabs(s->d) <= 100.0 * DBL_EPSILON * fabs(s->K[N - 2]))
        return 3;
    s->h = v * s->b;
    if (fabs(s->d) >= fabs(s->c)) {
        s->e = s->a / s->d;
        s->f = s->c / s->d;
        s->g = u * s->b;
        s->a3 = s->e * (s->g + s->a) + s->h * (s->b / s->d);
        s->a1 = s->f * s->b - s->a;
        s->a7 = s->h + (s->f + u) * s->a;
        return 2;
    }
    s->e = s->a / s->c;
    s->f = s->d / s->c;
    s->g = s->e * u;
    s->a3 = s->e * s->a + (s->g + s->h / s->c) * s->b;
    s->a1 = s->b - s->a * (s->d / s->c);
    s->a7 = s->g * s->d + s->h * s->f + s->a;
    return 1;
}

/* nextK_ak1 (rpoly.cpp:437-475) */
static void jt_next_k(jt_state *s, int type) {
    const int N = s->N;
    if (type == 3) {
        s->K[0] = s->K[1] = 0.0;
        for (int i = 2; i < N; i++) s->K[i] = s->qk[i - 2];
        return;
    }
    const double ref = type == 1 ? s->b : s->a;
    if (fabs(s->a1) > 10.0 * DBL_EPSILON * fabs(ref)) {
        s->a7 /= s->a1;
        s->a3 /= s->a1;
        s->K[0] = s->qp[0];
        s->K[1] = s->qp[1] - s->a7 * s->qp[0];
        for (int i = 2; i < N; i++) s->K[i] = (s->a3 * s->qk[i - 2] - s->a7 * s->qp[i - 1]) + s->qp[i];
    } else {
        s->K[0] = 0.0;
        s->K[1] = -s->a7 * s->qp[0];
        for (int i = 2; i < N; i++) s->K[i] = s->a3 * s->qk[i - 2] - s->a7 * s->qp[i - 1];
    }
}

/* newest_ak1 (rpoly.cpp:477-513): the next estimate (uu, vv) of the quadratic factor */
static void jt_newest(const jt_state *s, int type, double u, double v, double *uu, double *vv) {
    *uu = *vv = 0.0;
    if (type == 3) return;
    double a4, a5;
    if (type != 2) {
        a4 = (s->a + u * s->b) + s->h * s->f;
        a5 = s->c + (u + v * s->f) * s->d;
    } else {
        a4 = (s->a + s->g) * s->f + s->h;
        a5 = (s->f + u) * s->c + v * s->d;
    }
    const int N = s->N;
    const double b1 = -s->K[N - 1] / s->p[N];
    const double b2 = -(s->K[N - 2] + b1 * s->p[N - 1]) / s->p[N];
    const double c1 = v * b2 * s->a1, c2 = b1 * s->a7, c3 = b1 * b1 * s->a3;
    const double c4 = c1 - (c2 + c3);
    const double t = (a5 - c4) + b1 * a4;
    if (t != 0.0) {
        *uu = u - (u * (c3 + c2) + v * (b1 * s->a1 + b2 * s->a7)) / t;
        *vv = v * (1.0 + c4 / t);
    }
}

/* Quad_ak1 (rpoly.cpp:700-750): zeros of a z^2 + b1 z + c, (sr, si) and (lr, li) */
static void jt_quadratic(double a, double b1, double c, double *sr, double *si, double *lr, double *li) {
    *sr = *si = *lr = *li = 0.0;
    if (a == 0.0) {
        if (b1 != 0.0) *sr = -(c / b1);
        return;
    }
    if (c == 0.0) {
        *lr = -(b1 / a);
        return;
    }
    const double b = b1 / 2.0;
    double d, e;
    if (fabs(b) < fabs(c)) {
        e = c >= 0.0 ? a : -a;
        e = b * (b / fabs(c)) - e;
        d = sqrt(fabs(e)) * sqrt(fabs(c));
    } else {
        e = 1.0 - (a / b) * (c / b);
        d = sqrt(fabs(e)) * fabs(b);
    }
    if (e >= 0.0) {
        if (b >= 0.0) d = -d;
        *lr = (d - b) / a;
        if (*lr != 0.0) *sr = (c / *lr) / a;
    } else {
        *lr = *sr = -(b / a);
        *si = fabs(d / a);
        *li = -*si;
    }
}

/* QuadIT_ak1 (rpoly.cpp:515-607): variable-shift iteration for a quadratic factor from (uu, vv);
 * returns 2 (both zeros found, quotient in qp) or 0 */
static int jt_quad_iter(jt_state *s, double uu, double vv, double *szr, double *szi, double *lzr, double *lzi) {
    const int N = s->N, NN = s->NN;
    double u = uu, v = vv, relstp = 0.0, omp = 0.0, ui = 0.0, vi = 0.0;
    int j = 0, tried = 0;
    do {
        jt_quadratic(1.0, u, v, szr, szi, lzr, lzi);
        if (fabs(fabs(*szr) - fabs(*lzr)) > 0.01 * fabs(*lzr)) break;
        jt_divide(NN, u, v, s->p, s->qp, &s->a, &s->b);
        const double mp = fabs(s->a - *szr * s->b) + fabs(*szi * s->b);
        const double zm = sqrt(fabs(v));
        double ee = 2.0 * fabs(s->qp[0]);
        const double t = -(*szr * s->b);
        for (int i = 1; i < N; i++) ee = ee * zm + fabs(s->qp[i]);
        ee = ee * zm + fabs(s->a + t);
        ee = (9.0 * ee + 2.0 * fabs(t) - 7.0 * (fabs(s->a + t) + zm * fabs(s->b))) * DBL_EPSILON;
        if (mp <= 20.0 * ee) return 2;
        if (++j > 20) break;
        if (j >= 2 && relstp <= 0.01 && mp >= omp && !tried) { /* a cluster: five fixed shifts near it */
            relstp = relstp < DBL_EPSILON ? sqrt(DBL_EPSILON) : sqrt(relstp);
            u -= u * relstp;
            v += v * relstp;
            jt_divide(NN, u, v, s->p, s->qp, &s->a, &s->b);
            for (int i = 0; i < 5; i++) jt_next_k(s, jt_scalars(s, u, v));
            tried = 1;
            j = 0;
        }
        omp = mp;
        jt_next_k(s, jt_scalars(s, u, v));
        jt_newest(s, jt_scalars(s, u, v), u, v, &ui, &vi);
        if (vi != 0.0) {
            relstp = fabs((vi - v) / vi);
            u = ui;
            v = vi;
        }
    } while (vi != 0.0);
    return 0;
}

/* RealIT_ak1 (rpoly.cpp:609-698): variable-shift iteration for a real zero from *sx; returns 1
 * (zero found, quotient in qp) or 0, *flag = 1 (and *sx) asks for a quadratic iteration */
static int jt_real_iter(jt_state *s, double *sx, int *flag, double *szr, double *szi) {
    const int N = s->N, NN = s->NN;
    double x = *sx, t = 0.0, omp = 0.0;
    int j = 0;
    *flag = 0;
    for (;;) {
        double pv = s->p[0];
        s->qp[0] = pv;
        for (int i = 1; i < NN; i++) s->qp[i] = pv = pv * x + s->p[i];
        const double mp = fabs(pv), ms = fabs(x);
        double ee = 0.5 * fabs(s->qp[0]);
        for (int i = 1; i < NN; i++) ee = ee * ms + fabs(s->qp[i]);
        if (mp <= 20.0 * DBL_EPSILON * (2.0 * ee - mp)) {
            *szr = x;
            *szi = 0.0;
            return 1;
        }
        if (++j > 10) return 0;
        if (j >= 2 && fabs(t) <= 0.001 * fabs(x - t) && mp > omp) {
            *flag = 1;
            *sx = x;
            return 0;
        }
        omp = mp;
        double kv = s->K[0];
        s->qk[0] = kv;
        for (int i = 1; i < N; i++) s->qk[i] = kv = kv * x + s->K[i];
        if (fabs(kv) > fabs(s->K[N - 1]) * 10.0 * DBL_EPSILON) {
            const double tt = -(pv / kv);
            s->K[0] = s->qp[0];
            for (int i = 1; i < N; i++) s->K[i] = tt * s->qk[i - 1] + s->qp[i];
        } else {
            s->K[0] = 0.0;
            for (int i = 1; i < N; i++) s->K[i] = s->qk[i - 1];
        }
        kv = s->K[0];
        for (int i = 1; i < N; i++) kv = kv * x + s->K[i];
        t = fabs(kv) > fabs(s->K[N - 1]) * 10.0 * DBL_EPSILON ? -(pv / kv) : 0.0;
        x += t;
    }
}

/* Fxshfr_ak1 (rpoly.cpp:232-376): up to l2 fixed-shift steps with the quadratic z^2 + u z + v,
 * a variable-shift iteration once the s or v sequence converges; returns the zeros found */
static int jt_fixed_shift(jt_state *s, int l2, double sr, double v, double u, double *szr, double *szi, double *lzr,
                          double *lzi) {
    const int N = s->N;
    int iflag = 1, type;
    double betav = 0.25, betas = 0.25, oss = sr, ovv = v, ots = 0.0, otv = 0.0, ui = 0.0, vi = 0.0, xs = 0.0;
    double svk[11];
    jt_divide(s->NN, u, v, s->p, s->qp, &s->a, &s->b);
    type = jt_scalars(s, u, v);
    for (int j = 0; j < l2; j++) {
        int first = 1;
        jt_next_k(s, type);
        type = jt_scalars(s, u, v);
        jt_newest(s, type, u, v, &ui, &vi);
        const double vv = vi;
        const double ss = s->K[N - 1] != 0.0 ? -(s->p[N] / s->K[N - 1]) : 0.0;
        double tv = 1.0, ts = 1.0;
        if (j != 0 && type != 3) {
            if (vv != 0.0) tv = fabs((vv - ovv) / vv);
            if (ss != 0.0) ts = fabs((ss - oss) / ss);
            const double tvv = tv < otv ? tv * otv : 1.0;
            const double tss = ts < ots ? ts * ots : 1.0;
            const int vpass = tvv < betav, spass = tss < betas;
            if (spass || vpass) {
                memcpy(svk, s->K, sizeof(double) * (size_t)N);
                xs = ss;
                int stry = 0, vtry = 0;
                for (;;) {
                    const int linear_first = first && spass && (!vpass || tss < tvv);
                    first = 0;
                    if (!linear_first) {
                        const int nz = jt_quad_iter(s, ui, vi, szr, szi, lzr, lzi);
                        if (nz > 0) return nz;
                        iflag = vtry = 1;
                        betav *= 0.25;
                        if (stry || !spass) iflag = 0;
                        else memcpy(s->K, svk, sizeof(double) * (size_t)N);
                    }
                    if (iflag != 0) {
                        const int nz = jt_real_iter(s, &xs, &iflag, szr, szi);
                        if (nz > 0) return nz;
                        stry = 1;
                        betas *= 0.25;
                        if (iflag != 0) {
                            ui = -(xs + xs);
                            vi = xs * xs;
                            continue;
                        }
                    }
                    memcpy(s->K, svk, sizeof(double) * (size_t)N);
                    if (!vpass || vtry) break;
                }
                jt_divide(s->NN, u, v, s->p, s->qp, &s->a, &s->b);
                type = jt_scalars(s, u, v);
            }
        }
        ovv = vv;
        oss = ss;
        otv = tv;
        ots = ts;
    }
    return 0;
}

/* rpoly_ak1 (rpoly.cpp:7-230) on a[0..deg] (ascending powers; five_points.cpp:145-148 hands rpoly
 * the highest power first).  Writes the zeros in the order found; returns their number (deg, less
 * the ones not found after 20 shifts; 0 for a zero leading coefficient) */
static int jt_rpoly(const double *a, int deg, double *zr, double *zi) {
    const double cosr = -0x1.1db8f6d6a512ap-4, sinr = 0x1.fec0b7170fff6p-1; /* cos / sin (94 pi / 180), rpoly.cpp:14-18 */
    const double lo = DBL_MIN / DBL_EPSILON, lb2 = JT_LN2.hi;
    if (a[deg] == 0.0) return 0;
    for (int i = 0; i <= deg; i++)
        if (!isfinite(a[i])) return 0;
    jt_state s;
    int N = deg, found = 0;
    double xx = sqrt(0.5), yy = -xx;
    while (a[deg - N] == 0.0) { /* zeros at the origin */
        zr[found] = zi[found] = 0.0;
        N--;
        found++;
    }
    int NN = N + 1;
    for (int i = 0; i < NN; i++) s.p[i] = a[deg - i];
    while (N >= 1) {
        if (N <= 2) {
            if (N < 2) {
                zr[deg - 1] = -(s.p[1] / s.p[0]);
                zi[deg - 1] = 0.0;
            } else {
                jt_quadratic(s.p[0], s.p[1], s.p[2], &zr[deg - 2], &zi[deg - 2], &zr[deg - 1], &zi[deg - 1]);
            }
            return deg;
        }
        double mmax = 0.0, mmin = DBL_MAX;
        for (int i = 0; i < NN; i++) {
            const double x = fabs(s.p[i]);
            if (x > mmax) mmax = x;
            if (x != 0.0 && x < mmin) mmin = x;
        }
        double sc = lo / mmin;
        if ((sc <= 1.0 && mmax >= 10.0) || (sc > 1.0 && DBL_MAX / sc >= mmax)) {
            if (sc == 0.0) sc = DBL_MIN;
            const int l = (int)(jt_log(sc) / lb2 + 0.5);
            const double factor = ldexp(1.0, l); /* pow(2.0, l): exact */
            if (factor != 1.0)
                for (int i = 0; i < NN; i++) s.p[i] *= factor;
        }
        /* the lower bound of the zeros' moduli: the positive zero of |p0| z^N + ... - |pN| */
        double pt[11];
        for (int i = 0; i < NN; i++) pt[i] = fabs(s.p[i]);
        pt[N] = -pt[N];
        const int NM1 = N - 1;
        double x = jt_exp((jt_log(-pt[N]) - jt_log(pt[0])) / (double)N);
        if (pt[NM1] != 0.0) {
            const double xm = -pt[N] / pt[NM1];
            if (xm < x) x = xm;
        }
        double xm = x, ff = 0.0, df, dx;
        int trips = 0;
        do {
            x = xm;
            xm = 0.1 * x;
            ff = pt[0];
            for (int i = 1; i < NN; i++) ff = ff * xm + pt[i];
        } while (ff > 0.0 && ++trips < 2100);
        trips = 0;
        do {
            df = ff = pt[0];
            for (int i = 1; i < N; i++) {
                ff = x * ff + pt[i];
                df = x * df + ff;
            }
            ff = x * ff + pt[N];
            dx = ff / df;
            x -= dx;
        } while (fabs(dx / x) > 0.005 && ++trips < 500);
        const double bnd = x;
        /* K = p' / N, then five unshifted steps */
        for (int i = 1; i < N; i++) s.K[i] = (double)(N - i) * s.p[i] / (double)N;
        s.K[0] = s.p[0];
        const double aa = s.p[N], bb = s.p[NM1];
        int zerok = s.K[NM1] == 0.0;
        for (int jj = 0; jj < 5; jj++) {
            const double cc = s.K[NM1];
            if (zerok) {
                for (int j = NM1; j >= 1; j--) s.K[j] = s.K[j - 1];
                s.K[0] = 0.0;
                zerok = s.K[NM1] == 0.0;
            } else {
                const double t = -aa / cc;
                for (int j = NM1; j >= 1; j--) s.K[j] = t * s.K[j - 1] + s.p[j];
                s.K[0] = s.p[0];
                zerok = fabs(s.K[NM1]) <= fabs(bb) * DBL_EPSILON * 10.0;
            }
        }
        double saved[11];
        memcpy(saved, s.K, sizeof(double) * (size_t)N);
        s.N = N;
        s.NN = NN;
        int jj;
        for (jj = 1; jj <= 20; jj++) {
            /* a shift of modulus bnd, its amplitude rotated by 94 degrees from the last one */
            const double xr = cosr * xx - sinr * yy;
            yy = sinr * xx + cosr * yy;
            xx = xr;
            const double sr = bnd * xx, u = -(2.0 * sr);
            double szr, szi, lzr, lzi;
            const int nz = jt_fixed_shift(&s, 20 * jj, sr, bnd, u, &szr, &szi, &lzr, &lzi);
            if (nz != 0) {
                const int j = deg - N;
                zr[j] = szr;
                zi[j] = szi;
                NN -= nz;
                N = NN - 1;
                for (int i = 0; i < NN; i++) s.p[i] = s.qp[i];
                if (nz != 1) {
                    zr[j + 1] = lzr;
                    zi[j + 1] = lzi;
                }
                break;
            }
            memcpy(s.K, saved, sizeof(double) * (size_t)N);
        }
        if (jj > 20) return deg - N;
    }
    return deg;
}

/* real zeros (zero imaginary part) in rpoly's order (five_points.cpp:152-156) */
static int real_roots(const double *a, int n, double *roots) {
    double zr[10], zi[10];
    const int nz = jt_rpoly(a, n, zr, zi);
    int nr = 0;
    for (int k = 0; k < nz; k++)
        if (zi[k] == 0.0) roots[nr++] = zr[k];
    return nr;
}

static double det3d(const double P[3][4]) {
    return P[0][0] * (P[1][1] * P[2][2] - P[1][2] * P[2][1]) - P[0][1] * (P[1][0] * P[2][2] - P[1][2] * P[2][0]) +
           P[0][2] * (P[1][0] * P[2][1] - P[1][1] * P[2][0]);
}

/* CalcDepth (five_points.cpp:278-302) */
static double calc_depth(const double *X, const double P[3][4]) {
    double w = 0.0;
    for (int k = 0; k < 4; k++) w += P[2][k] * X[k];
    const double det = det3d(P);
    const double a = P[0][2], b = P[1][2], c = P[2][2];
    const double m3 = sqrt(a * a + b * b + c * c);
    const double sign = det > 0 ? 1.0 : -1.0;
    return (w / X[3]) * (sign / m3);
}

/* TriangulatePoint (five_points.cpp:304-334) with P1 = P_ref = [I|0].  The reference takes
 * the smallest right singular vector of the 4x4 DLT system.  A correspondence that satisfies
 * the epipolar constraint of E -- the five sample points do, up to rounding -- makes that
 * system rank 3, and its null vector lies on the first camera's ray: rows 0-1 give
 * X = (x1 s, y1 s, s, w) exactly, and (s, w) is the null vector of the remaining rank-1
 * 2x2 system, perpendicular to its larger row.  CalcDepth is scale- and sign-invariant in
 * X, so the depth signs are the reference's wherever they exceed the SVD's own rounding
 * noise -- at a few dozen operations instead of a 4x4 SVD. */
static void triangulate(double x1, double y1, double x2, double y2, const double P[3][4], double *X) {
    double b[2][2];
    for (int r = 0; r < 2; r++) {
        const double u = r == 0 ? x2 : y2;
        double row[4];
        for (int c = 0; c < 4; c++) row[c] = u * P[2][c] - P[r][c];
        b[r][0] = row[0] * x1 + row[1] * y1 + row[2];
        b[r][1] = row[3];
    }
    const double n0 = b[0][0] * b[0][0] + b[0][1] * b[0][1];
    const double n1 = b[1][0] * b[1][0] + b[1][1] * b[1][1];
    const int i = n0 >= n1 ? 0 : 1;
    const double sc = b[i][1], w = -b[i][0];
    X[0] = x1 * sc;
    X[1] = y1 * sc;
    X[2] = sc;
    X[3] = w;
}

/* ProjectionsFromEssential (five_points.cpp:336-371): P[j] = [R | t], R in {U W V^T, U W^T V^T},
 * t = +/- u3; U, V from the 3x3 SVD (rows Jacobi with accumulated rotations, singular values
 * descending, v3 = v1 x v2). */
static void projections(const double E[9], double P[4][3][4]) {
    double B[4][4], J[4][4];
    memset(B, 0, sizeof(B));
    memset(J, 0, sizeof(J));
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) B[i][k] = E[3 * i + k];
        J[i][i] = 1.0;
    }
    row_jacobi_small(B, 3, 3, J);
    double sg[3];
    for (int i = 0; i < 3; i++) {
        double a = 0.0;
        for (int k = 0; k < 3; k++) a += B[i][k] * B[i][k];
        sg[i] = sqrt(a);
    }
    int o[3] = {0, 1, 2};
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (sg[o[j]] > sg[o[i]]) {
                int t = o[i];
                o[i] = o[j];
                o[j] = t;
            }
    double U[3][3], V[3][3]; /* columns */
    for (int k = 0; k < 3; k++)
        for (int r = 0; r < 3; r++) U[r][k] = J[o[k]][r];
    for (int k = 0; k < 2; k++)
        for (int r = 0; r < 3; r++) V[r][k] = B[o[k]][r] / sg[o[k]];
    V[0][2] = V[1][0] * V[2][1] - V[2][0] * V[1][1];
    V[1][2] = V[2][0] * V[0][1] - V[0][0] * V[2][1];
    V[2][2] = V[0][0] * V[1][1] - V[1][0] * V[0][1];
    static const double Wm[3][3] = {{0, -1, 0}, {1, 0, 0}, {0, 0, 1}};
    for (int w = 0; w < 2; w++) {
        double T[3][3], R[3][3];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                double sum = 0.0;
                for (int k = 0; k < 3; k++) sum += U[r][k] * (w == 0 ? Wm[k][c] : Wm[c][k]);
                T[r][c] = sum;
            }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                double sum = 0.0;
                for (int k = 0; k < 3; k++) sum += T[r][k] * V[c][k];
                R[r][c] = sum;
            }
        for (int sgn = 0; sgn < 2; sgn++) {
            double(*Pj)[4] = P[2 * w + sgn];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) Pj[r][c] = R[r][c];
                Pj[r][3] = sgn == 0 ? U[r][2] : -U[r][2];
            }
        }
    }
}

/* steps 1-3: the null basis N of the five rows W (destroyed) and the degree-10 coefficients a
 * (ascending powers) of det M(z), interpolated at z = -5..5 (five_points.cpp:65-136) */
static void e5_poly(double W[9][9], double N[4][9], double a[11]) {
    double W0[5][9];
    memcpy(W0, W, sizeof(W0));
    if (!qr_null(W, 5, N)) {
        g_trace[ORC_TRACE_E5_FALLBACK]++;
        row_jacobi(W0, 5);
        null_complement(W0, 5, 4, N);
    }
    double Mz[10][10], dets[11], z[11];
    for (int k = 0; k < 11; k++) {
        z[k] = (double)(k - 5);
        e5_matrix((const double(*)[9])N, z[k], Mz);
        dets[k] = det10(Mz);
    }
    /* Newton divided differences, then monomial coefficients */
    double c[11];
    for (int k = 0; k < 11; k++) c[k] = dets[k];
    for (int j = 1; j < 11; j++)
        for (int i = 10; i >= j; i--) c[i] = (c[i] - c[i - 1]) / (z[i] - z[i - j]);
    for (int i = 0; i < 11; i++) a[i] = 0.0;
    a[0] = c[10];
    int deg = 0;
    for (int k = 9; k >= 0; k--) {
        a[deg + 1] = 0.0;
        for (int i = deg + 1; i >= 1; i--) a[i] = a[i - 1] - z[k] * a[i];
        a[0] = c[k] - z[k] * a[0];
        deg++;
    }
}

/* returns 1 and writes E (9 floats) when a root passes the cheirality test; with
 * cand != NULL every root's E (10 x 9) and cheirality flag are reported (test hook) */
static int essential_5pt_all(const orc_est *e, const int *sample, float *Eout, float *cand, int *cand_ok,
                             int *ncand) {
    double W[9][9];
    double p1[5][2], p2[5][2];
    for (int i = 0; i < 5; i++) {
        const float *p = e->pts + 4 * (size_t)sample[i];
        const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
        p1[i][0] = x1;
        p1[i][1] = y1;
        p2[i][0] = x2;
        p2[i][1] = y2;
        const double row[9] = {x1 * x2, x2 * y1, x2, x1 * y2, y1 * y2, y2, x1, y1, 1.0};
        for (int k = 0; k < 9; k++) W[i][k] = row[k];
    }
    double N[4][9], a[11], Mz[10][10];
    e5_poly(W, N, a);
    /* rpoly reports nothing for a zero leading coefficient or non-finite coefficients
     * (rpoly.cpp:224-227; its bounded loops all fail on NaN): no model */
    int fin = a[10] != 0.0;
    for (int i = 0; i <= 10; i++) fin = fin && isfinite(a[i]);
    if (!fin) return 0;
    double roots[10];
    const int nr = asc_real_roots(a, 10, roots);
    static const double Pref[3][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}};
    float Ec[10][9];
    int pass[10], npass = 0;
    for (int r = 0; r < nr; r++) {
        pass[r] = 0;
        const double zz = roots[r];
        e5_matrix((const double(*)[9])N, zz, Mz);
        double v[10];
        if (!null10(Mz, v)) continue;
        const double x = v[7], y = v[8];
        double E[9];
        for (int k = 0; k < 9; k++) E[k] = N[0][k] * x + N[1][k] * y + N[2][k] * zz + N[3][k];
        double P[4][3][4];
        projections(E, P);
        int found = 0;
        for (int j = 0; j < 4 && !found; j++) {
            double X[4];
            triangulate(p1[0][0], p1[0][1], p2[0][0], p2[0][1], P[j], X);
            if (!(calc_depth(X, Pref) > 0 && calc_depth(X, P[j]) > 0)) continue;
            int inl = 1;
            for (int k = 1; k < 5; k++) {
                triangulate(p1[k][0], p1[k][1], p2[k][0], p2[k][1], P[j], X);
                if (calc_depth(X, Pref) > 0 && calc_depth(X, P[j]) > 0) inl++;
            }
            if (inl >= 5) found = 1;
        }
        for (int k = 0; k < 9; k++) Ec[r][k] = (float)E[k];
        pass[r] = found;
        npass += found;
        if (cand) {
            for (int k = 0; k < 9; k++) cand[9 * *ncand + k] = (float)E[k];
            cand_ok[*ncand] = found;
            (*ncand)++;
        }
    }
    if (cand || npass == 0) return 0;
    /* five_points.cpp:239-273 keeps the first candidate in rpoly's order that passes cheirality
     * (with 5 points "found" needs all 5 in front, so the first found has the most and a later one
     * never replaces it).  With one passing candidate the order does not matter; with several, the
     * reference's order is the Jenkins-Traub restatement's (jt_rpoly: rpoly.cpp's zeros in the order
     * it deflates them): its real zeros are taken in that order, each stands for the candidate value
     * nearest to it (first on ties), and the first whose candidate passes wins -- the reference's
     * loop with each zero's model the candidate's.  No such zero (rpoly reports none, or only zeros
     * of failing candidates before a 20-shift failure): the first passing candidate ascending. */
    int best = -1;
    for (int r = 0; r < nr && best < 0; r++)
        if (pass[r] && npass == 1) best = r;
    if (npass > 1) {
        double z[10];
        const int nz = real_roots(a, 10, z);
        for (int j = 0; j < nz && best < 0; j++) {
            int near = -1;
            double dmin = INFINITY;
            for (int r = 0; r < nr; r++) {
                const double d = fabs(z[j] - roots[r]);
                if (d < dmin) {
                    dmin = d;
                    near = r;
                }
            }
            if (near >= 0 && pass[near]) best = near;
        }
        for (int r = 0; r < nr && best < 0; r++)
            if (pass[r]) best = r;
    }
    for (int k = 0; k < 9; k++) Eout[k] = Ec[best][k];
    return 1;
}

static int essential_5pt(const orc_est *e, const int *sample, float *Eout) {
    return essential_5pt_all(e, sample, Eout, NULL, NULL, NULL);
}

int orc_e5_candidates(orc_est *e, const int *sample, float *cand, int *cand_ok) {
    int n = 0;
    float dummy[9];
    essential_5pt_all(e, sample, dummy, cand, cand_ok, &n);
    return n;
}

/* EssentialEstimator::GetError (essential_estimator.hpp:76-107): mean of the two
 * point-to-epipolar-line distances, fp32 (sqrt of a float: C double sqrt, rounded). */
static inline float essential_error(const orc_est *e, unsigned int pidx) {
    const float *p = e->pts + 4 * (size_t)pidx;
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    const float *E = e->f;
    const float l1 = E[0] * x2 + E[3] * y2 + E[6];
    const float l2 = E[1] * x2 + E[4] * y2 + E[7];
    const float l3 = E[2] * x2 + E[5] * y2 + E[8];
    const float t1 = E[0] * x1 + E[1] * y1 + E[2];
    const float t2 = E[3] * x1 + E[4] * y1 + E[5];
    const float t3 = E[6] * x1 + E[7] * y1 + E[8];
    const float a1 = l1 * x1 + l2 * y1 + l3;
    const float a2 = (float)sqrt((double)(l1 * l1 + l2 * l2));
    const float b1 = t1 * x2 + t2 * y2 + t3;
    const float b2 = (float)sqrt((double)(t1 * t1 + t2 * t2));
    return (fabsf(a1 / a2) + fabsf(b1 / b2)) / 2;
}

/* test hook: the real zeros of a polynomial (ascending powers, degree <= 10) in rpoly's order */
int orc_real_roots(const double *a, int n, double *roots) { return real_roots(a, n, roots); }

/* test hook: the solver's candidate values, the real roots ascending */
int orc_asc_roots(const double *a, int n, double *roots) { return asc_real_roots(a, n, roots); }

/* test hook: every zero rpoly_ak1 reports (its order; returns their number) */
int orc_rpoly_zeros(const double *a, int n, double *zr, double *zi) { return n >= 1 && n <= 10 ? jt_rpoly(a, n, zr, zi) : -1; }

/* test hook: the portable correctly rounded log / exp of the restatement */
double orc_jt_log(double x) { return jt_log(x); }
double orc_jt_exp(double y) { return jt_exp(y); }

/* test hook: the degree-10 polynomial det M(z) of an essential sample (ascending powers), the
 * input of the root step -- pinned against the reference's rpoly_ak1 (oracle/rpoly_ref.cpp) */
void orc_e5_poly(orc_est *e, const int *sample, double *a) {
    double W[9][9];
    for (int i = 0; i < 5; i++) {
        const float *p = e->pts + 4 * (size_t)sample[i];
        const double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
        const double row[9] = {x1 * x2, x2 * y1, x2, x1 * y2, y1 * y2, y2, x1, y1, 1.0};
        for (int k = 0; k < 9; k++) W[i][k] = row[k];
    }
    double N[4][9];
    e5_poly(W, N, a);
}

int orc_est_estimate(orc_est *e, const int *sample, float *models) {
    if (e->kind == ORC_LINE2D) return line2d_estimate(e, sample, models);
    if (e->kind == ORC_FUNDAMENTAL) return fundamental_7pt(e, sample, models);
    if (e->kind == ORC_ESSENTIAL) return essential_5pt(e, sample, models);
    return homography_dlt4(e, sample, models);
}

int orc_est_nonminimal(orc_est *e, const int *sample, unsigned int n, float *model) {
    if (e->kind == ORC_LINE2D) return line2d_nonminimal(e, sample, n, model);
    if (e->kind == ORC_FUNDAMENTAL || e->kind == ORC_ESSENTIAL) return fundamental_8pt(e, sample, n, NULL, model);
    return homography_normalized_dlt(e, sample, n, NULL, model);
}

/* Estimator::EstimateModelNonMinimalSample(sample, n, weights, model) (estimator.hpp:26):
 * homography_estimator.hpp:69-77 (weighted NormalizedDLT, normalized_dlt.cpp:25-36) and
 * fundamental_estimator.hpp:78-86 (weighted EightPointsAlgorithm, eight_points.cpp:176-228);
 * the other estimators inherit the base's "NOT IMPLEMENTED": -1. */
int orc_est_nonminimal_weighted(orc_est *e, const int *sample, unsigned int n, const float *weights, float *model) {
    if (e->kind == ORC_FUNDAMENTAL) return fundamental_8pt(e, sample, n, weights, model);
    if (e->kind == ORC_HOMOGRAPHY) return homography_normalized_dlt(e, sample, n, weights, model);
    return -1;
}

/* test hook: the cubic solver spec */
int orc_cubic_roots(double c0, double c1, double c2, double c3, double *roots) {
    return cubic_roots(c0, c1, c2, c3, roots);
}

void orc_est_set_model(orc_est *e, const float *m) {
    if (e->kind == ORC_LINE2D) {
        e->a = m[0];
        e->b = m[1];
        e->c = m[2];
    } else if (e->kind == ORC_FUNDAMENTAL || e->kind == ORC_ESSENTIAL) {
        memcpy(e->f, m, sizeof(float) * 9);
    } else {
        memcpy(e->h, m, sizeof(float) * 9);
        orc_inv3x3(m, e->hi);
    }
}

/* HomographyEstimator::GetError (homography_estimator.hpp:85-110): symmetric transfer
 * error; fp32 projections (no z guard: SURVEY Q19), the two distances are double
 * sqrt()s summed in double and rounded to float, then halved. */
static inline float homography_error(const orc_est *e, unsigned int pidx) {
    const float *p = e->pts + 4 * (size_t)pidx;
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    const float *h = e->h, *hi = e->hi;
    float ex2 = h[0] * x1 + h[1] * y1 + h[2];
    float ey2 = h[3] * x1 + h[4] * y1 + h[5];
    float ez2 = h[6] * x1 + h[7] * y1 + h[8];
    ex2 /= ez2;
    ey2 /= ez2;
    float ex1 = hi[0] * x2 + hi[1] * y2 + hi[2];
    float ey1 = hi[3] * x2 + hi[4] * y2 + hi[5];
    float ez1 = hi[6] * x2 + hi[7] * y2 + hi[8];
    ex1 /= ez1;
    ey1 /= ez1;
    float d2 = (x2 - ex2) * (x2 - ex2) + (y2 - ey2) * (y2 - ey2);
    float d1 = (x1 - ex1) * (x1 - ex1) + (y1 - ey1) * (y1 - ey1);
    float error = (float)(sqrt((double)d2) + sqrt((double)d1));
    return error / 2;
}

/* Line2DEstimator::GetError (line2d_estimator.hpp:154-156) */
static inline float line2d_error(const orc_est *e, unsigned int pidx) {
    const float *p = e->pts + 2 * (size_t)pidx;
    return fabsf(e->a * p[0] + e->b * p[1] + e->c);
}

float orc_est_error(const orc_est *e, unsigned int pidx) {
    if (e->kind == ORC_LINE2D) return line2d_error(e, pidx);
    if (e->kind == ORC_FUNDAMENTAL) return fundamental_error(e, pidx);
    if (e->kind == ORC_ESSENTIAL) return essential_error(e, pidx);
    return homography_error(e, pidx);
}

/* ------------------------------------------------------------ quality */
/* Quality::getNumberInliers (quality.hpp:60-101): points in order; err < thr strict;
 * Σ err sequential fp32. */
void orc_quality(orc_est *e, const float *model, float thr, int *count, float *sum, int *inliers) {
    orc_est_set_model(e, model);
    int cnt = 0;
    float s = 0.f;
    if (e->kind == ORC_LINE2D) {
        for (unsigned int p = 0; p < e->n; p++) {
            float err = line2d_error(e, p);
            if (err < thr) {
                if (inliers) inliers[cnt] = (int)p;
                cnt++;
                s += err;
            }
        }
    } else if (e->kind == ORC_FUNDAMENTAL || e->kind == ORC_ESSENTIAL) {
        const int ess = e->kind == ORC_ESSENTIAL;
        for (unsigned int p = 0; p < e->n; p++) {
            float err = ess ? essential_error(e, p) : fundamental_error(e, p);
            if (err < thr) {
                if (inliers) inliers[cnt] = (int)p;
                cnt++;
                s += err;
            }
        }
    } else {
        for (unsigned int p = 0; p < e->n; p++) {
            float err = homography_error(e, p);
            if (err < thr) {
                if (inliers) inliers[cnt] = (int)p;
                cnt++;
                s += err;
            }
        }
    }
    *count = cnt;
    *sum = s;
}

void orc_score_models(orc_est *e, const float *models, int n_models, float thr, int *counts, float *sums) {
    for (int i = 0; i < n_models; i++) orc_quality(e, models + 9 * (size_t)i, thr, &counts[i], &sums[i], NULL);
}

/* models: n_samples x (9 * max_models) floats (max_models = 3 for F, else 1) */
void orc_estimate_batch(orc_est *e, const int *samples, int n_samples, float *models, int *n_models) {
    int m = orc_est_sample_size(e), km = orc_est_max_models(e);
    for (int i = 0; i < n_samples; i++)
        n_models[i] = orc_est_estimate(e, samples + (size_t)i * m, models + 9 * (size_t)km * i);
}

/* dataset/GetImage.h:209-231: Quality::getInliers with the model and with model.inv(),
 * keep the larger. */
int orc_gt_inliers_homography(const float *points, unsigned int n, const float *model, float thr) {
    orc_est *e = orc_est_new(ORC_HOMOGRAPHY, points, n, ORC_DLT_THIN);
    int c1, c2;
    float s;
    float inv[9];
    orc_quality(e, model, thr, &c1, &s, NULL);
    orc_inv3x3(model, inv);
    orc_quality(e, inv, thr, &c2, &s, NULL);
    orc_est_free(e);
    return c2 > c1 ? c2 : c1;
}

/* ------------------------------------------------------------ termination */
/* StandardTerminationCriteria (standard_termination_criteria.hpp:24-31, 52-62):
 * log_1_p = (float) log(1 - p) (double log), fp32 inlier ratio power, EPSILON 0.0005f,
 * k = log_1_p / log(1 - q) in double, truncated to unsigned. */
unsigned int orc_std_termination(unsigned int inliers, unsigned int points_size, unsigned int sample_size,
                                 float desired_prob, unsigned int max_iterations) {
    float log_1_p = (float)log((double)(1 - desired_prob));
    float inl_ratio = (float)inliers / (float)points_size;
    float inl_prob = inl_ratio * inl_ratio;
    int k = (int)sample_size;
    while (k > 2) {
        inl_prob *= inl_ratio;
        k--;
    }
    if (inl_prob < 0.0005f) return max_iterations;
    double r = (double)log_1_p / log((double)(1 - inl_prob));
    return (unsigned int)r;
}

/* ------------------------------------------------------------ mt19937 / PROSAC */
/* std::mt19937 (the PROSAC generator, uniform_random_generator.hpp:16-26).  The reference
 * seeds it from std::random_device (non-reproducible); this build seeds it with the run
 * seed.  uniform_int_distribution<int>(0, max) is restated as libstdc++'s classic
 * downscaling (GCC <= 10, the toolchain of the reference's era): scaling = 0xFFFFFFFF /
 * (max + 1), reject r >= (max + 1) * scaling, return r / scaling. */
void orc_mt_seed(orc_mt *g, uint32_t seed) {
    g->mt[0] = seed;
    for (int i = 1; i < 624; i++) g->mt[i] = 1812433253u * (g->mt[i - 1] ^ (g->mt[i - 1] >> 30)) + (uint32_t)i;
    g->i = 624;
}

uint32_t orc_mt_next(orc_mt *g) {
    if (g->i >= 624) {
        for (int k = 0; k < 624; k++) {
            uint32_t y = (g->mt[k] & 0x80000000u) | (g->mt[(k + 1) % 624] & 0x7fffffffu);
            g->mt[k] = g->mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        g->i = 0;
    }
    uint32_t y = g->mt[g->i++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

int orc_mt_uniform(orc_mt *g, unsigned int max) {
    const uint64_t urngrange = 0xFFFFFFFFull, urange = (uint64_t)max;
    if (urange == urngrange) return (int)orc_mt_next(g);
    const uint64_t uerange = urange + 1, scaling = urngrange / uerange, past = uerange * scaling;
    uint64_t r;
    do {
        r = orc_mt_next(g);
    } while (r >= past);
    return (int)(r / scaling);
}

/* UniformRandomGenerator::generateUniqueRandomSet(sample, k, max): closed <0; max>,
 * redraw on a repeat (uniform_random_generator.hpp:44-54) */
static void mt_unique_set(orc_mt *g, int *sample, unsigned int k, unsigned int max) {
    for (unsigned int i = 0; i < k; i++) {
        sample[i] = orc_mt_uniform(g, max);
        for (int j = (int)i - 1; j >= 0; j--) {
            if (sample[i] == sample[j]) {
                i--;
                break;
            }
        }
    }
}

struct orc_prosac {
    orc_mt g;
    unsigned int *growth;
    unsigned int subset, largest, hyp, m, n, growth_max;
    unsigned int term_len; /* = ProsacTerminationCriteria::termination_length (shared pointer) */
};

/* ProsacSampler::initProsacSampler (prosac_sampler.hpp:62-114) */
orc_prosac *orc_prosac_new(unsigned int sample_size, unsigned int points_size, uint32_t seed) {
    orc_prosac *p = (orc_prosac *)calloc(1, sizeof(*p));
    p->m = sample_size;
    p->n = points_size;
    p->growth_max = 200000;
    orc_mt_seed(&p->g, seed);
    p->growth = (unsigned int *)malloc(sizeof(unsigned int) * points_size);
    double T_n = p->growth_max;
    for (unsigned int i = 0; i < sample_size; ++i) T_n *= (double)(sample_size - i) / (points_size - i);
    unsigned int T_n_prime = 1;
    for (unsigned int i = 0; i < points_size; ++i) {
        if (i + 1 <= sample_size) {
            p->growth[i] = T_n_prime;
            continue;
        }
        double Tn_plus1 = (double)(i + 1) * T_n / (i + 1 - sample_size);
        p->growth[i] = T_n_prime + (unsigned int)ceil(Tn_plus1 - T_n);
        T_n = Tn_plus1;
        T_n_prime = p->growth[i];
    }
    p->largest = sample_size;
    p->subset = sample_size;
    p->hyp = 1;
    p->term_len = points_size;
    return p;
}

void orc_prosac_free(orc_prosac *p) {
    if (!p) return;
    free(p->growth);
    free(p);
}

const unsigned int *orc_prosac_growth(const orc_prosac *p) { return p->growth; }
unsigned int orc_prosac_largest(const orc_prosac *p) { return p->largest; }
void orc_prosac_set_term_len(orc_prosac *p, unsigned int t) { p->term_len = t; }

/* ProsacSampler::generateSample (prosac_sampler.hpp:117-172).  Reference quirks kept:
 * both uniform fall-backs draw from the CLOSED range <0; max>. */
void orc_prosac_sample(orc_prosac *p, int *sample) {
    if (p->hyp > p->growth_max) {
        mt_unique_set(&p->g, sample, p->m, p->n);
        return;
    }
    if (p->subset > p->term_len) {
        mt_unique_set(&p->g, sample, p->m, p->term_len);
        return;
    }
    if (p->hyp > p->growth[p->subset - 1]) {
        ++p->subset;
        if (p->subset > p->n) p->subset = p->n;
        if (p->largest < p->subset) p->largest = p->subset;
    }
    mt_unique_set(&p->g, sample, p->m - 1, p->subset - 2);
    sample[p->m - 1] = (int)p->subset - 1;
    p->hyp++;
}

struct orc_prosac_term {
    unsigned int *maximality, *non_random;
    const unsigned int *growth;
    unsigned int term_len, n, m, max_iters;
    float desired_prob;
};

/* ProsacTerminationCriteria ctor (prosac_termination_criteria.hpp:44-119) */
orc_prosac_term *orc_prosac_term_new(const unsigned int *growth, unsigned int points_size, unsigned int sample_size,
                                     float desired_prob, unsigned int max_iterations) {
    orc_prosac_term *t = (orc_prosac_term *)calloc(1, sizeof(*t));
    t->growth = growth;
    t->n = points_size;
    t->m = sample_size;
    t->max_iters = max_iterations;
    t->desired_prob = desired_prob;
    t->term_len = points_size;
    const float non_randomness = 0.95f, beta = 0.05f;
    t->non_random = (unsigned int *)calloc(points_size, sizeof(unsigned int));
    double *pn = (double *)malloc(sizeof(double) * points_size);
    for (size_t n = sample_size + 1; n <= points_size; ++n) {
        if (n - 1 > 1000) {
            t->non_random[n - 1] = t->non_random[n - 2];
            continue;
        }
        memset(pn, 0, sizeof(double) * points_size);
        pn[sample_size] = (beta)*pow((double)1 - beta, (double)n - sample_size - 1) * (n - sample_size);
        double pn_i = pn[sample_size];
        for (size_t i = sample_size + 2; i <= n; ++i) {
            if (i == n) {
                pn[n - 1] = pow((double)beta, (double)n - sample_size);
                break;
            }
            pn[i - 1] = pn_i * ((beta) / (1 - beta)) * ((double)(n - i) / (i - sample_size + 1));
            pn_i = pn[i - 1];
        }
        double acc = 0.0;
        unsigned int i_min = 0;
        for (size_t i = n; i >= sample_size + 1; --i) {
            acc += pn[i - 1];
            if (acc < 1 - non_randomness) i_min = (unsigned int)i;
            else break;
        }
        t->non_random[n - 1] = i_min;
    }
    free(pn);
    t->maximality = (unsigned int *)malloc(sizeof(unsigned int) * points_size);
    for (size_t i = 0; i < points_size; ++i) t->maximality[i] = 10000; /* max_hypotheses, :62 */
    return t;
}

void orc_prosac_term_free(orc_prosac_term *t) {
    if (!t) return;
    free(t->maximality);
    free(t->non_random);
    free(t);
}

unsigned int orc_prosac_term_length(const orc_prosac_term *t) { return t->term_len; }

/* ProsacTerminationCriteria::getUpBoundIterations(hypCount, model)
 * (prosac_termination_criteria.hpp:148-201) over the model's inlier flags of the sorted
 * points (flags[i] = GetError(i) < threshold); largest = the sampler's largest_sample_size
 * at the call.  Mutates non_random (reference quirk) and maximality. */
unsigned int orc_prosac_term_update(orc_prosac_term *t, unsigned int hypCount, const unsigned char *flags,
                                    unsigned int largest) {
    const unsigned int min_len = 20;
    unsigned int max_samples = t->maximality[t->term_len - 1];
    unsigned int inlier_count = 0;
    for (unsigned int i = 0; i < min_len; i++) inlier_count += flags[i];
    int in_next = 0, in_i = flags[min_len];
    for (unsigned int i = min_len; i < t->n; ++i) {
        if (i != t->n - 1) in_next = flags[i + 1];
        inlier_count += (unsigned int)in_i;
        if (t->non_random[i] < inlier_count) {
            t->non_random[i] = inlier_count;
            if ((i == t->n - 1) || (in_i && !in_next)) {
                unsigned int new_samples = orc_std_termination(inlier_count, i + 1, t->m, t->desired_prob, t->max_iters);
                if (i + 1 < largest) new_samples += hypCount - t->growth[i];
                if (new_samples < t->maximality[i]) {
                    t->maximality[i] = new_samples;
                    if ((new_samples < max_samples) || ((new_samples == max_samples) && (i + 1 >= t->term_len))) {
                        t->term_len = i + 1;
                        max_samples = new_samples;
                    }
                }
            }
        }
        in_i = in_next;
    }
    return max_samples;
}

/* ------------------------------------------------------------ SPRT */
typedef struct {
    double epsilon, delta, A;
    int k;
} sprt_hist;

struct orc_sprt {
    unsigned int *pool;
    unsigned int idx, n, m, max_iters, cur;
    int last_update, max_before;
    double t_M, m_S;
    sprt_hist *h;
    unsigned int nh, caph;
};

/* SPRT::estimateThresholdA (sprt.hpp:332-355) */
static double sprt_threshold_A(const orc_sprt *s, double epsilon, double delta) {
    double C = (1 - delta) * log((1 - delta) / (1 - epsilon)) + delta * (log(delta / epsilon));
    double K = (s->t_M * C) / s->m_S + 1;
    double An_1 = K, An = K;
    for (unsigned int i = 0; i < 10; ++i) {
        An = K + log(An_1);
        if (fabs(An - An_1) < 1.5e-8) break;
        An_1 = An;
    }
    return An;
}

static void sprt_push(orc_sprt *s, double eps, double delta, double A, int k) {
    if (s->nh == s->caph) {
        s->caph = s->caph ? 2 * s->caph : 16;
        s->h = (sprt_hist *)realloc(s->h, sizeof(sprt_hist) * s->caph);
    }
    s->h[s->nh].epsilon = eps;
    s->h[s->nh].delta = delta;
    s->h[s->nh].A = A;
    s->h[s->nh].k = k;
    s->nh++;
}

/* Point order of the SPRT test in the revision that wrote results/line2d/uniform_001.csv (test
 * switch, off by default = the current sprt.hpp).  That revision's harness header predates the
 * current store_results_line2d (test_line2d_fitting.cpp:146-154 writes "LO = ", the CSV has
 * "Standard LO / Graph Cut LO"), and its published SPRT statistics are reproduced -- under the
 * harness's time(NULL) seeding, tests/test_reference_statistics.py -- only when every model
 * is tested on the points in file order from point 0 (no random pool, no rolling index): the
 * line2d files hold their inliers last, so the true line is often rejected on the outlier
 * prefix, which is what made those runs longer and their results worse than without SPRT. */
static int g_sprt_file_order = 0;
void orc_set_sprt_file_order(int on) { g_sprt_file_order = on; }

/* SPRT ctor (sprt.hpp:89-175): the pool shuffle consumes points_size random() draws from
 * the shared glibc stream; per-estimator (epsilon0, delta0, t_M, m_S). */
orc_sprt *orc_sprt_new(int kind, unsigned int points_size, unsigned int sample_size, unsigned int max_iterations,
                       int max_hypothesis_test_before_sprt) {
    orc_sprt *s = (orc_sprt *)calloc(1, sizeof(*s));
    s->n = points_size;
    s->m = sample_size;
    s->max_iters = max_iterations;
    s->max_before = max_hypothesis_test_before_sprt;
    s->pool = (unsigned int *)malloc(sizeof(unsigned int) * points_size);
    for (unsigned int i = 0; i < points_size; i++) s->pool[i] = i;
    int max = (int)points_size;
    for (unsigned int i = 0; i < points_size && !g_sprt_file_order; i++) {
        unsigned int r = (unsigned int)random() % (unsigned int)max;
        unsigned int tmp = s->pool[r];
        max--;
        s->pool[r] = s->pool[max];
        s->pool[max] = tmp;
    }
    s->idx = 0;
    double eps0, delta0;
    if (kind == ORC_HOMOGRAPHY) {
        delta0 = 0.01; eps0 = 0.1; s->t_M = 200; s->m_S = 1;
    } else if (kind == ORC_FUNDAMENTAL) {
        delta0 = 0.05; eps0 = 0.2; s->t_M = 200; s->m_S = 2.48;
    } else if (kind == ORC_ESSENTIAL) {
        delta0 = 0.05; eps0 = 0.2; s->t_M = 300; s->m_S = 4;
    } else {
        delta0 = 0.0001; eps0 = 0.001; s->t_M = 100; s->m_S = 1;
    }
    sprt_push(s, eps0, delta0, sprt_threshold_A(s, eps0, delta0), 0);
    s->cur = 0;
    s->last_update = 0;
    return s;
}

void orc_sprt_free(orc_sprt *s) {
    if (!s) return;
    free(s->pool);
    free(s->h);
    free(s);
}

const unsigned int *orc_sprt_pool(const orc_sprt *s) { return s->pool; }
double orc_sprt_A(const orc_sprt *s) { return s->h[s->cur].A; }
unsigned int orc_sprt_histories(const orc_sprt *s) { return s->nh; }

/* SPRT::verifyModelAndGetModelScore (sprt.hpp:191-317) with the model already set in e.
 * Returns good (1/0); writes (count, score) when the reference writes them. */
int orc_sprt_verify(orc_sprt *s, orc_est *e, float thr, int current_hypothese, unsigned int maximum_score,
                    int *count, float *score, unsigned int *tested_out) {
    const double epsilon = s->h[s->cur].epsilon, delta = s->h[s->cur].delta, A = s->h[s->cur].A;
    double lambda_new, lambda = 1;
    unsigned int tested_point = 0, tested_inliers = 0;
    int good = 1;
    if (g_sprt_file_order) s->idx = 0;
    for (tested_point = 0; tested_point < s->n; tested_point++) {
        if (s->idx >= s->n) s->idx = 0;
        if (orc_est_error(e, s->pool[s->idx]) < thr) {
            tested_inliers++;
            lambda_new = lambda * (delta / epsilon);
        } else {
            lambda_new = lambda * ((1 - delta) / (1 - epsilon));
        }
        s->idx++;
        if (lambda_new > A) {
            good = 0;
            tested_point++;
            break;
        }
        lambda = lambda_new;
    }
    if (good) {
        *count = (int)tested_inliers;
        *score = (float)*count;
    } else if (current_hypothese < s->max_before) {
        unsigned int after = 0;
        for (unsigned int p = tested_point; p < s->n; p++) {
            if (s->idx >= s->n) s->idx = 0;
            if (orc_est_error(e, s->pool[s->idx]) < thr) after++;
            s->idx++;
        }
        *count = (int)(tested_inliers + after);
        *score = (float)*count;
    }
    if (tested_out) *tested_out = tested_point;
    if (good) {
        if (tested_inliers > maximum_score) {
            const double eps_new = (float)tested_inliers / s->n;
            sprt_push(s, eps_new, delta, sprt_threshold_A(s, eps_new, delta), current_hypothese - s->last_update);
            s->last_update = current_hypothese;
            s->cur++;
        }
    } else {
        const float delta_est = (float)tested_inliers / tested_point;
        if (delta_est > 0 && fabs(delta - delta_est) / delta > 0.05) {
            sprt_push(s, epsilon, delta_est, sprt_threshold_A(s, epsilon, delta_est), current_hypothese - s->last_update);
            s->last_update = current_hypothese;
            s->cur++;
        }
    }
    return good;
}

/* The throughput SPRT's test of one model (the loop of sprt.hpp:209-234 with a fixed epsilon, delta,
 * A -- the batch's -- and a given pool start instead of the rolling index; no history update):
 * lambda in fp64 as the reference multiplies it.  K models (K x 9), starts[k] = model k's first pool
 * position; good[k], count[k] = inliers over all points when good (-1 when rejected), tested[k] =
 * points read (nullable). */
void orc_sprt_fixed_batch(orc_est *e, const unsigned int *pool, unsigned int n, float thr, const float *models,
                          const unsigned int *starts, int K, double epsilon, double delta, double A, int *good,
                          int *count, unsigned int *tested) {
    for (int k = 0; k < K; k++) {
        orc_est_set_model(e, models + 9 * (size_t)k);
        double lambda_new, lambda = 1;
        unsigned int t, inl = 0, idx = starts[k];
        int g = 1;
        for (t = 0; t < n; t++) {
            if (idx >= n) idx = 0;
            if (orc_est_error(e, pool[idx]) < thr) {
                inl++;
                lambda_new = lambda * (delta / epsilon);
            } else {
                lambda_new = lambda * ((1 - delta) / (1 - epsilon));
            }
            idx++;
            if (lambda_new > A) {
                g = 0;
                t++;
                break;
            }
            lambda = lambda_new;
        }
        good[k] = g;
        count[k] = g ? (int)inl : -1;
        if (tested) tested[k] = t;
    }
}

/* SPRT::computeExponentH (sprt.hpp:442-491) */
static double sprt_exponent_h(double epsilon, double epsilon_new, double delta) {
    double a = log(delta / epsilon);
    double b = log((1 - delta) / (1 - epsilon));
    double x0 = log(1 / (1 - epsilon_new)) / b;
    double v0 = epsilon_new * exp(x0 * a);
    double x1 = log((1 - 2 * v0) / (1 - epsilon_new)) / b;
    double v1 = epsilon_new * exp(x1 * a) + (1 - epsilon_new) * exp(x1 * b);
    double h = x0 - (x0 - x1) / (1 + v0 - v1) * v0;
    if (isnan(h)) return 0;
    return h;
}

/* SPRT::getUpperBoundIterations (sprt.hpp:371-393) */
unsigned int orc_sprt_upper_bound(const orc_sprt *s, int inliers_size) {
    double epsilon = (double)inliers_size / s->n;
    double P_g = pow(epsilon, s->m);
    double log_eta_l_1 = 0;
    for (unsigned int test = 0; test < s->cur; test++) {
        double h = sprt_exponent_h(s->h[test].epsilon, epsilon, s->h[test].delta);
        log_eta_l_1 += log(1 - P_g * (1 - pow(s->h[test].A, -h))) * s->h[test].k;
    }
    double numerator = log(0.05) - log_eta_l_1;
    if (numerator >= 0) return 0;
    double denumerator = log(1 - P_g * (1 - 1 / s->h[s->cur].A));
    if (isnan(denumerator) || fabs(denumerator) < 0.00001) return s->max_iters;
    double kl = numerator / denumerator;
    unsigned int k = (unsigned int)kl;
    return k < s->max_iters ? k : s->max_iters;
}

static int score_bigger(int c1, float s1, int c2, float s2) {
    /* Score::bigger (quality.hpp:22-26) */
    if (c1 > c2) return 1;
    if (c1 == c2) return s1 > s2;
    return 0;
}

/* ------------------------------------------------------------ NAPSAC (grid) */
/* NearestNeighbors::getGridNearestNeighbors (nearest_neighbors.cpp:160-202): cell =
 * ((int)(x1/cs), (int)(y1/cs), (int)(x2/cs), (int)(y2/cs)) (float division, truncation);
 * a point's neighbours are the other points of its cell in ascending index order (the
 * pair loop over each cell's index-ordered list yields exactly that order). CSR output. */
typedef struct {
    int c[4];
    int i;
} cell_key;

static int cell_cmp(const void *a, const void *b) {
    const cell_key *x = (const cell_key *)a, *y = (const cell_key *)b;
    for (int k = 0; k < 4; k++)
        if (x->c[k] != y->c[k]) return x->c[k] < y->c[k] ? -1 : 1;
    return x->i < y->i ? -1 : x->i > y->i;
}

struct orc_grid {
    unsigned int n;
    int *off; /* n + 1 */
    int *nb;
};

orc_grid *orc_grid_new(const float *pts, unsigned int n, int cell_size) {
    orc_grid *g = (orc_grid *)calloc(1, sizeof(*g));
    g->n = n;
    cell_key *keys = (cell_key *)malloc(sizeof(cell_key) * (n ? n : 1));
    for (unsigned int i = 0; i < n; i++) {
        for (int k = 0; k < 4; k++) keys[i].c[k] = (int)(pts[4 * (size_t)i + k] / (float)cell_size);
        keys[i].i = (int)i;
    }
    qsort(keys, n, sizeof(cell_key), cell_cmp);
    int *cnt = (int *)calloc(n ? n : 1, sizeof(int));
    int *cell_start = (int *)malloc(sizeof(int) * (n ? n : 1)); /* per sorted position */
    for (unsigned int a = 0; a < n;) {
        unsigned int b = a;
        while (b < n && cell_cmp(&keys[a], &keys[b]) <= 0 && memcmp(keys[a].c, keys[b].c, sizeof(keys[a].c)) == 0) b++;
        for (unsigned int k = a; k < b; k++) {
            cnt[keys[k].i] = (int)(b - a) - 1;
            cell_start[k] = (int)a;
        }
        a = b;
    }
    g->off = (int *)malloc(sizeof(int) * (n + 1));
    g->off[0] = 0;
    for (unsigned int i = 0; i < n; i++) g->off[i + 1] = g->off[i] + cnt[i];
    g->nb = (int *)malloc(sizeof(int) * (size_t)(g->off[n] ? g->off[n] : 1));
    for (unsigned int k = 0; k < n;) {
        const unsigned int a = (unsigned int)cell_start[k];
        unsigned int b = k;
        while (b < n && cell_start[b] == (int)a) b++;
        for (unsigned int u = a; u < b; u++) {
            int w = g->off[keys[u].i];
            for (unsigned int v = a; v < b; v++)
                if (v != u) g->nb[w++] = keys[v].i;
        }
        k = b;
    }
    free(keys);
    free(cnt);
    free(cell_start);
    return g;
}

void orc_grid_free(orc_grid *g) {
    if (!g) return;
    free(g->off);
    free(g->nb);
    free(g);
}

int orc_grid_count(const orc_grid *g, unsigned int i) { return g->off[i + 1] - g->off[i]; }
const int *orc_grid_list(const orc_grid *g, unsigned int i) { return g->nb + g->off[i]; }

/* NapsacSampler with Grid neighbours (napsac_sampler.hpp:40-158) over the glibc stream;
 * ArrayRandomGenerator (array_random_generator.hpp:21-49) with its member `max` defined 0
 * (SURVEY Q8).  A point needs >= m neighbours (Q18); after n failed draws the sampler turns
 * uniform and thereafter rewrites only sample[0] (subset size 1, reference behaviour). */
struct orc_napsac {
    const orc_grid *g;
    unsigned int n, m, max;
    int *array, *next;
    int do_uniform;
};

orc_napsac *orc_napsac_new(const orc_grid *g, unsigned int n, unsigned int m) {
    orc_napsac *s = (orc_napsac *)calloc(1, sizeof(*s));
    s->g = g;
    s->n = n;
    s->m = m;
    s->array = (int *)malloc(sizeof(int) * (n ? n : 1));
    for (unsigned int i = 0; i < n; i++) s->array[i] = (int)i;
    s->next = (int *)calloc(n ? n : 1, sizeof(int));
    s->max = 0;
    return s;
}

void orc_napsac_free(orc_napsac *s) {
    if (!s) return;
    free(s->array);
    free(s->next);
    free(s);
}

static int napsac_random(orc_napsac *s) {
    if (s->max == 0) s->max = s->n;
    const unsigned int k = (unsigned int)random() % s->max;
    const int v = s->array[k];
    s->max--;
    s->array[k] = s->array[s->max];
    s->array[s->max] = v;
    return v;
}

void orc_napsac_sample(orc_napsac *s, int *sample) {
    if (s->do_uniform) {
        sample[0] = napsac_random(s);
        return;
    }
    unsigned int i;
    int initial = 0;
    for (i = 0; i < s->n; i++) {
        initial = napsac_random(s);
        if ((unsigned int)orc_grid_count(s->g, (unsigned int)initial) < s->m) continue;
        break;
    }
    if (i == s->n) {
        s->do_uniform = 1;
        return;
    }
    sample[0] = initial;
    const int *nb = orc_grid_list(s->g, (unsigned int)initial);
    const int sz = orc_grid_count(s->g, (unsigned int)initial);
    for (unsigned int k = 1; k < s->m; k++) {
        sample[k] = nb[s->next[initial]];
        s->next[initial]++;
        if (s->next[initial] >= sz) s->next[initial] = 0;
    }
}

/* ------------------------------------------------------------ KNN neighbours */
/* NearestNeighbors::getNearestNeighbors_nanoflann (nearest_neighbors.cpp:69-128): the k
 * nearest points of every point by nanoflann's L2_Adaptor squared distance in float --
 * components in groups of four, result += d0*d0 + d1*d1 + d2*d2 + d3*d3, then the rest one
 * by one (nanoflann.hpp L2_Adaptor::evalMetric; the version is unpinned, this form is the
 * same in all releases) -- the query itself excluded (the reference drops the first result,
 * which is the point itself).  Equal distances: ascending index (nanoflann keeps the order
 * its KD-tree visits them in -- unpinned).  Fewer than k other points: index -1, distance
 * +inf. */
float orc_l2_dist(const float *a, const float *b, unsigned int cols) {
    float r = 0.f;
    unsigned int d = 0;
    for (; d + 4 <= cols; d += 4) {
        const float d0 = a[d] - b[d], d1 = a[d + 1] - b[d + 1], d2 = a[d + 2] - b[d + 2], d3 = a[d + 3] - b[d + 3];
        r += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (; d < cols; d++) {
        const float d0 = a[d] - b[d];
        r += d0 * d0;
    }
    return r;
}

void orc_knn(const float *pts, unsigned int n, unsigned int cols, unsigned int k, int *idx, float *d2) {
    for (unsigned int p = 0; p < n; p++) {
        int *li = idx + (size_t)p * k;
        float *ld = d2 + (size_t)p * k;
        for (unsigned int t = 0; t < k; t++) {
            li[t] = -1;
            ld[t] = INFINITY;
        }
        for (unsigned int j = 0; j < n; j++) {
            if (j == p) continue;
            const float d = orc_l2_dist(pts + (size_t)p * cols, pts + (size_t)j * cols, cols);
            if (!(d < ld[k - 1])) continue; /* ties keep the earlier (smaller) index; NaN never enters */
            unsigned int t = k - 1;
            while (t > 0 && ld[t - 1] > d) {
                ld[t] = ld[t - 1];
                li[t] = li[t - 1];
                t--;
            }
            ld[t] = d;
            li[t] = (int)j;
        }
    }
}

/* NapsacSampler::generateSampleKNN (napsac_sampler.hpp:76-98): the initial point from the
 * ArrayRandomGenerator pool, then m - 1 points walking its neighbour row from the farthest
 * (column knn - 1) backwards, cyclically, the per-point cursor persisting across samples. */
struct orc_napsac_knn {
    const int *nb;
    unsigned int n, m, knn, max;
    int *array, *next;
};

orc_napsac_knn *orc_napsac_knn_new(const int *nb, unsigned int n, unsigned int m, unsigned int knn) {
    orc_napsac_knn *s = (orc_napsac_knn *)calloc(1, sizeof(*s));
    s->nb = nb;
    s->n = n;
    s->m = m;
    s->knn = knn;
    s->array = (int *)malloc(sizeof(int) * (n ? n : 1));
    for (unsigned int i = 0; i < n; i++) s->array[i] = (int)i;
    s->next = (int *)calloc(n ? n : 1, sizeof(int));
    s->max = 0;
    return s;
}

void orc_napsac_knn_free(orc_napsac_knn *s) {
    if (!s) return;
    free(s->array);
    free(s->next);
    free(s);
}

void orc_napsac_knn_sample(orc_napsac_knn *s, int *sample) {
    if (s->max == 0) s->max = s->n; /* ArrayRandomGenerator::getRandomNumber */
    const unsigned int r = (unsigned int)random() % s->max;
    const int init = s->array[r];
    s->max--;
    s->array[r] = s->array[s->max];
    s->array[s->max] = init;
    sample[0] = init;
    const int knn = (int)s->knn;
    for (unsigned int i = 1; i < s->m; i++) {
        sample[i] = s->nb[(size_t)knn * (size_t)init + (size_t)(s->next[init] + knn - 1)];
        s->next[init]--;
        if (s->next[init] == -knn) s->next[init] = 0;
    }
}

/* ------------------------------------------------------------ LO-RANSAC */
/* InnerLocalOptimization (inner_local_optimization.hpp:40-133) + IterativeLocalOptimization
 * (iterative_local_optimization.hpp:28-136).  Its UniformRandomGenerator is an mt19937 seeded
 * here with seed + 1 (the reference: std::random_device).  lo_model's threshold persists
 * across calls and compounds. */
typedef struct {
    orc_mt g;
    int limited;
    unsigned int inner, iters, limit, mult, m, n;
    float theta, lo_thr, step;
    int *max_inl, *lo_inl, *lo_sample;
    unsigned int inner_count, iterative_count;
    float lo_model[9];
} orc_lo;

static void lo_init(orc_lo *L, const orc_config *cfg, unsigned int n, unsigned int m) {
    memset(L, 0, sizeof(*L));
    orc_mt_seed(&L->g, cfg->seed + 1u);
    L->limited = cfg->lo == ORC_LO_INITFLORSC;
    L->inner = cfg->lo_inner_iterations;
    L->iters = cfg->lo_iterative_iterations;
    L->limit = cfg->lo_sample_size;
    L->mult = cfg->lo_threshold_multiplier;
    L->m = m;
    L->n = n;
    L->theta = cfg->threshold;
    L->lo_thr = cfg->threshold;
    L->step = (L->theta * L->mult - L->theta) / L->iters;
    L->max_inl = (int *)malloc(sizeof(int) * (n ? n : 1));
    L->lo_inl = (int *)malloc(sizeof(int) * (n ? n : 1));
    L->lo_sample = (int *)malloc(sizeof(int) * (L->limit ? L->limit : 1));
}

static void lo_free(orc_lo *L) {
    free(L->max_inl);
    free(L->lo_inl);
    free(L->lo_sample);
}

/* returns fail */
static int lo_iterative(orc_lo *L, orc_est *e, int *lo_cnt, float *lo_sum, int best_cnt, float best_sum) {
    for (unsigned int it = 0; it < L->iters; it++) {
        L->lo_thr -= L->step;
        if (*lo_cnt <= (int)L->m) break;
        if (L->limited) {
            if (*lo_cnt > (int)L->limit) {
                mt_unique_set(&L->g, L->lo_sample, L->limit, (unsigned int)(*lo_cnt - 1));
                for (unsigned int k = 0; k < L->limit; k++) L->lo_sample[k] = L->lo_inl[L->lo_sample[k]];
                if (!orc_est_nonminimal(e, L->lo_sample, L->limit, L->lo_model)) continue;
            } else {
                if (!orc_est_nonminimal(e, L->lo_inl, (unsigned int)*lo_cnt, L->lo_model)) break;
            }
            orc_quality(e, L->lo_model, L->lo_thr, lo_cnt, lo_sum, L->lo_inl);
        } else {
            if (!orc_est_nonminimal(e, L->lo_inl, (unsigned int)*lo_cnt, L->lo_model)) break;
            orc_quality(e, L->lo_model, L->lo_thr, lo_cnt, lo_sum, L->lo_inl);
            if (score_bigger(best_cnt, best_sum, *lo_cnt, *lo_sum)) break;
        }
        L->iterative_count++;
    }
    int fail = 0;
    if (fabsf(L->lo_thr - L->theta) > 0.00001) {
        fail = 1;
        L->lo_thr = L->theta;
    }
    return fail;
}

/* GetModelScore(model, score): model / (cnt, sum) improved in place */
static void lo_run(orc_lo *L, orc_est *e, float *model, int *cnt, float *sum) {
    if (*cnt < 12) return;
    int c0;
    float s0;
    orc_quality(e, model, L->theta, &c0, &s0, L->max_inl);
    for (unsigned int it = 0; it < L->inner; it++) {
        if (*cnt > (int)L->limit) {
            mt_unique_set(&L->g, L->lo_sample, L->limit, (unsigned int)(*cnt - 1));
            for (unsigned int k = 0; k < L->limit; k++) L->lo_sample[k] = L->max_inl[L->lo_sample[k]];
            if (!orc_est_nonminimal(e, L->lo_sample, L->limit, L->lo_model)) continue;
        } else {
            if (!orc_est_nonminimal(e, L->max_inl, (unsigned int)*cnt, L->lo_model)) return;
        }
        L->lo_thr = L->mult * L->lo_thr;
        int lo_cnt;
        float lo_sum;
        orc_quality(e, L->lo_model, L->lo_thr, &lo_cnt, &lo_sum, L->lo_inl);
        if (lo_cnt <= (int)L->m) continue;
        const int fail = lo_iterative(L, e, &lo_cnt, &lo_sum, *cnt, *sum);
        if (!fail && score_bigger(lo_cnt, lo_sum, *cnt, *sum)) {
            memcpy(model, L->lo_model, sizeof(float) * 9);
            *cnt = lo_cnt;
            *sum = lo_sum;
            memcpy(L->max_inl, L->lo_inl, sizeof(int) * (size_t)lo_cnt);
        }
        L->inner_count++;
    }
}

/* ------------------------------------------------------------ Graph-cut LO */
/* Boykov-Kolmogorov max-flow as the reference's vendored gco-v3.0 implements it
 * (include/gco-v3.0/graph.h, graph.inl, maxflow.inl; energy.h for the term encoding),
 * restated over index arrays: arcs in pairs (sister = a ^ 1) prepended to their node's arc
 * list, two-queue FIFO of active nodes, augmentation orphans pushed to the front of the
 * orphan list and adoption orphans to the rear, TIME/DIST distance heuristic.  Capacities,
 * flows and every comparison in float, in gco's operation order, so the final search trees
 * -- and so what_segment -- are the reference's.  Pinned against the gco sources themselves
 * (oracle/_ref/libgco_ref.so, built from /root/reference by oracle/Makefile). */
enum { BK_NONE = -1, BK_TERMINAL = -2, BK_ORPHAN = -3 };
#define BK_INF_D 0x7fffffff

struct orc_bk {
    int n, n_cap, m, m_cap;
    int *first, *parent, *next, *ts, *dist;
    unsigned char *is_sink;
    float *tr_cap;
    int *head, *anext;
    float *r_cap;
    int *op_node, *op_next, op_cap, op_used, op_free;
    int orphan_first, orphan_last, q_first[2], q_last[2], time;
    float flow;
};

orc_bk *orc_bk_new(int n_nodes, int n_edges) {
    orc_bk *g = (orc_bk *)calloc(1, sizeof(*g));
    g->n_cap = n_nodes > 16 ? n_nodes : 16;
    g->m_cap = 2 * (n_edges > 16 ? n_edges : 16);
    g->first = (int *)malloc(sizeof(int) * g->n_cap);
    g->parent = (int *)malloc(sizeof(int) * g->n_cap);
    g->next = (int *)malloc(sizeof(int) * g->n_cap);
    g->ts = (int *)malloc(sizeof(int) * g->n_cap);
    g->dist = (int *)malloc(sizeof(int) * g->n_cap);
    g->is_sink = (unsigned char *)malloc(g->n_cap);
    g->tr_cap = (float *)malloc(sizeof(float) * g->n_cap);
    g->head = (int *)malloc(sizeof(int) * g->m_cap);
    g->anext = (int *)malloc(sizeof(int) * g->m_cap);
    g->r_cap = (float *)malloc(sizeof(float) * g->m_cap);
    g->op_free = -1;
    return g;
}

void orc_bk_free(orc_bk *g) {
    if (!g) return;
    free(g->first); free(g->parent); free(g->next); free(g->ts); free(g->dist); free(g->is_sink);
    free(g->tr_cap); free(g->head); free(g->anext); free(g->r_cap); free(g->op_node); free(g->op_next);
    free(g);
}

int orc_bk_add_node(orc_bk *g) {
    if (g->n == g->n_cap) {
        g->n_cap += g->n_cap / 2;
        g->first = (int *)realloc(g->first, sizeof(int) * g->n_cap);
        g->parent = (int *)realloc(g->parent, sizeof(int) * g->n_cap);
        g->next = (int *)realloc(g->next, sizeof(int) * g->n_cap);
        g->ts = (int *)realloc(g->ts, sizeof(int) * g->n_cap);
        g->dist = (int *)realloc(g->dist, sizeof(int) * g->n_cap);
        g->is_sink = (unsigned char *)realloc(g->is_sink, g->n_cap);
        g->tr_cap = (float *)realloc(g->tr_cap, sizeof(float) * g->n_cap);
    }
    g->first[g->n] = -1;
    g->tr_cap[g->n] = 0.f;
    return g->n++;
}

/* graph.h add_tweights */
void orc_bk_add_tweights(orc_bk *g, int i, float cap_source, float cap_sink) {
    const float delta = g->tr_cap[i];
    if (delta > 0) cap_source += delta;
    else cap_sink -= delta;
    g->flow += (cap_source < cap_sink) ? cap_source : cap_sink;
    g->tr_cap[i] = cap_source - cap_sink;
}

/* graph.h add_edge: arc pair (i -> j, j -> i), each prepended to its tail's list */
void orc_bk_add_edge(orc_bk *g, int i, int j, float cap, float rev_cap) {
    if (g->m + 2 > g->m_cap) {
        g->m_cap += g->m_cap / 2;
        if (g->m_cap & 1) g->m_cap++;
        g->head = (int *)realloc(g->head, sizeof(int) * g->m_cap);
        g->anext = (int *)realloc(g->anext, sizeof(int) * g->m_cap);
        g->r_cap = (float *)realloc(g->r_cap, sizeof(float) * g->m_cap);
    }
    const int a = g->m, ar = g->m + 1;
    g->m += 2;
    g->anext[a] = g->first[i];
    g->first[i] = a;
    g->anext[ar] = g->first[j];
    g->first[j] = ar;
    g->head[a] = j;
    g->head[ar] = i;
    g->r_cap[a] = cap;
    g->r_cap[ar] = rev_cap;
}

/* energy.h add_term1 / add_term2 */
void orc_bk_add_term1(orc_bk *g, int x, float e0, float e1) { orc_bk_add_tweights(g, x, e1, e0); }
void orc_bk_add_term2(orc_bk *g, int x, int y, float A, float B, float C, float D) {
    orc_bk_add_tweights(g, x, D, A);
    B -= A;
    C -= D;
    if (B < 0) {
        orc_bk_add_tweights(g, x, 0, B);
        orc_bk_add_tweights(g, y, 0, -B);
        orc_bk_add_edge(g, x, y, 0, B + C);
    } else if (C < 0) {
        orc_bk_add_tweights(g, x, 0, -C);
        orc_bk_add_tweights(g, y, 0, C);
        orc_bk_add_edge(g, x, y, B + C, 0);
    } else {
        orc_bk_add_edge(g, x, y, B, C);
    }
}

static void bk_set_active(orc_bk *g, int i) {
    if (g->next[i] != -1) return;
    if (g->q_last[1] >= 0) g->next[g->q_last[1]] = i;
    else g->q_first[1] = i;
    g->q_last[1] = i;
    g->next[i] = i;
}

static int bk_next_active(orc_bk *g) {
    for (;;) {
        int i = g->q_first[0];
        if (i < 0) {
            g->q_first[0] = i = g->q_first[1];
            g->q_last[0] = g->q_last[1];
            g->q_first[1] = g->q_last[1] = -1;
            if (i < 0) return -1;
        }
        if (g->next[i] == i) g->q_first[0] = g->q_last[0] = -1;
        else g->q_first[0] = g->next[i];
        g->next[i] = -1;
        if (g->parent[i] != BK_NONE) return i;
    }
}

static int bk_np_new(orc_bk *g, int node) {
    int np;
    if (g->op_free >= 0) {
        np = g->op_free;
        g->op_free = g->op_next[np];
    } else {
        if (g->op_used == g->op_cap) {
            g->op_cap = g->op_cap ? 2 * g->op_cap : 128;
            g->op_node = (int *)realloc(g->op_node, sizeof(int) * g->op_cap);
            g->op_next = (int *)realloc(g->op_next, sizeof(int) * g->op_cap);
        }
        np = g->op_used++;
    }
    g->op_node[np] = node;
    return np;
}
static void bk_np_delete(orc_bk *g, int np) {
    g->op_next[np] = g->op_free;
    g->op_free = np;
}
static void bk_orphan_front(orc_bk *g, int i) {
    g->parent[i] = BK_ORPHAN;
    const int np = bk_np_new(g, i);
    g->op_next[np] = g->orphan_first;
    g->orphan_first = np;
}
static void bk_orphan_rear(orc_bk *g, int i) {
    g->parent[i] = BK_ORPHAN;
    const int np = bk_np_new(g, i);
    if (g->orphan_last >= 0) g->op_next[g->orphan_last] = np;
    else g->orphan_first = np;
    g->orphan_last = np;
    g->op_next[np] = -1;
}

static void bk_augment(orc_bk *g, int mid) {
    int i, a;
    float b = g->r_cap[mid];
    for (i = g->head[mid ^ 1];; i = g->head[a]) { /* source tree */
        a = g->parent[i];
        if (a == BK_TERMINAL) break;
        if (b > g->r_cap[a ^ 1]) b = g->r_cap[a ^ 1];
    }
    if (b > g->tr_cap[i]) b = g->tr_cap[i];
    for (i = g->head[mid];; i = g->head[a]) { /* sink tree */
        a = g->parent[i];
        if (a == BK_TERMINAL) break;
        if (b > g->r_cap[a]) b = g->r_cap[a];
    }
    if (b > -g->tr_cap[i]) b = -g->tr_cap[i];
    g->r_cap[mid ^ 1] += b;
    g->r_cap[mid] -= b;
    for (i = g->head[mid ^ 1];; i = g->head[a]) {
        a = g->parent[i];
        if (a == BK_TERMINAL) break;
        g->r_cap[a] += b;
        g->r_cap[a ^ 1] -= b;
        if (!g->r_cap[a ^ 1]) bk_orphan_front(g, i);
    }
    g->tr_cap[i] -= b;
    if (!g->tr_cap[i]) bk_orphan_front(g, i);
    for (i = g->head[mid];; i = g->head[a]) {
        a = g->parent[i];
        if (a == BK_TERMINAL) break;
        g->r_cap[a ^ 1] += b;
        g->r_cap[a] -= b;
        if (!g->r_cap[a]) bk_orphan_front(g, i);
    }
    g->tr_cap[i] += b;
    if (!g->tr_cap[i]) bk_orphan_front(g, i);
    g->flow += b;
}

/* process_source_orphan (sink = 0) / process_sink_orphan (sink = 1) */
static void bk_process_orphan(orc_bk *g, int i, int sink) {
    int a0, a0_min = BK_NONE, a, j, d, d_min = BK_INF_D;
    for (a0 = g->first[i]; a0 >= 0; a0 = g->anext[a0]) {
        if (!(sink ? g->r_cap[a0] : g->r_cap[a0 ^ 1])) continue;
        j = g->head[a0];
        if ((int)g->is_sink[j] != sink || (a = g->parent[j]) == BK_NONE) continue;
        d = 0; /* the origin of j */
        for (;;) {
            if (g->ts[j] == g->time) {
                d += g->dist[j];
                break;
            }
            a = g->parent[j];
            d++;
            if (a == BK_TERMINAL) {
                g->ts[j] = g->time;
                g->dist[j] = 1;
                break;
            }
            if (a == BK_ORPHAN) {
                d = BK_INF_D;
                break;
            }
            j = g->head[a];
        }
        if (d < BK_INF_D) {
            if (d < d_min) {
                a0_min = a0;
                d_min = d;
            }
            for (j = g->head[a0]; g->ts[j] != g->time; j = g->head[g->parent[j]]) {
                g->ts[j] = g->time;
                g->dist[j] = d--;
            }
        }
    }
    if ((g->parent[i] = a0_min) != BK_NONE) {
        g->ts[i] = g->time;
        g->dist[i] = d_min + 1;
        return;
    }
    for (a0 = g->first[i]; a0 >= 0; a0 = g->anext[a0]) {
        j = g->head[a0];
        if ((int)g->is_sink[j] != sink || (a = g->parent[j]) == BK_NONE) continue;
        if (sink ? g->r_cap[a0] : g->r_cap[a0 ^ 1]) bk_set_active(g, j);
        if (a != BK_TERMINAL && a != BK_ORPHAN && g->head[a] == i) bk_orphan_rear(g, j);
    }
}

/* Graph::maxflow() (reuse_trees = false) */
float orc_bk_maxflow(orc_bk *g) {
    int i, j, a, np, np_next, current = -1;
    g->q_first[0] = g->q_last[0] = g->q_first[1] = g->q_last[1] = -1;
    g->orphan_first = g->orphan_last = -1;
    g->time = 0;
    for (i = 0; i < g->n; i++) { /* maxflow_init */
        g->next[i] = -1;
        g->ts[i] = g->time;
        if (g->tr_cap[i] > 0) {
            g->is_sink[i] = 0;
            g->parent[i] = BK_TERMINAL;
            bk_set_active(g, i);
            g->dist[i] = 1;
        } else if (g->tr_cap[i] < 0) {
            g->is_sink[i] = 1;
            g->parent[i] = BK_TERMINAL;
            bk_set_active(g, i);
            g->dist[i] = 1;
        } else {
            g->parent[i] = BK_NONE;
        }
    }
    for (;;) {
        i = current;
        if (i >= 0) {
            g->next[i] = -1;
            if (g->parent[i] == BK_NONE) i = -1;
        }
        if (i < 0 && (i = bk_next_active(g)) < 0) break;
        if (!g->is_sink[i]) { /* grow the source tree */
            for (a = g->first[i]; a >= 0; a = g->anext[a]) {
                if (!g->r_cap[a]) continue;
                j = g->head[a];
                if (g->parent[j] == BK_NONE) {
                    g->is_sink[j] = 0;
                    g->parent[j] = a ^ 1;
                    g->ts[j] = g->ts[i];
                    g->dist[j] = g->dist[i] + 1;
                    bk_set_active(g, j);
                } else if (g->is_sink[j]) {
                    break;
                } else if (g->ts[j] <= g->ts[i] && g->dist[j] > g->dist[i]) {
                    g->parent[j] = a ^ 1;
                    g->ts[j] = g->ts[i];
                    g->dist[j] = g->dist[i] + 1;
                }
            }
        } else { /* grow the sink tree */
            for (a = g->first[i]; a >= 0; a = g->anext[a]) {
                if (!g->r_cap[a ^ 1]) continue;
                j = g->head[a];
                if (g->parent[j] == BK_NONE) {
                    g->is_sink[j] = 1;
                    g->parent[j] = a ^ 1;
                    g->ts[j] = g->ts[i];
                    g->dist[j] = g->dist[i] + 1;
                    bk_set_active(g, j);
                } else if (!g->is_sink[j]) {
                    a = a ^ 1;
                    break;
                } else if (g->ts[j] <= g->ts[i] && g->dist[j] > g->dist[i]) {
                    g->parent[j] = a ^ 1;
                    g->ts[j] = g->ts[i];
                    g->dist[j] = g->dist[i] + 1;
                }
            }
        }
        g->time++;
        if (a >= 0) {
            g->next[i] = i; /* stays active */
            current = i;
            bk_augment(g, a);
            while ((np = g->orphan_first) >= 0) { /* adoption */
                np_next = g->op_next[np];
                g->op_next[np] = -1;
                while ((np = g->orphan_first) >= 0) {
                    g->orphan_first = g->op_next[np];
                    i = g->op_node[np];
                    bk_np_delete(g, np);
                    if (g->orphan_first < 0) g->orphan_last = -1;
                    bk_process_orphan(g, i, g->is_sink[i]);
                }
                g->orphan_first = np_next;
            }
        } else {
            current = -1;
        }
    }
    return g->flow;
}

/* what_segment(i) == SINK (default segment SOURCE for free nodes) */
int orc_bk_is_sink(const orc_bk *g, int i) { return g->parent[i] != BK_NONE && g->is_sink[i]; }

/* gco_ref-compatible driver: n nodes, add_term1(i, unary[i], 0), then add_term2 for the m
 * listed pairs in order; sink_out[i] = what_segment(i) == SINK.  Returns the flow. */
float orc_bk_label(int n, const float *unary, int m, const int *ei, const int *ej, const float *e00,
                   const float *e01, const float *e10, const float *e11, int *sink_out) {
    orc_bk *g = orc_bk_new(n, m);
    for (int i = 0; i < n; i++) orc_bk_add_node(g);
    for (int i = 0; i < n; i++) orc_bk_add_term1(g, i, unary[i], 0.f);
    for (int k = 0; k < m; k++) orc_bk_add_term2(g, ei[k], ej[k], e00[k], e01[k], e10[k], e11[k]);
    const float f = orc_bk_maxflow(g);
    for (int i = 0; i < n; i++) sink_out[i] = orc_bk_is_sink(g, i);
    orc_bk_free(g);
    return f;
}

/* GraphCut::labeling (graphcut.cpp:7-101): residuals of `model`, unary energies
 * exp(-(e*e) / (2 thr^2)) (float argument, the C library's double exp -- the reference's
 * unqualified exp on a float, see DESIGN), pairwise terms over the neighbour lists
 * (skipping non-submodular / NaN terms), BK min cut; inliers = SINK nodes, ascending. */
typedef struct {
    const int *knn_tab; /* n x knn (NULL: grid) */
    unsigned int knn;
    const orc_grid *grid;
    float lambda, sqr_thr;
} orc_gc_graph;

static int gc_labeling(orc_est *e, const orc_gc_graph *G, const float *model, int *inliers, float *errors) {
    const unsigned int n = e->n;
    orc_est_set_model(e, model);
    orc_bk *g = orc_bk_new((int)n, (int)(G->knn_tab ? G->knn * n : n));
    for (unsigned int i = 0; i < n; i++) orc_bk_add_node(g);
    for (unsigned int i = 0; i < n; i++) {
        const float d = orc_est_error(e, i);
        errors[i] = d;
        const float energy = (float)exp(-(d * d) / G->sqr_thr);
        orc_bk_add_term1(g, (int)i, energy, 0.f);
    }
    const float e01 = 1.f, e10 = 1.f, lam = G->lambda;
    for (unsigned int i = 0; i < n; i++) {
        const float d1 = errors[i];
        const float energy1 = (float)exp(-(d1 * d1) / G->sqr_thr);
        const unsigned int cnt = G->knn_tab ? G->knn : (unsigned int)orc_grid_count(G->grid, i);
        const int *row = G->knn_tab ? G->knn_tab + (size_t)G->knn * i : orc_grid_list(G->grid, i);
        for (unsigned int k = 0; k < cnt; k++) {
            const int j = row[k];
            if (j == (int)i || j < 0) continue;
            const float d2 = errors[j];
            const float energy2 = (float)exp(-(d2 * d2) / G->sqr_thr);
            const float e00 = (energy1 + energy2) / 2;
            const float e11 = 1 - e00;
            if (e00 + e11 > e01 + e10 || isnan(e00)) continue;
            orc_bk_add_term2(g, (int)i, j, e00 * lam, e01 * lam, e10 * lam, e11 * lam);
        }
    }
    orc_bk_maxflow(g);
    int cnt = 0;
    for (unsigned int i = 0; i < n; i++)
        if (orc_bk_is_sink(g, (int)i)) inliers[cnt++] = (int)i;
    orc_bk_free(g);
    return cnt;
}

/* GraphCut::GetModelScore (graphcut.hpp:99-153): while the best improves: label, then up to
 * lo_inner_iterations least-squares fits on 7m-point random subsets of the labelling's
 * inliers (all of them, once, when there are <= 7m), each scored at the model threshold and
 * kept when Score::bigger.  Its mt19937 is seeded with seed + 1 (reference: random_device). */
typedef struct {
    orc_mt g;
    orc_gc_graph G;
    unsigned int inner, m, n, limit;
    float thr;
    int *inl, *sample;
    float *errors;
    unsigned int gc_iters, labelings;
} orc_gc;

static void gc_init(orc_gc *C, const orc_config *cfg, unsigned int n, unsigned int m) {
    memset(C, 0, sizeof(*C));
    orc_mt_seed(&C->g, cfg->seed + 1u);
    C->inner = cfg->lo_inner_iterations;
    C->m = m;
    C->n = n;
    C->limit = 7 * m;
    C->thr = cfg->threshold;
    C->G.lambda = cfg->spatial_coherence_gc; /* model.hpp:33 (default 0.1), graphcut.hpp:43 as given */
    C->G.sqr_thr = 2 * cfg->threshold * cfg->threshold;
    C->inl = (int *)malloc(sizeof(int) * (n ? n : 1));
    C->errors = (float *)malloc(sizeof(float) * (n ? n : 1));
    C->sample = (int *)malloc(sizeof(int) * C->limit);
}

static void gc_free(orc_gc *C) {
    free(C->inl);
    free(C->errors);
    free(C->sample);
}

static void gc_run(orc_gc *C, orc_est *e, float *model, int *cnt, float *sum) {
    int updated = 1;
    float gc_model[9];
    while (updated) {
        updated = 0;
        const int L = gc_labeling(e, &C->G, model, C->inl, C->errors);
        C->labelings++;
        if (L <= (int)C->m) break;
        for (unsigned int it = 0; it < C->inner; it++) {
            if ((unsigned int)L > C->limit) {
                mt_unique_set(&C->g, C->sample, C->limit, (unsigned int)(L - 1));
                for (unsigned int k = 0; k < C->limit; k++) C->sample[k] = C->inl[C->sample[k]];
                if (!orc_est_nonminimal(e, C->sample, C->limit, gc_model)) break;
            } else {
                if (it > 0) break;
                if (!orc_est_nonminimal(e, C->inl, (unsigned int)L, gc_model)) break;
            }
            int c;
            float s;
            orc_quality(e, gc_model, C->thr, &c, &s, NULL);
            if (score_bigger(c, s, *cnt, *sum)) {
                updated = 1;
                *cnt = c;
                *sum = s;
                memcpy(model, gc_model, sizeof(gc_model));
            }
            C->gc_iters++;
        }
    }
}

/* ------------------------------------------------------------ Ransac::run */

int orc_ransac_run_cfg(int kind, const float *points, unsigned int n, const orc_config *cfg, orc_result *out,
                       int *inliers_out, unsigned int *rec_iter, int *rec_count, float *rec_score, int rec_cap) {
    orc_est *e = orc_est_new(kind, points, n, cfg->dlt_mode);
    if (!e) return -1;
    const int m = orc_est_sample_size(e);
    const float threshold = cfg->threshold;
    const int prosac = cfg->sampler == ORC_SAMPLER_PROSAC;
    const int napsac = cfg->sampler == ORC_SAMPLER_NAPSAC;
    /* Ransac ctor order (ransac.hpp:41-93): sampler, termination, then SPRT (whose pool
     * shuffle consumes n glibc draws before the Uniform sampler's first). */
    orc_srandom(cfg->seed);
    orc_uniform *smp = (prosac || napsac) ? NULL : orc_uniform_new(n, (unsigned int)m);
    orc_prosac *ps = prosac ? orc_prosac_new((unsigned int)m, n, cfg->seed) : NULL;
    orc_lo lo;
    const int use_lo = cfg->lo == ORC_LO_INITLORSC || cfg->lo == ORC_LO_INITFLORSC;
    if (use_lo) lo_init(&lo, cfg, n, (unsigned int)m);
    const int use_gc = cfg->lo == ORC_LO_GC;
    /* NAPSAC + GC: the reference hands the neighbours to the sampler only and leaves the
     * graph cut's neighbour type uninitialised (ransac.hpp:62-78) -- not reproducible */
    if (use_gc && napsac) {
        orc_est_free(e);
        if (smp) orc_uniform_free(smp);
        return -2;
    }
    orc_gc gc;
    if (use_gc) gc_init(&gc, cfg, n, (unsigned int)m);
    /* Ransac ctor (ransac.hpp:60-78): Grid neighbours, or nanoflann KNN for any other type */
    const int knn_mode = napsac && cfg->neighbors != ORC_NEIGHBORS_GRID;
    orc_grid *grid = napsac && !knn_mode ? orc_grid_new(points, n, cfg->cell_size) : NULL;
    orc_napsac *ns = grid ? orc_napsac_new(grid, n, (unsigned int)m) : NULL;
    int *knn_tab = NULL;
    orc_napsac_knn *nk = NULL;
    const int gc_knn = use_gc && cfg->neighbors != ORC_NEIGHBORS_GRID;
    orc_grid *gc_grid = use_gc && !gc_knn ? orc_grid_new(points, n, cfg->cell_size) : NULL;
    if (knn_mode || gc_knn) {
        const unsigned int k = cfg->knn;
        knn_tab = (int *)malloc(sizeof(int) * (size_t)n * (k ? k : 1));
        float *kd = (float *)malloc(sizeof(float) * (size_t)n * (k ? k : 1));
        orc_knn(points, n, (unsigned int)orc_est_cols(e), k, knn_tab, kd);
        free(kd);
        if (knn_mode) nk = orc_napsac_knn_new(knn_tab, n, (unsigned int)m, k);
    }
    if (use_gc) {
        gc.G.knn_tab = gc_knn ? knn_tab : NULL;
        gc.G.knn = cfg->knn;
        gc.G.grid = gc_grid;
    }
    orc_prosac_term *pt = prosac ? orc_prosac_term_new(orc_prosac_growth(ps), n, (unsigned int)m, cfg->desired_prob,
                                                       cfg->max_iterations)
                                 : NULL;
    orc_sprt *sp = cfg->sprt ? orc_sprt_new(kind, n, (unsigned int)m, cfg->max_iterations, 20) : NULL;
    int *inl = (int *)malloc(sizeof(int) * (n ? n : 1));
    unsigned char *flags = (unsigned char *)malloc(n ? n : 1);
    int sample[16];
    memset(sample, 0, sizeof(sample));
    float models[27], best_model[9];
    memset(best_model, 0, sizeof(best_model));
    int best_cnt = 0, nrec = 0;
    float best_sum = 0.f;
    unsigned int iters = 0, max_iters = cfg->max_iterations;
    out->sprt_rejected = 0;

    /* ransac.cpp:58-139 */
    while (iters < max_iters) {
        if (prosac) {
            orc_prosac_set_term_len(ps, orc_prosac_term_length(pt));
            orc_prosac_sample(ps, sample);
        } else if (nk) {
            orc_napsac_knn_sample(nk, sample);
        } else if (napsac) {
            orc_napsac_sample(ns, sample);
        } else {
            orc_uniform_sample(smp, sample);
        }
        int nm = orc_est_estimate(e, sample, models);
        for (int i = 0; i < nm; i++) {
            int cnt = 0;
            float sum = 0.f;
            if (sp) {
                orc_est_set_model(e, models + 9 * i);
                int good = orc_sprt_verify(sp, e, threshold, (int)iters, (unsigned int)best_cnt, &cnt, &sum, NULL);
                if (!good) {
                    out->sprt_rejected++;
                    if ((int)iters >= 20) { /* max_hypothesis_test_before_sprt, SURVEY Q9 */
                        iters++;
                        continue;
                    }
                }
            } else {
                orc_quality(e, models + 9 * i, threshold, &cnt, &sum, NULL);
            }
            if (score_bigger(cnt, sum, best_cnt, best_sum)) {
                if (use_lo) lo_run(&lo, e, models + 9 * i, &cnt, &sum); /* ransac.cpp:110-112 */
                if (use_gc) gc_run(&gc, e, models + 9 * i, &cnt, &sum);
                best_cnt = cnt;
                best_sum = sum;
                memcpy(best_model, models + 9 * i, sizeof(best_model));
                if (prosac) {
                    orc_est_set_model(e, best_model);
                    for (unsigned int p = 0; p < n; p++) flags[p] = orc_est_error(e, p) < threshold;
                    max_iters = orc_prosac_term_update(pt, iters, flags, orc_prosac_largest(ps));
                } else {
                    max_iters = orc_std_termination((unsigned int)best_cnt, n, (unsigned int)m, cfg->desired_prob,
                                                    cfg->max_iterations);
                }
                if (sp) {
                    unsigned int ub = orc_sprt_upper_bound(sp, best_cnt);
                    if (ub < max_iters) max_iters = ub;
                }
                if (nrec < rec_cap) {
                    if (rec_iter) rec_iter[nrec] = iters;
                    if (rec_count) rec_count[nrec] = cnt;
                    if (rec_score) rec_score[nrec] = sum;
                }
                nrec++;
            }
        }
        iters++;
    }
    int rc = 0;
    out->iters = iters;
    out->n_records = nrec;
    out->polish_passes = 0;
    out->sprt_histories = sp ? (int)orc_sprt_histories(sp) : 0;
    out->prosac_term_len = pt ? orc_prosac_term_length(pt) : n;
    if (best_cnt != 0 && use_gc && gc.gc_iters == 0) /* ransac.cpp:149-153: GC set but never ran */
        gc_run(&gc, e, best_model, &best_cnt, &best_sum);
    out->lo_inner_iters = use_lo ? lo.inner_count : use_gc ? gc.gc_iters : 0;
    out->lo_iterative_iters = use_lo ? lo.iterative_count : use_gc ? gc.labelings : 0;
    memcpy(out->minimal_model, best_model, sizeof(best_model));
    out->minimal_inliers = best_cnt;
    if (best_cnt == 0) {
        rc = -111; /* ransac.cpp:143-147 */
    } else {
        /* ransac.cpp:157-207: <= 4 non-minimal passes */
        float nm_model[9];
        int prev = 0, cnt;
        float sum;
        orc_quality(e, best_model, threshold, &cnt, &sum, inl); /* getInliers */
        for (int norm = 0; norm < 4; norm++) {
            if (!orc_est_nonminimal(e, inl, (unsigned int)best_cnt, nm_model)) break;
            orc_quality(e, nm_model, threshold, &cnt, &sum, inl);
            if ((double)((float)cnt / (float)best_cnt) < 0.8) break;
            if (cnt <= prev) break;
            prev = cnt;
            best_cnt = cnt;
            best_sum = sum;
            memcpy(best_model, nm_model, sizeof(best_model));
            out->polish_passes++;
        }
        /* ransac.cpp:214 final inliers of the best model */
        orc_quality(e, best_model, threshold, &cnt, &sum, inliers_out ? inliers_out : inl);
    }
    memcpy(out->model, best_model, sizeof(best_model));
    out->inliers = best_cnt;
    free(inl);
    free(flags);
    orc_uniform_free(smp);
    orc_prosac_free(ps);
    orc_prosac_term_free(pt);
    orc_sprt_free(sp);
    orc_napsac_free(ns);
    orc_napsac_knn_free(nk);
    free(knn_tab);
    orc_grid_free(grid);
    if (use_lo) lo_free(&lo);
    if (use_gc) gc_free(&gc);
    orc_grid_free(gc_grid);
    orc_est_free(e);
    return rc;
}

int orc_ransac_run(int kind, const float *points, unsigned int n, float threshold, float desired_prob,
                   unsigned int max_iterations, unsigned int seed, int dlt_mode, orc_result *out,
                   int *inliers_out, unsigned int *rec_iter, int *rec_count, float *rec_score, int rec_cap) {
    orc_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.threshold = threshold;
    cfg.desired_prob = desired_prob;
    cfg.max_iterations = max_iterations;
    cfg.seed = seed;
    cfg.dlt_mode = dlt_mode;
    cfg.sampler = ORC_SAMPLER_UNIFORM;
    cfg.sprt = 0;
    cfg.lo = 0;
    cfg.lo_sample_size = 14;
    cfg.lo_iterative_iterations = 4;
    cfg.lo_inner_iterations = 20;
    cfg.lo_threshold_multiplier = 10;
    cfg.cell_size = 50;
    return orc_ransac_run_cfg(kind, points, n, &cfg, out, inliers_out, rec_iter, rec_count, rec_score, rec_cap);
}

int orc_hypothesis_loop(orc_est *e, orc_uniform *s, int count, float thr, float *best_score_sum) {
    int m = orc_est_sample_size(e);
    int sample[9];
    float models[27];
    int best_cnt = 0;
    float best_sum = 0.f;
    for (int it = 0; it < count; it++) {
        orc_uniform_sample(s, sample);
        int nm = orc_est_estimate(e, sample, models);
        (void)m;
        for (int i = 0; i < nm; i++) {
            int cnt;
            float sum;
            orc_quality(e, models + 9 * i, thr, &cnt, &sum, NULL);
            if (score_bigger(cnt, sum, best_cnt, best_sum)) {
                best_cnt = cnt;
                best_sum = sum;
            }
        }
    }
    if (best_score_sum) *best_score_sum = best_sum;
    return best_cnt;
}

/* All-cores CPU baseline: the same reference-style loop on `threads`
 * std-thread-like workers (pthreads) over disjoint ranges of one pre-drawn glibc sample stream,
 * each worker with its own estimator state (the reference's estimator caches the model, so
 * one instance per thread).  Returns the wall seconds of the parallel region; best via out. */
#include <pthread.h>
#include <time.h>

typedef struct {
    int kind, dlt_mode, m, count;
    const float *pts;
    unsigned int n;
    const int *samples;
    float thr;
    int best_cnt;
    float best_sum;
} orc_mt_job;

static void *orc_mt_worker(void *arg) {
    orc_mt_job *j = (orc_mt_job *)arg;
    orc_est *e = orc_est_new(j->kind, j->pts, j->n, j->dlt_mode);
    float models[90];
    int best_cnt = 0;
    float best_sum = 0.f;
    for (int it = 0; it < j->count; it++) {
        int nm = orc_est_estimate(e, j->samples + (size_t)it * j->m, models);
        for (int i = 0; i < nm; i++) {
            int cnt;
            float sum;
            orc_quality(e, models + 9 * i, j->thr, &cnt, &sum, NULL);
            if (score_bigger(cnt, sum, best_cnt, best_sum)) {
                best_cnt = cnt;
                best_sum = sum;
            }
        }
    }
    orc_est_free(e);
    j->best_cnt = best_cnt;
    j->best_sum = best_sum;
    return NULL;
}

double orc_hypothesis_loop_mt(int kind, const float *points, unsigned int n, int dlt_mode, float thr,
                              unsigned int seed, int count, int threads, int *best_cnt) {
    if (threads < 1) threads = 1;
    orc_est *e0 = orc_est_new(kind, points, n, dlt_mode);
    if (!e0) return -1.0;
    const int m = orc_est_sample_size(e0);
    orc_est_free(e0);
    int *samples = (int *)malloc(sizeof(int) * (size_t)m * (size_t)count);
    orc_srandom(seed);
    orc_uniform *u = orc_uniform_new(n, (unsigned int)m);
    orc_uniform_samples(u, samples, count);
    orc_uniform_free(u);
    orc_mt_job *jobs = (orc_mt_job *)calloc((size_t)threads, sizeof(orc_mt_job));
    pthread_t *tid = (pthread_t *)calloc((size_t)threads, sizeof(pthread_t));
    int start = 0;
    for (int t = 0; t < threads; t++) {
        int c = count / threads + (t < count % threads ? 1 : 0);
        jobs[t] = (orc_mt_job){kind, dlt_mode, m, c, points, n, samples + (size_t)start * m, thr, 0, 0.f};
        start += c;
    }
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int t = 0; t < threads; t++) pthread_create(&tid[t], NULL, orc_mt_worker, &jobs[t]);
    for (int t = 0; t < threads; t++) pthread_join(tid[t], NULL);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    int bc = 0;
    float bs = 0.f;
    for (int t = 0; t < threads; t++)
        if (score_bigger(jobs[t].best_cnt, jobs[t].best_sum, bc, bs)) {
            bc = jobs[t].best_cnt;
            bs = jobs[t].best_sum;
        }
    if (best_cnt) *best_cnt = bc;
    free(samples);
    free(jobs);
    free(tid);
    return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}

/* ------------------------------------------------------------ generator */
/* Generate2DLinePoints (generator/generator.cpp:98-148), SURVEY Q25: fp32 arithmetic on
 * glibc rand(); sin/cos/sqrt are the C double functions. */
void orc_generate_line2d(unsigned int seed, float noise, int inliers, int outliers, int border_x, int border_y,
                         float *pts, float *gt) {
    srand(seed);
    orc_generate_line2d_next(noise, inliers, outliers, border_x, border_y, pts, gt);
}

/* The same, continuing the process's rand() stream: generate_syntectic_dataset
 * (generator/generator.cpp:6-67) calls Generate2DLinePoints for its eight scenes in a row
 * without reseeding (default seed 1), which is how dataset/line2d/ was written. */
void orc_generate_line2d_next(float noise, int inliers, int outliers, int border_x, int border_y, float *pts,
                              float *gt) {
    const float RM = (float)RAND_MAX;
    float alpha = (float)(M_PI * (double)(float)rand() / (double)RAND_MAX);
    float nx = (float)sin((double)alpha);
    float ny = (float)cos((double)alpha);
    float tx = -ny, ty = nx;
    float cx = (float)(border_x / 2), cy = (float)(border_y / 2);
    float c = -(nx * cx + ny * cy);
    gt[0] = nx;
    gt[1] = ny;
    gt[2] = c;
    for (int i = 0; i < outliers; i++) {
        pts[2 * i] = (float)border_x * (float)rand() / RM;
        pts[2 * i + 1] = (float)border_y * (float)rand() / RM;
    }
    float diag = (float)sqrt((double)(border_x * border_x + border_y * border_y));
    for (int i = outliers; i < inliers + outliers; i++) {
        for (;;) {
            float t = (float)rand() / RM - 0.5f;
            float x = cx + t * tx * diag;
            if (x < 0 || x > (float)border_x) continue;
            float y = cy + t * ty * diag;
            if (y < 0 || y > (float)border_y) continue;
            x = x + nx * noise * (float)rand() / RM - noise / 2;
            y = y + ny * noise * (float)rand() / RM - noise / 2;
            pts[2 * i] = x;
            pts[2 * i + 1] = y;
            break;
        }
    }
}
