// The matrix-core homography scorer's prefilter bound (ransac_amd/csrc/usac_h16.hpp h16_rows_of, DESIGN.md §6
// "Matrix-core prefilter") checked on the host against long double, pair by pair: the library's own function
// produces the fp16 rows, the tile bounds D and the slack F_m; this program only plays the parts around it.
//   slack_check <case.bin>
// case.bin: uint32 N, uint32 M, float thr, N x 4 float points, M x 9 float models.
//
// Around the function: the dataset constants as k_h16_consts derives them (box of the finite points, fp32
// centres, power-of-two scales, fmax rounded up), the fp16 features as k_h16_points rounds them (double ->
// float -> half), and the 32x32x16 tile value of a (row, point): the sixteen exact fp16 x fp16 products summed
// in float32 -- in ascending, descending and pairwise order, the instruction's own order being unspecified.
// For every (model, point) pair:
//   (a) |tile value - exact row value 2^e| <= D[r] for the three rows, the exact value (x2 Z - X, y2 Z - Y,
//       trm' Z of the fp32 model and point) in long double;
//   (b) if the packed stage A of k_score_hf keeps the pair (stage_a_keep2's FMA chains, fp32), the tile keeps it:
//       |ex_m| <= R and |ey_m| <= R with R = |zr_m| + F_m in fp32, as k_score_h16 tests it.
// A hypothesis without a prefilter (F_m = +inf: D = +inf, zero rows or not) has nothing to check in (a); (b)
// runs for it like for any other.  Prints the largest error / bound ratio per row and "ok"; returns 1 at the
// first violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "usac_h16.hpp"

namespace {

using usac::H16Consts;
using usac::half8;

double pow2_at_least(double v) { return v > 0 ? std::ldexp(1.0, std::ilogb(v) + 1) : 1.0; }

void features64(const float *p, const H16Consts &k, double f[9]) {
    const double u = ((double)p[0] - k.cx1) / k.s1, v = ((double)p[1] - k.cy1) / k.s1;
    const double pp = ((double)p[2] - k.cx2) / k.s2, q = ((double)p[3] - k.cy2) / k.s2;
    const double g[9] = {u, v, 1.0, pp * u, pp * v, pp, q * u, q * v, q};
    for (int c = 0; c < 9; c++) f[c] = g[c];
}

bool finite4(const float *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]); }

H16Consts consts_of(const std::vector<float> &pts, uint32_t n) {
    double lo[4], hi[4];
    float ext[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4; k++) lo[k] = INFINITY, hi[k] = -INFINITY;
    for (uint32_t i = 0; i < n; i++) {
        if (!finite4(&pts[4 * i])) continue;
        for (int k = 0; k < 4; k++) {
            lo[k] = std::fmin(lo[k], (double)pts[4 * i + k]);
            hi[k] = std::fmax(hi[k], (double)pts[4 * i + k]);
            ext[k] = std::fmax(ext[k], std::fabs(pts[4 * i + k]));
        }
    }
    H16Consts k;
    double cc[4];
    for (int j = 0; j < 4; j++) cc[j] = (double)(float)(0.5 * (lo[j] + hi[j]));
    k.cx1 = cc[0], k.cy1 = cc[1], k.cx2 = cc[2], k.cy2 = cc[3];
    k.s1 = pow2_at_least(std::fmax(std::fmax(hi[0] - cc[0], cc[0] - lo[0]), std::fmax(hi[1] - cc[1], cc[1] - lo[1])));
    k.s2 = pow2_at_least(std::fmax(std::fmax(hi[2] - cc[2], cc[2] - lo[2]), std::fmax(hi[3] - cc[3], cc[3] - lo[3])));
    double mx[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < n; i++) {
        if (!finite4(&pts[4 * i])) continue;
        double f[9];
        features64(&pts[4 * i], k, f);
        for (int c = 0; c < 9; c++) mx[c] = std::fmax(mx[c], std::fabs(f[c]));
    }
    for (int c = 0; c < 9; c++) k.fmax[c] = (double)std::nextafterf((float)(mx[c] * (1.0 + 0x1p-40)), INFINITY);
    k.ext = make_float4(ext[0], ext[1], ext[2], ext[3]);
    return k;
}

// the tile value in three summation orders
void tile3(const float (&g)[16], const float (&f)[16], float out[3]) {
    float t[16];
    for (int c = 0; c < 16; c++) t[c] = g[c] * f[c];  // exact: 11 x 11 significant bits
    float up = 0.f, down = 0.f;
    for (int c = 0; c < 16; c++) up += t[c];
    for (int c = 15; c >= 0; c--) down += t[c];
    for (int w = 8; w > 0; w >>= 1)
        for (int c = 0; c < w; c++) t[c] = t[c] + t[c + w];
    out[0] = up, out[1] = down, out[2] = t[0];
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream file(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
    if (raw.size() < 12) return 2;
    const uint32_t N = *reinterpret_cast<const uint32_t *>(raw.data()), M = *reinterpret_cast<const uint32_t *>(raw.data() + 4);
    const float thr = *reinterpret_cast<const float *>(raw.data() + 8);
    if (raw.size() != 12 + (size_t)N * 16 + (size_t)M * 36) return 2;
    const float *fp = reinterpret_cast<const float *>(raw.data() + 12);
    const std::vector<float> pts(fp, fp + (size_t)N * 4), models(fp + (size_t)N * 4, fp + (size_t)N * 4 + (size_t)M * 9);

    const H16Consts kc = consts_of(pts, N);
    std::vector<float> feat((size_t)N * 16, 0.f);  // the fp16 features, as floats
    for (uint32_t i = 0; i < N; i++) {
        double f[9];
        features64(&pts[4 * i], kc, f);
        for (int c = 0; c < 9; c++) feat[(size_t)i * 16 + c] = (float)(_Float16)(float)f[c];
    }
    uint32_t at_fmax = 0;  // points on the box: some |f_k| = the maximum the bound assumes
    for (uint32_t i = 0; i < N; i++) {
        double f[9];
        features64(&pts[4 * i], kc, f);
        bool hit = false;
        for (int c = 0; c < 9; c++)
            if (c != 2) hit = hit || (double)std::nextafterf((float)(std::fabs(f[c]) * (1.0 + 0x1p-40)), INFINITY) == kc.fmax[c];
        at_fmax += hit;
    }

    long double worst[3] = {0, 0, 0};
    uint64_t pairs = 0, kept_a = 0, kept_m = 0, no_prefilter = 0;
    for (uint32_t h = 0; h < M; h++) {
        float Hm[9];
        for (int c = 0; c < 9; c++) Hm[c] = models[(size_t)h * 9 + c];
        half8 rows[6];
        float Fm;
        usac::H16RowBounds b;
        usac::h16_rows_of(Hm, &kc, thr, 0, rows, &Fm, &b);
        float g[3][16];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 16; c++) g[r][c] = (float)rows[2 * r + (c >> 3)][c & 7];
        usac::HModel Ms;
        for (int c = 0; c < 9; c++) Ms.h[c] = Hm[c];
        usac::stage_a_bounds(Ms, kc.ext, 2.0f * thr);
        const float trmi = Ms.trm * 1.0009765625f;
        const bool prefilter = std::isfinite(b.D[0]);
        no_prefilter += !prefilter;
        for (uint32_t i = 0; i < N; i++) {
            const float *p = &pts[4 * i];
            const float(&f)[16] = *reinterpret_cast<const float(*)[16]>(&feat[(size_t)i * 16]);
            float m[3][3];
            for (int r = 0; r < 3; r++) tile3(g[r], f, m[r]);
            pairs++;
            if (prefilter) {
                const long double x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
                const long double X = (long double)Hm[0] * x1 + (long double)Hm[1] * y1 + Hm[2];
                const long double Y = (long double)Hm[3] * x1 + (long double)Hm[4] * y1 + Hm[5];
                const long double Z = (long double)Hm[6] * x1 + (long double)Hm[7] * y1 + Hm[8];
                const long double exact[3] = {std::ldexp(x2 * Z - X, b.e), std::ldexp(y2 * Z - Y, b.e),
                                              std::ldexp((long double)trmi * Z, b.e)};
                for (int r = 0; r < 3; r++)
                    for (int o = 0; o < 3; o++) {
                        const long double err = std::fabs((long double)m[r][o] - exact[r]);
                        if (!(err <= (long double)b.D[r])) {
                            std::printf("model %u point %u row %d order %d: |tile - exact| = %Lg > D = %g\n", h, i, r, o, err,
                                        (double)b.D[r]);
                            return 1;
                        }
                        worst[r] = std::fmax(worst[r], err / (long double)b.D[r]);
                    }
            }
            // the packed stage A of k_score_hf (usac_hscore.hpp stage_a_keep2), one point
            const float Xf = std::fmaf(Hm[1], p[1], std::fmaf(Hm[0], p[0], Hm[2]));
            const float Yf = std::fmaf(Hm[4], p[1], std::fmaf(Hm[3], p[0], Hm[5]));
            const float Zf = std::fmaf(Hm[7], p[1], std::fmaf(Hm[6], p[0], Hm[8]));
            const float exf = std::fmaf(p[2], Zf, -Xf), eyf = std::fmaf(p[3], Zf, -Yf);
            const bool keep_a = !(std::fmax(std::fabs(exf), std::fabs(eyf)) > std::fmaf(std::fabs(Zf), Ms.trm, Ms.F));
            kept_a += keep_a;
            bool any_m = false;
            for (int o = 0; o < 3; o++) {
                const float R = std::fabs(m[2][o]) + Fm;
                const bool keep_m = std::fabs(m[0][o]) <= R && std::fabs(m[1][o]) <= R;
                any_m = any_m || keep_m;
                if (keep_a && !keep_m) {
                    std::printf("model %u point %u order %d: stage A keeps the pair, the tile drops it (ex %g ey %g zr %g F_m %g)\n",
                                h, i, o, (double)m[0][o], (double)m[1][o], (double)m[2][o], (double)Fm);
                    return 1;
                }
            }
            kept_m += any_m;
        }
    }
    std::printf("ratio ex %.4Lf ey %.4Lf zr %.4Lf\n", worst[0], worst[1], worst[2]);
    std::printf("pairs %llu stage_a_kept %llu tile_kept %llu models_without_prefilter %llu points_at_fmax %u\n",
                (unsigned long long)pairs, (unsigned long long)kept_a, (unsigned long long)kept_m,
                (unsigned long long)no_prefilter, at_fmax);
    std::printf("ok\n");
    return 0;
}
