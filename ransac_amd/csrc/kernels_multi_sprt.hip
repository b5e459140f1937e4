// kernels_multi_sprt.hip -- SPRT verification for multi-problem batches (DESIGN.md §8b "SPRT").
//
// The throughput SPRT of kernels_sprt.hip (k_sprt_head / k_sprt_tail, restated here) over the slots
// of a multi-problem round: the test (epsilon, delta, A) is one SprtConsts per ACTIVE ENTRY, fixed
// for the round; the points are the context's pool-ordered copy (N_total x float4, problem p's slice
// permuted by its SPRT pool), so a pool position is a wave-uniform scalar load.
//
//   head : grid (spk R / 64, A), one wave, lanes = the slots of slot tile blockIdx.x of active entry
//          blockIdx.y (H: slot a R + h; F: slot 3 (a R + h) + j, an empty slot -- count -1 from the
//          solve kernel -- stays idle).  Start pool position (blockIdx.x * 7919) mod n_p, the single
//          context's start for the same tile.  The first min(n_p, 64) pool points: counts and P =
//          a lu + b ld in fp64, rejected at the first certified P > lA; a walk that is not certified
//          (|P - lA| <= margin, or a climb >= climb) is decided by the reference's sequential fp64
//          product.  Undecided lanes go to a launch-wide survivor list.
//   tail : a 256-thread workgroup per survivor (grid-stride, fixed grid): the remaining n_p - 64
//          points in 256 contiguous chunks, a wave scan over the chunks, the sequential fall-back.
//
// A slot's result: rejected -> count -1, sum 0; accepted -> count = its inliers over all n_p points,
// sum = (float)count (sprt.hpp:276-281).  k_multi_argmax then runs over these unchanged.
// The per-entry statistics are integer wave reductions and integer atomics: deterministic.
#include <hip/hip_runtime.h>

#include "usac_device.hpp"
#include "usac_kernels.h"

namespace usac {

namespace {

constexpr uint32_t kMsHead = 64;  // the project's head length (kernels_sprt.hip kHead)

template <int EST>
__device__ __forceinline__ float msprt_error(const float *m, const float4 *__restrict__ pts, uint32_t p) {
    const float4 q = pts[p];
    if constexpr (EST == 2) return homography_error(m, m + 9, q.x, q.y, q.z, q.w);
    else return fundamental_error(m, q.x, q.y, q.z, q.w);
}

struct MultiSurvivor {
    uint32_t entry, slot;  // active entry, slot within the entry (< spk R)
    uint32_t start;        // pool position where the tail begins
    int cnt;               // inliers among the head's points
    uint32_t exact, pad;   // 1: the head could not certify the walk -> the sequential fp64 walk
    double pmin;           // min of P over the head's prefixes (P_0 = 0 included)
};
static_assert(sizeof(MultiSurvivor) == 32, "MultiSurvivor");

// the reference's own walk (sprt.hpp:209-234) from pool position `start`: good, inliers, points read
template <int EST>
__device__ bool msprt_exact_walk(const float *m, const float4 *__restrict__ pts, uint32_t n, float thr, uint32_t start,
                                 const SprtConsts &k, int &cnt, uint32_t &tested) {
    double lambda = 1.0;
    uint32_t p = start;
    cnt = 0;
    for (uint32_t t = 0; t < n; t++) {
        const bool in = msprt_error<EST>(m, pts, p) < thr;
        cnt += in ? 1 : 0;
        const double next = lambda * (in ? k.up : k.down);
        if (++p == n) p = 0;
        if (next > k.A) {
            tested = t + 1;
            return false;
        }
        lambda = next;
    }
    tested = n;
    return true;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void add64(uint64_t *p, uint64_t v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

}  // namespace

template <int EST>
__global__ __launch_bounds__(64) void k_multi_sprt_head(const float4 *__restrict__ pool_all,
                                                        const uint32_t *__restrict__ offsets,
                                                        const MultiItem *__restrict__ items,
                                                        const SprtConsts *__restrict__ consts,
                                                        const float *__restrict__ models, uint32_t S, float thr_s,
                                                        const float *__restrict__ thrs,
                                                        int32_t *__restrict__ counts, float *__restrict__ sums,
                                                        usac_multi_sprt_stats *__restrict__ stats,
                                                        MultiSurvivor *__restrict__ surv,
                                                        uint32_t *__restrict__ surv_n, uint32_t *__restrict__ starts) {
    constexpr int NC = EST == 2 ? 18 : 9;
    const uint32_t a = blockIdx.y;
    const uint32_t prob = items[a].problem;
    const float thr = thrs ? thrs[prob] : thr_s;  // per-problem thresholds: the workgroup's problem's
    const uint32_t base = offsets[prob], n = offsets[prob + 1] - base;
    const float4 *__restrict__ pts = pool_all + base;
    const SprtConsts kc = consts[a];
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    const size_t g = (size_t)a * S + i, stride = (size_t)gridDim.y * S;
    // an F slot the solve kernel left at -1 is empty: idle, keeps (-1, 0)
    const bool occ = EST == 2 ? true : counts[g] >= 0;
    float m[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) m[k] = models[(size_t)k * stride + g];
    const uint32_t start = (uint32_t)(((uint64_t)blockIdx.x * 7919u) % n);
    const uint32_t head = n < kMsHead ? n : kMsHead;
    double P = 0.0, pmin = 0.0;
    int cnt = 0;
    bool live = occ, amb = false;
    uint32_t tested = 0;
    uint32_t p = start;
    for (uint32_t t = 0; t < head; t += 4) {
        // four independent residuals per step (pool positions wave-uniform: scalar loads)
        float e[4];
        uint32_t q = p;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            e[u] = t + u < head ? msprt_error<EST>(m, pts, q) : __builtin_nanf("");
            if (++q == n) q = 0;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (live && t + u < head) {
                const bool in = e[u] < thr;
                cnt += in ? 1 : 0;
                P += in ? kc.lu : kc.ld;  // <= 64 fp64 adds: error < 1e-12
                tested++;
                if (fabs(P - kc.lA) <= kc.margin || P - pmin >= kc.climb) {
                    amb = true;  // not certified: the sequential walk decides
                    live = false;
                } else if (P > kc.lA) {
                    live = false;  // rejected
                }
                pmin = fmin(pmin, P);
            }
        }
        p = q;
        if (!__any(live)) break;
    }
    uint32_t acc = 0, rej = 0, hin = 0, hpt = 0;
    if (occ) {
        if (starts) starts[g] = start;
        if (amb && head == n) {  // no tail: walk it here
            int c2 = 0;
            uint32_t t2 = 0;
            const bool good = msprt_exact_walk<EST>(m, pts, n, thr, start, kc, c2, t2);
            counts[g] = good ? c2 : -1;
            sums[g] = good ? (float)c2 : 0.f;
            tested = t2;
            acc = good ? 1u : 0u;
            rej = good ? 0u : 1u;
            hin = good ? 0u : (uint32_t)c2;
            hpt = good ? 0u : t2;
        } else if (!live && !amb) {
            counts[g] = -1;
            sums[g] = 0.f;
            rej = 1;
            hin = (uint32_t)cnt;
            hpt = tested;
        } else if (head == n) {
            counts[g] = cnt;
            sums[g] = (float)cnt;
            acc = 1;
        } else {
            const uint32_t k = atomicAdd(surv_n, 1u);
            uint32_t nx = start + head;
            if (nx >= n) nx -= n;
            surv[k] = MultiSurvivor{a, i, nx, cnt, amb ? 1u : 0u, 0u, pmin};
        }
    } else {
        tested = 0;
        if (starts) starts[g] = 0xFFFFFFFFu;
    }
    acc = wave_sum(acc);
    rej = wave_sum(rej);
    hin = wave_sum(hin);
    hpt = wave_sum(hpt);
    const uint32_t tt = wave_sum(tested);
    if (threadIdx.x == 0) {
        usac_multi_sprt_stats *s = stats + a;
        if (acc) atomicAdd(&s->accepted, acc);
        if (rej) atomicAdd(&s->rejected_head, rej);
        if (hin) atomicAdd(&s->head_inliers, hin);
        if (hpt) atomicAdd(&s->head_points, hpt);
        if (tt) add64(&s->points_tested, tt);
    }
}

template <int EST>
__global__ __launch_bounds__(256) void k_multi_sprt_tail(const float4 *__restrict__ pool_all,
                                                         const uint32_t *__restrict__ offsets,
                                                         const MultiItem *__restrict__ items,
                                                         const SprtConsts *__restrict__ consts,
                                                         const float *__restrict__ models, uint32_t S, size_t stride,
                                                         float thr_s, const float *__restrict__ thrs,
                                                         const MultiSurvivor *__restrict__ surv,
                                                         const uint32_t *__restrict__ surv_n,
                                                         int32_t *__restrict__ counts, float *__restrict__ sums,
                                                         usac_multi_sprt_stats *__restrict__ stats) {
    constexpr int NC = EST == 2 ? 18 : 9;
    __shared__ int s_cnt[256];
    __shared__ double s_max[256], s_min[256], s_clb[256];
    __shared__ int s_exact;
    const uint32_t ns = *surv_n;
    for (uint32_t k = blockIdx.x; k < ns; k += gridDim.x) {
        const MultiSurvivor sv = surv[k];
        const uint32_t prob = items[sv.entry].problem;
        const float thr = thrs ? thrs[prob] : thr_s;  // per-problem thresholds: the survivor's problem's
        const uint32_t base = offsets[prob], n = offsets[prob + 1] - base;  // n > kMsHead: the head appended it
        const float4 *__restrict__ pts = pool_all + base;
        const SprtConsts kc = consts[sv.entry];
        usac_multi_sprt_stats *st = stats + sv.entry;
        const size_t g = (size_t)sv.entry * S + sv.slot;
        const uint32_t rest = n - kMsHead;
        const uint32_t per = (rest + 255) / 256;
        float m[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) m[c] = models[(size_t)c * stride + g];
        if (!sv.exact) {
            const uint32_t b = threadIdx.x * per;
            const uint32_t e = b + per < rest ? b + per : rest;
            int cnt = 0;
            double d = 0.0, dmax = -INFINITY, dmin = INFINITY, rmin = 0.0, clb = 0.0;
            uint32_t p = sv.start + (b < rest ? b : rest);
            if (p >= n) p -= n;
            for (uint32_t t = b; t < e; t++) {
                const bool in = msprt_error<EST>(m, pts, p) < thr;
                cnt += in ? 1 : 0;
                d += in ? kc.lu : kc.ld;  // a chunk's <= ceil(n / 256) adds
                dmax = fmax(dmax, d);
                dmin = fmin(dmin, d);
                clb = fmax(clb, d - rmin);
                rmin = fmin(rmin, d);
                if (++p == n) p = 0;
            }
            s_cnt[threadIdx.x] = cnt;
            s_max[threadIdx.x] = dmax;
            s_min[threadIdx.x] = dmin;
            s_clb[threadIdx.x] = clb;
        }
        __syncthreads();
        if (threadIdx.x < 64 && !sv.exact) {
            // wave 0: lane l holds chunks 4l .. 4l+3.  Exact inlier / point counts at every chunk
            // start by a wave scan; P there from the counts (no accumulated rounding); the prefix
            // minimum of P before each chunk by a second scan; then the first chunk (in pool
            // order) that reaches log A - kc.margin or a climb of kc.climb decides.
            const uint32_t l = threadIdx.x;
            int cc[4];
            double cmax[4], cmin[4], cclb[4];
            uint32_t clen[4];
            int lane_c = 0;
            uint32_t lane_len = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t j = 4 * l + u;
                const uint32_t cb = j * per, ce = cb + per < rest ? cb + per : rest;
                clen[u] = cb < ce ? ce - cb : 0;
                cc[u] = s_cnt[j];
                cmax[u] = s_max[j];
                cmin[u] = s_min[j];
                cclb[u] = s_clb[j];
                lane_c += clen[u] ? cc[u] : 0;
                lane_len += clen[u];
            }
            // exclusive scan of (inliers, points) over lanes
            int ex_c = lane_c;
            uint32_t ex_len = lane_len;
            for (int off = 1; off < 64; off <<= 1) {
                const int vc = __shfl_up(ex_c, off, 64);
                const uint32_t vl = __shfl_up(ex_len, off, 64);
                if ((int)l >= off) {
                    ex_c += vc;
                    ex_len += vl;
                }
            }
            ex_c -= lane_c;
            ex_len -= lane_len;
            // P at each chunk start; hi = its largest prefix P; lo = its smallest
            double hi[4], lo[4];
            int a = sv.cnt + ex_c;
            uint32_t t = kMsHead + ex_len;
            double lane_min = INFINITY;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double P0 = (double)a * kc.lu + (double)(int)(t - (uint32_t)a) * kc.ld;
                hi[u] = clen[u] ? P0 + cmax[u] : -INFINITY;
                lo[u] = clen[u] ? P0 + cmin[u] : INFINITY;
                lane_min = fmin(lane_min, lo[u]);
                a += clen[u] ? cc[u] : 0;
                t += clen[u];
            }
            // exclusive prefix minimum over lanes (the head's minimum included)
            double ex_min = lane_min;
            for (int off = 1; off < 64; off <<= 1) {
                const double v = __shfl_up(ex_min, off, 64);
                if ((int)l >= off) ex_min = fmin(ex_min, v);
            }
            const double prev_lane_min = __shfl_up(ex_min, 1, 64);
            double mb = fmin(sv.pmin, l ? prev_lane_min : INFINITY);
            // first deciding chunk of this lane: 0..3, or 4 = none
            int first = 4;
            bool rej = false;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (first == 4 && clen[u]) {
                    const bool climb = fmax(cclb[u], hi[u] - mb) >= kc.climb;
                    if (climb || hi[u] > kc.lA - kc.margin) {
                        first = u;
                        rej = !climb && hi[u] > kc.lA + kc.margin;
                    }
                    mb = fmin(mb, lo[u]);
                }
            }
            const uint64_t hit = __ballot(first < 4);
            int exact = 0;
            if (hit) {
                const int src = __builtin_ctzll(hit);  // the lane holding the first deciding chunk
                const int srej = __builtin_amdgcn_readlane(rej ? 1 : 0, src);
                const int sfirst = __builtin_amdgcn_readlane(first, src);
                if (!srej) {
                    exact = 1;
                } else if (l == 0) {
                    counts[g] = -1;
                    sums[g] = 0.f;
                    // points read up to the deciding chunk's end (an upper bound of the test's)
                    const uint32_t ce = (4u * (uint32_t)src + (uint32_t)sfirst + 1u) * per;
                    atomicAdd(&st->rejected_tail, 1u);
                    add64(&st->points_tested, ce < rest ? ce : rest);
                }
            } else if (l == 0) {
                const int total = sv.cnt + __builtin_amdgcn_readlane(ex_c + lane_c, 63);
                counts[g] = total;
                sums[g] = (float)total;
                atomicAdd(&st->accepted, 1u);
                add64(&st->points_tested, rest);
            }
            if (l == 0) s_exact = exact;
        }
        if (threadIdx.x == 0 && sv.exact) s_exact = 1;
        __syncthreads();
        if (s_exact && threadIdx.x == 0) {  // not certified: the reference's sequential walk
            int c2 = 0;
            uint32_t t2 = 0;
            const uint32_t start0 = (sv.start + n - kMsHead) % n;
            const bool good = msprt_exact_walk<EST>(m, pts, n, thr, start0, kc, c2, t2);
            counts[g] = good ? c2 : -1;
            sums[g] = good ? (float)c2 : 0.f;
            atomicAdd(good ? &st->accepted : &st->rejected_tail, 1u);
            if (t2 > kMsHead) add64(&st->points_tested, t2 - kMsHead);
        }
        __syncthreads();
    }
}

hipError_t launch_multi_sprt_score(hipStream_t st, const MultiRound &r) {
    if (!r.sprt || r.A == 0 || r.R == 0 || r.R % 64) return hipErrorInvalidValue;
    const MultiSprt &s = *r.sprt;
    const uint32_t spk = r.estimator == USAC_FUNDAMENTAL ? 3u : 1u, S = spk * r.R;
    const size_t total = (size_t)r.A * S;
    hipError_t e = hipMemsetAsync(s.surv_n, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(s.stats, 0, sizeof(usac_multi_sprt_stats) * (size_t)r.A, st);
    if (e != hipSuccess) return e;
    const dim3 grid(S / 64, r.A);
    const dim3 tgrid((uint32_t)(total < 2048 ? total : 2048));
    MultiSurvivor *sv = static_cast<MultiSurvivor *>(s.surv);
#define MS(E)                                                                                                        \
    do {                                                                                                             \
        hipLaunchKernelGGL(k_multi_sprt_head<E>, grid, dim3(64), 0, st, s.pool_pts, r.offsets, r.items, s.consts,    \
                           r.models, S, r.thr, r.thrs, r.counts, r.sums, s.stats, sv, s.surv_n, s.starts);                   \
        if (s.tail)                                                                                                  \
            hipLaunchKernelGGL(k_multi_sprt_tail<E>, tgrid, dim3(256), 0, st, s.pool_pts, r.offsets, r.items,        \
                               s.consts, r.models, S, total, r.thr, r.thrs, sv, s.surv_n, r.counts, r.sums, s.stats);        \
    } while (0)
    if (r.estimator == USAC_HOMOGRAPHY) MS(2);
    else if (r.estimator == USAC_FUNDAMENTAL) MS(3);
    else return hipErrorInvalidValue;
#undef MS
    return hipGetLastError();
}

size_t multi_sprt_survivor_bytes() { return sizeof(MultiSurvivor); }

}  // namespace usac
