"""Python restatements for the multi-problem PROSAC tests: the reference's sampler state machine
(prosac_sampler.hpp:62-172), the device random stream (usac_device.hpp splitmix64 / draw_unique), the
multi-problem sampler rule built from the two, and the plain termination scan
(prosac_termination_criteria.hpp:44-201).  No GPU, no library state."""
import functools
import math

import numpy as np

T_N = 200000
MASK64 = (1 << 64) - 1
UNIFORM_OVER_N = 0xFFFFFFFF


def growth_table(n, m):
    """prosac_sampler.hpp:62-114"""
    return list(_growth_table(n, m))


@functools.lru_cache(maxsize=None)
def _growth_table(n, m):
    g = [0] * n
    t_n = float(T_N)
    for i in range(m):
        t_n *= float(m - i) / (n - i)
    t_prime = 1
    for i in range(n):
        if i + 1 <= m:
            g[i] = t_prime
            continue
        t_next = float(i + 1) * t_n / (i + 1 - m)
        g[i] = t_prime + int(math.ceil(t_next - t_n))
        t_n = t_next
        t_prime = g[i]
    return tuple(g)


class SamplerState:
    """ProsacSampler::generateSample's state (prosac_sampler.hpp:117-172) without the random draws:
    step(term_len) returns the kind of the sample it would draw -- the subset size of a PROSAC sample,
    0 for the uniform draw over [0, term_len], UNIFORM_OVER_N past T_N -- and advances the state."""

    def __init__(self, n, m):
        self.g, self.n, self.m = growth_table(n, m), n, m
        self.subset = self.largest = m
        self.hyp = 1

    def step(self, term_len):
        if self.hyp > T_N:
            return UNIFORM_OVER_N
        if self.subset > term_len:
            return 0
        if self.hyp > self.g[self.subset - 1]:
            self.subset = min(self.subset + 1, self.n)
            self.largest = max(self.largest, self.subset)
        self.hyp += 1
        return self.subset


def splitmix64(st):
    st = (st + 0x9E3779B97F4A7C15) & MASK64
    z = st
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return st, z ^ (z >> 31)


def draw_unique(st, k, rng, taken):
    """k more distinct indices of [0, rng) appended to taken, from the stream st"""
    for _ in range(k):
        while True:
            st, r = splitmix64(st)
            v = ((r >> 32) * rng) >> 32
            if v not in taken:
                break
        taken.append(v)
    return st


def multi_prosac_samples(seed, first_hyp, R, n, m, clock, term_len):
    """The multi-problem PROSAC sampler's round (include/usac_gpu.h, ABI 17): R x m indices."""
    g = growth_table(n, m)

    def s(t):
        return min(n, m + sum(1 for i in range(m - 1, n) if g[i] < t))

    out = np.zeros((R, m), dtype=np.int32)
    for j in range(R):
        st = (seed ^ (((first_hyp + j) * 0xD1B54A32D192ED03) & MASK64)) & MASK64
        t = clock + j
        smp = []
        if t > T_N:
            draw_unique(st, m, n, smp)
        elif s(t - 1) > term_len:
            draw_unique(st, m, term_len + 1, smp)
        else:
            draw_unique(st, m - 1, s(t) - 1, smp)
            smp.append(s(t) - 1)
        out[j] = smp
    return out


def non_random_table(n_pts, m):
    """prosac_termination_criteria.hpp:44-119 (beta = 0.05, psi = 0.95 in float, as the reference)"""
    return list(_non_random_table(n_pts, m))


@functools.lru_cache(maxsize=None)
def _non_random_table(n_pts, m):
    psi32, beta32 = np.float32(0.95), np.float32(0.05)
    beta = float(beta32)
    ratio = float(beta32 / (np.float32(1) - beta32))  # float arithmetic in the reference
    rest = float(np.float32(1) - psi32)
    nr = [0] * n_pts
    for n in range(m + 1, n_pts + 1):
        if n - 1 > 1000:
            nr[n - 1] = nr[n - 2]
            continue
        pn = [0.0] * n
        pn[m] = beta * math.pow(1 - beta, n - m - 1) * (n - m)
        prev = pn[m]
        for i in range(m + 2, n + 1):
            if i == n:
                pn[n - 1] = math.pow(beta, n - m)
                break
            pn[i - 1] = prev * ratio * (float(n - i) / (i - m + 1))
            prev = pn[i - 1]
        acc, imin = 0.0, 0
        for i in range(n, m, -1):
            acc += pn[i - 1]
            if acc < rest:
                imin = i
            else:
                break
        nr[n - 1] = imin
    return tuple(nr)


class PlainScan:
    """prosac_termination_criteria.hpp:148-201 as written: every candidate's standard-termination
    value computed and applied in place.  std_term(count, points) is the two-argument
    StandardTerminationCriteria::getUpBoundIterations (ransac_amd.std_termination with m, p, max)."""

    K_MIN = 20

    def __init__(self, n, m, std_term):
        self.n, self.m, self.std = n, m, std_term
        self.g = growth_table(n, m)
        self.non_random = non_random_table(n, m)
        self.maximality = [10000] * n
        self.term_len = n
        self.ties = 0  # candidates whose value equalled the running minimum (the tie rule decided)

    def scan(self, hyp_count, flags, largest):
        """-> (bound, candidates [(i, count)]); flags: n booleans"""
        n = self.n
        max_samples = self.maximality[self.term_len - 1]
        count = sum(1 for i in range(self.K_MIN) if flags[i])
        cands = []
        for i in range(self.K_MIN, n):
            count += 1 if flags[i] else 0
            if self.non_random[i] < count:
                self.non_random[i] = count
                if i == n - 1 or (flags[i] and not flags[i + 1]):
                    cands.append((i, count))
                    samples = self.std(count, i + 1)
                    if i + 1 < largest:
                        samples = (samples + hyp_count - self.g[i]) & 0xFFFFFFFF
                    if samples < self.maximality[i]:
                        self.maximality[i] = samples
                        self.ties += 1 if samples == max_samples else 0
                        if samples < max_samples or (samples == max_samples and i + 1 >= self.term_len):
                            self.term_len = i + 1
                            max_samples = samples
        return max_samples, cands
