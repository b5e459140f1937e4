"""The batch record of every throughput scorer (k_argmax_part / k_argmax_final, the h16 finish that
k_argmax_part<true> restates, k_multi_argmax) against tests/helpers/record_ref.py: the slot that wins
under record_better (count, then Σ as fp32, then the earlier slot), hyp_index = first_hyp + slot // spk,
the model's bits.  Every case drives the throughput entry point -- hypothesize_score(samples=...,
per_hypothesis=False), which scores with the context's chunk count -- and then reads last_counts.

The inputs are tests/helpers/record_cases.py's; tests/test_batch_record_cpu.py asserts what makes them
meaningful (one slot at the maximum of the unique-best batches, many at count == n of the count-tie
batches).  Every comparison is exact, or uses the Σ bound the suite already states for the path
(tests/helpers/geometry.py h16_sum_bound / e16_sum_bound)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import geometry as G
from tests.helpers import prosac_ref
from tests.helpers import record_cases as cases
from tests.helpers import record_child
from tests.helpers import record_ref as ref

pytestmark = pytest.mark.gpu

# name: (estimator, settings) -- variant / chunks: set_score_variant / set_score_chunks (None: the
# default); h16 / e16: USAC_H16 / USAC_E16 while the context is created; sprt: set_sprt(True)
PATHS = {
    "H-exact": ("H", dict(variant=1, chunks=1)),           # k_score_h
    "H-hf": ("H", dict(variant=0, chunks=1)),              # k_score_hf, exact Σ
    "H-h16": ("H", dict(variant=0, chunks=8)),             # k_score_h16, finish in k_argmax_part<true>
    "H-hf8": ("H", dict(variant=0, chunks=8, h16="0")),    # k_score_hf over 8 chunks
    "H-sprt": ("H", dict(sprt=True)),
    "F-exact": ("F", dict(variant=1, chunks=4)),           # k_score_f (its launcher takes 1, 2, 4 or 8 chunks)
    "F-f2": ("F", dict(variant=0, chunks=1)),              # k_score_f2, exact Σ
    "F-f2x64": ("F", dict(variant=0, chunks=64)),          # k_score_f2 over 64 chunks
    "F-sprt": ("F", dict(sprt=True)),
    "E-exact": ("E", dict(variant=1, chunks=4)),
    "E-f2": ("E", dict(variant=0, chunks=1)),
    "E-e16": ("E", dict(variant=0, chunks=8)),             # k_score_e16
    "E-f2x8": ("E", dict(variant=0, chunks=8, e16="0")),   # k_score_f2 over 8 chunks
    "L-1": ("L", dict(chunks=1)),
    "L-8": ("L", dict(chunks=8)),
}
NO_SPRT = [p for p, (_, cfg) in PATHS.items() if not cfg.get("sprt")]
APPROX = {"H-h16": "h16", "E-e16": "e16"}  # Σ from integer chunk partials, within the stated bounds


@contextlib.contextmanager
def open_path(usac, path, pts):
    kind, cfg = PATHS[path]
    env = {"USAC_H16": cfg.get("h16", "1"), "USAC_E16": cfg.get("e16", "1")}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = usac.Context(cases.estimator(usac, kind), pts)  # the flags are read here
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        if cfg.get("variant") is not None:
            ctx.set_score_variant(cfg["variant"])
        if cfg.get("chunks") is not None:
            ctx.set_score_chunks(cfg["chunks"])
        if cfg.get("sprt"):
            ctx.set_sprt(True, seed=1)
        yield ctx
    finally:
        ctx.close()


def run_batch(ctx, samples, thr, first_hyp=0):
    """One throughput batch of host samples -> (record dict, counts, sums) over its S = B * spk slots."""
    _, _, rec = ctx.hypothesize_score(samples=samples, thr=thr, first_hyp=first_hyp, per_hypothesis=False)
    c, s = ctx.last_counts(len(samples) * ctx.spk)
    return rec, c, s


def slot_models(ctx, samples):
    """ctx.estimate_models as one row per slot (S x 9)"""
    m, _ = ctx.estimate_models(samples)
    return np.ascontiguousarray(m).reshape(len(samples) * ctx.spk, 9)


def check_own(ctx, samples, thr, first_hyp, what):
    """the record equals record_ref.record over the path's own counts and Σ; -> (rec, counts, sums, want)"""
    rec, c, s = run_batch(ctx, samples, thr, first_hyp)
    want = ref.record(c, s, slot_models(ctx, samples), ctx.spk, first_hyp)
    ref.assert_record(rec, want, what)
    return rec, c, s, want


_CACHE = {}


def unique_case(oracle, kind):
    """-> (points, base batch, thr, best slot, best row, filler row); the base batch of E is tiled to
    4 352 rows so that every estimator has rows 2 047 and 2 048"""
    if ("u", kind) not in _CACHE:
        pts, base, thr = cases.unique_best(oracle, kind)
        c, s, _ = cases.oracle_scores(oracle, kind, pts, base, thr)
        tied, _, _ = cases.top(c, s)
        assert len(tied) == 1
        spk = cases.SPK[kind]
        per_row = np.where(c >= 0, c, 0).reshape(-1, spk).max(1)
        _CACHE["u", kind] = (pts, base, thr, int(tied[0]), int(tied[0]) // spk, int(np.argmin(per_row)))
    return _CACHE["u", kind]


def tie_case(oracle, kind, n):
    if ("t", kind, n) not in _CACHE:
        _CACHE["t", kind, n] = cases.count_tie(oracle, kind, n)
    return _CACHE["t", kind, n]


# ------------------------------------------------------------------ a. own-input argmax
SIZES = (1, 63, 65, 255, 257, 2047, 2049, 4097)  # the 64-lane, 256-thread and 2 048-slot edges


@pytest.mark.parametrize("path", list(PATHS))
def test_record_is_argmax_of_own_counts(usac, oracle, path):
    """33 all-inlier points; B = 1, 63, 65, 255, 257, 2047, 2049, 4097 rows of the count-tie batch
    (2 304 / 1 024 rows, tiled; three slots per row for F): the record is record_ref.record over the
    path's own last_counts, models from estimate_models, bit for bit."""
    kind = PATHS[path][0]
    pts, base, thr = tie_case(oracle, kind, 33)
    with open_path(usac, path, pts) as ctx:
        for B in SIZES:
            samples = ref.tiled(base, B)
            first = 1000 + B
            rec, c, s, want = check_own(ctx, samples, thr, first, (path, B))
            if B >= len(base) and not PATHS[path][1].get("sprt"):  # the whole base batch: its ties are in
                assert want["valid"] and rec["inliers"] == 33 and (c == 33).sum() >= 4, (path, B)


# ------------------------------------------------------------------ b. placed ties
def tie_rows(kind, rows):
    """rows for the copies of the best row: slots 5, 70, 261, 2047, 2048 and the last one -- for F the
    rows of those slots (slot // 3; slot 2048's is the one after slot 2047's, so that the copies' slots
    3 r + j lie on both sides of k_argmax_part's 2 048-slot edge)"""
    if kind == "F":
        return [1, 23, 87, 682, 683, rows - 1]
    return [5, 70, 261, 2047, 2048, rows - 1]


@pytest.mark.parametrize("path", NO_SPRT)
def test_placed_ties_earliest_wins(usac, oracle, path):
    """1 000 points; 4 352 rows (2 048 for F: 6 144 slots) whose only best row is copied to rows
    {5, 70, 261, 2047, 2048, last} (F: {1, 23, 87, 682, 683, last}); the earliest copy wins, then the
    earliest is dropped until one is left.  The copies' counts and Σ bits are identical, whatever the slot."""
    kind = PATHS[path][0]
    pts, base, thr, best_slot, best_row, filler = unique_case(oracle, kind)
    spk, j = cases.SPK[kind], best_slot % cases.SPK[kind]
    rows = max(len(base), 2048 if kind == "F" else 4352)
    base = ref.tiled(base, rows)
    pos = tie_rows(kind, rows)
    first = 7
    with open_path(usac, path, pts) as ctx:
        while pos:
            samples = ref.tied_batch(base, best_row, filler, pos)
            rec, c, s, want = check_own(ctx, samples, thr, first, (path, pos))
            slots = [spk * r + j for r in pos]
            assert (c[slots] == c[slots[0]]).all(), (path, pos)
            assert c[slots[0]] == c.max() and (c == c.max()).sum() == len(pos), (path, pos)
            sb = s[slots].view(np.int32)
            assert (sb == sb[0]).all(), (path, pos, "the Σ of a model depends on its slot", sb.tolist())
            assert rec["hyp_index"] == first + pos[0], (path, pos)
            pos = pos[1:]


# ------------------------------------------------------------------ c. more than 256 partials
def _partial(slot):
    return slot // 2048


@pytest.mark.parametrize("path,rows", [("H-h16", 524289), ("H-h16", 260 * 2048 + 1),
                                       ("F-f2x64", 174763), ("F-f2x64", 177495)])
def test_more_than_256_partials(usac, oracle, path, rows):
    """1 000 points; the base batch tiled to 524 289 slots (H; F: 174 763 rows, the smallest B with
    3 B > 524 288) = 257 partials of k_argmax_part, and to 532 481 slots (F: 177 495 rows) = 261 partials.
    Every copy of the best row is the filler except three: in partials 0, 3 and the last at the smaller
    size, in partials 3, 259 (one lane of k_argmax_final's strided loop) and the last at the larger.  The
    earliest wins; dropped, the next.  The expected slot comes from the construction."""
    kind = PATHS[path][0]
    pts, base, thr, best_slot, best_row, filler = unique_case(oracle, kind)
    spk, j = cases.SPK[kind], best_slot % cases.SPK[kind]
    S = rows * spk
    nparts = (S + 2047) // 2048
    assert nparts > 256
    targets = (0, 3) if nparts < 260 else (3, 259)
    pos = [(2048 * p) // spk + 2 for p in targets] + [rows - 1]
    parts = [_partial(spk * r + j) for r in pos]
    assert parts[:2] == list(targets) and parts[2] > parts[1] and parts[2] >= 255
    if nparts >= 260:
        assert parts[0] % 256 == parts[1] % 256 and parts[2] == nparts - 1
    tiled = ref.tiled(base, rows)
    first = 11
    with open_path(usac, path, pts) as ctx:
        while pos:
            samples = ref.tied_batch(tiled, best_row, filler, pos)
            rec, c, s = run_batch(ctx, samples, thr, first)
            assert rec["hyp_index"] == first + pos[0], (path, rows, pos)
            want = ref.record(c, s, lambda slot: slot_models(ctx, samples[slot // spk][None])[slot % spk], spk, first)
            assert want["slot"] == spk * pos[0] + j
            ref.assert_record(rec, want, (path, rows, pos))
            pos = pos[1:]


# ------------------------------------------------------------------ d. empty and nearly empty batches
@pytest.mark.parametrize("path", [p for p in NO_SPRT if p[0] in "FE"])
def test_empty_and_nearly_empty_batches(usac, oracle, path):
    """1 000 points; 4 097 rows (F: 12 291 slots), every sample degenerate (points that share a
    coordinate, a non-finite point): valid == 0, inliers == 0, a zero model, hyp_index == first_hyp;
    then the same batch with one healthy sample in the last row: that row."""
    kind = PATHS[path][0]
    pts, thr, bad, healthy = cases.degenerate(oracle, kind)  # the oracle finds no model for `bad`: the CPU test
    B, first = 4097, 2 ** 33 + 5
    samples = ref.tiled(bad, B)
    with open_path(usac, path, pts) as ctx:
        rec, c, s, want = check_own(ctx, samples, thr, first, (path, "empty"))
        assert (c < 0).all()
        assert not rec["valid"] and rec["inliers"] == 0 and rec["hyp_index"] == first
        assert not rec["model"].view(np.int32).any()
        samples[B - 1] = healthy
        rec, c, s, want = check_own(ctx, samples, thr, first, (path, "one healthy row"))
        assert (c[: (B - 1) * ctx.spk] < 0).all()
        assert rec["valid"] and rec["hyp_index"] == first + B - 1 and rec["inliers"] > cases.M[kind]


# ------------------------------------------------------------------ e. the approximate-Σ contract
@pytest.mark.parametrize("n", [16, 33])
@pytest.mark.parametrize("path", ["H-h16", "H-hf8", "E-e16", "E-f2x8", "F-f2x64"])
def test_chunked_winner_within_the_sum_bounds(usac, oracle, path, n):
    """16 / 33 all-inlier points, the count-tie batch (2 304 rows H, 1 024 E / F).  Exact counts and Σ from
    variant 1, one chunk.  The chunked record's slot w has count[w] == the maximum, and for h16 / e16
    Σ_exact[w] >= Σ_exact[t] - (b(w) + b(t)), t the exact winner, b the path's stated Σ bound: each
    approximate Σ lies within b of the exact one and the path preferred w to t.  The chunked hf / f2
    paths have no stated Σ bound: the count half only."""
    kind = PATHS[path][0]
    pts, base, thr = tie_case(oracle, kind, n)
    with open_path(usac, kind + "-exact", pts) as ctx:
        ctx.set_score_chunks(1)
        ce, se, be = ctx.hypothesize_score(samples=base, thr=thr)
    t = ref.best_slot(ce, se)
    tied = int((ce == ce.max()).sum())
    assert ce.max() == n and tied >= 4
    with open_path(usac, path, pts) as ctx:
        rec, c, s, want = check_own(ctx, base, thr, 0, (path, n))
    np.testing.assert_array_equal(c, ce)
    w = want["slot"]
    print("%s n=%d: %d slots tied at count %d, chunked winner %d, exact winner %d, same %s"
          % (path, n, tied, n, w, t, w == t))
    assert rec["inliers"] == ce.max() and ce[w] == ce.max()
    if path in APPROX:
        b = G.h16_sum_bound(se, ce, pts, thr) if APPROX[path] == "h16" else G.e16_sum_bound(se, ce, thr)
        assert (np.abs(s.astype(np.float64) - se.astype(np.float64)) <= b)[ce >= 0].all()
        assert float(se[w]) >= float(se[t]) - (b[w] + b[t]), (path, n, w, t)


# ------------------------------------------------------------------ f. the two finishes
def test_two_finishes(usac, oracle, tmp_path, monkeypatch):
    """The h16 finish inside k_argmax_part<true> against k_h16_finish + the plain argmax (USAC_H16_DEFER=0,
    read once per process: one child process): the 4 352-row tied batch over 1 000 points and the 4 097-row
    batch over the 33 all-inlier points -- counts, Σ bits and the record are the same."""
    pts, base, thr, _, best_row, filler = unique_case(oracle, "H")
    tied = ref.tied_batch(base, best_row, filler, tie_rows("H", len(base)))
    pts33, base33, _ = tie_case(oracle, "H", 33)
    batches = [(pts, tied), (pts33, ref.tiled(base33, 4097))]
    first = 2 ** 40 + 3
    assert os.environ.get("USAC_H16_DEFER", "1") != "0"
    monkeypatch.setenv("USAC_H16", "1")
    mine = {}
    for i, (p, b) in enumerate(batches):
        r = record_child.run_batches(usac, p, thr, [b], first)
        mine.update({k[:-1] + str(i): v for k, v in r.items()})
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, thr=thr, first_hyp=np.uint64(first), **{"pts%d" % i: p for i, (p, _) in enumerate(batches)},
             **{"batch%d" % i: b for i, (_, b) in enumerate(batches)})
    env = dict(os.environ, USAC_H16_DEFER="0", USAC_H16="1")
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "record_child.py"), inp, outp],
                          env=env, timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    z = np.load(outp)
    assert sorted(z.files) == sorted(mine)
    for k in mine:
        np.testing.assert_array_equal(z[k], mine[k], err_msg=k)
    assert int(z["hyp0"]) == first + 5 and int(z["inl1"]) == 33


# ------------------------------------------------------------------ g. a 64-bit first_hyp
FIRST64 = 2 ** 40 + 3


def stream_samples(seed, first_hyp, B, n, m):
    """usac_device.hpp draw_sample, the uniform branch: the (seed, hypothesis) stream's m distinct indices"""
    out = np.zeros((B, m), np.int32)
    for h in range(B):
        st = (seed ^ (((first_hyp + h) * 0xD1B54A32D192ED03) & prosac_ref.MASK64)) & prosac_ref.MASK64
        smp = []
        prosac_ref.draw_unique(st, m, n, smp)
        out[h] = smp
    return out


@pytest.mark.parametrize("kind", ["H", "F", "E"])
def test_first_hyp_beyond_32_bits(usac, oracle, kind):
    """1 000 points, device sampler, B = 192, first_hyp = 2^40 + 3: draw_samples is the Python stream, the
    batch's counts are those of the same samples passed from the host, the record is record_ref.record
    with that first_hyp.  Then a MultiContext of two problems, R = 64, through k_multi_argmax."""
    pts, _, thr, _, _, _ = unique_case(oracle, kind)
    B, seed = 192, 12345
    with open_path(usac, kind + "-exact", pts) as ctx:
        drawn = ctx.draw_samples(B, seed, FIRST64)
        np.testing.assert_array_equal(drawn, stream_samples(seed, FIRST64, B, len(pts), ctx.m))
        assert (drawn != ctx.draw_samples(B, seed, FIRST64 % 2 ** 32)).any()
        _, _, rec = ctx.hypothesize_score(B=B, seed=seed, first_hyp=FIRST64, thr=thr, per_hypothesis=False)
        c, s = ctx.last_counts(B * ctx.spk)
        models = slot_models(ctx, drawn)
        ref.assert_record(rec, ref.record(c, s, models, ctx.spk, FIRST64), (kind, "device sampler"))
        assert rec["valid"] and rec["hyp_index"] >= FIRST64
        _, c2, s2 = run_batch(ctx, drawn, thr, FIRST64)
        np.testing.assert_array_equal(c2, c)
        np.testing.assert_array_equal(s2.view(np.int32), s.view(np.int32))
        sets, R, seeds = [pts, pts[:700]], 64, [seed, seed + 1]
        make = usac.MultiContext.essential if kind == "E" else (lambda p: usac.MultiContext(cases.estimator(usac, kind), p))
        with make(sets) as mc:
            md = mc.draw_samples(R, seeds, FIRST64)
            cm, sm, best = mc.hypothesize_score(R, seeds, first_hyp=FIRST64, thr=thr)
        for p, q in enumerate(sets):
            np.testing.assert_array_equal(md[p], stream_samples(seeds[p], FIRST64, R, len(q), ctx.m))
            with open_path(usac, kind + "-exact", q) as cq:
                mq = slot_models(cq, md[p])
            ref.assert_record(best[p], ref.record(cm[p], sm[p], mq, ctx.spk, FIRST64), (kind, "multi", p))
            assert best[p]["valid"]


# ------------------------------------------------------------------ h. k_multi_argmax
@pytest.mark.parametrize("kind,R,positions", [
    ("H", 64, ([5, 63], [17, 40, 41])),
    ("H", 256, ([70, 255], [5, 200, 201])),
    ("F", 128, ([23, 100, 127], [90, 127])),   # 384 slots: rows 90, 100 and 127 lie in the strided loop
])
def test_multi_argmax_placed_ties(usac, oracle, kind, R, positions):
    """MultiContext.hypothesize_score(samples=...) over two problems of 1 000 points, R = 64 / 256 (H) and
    128 (F, 384 slots): the first R rows of the base batch with the only best row copied to different rows
    in each problem.  Each problem's record is its earliest copy and record_ref.record over its own counts;
    then the earliest copies are dropped, down to one per problem."""
    pts, base, thr, best_slot, best_row, filler = unique_case(oracle, kind)
    spk = cases.SPK[kind]
    pool = np.concatenate([base[:R], base[best_row][None], base[filler][None]])
    pos = [list(p) for p in positions]
    first = 2 ** 32 + 9
    with open_path(usac, kind + "-exact", pts) as ctx, usac.MultiContext(cases.estimator(usac, kind), [pts, pts]) as mc:
        while True:
            samples = np.stack([ref.tied_batch(pool, R, R + 1, p)[:R] for p in pos])
            c, s, best = mc.hypothesize_score(R, first_hyp=first, thr=thr, samples=samples)
            _, _, best2 = mc.hypothesize_score(R, first_hyp=first, thr=thr, samples=samples, per_hypothesis=False)
            for p in range(2):
                assert (c[p] == c[p].max()).sum() == len(pos[p]), (kind, R, pos)
                assert best[p]["hyp_index"] == first + pos[p][0], (kind, R, pos)
                want = ref.record(c[p], s[p], slot_models(ctx, samples[p]), spk, first)
                assert want["slot"] == spk * pos[p][0] + best_slot % spk
                ref.assert_record(best[p], want, (kind, R, pos, p))
                ref.assert_record(best2[p], want, (kind, R, pos, p, "records alone"))
            if all(len(p) == 1 for p in pos):
                break
            pos = [p[1:] if len(p) > 1 else p for p in pos]
