"""The batch record's reference (tests/helpers/record_ref.py) and the inputs of
tests/test_gpu_batch_record.py, checked on the CPU: best_slot is the sequential first-best loop under
Score::bigger, usac_merge_records agrees with it, the unique-best inputs have exactly one slot at the
maximum count and the count-tie inputs have many.  Without these the GPU tests could pass vacuously
(a "tie" batch without a tie, a "unique" batch whose placed copies are not the only maxima)."""
import numpy as np
import pytest

from tests.helpers import record_cases as cases
from tests.helpers import record_ref as ref


def _loop(usac, counts, sums):
    """ransac.cpp's keep-the-first-best loop with Score::bigger, slots with count < 0 skipped"""
    best, best_score = None, None
    for i, (c, s) in enumerate(zip(counts, sums)):
        if c < 0:
            continue
        cur = usac.Score(int(c), float(s))
        if best is None or cur.bigger(best_score):
            best, best_score = i, cur
    return best


HAND = [
    ([3, 3, 3], [1.0, 2.0, 2.0]),                    # count tie, Σ tie between the last two: slot 1
    ([3, 5, 5, 5], [9.0, 1.0, 1.0, 1.0]),            # full tie of three: the first of them
    ([5, 5, 5], [1.0, 1.5, 1.25]),                   # count tie, distinct Σ: the largest Σ
    ([0, 0, 0], [0.0, 0.0, 0.0]),                    # all zero: slot 0
    ([-1, -1, -1, -1], [0.0, 0.0, 0.0, 0.0]),        # nothing occupied
    ([-1, -1, -1, 0], [0.0, 0.0, 0.0, 0.0]),         # one occupied slot at the end
    ([-1, 2, -1, 2], [7.0, 1.0, 9.0, 1.0]),          # a large Σ on an empty slot never wins
    ([4, 4], [np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))]),  # one ulp decides
    ([4, 4], [1.0, 1.0 + 2.0 ** -30]),               # equal as fp32 values: the earlier slot
]


def test_best_slot_is_the_sequential_loop(usac):
    """Hand-made arrays (3-4 slots) with ties at every level, and 200 random arrays of 1..40 slots with
    counts in -1..3 and Σ from four values, so that every level of the order ties often."""
    for counts, sums in HAND:
        c, s = np.array(counts, np.int32), np.array(sums, np.float32)
        assert ref.best_slot(c, s) == _loop(usac, c, s), (counts, sums)
        assert ref._fast_best_slot(c, s) == ref.best_slot(c, s), (counts, sums)
    assert ref.best_slot(*map(np.array, HAND[0])) == 1
    assert ref.best_slot(*map(np.array, HAND[1])) == 1
    assert ref.best_slot(*map(np.array, HAND[4])) is None
    assert ref.best_slot(*map(np.array, HAND[5])) == 3
    assert ref.best_slot(*map(np.array, HAND[8])) == 0
    rng = np.random.default_rng(0)
    for _ in range(200):
        n = int(rng.integers(1, 41))
        c = rng.integers(-1, 4, n).astype(np.int32)
        s = rng.choice(np.array([0.5, 1.0, 1.5, 2.0], np.float32), n)
        assert ref.best_slot(c, s) == _loop(usac, c, s)
        assert ref._fast_best_slot(c, s) == ref.best_slot(c, s)


def test_record_fields():
    """record(): hyp_index = first_hyp + slot // spk beyond 2^32, zeros when nothing is occupied."""
    models = np.arange(6 * 9, dtype=np.float32).reshape(6, 9)
    r = ref.record(np.array([-1, 2, 2, 2, 1, -1]), np.array([0, 1, 3, 3, 9, 0], np.float32), models, 3, 2 ** 40 + 3)
    assert (r["valid"], r["inliers"], r["slot"], r["hyp_index"]) == (True, 2, 2, 2 ** 40 + 3)
    np.testing.assert_array_equal(r["model"], models[2].view(np.int32))
    assert r["score"] == np.float32(3).view(np.int32)
    r = ref.record(np.array([-1, 2, 2, 2, 3, -1]), np.array([0, 1, 3, 3, 0, 0], np.float32), models, 3, 7)
    assert (r["slot"], r["hyp_index"]) == (4, 8)
    r = ref.record(np.full(6, -1), np.ones(6, np.float32), models, 3, 2 ** 40 + 3)
    assert (r["valid"], r["inliers"], r["hyp_index"], r["score"]) == (False, 0, 2 ** 40 + 3, 0)
    assert not r["model"].any()
    ref.assert_record({"valid": True, "inliers": 2, "hyp_index": 8, "score": 0.0, "model": models[4]},
                      ref.record(np.array([-1, 2, 2, 2, 2, -1]), np.array([-1, -1, -1, -1, 0, 0], np.float32), models, 3, 7))
    with pytest.raises(AssertionError):
        ref.assert_record({"valid": True, "inliers": 2, "hyp_index": 8, "score": -0.0, "model": models[4]},
                          ref.record(np.array([-1, 2, 2, 2, 2, -1]), np.array([-1, -1, -1, -1, 0, 0], np.float32), models,
                                     3, 7))


def test_merge_records_agrees(usac):
    """usac_merge_records over one-slot records (hyp_index = slot) picks best_slot's slot: 100 random
    arrays of 1..24 occupied slots (merge_records has no empty slots: invalid records lose)."""
    rng = np.random.default_rng(1)
    for _ in range(100):
        n = int(rng.integers(1, 25))
        c = rng.integers(-1, 4, n).astype(np.int32)
        s = rng.choice(np.array([0.5, 1.0, 1.5], np.float32), n)
        recs = []
        for i in range(n):
            r = usac.Record()
            r.hyp_index, r.inliers, r.score, r.valid = i, max(int(c[i]), 0), float(s[i]), int(c[i] >= 0)
            recs.append(r)
        out = usac.merge_records(recs)
        want = ref.best_slot(c, s)
        if want is None:
            assert not out.valid
        else:
            assert out.valid and out.hyp_index == want and out.inliers == c[want]


def test_tied_batch_and_tiled():
    base = np.array([[0, 1], [2, 3], [4, 5], [2, 3], [6, 7]], np.int32)
    out = ref.tied_batch(base, 1, 0, [2, 4])
    np.testing.assert_array_equal(out, [[0, 1], [0, 1], [2, 3], [0, 1], [2, 3]])
    np.testing.assert_array_equal(base[1], [2, 3])  # the input is left alone
    t = ref.tiled(base, 12)
    assert t.shape == (12, 2)
    np.testing.assert_array_equal(t[5:10], base)
    np.testing.assert_array_equal(t[10:], base[:2])


@pytest.mark.parametrize("kind", cases.KINDS)
def test_unique_best_inputs(oracle, kind):
    """1 000 points; 4 352 (H, L) / 2 048 (F: 6 144 slots) / 1 024 (E) samples: exactly one slot at the
    oracle's maximum count, so a placed copy of its row is the batch's only maximum."""
    pts, samples, thr = cases.unique_best(oracle, kind)
    c, s, _ = cases.oracle_scores(oracle, kind, pts, samples, thr)
    tied, mx, second = cases.top(c, s)
    print("unique-best %s: max %d, n_tied %d, runner-up %s" % (kind, mx, len(tied), second))
    assert len(tied) == 1
    best_row = int(tied[0]) // cases.SPK[kind]
    assert (samples == samples[best_row]).all(1).sum() == 1   # the row occurs once in the base batch
    assert second is not None and second < mx


@pytest.mark.parametrize("n", [16, 33])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_count_tie_inputs(oracle, kind, n):
    """All-inlier sets of 16 and 33 points; 2 304 (H) / 1 024 (F, E, L) samples: at least four slots tie
    at the maximum count, and for H at 16 points two of them also share their Σ bits."""
    pts, samples, thr = cases.count_tie(oracle, kind, n)
    c, s, _ = cases.oracle_scores(oracle, kind, pts, samples, thr)
    tied, mx, _ = cases.top(c, s)
    sb = s[tied].view(np.int32)
    shared = len(sb) - len(np.unique(sb))
    print("count-tie %s n=%d: max %d, n_tied %d, slots sharing Σ bits with an earlier one %d" % (kind, n, mx, len(tied), shared))
    assert mx == n
    assert len(tied) >= 4
    if kind == "H" and n == 16:
        assert shared >= 1


@pytest.mark.parametrize("kind", ["F", "E"])
def test_degenerate_inputs(oracle, kind):
    """1 000 points, m of them with one shared coordinate, one non-finite: the oracle finds no model for
    the two degenerate rows (so an all-degenerate batch is empty) and one for the healthy row, which
    keeps most of its inliers on the changed points."""
    pts, thr, bad, healthy = cases.degenerate(oracle, kind)
    est = oracle.Estimator(cases.okind(oracle, kind), pts)
    assert all(len(est.estimate(r)) == 0 for r in bad)
    models = est.estimate(healthy)
    assert len(models) > 0
    assert est.score_models(models, thr)[0].max() > 100
