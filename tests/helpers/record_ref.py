"""The batch record of a throughput batch, restated in numpy (no GPU, no library).

A batch of S slots ends in one usac_record: the slot that wins under record_better (usac_device.hpp:
larger count; then larger Σ, compared as fp32 values; then the earlier slot; a negative count never
wins), hyp_index = first_hyp + slot // spk and that slot's model.  k_argmax_part / k_argmax_final and
k_multi_argmax reduce by trees; record_better is a strict total order on finite Σ, so the result is the
sequential "first best under Score::bigger" that best_slot spells out.

Also the batch builders of the record tests: tied_batch places copies of one sample row at chosen
slots, tiled repeats a base batch to a given number of rows."""
import numpy as np


def best_slot(counts, sums):
    """The winning slot of (counts, sums), or None when no slot has count >= 0: one sequential pass
    that keeps the first best (a later slot replaces it only if strictly bigger)."""
    counts = np.asarray(counts)
    sums = np.asarray(sums, dtype=np.float32)
    best = None
    bc, bs = -1, np.float32(0)
    for i in range(len(counts)):
        c = int(counts[i])
        if c < 0:
            continue
        s = sums[i]
        if best is None or c > bc or (c == bc and s > bs):
            best, bc, bs = i, c, s
    return best


def _fast_best_slot(counts, sums):
    """best_slot for large batches: the same order through numpy (first index of the largest Σ among
    the slots of the largest count); tests/test_batch_record_cpu.py holds it to best_slot."""
    counts = np.asarray(counts)
    sums = np.asarray(sums, dtype=np.float32)
    if not (counts >= 0).any():
        return None
    top = np.flatnonzero(counts == counts.max())
    return int(top[np.argmax(sums[top])])  # argmax: the first of equal values


def record(counts, sums, models, spk, first_hyp):
    """The record k_argmax_final / k_multi_argmax write for a batch: a dict of valid, inliers (0 when
    invalid), score (int32 bits of the fp32 Σ), hyp_index = first_hyp + slot // spk (first_hyp when
    invalid), model (int32 bits of 9 floats, zeros when invalid) and slot (None when invalid).
    models: S x 9 (or S x k, zero-padded to 9), one row per slot, or a function slot -> that row."""
    counts = np.asarray(counts)
    sums = np.ascontiguousarray(sums, dtype=np.float32)
    slot = _fast_best_slot(counts, sums) if len(counts) > 4096 else best_slot(counts, sums)
    if slot is None:
        return {"valid": False, "inliers": 0, "score": np.int32(0), "hyp_index": int(first_hyp),
                "model": np.zeros(9, np.int32), "slot": None}
    m = np.zeros(9, np.float32)
    if callable(models):  # large batches: the winning slot's model alone
        row = np.asarray(models(slot), dtype=np.float32).reshape(-1)
    else:
        row = np.asarray(models, dtype=np.float32).reshape(len(counts), -1)[slot]
    m[: row.size] = row
    return {"valid": True, "inliers": int(counts[slot]), "score": sums[slot: slot + 1].view(np.int32)[0],
            "hyp_index": int(first_hyp) + slot // int(spk), "model": m.view(np.int32), "slot": slot}


def _get(rec, key):
    return rec[key] if isinstance(rec, dict) else getattr(rec, key)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def assert_record(got, want, what=""):
    """got: a Record (ctypes) or a record dict of the library; want: record()'s dict.  No tolerance:
    score and model are compared as int32 views."""
    assert bool(_get(got, "valid")) == want["valid"], (what, "valid")
    assert int(_get(got, "inliers")) == want["inliers"], (what, "inliers", int(_get(got, "inliers")), want["inliers"])
    assert int(_get(got, "hyp_index")) == want["hyp_index"], (what, "hyp_index", int(_get(got, "hyp_index")),
                                                                want["hyp_index"])
    score = bits([float(_get(got, "score"))])[0]
    assert score == want["score"], (what, "score bits", int(score), int(want["score"]))
    model = bits(np.array(_get(got, "model")[:], dtype=np.float32))
    np.testing.assert_array_equal(model, want["model"], err_msg="%s: model bits" % (what,))


def tied_batch(base_samples, best_row, filler_row, positions):
    """base_samples (rows x m) with row best_row copied to each row in positions; every other row
    equal to it (best_row itself included, unless listed) is replaced by row filler_row."""
    base = np.ascontiguousarray(base_samples, dtype=np.int32)
    best, filler = base[best_row].copy(), base[filler_row].copy()
    assert (best != filler).any()
    out = base.copy()
    out[(base == best).all(1)] = filler
    for p in positions:
        out[p] = best
    return out


def tiled(base, S):
    """base (rows x m) repeated to S rows: row i = base[i % rows]."""
    base = np.ascontiguousarray(base, dtype=np.int32)
    reps = -(-int(S) // len(base))
    return np.ascontiguousarray(np.tile(base, (reps, 1))[: int(S)])
