"""Device output of a multi context (usac_multi_export_device, ABI 27): what the call must write, restated in
numpy from what the same polishing call returned to the host -- the N_total mask bytes, the context's offsets and
its source columns (None: a context created from the host, the identity).  Everything here runs on the CPU."""
import numpy as np


def columns(offsets, source, p):
    """the column of every packed row of problem p"""
    o = np.asarray(offsets, dtype=np.int64)
    if source is None:
        return np.arange(o[p + 1] - o[p], dtype=np.int64)
    return np.asarray(source, dtype=np.int64)[o[p]:o[p + 1]]


def padded_mask(mask, offsets, source, n_max):
    """(P, n_max) uint8: out[p, column of row i] = mask[offsets[p] + i], every other cell 0"""
    o = np.asarray(offsets, dtype=np.int64)
    mask = np.asarray(mask, dtype=np.uint8)
    out = np.zeros((len(o) - 1, n_max), dtype=np.uint8)
    for p in range(len(o) - 1):
        out[p, columns(o, source, p)] = mask[o[p]:o[p + 1]]
    return out


def inlier_cols(mask, offsets, source, k_max):
    """(P, k_max) int32: the columns of problem p's set rows in packed-row order, the first k_max of them, -1
    behind the last"""
    o = np.asarray(offsets, dtype=np.int64)
    mask = np.asarray(mask, dtype=np.uint8)
    out = np.full((len(o) - 1, k_max), -1, dtype=np.int32)
    for p in range(len(o) - 1):
        cols = columns(o, source, p)[np.flatnonzero(mask[o[p]:o[p + 1]])][:k_max]
        out[p, :len(cols)] = cols
    return out


def by_hand(mask, offsets, source, n_max, k_max):
    """the two functions above as loops over single rows: (padded mask, inlier columns)"""
    P = len(offsets) - 1
    padded = [[0] * n_max for _ in range(P)]
    cols = [[-1] * k_max for _ in range(P)]
    for p in range(P):
        at = 0
        for i in range(int(offsets[p + 1]) - int(offsets[p])):
            row = int(offsets[p]) + i
            col = i if source is None else int(source[row])
            padded[p][col] = int(mask[row])
            if mask[row]:
                if at < k_max:
                    cols[p][at] = col
                at += 1
    return np.array(padded, dtype=np.uint8).reshape(P, n_max), np.array(cols, dtype=np.int32).reshape(P, k_max)
