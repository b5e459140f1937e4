"""The written rule of device input in quality order (usac_multi_create_device_sorted, ABI 26), in numpy, and the
score values the tests of it share.  The better score first; equal scores (+0 and -0 are) in ascending column
order; infinities are ordinary numbers; a NaN of any sign or payload after every number in either direction, in
ascending column order; scores of columns that are not kept are never looked at."""
import numpy as np

# NaNs of both signs and several payloads, as bit patterns
NAN_BITS = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fc12345], dtype=np.uint32)
# the numbers at which an integer key can go wrong: zeros, infinities, the smallest and largest of each sign
EDGE_BITS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff,
                      0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff, 0x3f800000, 0xbf800000], dtype=np.uint32)


def order(k, cols, descending):
    """k: the scores of the kept columns cols (ascending) -> the places of k / cols in sorted order"""
    k = np.asarray(k, dtype=np.float32)
    nan = np.isnan(k)
    k2 = np.where(nan, np.float32(0), k)
    return np.lexsort((cols, -k2 if descending else k2, nan))


def sorted_columns(scores, valid, descending):
    """scores, valid: (P, n_max) -> per problem the kept columns in quality order (uint32)"""
    out = []
    for s, v in zip(scores, valid):
        cols = np.flatnonzero(v)
        out.append(cols[order(s[cols], cols, descending)].astype(np.uint32))
    return out
