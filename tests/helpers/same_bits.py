"""Equality without tolerance for the results the multi-problem calls return."""
import struct

import numpy as np


def same(a, b, what):
    """dicts key by key, lists item by item, floats and float arrays by bit pattern, the rest by =="""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (what, list(a), list(b))
        for k in a:
            same(a[k], b[k], (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, (what, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert a.tobytes() == b.tobytes(), what
    elif isinstance(a, (float, np.floating)):
        assert type(a) is type(b) and struct.pack("<d", float(a)) == struct.pack("<d", float(b)), (what, a, b)
    else:
        assert type(a) is type(b) and a == b, (what, a, b)
