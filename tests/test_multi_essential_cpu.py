"""Multi contexts of essential-matrix problems (usac_multi_create_essential, ABI 21): the checks
that run before any device call, so they need no GPU.  A valid call needs a device and is left to
tests/test_gpu_multi_essential.py."""
import ctypes

import numpy as np
import pytest

PTS = np.arange(80, dtype=np.float32).reshape(20, 4)
ERR_ARG = -1
_F32P, _U32P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)


def _create(usac, offsets, P, out=True, pts=True, offs=True):
    """usac_multi_create_essential's return code; no handle may come back with an error"""
    L = usac.lib()
    p = np.ascontiguousarray(PTS, dtype=np.float32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    h = ctypes.c_void_p()
    rc = L.usac_multi_create_essential(ctypes.byref(h) if out else None, 0, p.ctypes.data_as(_F32P) if pts else None,
                                       off.ctypes.data_as(_U32P) if offs else None, P)
    assert not h.value or rc == 0
    if h.value:
        L.usac_multi_destroy(h)
    return rc


def test_abi_version_and_symbol(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 21
    assert hasattr(L, "usac_multi_create_essential")
    assert callable(usac.MultiContext.essential)


def test_create_essential_rejects_no_problems(usac):
    assert _create(usac, [0], 0) == ERR_ARG


def test_create_essential_rejects_bad_offsets(usac):
    assert _create(usac, [4, 12, 20], 2) == ERR_ARG        # offsets[0] must be 0
    assert _create(usac, [0, 12, 8, 20], 3) == ERR_ARG     # decreasing


def test_create_essential_rejects_a_problem_of_four_points(usac):
    assert _create(usac, [0, 4, 20], 2) == ERR_ARG         # the first problem
    assert _create(usac, [0, 16, 20], 2) == ERR_ARG        # the last problem


def test_create_essential_rejects_null_pointers(usac):
    assert _create(usac, [0, 10, 20], 2, out=False) == ERR_ARG
    assert _create(usac, [0, 10, 20], 2, pts=False) == ERR_ARG
    assert _create(usac, [0, 10, 20], 2, offs=False) == ERR_ARG


def test_classmethod_raises_on_bad_sets(usac):
    for sets in ([], [PTS[:10], PTS[:4]]):
        with pytest.raises(usac.UsacError) as e:
            usac.MultiContext.essential(sets)
        assert e.value.code == ERR_ARG
