"""Multi-problem contexts (usac_multi_*, ABI 15): the argument checks of usac_multi_create run
before any device call, so they need no GPU."""
import ctypes

import numpy as np
import pytest


def _create(usac, estimator, pts, offsets, P):
    L = usac.lib()
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    off = np.ascontiguousarray(offsets, dtype=np.uint32)
    h = ctypes.c_void_p()
    rc = L.usac_multi_create(ctypes.byref(h), 0, int(estimator), pts.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                             off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), P)
    assert not h.value or rc == 0
    if h.value:
        L.usac_multi_destroy(h)
    return rc


PTS = np.arange(80, dtype=np.float32).reshape(20, 4)
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def test_create_rejects_no_problems(usac):
    assert _create(usac, usac.ESTIMATOR.Homography, PTS, [0], 0) == ERR_ARG
    assert _create(usac, usac.ESTIMATOR.Fundamental, PTS, [0], 0) == ERR_ARG


def test_create_rejects_decreasing_offsets(usac):
    assert _create(usac, usac.ESTIMATOR.Homography, PTS, [0, 12, 8, 20], 3) == ERR_ARG
    assert _create(usac, usac.ESTIMATOR.Homography, PTS, [4, 12, 20], 2) == ERR_ARG  # offsets[0] must be 0


@pytest.mark.parametrize("est,m", [("Homography", 4), ("Fundamental", 7)])
def test_create_rejects_a_problem_below_the_sample_size(usac, est, m):
    assert _create(usac, usac.ESTIMATOR[est], PTS, [0, 10, 10 + m - 1], 2) == ERR_ARG
    assert _create(usac, usac.ESTIMATOR[est], PTS, [0, m - 1, 20], 2) == ERR_ARG


@pytest.mark.parametrize("est", ["Line2d", "Essential"])
def test_create_rejects_line_and_essential(usac, est):
    assert _create(usac, usac.ESTIMATOR[est], PTS, [0, 10, 20], 2) == ERR_UNSUPPORTED


def test_multicontext_raises(usac):
    H, F = usac.ESTIMATOR.Homography, usac.ESTIMATOR.Fundamental
    cases = [(H, [], ERR_ARG), (H, [PTS[:10], PTS[:3]], ERR_ARG), (F, [PTS[:6], PTS], ERR_ARG),
             (usac.ESTIMATOR.Line2d, [PTS], ERR_UNSUPPORTED), (usac.ESTIMATOR.Essential, [PTS], ERR_UNSUPPORTED)]
    for est, sets, code in cases:
        with pytest.raises(usac.UsacError) as e:
            usac.MultiContext(est, sets)
        assert e.value.code == code
    assert usac.lib().usac_multi_num_problems(None) == 0
