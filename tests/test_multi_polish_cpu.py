"""The multi-problem polish (usac_multi_polish, usac_multi_run_polished; ABI 16) without a GPU: the
yardstick of tests/test_gpu_multi_polish.py -- the reference's polish restated over the oracle's
quality / nonminimal (tests/helpers/multi_polish_ref.py) -- reproduces oracle.ransac_run's own polish
from its minimal model, and the new entry points reject NULL arguments before any device call."""
import ctypes

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import multi_polish_ref as ref

ERR_ARG = -1


@pytest.mark.parametrize("kind,n,seed", [("H", 333, 1), ("H", 1000, 2), ("H", 3000, 3), ("F", 333, 2), ("F", 1000, 3),
                                          ("F", 3000, 1)])
def test_restated_polish_equals_the_oracle_run(oracle, kind, n, seed):
    if kind == "H":
        pts = synthetic.homography_points(n=n, inlier_ratio=0.3, seed=seed)[0]
        est = oracle.Estimator(oracle.HOMOGRAPHY, pts)
        run = oracle.ransac_run(oracle.HOMOGRAPHY, pts, ref.THR, 0.95, seed)
    else:
        pts = synthetic.fundamental_points(n=n, inlier_ratio=0.3, seed=seed, prosac_order=False)[0]
        est = oracle.Estimator(oracle.FUNDAMENTAL, pts)
        run = oracle.ransac_run(oracle.FUNDAMENTAL, pts, ref.THR, 0.95, seed)
    assert run["ret"] == 0
    r = ref.polish_ref(est, run["minimal_model"], ref.THR)
    assert r["minimal_inliers"] == run["minimal_inliers"]
    assert r["passes"] == run["polish_passes"]
    assert r["inliers"] == run["inliers"]
    np.testing.assert_array_equal(ref.bits(r["model"]), ref.bits(run["model"]))
    np.testing.assert_array_equal(r["inlier_idx"], run["inlier_idx"])


def test_restated_polish_improves_the_minimal_model(oracle):
    """what the polish is for: more inliers than the best minimal model on both estimators"""
    for kind in "HF":
        pts = ref.make_set(kind, 1000, 0.3, 24 if kind == "H" else 34)
        est = ref.estimator(oracle, kind, pts)
        r = ref.polish_ref(est, ref.start_model(oracle, kind, pts, 44, 256, est), ref.THR)
        assert r["passes"] == 4 and r["inliers"] > r["minimal_inliers"] > 0


def test_null_arguments_are_rejected_without_a_device(usac):
    L = usac.lib()
    models = (ctypes.c_float * 9)()
    pol = (usac._MultiPolishOutput * 1)()
    out = (usac._MultiOutput * 1)()
    params = usac._Params()
    fake = ctypes.c_void_p(16)  # never dereferenced: every call below fails on a NULL first
    assert L.usac_multi_polish(None, models, ctypes.c_float(2.0), pol, None) == ERR_ARG
    assert L.usac_multi_polish(fake, None, ctypes.c_float(2.0), pol, None) == ERR_ARG
    assert L.usac_multi_polish(fake, models, ctypes.c_float(2.0), None, None) == ERR_ARG
    assert L.usac_multi_run_polished(None, ctypes.byref(params), None, out, pol, None) == ERR_ARG
    assert L.usac_multi_run_polished(fake, None, None, out, pol, None) == ERR_ARG
    assert L.usac_multi_run_polished(fake, ctypes.byref(params), None, None, pol, None) == ERR_ARG
    assert L.usac_multi_run_polished(fake, ctypes.byref(params), None, out, None, None) == ERR_ARG


def test_polish_output_layout(usac):
    """usac_multi_polish_output: 9 floats and 6 words, no padding (the kernel writes it in place)"""
    assert ctypes.sizeof(usac._MultiPolishOutput) == 60
    assert usac._MultiPolishOutput.status.offset == 56
    assert {"usac_multi_polish", "usac_multi_run_polished"} <= set(usac.ABI_SYMBOLS)
    assert usac.lib().usac_abi_version() >= 16
