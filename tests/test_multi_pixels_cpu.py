"""Essential multi contexts from pixel coordinates (usac_multi_create_essential_pixels,
usac_multi_set_pixel_thresholds, usac_multi_pixel_models, usac_multi_get_points; ABI 24), the parts that need
no device: the version and the symbols, the argument errors of the create entry (returned on a machine without
a GPU too: they come before any device call), the numpy restatement of the spec (tests/helpers/
multi_pixels_ref.py) against fp64 linear algebra within bounds derived from the spec's roundings, and the host
text (ransac_amd/csrc/usac_pixels.hpp) under the sanitizers in a stand-alone program."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import multi_pixels_ref as ref

DIR = os.path.join(ROOT, "tests", "cpp_multi_pixels")
BIN = os.path.join(DIR, "build", "consumer")
ERR_ARG = -1
U = 2.0 ** -24  # the unit roundoff of float32
NEW = ["usac_multi_create_essential_pixels", "usac_multi_set_pixel_thresholds", "usac_multi_pixel_models",
       "usac_multi_get_points"]


def test_abi_version_and_symbols(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 24
    assert set(NEW) <= set(usac.ABI_SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    for name in ("essential_pixels", "set_pixel_thresholds", "pixel_models", "resident_points"):
        assert callable(getattr(usac.MultiContext, name)), name


def _f32p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _u32p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _bad_ks():
    """name -> a K the create entry refuses"""
    good = ref.k_matrix(1000, 990, 500, 480, 1.5).reshape(9)
    bad = {}
    for name, k, v in (("fx == 0", 0, 0.0), ("fx < 0", 0, -1000.0), ("fy == 0", 4, 0.0), ("fy < 0", 4, -3.0),
                       ("NaN in K", 2, np.nan), ("inf in K", 5, np.inf), ("NaN fx", 0, np.nan), ("k[8] == 2", 8, 2.0),
                       ("k[3] != 0", 3, 1e-3), ("k[6] != 0", 6, -1.0), ("k[7] != 0", 7, 0.5)):
        b = good.copy()
        b[k] = v
        bad[name] = b
    return good, bad


def test_create_argument_errors_come_before_any_device_call(usac):
    L = usac.lib()
    good, bad = _bad_ks()
    P = 2
    pts = np.zeros((12, 4), dtype=np.float32)
    offs = np.array([0, 5, 12], dtype=np.uint32)
    K = np.ascontiguousarray(np.stack([good, good]))
    h = ctypes.c_void_p()

    def create(pts_=pts, offs_=offs, P_=P, K1=K, K2=None, out=h):
        h.value = 12345  # an error leaves NULL behind
        rc = L.usac_multi_create_essential_pixels(ctypes.byref(out) if out is not None else None, 0, _f32p(pts_),
                                                  _u32p(offs_), P_, _f32p(K1), _f32p(K2))
        if out is not None:
            assert out.value is None
        return rc

    assert create(out=None) == ERR_ARG
    assert create(pts_=None) == ERR_ARG
    assert create(offs_=None) == ERR_ARG
    assert create(K1=None) == ERR_ARG
    assert create(K1=None, K2=K) == ERR_ARG
    assert create(P_=0) == ERR_ARG
    assert create(P_=65536) == ERR_ARG
    assert create(offs_=np.array([0, 4, 12], dtype=np.uint32)) == ERR_ARG   # an n_p of 4
    assert create(offs_=np.array([1, 6, 12], dtype=np.uint32)) == ERR_ARG   # offsets[0] != 0
    assert create(offs_=np.array([0, 12, 6], dtype=np.uint32)) == ERR_ARG   # not monotonic
    for name, b in bad.items():
        for where in range(P):  # in either problem, as K1 and as K2
            Kb = K.copy()
            Kb[where] = b
            assert create(K1=Kb) == ERR_ARG, (name, where, "K1")
            assert create(K2=Kb) == ERR_ARG, (name, where, "K2")


def test_null_handles_are_refused(usac):
    L = usac.lib()
    a = np.ones(9, dtype=np.float32)
    assert L.usac_multi_set_pixel_thresholds(None, _f32p(a), 1) == ERR_ARG
    assert L.usac_multi_pixel_models(None, _f32p(a), _f32p(a)) == ERR_ARG
    assert L.usac_multi_get_points(None, _f32p(a)) == ERR_ARG
    assert (a == 1).all()


def test_python_layer_checks_the_shape_of_k(usac):
    sets = ref.pixel_sets()
    for K in (np.eye(4), np.zeros((5, 3, 3)), np.zeros(9)):
        with pytest.raises(ValueError):
            usac.MultiContext.essential_pixels(sets, K)
    with pytest.raises(ValueError):
        usac.MultiContext.essential_pixels(sets, np.eye(3), np.zeros((2, 3, 3)))


def test_calibrated_rows_agree_with_fp64_inverse():
    """The spec's x takes four roundings after y's two -- fl(u - cx), fl(s y), their difference, the division
    -- each of relative size u = 2^-24.  With a = u - cx, b = s y: |fl(a) - a| <= u |a|; y carries 2 u |y|
    (its own subtraction and division), so |fl(s fl(y)) - b| <= 3 u |b|; the difference adds u (|a| + |b|);
    the division adds u |x|, |x| <= (|a| + |b|) / fx.  The sum is (3 |a| + 5 |b|) u / fx to first order,
    so c = 6 covers x with the second-order terms, and c = 3 covers y's two roundings: the bounds are
    6 u (|u - cx| + |s y|) / fx and 3 u |v - cy| / fy.  The yardstick is inv(K) @ (u, v, 1) in fp64 over the
    float32 inputs widened exactly; its own error (~1e-16 relative) is eight orders below the bounds."""
    sets = ref.pixel_sets()
    K1, K2 = ref.intrinsics()
    rows = ref.calibrated_sets(sets, K1, K2)
    worst = 0.0
    for p, (px, got) in enumerate(zip(sets, rows)):
        assert got.dtype == np.float32 and got.shape == px.shape
        for view, K in ((0, K1[p]), (1, K2[p])):
            K64 = K.astype(np.float64)
            u, v = px[:, 2 * view].astype(np.float64), px[:, 2 * view + 1].astype(np.float64)
            want = np.linalg.inv(K64) @ np.stack([u, v, np.ones_like(u)])
            assert np.abs(want[2] - 1).max() < 1e-12
            fx, s, cx, fy, cy = K64[0, 0], K64[0, 1], K64[0, 2], K64[1, 1], K64[1, 2]
            bx = 6 * U * (np.abs(u - cx) + np.abs(s * want[1])) / fx
            by = 3 * U * np.abs(v - cy) / fy
            ex = np.abs(got[:, 2 * view].astype(np.float64) - want[0])
            ey = np.abs(got[:, 2 * view + 1].astype(np.float64) - want[1])
            assert (ex <= bx).all(), (p, view, float((ex / np.maximum(bx, 1e-300)).max()))
            assert (ey <= by).all(), (p, view, float((ey / np.maximum(by, 1e-300)).max()))
            worst = max(worst, float((ex / np.maximum(bx, 1e-300)).max()), float((ey / np.maximum(by, 1e-300)).max()))
    print("largest error / bound: %.3f" % worst)
    # one K for all problems, and K2 = None, are the same rows
    one = ref.calibrated_sets(sets, K1[1])
    assert all((a == b).all() for a, b in zip(one, ref.calibrated_sets(sets, np.stack([K1[1]] * 6), np.stack([K1[1]] * 6))))


def _some_e(P, seed=9):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, size=(P, 3, 3)).astype(np.float32)


def test_pixel_model_agrees_with_fp64_product():
    """F = K2^-T E K1^-1: the restatement's fp64 terms are negligible, what remains is the final cast (one u
    relative to the entry, itself at most the product of the absolute values) -- 8 u with slack."""
    K1, K2 = ref.intrinsics()
    E = _some_e(6)
    F = ref.pixel_models(E, K1, K2)
    assert F.dtype == np.float32 and F.shape == E.shape
    for p in range(6):
        i1, i2 = np.linalg.inv(K1[p].astype(np.float64)), np.linalg.inv(K2[p].astype(np.float64))
        want = i2.T @ E[p].astype(np.float64) @ i1
        bound = 8 * U * (np.abs(i2.T) @ np.abs(E[p].astype(np.float64)) @ np.abs(i1))
        assert (np.abs(F[p].astype(np.float64) - want) <= bound).all(), p
    # the algebra: x2_px^T F x1_px = x2^T E x1 for calibrated x = K^-1 x_px
    x1, x2 = np.array([640.0, 360.0, 1.0]), np.array([610.0, 377.0, 1.0])
    for p in range(6):
        i1, i2 = ref.k_inverse(K1[p]), ref.k_inverse(K2[p])
        lhs = x2 @ F[p].astype(np.float64) @ x1
        rhs = (i2 @ x2) @ E[p].astype(np.float64) @ (i1 @ x1)
        assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(rhs)), p


def test_threshold_rule():
    K1, K2 = ref.intrinsics()
    thr = ref.thresholds(1.5, K1, K2)
    assert thr.dtype == np.float32 and thr.shape == (6,)
    f = (K1[:, 0, 0].astype(np.float64) + K1[:, 1, 1] + K2[:, 0, 0] + K2[:, 1, 1]) / 4
    # f: three additions (the product with 0.25 is exact), r: one division, r * r doubles r's 4 u and adds one
    np.testing.assert_allclose(thr, (1.5 / f) ** 2, rtol=10 * U)
    vec = ref.thresholds([1.0, 1.5, 2.0, 2.5, 3.0, 0.5], K1)
    assert len(set(vec.tolist())) == 6


def test_host_text_under_sanitizers(tmp_path):
    """validation, the threshold rule and the F product of usac_pixels.hpp against the restatement's values"""
    _, bad = _bad_ks()
    K1, K2 = ref.intrinsics()
    P = 6
    t = np.array([1.5, 0.25, 2.0, 3.0, 1.0, 700.0], dtype=np.float32)
    E = _some_e(P)
    E[5, 1, 1] = np.float32(3e38)  # near FLT_MAX: the fp64 products stay finite, F[1][1] is about 3e32
    blob = np.concatenate([K1.ravel(), K2.ravel(), t, ref.thresholds(t, K1, K2), E.ravel(),
                           ref.pixel_models(E, K1, K2).ravel()] + [b for b in bad.values()]).astype(np.float32)
    path = tmp_path / "pixels.f32"
    blob.tofile(path)
    exe = str(tmp_path / "pixels_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"), os.path.join(DIR, "pixels_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, str(path), str(P), str(len(bad))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok %d %d" % (P, len(bad))), r.stdout + r.stderr


def test_cpp_consumer_compiles_and_agrees_on_the_abi(usac):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 24
