"""Pose refinement of multi contexts (usac_multi_refine_pose_device, usac_multi_refine_pose; ABI 29), the part that
needs no GPU.  The reference of the GPU tests is new text -- tests/helpers/multi_refine_ref.py, the rule of
include/usac_gpu.h "Pose refinement" in numpy -- so it gets anchors of its own here: its derivatives against central
differences of its own residual through its own update, its optimum against scipy's Levenberg-Marquardt on the
same residual, the geometry the synthetic scenes were generated with, and the edges of the rule.  Then the symbols,
the refusals that need no device, the struct as the C++ consumer sees it, and the host-only argument logic under
the sanitizers in a stand-alone program.

Measured here (DESIGN.md §8b "Pose refinement"), each bound ten times the largest measured value:
  derivatives, 60 rows, h = 1e-6: max |J - J_fd| / max |J| = 4.86e-11                       -> bound 4.9e-10
  the optimum, 63 / 64 / 65 / 257 / 1000 rows, max_iters = 50: |cost - cost_scipy| / cost_scipy
      = 4.77e-14, 1.03e-14, 2.96e-15, 1.14e-14, 3.93e-15 after 5, 6, 5, 5, 19 trial steps    -> bound 4.8e-13
      (and, whatever was measured: cost <= cost_scipy (1 + 1e-6))
  geometry, 64 noise-free rows, 3 degrees and 0.1 off: max |R - R_gt| = 6.04e-8, |t x t_gt| = 1.41e-7 after 7
      trial steps (the rows are fp32: a relative 6e-8 per coordinate)                       -> bounds 6.1e-7, 1.5e-6"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.conftest import ROOT
from tests.helpers import multi_refine_ref as ref

DIR = os.path.join(ROOT, "tests", "cpp_multi_refine")
BIN = os.path.join(DIR, "build", "consumer")
F = np.float64
J_TOL = 4.9e-10
COST_TOL = 4.8e-13
R_TOL, T_TOL = 6.1e-7, 1.5e-6


def _gt():
    _, R, t, _, _ = synthetic.two_view_geometry()
    return R, t / np.linalg.norm(t)


def _rotation(axis, deg):
    a = np.asarray(axis, dtype=F) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)


def _scene(n, seed, noise=0.5):
    """n inlier rows of the synthetic scene, calibrated"""
    return synthetic.fundamental_points(n=n, inlier_ratio=1.0, seed=seed, noise=noise, normalized=True,
                                        prosac_order=False)[0]


def _start(deg=3.0, off=(0.05, 0.08, -0.03)):
    R, t = _gt()
    return (_rotation((0.3, -0.5, 0.8), deg) @ R).astype(np.float32), (t + np.asarray(off)).astype(np.float32)


def _checked(r):
    """the invariant of every case of this file"""
    assert r["cost"] <= r["cost0"], (r["cost"], r["cost0"])
    return r


def _pose_lists(R32, t32):
    R = [[F(R32[r, c]) for c in range(3)] for r in range(3)]
    return R, ref.normalized([F(v) for v in t32])


def _residual_at(R, t, rows):
    used = np.ones(len(rows), dtype=bool)
    E, D, b1, b2 = ref.frame(R, t)
    with np.errstate(all="ignore"):
        r, J, ok = ref.residuals(E, D, rows, used)
    assert ok.all()
    return r, np.array(J), b1, b2


def test_derivatives_against_central_differences():
    rows = _scene(60, 9).astype(F)
    R, t = _pose_lists(*_start())
    r0, J, b1, b2 = _residual_at(R, t, rows)
    h = 1e-6
    worst = 0.0
    for j in range(5):
        d = [F(0)] * 5
        d[j] = F(h)
        Rp, tp = ref.update(R, t, b1, b2, d)
        d[j] = F(-h)
        Rm, tm = ref.update(R, t, b1, b2, d)
        fd = (_residual_at(Rp, tp, rows)[0] - _residual_at(Rm, tm, rows)[0]) / (2 * h)
        worst = max(worst, float(np.abs(J[j] - fd).max()))
    rel = worst / float(np.abs(J).max())
    print("derivatives: max |J - J_fd| / max |J| = %.3g (bound %.3g)" % (rel, J_TOL))
    assert rel <= J_TOL


def test_the_optimum_is_scipys():
    so = pytest.importorskip("scipy.optimize")
    R0, t0 = _start()
    for n, seed in ((63, 3), (64, 4), (65, 5), (257, 6), (1000, 7)):
        pts = _scene(n, seed)
        mine = _checked(ref.refine(R0, t0, pts, None, 50))
        rows = pts.astype(F)
        R, t = _pose_lists(R0, t0)
        _, _, b1, b2 = _residual_at(R, t, rows)

        def fun(d):
            Rn, tn = ref.update(R, t, b1, b2, [F(v) for v in d])
            return _residual_at(Rn, tn, rows)[0]

        sol = so.least_squares(fun, np.zeros(5), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        theirs = float((sol.fun ** 2).sum())
        rel = abs(float(mine["cost"]) - theirs) / theirs
        print("n = %4d: iterations %d, cost0 %.6g, cost %.17g, scipy %.17g, relative difference %.3g"
              % (n, mine["iterations"], mine["cost0"], mine["cost"], theirs, rel))
        assert 0 < mine["iterations"] < 50
        assert float(mine["cost"]) <= theirs * (1 + 1e-6), (n, mine["cost"], theirs)
        assert rel <= COST_TOL, (n, rel)


def test_geometry_returns_to_the_scenes_pose():
    R_gt, t_gt = _gt()
    pts = _scene(64, 11, noise=0.0)
    R0, t0 = _start(3.0, (0.1, 0.0, 0.0))
    r = _checked(ref.refine(R0, t0, pts, None, 50))
    r_err = float(np.abs(r["R64"] - R_gt).max())
    t_err = float(np.linalg.norm(np.cross(r["t64"], t_gt)))
    print("geometry: iterations %d, cost0 %.3g, cost %.3g, |R - R_gt| %.3g (bound %.3g), |t x t_gt| %.3g (bound %.3g)"
          % (r["iterations"], r["cost0"], r["cost"], r_err, R_TOL, t_err, T_TOL))
    assert float(np.abs(R0.astype(F) - R_gt).max()) > 0.03 and r["cost0"] > 1e-4  # the start was off
    assert r_err <= R_TOL and t_err <= T_TOL and float(r["t64"] @ t_gt) > 0
    assert abs(float(np.linalg.norm(r["t64"])) - 1.0) <= 1e-15
    assert abs(float(np.linalg.det(r["R64"])) - 1.0) <= 1e-6  # not re-orthonormalised: the start's, about 1e-7
    # the outputs are the doubles cast once, E = [t]x R
    np.testing.assert_array_equal(r["R"], r["R64"].astype(np.float32))
    np.testing.assert_array_equal(r["t"], r["t64"].astype(np.float32))
    tx = np.array([[0, -r["t64"][2], r["t64"][1]], [r["t64"][2], 0, -r["t64"][0]], [-r["t64"][1], r["t64"][0], 0]])
    assert float(np.abs(r["E"].astype(F) - tx @ r["R64"]).max()) <= 1e-7


def _is_skipped(r, R0, t0, used):
    assert r["iterations"] == -1 and r["used"] == used and r["cost0"] == 0 and r["cost"] == 0
    assert r["R"].tobytes() == np.asarray(R0, np.float32).tobytes() and r["t"].tobytes() == np.asarray(t0, np.float32).tobytes()
    assert not r["E"].any()
    _checked(r)


def test_rule_edges():
    R0, t0 = _start()
    pts = _scene(64, 12)
    n = len(pts)
    # max_iters = 0: the normalised start, one pass; 1: one trial
    zero = _checked(ref.refine(R0, t0, pts, None, 0))
    assert zero["iterations"] == 0 and zero["cost"] == zero["cost0"] > 0 and zero["used"] == n
    np.testing.assert_array_equal(zero["R"], R0)
    np.testing.assert_array_equal(zero["t64"], np.array(ref.normalized([F(v) for v in t0])))
    one = _checked(ref.refine(R0, t0, pts, None, 1))
    assert one["iterations"] == 1 and one["cost0"] == zero["cost0"] and one["cost"] < one["cost0"]
    assert one["lambdas"] == [ref.LAMBDA0]
    ten = _checked(ref.refine(R0, t0, pts, None, 10))
    assert 1 < ten["iterations"] <= 10 and ten["cost"] < one["cost"]
    # 4 used rows: skipped; exactly 5: refined
    mask = np.zeros(n, dtype=np.uint8)
    mask[[3, 17, 40, 63]] = 1
    _is_skipped(ref.refine(R0, t0, pts, mask, 10), R0, t0, 4)
    mask[20] = 1
    five = _checked(ref.refine(R0, t0, pts, mask, 10))
    assert five["used"] == 5 and five["iterations"] > 0 and five["cost"] < five["cost0"]
    _is_skipped(ref.refine(R0, t0, pts, np.zeros(n, dtype=np.uint8), 10), R0, t0, 0)
    bad = R0.copy()
    bad[1, 2] = np.nan
    _is_skipped(ref.refine(bad, t0, pts, None, 10), bad, t0, n)
    bad_t = np.array([0.1, np.inf, 0.2], dtype=np.float32)
    _is_skipped(ref.refine(R0, bad_t, pts, None, 10), R0, bad_t, n)
    _is_skipped(ref.refine(R0, np.zeros(3, np.float32), pts, None, 10), R0, np.zeros(3, np.float32), n)
    _is_skipped(ref.refine(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), pts, None, 10),  # export_pose's choice = -1
                np.eye(3, dtype=np.float32), np.zeros(3, np.float32), n)
    _is_skipped(ref.refine(R0, t0, pts, None, 10, status=-111), R0, t0, n)  # USAC_ERR_NO_MODEL
    # a non-finite row under a set mask byte is not used, and the result is that of the rows without it
    holed = pts.copy()
    holed[5] = (np.nan, 0.1, 0.2, 0.3)
    holed[6, 3] = np.inf
    a = _checked(ref.refine(R0, t0, holed, None, 10))
    keep = np.ones(n, dtype=np.uint8)
    keep[[5, 6]] = 0
    b = _checked(ref.refine(R0, t0, pts, keep, 10))
    assert a["used"] == b["used"] == n - 2 and a["iterations"] == b["iterations"]
    for key in ("R", "t", "E"):
        assert a[key].tobytes() == b[key].tobytes()
    assert a["cost"] == b["cost"] and np.isfinite(a["cost"])


def test_a_start_at_the_optimum_and_a_rejected_first_trial():
    R0, t0 = _start()
    pts = _scene(64, 12)
    first = _checked(ref.refine(R0, t0, pts, None, 50))
    # from the optimum: nothing to gain, and the loop ends on one of its own tests, never on max_iters.  With
    # noise the cost test ends it or lambda does; which one is asserted on the two cases below
    again = _checked(ref.refine(first["R"], first["t"], pts, None, 50))
    print("from the optimum: stop %s, iterations %d, lambdas %s, cost0 %.17g, cost %.17g"
          % (again["stop"], again["iterations"], ["%.0e" % v for v in again["lambdas"]], again["cost0"], again["cost"]))
    assert again["stop"] in ("cost", "step", "lambda") and again["iterations"] < 50
    assert again["cost0"] - again["cost"] <= 1e-6 * again["cost0"]
    # the small-step test: a noise-free scene, whose optimum has a cost of rounding alone and steps below 1e-10
    clean = _scene(64, 11, noise=0.0)
    there = _checked(ref.refine(*_start(3.0, (0.1, 0.0, 0.0)), clean, None, 50))
    stay = _checked(ref.refine(there["R"], there["t"], clean, None, 50))
    print("from the noise-free optimum: stop %s, iterations %d, cost %.3g" % (stay["stop"], stay["iterations"], stay["cost"]))
    assert stay["stop"] == "step" and 0 < stay["iterations"] < 5
    # lambda: a zero rotation (finite, so not skipped) makes E and every D zero, no row has S > 0, H is zero and
    # every solve is rejected by its first pivot without a pass: twelve solves from 1e-3 until lambda > 1e8
    flat = _checked(ref.refine(np.zeros((3, 3), np.float32), t0, pts, None, 50))
    assert flat["stop"] == "lambda" and flat["pivots"] == 12 and flat["iterations"] == 0 and flat["cost0"] == 0
    assert flat["lambdas"][0] == ref.LAMBDA0 and len(flat["lambdas"]) == 12
    assert flat["lambdas"][-1] * F(10) > ref.LAMBDA_MAX >= flat["lambdas"][-1]
    assert not flat["R"].any() and not flat["E"].any() and flat["used"] == len(pts)
    # and lambda after real passes: on 1 000 noisy rows the run ends with rejected trials up to 1e8
    big = _checked(ref.refine(R0, t0, _scene(1000, 7), None, 50))
    assert big["stop"] == "lambda" and big["pivots"] == 0 and big["iterations"] == len(big["lambdas"]) < 50
    # a first trial that is rejected, constructed: from a start far off the second trial of a run is rejected, so
    # the pose after its first trials (max_iters = 2) is one where the step at lambda = 1e-3 overshoots.  The
    # damping goes up by ten per rejection; every trial that ran a pass counts as an iteration
    found = None
    for deg, off in ((120, (0.9, -0.7, 0.5)), (90, (0.0, 0.0, 0.0)), (90, (0.9, -0.7, 0.5)), (120, (-2.0, 0.1, 0.3))):
        far = _checked(ref.refine(*_start(deg, off), pts, None, 2))
        R1, t1 = far["R"], far["t"]
        r = _checked(ref.refine(R1, t1, pts, None, 30))
        lam = r["lambdas"]
        if len(lam) >= 2 and lam[1] == F(10) * lam[0]:
            found = (deg, r)
            break
    assert found is not None, "no start of the list has its first trial rejected"
    deg, r = found
    print("rejected first trial: %d degrees, iterations %d, lambdas %s" % (deg, r["iterations"], ["%.0e" % v for v in lam]))
    assert lam[0] == ref.LAMBDA0 and lam[1] == F(10) * ref.LAMBDA0
    for a, b in zip(lam, lam[1:]):  # up by ten after a rejection, down by ten (not below 1e-12) after an acceptance
        assert b == F(10) * a or b == max(a / F(10), ref.LAMBDA_MIN)
    assert 2 <= r["iterations"] <= len(lam) and r["cost"] < r["cost0"]
    one = _checked(ref.refine(R1, t1, pts, None, 1))  # the rejected trial alone: the start comes back, normalised
    assert one["iterations"] == 1 and one["cost"] == one["cost0"] and one["lambdas"] == [ref.LAMBDA0]
    zero = ref.refine(R1, t1, pts, None, 0)
    assert one["R"].tobytes() == zero["R"].tobytes() and one["t"].tobytes() == zero["t"].tobytes()
    rejected = 0  # the leading rejections, then the first acceptance: iterations counts them all
    while lam[rejected + 1] == F(10) * lam[rejected]:
        rejected += 1
    upto = _checked(ref.refine(R1, t1, pts, None, rejected + 1))
    assert upto["iterations"] == rejected + 1 and upto["cost"] < upto["cost0"] and upto["lambdas"] == lam[:rejected + 1]


def test_sums_are_the_workgroups():
    """block_sum against the order spelt out lane by lane, on sizes around a stride, a wave and the four-wave step"""
    rng = np.random.default_rng(5)
    for n in (1, 5, 63, 64, 65, 255, 256, 257, 1000):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        ok = rng.random(n) < 0.8
        acc = [F(0)] * 256
        for i in range(n):
            if ok[i]:
                acc[i % 256] = acc[i % 256] + v[i]
        w = []
        for wave in range(4):
            lanes = acc[64 * wave:64 * wave + 64]
            for off in (32, 16, 8, 4, 2, 1):
                lanes = [lanes[k] + lanes[k ^ off] for k in range(64)]
            assert all(x == lanes[0] for x in lanes)  # the butterfly leaves one value in every lane
            w.append(lanes[0])
        assert ref.block_sum(v, ok) == (w[0] + w[1]) + (w[2] + w[3])


def test_batch_helper_is_the_rule_per_problem():
    pts = _scene(600, 13)
    R0, t0 = _start()
    offsets = np.array([0, 4, 70, 600], dtype=np.uint32)
    R = np.stack([R0, R0, np.eye(3, dtype=np.float32)])
    t = np.stack([t0, t0, np.zeros(3, np.float32)])
    got = ref.refine_batch(R, t, pts, offsets, None, 10)
    assert got["iterations"][0] == -1 and got["used"][0] == 4 and got["iterations"][1] > 0 and got["iterations"][2] == -1
    for p in range(3):
        one = _checked(ref.refine(R[p], t[p], pts[offsets[p]:offsets[p + 1]], None, 10))
        for key in ref.KEYS:
            assert np.asarray(got[key][p]).tobytes() == np.asarray(one[key], dtype=got[key].dtype).tobytes(), (p, key)


def test_abi_version_and_symbols(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 29
    for name in ("usac_multi_refine_pose_device", "usac_multi_refine_pose"):
        assert name in usac.ABI_SYMBOLS
        assert hasattr(L, name)
    assert callable(usac.MultiContext.refine_pose) and callable(usac.MultiContext.refine)


def test_null_contexts_are_refused(usac):
    L = usac.lib()
    fake = 0x7f0000001000  # an aligned address nothing dereferences: every case returns before it could
    o = usac._MultiRefineIO(n_max=10, max_iters=10, R_in=fake, t_in=fake, R=fake)
    assert L.usac_multi_refine_pose_device(None, ctypes.byref(o)) == -1
    assert L.usac_multi_refine_pose_device(None, None) == -1
    R = np.zeros(9, dtype=np.float32)
    t = np.zeros(3, dtype=np.float32)
    it = np.zeros(1, dtype=np.int32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    assert L.usac_multi_refine_pose(None, R.ctypes.data_as(fp), t.ctypes.data_as(fp), None, 10, None, None, None, None,
                                    None, it.ctypes.data_as(ip), None) == -1
    assert L.usac_multi_refine_pose(None, None, None, None, 10, None, None, None, None, None, None, None) == -1


def test_struct_mirror_matches_the_header(usac):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 29
    S = usac._MultiRefineIO
    assert ctypes.sizeof(S) == d["sizeof"]
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == d["offsets"]


def test_argument_logic_under_sanitizers(tmp_path):
    """the host-only argument logic of the refine entries (usac_pack.hpp), as g++ compiles it"""
    exe = str(tmp_path / "refine_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"), os.path.join(DIR, "refine_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
