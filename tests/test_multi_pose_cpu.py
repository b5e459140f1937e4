"""Pose of multi contexts (usac_multi_pose_device, usac_multi_pose; ABI 28), the part that needs no GPU.  The
reference of the GPU tests is new text -- tests/helpers/multi_pose_ref.py, the rule of include/usac_gpu.h "Pose"
in numpy -- so it gets anchors of its own here: the oracle's cheirality flag of 5-point candidates, the geometry
the synthetic scenes were generated with, and the edges of the rule.  Then the symbols, the refusals that need no
device, the struct as the C++ consumer sees it, and the host-only width rule under the sanitizers in a stand-alone
program.

Tolerances of the geometry test.  The restatement runs on E_gt as the library takes it, rounded to fp32: a
relative 2^-24 = 6e-8 per entry.  Measured here, on the three cases below: max |R - R_gt| = 1.34e-8 (all three),
|t x t_gt| = 1.5e-9 (E_gt, -E_gt) and 1.51e-8 (views swapped), with unit t.  The bounds are ten times the largest
measured value of each, 1.4e-7 and 1.6e-7 (DESIGN.md §8b "Pose")."""
import ctypes
import json
import os
import subprocess

import numpy as np

from ransac_amd import synthetic
from tests.conftest import ROOT
from tests.helpers import multi_pose_ref as ref

DIR = os.path.join(ROOT, "tests", "cpp_multi_pose")
BIN = os.path.join(DIR, "build", "consumer")
R_TOL, T_TOL = 1.4e-7, 1.6e-7
ANCHOR_SEEDS = (1, 2, 3, 4)  # chosen on the CPU: no disagreement on any of them


def test_anchor_to_the_oracles_cheirality_flag(oracle):
    """oracle.e5_candidates gives every candidate's fp32 E and whether some projection puts all five sample points
    in front.  The oracle tests the fp64 E before the cast, the restatement the widened fp32 E: the two can differ
    only where a depth lies within rounding of zero."""
    total = differ = 0
    for seed in ANCHOR_SEEDS:
        pts, _, _ = synthetic.fundamental_points(n=400, inlier_ratio=0.5, seed=seed, normalized=True, prosac_order=False)
        est = oracle.Estimator(oracle.ESSENTIAL, pts)
        rng = np.random.default_rng(seed)
        for _ in range(40):
            s = rng.choice(len(pts), 5, replace=False).astype(np.int32)
            cand, ok = est.e5_candidates(s)
            r = pts[s].astype(np.float64)
            for m, flag in zip(cand, ok):
                mine = any(ref.in_front(r[:, 0], r[:, 1], r[:, 2], r[:, 3], P).all() for P in ref.projections(m))
                total += 1
                differ += int(mine != bool(flag))
    print("candidates compared: %d, disagreeing: %d (%.3f %%)" % (total, differ, 100.0 * differ / max(total, 1)))
    assert total >= 500
    assert differ <= 0.01 * total


def _scene():
    pts, E32, inl = synthetic.fundamental_points(n=600, inlier_ratio=0.5, seed=3, normalized=True, prosac_order=False)
    _, R, t, _, _ = synthetic.two_view_geometry()
    return pts, E32, inl, R, t / np.linalg.norm(t)


def _check_geometry(r, R_gt, t_gt, n_in, what):
    r_err = float(np.abs(r["R64"] - R_gt).max())
    t_err = float(np.linalg.norm(np.cross(r["t64"], t_gt)))
    det = float(np.linalg.det(r["R64"]))
    print("%s: choice %d, front %d of %d, |R - R_gt| %.3g, |t x t_gt| %.3g, det R - 1 %.3g"
          % (what, r["choice"], r["front"], n_in, r_err, t_err, det - 1.0))
    assert r["choice"] >= 0 and r["front"] == n_in and int(r["front_mask"].sum()) == n_in
    assert r_err <= R_TOL, (what, r_err)
    assert t_err <= T_TOL and float(r["t64"] @ t_gt) > 0, (what, t_err)  # parallel, and not opposite
    assert abs(det - 1.0) <= 1e-12, (what, det)
    assert abs(float(np.linalg.norm(r["t64"])) - 1.0) <= 1e-12


def test_geometry_of_the_synthetic_scene():
    pts, E32, inl, R_gt, t_gt = _scene()
    mask = inl.astype(np.uint8)
    n_in = int(inl.sum())
    a = ref.pose(E32, pts, mask)
    _check_geometry(a, R_gt, t_gt, n_in, "E_gt")
    np.testing.assert_array_equal(a["front_mask"], mask)
    b = ref.pose(-E32, pts, mask)
    _check_geometry(b, R_gt, t_gt, n_in, "-E_gt")
    # the two views swapped: E^T on rows x2 y2 x1 y1 is the pose of camera 1 seen from camera 2
    c = ref.pose(np.ascontiguousarray(E32.reshape(3, 3).T), pts[:, [2, 3, 0, 1]], mask)
    t_sw = -R_gt.T @ t_gt
    _check_geometry(c, R_gt.T, t_sw / np.linalg.norm(t_sw), n_in, "views swapped")
    # the sort of the singular values is an odd permutation somewhere among the three: det U = -1 there, the
    # chosen projection's block is a reflection and the rule's sign s = -1 is what makes R a rotation
    dets = [ref.det3(ref.projections(m.astype(np.float64).reshape(9))[r["choice"]])
            for m, r in ((E32, a), (-E32, b), (E32.reshape(3, 3).T, c))]
    assert min(dets) < 0 < max(dets), dets
    # the outputs are the doubles cast once
    np.testing.assert_array_equal(a["R"], a["R64"].astype(np.float32))
    np.testing.assert_array_equal(a["t"], a["t64"].astype(np.float32))


def _is_nothing(r, n):
    assert r["choice"] == -1 and r["front"] == 0
    np.testing.assert_array_equal(r["R"], np.eye(3, dtype=np.float32))
    np.testing.assert_array_equal(r["t"], np.zeros(3, dtype=np.float32))
    assert r["front_mask"].shape == (n,) and not r["front_mask"].any()


def test_rule_edges():
    pts, E32, inl, _, _ = _scene()
    n = len(pts)
    _is_nothing(ref.pose(E32, pts, np.zeros(n, dtype=np.uint8)), n)
    _is_nothing(ref.pose(np.full(9, np.nan, dtype=np.float32), pts, None), n)
    _is_nothing(ref.pose(np.zeros(9, dtype=np.float32), pts, None), n)
    _is_nothing(ref.pose(E32, pts, inl.astype(np.uint8), status=-111), n)  # USAC_ERR_NO_MODEL
    # a mask of one row: an inlier, so the scene's candidate and a count of 1
    full = ref.pose(E32, pts, inl.astype(np.uint8))
    one = np.zeros(n, dtype=np.uint8)
    one[np.flatnonzero(inl)[7]] = 1
    r = ref.pose(E32, pts, one)
    assert r["choice"] == full["choice"] and r["front"] == 1
    np.testing.assert_array_equal(r["front_mask"], one)
    np.testing.assert_array_equal(r["R"], full["R"])
    # a row of non-finite values under a set mask byte is in front of nothing
    bad = pts.copy()
    bad[np.flatnonzero(inl)[7]] = (np.nan, np.inf, -np.inf, 1.0)
    _is_nothing(ref.pose(E32, bad, one), n)
    # also where the comparisons alone would not say so: x2 alone is not finite, n0 is NaN, and in_front
    # triangulates the point from y2's row
    k = int(np.flatnonzero(inl)[7])
    for x2 in (np.nan, np.inf, -np.inf):
        bad = pts.copy()
        bad[k, 2] = x2
        r = bad[k].astype(np.float64)
        assert any(bool(ref.in_front(r[0], r[1], r[2], r[3], P)) for P in ref.projections(E32)), "the case shows nothing"
        _is_nothing(ref.pose(E32, bad, one), n)
    # a tie goes to the lower j.  Rows that satisfy no epipolar constraint triangulate to anything: take those the
    # restatement puts in front under exactly the candidates a and b, and those in front under none
    wild = np.random.default_rng(11).uniform(-2, 2, size=(2000, 4)).astype(np.float32)
    rows = wild.astype(np.float64)
    Ps = ref.projections(E32)
    f = np.stack([ref.in_front(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], P) for P in Ps], 1)
    pairs = {}
    for pat in map(tuple, f[f.sum(1) == 2]):
        pairs[pat] = pairs.get(pat, 0) + 1
    assert pairs, "no row is in front under exactly two candidates"
    pat = max(pairs, key=pairs.get)
    lo, hi = np.flatnonzero(pat)
    tie = ((f == np.array(pat)).all(1) | ~f.any(1)).astype(np.uint8)
    r = ref.pose(E32, wild, tie)
    assert r["counts"][lo] == r["counts"][hi] == pairs[pat] > 0 and r["counts"].sum() == 2 * pairs[pat]
    assert r["choice"] == lo and r["front"] == pairs[pat] and 0 < r["front"] < int(tie.sum())
    np.testing.assert_array_equal(r["front_mask"], (f == np.array(pat)).all(1).astype(np.uint8))


def test_batch_helper_is_the_rule_per_problem():
    pts, E32, inl, _, _ = _scene()
    offsets = np.array([0, 5, 70, 600], dtype=np.uint32)
    models = np.stack([E32.reshape(9), -E32.reshape(9), np.zeros(9, dtype=np.float32)])
    mask = inl.astype(np.uint8)
    got = ref.pose_batch(models, pts, offsets, mask, status=[0, 0, 0])
    for p in range(3):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        one = ref.pose(models[p], pts[lo:hi], mask[lo:hi])
        np.testing.assert_array_equal(got["R"][p], one["R"])
        np.testing.assert_array_equal(got["t"][p], one["t"])
        assert got["front"][p] == one["front"] and got["choice"][p] == one["choice"]
        np.testing.assert_array_equal(got["front_mask"][lo:hi], one["front_mask"])
    assert got["choice"][2] == -1 and got["front"][0] == int(inl[:5].sum())


def test_abi_version_and_symbols(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 28
    for name in ("usac_multi_pose_device", "usac_multi_pose"):
        assert name in usac.ABI_SYMBOLS
        assert hasattr(L, name)
    assert callable(usac.MultiContext.export_pose) and callable(usac.MultiContext.pose)


def test_null_contexts_are_refused(usac):
    L = usac.lib()
    fake = 0x7f0000001000  # an aligned address nothing dereferences: both cases return before they could
    o = usac._MultiPoseOutput(n_max=10, R=fake)
    assert L.usac_multi_pose_device(None, ctypes.byref(o)) == -1
    assert L.usac_multi_pose_device(None, None) == -1
    E = np.zeros(9, dtype=np.float32)
    ch = np.zeros(1, dtype=np.int32)
    assert L.usac_multi_pose(None, E.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None, None, None, None,
                             ch.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None) == -1
    assert L.usac_multi_pose(None, None, None, None, None, None, None, None) == -1


def test_struct_mirror_matches_the_header(usac):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 28
    S = usac._MultiPoseOutput
    assert ctypes.sizeof(S) == d["sizeof"]
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == d["offsets"]


def test_width_rule_under_sanitizers(tmp_path):
    """the host-only argument rule the pose and export entries share (usac_pack.hpp), as g++ compiles it"""
    exe = str(tmp_path / "pose_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"), os.path.join(DIR, "pose_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
