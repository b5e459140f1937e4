"""Multi-problem SPRT (usac_multi_sprt_setup, usac_multi_hypothesize_score_sprt, usac_multi_sprt_update,
usac_multi_run_sprt; ABI 19), the parts that need no device: the exported per-round update against its
Python restatement (tests/helpers/multi_sprt_ref.py) over scripted rounds that take every branch, against
the oracle's SPRT handle where the sequences coincide, the argument errors decided before any device call,
and the update's host text under the sanitizers in a stand-alone program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import multi_sprt_ref as ref

ERR_ARG = -1
DIR = os.path.join(ROOT, "tests", "cpp_multi_sprt")


def test_abi_version_and_layout(usac):
    assert usac.lib().usac_abi_version() >= 19
    assert {"usac_multi_sprt_setup", "usac_multi_hypothesize_score_sprt", "usac_multi_sprt_update",
            "usac_multi_run_sprt"} <= set(usac.ABI_SYMBOLS)
    assert ctypes.sizeof(usac._MultiSprtStats) == 32 and usac._MultiSprtStats.points_tested.offset == 24
    assert ctypes.sizeof(usac._MultiSprtTest) == 32 and usac._MultiSprtTest.k.offset == 24
    assert ctypes.sizeof(usac._MultiSprtOutput) == 48 and usac._MultiSprtOutput.points_tested.offset == 40


# (head_inliers, head_points, improved, best_inliers, term_bound); n = 1000, R = 64.  H starts at
# (0.1, 0.01), F at (0.2, 0.05).
N, R, MAX = 1000, 64, 4096
SCRIPTS = {
    # every branch in one sequence: delta only; neither (delta^ within 5 % of the new delta); epsilon only
    # (no head points); both; the guard by epsilon^ = 1 on an all-inlier record, then by delta^ >= epsilon'
    "branches": [(300, 10000, False, 0, 0), (303, 10000, False, 0, 0), (0, 0, True, 300, 900),
                 (900, 10000, True, 350, 800), (0, 0, False, 0, 0), (0, 0, True, 1000, 3000),
                 (9000, 10000, False, 0, 0), (0, 0, True, 400, 700)],
    # a record of 2 % inliers: P_g ~ 1e-7 (H) / 1e-12 (F), |log(1 - P_g (1 - 1 / A))| < 1e-5 -> max_iterations
    "denominator": [(0, 0, True, 20, 4000)],
    # a long history under an epsilon far too low, then a 90 % record: log(0.05) - log_eta >= 0 -> 0
    "zero_bound": [(0, 0, True, 300, 4096), (0, 0, True, 320, 4096), (0, 0, True, 900, 4096)],
}


def _five_percent(kind):
    """delta^ just inside and just outside the 5 % test around the start delta"""
    d0 = ref.DEFAULTS[kind][1]
    pts = 1000000
    inside, outside = int(round(d0 * 1.0499 * pts)), int(round(d0 * 1.0501 * pts))
    return [(inside, pts, False, 0, 0), (outside, pts, False, 0, 0)]


def _drive(usac, kind, script):
    got = usac.MultiSprtState(ref.EST_ID[kind], N, ref.M[kind], MAX)
    want = ref.RefState(kind, N, MAX)
    ref.assert_same_state(got, want, (kind, "initial"))
    designed = []
    for r, (hi, hp, imp, best, tb) in enumerate(script):
        done = (r + 1) * R
        g = usac.multi_sprt_update(got, done, hi, hp, imp, best, tb)
        w = want.update(done, hi, hp, imp, best, tb)
        assert g == w, (kind, r)
        ref.assert_same_state(got, want, (kind, r))
        designed.append(w)
    return got, want, designed


@pytest.mark.parametrize("kind", ["H", "F"])
def test_update_equals_restatement_on_every_branch(usac, kind):
    got, want, designed = _drive(usac, kind, SCRIPTS["branches"])
    assert designed == [True, False, True, True, False, False, False, True]
    assert {"delta", "neither", "epsilon", "both", "no_head_points", "guard"} <= want.taken
    # k sits on the new entry: the hypotheses evaluated under the previous test
    assert [h[3] for h in got.history] == [0, 64, 128, 64, 256]
    assert got.last_update == 512 and sum(h[3] for h in got.history) == 512
    # the guard left the test alone in rounds 6 and 7, and round 6's all-inlier record still set the bound
    assert got.history[3][0] == float(np.float32(350) / np.float32(1000))
    assert got.bound == want.bound <= 700  # min(term_bound, getUpperBoundIterations) of the last improving round


@pytest.mark.parametrize("kind", ["H", "F"])
def test_update_five_percent_test(usac, kind):
    _, want, designed = _drive(usac, kind, _five_percent(kind))
    assert designed == [False, True]
    assert want.taken == {"neither", "delta"}


@pytest.mark.parametrize("kind", ["H", "F"])
def test_update_bound_exits(usac, kind):
    got, want, _ = _drive(usac, kind, SCRIPTS["denominator"])
    assert "denominator" in want.taken and got.bound == 4000       # min(term_bound, max_iterations)
    got, want, designed = _drive(usac, kind, SCRIPTS["zero_bound"])
    assert designed == [True, True, True]
    assert "numerator>=0" in want.taken and got.bound == 0
    # a round that does not improve the record keeps the bound
    assert not usac.multi_sprt_update(got, 4 * R, 0, 0, False)
    assert got.bound == 0


@pytest.mark.parametrize("kind,n", [("H", 1000), ("F", 1000), ("H", 64), ("F", 65)])
def test_update_equals_oracle_handle_where_the_sequences_coincide(usac, oracle, kind, n):
    """A_0, and after one accepted model found at hypothesis 64 with more inliers than the best so far -- an
    epsilon-only history, as an improving round without head rejections gives -- the history's k and A, and
    getUpperBoundIterations of the oracle's own SPRT object"""
    okind, m = ref.oracle_kind(oracle, kind), ref.M[kind]
    pts, inl = ref.sets(kind)
    p = ref.SIZES[kind].index(n)
    pts, inl = pts[p], inl[p]
    est = oracle.Estimator(okind, pts)
    L = oracle.lib()
    _, A0 = oracle.sprt_pool(5, okind, n, m, MAX)
    st = usac.MultiSprtState(ref.EST_ID[kind], n, m, MAX)
    assert ref.bits64(st.history[0][2]) == ref.bits64(A0)
    # a model the reference's walk accepts: the non-minimal fit to the known inliers
    mdl = est.nonminimal(np.flatnonzero(inl).astype(np.int32))
    assert mdl is not None
    mdl = np.ascontiguousarray(mdl, dtype=np.float32)
    L.orc_srandom(ctypes.c_uint(5))
    s = L.orc_sprt_new(okind, n, m, MAX, 20)
    L.orc_sprt_verify.restype = ctypes.c_int
    L.orc_sprt_verify.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_uint,
                                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint)]
    L.orc_est_set_model.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    L.orc_sprt_histories.restype = ctypes.c_uint
    L.orc_sprt_histories.argtypes = [ctypes.c_void_p]
    L.orc_est_set_model(est._h, mdl.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    cnt, sc, tested = ctypes.c_int(0), ctypes.c_float(0), ctypes.c_uint(0)
    try:
        good = L.orc_sprt_verify(s, est._h, ctypes.c_float(ref.THR), 64, 0, ctypes.byref(cnt), ctypes.byref(sc),
                                 ctypes.byref(tested))
        assert good and 0 < cnt.value < n and L.orc_sprt_histories(s) == 2
        assert st.update(64, 0, 0, True, cnt.value, MAX)
        assert st.history[1][3] == 64 and ref.bits64(st.history[1][2]) == ref.bits64(L.orc_sprt_A(s))
        assert st.bound == L.orc_sprt_upper_bound(s, cnt.value)
        # the same history, other counts: the restatement's bound is the oracle's
        w = ref.RefState(kind, n, MAX)
        w.update(64, 0, 0, True, cnt.value, MAX)
        for later in (cnt.value, min(n, cnt.value + 50), n // 2, n):
            assert w.upper_bound(later) == L.orc_sprt_upper_bound(s, later), later
    finally:
        L.orc_sprt_free(s)


def test_update_argument_errors(usac):
    L = usac.lib()
    hist = (usac._MultiSprtTest * 2)()
    nh, last, bound = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    args = (ctypes.byref(nh), 2, ctypes.byref(last), ctypes.byref(bound), 0, 0, 0, 0, 0, 0)
    assert L.usac_multi_sprt_update(2, 100, 4, 512, None, *args) == ERR_ARG
    assert L.usac_multi_sprt_update(1, 100, 4, 512, hist, *args) == ERR_ARG   # the line estimator
    assert L.usac_multi_sprt_update(4, 100, 5, 512, hist, *args) == ERR_ARG   # the essential estimator
    assert L.usac_multi_sprt_update(2, 3, 4, 512, hist, *args) == ERR_ARG     # n < m
    assert L.usac_multi_sprt_update(2, 100, 4, 512, hist, None, 2, ctypes.byref(last), ctypes.byref(bound), 0, 0, 0, 0, 0, 0) == ERR_ARG
    assert L.usac_multi_sprt_update(2, 100, 4, 512, hist, *args) == 0 and nh.value == 1 and bound.value == 512
    # a full history refuses a new test
    st = usac.MultiSprtState(2, 100, 4, 512, cap=2)
    assert st.update(64, 0, 0, True, 30, 512)
    with pytest.raises(usac.UsacError) as e:
        st.update(128, 0, 0, True, 40, 512)
    assert e.value.code == ERR_ARG


def test_null_arguments_are_rejected_without_a_device(usac):
    L = usac.lib()
    prm = usac._Params()
    prm.sprt = 1
    out = (usac._MultiOutput * 1)()
    fake = ctypes.c_void_p(16)  # never dereferenced: every call below fails on a NULL first
    assert L.usac_multi_run_sprt(None, ctypes.byref(prm), None, out, None, None, None, None) == ERR_ARG
    assert L.usac_multi_run_sprt(fake, None, None, out, None, None, None, None) == ERR_ARG
    assert L.usac_multi_run_sprt(fake, ctypes.byref(prm), None, None, None, None, None, None) == ERR_ARG
    assert L.usac_multi_sprt_setup(None, None) == ERR_ARG
    assert L.usac_multi_hypothesize_score_sprt(None, None, 0, None, 64, None, 0, ctypes.c_float(2.0), 0, None, None, None,
                                               None, None, None) == ERR_ARG


def test_update_host_text_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sprt_update_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"), os.path.join(DIR, "sprt_update_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, str(tmp_path / "scratch.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def test_cpp_multi_sprt_consumer_compiles_and_links(usac):
    import json

    subprocess.run(["make", "-s", "-C", DIR], check=True)
    r = subprocess.run([os.path.join(DIR, "build", "consumer"), "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 19
