"""LO-RANSAC on multi contexts of essential-matrix problems (usac_multi_lo_essential,
usac_multi_run_lo_essential; ABI 23), the parts that need no device: the symbols, the NULL-argument errors,
and the yardstick of tests/test_gpu_multi_essential_lo.py -- multi_lo_ref.lo_ref over the oracle's essential
estimator -- taking every branch the GPU tests rely on, on those tests' own inputs."""
import ctypes

import numpy as np
import pytest

from tests.helpers import multi_essential_lo_ref as eref
from tests.helpers import multi_lo_ref as ref
from tests.helpers import multi_polish_ref as pref

ERR_ARG = -1


def test_abi_version_and_symbols(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 23
    assert {"usac_multi_lo_essential", "usac_multi_run_lo_essential"} <= set(usac.ABI_SYMBOLS)
    assert hasattr(L, "usac_multi_lo_essential") and hasattr(L, "usac_multi_run_lo_essential")
    assert hasattr(usac.MultiContext, "lo_essential") and hasattr(usac.MultiContext, "run_lo_essential")


def test_null_arguments_are_rejected_without_a_device(usac):
    L = usac.lib()
    prm = usac._Params()
    prm.lo = int(usac.LocOpt.InItLORsc)
    out = (usac._MultiOutput * 1)()
    recs = (usac.Record * 1)()
    fake = ctypes.c_void_p(16)  # never dereferenced: every call below fails on a NULL first
    assert L.usac_multi_run_lo_essential(None, ctypes.byref(prm), None, out, None, None, None, None) == ERR_ARG
    assert L.usac_multi_run_lo_essential(fake, None, None, out, None, None, None, None) == ERR_ARG
    assert L.usac_multi_run_lo_essential(fake, ctypes.byref(prm), None, None, None, None, None, None) == ERR_ARG
    assert L.usac_multi_lo_essential(None, ctypes.byref(prm), 1, None, recs, None) == ERR_ARG
    assert L.usac_multi_lo_essential(fake, None, 1, None, recs, None) == ERR_ARG
    assert L.usac_multi_lo_essential(fake, ctypes.byref(prm), 1, None, None, None) == ERR_ARG


@pytest.fixture(scope="module")
def hook(oracle):
    return eref.hook_problems(oracle)


@pytest.fixture(scope="module")
def two_calls(usac, hook):
    """limited -> the hook test's two calls on the restatement (the copy left out of the tallies)"""
    _, ests, recs, seeds = hook
    n = len(eref.SIZES)
    return {lim: eref.ref_calls(usac, ests[:n], recs[:n], seeds[:n], ref.LoParams(thr=eref.THR, limited=lim, m=eref.M), 2)
            for lim in (False, True)}


def _total(calls):
    tot = {}
    for call in calls:
        for _, _, t in call:
            for key, v in t.items():
                tot[key] = tot.get(key, 0) + v
    return tot


def test_restatement_takes_every_branch_on_the_test_inputs(usac, oracle, hook, two_calls):
    t = {lim: _total(two_calls[lim]) for lim in (False, True)}
    for lim in (False, True):
        assert t[lim]["below12"] > 0                              # the < 12 return
        assert t[lim]["fit_all"] > 0                              # 12 .. lo_sample_size inliers
        assert t[lim]["sampled"] > 0
        assert t[lim]["stage_done"] > 0 and t[lim]["improved"] > 0
        assert t[lim]["fit_failed"] == 0                          # (no input of ours fails a fit: DESIGN §8b)
        assert t[lim]["capped"] == 0
    assert t[False]["stage_break"] > 0 and t[False]["stage_draw"] == 0   # best_score->bigger(lo_score)
    assert t[True]["stage_draw"] > 0 and t[True]["stage_break"] == 0     # the limited variant's draw
    # the unlimited variant lifts the two large problems well past their minimal models
    first = [r for r, _, _ in two_calls[False][0]]
    _, _, recs, _ = hook
    assert first[6]["inliers"] > 5 * recs[6]["inliers"] and first[5]["inliers"] > recs[5]["inliers"] + 50
    # a capped call: one fit (the first inner iteration's), whose list at 10 θ is past the cap
    pts, rec = eref.cap_problem(oracle)
    est, prm = eref.estimator(oracle, pts), ref.LoParams(thr=eref.THR, m=eref.M)
    assert rec["inliers"] == 3914 and len(pts) == eref.CAP_N > ref.FIT_MAX
    r, st, tl = ref.lo_ref(usac, est, rec, ref.fresh_state(prm), 32, prm)
    assert tl["capped"] == 1 and st["capped"] == 1 and st["fits"] == 1 and st["inner_iters"] == 0
    assert pref.bits(st["threshold"]) == pref.bits(prm.thr)
    ref.assert_same_record(r, rec)


def test_restatement_few_inliers_take_the_continue(usac, oracle):
    """a degenerate sample (14 copies of one correspondence): the fitted model has <= 5 inliers in some
    inner iterations -- the `<= m` continue, which leaves K * threshold in place -- and more in others,
    unlike H / F where all ten take it"""
    pts, rec = eref.few_problem(oracle)
    est, prm = eref.estimator(oracle, pts), ref.LoParams(thr=eref.THR, m=eref.M)
    assert rec["inliers"] == 16
    r, st, t = ref.lo_ref(usac, est, rec, ref.fresh_state(prm), 909, prm)
    assert 0 < t["few"] < prm.inner and t["sampled"] == prm.inner and st["draws"] == prm.inner
    assert st["inner_iters"] == prm.inner - t["few"]
    ref.assert_same_record(r, rec)


def test_restatement_properties(usac, oracle, hook, two_calls):
    """no record gets worse, a problem below the floor is untouched, and a threshold whose steps are inexact
    in fp32 persists as left"""
    pts, ests, recs, seeds = hook
    for lim in (False, True):
        for p, (rec, st, _) in enumerate(two_calls[lim][0]):
            assert not ref.bigger(recs[p]["inliers"], recs[p]["score"], rec["inliers"], rec["score"])
            assert rec["hyp_index"] == recs[p]["hyp_index"]
            if recs[p]["inliers"] < 12:
                ref.assert_same_record(rec, recs[p])
                assert st["fits"] == 0
    assert any(r["inliers"] < 12 for r in recs) and all(r["valid"] for r in recs)
    prm = ref.LoParams(thr=0.0017, iters=3, m=eref.M)
    rec = eref.start_record(oracle, pts[5], eref.START_SEED + 5, est=ests[5], thr=0.0017)
    _, st, _ = ref.lo_ref(usac, ests[5], rec, ref.fresh_state(prm), seeds[5], prm)
    assert pref.bits(st["threshold"]) != pref.bits(prm.thr) and abs(float(st["threshold"]) - 0.0017) < 1e-5
