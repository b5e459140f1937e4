"""Multi-problem LO-RANSAC (usac_multi_lo, usac_multi_run_lo; ABI 18), the parts that need no device:
the LO draw (usac_lo_draw), the NULL-argument errors of the new entry points, and the yardstick of
tests/test_gpu_multi_lo.py -- the LO's control flow restated over the oracle (tests/helpers/
multi_lo_ref.py) -- taking every branch the GPU tests rely on, on those tests' own inputs."""
import ctypes

import numpy as np
import pytest

from tests.helpers import multi_lo_ref as ref
from tests.helpers import multi_polish_ref as pref

ERR_ARG = -1


def test_abi_version_and_layout(usac):
    assert usac.lib().usac_abi_version() >= 18
    assert {"usac_lo_draw", "usac_multi_lo", "usac_multi_run_lo"} <= set(usac.ABI_SYMBOLS)
    assert ctypes.sizeof(usac._MultiLoOutput) == 32 and usac._MultiLoOutput.threshold.offset == 28


@pytest.mark.parametrize("k,top", [(1, 0), (1, 5), (14, 14), (14, 15), (14, 999), (64, 63), (64, 64), (64, 100000), (7, 2 ** 31 - 1)])
def test_lo_draw_sets(usac, k, top):
    seen = set()
    for seed, draw in [(1, 0), (1, 1), (1, 2), (2, 0), (2 ** 63 + 5, 7)]:
        d = usac.lo_draw(seed, draw, k, top)
        assert d.dtype == np.int32 and d.shape == (k,)
        assert (d >= 0).all() and (d <= top).all() and len(set(d.tolist())) == k
        np.testing.assert_array_equal(d, usac.lo_draw(seed, draw, k, top))  # deterministic
        seen.add(tuple(d.tolist()))
    if top >= 999:  # (a small range leaves few sets to tell apart)
        assert len(seen) == 5  # another draw or another seed: another set


def test_lo_draw_full_range_is_a_permutation(usac):
    for k in (1, 2, 14, 64):
        a, b = usac.lo_draw(3, 0, k, k - 1), usac.lo_draw(3, 1, k, k - 1)
        assert sorted(a.tolist()) == sorted(b.tolist()) == list(range(k))
        assert k < 14 or a.tolist() != b.tolist()


def test_lo_draw_argument_errors(usac):
    for k, top in [(0, 10), (65, 1000), (5, 3), (2, 0), (1, 2 ** 31)]:
        with pytest.raises(usac.UsacError) as e:
            usac.lo_draw(1, 0, k, top)
        assert e.value.code == ERR_ARG
    assert usac.lib().usac_lo_draw(1, 0, 4, 9, None) == ERR_ARG


def test_null_arguments_are_rejected_without_a_device(usac):
    L = usac.lib()
    prm = usac._Params()
    prm.lo = int(usac.LocOpt.InItLORsc)
    out = (usac._MultiOutput * 1)()
    recs = (usac.Record * 1)()
    fake = ctypes.c_void_p(16)  # never dereferenced: every call below fails on a NULL first
    assert L.usac_multi_run_lo(None, ctypes.byref(prm), None, out, None, None, None, None) == ERR_ARG
    assert L.usac_multi_run_lo(fake, None, None, out, None, None, None, None) == ERR_ARG
    assert L.usac_multi_run_lo(fake, ctypes.byref(prm), None, None, None, None, None, None) == ERR_ARG
    assert L.usac_multi_lo(None, ctypes.byref(prm), 1, None, recs, None) == ERR_ARG
    assert L.usac_multi_lo(fake, None, 1, None, recs, None) == ERR_ARG
    assert L.usac_multi_lo(fake, ctypes.byref(prm), 1, None, None, None) == ERR_ARG


def _tally(usac, oracle, kind, limited, calls=2):
    """the hook tests' calls on the restatement alone: the branch tallies summed, the per-problem results"""
    prm = ref.LoParams(limited=limited, m=pref.estimator(oracle, kind, ref.sets(kind)[0]).m)
    total, res = {}, []
    for p, pts in enumerate(ref.sets(kind)):
        est = pref.estimator(oracle, kind, pts)
        rec, st = ref.start_record(oracle, kind, pts, ref.START_SEED + p, est=est), ref.fresh_state(prm)
        for _ in range(calls):
            rec, st, t = ref.lo_ref(usac, est, rec, st, ref.DRAW_SEEDS[p], prm)
            for key, v in t.items():
                total[key] = total.get(key, 0) + v
        res.append((rec, st))
    return total, res


def test_restatement_takes_every_branch_on_the_test_inputs(usac, oracle):
    t = {(kind, lim): _tally(usac, oracle, kind, lim)[0] for kind in "HF" for lim in (False, True)}
    every = {key: sum(v[key] for v in t.values()) for key in t["H", False]}
    for kind in "HF":
        assert t[kind, False]["below12"] > 0                      # the < 12 return
        assert t[kind, False]["fit_all"] > 0                      # 12 .. lo_sample_size inliers
        assert t[kind, False]["sampled"] > 0 and t[kind, True]["sampled"] > 0
        assert t[kind, False]["improved"] > 0 and t[kind, False]["stage_done"] > 0   # a completed stage that improved
        assert t[kind, True]["stage_draw"] > 0 and t[kind, True]["improved"] > 0     # the limited variant's draw
        assert t[kind, False]["stage_draw"] == 0
    assert t["F", False]["stage_break"] > 0                       # best_score->bigger(lo_score): fail, reset
    assert every["fit_failed"] == 0                               # (no input of ours fails a fit: DESIGN §8b)
    # a capped call
    pts, rec = ref.cap_problem(oracle)
    est, prm = pref.estimator(oracle, "H", pts), ref.LoParams()
    assert rec["inliers"] == ref.CAP_N
    r, st, tl = ref.lo_ref(usac, est, rec, ref.fresh_state(prm), 5, prm)
    assert tl["capped"] == 1 and st["capped"] == 1 and st["fits"] == 1 and st["inner_iters"] == 0
    assert pref.bits(st["threshold"]) == pref.bits(prm.thr)
    ref.assert_same_record(r, rec)
    # without the caps the same call goes on and improves nothing less
    r2, st2, tl2 = ref.lo_ref(usac, est, rec, ref.fresh_state(prm), 5, prm, fit_max=10 ** 9)
    assert tl2["capped"] == 0 and st2["inner_iters"] == prm.inner


@pytest.mark.parametrize("kind", ["H", "F"])
def test_restatement_few_inliers_leaves_the_threshold_compounded(usac, oracle, kind):
    """a degenerate sample (14 copies of one correspondence) fits a NaN model without inliers: the
    `<= sample_size` continue, which leaves K * threshold in place for the next iteration"""
    pts, rec = ref.few_problem(oracle, kind)
    est = pref.estimator(oracle, kind, pts)
    prm = ref.LoParams(m=est.m)
    assert rec["inliers"] == 16
    r, st, t = ref.lo_ref(usac, est, rec, ref.fresh_state(prm), 9, prm)
    assert t["few"] == prm.inner and t["sampled"] == prm.inner and st["inner_iters"] == 0 and st["draws"] == prm.inner
    want = prm.thr
    for _ in range(prm.inner):
        want = np.float32(prm.mult * want)
    assert pref.bits(st["threshold"]) == pref.bits(want)
    ref.assert_same_record(r, rec)


def test_restatement_properties(usac, oracle):
    """no record gets worse, a problem below the floor is untouched, the copy with its original's seed and
    start gets its original's result, and a threshold whose steps are inexact in fp32 persists as left"""
    for kind in "HF":
        for lim in (False, True):
            _, res = _tally(usac, oracle, kind, lim, calls=1)
            for p, pts in enumerate(ref.sets(kind)):
                start = ref.start_record(oracle, kind, pts, ref.START_SEED + p)
                rec, st = res[p]
                assert not ref.bigger(start["inliers"], start["score"], rec["inliers"], rec["score"])
                assert rec["hyp_index"] == start["hyp_index"]
                if start["inliers"] < 12:
                    ref.assert_same_record(rec, start)
                    assert st["fits"] == 0
    pts = ref.sets("H")[5]
    est = pref.estimator(oracle, "H", pts)
    prm = ref.LoParams(thr=1.7, iters=3, m=4)
    rec = ref.start_record(oracle, "H", pts, ref.START_SEED + 5, est=est, thr=1.7)
    _, st, _ = ref.lo_ref(usac, est, rec, ref.fresh_state(prm), 1, prm)
    assert pref.bits(st["threshold"]) != pref.bits(prm.thr) and abs(float(st["threshold"]) - 1.7) < 1e-5
