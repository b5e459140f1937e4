"""Multi-problem PROSAC (ABI 17), the parts that need no device: the sampler's closed-form schedule
(usac_prosac_schedule) against a Python port of the reference's sampler state machine
(tests/helpers/prosac_ref.py) and against the host ProsacSampler, and usac_multi_run_prosac's NULL
argument errors."""
import ctypes

import numpy as np
import pytest

from tests.helpers import prosac_ref as ref

SHAPES = [(21, 4), (25, 7), (64, 4), (65, 7), (333, 7), (1000, 4), (1000, 7), (5000, 4)]
R = 64


def test_abi_version(usac):
    assert usac.lib().usac_abi_version() >= 17


def _term_lens(n, m, rounds, rng):
    """a termination length per round: n for a while, then shrunk, grown back, equal to n again"""
    out = []
    for r in range(rounds):
        phase = (r // 5) % 4
        if phase == 0 or phase == 3:
            out.append(n)
        elif phase == 1:
            out.append(int(rng.integers(m, max(m + 1, n // 2))))
        else:
            out.append(int(rng.integers(n // 2, n + 1)))
    return out


@pytest.mark.parametrize("n,m", SHAPES)
def test_schedule_equals_the_sampler_state_machine(usac, n, m):
    rng = np.random.default_rng(n * 10 + m)
    rounds = 400 if n <= 1000 else 120
    sm = ref.SamplerState(n, m)
    clock, largest = 1, m
    frozen = prosac = 0
    for L in _term_lens(n, m, rounds, rng):
        L = max(L, m)
        sub, clock_next, largest_next = usac.prosac_schedule(n, m, clock, L, R, largest)
        want = np.array([sm.step(L) for _ in range(R)], dtype=np.uint32)
        np.testing.assert_array_equal(sub, want)
        assert clock_next == sm.hyp and largest_next == sm.largest
        # the PROSAC lanes are a prefix, and the clock advances by their number
        k = int((sub != 0).sum())
        assert (sub[:k] != 0).all() and (sub[k:] == 0).all() and clock_next == clock + k
        frozen += R - k
        prosac += k
        clock, largest = clock_next, largest_next
    assert prosac > 0 and frozen > 0


def test_schedule_past_the_growth_table(usac):
    n, m = 333, 7
    sub, nxt, lg = usac.prosac_schedule(n, m, ref.T_N - 9, n, R, n)
    assert (sub[:10] == n).all() and (sub[10:] == usac.UNIFORM_OVER_N).all()
    assert nxt == ref.T_N + 1 and lg == n
    sub, nxt, _ = usac.prosac_schedule(n, m, ref.T_N + 1, 50, R, n)
    assert (sub == usac.UNIFORM_OVER_N).all() and nxt == ref.T_N + 1


@pytest.mark.parametrize("n,m,count", [(64, 4, 3000), (333, 7, 5000), (1000, 4, 2000)])
def test_schedule_equals_the_host_sampler(usac, n, m, count):
    """the host ProsacSampler's last sample point is subset - 1 (termination_length = n)"""
    smp = usac.prosac_samples(7, n, m, count)
    sub = np.concatenate([usac.prosac_schedule(n, m, 1 + k, n, R)[0] for k in range(0, count + R, R)])[:count]
    np.testing.assert_array_equal(smp[:, m - 1] + 1, sub)
    assert len(np.unique(sub)) > 3  # count runs past several subset changes


def test_schedule_argument_errors(usac):
    for n, m, clock, L in [(3, 4, 1, 3), (100, 4, 0, 100), (100, 4, 1, 3), (100, 4, 1, 101), (100, 1, 1, 100)]:
        with pytest.raises(usac.UsacError) as e:
            usac.prosac_schedule(n, m, clock, L, R)
        assert e.value.code == -1


def test_run_prosac_null_arguments(usac):
    L = usac.lib()
    prm = usac._Params()
    out = (usac._MultiOutput * 1)()
    handle = ctypes.c_void_p(1)  # never dereferenced: the NULL checks come first
    assert L.usac_multi_run_prosac(None, ctypes.byref(prm), None, out, None, None, None) == -1
    assert L.usac_multi_run_prosac(handle, None, None, out, None, None, None) == -1
    assert L.usac_multi_run_prosac(handle, ctypes.byref(prm), None, None, None, None, None) == -1
    assert L.usac_multi_draw_samples(None, None, 0, 64, None, 0, None, None, None) == -1
    assert L.usac_multi_prosac_scan(None, ctypes.byref(prm), 1, None, None, None, None, None, None, None) == -1
