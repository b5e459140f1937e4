"""Per-problem thresholds of a multi context (usac_multi_set_thresholds / usac_multi_get_thresholds,
ABI 22): what can be checked without a GPU -- the version, the symbols, the NULL-handle refusals and
the C++ consumer of the header (g++ -std=c++11 -Werror).  The calls on a context are left to
tests/test_gpu_multi_thresholds.py."""
import ctypes
import json
import os
import subprocess

import numpy as np

from tests.conftest import ROOT

DIR = os.path.join(ROOT, "tests", "cpp_multi_thresholds")
BIN = os.path.join(DIR, "build", "consumer")
ERR_ARG = -1


def test_abi_version(usac):
    assert usac.lib().usac_abi_version() >= 22


def test_symbols_resolve(usac):
    L = usac.lib()
    assert hasattr(L, "usac_multi_set_thresholds") and hasattr(L, "usac_multi_get_thresholds")
    assert {"usac_multi_set_thresholds", "usac_multi_get_thresholds"} <= set(usac.ABI_SYMBOLS)
    assert callable(usac.MultiContext.set_thresholds)
    assert isinstance(usac.MultiContext.thresholds, property)


def test_null_handle_is_refused(usac):
    L = usac.lib()
    t = np.ones(3, dtype=np.float32)
    tp = t.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.usac_multi_set_thresholds(None, tp) == ERR_ARG
    assert L.usac_multi_set_thresholds(None, None) == ERR_ARG
    assert L.usac_multi_get_thresholds(None, tp) == ERR_ARG
    assert (t == 1).all()


def test_cpp_consumer_compiles_and_agrees_on_the_abi(usac):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 22
