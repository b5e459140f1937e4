"""Device input in quality order (usac_multi_create_device_sorted, ABI 26), the part that needs no GPU: the symbol,
every refusal that comes before any device call, the Python layer's own checks of `scores`, the layout of
usac_multi_device_order as the C++ consumer sees it, and the sort key host and device share
(ransac_amd/csrc/usac_sort_key.hpp) held to the written rule (tests/helpers/multi_sorted_ref.py) under the
sanitizers in a stand-alone program."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import multi_sorted_ref as sref

DIR = os.path.join(ROOT, "tests", "cpp_multi_device_sorted")
BIN = os.path.join(DIR, "build", "consumer")
H, F, E, LINE = 2, 3, 4, 1
FAKE = 0x7f0000001000  # a 16-byte-aligned address nothing dereferences: every case below returns before it could


def test_abi_version_and_symbol(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 26
    assert "usac_multi_create_device_sorted" in usac.ABI_SYMBOLS
    assert hasattr(L, "usac_multi_create_device_sorted")


def _create(usac, estimator, order="scores", **fields):
    h = ctypes.c_void_p(12345)
    inp = usac._MultiDeviceInput(**fields)
    if order == "scores":
        order = usac._MultiDeviceOrder(scores=FAKE, descending=1)
    rc = usac.lib().usac_multi_create_device_sorted(ctypes.byref(h), 0, estimator, ctypes.byref(inp),
                                                    None if order is None else ctypes.byref(order))
    assert h.value is None, "a refused creation left *out set"
    return rc


def test_argument_errors_come_before_any_device_call(usac):
    """each case returns its code on a machine without a GPU: a device call would have returned -2 there"""
    L = usac.lib()
    a = dict(P=2, n_max=10, rows=FAKE)                                 # form a
    b = dict(P=2, n_max=10, kpts0=FAKE, kpts1=FAKE, n1=7, match=FAKE)  # form b
    for form in (a, b):
        for est in (H, F, E):
            assert _create(usac, est, order=None, **form) == -1        # NULL order
            assert _create(usac, est, order=usac._MultiDeviceOrder(scores=None, descending=1), **form) == -1
            assert _create(usac, est, order=usac._MultiDeviceOrder(scores=None, descending=0), **form) == -1
    msg = L.usac_multi_last_error(None)
    assert b"usac_multi_create_device_sorted" in msg and b"scores" in msg
    # what usac_multi_create_device refuses, with its codes
    order = usac._MultiDeviceOrder(scores=FAKE, descending=1)
    h = ctypes.c_void_p(12345)
    assert L.usac_multi_create_device_sorted(None, 0, H, ctypes.byref(usac._MultiDeviceInput(**a)), ctypes.byref(order)) == -1
    assert L.usac_multi_create_device_sorted(ctypes.byref(h), 0, H, None, ctypes.byref(order)) == -1 and h.value is None
    cases = [(LINE, a), (LINE, b), (H, dict(a, P=0)), (H, dict(b, P=0)), (H, dict(a, P=65536)), (H, dict(a, n_max=0)),
             (H, dict(a, P=65535, n_max=65538)), (H, dict(P=2, n_max=10)),
             (H, dict(a, **{k: v for k, v in b.items() if k not in a})),  # both forms
             (H, dict(a, valid=FAKE, counts=FAKE)), (F, dict(b, n1=0)), (F, {k: v for k, v in b.items() if k != "match"})]
    for est, fields in cases:
        h = ctypes.c_void_p(12345)
        want = L.usac_multi_create_device(ctypes.byref(h), 0, est, ctypes.byref(usac._MultiDeviceInput(**fields)))
        assert want in (-1, -3) and want == (-3 if est == LINE else -1)
        assert _create(usac, est, **fields) == want, (est, fields)
        assert _create(usac, est, order=None, **fields) == want, (est, fields)  # the input's refusal goes first


class _Dev:
    """a device array as far as the Python layer looks before it calls the library"""

    def __init__(self, shape, typestr, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (FAKE, False), "version": 3,
                                         "strides": strides}


def test_python_layer_checks_scores(usac, monkeypatch):
    MC = usac.MultiContext
    assert MC.sorted_by_score is False
    monkeypatch.setattr(usac, "lib", lambda: pytest.fail("the library was touched"))
    rows = _Dev((2, 10, 4), "<f4")
    k0, k1, m = _Dev((2, 10, 2), "<f4"), _Dev((2, 7, 2), "<f4"), _Dev((2, 10), "<i4")
    bad_scores = (_Dev((2, 9), "<f4"), _Dev((3, 10), "<f4"), _Dev((20,), "<f4"), _Dev((2, 10, 1), "<f4"),
                  _Dev((2, 10), "<f8"), _Dev((2, 10), "<f2"), _Dev((2, 10), "<i4"), _Dev((2, 10), "<f4", strides=(80, 8)),
                  _Dev((2, 7), "<f4"))  # the last: n1 columns, not n0
    for bad in bad_scores:
        for descending in (True, False):
            with pytest.raises(ValueError):
                MC.from_padded(usac.ESTIMATOR.Homography, rows, scores=bad, descending=descending)
            with pytest.raises(ValueError):
                MC.from_matches(usac.ESTIMATOR.Fundamental, k0, k1, m, scores=bad, descending=descending)
    for host in (np.zeros((2, 10), np.float32), np.zeros((2, 10), np.float32).tolist()):
        with pytest.raises(TypeError):
            MC.from_padded(usac.ESTIMATOR.Homography, rows, scores=host)
        with pytest.raises(TypeError):
            MC.from_matches(usac.ESTIMATOR.Fundamental, k0, k1, m, scores=host)


def test_struct_mirror_matches_the_header(usac):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 26
    S = usac._MultiDeviceOrder
    assert ctypes.sizeof(S) == d["sizeof"]
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == d["offsets"] and len(d["offsets"]) == 2


def _key_cases():
    """(descending, bits, cols): random scores with the edge values and NaNs among them, long tie runs, all NaN"""
    rng = np.random.default_rng(26)
    special = np.concatenate([sref.EDGE_BITS, sref.NAN_BITS])
    out = []
    for c in range(400):
        n = int(rng.integers(1, 200))
        how = c % 5
        if how == 0:    # any bit pattern
            bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        elif how == 1:  # ordinary numbers with the special values sprinkled in, each more than once
            bits = rng.normal(0, 3, size=n).astype(np.float32).view(np.uint32).copy()
            at = rng.random(n) < 0.4
            bits[at] = rng.choice(special, size=int(at.sum()))
        elif how == 2:  # four values only: long tie runs
            bits = rng.choice(np.array([0.25, 0.5, -1.0, 7.0], np.float32).view(np.uint32), size=n)
        elif how == 3:  # the special values alone
            bits = rng.choice(special, size=n)
        else:           # all NaN
            bits = rng.choice(sref.NAN_BITS, size=n)
        cols = np.sort(rng.permutation(5 * n)[:n]).astype(np.uint32)
        if c % 7 == 0:
            cols[-1] = 0xffffffff - 1  # the largest column P * n_max < 2^32 admits
        for descending in (0, 1):
            out.append((descending, bits.astype(np.uint32), cols))
    return out


def test_sort_key_equals_the_written_rule_under_sanitizers(tmp_path):
    cases = _key_cases()
    words = [len(cases)]
    for descending, bits, cols in cases:
        want = sref.order(bits.view(np.float32), cols, bool(descending))
        words += [descending, len(bits)] + bits.tolist() + cols.tolist() + want.tolist()
    path = tmp_path / "cases.u32"
    np.array(words, dtype=np.uint32).tofile(path)
    exe = str(tmp_path / "key_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"), os.path.join(DIR, "key_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok %d" % len(cases)), r.stdout + r.stderr


def test_the_rule_itself_on_a_case_written_out():
    """the helper the other tests trust, on values whose order can be read off"""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    k = np.array([0.5, nan, -0.0, inf, 0.0, -inf, 0.5, -nan], dtype=np.float32)
    cols = np.array([2, 3, 5, 7, 11, 13, 17, 19])
    assert cols[sref.order(k, cols, True)].tolist() == [7, 2, 17, 5, 11, 13, 3, 19]
    assert cols[sref.order(k, cols, False)].tolist() == [13, 5, 11, 2, 17, 7, 3, 19]
