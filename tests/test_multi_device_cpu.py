"""Device input of multi contexts (usac_multi_create_device, usac_multi_get_offsets, usac_multi_get_source,
usac_multi_padded_mask; ABI 25), the part that needs no GPU: the symbols, every refusal that comes before any
device call, the Python layer's own checks, the layout of usac_multi_device_input as the C++ consumer sees it,
and the host text between the two pack kernels (ransac_amd/csrc/usac_pack.hpp) under the sanitizers in a
stand-alone program."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

DIR = os.path.join(ROOT, "tests", "cpp_multi_device")
BIN = os.path.join(DIR, "build", "consumer")
H, F, E, LINE = 2, 3, 4, 1
FAKE = 0x7f0000001000  # a 16-byte-aligned address nothing dereferences: every case below returns before it could


def test_abi_version_and_symbols(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 25
    for name in ("usac_multi_create_device", "usac_multi_get_source", "usac_multi_padded_mask", "usac_multi_get_offsets"):
        assert name in usac.ABI_SYMBOLS
        assert hasattr(L, name)


def _create(usac, estimator, **fields):
    h = ctypes.c_void_p(12345)
    inp = usac._MultiDeviceInput(**fields)
    rc = usac.lib().usac_multi_create_device(ctypes.byref(h), 0, estimator, ctypes.byref(inp))
    assert h.value is None, "a refused creation left *out set"
    return rc


def _k(P, **change):
    k = np.tile(np.array([1000, 0, 500, 0, 1000, 500, 0, 0, 1], dtype=np.float32), (P, 1))
    for at, v in change.items():
        k[P - 1, int(at[1:])] = v
    return k


def _kp(k):
    return k.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def test_create_argument_errors_come_before_any_device_call(usac):
    """each case returns its code on a machine without a GPU: a device call would have returned -2 there"""
    L = usac.lib()
    a = dict(P=2, n_max=10, rows=FAKE)                               # form a
    b = dict(P=2, n_max=10, kpts0=FAKE, kpts1=FAKE, n1=7, match=FAKE)  # form b
    h = ctypes.c_void_p(12345)
    assert L.usac_multi_create_device(None, 0, H, ctypes.byref(usac._MultiDeviceInput(**a))) == -1
    assert L.usac_multi_create_device(ctypes.byref(h), 0, H, None) == -1 and h.value is None
    assert _create(usac, LINE, **a) == -3
    assert _create(usac, H, **dict(a, P=0)) == -1
    assert _create(usac, H, **dict(a, P=65536)) == -1
    assert _create(usac, H, **dict(a, n_max=0)) == -1
    assert _create(usac, H, **dict(a, P=65535, n_max=65538)) == -1      # P * n_max >= 2^32
    assert _create(usac, H, P=2, n_max=10) == -1                        # neither form
    assert _create(usac, H, **dict(a, **{k: v for k, v in b.items() if k not in a})) == -1  # both forms
    assert _create(usac, H, **dict(a, valid=FAKE, counts=FAKE)) == -1
    assert _create(usac, H, **dict(b, n1=0)) == -1
    for missing in ("kpts0", "kpts1", "match"):
        assert _create(usac, F, **{k: v for k, v in b.items() if k != missing}) == -1, missing
    good = _k(2)
    for est in (H, F):
        assert _create(usac, est, **dict(a, K1=_kp(good))) == -1        # K with a non-essential estimator
        assert _create(usac, est, **dict(a, K1=_kp(good), K2=_kp(good))) == -1
    assert _create(usac, E, **dict(a, K2=_kp(good))) == -1              # K2 without K1
    for change in (dict(k0=0.0), dict(k4=-1.0), dict(k3=1e-3), dict(k6=1.0), dict(k7=1.0), dict(k8=2.0),
                   dict(k2=np.nan), dict(k1=np.inf)):
        bad = _k(2, **change)
        assert _create(usac, E, **dict(a, K1=_kp(bad))) == -1, change
        assert _create(usac, E, **dict(b, K1=_kp(good), K2=_kp(bad))) == -1, change
    msg = L.usac_multi_last_error(None)
    assert b"usac_multi_create_device" in msg and b"problem 1" in msg   # the last case: the bad K is problem 1's


def test_null_handles_are_refused(usac):
    L = usac.lib()
    buf = np.zeros(4, dtype=np.uint32)
    mask = np.zeros(4, dtype=np.uint8)
    assert L.usac_multi_get_source(None, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == -1
    assert L.usac_multi_get_offsets(None, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == -1
    assert L.usac_multi_padded_mask(None, mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), FAKE, None) == -1


class _Dev:
    """a device array as far as the Python layer looks before it calls the library"""

    def __init__(self, shape, typestr, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (FAKE, False), "version": 3,
                                         "strides": strides}


def test_python_layer_refuses_host_arrays_and_wrong_layouts(usac, monkeypatch):
    MC = usac.MultiContext
    monkeypatch.setattr(usac, "lib", lambda: pytest.fail("the library was touched"))
    rows, valid = np.zeros((2, 10, 4), np.float32), np.ones((2, 10), np.uint8)
    with pytest.raises(TypeError):
        MC.from_padded(usac.ESTIMATOR.Homography, rows, valid)
    with pytest.raises(TypeError):
        MC.from_padded(usac.ESTIMATOR.Homography, _Dev((2, 10, 4), "<f4"), valid)
    with pytest.raises(TypeError):
        MC.from_padded(usac.ESTIMATOR.Homography, rows.tolist())
    with pytest.raises(TypeError):
        MC.from_matches(usac.ESTIMATOR.Fundamental, np.zeros((2, 10, 2), np.float32), np.zeros((2, 7, 2), np.float32),
                        np.zeros((2, 10), np.int32))
    try:
        import torch
    except ImportError:
        torch = None
    if torch is not None:
        with pytest.raises(TypeError):
            MC.from_padded(usac.ESTIMATOR.Homography, torch.zeros((2, 10, 4)))  # a host tensor
    ok = _Dev((2, 10, 4), "<f4")
    for bad_rows in (_Dev((2, 10, 3), "<f4"), _Dev((20, 4), "<f4"), _Dev((2, 10, 4), "<f8"),
                     _Dev((2, 10, 4), "<f4", strides=(320, 32, 4))):
        with pytest.raises(ValueError):
            MC.from_padded(usac.ESTIMATOR.Homography, bad_rows)
    for bad_valid in (_Dev((2, 9), "|u1"), _Dev((2, 10), "<i4"), _Dev((2, 10, 1), "|b1")):
        with pytest.raises(ValueError):
            MC.from_padded(usac.ESTIMATOR.Homography, ok, valid=bad_valid)
    for bad_counts in (_Dev((3,), "<i4"), _Dev((2,), "<i8"), _Dev((2, 1), "<i4")):
        with pytest.raises(ValueError):
            MC.from_padded(usac.ESTIMATOR.Homography, ok, counts=bad_counts)
    with pytest.raises(ValueError):
        MC.from_padded(usac.ESTIMATOR.Homography, ok, valid=_Dev((2, 10), "|b1"), counts=_Dev((2,), "<i4"))
    k0, k1, m = _Dev((2, 10, 2), "<f4"), _Dev((2, 7, 2), "<f4"), _Dev((2, 10), "<i4")
    for args in ((_Dev((2, 10, 4), "<f4"), k1, m), (k0, _Dev((3, 7, 2), "<f4"), m), (k0, k1, _Dev((2, 7), "<i4")),
                 (k0, k1, _Dev((2, 10), "<f4")), (k0, k1, _Dev((2, 10), "<i8"))):  # int64 is cast for tensors alone
        with pytest.raises(ValueError):
            MC.from_matches(usac.ESTIMATOR.Fundamental, *args)


def test_existing_constructors_keep_their_inlier_lists(usac):
    assert usac.MultiContext.inlier_lists is True and usac.MultiContext.n_max is None


def test_struct_mirror_matches_the_header(usac):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 25
    S = usac._MultiDeviceInput
    assert ctypes.sizeof(S) == d["sizeof"]
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == d["offsets"]


def _case(P, m, n_max, sizes, flags, status, bad):
    off = np.zeros(P + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(sizes, dtype=np.uint64))
    return [P, m, n_max, status, bad] + list(sizes) + list(flags) + (off % (1 << 32)).astype(np.uint64).tolist()


def test_host_text_under_sanitizers(tmp_path):
    """the sizes-to-offsets sum, the smallest-problem check, the overflow check and the first-bad-problem report of
    usac_pack.hpp, on vectors of exactly P and P + 1 values"""
    OK, BAD_COUNT, BAD_MATCH, TOO_FEW, OVERFLOW = 0, 1, 2, 3, 4
    big = 0xffffffff
    cases = [
        _case(6, 4, 300, [4, 64, 65, 256, 257, 300], [0] * 6, OK, 6),
        _case(1, 7, 7, [7], [0], OK, 1),
        _case(3, 5, 10, [5, 4, 3], [0, 0, 0], TOO_FEW, 1),            # the first of two short problems
        _case(3, 4, 10, [4, 0, 9], [0, 1, 2], BAD_COUNT, 1),          # a flag goes before the size it spoiled
        _case(3, 4, 10, [9, 9, 0], [0, 0, 2], BAD_MATCH, 2),
        _case(2, 4, 10, [3, 9], [2, 1], BAD_MATCH, 0),
        _case(2, 4, 10, [11, 9], [0, 0], BAD_COUNT, 0),               # a size no count of n_max columns is
        _case(2, 4, big, [big, 4], [0, 0], OVERFLOW, 1),              # the sum reaches 2^32
        _case(3, 4, big, [1 << 31, (1 << 31) - 1, 4], [0, 0, 0], OVERFLOW, 2),
        _case(2, 4, big, [1 << 31, (1 << 31) - 1], [0, 0], OK, 2),    # 2^32 - 1 rows: the largest total
    ]
    blob = np.array([len(cases)] + [w for c in cases for w in c], dtype=np.uint32)
    path = tmp_path / "cases.u32"
    blob.tofile(path)
    exe = str(tmp_path / "pack_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"), os.path.join(DIR, "pack_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok %d" % len(cases)), r.stdout + r.stderr


def test_other_consumers_still_compile_against_the_header():
    """the g++ consumers include the changed usac_gpu.hpp under -std=c++11 -Wall -Wextra -Werror"""
    for d in ("cpp_multi_pixels", "cpp_multi", "cpp_multi_essential_lo"):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", d)], check=True)
