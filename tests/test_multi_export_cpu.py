"""Device output of multi contexts (usac_multi_export_device, usac_multi_set_resident; ABI 27), the part that
needs no GPU: the symbols, the refusals of a NULL context, the layout of usac_multi_device_output as the C++
consumer sees it, the host-and-device text of usac_pixels.hpp and the extent rule under the sanitizers in a
stand-alone program, and the numpy reference of the GPU tests against loops written out by hand."""
import ctypes
import json
import os
import subprocess

import numpy as np

from tests.conftest import ROOT
from tests.helpers import multi_export_ref as xref

DIR = os.path.join(ROOT, "tests", "cpp_multi_export")
BIN = os.path.join(DIR, "build", "consumer")
FAKE = 0x7f0000001000  # an aligned address nothing dereferences: every case below returns before it could


def test_abi_version_and_symbols(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 27
    for name in ("usac_multi_export_device", "usac_multi_set_resident"):
        assert name in usac.ABI_SYMBOLS
        assert hasattr(L, name)
    assert usac.MultiContext.keep_on_device.fset is not None and callable(usac.MultiContext.export_device)


def test_null_contexts_are_refused(usac):
    L = usac.lib()
    o = usac._MultiDeviceOutput(n_max=10, k_max=0, mask=FAKE)
    assert L.usac_multi_export_device(None, ctypes.byref(o)) == -1
    assert L.usac_multi_export_device(None, None) == -1
    assert L.usac_multi_set_resident(None, 1) == -1
    assert L.usac_multi_set_resident(None, 0) == -1


def test_struct_mirror_matches_the_header(usac):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 27
    S = usac._MultiDeviceOutput
    assert ctypes.sizeof(S) == d["sizeof"]
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == d["offsets"]


def test_host_and_device_text_under_sanitizers(tmp_path):
    """usac_pixels.hpp as g++ compiles it (the device compiles the same text) against long double, and the extent
    rule at its edges"""
    exe = str(tmp_path / "export_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"), os.path.join(DIR, "export_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok 400"), r.stdout + r.stderr


def test_the_pixels_check_still_compiles_the_header():
    """tests/cpp_multi_pixels/pixels_check.cpp includes usac_pixels.hpp under g++: the host-and-device marks are
    nothing to it"""
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp_multi_pixels", "pixels_check.cpp")], check=True)


def test_reference_against_loops_by_hand():
    rng = np.random.default_rng(9)
    sizes = [4, 7, 1, 12]
    offsets = np.zeros(5, dtype=np.uint32)
    offsets[1:] = np.cumsum(sizes)
    mask = (rng.random(int(offsets[-1])) < 0.6).astype(np.uint8)
    mask[offsets[2]] = 0  # a problem without inliers: a zero row and a row of -1
    n_max = 15
    source = np.concatenate([rng.permutation(n_max)[:n] for n in sizes]).astype(np.uint32)  # no order: a sorted context
    for src, width in ((source, n_max), (None, 12), (None, 14)):
        for k in (1, 3, 12):
            want_mask, want_cols = xref.by_hand(mask, offsets, src, width, k)
            got_mask, got_cols = xref.padded_mask(mask, offsets, src, width), xref.inlier_cols(mask, offsets, src, k)
            assert got_mask.dtype == np.uint8 and got_cols.dtype == np.int32
            np.testing.assert_array_equal(got_mask, want_mask)
            np.testing.assert_array_equal(got_cols, want_cols)
    cols = xref.inlier_cols(mask, offsets, source, 12)
    assert (cols[2] == -1).all() and not xref.padded_mask(mask, offsets, source, n_max)[2].any()
    # one case written out in full: two problems of three rows, columns 5 1 3 and 0 2 4, the mask 1 0 1 | 0 1 1
    m = np.array([1, 0, 1, 0, 1, 1], dtype=np.uint8)
    o = np.array([0, 3, 6], dtype=np.uint32)
    s = np.array([5, 1, 3, 0, 2, 4], dtype=np.uint32)
    np.testing.assert_array_equal(xref.padded_mask(m, o, s, 6), [[0, 0, 0, 1, 0, 1], [0, 0, 1, 0, 1, 0]])
    np.testing.assert_array_equal(xref.inlier_cols(m, o, s, 3), [[5, 3, -1], [2, 4, -1]])
    np.testing.assert_array_equal(xref.inlier_cols(m, o, s, 1), [[5], [2]])
    np.testing.assert_array_equal(xref.inlier_cols(m, o, None, 2), [[0, 2], [1, 2]])
