"""NAPSAC for multi-problem batches (usac_multi_grid, usac_multi_draw_samples_napsac,
usac_multi_hypothesize_score_napsac, usac_multi_run_napsac; ABI 20), the parts that need no device: the
version, the exported symbols, the bindings' argument lists against the header's declarations, the
structures the run fills, and the NULL-context refusals."""
import ctypes
import os
import re

from tests.conftest import ROOT

ERR_ARG = -1
NEW = ["usac_multi_grid", "usac_multi_draw_samples_napsac", "usac_multi_hypothesize_score_napsac",
       "usac_multi_run_napsac"]


def _declared_args(name):
    """the parameter list of `name` in include/usac_gpu.h, one C type per parameter (names dropped)"""
    hdr = open(os.path.join(ROOT, "include", "usac_gpu.h")).read()
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, hdr, re.S)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = re.sub(r"/\*.*?\*/", "", " ".join(arg.split()))
        out.append(re.sub(r"\s*\w+$", "", arg).replace(" *", "*").replace("const ", ""))
    return out


def test_abi_version_and_symbols(usac):
    L = usac.lib()
    assert L.usac_abi_version() >= 20
    assert set(NEW) <= set(usac.ABI_SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name


def test_argument_lists_match_the_header(usac):
    L = usac.lib()
    P = ctypes.POINTER
    ctype = {"usac_multi*": ctypes.c_void_p, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
             "float": ctypes.c_float, "uint32_t*": P(ctypes.c_uint32), "int32_t*": P(ctypes.c_int32),
             "uint64_t*": P(ctypes.c_uint64), "float*": P(ctypes.c_float), "uint8_t*": P(ctypes.c_uint8),
             "usac_record*": P(usac.Record), "usac_params*": P(usac._Params), "usac_multi_output*": P(usac._MultiOutput),
             "usac_multi_lo_output*": P(usac._MultiLoOutput), "usac_multi_polish_output*": P(usac._MultiPolishOutput)}
    for name in NEW:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int, name
        assert list(fn.argtypes) == [ctype[t] for t in _declared_args(name)], (name, _declared_args(name))
    # the run takes usac_multi_run_lo's arguments without PROSAC's array
    assert len(L.usac_multi_run_napsac.argtypes) == len(L.usac_multi_run_lo.argtypes) - 1
    # the round hook: usac_multi_hypothesize_score's arguments without samples, plus cell_size
    assert len(L.usac_multi_hypothesize_score_napsac.argtypes) == len(L.usac_multi_hypothesize_score.argtypes)
    # the grid call: usac_grid_neighbors' arguments, the two counts as arrays
    assert list(L.usac_multi_grid.argtypes)[1:] == list(L.usac_grid_neighbors.argtypes)[1:]


def test_structures_the_run_fills(usac):
    assert ctypes.sizeof(usac._MultiOutput) == ctypes.sizeof(usac.Record) + 16
    assert ctypes.sizeof(usac._MultiLoOutput) == 32 and usac._MultiLoOutput.threshold.offset == 28
    assert usac._Params.cell_size.offset == 52 and usac._Params.neighbors.offset == 56
    assert int(usac.SAMPLER.Napsac) == 3 and int(usac.NeighborsSearch.Grid) == 2


def test_null_context_is_refused(usac):
    L = usac.lib()
    prm = usac._params(usac.Model(2.0, 4, 0.95, 5, usac.ESTIMATOR.Homography, usac.SAMPLER.Napsac))
    out = (usac._MultiOutput * 1)()
    seeds = (ctypes.c_uint64 * 1)(1)
    buf = (ctypes.c_int32 * 256)()
    assert L.usac_multi_grid(None, 50, None, None, None, None, None, None, None) == ERR_ARG
    assert L.usac_multi_draw_samples_napsac(None, None, 1, 64, seeds, 0, 50, buf) == ERR_ARG
    assert L.usac_multi_hypothesize_score_napsac(None, None, 1, 64, seeds, 0, 2.0, 0, 50, None, None, None) == ERR_ARG
    assert L.usac_multi_run_napsac(None, ctypes.byref(prm), None, out, None, None, None) == ERR_ARG
