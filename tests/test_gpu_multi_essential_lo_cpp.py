"""usac_gpu::MultiContext::runLoEssential / loEssential (include/usac_gpu.hpp, ABI 23) driven from C++:
tests/cpp_multi_essential_lo/consumer.cpp compiles with g++ -std=c++11 -Werror against the header (no GPU
needed), and on a GPU the consumer's LO run equals the C call and what the Python MultiContext returns.
(The consumer's host-only part is tests/cpp_multi_lo/consumer_host.hpp, which tests/test_gpu_multi_lo_cpp.py
runs under the sanitizers in a stand-alone program.)"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import multi_essential_lo_ref as eref
from tests.helpers import multi_lo_ref as ref

DIR = os.path.join(ROOT, "tests", "cpp_multi_essential_lo")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_essential_lo_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("sampler,limited", [("uniform", False), ("prosac", True)])
def test_cpp_run_lo_essential_equals_c_and_python(usac, tmp_path, sampler, limited):
    _build()
    sets = eref.run_sets()
    smp = usac.SAMPLER.Prosac if sampler == "prosac" else usac.SAMPLER.Uniform
    max_iters, R, seed = 1024, 64, 100
    model = eref.make_model(usac, limited, sampler=smp)
    model.max_iterations, model.batch, model.seed = max_iters, R, seed
    with usac.MultiContext.essential(sets) as mc:
        mc.points.tofile(tmp_path / "pts.f32")
        mc.offsets.tofile(tmp_path / "offsets.u32")
        runs = mc.run_lo_essential(model)
        hook_recs, hook_st = mc.lo_essential(model, [r["best"] for r in runs])
    args = ["run", len(sets), "pts.f32", "offsets.u32", eref.THR, 0.95, max_iters, R, seed, int(smp), int(model.lo)]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(r.stdout)
    out = doc["problems"]
    assert len(out) == len(sets)
    assert doc["run_lo_code"] == doc["lo_code"] == -3  # runLo() and lo() keep refusing the context
    keys = ["rounds", "hypotheses", "bound", "status"]
    if sampler == "prosac":
        keys += ["termination_length", "largest_sample_size", "clock", "scans"]
    for p, (o, py) in enumerate(zip(out, runs)):
        assert o["cpp"] == o["c"], p
        assert o["cpp"]["model"] == _bits(py["best"]["model"]) and o["cpp"]["inliers"] == py["best"]["inliers"]
        assert o["cpp"]["hyp_index"] == py["best"]["hyp_index"] and o["cpp"]["score"] == _bits(py["best"]["score"])[0]
        for key in keys:
            assert o["cpp"][key] == py[key], (p, key)
        assert ("scans" in o["cpp"]) == (sampler == "prosac")
        for blk, lo, rec in ((o["cpp"], py["lo"], None), (o["hook"], hook_st[p], hook_recs[p])):
            for key in ref.COUNTERS:
                assert blk["lo"][key] == lo[key], (p, key)
            assert blk["lo"]["threshold"] == _bits(lo["threshold"])[0]
            if rec is not None:
                assert blk["model"] == _bits(rec["model"]) and blk["inliers"] == rec["inliers"]
    assert sum(o["cpp"]["lo"]["improved"] for o in out) > 0
