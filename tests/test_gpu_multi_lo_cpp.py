"""usac_gpu::MultiContext::runLo / lo (include/usac_gpu.hpp) driven from C++: tests/cpp_multi_lo/
consumer.cpp compiles with g++ -std=c++11 -Werror against the header (no GPU needed); its host-only
part and the host text of the LO draw run under the address and undefined-behaviour sanitizers in a
stand-alone program (no GPU, no library); and on a GPU the consumer's LO run equals the C call and
what the Python MultiContext returns."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import multi_lo_ref as ref

DIR = os.path.join(ROOT, "tests", "cpp_multi_lo")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_lo_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 18


def test_lo_draw_host_text_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lo_draw_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "ransac_amd", "csrc"), os.path.join(DIR, "lo_draw_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe, str(tmp_path / "scratch.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,sampler,limited", [("H", "uniform", False), ("H", "prosac", True), ("F", "prosac", False),
                                                   ("F", "uniform", True)])
def test_cpp_run_lo_equals_c_and_python(usac, tmp_path, kind, sampler, limited):
    _build()
    sets = ref.run_sets(kind)
    est = usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental
    smp = usac.SAMPLER.Prosac if sampler == "prosac" else usac.SAMPLER.Uniform
    max_iters, R, seed = 512, 64, 7
    model = ref.make_model(usac, kind, limited, sampler=smp)
    model.max_iterations, model.batch, model.seed = max_iters, R, seed
    with usac.MultiContext(est, sets) as mc:
        mc.points.tofile(tmp_path / "pts.f32")
        mc.offsets.tofile(tmp_path / "offsets.u32")
        runs = mc.run_lo(model)
        hook_recs, hook_st = mc.lo(model, [r["best"] for r in runs])
    args = ["run", int(est), len(sets), "pts.f32", "offsets.u32", ref.THR, 0.95, max_iters, R, seed, int(smp), int(model.lo)]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout)["problems"]
    assert len(out) == len(sets)
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
