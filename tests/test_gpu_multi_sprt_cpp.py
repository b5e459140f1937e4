"""usac_gpu::MultiContext::runSprt (include/usac_gpu.hpp) driven from C++ on a GPU: the run of
tests/cpp_multi_sprt/consumer.cpp equals the C call and what the Python MultiContext returns.  (Its `abi`
mode and the host-only sanitizer program run without a GPU: tests/test_multi_sprt_cpu.py.)"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import multi_sprt_ref as ref

pytestmark = pytest.mark.gpu

DIR = os.path.join(ROOT, "tests", "cpp_multi_sprt")
BIN = os.path.join(DIR, "build", "consumer")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


@pytest.mark.parametrize("kind,sampler", [("H", "uniform"), ("H", "prosac"), ("F", "prosac"), ("F", "uniform")])
def test_cpp_run_sprt_equals_c_and_python(usac, tmp_path, kind, sampler):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    sets, _ = ref.sets(kind, sort=True, with_m=False)
    est = usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental
    smp = usac.SAMPLER.Prosac if sampler == "prosac" else usac.SAMPLER.Uniform
    max_iters, R, seed = 512, 64, 7
    model = usac.Model(ref.THR, ref.M[kind], 0.95, 5, est, smp)
    model.max_iterations, model.batch, model.seed = max_iters, R, seed
    model.setSprt(True)
    with usac.MultiContext(est, sets) as mc:
        mc.points.tofile(tmp_path / "pts.f32")
        mc.offsets.tofile(tmp_path / "offsets.u32")
        runs = mc.run_sprt(model)
    args = ["run", int(est), len(sets), "pts.f32", "offsets.u32", ref.THR, 0.95, max_iters, R, seed, int(smp)]
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
        sp = py["sprt"]
        assert [o["cpp"]["sprt"][k] for k in ("epsilon", "delta", "A")] == ref.bits64([sp["epsilon"], sp["delta"], sp["A"]])
        for key in ("tests", "accepted", "rejected", "points_tested"):
            assert o["cpp"]["sprt"][key] == sp[key], (p, key)
    assert sum(o["cpp"]["sprt"]["accepted"] for o in out) > 0
