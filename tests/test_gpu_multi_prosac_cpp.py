"""usac_gpu::MultiContext::runProsac (include/usac_gpu.hpp) driven from C++:
tests/cpp_multi_prosac/consumer.cpp compiles with g++ -std=c++11 -Werror against the header (no GPU
needed), and on a GPU its PROSAC run over three quality-sorted problems equals the C call and what the
Python MultiContext returns."""
import json
import os
import subprocess

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.conftest import ROOT

DIR = os.path.join(ROOT, "tests", "cpp_multi_prosac")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_prosac_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 17


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["H", "F"])
def test_cpp_run_prosac_equals_c_and_python(usac, tmp_path, kind):
    _build()
    shapes = ((200, 0.5, 41), (333, 0.3, 42), (1000, 0.3, 24))
    if kind == "H":
        est, m = usac.ESTIMATOR.Homography, 4
        sets = []
        for n, r, s in shapes:
            pts, _, inl = synthetic.homography_points(n=n, inlier_ratio=r, seed=s)
            sets.append(synthetic.quality_sort(pts, inl, s + 1000)[0])
    else:
        est, m = usac.ESTIMATOR.Fundamental, 7
        sets = [synthetic.fundamental_points(n=n, inlier_ratio=r, seed=s, prosac_order=True)[0] for n, r, s in shapes]
    thr, prob, max_iters, R, seed = 2.0, 0.95, 512, 64, 7
    with usac.MultiContext(est, sets) as mc:
        mc.points.tofile(tmp_path / "pts.f32")
        mc.offsets.tofile(tmp_path / "offsets.u32")
        model = usac.Model(thr, m, prob, 5, est, usac.SAMPLER.Prosac)
        model.max_iterations, model.batch, model.seed = max_iters, R, seed
        runs = mc.run_prosac(model)
    args = ["run", int(est), len(sets), "pts.f32", "offsets.u32", thr, prob, max_iters, R, seed]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout)["problems"]
    assert len(out) == len(sets)
    for p, (o, py) in enumerate(zip(out, runs)):
        assert o["cpp"] == o["c"], p
        assert o["cpp"]["model"] == _bits(py["best"]["model"]) and o["cpp"]["inliers"] == py["best"]["inliers"]
        assert o["cpp"]["hyp_index"] == py["best"]["hyp_index"] and o["cpp"]["score"] == _bits(py["best"]["score"])[0]
        for key in ("rounds", "hypotheses", "bound", "status", "termination_length", "largest_sample_size", "clock",
                    "scans"):
            assert o["cpp"][key] == py[key], (p, key)
    assert sum(o["cpp"]["scans"] for o in out) > 0
