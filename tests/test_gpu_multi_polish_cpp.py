"""usac_gpu::MultiContext::runPolished / polish (include/usac_gpu.hpp) driven from C++:
tests/cpp_multi_polish/consumer_multi_polish.cpp compiles with g++ -std=c++11 -Werror against the
header (no GPU needed), and on a GPU its polished run over three small problems prints what the
Python MultiContext returns."""
import json
import os
import subprocess

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.conftest import ROOT

DIR = os.path.join(ROOT, "tests", "cpp_multi_polish")
BIN = os.path.join(DIR, "build", "consumer_multi_polish")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_polish_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 16


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


def _polished_bits(d):
    return {"inliers": d["inliers"], "score": _bits(d["score"])[0], "minimal_inliers": d["minimal_inliers"],
            "minimal_score": _bits(d["minimal_score"])[0], "passes": d["passes"], "status": d["status"],
            "model": _bits(d["model"])}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["H", "F"])
def test_cpp_run_polished_equals_python(usac, tmp_path, kind):
    _build()
    if kind == "H":
        est, m = usac.ESTIMATOR.Homography, 4
        sets = [synthetic.homography_points(n=n, inlier_ratio=r, seed=s)[0]
                for n, r, s in ((200, 0.5, 41), (333, 0.3, 42), (1000, 0.3, 24))]
    else:
        est, m = usac.ESTIMATOR.Fundamental, 7
        sets = [synthetic.fundamental_points(n=n, inlier_ratio=r, seed=s, prosac_order=False)[0]
                for n, r, s in ((200, 0.5, 41), (333, 0.3, 42), (1000, 0.3, 34))]
    thr, prob, max_iters, R, seed = 2.0, 0.95, 512, 64, 7
    with usac.MultiContext(est, sets) as mc:
        mc.points.tofile(tmp_path / "pts.f32")
        mc.offsets.tofile(tmp_path / "offsets.u32")
        model = usac.Model(thr, m, prob, 5, est, usac.SAMPLER.Uniform)
        model.max_iterations, model.batch, model.seed = max_iters, R, seed
        runs = mc.run(model, polish=True)
    args = ["run", int(est), len(sets), "pts.f32", "offsets.u32", thr, prob, max_iters, R, seed]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout)["problems"]
    assert len(out) == len(sets)
    for p, (o, py) in enumerate(zip(out, runs)):
        assert o["best"]["model"] == _bits(py["best"]["model"]) and o["best"]["inliers"] == py["best"]["inliers"]
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert o[key] == py[key], (p, key)
        assert o["polished"] == _polished_bits(py["polished"]), p
        assert o["polish_again"] == o["polished"], p
        assert o["inliers"] == py["inliers"].tolist() == o["inliers_again"], p
    assert sum(o["polished"]["passes"] for o in out) > 0
