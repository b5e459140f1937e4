"""usac_gpu::MultiContext::runNapsac / gridNeighbors (include/usac_gpu.hpp) driven from C++: tests/
cpp_multi_napsac/consumer.cpp compiles with g++ -std=c++11 -Werror against the header (no GPU needed),
and on a GPU the consumer's NAPSAC run equals the C call and what the Python MultiContext returns."""
import json
import os
import subprocess

import numpy as np
import pytest

from ransac_amd import synthetic

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp_multi_napsac")
BIN = os.path.join(DIR, "build", "consumer")
THR = 2.0
COUNTERS = ("lo_calls", "inner_iters", "iterative_iters", "fits", "improved", "capped", "draws")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_napsac_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


def _sets(kind):
    if kind == "H":
        return [synthetic.homography_points(n=n, inlier_ratio=r, seed=s, cluster=(500, 500, 40))[0]
                for n, r, s in ((65, 0.3, 22), (333, 0.0, 23), (1000, 0.3, 24))]
    return [synthetic.fundamental_points(n=n, inlier_ratio=r, seed=s, prosac_order=False)[0]
            for n, r, s in ((65, 0.3, 32), (333, 0.0, 33), (1000, 0.3, 34))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,cs,lo", [("H", 50, False), ("H", 50, True), ("F", 400, True)])
def test_cpp_run_napsac_equals_c_and_python(usac, tmp_path, kind, cs, lo):
    _build()
    sets = _sets(kind)
    est = usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental
    max_iters, R, seed = 512, 64, 7
    model = usac.Model(THR, 4 if kind == "H" else 7, 0.95, 5, est, usac.SAMPLER.Napsac)
    model.setNeighborsType(usac.NeighborsSearch.Grid)
    model.setCellSize(cs)
    model.max_iterations, model.batch, model.seed = max_iters, R, seed
    if lo:
        model.lo = usac.LocOpt.InItLORsc
        model.setLOParametres(4, 10, 10)
    with usac.MultiContext(est, sets) as mc:
        mc.points.tofile(tmp_path / "pts.f32")
        mc.offsets.tofile(tmp_path / "offsets.u32")
        runs = mc.run_napsac(model)
        grid = mc.grid_neighbors(cs)
    args = ["run", int(est), len(sets), "pts.f32", "offsets.u32", THR, 0.95, max_iters, R, seed, cs, int(model.lo)]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout)["problems"]
    assert len(out) == len(sets)
    for p, (o, py) in enumerate(zip(out, runs)):
        assert o["cpp"] == o["c"], p
        assert o["cpp"]["model"] == _bits(py["best"]["model"]) and o["cpp"]["inliers"] == py["best"]["inliers"]
        assert o["cpp"]["hyp_index"] == py["best"]["hyp_index"] and o["cpp"]["score"] == _bits(py["best"]["score"])[0]
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert o["cpp"][key] == py[key], (p, key)
        assert ("lo" in o["cpp"]) == lo == ("lo" in py)
        if lo:
            for key in COUNTERS:
                assert o["cpp"]["lo"][key] == py["lo"][key], (p, key)
            assert o["cpp"]["lo"]["threshold"] == _bits(py["lo"]["threshold"])[0]
        g = grid[p]
        assert o["cells"] == len(g["start"]) - 1 and o["eligible"] == len(g["eligible"])
        assert o["members_sum"] == int(((np.arange(len(g["members"]), dtype=np.int64) + 1) * g["members"]).sum())
    assert any(o["eligible"] > 0 for o in out) and any(o["eligible"] == 0 for o in out)
