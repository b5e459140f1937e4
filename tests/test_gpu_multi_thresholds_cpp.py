"""usac_gpu::MultiContext::set_thresholds (include/usac_gpu.hpp, ABI 22) driven from C++:
tests/cpp_multi_thresholds/consumer.cpp runs two problems under two thresholds -- homography with
runLo, essential with run and the polish -- and prints the records the Python MultiContext returns
under the same thresholds, bit for bit.  The model's own threshold differs on the two sides: neither
may read it."""
import json
import os
import subprocess

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.conftest import ROOT

DIR = os.path.join(ROOT, "tests", "cpp_multi_thresholds")
BIN = os.path.join(DIR, "build", "consumer")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


def _record_bits(d):
    return {"hyp_index": d["hyp_index"], "inliers": d["inliers"], "score": _bits(d["score"])[0],
            "valid": int(d["valid"]), "model": _bits(d["model"])}


def _consumer(tmp_path, mc, est, thr, scalar, prob, max_iters, R, seed):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    mc.points.tofile(tmp_path / "pts.f32")
    mc.offsets.tofile(tmp_path / "offsets.u32")
    np.asarray(thr, dtype=np.float32).tofile(tmp_path / "thr.f32")
    args = ["run", int(est), mc.P, "pts.f32", "offsets.u32", "thr.f32", scalar, prob, max_iters, R, seed]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    assert got["thresholds"] == _bits(thr)
    assert got["cleared"] is True and got["bad_length_code"] == -1
    return got["problems"]


@pytest.mark.gpu
def test_cpp_homography_run_lo_under_thresholds_equals_python(usac, tmp_path):
    sets = [synthetic.homography_points(n=333, inlier_ratio=0.5, seed=51)[0],
            synthetic.homography_points(n=200, inlier_ratio=0.4, seed=52)[0]]
    thr, prob, max_iters, R, seed = [0.75, 3.5], 0.95, 512, 64, 7
    with usac.MultiContext(usac.ESTIMATOR.Homography, sets) as mc:
        model = usac.Model(9.0, 4, prob, 5, usac.ESTIMATOR.Homography, usac.SAMPLER.Uniform)
        model.max_iterations, model.batch, model.seed = max_iters, R, seed
        model.lo = usac.LocOpt.InItLORsc
        model.lo_inner_iterations = 10
        mc.set_thresholds(thr)
        runs = mc.run_lo(model)
        out = _consumer(tmp_path, mc, usac.ESTIMATOR.Homography, thr, 1.25, prob, max_iters, R, seed)
    assert len(out) == 2
    for p in range(2):
        assert out[p]["best"] == _record_bits(runs[p]["best"])
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert out[p][key] == runs[p][key]
        assert out[p]["lo_calls"] == runs[p]["lo"]["lo_calls"] and out[p]["fits"] == runs[p]["lo"]["fits"]
        assert out[p]["lo_threshold"] == _bits(runs[p]["lo"]["threshold"])[0]
    assert sum(o["best"]["inliers"] for o in out) > 0 and sum(o["lo_calls"] for o in out) > 0


@pytest.mark.gpu
def test_cpp_essential_run_and_polish_under_thresholds_equal_python(usac, tmp_path):
    sets = [synthetic.fundamental_points(n=200, inlier_ratio=0.5, seed=41, normalized=True, prosac_order=False)[0],
            synthetic.fundamental_points(n=333, inlier_ratio=0.3, seed=42, normalized=True, prosac_order=False)[0]]
    thr, prob, max_iters, R, seed = [0.0008, 0.003], 0.95, 512, 64, 7
    with usac.MultiContext.essential(sets) as mc:
        model = usac.Model(0.5, 5, prob, 5, usac.ESTIMATOR.Essential, usac.SAMPLER.Uniform)
        model.max_iterations, model.batch, model.seed = max_iters, R, seed
        mc.set_thresholds(thr)
        runs = mc.run(model)
        pol = mc.polish(np.stack([r["best"]["model"] for r in runs]), 0.5, with_inliers=True)
        out = _consumer(tmp_path, mc, usac.ESTIMATOR.Essential, thr, 0.01, prob, max_iters, R, seed)
    assert len(out) == 2
    for p in range(2):
        assert out[p]["best"] == _record_bits(runs[p]["best"])
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert out[p][key] == runs[p][key]
        q = out[p]["polished"]
        assert q["model"] == _bits(pol[p]["model"]) and q["score"] == _bits(pol[p]["score"])[0]
        assert (q["inliers"], q["passes"], q["status"]) == (pol[p]["inliers"], pol[p]["passes"], pol[p]["status"])
        assert q["n_mask"] == len(pol[p]["inlier_idx"])
    assert sum(o["best"]["inliers"] for o in out) > 0
