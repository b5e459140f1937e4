"""usac_gpu::MultiContext::essential (include/usac_gpu.hpp, ABI 21) driven from C++:
tests/cpp_multi_essential/consumer.cpp compiles with g++ -std=c++11 -Werror against the header (no
GPU needed), and on a GPU its run over two small essential problems prints the records the Python
MultiContext.essential returns, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.conftest import ROOT

DIR = os.path.join(ROOT, "tests", "cpp_multi_essential")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_essential_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 21


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


def _record_bits(d):
    return {"hyp_index": d["hyp_index"], "inliers": d["inliers"], "score": _bits(d["score"])[0],
            "valid": int(d["valid"]), "model": _bits(d["model"])}


@pytest.mark.gpu
def test_cpp_multi_essential_run_equals_python(usac, tmp_path):
    _build()
    sets = [synthetic.fundamental_points(n=200, inlier_ratio=0.5, seed=41, normalized=True, prosac_order=False)[0],
            synthetic.fundamental_points(n=333, inlier_ratio=0.3, seed=42, normalized=True, prosac_order=False)[0]]
    thr, prob, max_iters, R, seed = 0.002, 0.95, 512, 64, 7
    with usac.MultiContext.essential(sets) as mc:
        mc.points.tofile(tmp_path / "pts.f32")
        mc.offsets.tofile(tmp_path / "offsets.u32")
        model = usac.Model(thr, 5, prob, 5, usac.ESTIMATOR.Essential, usac.SAMPLER.Uniform)
        model.max_iterations, model.batch, model.seed = max_iters, R, seed
        first = mc.hypothesize_score(R, [seed, seed + 1], first_hyp=0, thr=thr, per_hypothesis=False)[2]
        runs = mc.run(model)
        inl = mc.inliers(np.stack([r["best"]["model"] for r in runs]), thr)
    args = ["run", 2, "pts.f32", "offsets.u32", thr, prob, max_iters, R, seed]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    assert got["constructor_code"] == -3
    out = got["problems"]
    assert len(out) == 2
    for p in range(2):
        assert out[p]["best"] == _record_bits(runs[p]["best"])
        assert out[p]["first_round"] == _record_bits(first[p])
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert out[p][key] == runs[p][key]
        assert out[p]["n_inliers"] == len(inl[p])
    assert sum(o["best"]["inliers"] for o in out) > 0
