"""usac_gpu::MultiContext::essentialPixels / setPixelThresholds / pixelModels / points (include/usac_gpu.hpp,
ABI 24) driven from C++: tests/cpp_multi_pixels/consumer.cpp compiles with g++ -std=c++11 -Werror against the
header (no GPU needed), and on a GPU its calibrated rows, thresholds, polished run and pixel-space models equal
what the Python MultiContext returns, bit for bit.  (The host text behind the entries, usac_pixels.hpp, runs
under the sanitizers in tests/test_multi_pixels_cpu.py's stand-alone program.)"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import multi_pixels_ref as ref

DIR = os.path.join(ROOT, "tests", "cpp_multi_pixels")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_pixels_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 24


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


@pytest.mark.gpu
# tolerances of tens of pixels: see TOLS in tests/test_gpu_multi_pixels.py
@pytest.mark.parametrize("two_k,tols", [(True, [30.0, 35.0, 40.0, 45.0, 50.0, 55.0]), (False, [45.0])],
                         ids=["K1_K2_six_tolerances", "K1_one_tolerance"])
def test_cpp_pixels_equal_python(usac, tmp_path, two_k, tols):
    _build()
    K1, K2 = ref.intrinsics()
    if not two_k:
        K2 = None
    sets = ref.pixel_sets(ref.SIZES, K1, K2)
    P, prob, max_iters, R, seed = len(sets), 0.95, 256, 64, 100
    with usac.MultiContext.essential_pixels(sets, K1, K2) as mc:
        rows, offsets = mc.points, mc.offsets
        mc.set_pixel_thresholds(tols)
        thr = mc.thresholds
        model = usac.Model(1.0, 5, prob, 5, usac.ESTIMATOR.Essential, usac.SAMPLER.Uniform)
        model.max_iterations, model.batch, model.seed = max_iters, R, seed
        runs = mc.run(model, polish=True)
        F = mc.pixel_models(np.stack([r["polished"]["model"] for r in runs]))
    np.concatenate(sets, axis=0).astype(np.float32).tofile(tmp_path / "px.f32")
    offsets.tofile(tmp_path / "offsets.u32")
    K1.astype(np.float32).tofile(tmp_path / "K1.f32")
    if two_k:
        K2.astype(np.float32).tofile(tmp_path / "K2.f32")
    np.asarray(tols, dtype=np.float32).tofile(tmp_path / "t.f32")
    args = ["run", P, "px.f32", "offsets.u32", "K1.f32", "K2.f32" if two_k else "-", "t.f32", len(tols), prob, max_iters,
            R, seed]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(r.stdout)
    assert doc["points"] == _bits(rows)
    assert doc["thresholds"] == _bits(thr)
    assert (doc["bad_tolerance_code"], doc["plain_set_code"], doc["plain_models_code"]) == (-1, -3, -3)
    out = doc["problems"]
    assert len(out) == P
    for p, (o, py) in enumerate(zip(out, runs)):
        b = py["best"]
        assert o["best"]["model"] == _bits(b["model"]) and o["best"]["score"] == _bits(b["score"])[0], p
        assert (o["best"]["hyp_index"], o["best"]["inliers"], bool(o["best"]["valid"])) == \
            (b["hyp_index"], b["inliers"], bool(b["valid"])), p
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert o[key] == py[key], (p, key)
        q, pol = o["polished"], py["polished"]
        assert q["model"] == _bits(pol["model"]) and q["score"] == _bits(pol["score"])[0], p
        assert (q["inliers"], q["passes"], q["status"]) == (pol["inliers"], pol["passes"], pol["status"]), p
        assert q["n_mask"] == len(py["inliers"]), p
        assert o["pixel_model"] == _bits(F[p]), p
    assert max(o["best"]["inliers"] for o in out) > 20
