"""usac_gpu::MultiContext::fromDeviceSorted (include/usac_gpu.hpp, ABI 26) driven from C++:
tests/cpp_multi_device_sorted/consumer.cpp is built with hipcc (it allocates the device memory it hands over)
against the header and the in-tree library, and on a GPU its sorted rows, offsets, source columns, PROSAC run,
polish and padded mask equal what the Python MultiContext returns from the same padded rows and scores, bit for
bit.  (The key behind the order, usac_sort_key.hpp, runs under the sanitizers in
tests/test_multi_device_sorted_cpu.py's stand-alone program.)"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

DIR = os.path.join(ROOT, "tests", "cpp_multi_device_sorted")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_device_sorted_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 26


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).reshape(-1).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,descending", [("H", 1), ("F", 0), ("E", 1)])
def test_cpp_sorted_device_input_equals_python(usac, tmp_path, kind, descending):
    from tests import test_gpu_multi_device_sorted as srt
    _build()
    w = srt.World(usac, kind, bool(descending))
    try:
        rows, valid, scores = w.rows, w.valid, w.scores
        P, n_max = valid.shape
        prob, max_iters, R, seed = srt.PROB, srt.MAX_IT, srt.R, 100
        mc = w.mc
        pts, offsets, src = mc.resident_points(), mc.offsets, mc.source_index
        runs = mc.run_prosac(srt._model(usac, kind, usac.SAMPLER.Prosac), polish=True)
        padded = mc.padded_mask().cpu().numpy()
    finally:
        w.close()
    rows.tofile(tmp_path / "rows.f32")
    valid.astype(np.uint8).tofile(tmp_path / "valid.u8")
    scores.tofile(tmp_path / "scores.f32")
    args = ["run", int(srt._est(usac, kind)), P, n_max, "rows.f32", "valid.u8", "scores.f32", descending, srt.THR[kind],
            prob, max_iters, R, seed]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(r.stdout)
    assert doc["n_max"] == n_max
    assert doc["points"] == _bits(pts)
    assert doc["offsets"] == offsets.tolist()
    assert doc["source"] == src.tolist() == np.concatenate(w.cols).tolist()
    assert doc["padded_mask"] == padded.astype(np.uint8).reshape(-1).tolist()
    assert not np.array(doc["padded_mask"], dtype=bool).reshape(P, n_max)[~valid].any()
    out = doc["problems"]
    assert len(out) == P
    for p, (o, py) in enumerate(zip(out, runs)):
        b = py["best"]
        assert o["best"]["model"] == _bits(b["model"]) and o["best"]["score"] == _bits(b["score"])[0], p
        assert (o["best"]["hyp_index"], o["best"]["inliers"], bool(o["best"]["valid"])) == \
            (b["hyp_index"], b["inliers"], bool(b["valid"])), p
        for key in ("rounds", "hypotheses", "bound", "status"):
            assert o[key] == py[key], (p, key)
        for key in ("termination_length", "largest_sample_size", "clock", "scans"):
            assert o["prosac"][key] == py[key], (p, key)
        q, pol = o["polished"], py["polished"]
        assert q["model"] == _bits(pol["model"]) and q["score"] == _bits(pol["score"])[0], p
        assert (q["inliers"], q["passes"], q["status"]) == (pol["inliers"], pol["passes"], pol["status"]), p
    assert max(o["best"]["inliers"] for o in out) > 20
