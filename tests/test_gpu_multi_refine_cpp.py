"""usac_gpu::MultiContext::refinePoseDevice / refinePose (include/usac_gpu.hpp, ABI 29) driven from C++:
tests/cpp_multi_refine/consumer.cpp is built with hipcc (it allocates the device memory it hands over) against the
header and the in-tree library, and on a GPU what its calls wrote equals what the Python MultiContext's refine_pose
and refine write from the same padded rows, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

DIR = os.path.join(ROOT, "tests", "cpp_multi_refine")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_refine_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 29


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32).reshape(-1).tolist()


@pytest.mark.gpu
def test_cpp_refine_equals_python(usac, tmp_path):
    from tests import test_gpu_multi_device as dev
    _build()
    kind = "E"
    case = dev._case("six", kind)
    rows, valid = case["rows"], case["valid"]
    P, n_max = valid.shape
    prob, max_iters, R, seed, refine_iters = 0.95, 256, 64, 100, 10
    model = dev._model(usac, kind)
    with usac.MultiContext.from_padded(dev._est(usac, kind), torch.from_numpy(rows).cuda(),
                                       valid=torch.from_numpy(valid).cuda()) as mc:
        mc.run(model, polish=True)
        pose = mc.export_pose(front_mask=True)
        py = {key: t.cpu().numpy() for key, t in
              mc.refine_pose(pose["R"], pose["t"], pose["front_mask"], max_iters=refine_iters).items()}
        R0, t0 = pose["R"].cpu().numpy(), pose["t"].cpu().numpy()
        every = mc.refine(R0, t0, None, refine_iters)
    rows.tofile(tmp_path / "rows.f32")
    valid.astype(np.uint8).tofile(tmp_path / "valid.u8")
    args = ["run", P, n_max, "rows.f32", "valid.u8", dev.THR[kind], prob, max_iters, R, seed, refine_iters]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(r.stdout)
    assert doc["refused_before_a_polish"] is True
    assert doc["R0"] == _bits(R0) and doc["t0"] == _bits(t0)
    for key in ("R", "t", "E", "cost0", "cost"):
        assert doc[key] == _bits(py[key]), key
        assert doc["all_" + key] == _bits(every[key]), key
    for key in ("iterations", "used"):
        assert doc[key] == py[key].tolist(), key
        assert doc["all_" + key] == every[key].tolist(), key
    assert max(doc["iterations"]) > 0 and max(doc["used"]) > 100
