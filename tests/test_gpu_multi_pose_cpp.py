"""usac_gpu::MultiContext::poseDevice / pose (include/usac_gpu.hpp, ABI 28) driven from C++:
tests/cpp_multi_pose/consumer.cpp is built with hipcc (it allocates the device memory it hands over) against the
header and the in-tree library, and on a GPU what its calls wrote equals what the Python MultiContext's export_pose
and pose write from the same padded rows, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

DIR = os.path.join(ROOT, "tests", "cpp_multi_pose")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_pose_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 28


@pytest.mark.gpu
def test_cpp_pose_equals_python(usac, tmp_path):
    from tests import test_gpu_multi_device as dev
    _build()
    kind = "E"
    case = dev._case("six", kind)
    rows, valid = case["rows"], case["valid"]
    P, n_max = valid.shape
    prob, max_iters, R, seed = 0.95, 256, 64, 100
    model = dev._model(usac, kind)
    with usac.MultiContext.from_padded(dev._est(usac, kind), torch.from_numpy(rows).cuda(),
                                       valid=torch.from_numpy(valid).cuda()) as mc:
        runs = mc.run(model, polish=True)
        py = {key: t.cpu().numpy() for key, t in mc.export_pose(front_mask=True).items()}
        models = np.stack([r_["polished"]["model"] for r_ in runs]).reshape(P, 9)
        every = mc.pose(models)
    rows.tofile(tmp_path / "rows.f32")
    valid.astype(np.uint8).tofile(tmp_path / "valid.u8")
    args = ["run", P, n_max, "rows.f32", "valid.u8", dev.THR[kind], prob, max_iters, R, seed]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(r.stdout)
    assert doc["refused_before_a_polish"] is True
    assert doc["models"] == models.view(np.int32).reshape(-1).tolist()
    assert doc["R"] == py["R"].view(np.int32).reshape(-1).tolist()
    assert doc["t"] == py["t"].view(np.int32).reshape(-1).tolist()
    assert doc["front"] == py["front"].tolist() and doc["choice"] == py["choice"].tolist()
    assert doc["front_mask"] == py["front_mask"].astype(np.uint8).reshape(-1).tolist()
    assert doc["all_R"] == every["R"].view(np.int32).reshape(-1).tolist()
    assert doc["all_t"] == every["t"].view(np.int32).reshape(-1).tolist()
    assert doc["all_front"] == every["front"].tolist() and doc["all_choice"] == every["choice"].tolist()
    assert doc["all_front_mask"] == every["front_mask"].tolist()
    assert max(doc["front"]) > 100 and max(doc["choice"]) >= 0
