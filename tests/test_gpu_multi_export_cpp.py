"""usac_gpu::MultiContext::setResident / exportDevice (include/usac_gpu.hpp, ABI 27) driven from C++:
tests/cpp_multi_export/consumer.cpp is built with hipcc (it allocates the device memory it hands over) against the
header and the in-tree library, and on a GPU what its export wrote equals what the Python MultiContext's export
writes from the same padded rows, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

DIR = os.path.join(ROOT, "tests", "cpp_multi_export")
BIN = os.path.join(DIR, "build", "consumer")


def _build():
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    assert os.path.exists(BIN)


def test_cpp_multi_export_consumer_compiles_and_links(usac):
    _build()
    r = subprocess.run([BIN, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout)
    assert d["abi"] == d["header"] == usac.lib().usac_abi_version() >= 27


@pytest.mark.gpu
def test_cpp_export_equals_python(usac, tmp_path):
    from tests import test_gpu_multi_device as dev
    _build()
    kind, k_max = "H", 100  # 100: the larger problems' lists are cut, the smaller ones' padded
    case = dev._case("six", kind)
    rows, valid = case["rows"], case["valid"]
    P, n_max = valid.shape
    prob, max_iters, R, seed = 0.95, 256, 64, 100
    model = dev._model(usac, kind)
    with usac.MultiContext.from_padded(dev._est(usac, kind), torch.from_numpy(rows).cuda(),
                                       valid=torch.from_numpy(valid).cuda()) as mc:
        runs = mc.run(model, polish=True)
        py = {key: t.cpu().numpy() for key, t in mc.export_device(inlier_cols=k_max).items()}
    rows.tofile(tmp_path / "rows.f32")
    valid.astype(np.uint8).tofile(tmp_path / "valid.u8")
    args = ["run", P, n_max, "rows.f32", "valid.u8", dev.THR[kind], prob, max_iters, R, seed, k_max]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads(r.stdout)
    assert doc["refused_before_a_polish"] is True and doc["resident_mode_same"] is True
    assert doc["models"] == py["models"].view(np.int32).reshape(-1).tolist()
    assert doc["inliers"] == py["inliers"].tolist() == doc["host_inliers"] == [r_["polished"]["inliers"] for r_ in runs]
    assert doc["status"] == py["status"].tolist()
    assert doc["mask"] == py["mask"].astype(np.uint8).reshape(-1).tolist()
    assert doc["inlier_cols"] == py["inlier_cols"].reshape(-1).tolist()
    assert max(doc["inliers"]) > k_max > min(doc["inliers"])
