"""bench.py's plain line and --dump-outputs: a run without --full prints the headline fields only
and writes what its last timed step returned; the dump is float32 / float64 .npy files within the
size limit, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}


def test_options_default_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_headline_fields():
    a = type("A", (), {"steps": 4, "warmup": 1})()
    line = bench.headline(a, 1, 1000.0, 0.002, "weak", {})
    assert HEADLINE <= set(line)
    assert line["ms_per_step"] == 0.5 and line["value"] == 1000.0 and line["unit"] == "hypotheses/s"
    json.dumps(line)


def test_dump_outputs_types(tmp_path):
    d = tmp_path / "o"
    bench.dump_outputs(str(d), {"counts": np.arange(5, dtype=np.int32), "sums": np.ones(5, np.float32),
                                "one": np.float64(3.0)})
    assert sorted(os.listdir(d)) == ["counts.npy", "one.npy", "sums.npy"]
    assert np.load(d / "counts.npy").dtype == np.float64 and np.load(d / "counts.npy").tolist() == [0, 1, 2, 3, 4]
    assert np.load(d / "sums.npy").dtype == np.float32
    assert np.load(d / "one.npy").tolist() == [3.0]


def test_dump_outputs_limit(tmp_path, monkeypatch):
    """Over the limit an array larger than its share is cut to a fixed sample of its rows."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = np.arange(3000, dtype=np.float32).reshape(1000, 3)
    small = np.arange(10, dtype=np.float32)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (2048 // 12, 3) and np.array_equal(a, b)
    assert (np.diff(a[:, 0]) > 0).all() and np.array_equal(a[:, 1], a[:, 0] + 1)  # whole rows, ascending
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= 4096


@pytest.mark.gpu
def test_plain_run_dumps_last_step(usac, tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1` at a small size: one line with the headline fields and
    nothing that --full adds; the dumped counts are those of the last timed batch (hypotheses
    3 B .. 4 B - 1 of the device stream) scored through the synchronous entry point."""
    from ransac_amd import synthetic

    B, n = 2048, 2000
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
                        "--points", str(n), "--prewarm-ms", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert HEADLINE <= set(d) and d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(3 * B / (3 * d["ms_per_step"] * 1e-3))
    assert not {"parity", "roofline", "cpu_baseline"} & set(d)
    counts, sums, rec = (np.load(out / (k + ".npy")) for k in ("counts", "sums", "best_record"))
    assert counts.dtype == np.float64 and sums.dtype == np.float32 and rec.dtype == np.float64
    assert counts.shape == sums.shape == (B,) and rec.shape == (13,)
    pts, _, _ = synthetic.homography_points(n=n, inlier_ratio=0.3, seed=1)
    with usac.Context(usac.ESTIMATOR.Homography, pts, device=0) as ctx:
        c, _, best = ctx.hypothesize_score(B=B, seed=1, first_hyp=3 * B, thr=2.0)
    assert np.array_equal(counts, c)
    # the record: the most inliers, of a hypothesis of this batch that has them (ties go by the Σ)
    assert rec[1] == c.max() == best["inliers"] and rec[3] == 1
    assert 3 * B <= rec[0] < 4 * B and c[int(rec[0]) - 3 * B] == c.max()
