"""The h16 prefilter bound on the host (no GPU): tests/cpp_h16_slack/slack_check.cpp calls the library's own
h16_rows_of (ransac_amd/csrc/usac_h16.hpp) and checks, pair by pair against long double, that the fp16 tile value
lies within the row's bound D and that every pair the packed stage A keeps is kept by the tile test with the slack
F_m (DESIGN.md §6 "Matrix-core prefilter").  Per seed (1 and 2): 2 032 points of the cfg2 generator plus the 16
corners of their box (every |f_k| at the maximum the bound assumes), 2 000 four-point DLT models of random
minimal samples and the adversarial models of tests/test_gpu_h16.py (perturbed ground truth, scales 1e±20,
1e-30 perspective terms, 1e±30, NaN / inf / zero / singular): 4 500 models and 9.2 M pairs in all.  The same
program built with the 2^-10 roundings the bound used to charge stays within half of that bound."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.conftest import ROOT

DIR = os.path.join(ROOT, "tests", "cpp_h16_slack")
THR = 2.0


def _dlt_models(pts, count, rng):
    """4-point DLT homographies (the fp64 null vector of the 8 x 9 system, largest coefficient 1, fp32)"""
    idx = np.stack([rng.choice(len(pts), 4, replace=False) for _ in range(count)])
    p = pts[idx].astype(np.float64)
    x1, y1, x2, y2 = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    z, o = np.zeros_like(x1), np.ones_like(x1)
    A = np.concatenate([np.stack([-x1, -y1, -o, z, z, z, x2 * x1, x2 * y1, x2], -1),
                        np.stack([z, z, z, -x1, -y1, -o, y2 * x1, y2 * y1, y2], -1)], 1)
    h = np.linalg.svd(A)[2][:, -1, :]
    return (h / np.abs(h).max(1, keepdims=True)).astype(np.float32)


def _adversarial_models(Hgt, rng):
    base = (Hgt / Hgt[2, 2]).reshape(9).astype(np.float32)
    models = [base]
    for scale in (1e-6, 1e-4, 1e-2, 1.0):
        models += [base * (1 + scale * rng.standard_normal(9).astype(np.float32)) for _ in range(40)]
    with np.errstate(over="ignore"):
        models += [rng.standard_normal(9).astype(np.float32) * np.float32(10 ** rng.uniform(-20, 20)) for _ in range(82)]
    tiny = base.copy()
    tiny[6:] = [1e-30, -1e-30, 1e-38]
    singular = np.array([1, 2, 3, 2, 4, 6, 1e-3, 2e-3, 3e-3], np.float32)
    models += [tiny, base * np.float32(1e30), base * np.float32(1e-30), np.full(9, np.nan, np.float32),
               np.full(9, np.inf, np.float32), np.zeros(9, np.float32), singular]
    return np.stack(models).astype(np.float32)


def _case(path, seed):
    pts, Hgt, _ = synthetic.homography_points(n=10000, inlier_ratio=0.3, seed=seed)
    pts = pts[:2032]
    lo, hi = pts.min(0), pts.max(0)
    corners = np.array([[(lo, hi)[b][k] for k, b in enumerate(bits)] for bits in itertools.product((0, 1), repeat=4)],
                       dtype=np.float32)
    pts = np.concatenate([pts, corners])
    rng = np.random.default_rng(seed)
    models = np.concatenate([_dlt_models(pts[:2032], 2000, rng), _adversarial_models(Hgt, rng)])
    assert len(pts) == 2048 and len(models) == 2250
    with open(path, "wb") as f:
        f.write(np.array([len(pts), len(models)], np.uint32).tobytes())
        f.write(np.array([THR], np.float32).tobytes())
        f.write(np.ascontiguousarray(pts, np.float32).tobytes())
        f.write(np.ascontiguousarray(models, np.float32).tobytes())
    return len(pts) * len(models)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", DIR], check=True)
    d = tmp_path_factory.mktemp("h16_slack")
    out = []
    for seed in (1, 2):
        path = str(d / ("seed%d.bin" % seed))
        out.append((path, _case(path, seed)))
    return out


def _run(exe, path, pairs):
    r = subprocess.run([os.path.join(DIR, "build", exe), path], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr
    ratios = [float(v) for v in re.search(r"ratio ex (\S+) ey (\S+) zr (\S+)", r.stdout).groups()]
    stats = dict(zip(*[iter(re.search(r"pairs .*", r.stdout).group(0).split())] * 2))
    assert int(stats["pairs"]) == pairs                     # no pair skipped
    assert int(stats["points_at_fmax"]) >= 16               # the box corners
    assert 0 < int(stats["models_without_prefilter"]) < 100  # NaN / inf / zero / out-of-range models, and only those
    assert int(stats["stage_a_kept"]) <= int(stats["tile_kept"])
    return ratios


@pytest.mark.parametrize("which", [0, 1])
def test_tile_within_bound_and_nothing_lost(cases, which):
    """(a) and (b) of slack_check.cpp with the library's constants: the program itself fails at the first pair
    outside the bound; the ratios it prints are the largest |tile - exact| / D per row"""
    ratios = _run("slack_check", *cases[which])
    assert all(0.0 < v <= 1.0 for v in ratios), ratios


@pytest.mark.parametrize("which", [0, 1])
def test_old_roundings_were_twice_too_wide(cases, which):
    """with 2^-10 charged for both fp16 roundings (the bound before) the same pairs use at most half of D"""
    ratios = _run("slack_check_loose", *cases[which])
    assert all(0.0 < v <= 0.5 for v in ratios), ratios
