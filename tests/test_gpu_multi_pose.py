"""Pose of multi contexts on the GPU (MultiContext.pose / export_pose, usac_multi_pose and usac_multi_pose_device;
ABI 28).  The yardstick is tests/helpers/multi_pose_ref.py, the rule of include/usac_gpu.h "Pose" in numpy, anchored
on the CPU by tests/test_multi_pose_cpu.py.  Every comparison is exact (floats by bit pattern): the kernel and the
restatement run the same fp64 operations in the same order, and the counts are integers.

The problems: n_p = 5, 6, 63, 64, 65, 257, 1000 and a copy of the 257-point one, in one context -- below, at and
above a wave, one row past a workgroup's stride of 256, several strides, and two problems that must agree."""
import ctypes

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import multi_export_ref as xref
from tests.helpers import multi_pixels_ref as pref
from tests.helpers import multi_pose_ref as ref
from tests.helpers.same_bits import same as _same

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

from tests import test_gpu_multi_device as dev  # noqa: E402  (its models and thresholds)

pytestmark = pytest.mark.gpu

SIZES = [5, 6, 63, 64, 65, 257, 1000]
RATIOS = [1.0, 1.0, 0.8, 0.7, 0.6, 0.5, 0.5]
SEEDS = [51, 52, 53, 54, 55, 56, 57]
DUP = 5  # problem 7 is a copy of problem 5
P = 8
N_MAX = 1000
KEYS = ("R", "t", "front", "choice")


def _sets():
    out = [synthetic.fundamental_points(n=n, inlier_ratio=r, seed=s, normalized=True, prosac_order=False)[0]
           for n, r, s in zip(SIZES, RATIOS, SEEDS)]
    out.append(out[DUP].copy())
    return out


def _pixel_sets(K1, K2):
    """the same scenes in pixels, problem p seen through K1[p] and K2[p] (multi_pixels_ref.pixel_sets' transform)"""
    Ki = np.linalg.inv(synthetic.two_view_geometry()[0])
    out = []
    for p in range(P):
        q = DUP if p == P - 1 else p
        pts = synthetic.fundamental_points(n=SIZES[q], inlier_ratio=RATIOS[q], seed=SEEDS[q], normalized=False,
                                           prosac_order=False)[0]
        views = []
        for v, k in ((0, K1[p]), (1, K2[p])):
            h = np.c_[pts[:, 2 * v:2 * v + 2].astype(np.float64), np.ones(len(pts))] @ (k.astype(np.float64) @ Ki).T
            views.append(h[:, :2] / h[:, 2:3])
        out.append(np.ascontiguousarray(np.concatenate(views, axis=1), dtype=np.float32))
    return out


def _e_gt():
    return synthetic.fundamental_points(n=10, seed=1, normalized=True)[1].reshape(9)


def _ff(shape, dtype, byte):
    size = torch.empty((), dtype=dtype).element_size()
    t = torch.full(tuple(shape[:-1]) + (shape[-1] * size,), byte, dtype=torch.uint8, device="cuda")
    return t.view(dtype)


def _outs(n_max, byte=255):
    return {"R": _ff((P, 3, 3), torch.float32, byte), "t": _ff((P, 3), torch.float32, byte),
            "front": _ff((P,), torch.int32, byte), "choice": _ff((P,), torch.int32, byte),
            "front_mask": _ff((P, n_max), torch.uint8, byte)}


def _width(mc):
    return mc.n_max if mc.n_max is not None else int(mc.sizes.max())


def _export_pose(mc, byte=255, **kw):
    """export_pose into tensors whose every byte is `byte` -> numpy arrays by key"""
    outs = _outs(_width(mc), byte)
    got = mc.export_pose(out=outs, **kw)
    assert set(got) == set(outs) and all(got[key] is outs[key] for key in outs)
    return {key: t.cpu().numpy() for key, t in got.items()}


def _source(mc):
    return None if mc.n_max is None else mc.source_index


def _packed(mc, padded):
    """a (P, n_max) mask in the layout of the exports -> the N_total bytes over the packed rows"""
    out = np.zeros(int(mc.offsets[-1]), dtype=np.uint8)
    for p in range(mc.P):
        lo, hi = int(mc.offsets[p]), int(mc.offsets[p + 1])
        out[lo:hi] = padded[p, xref.columns(mc.offsets, _source(mc), p)]
    return out


@pytest.fixture(scope="module")
def host(usac):
    """a context created from the host after run(polish=True): the polished models, the run's mask, the rows"""
    sets = _sets()
    with usac.MultiContext.essential(sets) as mc:
        res = mc.run(dev._model(usac, "E"), polish=True)
        points = mc.resident_points()
        _same(points, np.concatenate(sets), "the resident rows")
        yield {"mc": mc, "points": points, "mask": mc.last_mask.copy(),
               "models": np.stack([r["polished"]["model"] for r in res]).reshape(P, 9),
               "counts": [r["polished"]["inliers"] for r in res]}


def _one_row_masks(offsets):
    """one set byte per problem: its first row, its last row, or one in between"""
    out = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for p in range(P):
        n = int(offsets[p + 1] - offsets[p])
        out[int(offsets[p]) + (0, n - 1, n // 2)[p % 3]] = 1
    return out


def test_pose_equals_the_restatement(usac, host):
    mc, points, offsets = host["mc"], host["points"], host["mc"].offsets
    e_gt = _e_gt()
    mixed = host["models"].copy()  # one batch with every kind of model in it
    mixed[1], mixed[2], mixed[3], mixed[4] = e_gt, -e_gt, np.nan, 0.0
    models = {"polished": host["models"], "E_gt": np.tile(e_gt, (P, 1)), "-E_gt": np.tile(-e_gt, (P, 1)),
              "NaN": np.full((P, 9), np.nan, dtype=np.float32), "zero": np.zeros((P, 9), dtype=np.float32),
              "mixed": mixed}
    single = np.zeros(int(offsets[-1]), dtype=np.uint8)
    single[int(offsets[6]) + 999] = 1  # one row in the whole batch: the last thread's, in the last stride
    masks = {"polish": host["mask"], "none": None, "zero": np.zeros(int(offsets[-1]), dtype=np.uint8),
             "one per problem": _one_row_masks(offsets), "single": single}
    chosen = set()
    for mname, E in models.items():
        for kname, mask in masks.items():
            got = mc.pose(E, mask)
            want = ref.pose_batch(E, points, offsets, mask)
            _same(got, want, (mname, kname))
            chosen.update(got["choice"].tolist())
            if mname in ("NaN", "zero") or kname == "zero":
                assert (got["choice"] == -1).all() and not got["front_mask"].any() and not got["front"].any()
                _same(got["R"], np.tile(np.eye(3, dtype=np.float32), (P, 1, 1)), "identity")
    got = mc.pose(host["models"], host["mask"])
    assert (got["front"][2:] > 0).all() and got["front"][6] > 300, got["front"]  # the polished models have a pose
    twin = mc.pose(np.tile(host["models"][DUP], (P, 1)), None)  # one model on a problem and on its copy
    _same(twin["R"][DUP], twin["R"][P - 1], "the copy's rotation")
    _same(twin["front_mask"][offsets[DUP]:offsets[DUP + 1]], twin["front_mask"][offsets[P - 1]:offsets[P]], "the copy's mask")
    assert twin["front"][DUP] == twin["front"][P - 1] > 100 and twin["choice"][DUP] == twin["choice"][P - 1]
    assert got["front"].tolist() == [int(got["front_mask"][offsets[p]:offsets[p + 1]].sum()) for p in range(P)]
    assert (got["front_mask"] <= host["mask"]).all()
    assert len(chosen - {-1}) >= 2, "one candidate only: the fixtures show nothing about the choice"


def test_rows_that_are_not_finite(usac):
    sets = _sets()
    for p, i, row in ((2, 0, (np.nan, 0.1, 0.1, 0.1)), (3, 63, (0.1, np.inf, 0.1, 0.2)), (5, 256, (0.0, 0.1, -np.inf, 0.1)),
                      (6, 999, (np.nan,) * 4), (6, 255, (0.1, 0.2, 0.3, np.nan))):
        sets[p][i] = row
    e_gt = np.tile(_e_gt(), (P, 1))
    with usac.MultiContext.essential(sets) as mc:
        points = mc.resident_points()
        _same(points, np.concatenate(sets), "the resident rows")
        for mask in (None, np.ones(len(points), dtype=np.uint8)):
            got = mc.pose(e_gt, mask)
            _same(got, ref.pose_batch(e_gt, points, mc.offsets, mask), "non-finite rows")
            bad = ~np.isfinite(points).all(1)
            assert bad.sum() == 5 and not got["front_mask"][bad].any()
            assert (got["choice"] >= 0).all()


def _check_export(mc, what, status_of=None):
    """export_pose against pose() of the exported models and mask, and against the restatement"""
    exp = {key: t.cpu().numpy() for key, t in mc.export_device().items()}
    got = _export_pose(mc)
    packed = _packed(mc, exp["mask"].astype(np.uint8))
    models = exp["models"].reshape(P, 9)
    status = exp["status"]
    if status_of is not None:
        assert status.tolist() == status_of
    want = ref.pose_batch(models, mc.resident_points(), mc.offsets, packed, status)
    if (status == 0).all():
        _same(mc.pose(models, packed), want, (what, "pose() of the exported result"))
    for key in KEYS:
        _same(got[key], want[key], (what, key))
    width = _width(mc)
    _same(got["front_mask"], xref.padded_mask(want["front_mask"], mc.offsets, _source(mc), width), (what, "front_mask"))
    assert (got["front_mask"] <= exp["mask"].astype(np.uint8)).all()
    _same(_export_pose(mc, byte=0), got, (what, "into zero-filled tensors"))  # and twice the same bytes
    after = {key: t.cpu().numpy() for key, t in mc.export_device().items()}
    _same(after, exp, (what, "the resident result is untouched"))
    return got, exp


def _padded_pixels(K1, K2, seed):
    sets = _pixel_sets(K1, K2)
    rng = np.random.default_rng(seed)
    rows = rng.uniform(0, 1000, size=(P, N_MAX, 4)).astype(np.float32)  # columns that are not kept hold anything
    valid = np.zeros((P, N_MAX), dtype=bool)
    for p, s in enumerate(sets):
        cols = np.sort(rng.permutation(N_MAX)[:len(s)])
        valid[p, cols] = True
        rows[p, cols] = s
    return rows, valid


def test_export_pose_on_a_host_context(usac):
    with usac.MultiContext.essential(_sets()) as mc:
        mc.keep_on_device = True
        res = mc.run(dev._model(usac, "E"), polish=True)
        assert mc.last_mask is None
        got, exp = _check_export(mc, "host")
        assert (got["choice"][2:] >= 0).all() and got["front"][6] > 300
        fresh = mc.export_pose(front_mask=True)  # fresh tensors: the documented shapes and dtypes
        assert fresh["R"].dtype == torch.float32 and tuple(fresh["R"].shape) == (P, 3, 3) and fresh["R"].is_cuda
        assert fresh["t"].dtype == torch.float32 and tuple(fresh["t"].shape) == (P, 3)
        assert fresh["front"].dtype == torch.int32 and fresh["choice"].dtype == torch.int32
        assert fresh["front_mask"].dtype == torch.bool and tuple(fresh["front_mask"].shape) == (P, 1000)
        _same(fresh["front_mask"].cpu().numpy().astype(np.uint8), got["front_mask"], "fresh mask")
        assert set(mc.export_pose()) == set(KEYS)
        wide = mc.export_pose(front_mask=True, n_max=1007)  # from the host: any width >= the largest problem
        _same(wide["front_mask"].cpu().numpy().astype(np.uint8)[:, :1000], got["front_mask"], "a wider mask")
        assert not wide["front_mask"][:, 1000:].any()
        # a problem without a model: the zero matrix has no inlier
        starts = np.stack([r["polished"]["model"] for r in res]).reshape(P, 9).copy()
        starts[3] = 0.0
        mc.polish(starts, dev.THR["E"])
        got, exp = _check_export(mc, "no model", status_of=[0, 0, 0, -111, 0, 0, 0, 0])
        assert got["choice"][3] == -1 and got["front"][3] == 0 and not got["front_mask"][3].any()
        _same(got["R"][3], np.eye(3, dtype=np.float32), "identity")
        _same(got["t"][3], np.zeros(3, dtype=np.float32), "zero")
        assert (got["choice"][[2, 4, 5, 6, 7]] >= 0).all()


def test_export_pose_on_pixel_contexts(usac):
    K1, K2 = pref.intrinsics(P)
    assert not (K1 == K2).all()
    E = usac.ESTIMATOR.Essential
    rows, valid = _padded_pixels(K1, K2, 3)
    scores = np.random.default_rng(4).random((P, N_MAX)).astype(np.float32)
    made = [("essential_pixels", lambda: usac.MultiContext.essential_pixels(_pixel_sets(K1, K2), K1, K2)),
            ("from_padded", lambda: usac.MultiContext.from_padded(E, dev._dev(rows), valid=dev._dev(valid), K1=K1, K2=K2)),
            ("from_padded, sorted", lambda: usac.MultiContext.from_padded(E, dev._dev(rows), valid=dev._dev(valid), K1=K1,
                                                                         K2=K2, scores=dev._dev(scores)))]
    for what, make in made:
        with make() as mc:
            mc.set_pixel_thresholds(45.0)
            mc.keep_on_device = True
            mc.run(dev._model(usac, "E"), polish=True)
            got, exp = _check_export(mc, what)
            assert (got["choice"][2:] >= 0).all() and got["front"][6] > 300, (what, got["front"])
            if mc.n_max is not None:
                assert mc.n_max == N_MAX and not got["front_mask"].astype(bool)[~valid].any()
                src = mc.source_index
                if mc.sorted_by_score:  # quality order: the columns of some problem do not ascend
                    assert any((np.diff(src[mc.offsets[p]:mc.offsets[p + 1]].astype(np.int64)) < 0).any() for p in range(P))


def test_refusals(usac, host):
    sets = _sets()
    with usac.MultiContext.essential(sets) as mc:
        outs = _outs(1000)

        def refused(code, word, **kw):
            with pytest.raises(usac.UsacError) as e:
                mc.export_pose(out=outs, **kw)
            assert e.value.code == code and word in str(e.value), str(e.value)
            for key, t in outs.items():
                assert (t.contiguous().view(torch.uint8).cpu().numpy() == 255).all(), "%s was written" % key

        refused(-3, "no polishing call has run")
        res = mc.run(dev._model(usac, "E"), polish=True)
        mc.export_pose(front_mask=True)
        with pytest.raises(usac.UsacError) as e:  # a context from the host: below the largest problem
            mc.export_pose(front_mask=True, n_max=999)
        assert e.value.code == -1 and "n_max" in str(e.value)
        # host memory: the Python layer refuses it by type, the library (asked directly) before any launch
        with pytest.raises(TypeError):
            mc.export_pose(out={"R": np.zeros((P, 3, 3), np.float32)})
        hostR = np.full((P, 36), 255, dtype=np.uint8)
        o = usac._MultiPoseOutput(n_max=1000, R=hostR.ctypes.data, **{k: outs[k].data_ptr() for k in outs if k != "R"})
        assert usac.lib().usac_multi_pose_device(mc._h, ctypes.byref(o)) == -1
        msg = usac.lib().usac_multi_last_error(mc._h).decode()
        assert "R is not device memory" in msg, msg
        assert (hostR == 255).all()
        o = usac._MultiPoseOutput(n_max=1000)  # every output pointer is NULL
        assert usac.lib().usac_multi_pose_device(mc._h, ctypes.byref(o)) == -1
        assert usac.lib().usac_multi_pose_device(mc._h, None) == -1
        for key, bad in (("R", _ff((P, 9), torch.float32, 255)), ("front", _ff((P,), torch.float32, 255)),
                         ("front_mask", _ff((P, 1001), torch.uint8, 255))):
            with pytest.raises(ValueError):
                mc.export_pose(out={key: bad})
        with pytest.raises(ValueError):
            mc.export_pose(out={"rotation": outs["R"]})
        models = np.stack([r["polished"]["model"] for r in res])
        mc.inliers(models, dev.THR["E"])
        refused(-3, "usac_multi_inliers")
        # pose() from host arrays needs no resident result, and its NULL arguments are refused
        _same(mc.pose(models, None), host["mc"].pose(models, None), "pose() without a resident result")
        L = usac.lib()
        ch = np.zeros(P, dtype=np.int32)
        fp = ctypes.POINTER(ctypes.c_float)
        assert L.usac_multi_pose(mc._h, None, None, None, None, None, ch.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None) == -1
        assert L.usac_multi_pose(mc._h, models.ctypes.data_as(fp), None, None, None, None, None, None) == -1
    hsets = [synthetic.homography_points(n=n, inlier_ratio=0.7, seed=60 + n)[0].astype(np.float32) for n in (64, 65)]
    with usac.MultiContext(usac.ESTIMATOR.Homography, hsets) as hc:
        hc.run(dev._model(usac, "H"), polish=True)
        with pytest.raises(usac.UsacError) as e:
            hc.export_pose()
        assert e.value.code == -3 and "essential" in str(e.value)
        with pytest.raises(usac.UsacError) as e:
            hc.pose(np.zeros((2, 9), dtype=np.float32))
        assert e.value.code == -3 and "essential" in str(e.value)


def test_repeatable_and_on_a_side_stream(usac, host):
    mc = host["mc"]
    a = mc.pose(host["models"], host["mask"])
    b = mc.pose(host["models"], host["mask"])
    _same(a, b, "two identical calls")
    mc.run(dev._model(usac, "E"), polish=True)
    want = _export_pose(mc)
    outs = _outs(1000)
    torch.cuda.synchronize()  # the fill ran on the default stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = mc.export_pose(out=outs)  # the default: torch's current stream, s
        counted = got["front_mask"].to(torch.int32).sum(1)  # queued behind the export on s
    s.synchronize()
    _same({key: t.cpu().numpy() for key, t in got.items()}, want, "side stream")
    _same(counted.cpu().numpy().astype(np.int32), want["front"], "the operation queued behind it")
    outs = _outs(1000)
    torch.cuda.synchronize()
    again = mc.export_pose(out=outs, stream=s.cuda_stream)
    s.synchronize()
    _same({key: t.cpu().numpy() for key, t in again.items()}, want, "the stream given by handle")
