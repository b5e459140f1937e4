"""Pose refinement of multi contexts on the GPU (MultiContext.refine / refine_pose, usac_multi_refine_pose and
usac_multi_refine_pose_device; ABI 29).  The yardstick is tests/helpers/multi_refine_ref.py, the rule of
include/usac_gpu.h "Pose refinement" in numpy, anchored on the CPU by tests/test_multi_refine_cpu.py.  Every
comparison is exact (floats and doubles by bit pattern): the kernel and the restatement run the same fp64
operations in the same order, the order of the sums included.

The problems: n_p = 5, 6, 63, 64, 65, 255, 256, 257, 1000 and a copy of the 257-point one, in one context -- below,
at and above a wave, one row below, at and past a workgroup's stride of 256, several strides, and two problems
that must agree.  A problem of 4 rows does not exist: a context refuses a problem below the sample size of 5, so
fewer than 5 used rows come from masks."""
import ctypes

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import multi_export_ref as xref
from tests.helpers import multi_pixels_ref as pref
from tests.helpers import multi_refine_ref as ref
from tests.helpers.same_bits import same as _same

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

from tests import test_gpu_multi_device as dev  # noqa: E402  (its models and thresholds)

pytestmark = pytest.mark.gpu

SIZES = [5, 6, 63, 64, 65, 255, 256, 257, 1000]
RATIOS = [1.0, 1.0, 0.8, 0.7, 0.6, 0.6, 0.5, 0.5, 0.5]
SEEDS = [51, 52, 53, 54, 55, 58, 59, 56, 57]
DUP = 7  # problem 9 is a copy of problem 7
P = 10
N_MAX = 1000
KEYS = ref.KEYS


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


def _gt_pose():
    _, R, t, _, _ = synthetic.two_view_geometry()
    return np.tile(R.astype(np.float32), (P, 1, 1)), np.tile((t / np.linalg.norm(t)).astype(np.float32), (P, 1))


def _perturbed():
    """a pose per problem a few degrees and a few hundredths off the scene's, t of any length"""
    rng = np.random.default_rng(21)
    R, t = _gt_pose()
    for p in range(P):
        a = rng.standard_normal(3)
        a /= np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        ang = np.deg2rad(rng.uniform(0.5, 5.0))
        R[p] = ((np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)) @ R[p].astype(np.float64)).astype(np.float32)
        t[p] = ((t[p] + rng.uniform(-0.1, 0.1, 3)) * rng.uniform(0.2, 300.0)).astype(np.float32)
    return R, t


def _ff(shape, dtype, byte):
    size = torch.empty((), dtype=dtype).element_size()
    t = torch.full(tuple(shape[:-1]) + (shape[-1] * size,), byte, dtype=torch.uint8, device="cuda")
    return t.view(dtype)


def _outs(byte=255):
    return {"R": _ff((P, 3, 3), torch.float32, byte), "t": _ff((P, 3), torch.float32, byte),
            "E": _ff((P, 3, 3), torch.float32, byte), "cost0": _ff((P,), torch.float64, byte),
            "cost": _ff((P,), torch.float64, byte), "iterations": _ff((P,), torch.int32, byte),
            "used": _ff((P,), torch.int32, byte)}


def _np(d):
    return {key: t.cpu().numpy() for key, t in d.items()}


def _refine_pose(mc, R, t, mask, byte=255, **kw):
    """refine_pose into tensors whose every byte is `byte` -> numpy arrays by key"""
    outs = _outs(byte)
    got = mc.refine_pose(R, t, mask, out=outs, **kw)
    assert set(got) == set(outs) and all(got[key] is outs[key] for key in outs)
    return _np(got)


def _source(mc):
    return None if mc.n_max is None else mc.source_index


def _packed(mc, padded):
    """a (P, n_max) mask in the layout of the exports -> the N_total bytes over the packed rows"""
    out = np.zeros(int(mc.offsets[-1]), dtype=np.uint8)
    for p in range(mc.P):
        lo, hi = int(mc.offsets[p]), int(mc.offsets[p + 1])
        out[lo:hi] = padded[p, xref.columns(mc.offsets, _source(mc), p)]
    return out


def _few_rows(offsets, k):
    """k set bytes per problem: its first row, its last row, and rows in between"""
    out = np.zeros(int(offsets[-1]), dtype=np.uint8)
    for p in range(P):
        n = int(offsets[p + 1] - offsets[p])
        out[int(offsets[p]) + np.unique(np.linspace(0, n - 1, k).astype(np.int64))] = 1
    return out


@pytest.fixture(scope="module")
def host(usac):
    """a context created from the host after run(polish=True): the polished models, the run's mask, the rows, and
    pose() of the polished models over that mask"""
    sets = _sets()
    with usac.MultiContext.essential(sets) as mc:
        res = mc.run(dev._model(usac, "E"), polish=True)
        points = mc.resident_points()
        _same(points, np.concatenate(sets), "the resident rows")
        models = np.stack([r["polished"]["model"] for r in res]).reshape(P, 9)
        mask = mc.last_mask.copy()
        yield {"mc": mc, "points": points, "mask": mask, "models": models, "pose": mc.pose(models, mask)}


def _all_hold(got):
    assert (got["cost"] <= got["cost0"]).all()
    skipped = got["iterations"] < 0
    assert not got["E"][skipped].any() and not got["cost0"][skipped].any()


def test_refine_equals_the_restatement(usac, host):
    mc, points, offsets = host["mc"], host["points"], host["mc"].offsets
    n_total = int(offsets[-1])
    pose = host["pose"]
    Rg, tg = _gt_pose()
    Rp, tp = _perturbed()
    Rm, tm = Rp.copy(), tp.copy()  # one batch with every kind of start in it
    Rm[1, 1, 2] = np.nan
    tm[2] = (0.1, np.inf, 0.2)
    tm[3] = 0.0
    Rm[4], tm[4] = np.eye(3), 0.0  # export_pose's choice = -1
    Rm[6], tm[6] = pose["R"][6], pose["t"][6]
    Rm[5] = 0.0  # finite, so not skipped: E and every D are zero, H is zero, every solve ends at its first pivot
    starts = {"pose()": (pose["R"], pose["t"]), "the scene's": (Rg, tg), "perturbed": (Rp, tp), "mixed": (Rm, tm)}
    masks = {"polish": host["mask"], "front_mask": pose["front_mask"], "none": None,
             "zero": np.zeros(n_total, dtype=np.uint8), "four rows": _few_rows(offsets, 4), "five rows": _few_rows(offsets, 5)}
    cases = [(s, m, 10) for s in starts for m in masks]
    cases += [("perturbed", "polish", k) for k in (0, 1, 50)] + [("pose()", "front_mask", k) for k in (0, 1, 50)]
    cases += [("mixed", "none", 0), ("perturbed", "five rows", 50)]
    seen = set()
    for sname, mname, iters in cases:
        R, t = starts[sname]
        got = mc.refine(R, t, masks[mname], iters)
        want = ref.refine_batch(R, t, points, offsets, masks[mname], iters)
        _same(got, want, (sname, mname, iters))
        _all_hold(got)
        seen.update(got["iterations"].tolist())
        if mname in ("zero", "four rows"):
            assert (got["iterations"] == -1).all() and (got["used"] == (0 if mname == "zero" else 4)).all()
            _same(got["R"], np.ascontiguousarray(R, np.float32).reshape(P, 3, 3), "the inputs' bits")
            _same(got["t"], np.ascontiguousarray(t, np.float32).reshape(P, 3), "the inputs' bits")
        if mname == "five rows":
            assert (got["used"] == 5).all()
        if sname == "mixed" and mname in ("none", "five rows"):
            assert (got["iterations"][[1, 2, 3, 4]] == -1).all() and (got["iterations"][[0, 5, 6, 7, 8, 9]] >= 0).all()
        if iters == 0 and sname != "mixed":
            assert (got["iterations"] == 0).all() and (got["cost"] == got["cost0"]).all()
    assert {-1, 0, 1} <= seen and max(seen) > 3
    # the rejection by the pivot, without a pass: twelve solves until lambda > 1e8, on the device as in the rule
    lo, hi = int(offsets[5]), int(offsets[6])
    flat = ref.refine(Rm[5], tm[5], points[lo:hi], None, 10)
    assert flat["pivots"] == 12 and flat["stop"] == "lambda" and flat["iterations"] == 0
    got = mc.refine(Rm, tm, None, 10)
    assert got["iterations"][5] == 0 and got["cost0"][5] == 0 and got["used"][5] == hi - lo and not got["R"][5].any()
    _same(got["t"][5], flat["t"], "the normalised start")
    # the refinement does something: from a perturbed start the cost over the polish's inliers falls
    got = mc.refine(Rp, tp, host["mask"], 10)
    assert (got["cost"][2:] < got["cost0"][2:]).all(), (got["cost0"], got["cost"])
    assert got["used"].tolist() == [int(host["mask"][offsets[p]:offsets[p + 1]].sum()) for p in range(P)]
    # one start on a problem and on its copy
    Rq, tq = Rp.copy(), tp.copy()
    Rq[P - 1], tq[P - 1] = Rq[DUP], tq[DUP]
    twin = mc.refine(Rq, tq, None, 10)  # every row: the two runs need not have found the same inliers
    for key in KEYS:
        _same(twin[key][DUP], twin[key][P - 1], ("the copy", key))
    assert twin["iterations"][DUP] > 0
    # E is a model the context takes: pose() of it gives the refined rotation back on a clean problem
    back = mc.pose(got["E"], host["mask"])
    assert np.abs(back["R"][8] - got["R"][8]).max() < 1e-5 and back["front"][8] > 300


def test_rows_that_are_not_finite(usac):
    sets = _sets()
    for p, i, row in ((2, 0, (np.nan, 0.1, 0.1, 0.1)), (3, 63, (0.1, np.inf, 0.1, 0.2)), (7, 256, (0.0, 0.1, -np.inf, 0.1)),
                      (8, 999, (np.nan,) * 4), (8, 255, (0.1, 0.2, 0.3, np.nan))):
        sets[p][i] = row
    R, t = _perturbed()
    with usac.MultiContext.essential(sets) as mc:
        points = mc.resident_points()
        _same(points, np.concatenate(sets), "the resident rows")
        for mask in (None, np.ones(len(points), dtype=np.uint8)):
            got = mc.refine(R, t, mask, 10)
            _same(got, ref.refine_batch(R, t, points, mc.offsets, mask, 10), "non-finite rows")
            _all_hold(got)
            assert got["used"].tolist() == [5, 6, 62, 63, 65, 255, 256, 256, 998, 257]
            assert np.isfinite(got["cost"]).all() and (got["iterations"] >= 0).all()


def _check_device(mc, what, status_of=None, starts=None):
    """refine_pose of export_pose's outputs against refine() of the same inputs, and against the restatement"""
    exp = _np(mc.export_device())
    pose_t = mc.export_pose(front_mask=True)
    pose = _np(pose_t)
    R_t, t_t = pose_t["R"], pose_t["t"]
    if starts is not None:
        R_t, t_t = torch.from_numpy(starts[0]).cuda(), torch.from_numpy(starts[1]).cuda()
    R, t = R_t.cpu().numpy(), t_t.cpu().numpy()
    status = exp["status"]
    if status_of is not None:
        assert status.tolist() == status_of
    points, offsets = mc.resident_points(), mc.offsets
    results = {}
    for mname, mask_t, padded in (("front_mask", pose_t["front_mask"], pose["front_mask"].astype(np.uint8)),
                                  ("resident", None, exp["mask"].astype(np.uint8))):
        packed = _packed(mc, padded)
        got = _refine_pose(mc, R_t, t_t, mask_t)
        want = ref.refine_batch(R, t, points, offsets, packed, 10, status)
        _same(got, want, (what, mname, "the restatement"))
        if (status == 0).all():
            _same(mc.refine(R, t, packed, 10), got, (what, mname, "refine() of the same inputs"))
        _all_hold(got)
        _same(_refine_pose(mc, R_t, t_t, mask_t, byte=0), got, (what, mname, "into zero-filled tensors"))  # and twice
        results[mname] = got
    # a uint8 mask is a bool mask
    _same(_refine_pose(mc, R_t, t_t, pose_t["front_mask"].to(torch.uint8)), results["front_mask"], (what, "uint8 mask"))
    _same(_np(mc.export_device()), exp, (what, "the resident result is untouched"))
    _same(_np(mc.export_pose(front_mask=True)), pose, (what, "export_pose is unchanged"))
    return results["front_mask"], pose, exp


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


def test_refine_pose_on_a_host_context(usac):
    with usac.MultiContext.essential(_sets()) as mc:
        mc.keep_on_device = True
        res = mc.run(dev._model(usac, "E"), polish=True)
        assert mc.last_mask is None
        got, pose, exp = _check_device(mc, "host")
        assert (got["iterations"][2:] >= 0).all() and got["used"][8] > 300
        assert got["used"].tolist() == pose["front"].tolist()
        assert (got["cost"][2:] < got["cost0"][2:]).all()  # the algebraic fit is not the geometric optimum
        pose_t = mc.export_pose(front_mask=True)
        fresh = mc.refine_pose(pose_t["R"], pose_t["t"], pose_t["front_mask"])  # fresh tensors: shapes and dtypes
        assert set(fresh) == set(KEYS)
        assert fresh["R"].dtype == torch.float32 and tuple(fresh["R"].shape) == (P, 3, 3) and fresh["R"].is_cuda
        assert fresh["t"].dtype == torch.float32 and tuple(fresh["t"].shape) == (P, 3)
        assert fresh["E"].dtype == torch.float32 and tuple(fresh["E"].shape) == (P, 3, 3)
        assert fresh["cost0"].dtype == torch.float64 and fresh["cost"].dtype == torch.float64
        assert fresh["iterations"].dtype == torch.int32 and fresh["used"].dtype == torch.int32
        _same(_np(fresh), got, "fresh tensors")
        wide = mc.export_pose(front_mask=True, n_max=1007)  # from the host: any width >= the largest problem
        _same(_np(mc.refine_pose(pose_t["R"], pose_t["t"], wide["front_mask"], n_max=1007)), got, "a wider mask")
        for iters in (0, 1, 50):
            a = _np(mc.refine_pose(pose_t["R"], pose_t["t"], pose_t["front_mask"], max_iters=iters))
            b = mc.refine(pose["R"], pose["t"], _packed(mc, pose["front_mask"].astype(np.uint8)), iters)
            _same(a, b, ("max_iters", iters))
        # a problem without a model: the zero matrix has no inlier.  Its pose is choice = -1; a start of the
        # caller's own is skipped as well, by the status
        starts = np.stack([r["polished"]["model"] for r in res]).reshape(P, 9).copy()
        starts[3] = 0.0
        mc.polish(starts, dev.THR["E"])
        status = [0, 0, 0, -111, 0, 0, 0, 0, 0, 0]
        got, pose, exp = _check_device(mc, "no model", status_of=status)
        assert got["iterations"][3] == -1 and pose["choice"][3] == -1
        _same(got["R"][3], np.eye(3, dtype=np.float32), "identity")
        _same(got["t"][3], np.zeros(3, dtype=np.float32), "zero")
        Rp, tp = _perturbed()
        got, _, _ = _check_device(mc, "no model, a start of the caller's", status_of=status, starts=(Rp, tp))
        assert got["iterations"][3] == -1 and got["cost"][3] == 0 and not got["E"][3].any()
        _same(got["R"][3], Rp[3], "the input's bits")
        _same(got["t"][3], tp[3], "the input's bits")
        assert (got["iterations"][[2, 4, 5, 6, 7, 8, 9]] >= 0).all()


def test_refine_pose_on_pixel_contexts(usac):
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
            got, pose, exp = _check_device(mc, what)
            assert (got["iterations"][2:] >= 0).all() and got["used"][8] > 300, (what, got["used"])
            assert got["used"].tolist() == pose["front"].tolist()
            if mc.n_max is not None:
                assert mc.n_max == N_MAX
                src = mc.source_index
                if mc.sorted_by_score:  # quality order: the mask is read through columns that do not ascend
                    assert any((np.diff(src[mc.offsets[p]:mc.offsets[p + 1]].astype(np.int64)) < 0).any() for p in range(P))


def test_in_place_repeatable_and_on_a_side_stream(usac, host):
    mc = host["mc"]
    Rp, tp = _perturbed()
    a = mc.refine(Rp, tp, host["mask"], 10)
    b = mc.refine(Rp, tp, host["mask"], 10)
    _same(a, b, "two identical calls")
    mc.run(dev._model(usac, "E"), polish=True)
    pose_t = mc.export_pose(front_mask=True)
    want = _refine_pose(mc, pose_t["R"], pose_t["t"], pose_t["front_mask"])
    # R and t aliased: the refinement in place
    R_io, t_io = pose_t["R"].clone(), pose_t["t"].clone()
    outs = _outs()
    outs["R"], outs["t"] = R_io, t_io
    got = mc.refine_pose(R_io, t_io, pose_t["front_mask"], out=outs)
    assert got["R"] is R_io and got["t"] is t_io
    _same(_np(got), want, "in place")
    assert not torch.equal(R_io, pose_t["R"])
    # on a side stream: torch's current stream, then the stream given by handle
    outs = _outs()
    torch.cuda.synchronize()  # the fill ran on the default stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = mc.refine_pose(pose_t["R"], pose_t["t"], pose_t["front_mask"], out=outs)
        total = got["iterations"].sum()  # queued behind the refinement on s
    s.synchronize()
    _same(_np(got), want, "side stream")
    assert int(total.item()) == int(want["iterations"].sum())
    outs = _outs()
    torch.cuda.synchronize()
    again = mc.refine_pose(pose_t["R"], pose_t["t"], pose_t["front_mask"], out=outs, stream=s.cuda_stream)
    s.synchronize()
    _same(_np(again), want, "the stream given by handle")


def test_refusals(usac, host):
    sets = _sets()
    Rp, tp = _perturbed()
    with usac.MultiContext.essential(sets) as mc:
        outs = _outs()
        R_t, t_t = torch.from_numpy(Rp).cuda(), torch.from_numpy(tp).cuda()
        mask_t = torch.ones((P, 1000), dtype=torch.uint8, device="cuda")

        def refused(code, word, mask=mask_t, **kw):
            with pytest.raises(usac.UsacError) as e:
                mc.refine_pose(R_t, t_t, mask, out=outs, **kw)
            assert e.value.code == code and word in str(e.value), str(e.value)
            for key, t in outs.items():
                assert (t.contiguous().view(torch.uint8).cpu().numpy() == 255).all(), "%s was written" % key

        refused(-3, "no polishing call has run")
        res = mc.run(dev._model(usac, "E"), polish=True)
        mc.refine_pose(R_t, t_t, mask_t)
        refused(-1, "n_max", mask=None, n_max=999)  # a context from the host: below the largest problem
        with pytest.raises(ValueError):
            mc.refine_pose(R_t, t_t, mask_t, max_iters=101)
        with pytest.raises(ValueError):
            mc.refine(Rp, tp, None, 101)
        with pytest.raises(ValueError):
            mc.refine(Rp, tp, np.zeros(7, dtype=np.uint8))
        # host memory: the Python layer refuses it by type, the library (asked directly) before any launch
        with pytest.raises(TypeError):
            mc.refine_pose(Rp, t_t)
        with pytest.raises(TypeError):
            mc.refine_pose(R_t, t_t, out={"R": np.zeros((P, 3, 3), np.float32)})
        L = usac.lib()
        ptrs = {k: outs[k].data_ptr() for k in outs}

        def direct(**kw):
            args = dict(n_max=1000, max_iters=10, R_in=R_t.data_ptr(), t_in=t_t.data_ptr(), mask_in=mask_t.data_ptr(), **ptrs)
            args.update(kw)
            o = usac._MultiRefineIO(**args)
            rc = L.usac_multi_refine_pose_device(mc._h, ctypes.byref(o))
            return rc, L.usac_multi_last_error(mc._h).decode()

        hostR = np.full((P, 36), 255, dtype=np.uint8)
        rc, msg = direct(R=hostR.ctypes.data)
        assert rc == -1 and "R is not device memory" in msg, msg
        assert (hostR == 255).all()
        rc, msg = direct(R_in=hostR.ctypes.data)
        assert rc == -1 and "R_in is not device memory" in msg, msg
        rc, msg = direct(cost=outs["cost"].data_ptr() + 4)
        assert rc == -1 and "cost is not aligned to 8 bytes" in msg, msg
        assert direct(max_iters=101)[0] == -1 and direct(R_in=None)[0] == -1 and direct(t_in=None)[0] == -1
        assert direct(**{k: None for k in ptrs})[0] == -1  # every output pointer is NULL
        assert L.usac_multi_refine_pose_device(mc._h, None) == -1
        assert direct(max_iters=100)[0] == 0
        for key, t in outs.items():
            outs[key].view(torch.uint8).fill_(255)
        for key, bad in (("R", _ff((P, 9), torch.float32, 255)), ("cost", _ff((P,), torch.float32, 255)),
                         ("used", _ff((P + 1,), torch.int32, 255))):
            with pytest.raises(ValueError):
                mc.refine_pose(R_t, t_t, mask_t, out={key: bad})
        with pytest.raises(ValueError):
            mc.refine_pose(R_t, t_t, torch.ones((P, 1001), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            mc.refine_pose(R_t, t_t, mask_t, out={"rotation": outs["R"]})
        models = np.stack([r["polished"]["model"] for r in res])
        mc.inliers(models, dev.THR["E"])
        refused(-3, "usac_multi_inliers")
        # refine() from host arrays needs no resident result, and its NULL arguments are refused
        _same(mc.refine(Rp, tp, None), host["mc"].refine(Rp, tp, None), "refine() without a resident result")
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
        it = np.zeros(P, dtype=np.int32)
        Rc, tc = np.ascontiguousarray(Rp), np.ascontiguousarray(tp)
        assert L.usac_multi_refine_pose(mc._h, None, tc.ctypes.data_as(fp), None, 10, None, None, None, None, None,
                                        it.ctypes.data_as(ip), None) == -1
        assert L.usac_multi_refine_pose(mc._h, Rc.ctypes.data_as(fp), tc.ctypes.data_as(fp), None, 10, None, None, None,
                                        None, None, None, None) == -1
        assert L.usac_multi_refine_pose(mc._h, Rc.ctypes.data_as(fp), tc.ctypes.data_as(fp), None, 101, None, None, None,
                                        None, None, it.ctypes.data_as(ip), None) == -1
        assert L.usac_multi_refine_pose(mc._h, Rc.ctypes.data_as(fp), tc.ctypes.data_as(fp), None, 10, None, None, None,
                                        None, None, it.ctypes.data_as(ip), None) == 0
    hsets = [synthetic.homography_points(n=n, inlier_ratio=0.7, seed=60 + n)[0].astype(np.float32) for n in (64, 65)]
    with usac.MultiContext(usac.ESTIMATOR.Homography, hsets) as hc:
        hc.run(dev._model(usac, "H"), polish=True)
        R2 = torch.zeros((2, 3, 3), dtype=torch.float32, device="cuda")
        t2 = torch.ones((2, 3), dtype=torch.float32, device="cuda")
        with pytest.raises(usac.UsacError) as e:
            hc.refine_pose(R2, t2)
        assert e.value.code == -3 and "essential" in str(e.value)
        with pytest.raises(usac.UsacError) as e:
            hc.refine(np.zeros((2, 9), dtype=np.float32), np.ones((2, 3), dtype=np.float32))
        assert e.value.code == -3 and "essential" in str(e.value)
