"""Device output of multi contexts (MultiContext.export_device / keep_on_device, usac_multi_export_device and
usac_multi_set_resident; ABI 27).  The yardstick is what the same polishing call returned to the host -- the result
dicts and the N_total mask bytes -- restated in numpy (tests/helpers/multi_export_ref.py): the mask scattered by
the context's source columns, the set rows' columns in packed order padded with -1.  Every comparison is exact
(floats by bit pattern), so there is no tolerance to choose.  Every output tensor is filled with 0xFF bytes before
every export: a cell the kernel does not write shows up (and, since a list entry of 0xFF bytes is the -1 of the
padding, the lists are also exported into zero-filled tensors).

The shapes are tests/test_gpu_multi_device.py's, the smallest at which the walk over the packed rows can go
wrong: `six` (n_max = 300, kept counts m, 64, 65, 256, 257, 300: below, at and above a wave and the 256-row block,
the smallest problem with all its rows in the last block of columns), `edges` (n_max = 512: the first block only,
the second block only, every second column) and `one` (P = 1); one problem of 16 385 points for the polish's host
path."""
import ctypes

import numpy as np
import pytest

from ransac_amd import synthetic
from tests.helpers import multi_export_ref as xref
from tests.helpers import multi_pixels_ref as pref
from tests.helpers.same_bits import same as _same

# before the library is loaded: torch brings its own HIP runtime, and a process holds one
torch = pytest.importorskip("torch")

from tests import test_gpu_multi_device as dev  # noqa: E402  (its fixtures' shapes and models)
from tests import test_gpu_multi_device_sorted as srt  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = dev.KINDS
KEYS = ("models", "inliers", "status", "mask", "inlier_cols", "pixel_models")


def _ff(shape, dtype, byte=255):
    """a device tensor of the shape and dtype whose every byte is `byte`"""
    size = torch.empty((), dtype=dtype).element_size()
    t = torch.full(tuple(shape[:-1]) + (shape[-1] * size,), byte, dtype=torch.uint8, device="cuda")
    return t.view(dtype)


def _outs(P, n_max, k=None, pixel=False, byte=255):
    o = {"models": _ff((P, 3, 3), torch.float32, byte), "inliers": _ff((P,), torch.int32, byte),
         "status": _ff((P,), torch.int32, byte), "mask": _ff((P, n_max), torch.uint8, byte)}
    if k is not None:
        o["inlier_cols"] = _ff((P, k), torch.int32, byte)
    if pixel:
        o["pixel_models"] = _ff((P, 3, 3), torch.float32, byte)
    return o


def _untouched(outs):
    for key, t in outs.items():
        raw = t.contiguous().view(torch.uint8).cpu().numpy()
        assert (raw == 255).all(), "%s was written by a refused export" % key


def _export(mc, k=None, pixel=False, n_max=None, byte=255, **kw):
    """export_device into 0xFF-filled tensors -> numpy arrays by key"""
    width = n_max if n_max is not None else (mc.n_max if mc.n_max is not None else int(mc.sizes.max()))
    outs = _outs(mc.P, width, k, pixel, byte)
    got = mc.export_device(inlier_cols=k, pixel_models=pixel, n_max=n_max, out=outs, **kw)
    assert set(got) == set(outs) and all(got[key] is outs[key] for key in outs)
    return {key: t.cpu().numpy() for key, t in got.items()}


def _source(mc):
    return None if mc.n_max is None else mc.source_index


def _check(mc, polished, host_mask, got, what, n_max=None):
    """an export against the polish dicts and the host mask of the same call"""
    P = mc.P
    width = got["mask"].shape[1]
    assert width == (n_max if n_max is not None else mc.n_max if mc.n_max is not None else int(mc.sizes.max()))
    _same(got["models"], np.stack([d["model"] for d in polished]).reshape(P, 3, 3), (what, "models"))
    _same(got["inliers"], np.array([d["inliers"] for d in polished], dtype=np.int32), (what, "inliers"))
    _same(got["status"], np.array([d["status"] for d in polished], dtype=np.int32), (what, "status"))
    _same(got["mask"], xref.padded_mask(host_mask, mc.offsets, _source(mc), width), (what, "mask"))
    if "inlier_cols" in got:
        k = got["inlier_cols"].shape[1]
        _same(got["inlier_cols"], xref.inlier_cols(host_mask, mc.offsets, _source(mc), k), (what, "inlier_cols"))
        kept = np.minimum(got["inliers"], k)
        for p in range(P):  # the count is the mask's, whole; the list holds min(count, k_max) columns
            assert got["inliers"][p] == int(got["mask"][p].sum())
            assert (got["inlier_cols"][p, :kept[p]] >= 0).all() and (got["inlier_cols"][p, kept[p]:] == -1).all()


class Ran:
    """a context from device tensors after run(polish=True): the result dicts and the host mask of that run"""

    def __init__(self, usac, kind, name):
        self.kind = kind
        self.case = dev._case(name, kind)
        self.mc = dev._from_device(usac, kind, self.case)
        self.model = dev._model(usac, kind)
        self.rerun()

    def rerun(self):
        self.res = self.mc.run(self.model, polish=True)
        self.polished = [r["polished"] for r in self.res]
        self.host_mask = self.mc.last_mask.copy()


@pytest.fixture(scope="module", params=KINDS)
def six(usac, request):
    w = Ran(usac, request.param, "six")
    yield w
    w.mc.close()


def test_six_equals_the_host_results(usac, six):
    w = six
    w.rerun()
    got = _export(w.mc, k=300)
    _check(w.mc, w.polished, w.host_mask, got, "six")
    zeros = _export(w.mc, k=300, byte=0)  # a list entry never written would keep its 0
    _same(zeros, got, "into zero-filled tensors")
    padded = w.mc.padded_mask()  # of the same run; its upload ends the resident result, so it comes last
    _same(got["mask"], padded.cpu().numpy().astype(np.uint8), "padded_mask()")
    assert not got["mask"].astype(bool)[~w.case["valid"]].any(), "a column that was not kept is set"
    assert max(d["inliers"] for d in w.polished) > 20
    fresh = None
    w.rerun()
    fresh = w.mc.export_device(inlier_cols=300)  # fresh tensors: the documented shapes and dtypes
    assert fresh["mask"].dtype == torch.bool and tuple(fresh["mask"].shape) == (6, 300) and fresh["mask"].is_cuda
    assert fresh["models"].dtype == torch.float32 and tuple(fresh["models"].shape) == (6, 3, 3)
    assert fresh["inliers"].dtype == torch.int32 and fresh["status"].dtype == torch.int32
    assert fresh["inlier_cols"].dtype == torch.int32 and tuple(fresh["inlier_cols"].shape) == (6, 300)
    _same(fresh["mask"].cpu().numpy().astype(np.uint8), got["mask"], "fresh mask")
    _same(fresh["inlier_cols"].cpu().numpy(), got["inlier_cols"], "fresh list")


@pytest.mark.parametrize("k", [1, 64, 65])
def test_truncated_lists(usac, six, k):
    w = six
    w.rerun()
    counts = [d["inliers"] for d in w.polished]
    assert max(counts) > 65 and min(counts) < 64, counts  # a row that is cut and one that is padded
    got = _export(w.mc, k=k)
    _check(w.mc, w.polished, w.host_mask, got, ("truncated", k))
    _same(got["inliers"], np.array(counts, dtype=np.int32), "the counts are never truncated")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["edges", "one"])
def test_edges_and_one(usac, name, kind):
    w = Ran(usac, kind, name)
    try:
        n_max = w.mc.n_max
        _check(w.mc, w.polished, w.host_mask, _export(w.mc, k=n_max), name)
        _check(w.mc, w.polished, w.host_mask, _export(w.mc), (name, "no list"))
    finally:
        w.mc.close()


def test_quality_order(usac):
    """unsorted columns with scores: the list follows source_index, every mask bit lands on its own column"""
    w = srt.World(usac, "H", True)
    try:
        model = srt._model(usac, "H", usac.SAMPLER.Prosac)
        res = w.mc.run_prosac(model, polish=True)
        host_mask = w.mc.last_mask.copy()
        got = _export(w.mc, k=w.n_max)
        _check(w.mc, [r["polished"] for r in res], host_mask, got, "sorted")
        _same(got["mask"].astype(bool), w.scatter(host_mask), "every bit on its original column")
        unsorted = 0
        for p in range(w.P):
            cols = got["inlier_cols"][p, :got["inliers"][p]]
            unsorted += int((np.diff(cols) < 0).any())
            _same(np.sort(cols), np.flatnonzero(got["mask"][p]).astype(np.int32), ("the same columns", p))
        assert unsorted > 0, "the fixture's quality order is ascending columns: it shows nothing"
    finally:
        w.close()


def test_other_polishing_entries(usac):
    S = usac.SAMPLER
    for kind in KINDS:
        case = dev._case("six", kind)
        big = case["valid"].sum(1) > 20  # PROSAC refuses the smallest problem
        case = {key: (v[big] if isinstance(v, np.ndarray) else v) for key, v in case.items()}
        with dev._from_device(usac, kind, case) as mc:
            calls = [("run_prosac", lambda: mc.run_prosac(dev._model(usac, kind, S.Prosac), polish=True))]
            if kind == "H":
                calls.append(("run_lo", lambda: mc.run_lo(dev._lo_model(usac, kind), polish=True)))
            if kind == "E":
                calls.append(("run_lo_essential", lambda: mc.run_lo_essential(dev._lo_model(usac, kind), polish=True)))
            for name, call in calls:
                res = call()
                _check(mc, [r["polished"] for r in res], mc.last_mask.copy(), _export(mc, k=300), (kind, name))
            starts = np.stack([r["best"]["model"] for r in res])
            pol = mc.polish(starts, dev.THR[kind], with_inliers=True)
            _check(mc, pol, mc.last_mask.copy(), _export(mc, k=300), (kind, "polish"))


def test_a_problem_without_a_model(usac):
    w = Ran(usac, "H", "six")
    try:
        starts = np.stack([d["model"] for d in w.polished]).reshape(6, 9).copy()
        starts[3] = 0.0  # the zero matrix maps every point to 0 / 0
        pts = dev._sets(w.case)[3].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            h = np.c_[pts[:, :2], np.ones(len(pts))] @ np.zeros((3, 3))
            err = ((h[:, :2] / h[:, 2:3] - pts[:, 2:]) ** 2).sum(1)
        assert not (err < dev.THR["H"]).any(), "the start model has inliers on the CPU"
        pol = w.mc.polish(starts, dev.THR["H"], with_inliers=True)
        got = _export(w.mc, k=300)
        _check(w.mc, pol, w.mc.last_mask.copy(), got, "no model")
        assert got["status"][3] == -111 and got["inliers"][3] == 0
        assert not got["mask"][3].any() and (got["inlier_cols"][3] == -1).all()
        _same(got["models"][3], starts[3].reshape(3, 3), "the start model's bits")
        assert (got["status"][[1, 2, 4, 5]] == 0).all() and (got["inliers"][[1, 2, 4, 5]] > 20).all()
    finally:
        w.mc.close()


PTS_MAX = 16384  # kPolPtsMax: a larger problem is polished through the host path


def test_a_deferred_problem(usac):
    sets = [synthetic.homography_points(n=n, inlier_ratio=r, seed=s)[0].astype(np.float32)
            for n, r, s in ((300, 0.7, 71), (PTS_MAX + 1, 0.5, 77), (65, 0.8, 72))]
    model = dev._model(usac, "H")
    with usac.MultiContext(usac.ESTIMATOR.Homography, sets) as mc:
        res = mc.run(model, polish=True)
        assert res[1]["polished"]["inliers"] > 4096  # the host path's problem has a result worth comparing
        got = _export(mc, k=PTS_MAX + 1)
        _check(mc, [r["polished"] for r in res], mc.last_mask.copy(), got, "deferred")
        for p, r in enumerate(res):  # a context from the host: a column is a local index
            _same(got["inlier_cols"][p, :len(r["inliers"])], r["inliers"], ("local indices", p))
        mc.keep_on_device = True  # the host path's mask goes up from a temporary
        kept = mc.run(model, polish=True)
        assert mc.keep_on_device and all("inliers" not in r for r in kept)
        _same(_export(mc, k=PTS_MAX + 1), got, "deferred, resident mode")


def test_resident_mode(usac, six):
    w = six
    w.rerun()
    want = _export(w.mc, k=300)
    w.mc.last_mask = None
    w.mc.keep_on_device = True
    try:
        assert w.mc.keep_on_device is True
        res = w.mc.run(w.model, polish=True)
        assert w.mc.last_mask is None and all("inliers" not in r for r in res)
        _same(res, w.res, "the run's dicts")
        _same(_export(w.mc, k=300), want, "run, resident mode")
        starts = np.stack([r["best"]["model"] for r in res])
        pol = w.mc.polish(starts, dev.THR[w.kind], with_inliers=True)
        assert w.mc.last_mask is None and all("inlier_idx" not in d for d in pol)
        _same(pol, w.polished, "polish from the run's models")
        _same(_export(w.mc, k=300), want, "polish, resident mode")
        w.mc.polish(starts, dev.THR[w.kind])  # no mask asked for: resident mode computes it all the same
        _same(_export(w.mc, k=300), want, "polish without inliers, resident mode")
    finally:
        w.mc.keep_on_device = False
    assert w.mc.keep_on_device is False
    again = w.mc.run(w.model, polish=True)
    _same(again, w.res, "turned off again")
    _same(w.mc.last_mask, w.host_mask, "the host mask is back")


@pytest.mark.parametrize("kind", KINDS)
def test_context_from_the_host(usac, kind):
    sets = dev._sets(dev._case("six", kind))
    widest = max(len(s) for s in sets)
    with dev._from_host(usac, kind, sets) as mc:
        res = mc.run(dev._model(usac, kind), polish=True)
        polished, host_mask = [r["polished"] for r in res], mc.last_mask.copy()
        for n_max in (None, widest, widest + 7):
            got = _export(mc, k=widest, n_max=n_max)
            _check(mc, polished, host_mask, got, ("host", n_max), n_max=widest if n_max is None else n_max)
            for p, r in enumerate(res):
                _same(got["inlier_cols"][p, :len(r["inliers"])], r["inliers"], ("local indices", p))
        outs = _outs(mc.P, widest - 1, widest)
        with pytest.raises(usac.UsacError) as e:
            mc.export_device(inlier_cols=widest, n_max=widest - 1, out=outs)
        assert e.value.code == -1 and "n_max" in str(e.value)
        _untouched(outs)


def test_pixel_models(usac):
    K1, K2 = pref.intrinsics()
    assert not (K1[:, 0, 0] == K1[0, 0, 0]).all() and not (K1 == K2).all()  # focal lengths differ per pair and view
    px = np.stack(pref.pixel_sets([300] * 6, K1, K2))
    rng = np.random.default_rng(5)
    valid = np.zeros((6, 300), dtype=bool)
    for p, k in enumerate(dev._six_sizes("E")):
        valid[p, np.sort(rng.permutation(300)[:k])] = True
    sets = [np.ascontiguousarray(r[v]) for r, v in zip(px, valid)]
    tols = [30.0, 35.0, 40.0, 45.0, 50.0, 55.0]
    model = dev._model(usac, "E")
    E = usac.ESTIMATOR
    with usac.MultiContext.from_padded(E.Essential, dev._dev(px), valid=dev._dev(valid), K1=K1, K2=K2) as mc, \
            usac.MultiContext.essential_pixels(sets, K1, K2) as plain:
        for ctx in (mc, plain):
            ctx.set_pixel_thresholds(tols)
            res = ctx.run(model, polish=True)
            host_mask = ctx.last_mask.copy()
            got = _export(ctx, k=300, pixel=True)
            _check(ctx, [r["polished"] for r in res], host_mask, got, "pixels")
            _same(got["pixel_models"], ctx.pixel_models(got["models"]), "pixel models")
            _same(got["pixel_models"], pref.pixel_models(got["models"], K1, K2), "the restatement's pixel models")
            again = _export(ctx, pixel=True)  # the intrinsics are on the device by now
            _same(again["pixel_models"], got["pixel_models"], "the second export")
        assert max(r["polished"]["inliers"] for r in res) > 20
    w = Ran(usac, "H", "one")
    try:
        outs = _outs(1, 300, pixel=True)
        with pytest.raises(usac.UsacError) as e:
            w.mc.export_device(pixel_models=True, out=outs)
        assert e.value.code == -3 and "intrinsics" in str(e.value)
        _untouched(outs)
    finally:
        w.mc.close()
    with usac.MultiContext.from_padded(E.Essential, dev._dev(px), valid=dev._dev(valid)) as mc:  # essential, but no K
        mc.run(model, polish=True)
        with pytest.raises(usac.UsacError) as e:
            mc.export_device(pixel_models=True)
        assert e.value.code == -3


def _refused(usac, mc, code, word, **kw):
    outs = _outs(mc.P, mc.n_max, 300)
    with pytest.raises(usac.UsacError) as e:
        mc.export_device(inlier_cols=300, out=outs, **kw)
    assert e.value.code == code and word in str(e.value), str(e.value)
    _untouched(outs)


def test_what_ends_the_resident_result(usac):
    kind = "H"
    case = dev._case("six", kind)
    model, thr = dev._model(usac, kind), dev.THR[kind]
    with dev._from_device(usac, kind, case) as mc:
        _refused(usac, mc, -3, "no polishing call has run")
        res = mc.run(model)  # a run without the polish is no polishing call
        _refused(usac, mc, -3, "no polishing call has run")
        models = np.stack([r["best"]["model"] for r in res])
        res = mc.run(model, polish=True)
        want = _export(mc, k=300)
        mc.inliers(models, thr)
        _refused(usac, mc, -3, "usac_multi_inliers")
        mc.run(model, polish=True)
        _same(_export(mc, k=300), want, "the next polishing call brings it back")
        other = np.zeros(int(mc.offsets[-1]), dtype=np.uint8)
        other[::3] = 1
        mc.padded_mask(other)
        _refused(usac, mc, -3, "usac_multi_padded_mask")
        mc.polish(models, thr, with_inliers=True)
        _export(mc, k=300)
        mc.polish(models, thr, with_inliers=False)  # resident mode off: no mask was computed
        _refused(usac, mc, -3, "computed no mask")
        with pytest.raises(usac.UsacError):  # a failed polishing call: PROSAC refuses the smallest problem
            mc.run_prosac(dev._model(usac, kind, usac.SAMPLER.Prosac), polish=True)
        _refused(usac, mc, -3, "computed no mask")  # refused for its arguments: it changed nothing
        mc.run(model, polish=True)
        _same(_export(mc, k=300), want, "and the next one succeeds")


def _room_behind(ptr):
    """bytes from ptr to the end of its allocation, as the HIP runtime this process holds reports them
    (hipMemGetAddressRange of the loaded library: what the library's own check reads)"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    for path in paths:
        base, size = ctypes.c_void_p(), ctypes.c_size_t()
        if ctypes.CDLL(path).hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(ptr)) == 0:
            return (base.value or 0) + size.value - ptr
    raise AssertionError("no loaded HIP runtime knows the pointer: %s" % paths)


class _Raw:
    """device memory at an address, as the Python layer looks at it"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3,
                                         "strides": None}


def test_refused_outputs(usac, six):
    w = six
    w.rerun()
    mc, P, n_max = w.mc, 6, 300
    want = _export(mc, k=300)
    # host memory: the Python layer refuses it by type, the library (asked directly) with -1
    outs = _outs(P, n_max, 300)
    with pytest.raises(TypeError):
        mc.export_device(inlier_cols=300, out=dict(outs, mask=np.zeros((P, n_max), np.uint8)))
    host = np.full((P, n_max), 255, dtype=np.uint8)
    o = usac._MultiDeviceOutput(n_max=n_max, k_max=300, mask=host.ctypes.data,
                                **{key: outs[key].data_ptr() for key in outs if key != "mask"})
    assert usac.lib().usac_multi_export_device(mc._h, ctypes.byref(o)) == -1
    msg = usac.lib().usac_multi_last_error(mc._h).decode()
    assert "mask" in msg and "not device memory" in msg, msg
    assert (host == 255).all()
    _untouched(outs)
    # one element short: the list ends one int32 before its allocation does.  An allocation of 16 MiB is one the
    # caching allocator asks the runtime for as it is; the test looks before it calls
    torch.cuda.empty_cache()
    block = torch.full((16 << 20,), 255, dtype=torch.uint8, device="cuda")
    need = P * 300 * 4
    short = block.data_ptr() + block.numel() - (need - 4)
    assert _room_behind(short) == need - 4, "the block is not an allocation of its own"
    outs = _outs(P, n_max, 300)
    with pytest.raises(usac.UsacError) as e:
        mc.export_device(inlier_cols=300, out=dict(outs, inlier_cols=_Raw(short, (P, 300), "<i4")))
    assert e.value.code == -1 and "inlier_cols" in str(e.value) and "room" in str(e.value), str(e.value)
    assert (block.cpu().numpy() == 255).all()
    _untouched(outs)
    # a float array that is not aligned to a float
    outs = _outs(P, n_max, 300)
    odd = _Raw(block.data_ptr() + 2, (P, 3, 3), "<f4")
    with pytest.raises(usac.UsacError) as e:
        mc.export_device(inlier_cols=300, out=dict(outs, models=odd))
    assert e.value.code == -1 and "models" in str(e.value) and "aligned" in str(e.value), str(e.value)
    assert (block.cpu().numpy() == 255).all()
    _untouched(outs)
    # the Python layer's own checks: a wrong shape or dtype never reaches the library
    for key, bad in (("mask", _ff((P, n_max + 1), torch.uint8)), ("inliers", _ff((P,), torch.float32)),
                     ("models", _ff((P, 9), torch.float32)), ("inlier_cols", _ff((P, 299), torch.int32))):
        with pytest.raises(ValueError):
            mc.export_device(inlier_cols=300, out={key: bad})
    with pytest.raises(ValueError):
        mc.export_device(out={"masks": outs["mask"]})
    with pytest.raises(usac.UsacError) as e:  # a context from device input takes its own width alone
        mc.export_device(n_max=n_max + 4)
    assert e.value.code == -1
    _same(_export(mc, k=300), want, "after the refusals")


def test_on_a_side_stream(usac, six):
    w = six
    w.rerun()
    want = _export(w.mc, k=300)
    outs = _outs(6, 300, 300)
    torch.cuda.synchronize()  # the fill ran on the default stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = w.mc.export_device(inlier_cols=300, out=outs)  # the default: torch's current stream, s
        counted = got["mask"].to(torch.int32).sum(1)  # queued behind the export on s
        listed = (got["inlier_cols"] >= 0).sum(1)
    s.synchronize()
    _same({key: t.cpu().numpy() for key, t in got.items()}, want, "side stream")
    _same(counted.cpu().numpy().astype(np.int32), want["inliers"], "the operation queued behind it")
    _same(listed.cpu().numpy().astype(np.int32), want["inliers"], "the list's length")
    outs = _outs(6, 300, 300)
    torch.cuda.synchronize()
    again = w.mc.export_device(inlier_cols=300, out=outs, stream=s.cuda_stream)
    s.synchronize()
    _same({key: t.cpu().numpy() for key, t in again.items()}, want, "the stream given by handle")
