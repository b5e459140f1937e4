"""The multi-problem runs share one round loop and one staging helper (usac_api.cpp multi_run_driver,
pin_grow): what that can newly break is state leaking between modes on one context.  Every run of an
interleaved sequence of runs and hooks must equal, bit for bit, the same call made first on a fresh
context; the optional outputs may all be NULL; and a run refused by the shared checks leaves the
context as it was."""
import ctypes

import numpy as np
import pytest

from tests.helpers import multi_lo_ref as lo_ref
from tests.helpers import multi_sprt_ref as ref

pytestmark = pytest.mark.gpu

THR = ref.THR
M = ref.M
RUN_MAX, R = 512, 64


def _est(usac, kind):
    return usac.ESTIMATOR.Homography if kind == "H" else usac.ESTIMATOR.Fundamental


def _model(usac, kind, prosac, lo=False, sprt=False):
    sampler = usac.SAMPLER.Prosac if prosac else usac.SAMPLER.Uniform
    if lo:
        model = lo_ref.make_model(usac, kind, sampler=sampler)
    else:
        model = usac.Model(THR, M[kind], 0.95, 5, _est(usac, kind), sampler)
    model.max_iterations, model.batch, model.seed = RUN_MAX, R, 300
    model.setSprt(sprt)
    return model


def _same(a, b, what):
    """equal without tolerance: dicts key by key, lists item by item, floats and float arrays by bit pattern"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), (what, list(a), list(b))
        for k in a:
            _same(a[k], b[k], (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (what, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        kind = {4: np.int32, 8: np.int64}[a.dtype.itemsize] if a.dtype.kind == "f" else a.dtype
        np.testing.assert_array_equal(a.view(kind), b.view(kind), err_msg=str(what))
    elif isinstance(a, (float, np.floating)):
        assert type(a) is type(b) and ref.bits64(a) == ref.bits64(b), (what, a, b)
    else:
        assert type(a) is type(b) and a == b, (what, a, b)


@pytest.mark.parametrize("kind", ["H", "F"])
def test_interleaved_runs_equal_fresh_contexts(usac, kind):
    sets, _ = ref.sets(kind, sort=True, with_m=False)
    est, P, m = _est(usac, kind), len(sets), M[kind]

    def fresh(call):
        with usac.MultiContext(est, sets) as other:
            return call(other)

    runs = {
        1: lambda c: c.run_sprt(_model(usac, kind, True, sprt=True)),
        3: lambda c: c.run(_model(usac, kind, False)),
        5: lambda c: c.run_lo(_model(usac, kind, True, lo=True), polish=True),
        7: lambda c: c.run_prosac(_model(usac, kind, True)),
        8: lambda c: c.run_sprt(_model(usac, kind, False, sprt=True)),
        9: lambda c: c.run_lo(_model(usac, kind, False, lo=True)),
        10: lambda c: c.run(_model(usac, kind, False), polish=True),
    }
    with usac.MultiContext(est, sets) as mc:
        got = {}
        for step in range(1, 11):
            if step in runs:
                got[step] = runs[step](mc)
                assert len(got[step]) == P
                _same(got[step], fresh(runs[step]), (kind, "step", step))
            elif step == 2:  # the LO hook continues whatever LO state there is
                mc.lo(_model(usac, kind, False, lo=True), [g["best"] for g in got[1]], reset=False)
            elif step == 4:  # the scan hook raises the PROSAC state step 1 left (a problem without a model: identity)
                models = np.stack([g["best"]["model"] if g["best"]["valid"] else np.eye(3, dtype=np.float32).ravel()
                                   for g in got[3]])
                mc.prosac_scan(_model(usac, kind, True), models, [R] * P, [m] * P)
            elif step == 6:  # a smaller launch through the SPRT staging
                mc.hypothesize_score_sprt(R, seeds=[7, 8], thr=THR, problems=[4, 1])
    # the sequence did exercise the options
    assert any(g["scans"] > 0 for g in got[1]) and any(g["sprt"]["tests"] > 1 for g in got[8])
    assert any(g["lo"]["lo_calls"] > 0 for g in got[5]) and any(g["lo"]["lo_calls"] > 0 for g in got[9])
    assert "scans" in got[5][0] and "scans" not in got[8][0] and "scans" not in got[9][0]
    assert "polished" in got[5][0] and "polished" in got[10][0] and "polished" not in got[3][0]


def _outputs(out):
    return [{"best": o.best.as_dict(), "hypotheses": int(o.hypotheses), "rounds": int(o.rounds), "bound": int(o.bound),
             "status": int(o.status)} for o in out]


@pytest.mark.parametrize("prosac", [False, True])
def test_null_outputs(usac, prosac):
    sets, _ = ref.sets("H", sort=True, with_m=False)
    L, P = usac.lib(), len(sets)
    n_total = sum(len(s) for s in sets)
    with usac.MultiContext(usac.ESTIMATOR.Homography, sets) as mc:
        for name, own, model in (("usac_multi_run_lo", usac._MultiLoOutput, _model(usac, "H", prosac, lo=True)),
                                 ("usac_multi_run_sprt", usac._MultiSprtOutput, _model(usac, "H", prosac, sprt=True))):
            prm = usac._params(model)
            prm.seed = model.seed
            full, bare = (usac._MultiOutput * P)(), (usac._MultiOutput * P)()
            mask = np.zeros(n_total, dtype=np.uint8)
            rc = getattr(L, name)(mc._h, ctypes.byref(prm), None, full, (own * P)(), (usac._MultiProsacOutput * P)(),
                                  (usac._MultiPolishOutput * P)(), mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
            assert rc == 0, name
            assert getattr(L, name)(mc._h, ctypes.byref(prm), None, bare, None, None, None, None) == 0, name
            _same(_outputs(bare), _outputs(full), (name, prosac))
            assert any(o.rounds > 1 for o in full) and all(o.hypotheses > 0 for o in full)


def test_refused_run_leaves_the_context_alone(usac):
    sets, _ = ref.sets("H", sort=True, with_m=False)
    small = [sets[2], sets[2][:20]]  # n_p = 20: PROSAC needs more
    uniform = _model(usac, "H", False)
    with usac.MultiContext(usac.ESTIMATOR.Homography, small) as mc:
        for call, model in ((mc.run_prosac, _model(usac, "H", True)),
                            (mc.run_lo, _model(usac, "H", True, lo=True)),
                            (mc.run_sprt, _model(usac, "H", True, sprt=True))):
            with pytest.raises(usac.UsacError) as e:
                call(model)
            assert e.value.code == -1, call
        got = mc.run(uniform)
    with usac.MultiContext(usac.ESTIMATOR.Homography, small) as other:
        _same(got, other.run(uniform), "run after the refused runs")
