"""The posterior calls at sites z and arbitrary times tstar -- predict_at, predict_var, predict_masked, predict_functionals,
sample_posterior -- and loo share one front (cached uploads "pred_z" / "pred_tstar") and scratch ("pred_B", "pred_S", "pred_Pc",
"proj_W").  Their values are pinned by the per-feature tests; what is pinned here is that the members of the family do not disturb
each other: no order of calls and no change of request on one context changes a bit, and the family answers bad requests alike.

Golden model 1d_odd_17x37x5, type "both", sites and times off the training grid."""
import ctypes

import numpy as np
import pytest

import test_predict_at as PA

NAME = "1d_odd_17x37x5"
ORDER = ("predict_at", "predict_var", "predict_masked", "predict_functionals", "sample_posterior", "loo")


def _request(nz, ntstar, first=0, shift=0.0):
    """nz sites between the electrodes and ntstar times off the training grid."""
    c = PA._case(NAME)[0]
    x = np.asarray(c["x"], dtype=np.float64)
    z = np.ascontiguousarray(x[first:first + nz] + 0.25 * (x[1] - x[0]))
    return z, np.ascontiguousarray(PA._offgrid(c["t"], ntstar).reshape(-1) + shift)


def _boxes(z, ts):
    """J = 3 box averages: two disjoint boxes and the whole field."""
    from gpcsd_amd.utility_functions import roi_weights
    nz, h = z.shape[0], ts.size // 2
    return roi_weights(z, ts, [list(range(nz // 2)), list(range(nz // 2, nz)), list(range(nz))],
                       [(ts[0], ts[h - 1]), (ts[h], ts[-1]), (ts[0], ts[-1])])


def _calls(m, ctx, z, ts):
    """name -> a function that makes the call on ctx and returns its host results as a dict of arrays."""
    from gpcsd_amd import _hip
    c = PA._case(NAME)[0]
    nx, nt, R = np.shape(m.lfp)
    hp, _k0 = m._hparams(0.0)                                            # the model of the predictions: no jitter
    hpj, _k1 = m._hparams(m.JITTER)                                      # the model of loglik, and so of loo
    both, nz, nts = _hip.PRED_BOTH, z.shape[0], ts.size
    W = _boxes(z, ts)
    sample = lambda: {k: v for k, v in ctx.sample_posterior(hp, z, ts, both, 2, 1, R).items() if v is not None}
    calls = {"predict_at": lambda: ctx.predict(hp, z, ts, both, (nz, nts, R), at=True),
             "predict_var": lambda: ctx.predict_var(hp, z, ts, both),
             "predict_masked": lambda: ctx.predict_masked(hp, np.ones((nx, nt), dtype=bool), z, ts, both, (nz, nts, R)),
             "predict_functionals": lambda: ctx.predict_functionals(hp, z, ts, W, both, R),
             "sample_posterior": sample,
             "loo": lambda: ctx.loo(hpj, (nx, nt, R)),
             "predict": lambda: ctx.predict(hp, c["x"], c["t"], both, (nx, nt, R))}
    calls["_keep"] = (_k0, _k1)                                          # (what the hyper-parameter structs point to)
    return calls


def _fresh_context(m):
    """A second context with the model's resident data; the model keeps its own."""
    own = (m._ctx, m._resident)
    m._ctx = None
    try:
        return m._sync_device()
    finally:
        m._ctx, m._resident = own


def _assert_same_bits(got, ref, tag):
    assert sorted(got) == sorted(ref), (tag, sorted(got), sorted(ref))
    for k in ref:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %s differs (max |diff| %.3e)" % (tag, k, np.max(np.abs(a - b)))


@pytest.mark.gpu
def test_the_order_of_calls_changes_no_bit():
    m = PA._model(NAME)
    ctx = m._sync_device()
    calls = _calls(m, ctx, *_request(5, 7))
    first = {name: calls[name]() for name in ORDER}
    for name in ORDER:
        assert all(np.all(np.isfinite(v)) for v in first[name].values()), name
    for name in reversed(ORDER):
        _assert_same_bits(calls[name](), first[name], name + " in reverse order")
    for name in ORDER:
        calls["predict"]()
        _assert_same_bits(calls[name](), first[name], name + " after predict")


@pytest.mark.gpu
def test_changed_sites_and_times_between_calls():
    m = PA._model(NAME)
    ctx = m._sync_device()
    other = _request(3, 4, first=6, shift=0.21)
    fresh = _calls(m, _fresh_context(m), *other)
    ref = {name: fresh[name]() for name in ORDER}
    before, after = _calls(m, ctx, *_request(5, 7)), _calls(m, ctx, *other)
    for name in ORDER:
        before[name]()
    for name in ORDER:
        _assert_same_bits(after[name](), ref[name], name + " after another request")
    for name in ORDER:                                                   # ... and directly behind its own earlier request
        before[name]()
        _assert_same_bits(after[name](), ref[name], name + " behind its own earlier request")


ENTRIES = ["predict_at", "predict_var", "predict_masked", "predict_functionals", "sample_posterior"]


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_return_codes_of_the_family(entry, resident):
    from gpcsd_amd import _hip
    m = PA._model(NAME)
    ctx = m._sync_device()
    lib = ctx._lib
    nx, nt, R = np.shape(m.lfp)
    hp, _keep = m._hparams(0.0)
    z, ts = _request(3, 4)                                               # 4 doubles: a capacity check that read tstar would run past them
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    mask = np.ones((nx, nt, 1), dtype=np.uint8)
    W = np.ascontiguousarray(_boxes(z, ts))
    J, C = W.shape[0], hp.n_temporal
    out = [np.empty(C * 3 * 4 * R * 2) for _ in range(12)]               # every host output of every entry fits
    o = [dp(a) for a in out]
    head = lambda h, nts, typ: (h, ctypes.byref(hp), dp(z), 3, dp(ts), nts, typ)
    if entry == "predict_masked":
        head = lambda h, nts, typ: (h, ctypes.byref(hp), mask.ctypes.data_as(ctypes.c_void_p), 1, dp(z), 3, dp(ts), nts, typ)
    tail = {"predict_at": ((1,), tuple(o[:4])), "predict_var": ((), tuple(o[:4])), "predict_masked": ((1,), tuple(o[:4])),
            "predict_functionals": ((), tuple(o)), "sample_posterior": ((2, 1, None, None), (2, 1, None, None) + tuple(o[:2]))}[entry]
    fn = getattr(lib, "gpcsd_" + entry + ("_resident" if resident else ""))

    def call(h, nts, typ):
        args = head(h, nts, typ)
        if entry == "predict_functionals":                               # (..., W, J, type, outputs)
            args = args[:-1] + (dp(W), J, typ)
        return fn(*(args + tail[1 if not resident else 0]))

    assert call(ctx._h, 4, _hip.PRED_BOTH) == 0                          # (the arguments are fine as they stand)
    assert call(ctx._h, 0, _hip.PRED_BOTH) == -3
    assert call(ctx._h, 4, 0) == -3
    fresh = _hip.Context()
    assert call(fresh._h, 4, _hip.PRED_BOTH) == -4                       # an LFP that was never set
    assert call(ctx._h, 1 << 23, _hip.PRED_BOTH) == _hip.ERR_CAPACITY    # refused before tstar is read
    assert call(ctx._h, 4, _hip.PRED_BOTH) == 0                          # the context is as usable as before
