"""predict_at: posterior means at arbitrary prediction times (gpcsd_predict_at; no reference counterpart).

The expected values come from `_helper` below -- InvY from the oracle's eig_D, then the cross Gram's TRAINING axis contracted --
which the CPU tests pin to the oracle's predict on the training grid (where Kt(t, t) is symmetric and the reference's axis quirk,
gpcsd1d.py:277-279, vanishes) and to its own restriction to a subset of times.  Tolerance everywhere: the project's parity gate."""
import ctypes
import functools

import numpy as np
import pytest

import cases as C
from helpers import load_model_case, relerr
from oracle import gpcsd_oracle as O

GATE = 1e-6                       # tests/test_hip_parity.py
CASES = ["1d_odd_17x37x5", "1d_siglist_12x40x4", "2d_grid_48x40x2"]      # R = 5, 4, 2; C = 1, 2, 2; the second has a noise list
NAMES = ("csd", "lfp")


# ------------------------------------------------------------------------------------------------ NumPy reference
def _invy(Ks, Kt, sig2n, lfp):
    """InvY_r = Qs [(Qs^T Y_r Qt) / D] Qt^T, (R, nx, nt)."""
    nx, nt, _ = lfp.shape
    Qs, Qt, D = O.eig_D(Ks, Kt, sig2n)
    B = np.matmul(np.matmul(Qs.T, np.moveaxis(lfp, 2, 0)), Qt) / D.reshape(1, nx, nt)
    return np.matmul(np.matmul(Qs, B), Qt.T)


@functools.lru_cache(maxsize=None)
def _case(name):
    c, g, geom, hp, lfp = load_model_case(name)
    InvY = _invy(O.spatial_kphi(geom, hp), O.temporal_sum(hp["temporal"], geom.t), hp["sig2n"], lfp)   # no jitter in predict
    InvY.setflags(write=False)
    return c, g, geom, hp, lfp, InvY


def _contract(geom, hp, InvY, z, grams):
    """out_c[z, j, r] = sum_{x,i} Kcross[x, z] InvY_r[x, i] grams[c][j, i]; grams[c] = k_c(t*, t) of shape (ntstar, nt)."""
    out = {}
    for nm, Kc in (("csd", O.spatial_kphig(geom, hp, z)), ("lfp", O.spatial_kphi(geom, hp, xp=z))):
        out[nm + "_list"] = [np.einsum("xz,rxi,ji->zjr", Kc, InvY, G) for G in grams]
        out[nm] = sum(out[nm + "_list"])
    return out


def _helper(name, z, tstar):
    c, g, geom, hp, lfp, InvY = _case(name)
    return _contract(geom, hp, InvY, np.asarray(z, dtype=np.float64),
                     [O.temporal_gram(kind, tstar, geom.t, ell, s2) for kind, ell, s2 in hp["temporal"]])


def _offgrid(t, ntstar):
    """ntstar times off the training grid, spread over its span."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    dt = t[1] - t[0]
    return (t[0] + 0.37 * dt + np.arange(ntstar) * (0.93 * (t[-1] - t[0]) / max(ntstar, 1))).reshape(-1, 1)


def _assert_matches(got, ref, ncomp, tag=""):
    for nm in NAMES:
        errs = [relerr(got[nm], ref[nm])] + [relerr(got[nm + "_list"][i], ref[nm + "_list"][i]) for i in range(ncomp)]
        print("predict_at %s %s relerr sum / components: %s" % (tag, nm, " ".join("%.2e" % e for e in errs)))
        assert len(got[nm + "_list"]) == ncomp
        assert max(errs) < GATE, (tag, nm, errs)


# ------------------------------------------------------------------------------------------------ CPU: the helper rests on the oracle
@pytest.mark.parametrize("name", CASES)
def test_helper_equals_oracle_predict_on_the_training_grid(name):
    c, g, geom, hp, lfp, _ = _case(name)
    ref = O.predict(geom, hp, lfp, c["x"], c["t"], "both")
    _assert_matches(_helper(name, c["x"], c["t"]), ref, len(c["temporal"]), name)


@pytest.mark.parametrize("name", CASES)
def test_helper_on_a_subset_of_times_is_the_subset_of_the_helper(name):
    c = _case(name)[0]
    nt = c["t"].shape[0]
    idx = np.array([nt - 2, 3, 17, 0, 11, 4, nt - 1])                    # non-contiguous, unsorted
    full = _helper(name, c["x"], c["t"])
    sub = {k: ([a[:, idx, :] for a in v] if isinstance(v, list) else v[:, idx, :]) for k, v in full.items()}
    _assert_matches(_helper(name, c["x"], c["t"][idx]), sub, len(c["temporal"]), name)


# ------------------------------------------------------------------------------------------------ GPU
_MODELS = {}


def _model(name):
    """The mirrored Python class, configured as tests/test_hip_parity.py configures it; one per case for the module."""
    if name in _MODELS:
        return _MODELS[name]
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    c, g, geom, hp, lfp, _ = _case(name)
    np.random.seed(0)
    tcl = []
    for (kind, ell, _), s2 in zip(c["temporal"], g["temporal_sigma2"]):
        tc = GPCSDTemporalCovSE(c["t"]) if kind == C.SE else GPCSDTemporalCovMatern(c["t"])
        tc.params["ell"]["value"] = ell
        tc.params["sigma2"]["value"] = float(s2)
        tcl.append(tc)
    if c["dim"] == 1:
        m = GPCSD1D(lfp, c["x"], c["t"], a=c["a"], b=c["b"], ngl=c["ngl"], temporal_cov_list=tcl)
        m.spatial_cov.params["ell"]["value"] = c["ell_s"][0]
    else:
        m = GPCSD2D(lfp, c["x"], c["t"], ngl1=c["ngl1"], ngl2=c["ngl2"], temporal_cov_list=tcl, eps=c["eps"])
        m.spatial_cov.params["ell1"]["value"] = c["ell_s"][0]
        m.spatial_cov.params["ell2"]["value"] = c["ell_s"][1]
    m.R["value"] = c["R"]
    m.sig2n["value"] = c["sig2n"]
    _MODELS[name] = m
    return m


def _results(m):
    return {"csd": np.array(m.csd_pred), "csd_list": [np.array(a) for a in m.csd_pred_list],
            "lfp": np.array(m.lfp_pred), "lfp_list": [np.array(a) for a in m.lfp_pred_list]}


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [1, 5, None])                             # None: every electrode site
@pytest.mark.parametrize("ntstar", [1, 7, None, 95])                     # None: nt values, none of them on the grid
@pytest.mark.parametrize("name", CASES)
def test_predict_at_off_grid_vs_helper(name, ntstar, nz):
    m = _model(name)
    c = _case(name)[0]
    z = c["x"] if nz is None else c["x"][:nz]
    tstar = _offgrid(c["t"], c["t"].shape[0] if ntstar is None else ntstar)
    m.predict_at(z, tstar, type="both")
    assert m.csd_pred.shape == (z.shape[0], tstar.shape[0], c["R_trials"]) and m.lfp_pred.shape == m.csd_pred.shape
    assert m.t_pred is tstar or np.array_equal(m.t_pred, tstar)
    _assert_matches(_results(m), _helper(name, z, tstar), len(c["temporal"]), "%s nts=%d nz=%d" % (name, tstar.shape[0], z.shape[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_predict_at_on_the_training_grid_is_predict(name):
    m = _model(name)
    c = _case(name)[0]
    ncomp = len(c["temporal"])
    for typ in ("csd", "lfp"):
        m.predict(c["x"], c["t"], type=typ)
        ref = (np.array(getattr(m, typ + "_pred")), [np.array(a) for a in getattr(m, typ + "_pred_list")])
        m.predict_at(c["x"], c["t"], type=typ)
        errs = [relerr(getattr(m, typ + "_pred"), ref[0])] + [relerr(getattr(m, typ + "_pred_list")[i], ref[1][i]) for i in range(ncomp)]
        print("predict_at(t) vs predict(t) %s %s: %s" % (name, typ, " ".join("%.2e" % e for e in errs)))
        assert max(errs) < GATE


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_predict_at_on_a_subset_is_the_subset_of_predict(name):
    m = _model(name)
    c = _case(name)[0]
    nt = c["t"].shape[0]
    idx = np.array([nt - 2, 3, 17, 0, 11, 4, nt - 1])
    m.predict(c["x"], c["t"], type="both")
    full = _results(m)
    sub = {k: ([a[:, idx, :] for a in v] if isinstance(v, list) else v[:, idx, :]) for k, v in full.items()}
    m.predict_at(c["x"], c["t"][idx], type="both")
    _assert_matches(_results(m), sub, len(c["temporal"]), name + " subset")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_equal_length_shifted_times_differ_from_predict(name):
    """predict keeps the reference's axis quirk, predict_at does not: at nt times that are not the training grid the two differ."""
    m = _model(name)
    c, g = _case(name)[:2]
    m.predict(g["z2"], g["tq"], type="both")
    quirk = _results(m)
    m.predict_at(g["z2"], g["tq"], type="both")
    got = _results(m)
    for nm in NAMES:
        d = relerr(quirk[nm], got[nm])
        print("predict vs predict_at at (z2, tq) %s %s: %.3e" % (name, nm, d))
        assert d > GATE * 100
    _assert_matches(got, _helper(name, g["z2"], g["tq"]), len(c["temporal"]), name + " tq")


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_resident_views_hold_the_host_results(name):
    """resident=True and the host form share one compute path (the same launches, then a copy or none): bit for bit."""
    m = _model(name)
    c = _case(name)[0]
    z, tstar = c["x"][:5], _offgrid(c["t"], 23)
    m.predict_at(z, tstar, type="both")
    host = _results(m)
    m.predict_at(z, tstar, type="both", resident=True)
    ctx = m._context()
    shape = (5, 23, c["R_trials"])
    assert tuple(m.csd_pred.shape) == shape and hasattr(m.csd_pred, "__cuda_array_interface__")
    for nm in NAMES:
        assert np.array_equal(ctx.fetch("pred_out_" + nm, shape), host[nm])
        lst = ctx.fetch("pred_out_%s_list" % nm, (len(c["temporal"]),) + shape)
        for i in range(len(c["temporal"])):
            assert np.array_equal(lst[i], host[nm + "_list"][i])


class _RationalQuadraticCov:
    """A user-defined temporal covariance: any object with compute_Kt is accepted (covariances.py:235-238); non-stationary."""

    def __init__(self, t, ell, sigma2, alpha=1.5, trend=0.004):
        self.t, self.ell, self.sigma2, self.alpha, self.trend = t, ell, sigma2, alpha, trend

    def compute_Kt(self, t=None, tprime=None):
        a = np.asarray(self.t if t is None else t, dtype=np.float64).reshape(-1, 1)
        b = np.asarray(self.t if tprime is None else tprime, dtype=np.float64).reshape(1, -1)
        k = self.sigma2 * (1.0 + (a - b) ** 2 / (2 * self.alpha * self.ell ** 2)) ** (-self.alpha)
        return k * (1.0 + self.trend * a) * (1.0 + self.trend * b)


@pytest.mark.gpu
def test_user_defined_temporal_covariance():
    """Three components (SE, user-defined, Matern): the caller's compute_Kt(tstar) per component, and more components than one
    launch of the last product carries."""
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    x = np.linspace(0, 2300, 24)[:, None]
    t = np.linspace(0, 59, 60)[:, None]
    lfp = C.synth_lfp(261, 24, 60, 3)
    np.random.seed(0)
    se, ma = GPCSDTemporalCovSE(t), GPCSDTemporalCovMatern(t)
    se.params["ell"]["value"], se.params["sigma2"]["value"] = 9.0, 0.6
    ma.params["ell"]["value"], ma.params["sigma2"]["value"] = 3.0, 0.3
    rq = _RationalQuadraticCov(t, 4.0, 0.5)
    m = GPCSD1D(lfp, x, t, a=0.0, b=2300.0, ngl=60, temporal_cov_list=[se, rq, ma])
    m.R["value"], m.sig2n["value"] = 110.0, 0.07
    m.spatial_cov.params["ell"]["value"] = 210.0
    geom = O.Geometry1D(x, t, a=0.0, b=2300.0, ngl=60)
    hp = O.make_hparams(110.0, (210.0,), [(O.SE, 9.0, 0.6), (O.MATERN, 3.0, 0.3)], 0.07)
    Kt = O.temporal_sum(hp["temporal"], t) + rq.compute_Kt()
    InvY = _invy(O.spatial_kphi(geom, hp), Kt, 0.07, lfp)
    z, tstar = np.linspace(100.0, 2200.0, 9)[:, None], _offgrid(t, 41)
    grams = [O.temporal_gram(O.SE, tstar, t, 9.0, 0.6), rq.compute_Kt(tstar), O.temporal_gram(O.MATERN, tstar, t, 3.0, 0.3)]
    m.predict_at(z, tstar, type="both")
    _assert_matches(_results(m), _contract(geom, hp, InvY, z, grams), 3, "user-defined")


@pytest.mark.gpu
def test_c_abi_argument_checks():
    from gpcsd_amd import _hip
    m = _model("1d_odd_17x37x5")
    c = _case("1d_odd_17x37x5")[0]
    ctx = m._sync_device()
    hp, _keep = m._hparams(0.0)
    lib = ctx._lib
    z = np.ascontiguousarray(c["x"][:3], dtype=np.float64)
    ts = np.ascontiguousarray(_offgrid(c["t"], 4).reshape(-1))
    out = np.empty((3, 4, c["R_trials"]))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    call = lambda h, nts, typ: lib.gpcsd_predict_at(h, ctypes.byref(hp), dp(z), 3, dp(ts), nts, typ, None, dp(out), None, None)
    assert call(ctx._h, 4, _hip.PRED_CSD) == 0                           # (the arguments are fine as they stand)
    assert relerr(out, _helper("1d_odd_17x37x5", z, ts)["csd"]) < GATE
    assert call(ctx._h, 0, _hip.PRED_CSD) == -3
    assert call(ctx._h, 4, 0) == -3
    assert lib.gpcsd_predict_at_resident(ctx._h, ctypes.byref(hp), dp(z), 3, dp(ts), 0, _hip.PRED_CSD, 1) == -3
    # capacity: ntrials * ntstar beyond one flat operand row; the check precedes every read of tstar (4 doubles here)
    assert call(ctx._h, 1 << 23, _hip.PRED_CSD) == _hip.ERR_CAPACITY
    assert lib.gpcsd_predict_at_resident(ctx._h, ctypes.byref(hp), dp(z), 3, dp(ts), 1 << 23, _hip.PRED_CSD, 1) == _hip.ERR_CAPACITY
    with pytest.raises(_hip.GPCSDCapacityError):
        ctx.predict_resident(hp, z, np.zeros(1 << 23), _hip.PRED_CSD, at=True)
    # an LFP that was never set
    fresh = _hip.Context()
    assert call(fresh._h, 4, _hip.PRED_CSD) == -4
    # the context is as usable as before
    assert call(ctx._h, 4, _hip.PRED_CSD) == 0
    assert relerr(out, _helper("1d_odd_17x37x5", z, ts)["csd"]) < GATE
