"""predict_var: posterior variance of the CSD and LFP predictions (gpcsd_predict_var; no reference counterpart).

The expected values come from `_helper` below: Qs, Qt, D from the oracle's eig_D, then

    M1 = Kcross^T Qs,  P_c = Qt^T k_c(t*, t)^T,  G = (M1 o M1) / D,  E_c = G (P_c o P_c),  E_sum = G (sum_c P_c)^2,
    var_c = prior_s sigma2_c - E_c,  var_sum = prior_s sum_c sigma2_c - E_sum,

with prior_s = 1 for the CSD and diag(compKphi) on a geometry whose electrodes are the sites for the LFP.  The CPU tests pin the helper
to the dense form prior - k^T (Ks (x) Kt + sig2n I)^-1 k.  The GPU tests print the maxima they observe; on an
MI355X: explained term at most 4.6e-13 of its largest entry (gate 1e-6), elementwise |var - ref| / ref at most 6.0e-9 (gate 1e-2) with
var / prior down to 9.0e-7; gpcsd_var_contract at most 0.47 of its rounding bound."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import cases as C
from helpers import load_model_case
from oracle import gpcsd_oracle as O

GATE = 1e-6                       # tests/test_hip_parity.py, on the explained term relative to its largest entry
ELEM = 1e-2                       # |var - ref| <= ELEM * ref, every element
CASES = ["1d_odd_17x37x5", "1d_siglist_12x40x4", "2d_grid_48x40x2"]      # C = 1, 2, 2; the second has a noise list
THREE = "1d_odd_three"            # 1d_odd with three built-in components (SE, Matern, SE): C + 1 = 4 planes
THREE_TEMPORAL = [(C.SE, 7.0, 0.6), (C.MATERN, 9.0, 1.1), (C.SE, 2.5, 0.3)]
MODELS = CASES + [THREE]
NAMES = ("csd", "lfp")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ NumPy reference
@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (case dict, oracle geometry, oracle hparams, Qs, Qt, D (nx, nt)); no jitter, as predict."""
    c, g, geom, hp, lfp = load_model_case(CASES[0] if name == THREE else name)
    if name == THREE:
        c = dict(c, temporal=THREE_TEMPORAL)
        hp = O.make_hparams(c["R"], c["ell_s"], THREE_TEMPORAL, c["sig2n"], eps=c["eps"], jitter=0.0)
    Qs, Qt, D = O.eig_D(O.spatial_kphi(geom, hp), O.temporal_sum(hp["temporal"], geom.t), hp["sig2n"])
    D = D.reshape(Qs.shape[0], Qt.shape[0])
    for a in (Qs, Qt, D):
        a.setflags(write=False)
    return c, geom, hp, Qs, Qt, D


def _site_geometry(geom, z):
    """The same quadrature rule with the sites as electrodes: its compKphi has the prior variance of the potential on its diagonal."""
    if geom.dim == 1:
        return O.Geometry1D(z, geom.t, a=geom.a, b=geom.b, ngl=geom.ngl)
    return O.Geometry2D(z, geom.t, a1=geom.a1, b1=geom.b1, a2=geom.a2, b2=geom.b2, ngl1=geom.ngl1, ngl2=geom.ngl2)


def _spatial(geom, hp, z):
    """{"csd" / "lfp": (Kcross (nx, nz), prior_s (nz))}"""
    z = np.asarray(z, dtype=np.float64)
    return {"csd": (O.spatial_kphig(geom, hp, z), np.ones(z.shape[0])),
            "lfp": (O.spatial_kphi(geom, hp, xp=z), np.diag(O.spatial_kphi(_site_geometry(geom, z), hp)).copy())}


def _grams(hp, geom, tstar):
    return [O.temporal_gram(kind, tstar, geom.t, ell, s2) for kind, ell, s2 in hp["temporal"]]          # (ntstar, nt) each


def _helper(name, z, tstar):
    """{"csd" / "lfp": {"prior": (C + 1, nz, 1) prior_s sigma2, "expl": (C + 1, nz, ntstar)}}; plane C = the component sum."""
    c, geom, hp, Qs, Qt, D = _case(name)
    P = [Qt.T @ k.T for k in _grams(hp, geom, tstar)]                          # (nt, ntstar)
    kd = [s2 for _, _, s2 in hp["temporal"]]
    out = {}
    for nm, (Kc, prior_s) in _spatial(geom, hp, z).items():
        M1 = Kc.T @ Qs
        G = (M1 * M1) @ (1.0 / D)                                                 # (nz, nt)
        expl = [G @ (p * p) for p in P] + [G @ (sum(P) ** 2)]
        prior = [prior_s[:, None] * k for k in kd] + [prior_s[:, None] * sum(kd)]
        out[nm] = {"prior": np.stack(prior), "expl": np.stack(expl)}
    return out


def _dense(name, z, tstar):
    """The same by the dense algebra: k^T (Ks (x) Kt + sig2n I)^-1 k through a Cholesky factor (scalar noise only)."""
    import scipy.linalg
    c, geom, hp, _, _, _ = _case(name)
    Ks, Kt = O.spatial_kphi(geom, hp), O.temporal_sum(hp["temporal"], geom.t)
    nx, nt = Ks.shape[0], Kt.shape[0]
    L = np.linalg.cholesky(O.mykron(Ks, Kt) + float(hp["sig2n"]) * np.eye(nx * nt))
    grams = _grams(hp, geom, tstar)
    out = {}
    for nm, (Kc, _) in _spatial(geom, hp, z).items():
        planes = []
        for k in grams + [sum(grams)]:
            kk = np.einsum("xz,ji->xizj", Kc, k).reshape(nx * nt, -1)          # column (z, j) = Kc[:, z] (x) k(t*_j, t)
            v = scipy.linalg.solve_triangular(L, kk, lower=True)
            planes.append(np.sum(v * v, axis=0).reshape(Kc.shape[1], -1))
        out[nm] = np.stack(planes)
    return out


def _offgrid(t, ntstar):
    """ntstar times off the training grid, spread over its span (as tests/test_predict_at.py)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    dt = t[1] - t[0]
    return (t[0] + 0.37 * dt + np.arange(ntstar) * (0.93 * (t[-1] - t[0]) / max(ntstar, 1))).reshape(-1, 1)


def _sites(x, nz):
    """nz sites: None = the electrodes; up to nx the first electrodes; beyond, sites interpolated between consecutive electrodes."""
    if nz is None:
        return x
    if nz <= x.shape[0]:
        return x[:nz]
    u = np.linspace(0.0, x.shape[0] - 1.0, nz)
    lo = np.minimum(np.floor(u).astype(int), x.shape[0] - 2)
    f = (u - lo)[:, None]
    return np.ascontiguousarray(x[lo] * (1.0 - f) + x[lo + 1] * f)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ["1d_odd_17x37x5", "2d_grid_48x40x2"])
def test_helper_equals_the_dense_form(name):
    c = _case(name)[0]
    z, tstar = _sites(c["x"], 5), _offgrid(c["t"], 7)
    got, ref = _helper(name, z, tstar), _dense(name, z, tstar)
    for nm in NAMES:
        err = float(np.max(np.abs(got[nm]["expl"] - ref[nm])) / np.max(np.abs(ref[nm])))
        print("helper vs dense %s %s: %.2e" % (name, nm, err))
        assert err < 1e-11
        assert np.all(got[nm]["prior"] - ref[nm] > 0)


def test_surface_exists_and_fails_loudly_without_a_gpu():
    import torch
    from gpcsd_amd import _hip
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    assert callable(getattr(GPCSD1D, "predict_var", None)) and callable(getattr(GPCSD2D, "predict_var", None))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read(), flags=re.S)
    for fn in ("gpcsd_predict_var", "gpcsd_predict_var_resident", "gpcsd_var_contract"):
        assert re.search(r"\b%s\s*\(" % fn, src), "%s is not declared" % fn
        assert fn in _hip.SIGNATURES
    if not torch.cuda.is_available():
        m = GPCSD1D(np.zeros((24, 50, 2)), np.linspace(0, 2300, 24)[:, None], np.arange(50.0)[:, None])
        with pytest.raises(_hip.HipUnavailable):
            m.predict_var(m.x, m.t, type="both")


class _UserCov:
    """A user-defined temporal covariance (any object with compute_Kt, covariances.py:235-238)."""

    def __init__(self, t):
        self.t = t

    def compute_Kt(self, t=None, tprime=None):
        a = np.asarray(self.t if t is None else t, dtype=np.float64).reshape(-1, 1)
        b = np.asarray(self.t if tprime is None else tprime, dtype=np.float64).reshape(1, -1)
        return 0.5 / (1.0 + (a - b) ** 2 / 9.0)


def test_validation_runs_before_any_device_call():
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE
    x, t = np.linspace(0, 2300, 24)[:, None], np.arange(50.0)[:, None]
    np.random.seed(0)
    m = GPCSD1D(np.zeros((24, 50, 2)), x, t, temporal_cov_list=[GPCSDTemporalCovSE(t), _UserCov(t)])
    with pytest.raises(NotImplementedError):
        m.predict_var(x, t)
    m = GPCSD1D(np.zeros((24, 50, 2)), x, t)
    with pytest.raises(ValueError):
        m.predict_var(x, t, type="variance")
    with pytest.raises(ValueError):
        m.predict_var(x, np.zeros((0, 1)))
    assert getattr(m, "_ctx", None) is None                                    # no context was opened on the way


# ------------------------------------------------------------------------------------------------ GPU: the kernel alone
def _contract_ref(G, P, C, prior_s, kd):
    """(out, magnitude) in longdouble; magnitude = sum_k G (sum_c |P_c|)^2 resp. G P_c^2, what the rounding bound scales with."""
    ld = np.longdouble
    G, prior_s, kd = G.astype(ld), prior_s.astype(ld), kd.astype(ld)
    nts = P.shape[1] // C
    Pc = [P[:, i * nts:(i + 1) * nts].astype(ld) for i in range(C)]
    out = [prior_s[:, None] * kd[i] - G @ (Pc[i] * Pc[i]) for i in range(C)] + [prior_s[:, None] * kd.sum() - G @ (sum(Pc) ** 2)]
    mag = [G @ (Pc[i] * Pc[i]) for i in range(C)] + [G @ (sum(np.abs(p) for p in Pc) ** 2)]
    return np.stack(out), np.stack(mag)


@pytest.mark.gpu
def test_var_contract_against_extended_precision():
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    rs = np.random.RandomState(20240607)
    worst = {"zero prior": 0.0, "prior": 0.0, "signed": 0.0}
    for K in (1, 17, 37, 64):
        for nz in (1, 5, 70):
            for nts in (1, 7, 64, 95):
                for ncomp in (1, 2, 3):
                    G = rs.uniform(0.0, 1.0, (nz, K))
                    P = rs.uniform(0.0, 1.0, (K, ncomp * nts))
                    prior_s, kd = rs.uniform(0.5, 2.0, nz), rs.uniform(0.2, 1.5, ncomp)
                    runs = (("zero prior", P, np.zeros(nz)), ("prior", P, prior_s), ("signed", P * rs.choice([-1.0, 1.0], P.shape), prior_s))
                    for tag, Pv, pr in runs:
                        got = ctx.var_contract(G, Pv, ncomp, pr, kd)
                        ref, mag = _contract_ref(G, Pv, ncomp, pr, kd)
                        assert got.shape == (ncomp + 1, nz, nts)
                        pk = np.abs(np.stack([pr[:, None] * k for k in list(kd) + [kd.sum()]]).astype(np.longdouble))
                        bound = (K + 2 * ncomp + 4) * U * mag + (2 * U * (pk + np.abs(ref)) if tag != "zero prior" else 0.0)
                        ratio = float(np.max(np.abs(got.astype(np.longdouble) - ref) / bound))
                        worst[tag] = max(worst[tag], ratio)
                        assert ratio <= 1.0, (tag, K, nz, nts, ncomp, ratio)
    print("var_contract: largest error / bound:", " ".join("%s %.3f" % kv for kv in worst.items()))


# ------------------------------------------------------------------------------------------------ GPU: the models
_MODELS = {}


def _model(name, lfp=None):
    """The mirrored Python class, configured as tests/test_hip_parity.py configures it; one per case for the module (lfp given: a
    fresh model with these trials instead)."""
    if lfp is None and name in _MODELS:
        return _MODELS[name]
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    c, geom, hp, _, _, _ = _case(name)
    np.random.seed(0)
    tcl = []
    for kind, ell, s2 in hp["temporal"]:
        tc = GPCSDTemporalCovSE(c["t"]) if kind == C.SE else GPCSDTemporalCovMatern(c["t"])
        tc.params["ell"]["value"] = ell
        tc.params["sigma2"]["value"] = float(s2)
        tcl.append(tc)
    data = C.case_lfp(c) if lfp is None else lfp
    if c["dim"] == 1:
        m = GPCSD1D(data, c["x"], c["t"], a=c["a"], b=c["b"], ngl=c["ngl"], temporal_cov_list=tcl)
        m.spatial_cov.params["ell"]["value"] = c["ell_s"][0]
    else:
        m = GPCSD2D(data, c["x"], c["t"], ngl1=c["ngl1"], ngl2=c["ngl2"], temporal_cov_list=tcl, eps=c["eps"])
        m.spatial_cov.params["ell1"]["value"] = c["ell_s"][0]
        m.spatial_cov.params["ell2"]["value"] = c["ell_s"][1]
    m.R["value"] = c["R"]
    m.sig2n["value"] = c["sig2n"]
    if lfp is None:
        _MODELS[name] = m
    return m


def _planes(m, nm):
    """(C + 1, nz, ntstar): the components, then the sum."""
    return np.stack([np.array(a) for a in getattr(m, nm + "_var_list")] + [np.array(getattr(m, nm + "_var"))])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_predict_var_vs_helper(name):
    m = _model(name)
    c = _case(name)[0]
    nt, ncomp = c["t"].shape[0], len(c["temporal"])
    combos = [(nz, nts, _offgrid(c["t"], nt if nts is None else nts)) for nz in (1, 5, None, 70) for nts in (1, 7, None, 95)]
    combos.append((None, None, c["t"]))                    # all electrodes x the training grid itself: the hardest cancellation
    worst_expl = worst_elem = 0.0
    least = np.inf
    for nz, nts, tstar in combos:
        z = _sites(c["x"], nz)
        m.predict_var(z, tstar, type="both")
        ref = _helper(name, z, tstar)
        assert np.array_equal(m.t_var, tstar) and np.array_equal(m.x_var, z)
        for nm in NAMES:
            assert len(getattr(m, nm + "_var_list")) == ncomp
            got = _planes(m, nm)
            assert got.shape == (ncomp + 1, z.shape[0], tstar.shape[0])
            rv = ref[nm]["prior"] - ref[nm]["expl"]
            e_expl = float(np.max(np.abs((ref[nm]["prior"] - got) - ref[nm]["expl"])) / np.max(np.abs(ref[nm]["expl"])))
            e_elem = float(np.max(np.abs(got - rv) / rv))
            worst_expl, worst_elem = max(worst_expl, e_expl), max(worst_elem, e_elem)
            least = min(least, float(np.min(rv / ref[nm]["prior"])))
            assert np.all(rv > 0)
            assert e_expl < GATE, (name, nm, nz, nts, e_expl)
            assert e_elem <= ELEM, (name, nm, nz, nts, e_elem)
    print("predict_var %s: explained term %.2e of its largest entry, elementwise |var - ref| / ref %.2e, least var / prior %.2e"
          % (name, worst_expl, worst_elem, least))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_one_type_gives_the_bits_of_both_and_resident_views_those_of_the_host(name):
    m = _model(name)
    c = _case(name)[0]
    ncomp = len(c["temporal"])
    z, tstar = _sites(c["x"], 5), _offgrid(c["t"], 23)
    m.predict_var(z, tstar, type="both")
    both = {nm: _planes(m, nm) for nm in NAMES}
    for nm in NAMES:
        m.predict_var(z, tstar, type=nm)
        assert np.array_equal(_planes(m, nm), both[nm])
    m.predict_var(z, tstar, type="both", resident=True)
    ctx = m._context()
    for nm in NAMES:
        v = getattr(m, nm + "_var")
        assert tuple(v.shape) == (5, 23) and hasattr(v, "__cuda_array_interface__")
        assert len(getattr(m, nm + "_var_list")) == ncomp and tuple(getattr(m, nm + "_var_list")[0].shape) == (5, 23)
        assert np.array_equal(ctx.fetch("pred_var_" + nm, (5, 23)), both[nm][ncomp])
        assert np.array_equal(ctx.fetch("pred_var_%s_list" % nm, (ncomp, 5, 23)), both[nm][:ncomp])


@pytest.mark.gpu
def test_the_variance_does_not_depend_on_the_trials_and_leaves_the_means_alone():
    name = "1d_siglist_12x40x4"
    c = _case(name)[0]
    z, tstar = _sites(c["x"], 70), _offgrid(c["t"], 23)
    a = _model(name)
    a.predict_at(z, tstar, type="both")
    means = {k: np.array(getattr(a, k)) for k in ("csd_pred", "lfp_pred", "t_pred", "x_pred")}
    means_list = [np.array(v) for v in a.csd_pred_list + a.lfp_pred_list]
    held = (a.csd_pred, a.lfp_pred, a.t_pred, a.x_pred)
    a.predict_var(z, tstar, type="both")
    assert all(x is y for x, y in zip(held, (a.csd_pred, a.lfp_pred, a.t_pred, a.x_pred)))
    for k, v in means.items():
        assert np.array_equal(np.array(getattr(a, k)), v)
    for got, v in zip(a.csd_pred_list + a.lfp_pred_list, means_list):
        assert np.array_equal(np.array(got), v)
    b = _model(name, lfp=C.synth_lfp(977, c["x"].shape[0], c["t"].shape[0], 7))       # another seed, 7 trials instead of 4
    b.predict_var(z, tstar, type="both")
    for nm in NAMES:
        assert np.array_equal(_planes(a, nm), _planes(b, nm))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1d_odd_17x37x5", "1d_siglist_12x40x4"])
def test_far_outside_the_training_span_the_variance_is_the_prior(name):
    """An end-to-end sign and prior check that shares nothing with the helper's algebra: ten length-scales (of the slowest
    component) past the end of the data a Matern-1/2 cross-covariance is exp(-10) sigma2, an SE one far less, so the explained
    part is below exp(-20) of the prior."""
    m = _model(name)
    c, geom, hp = _case(name)[:3]
    assert any(kind == C.MATERN for kind, _, _ in hp["temporal"])
    far = float(c["t"][-1, 0]) + 10.0 * max(ell for _, ell, _ in hp["temporal"])
    tstar = far + np.arange(5.0)[:, None]
    z = _sites(c["x"], 9)
    m.predict_var(z, tstar, type="both")
    kd = [s2 for _, _, s2 in hp["temporal"]]
    worst = 0.0
    for nm, (_, prior_s) in _spatial(geom, hp, z).items():
        got = _planes(m, nm)
        for p, k in enumerate(kd + [sum(kd)]):
            prior = prior_s[:, None] * k
            worst = max(worst, float(np.max(np.abs(got[p] - prior) / prior)))
            assert np.all(np.abs(got[p] - prior) <= 1e-6 * prior), (nm, p)
    print("predict_var far from the data %s: |var - prior| / prior %.2e" % (name, worst))


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
    out = np.empty((3, 4))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    call = lambda h, nts, typ, p=hp: lib.gpcsd_predict_var(h, ctypes.byref(p), dp(z), 3, dp(ts), nts, typ, None, dp(out), None, None)
    ref = _helper("1d_odd_17x37x5", z, ts.reshape(-1, 1))["csd"]
    assert call(ctx._h, 4, _hip.PRED_CSD) == 0
    assert np.max(np.abs(out - (ref["prior"][1] - ref["expl"][1]))) < GATE * np.max(ref["expl"])
    assert call(ctx._h, 0, _hip.PRED_CSD) == -3
    assert call(ctx._h, 4, 0) == -3
    assert lib.gpcsd_predict_var_resident(ctx._h, ctypes.byref(hp), dp(z), 3, dp(ts), 0, _hip.PRED_CSD) == -3
    # capacity: n_temporal * ntstar beyond one flat operand row; the check precedes every read of tstar (4 doubles here)
    assert call(ctx._h, 1 << 23, _hip.PRED_CSD) == _hip.ERR_CAPACITY
    assert lib.gpcsd_predict_var_resident(ctx._h, ctypes.byref(hp), dp(z), 3, dp(ts), 1 << 23, _hip.PRED_CSD) == _hip.ERR_CAPACITY
    # a user-defined temporal covariance is refused with a message
    host = _hip.HParams.from_buffer_copy(hp)
    host.kind[0] = _hip.KIND_HOST
    assert call(ctx._h, 4, _hip.PRED_CSD, host) == -3
    assert b"user-defined" in lib.gpcsd_last_error(ctx._h)
    # the context is as usable as before
    assert call(ctx._h, 4, _hip.PRED_CSD) == 0
    assert np.max(np.abs(out - (ref["prior"][1] - ref["expl"][1]))) < GATE * np.max(ref["expl"])
