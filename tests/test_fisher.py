"""Hyper-parameter uncertainty: per-trial scores and the expected Fisher information (gpcsd_trial_scores / gpcsd_fisher; no
reference counterpart).

The expected values are the dense statements of tests/fisher_ref.py.  The CPU tests pin that file without trusting its formulas:
its derivative matrices against central differences of the oracle's Gram matrices, the sum of its scores against the oracle's
gradient, its information against central differences of the expected score, d2lpdf against central differences of dlpdf.  The
GPU tests gate the device results at 1e-6 (the project's gate for every gradient component, tests/test_hip_fit2d.py): a score
relative to |quadratic part| + |trace part| of the reference (the score itself is a difference that may cancel), I_ij relative to
sqrt(I_ii I_jj).  Each test prints the maxima it observes; DESIGN.md 4.12 records them."""
import ctypes
import functools

import numpy as np
import pytest

import cases as C
import fisher_ref as F
from helpers import load_model_case
from oracle import gpcsd_oracle as O

GATE = 1e-6
FD_GATE = 1e-7                    # tests/test_oracle_golden.py: 4th-order central differences, h = 1e-3 in the log-parameter
IRREGULAR = "2d_irregular_20x30x3"
MODELS = ["1d_odd_17x37x5", "1d_wide_24x60x3", "2d_grid_48x40x2", IRREGULAR]


# ------------------------------------------------------------------------------------------------ cases
def _irregular():
    """20 irregular sites x 30 non-uniform times x 3 trials, no mirror symmetry in either grid (the full-size path); the
    hyper-parameters are those of the golden case 2d_grid_48x40x2."""
    c0, g0, _, hp0, _ = load_model_case("2d_grid_48x40x2")
    rs = np.random.RandomState(20302)
    x = np.stack([rs.uniform(0.0, 48.0, 20), rs.uniform(0.0, 440.0, 20)], axis=1)
    t = np.cumsum(rs.uniform(0.3, 0.9, 30))[:, None]
    lfp = rs.standard_normal((20, 30, 3))
    c = dict(c0, x=x, t=t)
    geom = O.Geometry2D(x, t, ngl1=c["ngl1"], ngl2=c["ngl2"])
    return c, geom, dict(hp0, jitter=float(g0["jitter"])), lfp


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (case dict, oracle geometry, oracle hparams WITH loglik's jitter, lfp)"""
    if name == IRREGULAR:
        c, geom, hp, lfp = _irregular()
    else:
        c, g, geom, hp, lfp = load_model_case(name)
        hp = dict(hp, jitter=float(g["jitter"]))
    lfp.setflags(write=False)
    return c, geom, hp, lfp


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The dense reference of the case's own trials, computed once and left unchanged."""
    c, geom, hp, lfp = _case(name)
    out = F.scores_and_info(geom, hp, lfp)
    for a in out.values():
        a.setflags(write=False)
    return out


def _small(dim):
    """Models with nx * nt <= 400 for the finite differences of the expected score: 1D 8 x 24 with an SE and a Matern component,
    2D 12 x 20 (a 3 x 4 grid of sites; the temporal variances offset the scale of the 2D forward model, as in the golden cases, so
    that K is conditioned well enough for finite differences of traces of its inverse)."""
    if dim == 1:
        geom = O.Geometry1D(np.linspace(0, 700, 8)[:, None], np.linspace(0, 46, 24)[:, None], a=0.0, b=700.0, ngl=30)
        return geom, O.make_hparams(90.0, (140.0,), [(O.SE, 7.0, 0.6), (O.MATERN, 4.0, 0.9)], 0.15, jitter=1e-8)
    geom = O.Geometry2D(C.grid_xy(3, 4, 0.0, 40.0, 0.0, 150.0), 0.5 * np.arange(20.0)[:, None], ngl1=6, ngl2=10)
    return geom, O.make_hparams(50.0, (25.0, 60.0), [(O.SE, 3.0, 0.8e-6), (O.MATERN, 2.0, 0.5e-6)], 0.1, eps=15.0, jitter=1e-8)


def _with_value(geom, hp, j, v):
    """hp with natural parameter j (slot order) set to v"""
    vals = F.values(geom, hp)
    vals[j] = v
    d = geom.dim
    temporal = [(k, vals[1 + d + 2 * i], vals[2 + d + 2 * i]) for i, (k, _, _) in enumerate(hp["temporal"])]
    return O.make_hparams(vals[0], vals[1:1 + d], temporal, vals[-1], eps=hp["eps"], jitter=hp["jitter"])


def _fd(f, geom, hp, j, h=1e-3):
    """d f / d theta_j by 4th-order central differences in log theta_j (the scheme of tests/test_oracle_golden.py)"""
    v = F.values(geom, hp)[j]
    at = lambda k: f(_with_value(geom, hp, j, v * np.exp(k * h)))
    return (8.0 * (at(1) - at(-1)) - (at(2) - at(-2))) / (12.0 * h) / v


def _score_err(S, ref):
    return float(np.max(np.abs(S - ref["scores"]) / (np.abs(ref["quad"]) + np.abs(ref["trace"])[None, :])))


def _info_err(I, Iref):
    d = np.sqrt(np.diag(Iref))
    return float(np.max(np.abs(I - Iref) / np.outer(d, d)))


# ------------------------------------------------------------------------------------------------ CPU: the reference is pinned
@pytest.mark.parametrize("name", ["1d_odd_17x37x5", "2d_grid_48x40x2"])
def test_ref_scores_sum_to_the_oracle_gradient(name):
    """(a) sum_r s_ref[r, i] v_i == oracle.loglik_and_grad's gradient in log-parameters.  Both are closed forms (dense solves against
    the eigen-form), so they agree to the conditioning of K, far inside the finite-difference gate."""
    c, geom, hp, lfp = _case(name)
    if name == "2d_grid_48x40x2":                # the dense side at 12 sites: the statement is the same, the solve 16 x smaller
        geom = O.Geometry2D(c["x"][::4], c["t"], a1=geom.a1, b1=geom.b1, a2=geom.a2, b2=geom.b2, ngl1=c["ngl1"], ngl2=c["ngl2"])
        lfp = lfp[::4]
    ref = F.scores_and_info(geom, hp, lfp)
    v = F.values(geom, hp)
    kinds = [k for k, _, _ in hp["temporal"]]
    tp = np.log(v / np.array([100.0] * (1 + geom.dim) + [1.0] * (2 * len(kinds) + 1)))
    _, grad = O.loglik_and_grad(geom, lfp, tp, kinds, 1, eps=hp["eps"], jitter=hp["jitter"])
    got = ref["scores"].sum(axis=0) * v
    scale = (np.abs(ref["quad"]).sum(axis=0) + lfp.shape[2] * np.abs(ref["trace"])) * v
    err = float(np.max(np.abs(got - grad) / scale))
    print("sum of reference scores vs oracle gradient %s: %.2e of |quad| + |trace|" % (name, err))
    assert err < FD_GATE


@pytest.mark.parametrize("dim", [1, 2])
def test_ref_derivative_matrices_vs_central_differences(dim):
    """(b) every dKs, dKt of the reference == central differences of oracle.spatial_kphi / temporal_sum"""
    geom, hp = _small(dim)
    _, dKs = F.spatial(geom, hp)
    _, dKt = F.temporal(geom, hp)
    worst = 0.0
    for j, d in enumerate(dKs):
        fd = _fd(lambda h: O.spatial_kphi(geom, h), geom, hp, j)
        worst = max(worst, float(np.max(np.abs(d - fd)) / np.max(np.abs(fd))))
    for j, d in enumerate(dKt):
        fd = _fd(lambda h: O.temporal_sum(h["temporal"], geom.t), geom, hp, 1 + dim + j)
        worst = max(worst, float(np.max(np.abs(d - fd)) / np.max(np.abs(fd))))
    print("derivative matrices vs central differences (%dD): %.2e" % (dim, worst))
    assert worst < FD_GATE


@pytest.mark.parametrize("dim", [1, 2])
def test_ref_information_vs_central_differences_of_the_expected_score(dim):
    """(c) -I_ref[i, j] == d/d theta_j of 1/2 tr(K^-1 d_i K K^-1 S) - 1/2 tr(K^-1 d_i K) with S = K(theta_0) held fixed"""
    geom, hp = _small(dim)
    assert geom.x.shape[0] * geom.t.shape[0] <= 400
    K0, _ = F.dense(geom, hp)
    info = F.scores_and_info(geom, hp, np.zeros((geom.x.shape[0], geom.t.shape[0], 1)))["info"]
    ng = info.shape[0]
    g0 = F.expected_score(K0, F.dense(geom, hp)[1], K0)           # the expected score vanishes at theta_0
    assert np.max(np.abs(g0) / np.sqrt(np.diag(info))) < 1e-3 * FD_GATE, g0
    worst = 0.0
    for j in range(ng):
        fd = _fd(lambda h: F.expected_score(*F.dense(geom, h), K0), geom, hp, j)
        worst = max(worst, float(np.max(np.abs(-info[:, j] - fd) / np.sqrt(np.diag(info) * info[j, j]))))
    print("information vs central differences of the expected score (%dD): %.2e of sqrt(I_ii I_jj)" % (dim, worst))
    assert worst < FD_GATE


@pytest.mark.parametrize("name", ["1d_odd_17x37x5", IRREGULAR])
def test_ref_eigen_form_equals_the_dense_statement(name):
    """The eigen-form restatement (the reference of the one GPU case whose dense K would have 11520 rows) against dense solves."""
    c, geom, hp, lfp = _case(name)
    dense, eig = F.scores_and_info(geom, hp, lfp), F.scores_and_info_eig(geom, hp, lfp)
    e_s, e_i = _score_err(eig["scores"], dense), _info_err(eig["info"], dense["info"])
    e_p = float(np.max(np.abs(eig["quad"] - dense["quad"]) / np.abs(dense["quad"])))
    e_t = float(np.max(np.abs(eig["trace"] - dense["trace"]) / np.abs(dense["trace"])))
    print("eigen-form vs dense %s: scores %.2e, quadratic parts %.2e, trace parts %.2e, information %.2e" % (name, e_s, e_p, e_t, e_i))
    assert max(e_s, e_p, e_t, e_i) < FD_GATE


def test_d2lpdf_vs_central_differences_of_dlpdf():
    """(d)"""
    from gpcsd_amd import priors as P
    ig = P.GPCSDInvGammaPrior()
    ig.set_params(1.2, 80.0)
    for pr in (ig, P.GPCSDHalfNormalPrior(0.1)):
        for v in (0.3, 5.0, 40.0):
            h = 1e-6 * v
            fd = (pr.dlpdf(v + h) - pr.dlpdf(v - h)) / (2 * h)
            assert np.isclose(pr.d2lpdf(v), fd, rtol=1e-6)
    with pytest.raises(NotImplementedError):
        P.GPCSDPrior().d2lpdf(1.0)


def test_surface_and_noise_list_without_a_gpu():
    """The symbols exist; a per-electrode noise list is refused before anything touches the device."""
    from gpcsd_amd import _hip
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.priors import GPCSDHalfNormalPrior
    lib = _hip.load_library()
    for n in ("gpcsd_fisher", "gpcsd_trial_scores", "gpcsd_trial_scores_resident"):
        assert hasattr(lib, n) and n in _hip.SIGNATURES
    np.random.seed(5)
    x, t = np.linspace(0, 2300, 24)[:, None], np.arange(50.0)[:, None]
    m = GPCSD1D(np.zeros((24, 50, 2)), x, t, sig2n_prior=[GPCSDHalfNormalPrior(0.1) for _ in range(24)])
    for call in (m.trial_scores, m.fisher_information, m.hyperparameter_cov):
        with pytest.raises(NotImplementedError):
            call()
    m1 = GPCSD1D(np.zeros((24, 50, 2)), x, t)
    assert m1.hyperparameter_names() == ["R", "spatial_ell", "temporal1_ell", "temporal1_sigma2", "temporal2_ell",
                                         "temporal2_sigma2", "sig2n"]
    for bad in (lambda: m1.fisher_information(kind="observed"), lambda: m1.hyperparameter_cov(kind="empirical")):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ GPU
_MODELS = {}


def _model(name, lfp=None):
    """The mirrored Python class at the case's hyper-parameters; one per case for the module (lfp given: a fresh model with
    these trials instead)."""
    if lfp is None and name in _MODELS:
        return _MODELS[name]
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    c, geom, hp, data = _case(name)
    np.random.seed(0)
    tcl = []
    for kind, ell, s2 in hp["temporal"]:
        tc = GPCSDTemporalCovSE(c["t"]) if kind == C.SE else GPCSDTemporalCovMatern(c["t"])
        tc.params["ell"]["value"] = ell
        tc.params["sigma2"]["value"] = float(s2)
        tcl.append(tc)
    data = np.array(data) if lfp is None else lfp
    if c["dim"] == 1:
        m = GPCSD1D(data, c["x"], c["t"], a=c["a"], b=c["b"], ngl=c["ngl"], temporal_cov_list=tcl)
        m.spatial_cov.params["ell"]["value"] = c["ell_s"][0]
    else:
        m = GPCSD2D(data, c["x"], c["t"], ngl1=c["ngl1"], ngl2=c["ngl2"], temporal_cov_list=tcl, eps=c["eps"])
        m.spatial_cov.params["ell1"]["value"] = c["ell_s"][0]
        m.spatial_cov.params["ell2"]["value"] = c["ell_s"][1]
    m.R["value"] = c["R"]
    m.sig2n["value"] = c["sig2n"]
    assert m.JITTER == hp["jitter"]
    if lfp is None:
        _MODELS[name] = m
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_scores_and_information_vs_dense(name):
    """Observed on an MI355X (scores / column sums against the gradient / information): see DESIGN.md 4.12."""
    m, ref = _model(name), _ref(name)
    R, ng = ref["scores"].shape
    S = m.trial_scores()
    I = m.fisher_information(log_params=False) / R          # the information of one trial
    assert S.shape == (R, ng) and I.shape == (ng, ng) and len(m.hyperparameter_names()) == ng
    e_s, e_i = _score_err(S, ref), _info_err(I, ref["info"])
    _, grad = m._loglik_and_grad_natural()
    scale = np.abs(ref["quad"]).sum(axis=0) + R * np.abs(ref["trace"])
    e_g = float(np.max(np.abs(S.sum(axis=0) - grad) / scale))
    print("fisher %s: scores %.2e, column sums vs gradient %.2e, information %.2e (gate %.0e)" % (name, e_s, e_g, e_i, GATE))
    assert e_s < GATE and e_i < GATE and e_g < GATE
    assert np.array_equal(I, I.T)
    assert np.array_equal(m.trial_scores(), S) and np.array_equal(m.fisher_information(log_params=False) / R, I)
    Il = m.fisher_information()
    assert np.array_equal(Il, Il.T)
    v = F.values(*_case(name)[1:3])
    assert np.allclose(Il, R * I * np.outer(v, v), rtol=1e-14, atol=0)
    assert np.array_equal(m.fisher_information(fix_R=True), Il[1:, 1:])
    Ie = m.fisher_information(kind="empirical", log_params=False)
    assert np.allclose(Ie, S.T @ S, rtol=1e-13, atol=1e-13 * np.max(np.abs(Ie))) and np.array_equal(Ie, Ie.T)


@pytest.mark.gpu
def test_more_than_one_tile_in_both_directions():
    """2d_npx_96x120x3: 96 electrodes are two tile rows of the spatial score product and 120 times two tile columns of the
    temporal one, so both second stages add partials of more than one tile; R nt = 360 is no multiple of 64.  Its dense K would
    have 11520 rows: the reference is the eigen-form restatement, pinned to the dense one on the CPU."""
    name = "2d_npx_96x120x3"
    c, geom, hp, lfp = _case(name)
    m, ref = _model(name), F.scores_and_info_eig(geom, hp, lfp)
    R = lfp.shape[2]
    S = m.trial_scores()
    I = m._sync_device().fisher(m._hparams(m.JITTER)[0], ref["info"].shape[0])
    e_s, e_i = _score_err(S, ref), _info_err(I, ref["info"])
    _, grad = m._loglik_and_grad_natural()
    e_g = float(np.max(np.abs(S.sum(axis=0) - grad) / (np.abs(ref["quad"]).sum(axis=0) + R * np.abs(ref["trace"]))))
    print("fisher %s: scores %.2e, column sums vs gradient %.2e, information %.2e (gate %.0e)" % (name, e_s, e_g, e_i, GATE))
    assert e_s < GATE and e_i < GATE and e_g < GATE
    assert np.array_equal(I, I.T) and np.array_equal(m.trial_scores(), S)
    m2 = _model(name, np.ascontiguousarray(lfp[:, :, :2]))
    assert np.array_equal(m2.trial_scores(), S[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_trials_alone_and_resident_same_bits(name):
    """Trials [0:2] uploaded alone give rows 0-1 of the full call bit for bit; resident=True leaves the host result's bits."""
    m = _model(name)
    S = m.trial_scores()
    lfp = _case(name)[3]
    m2 = _model(name, np.ascontiguousarray(lfp[:, :, :2]))
    assert np.array_equal(m2.trial_scores(), S[:2])
    view = m.trial_scores(resident=True)
    assert tuple(view.shape) == S.shape
    assert np.array_equal(m._context().fetch("trial_scores", S.shape), S)


@pytest.mark.gpu
def test_return_codes_and_a_context_without_data():
    from gpcsd_amd import _hip
    m = _model("1d_odd_17x37x5")
    hp, _keep = m._hparams(m.JITTER)
    ng = len(m.hyperparameter_names())
    I = m._sync_device().fisher(hp, ng)
    lib = _hip.load_library()
    ctx = _hip.Context()
    sc = m.spatial_cov
    ctx.set_geometry_1d(np.asarray(sc.x, dtype=np.float64).reshape(-1), np.asarray(sc.gl_x), np.asarray(sc.gl_w))
    ctx.set_time(m.temporal_cov_list[0].t)
    out = np.empty((5, ng))
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.gpcsd_trial_scores(ctx._h, ctypes.byref(hp), out.ctypes.data_as(dp), ng) == -4       # no resident data
    assert lib.gpcsd_trial_scores_resident(ctx._h, ctypes.byref(hp), ng) == -4
    assert np.array_equal(ctx.fisher(hp, ng), I)                                                    # ... which gpcsd_fisher does not need
    info = np.empty((ng, ng))
    assert lib.gpcsd_fisher(ctx._h, ctypes.byref(hp), info.ctypes.data_as(dp), ng + 1) == -3         # bad ng
    # a per-electrode noise list: -3 from the C calls
    ml = _model("1d_siglist_12x40x4")
    with pytest.raises(NotImplementedError):
        ml.trial_scores()
    cl = ml._sync_device()
    hpl, _keepl = ml._hparams(ml.JITTER)
    ngl = 1 + 1 + 2 * 2 + 1
    outl, infol = np.empty((4, ngl)), np.empty((ngl, ngl))
    assert lib.gpcsd_fisher(cl._h, ctypes.byref(hpl), infol.ctypes.data_as(dp), ngl) == -3
    assert lib.gpcsd_trial_scores(cl._h, ctypes.byref(hpl), outl.ctypes.data_as(dp), ngl) == -3


class _UserMatern:
    """A user-defined temporal covariance (not one of the library's kinds: GPCSD_KIND_HOST) that happens to be the Matern kernel, so
    that the dense reference of the case applies unchanged; its matrices come from host NumPy."""

    def __init__(self, t, ell, sigma2, with_derivatives=True):
        from gpcsd_amd.priors import GPCSDHalfNormalPrior, GPCSDInvGammaPrior
        self.t = t
        self.params = {"ell": {"value": ell, "prior": GPCSDInvGammaPrior(3.0, 20.0), "min": 1e-3, "max": 1e3},
                       "sigma2": {"value": sigma2, "prior": GPCSDHalfNormalPrior(1.0), "min": 0.0, "max": np.inf}}
        if with_derivatives:
            self.compute_dKt = self._compute_dKt

    def compute_Kt(self, t=None, tprime=None):
        t = self.t if t is None else t
        tprime = self.t if tprime is None else tprime
        return O.temporal_gram(O.MATERN, t, tprime, self.params["ell"]["value"], self.params["sigma2"]["value"])

    def _compute_dKt(self, name):
        ell, s2 = self.params["ell"]["value"], self.params["sigma2"]["value"]
        k = O.temporal_gram(O.MATERN, self.t, self.t, ell, 1.0)
        ts = np.asarray(self.t, dtype=np.float64).reshape(-1)
        return s2 * k * np.abs(ts[:, None] - ts[None, :]) / ell ** 2 if name == "ell" else k


@pytest.mark.gpu
def test_user_defined_temporal_covariance():
    """GPCSD_KIND_HOST with the derivative matrices of gpcsd_set_host_temporal_dgram is accepted as for the gradient (the caller's
    Gram is not folded: the full-size eigensolver path); without them: NotImplementedError, and -3 from the C calls."""
    from gpcsd_amd import _hip
    from gpcsd_amd.gpcsd1d import GPCSD1D
    name = "1d_odd_17x37x5"
    c, geom, hp, lfp = _case(name)
    ref = _ref(name)
    (_, ell, s2), = hp["temporal"]

    def build(with_derivatives):
        np.random.seed(0)
        m = GPCSD1D(np.array(lfp), c["x"], c["t"], a=c["a"], b=c["b"], ngl=c["ngl"],
                    temporal_cov_list=[_UserMatern(c["t"], ell, s2, with_derivatives)])
        m.spatial_cov.params["ell"]["value"], m.R["value"], m.sig2n["value"] = c["ell_s"][0], c["R"], c["sig2n"]
        return m
    m = build(True)
    S = m.trial_scores()
    I = m.fisher_information(log_params=False) / lfp.shape[2]
    e_s, e_i = _score_err(S, ref), _info_err(I, ref["info"])
    print("fisher %s, user-defined Matern: scores %.2e, information %.2e (gate %.0e)" % (name, e_s, e_i, GATE))
    assert e_s < GATE and e_i < GATE and np.array_equal(I, I.T)
    m0 = build(False)
    with pytest.raises(NotImplementedError):
        m0.trial_scores()
    ctx = m0._sync_device()
    hp0, _keep = m0._hparams(m0.JITTER)                  # hands over the Gram matrix, and no derivative matrices
    lib, dp = _hip.load_library(), ctypes.POINTER(ctypes.c_double)
    out, info = np.empty((lfp.shape[2], 5)), np.empty((5, 5))
    assert lib.gpcsd_trial_scores(ctx._h, ctypes.byref(hp0), out.ctypes.data_as(dp), 5) == -3
    assert lib.gpcsd_fisher(ctx._h, ctypes.byref(hp0), info.ctypes.data_as(dp), 5) == -3


def _prior_curvature(pr, v):
    """-(v^2 lp''(v) + v lp'(v)) from the priors' parameters (closed forms written here, not the package's d2lpdf)"""
    from gpcsd_amd import priors as P
    if isinstance(pr, P.GPCSDInvGammaPrior):
        d1, d2 = -(pr.alpha + 1.0) / v + pr.beta / v ** 2, (pr.alpha + 1.0) / v ** 2 - 2.0 * pr.beta / v ** 3
    else:
        d1, d2 = -v / pr.sd ** 2, -1.0 / pr.sd ** 2
    return -(v * v * d2 + v * d1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["expected", "sandwich"])
def test_hyperparameter_cov_vs_numpy_assembly(kind):
    name = "1d_odd_17x37x5"
    m, ref = _model(name), _ref(name)
    c, geom, hp, lfp = _case(name)
    R = lfp.shape[2]
    v = F.values(geom, hp)
    priors = [s[2] for s in m._param_slots()] + [m.sig2n["prior"]]
    H = R * ref["info"] * np.outer(v, v) + np.diag([_prior_curvature(pr, x) for pr, x in zip(priors, v)])
    St = ref["scores"] * v[None, :]
    for fix_R in (False, True):
        k = 1 if fix_R else 0
        Hi = np.linalg.inv(H[k:, k:])
        want = Hi if kind == "expected" else Hi @ (St[:, k:].T @ St[:, k:]) @ Hi
        res = m.hyperparameter_cov(kind=kind, fix_R=fix_R)
        d = np.sqrt(np.diag(want))
        err = float(np.max(np.abs(res["cov"] - want) / np.outer(d, d)))
        print("hyperparameter_cov %s fix_R=%s: %.2e of sqrt(c_ii c_jj), cond(H) %.1e" % (kind, fix_R, err, np.linalg.cond(H[k:, k:])))
        assert err < GATE
        assert res["names"] == m.hyperparameter_names()[k:] and np.array_equal(res["value"], v[k:])
        assert np.allclose(res["se"], np.sqrt(np.diag(res["cov"])))
        lo, hi = res["interval"][:, 0], res["interval"][:, 1]
        assert np.all(lo < v[k:]) and np.all(v[k:] < hi)
        assert np.allclose(np.log(hi / lo), 2 * 1.96 * res["se"])


@pytest.mark.gpu
def test_hyperparameter_cov_refuses_an_indefinite_curvature():
    """A prior whose curvature outweighs the information makes H indefinite: LinAlgError, not a covariance."""
    m = _model("1d_odd_17x37x5", np.array(_case("1d_odd_17x37x5")[3]))

    class Convex:
        def dlpdf(self, x):
            return 0.0

        def d2lpdf(self, x):
            return 1e12

    m.sig2n["prior"] = Convex()
    with pytest.raises(np.linalg.LinAlgError):
        m.hyperparameter_cov()
