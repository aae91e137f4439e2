"""GPU parity tests: the HIP path (through the C ABI, via the mirrored Python surface) against the golden
fixtures (outputs of the reference itself) and the CPU oracle on the same seeded inputs.

Tolerances (float64 throughout):
  * elementwise operators: 1e-13 relative (libm vs ocml transcendental ulps);
  * Gram contractions: 1e-11 relative to max|K| (different summation order);
  * loglik and posterior mean: 1e-6 relative, the gate BASELINE.json states; observed values are ~1e-10.
"""
import numpy as np
import pytest

import cases as C
from helpers import golden, load_model_case, relerr, with_jitter
from oracle import gpcsd_oracle as O

pytestmark = pytest.mark.gpu

GATE = 1e-6
MODEL_CASES = list(C.model_cases().keys())


@pytest.fixture(scope="module")
def ctx():
    from gpcsd_amd import _hip
    return _hip.default_context()


# ------------------------------------------------------------------------------------------------ operators
def test_b_fwd_ops():
    from gpcsd_amd import forward_models as F
    g = golden("ops")
    assert relerr(F.b_fwd_1d(g["bf1_r"], 100.0), g["bf1_out0"]) < 1e-13
    assert relerr(F.b_fwd_1d(g["bf1_r"], 37.5), g["bf1_out1"]) < 1e-13
    assert F.b_fwd_1d(g["bf1_r"], 100.0).shape == g["bf1_r"].shape
    assert relerr(F.b_fwd_2d(g["bf2_d1"], g["bf2_d2"], 100.0, 80.0), g["bf2_out_R100_e80"]) < 1e-13
    assert relerr(F.b_fwd_2d(g["bf2_d1"], g["bf2_d2"], 30.0, 5.0), g["bf2_out_R30_e5"]) < 1e-13
    assert relerr(F.b_fwd_2d(None, None, 100.0, 80.0, w=g["bf2_w"]), g["bf2_out_w"]) < 1e-13
    # broadcasting form used by fwd_model_2d: (nx1,1) x (1,nx2)
    d1 = np.linspace(-3, 3, 5)[:, None]
    d2 = np.linspace(-100, 100, 7)[None, :]
    assert relerr(F.b_fwd_2d(d1, d2, 60.0, 20.0), O.b_fwd_2d(d1, d2, 60.0, 20.0)) < 1e-13
    assert F.b_fwd_1d(np.zeros((0,)), 1.0).shape == (0,)


def test_fwd_models():
    from gpcsd_amd import forward_models as F
    g = golden("ops")
    assert relerr(F.fwd_model_1d(g["fm1_arr"], g["fm1_x"], g["fm1_z"], 150.0), g["fm1_out"]) < 1e-12
    assert relerr(F.fwd_model_2d(g["fm2_arr"], g["fm2_x1"], g["fm2_x2"], g["fm2_z"], 60.0, 20.0), g["fm2_out"]) < 1e-12


def test_traditional_csd_estimators_bitwise():
    """predictcsd_trad_1d / _2d (predict_csd.py:3-31) on the device: the reference's outputs bit for bit, the oracle at a
    cfg2-sized block, and the degenerate shapes."""
    from gpcsd_amd import predict_csd
    g = golden("trad_csd")
    np.testing.assert_array_equal(predict_csd.predictcsd_trad_1d(g["lfp1"]), g["csd1"])
    np.testing.assert_array_equal(predict_csd.predictcsd_trad_1d(g["lfp1e"]), g["csd1e"])
    np.testing.assert_array_equal(predict_csd.predictcsd_trad_2d(g["lfp2"]), g["csd2"])
    big = np.random.RandomState(3).standard_normal((24, 500, 200))
    np.testing.assert_array_equal(predict_csd.predictcsd_trad_1d(big), O.trad_csd_1d(big))
    assert predict_csd.predictcsd_trad_1d(np.zeros((0, 4, 2))).shape == (0, 4, 2)
    one = predict_csd.predictcsd_trad_2d(np.ones((3, 1, 4, 2)))
    assert one.shape == (3, 1, 4, 2) and np.all(np.isnan(one))
    with pytest.raises(ValueError):
        predict_csd.predictcsd_trad_1d(np.zeros((4, 5)))


def test_temporal_cov_classes():
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    g = golden("ops")
    np.random.seed(1)
    t, tp = g["kt_t"], g["kt_tp"]
    se = GPCSDTemporalCovSE(t)
    se.params["ell"]["value"], se.params["sigma2"]["value"] = 4.5, 1.7
    ma = GPCSDTemporalCovMatern(t)
    ma.params["ell"]["value"], ma.params["sigma2"]["value"] = 2.5, 0.6
    assert relerr(se.compute_Kt(), g["kt_se_default"]) < 1e-13
    assert relerr(se.compute_Kt(tp, t), g["kt_se_t_tp"]) < 1e-13
    assert relerr(se.compute_Kt(tprime=tp), g["kt_se_tp_only"]) < 1e-13
    assert relerr(ma.compute_Kt(), g["kt_ma_default"]) < 1e-13
    assert relerr(ma.compute_Kt(tp, t), g["kt_ma_t_tp"]) < 1e-13
    assert se.compute_Kt(tp, t).shape == (47, 61)


@pytest.mark.parametrize("tag,a,b,ngl", [("a", 0.0, 2300.0, 100), ("b", -200.0, 2600.0, 30)])
def test_spatial_cov_1d(tag, a, b, ngl):
    from gpcsd_amd.covariances import GPCSD1DSpatialCovSE
    g = golden("ops")
    np.random.seed(2)
    sc = GPCSD1DSpatialCovSE(g["s1_x"], a=a, b=b, ngl=ngl)
    sc.params["ell"]["value"] = 200.0
    assert np.array_equal(sc.gl_x, O.gauss_legendre(a, b, ngl)[0])
    assert relerr(sc.compute_Ks(), g["s1%s_Ks" % tag]) < 1e-13
    assert relerr(sc.compKphi_1d(100.0), g["s1%s_Kphi" % tag]) < 1e-11
    assert relerr(sc.compKphi_1d(100.0, xp=g["s1_xp"]), g["s1%s_Kphi_xp" % tag]) < 1e-11
    assert relerr(sc.compKphig_1d(g["s1_z"], 100.0), g["s1%s_Kphig" % tag]) < 1e-11


def test_spatial_cov_2d():
    from gpcsd_amd.covariances import GPCSD2DSpatialCovSE
    g = golden("ops")
    np.random.seed(2)
    sc = GPCSD2DSpatialCovSE(g["s2_x"], a1=0.0, b1=48.0, a2=0.0, b2=440.0, ngl1=10, ngl2=24)
    sc.params["ell1"]["value"], sc.params["ell2"]["value"] = 30.0, 100.0
    assert np.array_equal(sc.gl_x_grid, g["s2_gl_x_grid"])
    assert relerr(sc.gl_w_prod, g["s2_gl_w_prod"]) < 1e-15
    assert relerr(sc.compute_Ks(), g["s2_Ks"]) < 1e-13
    assert relerr(sc.compKphi_2d(60.0, 20.0), g["s2_Kphi"]) < 1e-11
    assert relerr(sc.compKphi_2d(60.0, 20.0, xp=g["s2_xp"]), g["s2_Kphi_xp"]) < 1e-11
    assert relerr(sc.compKphig_2d(g["s2_z"], 60.0, 20.0), g["s2_Kphig"]) < 1e-11
    sc.reset_x(g["s2_xp"])
    assert relerr(sc.compKphi_2d(60.0, 20.0), g["s2_Kphi_after_reset"]) < 1e-11


@pytest.mark.parametrize("shape", [(1, 1, 1), (16, 16, 4), (24, 500, 24), (37, 53, 41), (130, 70, 257), (384, 96, 1200),
                                   (300, 300, 300)])
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_f64_mfma(ctx, shape, ta, tb):
    """fp64 MFMA core against numpy on asymmetric random operands (catches row/col swaps), all transposes, tile edges."""
    M, N, K = shape
    rs = np.random.RandomState(M * 7 + N * 3 + K)
    A = rs.standard_normal((K, M) if ta else (M, K))
    B = rs.standard_normal((N, K) if tb else (K, N))
    ref = (A.T if ta else A) @ (B.T if tb else B)
    out = ctx.gemm(A, B, transA=ta, transB=tb)
    assert relerr(out, ref) < 1e-13 * max(1, K) ** 0.5


def _check_eigh(ctx, A, tol_scale=1.0):
    n = A.shape[0]
    w, V = ctx.eigh(A)
    wr = np.linalg.eigvalsh(A)
    nrm = max(np.max(np.abs(wr)), 1e-300)
    assert np.all(np.diff(w) >= 0)
    assert np.max(np.abs(w - wr)) / nrm < 1e-13 * n * tol_scale
    assert np.max(np.abs(V.T @ V - np.eye(n))) < 1e-13 * n * tol_scale
    assert np.max(np.abs(A @ V - V * w[None, :])) / nrm < 1e-13 * n * tol_scale
    return w, V


@pytest.mark.parametrize("n", [1, 2, 3, 9, 24, 33, 64, 65, 100, 257])
def test_eigh_random(ctx, n):
    rs = np.random.RandomState(n)
    M = rs.standard_normal((n, n))
    _check_eigh(ctx, (M + M.T) * 0.5)


def test_eigh_structured(ctx):
    """Clusters / rank deficiency / indefinite / diagonal inputs -- the shapes the GPCSD Grams actually have."""
    rs = np.random.RandomState(0)
    Q, _ = np.linalg.qr(rs.standard_normal((96, 96)))
    lam = np.concatenate([np.zeros(60), np.full(10, 1.0), np.linspace(2, 5, 20), [1e6] * 6])
    _check_eigh(ctx, (Q * lam) @ Q.T)                                # clusters + exact rank deficiency
    _check_eigh(ctx, np.diag(np.arange(40.0)[::-1]))                  # already diagonal, descending
    _check_eigh(ctx, -np.eye(17))                                     # negative definite, fully degenerate
    t = np.arange(120.0)[:, None]
    Kt = 0.5 * np.exp(-0.5 * (t - t.T) ** 2 / 400.0) + 0.7 * np.exp(-np.abs(t - t.T) / 5.0)
    _check_eigh(ctx, Kt)
    g = golden("ops")
    w, V = _check_eigh(ctx, g["eig_Ks"])
    assert relerr(w, g["eig_es"]) < 1e-13


def test_comp_eig_D():
    from gpcsd_amd.utility_functions import comp_eig_D
    g = golden("ops")
    Qs, Qt, D = comp_eig_D(g["eig_Ks"], g["eig_Kt"], 0.3)
    assert relerr(D, g["eig_D_scalar"]) < 1e-12
    assert relerr(Qs @ np.diag(g["eig_es"]) @ Qs.T, g["eig_Ks"]) < 1e-12
    assert relerr(Qt @ np.diag(g["eig_et"]) @ Qt.T, g["eig_Kt"]) < 1e-12
    assert relerr(comp_eig_D(g["eig_Ks"], g["eig_Kt"], g["eig_siglist"])[2], g["eig_D_list"]) < 1e-12


@pytest.mark.parametrize("n", [1, 5, 64, 65, 130, 255, 256, 257, 300, 513, 700, 1100])
def test_potrf_trsm_logdet(ctx, n):
    rs = np.random.RandomState(n)
    M = rs.standard_normal((n, n))
    A = M @ M.T + n * np.eye(n)
    L = ctx.potrf(A)
    Lr = np.linalg.cholesky(A)
    assert relerr(L, Lr) < 1e-12
    assert np.all(np.triu(L, 1) == 0.0)
    assert abs(ctx.logdet_chol(L) - np.linalg.slogdet(A)[1]) < 1e-10 * n
    B = rs.standard_normal((n, 7))
    X = ctx.trsm_lower(Lr, B)
    assert relerr(Lr @ X, B) < 1e-11


def test_potrf_not_positive_definite(ctx):
    A = np.eye(70)
    A[40, 40] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        ctx.potrf(A)


# ------------------------------------------------------------------------------------------------ models
def _build_model(name):
    """The mirrored Python class, configured like the golden generator configured the reference."""
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    c, g, geom, hp, lfp = load_model_case(name)
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
    return m, c, g, geom, hp, lfp


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_loglik_vs_reference_golden(name):
    m, c, g, geom, hp, lfp = _build_model(name)
    ll = m.loglik()
    ref = float(g["loglik"])
    assert abs(ll - ref) / abs(ref) < GATE
    # oracle on the same inputs agrees as well (and much tighter than the gate)
    llo = O.loglik(geom, with_jitter(hp, float(g["jitter"])), lfp)
    assert abs(ll - llo) / abs(llo) < 1e-8
    # Ks / Kt assembled by the operator surface match the reference's
    if c["dim"] == 1:
        Ks = m.spatial_cov.compKphi_1d(c["R"])
    else:
        Ks = m.spatial_cov.compKphi_2d(c["R"], c["eps"])
    assert relerr(np.diag(Ks), g["Ks_diag"]) < 1e-11
    assert relerr(Ks[0], g["Ks_row0"]) < 1e-11


@pytest.mark.parametrize("name", [n for n in MODEL_CASES if not C.model_cases()[n].get("loglik_only")])
def test_model_predict_vs_reference_golden(name):
    m, c, g, geom, hp, lfp = _build_model(name)
    m.predict(c["x"], c["t"], type="both")
    assert relerr(m.csd_pred, g["csd_pred"]) < GATE
    assert m.csd_pred.shape == (c["x"].shape[0], c["t"].shape[0], c["R_trials"])
    assert m.t_pred is not None and m.x_pred is not None
    if c.get("predict_light"):
        assert relerr(m.lfp_pred[:, :, :1], g["lfp_pred_trial0"]) < GATE
        return
    assert relerr(m.lfp_pred, g["lfp_pred"]) < GATE
    assert len(m.csd_pred_list) == len(c["temporal"])
    for i in range(len(c["temporal"])):
        assert relerr(m.csd_pred_list[i], g["csd_pred_%d" % i]) < GATE
        assert relerr(m.lfp_pred_list[i], g["lfp_pred_%d" % i]) < GATE
    m.predict(g["z2"], c["t"], type="csd")
    assert relerr(m.csd_pred, g["csd_pred_z2"]) < GATE
    m.predict(g["z2"], g["tq"], type="lfp")                      # t* != t, equal length: reference axis quirk
    assert relerr(m.lfp_pred, g["lfp_pred_z2_tq"]) < GATE
    with pytest.raises(ValueError):
        m.predict(g["z2"], c["t"][:-1], type="csd")


def test_sample_prior_vs_reference_golden():
    g = golden("sample_prior")
    m, c, *_ = _build_model("cfg1_1d_24x100x1")
    np.random.seed(77)
    out = m.sample_prior(3)
    assert relerr(out, g["sp1_csd"]) < 1e-9
    m, c, *_ = _build_model("2d_grid_48x40x2")
    csd, lfp = m.sample_prior(2, type="csd", seed=5)
    assert relerr(csd, g["sp2_csd"]) < 1e-9
    assert np.all(np.isnan(lfp))


def test_dense_cholesky_crosscheck(ctx):
    """Kronecker-eigen loglik == dense potrf/log-det/trsm loglik on the GPU (scalar sig2n), and both == oracle."""
    m, c, g, geom, hp, lfp = _build_model("1d_odd_17x37x5")
    Ks = O.spatial_kphi(geom, hp) + 1e-8 * np.eye(17)
    Kt = O.temporal_sum(hp["temporal"], geom.t)
    dense = ctx.loglik_dense_chol(Ks, Kt, c["sig2n"], lfp)
    ll = m.loglik()
    assert abs(dense - ll) / abs(ll) < 1e-9
    assert abs(dense - O.loglik_dense_cholesky(lfp, Ks, Kt, c["sig2n"])) / abs(ll) < 1e-9


def test_update_lfp_and_param_mutation():
    """Device state follows the Python-side mutation pattern of the reference scripts."""
    m, c, g, geom, hp, lfp = _build_model("1d_wide_24x60x3")
    ll0 = m.loglik()
    m.R["value"] = 90.0
    hp2 = dict(hp)
    hp2["R"] = 90.0
    ll1 = m.loglik()
    assert abs(ll1 - O.loglik(geom, with_jitter(hp2, 1e-8), lfp)) / abs(ll1) < 1e-8 and ll1 != ll0
    new = C.synth_lfp(99, 24, 60, 2)
    m.update_lfp(new, c["t"])
    ll2 = m.loglik()
    assert abs(ll2 - O.loglik(geom, with_jitter(hp2, 1e-8), new)) / abs(ll2) < 1e-8
    p = m.extract_model_params()
    m.R["value"] = 10.0
    m.restore_model_params(p)
    assert m.loglik() == ll2          # deterministic kernels: bit-identical re-evaluation


def test_full_size_properties_cfg3():
    """BASELINE cfg3 shape (384 x 500, reduced trials): size-independent properties of the hot path."""
    from gpcsd_amd import _hip
    m, c, g, geom, hp, lfp = _build_model("cfg3s_2d_384x500x2")
    ll = m.loglik()
    assert m.loglik() == ll                                           # run-to-run determinism
    # linearity of the posterior mean in the data: predict(a*Y) == a*predict(Y)
    z = c["x"][::16]
    m.predict(z, c["t"], type="csd")
    p1 = m.csd_pred.copy()
    m.update_lfp(2.5 * lfp, c["t"])
    m.predict(z, c["t"], type="csd")
    assert relerr(m.csd_pred, 2.5 * p1) < 1e-10
    # sum over components == total; trial independence: each trial alone gives the same prediction
    assert relerr(sum(m.csd_pred_list), m.csd_pred) < 1e-12
    m.update_lfp(lfp[:, :, 1:2].copy(), c["t"])
    m.predict(z, c["t"], type="csd")
    assert relerr(m.csd_pred[:, :, 0], p1[:, :, 1]) < 1e-9
    # quadratic term is additive over trials: ll(Y1 u Y2) - logdet part
    hp_c, keep = m._hparams(m.JITTER)
    s1, q1 = m._sync_device().loglik_parts(hp_c)
    m.update_lfp(lfp[:, :, 0:1].copy(), c["t"])
    s0, q0 = m._sync_device().loglik_parts(hp_c)
    m.update_lfp(lfp, c["t"])
    s, q = m._sync_device().loglik_parts(hp_c)
    assert s0 == s1 == s and abs((q0 + q1) - q) / abs(q) < 1e-12


# ------------------------------------------------------------------------------------------------ large-n eigensolver stages
def _house_Q(V, tau):
    n = V.shape[0]
    Q = np.eye(n)
    for k in range(n - 2):
        v = V[k]
        Q = Q - tau[k] * (Q @ v)[:, None] * v[None, :]          # Q H_k
    return Q


# 130: register block only; 193 / 250 / 255: LDS strip in front of it (odd and even tails, no per-column launches);
# 300: 44 per-column launches, then a full 256-row tail with a pending rank-2 update
@pytest.mark.parametrize("n", [3, 4, 17, 65, 130, 193, 250, 255, 300])
def test_sytrd_stage(ctx, n):
    rs = np.random.RandomState(n)
    M = rs.standard_normal((n, n))
    A = (M + M.T) * 0.5
    d, e, V, tau = ctx.debug_sytrd(A)
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    Q = _house_Q(V, tau)
    nrm = np.max(np.abs(A))
    assert np.max(np.abs(Q.T @ Q - np.eye(n))) < 1e-13 * n
    assert np.max(np.abs(Q.T @ A @ Q - T)) / nrm < 1e-13 * n
    for k in range(n - 2):
        assert np.all(V[k, :k + 1] == 0.0) and V[k, k + 1] != 0.0     # H_k = I - tau_k v_k v_k^T, v_k starts at k + 1


@pytest.mark.parametrize("n", [2, 5, 33, 64, 65, 100, 257, 500])
def test_stedc_stage_random(ctx, n):
    rs = np.random.RandomState(n)
    d, e = rs.standard_normal(n), rs.standard_normal(n - 1)
    w, Z = ctx.debug_stedc(d, e)
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    wr = np.linalg.eigvalsh(T)
    nrm = np.max(np.abs(wr))
    assert np.all(np.diff(w) >= 0)
    assert np.max(np.abs(w - wr)) / nrm < 1e-13 * n
    assert np.max(np.abs(Z.T @ Z - np.eye(n))) < 1e-13 * n
    assert np.max(np.abs(T @ Z - Z * w[None, :])) / nrm < 1e-13 * n


def test_stedc_stage_hard_cases(ctx):
    def run(d, e, tol=1e-13):
        n = len(d)
        w, Z = ctx.debug_stedc(d, e)
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        wr = np.linalg.eigvalsh(T)
        nrm = max(np.max(np.abs(wr)), 1e-300)
        assert np.max(np.abs(w - wr)) / nrm < tol * n
        assert np.max(np.abs(Z.T @ Z - np.eye(n))) < tol * n
        assert np.max(np.abs(T @ Z - Z * w[None, :])) / nrm < tol * n
    n = 201
    run(np.abs(np.arange(n) - 100.0), np.ones(n - 1))                # Wilkinson W201+: pairs of nearly equal eigenvalues
    e = np.zeros(99)
    e[::7] = 1e-9
    run(np.ones(100), e)                                             # near-identity, tiny couplings
    run(np.zeros(128), np.ones(127))                                 # Toeplitz (all-deflating symmetries)
    run(np.arange(70.0), np.zeros(69))                               # already diagonal
    run(np.full(90, 3.0), np.full(89, -0.5))                         # negative off-diagonals


@pytest.mark.parametrize("n", [1100, 1400, 2048, 2049, 4096])
def test_eigh_beyond_1024_rows(ctx, n):
    """Round 3: one eigenproblem may have up to GPCSD_MAX_EIG_N = 4096 rows (per-column tridiagonalisation launches with up to
    64 column chunks per thread, the merge set-up of the divide & conquer at 37 bytes of LDS per row, GEMM-chain
    back-transformation; the reference takes any n, utility_functions.py:58-59 -- 0.13 s here at 4096 rows).  A GP
    covariance (clustered, rank-deficient spectrum) and a random symmetric matrix against LAPACK: eigenvalues to n eps ||A||,
    orthogonality and residual to 1e-13 n."""
    rs = np.random.RandomState(n)
    tt = np.sort(rs.uniform(0, 0.4 * n, n))
    gp = 0.5 * np.exp(-0.5 * (tt[:, None] - tt[None, :]) ** 2 / 20.0 ** 2) + 0.7 * np.exp(-np.abs(tt[:, None] - tt[None, :]) / 5.0)
    B = rs.standard_normal((n, n))
    for A in (gp, 0.5 * (B + B.T)):
        w, Z = ctx.eigh(A)
        wr = np.linalg.eigvalsh(A)
        nrm = np.max(np.abs(wr))
        assert np.max(np.abs(w - wr)) < 4 * n * np.finfo(float).eps * nrm
        assert np.max(np.abs(Z.T @ Z - np.eye(n))) < 1e-13 * n
        assert np.max(np.abs(A @ Z - Z * w[None, :])) < 1e-13 * n * nrm
    with pytest.raises(RuntimeError):
        ctx.eigh(np.eye(4097))


@pytest.mark.parametrize("n", [100, 384, 500])
def test_eigh_gpcsd_shaped(ctx, n):
    """The actual Gram matrices of the hot path: numerically rank-deficient Ks, slowly decaying Kt."""
    t = 0.4 * np.arange(n)[:, None]
    Kt = 0.5 * np.exp(-0.5 * (t - t.T) ** 2 / 400.0) + 0.7 * np.exp(-np.abs(t - t.T) / 5.0)
    _check_eigh(ctx, Kt)
    x = C.neuropixels_xy(n)
    geom = O.Geometry2D(x, t, ngl1=10, ngl2=30)
    hp = O.make_hparams(100.0, (40.0, 150.0), [(O.SE, 20.0, 0.5)], 0.05, eps=80.0)
    Ks = O.spatial_kphi(geom, hp)
    w, V = _check_eigh(ctx, Ks + 1e-7 * np.eye(n))


@pytest.mark.parametrize("ns,nl", [(24, 100), (17, 130), (40, 96), (64, 65), (16, 250)])
def test_small_problem_rides_in_the_large_batch(ctx, ns, nl):
    """A small Gram matrix next to a large one goes through the batched sytrd/D&C pipeline (not Jacobi): check both
    decompositions of the pair at eigenvector level."""
    rs = np.random.RandomState(ns * 1000 + nl)
    def spd(n):
        X = rs.standard_normal((n, n + 3))
        return X @ X.T / n
    Ks, Kt = spd(ns), spd(nl)
    Qs, Qt, D = ctx.eig_D(Ks, Kt, 0.1)
    for K, Q in ((Ks, Qs), (Kt, Qt)):
        n = K.shape[0]
        w = np.linalg.eigvalsh(K)
        lam = np.einsum("ij,ij->j", Q, K @ Q)
        assert np.max(np.abs(Q.T @ Q - np.eye(n))) < 1e-13 * n
        assert np.max(np.abs(np.sort(lam) - w)) < 1e-13 * n * np.abs(w).max()
        assert np.max(np.abs(K @ Q - Q * lam[None, :])) < 1e-12 * n * np.abs(w).max()
    es, et = np.linalg.eigvalsh(Ks), np.linalg.eigvalsh(Kt)
    assert relerr(np.sort(D), np.sort(np.outer(es, et).ravel() + 0.1)) < 1e-12


def test_whitened_quadratic_forms(ctx):
    """N4: per-trial quadratic forms against cached (Qs, Qt, Dvec), the projection kernel reused by downstream objectives."""
    from gpcsd_amd.utility_functions import comp_eig_D, whitened_quadratic_forms
    g = golden("ops")
    Qs, Qt, D = comp_eig_D(g["eig_Ks"], g["eig_Kt"], 0.3)
    nx, nt = Qs.shape[0], Qt.shape[0]
    rs = np.random.RandomState(5)
    resid = rs.standard_normal((nx, nt, 7))
    got = whitened_quadratic_forms(Qs, Qt, D, resid)
    ref = np.array([np.sum((Qs.T @ resid[:, :, b] @ Qt).reshape(-1) ** 2 / D) for b in range(7)])
    assert relerr(got, ref) < 1e-12
    assert relerr(whitened_quadratic_forms(Qs, Qt, D, resid[:, :, 0]), ref[:1]) < 1e-12


# ------------------------------------------------------------------------------------------------ gradient + fit
@pytest.mark.parametrize("name", ["1d_wide_24x60x3", "cfg1_1d_24x100x1", "1d_odd_17x37x5", "2d_grid_48x40x2"])
def test_loglik_gradient_vs_finite_differences(name):
    """Analytic GPU gradient (replaces the reference's autograd tape) against central differences of the ORACLE's loglik
    in log-parameter space.  No executable reference gradient exists (autograd is not installed)."""
    m, c, g, geom, hp, lfp = _build_model(name)
    ll, g_nat = m._loglik_and_grad_natural()
    assert abs(ll - float(g["loglik"])) / abs(float(g["loglik"])) < GATE
    kinds = [k for k, _, _ in hp["temporal"]]
    vals = [c["R"]] + list(c["ell_s"]) + [v for (_, ell, s2) in hp["temporal"] for v in (ell, s2)] + [c["sig2n"]]
    scales = [100.0] * (1 + c["dim"]) + [1.0] * (2 * len(kinds) + 1)
    tp = np.log(np.array(vals) / np.array(scales))
    g_log = g_nat * np.array(vals)                                  # d/dlog(v) = v d/dv
    fd = O.loglik_grad_fd(geom, lfp, tp, kinds, 1, eps=c["eps"], jitter=float(g["jitter"]), h=1e-5)
    scale = np.max(np.abs(fd))
    assert np.max(np.abs(g_log - fd)) / scale < 2e-5, (g_log, fd)


@pytest.mark.parametrize("scale_t", [1.0, 1e-3])
def test_gradient_with_per_electrode_noise_list(scale_t):
    """sig2n given per electrode (utility_functions.py:54-63 indexes it by eigen-row, so the objective is not a function of
    Ks alone): one gradient entry per list element, and the spatial parameters pick up the eigenvector-rotation term.
    Checked against central differences of the oracle, also with signal and noise of comparable size (scale_t = 1e-3),
    where dropping that term is wrong by 3-30 %."""
    from gpcsd_amd.priors import GPCSDHalfNormalPrior
    m, c, g, geom, hp, lfp = _build_model("1d_siglist_12x40x4")
    sig = np.array(c["sig2n"]) if scale_t == 1.0 else np.linspace(0.01, 0.4, 12)
    m.sig2n = {"value": sig.copy(), "prior": [GPCSDHalfNormalPrior(0.1) for _ in range(12)],
               "min": [1e-8] * 12, "max": [0.5] * 12}
    for tc, (_, ell, s2) in zip(m.temporal_cov_list, hp["temporal"]):
        tc.params["sigma2"]["value"] = s2 * scale_t
    ll, g_nat = m._loglik_and_grad_natural()
    assert g_nat.shape == (1 + 1 + 2 * len(hp["temporal"]) + 12,)
    if scale_t == 1.0:
        assert abs(ll - float(g["loglik"])) / abs(float(g["loglik"])) < GATE
    kinds = [k for k, _, _ in hp["temporal"]]
    vals = np.concatenate([[c["R"]], list(c["ell_s"]), [v for (_, ell, s2) in hp["temporal"] for v in (ell, s2 * scale_t)], sig])
    scales = np.array([100.0] * 2 + [1.0] * (2 * len(kinds) + 12))
    tp = np.log(vals / scales)
    fd = O.loglik_grad_fd(geom, lfp, tp, kinds, 12, eps=c["eps"], jitter=float(g["jitter"]), h=1e-5)
    assert np.max(np.abs(g_nat * vals - fd)) / np.max(np.abs(fd)) < 1e-7, (g_nat * vals, fd)
    # objective gradient (log-parameters, priors included) agrees with central differences of the GPU objective
    ga = m._objective_grad(tp, False)
    m._use_analytic_grad = False
    gfd = m._objective_grad(tp, False)
    m._use_analytic_grad = True
    assert np.max(np.abs(ga - gfd)) / np.max(np.abs(gfd)) < 1e-4, (ga, gfd)


def test_fit_improves_objective_and_matches_cpu_optimiser():
    """fit(): L-BFGS-B on the GPU objective/gradient reaches the same optimum as SciPy on the oracle objective."""
    import scipy.optimize
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE
    rs = np.random.RandomState(3)
    x = np.linspace(0, 1100, 12)[:, None]
    t = np.linspace(0, 39, 40)[:, None]
    np.random.seed(4)
    gen = GPCSD1D(np.zeros((12, 40, 1)), x, t, a=0.0, b=1100.0, ngl=40, temporal_cov_list=[GPCSDTemporalCovSE(t)])
    gen.R["value"], gen.sig2n["value"] = 120.0, 0.05
    gen.spatial_cov.params["ell"]["value"] = 180.0
    gen.temporal_cov_list[0].params["ell"]["value"], gen.temporal_cov_list[0].params["sigma2"]["value"] = 5.0, 1.0
    geom = O.Geometry1D(x, t, a=0.0, b=1100.0, ngl=40)
    hp_true = O.make_hparams(120.0, (180.0,), [(O.SE, 5.0, 1.0)], 0.05, jitter=1e-8)
    Ks = O.spatial_kphi(geom, hp_true)
    Kt = O.temporal_sum(hp_true["temporal"], t)
    es, Qs = np.linalg.eigh(Ks)
    et, Qt = np.linalg.eigh(Kt)
    Ls, Lt = Qs * np.sqrt(np.maximum(es, 0)), Qt * np.sqrt(np.maximum(et, 0))
    Y = np.stack([Ls @ rs.standard_normal((12, 40)) @ Lt.T for _ in range(6)], axis=2)
    Y = Y / Y.std() + 0.2 * rs.standard_normal(Y.shape)
    m = GPCSD1D(Y, x, t, a=0.0, b=1100.0, ngl=40, temporal_cov_list=[GPCSDTemporalCovSE(t)])
    start = np.log(np.array([100.0 / 100, 150.0 / 100, 4.0, 0.8, 0.1]))
    nll0 = m._objective(start, False)
    m.fit(n_restarts=1, starts=[start], options={"maxiter": 60, "disp": False, "gtol": 1e-6, "ftol": 1e-12})
    nll_fit = float(m.fit_nll_values_[0])
    assert nll_fit < nll0 - 1.0
    assert m.R["min"] <= m.R["value"] <= m.R["max"]

    def cpu_obj(tp):
        hp = O.hparams_from_tparams(tp, 1, [O.SE], 1, jitter=1e-8)
        lp = (m.R["prior"].lpdf(hp["R"]) + m.spatial_cov.params["ell"]["prior"].lpdf(hp["ell_s"][0])
              + m.temporal_cov_list[0].params["ell"]["prior"].lpdf(hp["temporal"][0][1])
              + m.temporal_cov_list[0].params["sigma2"]["prior"].lpdf(hp["temporal"][0][2])
              + m.sig2n["prior"].lpdf(hp["sig2n"]))
        return -(O.loglik(geom, hp, Y) + lp)
    assert abs(cpu_obj(start) - nll0) / abs(nll0) < 1e-8
    res = scipy.optimize.minimize(cpu_obj, start, method="L-BFGS-B", bounds=m._bounds(),
                                  options={"maxiter": 60, "gtol": 1e-6, "ftol": 1e-12})
    assert abs(res.fun - nll_fit) / abs(res.fun) < 1e-4


def test_fit_concurrent_restarts_match_sequential():
    """fit(workers=k): restarts run concurrently on one GPU, each on its own context / stream, and give the same optima
    as the sequential loop (deterministic kernels, starts drawn up front)."""
    m1, c, g, geom, hp, lfp = _build_model("1d_odd_17x37x5")
    m2, *_ = _build_model("1d_odd_17x37x5")
    np.random.seed(11)
    starts = [m1._sample_start(False) for _ in range(4)]
    opts = {"maxiter": 25, "disp": False, "gtol": 1e-5, "ftol": 1e7 * np.finfo(float).eps}
    m1.fit(n_restarts=4, options=opts, starts=starts, workers=1, batch=1)
    m2.fit(n_restarts=4, options=opts, starts=starts, workers=3, batch=1)
    assert np.allclose(m1.fit_nll_values_, m2.fit_nll_values_, rtol=1e-10, atol=0)
    assert abs(m1.R["value"] - m2.R["value"]) <= 1e-9 * abs(m1.R["value"])
    assert abs(m1.loglik() - m2.loglik()) <= 1e-9 * abs(m1.loglik())


# ------------------------------------------------------------------------------------------------ folded-basis GEMMs
# both sides fold (2D probes with > 64 sites) or only the temporal one (GPCSD1D: 24 electrodes go through Jacobi)
FOLD_CASES = [n for n in MODEL_CASES if (C.model_cases()[n]["x"].shape[0] > 64 or C.model_cases()[n]["t"].shape[0] > 64)
              and np.ndim(C.model_cases()[n]["sig2n"]) == 0]


@pytest.mark.parametrize("name", FOLD_CASES)
def test_folded_gemm_path_matches_unfolded(name):
    """Mirror-symmetric grids: loglik / predict run their projections as half-size GEMMs in the symmetric/antisymmetric
    basis.  Same numbers as the full-size path (and as the reference's goldens), and the folded path is the one taken."""
    m, c, g, geom, hp, lfp = _build_model(name)
    ctx = m._context()
    n0 = ctx.fold_gemm(True)
    ll_f = float(m.loglik())
    assert ctx.fold_gemm() == n0 + 1, "grids are symmetric: the folded path must be taken"
    pred_both = not c.get("loglik_only")
    if pred_both:
        m.predict(c["x"], c["t"], type="both")
        assert ctx.fold_gemm() == n0 + 2
        csd_f, lfp_f = m.csd_pred.copy(), m.lfp_pred.copy()
        lists_f = [a.copy() for a in m.csd_pred_list]
    n1 = ctx.fold_gemm(False)
    ll_u = float(m.loglik())
    assert ctx.fold_gemm() == n1
    assert abs(ll_f - ll_u) / abs(ll_u) < 1e-11
    assert abs(ll_f - float(g["loglik"])) / abs(float(g["loglik"])) < GATE
    if pred_both:
        m.predict(c["x"], c["t"], type="both")
        assert relerr(csd_f, m.csd_pred) < 1e-10 and relerr(lfp_f, m.lfp_pred) < 1e-10
        for a, b in zip(lists_f, m.csd_pred_list):
            assert relerr(a, b) < 1e-10
        assert relerr(csd_f, g["csd_pred"]) < GATE
    ctx.fold_gemm(True)


def test_folded_gemm_falls_back_when_symmetry_is_missing():
    """Prediction times other than the training grid, or a per-electrode noise list (indexed by eigen-rank in the reference),
    take the full-size path; prediction sites without the electrodes' mirror symmetry keep the folded TEMPORAL side and
    unfold only the spatial one (round 4); results agree with the full-size path."""
    name = "2d_npx_96x120x3"                                          # both sides folded: both output grids are constrained
    m, c, g, geom, hp, lfp = _build_model(name)
    ctx = m._context()
    ctx.fold_gemm(True)
    x, t = c["x"], c["t"]
    z_asym = np.array(x[: x.shape[0] - 3], dtype=np.float64)          # drop three sites: no longer mirror-symmetric
    n0 = ctx.fold_gemm()
    m.predict(z_asym, t, type="csd")
    assert ctx.fold_gemm() == n0 + 1                                  # folded in time, full-size in space
    p_asym = m.csd_pred.copy()
    m.predict(x, t, type="csd")
    assert ctx.fold_gemm() == n0 + 2
    assert relerr(p_asym, m.csd_pred[: z_asym.shape[0]]) < 1e-10      # same sites, either path
    ctx.fold_gemm(False)
    m.predict(z_asym, t, type="csd")
    assert relerr(p_asym, m.csd_pred) < 1e-10                         # and against the full-size path on the same sites
    ctx.fold_gemm(True)
    n0 += 1
    t_shift = t + 0.37 * (t[1] - t[0])
    m.predict(x, t_shift, type="csd")
    assert ctx.fold_gemm() == n0 + 1
    p_shift = m.csd_pred.copy()
    ctx.fold_gemm(False)
    m.predict(x, t_shift, type="csd")
    assert relerr(p_shift, m.csd_pred) < 1e-12
    ctx.fold_gemm(True)
    # a mirror-symmetric set of sites that is NOT the electrode grid folds as well
    z_sym = np.concatenate([x[:5], x[-5:]]) if c["dim"] == 1 else None
    if z_sym is not None:
        n1 = ctx.fold_gemm()
        m.predict(z_sym, t, type="csd")
        assert ctx.fold_gemm() == n1 + 1
    m.sig2n["value"] = list(np.full(x.shape[0], float(c["sig2n"])) * np.linspace(0.5, 1.5, x.shape[0]))
    n2 = ctx.fold_gemm()
    ll = float(m.loglik())
    assert ctx.fold_gemm() == n2 and np.isfinite(ll)


@pytest.mark.parametrize("ncomp,R", [(2, 3), (1, 21), (3, 5)])
def test_folded_gemm_1d_odd_sizes_vs_oracle(ncomp, R):
    """GPCSD1D with an odd number of electrodes and time points (fixed points of both reflections, ns != na), folded path
    against the oracle: loglik, predictions at the electrodes and at a symmetric subset of sites.  One and two temporal
    components go through the fused last product (unfold in its epilogue; partial tiles in every dimension: 36 / 35 time
    orbits, 41 / 40 site orbits, 3 or 21 trials), three through the GEMM + relayout pair with padded column blocks.  The fold,
    unfold and relayout kernels themselves are checked tightly, entry by entry against long double, in tests/test_fold_kernels.py."""
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    rs = np.random.RandomState(5)
    nx, nt = 81, 71
    x = np.linspace(0.0, 2400.0, nx).reshape(-1, 1)
    t = np.linspace(0.0, 70.0, nt).reshape(-1, 1)
    lfp = rs.standard_normal((nx, nt, R))
    spec = [(C.SE, 9.0, 0.8), (C.MATERN, 4.0, 0.3), (C.SE, 2.5, 0.2)][:ncomp]
    tcl = []
    for kind, ell, s2 in spec:
        tc = GPCSDTemporalCovSE(t) if kind == C.SE else GPCSDTemporalCovMatern(t)
        tc.params["ell"]["value"], tc.params["sigma2"]["value"] = ell, s2
        tcl.append(tc)
    m = GPCSD1D(lfp, x, t, a=0.0, b=2400.0, ngl=60, temporal_cov_list=tcl)
    m.spatial_cov.params["ell"]["value"] = 180.0
    m.R["value"] = 120.0
    m.sig2n["value"] = 0.07
    geom = O.Geometry1D(x, t, a=0.0, b=2400.0, ngl=60)
    hp = O.make_hparams(120.0, (180.0,), spec, 0.07)
    ctx = m._context()
    n0 = ctx.fold_gemm(True)
    ll = float(m.loglik())
    assert ctx.fold_gemm() == n0 + 1
    llo = O.loglik(geom, with_jitter(hp, m.JITTER), lfp)
    assert abs(ll - llo) / abs(llo) < 1e-8
    for z in (x, x[::2]):
        n1 = ctx.fold_gemm()
        m.predict(z, t, type="both")
        assert ctx.fold_gemm() == n1 + 1
        csd_f, lfp_f, lst_f = m.csd_pred.copy(), m.lfp_pred.copy(), [a.copy() for a in m.csd_pred_list]
        ctx.fold_gemm(False)
        m.predict(z, t, type="both")
        ctx.fold_gemm(True)
        ref = O.predict(geom, hp, lfp, z, t, type="both")
        # 81 electrodes 30 um apart under a 180 um length scale: Ks is numerically singular and predict adds no jitter
        # (gpcsd1d.py:258), so two correct fp64 evaluations differ by ~1e-7 in the small components
        assert relerr(csd_f, m.csd_pred) < 1e-7 and relerr(lfp_f, m.lfp_pred) < 1e-7
        assert relerr(csd_f, ref["csd"]) < 1e-6 and relerr(lfp_f, ref["lfp"]) < 1e-6
        for a, b in zip(lst_f, ref["csd_list"]):
            assert relerr(a, b) < 1e-6


# ------------------------------------------------------------------------------------------------ fp32 Gram build (cfg5)
def test_fp32_gram_build_variant(ctx):
    """BASELINE cfg5 names an "fp32 kernel build + fp64 factor" variant: the Gram builders evaluate in single precision,
    everything after them stays fp64.  The switch is per context; deviations are those of float rounding of the Gram
    entries (reported in DESIGN.md), the default path is untouched."""
    t = np.linspace(0.0, 499.0, 500).reshape(-1, 1)
    try:
        K64 = ctx.gram_temporal(C.SE, t, t, 20.0, 0.5) + ctx.gram_temporal(C.MATERN, t, t, 5.0, 0.7)
        ctx.set_gram_precision(32)
        K32 = ctx.gram_temporal(C.SE, t, t, 20.0, 0.5) + ctx.gram_temporal(C.MATERN, t, t, 5.0, 0.7)
    finally:
        ctx.set_gram_precision(64)
    dev = np.max(np.abs(K32 - K64)) / np.max(np.abs(K64))
    assert 1e-10 < dev < 3e-6, dev
    assert np.array_equal(ctx.gram_temporal(C.SE, t, t, 20.0, 0.5) + ctx.gram_temporal(C.MATERN, t, t, 5.0, 0.7), K64)
    with pytest.raises(ValueError):
        ctx.set_gram_precision(16)
    for name in ("cfg2s_1d_24x500x8", "2d_npx_96x120x3"):
        m, c, g, geom, hp, lfp = _build_model(name)
        ll64 = float(m.loglik())
        m.gram_precision = 32
        ll32 = float(m.loglik())
        _, g32 = m._loglik_and_grad_natural()
        m.gram_precision = 64
        assert float(m.loglik()) == ll64                       # switching back restores the reference arithmetic bit for bit
        dev_ll = abs(ll32 - ll64) / abs(ll64)
        print("fp32 Gram build, %s: loglik deviation %.2e" % (name, dev_ll))
        assert 0.0 < dev_ll < 1e-3 and np.all(np.isfinite(g32))


def test_folded_predict_without_component_lists(ctx):
    """gpcsd_predict_resident(want_lists=0) on the folded path: only the sum over temporal components is written; it equals
    the sum of the per-component predictions of a call that asks for the lists."""
    name = FOLD_CASES[0]
    m, c, g, geom, hp, lfp = _build_model(name)
    mctx = m._sync_device()
    hp0, keep = m._hparams(0.0)
    nz, nt, R = c["x"].shape[0], c["t"].shape[0], lfp.shape[2]
    C_ = len(c["temporal"])
    n0 = mctx.fold_gemm(True)
    mctx.predict_resident(hp0, c["x"], c["t"], 1, want_lists=True)
    lists = mctx.fetch("pred_out_csd_list", (C_, nz, nt, R))
    tot = mctx.fetch("pred_out_csd", (nz, nt, R))
    mctx.predict_resident(hp0, c["x"], c["t"], 1, want_lists=False)
    assert mctx.fold_gemm() == n0 + 2
    tot2 = mctx.fetch("pred_out_csd", (nz, nt, R))
    assert np.array_equal(tot, tot2)
    assert relerr(lists.sum(axis=0), tot) < 1e-13
    assert relerr(tot, g["csd_pred"]) < GATE


def test_one_sided_fold_takes_any_prediction_sites():
    """GPCSD1D with 24 electrodes: only the temporal side folds, the spatial one takes part as one full-size block, so the
    folded path serves arbitrary (asymmetric, finer) prediction sites; it still needs t* = t."""
    m, c, g, geom, hp, lfp = _build_model("cfg2s_1d_24x500x8")
    ctx = m._context()
    ctx.fold_gemm(True)
    x, t = c["x"], c["t"]
    z = np.linspace(float(x.min()) + 13.0, float(x.max()) - 111.0, 31).reshape(-1, 1)     # not mirror-symmetric, nz != nx
    n0 = ctx.fold_gemm()
    m.predict(z, t, type="both")
    assert ctx.fold_gemm() == n0 + 1
    csd_f, lfp_f = m.csd_pred.copy(), m.lfp_pred.copy()
    ctx.fold_gemm(False)
    m.predict(z, t, type="both")
    ctx.fold_gemm(True)
    assert relerr(csd_f, m.csd_pred) < 1e-10 and relerr(lfp_f, m.lfp_pred) < 1e-10
    ref = O.predict(geom, hp, lfp, z, t, type="both")
    assert relerr(csd_f, ref["csd"]) < GATE and relerr(lfp_f, ref["lfp"]) < GATE
    n1 = ctx.fold_gemm()
    m.predict(z, t + 0.25, type="csd")                                # shifted prediction times: full-size path
    assert ctx.fold_gemm() == n1


@pytest.mark.parametrize("name", ["cfg2s_1d_24x500x8", "2d_npx_96x120x3"])
def test_failed_call_leaves_a_clean_context(name):
    """A fused call that fails numerically (NaN hyper-parameter: the eigensolvers cannot converge) must not poison the next
    one: the status words are cleared between calls (at the end of a call, or at the start of one that follows a failure)."""
    m, c, g, geom, hp, lfp = _build_model(name)
    ref = float(g["loglik"])
    assert abs(float(m.loglik()) - ref) / abs(ref) < GATE
    sname = m._spatial_names[0]
    slots = [(m.temporal_cov_list[0].params["ell"], float("nan")), (m.spatial_cov.params[sname], float("nan")),
             (m.R, float("nan")), (m.temporal_cov_list[0].params["ell"], 0.0), (m.temporal_cov_list[-1].params["sigma2"], float("inf"))]
    for slot, badval in slots:
        good = slot["value"]
        slot["value"] = badval
        for call in (m.loglik, lambda: m.predict(c["x"], c["t"], type="csd")):
            try:
                out = call()
                assert out is None or not np.isfinite(out)
            except (np.linalg.LinAlgError, ValueError, RuntimeError):
                pass
        slot["value"] = good
        for _ in range(2):
            assert abs(float(m.loglik()) - ref) / abs(ref) < GATE
    m.predict(c["x"], c["t"], type="csd")
    assert relerr(m.csd_pred, g["csd_pred"]) < GATE


@pytest.mark.parametrize("n", [24, 70, 250, 384])
def test_eigh_edge_inputs(ctx, n):
    """Inputs at the edges of the solver's assumptions: zero / exactly low-rank / identity / badly scaled matrices stay
    accurate (exactly low-rank ones leave columns that are rounding noise of rounding noise: they once overflowed the
    reflector scalars and, through NaNs in the rank sorts, faulted the GPU), non-finite ones raise LinAlgError, and the
    context keeps working afterwards.  tools/eigh_edge.py is the long version."""
    rs = np.random.RandomState(n)
    X = rs.standard_normal((n, n))
    G = X + X.T
    cases = {"zeros": np.zeros((n, n)), "ones": np.ones((n, n)), "identity": np.eye(n), "tiny": 1e-300 * G, "huge": 1e290 * G,
             "graded": np.diag(np.logspace(-300, 300, n)), "rank2": np.outer(X[0], X[0]) + np.outer(X[1], X[1])}
    for name, A in cases.items():
        w, Z = ctx.eigh(A)
        wr = np.linalg.eigvalsh(A)
        sc = max(np.abs(wr).max(), 1e-300)
        assert np.abs(w - wr).max() / sc < 1e-12 * n, name
        assert np.abs(Z.T @ Z - np.eye(n)).max() < 1e-12 * n, name
        with np.errstate(all="ignore"):
            assert np.abs((A / sc) @ Z - Z * (w / sc)).max() < 1e-11 * n, name
    for bad in (np.nan, np.inf):
        A = G.copy()
        A[n // 3, n // 2] = A[n // 2, n // 3] = bad
        with pytest.raises(np.linalg.LinAlgError):
            ctx.eigh(A)
    w, Z = ctx.eigh(G)
    assert np.abs(w - np.linalg.eigvalsh(G)).max() < 1e-11 * n


def test_random_models_vs_oracle():
    """A short run of tools/fuzz_models.py: random 1D / 2D geometries (symmetric, perturbed, odd sizes, both sides of the
    64-row Jacobi limit), random well-scaled hyper-parameters, noise lists, predictions off the electrode grid and at shifted
    times -- every combination of folded / unfolded sides falls out of the draw.  1150 cases were run with the tool itself."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_models as F
    rs = np.random.RandomState(7)
    nfold = 0
    for k in range(40):
        try:
            desc, e_ll, e_c, e_l, folds = F.one_case(rs, k)
        except ZeroDivisionError:
            continue
        nfold += folds > 0
        # 1e-6 everywhere; with a per-electrode noise list the reference's objective depends on the order of the rounding-
        # noise eigenvalues of Ks (O.driver_spread): the gate there is 3x what LAPACK drivers disagree by on the same draw
        gates = [max(1e-6, 3.0 * v) for v in F.one_case.last_spread]
        assert e_ll < gates[0] and e_c < gates[1] and e_l < gates[2], (desc, e_ll, e_c, e_l, F.one_case.last_spread)
    if not (os.environ.get("GPCSD_NO_FOLD_GEMM") == "1" or os.environ.get("GPCSD_NO_SYMFOLD") == "1"):
        assert nfold > 5


@pytest.mark.gpu
@pytest.mark.parametrize("n,count", [(24, 5), (100, 3), (250, 8), (300, 2)])
def test_eigh_batch_is_bitwise_the_sequential_solver(ctx, n, count):
    """Replicated problems share every launch of the chain (kernel arguments describe classes, workgroups add
    replica * stride): each replica must get exactly the bits a solve on its own produces."""
    rs = np.random.RandomState(100 + n)
    t = np.arange(n, dtype=np.float64)[:, None]
    mats = []
    for k in range(count):
        G = np.exp(-0.5 * ((t - t.T) / (3.0 + k)) ** 2) + 0.3 * np.exp(-np.abs(t - t.T) / (2.0 + 0.5 * k))
        B = rs.standard_normal((n, n))
        mats.append(G + 1e-3 * (B + B.T))
    A = np.stack(mats)
    w, V, st = ctx.eigh_batch(A)
    assert np.all(st == 0)
    for k in range(count):
        wk, Vk = ctx.eigh(A[k])
        assert np.array_equal(w[k], wk) and np.array_equal(V[k], Vk)
        assert np.abs(w[k] - np.linalg.eigvalsh(A[k])).max() < 1e-12 * n * np.abs(wk).max()
    # a non-finite matrix fails alone
    A[1, 3, 4] = A[1, 4, 3] = np.nan
    w2, V2, st2 = ctx.eigh_batch(A)
    assert st2[1] != 0 and np.all(np.delete(st2, 1) == 0)
    assert np.array_equal(w2[0], w[0]) and np.array_equal(V2[0], V[0])
    if count > 2:
        assert np.array_equal(w2[count - 1], w[count - 1]) and np.array_equal(V2[count - 1], V[count - 1])
