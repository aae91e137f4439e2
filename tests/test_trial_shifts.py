"""The trial-shift objective and its analytic gradient (gpcsd_amd/csrc/shift.hip, gpcsd_shift_plan / gpcsd_shift_eval,
utility_functions.trial_shift_objective, fit_trial_shifts(jac=True)) against the extended-precision statement in shift_ref.py.

CPU: the reference statement itself is pinned -- to the reference package's own numbers (golden nll), to central differences off the
knots (where f is exactly quadratic) and to one-sided differences on them (the left-derivative convention).  GPU: f and g against it
under a rounding bound computed in the test (shift_ref.parts), at the golden shapes, at odd shapes on a non-uniform grid, in batches of
1, 7 and 130 points; errors; and the fit end to end against one SciPy L-BFGS-B(jac=True) per trial on the reference statement."""
import inspect

import numpy as np
import pytest

import shift_ref as SR

H = 2.0 ** -10


def _f(fx, j, tau):
    return SR.f(fx["Qs"], fx["Qt"], fx["Dvec"], fx["lfp"][:, :, j], fx["mu"], fx["t"], tau, fx["mutau"], fx["sigtau"])


def _g(fx, j, tau):
    return SR.g(fx["Qs"], fx["Qt"], fx["Dvec"], fx["lfp"][:, :, j], fx["mu"], fx["t"], tau, fx["mutau"], fx["sigtau"])


def _e(i, n=2):
    v = np.zeros(n)
    v[i] = 1.0
    return v


# ------------------------------------------------------------------------------------------------ CPU
def test_reference_statement_reproduces_the_golden_nll():
    """1. shift_ref.f == the reference package's own objective at all 5 x 4 (trial, tau) pairs, 1e-12 relative (observed 3e-16)."""
    fx = SR.golden_fixture()
    worst = 0.0
    for j in range(5):
        for q, tau in enumerate(fx["taus"]):
            got, want = _f(fx, j, tau), fx["nll"][j, q]
            worst = max(worst, float(abs(got - want) / abs(want)))
    print("golden nll: worst relative difference %.3g" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("tau", SR.OFF_KNOT_TAUS)
def test_reference_gradient_is_the_central_difference_off_knots(tau):
    """2. Off knots f is exactly quadratic in tau, so the central difference with h = 2^-10 IS the derivative up to rounding:
    1e-12 relative, every component of every trial (observed <= 2e-14)."""
    fx = SR.strong_fixture()
    tau = np.array(tau)
    worst = 0.0
    for j in range(5):
        g = _g(fx, j, tau)
        for i in range(2):
            cd = (_f(fx, j, tau + H * _e(i)) - _f(fx, j, tau - H * _e(i))) / (2 * SR.LD(H))
            worst = max(worst, float(abs(g[i] - cd) / abs(g[i])))
    print("tau = %s: worst relative difference to the central difference %.3g" % (tau, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("tau,on_knot", list(zip(SR.ON_KNOT_TAUS, ((0, 1), (0, 1), (1,)))))
def test_reference_gradient_is_the_left_derivative_on_knots(tau, on_knot):
    """3. At a tau that puts samples on knots g is the LEFT derivative: it equals the second-order backward difference
    (3 f(tau) - 4 f(tau - h e_i) + f(tau - 2 h e_i)) / (2 h) to 1e-10 relative (observed about 1e-11; f is quadratic on that side, the
    formula is exact up to rounding), and it is NOT the forward difference (observed off by 1e-3 relative or more)."""
    fx = SR.strong_fixture()
    tau = np.array(tau)
    h = SR.LD(H)
    worst_back, least_fwd = 0.0, np.inf
    for j in range(5):
        g = _g(fx, j, tau)
        f0 = _f(fx, j, tau)
        for i in on_knot:
            back = (3 * f0 - 4 * _f(fx, j, tau - H * _e(i)) + _f(fx, j, tau - 2 * H * _e(i))) / (2 * h)
            fwd = (-3 * f0 + 4 * _f(fx, j, tau + H * _e(i)) - _f(fx, j, tau + 2 * H * _e(i))) / (2 * h)
            worst_back = max(worst_back, float(abs(g[i] - back) / abs(g[i])))
            least_fwd = min(least_fwd, float(abs(g[i] - fwd) / abs(g[i])))
    print("tau = %s: backward difference within %.3g, forward difference off by at least %.3g (relative)" % (tau, worst_back, least_fwd))
    assert worst_back <= 1e-10
    assert least_fwd > 1e-6          # four orders above the backward agreement: a different derivative, not rounding


def test_fit_trial_shifts_keeps_its_defaults():
    """4. The new keywords default to the earlier behaviour; trial_shift_objective is part of the module's surface."""
    from gpcsd_amd import utility_functions as UF
    sig = inspect.signature(UF.fit_trial_shifts)
    assert sig.parameters["jac"].default is False and sig.parameters["return_evals"].default is False
    assert list(sig.parameters)[:11] == ["evec_s", "evec_t", "Dvec", "lfp_trials", "mu_lfp", "t", "tau0", "mutau", "sigtau", "width", "options"]
    obj = inspect.signature(UF.trial_shift_objective)
    assert list(obj.parameters) == ["evec_s", "evec_t", "Dvec", "lfp_trials", "mu_lfp", "t", "mutau", "sigtau", "ctx"]
    assert obj.parameters["mutau"].default == 0.0 and obj.parameters["sigtau"].default == 10.0


# ------------------------------------------------------------------------------------------------ GPU
def _objective(fx, ctx=None):
    from gpcsd_amd.utility_functions import trial_shift_objective
    return trial_shift_objective(fx["Qs"], fx["Qt"], fx["Dvec"], fx["lfp"], fx["mu"], fx["t"], mutau=fx["mutau"], sigtau=fx["sigtau"], ctx=ctx)


def _check_against_reference(label, fx, trials, taus, f, g):
    """f, g of the device within the rounding bounds of shift_ref.parts AND the project's gate of 1e-6 of the largest magnitude;
    prints the observed maxima as fractions of the bounds."""
    rf, rg, bf, bg = SR.batch(fx, trials, taus)
    ef, eg = np.abs(f.astype(SR.LD) - rf), np.abs(g.astype(SR.LD) - rg)
    worst = np.unravel_index(np.argmax(eg / bg), eg.shape)
    print("%s: B = %d, max |df| / bound = %.3g, max |dg| / bound = %.3g (point %d, tau = %s), max |df| / max |f| = %.3g, "
          "max |dg| / max |g| = %.3g" % (label, len(trials), float(np.max(ef / bf)), float(np.max(eg / bg)), worst[0], taus[worst[0]],
                                         float(ef.max() / np.abs(rf).max()), float(eg.max() / np.abs(rg).max())))
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    assert np.all(ef <= bf), ("f outside its rounding bound", float(np.max(ef / bf)))
    assert np.all(eg <= bg), ("g outside its rounding bound", float(np.max(eg / bg)))
    assert ef.max() <= 1e-6 * np.abs(rf).max() and eg.max() <= 1e-6 * np.abs(rg).max()


@pytest.mark.gpu
def test_golden_points_in_one_batch():
    """5. f of all 20 golden (trial, tau) points in ONE batch against the reference package's nll, rtol 1e-10: the gate of
    test_shift_objective_fixture_whitened_quadratic_forms."""
    fx = SR.golden_fixture()
    obj = _objective(fx)
    trials = np.repeat(np.arange(5), 4)
    taus = np.tile(fx["taus"], (5, 1))
    f, g = obj(trials, taus, grad=False)
    assert g is None
    print("golden points: worst relative difference %.3g" % float(np.max(np.abs(f - fx["nll"].reshape(-1)) / np.abs(fx["nll"].reshape(-1)))))
    assert np.allclose(f, fx["nll"].reshape(-1), rtol=1e-10, atol=0)


@pytest.mark.gpu
def test_strong_fixture_value_and_gradient_against_the_reference():
    """6. f and g at the three off-knot and the three on-knot taus of every trial, one batch, one trial index repeated once more,
    within the rounding bounds of shift_ref.parts and 1e-6 of the largest magnitude."""
    fx = SR.strong_fixture()
    obj = _objective(fx)
    points = [(j, tau) for j in range(5) for tau in SR.OFF_KNOT_TAUS + SR.ON_KNOT_TAUS] + [(3, SR.OFF_KNOT_TAUS[0])]
    trials = np.array([p[0] for p in points])
    taus = np.array([p[1] for p in points])
    f, g = obj(trials, taus)
    _check_against_reference("strong fixture", fx, trials, taus, f, g)
    assert f[-1] == f[3 * 6] and np.array_equal(g[-1], g[3 * 6])           # the repeated point: the same bits at another slot


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 7, 130])
def test_odd_shapes_nonuniform_grid(B):
    """7. nx = 17, nt = 37, a non-uniform grid, nseg = 3, random orthogonal Qs and Qt, D in [1e-2, 1e2]; B = 1, 7 and 130 (more than
    one reduction group's worth and more than 128); taus beyond the span of t on both sides, exactly on knots, and 0.  Bounds as
    in test 6.  Also: grad=False gives the bits of grad=True, and the same call twice gives the same bits."""
    fx = SR.odd_fixture(3)
    obj = _objective(fx)
    trials, taus = SR.odd_points(fx, B)
    f, g = obj(trials, taus)
    _check_against_reference("odd shapes", fx, trials, taus, f, g)
    f0, g0 = obj(trials, taus, grad=False)
    assert g0 is None and np.array_equal(f0, f)
    f2, g2 = obj(trials, taus)
    assert np.array_equal(f2, f) and np.array_equal(g2, g)


@pytest.mark.gpu
def test_a_point_alone_and_inside_a_batch():
    """7 (continued). Every point of the B = 130 batch evaluated alone agrees with its value inside the batch within the rounding
    bound, and -- as observed -- bit for bit."""
    fx = SR.odd_fixture(3)
    obj = _objective(fx)
    trials, taus = SR.odd_points(fx, 130)
    f, g = obj(trials, taus)
    _, _, bf, bg = SR.batch(fx, trials, taus)
    same = True
    for b in (0, 1, 3, 64, 129):
        f1, g1 = obj(trials[b:b + 1], taus[b:b + 1])
        assert abs(f1[0] - f[b]) <= bf[b] and np.all(np.abs(g1[0] - g[b]) <= bg[b])
        same = same and f1[0] == f[b] and np.array_equal(g1[0], g[b])
    print("a point alone and inside the batch of 130: %s" % ("the same bits" if same else "NOT the same bits"))
    assert same          # (observed on the MI355X: the same bits; both batch sizes run the same GEMM tile configuration here)


@pytest.mark.gpu
def test_chunked_batches_have_the_same_bits(monkeypatch):
    """7 (continued). The Python layer evaluates a batch that exceeds the library's operand row (B nt >= GPCSD_MAX_GEMM_LD_KMAJOR) in
    chunks; with the limit lowered so that 130 points go as 50 + 50 + 30, every point keeps its bits."""
    from gpcsd_amd import _hip
    fx = SR.odd_fixture(3)
    obj = _objective(fx)
    trials, taus = SR.odd_points(fx, 130)
    f, g = obj(trials, taus)
    monkeypatch.setattr(_hip, "MAX_GEMM_LD_KMAJOR", 50 * fx["t"].size + 1)
    f2, g2 = obj(trials, taus)
    assert np.array_equal(f2, f) and np.array_equal(g2, g)


@pytest.mark.gpu
def test_one_component():
    """7 (continued). nseg = 1: the shortest register array of the gradient kernel and a (B, 1) gradient."""
    fx = SR.odd_fixture(1)
    obj = _objective(fx)
    trials, taus = SR.odd_points(fx, 7)
    f, g = obj(trials, taus)
    assert g.shape == (7, 1)
    _check_against_reference("one component", fx, trials, taus, f, g)


@pytest.mark.gpu
def test_errors_launch_nothing():
    """8. Evaluation without a plan, a trial index out of range, a NaN tau, sigtau = 0 and a non-increasing t each raise the library's
    error, and none of them launches a kernel of the feature (the fenced profiling scopes record none)."""
    from gpcsd_amd import _hip
    fx = SR.odd_fixture(3)
    ctx = _hip.Context()
    try:
        ctx.prof_enable(1)
        ctx.prof_reset()
        with pytest.raises(RuntimeError, match="no plan"):
            ctx.shift_eval([0], np.zeros((1, 3)))
        bad_t = np.array(fx["t"], copy=True)
        bad_t[5] = bad_t[4]
        with pytest.raises(ValueError, match="strictly increasing"):
            ctx.shift_plan(fx["Qs"], fx["Qt"], fx["Dvec"], fx["lfp"], fx["mu"], bad_t)
        with pytest.raises(RuntimeError, match="no plan"):
            ctx.shift_eval([0], np.zeros((1, 3)))
        assert not any("shift" in k and v["count"] for k, v in ctx.prof_all().items())
        ctx.shift_plan(fx["Qs"], fx["Qt"], fx["Dvec"], fx["lfp"], fx["mu"], fx["t"])
        ctx.prof_reset()
        with pytest.raises(ValueError, match="trial index"):
            ctx.shift_eval([0, 4], np.zeros((2, 3)))
        with pytest.raises(ValueError, match="trial index"):
            ctx.shift_eval([-1], np.zeros((1, 3)))
        with pytest.raises(ValueError, match="not finite"):
            ctx.shift_eval([0, 1], np.array([[0.0, 0.0, 0.0], [0.0, np.nan, 0.0]]))
        with pytest.raises(ValueError, match="sigtau"):
            ctx.shift_eval([0], np.zeros((1, 3)), sigtau=0.0)
        assert not any("shift" in k and v["count"] for k, v in ctx.prof_all().items())
        f, g = ctx.shift_eval([0], np.zeros((1, 3)), mutau=fx["mutau"], sigtau=fx["sigtau"])       # the plan survived all of them
        rf, rg, bf, bg = SR.batch(fx, [0], np.zeros((1, 3)))
        assert abs(f[0] - rf[0]) <= bf[0] and np.all(np.abs(g[0] - rg[0]) <= bg[0])
        assert any("shift" in k and v["count"] for k, v in ctx.prof_all().items())                # (and the scopes do see a launch)
    finally:
        ctx.prof_enable(0)
        ctx.close()


@pytest.mark.gpu
def test_fit_with_the_analytic_gradient_end_to_end():
    """9. fit_trial_shifts(jac=True) on the strong fixture: against one SciPy L-BFGS-B(jac=True) per trial on shift_ref (cast to
    float64) tau_hat agrees within 2e-3 and f(tau_hat) <= ref.fun (1 + 1e-6) + 1e-9 (the gates of the existing lock-step test);
    it needs strictly fewer objective evaluations than jac=False on the same inputs (on the CPU: 33 against 105); and every
    |tau_hat - true_tau| < 1: the fixture has an optimum away from tau0."""
    import scipy.optimize
    from gpcsd_amd.utility_functions import fit_trial_shifts
    fx = SR.strong_fixture()
    args = (fx["Qs"], fx["Qt"], fx["Dvec"], fx["lfp"], fx["mu"], fx["t"])
    tau_hat, ok, msgs, ev = fit_trial_shifts(*args, mutau=fx["mutau"], sigtau=fx["sigtau"], jac=True, return_evals=True)
    tau_fd, ok_fd, msgs_fd, ev_fd = fit_trial_shifts(*args, mutau=fx["mutau"], sigtau=fx["sigtau"], return_evals=True)
    print("evaluations: %d points in %d batches with jac=True, %d points in %d batches without; max |tau_hat - tau_fd| = %.3g"
          % (ev["points"], ev["batches"], ev_fd["points"], ev_fd["batches"], float(np.max(np.abs(tau_hat - tau_fd)))))
    assert tau_hat.shape == (5, 2) and len(ok) == 5 and len(msgs) == 5
    assert ev["points"] < ev_fd["points"]
    assert np.all(np.abs(tau_hat - fx["true_tau"]) < 1.0)

    def fg(tau, j):
        p = SR.parts(fx["Qs"], fx["Qt"], fx["Dvec"], fx["lfp"][:, :, j], fx["mu"], fx["t"], tau, fx["mutau"], fx["sigtau"])
        return float(p["f"]), np.asarray(p["g"], dtype=np.float64)
    for j in range(5):
        ref = scipy.optimize.minimize(fg, np.zeros(2), args=(j,), jac=True, method="l-bfgs-b")
        assert np.allclose(tau_hat[j], ref.x, atol=2e-3), (j, tau_hat[j], ref.x)
        assert fg(tau_hat[j], j)[0] <= ref.fun * (1 + 1e-6) + 1e-9
