"""Matern-3/2 and Matern-5/2 temporal kernels on the device (GPCSD_KIND_MATERN32 / _MATERN52; no reference counterpart).

  1. Gram entries against long double: |dev - ref| <= (16 + 4 a) 2^-53 |ref| + 2^-1074 with a = sqrt(3) |d| / ell or sqrt(5) |d| / ell
     (about ten roundings in d, a, the polynomial, exp and the products: 16; a relative error of a few units in a is a times that in
     exp(-a): 4 a), a from 0 to 750 so that exp(-a) underflows; sigma2 = 0.7 (the absolute term 2^-1074 is half a unit of the last
     place of a subnormal result and holds for sigma2 <= 1 only: a unit-variance value that is a subnormal has lost that much before
     sigma2 multiplies it).  fp32 mode in the window of tests/test_hip_parity.py.
  2. temporal_grad through debug_grad_op, with the yardstick and the gate of tests/test_grad_kernels.py.
  3. Model level against the dense float64 statements of the existing tests, on three golden cases with only the kinds swapped
     (matern_ref.SWAPS), each at the tolerance of the existing test of the same call on the same golden case.
  4. The same three models through user-defined classes (GPCSD_KIND_HOST, host NumPy Gram and derivative matrices).
  5. Bits: batch = single evaluations, the paired call = the fenced calls, the same call twice; fit() through the lock-step batch.
  6. The calls that refuse host kernels: sample_posterior, predict_functionals, loglik_masked.
Every test prints what it observes; DESIGN.md 4.14 records the figures."""
import numpy as np
import pytest

import matern_ref as MT
from oracle import gpcsd_oracle as O

LD = np.longdouble
U = 2.0 ** -53
GATE = 1e-6                       # the project's gate (tests/test_hip_parity.py)
ODD, SIG, GRID = MT.CASES         # (MATERN32) / (MATERN52, MATERN32) with a noise list / (SE, MATERN52) on the mirror-folded path
SCALAR = [ODD, GRID]
NEW = (MT.MATERN32, MT.MATERN52)
gpu = pytest.mark.gpu
_MODELS = {}


@pytest.fixture(scope="module")
def ctx():
    from gpcsd_amd import _hip
    return _hip.default_context()


@pytest.fixture
def world(monkeypatch):
    return MT.world(monkeypatch)


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = MT.model_for(name)
    return _MODELS[name]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------ 1. Gram entries
def _gram_times(n, m):
    """Non-uniform times on [0, 100] with repeated values (d = 0) and the full span present whatever the shape."""
    rs = np.random.RandomState(100 * n + m)
    t, tp = np.sort(rs.uniform(0.0, 100.0, n)), np.sort(rs.uniform(0.0, 100.0, m))
    tp[0] = t[0]                                         # d = 0 off the diagonal as well
    if n > 1:
        t[1] = t[0]
        t[-1] = 100.0
    if m > 1:
        tp[1] = 0.0
        tp[m // 2] = t[n // 2]
    return t, tp


@gpu
@pytest.mark.parametrize("kind", NEW)
@pytest.mark.parametrize("n,m", [(1, 1), (16, 64), (17, 65), (37, 130)])          # the 64 x 16 tile and both of its edges
def test_gram_entries_against_long_double(ctx, kind, n, m):
    t, tp = _gram_times(n, m)
    s2 = 0.7
    worst = 0.0
    # a = 750 at the full span of 100 (exp(-a) underflows from a = 708, to zero from 745), and a moderate length scale
    for ell in (np.sqrt(3.0 if kind == MT.MATERN32 else 5.0) * 100.0 / 750.0, 7.0):
        got = ctx.gram_temporal(kind, t, tp, ell, s2)
        ref = MT.gram(kind, t, tp, ell, s2, LD)
        a = MT.scaled_distance(kind, t[:, None] - tp[None, :], ell)
        bound = (16.0 + 4.0 * a).astype(LD) * LD(U) * np.abs(ref) + LD(2.0) ** -1074
        frac = float(np.max(np.abs(got.astype(LD) - ref) / bound))
        worst = max(worst, frac)
        print("gram kind %d (%d, %d) ell %.4g: a up to %.0f, %d subnormal, %d zero entries; |dev - ref| at most %.3f of the bound"
              % (kind, n, m, ell, a.max(), int(np.sum((got != 0) & (np.abs(got) < 2.0 ** -1022))), int(np.sum(got == 0)), frac))
        assert got.shape == (n, m) and np.all(np.isfinite(got))
        assert frac <= 1.0
        assert _same_bits(got, ctx.gram_temporal(kind, t, tp, ell, s2))
        assert np.all(got[a == 0] == s2)


@gpu
def test_fp32_gram_mode(ctx):
    """The deviation of the single-precision Gram build from the fp64 one lies in the window tests/test_hip_parity.py uses for the
    built-in kinds; the fp64 bits return with set_gram_precision(64)."""
    t = np.linspace(0.0, 129.0, 130).reshape(-1, 1) + 0.25 * np.random.RandomState(3).uniform(size=(130, 1))
    both = lambda: ctx.gram_temporal(MT.MATERN32, t, t, 20.0, 0.5) + ctx.gram_temporal(MT.MATERN52, t, t, 5.0, 0.7)
    try:
        K64 = both()
        ctx.set_gram_precision(32)
        K32 = both()
    finally:
        ctx.set_gram_precision(64)
    dev = np.max(np.abs(K32 - K64)) / np.max(np.abs(K64))
    print("fp32 Gram build, Matern-3/2 + Matern-5/2: deviation %.2e of the largest entry" % dev)
    assert 1e-10 < dev < 3e-6, dev
    assert _same_bits(both(), K64)


# ------------------------------------------------------------------------------------------------ 2. temporal_grad
HP_G = {"m32": ((MT.MATERN32,), (5.0,), (0.7,)),
        "m52": ((MT.MATERN52,), (20.0,), (0.5,)),
        "four": ((MT.SE, MT.MATERN52, MT.MATERN, MT.MATERN32), (20.0, 8.0, 5.0, 3.0), (0.5, 0.3, 0.7, 1.1))}


def _grad_gate(TG, fam, label, got, Gt, t, hp):
    TG._gate("temporal_grad_matern", fam, label, got, MT.temporal_grad_f64(Gt, t, *hp), *MT.temporal_grad_ld(Gt, t, *hp))


@gpu
@pytest.mark.parametrize("nt", [37, 257])                # one block's share, and more elements (66049) than one pass of the grid (65536)
def test_temporal_grad_by_value(ctx, nt):
    import test_grad_kernels as TG
    for fam, Gt in TG._temporal_families(nt):
        t = TG._times(nt, fam == "normal")
        for name, hp in HP_G.items():
            _grad_gate(TG, fam, "nt=%d %s" % (nt, name), TG._k_temporal(ctx, Gt, t, hp), Gt, t, hp)


@gpu
@pytest.mark.parametrize("nt", [37, 257])
def test_temporal_grad_by_table(ctx, nt):
    """Three sets through the device table: each set's values are the bits of its own plain call and pass the gate."""
    import grad_ref as GR
    import test_grad_kernels as TG
    names = ("four", "m32", "m52")                       # (set 0 has the most components: the table's rule)
    sets = [HP_G[n] for n in names]
    for fam in ("normal", "spike"):
        Gts = [GR.weights(fam, (nt, nt), seed) for seed in range(3)]
        t = TG._times(nt, True)
        out = TG._k_temporal_table(ctx, Gts, t, sets)
        for b, (name, hp) in enumerate(zip(names, sets)):
            c2 = 2 * len(hp[0])
            assert _same_bits(out[b, :c2], TG._k_temporal(ctx, Gts[b], t, hp)), "set %d (%s) differs from its plain call" % (b, name)
            assert np.all(out[b, c2:] == 0.0)
            _grad_gate(TG, fam, "nt=%d table[%d] %s" % (nt, b, name), out[b, :c2], Gts[b], t, hp)


@gpu
def test_kinds_2_and_5_are_rejected_and_the_context_stays_usable(ctx):
    import grad_ref as GR
    import test_grad_kernels as TG
    nt = 37
    Gt, t, hp = GR.weights("normal", (nt, nt)), TG._times(nt, True), HP_G["four"]
    good = TG._k_temporal(ctx, Gt, t, hp)
    for bad in (2, 5, -1):
        hb = TG._hp([hp])
        hb.rec["kind"][0, 1] = bad
        with pytest.raises(ValueError):
            ctx.debug_grad_op("temporal_grad", [Gt, t], [8], n=[nt], l=[0, 0, 0, 8], hp=hb)
        with pytest.raises(ValueError):
            ctx.gram_temporal(bad, t, t, 5.0, 0.7)
        assert _same_bits(TG._k_temporal(ctx, Gt, t, hp), good)
        _grad_gate(TG, "normal", "after kind %d" % bad, TG._k_temporal(ctx, Gt, t, hp), Gt, t, hp)


# ------------------------------------------------------------------------------------------------ 3. model level
@gpu
@pytest.mark.parametrize("name", MT.CASES)
def test_loglik_vs_dense(world, name):
    """1e-8 relative: tests/test_hip_parity.py::test_model_loglik_vs_reference_golden against the oracle on the same golden cases."""
    c, g, geom, hp, lfp = world(name)
    Ks = O.spatial_kphi(geom, hp) + float(g["jitter"]) * np.eye(geom.x.shape[0])
    ref = O.loglik_from_K(lfp, Ks, O.temporal_sum(hp["temporal"], geom.t), hp["sig2n"])
    ll = _model(name).loglik()
    print("loglik %s: %.12g against %.12g, %.2e relative" % (name, ll, ref, abs(ll - ref) / abs(ref)))
    assert abs(ll - ref) / abs(ref) < 1e-8
    assert _model(name).loglik() == ll


@gpu
@pytest.mark.parametrize("name", SCALAR)
def test_gradient_scores_and_information_vs_dense(world, name):
    """The natural gradient against 1/2 tr((alpha alpha^T - R K^-1) d_i K), the per-trial scores and the expected information
    against fisher_ref's dense solves: the gates and scales of tests/test_fisher.py::test_scores_and_information_vs_dense."""
    import test_fisher as TF
    m, ref = _model(name), TF._ref(name)
    c, geom, hp, lfp = TF._case(name)
    R, ng = ref["scores"].shape
    assert m.JITTER == hp["jitter"]
    ll, grad = m._loglik_and_grad_natural()
    scale = np.abs(ref["quad"]).sum(axis=0) + R * np.abs(ref["trace"])
    e_grad = float(np.max(np.abs(grad - ref["scores"].sum(axis=0)) / scale))
    S = m.trial_scores()
    I = m.fisher_information("expected", log_params=False) / R
    e_s, e_i = TF._score_err(S, ref), TF._info_err(I, ref["info"])
    e_g = float(np.max(np.abs(S.sum(axis=0) - grad) / scale))
    print("matern %s: gradient vs dense closed form %.2e, scores %.2e, column sums vs gradient %.2e, information %.2e (gate %.0e)"
          % (name, e_grad, e_s, e_g, e_i, TF.GATE))
    assert grad.shape == (ng,) and S.shape == (R, ng) and I.shape == (ng, ng)
    assert e_grad < TF.GATE and e_s < TF.GATE and e_i < TF.GATE and e_g < TF.GATE
    assert np.array_equal(I, I.T) and np.array_equal(m.trial_scores(), S)


@gpu
def test_gradient_with_the_noise_list_vs_central_differences(world):
    """With a noise list the objective is defined through the eigen-index (no dense closed form of its gradient): central differences
    of the oracle, as tests/test_hip_parity.py::test_gradient_with_per_electrode_noise_list does on this golden case, at its 1e-7."""
    c, g, geom, hp, lfp = world(SIG)
    m = _model(SIG)
    ll, g_nat = m._loglik_and_grad_natural()
    kinds = [k for k, _, _ in hp["temporal"]]
    sig = np.array(c["sig2n"], dtype=np.float64)
    assert g_nat.shape == (1 + 1 + 2 * len(kinds) + sig.size,)
    vals = np.concatenate([[c["R"]], list(c["ell_s"]), [v for (_, ell, s2) in hp["temporal"] for v in (ell, s2)], sig])
    tp = np.log(vals / np.array([100.0] * 2 + [1.0] * (2 * len(kinds) + sig.size)))
    fd = O.loglik_grad_fd(geom, lfp, tp, kinds, sig.size, eps=c["eps"], jitter=float(g["jitter"]), h=1e-5)
    err = float(np.max(np.abs(g_nat * vals - fd)) / np.max(np.abs(fd)))
    print("matern %s: gradient vs central differences of the oracle %.2e" % (SIG, err))
    assert err < 1e-7, (g_nat * vals, fd)


@gpu
@pytest.mark.parametrize("name", MT.CASES)
def test_predict_at_and_predict_var_vs_dense(world, name):
    """Off-grid times; gates of tests/test_predict_at.py (1e-6 of the largest entry) and tests/test_predict_var.py (explained term 1e-6,
    every element 1e-2 of the variance)."""
    import test_predict_at as PA
    import test_predict_var as PV
    m = _model(name)
    c = PA._case(name)[0]
    ncomp = len(c["temporal"])
    for nz, nts in ((5, 7), (None, None)):
        z = c["x"] if nz is None else c["x"][:nz]
        tstar = PA._offgrid(c["t"], c["t"].shape[0] if nts is None else nts)
        m.predict_at(z, tstar, type="both")
        PA._assert_matches(PA._results(m), PA._helper(name, z, tstar), ncomp, "%s nts=%d nz=%d" % (name, tstar.shape[0], z.shape[0]))
        m.predict_var(z, tstar, type="both")
        ref = PV._helper(name, z, tstar)
        for nm in PV.NAMES:
            got = PV._planes(m, nm)
            rv = ref[nm]["prior"] - ref[nm]["expl"]
            e_expl = float(np.max(np.abs((ref[nm]["prior"] - got) - ref[nm]["expl"])) / np.max(np.abs(ref[nm]["expl"])))
            e_elem = float(np.max(np.abs(got - rv) / rv))
            print("predict_var %s %s nz=%d nts=%d: explained term %.2e, elementwise %.2e, least var / prior %.2e"
                  % (name, nm, z.shape[0], tstar.shape[0], e_expl, e_elem, float(np.min(rv / ref[nm]["prior"]))))
            assert got.shape == (ncomp + 1, z.shape[0], tstar.shape[0]) and np.all(rv > 0)
            assert e_expl < PV.GATE and e_elem <= PV.ELEM


@gpu
@pytest.mark.parametrize("name", MT.CASES)
def test_loo_vs_dense(world, name):
    """tests/test_loo.py::test_loo_vs_helper, its helper and its tolerances (1e-6, or 3 x the helper's own spread between LAPACK
    drivers where the noise list makes that larger)."""
    import test_loo as LO
    m, ref = _model(name), LO._helper(name)
    tol, spread = LO._tolerances(name)
    total = m.loo()
    err = {"var": float(np.max(np.abs(m.loo_var - ref["var"]) / ref["var"])),
           "resid": float(np.max(np.abs((np.asarray(m.lfp) - m.loo_mean) - ref["resid"])) / np.max(np.abs(ref["resid"]))),
           "lpd": float(np.max(np.abs(m.loo_lpd - ref["lpd"])) / np.max(np.abs(ref["lpd"]))),
           "sse": float(np.max(np.abs(m.loo_sse - ref["sse"])) / np.max(np.abs(ref["sse"]))),
           "total": abs(total - ref["total"]) / abs(ref["total"])}
    print("loo %s: " % name + ", ".join("%s %.2e (gate %.1e, driver spread %.1e)" % (k, err[k], tol[k], spread[k]) for k in err))
    assert np.all(m.loo_var > 0)
    for k in err:
        assert err[k] < tol[k], (name, k, err[k], tol[k])


@gpu
@pytest.mark.parametrize("name", MT.CASES)
def test_predict_masked_with_a_missing_window_vs_dense(world, name):
    """Six consecutive samples missing on every electrode of trial 1 (masked_ref's "window6"); gate of tests/test_predict_masked.py."""
    import masked_ref as MK
    import test_predict_at as PA
    m = _model(name)
    c = MK.case(name)["c"]
    mask, ref = MK.mask_for(name, "window6"), MK.dense(name, "window6")
    assert not mask.all()
    for z, ts, tag in ((c["x"], c["t"], "grid"), (MK.sites(name), PA._offgrid(c["t"], 4), "off")):
        m.predict_masked(z, ts, mask, type="both")
        PA._assert_matches(PA._results(m), MK.predictions(name, ref["alpha"], z, ts), len(c["temporal"]), "masked %s window6 %s" % (name, tag))


# ------------------------------------------------------------------------------------------------ 4. the host path
class _UserMatern:
    """A user-defined temporal covariance (GPCSD_KIND_HOST: no `kind` the library knows) that happens to be one of the new kernels:
    Gram and derivative matrices are matern_ref's NumPy formulas, priors and bounds those of the library's class."""

    def __init__(self, kind, t):
        from gpcsd_amd import covariances as CV
        self._k = kind
        self.t = t
        self.params = {MT.MATERN32: CV.GPCSDTemporalCovMatern32, MT.MATERN52: CV.GPCSDTemporalCovMatern52}[kind](t).params

    def compute_Kt(self, t=None, tprime=None):
        return MT.gram(self._k, self.t if t is None else t, self.t if tprime is None else tprime, self.params["ell"]["value"],
                       self.params["sigma2"]["value"])

    def compute_dKt(self, name):
        return MT.dgram(self._k, self.t, self.params["ell"]["value"], self.params["sigma2"]["value"], name)


@gpu
@pytest.mark.parametrize("name", MT.CASES)
def test_host_path_agrees_with_the_device_kinds(name):
    """The same model with its new-kind components as user-defined classes (the existing GPCSD_KIND_HOST path: host Gram, no fold)
    at three parameter points: objective 1e-9 relative (tests/test_hip_fullsize.py's host-kernel test against the oracle), gradient
    1e-6 of its largest component (the project's gate for a gradient component; both sides are analytic)."""
    from gpcsd_amd import covariances as CV
    dev = MT.model_for(name)
    host = MT.model_for(name, classes={MT.SE: CV.GPCSDTemporalCovSE, MT.MATERN: CV.GPCSDTemporalCovMatern,
                                       MT.MATERN32: lambda t: _UserMatern(MT.MATERN32, t), MT.MATERN52: lambda t: _UserMatern(MT.MATERN52, t)})
    assert host._uses_host_kt() and host._host_kt_is_differentiable() and not dev._uses_host_kt()
    tp0 = dev._current_tparams()
    assert np.array_equal(tp0, host._current_tparams())
    rs = np.random.RandomState(7)
    for k in range(3):
        tp = tp0 + (0.0 if k == 0 else 0.08) * rs.standard_normal(tp0.size)
        fd, gd = dev._objective_and_grad(tp, False)
        fh, gh = host._objective_and_grad(tp, False)
        e_f, e_g = abs(fd - fh) / abs(fh), float(np.max(np.abs(gd - gh)) / np.max(np.abs(gh)))
        print("host vs device kinds %s point %d: objective %.2e, gradient %.2e of its largest component" % (name, k, e_f, e_g))
        assert e_f < 1e-9 and e_g < 1e-6


# ------------------------------------------------------------------------------------------------ 5. bits
@gpu
@pytest.mark.parametrize("name", MT.CASES)
def test_batch_of_three_equals_three_single_evaluations(name):
    m = MT.model_for(name)
    assert m._uses_host_kt() is False and m._batch_can_evaluate() is True
    ctx = m._sync_device()
    tp0 = m._current_tparams()
    rs = np.random.RandomState(5)
    ng = tp0.size
    hps, keep, seq = [], [], []
    for _ in range(3):
        m._set_from_tparams(tp0 + 0.08 * rs.standard_normal(tp0.size), False)
        h, k = m._hparams(m.JITTER)
        hps.append(h)
        keep.append(k)
        seq.append(ctx.loglik_grad(h, ng))
        again = ctx.loglik_grad(h, ng)                   # two identical calls: identical bits
        assert again[0] == seq[-1][0] and again[1] == seq[-1][1] and _same_bits(again[2], seq[-1][2])
    sumlog, quad, grad, st = ctx.loglik_grad_batch(hps, ng)
    assert np.all(st == 0)
    for b in range(3):
        assert sumlog[b] == seq[b][0] and quad[b] == seq[b][1] and _same_bits(grad[b], seq[b][2])
        assert np.all(np.isfinite(grad[b]))


@gpu
@pytest.mark.parametrize("name", [ODD, GRID])
def test_paired_call_equals_the_fenced_calls(name):
    from gpcsd_amd import _hip
    m = MT.model_for(name)
    ctx = m._sync_device()
    nx, nt, R = np.atleast_3d(m.lfp).shape
    z, t = np.ascontiguousarray(m.x), m.t
    ncomp = len(m.temporal_cov_list)
    ctx.pair_share_s(False)        # (bit for bit against the fenced calls: the pair decomposes both spatial matrices, as they do)
    ctx.decomposition_cache(False)
    try:
        h1, k1 = m._hparams(m.JITTER)
        h0, k0 = m._hparams(0.0)
        ctx.loglik_predict_async(h1, h0, z, t, _hip.PRED_CSD, want_lists=True)
        parts = ctx.loglik_parts_wait()
        pair = np.array(ctx.fetch("pred_out_csd", (nx, nt, R))), np.array(ctx.fetch("pred_out_csd_list", (ncomp, nx, nt, R)))
        fenced = ctx.loglik_parts(h1)
        ctx.predict_resident(h0, z, t, _hip.PRED_CSD, want_lists=True)
        ctx.synchronize()
        assert fenced == parts
        assert _same_bits(ctx.fetch("pred_out_csd", (nx, nt, R)), pair[0])
        assert _same_bits(ctx.fetch("pred_out_csd_list", (ncomp, nx, nt, R)), pair[1])
        assert np.all(np.isfinite(pair[0])) and -0.5 * R * parts[0] - 0.5 * parts[1] == m.loglik()
    finally:
        ctx.pair_share_s(True)
        ctx.decomposition_cache(True)


@gpu
def test_fit_runs_through_the_lock_step_batch(world):
    """Two restarts on 1d_odd with the Matern-3/2 component: the evaluations share launches, the optima are finite, and the device
    objective at each IS the oracle's loglik_from_K plus the priors there (1e-8, the log-likelihood's tolerance above)."""
    c, g, geom, hp, lfp = world(ODD)
    m = MT.model_for(ODD)
    assert m._uses_host_kt() is False and m._batch_can_evaluate() is True
    tp0 = m._current_tparams()
    starts = [tp0 + 0.1, tp0 - 0.1]
    start_values = [m._objective_and_grad(s, False)[0] for s in starts]
    m.fit(n_restarts=2, starts=starts, options={"maxiter": 8, "disp": False, "gtol": 1e-5, "ftol": 1e7 * np.finfo(float).eps})
    nb, npts = m.fit_batches_
    assert npts > nb                                     # evaluations really shared launches
    got = np.asarray(m.fit_nll_values_)
    assert got.shape == (2,) and np.all(np.isfinite(got)) and np.all(got < np.asarray(start_values))
    kinds = [k for k, _, _ in hp["temporal"]]
    for k in range(2):
        tp = np.asarray(m.fit_params_[k])
        assert np.all(np.isfinite(tp))
        ll = O.loglik(geom, O.hparams_from_tparams(tp, 1, kinds, 1, eps=c["eps"], jitter=float(g["jitter"])), lfp)
        m._set_from_tparams(tp, False)
        want = -(ll + m._log_prior())
        print("fit restart %d: device objective %.12g, oracle + priors %.12g (%.2e)" % (k, got[k], want, abs(got[k] - want) / abs(want)))
        assert abs(got[k] - want) / abs(want) < 1e-8


# ------------------------------------------------------------------------------------------------ 6. calls that used to refuse
@gpu
def test_loglik_masked_vs_dense(world):
    """tests/test_predict_masked.py::test_loglik_masked_vs_dense on the (MATERN52, MATERN32) case with a missing window."""
    import masked_ref as MK
    from helpers import relerr
    m = _model(SIG)
    mask, ref = MK.mask_for(SIG, "window6"), MK.dense(SIG, "window6")
    ll = m.loglik_masked(mask)
    rows = np.array(m.loglik_masked_trials)
    tot = ref["rows"].sum(0)
    errs = [relerr(rows[:, k], ref["rows"][:, k]) for k in range(2)] + [abs(rows[:, k].sum() - tot[k]) / abs(tot[k]) for k in range(2)]
    e_ll = abs(ll - (-0.5 * tot[0] - 0.5 * tot[1])) / abs(0.5 * tot[0] + 0.5 * tot[1])
    print("loglik_masked %s window6 rows log det / quad, sums log det / quad, value: %s %.2e" % (SIG, " ".join("%.2e" % e for e in errs), e_ll))
    assert max(errs) < GATE and e_ll < GATE and m.n_obs == ref["n_obs"]


@gpu
def test_predict_functionals_vs_reference(world):
    """Two box averages (functional_ref's box and its contrast of two boxes) on the (MATERN52, MATERN32) case: the gates of
    tests/test_predict_functionals.py::test_predict_functionals_vs_reference."""
    import functional_ref as FR
    import test_predict_functionals as TPF
    import test_predict_var as PV
    m = _model(SIG)
    c = PV._case(SIG)[0]
    ncomp = len(c["temporal"])
    z, tstar = PV._sites(c["x"], 5), PV._offgrid(c["t"], 7)
    W = FR.functionals(5, 7, seed=12)[1:3]
    res = m.predict_functionals(z, tstar, W, type="both")
    ref = FR.functional_ref(SIG, z, tstar, W)
    for nm in FR.NAMES:
        assert res[nm + "_fun_cov"] is getattr(m, nm + "_fun_cov")
        got = TPF._got(m, nm)
        for p in range(ncomp + 1):
            gp, rp = {k: v[p] for k, v in got.items()}, {k: v[p] for k, v in ref[nm].items()}
            e_expl, e_prior, e_mean = FR.scaled_errors(gp, rp)
            e = np.sqrt(np.abs(np.diag(rp["expl"])))
            tol = GATE * np.outer(e, e)
            print("predict_functionals %s %s plane %d: explained %.2e, prior %.2e, mean %.2e" % (SIG, nm, p, e_expl, e_prior, e_mean))
            assert e_expl < GATE and e_prior < GATE and e_mean < GATE
            assert np.all(np.abs(gp["cov"] - (rp["prior"] - rp["expl"])) <= tol)
            assert np.array_equal(gp["cov"], gp["cov"].T)


@gpu
def test_sample_posterior_vs_dense(world):
    """sample_posterior(nsamples=2) runs on the (MATERN52, MATERN32) case and repeats its bits; the affine map normals -> draws behind
    it has the mean of predict_at (1e-12) and the dense posterior covariance (1e-9 of the largest prior entry): the statement and the
    gates of tests/test_sample_posterior.py::test_affine_map_has_the_mean_of_predict_at_and_the_dense_posterior_covariance, which
    covers the joint Gram over [t*; t] of the new kinds."""
    import posterior_ref as PR
    import test_predict_var as PV
    import test_sample_posterior as TS
    z, tstar = PR.sites(SIG), PR.times(SIG, "offgrid")
    m4 = _model(SIG)
    a = m4.sample_posterior(z, tstar, nsamples=2, type="both", seed=11)
    b = m4.sample_posterior(z, tstar, nsamples=2, type="both", seed=11)
    R = np.atleast_3d(m4.lfp).shape[2]
    assert a[0].shape == (3, 4, R, 2) and a[1].shape == (3, 4, R, 2)
    assert all(np.all(np.isfinite(x)) for x in a) and _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    assert not np.array_equal(a[0][..., 0], a[0][..., 1])
    c = PV._case(SIG)[0]
    m = MT.model_for(SIG, lfp=np.ascontiguousarray(np.atleast_3d(PV.C.case_lfp(c))[:, :, :1]))
    nx, nt = c["x"].shape[0], c["t"].shape[0]
    ns, ntt = 2 * z.shape[0] + nx, tstar.shape[0] + nt
    nxi, ne = ns * ntt, nx * nt
    K = nxi + ne
    xi, eps = np.zeros((1, K + 1, ns, ntt)), np.zeros((1, K + 1, nx, nt))
    xi.reshape(K + 1, nxi)[np.arange(1, nxi + 1), np.arange(nxi)] = 1.0
    eps.reshape(K + 1, ne)[np.arange(nxi + 1, K + 1), np.arange(ne)] = 1.0
    draws = TS._stack(*m._sample_posterior_from_normals(z, tstar, "both", xi, eps))[0]
    m.predict_at(z, tstar, type="both")
    mean = np.concatenate([np.array(m.csd_pred)[:, :, 0].reshape(-1), np.array(m.lfp_pred)[:, :, 0].reshape(-1)])
    half = mean.size // 2
    e_mean = max(float(np.max(np.abs(draws[s, 0] - mean[s])) / np.max(np.abs(mean[s]))) for s in (slice(0, half), slice(half, None)))
    M = draws[:, 1:] - draws[:, :1]
    post, prior = PR.dense_posterior(SIG, z, tstar, "both")
    e_cov = float(np.max(np.abs(M @ M.T - post)) / np.max(np.abs(prior)))
    print("sample_posterior %s: draw 0 vs predict_at %.2e, M M^T vs dense %.2e of the largest prior entry" % (SIG, e_mean, e_cov))
    assert e_mean <= 1e-12 and e_cov <= 1e-9
