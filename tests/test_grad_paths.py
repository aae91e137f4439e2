"""The gradient evaluation's two paths over one shared tail (-m gpu): folded basis and full size, at shapes whose (electrode, trial)
rows exceed one 512-row chunk of the Ghat_t sums by a remainder -- no golden case does -- and with a scalar noise on the full-size
path, which only fold_gemm(False) reaches for the larger shapes.

  A   1D 24 electrodes x 37 samples x 23 trials, SE + Matern: 552 rows = one chunk + 40.
  B   2D the 2d_grid_48x40x2 geometry with 11 trials drawn from the model: 528 rows = one chunk + 16.
  A2  1D 24 x 73 x 23: as A with a time grid that folds (parity blocks 37 | 36, so the quadratic form arrives in two parts) beside
      an identity spatial block.
  B2  2D the 2d_npx_96x120x3 geometry with 6 trials: 576 rows = one chunk + 64; both sides fold, in equal parity blocks (48 | 48 and
      60 | 60), so the pair of EPI_GRAD products is one batched launch.

The eigensolver folds a side only above 64 rows (below, the whole matrix is one Jacobi problem), so A and B run full-size either
way -- 37 samples do not give parity blocks of 19 and 18, and the 48 x 40 grid folds neither side: fold_gemm(None) stays where it is
on both evaluations there.  A2 and B2 are the shapes at which the default evaluation is the folded one and the counter rises.

Per shape: both settings against the oracle's closed-form gradient (O.loglik_and_grad) at the project's gates -- value 1e-9 relative,
every component 1e-6 of the largest --, the two settings against each other at 1e-6 with the counter of folded evaluations rising
exactly on a folded one, and on the full-size path a batch of three sets bit for bit the three single calls."""
import functools

import numpy as np
import pytest

from helpers import load_model_case
from oracle import gpcsd_oracle as O
from test_hip_fit2d import _draw_from_model, _model_2d

pytestmark = pytest.mark.gpu
SHAPES = {"A": False, "B": False, "A2": True, "B2": True}      # name -> the default evaluation is folded (a side above 64 rows)


def _model_1d(nt, ntrials, seed):
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    x, t = np.linspace(0, 2300, 24)[:, None], 2.0 * np.arange(float(nt))[:, None]
    temporal = [(O.SE, 20.0, 0.5), (O.MATERN, 5.0, 0.7)]
    geom = O.Geometry1D(x, t, a=0.0, b=2300.0, ngl=60)
    lfp = _draw_from_model(geom, O.make_hparams(100.0, (200.0,), temporal, 0.05), ntrials, seed, 0.05)
    np.random.seed(0)
    tcl = [GPCSDTemporalCovSE(t), GPCSDTemporalCovMatern(t)]
    for tc, (_, ell, s2) in zip(tcl, temporal):
        tc.params["ell"]["value"], tc.params["sigma2"]["value"] = ell, s2
    m = GPCSD1D(lfp, x, t, a=0.0, b=2300.0, ngl=60, temporal_cov_list=tcl)
    m.R["value"], m.sig2n["value"] = 100.0, 0.05
    m.spatial_cov.params["ell"]["value"] = 200.0
    return m, geom, lfp, [O.SE, O.MATERN], 0.0


def _model_2d_case(name, ntrials, seed):
    c, g, geom, hp, _ = load_model_case(name)
    lfp = _draw_from_model(geom, hp, ntrials, seed, 0.05)
    m = _model_2d(c["x"], c["t"], c["ngl1"], c["ngl2"], c["eps"], lfp, c["R"], c["ell_s"], hp["temporal"], c["sig2n"])
    return m, geom, lfp, [k for k, _, _ in hp["temporal"]], c["eps"]


@functools.lru_cache(maxsize=None)
def _shape(name):
    """One model per shape, shared by the tests (each leaves fold_gemm switched on), with the oracle's value and gradient in the
    log-parameters, computed once."""
    m, geom, lfp, kinds, eps = {"A": lambda: _model_1d(37, 23, 41), "A2": lambda: _model_1d(73, 23, 42),
                                "B": lambda: _model_2d_case("2d_grid_48x40x2", 11, 43),
                                "B2": lambda: _model_2d_case("2d_npx_96x120x3", 6, 44)}[name]()
    nx, nt, R = lfp.shape
    assert nx * R > 512 and (nx * R) % 512 != 0                     # one full chunk and a remainder
    tp = m._current_tparams()
    ll_ref, g_ref = O.loglik_and_grad(geom, lfp, tp, kinds, 1, eps=eps, jitter=m.JITTER)
    hp = O.hparams_from_tparams(tp, m.dim, kinds, 1, eps=eps)
    nat = np.array([hp["R"]] + list(hp["ell_s"]) + [v for (_, ell, s2) in hp["temporal"] for v in (ell, s2)] + [hp["sig2n"]])
    return dict(m=m, ctx=m._sync_device(), tp=tp, nat=nat, ll_ref=ll_ref, g_ref=g_ref)


def _evaluate(s, fold):
    """(loglik, gradient in the log-parameters, folded evaluations counted) with the folded basis allowed or not."""
    s["ctx"].fold_gemm(fold)
    try:
        n0 = s["ctx"].fold_gemm(None)
        ll, g_nat = s["m"]._loglik_and_grad_natural()
        return ll, np.asarray(g_nat) * s["nat"], s["ctx"].fold_gemm(None) - n0        # d / d log(theta) = theta d / d theta
    finally:
        s["ctx"].fold_gemm(True)


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gradient_vs_oracle_closed_form(name, fold):
    s = _shape(name)
    ll, g, _ = _evaluate(s, fold)
    e_ll = abs(ll - s["ll_ref"]) / abs(s["ll_ref"])
    e_g = float(np.max(np.abs(g - s["g_ref"])) / np.max(np.abs(s["g_ref"])))
    print("shape %s fold_gemm(%s): value %.2e relative, gradient %.2e of the largest component" % (name, fold, e_ll, e_g))
    assert e_ll < 1e-9 and e_g < 1e-6, (ll, s["ll_ref"], g, s["g_ref"])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_folded_and_full_size_agree_and_only_a_folded_evaluation_is_counted(name):
    s = _shape(name)
    ll1, g1, n1 = _evaluate(s, True)
    ll0, g0, n0 = _evaluate(s, False)
    e_ll, e_g = abs(ll1 - ll0) / abs(ll0), float(np.max(np.abs(g1 - g0)) / np.max(np.abs(g0)))
    print("shape %s default against fold_gemm(False): value %.2e, gradient %.2e; counted %d and %d" % (name, e_ll, e_g, n1, n0))
    assert e_ll < 1e-6 and e_g < 1e-6
    assert n0 == 0 and n1 == (1 if SHAPES[name] else 0)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_full_size_batch_of_three_is_bitwise_three_single_calls(name):
    s = _shape(name)
    m, ctx = s["m"], s["ctx"]
    rs = np.random.RandomState(7)
    ng = s["tp"].size
    hps, keep = [], []
    for _ in range(3):
        m._set_from_tparams(s["tp"] + 0.08 * rs.standard_normal(ng), False)
        h, k = m._hparams(m.JITTER)
        hps.append(h)
        keep.append(k)
    m._set_from_tparams(s["tp"], False)
    ctx.fold_gemm(False)
    try:
        n0 = ctx.fold_gemm(None)
        seq = [ctx.loglik_grad(h, ng) for h in hps]
        sumlog, quad, grad, st = ctx.loglik_grad_batch(hps, ng)
        assert ctx.fold_gemm(None) == n0
    finally:
        ctx.fold_gemm(True)
    assert np.all(st == 0)
    for b in range(3):
        assert sumlog[b] == seq[b][0] and quad[b] == seq[b][1] and np.array_equal(grad[b], seq[b][2])
