"""loo: leave-one-out predictive mean, variance and log score (gpcsd_loo; no reference counterpart).

The expected values come from `_helper` below: Qs, Qt, D from the oracle's eig_D of the matrices loglik() decomposes (the jitter on
Ks, a noise list on the eigen-index), then (Rasmussen & Williams, Gaussian Processes for Machine Learning, 5.4.2)

    c = (Qs o Qs) (1 / D) (Qt o Qt)^T,   beta_r = Qs ((Qs^T Y_r Qt) / D) Qt^T,
    loo_var = 1 / c,   loo_mean_r = y_r - beta_r / c,   lpd_r = 1/2 log c - 1/2 beta_r^2 / c - 1/2 log 2 pi,

loo_lpd / loo_sse = the sums over t of lpd_r and (beta_r / c)^2.  The CPU test pins the helper to brute-force deletion: row and
column i removed from the dense K, the rest solved through a Cholesky factor.  The GPU tests print the maxima they observe; on an
MI355X every quantity of every model is within 5.7e-10 of the helper (gate 1e-6; the largest is cfg1, cond(D) 3e8), and
gpcsd_loo_contract within 0.984 / 0.463 / 0.399 of its rounding bound for the mean / lpd / sse."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import cases as C
from helpers import load_model_case
from oracle import gpcsd_oracle as O

GATE = 1e-6                       # the project's contract (tests/test_hip_parity.py)
DELETION = ["1d_odd_17x37x5", "1d_siglist_12x40x4", "cfg1_1d_24x100x1"]
MODELS = ["1d_odd_17x37x5", "1d_siglist_12x40x4", "2d_grid_48x40x2", "2d_npx_96x120x3", "cfg1_1d_24x100x1"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
HALF_LOG_2PI = 0.91893853320467274178                      # log(2 pi) / 2 correctly rounded (0.5 * np.log(2 * np.pi) is an ulp off)
HALF_LOG_2PI_LD = np.longdouble("0.91893853320467274178032973640562")


# ------------------------------------------------------------------------------------------------ NumPy reference
@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (case dict, oracle geometry, oracle hparams WITH loglik's jitter, lfp)"""
    c, g, geom, hp, lfp = load_model_case(name)
    hp = dict(hp, jitter=float(g["jitter"]))
    lfp.setflags(write=False)
    return c, geom, hp, lfp


def _eig(name):
    """Qs, Qt, D (nx, nt) of the matrices loglik() decomposes, by the LAPACK driver the oracle is set to."""
    c, geom, hp, lfp = _case(name)
    Ks = O.spatial_kphi(geom, hp) + hp["jitter"] * np.eye(geom.x.shape[0])
    Qs, Qt, D = O.eig_D(Ks, O.temporal_sum(hp["temporal"], geom.t), hp["sig2n"])
    return Qs, Qt, D.reshape(Qs.shape[0], Qt.shape[0])


def _formulas(name, lfp=None):
    """{"var" (nx, nt), "resid" = y - loo_mean (nx, nt, R), "mean", "lpd" (nx, R), "sse" (nx, R), "total"}"""
    Y = _case(name)[3] if lfp is None else lfp
    Qs, Qt, D = _eig(name)
    cd = (Qs * Qs) @ (1.0 / D) @ (Qt * Qt).T
    alpha = Qs.T @ np.moveaxis(Y, 2, 0) @ Qt                                    # (R, nx, nt)
    beta = np.moveaxis(Qs @ (alpha / D) @ Qt.T, 0, 2)                           # (nx, nt, R)
    resid = beta / cd[:, :, None]
    lpd = (0.5 * np.log(cd)[:, :, None] - 0.5 * beta * resid - HALF_LOG_2PI).sum(axis=1)
    return {"var": 1.0 / cd, "resid": resid, "mean": Y - resid, "lpd": lpd, "sse": (resid * resid).sum(axis=1), "total": float(lpd.sum())}


@functools.lru_cache(maxsize=None)
def _helper(name, driver=None):
    """_formulas of the case's own trials, computed once per LAPACK driver and left unchanged."""
    assert O.EIGH_DRIVER == driver
    out = _formulas(name)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _tolerances(name):
    """The gate per quantity: 1e-6, or 3 x the spread of the helper itself between LAPACK drivers where that exceeds a third of the
    gate (the rule tests/test_hip_fullsize.py applies to noise lists: with a list the reference ties noise x to eigen-RANK x)."""
    base = _helper(name)
    now = lambda: _helper(name, O.EIGH_DRIVER)                                   # (driver_spread switches the oracle's driver)
    spread = {"var": O.driver_spread(lambda: now()["var"] / base["var"])}       # elementwise relative
    for k in ("resid", "lpd", "sse", "total"):
        spread[k] = O.driver_spread(lambda: now()[k])
    return {k: (3.0 * s if s > GATE / 3.0 else GATE) for k, s in spread.items()}, spread


def _dense_K(name):
    """The covariance of one trial's samples, index (x, t): Kronecker form + noise for a scalar noise (nothing shared with the
    helper's eigen-form); with a noise list the eigen-form itself is the definition (utility_functions.py:54-63)."""
    c, geom, hp, lfp = _case(name)
    nx, nt = geom.x.shape[0], geom.t.shape[0]
    if np.ndim(hp["sig2n"]) == 0:
        Ks = O.spatial_kphi(geom, hp) + hp["jitter"] * np.eye(nx)
        return O.mykron(Ks, O.temporal_sum(hp["temporal"], geom.t)) + float(hp["sig2n"]) * np.eye(nx * nt)
    Qs, Qt, D = _eig(name)
    Q = O.mykron(Qs, Qt)
    return (Q * D.reshape(1, -1)) @ Q.T


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", DELETION)
def test_helper_equals_brute_force_deletion(name):
    """Observed (mean relative to max|y|, variance relative to itself): 1d_odd 4.9e-10 / 3.5e-10, 1d_siglist 6.0e-13 / 2.8e-13,
    cfg1 2.9e-9 / 7.7e-10 -- the reference's own error, more than two orders of magnitude inside the gate."""
    import scipy.linalg
    c, geom, hp, lfp = _case(name)
    nx, nt, R = lfp.shape
    K = _dense_K(name)
    y = lfp.reshape(nx * nt, R)
    h = _helper(name)
    rs = np.random.RandomState(4242)
    e_mean = e_var = 0.0
    for i in rs.choice(nx * nt, 25, replace=False):
        keep = np.delete(np.arange(nx * nt), i)
        cf = scipy.linalg.cho_factor(K[np.ix_(keep, keep)], lower=True)
        sol = scipy.linalg.cho_solve(cf, np.column_stack([K[keep, i], y[keep]]))
        var = K[i, i] - K[keep, i] @ sol[:, 0]
        mean = K[keep, i] @ sol[:, 1:]
        x, t = divmod(int(i), nt)
        e_var = max(e_var, abs(h["var"][x, t] - var) / var)
        e_mean = max(e_mean, float(np.max(np.abs(h["mean"][x, t] - mean)) / np.max(np.abs(y))))
    print("helper vs deletion %s: mean %.2e of max|y|, variance %.2e of itself" % (name, e_mean, e_var))
    assert e_mean < GATE and e_var < GATE


def test_surface_exists_and_fails_loudly_without_a_gpu():
    import torch
    from gpcsd_amd import build, _hip
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    assert callable(getattr(GPCSD1D, "loo", None)) and callable(getattr(GPCSD2D, "loo", None))
    build.build(verbose=False)
    lib = _hip.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read(), flags=re.S)
    for fn in ("gpcsd_loo", "gpcsd_loo_resident", "gpcsd_loo_contract"):
        assert re.search(r"\b%s\s*\(" % fn, src), "%s is not declared" % fn
        assert fn in _hip.SIGNATURES
        assert hasattr(lib, fn), "libgpcsd_hip.so does not export %s" % fn
    if not torch.cuda.is_available():
        m = GPCSD1D(np.zeros((24, 50, 2)), np.linspace(0, 2300, 24)[:, None], np.arange(50.0)[:, None])
        with pytest.raises(_hip.HipUnavailable):
            m.loo()


# ------------------------------------------------------------------------------------------------ GPU: the kernel alone
def _contract_bound(V, Qt, cd, Y, R):
    """Reference values in longdouble and a first-order rounding bound for every output of gpcsd_loo_contract, from the kernel's
    own operations (u = 2^-53; a bar marks the computed value, d. its error bound):

      beta  = sum_k V Qt          the multiplier's K fused multiply-adds plus the order of its four-term groups:
                                  d.beta = (K + 2) u sum_k |V| |Qt|
      e     = beta / c            one correctly rounded division:           d.e = d.beta / c + u |e|
      mean  = y - e               one rounding:                             d.mean = d.e + u |mean|
      q     = beta e              a product (rounded or fused, at most one rounding): d.q = |beta| d.e + |e| d.beta + u |q|
      L     = log c               the device's log, within one ulp of the result:    d.L = 2 u |log c|
      l     = (L / 2 - q / 2) - h the halvings are exact; two roundings, and h = log(2 pi) / 2 is itself a rounded constant:
                                  d.l = d.L / 2 + d.q / 2 + u |L / 2 - q / 2| + u |l| + u h
      e^2                         one rounding (or fused into the sum):    d.(e^2) = 2 |e| d.e + u e^2
      the sums over the nt times, in whatever order (registers, lane groups, the two waves, the time tiles):
                                  d.lpd = sum_t d.l + (nt - 1) u sum_t |l|,     d.sse = sum_t d.(e^2) + (nt - 1) u sum_t e^2"""
    ld = np.longdouble
    V, Qt, cd, Y = V.astype(ld), Qt.astype(ld), cd.astype(ld), Y.astype(ld)
    nx, nt = cd.shape
    K = V.shape[1]
    beta = (V @ Qt.T).reshape(nx, R, nt)
    d_beta = (K + 2) * U * (np.abs(V) @ np.abs(Qt).T).reshape(nx, R, nt)
    c3 = cd[:, None, :]
    e = beta / c3
    d_e = d_beta / c3 + U * np.abs(e)
    mean = Y.reshape(nx, R, nt) - e
    d_mean = d_e + U * np.abs(mean)
    q = beta * e
    d_q = np.abs(beta) * d_e + np.abs(e) * d_beta + U * np.abs(q)
    L = np.log(c3)
    t1 = 0.5 * L - 0.5 * q
    l = t1 - HALF_LOG_2PI_LD
    d_l = 0.5 * (2 * U * np.abs(L)) + 0.5 * d_q + U * np.abs(t1) + U * np.abs(l) + U * HALF_LOG_2PI_LD
    d_e2 = 2 * np.abs(e) * d_e + U * e * e
    ref = {"mean": mean.transpose(0, 2, 1), "lpd": l.sum(axis=2), "sse": (e * e).sum(axis=2)}
    bound = {"mean": d_mean.transpose(0, 2, 1), "lpd": d_l.sum(axis=2) + (nt - 1) * U * np.abs(l).sum(axis=2),
             "sse": d_e2.sum(axis=2) + (nt - 1) * U * (e * e).sum(axis=2)}
    return ref, bound


@pytest.mark.gpu
def test_loo_contract_against_extended_precision():
    """Observed on an MI355X: largest error / bound 0.984 (mean: where |e| << |y| the error is the one rounding of y - e, which
    reaches u |mean| just above a power of two and never exceeds it), 0.463 (lpd), 0.399 (sse)."""
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    rs = np.random.RandomState(20241019)
    worst = {"mean": 0.0, "lpd": 0.0, "sse": 0.0}
    for K in (1, 17, 64, 65):
        for nx, R in ((1, 1), (1, 5), (14, 5), (10, 13)):                     # nx * R = 1, 5, 70, 130 rows
            for nt in (1, 7, 64, 95):
                V, Qt = rs.uniform(-1.0, 1.0, (nx * R, K)), rs.uniform(-1.0, 1.0, (nt, K))
                cd = 10.0 ** rs.uniform(-1.5, 1.5, (nx, nt))                     # positive, three decades
                Y = rs.standard_normal((nx * R, nt))
                mean, lpd, sse = ctx.loo_contract(V, Qt, cd, Y, R)
                assert mean.shape == (nx, nt, R) and lpd.shape == (nx, R) and sse.shape == (nx, R)
                ref, bound = _contract_bound(V, Qt, cd, Y, R)
                for k, got in (("mean", mean), ("lpd", lpd), ("sse", sse)):
                    ratio = float(np.max(np.abs(got.astype(np.longdouble) - ref[k]) / bound[k]))
                    worst[k] = max(worst[k], ratio)
                    assert ratio <= 1.0, (k, K, nx, R, nt, ratio)
                none, lpd2, sse2 = ctx.loo_contract(V, Qt, cd, Y, R, want_mean=False)
                assert none is None and np.array_equal(lpd2, lpd) and np.array_equal(sse2, sse)
    print("loo_contract: largest error / bound:", " ".join("%s %.3f" % kv for kv in worst.items()))


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
def test_loo_vs_helper(name):
    m = _model(name)
    ref = _helper(name)
    tol, spread = _tolerances(name)
    nx, nt, R = _case(name)[3].shape
    total = m.loo()
    assert isinstance(total, float)
    assert m.loo_var.shape == (nx, nt) and m.loo_mean.shape == (nx, nt, R) and m.loo_lpd.shape == (nx, R) and m.loo_sse.shape == (nx, R)
    err = {"var": float(np.max(np.abs(m.loo_var - ref["var"]) / ref["var"])),
           "resid": float(np.max(np.abs((np.asarray(m.lfp) - m.loo_mean) - ref["resid"])) / np.max(np.abs(ref["resid"]))),
           "lpd": float(np.max(np.abs(m.loo_lpd - ref["lpd"])) / np.max(np.abs(ref["lpd"]))),
           "sse": float(np.max(np.abs(m.loo_sse - ref["sse"])) / np.max(np.abs(ref["sse"]))),
           "total": abs(total - ref["total"]) / abs(ref["total"])}
    print("loo %s: " % name + ", ".join("%s %.2e (gate %.1e, driver spread %.1e)" % (k, err[k], tol[k], spread[k]) for k in err))
    assert np.all(m.loo_var > 0)
    for k in err:
        assert err[k] < tol[k], (name, k, err[k], tol[k])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1d_odd_17x37x5", "2d_npx_96x120x3"])
def test_bit_identities(name):
    m = _model(name)
    nx, nt, R = _case(name)[3].shape
    total = m.loo()
    first = {k: np.array(getattr(m, k)) for k in ("loo_var", "loo_mean", "loo_lpd", "loo_sse")}
    assert total == float(np.sum(first["loo_lpd"]))                              # the sum of loo_lpd, formed the same way
    assert m.loo() == total                                                      # a second call: the same bits
    for k, v in first.items():
        assert np.array_equal(np.array(getattr(m, k)), v), k
    assert m.loo(mean=False) == total and m.loo_mean is None                     # without the mean: the bits of the other outputs
    for k in ("loo_var", "loo_lpd", "loo_sse"):
        assert np.array_equal(np.array(getattr(m, k)), first[k]), k
    assert m.loo(resident=True) == total                                         # resident views: the bits of the host arrays
    ctx = m._context()
    for k, shape in (("loo_var", (nx, nt)), ("loo_mean", (nx, nt, R)), ("loo_lpd", (nx, R)), ("loo_sse", (nx, R))):
        v = getattr(m, k)
        assert tuple(v.shape) == shape and hasattr(v, "__cuda_array_interface__")
        assert np.array_equal(ctx.fetch(k, shape), first[k]), k
    assert m.loo(mean=False, resident=True) == total and m.loo_mean is None


@pytest.mark.gpu
def test_the_variance_does_not_depend_on_the_trials_and_leaves_the_predictions_alone():
    name = "1d_siglist_12x40x4"
    c = _case(name)[0]
    a = _model(name)
    a.predict(c["x"], c["t"], type="both")
    held = (a.csd_pred, a.lfp_pred, a.t_pred, a.x_pred)
    pred = [np.array(v) for v in (a.csd_pred, a.lfp_pred)]
    a.loo()
    assert all(x is y for x, y in zip(held, (a.csd_pred, a.lfp_pred, a.t_pred, a.x_pred)))
    assert np.array_equal(a.csd_pred, pred[0]) and np.array_equal(a.lfp_pred, pred[1])
    lfp_b = C.synth_lfp(977, c["x"].shape[0], c["t"].shape[0], 7)                 # another seed, 7 trials instead of 4
    b = _model(name, lfp=lfp_b)
    b.loo()
    assert np.array_equal(a.loo_var, b.loo_var)
    assert b.loo_lpd.shape == (c["x"].shape[0], 7)
    ref = _formulas(name, lfp=lfp_b)                                              # ... and the other trials' scores are theirs
    tol = _tolerances(name)[0]
    assert np.max(np.abs(b.loo_lpd - ref["lpd"])) / np.max(np.abs(ref["lpd"])) < tol["lpd"]


@pytest.mark.gpu
def test_trial_shards_give_the_unsharded_columns_and_total():
    """Two ranks one after the other in this process (a process group per test does not fit a few seconds): a stand-in for
    gpcsd_amd.dist.TrialSharding with its partition and an all-reduce that records what it was given and returns it, so the
    test forms the sum over the ranks itself."""
    from gpcsd_amd.dist import TrialSharding

    class Rank(TrialSharding):
        def __init__(self, rank, world_size):
            self.rank, self.world_size, self.gather_predictions, self.sent = rank, world_size, False, []

        def allreduce_sum(self, values):
            self.sent.append(np.array(values, dtype=np.float64))
            return self.sent[-1]

    name = "1d_odd_17x37x5"                                                      # 5 trials: blocks of 3 and 2
    lfp = np.array(_case(name)[3])
    full = _model(name)
    total = full.loo()
    whole = {k: np.array(getattr(full, k)) for k in ("loo_var", "loo_mean", "loo_lpd", "loo_sse")}
    parts = []
    for r in range(2):
        m = _model(name, lfp=lfp)
        sh = Rank(r, 2)
        m.shard_trials(sh)
        sl = sh.local_slice(lfp.shape[2])
        part = m.loo()
        assert len(sh.sent) == 1 and sh.sent[0].shape == (1,) and sh.sent[0][0] == part == float(np.sum(m.loo_lpd))
        assert np.array_equal(m.loo_var, whole["loo_var"])                       # the same on every rank
        assert m.loo_mean.shape == whole["loo_mean"][:, :, sl].shape
        for k in ("loo_mean", "loo_lpd", "loo_sse"):                             # this rank's block of trials
            ref = whole[k][..., sl]
            assert np.max(np.abs(getattr(m, k) - ref)) <= 1e-12 * np.max(np.abs(ref)), (k, r)
        parts.append(part)
    assert abs(sum(parts) - total) <= 1e-12 * abs(total)


@pytest.mark.gpu
def test_errors():
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    lib = ctx._lib
    hp, _keep = ctx.make_hparams(100.0, 0.0, [200.0], [(_hip.KIND_SE, 20.0, 0.5)], 0.05, 1e-8)
    # no resident data: the library's -4, from both entry points
    one = np.zeros(1)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.gpcsd_loo_resident(ctx._h, ctypes.byref(hp), 1) == -4
    assert lib.gpcsd_loo(ctx._h, ctypes.byref(hp), dp(one), None, dp(one), dp(one)) == -4
    assert b"lfp not set" in lib.gpcsd_last_error(ctx._h)
    assert lib.gpcsd_loo_resident(ctx._h, None, 1) == -3
    # capacity, before anything is read or launched: the arrays hold ONE double each.  R * nt = 2^23 is the first row length a flat
    # operand cannot hold; nx * R = 2^31 the first row count
    call = lambda nx, R, nt, K: lib.gpcsd_loo_contract(ctx._h, dp(one), dp(one), dp(one), dp(one), nx, R, nt, K, None, dp(one), dp(one))
    assert call(1, 1 << 12, 1 << 11, 1) == _hip.ERR_CAPACITY
    assert call(1 << 20, 1 << 11, 1, 1) == _hip.ERR_CAPACITY
    assert call(1, 1, 1, 1 << 22) == _hip.ERR_CAPACITY
    assert call(0, 1, 1, 1) == -3 and call(1, 1, 1, 0) == -3
    # the context is as usable as before
    one[0] = 2.0
    lpd, sse = np.empty(1), np.empty(1)
    assert lib.gpcsd_loo_contract(ctx._h, dp(one), dp(one), dp(one), dp(one), 1, 1, 1, 1, None, dp(lpd), dp(sse)) == 0
    assert sse[0] == 4.0 and abs(lpd[0] - (0.5 * np.log(2.0) - 4.0 - HALF_LOG_2PI)) < 4e-15     # beta = 4, c = 2, e = 2
