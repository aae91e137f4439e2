"""Extended-precision statement of the trial-shift objective, its gradient and their rounding bounds (gpcsd_amd/csrc/shift.hip), and the
fixtures the tests share.  Everything is NumPy longdouble and follows include/gpcsd_hip.h (gpcsd_shift_eval) line by line:

    mean(tau)[x, k] = mu[x, k, 0] + sum_i  y_i[x, lo] + s_i[x, lo] ((t_k + tau_i) - t_lo)
    lo = clip(searchsorted_left(t, t_k + tau_i), 1, nt - 1) - 1,   s_i[x, lo] = (y_i[x, lo+1] - y_i[x, lo]) / (t_{lo+1} - t_lo)
    r = lfp_j - mean,  alpha = Qs^T r Qt,  beta = alpha / D,  Z = Qs beta Qt^T
    f = 1/2 sum alpha beta + 1/2 sum_i ((tau_i - mutau) / sigtau)^2
    g_i = -sum_{x,k} Z[x, k] s_i[x, lo(i, k)] + (tau_i - mutau) / sigtau^2

The new sample times t_k + tau_i are formed in float64, as SciPy's interp1d receives them: which segment a sample falls into -- and so
which one-sided derivative g is at a knot -- is decided by those doubles.  Nothing here knows about layouts, batches or the device."""
import functools
import os

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shift_objective.npz")

OFF_KNOT_TAUS = ((1.5, -2.3), (-3.25, 0.75), (45.2, -41.7))     # the last: every sample extrapolated, one component on each side
ON_KNOT_TAUS = ((0.0, 0.0), (6.0, 4.0), (1.5, -2.0))            # (the last: only the second component sits on knots)


def locate(t, tau):
    """(v, lo): the shifted sample times v[i, k] = t_k + tau_i (float64) and their segments lo[i, k], SciPy's choice."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    v = t[None, :] + np.asarray(tau, dtype=np.float64).reshape(-1)[:, None]
    lo = np.clip(np.searchsorted(t, v, side="left"), 1, t.size - 1) - 1
    return v, lo


def slopes(mu, t):
    """s[i, x, k] = (y_i[x, k+1] - y_i[x, k]) / (t[k+1] - t[k]), y_i = mu[:, :, i + 1]: (nseg, nx, nt - 1), longdouble."""
    y = np.moveaxis(np.asarray(mu, dtype=LD)[:, :, 1:], 2, 0)
    t = np.asarray(t, dtype=LD).reshape(-1)
    return (y[:, :, 1:] - y[:, :, :-1]) / (t[1:] - t[:-1])


def terms(mu, t, tau):
    """(interpolated term_i (nseg, nx, nt), gathered slopes s_i[x, lo(i, k)] (nseg, nx, nt)), longdouble."""
    y = np.moveaxis(np.asarray(mu, dtype=LD)[:, :, 1:], 2, 0)
    tl = np.asarray(t, dtype=LD).reshape(-1)
    s = slopes(mu, t)
    v, lo = locate(t, tau)
    i = np.arange(y.shape[0])[:, None, None]
    x = np.arange(y.shape[1])[None, :, None]
    sg = s[i, x, lo[:, None, :]]
    return y[i, x, lo[:, None, :]] + sg * (v.astype(LD) - tl[lo])[:, None, :], sg


def mean(mu, t, tau):
    return np.asarray(mu, dtype=LD)[:, :, 0] + terms(mu, t, tau)[0].sum(axis=0)


def parts(Qs, Qt, D, lfp_j, mu, t, tau, mutau=0.0, sigtau=10.0):
    """Everything about one point, longdouble: r, alpha, beta, Z, the gathered slopes sg, f, g, and the rounding bounds bound_f and
    bound_g (nseg,) a float64 evaluation of f and g is allowed (u = 2^-53):

        A = (2 nx + 2 nt + 33) |r| + (nseg + 6) (|lfp| + |mu_0| + sum_i |interpolated term_i|)
        C = |Qs| ((|Qs|^T A |Qt|) / D) |Qt|^T
        bound_g_i = u sum |s_i| C + (nx nt + 8) u sum |Z| |s_i| + 2 u |prior term of g_i|      (bound_f: |r| in place of |s_i|)

    The four products each carry (K + 8) u sum |a| |b| of the GEMM core and there is one division: (2 nx + 2 nt + 33) u on |r|
    pushed through the absolute values of the chain; the rounding of the residual itself goes through |K^-1| the same way; the
    final sum may run in any order."""
    Qs, Qt = np.asarray(Qs, dtype=LD), np.asarray(Qt, dtype=LD)
    nx, nt = Qs.shape[0], Qt.shape[0]
    D = np.asarray(D, dtype=LD).reshape(nx, nt)
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    nseg = tau.size
    lfp_j, mu0 = np.asarray(lfp_j, dtype=LD), np.asarray(mu, dtype=LD)[:, :, 0]
    term, sg = terms(mu, t, tau)
    r = lfp_j - (mu0 + term.sum(axis=0))
    alpha = Qs.T @ r @ Qt
    beta = alpha / D
    Z = Qs @ beta @ Qt.T
    z = (tau.astype(LD) - LD(mutau)) / LD(sigtau)
    f = (alpha * beta).sum() / 2 + (z * z).sum() / 2
    gprior = (tau.astype(LD) - LD(mutau)) / (LD(sigtau) * LD(sigtau))
    g = -(Z[None] * sg).sum(axis=(1, 2)) + gprior
    aQs, aQt = np.abs(Qs), np.abs(Qt)
    A = (2 * nx + 2 * nt + 33) * np.abs(r) + (nseg + 6) * (np.abs(lfp_j) + np.abs(mu0) + np.abs(term).sum(axis=0))
    C = aQs @ ((aQs.T @ A @ aQt) / D) @ aQt.T
    u = LD(U)
    bound_g = u * (np.abs(sg) * C[None]).sum(axis=(1, 2)) + (nx * nt + 8) * u * (np.abs(Z)[None] * np.abs(sg)).sum(axis=(1, 2)) \
        + 2 * u * np.abs(gprior)
    bound_f = u * (np.abs(r) * C).sum() + (nx * nt + 8) * u * (np.abs(Z) * np.abs(r)).sum() + 2 * u * (z * z).sum() / 2
    return {"r": r, "alpha": alpha, "beta": beta, "Z": Z, "sg": sg, "f": f, "g": g, "bound_f": bound_f, "bound_g": bound_g}


def f(Qs, Qt, D, lfp_j, mu, t, tau, mutau=0.0, sigtau=10.0):
    return parts(Qs, Qt, D, lfp_j, mu, t, tau, mutau, sigtau)["f"]


def g(Qs, Qt, D, lfp_j, mu, t, tau, mutau=0.0, sigtau=10.0):
    return parts(Qs, Qt, D, lfp_j, mu, t, tau, mutau, sigtau)["g"]


def batch(fx, trials, taus):
    """(f, g, bound_f, bound_g) of the points (trials[b], taus[b]) of a fixture dict, stacked, longdouble."""
    p = [parts(fx["Qs"], fx["Qt"], fx["Dvec"], fx["lfp"][:, :, j], fx["mu"], fx["t"], tau, fx["mutau"], fx["sigtau"])
         for j, tau in zip(trials, taus)]
    return tuple(np.array([q[k] for q in p]) for k in ("f", "g", "bound_f", "bound_g"))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def golden_fixture():
    """tests/golden/shift_objective.npz as it is: 12 x 40 x 5, nseg = 2, with the reference package's own nll at 5 x 4 points."""
    z = np.load(GOLDEN)
    return _freeze({"Qs": z["Qs"], "Qt": z["Qt"], "Dvec": z["Dvec"], "lfp": z["lfp"], "mu": z["mu_lfp"], "t": z["t"].reshape(-1),
                    "mutau": float(z["mutau"]), "sigtau": float(z["sigtau"]), "taus": z["taus"], "nll": z["nll"]})


@functools.lru_cache(maxsize=None)
def strong_fixture():
    """The golden fixture with component means that matter: mu[..., 1:] * 100, trials = mean(true_tau_j) + 0.1 golden lfp_j with
    true_tau = RandomState(3).uniform(-4, 4, (5, 2)).  (In the golden file the means are tiny against the noise: the data term of
    the gradient is about 1e-5 and a fit stops at tau0.)  Computed once and left unchanged."""
    g0 = golden_fixture()
    mu = np.array(g0["mu"], dtype=np.float64, copy=True)
    mu[..., 1:] *= 100
    true_tau = np.random.RandomState(3).uniform(-4.0, 4.0, (5, 2))
    lfp = np.stack([np.asarray(mean(mu, g0["t"], true_tau[j]), dtype=np.float64) + 0.1 * g0["lfp"][:, :, j] for j in range(5)], axis=2)
    return _freeze({"Qs": g0["Qs"], "Qt": g0["Qt"], "Dvec": g0["Dvec"], "lfp": lfp, "mu": mu, "t": g0["t"], "mutau": g0["mutau"],
                    "sigtau": g0["sigtau"], "true_tau": true_tau})


@functools.lru_cache(maxsize=None)
def odd_fixture(nseg=3):
    """Shapes at which the kernels can go wrong: nx = 17 (no multiple of the residual kernel's four electrodes per thread), nt = 37
    (no multiple of a wave), a NON-UNIFORM strictly increasing grid whose knots are multiples of 1/8 (so a tau that is a difference of
    two knots puts a sample exactly on a knot), random orthogonal Qs and Qt, D in [1e-2, 1e2], 4 trials.  Computed once."""
    nx, nt, ntrials = 17, 37, 4
    rs = np.random.RandomState(1700 + nseg)
    t = np.cumsum(rs.randint(2, 17, nt) / 8.0) - 3.0
    Qs = np.linalg.qr(rs.standard_normal((nx, nx)))[0]
    Qt = np.linalg.qr(rs.standard_normal((nt, nt)))[0]
    D = 10.0 ** rs.uniform(-2, 2, nx * nt)
    mu = np.cumsum(rs.standard_normal((nx, nt, nseg + 1)), axis=1)
    lfp = np.cumsum(rs.standard_normal((nx, nt, ntrials)), axis=1)
    return _freeze({"Qs": Qs, "Qt": Qt, "Dvec": D, "lfp": lfp, "mu": mu, "t": t, "mutau": 0.5, "sigtau": 3.0})


def odd_points(fx, B, seed=5):
    """(trials (B,), taus (B, nseg)) for odd_fixture: random shifts, and among the first seven points tau = 0, shifts beyond the span
    of t on either side (every sample extrapolated) and shifts that are differences of knots (samples exactly on knots)."""
    t = fx["t"]
    nseg = fx["mu"].shape[2] - 1
    rs = np.random.RandomState(seed)
    span = float(t[-1] - t[0])
    taus = rs.uniform(-6.0, 6.0, (B, nseg))
    special = [np.zeros(nseg), np.full(nseg, span + 1.25), np.full(nseg, -span - 2.5), np.resize([t[9] - t[4], t[3] - t[20], t[36] - t[35]], nseg),
               np.resize([span + 0.5, -span - 0.5, 0.0], nseg), np.resize([t[1] - t[0], 0.0, t[0] - t[36]], nseg)]
    order = [1, 0, 2, 3, 4, 5] if B == 1 else range(len(special))       # (B = 1: the point beyond the span)
    for b, k in zip(range(min(B, len(special))), order):
        taus[b] = special[k]
    trials = rs.randint(0, fx["lfp"].shape[2], B)
    return trials.astype(np.intc), taus
