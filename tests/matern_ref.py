"""Reference statements for the Matern-3/2 and Matern-5/2 temporal kernels (TEST INFRASTRUCTURE ONLY; no GPU, no library of the
project): the two kernels and their ell-derivatives in float64 and in numpy.longdouble (the 80-bit x87 format, as grad_ref.py),
and what the dense references of the other test files need to be reused for models of the new kinds.

    kind 3   k = sigma2 (1 + a) exp(-a),            a = sqrt(3) |d| / ell     dk/dell = sigma2 a^2 exp(-a) / ell
    kind 4   k = sigma2 (1 + a + a^2/3) exp(-a),    a = sqrt(5) |d| / ell     dk/dell = sigma2 a^2 (1 + a) exp(-a) / (3 ell)

The dense references (posterior_ref, fisher_ref, masked_ref, functional_ref, the helpers of test_predict_at / test_predict_var /
test_loo) reach the kernel through oracle.temporal_gram and their case through helpers.load_model_case(name).  `world` swaps both
for the duration of ONE test (pytest's monkeypatch undoes it): temporal_gram also knows kinds 3 and 4, and a name "matern:<golden
case>" loads that golden case -- geometry, data, every hyper-parameter value -- with only the kinds swapped (SWAPS).  The references
cache by name, and no other test uses these names, so nothing a test outside `world` sees is changed.  fisher_ref.temporal writes
the ell-derivative out per kind; its restatement for all four kinds is `fisher_temporal`."""
import numpy as np

import grad_ref as GR
from oracle import gpcsd_oracle as O

LD = np.longdouble
SE, MATERN, HOST, MATERN32, MATERN52 = 0, 1, 2, 3, 4
PREFIX = "matern:"
SWAPS = {"1d_odd_17x37x5": (MATERN32,),                      # odd sizes, one component
         "1d_siglist_12x40x4": (MATERN52, MATERN32),         # noise list
         "2d_grid_48x40x2": (SE, MATERN52)}                  # mirror-folded path, an old and a new kind in one sum
CASES = [PREFIX + n for n in SWAPS]

if np.finfo(LD).eps > 2.0 ** -60:          # (as grad_ref.py: a long double that is float64 would make every measure blind below 1 u)
    raise ImportError("matern_ref needs a long double wider than float64 (eps %g here)" % np.finfo(LD).eps)

_ORACLE_GRAM = O.temporal_gram             # the oracle's own, taken at import: `world` replaces the module attribute


# ------------------------------------------------------------------------------------------------ the kernels
def unit_kernel(kind, d, ell, ft=np.float64):
    """(k, dk/dell) at unit variance for distances d (any shape), in the float type ft; d and ell are taken as exact float64."""
    d = np.asarray(d, dtype=np.float64).astype(ft)
    ell = ft(ell)
    with np.errstate(under="ignore"):
        if kind == SE:
            k = np.exp(ft(-0.5) * (d * d) / (ell * ell))
            return k, k * (d * d) / (ell * ell * ell)
        if kind == MATERN:
            k = np.exp(-np.abs(d) / ell)
            return k, k * np.abs(d) / (ell * ell)
        if kind == MATERN32:
            a = np.sqrt(ft(3)) * np.abs(d) / ell
            e = np.exp(-a)
            return (ft(1) + a) * e, a * a * e / ell
        if kind == MATERN52:
            a = np.sqrt(ft(5)) * np.abs(d) / ell
            e = np.exp(-a)
            return (ft(1) + a + a * a / ft(3)) * e, a * a * (ft(1) + a) * e / (ft(3) * ell)
    raise ValueError("unknown temporal kernel kind %r" % (kind,))


def scaled_distance(kind, d, ell):
    """a = sqrt(3) |d| / ell or sqrt(5) |d| / ell (float64), the argument of the exponential."""
    return np.sqrt({MATERN32: 3.0, MATERN52: 5.0}[kind]) * np.abs(np.asarray(d, dtype=np.float64)) / ell


def gram(kind, t, tprime, ell, sigma2, ft=np.float64):
    """sigma2 k(t_i - t'_j) as (len(t), len(t')), in the float type ft."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    tp = np.asarray(tprime, dtype=np.float64).reshape(1, -1)
    if ft is LD:
        d = t.astype(LD) - tp.astype(LD)
        return LD(sigma2) * _unit_ld(kind, d, ell)[0]
    return sigma2 * unit_kernel(kind, t - tp, ell)[0]


def _unit_ld(kind, d, ell):
    """unit_kernel for distances that are long double already (differences of float64 times are not float64 numbers)"""
    ell = LD(ell)
    if kind == SE:
        k = np.exp(LD(-0.5) * (d * d) / (ell * ell))
        return k, k * (d * d) / (ell * ell * ell)
    if kind == MATERN:
        k = np.exp(-np.abs(d) / ell)
        return k, k * np.abs(d) / (ell * ell)
    a = np.sqrt(LD({MATERN32: 3, MATERN52: 5}[kind])) * np.abs(d) / ell
    e = np.exp(-a)
    if kind == MATERN32:
        return (LD(1) + a) * e, a * a * e / ell
    return (LD(1) + a + a * a / LD(3)) * e, a * a * (LD(1) + a) * e / (LD(3) * ell)


def dgram(kind, t, ell, sigma2, name, ft=np.float64):
    """d (sigma2 k) / d ell or / d sigma2 on the grid t, in the float type ft."""
    t = np.asarray(t, dtype=np.float64).reshape(-1).astype(ft)
    d = t[:, None] - t[None, :]
    k, dk = _unit_ld(kind, d, ell) if ft is LD else unit_kernel(kind, d, ell)
    if name == "ell":
        return ft(sigma2) * dk
    if name == "sigma2":
        return k
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ temporal_grad (grad_ref's, four kinds)
def _temporal_terms(Gt, t, kinds, ell, sigma2, ft):
    """grad_ref._temporal_terms with the two new kinds: terms[2c] = Gt sigma2_c dk_c / d ell_c, terms[2c + 1] = Gt k_c."""
    G = np.asarray(Gt, dtype=np.float64).astype(ft)
    tt = np.asarray(t, dtype=np.float64).reshape(-1).astype(ft)
    d = tt[:, None] - tt[None, :]
    out = []
    for kind, l, s2 in zip(kinds, ell, sigma2):
        k, dk = _unit_ld(kind, d, l) if ft is LD else unit_kernel(kind, d, l)
        out += [G * ft(s2) * dk, G * k]
    return out


def temporal_grad_ld(Gt, t, kinds, ell, sigma2):
    vd = [GR._both(x) for x in _temporal_terms(Gt, t, kinds, ell, sigma2, LD)]
    return np.array([v for v, _ in vd], dtype=LD), np.array([d for _, d in vd], dtype=LD)


def temporal_grad_f64(Gt, t, kinds, ell, sigma2):
    with np.errstate(under="ignore"):
        return np.array([np.sum(x) for x in _temporal_terms(Gt, t, kinds, ell, sigma2, np.float64)])


# ------------------------------------------------------------------------------------------------ the dense references' two hooks
def temporal_gram(kind, t, tprime, ell, sigma2):
    """oracle.temporal_gram that also knows kinds 3 and 4 (kinds 0 and 1 are the oracle's own lines)."""
    if kind in (MATERN32, MATERN52):
        return gram(kind, t, tprime, ell, sigma2)
    return _ORACLE_GRAM(kind, t, tprime, ell, sigma2)


def fisher_temporal(geom, hp):
    """fisher_ref.temporal for all four kinds: -> Kt, [dKt/dell_c, dKt/dsigma2_c per component]"""
    out = []
    for kind, ell, s2 in hp["temporal"]:
        out += [dgram(kind, geom.t, ell, s2, "ell"), dgram(kind, geom.t, ell, s2, "sigma2")]
    return sum(temporal_gram(kind, geom.t, geom.t, ell, s2) for kind, ell, s2 in hp["temporal"]), out


def swapped(name):
    """helpers.load_model_case of the golden case behind "matern:<golden case>", only the kinds swapped"""
    import helpers
    golden = name[len(PREFIX):]
    c, g, geom, hp, lfp = helpers.load_model_case(golden)
    kinds = SWAPS[golden]
    assert len(kinds) == len(c["temporal"])
    c = dict(c, temporal=[(k,) + tuple(tc[1:]) for k, tc in zip(kinds, c["temporal"])])
    hp = dict(hp, temporal=[(k, ell, s2) for k, (_, ell, s2) in zip(kinds, hp["temporal"])])
    return c, g, geom, hp, lfp


def world(monkeypatch):
    """For the rest of the calling test: the oracle's temporal_gram knows the new kinds, fisher_ref.temporal too, and every reference
    module loads "matern:<golden case>" as that case with the kinds of SWAPS."""
    import fisher_ref
    import helpers
    import masked_ref
    import test_fisher
    import test_loo
    import test_predict_at
    import test_predict_var
    real_load, real_mask = helpers.load_model_case, masked_ref.mask_for

    def load(name):
        return swapped(name) if name.startswith(PREFIX) else real_load(name)

    def mask_for(name, pattern):                 # (seeded by the golden case's name and shape: the kinds play no part)
        return real_mask(name[len(PREFIX):] if name.startswith(PREFIX) else name, pattern)

    monkeypatch.setattr(O, "temporal_gram", temporal_gram)
    monkeypatch.setattr(fisher_ref, "temporal", fisher_temporal)
    monkeypatch.setattr(masked_ref, "mask_for", mask_for)
    for mod in (masked_ref, test_fisher, test_loo, test_predict_at, test_predict_var):
        monkeypatch.setattr(mod, "load_model_case", load)
    return load


def model_for(name, lfp=None, classes=None):
    """The mirrored Python class of case `name` ("matern:..." or a golden case), configured as tests/test_hip_parity.py configures
    it, its temporal covariances built by classes[kind](t) (default: the library's own classes per kind)."""
    from gpcsd_amd import covariances as CV
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    import helpers
    c, g, geom, hp, data = swapped(name) if name.startswith(PREFIX) else helpers.load_model_case(name)
    if classes is None:
        classes = {SE: CV.GPCSDTemporalCovSE, MATERN: CV.GPCSDTemporalCovMatern, MATERN32: CV.GPCSDTemporalCovMatern32,
                   MATERN52: CV.GPCSDTemporalCovMatern52}
    np.random.seed(0)
    tcl = []
    for kind, ell, s2 in hp["temporal"]:
        tc = classes[kind](c["t"])
        tc.params["ell"]["value"] = ell
        tc.params["sigma2"]["value"] = float(s2)
        tcl.append(tc)
    data = np.array(data if lfp is None else lfp)
    if c["dim"] == 1:
        m = GPCSD1D(data, c["x"], c["t"], a=c["a"], b=c["b"], ngl=c["ngl"], temporal_cov_list=tcl)
        m.spatial_cov.params["ell"]["value"] = c["ell_s"][0]
    else:
        m = GPCSD2D(data, c["x"], c["t"], ngl1=c["ngl1"], ngl2=c["ngl2"], temporal_cov_list=tcl, eps=c["eps"])
        m.spatial_cov.params["ell1"]["value"] = c["ell_s"][0]
        m.spatial_cov.params["ell2"]["value"] = c["ell_s"][1]
    m.R["value"] = c["R"]
    if np.ndim(c["sig2n"]) == 0:
        m.sig2n["value"] = c["sig2n"]
    else:                                        # a noise list with its list of priors (tests/test_hip_parity.py's gradient test)
        from gpcsd_amd.priors import GPCSDHalfNormalPrior
        n = len(c["sig2n"])
        m.sig2n = {"value": np.array(c["sig2n"], dtype=np.float64), "prior": [GPCSDHalfNormalPrior(0.1) for _ in range(n)],
                   "min": [1e-8] * n, "max": [0.5] * n}
    return m


# ------------------------------------------------------------------------------------------------ the dense gradient
def dense_loglik_and_grad(geom, hp, lfp):
    """(loglik, gradient in the natural parameters [R, ell_s.., (ell_t, sigma2_t).., sig2n]) of
    K = kron(Ks + jitter I, Kt) + sig2n I (scalar noise), the gradient as 1/2 tr((alpha alpha^T - R K^-1) d_i K) by dense solves:
    fisher_ref.scores_and_info's scores summed over the trials (call inside `world`)."""
    import fisher_ref
    nx, nt, R = lfp.shape
    ref = fisher_ref.scores_and_info(geom, hp, lfp)
    Ks = O.spatial_kphi(geom, hp) + hp["jitter"] * np.eye(nx)
    ll = O.loglik_from_K(lfp, Ks, O.temporal_sum(hp["temporal"], geom.t), hp["sig2n"])
    scale = np.abs(ref["quad"]).sum(axis=0) + R * np.abs(ref["trace"])
    return ll, ref["scores"].sum(axis=0), scale, ref
