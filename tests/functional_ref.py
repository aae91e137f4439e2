"""NumPy restatement behind tests/test_predict_functionals.py: posterior mean and covariance of linear functionals <W_j, f> of the
CSD / LFP field in the eigen-basis (gpcsd_predict_functionals), and the seven functionals the tests use.

With (Qs, Qt, D) of test_predict_var._case (no jitter), M1 = Kcross^T Qs, P_c = Qt^T k_c(t*, t)^T, Bm_r = (Qs^T y_r Qt) / D, Kzz the
prior spatial covariance at the sites (posterior_ref._spatial_blocks, both triangles from the lower one) and Ktt_c = k_c(t*, t*):

    alpha_j^c = M1^T W_j P_c^T  (nx, nt),  alpha_j^C = sum_c alpha_j^c
    expl_p[j, k] = <alpha_j^p, alpha_k^p / D>,  mean_p[j, r] = <alpha_j^p, Bm_r>,  prior_c[j, k] = <W_j, Kzz W_k Ktt_c>,  prior_C = sum_c

Planes 0 .. C - 1 are the temporal components, plane C their sum."""
import functools

import numpy as np

import cases as C
import posterior_ref as PR
import test_predict_var as PV
from oracle import gpcsd_oracle as O

NAMES = ("csd", "lfp")
DISTINCT = (0, 1, 2, 3, 4)        # the distinct non-zero ones of functionals(): point, box, contrast, two random fields
ZERO, DUPLICATE = 5, 6            # ... the zero field, and the box once more


def functionals(nz, nts, seed=0):
    """(7, nz, nts): a point mass, a box average, a contrast of two boxes, two random fields (the second scaled by 1e3), the zero
    field, a duplicate of the box.  Any nz, nts >= 1 (degenerate grids give degenerate boxes)."""
    rs = np.random.RandomState(1000 + seed)
    W = np.zeros((7, nz, nts))
    W[0, nz // 2, nts // 2] = 1.0
    z1, s0, s1 = max(1, (nz + 1) // 2), nts // 4, max(nts // 4 + 1, (3 * nts) // 4)
    W[1, :z1, s0:s1] = 1.0 / (z1 * (s1 - s0))
    if nz >= 2:
        h = nz // 2
        W[2, :h, :s1] = 1.0 / (h * s1)
        W[2, nz - h:, s0:] -= 1.0 / (h * (nts - s0))
    elif nts >= 2:
        h = nts // 2
        W[2, :, :h] = 1.0 / h
        W[2, :, nts - h:] -= 1.0 / h
    else:
        W[2] = -0.5
    W[3] = rs.standard_normal((nz, nts))
    W[4] = 1e3 * rs.standard_normal((nz, nts))
    W[6] = W[1]
    return W


def point_masses(nz, nts):
    """(nz nts, nz, nts): functional z nts + s picks f(z, t*_s)."""
    return np.eye(nz * nts).reshape(nz * nts, nz, nts)


@functools.lru_cache(maxsize=None)
def _projected_data(name):
    """Bm (nx, nt, R) = (Qs^T y_r Qt) / D of the case's own trials."""
    c, _, _, Qs, Qt, D = PV._case(name)
    y = np.atleast_3d(C.case_lfp(c))
    Bm = np.einsum("xa,xtr,tb->abr", Qs, y, Qt) / D[:, :, None]
    Bm.setflags(write=False)
    return Bm


def functional_ref(name, z, tstar, W):
    """{"csd" / "lfp": {"mean": (C + 1, J, R), "expl": (C + 1, J, J), "prior": (C + 1, J, J)}}; cov = prior - expl."""
    c, geom, hp, Qs, Qt, D = PV._case(name)
    z = np.asarray(z, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    zz, cross = PR._spatial_blocks(geom, hp, z)
    P = [Qt.T @ k.T for k in PV._grams(hp, geom, tstar)]                              # (nt, ntstar)
    Ktt = [O.temporal_gram(kind, tstar, tstar, ell, s2) for kind, ell, s2 in hp["temporal"]]
    Bm = _projected_data(name)
    out = {}
    for nm in NAMES:
        M1 = cross[nm].T @ Qs                                                            # (nz, nx)
        Kzz = np.tril(zz[(nm, nm)]) + np.tril(zz[(nm, nm)], -1).T
        alpha = [np.einsum("zx,jzs,is->jxi", M1, W, p) for p in P]
        alpha.append(sum(alpha))
        prior = [np.einsum("jzs,zw,kwu,us->jk", W, Kzz, W, k, optimize=True) for k in Ktt]
        prior.append(sum(prior))
        out[nm] = {"mean": np.stack([np.einsum("jxi,xir->jr", a, Bm) for a in alpha]),
                   "expl": np.stack([np.einsum("jxi,kxi->jk", a / D[None], a) for a in alpha]),
                   "prior": np.stack([0.5 * (p + p.T) for p in prior])}
    return out


def dense_functionals(name, z, tstar, W):
    """The component SUM by the dense statement: {"csd" / "lfp": {"mean": (J, R), "expl": (J, J), "prior": (J, J)}} from
    W (K** - K*^T K^-1 K*) W^T of posterior_ref.dense_posterior and the dense posterior mean field K*^T K^-1 y."""
    c, _, _, Qs, Qt, D = PV._case(name)
    y = np.atleast_3d(C.case_lfp(c))
    Wf = np.asarray(W, dtype=np.float64).reshape(W.shape[0], -1)
    out = {}
    for nm in NAMES:
        post, prior = PR.dense_posterior(name, z, tstar, nm)
        B = PR._projected_cross(name, z, tstar, nm)[0]                                 # ((x', i'), (z, j))
        U = O.mykron(Qs, Qt)
        field = B.T @ ((U.T @ y.reshape(-1, y.shape[2])) / D.reshape(-1, 1))            # ((z, j), R)
        out[nm] = {"mean": Wf @ field, "expl": Wf @ (prior - post) @ Wf.T, "prior": Wf @ prior @ Wf.T}
    return out


def scaled_errors(got, ref):
    """(explained, prior, mean) errors of one plane as the tests gate them: the explained term elementwise relative to
    sqrt(e_jj e_kk) over the non-zero functionals, the prior and the means relative to their largest entry.  got / ref: dicts with
    "expl", "prior", "mean"."""
    e = np.sqrt(np.abs(np.diag(ref["expl"])))
    on = e > 0
    scale = np.outer(e[on], e[on])
    d_expl = np.abs(got["expl"] - ref["expl"])[np.ix_(on, on)] / scale
    return (float(d_expl.max()) if d_expl.size else 0.0,
            float(np.max(np.abs(got["prior"] - ref["prior"])) / np.max(np.abs(ref["prior"]))),
            float(np.max(np.abs(got["mean"] - ref["mean"])) / max(np.max(np.abs(ref["mean"])), np.finfo(float).tiny)))
