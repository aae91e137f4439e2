"""NumPy restatements behind tests/test_masked_ref.py and tests/test_predict_masked.py: posterior means and the log-likelihood
when samples of a trial are missing (gpcsd_predict_masked / gpcsd_loglik_masked; no reference counterpart), stated twice on the
oracle's pieces.

  dense(name, pattern)   Cholesky of K_OO per trial with one float64 refinement step: alpha = K_OO^-1 y_O scattered to the grid
                         (zeros on the missing samples), y_O^T K_OO^-1 y_O and log det K_OO
  schur(name, pattern)   the same three things from the full-grid decomposition K = (Qs (x) Qt) diag(D) (Qs (x) Qt)^T and the Schur
                         complement G = (K^-1)_MM of the missing set -- what the library computes

Both return {"alpha": (R, nx, nt), "rows": (R, 2) = (log det K_OO, quadratic form) per trial, "n_obs": int}; a trial without an
observed sample has alpha = 0 and the row (0, 0).  K is the model of predict / predict_at: no jitter, a noise list on the
eigen-index (oracle.eig_D).  `predictions` contracts an alpha with the cross-covariances as test_predict_at._contract does."""
import functools

import numpy as np

import test_predict_at as PA
from helpers import load_model_case
from oracle import gpcsd_oracle as O

CASES = ["1d_odd_17x37x5", "1d_siglist_12x40x4", "2d_grid_48x40x2", "1d_wide_24x60x3"]      # the second has a noise list; the last cond 2e8
PATTERNS = ["scattered3", "window6", "electrode", "random30", "mixed", "one_observed", "none_observed", "all", "electrode2d"]


def mask_for(name, pattern):
    """Boolean mask (nx, nt, R) -- (nx, nt) for "electrode2d" --, True = observed; seeded by case and pattern.  Every pattern but
    "random30" (every trial) and "electrode2d" (all trials by construction) sits in trial 1; the other trials are fully observed."""
    c = PA.C.model_cases()[name]
    nx, nt, R = c["x"].shape[0], c["t"].shape[0], c["R_trials"]
    rng = np.random.RandomState(1000 * CASES.index(name) + PATTERNS.index(pattern))
    full = np.ones((nx, nt, R), dtype=bool)
    one = np.ones((nx, nt), dtype=bool)
    xe, t0 = int(rng.randint(nx)), int(rng.randint(nt - 6))
    if pattern == "scattered3":
        one[0, 0] = one[nx - 1, nt - 1] = False
        one[1 + rng.randint(nx - 2), 1 + rng.randint(nt - 2)] = False
    elif pattern == "window6":
        one[:, t0:t0 + 6] = False
    elif pattern in ("electrode", "electrode2d"):
        one[xe, :] = False
    elif pattern == "random30":
        return rng.random_sample((nx, nt, R)) >= 0.30
    elif pattern == "mixed":
        one[:, t0:t0 + 6] = False
        one[xe, :] = False
        one &= rng.random_sample((nx, nt)) >= 0.05
    elif pattern == "one_observed":
        one[:] = False
        one[rng.randint(nx), rng.randint(nt)] = True
    elif pattern == "none_observed":
        one[:] = False
    elif pattern != "all":
        raise KeyError(pattern)
    if pattern == "electrode2d":
        return one
    full[:, :, 1] = one
    return full


def mask3(mask, R):
    return mask if mask.ndim == 3 else np.repeat(mask[:, :, None], R, axis=2)


@functools.lru_cache(maxsize=None)
def case(name):
    c, g, geom, hp, lfp = load_model_case(name)
    Ks, Kt = O.spatial_kphi(geom, hp), O.temporal_sum(hp["temporal"], geom.t)
    Qs, Qt, D = O.eig_D(Ks, Kt, hp["sig2n"])
    nx, nt = Ks.shape[0], Kt.shape[0]
    if np.ndim(hp["sig2n"]) == 0:
        K = O.mykron(Ks, Kt) + float(hp["sig2n"]) * np.eye(nx * nt)      # independent of the decomposition
    else:
        Phi = O.mykron(Qs, Qt)                                            # the noise list lives on the eigen-index: K is defined by it
        K = (Phi * D[None, :]) @ Phi.T
        K = 0.5 * (K + K.T)
    for a in (Qs, Qt, D, K, lfp):
        a.setflags(write=False)
    return {"c": c, "g": g, "geom": geom, "hp": hp, "lfp": lfp, "Qs": Qs, "Qt": Qt, "D": D.reshape(nx, nt), "K": K}


@functools.lru_cache(maxsize=None)
def dense(name, pattern):
    cs = case(name)
    lfp, K = cs["lfp"], cs["K"]
    nx, nt, R = lfp.shape
    mask = mask3(mask_for(name, pattern), R)
    alpha, rows = np.zeros((R, nx, nt)), np.zeros((R, 2))
    factors = {}
    for r in range(R):
        obs = np.flatnonzero(mask[:, :, r].reshape(-1))
        if obs.size == 0:
            continue
        key = mask[:, :, r].tobytes()
        if key not in factors:
            Koo = K[np.ix_(obs, obs)]
            factors[key] = (Koo, np.linalg.cholesky(Koo))
        Koo, L = factors[key]
        solve = lambda b: np.linalg.solve(L.T, np.linalg.solve(L, b))
        y = lfp[:, :, r].reshape(-1)[obs]
        a = solve(y)
        a = a + solve(y - Koo @ a)                                        # one refinement step
        alpha[r].reshape(-1)[obs] = a
        rows[r] = (2.0 * np.sum(np.log(np.diag(L))), y @ a)
    alpha.setflags(write=False)
    rows.setflags(write=False)
    return {"alpha": alpha, "rows": rows, "n_obs": int(mask.sum())}


@functools.lru_cache(maxsize=None)
def schur(name, pattern):
    cs = case(name)
    lfp, Qs, Qt, D = cs["lfp"], cs["Qs"], cs["Qt"], cs["D"]
    nx, nt, R = lfp.shape
    mask = mask3(mask_for(name, pattern), R)
    ainv = lambda Y: Qs @ ((Qs.T @ Y @ Qt) / D) @ Qt.T                   # A^-1 on a (nx, nt) grid
    logdet_a = np.sum(np.log(D))
    alpha, rows = np.zeros((R, nx, nt)), np.zeros((R, 2))
    for r in range(R):
        obs = mask[:, :, r]
        if not obs.any():
            continue
        yt = np.where(obs, lfp[:, :, r], 0.0)
        V = ainv(yt)
        xi, ti = np.nonzero(~obs)
        if xi.size == 0:
            alpha[r], rows[r] = V, (logdet_a, np.sum(yt * V))
            continue
        Phi = (Qs[xi][:, :, None] * Qt[ti][:, None, :]).reshape(xi.size, nx * nt)
        G = (Phi / D.reshape(1, -1)) @ Phi.T
        G = 0.5 * (G + G.T)
        L = np.linalg.cholesky(G)
        cm = V[xi, ti]
        w = np.linalg.solve(L, cm)
        U = np.zeros((nx, nt))
        U[xi, ti] = -np.linalg.solve(L.T, w)
        alpha[r] = np.where(obs, ainv(yt + U), 0.0)
        rows[r] = (logdet_a + 2.0 * np.sum(np.log(np.diag(L))), np.sum(yt * V) - w @ w)
    return {"alpha": alpha, "rows": rows, "n_obs": int(mask.sum())}


def sites(name):
    """3 sites interpolated between consecutive electrodes."""
    import posterior_ref
    return posterior_ref.sites(name)


def predictions(name, alpha, z, tstar):
    """{"csd", "csd_list", "lfp", "lfp_list"} at sites z and times tstar from the weights alpha (R, nx, nt)."""
    cs = case(name)
    geom, hp = cs["geom"], cs["hp"]
    grams = [O.temporal_gram(kind, tstar, geom.t, ell, s2) for kind, ell, s2 in hp["temporal"]]
    return PA._contract(geom, hp, alpha, np.asarray(z, dtype=np.float64), grams)
