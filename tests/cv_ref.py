"""References of the leave-electrodes-out scores (cv_electrodes; no reference counterpart): the formulas in NumPy, brute-force
deletion from the dense covariance, and the kernels' operations in long double with a first-order rounding bound."""
import numpy as np

U = 2.0 ** -53
HALF_LOG_2PI = 0.91893853320467274178                      # log(2 pi) / 2 correctly rounded
HALF_LOG_2PI_LD = np.longdouble("0.91893853320467274178032973640562")


# ------------------------------------------------------------------------------------------------ the formulas in NumPy
def cv_formulas(Qs, Qt, D, Y, folds):
    """The closed form from the eigen-form K = (Qs (x) Qt) diag(D) (Qs (x) Qt)^T (D (nx, nt)) and the data Y (nx, nt, R), for a
    sequence of disjoint folds:  G_j[a][b] = sum_x' Qs[a][x'] Qs[b][x'] / D[x'][j],  u_j,r = (Qs ((Qs^T Y_r Qt) / D))[F][j],
    e_j,r = G_j^-1 u_j,r.  -> {"var" (nx, nt), "resid" = y - cv_mean (nx, nt, R), "mean", "lpd" (nfolds, R), "sse" (nx, R),
    "total"}; rows of electrodes in no fold are NaN."""
    nx, nt, R = Y.shape
    Dinv = 1.0 / D
    alpha = Qs.T @ np.moveaxis(Y, 2, 0) @ Qt                                    # (R, nx, nt)
    V = Qs @ (alpha / D)                                                        # (R, nx, nt): K^-1 y in the temporal eigen-basis
    out = {"var": np.full((nx, nt), np.nan), "resid": np.full((nx, nt, R), np.nan), "lpd": np.empty((len(folds), R)),
           "sse": np.full((nx, R), np.nan)}
    Q2 = Qt * Qt
    for n, F in enumerate(folds):
        F = np.asarray(F, dtype=np.int64)
        f = F.size
        G = np.einsum("ax,bx,xj->jab", Qs[F], Qs[F], Dinv)                      # (nt, f, f)
        u = np.transpose(V[:, F, :], (2, 1, 0))                                 # (nt, f, R)
        e = np.linalg.solve(G, u)
        Ginv = np.linalg.inv(G)
        logdet = np.linalg.slogdet(G)[1].sum()
        out["lpd"][n] = 0.5 * logdet - 0.5 * np.einsum("jar,jar->r", u, e) - f * nt * HALF_LOG_2PI
        out["sse"][F] = np.einsum("jar,jar->ar", e, e)
        out["var"][F] = np.einsum("tj,jaa->at", Q2, Ginv)
        out["resid"][F] = np.einsum("tj,jar->atr", Qt, e)
    out["mean"] = Y - out["resid"]
    out["total"] = float(out["lpd"].sum())
    return out


# ------------------------------------------------------------------------------------------------ brute-force deletion
def brute_force_fold(K, y, F, nt):
    """All f nt rows and columns of the fold removed from the dense K (index (x, t)), the rest factored: the conditional mean
    (f, nt, R), the diagonal of the conditional covariance (f, nt) and the joint log density (R,) of the held-out block."""
    import scipy.linalg
    F = np.asarray(F, dtype=np.int64)
    n, R = y.shape
    held = (F[:, None] * nt + np.arange(nt)[None, :]).ravel()
    keep = np.setdiff1d(np.arange(n), held)
    if keep.size:
        cf = scipy.linalg.cho_factor(K[np.ix_(keep, keep)], lower=True)
        sol = scipy.linalg.cho_solve(cf, np.column_stack([K[np.ix_(keep, held)], y[keep]]))
        cov = K[np.ix_(held, held)] - K[np.ix_(held, keep)] @ sol[:, :held.size]
        mean = K[np.ix_(held, keep)] @ sol[:, held.size:]
    else:                                                                       # everything held out: the prior
        cov, mean = K[np.ix_(held, held)], np.zeros((held.size, R))
    cov = 0.5 * (cov + cov.T)
    L = np.linalg.cholesky(cov)
    z = scipy.linalg.solve_triangular(L, y[held] - mean, lower=True)
    lpd = -0.5 * (z * z).sum(axis=0) - np.log(np.diag(L)).sum() - held.size * HALF_LOG_2PI
    return mean.reshape(F.size, nt, R), np.diag(cov).reshape(F.size, nt), lpd


# ------------------------------------------------------------------------------------------------ the kernels in long double
def _chol_ld(G):
    """Lower Cholesky factors of a batch (nb, f, f) in long double."""
    f = G.shape[1]
    L = np.zeros_like(G)
    for i in range(f):
        for k in range(i + 1):
            s = G[:, i, k] - (L[:, i, :k] * L[:, k, :k]).sum(axis=1)
            L[:, i, k] = np.sqrt(s) if k == i else s / L[:, k, k]
    return L


def _inv_lower_ld(L):
    """Inverses of a batch of lower triangular matrices, by forward substitution."""
    f = L.shape[1]
    X = np.zeros_like(L)
    for a in range(f):
        for k in range(a, f):
            s = (1.0 if k == a else 0.0) - (L[:, k, a:k] * X[:, a:k, a]).sum(axis=1)
            X[:, k, a] = s / L[:, k, k]
    return X


def efold_bound(A, W, V, folds):
    """Reference values in long double and a first-order rounding bound for every output of gpcsd_efold_contract, from the
    kernels' own operations (u = 2^-53, gamma_n = n u / (1 - n u); d. marks an error bound; F a fold of f electrodes, j the column):

      G     = sum_k (A_a A_b) W     the operand product, the multiplier's K fused multiply-adds, the order of its groups:
                                    d.G = (K + 2) u sum_k |A_a| |A_b| W
      L L^T = G, L z = u, L^T e = z Cholesky and two substitutions, together backward stable with gamma_{3f+1} |L| |L^T|:
                                    d.e = |G^-1| (d.G + gamma_{3f+1} |L| |L^T|) |e|                         (the output E)
      p_a   = sum_k x_k^2           x = column a of L^-1 by substitution -- the same perturbation of G seen through G^-1 --, then f
                                    products and f - 1 additions:
                                    d.p = (|G^-1| (d.G + gamma_{3f+1} |L| |L^T|) |G^-1|)_aa + f u p        (the output pdiag)
      q     = sum_i u_i e_i         d.q = sum_i |u_i| d.e_i + f u sum_i |u_i e_i|
      ld    = sum_i log(pivot_i)    log det of the perturbed G, the square roots (u each, twice in the log), each log within an ulp
                                    of its result, f - 1 additions:
                                    d.ld = sum_ab |G^-1|_ab (d.G + gamma_{3f+1} |L| |L^T|)_ab + 2 f u + (f + 1) u sum_i |log pivot_i|
      e^2                           d.(e^2) = 2 |e| d.e + u e^2
      the sums over the nt columns, in whatever order (the lanes of a chunk, the chunks):
                                    d.S = sum_j d.s_j + (nt - 1) u sum_j |s_j|            for s = ld, q, e^2
      lpd   = (S_ld / 2 - S_q / 2) - (f nt) h     the halvings are exact; h = log(2 pi) / 2 is a rounded constant, its product
                                    with the integer f nt one rounding:
                                    d.lpd = d.S_ld / 2 + d.S_q / 2 + u |S_ld / 2 - S_q / 2| + 2 u f nt h + u |lpd|

    -> (ref, bound): dicts with "E" (nx, R, nt), "pdiag" (nx, nt), "lpd" (nfolds, R), "sse" (nx, R); rows of electrodes in no
    fold are NaN in both."""
    ld = np.longdouble
    A, W, V = A.astype(ld), W.astype(ld), V.astype(ld)
    nx, K = A.shape
    nt = W.shape[1]
    R = V.shape[1]
    nan = ld(np.nan)
    ref = {"E": np.full((nx, R, nt), nan), "pdiag": np.full((nx, nt), nan), "lpd": np.zeros((len(folds), R), dtype=ld),
           "sse": np.full((nx, R), nan)}
    bound = {k: v.copy() for k, v in ref.items()}
    for n, F in enumerate(folds):
        F = np.asarray(F, dtype=np.int64)
        f = F.size
        gam = (3 * f + 1) * U / (1 - (3 * f + 1) * U)
        G = np.einsum("ak,bk,kj->jab", A[F], A[F], W)                           # (nt, f, f)
        dG = (K + 2) * U * np.einsum("ak,bk,kj->jab", np.abs(A[F]), np.abs(A[F]), W)
        L = _chol_ld(G)
        Li = _inv_lower_ld(L)
        Gi = np.einsum("jka,jkb->jab", Li, Li)
        aL = np.abs(L)
        pert = dG + gam * np.einsum("jak,jbk->jab", aL, aL)                     # d.G + gamma |L| |L^T|
        aGi = np.abs(Gi)
        u = np.transpose(V[F], (2, 0, 1))                                       # (nt, f, R)
        e = Gi @ u
        d_e = aGi @ (pert @ np.abs(e))
        ref["E"][F] = np.transpose(e, (1, 2, 0))
        bound["E"][F] = np.transpose(d_e, (1, 2, 0))
        p = np.einsum("jaa->ja", Gi)
        d_p = np.einsum("jaa->ja", aGi @ pert @ aGi) + f * U * p
        ref["pdiag"][F] = p.T
        bound["pdiag"][F] = d_p.T
        q = (u * e).sum(axis=1)                                                 # (nt, R)
        d_q = (np.abs(u) * d_e).sum(axis=1) + f * U * np.abs(u * e).sum(axis=1)
        logp = 2 * np.log(np.einsum("jaa->ja", L))                              # log pivot_i
        ldet = logp.sum(axis=1)                                                 # (nt,)
        d_ld = (aGi * pert).sum(axis=(1, 2)) + 2 * f * U + (f + 1) * U * np.abs(logp).sum(axis=1)
        e2 = e * e
        d_e2 = 2 * np.abs(e) * d_e + U * e2
        S_ld, dS_ld = ldet.sum(), d_ld.sum() + (nt - 1) * U * np.abs(ldet).sum()
        S_q, dS_q = q.sum(axis=0), d_q.sum(axis=0) + (nt - 1) * U * np.abs(q).sum(axis=0)
        ref["sse"][F] = e2.sum(axis=0)
        bound["sse"][F] = d_e2.sum(axis=0) + (nt - 1) * U * e2.sum(axis=0)
        half = 0.5 * S_ld - 0.5 * S_q
        ref["lpd"][n] = half - f * nt * HALF_LOG_2PI_LD
        bound["lpd"][n] = 0.5 * dS_ld + 0.5 * dS_q + U * np.abs(half) + 2 * U * f * nt * HALF_LOG_2PI_LD + U * np.abs(ref["lpd"][n])
    return ref, bound
