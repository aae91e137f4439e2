"""Dense NumPy statement of the phase-difference torus graph estimator (score matching), in extended precision.

Written from the per-trial Jacobian D (m x d) and sufficient statistics S (m) alone -- no node blocks, no sparsity -- so that an
indexing or sign error in the device's node-block gather cannot cancel against the same error here:

    pairs p = (i, j), i < j, in the order of np.triu_indices(d, 1); c_p = cos(x_i - x_j), s_p = sin(x_i - x_j)
    S[2p] = c_p, S[2p+1] = s_p;  D[2p][i] = -s_p, D[2p][j] = s_p, D[2p+1][i] = c_p, D[2p+1][j] = -c_p
    Gamma = 1/W sum_n w_n D_n D_n^T,  H = 2/W sum_n w_n S_n,  phi = Gamma^-1 H
    r_n = D_n (D_n^T phi) - 2 S_n,  V = 1/W sum_n w_n r_n r_n^T,  Sigma = Gamma^-1 V Gamma^-1 / W
    chi2[p] = phi_p^T (Sigma_pp)^-1 phi_p,  pval = exp(-chi2 / 2),  cond_coupling = I1(k) / I0(k), k = |phi_p|

The inputs are the unit phasors as float64 arrays (what the device is given); everything after that runs in `dtype` (np.longdouble by
default, np.float64 as a switch for the larger shapes).  No linear algebra of NumPy's is used in extended precision (it has none):
the Cholesky factorisation and the substitutions are written out."""
import numpy as np

LD = np.longdouble


def pairs(d):
    i, j = np.triu_indices(d, 1)
    return np.stack([i, j], axis=1)


def phasors(x):
    x = np.asarray(x, dtype=np.float64)
    return np.cos(x), np.sin(x)


def trial_terms(u_re, u_im, dtype=LD):
    """S (N, m) and D (N, m, d) of every trial."""
    re, im = np.asarray(u_re, dtype=dtype), np.asarray(u_im, dtype=dtype)
    d, N = re.shape
    i, j = np.triu_indices(d, 1)
    P = i.size
    c = (re[i] * re[j] + im[i] * im[j]).T                     # (N, P)
    s = (im[i] * re[j] - re[i] * im[j]).T
    S = np.zeros((N, 2 * P), dtype=dtype)
    S[:, 0::2], S[:, 1::2] = c, s
    D = np.zeros((N, 2 * P, d), dtype=dtype)
    p = np.arange(P)
    D[:, 2 * p, i] = -s
    D[:, 2 * p, j] = s
    D[:, 2 * p + 1, i] = c
    D[:, 2 * p + 1, j] = -c
    return S, D


def cholesky(A):
    """Lower factor of a symmetric positive definite matrix in the precision of A (right-looking, written out)."""
    A = np.array(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for k in range(n):
        piv = A[k, k]
        if not piv > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % k)
        L[k, k] = np.sqrt(piv)
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return L


def solve_lower(L, B):
    """L X = B by forward substitution in the precision of L."""
    X = np.array(B, dtype=L.dtype)
    for k in range(L.shape[0]):
        X[k] = (X[k] - L[k, :k] @ X[:k]) / L[k, k]
    return X


def solve_lower_trans(L, B):
    """L^T X = B by back substitution in the precision of L."""
    X = np.array(B, dtype=L.dtype)
    for k in range(L.shape[0] - 1, -1, -1):
        X[k] = (X[k] - L[k + 1:, k] @ X[k + 1:]) / L[k, k]
    return X


def solve_spd(A, B):
    if A.dtype == np.float64:
        return np.linalg.solve(A, B)
    L = cholesky(A)
    return solve_lower_trans(L, solve_lower(L, B))


def fit(u_re, u_im, weights=None, dtype=LD, inference=True):
    """One replicate.  Dict: Gamma (m, m), H (m), phi (P, 2), and with inference chi2 (P), pvals (P), Sigma (m, m); cond2: the
    2-norm condition number of Gamma (float64)."""
    S, D = trial_terms(u_re, u_im, dtype)
    N, m, d = D.shape
    w = np.ones(N, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    W = w.sum()
    A = D.transpose(0, 2, 1).reshape(N * d, m)                # rows (n, a): column a of D_n
    Aw = (D * w[:, None, None]).transpose(0, 2, 1).reshape(N * d, m)
    Gamma = (Aw.T @ A) / W
    H = 2 * (w @ S) / W
    out = {"Gamma": Gamma, "H": H, "cond2": float(np.linalg.cond(Gamma.astype(np.float64)))}
    phi = solve_spd(Gamma, H)
    out["phi"] = phi.reshape(-1, 2)
    if inference:
        g = np.einsum("nad,a->nd", D, phi)
        r = np.einsum("nad,nd->na", D, g) - 2 * S
        V = ((r * w[:, None]).T @ r) / W
        Y = solve_spd(Gamma, V)
        Sigma = solve_spd(Gamma, Y.T).T / W
        chi2 = np.empty(m // 2, dtype=dtype)
        for p in range(m // 2):
            blk = Sigma[2 * p:2 * p + 2, 2 * p:2 * p + 2]
            f = phi[2 * p:2 * p + 2]
            det = blk[0, 0] * blk[1, 1] - blk[0, 1] * blk[1, 0]
            chi2[p] = (f[0] * f[0] * blk[1, 1] - f[0] * f[1] * (blk[0, 1] + blk[1, 0]) + f[1] * f[1] * blk[0, 0]) / det
        out.update(Sigma=Sigma, chi2=chi2, pvals=np.exp(-chi2 / 2))
    return out


def cond_coupling(phi):
    """I1(k) / I0(k), k = |phi_p|: the partial phase-locking value of a pair given all other nodes."""
    import scipy.special
    k = np.hypot(np.asarray(phi, dtype=np.float64)[..., 0], np.asarray(phi, dtype=np.float64)[..., 1])
    return scipy.special.i1e(k) / scipy.special.i0e(k)
