"""Extended-precision reference and yardsticks for the dense Cholesky path (chol.hip: potrf_device, trsm_lower_device,
trsm_lower_trans_device, logdet_chol_device).  No GPU, no library of the project: numpy.longdouble (the 80-bit x87 format, eps
1.1e-19 -- 11 more bits than float64) beside LAPACK in float64.  A 50-digit factorisation would say no more about a float64
kernel and takes minutes at n = 1025.

Every float64 operand is taken as exact; products, differences and denominators are formed in long double.

Measures (all backward errors: they stay meaningful at the condition numbers 1e8 .. 1e10 the library's own matrices have, where
a forward error of L says nothing)
  rho(A, L)          max_ij |A - L L^T|_ij / sqrt(a_ii a_jj) -- invariant under A -> D A D, so one gate serves badly scaled inputs
  omega(L, X, B)     Oettli-Prager componentwise backward error of L X = B (trans: L^T X = B): max over rows and columns of
                     |B - L X| / (|L| |X| + |B|), 0/0 counted as 0
  forward_error      max |X - X_ld| / max |X_ld| against a long-double substitution (reported, not gated)
  logdet_error       |value - 2 sum log L_ii| / sum max(1, |log L_ii^2|): the terms have both signs, so their sum says nothing
                     about the size of what was added (test_tridiag_kernels.py)
Yardsticks: the same measures of numpy.linalg.cholesky / scipy.linalg.solve_triangular (LAPACK, float64) / a plain float64 sum
of logarithms on the same operands -- what an unhurried float64 implementation loses.  A yardstick is never a kernel.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53          # unit roundoff of float64

if np.finfo(LD).eps > 2.0 ** -60:          # (a platform whose long double is float64 would make every measure blind below 1 u)
    raise ImportError("chol_ref needs a long double wider than float64 (eps %g here)" % np.finfo(LD).eps)


# ------------------------------------------------------------------------------------------------ long-double arithmetic
def cholesky_ld(A):
    """Lower Cholesky factor in long double (column by column); raises numpy.linalg.LinAlgError at a non-positive pivot."""
    A = np.asarray(A)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    W = np.tril(A).astype(LD)
    for j in range(n):
        col = W[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % j)
        piv = np.sqrt(col[0])
        L[j, j] = piv
        L[j + 1:, j] = col[1:] / piv
    return L


def solve_lower_ld(L, B, trans=False):
    """L X = B (trans: L^T X = B) by substitution in long double; B (n,) or (n, nrhs)."""
    Ll = np.asarray(L).astype(LD)
    B = np.asarray(B)
    n = Ll.shape[0]
    X = B.astype(LD).reshape(n, -1).copy()
    if not trans:
        for i in range(n):
            X[i] = (X[i] - Ll[i, :i] @ X[:i]) / Ll[i, i]
    else:
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - Ll[i + 1:, i] @ X[i + 1:]) / Ll[i, i]
    return X.reshape(B.shape)


def _residual_lower(A, L, bs=128):
    """The block columns' parts on and below the diagonal blocks of A - L L^T in long double, L lower triangular (entries above
    the diagonal are not read: a caller that cares asserts they are zero); everything else of the result is zero.  By
    symmetry that is the whole residual, at a sixth of the full product's operations."""
    n = A.shape[0]
    Ll = np.tril(np.asarray(L)).astype(LD)
    R = np.zeros((n, n), dtype=LD)
    for j0 in range(0, n, bs):
        j1 = min(n, j0 + bs)
        R[j0:, j0:j1] = A[j0:, j0:j1].astype(LD) - Ll[j0:, :j1] @ Ll[j0:j1, :j1].T
    return R


# ------------------------------------------------------------------------------------------------ measures
def rho(A, L):
    """max_ij |A - L L^T|_ij / sqrt(a_ii a_jj); inf if L is not finite.  A symmetric with a positive diagonal."""
    A = np.asarray(A, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    if not np.all(np.isfinite(L)):
        return float("inf")
    d = np.sqrt(np.diag(A).astype(LD))
    R = np.abs(_residual_lower(A, L)) / (d[:, None] * d[None, :])
    return float(np.max(R))


def omega(L, X, B, trans=False):
    """Componentwise backward error of the triangular solve: max |B - T X| / (|T| |X| + |B|), T = L or L^T; 0/0 counts as 0."""
    T = np.tril(np.asarray(L, dtype=np.float64)).astype(LD)
    if trans:
        T = np.ascontiguousarray(T.T)
    n = T.shape[0]
    Xl = np.asarray(X, dtype=np.float64).astype(LD).reshape(n, -1)
    Bl = np.asarray(B, dtype=np.float64).astype(LD).reshape(n, -1)
    if not np.all(np.isfinite(Xl)):
        return float("inf")
    num = np.abs(Bl - T @ Xl)
    den = np.abs(T) @ np.abs(Xl) + np.abs(Bl)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(num == 0, LD(0), num / den)           # (num > 0 over den == 0 is inf: no perturbation of that size exists)
    return float(np.max(q))


def forward_error(X, X_ref):
    """max |X - X_ref| / max |X_ref|, X_ref in long double."""
    X_ref = np.asarray(X_ref)
    return float(np.max(np.abs(np.asarray(X).astype(LD).reshape(X_ref.shape) - X_ref)) / np.max(np.abs(X_ref)))


def logdet_error(value, L):
    """|value - 2 sum log L_ii| / sum max(1, |log L_ii^2|), the sums in long double."""
    logs = 2.0 * np.log(np.diag(np.asarray(L, dtype=np.float64)).astype(LD))
    return float(np.abs(LD(value) - np.sum(logs)) / np.sum(np.maximum(LD(1), np.abs(logs))))


# ------------------------------------------------------------------------------------------------ yardsticks (LAPACK, float64)
def lapack_factor(A):
    return np.linalg.cholesky(np.asarray(A, dtype=np.float64))


def lapack_solve(L, B, trans=False):
    from scipy.linalg import solve_triangular
    return solve_triangular(np.asarray(L, dtype=np.float64), np.asarray(B, dtype=np.float64), lower=True, trans="T" if trans else "N",
                            check_finite=False)


def logdet_f64(L):
    """2 sum log L_ii, summed in float64 in index order."""
    s = 0.0
    for v in np.log(np.diag(np.asarray(L, dtype=np.float64))):
        s += float(v)
    return 2.0 * s


# ------------------------------------------------------------------------------------------------ matrix families
def _mirror(A):
    """The lower triangle on both sides: symmetric bit for bit whatever the product routine did."""
    return np.tril(A) + np.tril(A, -1).T


def _wishart(n, rs):                  # cond ~ 5
    M = rs.standard_normal((n, n))
    return _mirror(M @ M.T + n * np.eye(n))


def _exp64(n, rs):                    # the bench's matrix; cond 1.5e4 at n = 513
    i = np.arange(n, dtype=np.float64)
    return np.exp(-np.abs(i[:, None] - i[None, :]) / 64.0)


def _se_jitter(n, rs):                # a sample_prior Gram matrix with its jitter; cond 5e9
    i = np.arange(n, dtype=np.float64)
    return np.exp(-0.5 * (i[:, None] - i[None, :]) ** 2 / 400.0) + 1e-8 * np.eye(n)


def _se_matern(n, rs):                # cond 2e2
    i = np.arange(n, dtype=np.float64)
    r = i[:, None] - i[None, :]
    return 0.5 * np.exp(-0.5 * r ** 2 / 25.0) + 0.7 * np.exp(-np.abs(r) / 5.0) + 1e-6 * np.eye(n)


def _scaled(n, rs):                   # well conditioned up to a diagonal scaling over 24 decades; cond 8e23
    M = rs.standard_normal((n, n))
    s = 10.0 ** rs.uniform(-6.0, 6.0, n)
    return _mirror(M @ M.T / n + np.eye(n)) * (s[:, None] * s[None, :])


def _equilibrated(n, rs):             # spectrum over ten decades, unit diagonal: what k_sym_equilibrate hands to potrf; cond 9e9
    Q = np.linalg.qr(rs.standard_normal((n, n)))[0]
    A = (Q * np.logspace(0.0, -10.0, n)[None, :]) @ Q.T
    A = _mirror(0.5 * (A + A.T))
    d = 1.0 / np.sqrt(np.diag(A))
    return A * (d[:, None] * d[None, :])


FAMILIES = {"wishart": _wishart, "exp64": _exp64, "se_jitter": _se_jitter, "se_matern": _se_matern, "scaled": _scaled,
            "equilibrated": _equilibrated}


def family(name, n, seed=0):
    """The matrix of family `name` at order n: float64, C-contiguous, read-only."""
    A = np.ascontiguousarray(FAMILIES[name](n, np.random.RandomState((1000003 * seed + 7919 * n + 17) % 2 ** 32)), dtype=np.float64)
    A.setflags(write=False)
    return A


def families(n, seed=0, names=None):
    """Yields (name, A) for every family (or those in `names`)."""
    for name in (names or FAMILIES):
        yield name, family(name, n, seed)
