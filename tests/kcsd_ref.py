"""Dense statement of kernel CSD in one dimension with Gaussian sources (gpcsd_amd/kcsd.py, kcsd.hip) in numpy.longdouble (the
80-bit x87 format, 11 more bits than float64).  No GPU, no library of the project.  Every float64 operand is taken as exact.

  g(u) = exp(-u^2 / (2 sb^2)) / (sqrt(2 pi) sb), sb = R / 3
  b_j(x) = 1 / (2 sigma) int_{-R}^{R} [sqrt((u - d)^2 + h^2) - |u - d|] g(u) du, d = x - s_j, the bracket as h^2 / (sqrt(v^2 + h^2) + v)
  K = B_pot^T B_pot / M, K~ = B_src^T B_pot / M, A = K + lambda I, beta = A^-1 V, estimate K~ beta
  err(R, lambda) = sum_i ||V_i - V^_i^(-i)||_2: by explicit refits without electrode i (long-double Cholesky, chol_ref), and by the
  closed form V_i - V^_i^(-i) = beta_i / (A^-1)_ii

dtype=np.float64 gives the same statements in float64 (the yardstick tools/kcsd_timing.py times).

Rounding bounds (U = 2^-53), what a float64 evaluation in the stated order may lose:
  potential basis   (2 ngl + 24) U sum_q |term_q|: 2 ngl additions in node order, and 24 U for a term's own chain (node, distance to
                    the kink, square root, division, exponent, exponential, three products)
  source basis      (8 + u^2 / sb^2) U |g|: the exponent u^2 / (2 sb^2) enters the value with its own size as the factor
  CV entry          sum_i [ (n + 8) U sqrt(sum_t (sum_k |U_ik d_k W_kt|)^2) / a_ii + (T + n + 8) U err_i ]: an n-term product sum with
                    rounded d_k and U_ik d_k per beta; a_ii (n terms), the division, the square, T additions and the root per electrode
"""
import numpy as np

import chol_ref

LD = np.longdouble
U = 2.0 ** -53

if np.finfo(LD).eps > 2.0 ** -60:
    raise ImportError("kcsd_ref needs a long double wider than float64 (eps %g here)" % np.finfo(LD).eps)


# ------------------------------------------------------------------------------------------------ quadrature
def gauss_legendre(n):
    """float64 nodes and weights on [-1, 1]: what the product hands to the device."""
    return np.polynomial.legendre.leggauss(n)


def gauss_legendre_ld(n):
    """Nodes and weights in long double: numpy's float64 nodes polished by Newton steps on P_n in long double."""
    x = np.polynomial.legendre.leggauss(n)[0].astype(LD)
    for _ in range(3):
        p0, p1 = np.ones_like(x), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / LD(k)
        dp = n * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    p0, p1 = np.ones_like(x), x.copy()
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / LD(k)
    dp = n * (x * p1 - p0) / (x * x - 1)
    return x, 2 / ((1 - x * x) * dp * dp)


def _pi_ld():
    return LD(4) * np.arctan(LD(1))


def _g(u, R, dtype):
    sb = dtype(R) / dtype(3)
    pi = _pi_ld() if dtype is LD else dtype(np.pi)
    return np.exp(-(u * u) / (2 * sb * sb)) / (np.sqrt(2 * pi) * sb)


def potential_basis(src, pts, R, h, sigma, gx, gw, dtype=LD):
    """(values (M, npts), sum of |terms| (M, npts)) of the two-panel rule at the nodes gx / weights gw on [-1, 1]; the terms are
    half-width * weight * bracket * g / (2 sigma), panel [-R, c] first, nodes in order."""
    src, pts = np.asarray(src).astype(dtype), np.asarray(pts).astype(dtype)
    gx, gw = np.asarray(gx).astype(dtype), np.asarray(gw).astype(dtype)
    R, h, sigma = dtype(R), dtype(h), dtype(sigma)
    d = pts[None, :] - src[:, None]
    c = np.clip(d, -R, R)
    val, mag = np.zeros(d.shape, dtype=dtype), np.zeros(d.shape, dtype=dtype)
    for lo, hi in ((-R + 0 * c, c), (c, R + 0 * c)):
        half, mid = (hi - lo) / 2, (hi + lo) / 2
        for q in range(gx.size):
            u = mid + half * gx[q]
            v = np.abs(u - d)
            term = half * gw[q] * (h * h / (np.sqrt(v * v + h * h) + v)) * _g(u, R, dtype) / (2 * sigma)
            val = val + term
            mag = mag + np.abs(term)
    return val, mag


def source_basis(src, pts, R, dtype=LD):
    """g(pts[p] - src[j]) (M, npts)"""
    src, pts = np.asarray(src).astype(dtype), np.asarray(pts).astype(dtype)
    return _g(pts[None, :] - src[:, None], dtype(R), dtype)


def potential_bound(mag, ngl):
    return (2 * ngl + 24) * U * mag


def source_bound(src, pts, R, gval):
    u = np.asarray(pts).astype(LD)[None, :] - np.asarray(src).astype(LD)[:, None]
    sb = LD(R) / 3
    return (8 + u * u / (sb * sb)) * U * np.abs(gval)


# ------------------------------------------------------------------------------------------------ kernels and estimates
def kernels(src, ele, est, R, h, sigma, gx, gw, dtype=LD):
    """K (n, n) and K~ (n_est, n)"""
    Bp = potential_basis(src, ele, R, h, sigma, gx, gw, dtype)[0]
    Bs = source_basis(src, est, R, dtype)
    M = dtype(len(src))
    return Bp.T @ Bp / M, Bs.T @ Bp / M


def solve_spd(A, B):
    """A^-1 B through the long-double Cholesky factor"""
    L = chol_ref.cholesky_ld(A)
    return chol_ref.solve_lower_ld(L, chol_ref.solve_lower_ld(L, B), trans=True)


def _solve(A, B, dtype):
    if dtype is LD:
        return solve_spd(A, B)
    return np.linalg.solve(A, B)


def estimate(K, Kc, V, lam, dtype=LD):
    """(K~ (K + lam I)^-1 V, K (K + lam I)^-1 V)"""
    K, Kc, V = np.asarray(K).astype(dtype), np.asarray(Kc).astype(dtype), np.asarray(V).astype(dtype)
    beta = _solve(K + dtype(lam) * np.eye(K.shape[0], dtype=dtype), V, dtype)
    return Kc @ beta, K @ beta


def cv_refit(K, V, lam, dtype=LD):
    """sum_i ||V_i - K[i, -i] (K[-i, -i] + lam I)^-1 V[-i]||_2: one explicit refit per held-out electrode"""
    K, V = np.asarray(K).astype(dtype), np.asarray(V).astype(dtype)
    n = K.shape[0]
    tot = dtype(0)
    for i in range(n):
        keep = np.arange(n) != i
        A = K[np.ix_(keep, keep)] + dtype(lam) * np.eye(n - 1, dtype=dtype)
        res = V[i] - K[i, keep] @ _solve(A, V[keep], dtype)
        tot = tot + np.sqrt(np.sum(res * res))
    return tot


def cv_closed_dense(K, V, lam, dtype=LD):
    """the closed form from A^-1 itself: sum_i ||beta_i / (A^-1)_ii||_2"""
    K, V = np.asarray(K).astype(dtype), np.asarray(V).astype(dtype)
    n = K.shape[0]
    A = K + dtype(lam) * np.eye(n, dtype=dtype)
    Ainv = _solve(A, np.eye(n, dtype=dtype), dtype)
    beta = Ainv @ V
    e = beta / np.diag(Ainv)[:, None]
    return np.sum(np.sqrt(np.sum(e * e, axis=1)))


def cv_spectral(Umat, s, W, lam):
    """The closed form from an eigen-decomposition, as the device states it, in long double, with its rounding gate:
    (err, gate, singular).  Umat (n, n) eigenvectors in columns, s (n), W = U^T V (n, T)."""
    Umat, s, W = np.asarray(Umat).astype(LD), np.maximum(np.asarray(s).astype(LD), 0), np.asarray(W).astype(LD)
    n, T = W.shape
    lam = LD(lam)
    if not (s.min() + lam > 0) or s.min() + lam < n * LD(2.0 ** -52) * s.max():
        return LD(np.inf), LD(0), True
    d = 1 / (s + lam)
    a = (Umat * Umat) @ d
    beta = (Umat * d[None, :]) @ W
    mag = (np.abs(Umat) * d[None, :]) @ np.abs(W)
    erri = np.sqrt(np.sum((beta / a[:, None]) ** 2, axis=1))
    gate = np.sum((n + 8) * U * np.sqrt(np.sum(mag * mag, axis=1)) / a + (T + n + 8) * U * erri)
    return np.sum(erri), gate, False
