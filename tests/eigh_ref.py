"""Extended-precision reference and yardsticks for the symmetric eigensolver (eigh.hip, eigh_dc.hip, sytrd_regtail.hpp, stedc.hip,
wy.hip, wy_prep.hpp, jacobi.hpp).  No GPU, no library of the project: numpy.longdouble (the 80-bit x87 format, eps 1.1e-19 -- 11
more bits than float64) beside LAPACK in float64.

Every float64 operand is taken as exact; products, differences and sums are formed in long double.

Measures
  residual(A, w, V)            max |A V - V diag(w)| / ||A||_inf            (tridiag_residual: the same for T = tridiag(d, e))
  orthogonality(V)             max |V^T V - I|
  eigenvalue_error(w, w_ld)    max |w - w_ld| / max |w_ld|
  tridiagonalisation(A, d, e, V, tau)
                               max |Q^T A Q - T| / ||A||_inf, max |Q^T Q - I| with Q = H_0 H_1 .. accumulated in long double from
                               the reflectors H_k = I - tau_k v_k v_k^T (v_k = row k of V), and the eigenvalue error of T against
                               w_ld of A: the tridiagonal carries A's spectrum
Every measure is inf for non-finite output.

w_ld: the eigenvalues in long double -- Householder tridiagonalisation in long double for a dense matrix (eigvals_ld), then
Sturm bisection in long double on the tridiagonal (eigvals_tridiag_ld), vectorised over the n eigenvalues with a sequential loop
over the rows.  The brackets start at LAPACK's float64 eigenvalues +- 2^-46 ||T||_inf (LAPACK's own error is ~2^-50) and are CHECKED
with Sturm counts (an eigenvalue whose bracket does not hold starts from the Gershgorin interval instead), so 15 halvings reach the
width 2^-60 ||T||_inf that 62 halvings from the Gershgorin interval reach.  Error: 2^-61 ||T||_inf, 0.004 u.

Yardsticks: the same measures of numpy.linalg.eigh (LAPACK dsyevd, float64) on the same operand, and for the tridiagonalisation
stage a plain float64 Householder loop in this file (householder_f64).  A yardstick is never a kernel.
"""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53          # unit roundoff of float64

if np.finfo(LD).eps > 2.0 ** -60:          # (a platform whose long double is float64 would make every measure blind below 1 u)
    raise ImportError("eigh_ref needs a long double wider than float64 (eps %g here)" % np.finfo(LD).eps)

INF = float("inf")


def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


def _finite(*arrays):
    return all(np.all(np.isfinite(np.asarray(a))) for a in arrays)


# ------------------------------------------------------------------------------------------------ long-double arithmetic
def tridiagonalise_ld(A):
    """Householder tridiagonalisation of the symmetric float64 matrix A in long double: (d, e) with Q^T A Q = tridiag(d, e)."""
    W = _ld(A).copy()
    n = W.shape[0]
    d, e = np.zeros(n, dtype=LD), np.zeros(max(n - 1, 0), dtype=LD)
    for k in range(n - 2):
        x = W[k + 1:, k].copy()
        alpha = x[0]
        s = np.sqrt(x @ x)
        d[k] = W[k, k]
        if not s > 0 or not (x[1:] @ x[1:]) > 0:          # nothing below the sub-diagonal: H = I
            e[k] = alpha
            continue
        beta = -s if alpha >= 0 else s
        x[0] = alpha - beta                                # v, un-normalised; H = I - 2 v v^T / (v^T v)
        x /= np.sqrt(x @ x)
        S = W[k + 1:, k + 1:]
        p = 2 * (S @ x)
        w = p - (x @ p) * x
        S -= np.stack([x, w], axis=1) @ np.stack([w, x], axis=0)      # the rank-2 update in one pass
        e[k] = beta
    if n >= 2:
        d[n - 2], e[n - 2] = W[n - 2, n - 2], W[n - 1, n - 2]
    if n >= 1:
        d[n - 1] = W[n - 1, n - 1]
    return d, e


def _sturm_counts(d, e2, x):
    """The number of eigenvalues of tridiag(d, sqrt(e2)) below each entry of x (long double; one pass over the rows).  A zero
    pivot is left to IEEE arithmetic: e2 / 0 = inf makes the NEXT pivot -inf, which is counted in its place, and the one after
    d - x again; a row with e2 = 0 starts afresh (no 0 / 0)."""
    q = d[0] - x
    cnt = (q < 0).astype(np.int64)
    t, neg = np.empty_like(q), np.empty(q.shape, dtype=bool)
    with np.errstate(divide="ignore"):
        for i in range(1, d.shape[0]):
            if e2[i - 1] == 0:
                np.subtract(d[i], x, out=q)
            else:
                np.divide(e2[i - 1], q, out=t)
                np.subtract(d[i] - t, x, out=q)
            np.less(q, 0, out=neg)
            cnt += neg
    return cnt


def eigvals_tridiag_ld(d, e, halvings=None):
    """The eigenvalues of tridiag(d, e), ascending, by Sturm bisection in long double; d, e float64 (exact) or long double."""
    d, e = np.asarray(d).astype(LD), np.asarray(e).astype(LD)
    n = d.shape[0]
    if n == 0 or not _finite(d, e):
        return np.full(n, np.nan, dtype=LD)
    if n == 1:
        return d.copy()
    e2 = e * e
    ae = np.abs(e)
    rad = np.concatenate([ae, [LD(0)]]) + np.concatenate([[LD(0)], ae])
    nrm = np.max(np.abs(d) + rad)
    if nrm == 0:
        return np.zeros(n, dtype=LD)
    gl, gu = np.min(d - rad), np.max(d + rad)
    gl, gu = gl - 2 * np.finfo(LD).eps * nrm, gu + 2 * np.finfo(LD).eps * nrm
    k = np.arange(n)
    lo, hi = np.full(n, gl, dtype=LD), np.full(n, gu, dtype=LD)
    if halvings is None:
        ok = np.zeros(n, dtype=bool)
        # LAPACK's float64 eigenvalues of the rounded tridiagonal (scaled into float64's range), as brackets that are verified
        from scipy.linalg import eigvalsh_tridiagonal
        sc = LD(2.0) ** -int(np.floor(np.log2(nrm)))
        try:
            w0 = eigvalsh_tridiagonal((d * sc).astype(np.float64), (e * sc).astype(np.float64)).astype(LD) / sc
        except Exception:                                  # (LAPACK gave up: Gershgorin brackets and the full count of halvings)
            w0 = None
        if w0 is not None and _finite(w0):
            delta = nrm * LD(2.0) ** -46
            a, b = np.maximum(w0 - delta, gl), np.minimum(w0 + delta, gu)
            ok = (_sturm_counts(d, e2, a) <= k) & (_sturm_counts(d, e2, b) >= k + 1)
            lo, hi = np.where(ok, a, lo), np.where(ok, b, hi)
        halvings = 15 if np.all(ok) else 62
    for _ in range(halvings):
        mid = lo + (hi - lo) / 2
        below = _sturm_counts(d, e2, mid) >= k + 1          # eigenvalue k lies below mid
        hi = np.where(below, mid, hi)
        lo = np.where(below, lo, mid)
    return lo + (hi - lo) / 2


def eigvals_ld(A):
    """The eigenvalues of the symmetric float64 matrix A, ascending, in long double."""
    A = np.asarray(A, dtype=np.float64)
    if not _finite(A):
        return np.full(A.shape[0], np.nan, dtype=LD)
    return eigvals_tridiag_ld(*tridiagonalise_ld(A))


def _gram_minus_identity(V, bs=128):
    """max |V^T V - I| in long double, from the block rows on and right of the diagonal blocks (the rest by symmetry)."""
    Vl = V if V.dtype == LD else _ld(V)
    n = Vl.shape[1]
    worst = LD(0)
    for j0 in range(0, n, bs):
        j1 = min(n, j0 + bs)
        G = np.ascontiguousarray(Vl[:, j0:j1].T) @ Vl[:, j0:]
        G[np.arange(j1 - j0), np.arange(j1 - j0)] -= 1
        worst = max(worst, np.max(np.abs(G)))
    return float(worst)


def house_Q_ld(V, tau):
    """Q = H_0 H_1 .. H_{n-3} in long double, H_k = I - tau_k v_k v_k^T, v_k = V[k] (zero up to and including column k).  Accumulated
    from the last reflector to the first: H_k then meets the identity outside the trailing block."""
    Vl, tl = _ld(V), _ld(tau)
    n = Vl.shape[0]
    Q = np.eye(n, dtype=LD)
    for k in range(n - 3, -1, -1):
        v = Vl[k, k + 1:]
        Qs = Q[k + 1:, k + 1:]
        Qs -= np.multiply.outer(tl[k] * v, v @ Qs)                   # H_k Q
    return Q


# ------------------------------------------------------------------------------------------------ measures
def norm_inf(A):
    return np.max(np.sum(np.abs(_ld(A)), axis=1))


def residual(A, w, V, cols=None):
    """max |A V - V diag(w)| / ||A||_inf; inf for non-finite w or V.  cols: only these columns of V (and entries of w)."""
    if not _finite(w, V):
        return INF
    Vl, wl = _ld(V), _ld(w)
    if cols is not None:
        Vl, wl = np.ascontiguousarray(Vl[:, cols]), wl[cols]
    nrm = norm_inf(A)
    R = np.max(np.abs(_ld(A) @ Vl - Vl * wl[None, :]))
    return float(R / nrm) if nrm > 0 else float(R)


def tridiag_norm_inf(d, e):
    ae = np.abs(_ld(e))
    return np.max(np.abs(_ld(d)) + np.concatenate([ae, [LD(0)]]) + np.concatenate([[LD(0)], ae]))


def tridiag_residual(d, e, w, Z):
    """residual() for A = tridiag(d, e) without forming A."""
    if not _finite(w, Z):
        return INF
    dl, el, Zl = _ld(d), _ld(e), _ld(Z)
    R = dl[:, None] * Zl - Zl * _ld(w)[None, :]
    R[:-1] += el[:, None] * Zl[1:]
    R[1:] += el[:, None] * Zl[:-1]
    nrm = tridiag_norm_inf(d, e)
    R = np.max(np.abs(R))
    return float(R / nrm) if nrm > 0 else float(R)


def orthogonality(V, cols=None):
    """max |V^T V - I|; inf for non-finite V.  cols: only the rows `cols` of V^T V - I (these columns against every column)."""
    if not _finite(V):
        return INF
    if cols is None:
        return _gram_minus_identity(V)
    Vl = _ld(V)
    cols = np.asarray(cols)
    G = np.ascontiguousarray(Vl[:, cols].T) @ Vl
    G[np.arange(cols.size), cols] -= 1
    return float(np.max(np.abs(G)))


def eigenvalue_error(w, w_ld):
    """max |w - w_ld| / max |w_ld| (absolute for a zero spectrum); inf for non-finite w."""
    if not _finite(w):
        return INF
    w_ld = np.asarray(w_ld)
    err, top = np.max(np.abs(_ld(w) - w_ld)), np.max(np.abs(w_ld))
    return float(err / top) if top > 0 else float(err)


def tridiagonalisation(A, d, e, V, tau, w_ld=None):
    """(max |Q^T A Q - T| / ||A||_inf, max |Q^T Q - I|, eigenvalue error of T = tridiag(d, e) against w_ld of A)."""
    if not _finite(d, e, V, tau):
        return INF, INF, INF
    Q = house_Q_ld(V, tau)
    n = Q.shape[0]
    AQ, dl, el = _ld(A) @ Q, _ld(d), _ld(e)
    back, bs = LD(0), 128
    for j0 in range(0, n, bs):                                         # Q^T A Q - T is symmetric: the block rows from their diagonal blocks on
        j1 = min(n, j0 + bs)
        B = np.ascontiguousarray(Q[:, j0:j1].T) @ AQ[:, j0:]
        r = np.arange(j1 - j0)
        B[r, r] -= dl[j0:j1]
        B[r[1:], r[1:] - 1] -= el[j0:j1 - 1]
        m = min(j1, n - 1) - j0
        B[r[:m], r[:m] + 1] -= el[j0:j0 + m]
        back = max(back, np.max(np.abs(B)))
    nrm = norm_inf(A)
    back = float(back / nrm) if nrm > 0 else float(back)
    orth = _gram_minus_identity(Q)
    if w_ld is None:
        w_ld = eigvals_ld(A)
    return back, orth, eigenvalue_error(eigvals_tridiag_ld(d, e).astype(LD), w_ld)


# ------------------------------------------------------------------------------------------------ yardsticks (float64)
def lapack_eigh(A):
    return np.linalg.eigh(np.asarray(A, dtype=np.float64))


def dense_of(d, e):
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def householder_f64(A):
    """A plain float64 Householder tridiagonalisation (unblocked, LAPACK dsytd2's arithmetic) in the layout of debug_sytrd:
    (d, e, V, tau) with V[k] = v_k, v_k[:k + 1] = 0, v_k[k + 1] = 1, H_k = I - tau_k v_k v_k^T."""
    W = np.array(A, dtype=np.float64)
    n = W.shape[0]
    d, e, tau, V = np.zeros(n), np.zeros(max(n - 1, 0)), np.zeros(n), np.zeros((n, n))
    for k in range(n - 2):
        x = W[k + 1:, k].copy()
        d[k] = W[k, k]
        V[k, k + 1] = 1.0
        top = float(np.max(np.abs(x[1:])))
        if top == 0.0:
            e[k] = x[0]
            continue
        m = max(top, abs(x[0]))                            # (dlarfg rescales too: the squares of a column of 1e-160 are subnormal)
        xs = x / m
        alpha, xn2 = xs[0], float(xs[1:] @ xs[1:])
        beta = -np.copysign(np.sqrt(alpha * alpha + xn2), alpha)
        tau[k] = (beta - alpha) / beta
        v = xs / (alpha - beta)
        v[0] = 1.0
        V[k, k + 1:] = v
        beta *= m
        S = W[k + 1:, k + 1:]
        p = tau[k] * (S @ v)
        w = p - (0.5 * tau[k] * (p @ v)) * v
        S -= np.outer(v, w) + np.outer(w, v)
        e[k] = beta
    if n >= 2:
        d[n - 2], e[n - 2] = W[n - 2, n - 2], W[n - 1, n - 2]
    if n >= 1:
        d[n - 1] = W[n - 1, n - 1]
    return d, e, V, tau


def negligible_columns(A, threshold=1e-100):
    """The columns k whose Householder step the kernels skip as rounding noise of rounding noise: a float64 replay of the
    tridiagonalisation of A / max|a| in which a column with 0 < |x|^2 and alpha^2 + |x|^2 <= threshold counts as zero (H = I), as in
    sytrd_step_kernel and rt_house.  (The kernels' arithmetic differs in its roundings, not in these magnitudes.)"""
    W = np.array(A, dtype=np.float64)
    W /= max(np.max(np.abs(W)), 1e-300)
    n = W.shape[0]
    found = []
    for k in range(n - 2):
        x = W[k + 1:, k].copy()
        alpha, xn2 = x[0], float(x[1:] @ x[1:])
        s2 = alpha * alpha + xn2
        if xn2 == 0.0:
            continue
        if s2 <= threshold:
            found.append(k)
            continue
        beta = -np.copysign(np.sqrt(s2), alpha)
        tau = (beta - alpha) / beta
        v = x / (alpha - beta)
        v[0] = 1.0
        S = W[k + 1:, k + 1:]
        p = tau * (S @ v)
        w = p - (0.5 * tau * (p @ v)) * v
        S -= np.outer(v, w) + np.outer(w, v)
    return found


# ------------------------------------------------------------------------------------------------ dense families
def _sym(A):
    """The lower triangle on both sides: symmetric bit for bit whatever the product routine did."""
    return np.tril(A) + np.tril(A, -1).T


def _orth(n, rs):
    return np.linalg.qr(rs.standard_normal((n, n)))[0]


def _from_spectrum(lam, rs):
    Q = _orth(len(lam), rs)
    A = (Q * np.asarray(lam, dtype=np.float64)[None, :]) @ Q.T
    return _sym(0.5 * (A + A.T))


def _random(n, rs):
    M = rs.standard_normal((n, n))
    return _sym(0.5 * (M + M.T))


def _gp_temporal(n, rs):              # the SE + exponential Gram of a uniform time grid (test_eigh_gpcsd_shaped)
    t = 0.4 * np.arange(n, dtype=np.float64)[:, None]
    return 0.5 * np.exp(-0.5 * (t - t.T) ** 2 / 400.0) + 0.7 * np.exp(-np.abs(t - t.T) / 5.0)


def _se_rank_deficient(n, rs):        # a pure SE Gram: eigenvalues fall below u max|lambda| after ~ a quarter of them
    i = np.arange(n, dtype=np.float64)[:, None]
    return np.exp(-0.5 * (i - i.T) ** 2 / (0.15 * n + 1.0) ** 2)


def _graded(n, rs):
    return _from_spectrum(np.logspace(0.0, -14.0, n), rs)


def _clustered(n, rs):                # test_eigh_structured's spectrum: 60 % exact zeros, a plateau, a ramp, six values at 1e6
    nbig = min(6, n // 8)
    nz = (6 * n) // 10
    nplat = (n - nz - nbig) // 3
    nramp = n - nz - nbig - nplat
    return _from_spectrum(np.concatenate([np.zeros(nz), np.ones(nplat), np.linspace(2.0, 5.0, nramp), np.full(nbig, 1e6)]), rs)


def _indefinite_pairs(n, rs):         # +-lambda pairs (and a zero at odd n)
    lam = rs.uniform(0.1, 10.0, n // 2)
    return _from_spectrum(np.concatenate([lam, -lam, np.zeros(n % 2)]), rs)


def _centrosymmetric(n, rs):          # J K J = K on a uniform grid, not Toeplitz: the symmetric and antisymmetric spectra interleave
    t = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    a = 1.0 + 0.5 * np.cos(2.0 * np.pi * t / max(n, 2))
    r = t[:, None] - t[None, :]
    K = (a[:, None] * a[None, :]) * (np.exp(-0.5 * r ** 2 / 9.0) + 0.3 * np.exp(-np.abs(r) / 7.0))
    return _sym(0.5 * (K + K[::-1, ::-1]))


def _diagonal_descending(n, rs):
    return np.diag(np.arange(n, dtype=np.float64)[::-1])


def _scaled(n, rs):                   # D A D, D = diag(2^+-30) with random signs of the exponent: exact, entries over 36 decades
    s = 2.0 ** (30.0 * rs.choice([-1.0, 1.0], n))
    return _random(n, rs) * (s[:, None] * s[None, :])


def _exact_low_rank(n, rs):           # s s^T, s = +-1: rank one, exact in float64, every row the first one up to its sign
    sg = rs.choice([-1.0, 1.0], n)
    return np.multiply.outer(sg, sg)


def _huge(n, rs):
    return _random(n, rs) * 2.0 ** 400


def _tiny(n, rs):
    return _random(n, rs) * 2.0 ** -400


FAMILIES = {"random": _random, "gp_temporal": _gp_temporal, "se_rank_deficient": _se_rank_deficient, "graded": _graded,
            "clustered": _clustered, "indefinite_pairs": _indefinite_pairs, "centrosymmetric": _centrosymmetric,
            "diagonal_descending": _diagonal_descending, "exact_low_rank": _exact_low_rank, "scaled": _scaled, "huge": _huge, "tiny": _tiny}


def _rs(n, seed):
    return np.random.RandomState((1000003 * seed + 7919 * n + 17) % 2 ** 32)


@functools.lru_cache(maxsize=None)
def family(name, n, seed=0):
    """The matrix of family `name` at order n: float64, symmetric bit for bit, C-contiguous, read-only.  (huge and tiny are
    2^+-400 times the `random` matrix of the same order and seed, exactly.)"""
    A = np.ascontiguousarray(FAMILIES[name](n, _rs(n, seed)), dtype=np.float64)
    A.setflags(write=False)
    return A


# ------------------------------------------------------------------------------------------------ tridiagonal families
def _t_random(n, rs):
    return rs.standard_normal(n), rs.standard_normal(n - 1)


def _t_wilkinson(n, rs):              # W_n^+: pairs of eigenvalues that agree to many digits
    return np.abs(np.arange(n, dtype=np.float64) - 0.5 * (n - 1)), np.ones(n - 1)


def _glued(glue):
    def make(n, rs):                  # copies of W_21^+ joined by `glue`: clusters of as many eigenvalues as there are copies
        i = np.arange(n)
        d = np.abs((i % 21) - 10.0)
        e = np.where((i[1:] % 21) == 0, glue, 1.0)
        return d, e
    return make


def _t_toeplitz(n, rs):               # eigenvalues 2 cos(k pi / (n + 1))
    return np.zeros(n), np.ones(n - 1)


def _t_graded(n, rs):
    d = np.logspace(0.0, -14.0, n)
    return d, 0.3 * np.sqrt(d[:-1] * d[1:])


def _t_cluster(n, rs):                # every eigenvalue within ~3e-10 of 1
    return 1.0 + 1e-10 * rs.choice([-1.0, 1.0], n), 1e-10 * rs.uniform(0.1, 1.0, n - 1)


def _t_tiny_couplings(n, rs):         # ones, every 7th coupling 1e-9, the rest exact zeros
    e = np.zeros(n - 1)
    e[::7] = 1e-9
    return np.ones(n), e


def _t_negative_offdiag(n, rs):
    return np.full(n, 3.0), np.full(n - 1, -0.5)


def _t_already_diagonal(n, rs):       # distinct integers in no order, every coupling an exact zero
    return rs.permutation(n).astype(np.float64), np.zeros(n - 1)


def _t_huge(n, rs):
    d, e = _t_random(n, rs)
    return d * 2.0 ** 400, e * 2.0 ** 400


def _t_tiny(n, rs):
    d, e = _t_random(n, rs)
    return d * 2.0 ** -400, e * 2.0 ** -400


TRIDIAG_FAMILIES = {"random": _t_random, "wilkinson": _t_wilkinson, "glued_wilkinson_1e-8": _glued(1e-8),
                    "glued_wilkinson_1e-14": _glued(1e-14), "toeplitz": _t_toeplitz, "graded": _t_graded, "cluster": _t_cluster,
                    "tiny_couplings": _t_tiny_couplings, "negative_offdiag": _t_negative_offdiag,
                    "already_diagonal": _t_already_diagonal, "huge": _t_huge, "tiny": _t_tiny}


def tridiag_family(name, n, seed=0):
    """(d, e) of family `name` at order n: float64, read-only."""
    d, e = TRIDIAG_FAMILIES[name](n, _rs(n, seed))
    d, e = np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(e, dtype=np.float64)
    d.setflags(write=False)
    e.setflags(write=False)
    return d, e
