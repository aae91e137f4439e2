"""Extended-precision reference and yardsticks for the analytic gradient's contraction kernels (grad.hip: temporal_grad_kernel,
frob_inner_kernel, kgl_grad_kernel, frob_pair_kernel, fwdR_grad_kernel, d_rowsums / d_colsums_kernel, batch_reduce_kernel,
siglist_eigvec_term_kernel, rowgroup_sumsq_kernel, per_trial_quad_kernel).  No GPU, no library of the project: numpy.longdouble
(the 80-bit x87 format, eps 1.1e-19 -- 11 more bits than float64) beside plain float64 numpy.

Every float64 operand is taken as exact; differences, squares, exp, sqrt, divisions and sums are formed in long double, from the
formulas in the comments of grad.hip.  Each reference returns (value, den): the value and the sum of the magnitudes of its terms.

The measure of a result is |got - ref| / max(den, 2^-960), inf for non-finite output: the error relative to what was added, which
stays meaningful where the terms cancel.  The floor: long double has a wider exponent range than float64, so a term that
correctly underflows to 0 in float64 (exp(-5290): a one-hot Gt at distance 72 under an SE length scale of 0.7) is non-zero in
the reference; without the floor the measure would read 1.

Yardsticks (*_f64): the same formulas written plainly in float64 numpy and summed with np.sum -- what an unhurried float64
implementation loses on the same operands, the input-dependent part included (exp(x) loses about |x| u to the rounding of its
argument; sqrt(q) - q / sqrt(q + 1) cancels at large q).  A yardstick is never a kernel.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53          # unit roundoff of float64
FLOOR = 2.0 ** -960     # floor of a measure's denominator
KIND_SE, KIND_MATERN = 0, 1

if np.finfo(LD).eps > 2.0 ** -60:          # (a platform whose long double is float64 would make every measure blind below 1 u)
    raise ImportError("grad_ref needs a long double wider than float64 (eps %g here)" % np.finfo(LD).eps)


def measure(got, ref, den):
    """max over the components of |got - ref| / max(den, 2^-960); inf if got is not finite."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    ref, den = np.atleast_1d(np.asarray(ref, dtype=LD)), np.atleast_1d(np.asarray(den, dtype=LD))
    if got.shape != ref.shape:
        raise ValueError("measure: shapes %s and %s" % (got.shape, ref.shape))
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got.astype(LD) - ref) / np.maximum(den, LD(FLOOR))))


def _both(terms, axis=None):
    return np.sum(terms, axis=axis), np.sum(np.abs(terms), axis=axis)


# ------------------------------------------------------------------------------------------------ temporal contraction
def _temporal_terms(Gt, t, kinds, ell, sigma2, ft):
    """terms[2c] = Gt sigma2_c dk_c / d ell_c, terms[2c + 1] = Gt k_c (each nt x nt), in the float type ft."""
    G = np.asarray(Gt, dtype=np.float64).astype(ft)
    tt = np.asarray(t, dtype=np.float64).reshape(-1).astype(ft)
    d = tt[:, None] - tt[None, :]
    out = []
    for kind, l, s2 in zip(kinds, ell, sigma2):
        l, s2 = ft(l), ft(s2)
        if kind == KIND_SE:
            k = np.exp(ft(-0.5) * (d * d) / (l * l))
            dk = k * (d * d) / (l * l * l)
        elif kind == KIND_MATERN:
            ad = np.abs(d)
            k = np.exp(-ad / l)
            dk = k * ad / (l * l)
        else:
            raise ValueError("kind %r" % (kind,))
        out += [G * s2 * dk, G * k]
    return out


def temporal_grad_ld(Gt, t, kinds, ell, sigma2):
    """out[2c] = <Gt, sigma2_c dk_c/d ell_c>, out[2c + 1] = <Gt, k_c>: (value (2C), den (2C))."""
    vd = [_both(x) for x in _temporal_terms(Gt, t, kinds, ell, sigma2, LD)]
    return np.array([v for v, _ in vd], dtype=LD), np.array([d for _, d in vd], dtype=LD)


def temporal_grad_f64(Gt, t, kinds, ell, sigma2):
    with np.errstate(under="ignore"):
        return np.array([np.sum(x) for x in _temporal_terms(Gt, t, kinds, ell, sigma2, np.float64)])


# ------------------------------------------------------------------------------------------------ plain inner products
def frob_inner_ld(Gt, dK):
    """out[k] = <Gt, dK_k>; Gt (n2), dK (nm, n2)."""
    G = np.asarray(Gt, dtype=np.float64).reshape(-1).astype(LD)
    D = np.asarray(dK, dtype=np.float64).reshape(-1, G.size).astype(LD)
    return _both(G[None, :] * D, axis=1)


def frob_inner_f64(Gt, dK):
    G = np.asarray(Gt, dtype=np.float64).reshape(-1)
    D = np.asarray(dK, dtype=np.float64).reshape(-1, G.size)
    return np.array([np.sum(G * D[k]) for k in range(D.shape[0])])


def frob_pair_ld(P, T1, T2):
    """out = (<P, T1>, <P, T2>)."""
    return frob_inner_ld(P, np.stack([np.asarray(T1).reshape(-1), np.asarray(T2).reshape(-1)]))


def frob_pair_f64(P, T1, T2):
    return frob_inner_f64(P, np.stack([np.asarray(T1).reshape(-1), np.asarray(T2).reshape(-1)]))


# ------------------------------------------------------------------------------------------------ spatial length scales
def se_gram_ld(gx1, ell1, gx2=None, ell2=None):
    """The SE Gram matrix on the quadrature nodes in long double, rounded to float64 (1D: gx1; 2D: the tensor grid g = g1 ngl2 + g2)."""
    a = np.asarray(gx1, dtype=np.float64).astype(LD)
    if gx2 is None:
        d = a[:, None] - a[None, :]
        return np.exp(LD(-0.5) * d * d / (LD(ell1) * LD(ell1))).astype(np.float64)
    b = np.asarray(gx2, dtype=np.float64).astype(LD)
    p1 = np.repeat(a, b.size), np.tile(b, a.size)
    d1, d2 = p1[0][:, None] - p1[0][None, :], p1[1][:, None] - p1[1][None, :]
    return np.exp(LD(-0.5) * (d1 * d1 / (LD(ell1) * LD(ell1)) + d2 * d2 / (LD(ell2) * LD(ell2)))).astype(np.float64)


def _kgl_terms(M, Kgl, gx1, ell1, gx2, ell2, ft):
    a = np.asarray(gx1, dtype=np.float64).reshape(-1).astype(ft)
    if gx2 is None:
        p1, G = a, a.size
    else:
        b = np.asarray(gx2, dtype=np.float64).reshape(-1).astype(ft)
        p1, p2, G = np.repeat(a, b.size), np.tile(b, a.size), a.size * b.size      # node g: (g / ngl2, g % ngl2)
    mk = np.asarray(M, dtype=np.float64).reshape(G, G).astype(ft) * np.asarray(Kgl, dtype=np.float64).reshape(G, G).astype(ft)
    d1 = p1[:, None] - p1[None, :]
    l1 = ft(ell1)
    out = [mk * (d1 * d1) / (l1 * l1 * l1)]
    if gx2 is not None:
        d2 = p2[:, None] - p2[None, :]
        l2 = ft(ell2)
        out.append(mk * (d2 * d2) / (l2 * l2 * l2))
    return out


def kgl_grad_ld(M, Kgl, gx1, ell1, gx2=None, ell2=None):
    """out[q] = sum_gh M_gh Kgl_gh d_q,gh^2 / ell_q^3, q = 0 (1D) or 0, 1 (2D tensor grid)."""
    vd = [_both(x) for x in _kgl_terms(M, Kgl, gx1, ell1, gx2, ell2, LD)]
    return np.array([v for v, _ in vd], dtype=LD), np.array([d for _, d in vd], dtype=LD)


def kgl_grad_f64(M, Kgl, gx1, ell1, gx2=None, ell2=None):
    return np.array([np.sum(x) for x in _kgl_terms(M, Kgl, gx1, ell1, gx2, ell2, np.float64)])


# ------------------------------------------------------------------------------------------------ forward-model radius
def _fwdR_terms(S, x, gx1, gw1, R, gx2, gw2, eps, ft):
    a, wa = np.asarray(gx1, dtype=np.float64).reshape(-1).astype(ft), np.asarray(gw1, dtype=np.float64).reshape(-1).astype(ft)
    R = ft(R)
    if gx2 is None:
        xx = np.asarray(x, dtype=np.float64).reshape(-1).astype(ft)
        r = a[None, :] - xx[:, None]
        q = (r / R) * (r / R)
        dA = wa[None, :] * (np.sqrt(q) - q / np.sqrt(q + ft(1))) / R
    else:
        b, wb = np.asarray(gx2, dtype=np.float64).reshape(-1).astype(ft), np.asarray(gw2, dtype=np.float64).reshape(-1).astype(ft)
        xx = np.asarray(x, dtype=np.float64).reshape(-1, 2).astype(ft)
        p1, p2, w = np.repeat(a, b.size), np.tile(b, a.size), np.repeat(wa, b.size) * np.tile(wb, a.size)
        d1, d2 = p1[None, :] - xx[:, 0][:, None], p2[None, :] - xx[:, 1][:, None]
        re = R + ft(eps)
        dA = w[None, :] / np.sqrt(re * re + (d1 * d1 + d2 * d2))
    return ft(2) * np.asarray(S, dtype=np.float64).reshape(dA.shape).astype(ft) * dA


def fwdR_grad_ld(S, x, gx1, gw1, R, gx2=None, gw2=None, eps=0.0):
    """2 sum_xg S_xg dA_xg/dR;  1D dA/dR = w_g (sqrt(q) - q / sqrt(q + 1)) / R, q = (r / R)^2;  2D dA/dR = w_g / sqrt((R + eps)^2 + w^2)."""
    return _both(_fwdR_terms(S, x, gx1, gw1, R, gx2, gw2, eps, LD))


def fwdR_grad_f64(S, x, gx1, gw1, R, gx2=None, gw2=None, eps=0.0):
    return np.sum(_fwdR_terms(S, x, gx1, gw1, R, gx2, gw2, eps, np.float64))


# ------------------------------------------------------------------------------------------------ sums over D
def _D_terms(D, es, et, ft):
    es, et = np.asarray(es, dtype=np.float64).reshape(-1).astype(ft), np.asarray(et, dtype=np.float64).reshape(-1).astype(ft)
    inv = ft(1) / np.asarray(D, dtype=np.float64).reshape(es.size, et.size).astype(ft)
    return et[None, :] * inv, es[:, None] * inv, inv


def D_sums_ld(D, es, et):
    """a_x = sum_i et_i / D_xi, b_i = sum_x es_x / D_xi, s1 = sum 1/D, s1row_x = sum_i 1/D_xi: four (value, den) pairs."""
    ta, tb, inv = _D_terms(D, es, et, LD)
    return _both(ta, axis=1), _both(tb, axis=0), _both(inv), _both(inv, axis=1)


def D_sums_f64(D, es, et):
    ta, tb, inv = _D_terms(D, es, et, np.float64)
    return np.sum(ta, axis=1), np.sum(tb, axis=0), np.sum(inv), np.sum(inv, axis=1)


# ------------------------------------------------------------------------------------------------ sum of symmetric products
def _batch_terms(terms, n, ft):
    """terms (nb, n, n), of which only the lower triangles count: (nb, n, n) with the lower triangle mirrored."""
    T = np.asarray(terms, dtype=np.float64).reshape(-1, n, n)
    low = np.tril(np.ones((n, n), dtype=bool))
    L = np.where(low[None], T, 0.0)
    return (L + np.transpose(np.where(low[None] & ~np.eye(n, dtype=bool)[None], T, 0.0), (0, 2, 1))).astype(ft)


def batch_reduce_ld(terms, n, scale, dvec, dscale):
    """out = scale sum_b sym(terms_b) + dscale diag(dvec), sym: the lower triangle on both sides."""
    S = _batch_terms(terms, n, LD)
    dv = LD(dscale) * np.asarray(dvec, dtype=np.float64).reshape(n).astype(LD)
    val = LD(scale) * np.sum(S, axis=0) + np.diag(dv)
    den = abs(LD(scale)) * np.sum(np.abs(S), axis=0) + np.diag(np.abs(dv))
    return val, den


def batch_reduce_f64(terms, n, scale, dvec, dscale):
    S = _batch_terms(terms, n, np.float64)
    return scale * np.sum(S, axis=0) + np.diag(dscale * np.asarray(dvec, dtype=np.float64).reshape(n))


# ------------------------------------------------------------------------------------------------ eigenvector-rotation term
def _siglist(Ghs, Ssum, es, sig, tiny, ft):
    es, sig = np.asarray(es, dtype=np.float64).reshape(-1), np.asarray(sig, dtype=np.float64).reshape(-1)
    nx = es.size
    G = np.asarray(Ghs, dtype=np.float64).reshape(nx, nx).astype(ft)
    S = np.asarray(Ssum, dtype=np.float64).reshape(nx, nx).astype(ft)
    de64 = es[None, :] - es[:, None]                                   # [y, x] = es_x - es_y: the kernel's own test, in float64
    touched = (np.abs(de64) > tiny) & ~np.eye(nx, dtype=bool)
    de = es.astype(ft)[None, :] - es.astype(ft)[:, None]
    ds = sig.astype(ft)[:, None] - sig.astype(ft)[None, :]             # [y, x] = sig_y - sig_x
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(touched, ft(-0.5) * ds / np.where(touched, de, ft(1)) * S.T, ft(0))
    return G, term, touched


def siglist_eigvec_term_ld(Ghs, Ssum, es, sig, tiny):
    """Ghs[y][x] + (-1/2 (sig_y - sig_x) / (es_x - es_y) Ssum[x][y]) for x != y, |es_x - es_y| > tiny: (value, den, touched), den =
    |Ghs| + |term| elementwise."""
    G, term, touched = _siglist(Ghs, Ssum, es, sig, tiny, LD)
    return G + term, np.abs(G) + np.abs(term), touched


def siglist_eigvec_term_f64(Ghs, Ssum, es, sig, tiny):
    G, term, _ = _siglist(Ghs, Ssum, es, sig, tiny, np.float64)
    return G + term


# ------------------------------------------------------------------------------------------------ per-row / per-trial sums
def rowgroup_sumsq_ld(Bm, nrows):
    b = np.asarray(Bm, dtype=np.float64).reshape(nrows, -1).astype(LD)
    v = np.sum(b * b, axis=1)
    return v, v


def rowgroup_sumsq_f64(Bm, nrows):
    b = np.asarray(Bm, dtype=np.float64).reshape(nrows, -1)
    return np.sum(b * b, axis=1)


def per_trial_quad_ld(alpha, D, nx, nb, nt):
    """out[b] = sum_x sum_i alpha[x, b, i]^2 / D[x, i]."""
    a = np.asarray(alpha, dtype=np.float64).reshape(nx, nb, nt).astype(LD)
    d = np.asarray(D, dtype=np.float64).reshape(nx, 1, nt).astype(LD)
    return _both(a * a / d, axis=(0, 2))


def per_trial_quad_f64(alpha, D, nx, nb, nt):
    a = np.asarray(alpha, dtype=np.float64).reshape(nx, nb, nt)
    return np.sum(a * a / np.asarray(D, dtype=np.float64).reshape(nx, 1, nt), axis=(0, 2))


# ------------------------------------------------------------------------------------------------ operand families
def weights(fam, shape, seed=0, hot=None):
    """The weight operand of family `fam`: float64, C-contiguous, read-only.
      normal  standard normal (not symmetric)
      spike   1e-3 x standard normal with 1.0 at the last element and at the last row's first element
      onehot  zeros with a single 1.0 at the flat index `hot` (default: the last element)"""
    shape = tuple(int(s) for s in np.atleast_1d(shape))
    n = int(np.prod(shape))
    rs = np.random.RandomState((1000003 * seed + 7919 * n + 31 * len(shape) + 17) % 2 ** 32)
    if fam == "normal":
        W = rs.standard_normal(shape)
    elif fam == "spike":
        W = 1e-3 * rs.standard_normal(shape)
        W.reshape(-1)[-1] = 1.0
        W.reshape(-1)[n - shape[-1]] = 1.0
    elif fam == "onehot":
        W = np.zeros(shape)
        W.reshape(-1)[n - 1 if hot is None else int(hot)] = 1.0
    else:
        raise ValueError("family %r" % (fam,))
    W = np.ascontiguousarray(W, dtype=np.float64)
    W.setflags(write=False)
    return W


def gauss_legendre(n, a, b):
    """Gauss-Legendre nodes and weights on [a, b] (float64: operands like any other)."""
    x, w = np.polynomial.legendre.leggauss(int(n))
    return 0.5 * (b - a) * x + 0.5 * (b + a), 0.5 * (b - a) * w
