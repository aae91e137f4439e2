"""Reference statements for the folded-basis and relayout kernels (TEST INFRASTRUCTURE ONLY; no GPU, no library of the project).

An involution perm of n points (perm[perm[i]] == i) has na pairs and ns = n - na orbits: the pairs in the order of their first
members, then the fixed points.  The fold operator F (n x n, orthogonal) has one row per symmetric orbit -- (e_i + e_j) / sqrt2 for
a pair, e_i for a fixed point -- followed by one row (e_i - e_j) / sqrt2 per pair.  Every reference below is the definition, as a
product with F in numpy.longdouble (the 80-bit x87 format, as grad_ref.py); none of them looks at what kind of orbit an index is in.
Each returns (value, magnitude): the magnitude is the same product with |F| and |operand|, the sum of |weight x input| that the
counted rounding bounds of test_fold_kernels.py multiply."""
import numpy as np

import grad_ref as GR
import matern_ref as MT

LD = GR.LD
U = GR.U
ISQ2 = LD(1) / np.sqrt(LD(2))
FAMILIES = ("mirror_even", "mirror_odd", "identity", "scattered")


# ------------------------------------------------------------------------------------------------ involutions and their tables
def involution(family, n, seed=0):
    """perm (n,) of the family; mirror_even / mirror_odd are the reflection of a grid of n points (n even / odd)."""
    if family in ("mirror_even", "mirror_odd"):
        assert n % 2 == (family == "mirror_odd"), (family, n)
        return np.arange(n - 1, -1, -1)
    if family == "identity":
        return np.arange(n)
    if family == "scattered":                    # several fixed points, pairs that are not neighbours (what a 2D probe gives)
        rs = np.random.RandomState(1000 * n + seed)
        idx = rs.permutation(n)
        nfix = max(1, n // 4)
        nfix += (n - nfix) % 2                   # (an even number of points left for the pairs)
        perm = np.arange(n)
        rest = idx[nfix:]
        perm[rest[0::2]], perm[rest[1::2]] = rest[1::2], rest[0::2]
        return perm
    raise KeyError(family)


def mirror(n):
    return involution("mirror_odd" if n % 2 else "mirror_even", n)


def orbit_tables(perm):
    """ns, na, rep_i, rep_j (ns), orb, sgn (n): the pairs in the order of their first members, then the fixed points."""
    perm = np.asarray(perm)
    n = perm.size
    assert np.array_equal(perm[perm], np.arange(n)), "no involution"
    first = np.array([i for i in range(n) if perm[i] > i], dtype=int)
    fixed = np.array([i for i in range(n) if perm[i] == i], dtype=int)
    rep_i = np.concatenate([first, fixed])
    rep_j = perm[rep_i]
    orb, sgn = np.empty(n, dtype=int), np.zeros(n, dtype=int)
    orb[rep_j] = orb[rep_i] = np.arange(rep_i.size)
    sgn[first], sgn[perm[first]] = 1, -1
    return dict(ns=rep_i.size, na=first.size, rep_i=rep_i, rep_j=rep_j, orb=orb, sgn=sgn)


def fold_matrix(perm):
    """F (n, n) in long double: rows [0, ns) the symmetric orbits, rows [ns, n) the antisymmetric pairs."""
    tb = orbit_tables(perm)
    n, ns, na = np.asarray(perm).size, tb["ns"], tb["na"]
    E = np.eye(n, dtype=LD)
    S = E[tb["rep_i"]] + E[tb["rep_j"]]                          # (a fixed point's row counts its point twice ...)
    S = S / np.sqrt(np.sum(S * S, axis=1, keepdims=True))        # ... rows of unit length: 2 / sqrt(4) = 1, 1 / sqrt2 for a pair
    A = (E[tb["rep_i"][:na]] - E[tb["rep_j"][:na]]) * ISQ2
    return np.vstack([S, A])


def symmetric_grid(perm, seed=0, span=100.0):
    """Points t (n,) with t[perm[i]] = span - t[i]: a grid whose reflection about span / 2 is perm (exactly, in float64: the
    coordinates are multiples of 1/8 below 2^7).  Fixed points sit at span / 2 -- several of them coincide."""
    perm = np.asarray(perm)
    rs = np.random.RandomState(77 + seed + perm.size)
    t = np.empty(perm.size)
    for i in range(perm.size):
        if perm[i] > i:
            t[i] = np.round(rs.uniform(0.0, span / 2 - 1.0) * 8) / 8
            t[perm[i]] = span - t[i]
        elif perm[i] == i:
            t[i] = span / 2
    return t


# ------------------------------------------------------------------------------------------------ the operations
def _ld(x):
    x = np.asarray(x)
    return x if x.dtype == LD else x.astype(np.float64).astype(LD)    # (a long-double operand stays what it is)


def fold_rect(K, perm_r, perm_c):
    """F_r K F_c^T: ((ss, aa), (|.| ss, |.| aa))"""
    Fr, Fc = fold_matrix(perm_r), fold_matrix(perm_c)
    nsr, nsc = orbit_tables(perm_r)["ns"], orbit_tables(perm_c)["ns"]
    M, A = Fr @ _ld(K) @ Fc.T, np.abs(Fr) @ np.abs(_ld(K)) @ np.abs(Fc).T
    return (M[:nsr, :nsc], M[nsr:, nsc:]), (A[:nsr, :nsc], A[nsr:, nsc:])


def fold_rect_cross(K, perm_r, perm_c):
    """the off-diagonal blocks of F_r K F_c^T, which vanish when K commutes with the involutions"""
    Fr, Fc = fold_matrix(perm_r), fold_matrix(perm_c)
    nsr, nsc = orbit_tables(perm_r)["ns"], orbit_tables(perm_c)["ns"]
    M = Fr @ _ld(K) @ Fc.T
    return M[:nsr, nsc:], M[nsr:, :nsc]


def _blockdiag(Gss, Gaa):
    ns, na = Gss.shape[0], Gaa.shape[0]
    D = np.zeros((ns + na, ns + na), dtype=LD)
    D[:ns, :ns], D[ns:, ns:] = Gss, Gaa
    return D


def unfold_mat(Gss, Gaa, perm):
    """F^T diag(Gss, Gaa) F"""
    F = fold_matrix(perm)
    return F.T @ _blockdiag(_ld(Gss), _ld(Gaa)) @ F, np.abs(F).T @ _blockdiag(np.abs(_ld(Gss)), np.abs(_ld(Gaa))) @ np.abs(F)


def fold_lfp(Y, perm_s, perm_t):
    """(F_s (x) F_t) Y for Y (nx, R, nt) -> (nx, R, nt) in fold order on both sides"""
    Fs, Ft = fold_matrix(perm_s), fold_matrix(perm_t)
    return (np.einsum("qx,xrt,bt->qrb", Fs, _ld(Y), Ft), np.einsum("qx,xrt,bt->qrb", np.abs(Fs), np.abs(_ld(Y)), np.abs(Ft)))


def unfold_pred(X, perm_z, perm_t):
    """The inverse of (F_z (x) F_t) -- its transpose -- on folded predictions X (nz, R, C, nt), both fold orders: per component
    (C, nz, nt, R), values and magnitudes."""
    Fz, Ft = fold_matrix(perm_z), fold_matrix(perm_t)
    return (np.einsum("qz,qrcb,bt->cztr", Fz, _ld(X), Ft), np.einsum("qz,qrcb,bt->cztr", np.abs(Fz), np.abs(_ld(X)), np.abs(Ft)))


def pack_pred(X, perm_t, nsP=0, naP=0, ldin=0, pad=np.nan):
    """Folded predictions X (nz, R, C, nt) in the layout unfold_swap_sum reads: rows (zq, r) ldin apart, the C symmetric time blocks
    of nsP columns each, then the C antisymmetric blocks of naP; every padding column holds `pad`."""
    nz, R, C, nt = X.shape
    tb = orbit_tables(perm_t)
    ns, na = tb["ns"], tb["na"]
    nsP, naP = nsP or ns, naP or na
    ldin = ldin or C * (nsP + naP)
    out = np.full((nz * R, ldin), pad)
    Xr = X.reshape(nz * R, C, nt)
    for c in range(C):
        out[:, c * nsP:c * nsP + ns] = Xr[:, c, :ns]
        out[:, C * nsP + c * naP:C * nsP + c * naP + na] = Xr[:, c, ns:]
    return out


# ------------------------------------------------------------------------------------------------ scales
def pow2_above(b):
    """the power of two m with m / 2 <= b < m (what frexp / ldexp give), 1 for b = 0, non-finite b or b > 1.7e308; b itself where
    that power of two is 2^1024"""
    b = float(b)
    if not (b > 0.0 and b <= 1.7e308):
        return 1.0
    m = 1.0
    while m <= b and m < 2.0 ** 1023:
        m *= 2.0
    while m / 2.0 > b:
        m /= 2.0
    return m if m > b else b                     # (b >= 2^1023: the next power of two is not a float64)


def temporal_scale(sigma2):
    """the power of two above 2 sum |sigma2_c|, summed in float64 in index order as the host and the device form it"""
    bound = 0.0
    for s in sigma2:
        bound += abs(float(s))
    return pow2_above(2.0 * bound)


def psd_scales(K, perm, shift):
    """(m_s, m_a, margin): the power of two above the largest diagonal entry of each block of F K F^T + shift I, each block's
    entry floored at 2^-30 of the larger block's; margin: how far (relative) the nearest deciding value is from a power of two."""
    (ss, aa), _ = fold_rect(K, perm, perm)
    ds = float(np.max(np.abs(np.diag(ss) + LD(shift)))) if ss.size else 0.0
    da = float(np.max(np.abs(np.diag(aa) + LD(shift)))) if aa.size else 0.0
    big = max(ds, da)
    vs, va = max(ds, big * 2.0 ** -30), max(da, big * 2.0 ** -30)
    margin = min([abs(v / pow2_above(v) - f) for v in (vs, va) if v > 0 for f in (0.5, 1.0)] + [1.0])
    return pow2_above(vs), pow2_above(va), margin


# ------------------------------------------------------------------------------------------------ temporal Gram in long double
def temporal_exponent(kind, d, ell):
    """a: the magnitude of the exponential's argument of one kernel value (float64)"""
    d = np.abs(np.asarray(d, dtype=np.float64))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if kind == MT.SE:
            return 0.5 * (d / ell) ** 2
        if kind == MT.MATERN:
            return d / ell
        return MT.scaled_distance(kind, d, ell)


def temporal_gram(t, kinds, ell, sigma2):
    """Kt = sum_c sigma2_c k_c on the grid t in long double, with the propagated error bound of a float64 evaluation entry by entry:
    (16 + 4 a) u |sigma2 k| + max(1, sigma2) 2^-1074 per component (test_matern_kinds.py, item 1), C - 1 additions of the running
    sum.  -> (Kt, bound, magnitude sum_c |sigma2_c k_c|)"""
    t = np.asarray(t, dtype=np.float64)
    n = t.size
    K, bound, mag = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    d = t[:, None] - t[None, :]
    with np.errstate(under="ignore"):
        for kind, l, s2 in zip(kinds, ell, sigma2):
            v = MT.gram(kind, t, t, l, s2, LD)
            a = np.minimum(temporal_exponent(kind, d, l), 1e6)
            K += v
            mag += np.abs(v)
            bound += (16.0 + 4.0 * a).astype(LD) * LD(U) * np.abs(v) + LD(max(1.0, abs(s2))) * LD(2.0) ** -1074
    bound += LD(max(len(kinds) - 1, 0)) * LD(U) * mag
    return K, bound, mag


def se_gram(t, ell):
    """exp(-(t_i - t_j)^2 / (2 ell^2)) generated in long double and rounded to float64"""
    return np.asarray(MT.gram(MT.SE, t, t, ell, 1.0, LD), dtype=np.float64)
