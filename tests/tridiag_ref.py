"""Extended-precision reference for the shifted symmetric tridiagonal systems of the basis U (x) Q (gram.hip: ll_tridiag_kernel,
ll_tridiag_scan_kernel, tridiag_solve_kernel).  No GPU, no library: mpmath at 50 digits beside plain NumPy.

One item is A = lam m T + sig2 I with T = tridiag(d, e) and a set of right-hand sides (rows).  `reference_item` takes the float64
operands as they are (every float64 is an exact rational: lam m d_k + sig2 is formed without rounding in the 50-digit arithmetic) and
returns

  * the L D L^T pivots D_k = a_k - b_{k-1}^2 / D_{k-1}, sum log D_k, w^T A^-1 w per row and the solutions A^-1 w, to 50 digits;
  * the same four quantities from the textbook sequential recurrence in float64 (NumPy, IEEE division, no fused operations): the
    YARDSTICK a kernel's error is measured against -- what an unhurried float64 implementation loses on the same operands.

Values that tests subtract kernel results from are kept as unevaluated sums hi + lo of two float64 (~32 digits): the difference
of a kernel's float64 result and the reference is then formed without rounding the reference to float64 first.
"""
import math

import numpy as np
from mpmath import mp, mpf
from mpmath import log as mp_log
from mpmath.libmp import from_float, fzero, mpf_add, mpf_mul, mpf_sub, to_float

DPS = 50
U = 2.0 ** -53          # unit roundoff of float64


def _split(x):
    hi = float(x)
    return hi, float(x - hi)


class ItemRef:
    """Reference of one item.  n columns, R rows.
    pivots: list of mpf;  pivots_f64: the yardstick's
    logdet (hi, lo), logdet_scale = sum max(1, |log D_k|) (float), logdet_f64
    quad (hi, lo) arrays (R,): w^T A^-1 w per row;  quad_f64 (R,)
    x (hi, lo) arrays (R, n);  x_f64 (R, n)"""

    def quad_err(self, value, R):
        """|value - sum of the first R rows' quadratic forms|, the reference taken at its full precision"""
        return abs(math.fsum([value] + [-v for v in self.quad_hi[:R]] + [-v for v in self.quad_lo[:R]]))

    def quad_sum(self, R):
        return math.fsum(list(self.quad_hi[:R]) + list(self.quad_lo[:R]))

    def quad_f64_sum(self, R):
        s = 0.0
        for v in self.quad_f64[:R]:          # sequential float64 sum over the rows
            s += float(v)
        return s

    def logdet_err(self, value):
        return abs(math.fsum([value, -self.logdet_hi, -self.logdet_lo]))

    def x_err(self, X):
        """per row: max_k |X - x| / max_k |x| against the 50-digit solutions; X (R', n) with R' <= R"""
        r = X.shape[0]
        diff = (X - self.x_hi[:r]) - self.x_lo[:r]
        return np.max(np.abs(diff), axis=1) / np.max(np.abs(self.x_hi[:r]), axis=1)


def recurrence_f64(lam, m, d, e, sig2, rows):
    """The plain sequential recurrence in float64: pivots, sum log D, per-row quadratic forms, solutions."""
    d = np.asarray(d, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    W = np.asarray(rows, dtype=np.float64).reshape(-1, d.size)
    n = d.size
    lm = np.float64(lam) * np.float64(m)
    a = lm * d + np.float64(sig2)
    b = lm * e
    D = np.empty(n)
    l = np.zeros(n)
    Z = np.empty_like(W)
    q = np.zeros(W.shape[0])
    logdet = 0.0
    for k in range(n):
        if k == 0:
            D[0] = a[0]
            Z[:, 0] = W[:, 0]
        else:
            l[k] = b[k - 1] / D[k - 1]
            D[k] = a[k] - l[k] * b[k - 1]
            Z[:, k] = W[:, k] - l[k] * Z[:, k - 1]
        q = q + Z[:, k] * Z[:, k] / D[k]
        logdet = logdet + (math.log(D[k]) if D[k] > 0 else float("nan"))
    X = np.empty_like(W)
    for k in range(n - 1, -1, -1):
        X[:, k] = Z[:, k] / D[k]
        if k + 1 < n:
            X[:, k] = X[:, k] - l[k + 1] * X[:, k + 1]
    return D, logdet, q, X


def reference_item(lam, m, d, e, sig2, rows):
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    n = d.size
    if n < 1 or e.size != n - 1:
        raise ValueError("a tridiagonal matrix of order n >= 1 needs n diagonal and n - 1 off-diagonal entries")
    W = np.asarray(rows, dtype=np.float64).reshape(-1, n)
    R = W.shape[0]
    ref = ItemRef()
    with mp.workdps(DPS):
        lm = mpf(float(lam)) * mpf(float(m))
        s2 = mpf(float(sig2))
        a = [lm * mpf(float(v)) + s2 for v in d]
        b = [lm * mpf(float(v)) for v in e]
        D, l, Dinv = [a[0]], [mpf(0)], []
        for k in range(1, n):
            l.append(b[k - 1] / D[k - 1])
            D.append(a[k] - l[k] * b[k - 1])
        ref.pivots = D
        ref.positive = all(v > 0 for v in D)
        x_hi, x_lo = np.zeros((R, n)), np.zeros((R, n))
        q_hi, q_lo = np.zeros(R), np.zeros(R)
        if ref.positive:
            logs = [mp_log(v) for v in D]
            ref.logdet_hi, ref.logdet_lo = _split(sum(logs, mpf(0)))
            ref.logdet_scale = float(sum((max(abs(v), mpf(1)) for v in logs), mpf(0)))
            # the sweeps over the rows on mpmath's raw values (libmp: the same arithmetic without the mpf objects around it,
            # a third of the time): z_k = w_k - l_k z_{k-1}, t_k = z_k / D_k, q = sum z_k t_k, x_k = t_k - l_{k+1} x_{k+1}
            prec, rnd = mp.prec, "n"
            lr = [v._mpf_ for v in l]
            Dinv = [(1 / v)._mpf_ for v in D]

            def split(v):
                hi = to_float(v, rnd=rnd)
                return hi, to_float(mpf_sub(v, from_float(hi), prec, rnd), rnd=rnd)

            for r in range(R):
                z = [from_float(float(v)) for v in W[r]]
                for k in range(1, n):
                    z[k] = mpf_sub(z[k], mpf_mul(lr[k], z[k - 1], prec, rnd), prec, rnd)
                t = [mpf_mul(z[k], Dinv[k], prec, rnd) for k in range(n)]
                q = fzero
                for k in range(n):
                    q = mpf_add(q, mpf_mul(z[k], t[k], prec, rnd), prec, rnd)
                q_hi[r], q_lo[r] = split(q)
                x = t[n - 1]
                x_hi[r, n - 1], x_lo[r, n - 1] = split(x)
                for k in range(n - 2, -1, -1):
                    x = mpf_sub(t[k], mpf_mul(lr[k + 1], x, prec, rnd), prec, rnd)
                    x_hi[r, k], x_lo[r, k] = split(x)
        ref.quad_hi, ref.quad_lo, ref.x_hi, ref.x_lo = q_hi, q_lo, x_hi, x_lo
    ref.pivots_f64, ref.logdet_f64, ref.quad_f64, ref.x_f64 = recurrence_f64(lam, m, d, e, sig2, W)
    return ref
