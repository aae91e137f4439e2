"""The dense Cholesky path on its own (chol.hip: potrf_device, trsm_lower_device, trsm_lower_trans_device, logdet_chol_device,
through gpcsd_potrf / gpcsd_trsm_lower / gpcsd_trsm_lower_trans / gpcsd_logdet_chol, which put nothing between the caller and the
kernels) against long-double measures (chol_ref.py), at the orders where potrf_device changes path -- NB = 128, NBO = 256: one
sub-block up to 128, two with the deferred L21 copy up to 256, the first panel product and trailing update at 257, look-ahead and
gates from 513, the update split behind two gates at 769, look-ahead steps following one another at 1025 -- and on the matrices its
consumers hand it (condition up to 1e10; chol_ref.FAMILIES).

The gate.  A kernel's measure -- rho for the factor, the componentwise backward error omega for the solves, the log-determinant's
error -- must be at most MARGIN x max(the yardstick's measure, u), u = 2^-53; the yardstick is LAPACK in float64 (a float64 sum
for the log-determinant) on the same operands, never a kernel.  MARGIN = 100 is what this project gives a float64 kernel over an
unhurried float64 implementation (test_tridiag_kernels.py).  From above: a kernel that is wrong -- a dropped rank-16 update, a
stale entry of the shared inverse buffer read as data, a padding row that leaks, a mirrored index -- leaves rho, omega >= 1e-6,
1e10 u, against a gate of at most ~2000 u (test_measures_see_a_skipped_rank16_update shows it on the CPU).  From below: 2-ulp
roots, MFMA's four-wide association and rank-256 updates are factors of order one.  What lies between is the growth from the
explicitly inverted diagonal blocks every panel solve and triangular solve multiplies by (backward error can grow with
|| |L11| |inv L11| ||; LAPACK's substitution has no such term): the quantity this file measures.

Measured on the MI355X, worst ratio of a kernel's measure to max(yardstick's, u) over the sizes and right-hand-side counts below
(both factors for the solves), per family:

                      wishart   exp64   se_jitter   se_matern   scaled   equilibrated
  potrf                  9.3      3.0       2.7         6.6       8.7        1.0
  trsm_lower             2.1       -        1.2          -         -         1.4
  trsm_lower_trans       2.5       -        1.6          -         -         1.6
  logdet_chol            0.7      0.4       0.7         0.4       1.0        1.3

(potrf's own ~10 .. 35 u on wishart / scaled against LAPACK's 2.5 .. 4 u is there from n = 127 on: the order of summation in the
diagonal workgroup, not the inverses.)  No family needed a strict xfail.  One needed a fix: BEFORE every product with an
explicitly inverted diagonal block was followed by its correction step (chol.hip, header) the se_jitter family -- condition 5e9,
|| |L11| |inv L11| ||_inf = 2.6e5 on its leading 256 rows, against 2e3 for equilibrated, 126 for exp64, 30 for wishart -- failed
this gate in every case above 128 rows: potrf 6.8e3 (rho = 3.8e4 u = 4e-12 from n = 385 on), trsm_lower 5.6e5, trsm_lower_trans
7.2e5 (omega = 6e-11; forward error 5.5e-10 against LAPACK's 1.4e-12 at n = 128, nrhs = 1).  The other families were where they
are now (potrf within 8.7, the solves within 4.8).
Roots (test_roots_of_a_diagonal_matrix, 512 pivots): worst error 0.499 ulp -- correctly rounded on every one of them; the 2 ulp
chol.hip allows are not used.  Scale (test_potrf_at_extreme_scales): the factor of 2^+-600 A IS 2^+-300 times the factor of A bit
for bit, at n = 129 and 300.
"""
import functools
import re

import numpy as np
import pytest

import chol_ref as CR

MARGIN = 100.0
U = CR.U

POTRF_SIZES = [1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 383, 385, 512, 513, 769, 1025]
# the long-double residual is what the time goes to (seconds at 1025): two families there, three at 769
POTRF_FAMILIES_AT = {1025: ("wishart", "se_jitter"), 769: ("wishart", "se_jitter", "equilibrated")}
SOLVE_SIZES = [1, 17, 128, 129, 256, 257, 300, 513]
SOLVE_NRHS = [1, 5, 33, 130]
SOLVE_FAMILIES = ("wishart", "se_jitter", "equilibrated")
PIVOT_SIZES = [130, 300, 700]
PIVOTS = [0, 6, 15, 16, 127, 128, 200, 255, 256, 300, 511, 512, 600]
UPPER_SIZES = [129, 300, 700]
SCALE_SIZES = [129, 300]

POTRF_CASES = [(fam, n) for n in POTRF_SIZES for fam in POTRF_FAMILIES_AT.get(n, tuple(CR.FAMILIES))]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(fam, n):
    """A family's matrix and LAPACK's factor of it, once per process: every test of the case reads them, none writes."""
    c = Case()
    c.fam, c.n = fam, n
    c.A = CR.family(fam, n)
    c.L_lapack = CR.lapack_factor(c.A)
    c.L_lapack.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _rho_lapack(fam, n):
    c = _case(fam, n)
    return CR.rho(c.A, c.L_lapack)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------ the reference itself (no GPU)
@pytest.mark.parametrize("fam", ["wishart", "se_matern", "scaled"])
def test_long_double_factor_and_solves_agree_with_lapack(fam):
    n = 40
    A = CR.family(fam, n)
    L = CR.cholesky_ld(A)
    Lr = CR.lapack_factor(A)
    assert L.dtype == CR.LD and np.all(np.triu(L, 1) == 0)
    scale = np.sqrt(np.diag(A))[:, None]                               # |l_ij| <= sqrt(a_ii): rows of the scaled family differ by decades
    assert float(np.max(np.abs(L - Lr) / scale)) <= 1e-12
    B = np.random.RandomState(3).standard_normal((n, 4))
    for trans in (False, True):
        X = CR.solve_lower_ld(Lr, B, trans)
        Xr = CR.lapack_solve(Lr, B, trans)
        assert CR.forward_error(Xr, X) <= 1e-12 * np.linalg.cond(Lr)
        assert CR.omega(Lr, X.astype(np.float64), B, trans) <= 2 * U   # the long-double solution, rounded: half an ulp of each entry
    assert CR.solve_lower_ld(Lr, B[:, 0]).shape == (n,)
    assert CR.logdet_error(CR.logdet_f64(Lr), Lr) <= 1e-14
    assert abs(CR.logdet_f64(Lr) - np.linalg.slogdet(A)[1]) <= 1e-12 * n * max(1.0, np.max(np.abs(np.log(np.diag(Lr)))))


def test_rho_reports_a_perturbed_factor():
    for fam, (i, j) in (("wishart", (10, 10)), ("se_matern", (20, 19)), ("se_matern", (63, 63))):
        A = CR.family(fam, 64)
        L = CR.lapack_factor(A)
        assert CR.rho(A, L) <= 64 * U
        Lp = L.copy()
        Lp[i, j] += 1e-9 * abs(Lp[i, j])
        assert CR.rho(A, Lp) > 1e-10, (fam, i, j)
    Lp = L.copy()
    Lp[5, 2] = np.nan
    assert CR.rho(A, Lp) == float("inf")
    # invariant under diagonal scaling by powers of two, bit for bit
    s = 2.0 ** np.random.RandomState(0).randint(-200, 200, 64)
    assert CR.rho(A * (s[:, None] * s[None, :]), L * s[:, None]) == CR.rho(A, L)


@pytest.mark.parametrize("trans", [False, True])
def test_omega_reports_a_perturbed_solution(trans):
    A = CR.family("wishart", 64)
    L = CR.lapack_factor(A)
    B = np.random.RandomState(1).standard_normal((64, 3))
    X = CR.lapack_solve(L, B, trans)
    assert CR.omega(L, X, B, trans) <= 64 * U
    Xp = X.copy()
    Xp[17, 1] += 1e-9 * abs(Xp[17, 1])
    assert CR.omega(L, Xp, B, trans) > 1e-10
    assert CR.forward_error(Xp, CR.solve_lower_ld(L, B, trans)) > 1e-11
    # 0/0 counts as 0: a zero right-hand side with its zero solution, and a leading zero row
    Z = np.zeros((64, 2))
    assert CR.omega(L, Z, Z, trans) == 0.0
    # a solution of the transposed system is none of the plain one
    assert CR.omega(L, X, B, not trans) > 1e-3


def test_measures_see_a_skipped_rank16_update():
    """What the margin is justified with from above: a right-looking factorisation in panels of 16 that skips ONE rank-16 update
    of one 16 x 16 fragment is off by ten orders of magnitude and more, not by a factor."""
    n = 129

    def blocked(A, skip):
        W = np.tril(A).copy()
        for k0 in range(0, n, 16):
            k1 = min(n, k0 + 16)
            W[k0:k1, k0:k1] = np.linalg.cholesky(W[k0:k1, k0:k1] + np.tril(W[k0:k1, k0:k1], -1).T)
            if k1 < n:
                W[k1:, k0:k1] = CR.lapack_solve(W[k0:k1, k0:k1], W[k1:, k0:k1].T).T
                upd = W[k1:, k0:k1] @ W[k1:, k0:k1].T
                if skip and k0 == 32:
                    upd[64 - k1:80 - k1, 48 - k1:64 - k1] = 0.0          # fragment rows 64..79, columns 48..63: not updated
                W[k1:, k1:] -= np.tril(upd)
        return W

    for fam in ("wishart", "se_matern", "exp64"):
        A = CR.family(fam, n)
        good = CR.rho(A, CR.lapack_factor(A))
        assert CR.rho(A, blocked(A, False)) <= MARGIN * max(good, U)
        try:
            bad = CR.rho(A, blocked(A, True))
        except np.linalg.LinAlgError:          # (the missing update left a non-positive pivot: potrf would raise, which fails the test too)
            bad = float("inf")
        assert bad >= 1e-6 and bad > 1e6 * MARGIN * max(good, U), (fam, bad, good)


@pytest.mark.parametrize("fam", list(CR.FAMILIES))
def test_families_are_symmetric_and_lapack_factors_them(fam):
    sizes = sorted({n for f, n in POTRF_CASES if f == fam} | (set(SOLVE_SIZES) if fam in SOLVE_FAMILIES else set())
                   | set(UPPER_SIZES + SCALE_SIZES))
    for n in sizes:
        A = CR.family(fam, n)
        assert A.shape == (n, n) and A.dtype == np.float64 and not A.flags.writeable
        assert _same_bits(A, A.T.copy()), "%s at n = %d is not symmetric bit for bit" % (fam, n)
        assert _same_bits(A, CR.family(fam, n)), "not reproducible"
        L = CR.lapack_factor(A)                                       # raises LinAlgError if LAPACK meets a non-positive pivot
        assert np.all(np.isfinite(L)) and np.all(np.diag(L) > 0)
    for n in (17, 129):                  # (the residual at every size is the GPU tests' yardstick; here only that it is sane)
        r = CR.rho(CR.family(fam, n), CR.lapack_factor(CR.family(fam, n)))
        # |A - L L^T| <= gamma_{n+1} |L| |L^T| (Higham, Accuracy and Stability, Thm 10.3) and (|L| |L^T|)_ij <= sqrt((a_ii + e)(a_jj + e))
        assert 0.0 < r <= 2.0 * (n + 1) * U, (fam, n, r)


# ------------------------------------------------------------------------------------------------ the gate
WORST = {}                   # (routine, family) -> worst ratio of the kernel's measure to max(yardstick's, u) in this process


def _gate(routine, fam, label, m_kernel, m_yard):
    ratio = m_kernel / max(m_yard, U)
    WORST[(routine, fam)] = max(WORST.get((routine, fam), 0.0), ratio)
    print("[chol] %-16s %-12s %-28s kernel %9.3g u   yardstick %9.3g u   ratio %8.3g" % (routine, fam, label, m_kernel / U, m_yard / U, ratio))
    assert m_kernel <= MARGIN * max(m_yard, U), \
        "%s, %s %s: %.3e (%.1f u) against the yardstick's %.3e (%.1f u): ratio %.1f > %g" \
        % (routine, fam, label, m_kernel, m_kernel / U, m_yard, m_yard / U, ratio, MARGIN)


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    from gpcsd_amd import _hip
    yield _hip.default_context()
    for (routine, fam), r in sorted(WORST.items()):
        print("[chol] worst ratio  %-16s %-12s %.3g" % (routine, fam, r))


def _fresh(call):
    """call(context) on a context of its own that has done nothing else."""
    from gpcsd_amd import _hip
    c = _hip.Context()
    try:
        return call(c)
    finally:
        c.close()


_KERNEL_FACTOR = {}


def _kernel_factor(ctx, fam, n):
    if (fam, n) not in _KERNEL_FACTOR:
        L = ctx.potrf(_case(fam, n).A)
        L.setflags(write=False)
        _KERNEL_FACTOR[(fam, n)] = L
    return _KERNEL_FACTOR[(fam, n)]


def _check_factor(ctx, fam, label, A, L, rho_yard):
    assert L.shape == A.shape and np.all(np.isfinite(L))
    assert np.all(np.triu(L, 1) == 0.0), "the strictly upper part of the factor is not exactly zero"
    assert np.all(np.diag(L) > 0)
    _gate("potrf", fam, label, CR.rho(A, L), rho_yard)
    _gate("logdet_chol", fam, label, CR.logdet_error(ctx.logdet_chol(L), L), CR.logdet_error(CR.logdet_f64(L), L))


@pytest.mark.gpu
@pytest.mark.parametrize("fam,n", POTRF_CASES, ids=["%s-%d" % c for c in POTRF_CASES])
def test_potrf_accuracy(ctx, fam, n):
    c = _case(fam, n)
    L = ctx.potrf(c.A)
    _KERNEL_FACTOR.setdefault((fam, n), L)
    _check_factor(ctx, fam, "n=%d" % n, c.A, L, _rho_lapack(fam, n))


@pytest.mark.gpu
@pytest.mark.parametrize("nrhs", SOLVE_NRHS)
@pytest.mark.parametrize("n", SOLVE_SIZES)
@pytest.mark.parametrize("fam", SOLVE_FAMILIES)
@pytest.mark.parametrize("routine", ["trsm_lower", "trsm_lower_trans"])
def test_solves_on_both_factors(ctx, routine, fam, n, nrhs):
    trans = routine == "trsm_lower_trans"
    solve = getattr(ctx, routine)
    B = np.random.RandomState(131 * n + nrhs).standard_normal((n, nrhs))
    for src, L in (("lapack's L", _case(fam, n).L_lapack), ("potrf's L", _kernel_factor(ctx, fam, n))):
        X = solve(L, B)
        assert X.shape == B.shape and np.all(np.isfinite(X))
        Xy = CR.lapack_solve(L, B, trans)
        Xld = CR.solve_lower_ld(L, B, trans)
        label = "n=%d nrhs=%d %s" % (n, nrhs, src)
        print("[chol] %-16s %-12s %-28s forward error %9.3g   yardstick's %9.3g" % (routine, fam, label, CR.forward_error(X, Xld), CR.forward_error(Xy, Xld)))
        _gate(routine, fam, label, CR.omega(L, X, B, trans), CR.omega(L, Xy, B, trans))
        if nrhs == 1:                                                  # a 1-D right-hand side keeps its shape (and its result)
            x1 = solve(L, B[:, 0])
            assert x1.shape == (n,) and _same_bits(x1, X[:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("spread", ["[1, 4)", "1e-290 .. 1e290"])
def test_roots_of_a_diagonal_matrix(ctx, spread):
    """The factor of diag(d) is diag(sqrt(d)): sqrt_rsqrt's roots (v_rsq_f64 + two Goldschmidt steps + one correction) on their
    own, every pivot of both sub-blocks.  chol.hip promises 2 ulp; everything off the diagonal must stay an exact zero."""
    n = 256
    rs = np.random.RandomState(len(spread))
    d = rs.uniform(1.0, 4.0, n) if spread == "[1, 4)" else 10.0 ** rs.uniform(-290.0, 290.0, n)
    d[:4] = [1.0, 4.0, 2.0, 3.0] if spread == "[1, 4)" else [1e-290, 1e290, 2.0 ** -600, 2.0 ** 601]
    L = ctx.potrf(np.diag(d))
    assert np.all(L[~np.eye(n, dtype=bool)] == 0.0)
    root = np.sqrt(d.astype(CR.LD))
    ulps = np.abs(np.diag(L).astype(CR.LD) - root) / np.spacing(root.astype(np.float64)).astype(CR.LD)
    print("[chol] roots            diagonal     d in %-18s worst error %.3f ulp, mean %.3f ulp" % (spread, float(np.max(ulps)), float(np.mean(ulps))))
    assert float(np.max(ulps)) <= 2.0
    # a representable root comes out exact: the last step adds (d - g^2) h, formed without rounding d - g^2, to a g one ulp off at most
    squares = [0, 1] if spread == "[1, 4)" else [2]
    assert all(L[i, i] * L[i, i] == d[i] for i in squares)


# ---- the reported pivot
@functools.lru_cache(maxsize=None)
def _pivot_base(n):
    M = np.random.RandomState(n).standard_normal((n, n))
    A0 = M @ M.T / n + np.eye(n)
    A0 = np.tril(A0) + np.tril(A0, -1).T
    A0.setflags(write=False)
    return A0, CR.lapack_factor(A0)


_FRESH_FACTOR = {}


def _fresh_pivot_factor(n):
    if n not in _FRESH_FACTOR:
        A0, L0 = _pivot_base(n)
        L = _fresh(lambda c: c.potrf(A0))
        assert CR.rho(A0, L) <= MARGIN * max(CR.rho(A0, L0), U)
        _FRESH_FACTOR[n] = L
    return _FRESH_FACTOR[n]


def _expect_status(ctx, A, status):
    with pytest.raises(np.linalg.LinAlgError) as e:
        ctx.potrf(A)
    m = re.search(r"\(status (-?\d+)\)", str(e.value))
    assert m and int(m.group(1)) == status, "expected status %d (first failing pivot + 1), got: %s" % (status, e.value)


def _good_again(ctx, n):
    L = ctx.potrf(_pivot_base(n)[0])
    assert _same_bits(L, _fresh_pivot_factor(n)), "after a failed factorisation the next one differs from a fresh context's"


PIVOT_CASES = [(n, k) for n in PIVOT_SIZES for k in sorted({k for k in PIVOTS if k < n} | {n - 1})]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", PIVOT_CASES, ids=["n%d-k%d" % c for c in PIVOT_CASES])
def test_potrf_reports_the_first_failing_pivot(ctx, n, k):
    """status = first failing pivot + 1, whichever sub-block, outer block or look-ahead step meets it (the index is kept by an
    atomicCAS: the first IN TIME, while the next diagonal block runs on a side stream).  k = 6: status 7 has a meaning of its own
    in the prediction calls; potrf reports it as a pivot all the same."""
    A0, L0 = _pivot_base(n)
    A = A0.copy()
    A[k, k] -= L0[k, k] ** 2 + 1.0                                     # pivots before k as they were, pivot k about -1
    _expect_status(ctx, A, k + 1)
    _good_again(ctx, n)


@pytest.mark.gpu
@pytest.mark.parametrize("i,j", [(200, 200), (200, 3), (260, 130)])
def test_potrf_reports_a_nan_as_a_failing_pivot(ctx, i, j):
    n = 300
    A = _pivot_base(n)[0].copy()
    A[i, j] = A[j, i] = np.nan                                         # reaches pivot i first: row i of L from column j on
    _expect_status(ctx, A, i + 1)
    _good_again(ctx, n)


# ---- only the lower triangle is read
@pytest.mark.gpu
@pytest.mark.parametrize("fill", ["finite", "nan"])
@pytest.mark.parametrize("n", UPPER_SIZES)
def test_potrf_reads_only_the_lower_triangle(ctx, n, fill):
    A = _case("se_matern", n).A
    L = ctx.potrf(A)
    junk = 1e3 * np.random.RandomState(n).standard_normal((n, n)) if fill == "finite" else np.full((n, n), np.nan)
    Au = np.tril(A) + np.triu(junk, 1)
    assert _same_bits(np.tril(Au), np.tril(A))
    Lu = ctx.potrf(Au)
    assert _same_bits(Lu, L), "the factor depends on what lies above the diagonal of the input"


@pytest.mark.gpu
@pytest.mark.parametrize("routine", ["trsm_lower", "trsm_lower_trans"])
def test_solves_read_only_the_lower_triangle(ctx, routine):
    """The solves' correction step forms its residual with L: the diagonal blocks come from a copy with zeros above the diagonal,
    so what the caller leaves there -- potrf leaves zeros, another producer may not -- stays unread."""
    n = 300
    L = _case("equilibrated", n).L_lapack
    B = np.random.RandomState(5).standard_normal((n, 5))
    X = getattr(ctx, routine)(L, B)
    Xn = getattr(ctx, routine)(L + np.triu(np.full((n, n), np.nan), 1), B)
    assert _same_bits(Xn, X), "the solution depends on what lies above the diagonal of L"


# ---- no state carries over
@pytest.mark.gpu
def test_no_state_carries_over_between_calls():
    """chol_Linv, chol_inv_tmp, chol_panel, trsm_xblk and chol_token are shared between the routines and between calls: a
    sequence on one context gives, call by call, the bits of the same call made first on a fresh context."""
    A700, A100 = _case("se_matern", 700).A, _case("se_jitter", 100).A
    rs = np.random.RandomState(11)
    L300, L129, L17 = _case("equilibrated", 300).L_lapack, _case("se_jitter", 129).L_lapack, _case("wishart", 17).L_lapack
    B300, b129, B17 = rs.standard_normal((300, 130)), rs.standard_normal(129), rs.standard_normal((17, 5))
    calls = [("potrf(700)", lambda c: c.potrf(A700)),
             ("potrf(100)", lambda c: c.potrf(A100)),
             ("trsm_lower(300, 130)", lambda c: c.trsm_lower(L300, B300)),
             ("trsm_lower_trans(129, 1)", lambda c: c.trsm_lower_trans(L129, b129)),
             ("potrf(700) again", lambda c: c.potrf(A700)),
             ("trsm_lower(17, 5)", lambda c: c.trsm_lower(L17, B17))]
    from gpcsd_amd import _hip
    seq = _hip.Context()
    try:
        got = [call(seq) for _, call in calls]
        timeouts = seq.potrf_gate_timeouts()
    finally:
        seq.close()
    for (name, call), g in zip(calls, got):
        assert _same_bits(g, _fresh(call)), "%s in a sequence differs from the same call on a fresh context" % name
    assert timeouts == 0


# ---- scale
@pytest.mark.gpu
@pytest.mark.parametrize("n", SCALE_SIZES)
def test_potrf_at_extreme_scales(ctx, n):
    """rho is invariant under scaling, so A and 2^+-600 A pass the same gate (entries near 1e+-180, factors near 1e+-90: roots,
    reciprocal roots and the explicit inverses far from 1).  Whether L scales bit for bit by 2^+-300 is printed, not asserted."""
    c = _case("se_jitter", n)
    L1 = _kernel_factor(ctx, "se_jitter", n)
    _check_factor(ctx, "se_jitter", "n=%d" % n, c.A, L1, _rho_lapack("se_jitter", n))
    for e in (600, -600):
        As = c.A * 2.0 ** e                                            # exact
        Ls = ctx.potrf(As)
        _check_factor(ctx, "se_jitter", "n=%d x 2^%d" % (n, e), As, Ls, CR.rho(As, CR.lapack_factor(As)))
        print("[chol] scale            se_jitter    n=%d x 2^%d: L %s the unscaled factor times 2^%d bit for bit"
              % (n, e, "IS" if _same_bits(Ls, L1 * 2.0 ** (e // 2)) else "is NOT", e // 2))
