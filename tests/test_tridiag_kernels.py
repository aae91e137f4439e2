"""The shifted-tridiagonal kernels of the default step on their own (gram.hip: ll_tridiag_kernel, ll_tridiag_scan_kernel,
tridiag_solve_kernel<32 / 64>, through gpcsd_debug_ll_tridiag / gpcsd_debug_tridiag_solve) against a 50-digit reference
(tridiag_ref.py), at the block sizes, trial counts and conditions where they take another path.

The accuracy gate.  Per item (spatial eigen-row x', parity block p) the kernel's error against the 50-digit value -- of the
log-determinant, of the quadratic form summed over the trials, and of every trial's solution in the max norm relative to the
solution's -- must be at most MARGIN times the error of the plain sequential float64 recurrence (IEEE division, NumPy) on the
same operands, plus a floor of 8 np u relative (u = 2^-53) for items on which that yardstick happens to be exact.  The yardstick
is the reference recurrence, never a kernel.  "Relative" is to the quantity itself for the quadratic form (a sum of positive
terms) and the solution; for the log-determinant it is to sum_k max(1, |log D_k|): the terms have both signs, so their sum says
nothing about the size of what was added, and a relative error u of a pivot near 1 moves its logarithm by u absolutely whatever
that logarithm's own size.

MARGIN = 100: three times the worst ratio (35 on a pivot, 24 on a log-determinant) that a NumPy transcription of the scan kernel's
association order gave against the sequential recurrence at lam m / sig2 up to 1e13; the serial kernel's 2-ulp reciprocal stays far
inside it.  A kernel that is wrong -- an off-by-one in e, a dropped column, a lane with its neighbour's trial, an unsolved padding
column -- is wrong by 1e-3 or more.

Measured on the MI355X, worst ratio of a kernel's error to the yardstick's over the items above the floor, at lam m / sig2 = 1e4,
1e8, 1e12 (at 1 everything is below the floor): serial kernel 3.7, 2.3, 2.1; scan kernel 1.0, 2.0, 8.8; solve 21.9, 1.8, 8.8.
Before the scan's pivots were corrected by a Newton step (gram.hip) this gate failed: scan kernel 520, 52, 988 (quadratic forms
of the Toeplitz and decoupled families), solve 1430, 260, 694.  The worst ratio is above 10: MARGIN stays at 100.
"""
import functools
import math

import numpy as np
import pytest

import tridiag_ref as TR

MARGIN = 100.0
U = TR.U
PAD = 3                      # NaN columns in front of, between and behind the two blocks
M_BLOCK = (2.5, 0.37)        # the scales m_p of the two parity blocks


# ------------------------------------------------------------------------------------------------ the reference itself (no GPU)
def _random_spd_tridiagonal(n, rng):
    e = rng.uniform(-1.0, 1.0, max(n - 1, 0))
    d = rng.uniform(0.5, 1.5, n)
    d[:n - 1] += np.abs(e)
    d[1:] += np.abs(e)                      # strictly diagonally dominant
    return d, e


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_reference_matches_dense_linear_algebra(n):
    rng = np.random.RandomState(100 + n)
    d, e = _random_spd_tridiagonal(n, rng)
    lam, m, sig2 = 0.7, 1.3, 0.2
    W = rng.standard_normal((3, n))
    ref = TR.reference_item(lam, m, d, e, sig2, W)
    A = lam * m * (np.diag(d) + np.diag(e, 1) + np.diag(e, -1)) + sig2 * np.eye(n)
    sign, logdet = np.linalg.slogdet(A)
    X = np.linalg.solve(A, W.T).T
    assert sign == 1.0 and ref.positive
    assert abs(ref.logdet_hi - logdet) <= 1e-12 * max(1.0, abs(logdet))
    assert np.max(np.abs(ref.x_hi - X)) <= 1e-12 * np.max(np.abs(X))
    assert np.max(np.abs(ref.quad_hi - np.sum(W * X, axis=1))) <= 1e-12 * np.max(ref.quad_hi)
    # the pivots multiply to the determinant; the yardstick agrees with the 50-digit values at this condition
    assert abs(math.fsum(math.log(float(v)) for v in ref.pivots) - logdet) <= 1e-12 * max(1.0, abs(logdet))
    assert np.max(np.abs(ref.pivots_f64 / np.array([float(v) for v in ref.pivots]) - 1.0)) <= 1e-12
    assert ref.logdet_err(ref.logdet_f64) <= 1e-12 * max(1.0, abs(logdet))
    assert np.max(ref.x_err(ref.x_f64)) <= 1e-12
    assert ref.quad_err(ref.quad_f64_sum(3), 3) <= 1e-12 * ref.quad_sum(3)


@pytest.mark.parametrize("sig2", [1.0, 1e-4, 0.3])
def test_reference_closed_forms_for_lam_zero(sig2):
    n, R = 7, 4
    rng = np.random.RandomState(5)
    d, e = _random_spd_tridiagonal(n, rng)
    W = rng.standard_normal((R, n))
    ref = TR.reference_item(0.0, 2.5, d, e, sig2, W)
    from mpmath import mp, mpf, log
    with mp.workdps(TR.DPS):
        assert all(v == mpf(sig2) for v in ref.pivots)
        want = n * log(mpf(sig2))
        assert (ref.logdet_hi, ref.logdet_lo) == (float(want), float(want - float(want)))
        for r in range(R):
            q = sum((mpf(float(v)) ** 2 for v in W[r]), mpf(0)) / mpf(sig2)
            assert (ref.quad_hi[r], ref.quad_lo[r]) == (float(q), float(q - float(q)))
            for k in range(n):
                x = mpf(float(W[r, k])) / mpf(sig2)
                assert (ref.x_hi[r, k], ref.x_lo[r, k]) == (float(x), float(x - float(x)))
    # and the float64 yardstick: the pivots are sig2 itself, every solution one correctly rounded division
    assert np.all(ref.pivots_f64 == sig2) and np.array_equal(ref.x_f64, W / sig2)


# ------------------------------------------------------------------------------------------------ operands (CPU, seeded)
def _gram_tridiagonal(kind, n, ell_rel, p, odd):
    """Tridiagonal form of the parity block p of an SE / Matern Gram matrix of a time grid folded about its centre: the grid has
    2 n points (odd: 2 n - 1 for p = 0, 2 n + 1 for p = 1, the centre point belongs to the symmetric block), unit spacing, length
    scale ell_rel * n.  Divided by its largest entry, reduced with scipy.linalg.hessenberg."""
    from scipy.linalg import hessenberg
    if n == 0:
        return np.zeros(0), np.zeros(0)
    tau = np.arange(n) + ((0.0 if p == 0 else 1.0) if odd else 0.5)
    ell = ell_rel * max(n, 2)
    k = (lambda r: np.exp(-0.5 * (r / ell) ** 2)) if kind == "se" else (lambda r: np.exp(-np.abs(r) / ell))
    G = k(tau[:, None] - tau[None, :]) + (1.0 if p == 0 else -1.0) * k(tau[:, None] + tau[None, :])
    G = G / np.max(np.abs(G))
    H = hessenberg(G) if n > 2 else G
    return np.ascontiguousarray(np.diag(H)), np.ascontiguousarray(np.diag(H, -1))


def _toeplitz(n, p, odd):
    return np.full(n, 2.0) / 4.0, np.full(max(n - 1, 0), -1.0) / 4.0          # (2, -1) over its norm bound 4


def _graded(n, p, odd):
    d = 10.0 ** (-16.0 * np.arange(n) / max(n - 1, 1))
    return d, 0.5 * np.sqrt(d[:-1] * d[1:]) if n > 1 else np.zeros(0)


def _split_blocks(n, p, odd):
    rng = np.random.RandomState(7 + n + p)
    d, e = _random_spd_tridiagonal(n, rng)
    for k in range(n - 1):
        if k % 7 == 3 or k in (30, 31, 32, 62, 63, 64, n - 2):           # exact zeros: decoupled blocks, some of order 1
            e[k] = 0.0
    s = np.max(d) if n else 1.0
    return d / s, e / s


FAMILIES = {
    "se_short": functools.partial(_gram_tridiagonal, "se", ell_rel=0.002),        # nearly diagonal
    "se_mid": functools.partial(_gram_tridiagonal, "se", ell_rel=0.05),
    "se_long": functools.partial(_gram_tridiagonal, "se", ell_rel=20.0),          # nearly rank one
    "mat_short": functools.partial(_gram_tridiagonal, "matern", ell_rel=0.002),
    "mat_mid": functools.partial(_gram_tridiagonal, "matern", ell_rel=0.05),
    "mat_long": functools.partial(_gram_tridiagonal, "matern", ell_rel=20.0),
    "toeplitz": _toeplitz,
    "graded": _graded,
    "split": _split_blocks,
}


def _family(name, n, p, odd):
    f = FAMILIES[name]
    return f(n=n, p=p, odd=odd) if isinstance(f, functools.partial) else f(n, p, odd)


def _spectrum(nx, top):
    """A decaying positive spectrum under `top`, an exact zero, and -1e-18 top (what an eigensolver returns for a rank-deficient Ks);
    the last two from nx = 3 on."""
    if nx == 1:
        return np.array([top])
    if nx == 2:
        return np.array([top, 1e-3 * top])
    es = np.empty(nx)
    es[:nx - 2] = top * 10.0 ** (-6.0 * np.arange(nx - 2) / max(nx - 3, 1))
    es[nx - 2] = 0.0
    es[nx - 1] = -1e-18 * top
    return np.roll(es, nx // 2)               # (fold order is not sorted)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(np0, np1, fam0, fam1, nx, R, cond, sig2):
    """Operands and their reference, once per process: every test of the case reads them, none writes."""
    c = Case()
    c.np, c.nx, c.R, c.cond, c.sig2 = (np0, np1), nx, R, cond, sig2
    c.c0 = (PAD, PAD + np0 + PAD)
    c.nt = c.c0[1] + np1 + PAD
    odd = np0 == np1 + 1
    c.blocks = []
    for p, (n, fam) in enumerate(((np0, fam0), (np1, fam1))):
        d, e = _family(fam, n, p, odd)
        c.blocks.append((d, e, M_BLOCK[p], c.c0[p]))
    c.es = _spectrum(nx, cond * sig2 / M_BLOCK[0])           # lam m / sig2 reaches `cond` in block 0
    rng = np.random.RandomState((np0 * 7919 + np1 * 31 + nx * 3 + R) % (2 ** 31))
    c.W = np.full((nx, R, c.nt), np.nan)
    for p in range(2):
        c.W[:, :, c.c0[p]:c.c0[p] + c.np[p]] = rng.standard_normal((nx, R, c.np[p]))
    c.ref = [[TR.reference_item(c.es[x], M_BLOCK[p], c.blocks[p][0], c.blocks[p][1], sig2, c.W[x, :, c.c0[p]:c.c0[p] + c.np[p]])
              if c.np[p] else None for p in range(2)] for x in range(nx)]
    c.W.setflags(write=False)
    return c


def _operands(c, R):
    return np.ascontiguousarray(c.W[:, :R, :]), c.es, c.blocks, c.sig2


# shapes: (np0, np1), nx, trial counts of the log-likelihood kernels, trial counts of the solve (empty: the solve refuses the
# shape), the two blocks' families.  One sweep at a moderate condition; nx = 100 (2 nx items > the solve's grid of 192) rides on
# the two smallest shapes, 130 trials (three passes of 64) on a middle one.
SHAPES = [
    ((1, 0), 3, (1, 33), (16, 33), ("se_mid", "se_mid")),
    ((5, 0), 100, (2,), (16,), ("mat_mid", "se_mid")),
    ((1, 1), 100, (2, 65), (32, 65), ("toeplitz", "graded")),
    ((32, 31), 3, (64,), (64,), ("se_mid", "mat_mid")),
    ((33, 32), 3, (1, 64), (16, 64), ("se_long", "mat_short")),
    ((64, 63), 3, (65,), (33, 65), ("graded", "toeplitz")),
    ((65, 64), 3, (33,), (70,), ("split", "se_short")),
    ((125, 125), 1, (130,), (64, 70), ("mat_long", "split")),
    ((250, 250), 3, (2, 33), (32, 33), ("se_mid", "mat_mid")),
    ((256, 255), 1, (64,), (65,), ("toeplitz", "se_long")),
    ((257, 256), 1, (2,), (), ("se_mid", "split")),
    ((300, 299), 1, (33,), (), ("mat_mid", "graded")),
]
SHAPE_COND, SHAPE_SIG2 = 1e4, 1e-4
CONDS = [1.0, 1e4, 1e8, 1e12]
SIG2S = [1.0, 1e-4]
FAMILY_PAIRS = [("se_short", "mat_long"), ("se_mid", "mat_mid"), ("se_long", "mat_short"), ("toeplitz", "graded"), ("split", "toeplitz")]
# conditions: every family pair at every lam m / sig2; at 33 / 32 with both noise variances, at 250 / 250 with one of them per
# case in turn (each pair and each condition still meets both) and the two largest eigenvalues only: the 50-digit sweeps over
# 500 columns are what this file's time goes to
COND_CASES = [((33, 32), 4, 16, fp, cond, sig2) for fp in FAMILY_PAIRS for cond in CONDS for sig2 in SIG2S] + \
             [((250, 250), 2, 16, fp, cond, SIG2S[(i + j) % 2]) for i, fp in enumerate(FAMILY_PAIRS) for j, cond in enumerate(CONDS)]


def _shape_case(shape):
    (np0, np1), nx, r_ll, r_solve, fams = shape
    return _case(np0, np1, fams[0], fams[1], nx, max(r_ll + r_solve), SHAPE_COND, SHAPE_SIG2)


def _cond_case(cc):
    (np0, np1), nx, R, fams, cond, sig2 = cc
    return _case(np0, np1, fams[0], fams[1], nx, R, cond, sig2)


def _shape_id(shape):
    return "%dx%d-nx%d" % (shape[0][0], shape[0][1], shape[1])


def _cond_id(cc):
    return "%dx%d-%s+%s-cond%g-sig%g" % (cc[0][0], cc[0][1], cc[3][0], cc[3][1], cc[4], cc[5])


# ------------------------------------------------------------------------------------------------ the gate
WORST = {}                   # (kernel, lam m / sig2) -> worst ratio of the kernel's error to the yardstick's seen in this process


def _gate(kernel, what, c, x, p, err_k, err_y, scale, failures):
    n = c.np[p]
    floor = 8.0 * n * U * scale
    err_k, err_y = np.atleast_1d(err_k), np.atleast_1d(err_y)
    assert np.all(np.isfinite(err_k)), "%s %s of item (%d, %d) is not finite" % (kernel, what, x, p)
    above = err_k > floor
    if np.any(above):
        with np.errstate(divide="ignore"):
            ratio = float(np.max(np.where(err_y[above] > 0, err_k[above] / err_y[above], np.inf)))
        key = (kernel, c.cond)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
    bad = err_k > MARGIN * err_y + floor
    if np.any(bad):
        i = int(np.argmax(err_k - MARGIN * err_y))
        failures.append("%s %s, item (x'=%d, p=%d) lam=%.3g np=%d: error %.3e against the yardstick's %.3e (floor %.1e)"
                        % (kernel, what, x, p, c.es[x], n, err_k[i], err_y[i], floor))


def _report(kernels, c):
    for k in kernels:
        print("[tridiag] %-14s lam*m/sig2=%-6g sig2=%-6g np=%s: worst error ratio to the sequential float64 recurrence so far %.3g"
              % (k, c.cond, c.sig2, c.np, WORST.get((k, c.cond), 0.0)))


def _assert_valid(c):
    for x in range(c.nx):
        for p in range(2):
            if c.ref[x][p] is not None:
                assert c.ref[x][p].positive, "not a valid input: item (%d, %d) has a non-positive exact pivot" % (x, p)


def _check_loglik(ctx, c, R, variants):
    W, es, blocks, sig2 = _operands(c, R)
    out = {}
    for v in variants:
        quad, logdet, sums = ctx.debug_ll_tridiag(W, es, blocks, sig2, variant=v)
        out[v] = (quad, logdet, sums)
        kernel = {0: "ll_default", 1: "ll_serial", 2: "ll_scan"}[v]
        assert np.all(np.isfinite(quad)) and np.all(np.isfinite(logdet)) and np.all(np.isfinite(sums)), "%s read a NaN column" % kernel
        failures = []
        for x in range(c.nx):
            for p in range(2):
                ref = c.ref[x][p]
                if ref is None:
                    assert quad[x, p] == 0.0 and logdet[x, p] == 0.0, "an item of an empty block must report 0"
                    continue
                _gate(kernel, "log-determinant", c, x, p, ref.logdet_err(logdet[x, p]), ref.logdet_err(ref.logdet_f64),
                      ref.logdet_scale, failures)
                _gate(kernel, "quadratic form", c, x, p, ref.quad_err(quad[x, p], R), ref.quad_err(ref.quad_f64_sum(R), R),
                      ref.quad_sum(R), failures)
        for part, total in ((quad, sums[0]), (logdet, sums[1])):
            flat = [float(v) for v in part.reshape(-1)]
            assert abs(total - math.fsum(flat)) <= 4.0 * np.spacing(math.fsum(abs(v) for v in flat)), \
                "%s: the reduced sum %r is not the sum of the partials %r" % (kernel, total, math.fsum(flat))
        assert not failures, "\n".join(failures)
    if 0 in out:                                           # the launcher's own choice is one of the two kernels, bit for bit
        same = [all(np.array_equal(a, b) for a, b in zip(out[0], out[v])) for v in variants if v != 0]
        assert (same[0] if max(c.np) > 256 else any(same)), "variant 0 reproduces neither kernel"
    return out


def _check_solve(ctx, c, R):
    W, es, blocks, sig2 = _operands(c, R)
    B = {P: ctx.debug_tridiag_solve(W, es, blocks, sig2, trials_per_pass=P) for P in (32, 64)}
    assert np.array_equal(B[32].view(np.uint64), B[64].view(np.uint64)), "32 and 64 trials per pass differ in their bits"
    X = B[32]
    inside = np.zeros(c.nt, dtype=bool)
    for p in range(2):
        inside[c.c0[p]:c.c0[p] + c.np[p]] = True
    assert np.array_equal(X[:, :, ~inside].view(np.uint64), W[:, :, ~inside].view(np.uint64)), "the solve wrote outside the blocks"
    assert np.all(np.isfinite(X[:, :, inside])), "the solve read a NaN column into a result"
    failures = []
    for x in range(c.nx):
        for p in range(2):
            ref = c.ref[x][p]
            if ref is None:
                continue
            Xi = X[x, :, c.c0[p]:c.c0[p] + c.np[p]]
            _gate("tridiag_solve", "solution", c, x, p, ref.x_err(Xi), ref.x_err(ref.x_f64[:R]), 1.0, failures)
    assert not failures, "\n".join(failures[:20])
    auto = ctx.debug_tridiag_solve(W, es, blocks, sig2)
    assert np.array_equal(auto.view(np.uint64), X.view(np.uint64)), "the launcher's own choice of the pass differs in its bits"


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    from gpcsd_amd import _hip
    return _hip.default_context()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_loglik_kernels_over_shapes(ctx, shape):
    c = _shape_case(shape)
    _assert_valid(c)
    variants = (0, 1, 2) if max(c.np) <= 256 else (0, 1)
    for R in shape[2]:
        _check_loglik(ctx, c, R, variants)
    _report(["ll_serial", "ll_scan"], c)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3]], ids=_shape_id)
def test_solve_kernel_over_shapes(ctx, shape):
    c = _shape_case(shape)
    _assert_valid(c)
    for R in shape[3]:
        _check_solve(ctx, c, R)
    _report(["tridiag_solve"], c)


@pytest.mark.gpu
@pytest.mark.parametrize("cc", COND_CASES, ids=_cond_id)
def test_loglik_kernels_over_conditions(ctx, cc):
    c = _cond_case(cc)
    _assert_valid(c)
    _check_loglik(ctx, c, 1, (1, 2))
    _check_loglik(ctx, c, c.R, (0, 1, 2))
    _report(["ll_serial", "ll_scan"], c)


@pytest.mark.gpu
@pytest.mark.parametrize("cc", COND_CASES, ids=_cond_id)
def test_solve_kernel_over_conditions(ctx, cc):
    c = _cond_case(cc)
    _assert_valid(c)
    _check_solve(ctx, c, c.R)
    _report(["tridiag_solve"], c)


@pytest.mark.gpu
def test_refusals(ctx):
    c = _shape_case(SHAPES[0])
    W, es, blocks, sig2 = _operands(c, 16)
    with pytest.raises(ValueError):                                    # rc -3: fewer than 16 trials
        ctx.debug_tridiag_solve(np.ascontiguousarray(W[:, :15]), es, blocks, sig2)
    n = 257
    wide = [(np.full(n, 0.5), np.full(n - 1, 0.1), M_BLOCK[0], 0), (np.zeros(0), np.zeros(0), M_BLOCK[1], n)]
    Ww = np.random.RandomState(0).standard_normal((1, 16, n))
    with pytest.raises(ValueError):                                    # rc -3: a block of 257 columns does not fit the solve
        ctx.debug_tridiag_solve(Ww, np.ones(1), wide, 0.1)
    with pytest.raises(ValueError):                                    # rc -3: nor the scan
        ctx.debug_ll_tridiag(Ww, np.ones(1), wide, 0.1, variant=2)
    quad, logdet, sums = ctx.debug_ll_tridiag(Ww, np.ones(1), wide, 0.1, variant=1)      # the context is usable afterwards
    assert np.all(np.isfinite(quad)) and quad[0, 1] == 0.0 and logdet[0, 1] == 0.0
