"""The analytic gradient's contraction kernels on their own (grad.hip: k_temporal_grad, k_frob_inner, k_kgl_grad, k_frob_pair,
k_fwdR_grad, k_D_sums, k_batch_reduce, k_siglist_eigvec_term, k_rowgroup_sumsq, k_per_trial_quad, through gpcsd_debug_grad_op,
which puts nothing between the caller and the launchers) against long-double references (grad_ref.py), at the sizes where each
kernel changes path -- 65 536 elements for the 256 x 256-thread grid-stride loops, 131 072 for kgl_grad's 512 blocks, 32 columns
and 8 row groups in d_colsums, nb = 32 for batch_reduce's eight lanes per element, 256 terms in the per-row and per-trial sums,
up to all 8 slots of the unrolled temporal loop -- and over the hyper-parameters at the edges of the optimiser's box.

The gate.  A kernel's measure -- |got - ref| / max(sum of the magnitudes of the terms, 2^-960) -- must be at most MARGIN x max(the
yardstick's measure, u), u = 2^-53; the yardstick is the same formula written plainly in float64 numpy on the same operands, never a
kernel.  MARGIN = 100 is what this project gives a float64 kernel over an unhurried float64 implementation (test_chol_kernels.py,
test_tridiag_kernels.py).  From above: a dropped tail element, a mirrored index, g / ngl2 for g % ngl2, ell^2 for ell^3, SE for
Matern, a set reading its neighbour's partials stand at 1e-8 and far more (test_measure_reports_planted_faults, on the CPU).  From
below: the order of summation and fused multiply-adds are factors of order one; the input-dependent part (exp's argument rounding,
the cancellation of sqrt(q) - q / sqrt(q + 1) at R = 1) is in the yardstick as well.

Operand families (grad_ref.weights): normal; spike (1e-3 x normal, 1.0 at the last element and at the last row's first element);
onehot (one term: the measure is that term's own relative error), at the last element, at the last row's first element, on the
diagonal and at the first element of the second grid-stride pass.  One-hot terms run under the hyper-parameter sets that keep the
term above 2^-900; the short length scales (every off-diagonal kernel value underflows) run with the dense families.

Every operation is run twice on the same operands and must return the same bits; the table forms must return the bits of the
plain calls, set by set.

Measured on the MI355X, worst ratio of a kernel's measure to max(yardstick's, u) per operation and family over all the cases
below (onehot: every placement; D_sums has its own operands, a twelve-decade spectrum, with a, b, the sum and the row sums
each against its own den):

                         normal   spike   onehot   spectrum
  temporal_grad            1.0     2.8      1.2       -
  frob_inner               0.8     1.0      0         -
  kgl_grad                 0.8     2.0      1.0       -
  frob_pair                0.9     3.0      0         -
  fwdR_grad                1.0     1.0      2.0       -
  D_sums                    -       -        -       2.5
  batch_reduce             1.0     1.5       -        -
  siglist_eigvec_term      1.0      -        -        -
  rowgroup_sumsq           1.6     2.8      0         -
  per_trial_quad           1.5     2.0      0.4       -

No kernel failed the gate, none needed a fix or an xfail; every table form returned the bits of its plain calls and every
operation the same bits twice.  What the kernels lose is what the formulas lose, and the yardstick loses it with them:
  - exp's argument: a one-hot temporal term at distance 254 .. 299 stands at 11 .. 36 u in the kernel and in the yardstick alike.
  - the 1D radius derivative sqrt(q) - q / sqrt(q + 1), q = (r / R)^2, cancels: one term at r = 2300 stands at 900 .. 3100 u at the
    box's lower bound R = 50 and at 0.7e7 .. 2e7 u (2e-9) at R = 1 -- kernel and yardstick to the same digits (ratio 1.0); the dense
    sums stand at 1 .. 42 u at R = 50 and 800 .. 16000 u at R = 1.  The equal form sqrt(q) / (sqrt(q + 1) (sqrt(q + 1) + sqrt(q)))
    has no cancellation; the kernel keeps the form of the forward model it differentiates, and the gate allows it.
"""
import functools

import numpy as np
import pytest

import grad_ref as GR

MARGIN = 100.0
U = GR.U
LD = GR.LD
SE, MAT = GR.KIND_SE, GR.KIND_MATERN
S_OUT = 64                  # distance of the sets' outputs, as in a gradient evaluation (GradRes::NG)
WRAP, WRAP_KGL = 65536, 131072

# temporal hyper-parameter sets: (kinds, ell, sigma2)
HP_T = {
    "usual": ((SE, MAT), (20.0, 5.0), (0.5, 0.7)),
    "short": ((SE, MAT), (1e-2, 5e-4), (0.5, 0.7)),              # every off-diagonal kernel value underflows to zero
    "long": ((MAT, SE), (1e6, 1e6), (0.7, 0.5)),
    "mixed": ((SE, MAT, SE), (0.3, 300.0, 3e4), (1e-6, 1.0, 1e4)),
    "zero_s2": ((MAT,), (5.0,), (0.0,)),                         # the Matern lower bound of the optimiser's box
    "se_only": ((SE,), (20.0,), (0.5,)),
    "eight": ((SE, MAT, SE, MAT, MAT, SE, SE, MAT), (20.0, 2.0, 60.0, 5.0, 40.0, 150.0, 400.0, 1000.0),
              (0.5, 0.7, 1e-3, 2.0, 0.0, 30.0, 1.0, 0.1)),
}
HP_T_ONEHOT = ("usual", "long", "zero_s2", "se_only", "eight")   # a term at distance nt - 1 <= 299 stays above 2^-900
T_SIZES = [1, 2, 37, 255, 256, 257, 300]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _times(nt, jitter):
    t = np.arange(nt, dtype=np.float64)
    if jitter:
        t = t + 0.37 * np.random.RandomState(nt).uniform(size=nt)
    return t


def _hot_positions(rows, cols, wrap=WRAP):
    """One-hot places of a rows x cols operand: name -> flat index."""
    n = rows * cols
    pos = {"onehot_last": n - 1, "onehot_corner": (rows - 1) * cols, "onehot_diag": (min(rows, cols) // 2) * (cols + 1)}
    if n > wrap:
        pos["onehot_wrap"] = wrap
    return pos


def _families(rows, cols, wrap=WRAP, seed=0):
    """Yields (family name, weights (rows, cols)) for the dense and the one-hot families."""
    yield "normal", GR.weights("normal", (rows, cols), seed)
    yield "spike", GR.weights("spike", (rows, cols), seed)
    for name, hot in _hot_positions(rows, cols, wrap).items():
        yield name, GR.weights("onehot", (rows, cols), seed, hot)


# ------------------------------------------------------------------------------------------------ the reference itself (no GPU)
def _yard_ok(op, label, yard, ref, den, bound=100.0):
    m = GR.measure(yard, ref, den)
    print("[grad-ref] %-20s %-40s yardstick %9.3g u" % (op, label, m / U))
    assert m <= bound * U, "%s %s: the yardstick stands at %.1f u" % (op, label, m / U)
    return m


def test_yardsticks_stay_under_100u():
    rs = np.random.RandomState(0)
    nt = 60
    for fam, Gt in _families(nt, nt):
        for name in (HP_T if fam in ("normal", "spike") else HP_T_ONEHOT):
            hp = HP_T[name]
            _yard_ok("temporal_grad", "%s %s" % (fam, name), GR.temporal_grad_f64(Gt, _times(nt, True), *hp),
                     *GR.temporal_grad_ld(Gt, _times(nt, True), *hp))
    # the input-dependent part: one term at distance 512 under an SE length scale of 20, exp(-327.68)
    nt = 513
    Gt = GR.weights("onehot", (nt, nt), 0, (nt - 1) * nt)
    m = _yard_ok("temporal_grad", "onehot distance 512, ell 20", GR.temporal_grad_f64(Gt, _times(nt, False), (SE,), (20.0,), (0.5,)),
                 *GR.temporal_grad_ld(Gt, _times(nt, False), (SE,), (20.0,), (0.5,)))
    assert m > 4 * U                       # (about |x| u / 2: it must be the yardstick that carries it)
    G = rs.standard_normal(500)
    dK = rs.standard_normal((3, 500))
    _yard_ok("frob_inner", "normal", GR.frob_inner_f64(G, dK), *GR.frob_inner_ld(G, dK))
    _yard_ok("frob_pair", "normal", GR.frob_pair_f64(G, dK[0], dK[1]), *GR.frob_pair_ld(G, dK[0], dK[1]))
    gx1, gw1 = GR.gauss_legendre(12, 0.0, 2300.0)
    gx2, gw2 = GR.gauss_legendre(5, 0.0, 440.0)
    M1, M2 = rs.standard_normal((12, 12)), rs.standard_normal((60, 60))
    _yard_ok("kgl_grad", "1D", GR.kgl_grad_f64(M1, GR.se_gram_ld(gx1, 200.0), gx1, 200.0), *GR.kgl_grad_ld(M1, GR.se_gram_ld(gx1, 200.0), gx1, 200.0))
    K2 = GR.se_gram_ld(gx1, 200.0, gx2, 50.0)
    _yard_ok("kgl_grad", "2D", GR.kgl_grad_f64(M2, K2, gx1, 200.0, gx2, 50.0), *GR.kgl_grad_ld(M2, K2, gx1, 200.0, gx2, 50.0))
    x1 = np.linspace(0.0, 2300.0, 7)
    S1 = rs.standard_normal((7, 12))
    for R in (200.0, 50.0):
        _yard_ok("fwdR_grad", "1D R=%g" % R, GR.fwdR_grad_f64(S1, x1, gx1, gw1, R), *GR.fwdR_grad_ld(S1, x1, gx1, gw1, R))
    x2 = rs.uniform(0.0, 400.0, (7, 2))
    S2 = rs.standard_normal((7, 60))
    _yard_ok("fwdR_grad", "2D", GR.fwdR_grad_f64(S2, x2, gx1, gw1, 200.0, gx2, gw2, 80.0), *GR.fwdR_grad_ld(S2, x2, gx1, gw1, 200.0, gx2, gw2, 80.0))
    D, es, et = _D_operands(9, 40, 1e-8, 0)
    for name, y, (ref, den) in zip(("a", "b", "sum", "rows"), GR.D_sums_f64(D, es, et), GR.D_sums_ld(D, es, et)):
        _yard_ok("D_sums", name, y, ref, den)
    T = rs.standard_normal((40, 6, 6))
    dv = rs.standard_normal(6)
    _yard_ok("batch_reduce", "normal", GR.batch_reduce_f64(T, 6, 0.5, dv, -20.0), *GR.batch_reduce_ld(T, 6, 0.5, dv, -20.0))
    Ghs, Ssum, es, sig = _siglist_operands(12, 0)
    v, den, touched = GR.siglist_eigvec_term_ld(Ghs, Ssum, es, sig, 0.0)
    _yard_ok("siglist_eigvec_term", "nx=12", GR.siglist_eigvec_term_f64(Ghs, Ssum, es, sig, 0.0), v, den)
    assert not touched[3, 7] and not touched[7, 3] and touched.sum() == 12 * 11 - 2
    Bm = rs.standard_normal((3, 300))
    _yard_ok("rowgroup_sumsq", "normal", GR.rowgroup_sumsq_f64(Bm, 3), *GR.rowgroup_sumsq_ld(Bm, 3))
    al, Dq = rs.standard_normal((5, 3, 40)), rs.uniform(0.1, 2.0, (5, 40))
    _yard_ok("per_trial_quad", "normal", GR.per_trial_quad_f64(al, Dq, 5, 3, 40), *GR.per_trial_quad_ld(al, Dq, 5, 3, 40))


def test_measure_floor_and_non_finite():
    # a term that underflows in float64 and not in long double: distance 72 under an SE length scale of 0.7, exp(-5290)
    nt = 73
    Gt = GR.weights("onehot", (nt, nt), 0, (nt - 1) * nt)
    hp = ((SE,), (0.7,), (0.5,))
    ref, den = GR.temporal_grad_ld(Gt, _times(nt, False), *hp)
    y = GR.temporal_grad_f64(Gt, _times(nt, False), *hp)
    assert np.all(y == 0.0) and np.all(ref > 0) and np.all(den < GR.FLOOR)
    assert GR.measure(y, ref, den) < 1e-300
    assert GR.measure([np.nan, 0.0], ref, den) == float("inf") and GR.measure([0.0, np.inf], ref, den) == float("inf")
    assert GR.measure(1.0 + 2 * U, LD(1), LD(1)) == 2 * U
    with pytest.raises(ValueError):
        GR.measure(np.zeros(3), ref, den)


def test_measure_reports_planted_faults():
    """Each fault is planted in the yardstick's result (a term left out of its sum, an index exchanged in its formula), never in a
    kernel: the measure must stand above 1e-8 -- the gate is at most a few thousand u = 1e-13."""
    seen = {}

    def planted(name, bad, ref, den, good):
        m, m0 = GR.measure(bad, ref, den), GR.measure(good, ref, den)
        seen[name] = min(seen.get(name, np.inf), m)
        print("[grad-ref] planted %-44s measure %9.3g (%9.3g u)   unplanted %9.3g u" % (name, m, m / U, m0 / U))
        assert m > 1e-8 and m > 1e4 * MARGIN * max(m0, U), name

    def without(W, flat):
        W = np.array(W)
        W.reshape(-1)[flat] = 0.0
        return W

    usual = HP_T["usual"]
    # ---- the last element / the first element of the second grid-stride pass dropped
    nt = 257
    t = _times(nt, True)
    for fam in ("normal", "spike"):
        Gt = GR.weights(fam, (nt, nt))
        ref, den = GR.temporal_grad_ld(Gt, t, *usual)
        good = GR.temporal_grad_f64(Gt, t, *usual)
        planted("temporal_grad: last element dropped", GR.temporal_grad_f64(without(Gt, nt * nt - 1), t, *usual), ref, den, good)
        far = HP_T["long"]                 # (element 65536 is (255, 1): under the usual length scales its term is 1e-22 of the sum)
        ref, den = GR.temporal_grad_ld(Gt, t, *far)
        planted("temporal_grad: element 65536 dropped", GR.temporal_grad_f64(without(Gt, WRAP), t, *far), ref, den,
                GR.temporal_grad_f64(Gt, t, *far))
        n = WRAP + 1
        P, T1, T2 = (GR.weights(fam, (n,), s) for s in (0, 1, 2))
        ref, den = GR.frob_pair_ld(P, T1, T2)
        planted("frob_pair: last element dropped", GR.frob_pair_f64(without(P, n - 1), T1, T2), ref, den, GR.frob_pair_f64(P, T1, T2))
        dK = np.stack([T1, T2])
        ref, den = GR.frob_inner_ld(P, dK)
        planted("frob_inner: element 65536 dropped", GR.frob_inner_f64(without(P, WRAP), dK), ref, den, GR.frob_inner_f64(P, dK))
        Bm = GR.weights(fam, (3, 257))
        ref, den = GR.rowgroup_sumsq_ld(Bm, 3)
        planted("rowgroup_sumsq: last element dropped", GR.rowgroup_sumsq_f64(without(Bm, 3 * 257 - 1), 3), ref, den, GR.rowgroup_sumsq_f64(Bm, 3))
        al, Dq = GR.weights(fam, (5, 3, 60)), np.random.RandomState(1).uniform(0.1, 2.0, (5, 60))
        ref, den = GR.per_trial_quad_ld(al, Dq, 5, 3, 60)
        planted("per_trial_quad: last element dropped", GR.per_trial_quad_f64(without(al, al.size - 1), Dq, 5, 3, 60), ref, den,
                GR.per_trial_quad_f64(al, Dq, 5, 3, 60))
        G = 363
        gx, gw = GR.gauss_legendre(G, 0.0, 2300.0)
        M, Kgl = GR.weights(fam, (G, G)), GR.se_gram_ld(gx, 2000.0)
        ref, den = GR.kgl_grad_ld(M, Kgl, gx, 2000.0)
        good = GR.kgl_grad_f64(M, Kgl, gx, 2000.0)
        planted("kgl_grad: last row's first element dropped", GR.kgl_grad_f64(without(M, (G - 1) * G), Kgl, gx, 2000.0), ref, den, good)
        planted("kgl_grad: element 131072 dropped", GR.kgl_grad_f64(without(M, WRAP_KGL), Kgl, gx, 2000.0), ref, den, good)
        x = np.linspace(0.0, 2300.0, 257)
        gx, gw = GR.gauss_legendre(256, 0.0, 2300.0)
        S = GR.weights(fam, (257, 256))
        ref, den = GR.fwdR_grad_ld(S, x, gx, gw, 200.0)
        good = GR.fwdR_grad_f64(S, x, gx, gw, 200.0)
        planted("fwdR_grad: last row's first element dropped", GR.fwdR_grad_f64(without(S, 256 * 256), x, gx, gw, 200.0), ref, den, good)
        planted("fwdR_grad: element 65536 dropped", GR.fwdR_grad_f64(without(S, WRAP), x, gx, gw, 200.0), ref, den, good)
    for seed in (0, 1):
        D, es, et = _D_operands(9, 257, 0.05, seed)
        (ra, rb, rs1, rrow), (ya, yb, ys1, yrow) = GR.D_sums_ld(D, es, et), GR.D_sums_f64(D, es, et)
        if seed == 0:
            bad = ya.copy()
            bad[8] -= et[256] / D[8, 256]
            planted("D_sums: a's last term dropped", bad, ra[0], ra[1], ya)
        else:
            bad = yb.copy()
            bad[256] -= es[8] / D[8, 256]
            planted("D_sums: b's last term dropped", bad, rb[0], rb[1], yb)
        planted("D_sums: sum's last term dropped", ys1 - 1.0 / D[8, 256], rs1[0], rs1[1], ys1)
    # ---- i and j exchanged in a non-symmetric operand
    Ghs, Ssum, es, sig = _siglist_operands(17, 0)
    ref, den, _ = GR.siglist_eigvec_term_ld(Ghs, Ssum, es, sig, 0.0)
    planted("siglist_eigvec_term: Ssum[y][x] for Ssum[x][y]", GR.siglist_eigvec_term_f64(Ghs, Ssum.T, es, sig, 0.0), ref, den,
            GR.siglist_eigvec_term_f64(Ghs, Ssum, es, sig, 0.0))
    x = np.linspace(0.0, 2300.0, 60)
    gx, gw = GR.gauss_legendre(60, 0.0, 2300.0)
    S = GR.weights("normal", (60, 60))
    ref, den = GR.fwdR_grad_ld(S, x, gx, gw, 200.0)
    planted("fwdR_grad: S[g][i] for S[i][g]", GR.fwdR_grad_f64(S.T, x, gx, gw, 200.0), ref, den, GR.fwdR_grad_f64(S, x, gx, gw, 200.0))
    # ---- g / ngl2 and g % ngl2 exchanged with ngl1 != ngl2: the tensor grid flattened the other way round
    g1, _ = GR.gauss_legendre(3, 0.0, 200.0)
    g2, _ = GR.gauss_legendre(5, 0.0, 440.0)
    M, Kgl = GR.weights("normal", (15, 15)), GR.se_gram_ld(g1, 200.0, g2, 50.0)
    ref, den = GR.kgl_grad_ld(M, Kgl, g1, 200.0, g2, 50.0)
    g = np.arange(15)
    p1, p2 = g1[g % 3], g2[g // 3]
    d1, d2 = p1[:, None] - p1[None, :], p2[:, None] - p2[None, :]
    bad = np.array([np.sum(M * Kgl * d1 * d1 / 200.0 ** 3), np.sum(M * Kgl * d2 * d2 / 50.0 ** 3)])
    planted("kgl_grad: g / ngl2 and g % ngl2 exchanged", bad, ref, den, GR.kgl_grad_f64(M, Kgl, g1, 200.0, g2, 50.0))
    # ---- ell^2 for ell^3, SE taken for Matern
    nt = 60
    t, Gt = _times(nt, True), GR.weights("normal", (nt, nt))
    ref, den = GR.temporal_grad_ld(Gt, t, *usual)
    good = GR.temporal_grad_f64(Gt, t, *usual)
    bad = good.copy()
    bad[0] *= usual[1][0]
    planted("temporal_grad: ell^2 for ell^3", bad, ref, den, good)
    planted("temporal_grad: SE taken for Matern", GR.temporal_grad_f64(Gt, t, (SE, SE), usual[1], usual[2]), ref, den, good)
    gx, _ = GR.gauss_legendre(12, 0.0, 2300.0)
    M, Kgl = GR.weights("normal", (12, 12)), GR.se_gram_ld(gx, 200.0)
    ref, den = GR.kgl_grad_ld(M, Kgl, gx, 200.0)
    good = GR.kgl_grad_f64(M, Kgl, gx, 200.0)
    planted("kgl_grad: ell^2 for ell^3", good * 200.0, ref, den, good)
    # ---- set 1 of a batch given set 0's result
    Gt1 = GR.weights("normal", (nt, nt), 1)
    ref1, den1 = GR.temporal_grad_ld(Gt1, t, *HP_T["long"])
    planted("temporal_grad: set 1 given set 0's result", GR.temporal_grad_f64(Gt, t, *usual), ref1, den1,
            GR.temporal_grad_f64(Gt1, t, *HP_T["long"]))
    P0, P1 = GR.weights("normal", (300,), 0), GR.weights("normal", (300,), 1)
    ref1, den1 = GR.frob_pair_ld(P1, P0, P1)
    planted("frob_pair: set 1 given set 0's result", GR.frob_pair_f64(P0, P1, P0), ref1, den1, GR.frob_pair_f64(P1, P0, P1))
    # ---- the mirrored read of batch_reduce taken from the upper triangle
    T = np.random.RandomState(2).standard_normal((33, 5, 5))
    dv = np.random.RandomState(3).standard_normal(5)
    ref, den = GR.batch_reduce_ld(T, 5, 0.5, dv, -16.5)
    planted("batch_reduce: mirrored read from the upper triangle", GR.batch_reduce_f64(np.transpose(T, (0, 2, 1)), 5, 0.5, dv, -16.5),
            ref, den, GR.batch_reduce_f64(T, 5, 0.5, dv, -16.5))
    assert len(seen) >= 20


def test_families_are_reproducible_and_placed():
    W = GR.weights("spike", (7, 9))
    assert W[6, 8] == 1.0 and W[6, 0] == 1.0 and np.max(np.abs(W[:6])) < 0.01 and not W.flags.writeable
    assert _same_bits(W, GR.weights("spike", (7, 9))) and not _same_bits(W, GR.weights("spike", (7, 9), 1))
    H = GR.weights("onehot", (300, 300), 0, WRAP)
    assert H.sum() == 1.0 and H[WRAP // 300, WRAP % 300] == 1.0
    N = GR.weights("normal", (40, 40))
    assert not np.array_equal(N, N.T)
    x, w = GR.gauss_legendre(60, 0.0, 2300.0)
    assert abs(np.sum(w) - 2300.0) < 1e-9 and np.all(np.diff(x) > 0)


# ------------------------------------------------------------------------------------------------ operands shared with the GPU tests
def _D_operands(nx, nt, sig2, seed):
    """D = es (x) et + sig2 with spectra spanning twelve decades, in random order but for the last entries: an even seed ends es with
    its smallest and et with its largest value (the last term of a's last sum and of the sum of 1/D are among the largest), an odd
    seed the other way round (the same for b) -- a lost tail then shows at full size, as with the spike family."""
    rs = np.random.RandomState(97 * nx + nt + 1009 * seed)
    es = np.sort(10.0 ** np.linspace(-9.0, 3.0, nx)) if nx > 1 else np.array([1.0 + seed])
    et = np.sort(10.0 ** np.linspace(-8.0, 4.0, nt)) if nt > 1 else np.array([0.5 + seed])
    if seed % 2:
        es, et = np.append(rs.permutation(es[:-1]), es[-1]), np.append(rs.permutation(et[1:]), et[0])
    else:
        es, et = np.append(rs.permutation(es[1:]), es[0]), np.append(rs.permutation(et[:-1]), et[-1])
    return es[:, None] * et[None, :] + sig2, es, et


def _siglist_operands(nx, seed):
    """Ghs, Ssum (non-symmetric), es with one exactly repeated eigenvalue (3 and 7; 0 and 1 at nx = 2) and, from nx = 12 on, one
    pair 1e-13 apart (4 and 9), sig."""
    rs = np.random.RandomState(nx + 1000 * seed)
    es = np.sort(rs.uniform(0.1, 10.0, nx))[::-1].copy()
    if nx >= 12:
        es[7] = es[3]
        es[9] = es[4] + 1e-13
    else:
        es[1] = es[0]
    return rs.standard_normal((nx, nx)), rs.standard_normal((nx, nx)), es, rs.uniform(0.01, 0.5, nx)


# ------------------------------------------------------------------------------------------------ the gate
WORST = {}                   # (operation, family) -> worst ratio of the kernel's measure to max(yardstick's, u) in this process


def _gate(op, fam, label, got, yard, ref, den):
    m_kernel, m_yard = GR.measure(got, ref, den), GR.measure(yard, ref, den)
    ratio = m_kernel / max(m_yard, U)
    key = (op, fam.split("_")[0])
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("[grad] %-20s %-14s %-44s kernel %9.3g u   yardstick %9.3g u   ratio %8.3g" % (op, fam, label, m_kernel / U, m_yard / U, ratio))
    assert m_kernel <= MARGIN * max(m_yard, U), \
        "%s, %s %s: %.3e (%.1f u) against the yardstick's %.3e (%.1f u): ratio %.1f > %g" \
        % (op, fam, label, m_kernel, m_kernel / U, m_yard, m_yard / U, ratio, MARGIN)


# ------------------------------------------------------------------------------------------------ GPU tests
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from gpcsd_amd import _hip
    yield _hip.default_context()
    for (op, fam), r in sorted(WORST.items()):
        print("[grad] worst ratio  %-20s %-8s %.3g" % (op, fam, r))


def _twice(call):
    """The result of call(), which must come out bit for bit the same a second time (the kernels sum in a fixed order)."""
    a, b = call(), call()
    for x, y in zip(a, b):
        assert _same_bits(x, y), "two runs on the same operands differ"
    return a


def _hp(temporal=None, R=None, eps=None, ell_s=None):
    """B hyper-parameter sets as one block; temporal: per set (kinds, ell, sigma2), the number of components may differ."""
    from gpcsd_amd import _hip
    B = len(temporal) if temporal is not None else len(R) if R is not None else len(ell_s)
    temporal = temporal if temporal is not None else [((SE,), (1.0,), (1.0,))] * B
    C = max(len(s[0]) for s in temporal)
    hb = _hip.HParamsBatch(np.ones(B) if R is None else np.asarray(R, dtype=np.float64), 0.0 if eps is None else np.asarray(eps, dtype=np.float64),
                           np.ones((B, 2)) if ell_s is None else np.asarray(ell_s, dtype=np.float64).reshape(B, 2), [SE] * C,
                           np.ones((B, C)), np.ones((B, C)), np.full(B, 0.1), 0.0)
    for b, (kinds, ell, s2) in enumerate(temporal):
        c = len(kinds)
        hb.rec["n_temporal"][b] = c
        hb.rec["kind"][b] = 0
        hb.rec["ell_t"][b] = 0.0
        hb.rec["sigma2_t"][b] = 0.0
        hb.rec["kind"][b, :c] = kinds
        hb.rec["ell_t"][b, :c] = ell
        hb.rec["sigma2_t"][b, :c] = s2
    return hb


# ---- temporal_grad
def _k_temporal(ctx, Gt, t, hp):
    nt = t.size
    return _twice(lambda: ctx.debug_grad_op("temporal_grad", [Gt, t], [2 * len(hp[0])], n=[nt], l=[0, 0, 0, 2 * len(hp[0])], hp=_hp([hp])))[0]


def _k_temporal_table(ctx, Gts, t, sets):
    nt, B = t.size, len(sets)
    out = _twice(lambda: ctx.debug_grad_op("temporal_grad", [np.stack(Gts), t], [B * S_OUT], n=[nt], l=[0, 0, 0, S_OUT], B=B, hp=_hp(sets),
                                            table=True))[0]
    return out.reshape(B, S_OUT)


def _temporal_families(nt):
    if nt == 1:
        yield "normal", GR.weights("normal", (1, 1))
        yield "onehot_last", GR.weights("onehot", (1, 1))
    else:
        yield from _families(nt, nt)


@gpu
@pytest.mark.parametrize("nt", T_SIZES)
def test_temporal_grad(ctx, nt):
    for fam, Gt in _temporal_families(nt):
        t = _times(nt, fam == "normal")
        for name in (HP_T if fam in ("normal", "spike") else HP_T_ONEHOT):
            hp = HP_T[name]
            got = _k_temporal(ctx, Gt, t, hp)
            _gate("temporal_grad", fam, "nt=%d %s" % (nt, name), got, GR.temporal_grad_f64(Gt, t, *hp), *GR.temporal_grad_ld(Gt, t, *hp))
            if name == "zero_s2":
                assert got[0] == 0.0


@gpu
@pytest.mark.parametrize("names", [("mixed", "usual", "long"), ("eight", "zero_s2"), ("eight", "short", "se_only")], ids="-".join)
@pytest.mark.parametrize("nt", [37, 257, 300])
def test_temporal_grad_table_equals_plain_calls(ctx, nt, names):
    """B sets through the device table: each set's values are the bits of its own plain call, the slots of the components a set does
    not have are zero, and nothing else of the output is written."""
    sets = [HP_T[n] for n in names]
    for fam in ("normal", "spike"):
        Gts = [GR.weights(fam, (nt, nt), seed) for seed in range(len(sets))]
        t = _times(nt, True)
        out = _k_temporal_table(ctx, Gts, t, sets)
        C0 = len(sets[0][0])
        for b, (name, hp) in enumerate(zip(names, sets)):
            c2 = 2 * len(hp[0])
            assert _same_bits(out[b, :c2], _k_temporal(ctx, Gts[b], t, hp)), "set %d (%s) differs from its plain call" % (b, name)
            assert np.all(out[b, c2:2 * C0] == 0.0) and np.all(out[b, 2 * C0:] == 0.0)
            _gate("temporal_grad", fam, "nt=%d table %s[%d]" % (nt, "-".join(names), b), out[b, :c2], GR.temporal_grad_f64(Gts[b], t, *hp),
                  *GR.temporal_grad_ld(Gts[b], t, *hp))


# ---- frob_inner, frob_pair
def _flat_families(n, seed=0):
    yield "normal", GR.weights("normal", (n,), seed)
    if n > 1:
        yield "spike", GR.weights("spike", (n,), seed)
    yield "onehot_last", GR.weights("onehot", (n,), seed)
    if n > WRAP:
        yield "onehot_wrap", GR.weights("onehot", (n,), seed, WRAP)


@gpu
@pytest.mark.parametrize("nm", [1, 2, 16])
@pytest.mark.parametrize("n2", [1, 255, 65536, 65537])
def test_frob_inner(ctx, n2, nm):
    dK = GR.weights("normal", (nm, n2), 5)
    for fam, Gt in _flat_families(n2):
        got = _twice(lambda: ctx.debug_grad_op("frob_inner", [Gt, dK], [nm], n=[nm], l=[n2]))[0]
        _gate("frob_inner", fam, "n2=%d nm=%d" % (n2, nm), got, GR.frob_inner_f64(Gt, dK), *GR.frob_inner_ld(Gt, dK))


@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 65536, 65537, 100003])
def test_frob_pair(ctx, n, B):
    for fam in [f for f, _ in _flat_families(n)]:
        Ps = [dict(_flat_families(n, b))[fam] for b in range(B)]
        T1 = [GR.weights("normal", (n,), 10 + b) for b in range(B)]
        T2 = [GR.weights("spike", (n,), 20 + b) if n > 1 else GR.weights("normal", (n,), 20 + b) for b in range(B)]
        out = _twice(lambda: ctx.debug_grad_op("frob_pair", [np.stack(Ps), np.stack(T1), np.stack(T2)], [B * S_OUT], l=[n, 0, 0, S_OUT], B=B))[0]
        out = out.reshape(B, S_OUT)
        assert np.all(out[:, 2:] == 0.0)
        for b in range(B):
            _gate("frob_pair", fam, "n=%d set %d of %d" % (n, b, B), out[b, :2], GR.frob_pair_f64(Ps[b], T1[b], T2[b]), *GR.frob_pair_ld(Ps[b], T1[b], T2[b]))
            if B > 1:
                alone = ctx.debug_grad_op("frob_pair", [Ps[b], T1[b], T2[b]], [2], l=[n, 0, 0, 2])[0]
                assert _same_bits(alone, out[b, :2]), "set %d of %d differs from the same set alone" % (b, B)


# ---- kgl_grad
ELL_1D = {"usual": 200.0, "short": 1e-3, "long": 1e6}
ELL_2D = {"usual": (200.0, 50.0), "short": (1e-3, 1e-3), "long": (1e6, 2e6), "mixed": (3.0, 3000.0)}


@functools.lru_cache(maxsize=None)
def _nodes(n, b):
    x, w = GR.gauss_legendre(n, 0.0, b)
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


@functools.lru_cache(maxsize=None)
def _kgl(G1, ell1, G2=None, ell2=None):
    K = GR.se_gram_ld(_nodes(G1, 2300.0)[0], ell1) if G2 is None else GR.se_gram_ld(_nodes(G1, 200.0)[0], ell1, _nodes(G2, 440.0)[0], ell2)
    K.setflags(write=False)
    return K


def _k_kgl(ctx, M, Kgl, gx1, gx2, ell):
    G = Kgl.shape[0]
    if gx2 is None:
        return _twice(lambda: ctx.debug_grad_op("kgl_grad", [M, Kgl, gx1], [1], n=[G, 0], l=[0, 0, 0, 1], s=[ell, 0.0]))[0]
    return _twice(lambda: ctx.debug_grad_op("kgl_grad", [M, Kgl, gx1, gx2], [2], n=[G, gx2.size], l=[0, 0, 0, 2], s=list(ell)))[0]


@gpu
@pytest.mark.parametrize("G", [1, 7, 60, 362, 363])
def test_kgl_grad_1d(ctx, G):
    gx = _nodes(G, 2300.0)[0]
    fams = list(_families(G, G, WRAP_KGL)) if G > 1 else [("normal", GR.weights("normal", (1, 1)))]
    for fam, M in fams:
        for name, ell in ELL_1D.items():
            if fam.startswith("onehot") and name == "short":
                continue
            Kgl = _kgl(G, ell)
            got = _k_kgl(ctx, M, Kgl, gx, None, ell)
            _gate("kgl_grad", fam, "G=%d %s" % (G, name), got, GR.kgl_grad_f64(M, Kgl, gx, ell), *GR.kgl_grad_ld(M, Kgl, gx, ell))
            if fam in ("onehot_last", "onehot_diag") or (name == "short" and fam != "normal"):
                assert got[0] == 0.0                 # a diagonal entry has distance zero; a lone off-diagonal one a kernel value of zero


@gpu
@pytest.mark.parametrize("ngl", [(3, 5), (10, 24), (19, 20), (20, 19)], ids=lambda p: "%dx%d" % p)
def test_kgl_grad_2d(ctx, ngl):
    n1, n2 = ngl
    G = n1 * n2
    g1, g2 = _nodes(n1, 200.0)[0], _nodes(n2, 440.0)[0]
    for fam, M in _families(G, G, WRAP_KGL):
        for name, ell in ELL_2D.items():
            if fam.startswith("onehot") and name in ("short", "mixed"):
                continue
            Kgl = _kgl(n1, ell[0], n2, ell[1])
            got = _k_kgl(ctx, M, Kgl, g1, g2, ell)
            _gate("kgl_grad", fam, "%dx%d %s" % (n1, n2, name), got, GR.kgl_grad_f64(M, Kgl, g1, ell[0], g2, ell[1]),
                  *GR.kgl_grad_ld(M, Kgl, g1, ell[0], g2, ell[1]))


@gpu
@pytest.mark.parametrize("dim", [1, 2])
def test_kgl_grad_table_equals_plain_calls(ctx, dim):
    ells = [(200.0, 50.0), (3.0, 3000.0)]
    if dim == 1:
        G, g1, g2 = 363, _nodes(363, 2300.0)[0], None
        Ks = [_kgl(G, e[0]) for e in ells]
    else:
        G, g1, g2 = 380, _nodes(20, 200.0)[0], _nodes(19, 440.0)[0]
        Ks = [_kgl(20, e[0], 19, e[1]) for e in ells]
    nv = dim
    for fam in ("normal", "spike"):
        Ms = [GR.weights(fam, (G, G), b) for b in range(2)]
        ins = [np.stack(Ms), np.stack(Ks), g1] + ([g2] if dim == 2 else [])
        out = _twice(lambda: ctx.debug_grad_op("kgl_grad", ins, [2 * S_OUT], n=[G, 0 if dim == 1 else 19], l=[0, 0, 0, S_OUT], B=2,
                                                hp=_hp(ell_s=ells), table=True))[0].reshape(2, S_OUT)
        assert np.all(out[:, nv:] == 0.0)
        for b in range(2):
            plain = _k_kgl(ctx, Ms[b], Ks[b], g1, g2, ells[b][0] if dim == 1 else ells[b])
            assert _same_bits(out[b, :nv], plain), "set %d differs from its plain call" % b
            e2 = (g2, ells[b][1]) if dim == 2 else (None, None)
            _gate("kgl_grad", fam, "%dD table set %d" % (dim, b), out[b, :nv], GR.kgl_grad_f64(Ms[b], Ks[b], g1, ells[b][0], *e2),
                  *GR.kgl_grad_ld(Ms[b], Ks[b], g1, ells[b][0], *e2))


# ---- fwdR_grad
R_1D = (200.0, 50.0, 1.0, 1e6)                       # usual; the box's lower bound; q = (r / R)^2 up to 5e6; far field
R_EPS_2D = ((200.0, 80.0), (50.0, 0.0), (1.0, 16.0), (1e6, 80.0))


def _geometry_1d(nx, G):
    """Electrodes and nodes on [0, 2300]; electrode nx // 2 sits exactly on node G // 3 (r = 0)."""
    gx, gw = _nodes(G, 2300.0)
    x = np.linspace(0.0, 2300.0, nx) if nx > 1 else np.array([1150.0])
    x[nx // 2] = gx[G // 3]
    return x, gx, gw


def _geometry_2d(nx, n1, n2):
    """Electrodes on a grid over [0, 200] x [0, 440]; electrode nx // 2 sits exactly on node (n1 // 2, n2 // 3) (w = 0)."""
    (g1, w1), (g2, w2) = _nodes(n1, 200.0), _nodes(n2, 440.0)
    x = np.stack([np.repeat(np.linspace(20.0, 180.0, nx // 6), 6), np.tile(np.linspace(10.0, 430.0, 6), nx // 6)], axis=1)
    x[nx // 2] = (g1[n1 // 2], g2[n2 // 3])
    return np.ascontiguousarray(x), g1, w1, g2, w2


def _k_fwdR(ctx, S, x, gx1, gw1, R, gx2=None, gw2=None, eps=0.0):
    nx = S.shape[0]
    if gx2 is None:
        return _twice(lambda: ctx.debug_grad_op("fwdR_grad", [S, x, gx1, gw1], [1], n=[nx, gx1.size, 0], l=[0, 0, 0, 1], s=[R, eps]))[0]
    return _twice(lambda: ctx.debug_grad_op("fwdR_grad", [S, x, gx1, gw1, gx2, gw2], [1], n=[nx, gx1.size * gx2.size, gx2.size],
                                            l=[0, 0, 0, 1], s=[R, eps]))[0]


@gpu
@pytest.mark.parametrize("nx,G", [(1, 1), (24, 60), (17, 100), (256, 256), (257, 256)])
def test_fwdR_grad_1d(ctx, nx, G):
    x, gx, gw = _geometry_1d(nx, G)
    fams = dict(_families(nx, G)) if nx * G > 1 else {"normal": GR.weights("normal", (1, 1))}
    fams["onehot_r0"] = GR.weights("onehot", (nx, G), 0, (nx // 2) * G + G // 3)          # the node on an electrode
    for fam, S in fams.items():
        for R in R_1D:
            got = _k_fwdR(ctx, S, x, gx, gw, R)
            _gate("fwdR_grad", fam, "1D %dx%d R=%g" % (nx, G, R), got, GR.fwdR_grad_f64(S, x, gx, gw, R), *GR.fwdR_grad_ld(S, x, gx, gw, R))
            if fam == "onehot_r0":
                assert got[0] == 0.0


@gpu
@pytest.mark.parametrize("nx", [12, 48])
@pytest.mark.parametrize("ngl", [(3, 5), (10, 24)], ids=lambda p: "%dx%d" % p)
def test_fwdR_grad_2d(ctx, nx, ngl):
    n1, n2 = ngl
    x, g1, w1, g2, w2 = _geometry_2d(nx, n1, n2)
    fams = dict(_families(nx, n1 * n2))
    fams["onehot_w0"] = GR.weights("onehot", (nx, n1 * n2), 0, (nx // 2) * n1 * n2 + (n1 // 2) * n2 + n2 // 3)
    for fam, S in fams.items():
        for R, eps in R_EPS_2D:
            if fam == "onehot_w0" and eps == 0.0:
                continue
            got = _k_fwdR(ctx, S, x, g1, w1, R, g2, w2, eps)
            _gate("fwdR_grad", fam, "2D nx=%d %dx%d R=%g eps=%g" % (nx, n1, n2, R, eps), got, GR.fwdR_grad_f64(S, x, g1, w1, R, g2, w2, eps),
                  *GR.fwdR_grad_ld(S, x, g1, w1, R, g2, w2, eps))


@gpu
@pytest.mark.parametrize("dim", [1, 2])
def test_fwdR_grad_table_equals_plain_calls(ctx, dim):
    Rs, epss = [200.0, 1.0, 50.0], [80.0, 16.0, 5.0]
    if dim == 1:
        nx, G, ngl2 = 257, 256, 0
        x, g1, w1 = _geometry_1d(nx, G)
        g2 = w2 = None
    else:
        nx, G, ngl2 = 48, 240, 24
        x, g1, w1, g2, w2 = _geometry_2d(nx, 10, 24)
    for fam in ("normal", "spike"):
        Ss = [GR.weights(fam, (nx, G), b) for b in range(3)]
        ins = [np.stack(Ss), x, g1, w1] + ([g2, w2] if dim == 2 else [])
        out = _twice(lambda: ctx.debug_grad_op("fwdR_grad", ins, [3 * S_OUT], n=[nx, G, ngl2], l=[0, 0, 0, S_OUT], B=3,
                                                hp=_hp(R=Rs, eps=epss), table=True))[0].reshape(3, S_OUT)
        assert np.all(out[:, 1:] == 0.0)
        for b in range(3):
            eps = epss[b] if dim == 2 else 0.0
            assert _same_bits(out[b, :1], _k_fwdR(ctx, Ss[b], x, g1, w1, Rs[b], g2, w2, eps)), "set %d differs from its plain call" % b
            _gate("fwdR_grad", fam, "%dD table set %d" % (dim, b), out[b, :1], GR.fwdR_grad_f64(Ss[b], x, g1, w1, Rs[b], g2, w2, eps),
                  *GR.fwdR_grad_ld(Ss[b], x, g1, w1, Rs[b], g2, w2, eps))


# ---- D_sums
@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nx,nt", [(1, 1), (3, 31), (7, 32), (8, 33), (9, 255), (24, 256), (81, 257), (24, 600)])
def test_D_sums(ctx, nx, nt, B):
    for sig2, first in ((1e-8, 0), (0.05, 0), (1e-8, 1), (0.05, 1)):
        ops = [_D_operands(nx, nt, sig2 * (1 + b), b + first) for b in range(B)]
        ins = [np.stack([o[k] for o in ops]) for k in range(3)]
        a, b_, s1, rows = _twice(lambda: ctx.debug_grad_op("D_sums", ins, [B * nx, B * nt, B * 8, B * nx], n=[nx, nt], l=[0, 0, 0, 8], B=B))
        a, b_, s1, rows = a.reshape(B, nx), b_.reshape(B, nt), s1.reshape(B, 8), rows.reshape(B, nx)
        assert np.all(s1[:, 1:] == 0.0)
        for q, (D, es, et) in enumerate(ops):
            label = "%dx%d sig2=%g set %d of %d" % (nx, nt, sig2, q, B)
            for name, got, yard, (ref, den) in zip(("a", "b", "sum", "rows"), (a[q], b_[q], s1[q, 0], rows[q]), GR.D_sums_f64(D, es, et),
                                                   GR.D_sums_ld(D, es, et)):
                _gate("D_sums", "spectrum", "%s %s" % (name, label), got, yard, ref, den)
            if B > 1:
                alone = ctx.debug_grad_op("D_sums", [D, es, et], [nx, nt, 1, nx], n=[nx, nt], l=[0, 0, 0, 1])
                assert all(_same_bits(x, y) for x, y in zip(alone, (a[q], b_[q], s1[q, :1], rows[q]))), "set %d differs from the same set alone" % q


# ---- batch_reduce
@gpu
@pytest.mark.parametrize("n", [1, 5, 24, 37])
@pytest.mark.parametrize("nb", [1, 2, 31, 32, 33, 200])
def test_batch_reduce(ctx, nb, n):
    """Sums of symmetric products of which only the lower triangles were formed: everything strictly above the diagonals, and the
    padding between the terms, is NaN here and must stay unread; the result is finite and exactly symmetric."""
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    for fam in ("normal", "spike"):
        for stride in (n * n, n * n + 3):
            for B, s_dvec in ((1, n), (2, 0), (2, n)):
                s_in = nb * stride + 5
                src = np.full((B, s_in), np.nan)
                terms = []
                for q in range(B):
                    T = np.array(GR.weights(fam, (nb, n, n), q))
                    T[:, up] = np.nan
                    terms.append(T)
                    for k in range(nb):
                        src[q, k * stride:k * stride + n * n] = T[k].reshape(-1)
                dvec = np.random.RandomState(n + nb).standard_normal((B - 1) * s_dvec + n)
                for scale, dscale in ((0.5, -0.5 * nb), (1.0, 0.0)):
                    out = _twice(lambda: ctx.debug_grad_op("batch_reduce", [src, dvec], [B * (n * n + 2)], n=[nb, n], l=[stride, s_in, s_dvec, n * n + 2],
                                                            s=[scale, dscale], B=B))[0].reshape(B, n * n + 2)
                    assert np.all(out[:, n * n:] == 0.0)
                    for q in range(B):
                        got, dv = out[q, :n * n].reshape(n, n), dvec[q * s_dvec:q * s_dvec + n]
                        assert np.all(np.isfinite(got)) and _same_bits(got, got.T.copy()), "not finite or not symmetric bit for bit"
                        _gate("batch_reduce", fam, "nb=%d n=%d stride=%d B=%d s_dvec=%d dscale=%g" % (nb, n, stride, B, s_dvec, dscale), got,
                              GR.batch_reduce_f64(terms[q], n, scale, dv, dscale), *GR.batch_reduce_ld(terms[q], n, scale, dv, dscale))


# ---- siglist_eigvec_term
@gpu
@pytest.mark.parametrize("tiny", [0.0, 1e-12])
@pytest.mark.parametrize("nx", [2, 12, 16, 17, 40])
def test_siglist_eigvec_term(ctx, nx, tiny):
    ops = [_siglist_operands(nx, b) for b in range(2)]
    ins = [np.stack([o[k] for o in ops]) for k in range(4)]
    out = _twice(lambda: ctx.debug_grad_op("siglist_eigvec_term", ins, [2 * nx * nx], n=[nx], s=[tiny], B=2))[0].reshape(2, nx, nx)
    for q, (Ghs, Ssum, es, sig) in enumerate(ops):
        ref, den, touched = GR.siglist_eigvec_term_ld(Ghs, Ssum, es, sig, tiny)
        expect = nx * (nx - 1) - (2 if tiny == 0.0 else 4 if nx >= 12 else 2)
        assert touched.sum() == expect
        assert _same_bits(out[q][~touched], Ghs[~touched]), "an entry of the diagonal or of a coinciding pair was written"
        assert np.all(out[q][touched] != Ghs[touched]), "an entry that should have been updated was not"
        _gate("siglist_eigvec_term", "normal", "nx=%d tiny=%g set %d" % (nx, tiny, q), out[q], GR.siglist_eigvec_term_f64(Ghs, Ssum, es, sig, tiny),
              ref, den)
        alone = ctx.debug_grad_op("siglist_eigvec_term", [Ghs, Ssum, es, sig], [nx * nx], n=[nx], s=[tiny])[0]
        assert _same_bits(alone, out[q].reshape(-1))


# ---- rowgroup_sumsq, per_trial_quad
@gpu
@pytest.mark.parametrize("nrows", [1, 3, 25])
@pytest.mark.parametrize("rowlen", [1, 255, 256, 257, 1000])
def test_rowgroup_sumsq(ctx, rowlen, nrows):
    fams = [("normal", GR.weights("normal", (nrows, rowlen))), ("spike", GR.weights("spike", (nrows, rowlen))),
            ("onehot_last", GR.weights("onehot", (nrows, rowlen)))]
    if rowlen > 256:
        fams.append(("onehot_wrap", GR.weights("onehot", (nrows, rowlen), 0, (nrows - 1) * rowlen + 256)))
    for fam, Bm in fams:
        got = _twice(lambda: ctx.debug_grad_op("rowgroup_sumsq", [Bm], [nrows], n=[nrows], l=[rowlen]))[0]
        _gate("rowgroup_sumsq", fam, "%d rows of %d" % (nrows, rowlen), got, GR.rowgroup_sumsq_f64(Bm, nrows), *GR.rowgroup_sumsq_ld(Bm, nrows))


@gpu
@pytest.mark.parametrize("nb", [1, 3, 25])
@pytest.mark.parametrize("nx,nt", [(1, 1), (5, 51), (16, 16), (1, 257), (257, 1), (8, 125)])
def test_per_trial_quad(ctx, nx, nt, nb):
    D = _D_operands(nx, nt, 0.05, 0)[0]
    fams = [("normal", GR.weights("normal", (nx, nb, nt))), ("spike", GR.weights("spike", (nx, nb, nt))),
            ("onehot_last", GR.weights("onehot", (nx, nb, nt)))]
    if nx * nt > 256:                                                  # element 256 of the last trial's sum, the first of the second pass
        x, i = 256 // nt, 256 % nt
        fams.append(("onehot_wrap", GR.weights("onehot", (nx, nb, nt), 0, (x * nb + nb - 1) * nt + i)))
    for fam, al in fams:
        got = _twice(lambda: ctx.debug_grad_op("per_trial_quad", [al, D], [nb], n=[nx, nb, nt]))[0]
        _gate("per_trial_quad", fam, "nx=%d nb=%d nt=%d" % (nx, nb, nt), got, GR.per_trial_quad_f64(al, D, nx, nb, nt),
              *GR.per_trial_quad_ld(al, D, nx, nb, nt))


# ---- bad arguments
@gpu
def test_bad_arguments_are_rejected_and_the_context_stays_usable(ctx):
    """Every class of rejected argument raises before anything is launched; a valid call on the same context afterwards passes."""
    nt = 37
    Gt, t, hp = GR.weights("normal", (nt, nt)), _times(nt, True), HP_T["usual"]
    dK = GR.weights("normal", (2, nt * nt), 5)

    def good(tag):
        _gate("temporal_grad", "normal", "after %s" % tag, _k_temporal(ctx, Gt, t, hp), GR.temporal_grad_f64(Gt, t, *hp), *GR.temporal_grad_ld(Gt, t, *hp))

    def temporal(Gt=Gt, t=t, nt=nt, hps=None, s_out=4, nout=4, **kw):
        return ctx.debug_grad_op("temporal_grad", [Gt, t], [nout], n=[nt], l=[0, 0, 0, s_out], hp=hps if hps is not None else _hp([hp]), **kw)

    nine = _hp([HP_T["eight"]])
    nine.rec["n_temporal"][0] = 9
    none = _hp([hp])
    none.rec["n_temporal"][0] = 0
    kind = _hp([hp])
    kind.rec["kind"][0, 1] = 2
    two = _hp([HP_T["se_only"], hp])                                   # the second set has more components than the first
    bad = {
        "a null operand": lambda: temporal(Gt=None),
        "a null second operand": lambda: ctx.debug_grad_op("frob_inner", [Gt, None], [2], n=[2], l=[nt * nt]),
        "no hyper-parameters": lambda: ctx.debug_grad_op("temporal_grad", [Gt, t], [4], n=[nt], l=[0, 0, 0, 4]),
        "a size of zero": lambda: temporal(nt=0),
        "a negative size": lambda: temporal(nt=-3),
        "a short operand": lambda: temporal(Gt=Gt[:-1]),
        "a short output": lambda: temporal(nout=3),
        "outputs too close": lambda: temporal(s_out=3, nout=3),
        "ncomp = 9": lambda: temporal(hps=nine, s_out=18, nout=18),
        "ncomp = 0": lambda: temporal(hps=none),
        "an unknown kind": lambda: temporal(hps=kind),
        "a later set with more components": lambda: temporal(Gt=np.stack([Gt, Gt]), hps=two, B=2, table=True, s_out=S_OUT, nout=2 * S_OUT),
        "sets by value": lambda: temporal(Gt=np.stack([Gt, Gt]), hps=_hp([hp, hp]), B=2, nout=8),
        "no sets": lambda: temporal(B=0),
        "nm = 0": lambda: ctx.debug_grad_op("frob_inner", [Gt, dK], [1], n=[0], l=[nt * nt]),
        "nm = 17": lambda: ctx.debug_grad_op("frob_inner", [Gt, np.zeros((17, nt * nt))], [17], n=[17], l=[nt * nt]),
        "ngl2 that does not divide G": lambda: ctx.debug_grad_op("kgl_grad", [Gt, Gt, t, t], [2], n=[nt, 5], l=[0, 0, 0, 2], s=[1.0, 1.0]),
        "a stride below n n": lambda: ctx.debug_grad_op("batch_reduce", [Gt, t], [nt * nt], n=[1, nt], l=[nt * nt - 1, nt * nt, nt, nt * nt],
                                                         s=[1.0, 0.0]),
        "a short dvec": lambda: ctx.debug_grad_op("batch_reduce", [np.stack([Gt, Gt]), t], [2 * nt * nt], n=[1, nt],
                                                   l=[nt * nt, nt * nt, nt, nt * nt], s=[1.0, 0.0], B=2),
        "a table for an op without one": lambda: ctx.debug_grad_op("frob_inner", [Gt, dK], [2], n=[2], l=[nt * nt], table=True),
    }
    for tag, call in bad.items():
        with pytest.raises(ValueError):
            call()
        good(tag)
    from gpcsd_amd import _hip
    a = _hip.DebugGradArgs()
    a.op, a.B = 99, 1
    assert ctx._lib.gpcsd_debug_grad_op(ctx._h, a) == -3 and ctx._lib.gpcsd_debug_grad_op(ctx._h, None) == -3
    good("an unknown op")
