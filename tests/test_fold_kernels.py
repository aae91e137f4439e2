"""The folded-basis and relayout kernels on their own (gram.hip: k_swap_last2, k_swap_last2_sum, k_sym_fold_rect, k_sym_unfold_mat,
k_fold_lfp, k_unfold_swap_sum, k_temporal_fold_fill / _tab; eigh.hip: k_psd_fold_fill, plain and table forms) through
gpcsd_debug_fold_op, which puts nothing between the caller and the launchers, against the definitions in long double (fold_ref.py:
products with the explicit fold operator F), over four families of involutions -- mirror_even (no fixed point), mirror_odd (one, in
the middle), identity, scattered (several fixed points, pairs that are not neighbours) -- and at the smallest shapes that reach
every path: ns^2 on both sides of one 256-thread block, 16 time orbits x 64 trials per workgroup of unfold_swap_sum with R = 63 /
64 / 65 and up to three steps in time, padded and unpadded column blocks, list on and off, replicas by value and by table.

Gates.  Exact operations (the two transposes, the lists against the sum at C = 1, everything no kernel may write) are compared bit
for bit; every output starts as a fill pattern, and every input's padding holds NaN, so that a kernel that writes or reads beside
its operands shows.  A rounded operation's output is a signed sum of at most four inputs times one or two of the constants 1/sqrt2,
1/2: |got - ref| <= gamma_c sum |w x|, gamma_c = c u / (1 - c u), u = 2^-53, with c the roundings on the kernel's longest path,
counted from its source -- either contraction of a multiply-add leaves out a rounding and is allowed for:
    sym_fold_rect     ss 7: the two constants (wa, wb: fl(1/sqrt2)), wa wb, three additions, the product with the sum;  aa 3: three
                      additions (1/2 is exact)
    sym_unfold_mat    5: two constants, w_i w_j, the product with Gss, the addition of the (exact) antisymmetric term
    fold_lfp          6: two additions on an input's way into v, two constants, wq wb, the product
    unfold_swap_sum   6 per component: two constants, their product, the product with the tile (aa: none, 1/2 is exact), two additions;
                      the sum over C components adds u x the running magnitudes of the C - 1 additions (the first adds to zero)
    psd_fold_fill     8: sym_fold_rect's 7 and the addition of the shift; the division by the power of two is exact
    temporal fill     7 on the combination of four kernel values, each of which carries the propagated bound of
                      test_matern_kinds.py item 1 -- (16 + 4 a) u |sigma2 k| + max(1, sigma2) 2^-1074 per component, a the magnitude
                      of the exponential's argument (SE: d^2 / (2 ell^2)), and u x the magnitudes for each of the C - 1 additions of
                      the components --, all divided by the scale, plus 2^-1074 for a quotient that is subnormal
The scale words must equal the reference's exactly: the power of two above 2 sum |sigma2| (temporal), above the largest diagonal
entry of each block after the shift, floored at 2^-30 of the larger block's (PSD).

From above (test_planted_faults_miss_the_gates, on the CPU, each in a float64 numpy transcription of the kernel that itself
passes the gate): 1/sqrt2 on a fixed point, the sign of the second pair member dropped, the antisymmetric block indexed with ns for
na, the time orbit at a tile's edge dropped, the last component left out of the sum, the scale without its factor 2 -- each misses
its gate by a factor of 1e13 and more.

Every operation is run twice on the same operands and must return the same bits; the table forms must return the bits of the
by-value calls, set by set.

Measured on the MI355X, worst ratio of error to bound per operation and family (time-side family for the two-sided kernels):

                                         mirror_even  mirror_odd  identity  scattered
  sym_fold_rect                              0.54        0.55       0.17      0.52
  sym_unfold_mat                             0.61        0.60       0         0.62
  fold_lfp                                   0.62        0.62       0.38      0.64
  unfold_swap_sum                            0.66        0.64       0.39      0.58
  temporal_fold_fill                         0.31        0.29        -        0.31
  psd_fold_fill                              0.48        0.48        -        0.48
  round trip unfold_mat(fold_rect(K))        0.43        0.45       0         0.39
  round trip unfold_swap_sum(fold_lfp(Y))    0.36        0.39        -        0.36

Found and fixed: nothing.  No kernel exceeded its counted bound; every exact comparison held to the bit, every table form returned
the bits of its plain calls and every operation the same bits twice; the fp32 temporal fill deviates by 5.8e-8 / 8.6e-8 of the
largest entry.  What the suite did settle are two statements of the sources:

"The same expressions, in the same order" (kernels.hpp, k_temporal_fold_fill): proven by bits.  A0 amax of the temporal fill
equals A0 amax of the PSD fill with zero shift applied to gpcsd_gram_temporal's output, 0 ulp apart on every entry, for the sets of
one component (the public Gram entry point evaluates one component; a sum of its outputs on the host is not the kernel's sum) of
all four kinds.  gram.hip is compiled without contraction, so the two instantiations round alike; the comment stands.

tau and the progress word (eigh_dc.hip): the word behind tau's n + 64 entries exists for the register tail of a staged TEMPORAL
chain (EighCall::progress, set by the temporal chain's queuing routine alone); the spatial classes never carry one.  The temporal
fill therefore clears n + 66 words and the PSD fill n + 64 -- the code was right, the comment in eigh_dc.hip was loose and now says
so -- and both extents are asserted here, with the words behind them.  (Slices of an arena start at even offsets: the word behind
V's (n + 64) n words is a padding word that keeps the fill pattern when that count is odd, and tau's first word, a zero, when it
is even.)
"""
import numpy as np
import pytest

import fold_ref as FR
import matern_ref as MT

LD = FR.LD
U = FR.U
SE, MAT, M32, M52 = MT.SE, MT.MATERN, MT.MATERN32, MT.MATERN52
FILL = -1.2345678901234567e+123                 # what every output starts as
ISQ2 = 0.70710678118654752440                   # the kernels' constant
C_FOLD_SS, C_FOLD_AA, C_UNFOLD_MAT, C_FOLD_LFP, C_UNFOLD, C_PSD, C_TFILL = 7, 3, 5, 6, 6, 8, 7
TINY = LD(2.0) ** -1074
gpu = pytest.mark.gpu
WORST = {}

# temporal hyper-parameter sets of the fills: test_grad_kernels.HP_T's and the two new kinds
HP_NEW = {"m32": ((M32,), (5.0,), (0.7,)),
          "m52": ((M52,), (20.0,), (0.5,)),
          "four": ((SE, M52, MAT, M32), (20.0, 8.0, 5.0, 3.0), (0.5, 0.3, 0.7, 1.1))}


def _hp_sets():
    import test_grad_kernels as TG
    sets = {k: TG.HP_T[k] for k in ("usual", "short", "long", "mixed", "zero_s2", "eight", "se_only")}
    sets.update(HP_NEW)
    sets["m12"] = ((MAT,), (5.0,), (0.7,))
    return sets


def gamma(c):
    return LD(c) * LD(U) / (LD(1) - LD(c) * LD(U))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _is_fill(a):
    return bool(np.all(_bits(a) == _bits(np.array([FILL]))[0]))


def _ratio(got, ref, bound):
    """worst |got - ref| / bound; an error where the bound is zero counts as infinite"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    if err.size == 0:
        return 0.0
    if np.any(~np.isfinite(err)):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    return float(np.max(r))


def _gate(op, fam, label, got, ref, bound):
    r = _ratio(got, ref, bound)
    WORST[(op, fam)] = max(WORST.get((op, fam), 0.0), r)
    print("[fold] %-18s %-12s %-46s error / bound %9.3g" % (op, fam, label, r))
    assert r <= 1.0, "%s, %s %s: the error is %.3g of the counted bound" % (op, fam, label, r)
    return r


def _families(n):
    fams = ["mirror_odd" if n % 2 else "mirror_even", "identity"]
    if n >= 3:
        fams.append("scattered")
    return fams


def _sum_bound(mags, c):
    """bound of the sum over components in index order: each component's counted bound, and u x the running magnitude for each
    addition but the first (which adds to zero)"""
    run, b = np.zeros_like(mags[0]), np.zeros_like(mags[0])
    for k, m in enumerate(mags):
        run = run + m * (LD(1) + gamma(c))
        b = b + gamma(c) * m
        if k > 0:
            b = b + LD(U) * run
    return b


# ------------------------------------------------------------------------------------------------ float64 transcriptions (CPU)
def _w(tb, fault=None):
    w = np.where(tb["rep_i"] == tb["rep_j"], 1.0, ISQ2)
    return np.full(tb["ns"], ISQ2) if fault == "fixed_weight" else w


def t_fold_rect(K, pr, pc, fault=None, shift=0.0):
    """sym_fold_rect_kernel in float64 numpy -> (ss, aa); shift: psd_fold_fill's entries before the scaling"""
    r, c = FR.orbit_tables(pr), FR.orbit_tables(pc)
    i, j, k, l = r["rep_i"][:, None], r["rep_j"][:, None], c["rep_i"][None, :], c["rep_j"][None, :]
    lk, ji = l != k, j != i
    kil, kjk, kjl = np.where(lk, K[i, l], 0.0), np.where(ji, K[j, k], 0.0), np.where(ji & lk, K[j, l], 0.0)
    ssum = ((K[i, k] + kil) + kjk) + kjl
    sg = 1.0 if fault == "second_sign" else -1.0
    asum = ((K[i, k] + sg * kil) + sg * kjk) + kjl
    dshift = shift * (np.arange(r["ns"])[:, None] == np.arange(c["ns"])[None, :])
    ss = (_w(r, fault)[:, None] * _w(c, fault)[None, :]) * ssum + dshift
    return ss, (0.5 * asum + dshift)[:r["na"], :c["na"]]


def t_unfold_mat(Gf, perm, fault=None):
    """sym_unfold_mat_kernel for one set: Gf flat (Gss, then Gaa)"""
    tb = FR.orbit_tables(perm)
    ns, na = tb["ns"], tb["na"]
    a, b, si, sj = tb["orb"][:, None], tb["orb"][None, :], tb["sgn"][:, None], tb["sgn"][None, :]
    wi, wj = np.where(si == 0, 1.0, ISQ2), np.where(sj == 0, 1.0, ISQ2)
    if fault == "fixed_weight":
        wi, wj = np.full_like(wi, ISQ2), np.full_like(wj, ISQ2)
    if fault == "second_sign":
        si, sj = np.abs(si), np.abs(sj)
    v = (wi * wj) * Gf[a * ns + b]
    both = (si != 0) & (sj != 0)
    idx = np.minimum(ns * ns + a * (ns if fault == "ns_for_na" else na) + b, Gf.size - 1)
    return v + np.where(both, 0.5 * (si * sj) * Gf[np.where(both, idx, 0)], 0.0)


def t_fold_lfp(Y, ps, pt, fault=None):
    """fold_lfp_kernel: Y (nx, R, nt) -> (nx, R, nt) in fold order"""
    S, T = FR.orbit_tables(ps), FR.orbit_tables(pt)
    q, b = np.arange(Y.shape[0]), np.arange(Y.shape[2])
    qa, ba = q >= S["ns"], b >= T["ns"]
    a, bb = np.where(qa, q - S["ns"], q), np.where(ba, b - T["ns"], b)
    i, j, k, l = S["rep_i"][a], S["rep_j"][a], T["rep_i"][bb], T["rep_j"][bb]
    sj, sl = np.where(qa, -1.0, 1.0), np.where(ba, -1.0, 1.0)
    if fault == "second_sign":
        sj, sl = np.ones_like(sj), np.ones_like(sl)
    wq, wb = _w(S, fault)[a], _w(T, fault)[bb]
    v = Y[i][:, :, k] + np.where(l != k, sl * Y[i][:, :, l], 0.0)
    u = Y[j][:, :, k] + np.where(l != k, sl * Y[j][:, :, l], 0.0)
    v = v + np.where(j != i, sj, 0.0)[:, None, None] * u
    return (wq[:, None, None] * wb[None, None, :]) * v


def t_unfold_swap_sum(inp, C, R, pz, pt, nsP=0, naP=0, fault=None):
    """unfold_swap_sum_kernel: inp (nz R, ldin) -> (list (C, nz, nt, R), sum (nz, nt, R)); what it does not write holds FILL"""
    Z, T = FR.orbit_tables(pz), FR.orbit_tables(pt)
    nz, nt, zs, za, ts, ta = np.asarray(pz).size, np.asarray(pt).size, Z["ns"], Z["na"], T["ns"], T["na"]
    nsP, naP = nsP or ts, naP or ta
    in3 = inp.reshape(nz, R, -1)
    zi, zj, tk, tl = Z["rep_i"], Z["rep_j"], T["rep_i"], T["rep_j"]
    wz, wt = _w(Z, fault)[:, None, None], _w(T, fault)[None, None, :]
    lst, acc = np.full((C, nz, nt, R), FILL), [np.zeros((zs, R, ts)) for _ in range(4)]
    keep = np.ones(ts, dtype=bool)
    if fault == "tile_edge":
        keep[16] = False
    for c in range(C):
        t00 = in3[:zs, :, c * nsP:c * nsP + ts]
        t01, t10, t11 = np.zeros_like(t00), np.zeros_like(t00), np.zeros_like(t00)
        t01[:, :, :ta] = in3[:zs, :, C * nsP + c * naP:C * nsP + c * naP + ta]
        t10[:za] = in3[zs:, :, c * nsP:c * nsP + ts]
        t11[:za, :, :ta] = in3[zs:, :, C * nsP + c * naP:C * nsP + c * naP + ta]
        ss, sa, as_, aa = wz * wt * t00, wz * ISQ2 * t01, ISQ2 * wt * t10, 0.5 * t11
        if fault == "second_sign":
            vs = [(ss + sa) + (as_ + aa)] * 4
        else:
            vs = [(ss + sa) + (as_ + aa), (ss - sa) + (as_ - aa), (ss + sa) - (as_ + aa), (ss - sa) - (as_ - aa)]
        for m in (3, 2, 1, 0):                       # (v0 last: an orbit that is a fixed point holds v0)
            z_, t_ = (zi, zj)[m >> 1], (tk, tl)[m & 1]
            lst[c][z_[:, None], t_[None, keep]] = vs[m].transpose(0, 2, 1)[:, keep]
            if not (fault == "last_component" and c == C - 1 and C > 1):
                acc[m] = acc[m] + vs[m]
    out = np.full((nz, nt, R), FILL)
    for m in (3, 2, 1, 0):
        z_, t_ = (zi, zj)[m >> 1], (tk, tl)[m & 1]
        out[z_[:, None], t_[None, keep]] = acc[m].transpose(0, 2, 1)[:, keep]
    return lst, out


# ------------------------------------------------------------------------------------------------ shared references
def _rect_case(pr, pc, seed=0):
    rs = np.random.RandomState(seed + 13 * len(pr) + len(pc))
    K = rs.standard_normal((len(pr), len(pc)))
    (ss, aa), (mss, maa) = FR.fold_rect(K, pr, pc)
    return K, ss, aa, gamma(C_FOLD_SS) * mss, gamma(C_FOLD_AA) * maa


def _unfold_mat_case(perm, B, seed=0):
    tb = FR.orbit_tables(perm)
    ns, na = tb["ns"], tb["na"]
    rs = np.random.RandomState(seed + 7 * len(perm))
    sets = [(rs.standard_normal((ns, ns)), rs.standard_normal((na, na))) for _ in range(B)]
    refs = [FR.unfold_mat(gss, gaa, perm) for gss, gaa in sets]
    return sets, refs


def _pred_case(pz, pt, R, C, seed=0):
    rs = np.random.RandomState(seed + 31 * len(pz) + 7 * len(pt) + R)
    X = rs.standard_normal((len(pz), R, C, len(pt))) * (10.0 ** rs.uniform(-2, 2, size=(1, 1, C, 1)))
    comp, mags = FR.unfold_pred(X, pz, pt)
    return X, comp, mags


def _tfill_ref(t, perm, hp):
    """scaled blocks of the temporal fill in long double, their bounds, the scale"""
    K, kb, mag = FR.temporal_gram(t, *hp)
    F, tb = FR.fold_matrix(perm), FR.orbit_tables(perm)
    ns = tb["ns"]
    m = FR.temporal_scale(hp[2])
    M = F @ K @ F.T
    A = np.abs(F)
    bound = (A @ kb @ A.T) * (LD(1) + gamma(C_TFILL)) + gamma(C_TFILL) * (A @ (mag + kb) @ A.T)
    return (M[:ns, :ns] / LD(m), M[ns:, ns:] / LD(m)), (bound[:ns, :ns] / LD(m) + TINY, bound[ns:, ns:] / LD(m) + TINY), m


def _psd_ref(K, perm, shift):
    (ss, aa), (mss, maa) = FR.fold_rect(K, perm, perm)
    ms, ma, margin = FR.psd_scales(K, perm, shift)
    s = LD(shift)
    ss, aa = ss + s * np.eye(ss.shape[0], dtype=LD), aa + s * np.eye(aa.shape[0], dtype=LD)
    mss, maa = mss + abs(s) * np.eye(ss.shape[0], dtype=LD), maa + abs(s) * np.eye(aa.shape[0], dtype=LD)
    return (ss / LD(ms), aa / LD(ma)), (gamma(C_PSD) * mss / LD(ms) + TINY, gamma(C_PSD) * maa / LD(ma) + TINY), (ms, ma), margin


# ------------------------------------------------------------------------------------------------ CPU: the references themselves
@pytest.mark.parametrize("family", FR.FAMILIES)
def test_fold_operator_is_orthogonal(family):
    for n in (2, 3, 16, 17, 33, 70):
        if family.startswith("mirror") and n % 2 != (family == "mirror_odd"):
            continue
        perm = FR.involution(family, n)
        F, tb = FR.fold_matrix(perm), FR.orbit_tables(perm)
        dev = float(np.max(np.abs(F @ F.T - np.eye(n, dtype=LD))))
        print("[fold-ref] %-12s n = %2d: ns = %2d, na = %2d, |F F^T - I| = %.2g" % (family, n, tb["ns"], tb["na"], dev))
        assert dev <= 4 * np.finfo(LD).eps
        assert tb["ns"] + tb["na"] == n and np.all(tb["rep_i"][:tb["na"]] < tb["rep_j"][:tb["na"]])
        assert np.all(np.diff(tb["rep_i"][:tb["na"]]) > 0) and np.all(np.diff(tb["rep_i"][tb["na"]:]) > 0)
        if family == "identity":
            assert tb["na"] == 0
        if family == "mirror_even":
            assert tb["ns"] == tb["na"]
        if family == "mirror_odd":
            assert tb["ns"] == tb["na"] + 1
        if family == "scattered" and n >= 16:
            assert tb["ns"] - tb["na"] >= 3 and np.any(tb["rep_j"][:tb["na"]] - tb["rep_i"][:tb["na"]] > 1)
        # the reflection itself: F P F^T = diag(+1 (ns), -1 (na))
        P = np.eye(n, dtype=LD)[perm]
        sig = np.concatenate([np.ones(tb["ns"]), -np.ones(tb["na"])]).astype(LD)
        assert float(np.max(np.abs(F @ P @ F.T - np.diag(sig)))) <= 4 * np.finfo(LD).eps


@pytest.mark.parametrize("family", FR.FAMILIES)
def test_reference_fold_then_unfold_is_the_identity(family):
    n = 17 if family != "mirror_even" else 16
    perm, pt = FR.involution(family, n), FR.mirror(9)
    t = FR.symmetric_grid(perm)
    K = FR.se_gram(t, 20.0)                                      # commutes with the reflection
    (ss, aa), _ = FR.fold_rect(K, perm, perm)
    x1, x2 = FR.fold_rect_cross(K, perm, perm)
    assert max(float(np.max(np.abs(x1), initial=0)), float(np.max(np.abs(x2), initial=0))) <= 64 * np.finfo(LD).eps
    back, _ = FR.unfold_mat(ss, aa, perm)                         # (long double in, long double out)
    assert float(np.max(np.abs(back - K.astype(LD)))) <= 64 * np.finfo(LD).eps
    Y = np.random.RandomState(1).standard_normal((n, 3, 9))
    Yf, _ = FR.fold_lfp(Y, perm, pt)
    back, _ = FR.unfold_pred(Yf[:, :, None, :], perm, pt)
    assert float(np.max(np.abs(back[0].transpose(0, 2, 1) - Y.astype(LD)))) <= 64 * np.finfo(LD).eps


def test_scale_rules():
    assert FR.pow2_above(1.0) == 2.0 and FR.pow2_above(0.75) == 1.0 and FR.pow2_above(3.0) == 4.0 and FR.pow2_above(2.0 ** -40) == 2.0 ** -39
    assert FR.pow2_above(0.0) == 1.0 and FR.pow2_above(np.inf) == 1.0 and FR.pow2_above(np.nan) == 1.0 and FR.pow2_above(1.75e308) == 1.0
    assert FR.pow2_above(1.0e308) == 1.0e308 and FR.pow2_above(2.0 ** 1022) == 2.0 ** 1023
    assert FR.temporal_scale((0.5, 0.7)) == 4.0 and FR.temporal_scale((0.0,)) == 1.0 and FR.temporal_scale((0.5,)) == 2.0
    assert FR.temporal_scale((1e-6, 1.0, 1e4)) == 32768.0 and FR.temporal_scale((-0.5, 0.25)) == 2.0


def test_transcriptions_pass_the_gates():
    """The float64 numpy transcriptions (no contraction) stay inside the counted bounds the kernels are held to."""
    for fam in FR.FAMILIES:
        n = 16 if fam == "mirror_even" else 17
        perm, pc = FR.involution(fam, n), FR.involution("scattered", 21)
        K, ss, aa, bss, baa = _rect_case(perm, pc)
        gss, gaa = t_fold_rect(K, perm, pc)
        _gate("t:sym_fold_rect", fam, "ss", gss, ss, bss)
        _gate("t:sym_fold_rect", fam, "aa", gaa, aa, baa)
        sets, refs = _unfold_mat_case(perm, 1)
        _gate("t:sym_unfold_mat", fam, "", t_unfold_mat(np.concatenate([sets[0][0].ravel(), sets[0][1].ravel()]), perm), refs[0][0],
              gamma(C_UNFOLD_MAT) * refs[0][1])
        Y = np.random.RandomState(2).standard_normal((n, 3, 21))
        ref, mag = FR.fold_lfp(Y, perm, pc)
        _gate("t:fold_lfp", fam, "", t_fold_lfp(Y, perm, pc), ref, gamma(C_FOLD_LFP) * mag)
        X, comp, mags = _pred_case(perm, pc, 5, 3)
        lst, tot = t_unfold_swap_sum(FR.pack_pred(X, pc), 3, 5, perm, pc)
        _gate("t:unfold_swap_sum", fam, "list", lst, comp, gamma(C_UNFOLD) * mags)
        _gate("t:unfold_swap_sum", fam, "sum", tot, comp.sum(axis=0), _sum_bound(list(mags), C_UNFOLD))


def test_planted_faults_miss_the_gates():
    """Each fault, planted in a transcription that passes the gate without it, misses that gate by at least 1e6."""
    n = 35                                                       # mirror_odd: ns = 18, na = 17 -- a fixed point, ns != na, ns > 16
    perm, pz = FR.mirror(n), FR.involution("scattered", 7)
    K, ss, aa, bss, baa = _rect_case(perm, perm)
    sets, refs = _unfold_mat_case(perm, 1)
    Gf = np.concatenate([sets[0][0].ravel(), sets[0][1].ravel()])
    Y = np.random.RandomState(3).standard_normal((7, 3, n))
    fref, fmag = FR.fold_lfp(Y, pz, perm)
    X, comp, mags = _pred_case(pz, perm, 5, 3)
    packed = FR.pack_pred(X, perm)
    sum_ref, sum_bound = comp.sum(axis=0), _sum_bound(list(mags), C_UNFOLD)
    hp = ((SE, MAT), (20.0, 5.0), (0.5, 0.7))
    t = FR.symmetric_grid(perm)
    (rs_, ra_), (bs_, ba_), m = _tfill_ref(t, perm, hp)
    Kt = np.asarray(FR.temporal_gram(t, *hp)[0], dtype=np.float64)
    found = {
        "1/sqrt2 on a fixed point (sym_fold_rect)": _ratio(t_fold_rect(K, perm, perm, "fixed_weight")[0], ss, bss),
        "1/sqrt2 on a fixed point (sym_unfold_mat)": _ratio(t_unfold_mat(Gf, perm, "fixed_weight"), refs[0][0], gamma(C_UNFOLD_MAT) * refs[0][1]),
        "1/sqrt2 on a fixed point (fold_lfp)": _ratio(t_fold_lfp(Y, pz, perm, "fixed_weight"), fref, gamma(C_FOLD_LFP) * fmag),
        "1/sqrt2 on a fixed point (unfold_swap_sum)": _ratio(t_unfold_swap_sum(packed, 3, 5, pz, perm, fault="fixed_weight")[1], sum_ref, sum_bound),
        "second member's sign dropped (sym_fold_rect)": _ratio(t_fold_rect(K, perm, perm, "second_sign")[1], aa, baa),
        "second member's sign dropped (sym_unfold_mat)": _ratio(t_unfold_mat(Gf, perm, "second_sign"), refs[0][0], gamma(C_UNFOLD_MAT) * refs[0][1]),
        "second member's sign dropped (fold_lfp)": _ratio(t_fold_lfp(Y, pz, perm, "second_sign"), fref, gamma(C_FOLD_LFP) * fmag),
        "second member's sign dropped (unfold_swap_sum)": _ratio(t_unfold_swap_sum(packed, 3, 5, pz, perm, fault="second_sign")[1], sum_ref, sum_bound),
        "antisymmetric block indexed with ns for na": _ratio(t_unfold_mat(Gf, perm, "ns_for_na"), refs[0][0], gamma(C_UNFOLD_MAT) * refs[0][1]),
        "time orbit dropped at a tile's edge": _ratio(t_unfold_swap_sum(packed, 3, 5, pz, perm, fault="tile_edge")[1], sum_ref, sum_bound),
        "the last component left out": _ratio(t_unfold_swap_sum(packed, 3, 5, pz, perm, fault="last_component")[1], sum_ref, sum_bound),
        "scale from sum sigma2 without the factor 2": _ratio(t_fold_rect(Kt, perm, perm)[0] / FR.pow2_above(sum(hp[2])), rs_, bs_),
    }
    # (... and without the fault the same transcriptions pass)
    assert _ratio(t_fold_rect(Kt, perm, perm)[0] / m, rs_, bs_) <= 1.0 and FR.pow2_above(sum(hp[2])) != m
    assert _ratio(t_unfold_swap_sum(packed, 3, 5, pz, perm)[1], sum_ref, sum_bound) <= 1.0
    for name, r in found.items():
        print("[fold-fault] %-50s misses its gate by a factor of %.3g" % (name, r))
        assert r >= 1e6, "%s would pass: %.3g of the bound" % (name, r)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from gpcsd_amd import _hip
    yield _hip.default_context()
    for (op, fam), r in sorted(WORST.items()):
        print("[fold] worst ratio  %-18s %-12s %.3g" % (op, fam, r))


def _twice(call):
    a, b = call(), call()
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), "two runs on the same operands differ"
    return a


def _hp(sets, jitter=None):
    import test_grad_kernels as TG
    hb = TG._hp(list(sets))
    if jitter is not None:
        hb.rec["jitter"] = jitter
    return hb


# ---- exact operations
@gpu
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 31, 33), (3, 32, 32), (2, 33, 65), (1, 1, 70), (1, 70, 1)])
def test_swap_last2(ctx, shape):
    n0, n1, n2 = shape
    x = np.random.RandomState(sum(shape)).standard_normal(shape)
    tot = x.size
    out = _twice(lambda: ctx.debug_fold_op("swap_last2", [x], [tot + 5], n=shape, fill=FILL))[0]
    assert _same_bits(out[:tot].reshape(n0, n2, n1), np.swapaxes(x, 1, 2)) and _is_fill(out[tot:])


@gpu
@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_swap_last2_sum(ctx, C, with_list):
    for n0, n1, n2 in [(2, 33, 65), (3, 32, 32), (1, 1, 70), (1, 70, 1)]:
        x = np.random.RandomState(n1 + C).standard_normal((n0, n1, C, n2))
        tot = n0 * n1 * n2
        ls = tot + 7                                             # a list stride beyond the block: seven words of padding each
        lens = [tot + 5] + ([C * ls] if with_list else [])
        outs = _twice(lambda: ctx.debug_fold_op("swap_last2_sum", [x], lens, n=[n0, n1, n2, C], l=[ls], with_list=with_list, fill=FILL))
        acc = np.zeros((n0, n2, n1))
        for c in range(C):                                       # additions only, in index order: the bits are defined
            acc = acc + np.swapaxes(x[:, :, c, :], 1, 2)
        assert _same_bits(outs[0][:tot].reshape(n0, n2, n1), acc) and _is_fill(outs[0][tot:])
        if with_list:
            lst = outs[1].reshape(C, ls)
            for c in range(C):
                assert _same_bits(lst[c, :tot].reshape(n0, n2, n1), np.swapaxes(x[:, :, c, :], 1, 2))
            assert _is_fill(lst[:, tot:])


# ---- rounded operations
@gpu
@pytest.mark.parametrize("n", [2, 3, 16, 17, 31, 32, 33])
def test_sym_fold_rect_square(ctx, n):
    for fam in _families(n):
        perm = FR.involution(fam, n)
        tb = FR.orbit_tables(perm)
        K, ss, aa, bss, baa = _rect_case(perm, perm)
        nss, naa = tb["ns"] ** 2, tb["na"] ** 2
        o_ss, o_aa = _twice(lambda: ctx.debug_fold_op("sym_fold_rect", [K], [nss + 3, naa + 3], perms=[perm, perm], l=[n], fill=FILL))
        _gate("sym_fold_rect", fam, "n=%d ss" % n, o_ss[:nss].reshape(ss.shape), ss, bss)
        _gate("sym_fold_rect", fam, "n=%d aa" % n, o_aa[:naa].reshape(aa.shape), aa, baa)
        assert _is_fill(o_ss[nss:]) and _is_fill(o_aa[naa:])     # (na = 0: the whole of out_aa)


@gpu
def test_sym_fold_rect_rectangular(ctx):
    """different involutions on rows and columns, rows ldk apart with NaN in the padding"""
    for (fr, nr), (fc, nc) in [(("scattered", 17), ("mirror_odd", 33)), (("mirror_even", 32), ("scattered", 9)),
                               (("identity", 5), ("mirror_even", 34)), (("mirror_odd", 3), ("identity", 19))]:
        pr, pc = FR.involution(fr, nr), FR.involution(fc, nc)
        tr, tc = FR.orbit_tables(pr), FR.orbit_tables(pc)
        K, ss, aa, bss, baa = _rect_case(pr, pc)
        ldk = nc + 5
        Kp = np.full((nr, ldk), np.nan)
        Kp[:, :nc] = K
        nss, naa = tr["ns"] * tc["ns"], tr["na"] * tc["na"]
        o_ss, o_aa = _twice(lambda: ctx.debug_fold_op("sym_fold_rect", [Kp.ravel()[:(nr - 1) * ldk + nc]], [nss + 3, naa + 3], perms=[pr, pc],
                                                       l=[ldk], fill=FILL))
        _gate("sym_fold_rect", fc, "%s %d x %s %d ss" % (fr, nr, fc, nc), o_ss[:nss].reshape(ss.shape), ss, bss)
        _gate("sym_fold_rect", fc, "%s %d x %s %d aa" % (fr, nr, fc, nc), o_aa[:naa].reshape(aa.shape), aa, baa)
        assert _is_fill(o_ss[nss:]) and _is_fill(o_aa[naa:])


@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [2, 3, 16, 17, 31, 32, 33])
def test_sym_unfold_mat(ctx, n, B):
    for fam in _families(n):
        perm = FR.involution(fam, n)
        tb = FR.orbit_tables(perm)
        blk = tb["ns"] ** 2 + tb["na"] ** 2
        s_in = blk + 3                                           # sets further apart than their blocks: NaN in the gaps
        sets, refs = _unfold_mat_case(perm, B)
        Gf = np.full((B, s_in), np.nan)
        for b, (gss, gaa) in enumerate(sets):
            Gf[b, :blk] = np.concatenate([gss.ravel(), gaa.ravel()])
        out = _twice(lambda: ctx.debug_fold_op("sym_unfold_mat", [Gf.ravel()[:(B - 1) * s_in + blk]], [B * n * n + 3], perms=[perm], l=[s_in],
                                                B=B, fill=FILL))[0]
        for b in range(B):
            _gate("sym_unfold_mat", fam, "n=%d set %d of %d" % (n, b, B), out[b * n * n:(b + 1) * n * n].reshape(n, n), refs[b][0],
                  gamma(C_UNFOLD_MAT) * refs[b][1])
        assert _is_fill(out[B * n * n:])


@gpu
@pytest.mark.parametrize("shape", [(2, 1, 2), (3, 1, 3), (5, 3, 17), (17, 3, 33), (24, 2, 70)])
def test_fold_lfp(ctx, shape):
    nx, R, nt = shape
    for fs, ft in [("mirror", "mirror"), ("identity", "mirror"), ("scattered", "scattered"), ("mirror", "identity"), ("scattered", "mirror")]:
        if (fs == "scattered" and nx < 3) or (ft == "scattered" and nt < 3):
            continue
        ps = FR.mirror(nx) if fs == "mirror" else FR.involution(fs, nx)
        pt = FR.mirror(nt) if ft == "mirror" else FR.involution(ft, nt)
        Y = np.random.RandomState(nx + nt).standard_normal(shape)
        ref, mag = FR.fold_lfp(Y, ps, pt)
        out = _twice(lambda: ctx.debug_fold_op("fold_lfp", [Y], [Y.size + 3], perms=[ps, pt], n=[R], fill=FILL))[0]
        fam = ("mirror_odd" if nt % 2 else "mirror_even") if ft == "mirror" else ft
        _gate("fold_lfp", fam, "%s x %s (%d, %d, %d)" % (fs, ft, nx, R, nt), out[:Y.size].reshape(shape), ref, gamma(C_FOLD_LFP) * mag)
        assert _is_fill(out[Y.size:])


def _unfold_cases():
    """every pair (time grid, R), every value of every knob; the site family, C, the padding and the list cycle through"""
    nts, Rs = [2, 3, 31, 32, 33, 34, 70], [1, 5, 63, 64, 65]
    site = [("mirror_even", 4), ("mirror_odd", 5), ("identity", 3), ("scattered", 6)]
    cases, k = [], 0
    for nt in nts:
        for R in Rs:
            cases.append((nt, "mirror", R, (1, 3)[k % 2], site[k % 4], (k // 2) % 2 == 1, (k // 4) % 2 == 0))
            k += 1
    for nt, R in [(70, 65), (33, 5)]:                            # every combination of C, padding and list at two shapes
        for C in (1, 3):
            for padded in (False, True):
                for lst in (False, True):
                    cases.append((nt, "mirror", R, C, site[k % 4], padded, lst))
                    k += 1
    for nt in (17, 33, 70):                                      # a time involution with several fixed points; none at all
        cases.append((nt, "scattered", 5, 3, site[k % 4], True, True))
        cases.append((nt, "identity", 64, 1, site[(k + 1) % 4], False, True))
        k += 1
    return cases


@gpu
@pytest.mark.parametrize("nt,tfam,R,C,site,padded,with_list", _unfold_cases())
def test_unfold_swap_sum(ctx, nt, tfam, R, C, site, padded, with_list):
    pz = FR.involution(*site)
    pt = FR.mirror(nt) if tfam == "mirror" else FR.involution(tfam, nt)
    T = FR.orbit_tables(pt)
    nz = pz.size
    X, comp, mags = _pred_case(pz, pt, R, C)
    # padded as the prediction pads: column blocks rounded up to 16 doubles, rows 16 doubles beyond
    nsP, naP = ((T["ns"] + 15) & ~15, (T["na"] + 15) & ~15) if padded else (0, 0)
    ldin = C * (nsP + naP) + 16 if padded else 0
    packed = FR.pack_pred(X, pt, nsP, naP, ldin)
    tot = nz * nt * R
    ls = tot + 9
    lens = [tot + 3] + ([C * ls] if with_list else [])
    outs = _twice(lambda: ctx.debug_fold_op("unfold_swap_sum", [packed], lens, perms=[pz, pt], n=[R, C, nsP, naP], l=[ls, ldin],
                                             with_list=with_list, fill=FILL))
    fam = ("mirror_odd" if nt % 2 else "mirror_even") if tfam == "mirror" else tfam
    label = "nt=%d R=%d C=%d %s %s%s" % (nt, R, C, site[0], "padded " if padded else "", "list" if with_list else "")
    _gate("unfold_swap_sum", fam, label + " sum", outs[0][:tot].reshape(nz, nt, R), comp.sum(axis=0), _sum_bound(list(mags), C_UNFOLD))
    assert _is_fill(outs[0][tot:])
    if with_list:
        lst = outs[1].reshape(C, ls)
        _gate("unfold_swap_sum", fam, label + " list", lst[:, :tot].reshape(C, nz, nt, R), comp, gamma(C_UNFOLD) * mags)
        assert _is_fill(lst[:, tot:])
        if C == 1:
            assert _same_bits(lst[0, :tot], outs[0][:tot]), "one component: the list is the sum"


# ---- the two fills
def _fill_call(ctx, op, perm, operand, B, **kw):
    """-> per set: dict(ss, aa, Vs, Va, Vs_next, Va_next, taus, taua, amax, status); V / tau as returned (the word behind included)"""
    tb = FR.orbit_tables(perm)
    ns, na = tb["ns"], tb["na"]
    nv, ntau = ((ns + 64) * ns + 1, (na + 64) * na + 1), (ns + 67, na + 67)
    lens = [B * ns * ns + 2, B * na * na + 2, B * sum(nv), B * sum(ntau), 2 * B + 1]
    o = _twice(lambda: ctx.debug_fold_op(op, [operand], lens, perms=[perm], B=B, fill=FILL, nstatus=B, **kw))
    assert _is_fill(o[0][B * ns * ns:]) and _is_fill(o[1][B * na * na:]) and _is_fill(o[4][2 * B:])
    sets = []
    for b in range(B):
        V, tau = o[2][b * sum(nv):(b + 1) * sum(nv)], o[3][b * sum(ntau):(b + 1) * sum(ntau)]
        sets.append(dict(ss=o[0][b * ns * ns:(b + 1) * ns * ns].reshape(ns, ns), aa=o[1][b * na * na:(b + 1) * na * na].reshape(na, na),
                         V=(V[:nv[0]], V[nv[0]:]), tau=(tau[:ntau[0]], tau[ntau[0]:]), amax=(o[4][2 * b], o[4][2 * b + 1]),
                         status=int(o[5][b])))
    return sets


def _check_storage(s, tau_words, label):
    """reflector storage and tau zeroed to their extents, the word behind each untouched.  (Slices of the arena start at even
    offsets: behind an odd number of reflector words there is a padding word, behind an even number tau's first word, a zero.)"""
    for h in range(2):
        V, tau = s["V"][h], s["tau"][h]
        np_ = tau.size - 67
        assert np.all(_bits(V[:-1]) == 0), "%s: V of class %d" % (label, h)
        assert _is_fill(V[-1:]) if ((np_ + 64) * np_) % 2 else _bits(V[-1:])[0] == 0, "%s: the word behind V of class %d" % (label, h)
        assert np.all(_bits(tau[:np_ + tau_words]) == 0) and _is_fill(tau[np_ + tau_words:]), "%s: tau of class %d" % (label, h)


def _same_set(a, b):
    return (_same_bits(a["ss"], b["ss"]) and _same_bits(a["aa"], b["aa"]) and a["amax"] == b["amax"] and a["status"] == b["status"]
            and all(_same_bits(x, y) for x, y in zip(a["V"] + a["tau"], b["V"] + b["tau"])))


def _tfill_grids(nt):
    yield "mirror_odd" if nt % 2 else "mirror_even", FR.mirror(nt)
    if nt >= 31:
        yield "scattered", FR.involution("scattered", nt)


@gpu
@pytest.mark.parametrize("nt", [2, 3, 31, 32, 33, 70])
def test_temporal_fold_fill(ctx, nt):
    hps = _hp_sets()
    for fam, perm in _tfill_grids(nt):
        t = FR.symmetric_grid(perm)
        alone = {}
        for name, hp in hps.items():
            s = _fill_call(ctx, "temporal_fold_fill", perm, t, 1, hp=_hp([hp]))[0]
            alone[name] = s
            (rs_, ra_), (bs_, ba_), m = _tfill_ref(t, perm, hp)
            _gate("temporal_fold_fill", fam, "nt=%d %s ss" % (nt, name), s["ss"], rs_, bs_)
            _gate("temporal_fold_fill", fam, "nt=%d %s aa" % (nt, name), s["aa"], ra_, ba_)
            assert s["amax"] == (m, m) and s["status"] == 0, (name, s["amax"], m, s["status"])
            _check_storage(s, 66, "temporal fill nt=%d %s" % (nt, name))
        # two sets by value, three by table: each set has the bits of its own call
        for pair in (("usual", "eight"), ("four", "zero_s2")):
            two = _fill_call(ctx, "temporal_fold_fill", perm, t, 2, hp=_hp([hps[p] for p in pair]))
            assert all(_same_set(two[k], alone[p]) for k, p in enumerate(pair)), "two sets by value %s" % (pair,)
        names = ("eight", "m32", "short")                        # (set 0 has the most components)
        tab = _fill_call(ctx, "temporal_fold_fill", perm, t, 3, hp=_hp([hps[p] for p in names]), table=True)
        assert all(_same_set(tab[k], alone[p]) for k, p in enumerate(names)), "three sets by table"


@gpu
@pytest.mark.parametrize("nt", [3, 32, 33, 70])
def test_temporal_fill_is_gram_then_fold(ctx, nt):
    """kernels.hpp: "the same expressions, in the same order, as k_temporal_gram followed by the eigensolver's fold" -- bit for bit,
    for the sets of one component (what gpcsd_gram_temporal evaluates), all entries normal numbers after both scalings"""
    hps = _hp_sets()
    for fam, perm in _tfill_grids(nt):
        t = FR.symmetric_grid(perm)
        for name in ("se_only", "m12", "m32", "m52"):
            (kind,), (ell,), (s2,) = hps[name]
            a = _fill_call(ctx, "temporal_fold_fill", perm, t, 1, hp=_hp([hps[name]]))[0]
            Kt = ctx.gram_temporal(kind, t, t, ell, s2)
            b = _fill_call(ctx, "psd_fold_fill", perm, Kt, 1, s=[0.0], l=[0])[0]
            for blk, h in (("ss", 0), ("aa", 1)):
                x, y = a[blk] * a["amax"][h], b[blk] * b["amax"][h]
                normal = (np.abs(a[blk]) >= 2.0 ** -1000) & (np.abs(b[blk]) >= 2.0 ** -1000)
                ulps = np.abs(_bits(x)[normal].astype(np.int64) - _bits(y)[normal].astype(np.int64))
                print("[fold] fill = gram then fold  %-10s nt=%d %-8s %s: %d of %d entries normal, at most %d ulp apart"
                      % (fam, nt, name, blk, int(normal.sum()), normal.size, int(ulps.max(initial=0))))
                assert normal.sum() >= normal.size // 2 and np.array_equal(_bits(x)[normal], _bits(y)[normal])


@gpu
def test_temporal_fill_non_finite_set(ctx):
    """a non-finite length scale in one of two sets: that set reports 4 and is zeroed, the other keeps its bits"""
    hps = _hp_sets()
    for nt in (33, 70):
        perm = FR.mirror(nt)
        t = FR.symmetric_grid(perm)
        good = _fill_call(ctx, "temporal_fold_fill", perm, t, 1, hp=_hp([hps["usual"]]))[0]
        for bad_ell in (np.nan,):
            bad = ((SE, MAT), (bad_ell, 5.0), (0.5, 0.7))
            for order in ((0, 1), (1, 0)):
                both = _fill_call(ctx, "temporal_fold_fill", perm, t, 2, hp=_hp([(hps["usual"], bad)[k] for k in order]))
                g, b = both[order.index(0)], both[order.index(1)]
                assert _same_set(g, good)
                assert b["status"] == 4 and np.all(_bits(b["ss"]) == 0) and np.all(_bits(b["aa"]) == 0) and b["amax"] == (4.0, 4.0)
                _check_storage(b, 66, "non-finite set")


@gpu
def test_temporal_fill_fp32_mode(ctx):
    hps = _hp_sets()
    perm = FR.mirror(70)
    t = FR.symmetric_grid(perm)
    call = lambda: _fill_call(ctx, "temporal_fold_fill", perm, t, 1, hp=_hp([hps["usual"]]))[0]
    try:
        s64 = call()
        ctx.set_gram_precision(32)
        s32 = call()
    finally:
        ctx.set_gram_precision(64)
    for blk in ("ss", "aa"):
        dev = np.max(np.abs(s32[blk] - s64[blk])) / np.max(np.abs(s64[blk]))
        print("[fold] fp32 temporal fill, block %s: deviation %.2e of the largest entry" % (blk, dev))
        assert 1e-10 < dev < 3e-6, dev
    assert s32["amax"] == s64["amax"] and _same_set(call(), s64)


def _psd_gate(fam, label, s, K, perm, shift):
    (rs_, ra_), (bs_, ba_), scales, margin = _psd_ref(K, perm, shift)
    assert margin > 1e-9, "the case sits on a power of two"
    _gate("psd_fold_fill", fam, label + " ss", s["ss"], rs_, bs_)
    _gate("psd_fold_fill", fam, label + " aa", s["aa"], ra_, ba_)
    assert s["amax"] == scales and s["status"] == 0, (label, s["amax"], scales, s["status"])
    _check_storage(s, 64, "psd fill " + label)


@gpu
@pytest.mark.parametrize("n", [2, 3, 31, 32, 33, 70])
def test_psd_fold_fill(ctx, n):
    for fam, perm in _tfill_grids(n):
        t = FR.symmetric_grid(perm, span=40.0)
        K, K2, K3 = FR.se_gram(t, 20.0), 3.0 * FR.se_gram(t, 7.0), 0.01 * FR.se_gram(t, 45.0)
        # one source, two shifts
        one = _fill_call(ctx, "psd_fold_fill", perm, K, 2, s=[0.0, 1e-8], l=[0])
        for b, sh in enumerate((0.0, 1e-8)):
            _psd_gate(fam, "n=%d one source, shift %g" % (n, sh), one[b], K, perm, sh)
        # two sources further apart than their size (NaN in the gap), two shifts
        sK = n * n + 5
        src = np.full(2 * sK, np.nan)
        src[:n * n], src[sK:sK + n * n] = K.ravel(), K2.ravel()
        two = _fill_call(ctx, "psd_fold_fill", perm, src[:sK + n * n], 2, s=[1e-6, 0.25], l=[sK])
        _psd_gate(fam, "n=%d two sources [0]" % n, two[0], K, perm, 1e-6)
        _psd_gate(fam, "n=%d two sources [1]" % n, two[1], K2, perm, 0.25)
        # three sets by table: the jitters of the sets
        jit = (0.0, 1e-8, 1e-3)
        tab = _fill_call(ctx, "psd_fold_fill", perm, np.stack([K, K2, K3]), 3, l=[n * n], table=True,
                         hp=_hp([((SE,), (1.0,), (1.0,))] * 3, jitter=np.array(jit)))
        for b, (Kb, j) in enumerate(zip((K, K2, K3), jit)):
            _psd_gate(fam, "n=%d table [%d]" % (n, b), tab[b], Kb, perm, j)
        alone = _fill_call(ctx, "psd_fold_fill", perm, K2, 1, s=[1e-8], l=[0])[0]
        assert _same_set(alone, tab[1]), "the table form differs from the plain call"


@gpu
def test_psd_fill_scales_at_the_edges(ctx):
    for n in (32, 33):
        perm = FR.mirror(n)
        fam = "mirror_odd" if n % 2 else "mirror_even"
        # the antisymmetric block is rounding noise: its scale is 2^-30 of the symmetric block's
        K = 3e-6 + 1e-20 * np.random.RandomState(n).standard_normal((n, n))
        assert np.unique(K).size > 16                                    # (the noise survives the rounding to float64: 24 ulp)
        s = _fill_call(ctx, "psd_fold_fill", perm, K, 1, s=[0.0], l=[0])[0]
        _psd_gate(fam, "n=%d noise block" % n, s, K, perm, 0.0)
        assert s["amax"][1] == s["amax"][0] * 2.0 ** -30
        # zero blocks: no entry at all, then the shift alone
        z = _fill_call(ctx, "psd_fold_fill", perm, np.zeros((n, n)), 2, s=[0.0, 1e-8], l=[0])
        assert z[0]["amax"] == (1.0, 1.0) and np.all(_bits(z[0]["ss"]) == 0) and np.all(_bits(z[0]["aa"]) == 0) and z[0]["status"] == 0
        _psd_gate(fam, "n=%d zero matrix, shift 1e-8" % n, z[1], np.zeros((n, n)), perm, 1e-8)
        # a constant matrix: the antisymmetric block is exactly zero
        c = _fill_call(ctx, "psd_fold_fill", perm, np.full((n, n), 0.3), 1, s=[0.0], l=[0])[0]
        _psd_gate(fam, "n=%d constant matrix" % n, c, np.full((n, n), 0.3), perm, 0.0)
        assert np.all(_bits(c["aa"]) == 0)


@gpu
def test_psd_fill_nan_entry(ctx):
    """a NaN in K: status 4, the entries it reaches are zero, everything else keeps its bits"""
    for n in (32, 33):
        perm = FR.mirror(n)
        K = FR.se_gram(FR.symmetric_grid(perm), 20.0)
        clean = _fill_call(ctx, "psd_fold_fill", perm, K, 1, s=[1e-8], l=[0])[0]
        Kn = K.copy()
        Kn[0, 2] = np.nan                                        # (off the diagonals the scales are taken from)
        s = _fill_call(ctx, "psd_fold_fill", perm, Kn, 1, s=[1e-8], l=[0])[0]
        _, (hit_s, hit_a) = FR.fold_rect(np.isnan(Kn), perm, perm)      # where |F| [K is NaN] |F|^T is not zero: the entries it reaches
        assert s["status"] == 4 and s["amax"] == clean["amax"]
        for got, ref, hit in ((s["ss"], clean["ss"], hit_s > 0), (s["aa"], clean["aa"], hit_a > 0)):
            assert hit.sum() == 1 and np.all(_bits(got[hit]) == 0) and np.array_equal(_bits(got[~hit]), _bits(ref[~hit]))
        _check_storage(s, 64, "psd fill with a NaN")


# ---- round trips, as measures in long double of device outputs
@gpu
@pytest.mark.parametrize("n", [3, 32, 33])
def test_round_trip_matrix(ctx, n):
    for fam in _families(n):
        perm = FR.involution(fam, n)
        tb = FR.orbit_tables(perm)
        K = FR.se_gram(FR.symmetric_grid(perm), 20.0)            # commutes with the involution, exactly
        nss, naa = tb["ns"] ** 2, tb["na"] ** 2
        o_ss, o_aa = ctx.debug_fold_op("sym_fold_rect", [K], [nss, max(naa, 1)], perms=[perm, perm], l=[n], fill=0.0)
        Gf = np.concatenate([o_ss, o_aa[:naa]])
        back = ctx.debug_fold_op("sym_unfold_mat", [Gf], [n * n], perms=[perm], l=[nss + naa], fill=FILL)[0].reshape(n, n)
        _, (mss, maa) = FR.fold_rect(K, perm, perm)
        _, through = FR.unfold_mat(gamma(C_FOLD_SS) * mss, gamma(C_FOLD_AA) * maa, perm)     # the fold's bound, unfolded
        _, mag = FR.unfold_mat(o_ss.reshape(tb["ns"], tb["ns"]), o_aa[:naa].reshape(tb["na"], tb["na"]), perm)
        _gate("round trip matrix", fam, "n=%d" % n, back, K.astype(LD), through + gamma(C_UNFOLD_MAT) * mag)


@gpu
@pytest.mark.parametrize("shape", [(5, 3, 17), (6, 65, 33), (4, 5, 70)])
def test_round_trip_data(ctx, shape):
    nx, R, nt = shape
    for fs, ft in [("mirror", "mirror"), ("scattered", "scattered"), ("identity", "mirror")]:
        ps = FR.mirror(nx) if fs == "mirror" else FR.involution(fs, nx)
        pt = FR.mirror(nt) if ft == "mirror" else FR.involution(ft, nt)
        Y = np.random.RandomState(nx * nt).standard_normal(shape)
        Yf = ctx.debug_fold_op("fold_lfp", [Y], [Y.size], perms=[ps, pt], n=[R], fill=FILL)[0]
        # (the fold's output [q][r][b] is the unpadded one-component layout unfold_swap_sum reads)
        back = ctx.debug_fold_op("unfold_swap_sum", [Yf], [Y.size], perms=[ps, pt], n=[R, 1, 0, 0], l=[0, 0], fill=FILL)[0]
        _, fmag = FR.fold_lfp(Y, ps, pt)
        _, through = FR.unfold_pred((gamma(C_FOLD_LFP) * fmag)[:, :, None, :], ps, pt)
        _, mag = FR.unfold_pred(Yf.reshape(nx, R, 1, nt), ps, pt)
        fam = ("mirror_odd" if nt % 2 else "mirror_even") if ft == "mirror" else ft
        _gate("round trip data", fam, "%s x %s (%d, %d, %d)" % (fs, ft, nx, R, nt), back.reshape(nx, nt, R),
              np.swapaxes(Y, 1, 2).astype(LD), through[0] + gamma(C_UNFOLD) * mag[0])


# ---- the entry point itself
@gpu
def test_bad_arguments_are_rejected_and_the_context_stays_usable(ctx):
    n = 17
    perm, K = FR.mirror(n), np.random.RandomState(0).standard_normal((n, n))
    tb = FR.orbit_tables(perm)
    nss, naa = tb["ns"] ** 2, tb["na"] ** 2
    t = FR.symmetric_grid(perm)
    usual = _hp_sets()["usual"]
    _, ss, aa, bss, baa = _rect_case(perm, perm)

    def good(tag):
        o_ss, o_aa = ctx.debug_fold_op("sym_fold_rect", [_rect_case(perm, perm)[0]], [nss, naa], perms=[perm, perm], l=[n], fill=FILL)
        _gate("sym_fold_rect", "mirror_odd", "after %s" % tag, o_ss.reshape(ss.shape), ss, bss)

    fold = lambda K=K, lens=(nss, naa), perms=(perm, perm), ldk=n, **kw: ctx.debug_fold_op("sym_fold_rect", [K], list(lens), perms=list(perms),
                                                                                            l=[ldk], fill=FILL, **kw)
    cycle = np.roll(np.arange(n), 1)
    out_of_range = perm.copy()
    out_of_range[3] = n
    unfold = lambda **kw: ctx.debug_fold_op("unfold_swap_sum", [np.zeros(5 * 2 * n)], [5 * n * 2], perms=[FR.mirror(5), perm], fill=FILL, **kw)
    fills = [B * x for B in (1,) for x in (nss, naa, (tb["ns"] + 64) * tb["ns"] + 1 + (tb["na"] + 64) * tb["na"] + 1, n + 134, 2)]
    bad = {
        "a null operand": lambda: fold(K=None),
        "a short operand": lambda: fold(K=K.ravel()[:-1]),
        "a short output": lambda: fold(lens=(nss - 1, naa)),
        "rows closer than the columns": lambda: fold(ldk=n - 1),
        "a permutation that is a cycle": lambda: fold(perms=(cycle, perm)),
        "a permutation out of range": lambda: fold(perms=(perm, out_of_range)),
        "no permutation": lambda: fold(perms=(perm,)),
        "sets for an op without them": lambda: fold(B=2),
        "a table for an op without one": lambda: fold(table=True),
        "no sets": lambda: fold(B=0),
        "a size of zero": lambda: ctx.debug_fold_op("swap_last2", [K], [n * n], n=[1, 0, n], fill=FILL),
        "a negative size": lambda: ctx.debug_fold_op("swap_last2", [K], [n * n], n=[1, -n, n], fill=FILL),
        "nine components": lambda: ctx.debug_fold_op("swap_last2_sum", [np.zeros(9 * n)], [n], n=[1, 1, n, 9], fill=FILL),
        "lists closer than their blocks": lambda: ctx.debug_fold_op("swap_last2_sum", [np.zeros(2 * n)], [n, 2 * n], n=[1, 1, n, 2], l=[n - 1],
                                                                    with_list=True, fill=FILL),
        "folded sets closer than their blocks": lambda: ctx.debug_fold_op("sym_unfold_mat", [np.zeros(2 * (nss + naa))], [2 * n * n], perms=[perm],
                                                                          l=[nss + naa - 1], B=2, fill=FILL),
        "a padded width below the block": lambda: unfold(n=[2, 1, tb["ns"] - 1, 0], l=[0, 0]),
        "rows closer than their blocks": lambda: unfold(n=[2, 1, 0, 0], l=[0, n - 1]),
        "no trials": lambda: unfold(n=[0, 1, 0, 0], l=[0, 0]),
        "a fill without a pair": lambda: ctx.debug_fold_op("psd_fold_fill", [K], fills, perms=[np.arange(n)], s=[0.0], fill=FILL, nstatus=1),
        "a fill without status words": lambda: ctx.debug_fold_op("psd_fold_fill", [K], fills, perms=[perm], s=[0.0], fill=FILL),
        "three sets by value": lambda: ctx.debug_fold_op("temporal_fold_fill", [t], [3 * x for x in fills], perms=[perm], B=3, hp=_hp([usual] * 3),
                                                         fill=FILL, nstatus=3),
        "a temporal fill without hyper-parameters": lambda: ctx.debug_fold_op("temporal_fold_fill", [t], fills, perms=[perm], fill=FILL, nstatus=1),
        "an unknown kind": lambda: ctx.debug_fold_op("temporal_fold_fill", [t], fills, perms=[perm], hp=_hp([((2,), (1.0,), (1.0,))]), fill=FILL,
                                                     nstatus=1),
        "sources closer than their size": lambda: ctx.debug_fold_op("psd_fold_fill", [np.zeros(2 * n * n)], [2 * x for x in fills], perms=[perm],
                                                                    B=2, s=[0.0, 0.0], l=[n * n - 1], fill=FILL, nstatus=2),
    }
    for tag, call in bad.items():
        with pytest.raises(ValueError):
            call()
        good(tag)
    from gpcsd_amd import _hip
    a = _hip.DebugFoldArgs()
    a.op, a.B = 99, 1
    assert ctx._lib.gpcsd_debug_fold_op(ctx._h, a) == -3 and ctx._lib.gpcsd_debug_fold_op(ctx._h, None) == -3
    good("an unknown op")


@gpu
def test_model_calls_keep_their_bits_after_a_debug_fill():
    """ops 6 and 7 write into the class arenas of the model's own chains: a model call afterwards returns what it returned before"""
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE, GPCSDTemporalCovMatern
    rs = np.random.RandomState(4)
    nx, nt, R = 9, 21, 3
    x, t = np.linspace(0.0, 800.0, nx).reshape(-1, 1), np.linspace(0.0, 20.0, nt).reshape(-1, 1)
    tcl = [GPCSDTemporalCovSE(t), GPCSDTemporalCovMatern(t)]
    for tc, (ell, s2) in zip(tcl, ((6.0, 0.8), (3.0, 0.3))):
        tc.params["ell"]["value"], tc.params["sigma2"]["value"] = ell, s2
    m = GPCSD1D(rs.standard_normal((nx, nt, R)), x, t, a=0.0, b=800.0, ngl=30, temporal_cov_list=tcl)
    m.spatial_cov.params["ell"]["value"] = 150.0
    m.R["value"] = 100.0
    m.sig2n["value"] = 0.05
    ctx = m._context()

    def calls():
        ll = float(m.loglik())
        m.predict(x, t, type="both")
        return ll, m.csd_pred.copy(), m.lfp_pred.copy()

    before = calls()
    for n in (nt, nx, 33):
        perm = FR.mirror(n)
        tg = FR.symmetric_grid(perm)
        _fill_call(ctx, "temporal_fold_fill", perm, tg, 2, hp=_hp([_hp_sets()["usual"], _hp_sets()["eight"]]))
        _fill_call(ctx, "psd_fold_fill", perm, FR.se_gram(tg, 20.0), 2, s=[0.0, 1e-8], l=[0])
        after = calls()
        assert before[0] == after[0] and _same_bits(before[1], after[1]) and _same_bits(before[2], after[2]), "after fills of order %d" % n
