"""The fp64 MFMA GEMM core on its own (gemm_f64.hip: gemm_f64_kernel, through gpcsd_debug_gemm) against an extended-precision
transcription of every epilogue's definition (gemm_ref.py), with the tile configuration forced so that every configuration, operand
layout, epilogue, batch level, tile remap and K-loop exit is reached at the smallest size that reaches it.

Every case runs on two kinds of operands.

Exact operands: A, B integers in [-8, 8]; alpha, D, colscale, rowscale, kscale powers of two in [2^-3, 1]; the initial C small
integers.  Every product and every partial sum in any order is then exactly representable (asserted: every magnitude sum stays
2^12 below 2^53), so the gate is EQUALITY of every stored element and of the EPI_QUAD / EPI_GRAD sums with the reference rounded
to float64 (itself asserted exact) -- no tolerance.  (Equality of finite values is bit equality but for the sign of a zero, which
no epilogue defines.)

Random operands: standard normal, and one family whose rows of A and columns of B are scaled by 10^-6 .. 10^6.  Gate per element
|got - ref| <= (K + 8) u mag_ij with u = 2^-53 and mag = |alpha| (|A||B|)_ij times the absolute epilogue factor, plus |C0| where
C is read: the standard bound of a length-K inner product in any association with eight roundings allowed for the epilogue.  The
EPI_QUAD / EPI_GRAD sums (non-negative terms: D > 0) are gated at (2 K + 8 + n_terms) u sum(mag), n_terms = M N batch.

Layout in every case: leading dimensions minimum + 5, gaps between batch entries, a guard block behind every operand, all NaN:
every result must be finite (edge rows and the K tail are clamped to the last valid element, never read from padding).  C starts
as NaN (or its initial values inside, NaN in the padding); afterwards every element inside M x N is written and everything
else is bit-identical to before.

EPI_DUAL_INIT is declared in enum Epi but has no instantiation and no caller: the launcher refuses it (-3), and that is what is
asserted here.

Measured on the MI355X (119 cases, 14 s), worst ratio of an element's error to its bound, random operands, cfg 1 / 2 / 3 / 5:
plain store 0.22 / 0.20 / 0.20 / 0.19; store + colscale 0.19 / 0.23 / 0.17 / 0.07; store + kscale - / - / 0.18 / 0.07;
div_d 0.16 / 0.20 / 0.14 / 0.07; accum 0.14 / 0.19 / 0.11 / 0.04; grad 0.20 / 0.22 / 0.18 / 0.05; sub 0.30 / 0.31 / 0.26 / 0.16;
lower store 0.17 / - / 0.19 / 0.17, lower sub 0.18 / - / 0.18 / 0.15; dyn 0.13 / 0.20 / 0.12 / 0.14; batched 0.15 / 0.19 / 0.17 / 0.05;
the quad / grad sums against their own bound 1.3e-4 / 3.8e-4 / 3.0e-4 / 9.1e-5.  Every exact-operand case was equal.  No defect found.
"""
import numpy as np
import pytest

import gemm_ref as GR
from gemm_ref import (EPI_STORE, EPI_DIV_D, EPI_QUAD, EPI_ACCUM, EPI_GRAD, EPI_DUAL_INIT, EPI_SUB, CFG_TILE, CFG_BK, LD, U, Packed,
                      pack_vec, same_bits)

CFGS = (1, 2, 3, 5)
LAYOUTS = ((False, False), (True, False), (False, True), (True, True))          # (transA, transB)
KINDS = ("exact", "normal", "spread")
WORST = {}                                         # (cfg, epilogue name) -> worst ratio of an error to its bound so far


def _lid(l):
    return ("T" if l[0] else "N") + ("T" if l[1] else "N")


# ------------------------------------------------------------------------------------------------ the reference itself (no GPU)
def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63


def _int_operands(seed, b2=2, b1=3, M=7, N=5, K=6, rdiv=3):
    rng = np.random.RandomState(seed)
    rD = -(-M // rdiv)
    return dict(A=rng.randint(-8, 9, (b2, b1, M, K)), B=rng.randint(-8, 9, (b2, b1, K, N)), C0=rng.randint(-50, 51, (b2, b1, M, N)),
                D=rng.randint(1, 9, (b2, b1, rD, N)), cs=rng.randint(-4, 5, (b2, b1, N)), rs=rng.randint(-4, 5, (b2, rD)),
                ks=rng.randint(-3, 4, (b2, b1, K)))


@pytest.mark.parametrize("rdiv", [1, 3])
def test_reference_epilogues_against_integer_loops(rdiv):
    """Every epilogue's transcription on integer operands against int64 einsum / explicit loops over the definition."""
    o = _int_operands(11 + rdiv, rdiv=rdiv)
    A, B, C0, D, cs, rs, ks = (o[k].astype(np.int64) for k in ("A", "B", "C0", "D", "cs", "rs", "ks"))
    b2, b1, M, K = A.shape
    N = B.shape[-1]
    acc = np.einsum("zymk,zykn->zymn", A, B)
    Dfull = np.zeros_like(acc)
    for i in range(M):
        Dfull[:, :, i, :] = D[:, :, i // rdiv, :]
    f = lambda x: np.asarray(x, dtype=np.float64)

    def same(got, want):
        return got.dtype == LD and np.array_equal(got, want.astype(LD))

    r = GR.reference(EPI_STORE, f(A), f(B), alpha=-4.0)
    assert same(r.C, -4 * acc) and same(r.C_mag, 4 * np.einsum("zymk,zykn->zymn", np.abs(A), np.abs(B)))
    r = GR.reference(EPI_STORE, f(A), f(B), alpha=2.0, colscale=f(cs))
    assert same(r.C, 2 * acc * cs[:, :, None, :])
    r = GR.reference(EPI_STORE, f(A), f(B), kscale=f(ks))
    assert same(r.C, np.einsum("zymk,zyk,zykn->zymn", A, ks, B))
    r = GR.reference(EPI_ACCUM, f(A), f(B), alpha=-2.0, C0=f(C0))
    assert same(r.C, C0 - 2 * acc)
    r = GR.reference(EPI_SUB, f(A), f(B), C0=f(C0))
    assert same(r.C, C0 - acc) and same(r.C_mag, np.abs(C0) + np.einsum("zymk,zykn->zymn", np.abs(A), np.abs(B)))
    r = GR.reference(EPI_DIV_D, f(A), f(B), D=f(D), rdiv=rdiv)
    assert same(r.C, acc * Dfull)
    r = GR.reference(EPI_QUAD, f(A), f(B), D=f(D), rdiv=rdiv)
    want = np.zeros((b2, 1), dtype=np.int64)
    for z in range(b2):
        for y in range(b1):
            for i in range(M):
                for j in range(N):
                    want[z, 0] += acc[z, y, i, j] ** 2 * D[z, y, i // rdiv, j]
    assert r.C is None and same(r.quad, want) and r.n_terms == b1 * M * N
    r = GR.reference(EPI_GRAD, f(A), f(B), D=f(D), rdiv=rdiv, colscale=f(cs), rowscale=f(rs))
    b = acc * Dfull
    rsfull = np.stack([rs[:, i // rdiv] for i in range(M)], axis=1)             # (b2, M)
    assert same(r.C, b) and same(r.C2, b * cs[:, :, None, :]) and same(r.C3, b * rsfull[:, None, :, None])
    assert same(r.quad, np.stack([np.sum(acc * b, axis=(1, 2, 3)), np.sum(b * b, axis=(1, 2, 3))], axis=1))
    r = GR.reference(EPI_GRAD, f(A), f(B), D=f(D), rdiv=rdiv, rowscale=f(rs), want_c2=False, want_c3=False)
    assert r.C2 is None and r.C3 is None and same(r.C, b)
    with pytest.raises(ValueError):
        GR.reference(EPI_DUAL_INIT, f(A), f(B))


def test_reference_is_more_accurate_than_float64():
    """On random operands the long-double product sits within 2^-60 K |A||B| of the exact (rational) value of a small case."""
    from fractions import Fraction
    rng = np.random.RandomState(3)
    A, B = rng.standard_normal((1, 1, 3, 40)), rng.standard_normal((1, 1, 40, 2))
    r = GR.reference(EPI_STORE, A, B)
    for i in range(3):
        for j in range(2):
            exact = sum(Fraction(float(A[0, 0, i, k])) * Fraction(float(B[0, 0, k, j])) for k in range(40))
            err = abs(Fraction(float(r.C[0, 0, i, j])) + Fraction(float(r.C[0, 0, i, j] - LD(float(r.C[0, 0, i, j])))) - exact)
            assert err <= Fraction(41, 2 ** 63) * Fraction(float(r.C_mag[0, 0, i, j])) * Fraction(1001, 1000)


def test_packed_layout_and_remap_transcriptions():
    X = np.arange(2 * 3 * 4 * 5, dtype=float).reshape(2, 3, 4, 5)
    p = Packed(X, base=2)
    assert p.ld == 12 and p.s1 == 4 * 12 + 7 and p.s2 == 2 * p.s1 + 4 * 12 + 11
    assert np.array_equal(p.take(p.given), X) and np.isnan(p.flat[~p.inside]).all() and p.flat.size == p.idx.max() + 65
    assert p.flat[2 + p.s2 + 2 * p.s1 + 3 * p.ld + 4] == X[1, 2, 3, 4]
    assert Packed(X[:, :1], share1=True).s1 == 0
    # the launcher's XCD remap (gemm_f64_kernel) is a bijection of the grid for any tile counts
    for tm in range(1, 40, 3):
        for tn in range(1, 40):
            total = tm * tn
            if total < 64:
                continue
            q, r = total >> 3, total & 7
            assert sorted((L & 7) * q + min(L & 7, r) + (L >> 3) for L in range(total)) == list(range(total))
    assert GR.auto_cfg(384, 1200, 384) == 5 and GR.auto_cfg(19200, 250, 250) == 2 and GR.auto_cfg(19200, 500, 500) == 3


# ------------------------------------------------------------------------------------------------ cases
class Prob:
    def __init__(self, cfg, epi, M, N, K, ta=False, tb=False, alpha=1.0, batch=1, batch2=1, shareB=False, rdiv=1, colscale=False,
                 kscale=False, c2=True, c3=True, dyn=None, lower=False, lower_shift=0):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.reads_c = epi in (EPI_ACCUM, EPI_SUB)
        self.uses_d = epi in (EPI_DIV_D, EPI_QUAD, EPI_GRAD)
        self.nsum = {EPI_QUAD: 1, EPI_GRAD: 2}.get(epi, 0)

    def __repr__(self):
        return "cfg %d epi %d %dx%dx%d %s%s alpha %g batch %dx%d%s rdiv %d%s%s%s%s" % (
            self.cfg, self.epi, self.M, self.N, self.K, "T" if self.ta else "N", "T" if self.tb else "N", self.alpha, self.batch2,
            self.batch, " shared B" if self.shareB else "", self.rdiv, " colscale" if self.colscale else "",
            " kscale" if self.kscale else "", " dyn %s" % (self.dyn,) if self.dyn is not None else "",
            " lower+%d" % self.lower_shift if self.lower else "")


class Ops:
    pass


def operands(p, kind, seed):
    rng = np.random.RandomState(seed)
    b2, b1, M, N, K = p.batch2, p.batch, p.M, p.N, p.K
    bB = 1 if p.shareB else b1
    rD = -(-M // p.rdiv)
    o = Ops()
    if kind == "exact":
        ri = lambda *s: rng.randint(-8, 9, size=s).astype(np.float64)
        sc = lambda *s: 2.0 ** -rng.randint(0, 4, size=s)
        o.A, o.B, o.C0 = ri(b2, b1, M, K), ri(b2, bB, K, N), rng.randint(-50, 51, size=(b2, b1, M, N)).astype(np.float64)
        o.D, o.cs, o.rs, o.ks = sc(b2, b1, rD, N), sc(b2, b1, N), sc(b2, rD), sc(b2, b1, K)
    else:
        o.A, o.B, o.C0 = rng.standard_normal((b2, b1, M, K)), rng.standard_normal((b2, bB, K, N)), rng.standard_normal((b2, b1, M, N))
        if kind == "spread":                       # elements twelve decades apart
            o.A = o.A * 10.0 ** rng.randint(-6, 7, size=(b2, b1, M, 1))
            o.B = o.B * 10.0 ** rng.randint(-6, 7, size=(b2, bB, 1, N))
        o.D = rng.uniform(0.25, 4.0, (b2, b1, rD, N))                  # reciprocals of positive eigenvalue sums
        o.cs, o.rs, o.ks = rng.standard_normal((b2, b1, N)), rng.standard_normal((b2, rD)), rng.standard_normal((b2, b1, K))
    return o


def entry(p, o, z2, z1):
    """The problem and operands of one batch entry on its own."""
    q = Prob(**{k: getattr(p, k) for k in ("cfg", "epi", "M", "N", "K", "ta", "tb", "alpha", "rdiv", "colscale", "kscale", "c2", "c3",
                                            "lower", "lower_shift")})
    if p.dyn is not None:
        q.dyn = np.asarray(p.dyn).reshape(p.batch2, p.batch)[z2:z2 + 1, z1:z1 + 1]
    e = Ops()
    e.A, e.C0, e.D, e.cs, e.ks = (x[z2:z2 + 1, z1:z1 + 1] for x in (o.A, o.C0, o.D, o.cs, o.ks))
    e.B = o.B[z2:z2 + 1, (0 if p.shareB else z1):(0 if p.shareB else z1) + 1]
    e.rs = o.rs[z2:z2 + 1]
    return q, e


class Run:
    pass


def launch(ctx, p, o, cfg=None):
    r = Run()
    r.pA = Packed(o.A.swapaxes(-1, -2) if p.ta else o.A)
    r.pB = Packed(o.B.swapaxes(-1, -2) if p.tb else o.B, share1=p.shareB)
    kw = dict(transA=p.ta, transB=p.tb, cfg=p.cfg if cfg is None else cfg, epi=p.epi, alpha=p.alpha, batch=p.batch, batch2=p.batch2,
              rdiv=p.rdiv, lda=r.pA.ld, sA=r.pA.s1, sA2=r.pA.s2, ldb=r.pB.ld, sB=r.pB.s1, sB2=r.pB.s2, lower=p.lower,
              lower_shift=p.lower_shift)
    arr = {}
    r.pC = None
    if p.epi != EPI_QUAD:
        r.pC = Packed(o.C0 if p.reads_c else np.full((p.batch2, p.batch, p.M, p.N), np.nan))
        arr["C"] = r.pC.flat
        kw.update(ldc=r.pC.ld, sC=r.pC.s1, sC2=r.pC.s2)
        if p.epi == EPI_GRAD and p.c2:
            arr["C2"] = np.full(r.pC.flat.size, np.nan)
        if p.epi == EPI_GRAD and p.c3:
            arr["C3"] = np.full(r.pC.flat.size, np.nan)
    if p.uses_d:
        r.pD = Packed(o.D, base=3)                 # a column offset into wider rows, as production addresses D
        arr["D"] = r.pD.given
        kw.update(ldd=r.pD.ld, sD=r.pD.s1, sD2=r.pD.s2)
    if p.colscale or p.epi == EPI_GRAD:
        pc = pack_vec(o.cs)
        arr["colscale"] = pc.flat
        kw.update(sColscale=pc.s1, sColscale2=pc.s2)
    if p.epi == EPI_GRAD:
        pr = pack_vec(o.rs)
        arr["rowscale"] = pr.flat
        kw.update(sRowscale2=pr.s2)
    if p.kscale:
        pk = pack_vec(o.ks)
        arr["kscale"] = pk.flat
        kw.update(sKscale=pk.s1, sKscale2=pk.s2)
    if p.nsum:
        r.sQ = p.nsum + 3
        arr["quad"] = np.full((p.batch2 - 1) * r.sQ + p.nsum + 4, np.nan)
        kw.update(sQuad2=r.sQ)
    if p.dyn is not None:
        r.sDyn2 = p.batch + 2
        d = np.zeros((p.batch2, r.sDyn2), dtype=np.int32)
        d[:, :p.batch] = np.asarray(p.dyn).reshape(p.batch2, p.batch)
        arr["dyn"] = d.reshape(-1)
        kw.update(sDyn2=r.sDyn2)
    r.init = {k: (None if v is None else v.copy()) for k, v in arr.items()}
    r.out = ctx.debug_gemm(p.M, p.N, p.K, r.pA.flat, r.pB.flat, **arr, **kw)
    return r


def _gate_matrix(p, what, got, ref, mag, Keff, exact, must, name):
    if not must.any():
        return
    assert np.all(np.isfinite(got[must])), "%r: %s has an element that was not written, or read NaN padding" % (p, what)
    if exact:
        assert float(np.max(mag)) * 2.0 ** 12 < 2.0 ** 53
        ref64 = ref.astype(np.float64)
        assert np.array_equal(ref64.astype(LD), ref), "the reference is not exact in float64: not an exact-operand case"
        bad = must & (got != ref64)
        if bad.any():
            i = tuple(int(v[0]) for v in np.nonzero(bad))
            raise AssertionError("%r: %s differs at %d elements, first at (z2, z1, row, col) = %s: %r for %r"
                                 % (p, what, int(bad.sum()), i, got[i], ref64[i]))
        return
    err = np.abs(got.astype(LD) - ref)
    bound = (Keff + 8) * LD(U) * mag
    assert np.all(bound[must] > 0)
    ratio = float(np.max(err[must] / bound[must]))
    key = (p.cfg, name)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    if ratio > 1.0:
        i = np.unravel_index(int(np.argmax(np.where(must, err / np.where(bound > 0, bound, 1), 0))), err.shape)
        raise AssertionError("%r: %s error %.3e is %.3g times the bound (K + 8) u mag = %.3e at %s"
                             % (p, what, float(err[i]), ratio, float(bound[i]), i))


def check(p, o, r, exact, name=None):
    """Every stored element right, everything else untouched.  Returns the logical outputs {"C", "C2", "C3", "quad"}."""
    name = name or GR.EPI_NAME[p.epi] + ("+kscale" if p.kscale else "") + ("+colscale" if p.colscale and p.epi == EPI_STORE else "")
    shape = (p.batch2, p.batch, p.M, p.N)
    must = np.ones(shape, dtype=bool)
    Keff = np.full(shape, p.K)
    if p.dyn is None:
        ref = GR.reference(p.epi, o.A, o.B, alpha=p.alpha, C0=o.C0, D=o.D, rdiv=p.rdiv, colscale=o.cs if (p.colscale or p.epi == EPI_GRAD) else None,
                           rowscale=o.rs, kscale=o.ks if p.kscale else None, want_c2=p.c2, want_c3=p.c3)
    else:                                          # entry (z2, z1): N = K = dyn, columns >= dyn untouched
        assert p.epi == EPI_STORE and not p.shareB
        ref = GR.Ref()
        ref.C, ref.C_mag = np.zeros(shape, dtype=LD), np.zeros(shape, dtype=LD)
        dyn = np.asarray(p.dyn).reshape(p.batch2, p.batch)
        for z2 in range(p.batch2):
            for z1 in range(p.batch):
                d = int(dyn[z2, z1])
                must[z2, z1, :, d:] = False
                Keff[z2, z1] = d
                if d:
                    e = GR.reference(EPI_STORE, o.A[z2, z1, :, :d], o.B[z2, z1, :d, :d], alpha=p.alpha)
                    ref.C[z2, z1, :, :d], ref.C_mag[z2, z1, :, :d] = e.C, e.C_mag
    got = {"C": None, "C2": None, "C3": None, "quad": None}
    for k, rf, mg in (("C", ref.C, ref.C_mag), ("C2", ref.C2, ref.C2_mag), ("C3", ref.C3, ref.C3_mag)):
        buf = r.out[k]
        if rf is None:
            assert buf is None or same_bits(buf, r.init[k]), "%r: %s is not an output of this epilogue and was written" % (p, k)
            continue
        got[k] = r.pC.take(buf)
        if p.lower:
            got["skipped"] = _check_lower(p, k, got[k], rf, mg, r.pC.take(r.init[k]), exact, name)
            written = np.ones(shape, dtype=bool)
        else:
            _gate_matrix(p, k, got[k], rf, mg, Keff, exact, must, name)
            written = must
        outside = np.ones(buf.size, dtype=bool)
        outside[r.pC.idx[written]] = False
        assert same_bits(buf[outside], r.init[k][outside]), "%r: %s was written outside its %d x %d elements" % (p, k, p.M, p.N)
    if p.nsum:
        q = r.out["quad"]
        at = (np.arange(p.batch2) * r.sQ)[:, None] + np.arange(p.nsum)[None, :]
        got["quad"] = q[at]
        outside = np.ones(q.size, dtype=bool)
        outside[at] = False
        assert same_bits(q[outside], r.init["quad"][outside]), "%r: quad_out was written outside its sums" % (p,)
        assert np.all(np.isfinite(got["quad"])), "%r: a sum is not finite" % (p,)
        if exact:
            assert float(np.max(ref.quad_mag)) * 2.0 ** 12 < 2.0 ** 53
            assert np.array_equal(ref.quad.astype(np.float64).astype(LD), ref.quad)
            assert np.array_equal(got["quad"], ref.quad.astype(np.float64)), \
                "%r: sums %r, exact %r" % (p, got["quad"], ref.quad.astype(np.float64))
        else:
            err = np.abs(got["quad"].astype(LD) - ref.quad)
            bound = (2 * p.K + 8 + ref.n_terms) * LD(U) * ref.quad_mag
            ratio = float(np.max(err / bound))
            key = (p.cfg, name + " sums")
            WORST[key] = max(WORST.get(key, 0.0), ratio)
            assert ratio <= 1.0, "%r: sums off by %.3g times the bound" % (p, ratio)
    else:
        assert r.out["quad"] is None
    return got


def _check_lower(p, what, got, ref, mag, init, exact, name):
    """Elements with col <= row + lower_shift are right; every tile is either right as a whole or untouched as a whole."""
    T = CFG_TILE[p.cfg]
    rows, cols = np.arange(p.M)[:, None], np.arange(p.N)[None, :]
    must = np.broadcast_to(cols <= rows + p.lower_shift, got.shape)
    _gate_matrix(p, what, got, ref, mag, np.full(got.shape, p.K), exact, must, name)
    if exact:
        right = got == ref.astype(np.float64)
    else:
        right = np.abs(got.astype(LD) - ref) <= (p.K + 8) * LD(U) * mag
    untouched = np.ascontiguousarray(got).view(np.uint64) == np.ascontiguousarray(init).view(np.uint64)
    skipped = 0
    for z in np.ndindex(got.shape[:2]):
        for i in range(0, p.M, T):
            for j in range(0, p.N, T):
                t = z + (slice(i, i + T), slice(j, j + T))
                ok_r, ok_u = bool(right[t].all()), bool(untouched[t].all())
                assert ok_r or ok_u, "%r: %s tile (%d, %d) of entry %s is neither right nor untouched as a whole" % (p, what, i // T, j // T, z)
                skipped += ok_u and not ok_r
    return skipped


def run_checked(ctx, p, kind, seed, name=None):
    o = operands(p, kind, seed)
    r = launch(ctx, p, o)
    return o, r, check(p, o, r, kind == "exact", name)


def report(prefix, cfgs=CFGS):
    for key in sorted(WORST):
        if key[0] in cfgs and key[1].startswith(prefix):
            print("[gemm] cfg %d %-16s worst error / bound so far %.3g" % (key[0], key[1], WORST[key]))


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx():
    from gpcsd_amd import _hip
    return _hip.default_context()


def _edge_shapes(cfg):
    T, BK = CFG_TILE[cfg], CFG_BK[cfg]
    MN = [(1, 1), (17, T - 1), (T, T + 1), (T + 1, 17), (2 * T + 3, T)]
    Ks = [1, 3, BK - 1, BK, BK + 1, 2 * BK, 2 * BK + 2, 3 * BK + 1, 4 * BK, 5 * BK + 3]
    return MN, Ks


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
@pytest.mark.parametrize("cfg", CFGS)
def test_edges_plain_store(ctx, cfg, layout):
    """1. Tile edges and every exit of the K loop (nk = 1, 2, 3, the steady-state loop with even and odd nfull, every last_steps,
    the all-full last tile), every configuration x layout."""
    MN, Ks = _edge_shapes(cfg)
    seed = 1000 * cfg
    for M, N in MN:
        for K in Ks:
            for kind in KINDS:
                seed += 1
                run_checked(ctx, Prob(cfg, EPI_STORE, M, N, K, ta=layout[0], tb=layout[1]), kind, seed)
    report("store", (cfg,))


EPI_VARIANTS = [("div_d", EPI_DIV_D, {}), ("quad", EPI_QUAD, {}), ("accum-1", EPI_ACCUM, dict(alpha=-1.0)),
                ("accum.5", EPI_ACCUM, dict(alpha=0.5)), ("grad", EPI_GRAD, {}), ("grad-noC2C3", EPI_GRAD, dict(c2=False, c3=False)),
                ("sub", EPI_SUB, {})]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", EPI_VARIANTS, ids=[v[0] for v in EPI_VARIANTS])
@pytest.mark.parametrize("cfg", CFGS)
def test_epilogues(ctx, cfg, variant):
    """2. Every epilogue the launcher has, at a shape with partial tiles in both directions and at one with a partial K tile only;
    rdiv 1 and 3 (M no multiple of 3); D with a column offset."""
    vname, epi, extra = variant
    T, BK = CFG_TILE[cfg], CFG_BK[cfg]
    seed = 100000 + 1000 * cfg + 37 * epi
    layouts = ((False, True),) if epi == EPI_SUB else LAYOUTS
    for M, N, K in ((T + 1, 2 * T + 3, 2 * BK + 2), (2 * T + 3, 17, BK - 1)):
        # (B + 1 is a multiple of 3 for B = 128 and 32: there rdiv = 4 is added, so that M is never only a multiple of rdiv)
        for rdiv in (((1, 3) if M % 3 else (1, 3, 4)) if epi in (EPI_DIV_D, EPI_QUAD, EPI_GRAD) else (1,)):
            assert rdiv == 1 or M % rdiv or M % 4
            for ta, tb in layouts:
                for kind in KINDS if (ta, tb) == layouts[0] else KINDS[:2]:
                    seed += 1
                    run_checked(ctx, Prob(cfg, epi, M, N, K, ta=ta, tb=tb, rdiv=rdiv, **extra), kind, seed)
    report(GR.EPI_NAME[epi], (cfg,))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [(True, False), (False, True)], ids=_lid)
@pytest.mark.parametrize("cfg", (3, 5))
def test_kscale(ctx, cfg, layout):
    """3. A scaled along K on its way to LDS: both supported layouts, over both batch levels; bit-identical to the plain product
    of a pre-scaled copy of A; a request for configuration 2 (or 1) runs as 3."""
    T, BK = CFG_TILE[cfg], CFG_BK[cfg]
    seed = 200000 + 1000 * cfg
    for M, N, K in ((T + 1, 2 * T + 3, 2 * BK + 2), (2 * T + 3, 17, BK - 1), (17, T + 1, 5 * BK + 3)):
        for batch, batch2 in ((1, 1), (3, 1), (2, 2)):
            for kind in KINDS:
                seed += 1
                p = Prob(cfg, EPI_STORE, M, N, K, ta=layout[0], tb=layout[1], kscale=True, batch=batch, batch2=batch2, alpha=0.5)
                o, r, got = run_checked(ctx, p, kind, seed)
                q = Prob(cfg, EPI_STORE, M, N, K, ta=layout[0], tb=layout[1], batch=batch, batch2=batch2, alpha=0.5)
                o2 = operands(p, kind, seed)
                o2.A = o.A * o.ks[:, :, None, :]                      # one rounded product per element
                r2 = launch(ctx, q, o2)
                assert same_bits(r2.out["C"], r.out["C"]), "%r: differs in its bits from the product of a pre-scaled copy of A" % (p,)
                if cfg == 3:
                    for other in (1, 2):
                        r3 = launch(ctx, p, o, cfg=other)
                        assert same_bits(r3.out["C"], r.out["C"]), "%r: requested as configuration %d it must run as 3" % (p, other)
    report("store+kscale", (cfg,))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_colscale_on_the_plain_store(ctx, cfg):
    """4. C = alpha * acc * colscale[col], colscale with a batch stride on both levels."""
    T, BK = CFG_TILE[cfg], CFG_BK[cfg]
    seed = 300000 + 1000 * cfg
    for M, N, K in ((T + 1, 2 * T + 3, 2 * BK + 2), (2 * T + 3, 17, BK - 1)):
        for batch, batch2 in ((1, 1), (3, 1), (2, 2)):
            for ta, tb in ((False, False), (True, True)):
                for kind in KINDS:
                    seed += 1
                    run_checked(ctx, Prob(cfg, EPI_STORE, M, N, K, ta=ta, tb=tb, colscale=True, batch=batch, batch2=batch2, alpha=0.25),
                                kind, seed)
    report("store+colscale", (cfg,))


BATCH_CASES = [("shared-B", EPI_STORE, dict(batch=3, shareB=True)), ("batch3", EPI_STORE, dict(batch=3)),
               ("2x2", EPI_STORE, dict(batch=2, batch2=2)), ("2x2-grad", EPI_GRAD, dict(batch=2, batch2=2, rdiv=3)),
               ("2x2-quad", EPI_QUAD, dict(batch=2, batch2=2, rdiv=3)), ("2x3-accum", EPI_ACCUM, dict(batch=3, batch2=2, alpha=-1.0)),
               ("2x2-div_d", EPI_DIV_D, dict(batch=2, batch2=2))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
@pytest.mark.parametrize("cfg", CFGS)
def test_batches(ctx, cfg, case):
    """5. Both batch levels with every stride set; every entry of a batched launch is bit-identical to the same entry launched alone
    at the same configuration; EPI_QUAD / EPI_GRAD: one sum (pair) per outer entry at sQuad2."""
    _, epi, extra = case
    T, BK = CFG_TILE[cfg], CFG_BK[cfg]
    seed = 400000 + 1000 * cfg + 37 * epi
    for M, N, K in ((T + 1, T + 3, 2 * BK + 2), (T + 3, 17, BK - 1)):
        for kind in KINDS[:2]:
            seed += 1
            p = Prob(cfg, epi, M, N, K, **extra)
            o, r, got = run_checked(ctx, p, kind, seed, name="batched " + GR.EPI_NAME[epi])
            if epi == EPI_QUAD:
                continue                                   # (a sum over the inner entries has no single-entry counterpart)
            for z2 in range(p.batch2):
                for z1 in range(p.batch):
                    q, e = entry(p, o, z2, z1)
                    alone = check(q, e, launch(ctx, q, e), kind == "exact", name="batched " + GR.EPI_NAME[epi])
                    for k in ("C", "C2", "C3"):
                        if got[k] is not None:
                            assert same_bits(alone[k][0, 0], got[k][z2, z1]), \
                                "%r: %s of entry (%d, %d) differs in its bits from the entry launched alone" % (p, k, z2, z1)
    report("batched", (cfg,))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_quad_sums_of_outer_entries_match_the_entries_alone(ctx, cfg):
    """5. EPI_QUAD / EPI_GRAD with batch2: the sums of outer entry z2 are bit-identical to that outer entry launched alone (the same
    tiles in the same order through the same two-stage reduce: what a hyper-parameter set relies on)."""
    T, BK = CFG_TILE[cfg], CFG_BK[cfg]
    seed = 450000 + 1000 * cfg
    for epi in (EPI_QUAD, EPI_GRAD):
        for kind in KINDS[:2]:
            seed += 1
            p = Prob(cfg, epi, T + 3, T + 1, 2 * BK + 2, batch=2, batch2=3, rdiv=3)
            o, r, got = run_checked(ctx, p, kind, seed, name="batched " + GR.EPI_NAME[epi])
            for z2 in range(p.batch2):
                q = Prob(cfg, epi, p.M, p.N, p.K, batch=2, rdiv=3)
                e = Ops()
                e.A, e.B, e.C0, e.D, e.cs, e.ks, e.rs = (x[z2:z2 + 1] for x in (o.A, o.B, o.C0, o.D, o.cs, o.ks, o.rs))
                alone = check(q, e, launch(ctx, q, e), kind == "exact", name="batched " + GR.EPI_NAME[epi])
                assert same_bits(alone["quad"][0], got["quad"][z2]), "%r: sums of outer entry %d differ from the entry alone" % (p, z2)


REMAP_CASES = [("cfg5-257x257", 5, 257, 257, 70, {}), ("cfg5-70x600", 5, 70, 600, 70, {}),
               ("cfg5-70x600-batch2", 5, 70, 600, 70, dict(batch=2, shareB=True)), ("cfg1-2x3-tiles-batch11", 1, 200, 300, 40, dict(batch=11)),
               ("cfg2-3x3-tiles-2x4", 2, 130, 190, 21, dict(batch=4, batch2=2)), ("cfg5-quad-9x9", 5, 259, 270, 70, dict(epi=EPI_QUAD)),
               ("cfg3-grad-2x3x11", 3, 100, 150, 35, dict(epi=EPI_GRAD, batch=11, rdiv=3))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", REMAP_CASES, ids=[c[0] for c in REMAP_CASES])
def test_tile_remaps(ctx, case):
    """6. Grids of 64 tiles and more take the per-XCD remap; tile_m fastest and the grouped sweep: every element written once and
    right (and, for the sums, every tile's partial counted once)."""
    _, cfg, M, N, K, extra = case
    extra = dict(extra)
    epi = extra.pop("epi", EPI_STORE)
    T = CFG_TILE[cfg]
    assert -(-M // T) * -(-N // T) * extra.get("batch", 1) * extra.get("batch2", 1) >= 64 or "70x600" == case[0][5:]
    for i, kind in enumerate(KINDS[:2]):
        run_checked(ctx, Prob(cfg, epi, M, N, K, **extra), kind, 500000 + 10 * cfg + i, name="remap " + GR.EPI_NAME[epi])
    report("remap", (cfg,))


@pytest.mark.gpu
def test_tile_remap_with_a_short_last_group(ctx):
    """6. Configuration 3 at 520 x 300 x 1000, two entries sharing B: 90 tiles, n_group = 4 < tn = 5, so the grouped sweep has a
    short last group.  Exact operands only, reference float64 NumPy (exact on these operands: every sum is an integer < 2^53)."""
    p = Prob(3, EPI_STORE, 520, 300, 1000, batch=2, shareB=True)
    assert (2 << 20) // (p.K * 64 * 8) == 4 and -(-p.N // 64) == 5 and -(-p.M // 64) * 5 * 2 == 90
    o = operands(p, "exact", 77)
    r = launch(ctx, p, o)
    want = np.matmul(o.A, o.B)
    assert float(np.max(np.matmul(np.abs(o.A), np.abs(o.B)))) < 2.0 ** 53
    assert np.array_equal(want, np.matmul(o.A.astype(np.int64), o.B.astype(np.int64)).astype(np.float64))
    got = r.pC.take(r.out["C"])
    assert np.all(np.isfinite(got)) and np.array_equal(got, want), "%d elements differ" % int(np.sum(got != want))
    assert same_bits(r.out["C"][~r.pC.inside], r.init["C"][~r.pC.inside])


LOWER_CASES = [(1, 9), (3, 9), (5, 9), (5, 11), (3, 3), (5, 3), (1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("epi", (EPI_STORE, EPI_SUB), ids=["store", "sub"])
@pytest.mark.parametrize("case", LOWER_CASES, ids=["cfg%d-%dx%d" % (c[0], c[1], c[1]) for c in LOWER_CASES])
def test_lower(ctx, case, epi):
    """7. Symmetric updates that want the lower triangle only: tiles strictly above the (shifted) diagonal are skipped, whole tiles
    and nothing finer; 9 x 9 tiles and more engage the second remap."""
    cfg, nt = case
    T, K = CFG_TILE[cfg], 2 * CFG_BK[cfg] + 2 if case[1] == 3 else 19
    N = (nt - 1) * T + 7
    for i, shift in enumerate((0, T // 2, T + 5)):
        for j, kind in enumerate(KINDS[:2]):
            p = Prob(cfg, epi, N - shift, N, K, ta=False, tb=True, lower=True, lower_shift=shift)
            if nt >= 9:
                assert -(-p.M // T) * nt >= 64
            o = operands(p, kind, 600000 + 100 * cfg + 10 * i + j)
            r = launch(ctx, p, o)
            got = check(p, o, r, kind == "exact", name="lower " + GR.EPI_NAME[epi])
            above = sum(j * T > i * T + T - 1 + shift for i in range(-(-p.M // T)) for j in range(nt))
            assert above > 0 or nt == 3
            if epi == EPI_STORE:                           # (NaN before: a tile that ran cannot pass for untouched)
                assert got["skipped"] == above, "%r: %d tiles were skipped, %d lie strictly above the diagonal" % (p, got["skipped"], above)
    report("lower", (cfg,))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [(False, False), (False, True), (True, False)], ids=_lid)
@pytest.mark.parametrize("cfg", CFGS)
def test_dyn(ctx, cfg, layout):
    """8. Sizes decided on the device: entry z runs with N = K = dyn[z]; columns below dyn equal the product of that size, columns
    from dyn on are untouched; dyn per inner entry and, at sDyn2, per outer entry."""
    T, BK = CFG_TILE[cfg], CFG_BK[cfg]
    N = max(T + 7, BK + 5)
    vals = [1, BK, BK + 1, N - 1, N, 0, T]
    seed = 700000 + 1000 * cfg
    for batch2, dyn in ((1, vals), (2, vals[:5] + vals[4:1:-1] + [3, 1])):
        for kind in KINDS:
            seed += 1
            p = Prob(cfg, EPI_STORE, 37, N, N, ta=layout[0], tb=layout[1], batch=len(dyn) // batch2, batch2=batch2, dyn=dyn, alpha=0.5)
            run_checked(ctx, p, kind, seed, name="dyn store")
    report("dyn", (cfg,))


@pytest.mark.gpu
def test_refusals(ctx):
    """9. What the launcher and the debug entry refuse, each with -3 (ValueError) -- a leading dimension at the capacity limit with
    ERR_CAPACITY -- and after each refusal a correct call on the same context succeeds."""
    from gpcsd_amd import _hip
    M, N, K = 33, 20, 17
    rng = np.random.RandomState(5)
    A, B, C = rng.randint(-8, 9, M * K).astype(float), rng.randint(-8, 9, K * N).astype(float), np.zeros(M * N)
    good = dict(lda=K, ldb=N, ldc=N, cfg=5)
    want = A.reshape(M, K) @ B.reshape(K, N)

    def ok():
        assert np.array_equal(ctx.debug_gemm(M, N, K, A, B, C, **good)["C"].reshape(M, N), want)

    def refused(exc, *args, **kw):
        with pytest.raises(exc):
            ctx.debug_gemm(*args, **kw)
        ok()

    ok()
    sq = np.ones(K * K)
    for ta, tb in ((False, False), (True, False), (True, True)):                    # EPI_SUB in another layout
        refused(ValueError, K, K, K, sq, sq, sq, lda=K, ldb=K, ldc=K, cfg=5, epi=EPI_SUB, transA=ta, transB=tb)
    ks = np.ones(K)
    for ta, tb in ((False, False), (True, True)):                                   # kscale with both or neither operand transposed
        refused(ValueError, K, K, K, sq, sq, sq, kscale=ks, lda=K, ldb=K, ldc=K, cfg=5, transA=ta, transB=tb)
    refused(ValueError, K, K, K, sq, sq, sq, kscale=ks, lda=K, ldb=K, ldc=K, cfg=5, transA=True, epi=EPI_ACCUM)   # ... a non-store epilogue
    for epi in (5, EPI_DUAL_INIT, 8, -1, 99):                                       # no such epilogue (6 is declared, not instantiated)
        refused(ValueError, M, N, K, A, B, C, epi=epi, **good)
    refused(ValueError, 0, N, K, A, B, C, **good)
    refused(ValueError, M, 0, K, A, B, C, **good)
    refused(ValueError, M, N, 0, A, B, C, **good)
    refused(ValueError, M, N, K, A, B, C, lda=K + 1, ldb=N, ldc=N, cfg=5)           # strides that address past the buffer
    refused(ValueError, M, N, K, A, B, C, lda=K, ldb=N + 1, ldc=N, cfg=5)
    refused(ValueError, M, N, K, A, B, C, lda=K, ldb=N, ldc=N + 1, cfg=5)
    refused(ValueError, M, N, K, A, B, C, lda=K - 1, ldb=N, ldc=N, cfg=5)           # ... below the minimum
    refused(ValueError, M, N, K, A, B, C, batch=2, sA=1, sB=0, sC=0, **good)
    refused(ValueError, M, N, K, A, B, C, batch2=2, sB2=1, **good)
    refused(ValueError, M, N, K, A, B, C, batch=2, sC=-1, **good)
    refused(ValueError, M, N, K, A, B, C, transA=True, **good)                      # (K, M) storage needs lda >= M
    D = np.ones(M * N)
    refused(ValueError, M, N, K, A, B, C, D=D, epi=EPI_DIV_D, ldd=N + 1, **good)
    refused(ValueError, M, N, K, A, B, C, D=D[:11 * N - 1], epi=EPI_DIV_D, ldd=N, rdiv=3, **good)
    refused(ValueError, M, N, K, A, B, C, epi=EPI_DIV_D, ldd=N, **good)             # no D
    refused(ValueError, M, N, K, A, B, C, D=D, epi=EPI_QUAD, ldd=N, **good)         # no quad_out
    refused(ValueError, M, N, K, A, B, C, D=D, epi=EPI_GRAD, ldd=N, quad=np.zeros(2), **good)      # no rowscale
    refused(ValueError, M, N, K, A, B, C, D=D, epi=EPI_GRAD, ldd=N, quad=np.zeros(1), rowscale=np.ones(M), **good)
    refused(ValueError, M, N, K, A, B, C, colscale=np.ones(N - 1), **good)
    refused(ValueError, M, N, K, A, B, C, dyn=[K + 1], **good)
    refused(ValueError, M, N, K, A, B, C, dyn=[1], batch=2, **good)
    refused(ValueError, M, N, K, A, B, C, batch=70000, **good)
    assert np.array_equal(ctx.debug_gemm(M, N, K, A, B, C, D=D[:11 * N], epi=EPI_DIV_D, ldd=N, rdiv=3, **good)["C"].reshape(M, N), want)
    # a leading dimension at the capacity limit of one operand row: one row of A with lda = 2^22, one row of B (N, K) likewise
    refused(_hip.GPCSDCapacityError, 1, N, K, A[:K], B, C, lda=1 << 22, ldb=N, ldc=N, cfg=5)
    refused(_hip.GPCSDCapacityError, M, 1, K, A, B[:K], C, lda=K, ldb=1 << 22, ldc=1, cfg=5, transB=True)
    refused(_hip.GPCSDCapacityError, M, N, 1, A[:M], B[:N], C, lda=_hip.MAX_GEMM_LD_KMAJOR, ldb=N, ldc=N, cfg=5, transA=True)
    with pytest.raises(TypeError):
        ctx.debug_gemm(M, N, K, A, B, C, nA=5, **good)
