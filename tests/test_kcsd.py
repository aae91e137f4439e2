"""Kernel CSD in one dimension (gpcsd_amd/kcsd.py, csrc/kcsd.hip) against its dense long-double statement (tests/kcsd_ref.py).

CPU: the surface, argument checks, the truncation of the two-panel rule, closed-form leave-one-out against explicit refits.
GPU: the basis kernel against the long-double rule at the same nodes (rounding alone), the cross-validation kernel against the
long-double closed form on the same float64 operands, bitwise properties, and KCSD1D against explicit refits.

Observed on MI355X (every test prints its figure before it asserts, run with -s): potential basis at most 0.107 of its
rounding bound, source basis 0.391, cross-validation table 0.060 of its gate (n = 2: 0.055, 3: 0.060, 17: 0.020, 24: 0.037, 65: 0.013,
130: 0.007, 257: 0.005); model level cv_error 2.3e-12, values() 1.4e-13, values('POT') 4.7e-14 against the 1e-6 gate.
"""
import functools
import os
import re

import numpy as np
import pytest

import kcsd_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = KR.LD


# ------------------------------------------------------------------------------------------------ the two model-level cases
def _forward(x, z, csd, R, sigma=1.0):
    """potentials of a CSD profile on the grid z through the project's 1D forward model at cylinder radius R"""
    r = x[:, None] - z[None, :]
    return (np.sqrt(r * r + R * R) - np.abs(r)) @ csd * (z[1] - z[0]) / (2.0 * sigma)


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "A":
        n, M, T = 24, 64, 40
        x = 100.0 * np.arange(n)
    else:
        n, M, T = 17, 65, 33
        x = 100.0 * np.arange(n) + np.random.default_rng(0).uniform(-30.0, 30.0, n)
    lo, hi = x.min(), x.max()
    z = np.linspace(lo, hi, 401)
    t = np.arange(T) / T
    c1, c2, w = lo + 0.3 * (hi - lo), lo + 0.7 * (hi - lo), 0.08 * (hi - lo)
    csd = (np.exp(-0.5 * ((z - c1) / w) ** 2)[:, None] * np.sin(2 * np.pi * 2 * t)[None, :]
           - 0.7 * np.exp(-0.5 * ((z - c2) / w) ** 2)[:, None] * np.cos(2 * np.pi * 3 * t)[None, :])
    V = _forward(x, z, csd, 250.0)
    V = V + 0.05 * V.std() * np.random.default_rng(1).standard_normal(V.shape)
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return dict(n=n, M=M, T=T, x=x, V=V, h=200.0, Rs=(150.0, 300.0, 600.0), lambdas=(1e-2, 1.0, 1e2, 1e4))


def _model(name, pots=None):
    from gpcsd_amd.kcsd import KCSD1D
    c = _case(name)
    return KCSD1D(c["x"], c["V"] if pots is None else pots, h=c["h"], n_src_init=c["M"])


@functools.lru_cache(maxsize=None)
def _case_ref(name):
    """long-double kernels per R, the table by explicit refits and by the closed form, the selected pair and its estimates"""
    c = _case(name)
    m = _model(name)
    gx, gw = KR.gauss_legendre(48)
    KK = [KR.kernels(m.src_x, c["x"], m.estm_x, R, c["h"], 1.0, gx, gw) for R in c["Rs"]]
    refit = np.array([[KR.cv_refit(K, c["V"], lam) for lam in c["lambdas"]] for K, _ in KK])
    closed = np.array([[KR.cv_closed_dense(K, c["V"], lam) for lam in c["lambdas"]] for K, _ in KK])
    ri, li = np.unravel_index(np.argmin(refit), refit.shape)
    csd, pot = KR.estimate(KK[ri][0], KK[ri][1], c["V"], c["lambdas"][li])
    A = (KK[ri][0] + LD(c["lambdas"][li]) * np.eye(c["n"])).astype(np.float64)
    return dict(refit=refit, closed=closed, best=(int(ri), int(li)), csd=csd, pot=pot, cond=float(np.linalg.cond(A)))


# ------------------------------------------------------------------------------------------------ CPU
def test_surface_exists_and_fails_loudly_without_a_gpu():
    import torch
    from gpcsd_amd import build, _hip, kcsd
    for fn in ("kcsd_basis_1d", "kcsd_cv", "kcsd_cross_validate", "kcsd_estimate"):
        assert callable(getattr(_hip.Context, fn, None))
    for fn in ("cross_validate", "values"):
        assert callable(getattr(kcsd.KCSD1D, fn, None))
    assert "kcsd.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _hip.load_library()
    src = open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read()
    for fn in ("gpcsd_kcsd_basis_1d", "gpcsd_kcsd_cv", "gpcsd_kcsd_cross_validate", "gpcsd_kcsd_estimate"):
        decl = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % fn, src, flags=re.S)
        assert decl, "%s is not declared under a comment" % fn
        assert "sim_from_gp_1D.py:" in decl.group(1), "%s does not cite the script lines it replaces" % fn
        assert fn in _hip.SIGNATURES and hasattr(lib, fn)
    m = _model("A")
    assert m.estm_x.shape == (101,) and m.estm_x[0] == 0.0 and np.isclose(m.estm_x[-1], 2300.0)
    assert m.src_x.shape == (64,) and m.src_x[0] == 0.0 and m.src_x[-1] == 2300.0
    assert m.R == 0.23 and m.lambd == 0.0 and m.ngl == 48 and np.isclose(m.gdx, 23.0)
    assert np.array_equal(kcsd.DEFAULT_LAMBDAS, np.logspace(1, -15, 25))
    ext = kcsd.KCSD1D(np.arange(4.0), np.zeros((4, 3, 2)), ext_x=2.0, n_src_init=5, gdx=0.5, xmin=-1.0, xmax=4.0)
    assert ext.src_x[0] == -3.0 and ext.src_x[-1] == 6.0 and ext.estm_x[0] == -1.0 and ext.estm_x[-1] == 4.0 and ext.estm_x.size == 11
    assert ext.pots.shape == (4, 6)
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipUnavailable):
            m.cross_validate(Rs=[100.0], lambdas=[1.0])
        with pytest.raises(_hip.HipUnavailable):
            m.values()


def test_host_side_argument_checks():
    from gpcsd_amd.kcsd import KCSD1D
    x, V = np.arange(5.0), np.ones((5, 7))
    with pytest.raises(NotImplementedError):
        KCSD1D(x, V, src_type='step')
    for kw in (dict(sigma=0.0), dict(h=-1.0), dict(R_init=0.0), dict(lambd=-1e-3), dict(n_src_init=0), dict(ngl=1), dict(gdx=0.0),
               dict(ext_x=-1.0), dict(h=np.nan), dict(xmin=3.0, xmax=1.0)):
        with pytest.raises(ValueError):
            KCSD1D(x, V, **kw)
    with pytest.raises(ValueError):
        KCSD1D(x, np.ones((4, 7)))
    with pytest.raises(ValueError):
        KCSD1D(x, np.ones(5))
    with pytest.raises(ValueError):
        KCSD1D(x, np.where(np.arange(35).reshape(5, 7) == 3, np.inf, 1.0))
    m = KCSD1D(x, V)
    for kw in (dict(Rs=[1.0, -2.0]), dict(Rs=[]), dict(lambdas=[-1.0]), dict(lambdas=[np.nan]), dict(lambdas=[])):
        with pytest.raises(ValueError):
            m.cross_validate(**kw)
    with pytest.raises(ValueError):
        m.values('LFP')


# twice the truncation figures measured for 48 nodes per panel (relative to the largest entry); h / R = 1 and 10 sit at rounding level
_TRUNCATION = {0.05: 2 * 1.3e-13, 0.1: 2 * 7.7e-14, 1.0: 2 * 1e-14, 10.0: 2 * 1e-14}


@pytest.mark.parametrize("ratio", sorted(_TRUNCATION))
def test_truncation_of_the_two_panel_rule(ratio):
    R = 300.0
    d = np.concatenate([np.linspace(-3 * R, 3 * R, 241), [0.0, R, -R, R * (1 + 1e-12), 1e-9]])
    gx, gw = KR.gauss_legendre(48)
    got = KR.potential_basis([0.0], d, R, ratio * R, 1.0, gx, gw, dtype=np.float64)[0]
    ref = KR.potential_basis([0.0], d, R, ratio * R, 1.0, *KR.gauss_legendre_ld(400))[0]
    err = float(np.max(np.abs(got.astype(LD) - ref)) / np.max(np.abs(ref)))
    print("h/R = %g: 48 nodes per panel (float64) against 400 (long double): %.2e of the largest entry" % (ratio, err))
    assert err <= _TRUNCATION[ratio]


@pytest.mark.parametrize("name", ["A", "B"])
def test_closed_form_equals_explicit_refits_in_the_reference(name):
    r = _case_ref(name)
    rel = float(np.max(np.abs(r["closed"] - r["refit"]) / r["refit"]))
    print("case %s: closed form against refits %.2e, cond(A) %.3g, selected %s" % (name, rel, r["cond"], r["best"]))
    assert rel <= 1e-9


@pytest.mark.parametrize("name", ["A", "B"])
def test_model_cases_meet_their_preconditions(name):
    r = _case_ref(name)
    assert r["cond"] <= 1e7
    e = np.sort(r["refit"].ravel().astype(np.float64))
    print("case %s: best %.6g, runner-up %.6g (%.1f %% apart)" % (name, e[0], e[1], 100 * (e[1] / e[0] - 1)))
    assert e[1] > 1.01 * e[0]


# ------------------------------------------------------------------------------------------------ GPU
def _ctx():
    from gpcsd_amd import _hip
    return _hip.default_context()


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [0.1, 1.0, 10.0])
@pytest.mark.parametrize("R", [30.0, 300.0])
def test_basis_kernel_against_the_long_double_rule_at_the_same_nodes(R, ratio):
    ctx = _ctx()
    h = ratio * R
    gx, gw = KR.gauss_legendre(48)
    worst_pot = worst_src = 0.0
    for im, M in enumerate((1, 5, 64, 65)):
        src = np.linspace(0.0, 2300.0, M) if M > 1 else np.array([0.0])
        special = [src[0], src[0] + R, src[0] + R * (1 + 1e-12), src[0] + 3.5 * R]      # on a centre, at R, just past R, beyond 3 R
        for npts in (1, 3, 24, 65):
            pts = 100.0 * np.arange(npts)
            for k in range(min(npts, 4)):
                pts[npts - 1 - k] = special[(k + im) % 4]
            got = ctx.kcsd_basis_1d(src, pts, R, h, 1.3, gx, gw, 0)
            ref, mag = KR.potential_basis(src, pts, R, h, 1.3, gx, gw)
            assert got.shape == (M, npts) and np.all(np.isfinite(got))
            frac = np.abs(got.astype(LD) - ref) / KR.potential_bound(mag, 48)
            worst_pot = max(worst_pot, float(frac.max()))
            got = ctx.kcsd_basis_1d(src, pts, R, h, 1.3, gx, gw, 1)
            ref = KR.source_basis(src, pts, R)
            # the relative bound is float64's as long as the value is a normal float64; below that the format has no 2^-53 to give
            tiny = np.finfo(np.float64).tiny
            live = ref >= tiny
            frac = np.abs(got.astype(LD) - ref)[live] / KR.source_bound(src, pts, R, ref)[live]
            worst_src = max(worst_src, float(frac.max()))
            assert np.all((got[~live] >= 0.0) & (got[~live] <= tiny))
    print("R = %g, h/R = %g: largest fraction of the rounding bound: potential basis %.3f, source basis %.3f" % (R, ratio, worst_pot, worst_src))
    assert worst_pot <= 1.0
    assert worst_src <= 1.0


def _cv_operands(n, T, nR, seed=0):
    rs = np.random.default_rng(1000 * n + 10 * T + nR + seed)
    Umat = np.stack([np.linalg.qr(rs.standard_normal((n, n)))[0] for _ in range(nR)])
    s = np.stack([np.logspace(0, -8, n) * (1.0 + r) for r in range(nR)])
    W = rs.standard_normal((nR, n, T))
    return np.ascontiguousarray(Umat), s, W


def _cv_check(ctx, n, T, nR, lambdas):
    Umat, s, W = _cv_operands(n, T, nR)
    err, status = ctx.kcsd_cv(Umat, s, W, lambdas)
    assert err.shape == (nR, len(lambdas)) and not status.any()
    worst = 0.0
    for r in range(nR):
        for l, lam in enumerate(lambdas):
            ref, gate, singular = KR.cv_spectral(Umat[r], s[r], W[r], lam)
            assert not singular
            worst = max(worst, float(abs(LD(err[r, l]) - ref) / gate))
    return worst


# n = 130 (two panels of U, W in LDS) and 257 (past the LDS-resident limit: W through the caches) are this kernel's own thresholds
@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 17, 24, 65, 130, 257])
def test_cv_kernel_against_the_long_double_closed_form(n):
    ctx = _ctx()
    worst = 0.0
    for T in ((1, 63, 64, 65, 300) if n <= 65 else (1, 65)):
        for nR in ((1, 3) if n <= 65 else (1,)):
            worst = max(worst, _cv_check(ctx, n, T, nR, [1e-6, 1e-3, 1.0]))
    worst = max(worst, _cv_check(ctx, n, 65, 1, np.logspace(0, -6, 25)))
    print("n = %d: largest fraction of the rounding gate %.3f" % (n, worst))
    assert worst <= 1.0


@pytest.mark.gpu
def test_cv_kernel_singular_pair_and_bits():
    ctx = _ctx()
    n, T, nR = 24, 300, 3
    Umat, s, W = _cv_operands(n, T, nR)
    lambdas = np.array([1e-6, 1e-3, 1.0])
    err, status = ctx.kcsd_cv(Umat, s, W, lambdas)
    err2, status2 = ctx.kcsd_cv(Umat, s, W, lambdas)
    assert np.array_equal(err, err2) and np.array_equal(status, status2)                 # the same call twice
    sub, _ = ctx.kcsd_cv(Umat, s, W, lambdas[[2, 0]])
    assert np.array_equal(sub, err[:, [2, 0]])                                           # a lambda subset, in another order
    full25, _ = ctx.kcsd_cv(Umat, s, W, np.concatenate([np.logspace(0, -6, 25), lambdas]))
    assert np.array_equal(full25[:, 25:], err)
    # a singular pair: s_min = 0 and lambda = 0 in the second R only
    s0 = s.copy()
    s0[1, -1] = 0.0
    lam0 = np.array([0.0, 1e-3, 1.0])
    e0, st0 = ctx.kcsd_cv(Umat, s0, W, lam0)
    assert st0[1, 0] == 1 and np.isposinf(e0[1, 0]) and st0.sum() == 1
    e1, st1 = ctx.kcsd_cv(Umat, s0, W, lam0[1:])
    assert not st1.any() and np.array_equal(e0[:, 1:], e1) and np.all(np.isfinite(e1))
    assert np.array_equal(e0[[0, 2]], ctx.kcsd_cv(Umat[[0, 2]], s0[[0, 2]], W[[0, 2]], lam0)[0])
    # blocks of 64 columns: a block's partial sums must not depend on where the block sits.  The blocks are added in index order,
    # so exchanging the first two whole blocks exchanges the operands of the first (commutative) addition and nothing else.
    for TT in (192, 300):
        Wp = W[:, :, :TT].copy()
        base, _ = ctx.kcsd_cv(Umat, s, Wp, lambdas)
        perm = np.concatenate([np.arange(64, 128), np.arange(0, 64), np.arange(128, TT)])
        moved, _ = ctx.kcsd_cv(Umat, s, np.ascontiguousarray(Wp[:, :, perm]), lambdas)
        assert np.array_equal(base, moved)


@pytest.mark.gpu
def test_cv_kernel_argument_and_capacity_checks():
    from gpcsd_amd import _hip
    ctx = _ctx()
    Umat, s, W = _cv_operands(3, 5, 1)
    gx, gw = KR.gauss_legendre(4)
    with pytest.raises(ValueError):
        ctx.kcsd_cv(Umat, s, W, [-1.0])
    with pytest.raises(ValueError):
        ctx.kcsd_cv(Umat, np.where(np.arange(3) == 1, np.nan, s), W, [1.0])
    with pytest.raises(_hip.GPCSDCapacityError):
        ctx.kcsd_cv(Umat, s, W, np.ones(65536))
    for kw in (dict(R=0.0), dict(h=0.0), dict(R=-1.0)):
        a = dict(R=1.0, h=1.0)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.kcsd_basis_1d([0.0], [1.0], a["R"], a["h"], 1.0, gx, gw, 0)
    with pytest.raises(ValueError):
        ctx.kcsd_basis_1d([0.0], [1.0], 1.0, 1.0, 1.0, gx[:1], gw[:1], 0)
    with pytest.raises(ValueError):
        ctx.kcsd_basis_1d([np.inf], [1.0], 1.0, 1.0, 1.0, gx, gw, 0)
    from gpcsd_amd.kcsd import KCSD1D
    c = _case("A")
    one = KCSD1D(c["x"], c["V"], h=c["h"], n_src_init=1)         # one source: K has rank 1, and lambda = 0 leaves every pair singular
    with pytest.raises(np.linalg.LinAlgError):
        one.cross_validate(Rs=[300.0, 600.0], lambdas=[0.0])
    assert one.cv_status.all() and np.all(np.isposinf(one.cv_error))
    with pytest.raises(np.linalg.LinAlgError):
        one.values()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_model_against_explicit_refits(name):
    c, r = _case(name), _case_ref(name)
    m = _model(name)
    R, lam = m.cross_validate(Rs=c["Rs"], lambdas=c["lambdas"])
    assert m.cv_error.shape == (3, 4) and not m.cv_status.any()
    rel = float(np.max(np.abs(m.cv_error.astype(LD) - r["refit"]) / r["refit"]))
    csd, pot = m.values(), m.values('POT')
    assert csd.shape == (m.estm_x.size, c["T"]) and pot.shape == (c["n"], c["T"])
    e_csd = float(np.max(np.abs(csd.astype(LD) - r["csd"])) / np.max(np.abs(r["csd"])))
    e_pot = float(np.max(np.abs(pot.astype(LD) - r["pot"])) / np.max(np.abs(r["pot"])))
    print("case %s: cv_error %.2e, CSD %.2e, POT %.2e (gate 1e-6)" % (name, rel, e_csd, e_pot))
    assert (R, lam) == (c["Rs"][r["best"][0]], c["lambdas"][r["best"][1]])
    assert rel <= 1e-6 and e_csd <= 1e-6 and e_pot <= 1e-6
    assert m.k_pot.shape == (c["n"], c["n"]) and m.k_interp_cross.shape == (m.estm_x.size, c["n"])
    # a model built with the selected pair gives the estimate without the scan (the scripts' second use), same bits
    from gpcsd_amd.kcsd import KCSD1D
    again = KCSD1D(c["x"], c["V"], h=c["h"], n_src_init=c["M"], R_init=R, lambd=lam)
    assert np.array_equal(again.values(), csd) and np.array_equal(again.values('POT'), pot)
    # 3-D potentials come back 3-D, with the bits of the flattened call
    nt = 8 if name == "A" else 11
    m3 = _model(name, pots=c["V"].reshape(c["n"], nt, -1))
    assert m3.cross_validate(Rs=c["Rs"], lambdas=c["lambdas"]) == (R, lam)
    assert np.array_equal(m3.cv_error, m.cv_error)
    v3 = m3.values()
    assert v3.shape == (m.estm_x.size, nt, c["T"] // nt) and np.array_equal(v3.reshape(csd.shape), csd)


@pytest.mark.gpu
def test_the_kcsd_block_of_sim_from_gp_1D_runs_with_the_import_swapped():
    """simulation_studies/sim_from_gp_1D.py:112-127 on synthetic trials of the script's shapes: the scan over 15 basis widths with the
    default ridge grid on five concatenated trials, then one model per test trial built from the selected pair."""
    from gpcsd_amd.kcsd import KCSD1D, DEFAULT_LAMBDAS
    nx, nt, ntrials = 24, 60, 2
    x = np.linspace(0, 2300, nx)[:, None]
    t = np.linspace(0, nt, nt)[:, None]
    deltax = x[1] - x[0]
    R_true = 100
    rs = np.random.default_rng(5)
    z = np.linspace(0, 2300, 100)
    csd = np.exp(-0.5 * ((z[:, None] - rs.uniform(0, 2300, 5)[None, :]) / 200.0) ** 2) @ rs.standard_normal((5, nt * (5 + ntrials)))
    lfp = _forward(x[:, 0], z, csd, R_true).reshape(nx, nt, 5 + ntrials)
    lfp = lfp / lfp.std() + 0.01 * rs.standard_normal(lfp.shape)
    kcsd_model = KCSD1D(x, lfp[:, :, :5].reshape((nx, -1)), gdx=deltax / 20, h=R_true)
    kcsd_model.cross_validate(Rs=np.linspace(100, 1000, 15))
    kcsd_R, kcsd_lambda = kcsd_model.R, kcsd_model.lambd
    err, st = kcsd_model.cv_error, kcsd_model.cv_status
    assert err.shape == (15, 25) and np.all(np.isposinf(err[st == 1])) and np.all(np.isfinite(err[st == 0]))
    ri, li = np.unravel_index(np.argmin(np.where(st == 0, err, np.inf)), err.shape)      # (first minimum in row-major order)
    assert (kcsd_R, kcsd_lambda) == (np.linspace(100, 1000, 15)[ri], DEFAULT_LAMBDAS[li])
    for i in range(ntrials):
        kcsd_model_tmp = KCSD1D(x, lfp[:, :, 5 + i].squeeze(), gdx=deltax / 20, h=R_true, R_init=kcsd_R, lambd=kcsd_lambda)
        kcsd_values_tmp = kcsd_model_tmp.values()
        assert kcsd_values_tmp.shape == (kcsd_model_tmp.estm_x.size, nt) and np.all(np.isfinite(kcsd_values_tmp))
        assert kcsd_model_tmp.estm_x.size == 20 * (nx - 1) + 1
