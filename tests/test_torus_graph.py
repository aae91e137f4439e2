"""Phase-difference torus graph on the device (gpcsd_torus_graph, gpcsd_torus_graph_resident, gpcsd_trsm_lower_trans; no reference
counterpart in the package).

The expected values come from tests/torus_ref.py, the dense per-trial statement of the estimator in np.longdouble (float64 for
d = 33), given the same float64 unit phasors as the device.  Inputs: rng = default_rng(0), X = rng.vonmises(0, 1, (d, N)) +
rng.vonmises(0, 2, N), then four multinomial replicates from the same generator.  Bounds, u = 2^-53:

  Gamma, H entrywise: (N + 16) u -- weighted means of products of numbers in [-1, 1], each formed with two multiply-adds: the GEMM
      rounding bound of DESIGN.md 4.6 (d = 33: float64 reference, twice that);
  phi: |phi - ref|_2 / |ref|_2 <= cond2(Gamma_ref) (4 d (N + 16) + 8 m) u -- the perturbation bound: a row of Gamma has about 4 d
      non-zeros, each within the bound above, |Gamma|_2 >= its O(1) diagonal, 8 m for the factorisation and the two solves -- under
      the PRECONDITION cond2(Gamma_ref) <= 1e3, asserted for every replicate solved (on the CPU: <= 110 for the unit-weight fits of
      these shapes, <= 18 for the multinomial replicates at N >= 8 d);
  chi2 (relative to max(chi2_ref, 1)) and cond_coupling: the project's parity gate 1e-6.

The GPU tests print the maxima they observe."""
import functools
import os
import re

import numpy as np
import pytest

import torus_ref as T

U = 2.0 ** -53
GATE = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(d, N) for d in (2, 3, 9, 17) for N in (2 * d + 1, 8 * d, 8 * d + 1)] + [(33, 70)]
NBOOT = 4


@functools.lru_cache(maxsize=None)
def _data(d, N):
    rng = np.random.default_rng(0)
    X = rng.vonmises(0, 1, (d, N)) + rng.vonmises(0, 2, N)
    u_re, u_im = T.phasors(X)
    Wt = rng.multinomial(N, [1.0 / N] * N, size=NBOOT).astype(np.float64)
    for a in (X, u_re, u_im, Wt):
        a.setflags(write=False)
    return X, u_re, u_im, Wt


@functools.lru_cache(maxsize=None)
def _ref(d, N, rep):
    """rep = -1: the unit-weight fit (with inference), rep >= 0: that multinomial replicate.  Computed once, shared, read-only."""
    _, u_re, u_im, Wt = _data(d, N)
    res = T.fit(u_re, u_im, weights=None if rep < 0 else Wt[rep], dtype=np.float64 if d == 33 else T.LD, inference=rep < 0)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def _phi_gate(d, N, cond):
    return cond * (4 * d * (N + 16) + 8 * d * (d - 1)) * U


def _relerr(a, b):
    a, b = np.asarray(a, dtype=T.LD), np.asarray(b, dtype=T.LD)
    return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b ** 2)))


# ------------------------------------------------------------------------------------------------ CPU
def test_surface_exists_and_fails_loudly_without_a_gpu():
    import torch
    from gpcsd_amd import build, _hip, utility_functions as UF
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    for cls in (GPCSD1D, GPCSD2D):
        assert callable(getattr(cls, "torus_graph", None))
    for fn in ("torus_graph", "torus_graph_resident", "trsm_lower_trans"):
        assert callable(getattr(_hip.Context, fn, None))
    assert "torus.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _hip.load_library()
    src = open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read()
    for fn in ("gpcsd_torus_graph", "gpcsd_torus_graph_resident", "gpcsd_trsm_lower_trans"):
        decl = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % fn, src, flags=re.S)
        assert decl, "%s is not declared under a comment" % fn
        text = " ".join(decl.group(1).replace("*", " ").split()).lower()
        assert "no reference counterpart in the package" in text, fn
        assert "auditory_lfp/torus_graph_fit.py" in text and "neuropixels/fit_torus_graph.py" in text, fn
        assert fn in _hip.SIGNATURES and hasattr(lib, fn)
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipUnavailable):
            UF.torus_graph(np.zeros((3, 20)))


def test_host_side_argument_checks():
    from gpcsd_amd import utility_functions as UF
    with pytest.raises(ValueError):
        UF.torus_graph(np.zeros((3, 20)), weights=np.ones((1, 20)), nboot=2)
    with pytest.raises(ValueError):
        UF.torus_graph(np.zeros((3, 20)), weights=np.ones((1, 19)))
    with pytest.raises(ValueError):
        UF.torus_graph(np.zeros(20))
    w = UF._torus_graph_weights(7, None, 3, 11)
    assert w.shape == (4, 7) and np.all(w[0] == 1.0)
    assert np.array_equal(w[1:], np.random.default_rng(11).multinomial(7, [1.0 / 7] * 7, size=3))
    assert UF._torus_graph_weights(7, None, 0, None) is None


# ------------------------------------------------------------------------------------------------ GPU
_CTX = []


def _ctx():
    if not _CTX:
        from gpcsd_amd import _hip
        _CTX.append(_hip.Context())
    return _CTX[0]


@pytest.mark.gpu
@pytest.mark.parametrize("d,N", SHAPES)
def test_gamma_and_h_against_extended_precision(d, N):
    """Node-block orders 2 d - 1 = 3, 5, 17, 33, 65 cross the 16, 32 and 64 fragment and tile edges; N = 2 d + 1, 8 d, 8 d + 1 cross
    the K-tile edge of 16.  Replicate 0 with unit weights, and one multinomial replicate passed as the first row of weights."""
    from gemm_ref import same_bits
    ctx = _ctx()
    _, u_re, u_im, Wt = _data(d, N)
    pairs = T.pairs(d)
    share = (pairs[:, None, :, None] == pairs[None, :, None, :]).any(axis=(2, 3))          # (P, P): a common node
    disjoint = np.repeat(np.repeat(~share, 2, axis=0), 2, axis=1)
    gate = (N + 16) * U * (2 if d == 33 else 1)
    worst = 0.0
    for rep in (-1, 0):
        res = ctx.torus_graph(u_re, u_im, weights=None if rep < 0 else Wt[rep][None], inference=False, want_gamma=True)
        ref = _ref(d, N, rep)
        G, H = res["gamma0"], res["h0"]
        assert G.shape == ref["Gamma"].shape and H.shape == ref["H"].shape
        e_g = float(np.max(np.abs(G - ref["Gamma"])))
        e_h = float(np.max(np.abs(H - ref["H"])))
        worst = max(worst, e_g / gate, e_h / gate)
        print("gamma / h d=%d N=%d rep=%d: %.3g / %.3g of the bound %.3g" % (d, N, rep, e_g / gate, e_h / gate, gate))
        assert e_g <= gate and e_h <= gate, (d, N, rep, e_g, e_h, gate)
        assert same_bits(G, np.ascontiguousarray(G.T)), "Gamma is not symmetric bit for bit"
        assert np.all(G[disjoint] == 0.0) and not np.any(np.signbit(G[disjoint]))
        assert np.all(ref["Gamma"][disjoint] == 0)
    print("gamma / h d=%d N=%d: largest error / bound %.3g" % (d, N, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("d,N", SHAPES)
def test_phi_against_extended_precision(d, N):
    ctx = _ctx()
    _, u_re, u_im, Wt = _data(d, N)
    nb = NBOOT if N >= 8 * d else 0
    w = np.concatenate([np.ones((1, N)), Wt]) if nb else None
    res = ctx.torus_graph(u_re, u_im, weights=w, inference=False)
    assert res["phi"].shape == (1 + nb, d * (d - 1) // 2, 2) and np.all(res["status"] == 0)
    worst = 0.0
    for r in range(1 + nb):
        ref = _ref(d, N, r - 1)
        assert ref["cond2"] <= 1e3, ("precondition", d, N, r, ref["cond2"])
        e = _relerr(res["phi"][r], ref["phi"])
        gate = _phi_gate(d, N, ref["cond2"])
        worst = max(worst, e / gate)
        print("phi d=%d N=%d replicate %d: relative error %.3g, bound %.3g (cond2 %.1f)" % (d, N, r, e, gate, ref["cond2"]))
        assert e <= gate, (d, N, r, e, gate)
    if nb:
        # a replicate as weights == the same replicate as physically repeated columns
        idx = np.repeat(np.arange(N), Wt[0].astype(np.intp))
        rep = ctx.torus_graph(np.ascontiguousarray(u_re[:, idx]), np.ascontiguousarray(u_im[:, idx]), inference=False)
        assert rep["status"][0] == 0
        e = _relerr(rep["phi"][0], res["phi"][1])
        gate = _phi_gate(d, N, _ref(d, N, 0)["cond2"])
        print("phi d=%d N=%d weights against repeated columns: %.3g, bound %.3g" % (d, N, e, gate))
        assert e <= gate
    print("phi d=%d N=%d: largest error / bound %.3g" % (d, N, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("d,N", SHAPES)
def test_chi2_and_cond_coupling_of_replicate_0(d, N):
    from gpcsd_amd import utility_functions as UF
    X, u_re, u_im, _ = _data(d, N)
    ref = _ref(d, N, -1)
    assert ref["cond2"] <= 1e3, ("precondition", d, N, ref["cond2"])
    out = UF.torus_graph(X, ctx=_ctx())
    assert np.array_equal(out["pairs"], T.pairs(d)) and "phi_boot" not in out
    chi_ref = np.asarray(ref["chi2"], dtype=np.float64)
    e_chi = float(np.max(np.abs(out["chi2"] - chi_ref) / np.maximum(chi_ref, 1.0)))
    cc_ref = T.cond_coupling(ref["phi"])
    e_cc = float(np.max(np.abs(out["cond_coupling"] - cc_ref) / cc_ref))
    print("chi2 / cond_coupling d=%d N=%d: %.3g / %.3g (gate %.0e)" % (d, N, e_chi, e_cc, GATE))
    assert e_chi <= GATE and e_cc <= GATE
    assert np.allclose(out["pvals"], np.exp(-0.5 * out["chi2"]), rtol=0, atol=0)
    assert _relerr(out["phi"], ref["phi"]) <= _phi_gate(d, N, ref["cond2"])


@pytest.mark.gpu
def test_call_forms_and_failures(monkeypatch):
    from gemm_ref import same_bits
    from gpcsd_amd import _hip, utility_functions as UF
    ctx = _ctx()
    d, N = 9, 72
    X, u_re, u_im, Wt = _data(d, N)
    w = np.concatenate([np.ones((1, N)), Wt])
    a = ctx.torus_graph(u_re, u_im, weights=w, want_gamma=True)
    b = ctx.torus_graph(u_re, u_im, weights=w, want_gamma=True)
    for k in ("phi", "chi2", "gamma0", "h0"):                                   # the same call: the same bits
        assert same_bits(a[k], b[k]), k
    assert np.all(a["status"] == 0) and np.all(np.isfinite(a["phi"])) and np.all(a["chi2"] >= 0)
    # one replicate per chunk (GPCSD_TORUS_CHUNK_MB=0: DESIGN.md 9) against all five in one
    monkeypatch.setenv("GPCSD_TORUS_CHUNK_MB", "0")
    c = ctx.torus_graph(u_re, u_im, weights=w)
    monkeypatch.delenv("GPCSD_TORUS_CHUNK_MB")
    assert same_bits(c["phi"], a["phi"]) and same_bits(c["chi2"], a["chi2"]) and np.array_equal(c["status"], a["status"])
    # two nodes
    two = UF.torus_graph(X[:2], nboot=3, seed=5, ctx=ctx)
    assert two["phi"].shape == (1, 2) and two["phi_boot"].shape == (3, 1, 2) and np.all(np.isfinite(two["phi_boot"]))
    assert np.all(two["status_boot"] == 0) and two["cond_coupling_boot"].shape == (3, 1) and 0 <= two["pvals"][0] <= 1
    again = UF.torus_graph((u_re[:2], u_im[:2]), nboot=3, seed=5, ctx=ctx)      # phases and phasors: the same fit, the same seed
    assert same_bits(again["phi_boot"], two["phi_boot"])
    # one trial: Gamma = D D^T has rank 2 of 6
    one = ctx.torus_graph(u_re[:3, :1], u_im[:3, :1])
    assert one["status"][0] > 0 and np.all(np.isnan(one["phi"])) and np.all(np.isnan(one["chi2"]))
    with pytest.raises(np.linalg.LinAlgError):
        UF.torus_graph(X[:3, :1], ctx=ctx)
    # a replicate with all its weight on one trial among good ones: NaN in that row only, the others keep their bits
    lone = np.zeros((1, N))
    lone[0, 7] = N
    bad = ctx.torus_graph(u_re, u_im, weights=np.concatenate([w[:2], lone, w[2:]]), inference=False)
    assert bad["status"][2] > 0 and np.all(np.isnan(bad["phi"][2]))
    keep = [0, 1, 3, 4, 5]
    assert np.all(bad["status"][keep] == 0) and same_bits(bad["phi"][keep], a["phi"])
    with pytest.warns(UserWarning):
        out = UF.torus_graph(X, weights=np.concatenate([lone, Wt[:1]]), ctx=ctx)
    assert np.all(np.isnan(out["phi_boot"][0])) and np.all(np.isnan(out["cond_coupling_boot"][0])) and same_bits(out["phi_boot"][1], a["phi"][1])
    assert list(out["status_boot"] > 0) == [True, False]
    # bad weights, too many nodes
    neg = np.ones((2, N))
    neg[1, 3] = -1.0
    with pytest.raises(ValueError):
        ctx.torus_graph(u_re, u_im, weights=neg)
    with pytest.raises(ValueError):
        ctx.torus_graph(u_re, u_im, weights=np.zeros((1, N)))
    with pytest.raises(ValueError):
        ctx.torus_graph(u_re, u_im, weights=np.full((1, N), np.nan))
    with pytest.raises(ValueError):
        ctx.torus_graph(u_re[:1], u_im[:1])
    with pytest.raises(_hip.GPCSDCapacityError):
        ctx.torus_graph(np.ones((129, 4)), np.zeros((129, 4)))
    d_again = ctx.torus_graph(u_re, u_im, weights=w)                            # the context is as usable as before
    assert same_bits(d_again["phi"], a["phi"])


@pytest.mark.gpu
@pytest.mark.parametrize("nrhs", [1, 5, 70])
@pytest.mark.parametrize("n", [1, 17, 128, 130, 300])
def test_trsm_lower_trans(n, nrhs):
    """n = 128 / 130 / 300: one inverted 128-block, a ragged second one, a second outer block of 256.  The gate is the one
    tests/test_hip_parity.py uses for trsm_lower."""
    rs = np.random.RandomState(100 * n + nrhs)
    A = rs.standard_normal((n, n))
    L = np.linalg.cholesky(A @ A.T / n + np.eye(n))
    B = rs.standard_normal((n, nrhs))
    L0 = L.copy()
    X = _ctx().trsm_lower_trans(L, B)
    assert X.shape == B.shape and np.array_equal(L, L0)
    err = float(np.linalg.norm(L.T @ X - B) / np.linalg.norm(B))
    ref = np.asarray(T.solve_lower_trans(L.astype(T.LD), B), dtype=np.float64)
    print("trsm_lower_trans n=%d nrhs=%d: residual %.3g, against back substitution %.3g" % (n, nrhs, err, np.linalg.norm(X - ref) / np.linalg.norm(ref)))
    assert err < 1e-11
    if nrhs == 1:
        assert _ctx().trsm_lower_trans(L, B[:, 0]).shape == (n,)


@pytest.mark.gpu
def test_through_a_model_resident_and_host_give_the_same_bits():
    from gemm_ref import same_bits
    from gpcsd_amd import _hip, utility_functions as UF
    from test_loo import _model, _case
    from test_phase_plv import _operator
    name = "1d_odd_17x37x5"
    c = _case(name)[0]
    m = _model(name)
    ctx = m._context()
    nz, n, R = _case(name)[3].shape
    at = (20, 5)
    A = _operator("sos37", at)
    m.predict_at(c["x"], c["t"], type="both", resident=True)
    m.phase(A, type="csd", at=at)
    pred = np.array(m.csd_pred.numpy())
    phase_before, amp_before = np.array(m.csd_phase), np.array(m.csd_amp)
    u_re, u_im = (np.array(ctx.fetch(b, (nz, 2, R))) for b in ("phasor_re", "phasor_im"))
    # five trials: three nodes (six parameters) if that keeps the precondition, else two
    chosen = None
    for sites in ((2, 9, 15), (2, 15)):
        ref = T.fit(u_re[list(sites), 1], u_im[list(sites), 1])
        if ref["cond2"] <= 1e3:
            chosen = sites
            break
    assert chosen is not None, "no site set keeps cond2(Gamma) <= 1e3 with five trials"
    d = len(chosen)
    m.torus_graph(type="csd", at=1, sites=chosen, nboot=3, seed=2)
    tg = m.csd_tg
    host = UF.torus_graph((u_re, u_im), nboot=3, seed=2, ctx=ctx, at=1, sites=chosen)       # the host entry point on the fetched phasors
    for k in ("phi", "chi2", "pvals", "cond_coupling", "phi_boot", "cond_coupling_boot"):
        assert same_bits(np.asarray(tg[k]), np.asarray(host[k])), k
    assert np.array_equal(tg["pairs"], T.pairs(d)) and np.array_equal(tg["status_boot"], host["status_boot"])
    e = _relerr(tg["phi"], ref["phi"])
    print("model: sites %s, cond2 %.1f, phi relative error %.3g" % (chosen, ref["cond2"], e))
    assert e <= _phi_gate(d, R, ref["cond2"])
    assert float(np.max(np.abs(tg["chi2"] - np.asarray(ref["chi2"], dtype=np.float64)) / np.maximum(np.asarray(ref["chi2"], dtype=np.float64), 1.0))) <= GATE
    # prediction and phase buffers are untouched
    assert same_bits(m.csd_pred.numpy(), pred) and same_bits(ctx.fetch("pred_out_csd", pred.shape), pred)
    assert same_bits(ctx.fetch("phasor_re", u_re.shape), u_re) and same_bits(ctx.fetch("phasor_im", u_im.shape), u_im)
    assert same_bits(ctx.fetch("phase_out", phase_before.shape), phase_before) and same_bits(m.csd_phase, phase_before) and same_bits(m.csd_amp, amp_before)
    # a host prediction's phasors take the host path: the same bits again
    m.predict_at(c["x"], c["t"], type="csd")
    m.phase(A, type="csd", at=at)
    m.torus_graph(type="csd", at=1, sites=chosen, nboot=3, seed=2)
    assert same_bits(m.csd_tg["phi"], tg["phi"]) and same_bits(m.csd_tg["phi_boot"], tg["phi_boot"])
    # rc -4: no resident phasors of that shape (a fresh context; phase and amplitude only)
    fresh = _hip.Context()
    with pytest.raises(RuntimeError, match="-4"):
        fresh.torus_graph_resident([0, 1], 0, (2, 1, 8))
    x = np.random.RandomState(3).standard_normal((3, 37, 8))
    fresh.analytic(x, _operator("sos37", (20,)), want=("phase",))                   # leaves "op_out", not the phasors
    fresh.analytic_resident("op_in0", 0, (3, 37, 8), _operator("sos37", (20,)), want=("phase", "amp"))
    with pytest.raises(RuntimeError, match="-4"):
        fresh.torus_graph_resident([0, 1, 2], 0, (3, 1, 8))
    fresh.analytic_resident("op_in0", 0, (3, 37, 8), _operator("sos37", (20,)), want=("u_re", "u_im"))
    got = fresh.torus_graph_resident([0, 1, 2], 0, (3, 1, 8))
    ur, ui = (fresh.fetch(b, (3, 1, 8)) for b in ("phasor_re", "phasor_im"))
    assert same_bits(got["phi"], fresh.torus_graph(ur[:, 0], ui[:, 0])["phi"])
    with pytest.raises(ValueError):
        fresh.torus_graph_resident([0, 3], 0, (3, 1, 8))
