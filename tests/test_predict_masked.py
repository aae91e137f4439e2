"""predict_masked / loglik_masked: posterior means and the log-likelihood with missing samples (gpcsd_predict_masked,
gpcsd_loglik_masked, gpcsd_masked_gram; no reference counterpart).

Expected values: the DENSE statement of tests/masked_ref.py (Cholesky of K_OO per trial, one refinement step), which
tests/test_masked_ref.py pins to the oracle and to the Schur restatement on the CPU.  Tolerance everywhere: the project's parity
gate (tests/test_predict_at.py: GATE).  The assembly kernel alone is held to a rounding bound of its own."""
import os
import types

import numpy as np
import pytest

import masked_ref as MR
import test_predict_at as PA
from helpers import relerr

GATE = PA.GATE
U = 2.0 ** -53


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _points(name):
    c = MR.case(name)["c"]
    return ((c["x"], c["t"], "grid"), (MR.sites(name), PA._offgrid(c["t"], 4), "off"))


# ------------------------------------------------------------------------------------------------ the model calls
@pytest.mark.gpu
@pytest.mark.parametrize("pattern", MR.PATTERNS)
@pytest.mark.parametrize("name", MR.CASES)
def test_predict_masked_vs_dense(name, pattern):
    m = PA._model(name)
    c = MR.case(name)["c"]
    mask, ref = MR.mask_for(name, pattern), MR.dense(name, pattern)
    for z, ts, tag in _points(name):
        out = m.predict_masked(z, ts, mask, type="both")
        assert out["csd"] is m.csd_pred and m.csd_pred.shape == (z.shape[0], ts.shape[0], c["R_trials"])
        assert m.t_pred is ts or np.array_equal(m.t_pred, ts)
        PA._assert_matches(PA._results(m), MR.predictions(name, ref["alpha"], z, ts), len(c["temporal"]),
                           "masked %s %s %s" % (name, pattern, tag))
        if pattern == "none_observed":                                   # exactly 0, not merely small
            for nm in PA.NAMES:
                assert not PA._results(m)[nm][:, :, 1].any() and not any(a[:, :, 1].any() for a in PA._results(m)[nm + "_list"])


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", MR.PATTERNS)
@pytest.mark.parametrize("name", MR.CASES)
def test_loglik_masked_vs_dense(name, pattern):
    m = PA._model(name)
    mask, ref = MR.mask_for(name, pattern), MR.dense(name, pattern)
    ll = m.loglik_masked(mask)
    rows = np.array(m.loglik_masked_trials)
    tot = ref["rows"].sum(0)
    errs = [relerr(rows[:, k], ref["rows"][:, k]) for k in range(2)] + [abs(rows[:, k].sum() - tot[k]) / abs(tot[k]) for k in range(2)]
    e_ll = abs(ll - (-0.5 * tot[0] - 0.5 * tot[1])) / abs(0.5 * tot[0] + 0.5 * tot[1])
    print("loglik_masked %s %s rows log det / quad, sums log det / quad, value: %s %.2e" % (name, pattern, " ".join("%.2e" % e for e in errs), e_ll))
    assert max(errs) < GATE and e_ll < GATE
    assert m.n_obs == ref["n_obs"]
    if pattern == "none_observed":
        assert rows[1, 0] == 0.0 and rows[1, 1] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", MR.CASES)
def test_all_true_mask_is_predict_at_and_loglik(name):
    """With nothing missing the calls are predict_at and the two parts of the log-likelihood of the same model (no jitter, as in
    every prediction)."""
    m = PA._model(name)
    c = MR.case(name)["c"]
    R = c["R_trials"]
    mask = np.ones(m.lfp.shape, dtype=bool)
    for z, ts, tag in _points(name):
        m.predict_at(z, ts, type="both")
        ref = PA._results(m)
        m.predict_masked(z, ts, mask, type="both")
        PA._assert_matches(PA._results(m), ref, len(c["temporal"]), "all-true %s %s" % (name, tag))
    m.loglik_masked(mask)
    ctx = m._sync_device()
    hp, _keep = m._hparams(0.0)
    sumlog, quad = ctx.loglik_parts(hp)
    got = np.array(m.loglik_masked_trials).sum(0)
    errs = [abs(got[0] - R * sumlog) / abs(R * sumlog), abs(got[1] - quad) / abs(quad)]
    print("all-true %s vs loglik parts: %.2e %.2e" % (name, errs[0], errs[1]))
    assert max(errs) < GATE and m.n_obs == m.lfp.size


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1d_odd_17x37x5", "2d_grid_48x40x2"])
def test_masked_out_values_are_never_operands(name):
    """NaN, Inf or 1e300 at the masked-out samples return the bits that zeros return; the same call twice returns the same bits."""
    m = PA._model(name)
    mask = MR.mask_for(name, "mixed")
    z, ts, _ = _points(name)[1]
    keep = m.lfp

    def run(fill):
        m.lfp = np.where(mask, keep, fill)
        m.invalidate()                                                   # (a new array may reuse the address of the last one)
        m.predict_masked(z, ts, mask, type="both")
        res = PA._results(m)
        ll = m.loglik_masked(mask)
        return res, ll, np.array(m.loglik_masked_trials)

    try:
        base = run(0.0)
        for fill in (0.0, np.nan, np.inf, 1e300):
            res, ll, rows = run(fill)
            for nm in PA.NAMES:
                assert _same_bits(res[nm], base[0][nm]), (name, fill, nm)
                assert all(_same_bits(a, b) for a, b in zip(res[nm + "_list"], base[0][nm + "_list"]))
            assert _same_bits(np.float64(ll), np.float64(base[1])) and _same_bits(rows, base[2]), (name, fill)
    finally:
        m.lfp = keep
        m.invalidate()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MR.CASES)
def test_the_2d_mask_agrees_with_its_repetition(name):
    m = PA._model(name)
    c = MR.case(name)["c"]
    m2 = MR.mask_for(name, "electrode2d")
    m3 = MR.mask3(m2, c["R_trials"])
    z, ts, _ = _points(name)[1]
    m.predict_masked(z, ts, m3, type="both")
    ref = PA._results(m)
    ll3, rows3 = m.loglik_masked(m3), np.array(m.loglik_masked_trials)
    m.predict_masked(z, ts, m2, type="both")
    PA._assert_matches(PA._results(m), ref, len(c["temporal"]), "2-D mask " + name)
    ll2 = m.loglik_masked(m2)
    assert abs(ll2 - ll3) < GATE * abs(ll3) and max(relerr(m.loglik_masked_trials[:, k], rows3[:, k]) for k in range(2)) < GATE
    assert m.n_obs == int(m3.sum())


@pytest.mark.gpu
def test_resident_views_hold_the_host_results():
    name = "1d_odd_17x37x5"
    m = PA._model(name)
    c = MR.case(name)["c"]
    mask = MR.mask_for(name, "window6")
    z, ts, _ = _points(name)[1]
    m.predict_masked(z, ts, mask, type="both")
    host = PA._results(m)
    m.predict_masked(z, ts, mask, type="both", resident=True)
    shape = (z.shape[0], ts.shape[0], c["R_trials"])
    assert tuple(m.csd_pred.shape) == shape and hasattr(m.csd_pred, "__cuda_array_interface__")
    ctx = m._context()
    for nm in PA.NAMES:
        assert _same_bits(ctx.fetch("pred_out_" + nm, shape), host[nm])


# ------------------------------------------------------------------------------------------------ the assembly kernel alone
def _orthogonal(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return np.ascontiguousarray(q * np.sign(np.diag(r))[None, :])


def _missing_sets(nx, nt):
    """{tag: (xi, ti)}: time groups of 1, 16, 17, 65 and 80 members (as far as nx electrodes allow), nu in {1, 2, 24}, m = 1."""
    sizes = [s for s in (1, 16, 17, 65, 80) if s <= nx]
    rng = np.random.RandomState(nx)
    grp = lambda t, n: (rng.permutation(nx)[:n], np.full(n, t))
    sets = {"m1": grp(7, 1)}
    for s in sizes[1:] or sizes:
        sets["nu1_g%d" % s] = grp(3, s)
    sets["nu2"] = tuple(np.concatenate(p) for p in zip(grp(nt - 1, sizes[-1]), grp(0, 1)))
    parts = [grp(t, sizes[t % len(sizes)]) for t in rng.permutation(nt)]          # times in a shuffled order: the call sorts
    sets["nu24"] = tuple(np.concatenate(p) for p in zip(*parts))
    return sets


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [5, 16, 17, 80])
def test_masked_gram_against_numpy(nx, monkeypatch):
    """|G - G_ref| <= 8 (nx nt + 16) u sum|terms| entrywise (the form of the Gamma bound in test_torus_graph.py; G_ref in float64,
    whose own error is far inside it), G equal to its transpose bit for bit, and the same bits however the rows are chunked."""
    from gpcsd_amd import _hip
    nt = 24
    rng = np.random.RandomState(100 + nx)
    Qs, Qt = _orthogonal(rng, nx), _orthogonal(rng, nt)
    D = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (nx, nt)))
    ctx = _hip.Context()
    worst = 0.0
    for tag, (xi, ti) in _missing_sets(nx, nt).items():
        Phi = (Qs[xi][:, :, None] * Qt[ti][:, None, :]).reshape(xi.size, nx * nt)
        ref = (Phi / D.reshape(1, -1)) @ Phi.T
        bound = 8 * (nx * nt + 16) * U * ((np.abs(Phi) / D.reshape(1, -1)) @ np.abs(Phi).T)
        G = ctx.masked_gram(Qs, Qt, D, xi, ti)
        frac = float(np.max(np.abs(G - ref) / bound))
        worst = max(worst, frac)
        print("masked_gram nx=%d %s m=%d: %.3g of the bound" % (nx, tag, xi.size, frac))
        assert frac <= 1.0
        assert _same_bits(G, G.T), "G is not symmetric bit for bit"
        assert _same_bits(G, ctx.masked_gram(Qs, Qt, D, xi, ti)), "the same call returned other bits"
        monkeypatch.setenv("GPCSD_MASKED_SCRATCH_MB", "0.03")            # a few time groups per launch
        assert _same_bits(G, ctx.masked_gram(Qs, Qt, D, xi, ti)), "chunking changed the bits"
        monkeypatch.delenv("GPCSD_MASKED_SCRATCH_MB")
    print("masked_gram nx=%d: largest error / bound %.3g" % (nx, worst))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_capacity_and_argument_errors():
    from gpcsd_amd import _hip
    m = PA._model("cfg3s_2d_384x500x2")
    z, ts = m.spatial_cov.x[:2], np.asarray(m.temporal_cov_list[0].t)[:3]
    mask = np.ones(m.lfp.shape, dtype=bool)
    mask.reshape(-1, mask.shape[2])[:_hip.MAX_MISSING + 1, 1] = False
    with pytest.raises(_hip.GPCSDCapacityError):
        m.predict_masked(z, ts, mask)
    with pytest.raises(_hip.GPCSDCapacityError):
        m.loglik_masked(mask)
    for bad in (mask[:, :, :1], mask[:-1], mask.reshape(-1)):
        with pytest.raises(ValueError):
            m.predict_masked(z, ts, bad)
        with pytest.raises(ValueError):
            m.loglik_masked(bad)
    with pytest.raises(ValueError):
        m.predict_masked(z, ts, mask, type="neither")
    small = PA._model("1d_odd_17x37x5")
    small._sharding = types.SimpleNamespace(rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError):
            small.predict_masked(z, ts, np.ones(small.lfp.shape, dtype=bool))
        with pytest.raises(NotImplementedError):
            small.loglik_masked(np.ones(small.lfp.shape, dtype=bool))
    finally:
        small._sharding = None


def test_refusals_that_need_no_device():
    """Wrong mask shapes, trial-sharded models and user-defined temporal covariances are refused before anything is uploaded."""
    from gpcsd_amd.gpcsd1d import GPCSD1D
    x, t = np.linspace(0, 700, 8)[:, None], np.arange(30.0)[:, None]
    ok = np.ones((8, 30), dtype=bool)
    m = GPCSD1D(np.zeros((8, 30, 2)), x, t)
    for bad in (np.ones((8, 30, 3), dtype=bool), np.ones((30, 8), dtype=bool), np.ones(240, dtype=bool)):
        with pytest.raises(ValueError):
            m.predict_masked(x, t, bad)
        with pytest.raises(ValueError):
            m.loglik_masked(bad)
    m.shard_trials(types.SimpleNamespace(rank=0, world_size=1))
    with pytest.raises(NotImplementedError):
        m.predict_masked(x, t, ok)
    with pytest.raises(NotImplementedError):
        m.loglik_masked(ok)
    um = GPCSD1D(np.zeros((8, 30, 2)), x, t, temporal_cov_list=[PA._RationalQuadraticCov(t, 4.0, 0.5)])
    with pytest.raises(NotImplementedError):
        um.predict_masked(x, t, ok)
    with pytest.raises(NotImplementedError):
        um.loglik_masked(ok)


def test_surface_exists():
    import re
    from gpcsd_amd import build, _hip
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    for cls in (GPCSD1D, GPCSD2D):
        assert callable(getattr(cls, "predict_masked", None)) and callable(getattr(cls, "loglik_masked", None))
    build.build(verbose=False)
    lib = _hip.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gpcsd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for fn in ("gpcsd_predict_masked", "gpcsd_predict_masked_resident", "gpcsd_loglik_masked", "gpcsd_masked_gram"):
        assert re.search(r"\b%s\s*\(" % fn, src), "%s is not declared" % fn
        assert fn in _hip.SIGNATURES
        assert hasattr(lib, fn), "libgpcsd_hip.so does not export %s" % fn
    assert re.search(r"#define\s+GPCSD_MAX_MISSING\s+8192\b", src) and _hip.MAX_MISSING == 8192
