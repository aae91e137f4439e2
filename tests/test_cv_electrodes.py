"""cv_electrodes: leave-electrodes-out cross-validation in closed form (gpcsd_cv_electrodes; no reference counterpart).

The expected values come from cv_ref.cv_formulas: Qs, Qt, D from the oracle's eig_D of the matrices loglik() decomposes (test_loo's
_eig), then per fold F and temporal eigen-index j the f x f block G_j = Qs[F] diag(1 / D[:, j]) Qs[F]^T of K^-1, the held-out residual
e = G_j^-1 u in the temporal eigen-basis and the sums over j.  The CPU test pins those formulas to brute-force deletion: every row
and column of the fold removed from the dense K, the rest solved through a Cholesky factor.  gpcsd_efold_contract -- the new
kernels alone -- is held to a first-order rounding bound computed in long double (cv_ref.efold_bound).  The GPU tests print the
maxima they observe; on an MI355X every quantity of every model is within 1.3e-9 of the helper (gate 1e-6; the largest is cfg1),
and holding out everything reproduces loglik() plus its constant to the last printed digit."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import cases as C
import cv_ref
from oracle import gpcsd_oracle as O
from test_loo import GATE, ROOT, _case, _dense_K, _eig, _model

DELETION = ["1d_odd_17x37x5", "1d_siglist_12x40x4", "cfg1_1d_24x100x1"]
MODELS = ["1d_odd_17x37x5", "1d_siglist_12x40x4", "2d_grid_48x40x2", "2d_npx_96x120x3", "cfg1_1d_24x100x1"]
ATTRS = ("cv_var", "cv_mean", "cv_lpd", "cv_sse")


def _mixed(nx):
    """An unsorted, non-contiguous list with electrodes in no fold; a 16-electrode fold where nx >= 20."""
    if nx >= 20:
        return (tuple(range(18, 2, -1)), (nx - 1, 0), (nx - 2,), (1, 19))
    return ((5, 1, 3), (nx - 1, 0), (2,), (8, 6, 7, 4))


def _k(name):
    """folds=4 -- or 8 where four folds would hold more than 16 electrodes each (2d_npx: 96 electrodes, folds=4 is 24 per fold,
    which the call refuses with GPCSDCapacityError; test_cv_vs_helper checks that it does)."""
    return 4 if -(-_case(name)[3].shape[0] // 4) <= 16 else 8


def _folds(name, choice):
    nx = _case(name)[3].shape[0]
    if choice == "none":
        return tuple((i,) for i in range(nx))
    if choice == "k4":
        return tuple(tuple(range(i, nx, _k(name))) for i in range(_k(name)))
    return _mixed(nx)


def _arg(name, choice):
    """What the caller passes for the choice"""
    return {"none": None, "k4": _k(name)}.get(choice, _folds(name, choice))


def _formulas(name, folds, lfp=None):
    Y = _case(name)[3] if lfp is None else lfp
    Qs, Qt, D = _eig(name)
    return cv_ref.cv_formulas(Qs, Qt, D, Y, folds)


@functools.lru_cache(maxsize=None)
def _helper(name, choice, driver=None):
    """cv_formulas of the case's own trials, computed once per LAPACK driver and left unchanged."""
    assert O.EIGH_DRIVER == driver
    out = _formulas(name, _folds(name, choice))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _tolerances(name, choice):
    """test_loo._tolerances' rule: 1e-6, or 3 x the spread of the helper itself between LAPACK drivers where that exceeds a third
    of the gate (with a noise list the reference ties noise x to eigen-RANK x)."""
    base = _helper(name, choice)
    held = ~np.isnan(base["var"][:, 0])
    now = lambda: _helper(name, choice, O.EIGH_DRIVER)
    spread = {"var": O.driver_spread(lambda: now()["var"][held] / base["var"][held])}
    for k in ("resid", "sse"):
        spread[k] = O.driver_spread(lambda: now()[k][held])
    for k in ("lpd", "total"):
        spread[k] = O.driver_spread(lambda: now()[k])
    return {k: (3.0 * s if s > GATE / 3.0 else GATE) for k, s in spread.items()}, spread


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", DELETION)
def test_helper_equals_brute_force_deletion(name):
    """Observed here (residual relative to max|y|, variance to itself, lpd and sse to their maxima over the folds): 1d_odd 7.9e-9 /
    2.6e-10 / 5.7e-11 / 1.8e-10, 1d_siglist 3.5e-13 / 3.1e-14 / 1.7e-15 / 9.9e-14, cfg1 2.0e-7 / 2.1e-9 / 1.8e-9 / 3.9e-9 -- the
    reference's own error (cond(G_j) up to 3.4e7 on cfg1), inside the gate."""
    c, geom, hp, lfp = _case(name)
    nx, nt, R = lfp.shape
    K = _dense_K(name)
    y = lfp.reshape(nx * nt, R)
    folds = [(0,), (nx // 2,), (nx - 1,), (1, 2, 3), tuple(int(v) for v in np.arange(8) * (nx // 8)), tuple(range(nx - 5, nx))]
    if name.startswith("cfg1"):
        folds.append(tuple(range(3, 19)))
    got, ref = [], []
    for F in folds:                                                              # one at a time: these folds overlap
        h = _formulas(name, (F,))
        mean, var, lpd = cv_ref.brute_force_fold(K, y, F, nt)
        F = list(F)
        got.append((h["resid"][F], h["var"][F], h["lpd"][0], h["sse"][F]))
        resid = lfp[F] - mean
        ref.append((resid, var, lpd, (resid * resid).sum(axis=1)))
    lpd_max = max(float(np.max(np.abs(r[2]))) for r in ref)
    sse_max = max(float(np.max(np.abs(r[3]))) for r in ref)
    err = {"resid": 0.0, "var": 0.0, "lpd": 0.0, "sse": 0.0}
    for g, r in zip(got, ref):
        err["resid"] = max(err["resid"], float(np.max(np.abs(g[0] - r[0])) / np.max(np.abs(y))))
        err["var"] = max(err["var"], float(np.max(np.abs(g[1] - r[1]) / r[1])))
        err["lpd"] = max(err["lpd"], float(np.max(np.abs(g[2] - r[2])) / lpd_max))
        err["sse"] = max(err["sse"], float(np.max(np.abs(g[3] - r[3])) / sse_max))
    print("cv helper vs deletion %s: " % name + ", ".join("%s %.2e" % kv for kv in err.items()))
    for k, v in err.items():
        assert v < GATE, (name, k, v)


def test_surface_exists_and_fails_loudly_without_a_gpu():
    import torch
    from gpcsd_amd import build, _hip
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    assert callable(getattr(GPCSD1D, "cv_electrodes", None)) and callable(getattr(GPCSD2D, "cv_electrodes", None))
    build.build(verbose=False)
    lib = _hip.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read(), flags=re.S)
    for fn in ("gpcsd_cv_electrodes", "gpcsd_cv_electrodes_resident", "gpcsd_efold_contract"):
        assert re.search(r"\b%s\s*\(" % fn, src), "%s is not declared" % fn
        assert fn in _hip.SIGNATURES
        assert hasattr(lib, fn), "libgpcsd_hip.so does not export %s" % fn
    if not torch.cuda.is_available():
        m = GPCSD1D(np.zeros((24, 50, 2)), np.linspace(0, 2300, 24)[:, None], np.arange(50.0)[:, None])
        with pytest.raises(_hip.HipUnavailable):
            m.cv_electrodes()


def test_fold_normalisation_needs_no_gpu():
    from gpcsd_amd import _hip
    from gpcsd_amd.gpcsd1d import GPCSD1D
    norm = GPCSD1D._normalise_folds
    as_lists = lambda folds: [list(int(v) for v in f) for f in folds]
    assert as_lists(norm(None, 5)) == [[0], [1], [2], [3], [4]]
    assert as_lists(norm(3, 8)) == [[0, 3, 6], [1, 4, 7], [2, 5]]
    assert as_lists(norm([[4, 1], (7,), np.array([6, 0, 2])], 9)) == [[4, 1], [7], [6, 0, 2]]    # sizes differ, order kept, 3 5 8 unheld
    assert as_lists(norm([range(16)], 16)) == [list(range(16))]
    got = norm([[2, 0]], 3)
    assert isinstance(got, tuple) and all(isinstance(f, np.ndarray) and f.dtype.kind == "i" for f in got)
    for bad in ([[0, 1], [1, 2]], [[0, 0]], [[0], [5]], [[-1]], [[0], []], [], 0, 6, [[0.5]]):
        with pytest.raises(ValueError):
            norm(bad, 5)
    with pytest.raises(_hip.GPCSDCapacityError):
        norm([list(range(17))], 40)
    m = GPCSD1D(np.zeros((24, 50, 2)), np.linspace(0, 2300, 24)[:, None], np.arange(50.0)[:, None])
    with pytest.raises(ValueError):                                              # before a context is opened
        m.cv_electrodes(folds=[[0, 24]])
    with pytest.raises(_hip.GPCSDCapacityError):
        m.cv_electrodes(folds=[list(range(17))])


# ------------------------------------------------------------------------------------------------ GPU: the kernels alone
def _contract_folds(rs, nx, cap):
    """Folds of sizes 16, 15, 2 and 1 where nx and cap (the rank of the Gram blocks) allow, members drawn from a permutation --
    unsorted and non-contiguous --, one electrode in no fold where nx > 1."""
    perm = [int(v) for v in rs.permutation(nx)]
    room = nx - 1 if nx > 1 else 1
    folds = []
    for size in (16, 15, 2, 1):
        if size <= cap and size <= room:
            folds.append(tuple(perm[:size]))
            perm, room = perm[size:], room - size
    return tuple(folds)


@pytest.mark.gpu
def test_efold_contract_against_extended_precision():
    """Every output of the new kernels within its first-order rounding bound (cv_ref.efold_bound states it).  Observed on an
    MI355X: largest error / bound 0.503 (E), 0.438 (pdiag), 0.297 (lpd), 0.413 (sse)."""
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    rs = np.random.RandomState(20261021)
    worst = {"E": 0.0, "pdiag": 0.0, "lpd": 0.0, "sse": 0.0}
    sizes_seen = set()
    combos = (((1, 5), (7, 13), (65, 1)), ((1, 13), (7, 1), (65, 5)), ((1, 1), (7, 5), (65, 13)))
    n = 0
    for nx in (1, 5, 17, 68):
        for orth, K in [(True, nx)] + [(False, K) for K in (1, 17, 64, 65) if K != nx]:
            for nt, R in combos[n % 3]:
                if orth:
                    A = np.linalg.qr(rs.standard_normal((nx, nx)))[0]
                else:
                    A = rs.uniform(-1.0, 1.0, (nx, K))
                W = 10.0 ** rs.uniform(-1.5, 1.5, (K, nt))                       # positive, three decades
                V = rs.standard_normal((nx, R, nt))
                folds = _contract_folds(rs, nx, nx if orth else K)
                sizes_seen.update(len(f) for f in folds)
                E, pdiag, lpd, sse, status = ctx.efold_contract(A, W, V, folds)
                assert E.shape == (nx, R, nt) and pdiag.shape == (nx, nt) and lpd.shape == (len(folds), R) and sse.shape == (nx, R)
                assert np.all(status == 0), (nx, K, nt, R, status)
                ref, bound = cv_ref.efold_bound(A, W, V, folds)
                held = np.zeros(nx, dtype=bool)
                held[[a for f in folds for a in f]] = True
                for k, got in (("E", E), ("pdiag", pdiag), ("lpd", lpd), ("sse", sse)):
                    if k != "lpd":
                        assert np.all(np.isnan(got[~held])) and not np.any(np.isnan(got[held])), (k, nx, K, nt, R)
                        got, r, b = got[held], ref[k][held], bound[k][held]
                    else:
                        r, b = ref[k], bound[k]
                    ratio = float(np.max(np.abs(got.astype(np.longdouble) - r) / b))
                    worst[k] = max(worst[k], ratio)
                    assert ratio <= 1.0, (k, nx, K, nt, R, ratio)
                none, pdiag2, lpd2, sse2, status2 = ctx.efold_contract(A, W, V, folds, want_E=False)
                assert none is None and np.array_equal(status2, status)
                for a, b in ((pdiag2, pdiag), (lpd2, lpd), (sse2, sse)):
                    assert np.array_equal(a, b, equal_nan=True)
            n += 1
    assert sizes_seen == {1, 2, 15, 16}
    print("efold_contract: largest error / bound:", " ".join("%s %.3f" % kv for kv in worst.items()))


@pytest.mark.gpu
def test_a_block_that_is_not_positive_definite_sets_its_status_and_nothing_else():
    """A fold of three electrodes over a rank-one Gram block (K = 1, rows 1.0, weights powers of four: the second pivot is exactly
    zero) beside two sound folds: status 1 and NaN for that fold, the others' outputs the bits of a call without it."""
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    rs = np.random.RandomState(7)
    nx, nt, R = 6, 70, 3
    A, W, V = np.ones((nx, 1)), 4.0 ** rs.randint(-3, 4, (1, nt)), rs.standard_normal((nx, R, nt))
    A[[0, 5], 0] = (0.75, 1.5)
    E, pdiag, lpd, sse, status = ctx.efold_contract(A, W, V, ((0,), (4, 1, 3), (5,)))
    assert list(status) == [0, 1, 0]
    assert np.all(np.isnan(lpd[1])) and np.all(np.isnan(sse[[4, 1, 3]])) and np.all(np.isnan(sse[2]))
    E2, pdiag2, lpd2, sse2, status2 = ctx.efold_contract(A, W, V, ((0,), (5,)))
    assert list(status2) == [0, 0] and np.array_equal(lpd2, lpd[[0, 2]])
    for a, b in ((E2, E), (pdiag2, pdiag), (sse2, sse)):
        assert np.array_equal(a[[0, 5]], b[[0, 5]]) and not np.any(np.isnan(a[[0, 5]]))


# ------------------------------------------------------------------------------------------------ GPU: the models
@pytest.mark.gpu
@pytest.mark.parametrize("choice", ["none", "k4", "mixed"])
@pytest.mark.parametrize("name", MODELS)
def test_cv_vs_helper(name, choice):
    m = _model(name)
    ref = _helper(name, choice)
    tol, spread = _tolerances(name, choice)
    folds = _folds(name, choice)
    nx, nt, R = _case(name)[3].shape
    if choice == "k4" and _k(name) != 4:
        from gpcsd_amd import _hip
        with pytest.raises(_hip.GPCSDCapacityError):
            m.cv_electrodes(folds=4)
    total = m.cv_electrodes(folds=_arg(name, choice))
    assert isinstance(total, float)
    assert m.cv_var.shape == (nx, nt) and m.cv_mean.shape == (nx, nt, R) and m.cv_lpd.shape == (len(folds), R)
    assert m.cv_sse.shape == (nx, R) and m.cv_status.shape == (len(folds),) and np.all(m.cv_status == 0)
    assert len(m.cv_folds) == len(folds) and all(list(a) == list(b) for a, b in zip(m.cv_folds, folds))
    held = np.zeros(nx, dtype=bool)
    held[[a for f in folds for a in f]] = True
    for k in ("cv_var", "cv_mean", "cv_sse"):                                    # NaN rows exactly for the unheld electrodes
        v = getattr(m, k)
        assert np.all(np.isnan(v[~held])) and not np.any(np.isnan(v[held])), k
    assert not np.any(np.isnan(m.cv_lpd)) and np.all(m.cv_var[held] > 0)
    resid = (np.asarray(m.lfp) - m.cv_mean)[held]
    err = {"var": float(np.max(np.abs(m.cv_var[held] - ref["var"][held]) / ref["var"][held])),
           "resid": float(np.max(np.abs(resid - ref["resid"][held])) / np.max(np.abs(ref["resid"][held]))),
           "lpd": float(np.max(np.abs(m.cv_lpd - ref["lpd"])) / np.max(np.abs(ref["lpd"]))),
           "sse": float(np.max(np.abs(m.cv_sse[held] - ref["sse"][held])) / np.max(np.abs(ref["sse"][held]))),
           "total": abs(total - ref["total"]) / abs(ref["total"])}
    print("cv %s %s: " % (name, choice) + ", ".join("%s %.2e (gate %.1e, driver spread %.1e)" % (k, err[k], tol[k], spread[k]) for k in err))
    for k in err:
        assert err[k] < tol[k], (name, choice, k, err[k], tol[k])


@pytest.mark.gpu
def test_holding_out_everything_gives_the_marginal_likelihood():
    """One fold of all 12 electrodes: the block is the whole of K, so the joint log predictive density of every trial is its log
    marginal likelihood -- loglik() with the 2 pi constant put back.  Nothing here shares a formula with the helper."""
    name = "1d_siglist_12x40x4"
    m = _model(name)
    nx, nt, R = _case(name)[3].shape
    total = m.cv_electrodes(folds=[list(range(nx))], mean=False)
    want = float(m.loglik()) - R * nx * nt * cv_ref.HALF_LOG_2PI
    err = abs(total - want) / abs(want)
    print("cv of everything %s: %.12e, loglik + constant %.12e, relative difference %.2e" % (name, total, want, err))
    assert total == float(np.sum(m.cv_lpd)) and err < GATE


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1d_odd_17x37x5", "2d_npx_96x120x3"])
def test_bit_identities(name):
    m = _model(name)
    nx, nt, R = _case(name)[3].shape
    folds = _mixed(nx)
    nf = len(folds)
    total = m.cv_electrodes(folds=folds)
    first = {k: np.array(getattr(m, k)) for k in ATTRS + ("cv_status",)}
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert total == float(np.sum(first["cv_lpd"]))
    assert m.cv_electrodes(folds=folds) == total                                 # a second call: the same bits
    for k, v in first.items():
        assert same(np.array(getattr(m, k)), v), k
    assert m.cv_electrodes(folds=folds, mean=False) == total and m.cv_mean is None       # without the mean: the bits of the others
    for k in ("cv_var", "cv_lpd", "cv_sse"):
        assert same(np.array(getattr(m, k)), first[k]), k
    assert m.cv_electrodes(folds=folds, resident=True) == total                  # resident views: the bits of the host arrays
    ctx = m._context()
    for k, shape in (("cv_var", (nx, nt)), ("cv_mean", (nx, nt, R)), ("cv_lpd", (nf, R)), ("cv_sse", (nx, R))):
        v = getattr(m, k)
        assert tuple(v.shape) == shape and hasattr(v, "__cuda_array_interface__")
        assert same(ctx.fetch(k, shape), first[k]), k
    assert same(m.cv_status, first["cv_status"])
    assert m.cv_electrodes(folds=folds, mean=False, resident=True) == total and m.cv_mean is None
    # a fold alone, and the list reversed: the fold's score and its electrodes' rows keep their bits
    m.cv_electrodes(folds=folds[::-1])
    assert same(m.cv_lpd, first["cv_lpd"][::-1])
    for k in ("cv_var", "cv_mean", "cv_sse"):
        assert same(getattr(m, k), first[k]), k
    for n, F in enumerate(folds):
        m.cv_electrodes(folds=[F])
        assert same(m.cv_lpd[0], first["cv_lpd"][n]), n
        for k in ("cv_var", "cv_mean", "cv_sse"):
            assert same(getattr(m, k)[list(F)], first[k][list(F)]), (k, n)
            assert np.all(np.isnan(np.delete(getattr(m, k), list(F), axis=0))), (k, n)


@pytest.mark.gpu
def test_the_variance_does_not_depend_on_the_trials_and_leaves_the_other_results_alone():
    name = "1d_siglist_12x40x4"
    c = _case(name)[0]
    a = _model(name)
    a.predict(c["x"], c["t"], type="both")
    a.loo()
    names = ("csd_pred", "lfp_pred", "t_pred", "x_pred", "loo_var", "loo_mean", "loo_lpd", "loo_sse")
    held = [getattr(a, k) for k in names]
    copies = [np.array(v) for v in held]
    a.cv_electrodes(folds=4)
    assert all(getattr(a, k) is v for k, v in zip(names, held))
    assert all(np.array_equal(v, w) for v, w in zip(held, copies))
    lfp_b = C.synth_lfp(977, c["x"].shape[0], c["t"].shape[0], 7)                 # another seed, 7 trials instead of 4
    b = _model(name, lfp=lfp_b)
    b.cv_electrodes(folds=4)
    assert np.array_equal(a.cv_var, b.cv_var)
    assert b.cv_lpd.shape == (4, 7)
    ref = _formulas(name, _folds(name, "k4"), lfp=lfp_b)                          # ... and the other trials' scores are theirs
    tol = _tolerances(name, "k4")[0]
    assert np.max(np.abs(b.cv_lpd - ref["lpd"])) / np.max(np.abs(ref["lpd"])) < tol["lpd"]


@pytest.mark.gpu
def test_trial_shards_give_the_unsharded_columns_and_total():
    """test_loo's stand-in: two ranks one after the other in this process, with TrialSharding's partition and an all-reduce that
    records what it was given and returns it, so the test forms the sum over the ranks itself."""
    from gpcsd_amd.dist import TrialSharding

    class Rank(TrialSharding):
        def __init__(self, rank, world_size):
            self.rank, self.world_size, self.gather_predictions, self.sent = rank, world_size, False, []

        def allreduce_sum(self, values):
            self.sent.append(np.array(values, dtype=np.float64))
            return self.sent[-1]

    name = "1d_odd_17x37x5"                                                      # 5 trials: blocks of 3 and 2
    lfp = np.array(_case(name)[3])
    full = _model(name)
    total = full.cv_electrodes(folds=4)
    whole = {k: np.array(getattr(full, k)) for k in ATTRS}
    parts = []
    for r in range(2):
        m = _model(name, lfp=lfp)
        sh = Rank(r, 2)
        m.shard_trials(sh)
        sl = sh.local_slice(lfp.shape[2])
        part = m.cv_electrodes(folds=4)
        assert len(sh.sent) == 1 and sh.sent[0].shape == (1,) and sh.sent[0][0] == part == float(np.sum(m.cv_lpd))
        assert np.array_equal(m.cv_var, whole["cv_var"])                         # the same on every rank
        assert m.cv_mean.shape == whole["cv_mean"][:, :, sl].shape
        for k in ("cv_mean", "cv_lpd", "cv_sse"):                                # this rank's block of trials
            ref = whole[k][..., sl]
            assert np.max(np.abs(getattr(m, k) - ref)) <= 1e-12 * np.max(np.abs(ref)), (k, r)
        parts.append(part)
    assert abs(sum(parts) - total) <= 1e-12 * abs(total)


@pytest.mark.gpu
def test_errors():
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    lib = ctx._lib
    hp, _keep = ctx.make_hparams(100.0, 0.0, [200.0], [(_hip.KIND_SE, 20.0, 0.5)], 0.05, 1e-8)
    one = np.zeros(1)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    st = np.zeros(1, dtype=np.int32)
    ptr1, idx1 = np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32)
    # no resident data: the library's -4, from both entry points; null arguments: -3
    assert lib.gpcsd_cv_electrodes_resident(ctx._h, ctypes.byref(hp), ip(ptr1), ip(idx1), 1, 1) == -4
    assert lib.gpcsd_cv_electrodes(ctx._h, ctypes.byref(hp), ip(ptr1), ip(idx1), 1, dp(one), None, dp(one), dp(one), ip(st)) == -4
    assert b"lfp not set" in lib.gpcsd_last_error(ctx._h)
    assert lib.gpcsd_cv_electrodes_resident(ctx._h, None, ip(ptr1), ip(idx1), 1, 1) == -3
    assert lib.gpcsd_cv_electrodes_resident(ctx._h, ctypes.byref(hp), None, ip(idx1), 1, 1) == -3
    assert lib.gpcsd_cv_electrodes_resident(ctx._h, ctypes.byref(hp), ip(ptr1), ip(idx1), 0, 1) == -3

    # malformed fold lists and capacity, before anything is read or launched: the data arrays hold ONE double each
    def call(nx, ptr, idx, R=1, nt=1, K=1):
        ptr, idx = np.array(ptr, dtype=np.int32), np.array(idx, dtype=np.int32)
        return lib.gpcsd_efold_contract(ctx._h, dp(one), dp(one), dp(one), nx, K, nt, R, ip(ptr), ip(idx), len(ptr) - 1, None, dp(one),
                                        dp(one), dp(one), ip(st))
    assert call(40, [0, 1], [40]) == -3 and call(40, [0, 1], [-1]) == -3          # an index out of range
    assert call(40, [0, 2], [3, 3]) == -3 and call(40, [0, 1, 2], [3, 3]) == -3   # a repeated electrode, within a fold and across
    assert call(40, [0, 1, 1], [3]) == -3                                         # an empty fold
    assert call(40, [1, 2], [3, 4]) == -3                                         # fold_ptr does not start at 0
    assert call(0, [0, 1], [0]) == -3
    assert call(40, [0, 17], list(range(17))) == _hip.ERR_CAPACITY                # 17 electrodes in one fold
    assert b"GPCSD_CV_MAX_FOLD" in lib.gpcsd_last_error(ctx._h)
    assert call(40, [0, 16], list(range(16)), R=1 << 12, nt=1 << 11) == _hip.ERR_CAPACITY       # loo's row capacity
    # ... and through the model's context, which has data
    m = _model("1d_siglist_12x40x4")
    m.cv_electrodes(folds=3)
    mctx = m._context()
    mhp, _keep2 = m._hparams(m.JITTER)
    bad = lambda ptr, idx: mctx._lib.gpcsd_cv_electrodes_resident(mctx._h, ctypes.byref(mhp), ip(np.array(ptr, dtype=np.int32)),
                                                                  ip(np.array(idx, dtype=np.int32)), len(ptr) - 1, 0)
    assert bad([0, 1], [12]) == -3 and bad([0, 2], [5, 5]) == -3 and bad([0, 0], [0]) == -3
    first = np.array(m.cv_lpd)
    m.cv_electrodes(folds=3)
    assert np.array_equal(m.cv_lpd, first)
    # the context is as usable as before: G = 2 * 2 * 1 = 4 (an exact root), u = 3 -> e = 3 / 4, pdiag = 1 / 4, u e = 9 / 4,
    # lpd = log(4) / 2 - 9 / 8 - h
    A, W, V = np.array([2.0]), np.array([1.0]), np.array([3.0])
    pd, lpd, sse, E = np.empty(1), np.empty(1), np.empty(1), np.empty(1)
    z1 = np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32)
    assert lib.gpcsd_efold_contract(ctx._h, dp(A), dp(W), dp(V), 1, 1, 1, 1, ip(z1[0]), ip(z1[1]), 1, dp(E), dp(pd), dp(lpd), dp(sse), ip(st)) == 0
    assert st[0] == 0 and E[0] == 0.75 and pd[0] == 0.25 and sse[0] == 0.5625
    assert abs(lpd[0] - (np.log(2.0) - 1.125 - cv_ref.HALF_LOG_2PI)) < 4e-15
