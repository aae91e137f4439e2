"""CPU: the mathematics of the masked calls before any kernel runs (tests/masked_ref.py).  The dense statement (Cholesky of K_OO)
and the Schur restatement on the full-grid decomposition must agree within the project's parity gate for every case and pattern
-- weights on the grid, predictions on and off the grid, both parts of the log-likelihood --, and with nothing missing both are
the oracle's predict and loglik."""
import numpy as np
import pytest

import masked_ref as MR
import test_predict_at as PA
from helpers import relerr
from oracle import gpcsd_oracle as O

GATE = PA.GATE


def _rows_err(got, ref):
    return [relerr(got[:, k], ref[:, k]) for k in range(2)]


@pytest.mark.parametrize("pattern", MR.PATTERNS)
@pytest.mark.parametrize("name", MR.CASES)
def test_schur_equals_dense(name, pattern):
    d, s = MR.dense(name, pattern), MR.schur(name, pattern)
    c = MR.case(name)["c"]
    assert d["n_obs"] == s["n_obs"] == int(MR.mask3(MR.mask_for(name, pattern), c["R_trials"]).sum())
    errs = _rows_err(s["rows"], d["rows"])
    print("masked ref %s %s: log det %.2e quad %.2e" % (name, pattern, errs[0], errs[1]))
    assert max(errs) < GATE
    for z, ts, tag in ((c["x"], c["t"], "grid"), (MR.sites(name), PA._offgrid(c["t"], 4), "off")):
        pd, ps = MR.predictions(name, d["alpha"], z, ts), MR.predictions(name, s["alpha"], z, ts)
        PA._assert_matches(ps, pd, len(c["temporal"]), "%s %s %s" % (name, pattern, tag))
    if pattern == "none_observed":
        assert not d["alpha"][1].any() and not s["alpha"][1].any() and not d["rows"][1].any() and not s["rows"][1].any()


@pytest.mark.parametrize("name", MR.CASES)
def test_nothing_missing_is_the_oracle(name):
    cs = MR.case(name)
    c, geom, hp, lfp = cs["c"], cs["geom"], cs["hp"], cs["lfp"]
    R = lfp.shape[2]
    ref = O.predict(geom, hp, lfp, c["x"], c["t"], "both")
    B = np.matmul(np.matmul(cs["Qs"].T, np.moveaxis(lfp, 2, 0)), cs["Qt"])
    parts = np.array([R * np.sum(np.log(cs["D"])), np.sum(np.square(B) / cs["D"][None])])
    for stmt in (MR.dense, MR.schur):
        got = stmt(name, "all")
        PA._assert_matches(MR.predictions(name, got["alpha"], c["x"], c["t"]), ref, len(c["temporal"]), name + " " + stmt.__name__)
        tot = got["rows"].sum(0)
        errs = [abs(tot[k] - parts[k]) / abs(parts[k]) for k in range(2)]
        print("masked ref %s %s all observed vs loglik parts: %.2e %.2e" % (name, stmt.__name__, errs[0], errs[1]))
        assert max(errs) < GATE
        ll = O.loglik(geom, hp, lfp)                                      # (hp carries no jitter)
        assert abs(-0.5 * tot[0] - 0.5 * tot[1] - ll) < GATE * abs(ll)
        assert got["n_obs"] == lfp.size


def test_the_2d_mask_is_its_repetition():
    name = MR.CASES[0]
    m2 = MR.mask_for(name, "electrode2d")
    assert m2.ndim == 2 and not m2.all() and (~m2).sum() == m2.shape[1]
    R = MR.case(name)["lfp"].shape[2]
    assert MR.mask3(m2, R).shape == m2.shape + (R,) and MR.dense(name, "electrode2d")["n_obs"] == R * int(m2.sum())
