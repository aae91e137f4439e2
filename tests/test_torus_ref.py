"""CPU checks of the dense extended-precision statement of the torus graph estimator (tests/torus_ref.py) itself: it recovers a
known coupling, weights are resampling, and its p-values are uniform under independence.  tests/test_torus_graph.py pins the device
to this reference."""
import numpy as np

import torus_ref as T


def test_von_mises_coupling_is_recovered():
    """d = 2 with x_1 - x_2 ~ vonMises(mu, kappa): the model is exact with phi = kappa (cos mu, sin mu)."""
    rng = np.random.default_rng(1)
    N, mu, kappa = 4000, 0.7, 1.5
    x2 = rng.uniform(-np.pi, np.pi, N)
    x = np.stack([x2 + rng.vonmises(mu, kappa, N), x2])
    res = T.fit(*T.phasors(x), dtype=np.float64)
    truth = kappa * np.array([np.cos(mu), np.sin(mu)])
    print("von Mises: phi %s, truth %s" % (res["phi"][0], truth))
    assert np.max(np.abs(res["phi"][0] - truth)) <= 0.05
    assert res["pvals"][0] < 1e-6
    assert abs(T.cond_coupling(res["phi"])[0] - 0.5962) <= 0.02                  # I1(1.5) / I0(1.5)


def test_weights_are_resampling():
    rng = np.random.default_rng(2)
    d, N = 4, 60
    x = rng.vonmises(0, 1, (d, N)) + rng.vonmises(0, 2, N)
    u_re, u_im = T.phasors(x)
    idx = rng.integers(0, N, N)
    w = np.bincount(idx, minlength=N)
    a = T.fit(u_re, u_im, weights=w)
    b = T.fit(u_re[:, np.sort(idx)], u_im[:, np.sort(idx)])
    e_phi = float(np.max(np.abs(a["phi"] - b["phi"])))
    e_chi = float(np.max(np.abs(a["chi2"] - b["chi2"]) / np.maximum(np.abs(b["chi2"]), 1)))
    print("weights against resampled columns: phi %.2e, chi2 %.2e" % (e_phi, e_chi))
    assert e_phi <= 1e-12 and e_chi <= 1e-12


def test_null_p_values_are_uniform():
    rng = np.random.default_rng(3)
    d, N, reps = 4, 150, 60
    pv = []
    for _ in range(reps):
        x = rng.uniform(-np.pi, np.pi, (d, N))
        pv.append(T.fit(*T.phasors(x), dtype=np.float64)["pvals"])
    pv = np.concatenate(pv)
    q = np.quantile(pv, [0.1, 0.25, 0.5, 0.75, 0.9])
    print("null p-value quantiles at 0.1 / 0.25 / 0.5 / 0.75 / 0.9: " + " / ".join("%.2f" % v for v in q))
    assert 0.35 <= q[2] <= 0.65


def test_transposed_back_substitution():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((12, 12))
    L = np.linalg.cholesky(A @ A.T + 12 * np.eye(12)).astype(T.LD)
    B = rng.standard_normal((12, 3))
    X = T.solve_lower_trans(L, B)
    assert np.max(np.abs(L.T @ X - B)) <= 1e-15
    assert np.max(np.abs(T.cholesky(L @ L.T) - L)) <= 1e-15
