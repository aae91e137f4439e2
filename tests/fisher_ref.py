"""Dense NumPy statement of the per-trial scores and the expected Fisher information (TEST INFRASTRUCTURE ONLY; no GPU).

Model of loglik(): K = kron(Ks + jitter I, Kt) + sig2n I in the project's (x, t) ordering (row x * nt + t), scalar sig2n.
Natural parameters in the order of gpcsd_loglik_grad: [R, ell_s (dim), (ell_t, sigma2_t) per component, sig2n].

    s[r, i] = 1/2 y_r^T K^-1 d_i K K^-1 y_r - 1/2 tr(K^-1 d_i K)            I_ij = 1/2 tr(K^-1 d_i K K^-1 d_j K)

d_i K comes from closed-form dKs / dKt, written with the oracle's fwd_weights_*, kgl_2d, temporal_gram and the dA, dKgl
expressions of oracle.loglik_and_grad; everything else is dense solves.  tests/test_fisher.py pins these formulas on the CPU
(finite differences of the oracle's Gram matrices, the oracle's gradient, finite differences of the expected score).

`scores_and_info_eig` states the same quantities in the Kronecker eigen-basis with numpy.linalg.eigh (O(nx^3 + nt^3), for shapes
whose dense K does not fit a test); the CPU tests pin it to the dense statement."""
import numpy as np
import scipy.linalg

from oracle import gpcsd_oracle as O


def names(geom, hp):
    out = ["R"] + ["ell_s%d" % (k + 1) for k in range(geom.dim)]
    for c in range(len(hp["temporal"])):
        out += ["ell_t%d" % (c + 1), "sigma2_t%d" % (c + 1)]
    return out + ["sig2n"]


def values(geom, hp):
    v = [hp["R"]] + list(hp["ell_s"])
    for _, ell, s2 in hp["temporal"]:
        v += [ell, s2]
    return np.array(v + [float(hp["sig2n"])])


def spatial(geom, hp):
    """-> Ks = A Kgl A^T (no jitter), [dKs/dR, dKs/dell_k ..]"""
    Rv, ell = hp["R"], hp["ell_s"]
    if geom.dim == 1:
        A = O.fwd_weights_1d(geom.x, geom.gl_x, geom.gl_w, Rv)
        dx = geom.gl_x[:, None] - geom.gl_x[None, :]
        Kgl = np.exp(-0.5 * np.square(dx / ell[0]))
        dKgl = [Kgl * np.square(dx) / ell[0] ** 3]
        r = geom.gl_x[None, :] - geom.x
        q = np.square(r / Rv)
        dA = geom.gl_w[None, :] * (np.sqrt(q) - q / np.sqrt(q + 1.0)) / Rv
    else:
        A = O.fwd_weights_2d(geom.x, geom.gl_x1, geom.gl_w1, geom.gl_x2, geom.gl_w2, Rv, hp["eps"])
        g = O.expand_grid(geom.gl_x1, geom.gl_x2)
        s1 = np.square(g[:, 0][:, None] - g[:, 0][None, :])
        s2 = np.square(g[:, 1][:, None] - g[:, 1][None, :])
        Kgl = O.kgl_2d(geom.gl_x1, geom.gl_x2, ell[0], ell[1])
        dKgl = [Kgl * s1 / ell[0] ** 3, Kgl * s2 / ell[1] ** 3]
        wprod = np.prod(O.expand_grid(geom.gl_w1, geom.gl_w2), axis=1)
        w2 = np.square(g[:, 0][None, :] - geom.x[:, 0][:, None]) + np.square(g[:, 1][None, :] - geom.x[:, 1][:, None])
        dA = wprod[None, :] / np.sqrt((Rv + hp["eps"]) ** 2 + w2)
    T = A @ Kgl
    dR = dA @ T.T
    return T @ A.T, [dR + dR.T] + [A @ dk @ A.T for dk in dKgl]


def temporal(geom, hp):
    """-> Kt, [dKt/dell_c, dKt/dsigma2_c per component]"""
    tt = geom.t.reshape(-1, 1)
    d = tt - tt.T
    Kt = O.temporal_sum(hp["temporal"], geom.t)
    out = []
    for kind, ell, s2 in hp["temporal"]:
        Kc = O.temporal_gram(kind, tt, tt, ell, s2)
        out.append(Kc * np.square(d) / ell ** 3 if kind == O.SE else Kc * np.abs(d) / ell ** 2)
        out.append(Kc / s2)
    return Kt, out


def dense(geom, hp):
    """-> K, [d_i K] in slot order"""
    nx, nt = geom.x.shape[0], geom.t.shape[0]
    Ks, dKs = spatial(geom, hp)
    Ks = Ks + hp["jitter"] * np.eye(nx)
    Kt, dKt = temporal(geom, hp)
    K = O.mykron(Ks, Kt) + float(hp["sig2n"]) * np.eye(nx * nt)
    return K, [O.mykron(d, Kt) for d in dKs] + [O.mykron(Ks, d) for d in dKt] + [np.eye(nx * nt)]


def expected_score(K, dK, S):
    """1/2 tr(K^-1 d_i K K^-1 S) - 1/2 tr(K^-1 d_i K) for every direction: the mean score under data covariance S"""
    cf = scipy.linalg.cho_factor(K, lower=True)
    KiS = scipy.linalg.cho_solve(cf, S)
    out = []
    for d in dK:
        KiD = scipy.linalg.cho_solve(cf, d)
        out.append(0.5 * np.sum(KiD * KiS.T) - 0.5 * np.trace(KiD))
    return np.array(out)


def scores_and_info(geom, hp, lfp):
    """{"scores" (R, ng), "quad" (R, ng) = 1/2 y^T K^-1 d_i K K^-1 y, "trace" (ng) = 1/2 tr(K^-1 d_i K), "info" (ng, ng)}:
    scores = quad - trace, the two parts kept apart because their difference may cancel."""
    lfp = np.atleast_3d(lfp)
    nx, nt, R = lfp.shape
    K, dK = dense(geom, hp)
    cf = scipy.linalg.cho_factor(K, lower=True)
    alpha = scipy.linalg.cho_solve(cf, lfp.reshape(nx * nt, R))            # K^-1 y_r in the columns
    KiD = [scipy.linalg.cho_solve(cf, d) for d in dK]
    quad = np.stack([0.5 * np.sum(alpha * (d @ alpha), axis=0) for d in dK], axis=1)
    trace = np.array([0.5 * np.trace(m) for m in KiD])
    ng = len(dK)
    info = np.zeros((ng, ng))
    for i in range(ng):
        for j in range(i, ng):
            info[i, j] = info[j, i] = 0.5 * np.sum(KiD[i] * KiD[j].T)
    return {"scores": quad - trace[None, :], "quad": quad, "trace": trace, "info": info}


def scores_and_info_eig(geom, hp, lfp):
    """The dict of scores_and_info from the eigen-form: Ks + jitter I = Qs diag(es) Qs^T, Kt = Qt diag(et) Qt^T, D = es et^T + sig2n,
    B_r = (Qs^T Y_r Qt) / D, Ahat = Qs^T dKs Qs, Bhat = Qt^T dKt Qt (the issue's formulas, in NumPy)."""
    lfp = np.atleast_3d(lfp)
    nx, nt, R = lfp.shape
    Ks, dKs = spatial(geom, hp)
    Kt, dKt = temporal(geom, hp)
    es, Qs = np.linalg.eigh(Ks + hp["jitter"] * np.eye(nx))
    et, Qt = np.linalg.eigh(Kt)
    U = 1.0 / (es[:, None] * et[None, :] + float(hp["sig2n"]))
    B = (Qs.T @ np.moveaxis(lfp, 2, 0) @ Qt) * U[None]                     # (R, nx, nt)
    Ah = [Qs.T @ d @ Qs for d in dKs]
    Bh = [Qt.T @ d @ Qt for d in dKt]
    quad = [0.5 * np.sum((a @ B) * B * et[None, None, :], axis=(1, 2)) for a in Ah]
    quad += [0.5 * np.sum((B @ b) * B * es[None, :, None], axis=(1, 2)) for b in Bh]
    quad.append(0.5 * np.sum(B * B, axis=(1, 2)))
    sv = [np.diag(a) for a in Ah] + [es] * len(Bh) + [np.ones(nx)]
    tv = [et] * len(Ah) + [np.diag(b) for b in Bh] + [np.ones(nt)]
    ng = len(sv)
    trace = np.array([0.5 * np.sum(np.outer(sv[i], tv[i]) * U) for i in range(ng)])
    info = np.zeros((ng, ng))
    for i in range(ng):
        for j in range(ng):
            info[i, j] = 0.5 * np.sum(np.outer(sv[i] * sv[j], tv[i] * tv[j]) * U * U)
    M, N = (U * (et * et)[None, :]) @ U.T, U.T @ (U * (es * es)[:, None])
    ns = len(Ah)
    for i, a in enumerate(Ah):
        for j, a2 in enumerate(Ah):
            info[i, j] = 0.5 * np.sum(a * a2 * M)
    for i, b in enumerate(Bh):
        for j, b2 in enumerate(Bh):
            info[ns + i, ns + j] = 0.5 * np.sum(b * b2 * N)
    quad = np.stack(quad, axis=1)
    return {"scores": quad - trace[None, :], "quad": quad, "trace": trace, "info": info}
