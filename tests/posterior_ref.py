"""NumPy restatements behind tests/test_sample_posterior.py: the device generator (Philox4x32-10 + Box-Muller), the affine map
normals -> posterior draw of gpcsd_sample_posterior (Matheron's rule), and the dense posterior covariance it must reproduce.

Ordering conventions (those of include/gpcsd_hip.h): the spatial joint rows are [CSD(z) if asked; LFP(z) if asked; LFP(x)], the
temporal joint columns [t*; t]; an output vector is [csd (z, j) if asked; lfp (z, j) if asked]; a vector of normals is
[Xi (ns, ntt) C order; E (nx, nt) C order]."""
import numpy as np

import test_predict_var as PV
from oracle import gpcsd_oracle as O

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


# ------------------------------------------------------------------------------------------------ generator
def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) of 32-bit words (any integer dtype) -> (..., 4) uint64 holding the 32-bit output words."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1)


def _u53(lo, hi):
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, stream, first, count):
    """Standard normals first .. first + count - 1 of stream `stream` under `seed`."""
    first, count = int(first), int(count)
    i = np.arange(first >> 1, (first + count + 1) >> 1, dtype=np.uint64)
    ctr = np.stack([i & MASK, i >> S32, np.full_like(i, stream), np.zeros_like(i)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    w = philox4x32_10(ctr, np.broadcast_to(key, (i.size, 2)))
    u1, u2 = _u53(w[:, 0], w[:, 1]), _u53(w[:, 2], w[:, 3])
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    out = np.stack([r * np.cos(a), r * np.sin(a)], axis=-1).reshape(-1)
    off = first - 2 * (first >> 1)
    return out[off:off + count]


# ------------------------------------------------------------------------------------------------ the model's pieces
def times(name, choice):
    """"offgrid": 4 times off the training grid; "train": the first 5 training times (the temporal joint is then singular)."""
    t = PV._case(name)[0]["t"]
    return PV._offgrid(t, 4) if choice == "offgrid" else np.ascontiguousarray(t[:5])


def sites(name, choice="between"):
    """"between": 3 sites interpolated between consecutive electrodes; "electrodes": the first 3 electrodes (singular spatial joint)."""
    x = PV._case(name)[0]["x"]
    if choice == "electrodes":
        return np.ascontiguousarray(x[:3])
    return np.ascontiguousarray(0.5 * (x[:3] + x[1:4]) + 0.13 * (x[1:4] - x[:3]))


def _quantities(type):
    return {"csd": ("csd",), "lfp": ("lfp",), "both": ("csd", "lfp")}[type]


def _spatial_blocks(geom, hp, z):
    """Prior spatial covariances among CSD(z), LFP(z) and with LFP(x): dicts keyed by quantity (pairs)."""
    gz = PV._site_geometry(geom, z)
    gzhp = dict(hp)
    zz = {("csd", "csd"): O.spatial_ks_csd(gz, gzhp), ("lfp", "csd"): O.spatial_kphig(gz, gzhp, z), ("lfp", "lfp"): O.spatial_kphi(gz, gzhp)}
    zz[("csd", "lfp")] = zz[("lfp", "csd")].T
    cross = {"csd": O.spatial_kphig(geom, hp, z), "lfp": O.spatial_kphi(geom, hp, xp=z)}          # (nx, nz)
    return zz, cross


def _eig_factor(J, equilibrate):
    """F with F F^T = J (positive semi-definite) from the symmetric eigensolver; negative eigenvalues of rounding size count as zero."""
    J = np.tril(J) + np.tril(J, -1).T
    d = np.sqrt(np.diag(J)) if equilibrate else np.ones(J.shape[0])
    w, Q = np.linalg.eigh(J / np.outer(d, d))
    return d[:, None] * Q * np.sqrt(np.maximum(w, 0.0))[None, :]


def _projected_cross(name, z, tstar, type):
    """B ((x', i'), (quantity, z, j)) = (Qs (x) Qt)^T k, and (Qs, Qt, D, cross Gram k(t*, t))."""
    c, geom, hp, Qs, Qt, D = PV._case(name)
    z = np.asarray(z, dtype=np.float64)
    _, cross = _spatial_blocks(geom, hp, z)
    kts = O.temporal_sum(hp["temporal"], tstar, geom.t)                                           # (ntstar, nt)
    Pt = Qt.T @ kts.T                                                                             # (nt', ntstar)
    B = np.concatenate([np.einsum("xz,ij->xizj", Qs.T @ cross[q], Pt).reshape(D.size, -1) for q in _quantities(type)], axis=1)
    return B, Qs, Qt, D


def dense_posterior(name, z, tstar, type):
    """(posterior covariance, prior covariance) of the requested quantities at (z, t*): prior - k^T K^-1 k with
    K = (Qs (x) Qt) diag(D) (Qs (x) Qt)^T, D = es (x) et + sig2n (a noise list on the eigen-index) -- the model of predict_at."""
    c, geom, hp, _, _, _ = PV._case(name)
    z = np.asarray(z, dtype=np.float64)
    zz, _ = _spatial_blocks(geom, hp, z)
    ktt = O.temporal_sum(hp["temporal"], tstar, tstar)
    qs = _quantities(type)
    prior = np.block([[O.mykron(zz[(a, b)], ktt) for b in qs] for a in qs])
    B, _, _, D = _projected_cross(name, z, tstar, type)
    return prior - B.T @ (B / D.reshape(-1, 1)), prior


def matheron_map(name, z, tstar, type, trial=0):
    """(mean, M): the draw of trial `trial` is mean + M n for a vector n of standard normals [Xi; E]."""
    c, geom, hp, _, _, _ = PV._case(name)
    z = np.asarray(z, dtype=np.float64)
    nz, nts, nx, nt = z.shape[0], np.size(tstar), geom.x.shape[0], geom.t.shape[0]
    zz, cross = _spatial_blocks(geom, hp, z)
    qs = _quantities(type)
    rows = list(qs) + ["x"]
    blocks = dict(zz)
    for q in qs:
        blocks[("x", q)], blocks[(q, "x")] = cross[q], cross[q].T
    blocks[("x", "x")] = O.spatial_kphi(geom, hp)
    Fs = _eig_factor(np.block([[blocks[(a, b)] for b in rows] for a in rows]), True)
    tt = np.concatenate([np.asarray(tstar, dtype=np.float64).reshape(-1), geom.t.reshape(-1)])
    Ft = _eig_factor(O.temporal_sum(hp["temporal"], tt, tt), False)
    B, Qs, Qt, D = _projected_cross(name, z, tstar, type)
    Pmap = (B / D.reshape(-1, 1)).T @ O.mykron(Qs, Qt).T                                          # y (x, t) -> (quantity, z, j)
    nq = len(qs) * nz
    sig = np.broadcast_to(np.asarray(hp["sig2n"], dtype=np.float64), (nx,))
    Fn = Qs * np.sqrt(sig)[None, :]
    M = np.concatenate([O.mykron(Fs[:nq], Ft[:nts]) - Pmap @ O.mykron(Fs[nq:], Ft[nts:]), -Pmap @ O.mykron(Fn, np.eye(nt))], axis=1)
    y = np.atleast_3d(PV.C.case_lfp(c))[:, :, trial]
    return Pmap @ y.reshape(-1), M
