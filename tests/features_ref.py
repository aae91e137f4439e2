"""NumPy restatement of the region features (gpcsd_region_features; csrc/features.hip): extrema and first-occurrence indices with
np.argmax / np.argmin on a region's points in row-major (z, t) order, sums in np.longdouble.  Not imported by the product."""
import numpy as np

NFEAT = 10


def isd_from_var(var, floor=1e-10):
    """1 / sqrt(var) where var > floor * max(var), 0 elsewhere: the documented rule of sample_features(band=True)."""
    var = np.asarray(var, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(var > floor * var.max(), 1.0 / np.sqrt(var), 0.0)


def region_slots(x, labels, J, tau=None, zeta=None, mean=None, isd=None, S=1):
    """x (nz, nts, M) -> (feat (J, NFEAT, M) longdouble, mag (J, NFEAT, M) longdouble, npts (J,)): the slots the header documents and,
    for the sum slots 4-8, mag = sum |x c| over the region (c the coordinate; 1 for slots 4-5) -- what a rounding bound scales with.
    A region without a point: -inf, -1, +inf, -1, zeros, and -inf in slot 9 when mean / isd are given (NaN otherwise)."""
    ld = np.longdouble
    x = np.asarray(x, dtype=np.float64)
    nz, nts, M = x.shape
    labels = np.asarray(labels)
    assert labels.shape == (nz, nts)
    tau = np.arange(nts, dtype=np.float64) if tau is None else np.asarray(tau, dtype=np.float64).reshape(-1)
    zeta = np.arange(nz, dtype=np.float64) if zeta is None else np.asarray(zeta, dtype=np.float64)
    zeta = zeta.reshape(nz, -1)
    flat, lab = x.reshape(nz * nts, M), labels.reshape(-1)
    feat, mag = np.zeros((J, NFEAT, M), dtype=ld), np.zeros((J, NFEAT, M), dtype=ld)
    npts = np.zeros(J, dtype=np.int64)
    band = mean is not None
    if band:
        mflat = np.asarray(mean, dtype=np.float64).reshape(nz * nts, -1)[:, np.arange(M) // int(S)]          # (points, M)
        iflat = np.asarray(isd, dtype=np.float64).reshape(-1)
    for j in range(1, J + 1):
        pts = np.flatnonzero(lab == j)                      # ascending: row-major order
        npts[j - 1] = pts.size
        f = feat[j - 1]
        f[9] = -np.inf if band else np.nan
        if pts.size == 0:
            f[0], f[1], f[2], f[3] = -np.inf, -1, np.inf, -1
            continue
        v = flat[pts]                                       # (n, M)
        a, b = np.argmax(v, axis=0), np.argmin(v, axis=0)   # first occurrences
        f[0], f[1] = v[a, np.arange(M)], pts[a]
        f[2], f[3] = v[b, np.arange(M)], pts[b]
        vl, al = v.astype(ld), np.abs(v).astype(ld)
        coords = [None, None, tau[pts % nts], zeta[pts // nts, 0], zeta[pts // nts, 1] if zeta.shape[1] == 2 else np.zeros(pts.size)]
        f[4], mag[j - 1, 4] = vl.sum(axis=0), al.sum(axis=0)
        f[5] = mag[j - 1, 5] = al.sum(axis=0)
        for k in (2, 3, 4):
            c = coords[k].astype(ld)[:, None]
            f[4 + k], mag[j - 1, 4 + k] = (al * c).sum(axis=0), (al * np.abs(c)).sum(axis=0)
        if band:
            f[9] = (np.abs(vl - mflat[pts].astype(ld)) * iflat[pts].astype(ld)[:, None]).max(axis=0)
    return feat, mag, npts


def check_slots(got, ref, mag, npts, band, what=""):
    """The gates of the tests: slots 0-3 exactly; slots 4-8 within (n + 2) 2^-53 sum |x c| (the bound of a fixed-order sum of rounded
    products); slot 9 within `band` relative (None: NaN expected).  Returns the largest ratio to the sum bound (printed by callers)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got[:, :4], ref[:, :4].astype(np.float64)), what + ": extrema or their first occurrences differ"
    bound = (npts[:, None, None] + 2) * 2.0 ** -53 * mag[:, 4:9]
    err = np.abs(got[:, 4:9].astype(np.longdouble) - ref[:, 4:9])
    assert np.all(err <= bound), (what, float(np.max(err - bound)))
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))) if bound.size else 0.0
    if band is None:
        assert np.all(np.isnan(got[:, 9])), what + ": slot 9 without a mean is NaN"
    else:
        r9 = ref[:, 9]
        fin = np.isfinite(r9.astype(np.float64))
        assert np.array_equal(got[:, 9][~fin], r9.astype(np.float64)[~fin]), what + ": slot 9 of a region without a point"
        assert np.all(np.abs(got[:, 9][fin].astype(np.longdouble) - r9[fin]) <= band * np.abs(r9[fin])), what + ": slot 9"
    return ratio
