"""References for the power spectrum, cross-spectrum and coherence (gpcsd_amd/csrc/spectrum.hip).  The yardstick is SciPy itself, called
the way the reference's analysis scripts call it (scipy.signal.periodogram(..., axis=1) then a mean over the trials; scipy.signal.csd;
scipy.signal.coherence on the concatenated trials with nperseg = the trial length and no overlap, which equals the trial-averaged
definition), and, where a kernel is tested alone, a longdouble einsum of the definitions in include/gpcsd_hip.h.  Nothing here knows
about tiles, layouts or the device."""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FLOOR = 1e-3

# (n, nfft, window, scaling, detrend): the parameter sets the operator was designed against
OPERATOR_CASES = [(37, None, "boxcar", "density", False), (40, 64, "hann", "density", False), (37, 51, "hamming", "spectrum", "constant"),
                  (40, None, "tukey", "density", "linear"), (150, 512, "boxcar", "density", False)]


def signal(seed, nz, n, R, S=1):
    """A seeded random walk plus white noise along the time axis, (nz, n, R, S): broadband, with power at every frequency."""
    rs = np.random.RandomState(seed)
    return np.cumsum(rs.standard_normal((nz, n, R, S)), axis=1) + rs.standard_normal((nz, n, R, S))


def periodogram(x, fs=1.0, window="boxcar", nfft=None, detrend=False, scaling="density", return_onesided=True):
    """(f, per-trial periodogram shaped like x with n -> nf): the direct SciPy call along axis 1."""
    import scipy.signal as ss
    return ss.periodogram(x, fs, window, nfft, detrend, return_onesided, scaling, axis=1)


def psd(x, **kw):
    """(f, trial-averaged periodogram): x (nz, n, R) -> (nz, nf); x (nz, n, R, S) -> (nz, nf, S)."""
    f, p = periodogram(x, **kw)
    return f, p.mean(axis=2)


def coefficients(A, x, dtype=LD):
    """X = A x along axis 1 of x (nz, n, R, S) in `dtype`: (re, im, mag_re, mag_im), the parts and the magnitude sums
    sum_t |A||x| the GEMM rounding bound is relative to."""
    A = np.asarray(A)
    Ar, Ai, xx = A.real.astype(dtype), A.imag.astype(dtype), np.asarray(x, dtype=dtype)
    ax = np.abs(xx)
    return (np.einsum("jt,ztrs->zjrs", Ar, xx), np.einsum("jt,ztrs->zjrs", Ai, xx),
            np.einsum("jt,ztrs->zjrs", np.abs(Ar), ax), np.einsum("jt,ztrs->zjrs", np.abs(Ai), ax))


def cross_spectrum(re, im, dtype=LD):
    """(s_re, s_im) (S, nrow, nz, nz) = 1/R sum_r X_a conj(X_b) from coefficients (nz, nrow, R, S), in `dtype`."""
    xr, xi = np.asarray(re, dtype=dtype), np.asarray(im, dtype=dtype)
    R = xr.shape[2]
    s_re = (np.einsum("ajrs,bjrs->sjab", xr, xr) + np.einsum("ajrs,bjrs->sjab", xi, xi)) / dtype(R)
    s_im = (np.einsum("ajrs,bjrs->sjab", xi, xr) - np.einsum("ajrs,bjrs->sjab", xr, xi)) / dtype(R)
    return s_re, s_im


def coherence(s_re, s_im):
    """(coh, den): |Sx|^2 / (S_aa S_bb) with 0 where the denominator is 0, and the denominator S_aa S_bb itself."""
    d = np.diagonal(s_re, axis1=-2, axis2=-1)
    den = d[..., :, None] * d[..., None, :]
    num = s_re * s_re + s_im * s_im
    return np.where(den > 0, num / np.where(den > 0, den, 1), 0), den


def scipy_csd_mean(x, rows, **kw):
    """Sx[j, a, b] (nrow, nz, nz) as SciPy defines it: scipy.signal.csd(x_b, x_a) per trial (SciPy conjugates its FIRST argument),
    averaged over the trials of x (nz, n, R)."""
    import scipy.signal as ss
    nz, n, R = x.shape
    xt = np.moveaxis(x, 1, 2)                                                    # (nz, R, n)
    _, s = ss.csd(xt[None, :], xt[:, None], nperseg=n, noverlap=0, **kw)         # [a, b] = csd(x_b, x_a)
    return np.moveaxis(s.mean(axis=2), 2, 0)[np.asarray(rows)]


def scipy_coherence(x, rows, **kw):
    """coh[j, a, b] (nrow, nz, nz): scipy.signal.coherence on the concatenated trials of x (nz, n, R), one segment per trial."""
    import scipy.signal as ss
    nz, n, R = x.shape
    cat = np.moveaxis(x, 1, 2).reshape(nz, R * n)
    f, c = ss.coherence(cat[:, None], cat[None, :], nperseg=n, noverlap=0, **kw)
    return f[np.asarray(rows)], np.moveaxis(c, 2, 0)[np.asarray(rows)]


@functools.lru_cache(maxsize=None)
def coherence_case(S):
    """The cross-spectrum test's input: nz = 70 sites (a diagonal and an off-diagonal 64-wide tile), n = 40, R = 5 trials, S draws;
    white noise plus a sinusoid of 0.2 cycles per sample that all sites share with a site-dependent phase and gain, so that every site
    has power at the three kept frequencies (indices 7, 8, 9 of a Hann-windowed 64-point periodogram, around the sinusoid) and the
    pairs are neither incoherent nor fully coherent.  Returns (x, A, re, im, s_re, s_im, coh, ok): the field, the operator, its
    coefficients rounded to double (the kernel's input), the longdouble cross-spectrum and coherence OF THOSE DOUBLES, and the mask of
    the entries whose S_aa S_bb is at least (FLOOR max S_aa)^2.  Asserts, here on the CPU, that the reference alone leaves fewer than
    1 % of the entries under that floor.  Computed once and left unchanged."""
    from gpcsd_amd import utility_functions as UF
    nz, n, R = 70, 40, 5
    rs = np.random.RandomState(2024 + S)
    tt = np.arange(n)[None, :, None, None]
    gain = rs.uniform(0.5, 2.0, (nz, 1, 1, 1))
    phase = rs.uniform(-np.pi, np.pi, (nz, 1, 1, 1))
    trial = rs.uniform(-np.pi, np.pi, (1, 1, R, S))
    x = gain * np.cos(2 * np.pi * 0.2 * tt + phase + trial) + rs.standard_normal((nz, n, R, S))
    _, A = UF.spectral_operator(n, fs=1.0, nfft=64, window="hann", rows=[7, 8, 9])
    re, im = (np.asarray(v, dtype=np.float64) for v in coefficients(A, x)[:2])
    s_re, s_im = cross_spectrum(re, im)
    coh, den = coherence(s_re, s_im)
    top = np.max(np.diagonal(s_re, axis1=-2, axis2=-1))
    ok = den >= (FLOOR * top) ** 2
    assert np.count_nonzero(~ok) < 0.01 * ok.size, ("entries under the floor", np.count_nonzero(~ok), ok.size)
    for v in (x, A, re, im, s_re, s_im, coh, ok):
        v.setflags(write=False)
    return x, A, re, im, s_re, s_im, coh, ok
