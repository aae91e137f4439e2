"""NumPy references for band phase and phase locking (gpcsd_amd/csrc/phase.hip): plain transcriptions of the definitions in
include/gpcsd_hip.h (gpcsd_analytic, gpcsd_plv), written as einsums; nothing here knows about tiles, layouts or the device."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def signal(seed, nz, n, M):
    """A seeded random walk plus white noise along the time axis, (nz, n, M): broadband, with power in every band the tests use."""
    rs = np.random.RandomState(seed)
    return np.cumsum(rs.standard_normal((nz, n, M)), axis=1) + rs.standard_normal((nz, n, M))


def filters():
    """The operator cases: name -> (n, kind, design).  Order-1 second-order-section band-passes and the order-3 transfer-function
    form, designed here with SciPy as a caller would."""
    import scipy.signal as ss
    return {
        "sos37": (37, "sos", ss.butter(1, (80.0, 120.0), btype="bandpass", fs=1000.0, output="sos")),
        "sos95": (95, "sos", ss.butter(1, (20.0, 24.0), btype="bandpass", fs=2500.0, output="sos")),
        "sos40": (40, "sos", ss.butter(1, (80.0, 120.0), btype="bandpass", fs=1000.0, output="sos")),
        "ba40": (40, "ba", ss.butter(3, (80.0, 120.0), btype="bandpass", fs=1000.0)),
        "ba100": (100, "ba", ss.butter(3, (8.0, 12.0), btype="bandpass", fs=1000.0)),
    }


def direct_analytic(x, kind=None, design=None, axis=1):
    """The direct SciPy call an analysis script makes: filter along `axis`, then the analytic signal."""
    import scipy.signal as ss
    if kind == "sos":
        x = ss.sosfiltfilt(design, x, axis=axis)
    elif kind == "ba":
        x = ss.filtfilt(design[0], design[1], x, axis=axis)
    return ss.hilbert(x, axis=axis)


def analytic(A, x):
    """(complex analytic signal (nz, nsel, M), magnitude sums (mag_re, mag_im) the GEMM rounding bound is relative to)."""
    A = np.asarray(A)
    w = np.einsum("jt,ztm->zjm", A, x)
    ax = np.abs(x)
    return w, (np.einsum("jt,ztm->zjm", np.abs(A.real), ax), np.einsum("jt,ztm->zjm", np.abs(A.imag), ax))


def phasors(w):
    """amp, phase, unit phasor of a complex field with the library's convention at zero: phase 0, phasor (1, 0)."""
    amp = np.abs(w)
    zero = amp == 0
    u = np.where(zero, 1.0, w / np.where(zero, 1.0, amp))
    return amp, np.where(zero, 0.0, np.angle(w)), u


def plv(u_re, u_im, dtype=np.float64):
    """c (S, nsel, nz, nz) complex pair (c_re, c_im) and plv from unit phasors (nz, nsel, R, S), in `dtype`."""
    ur, ui = np.asarray(u_re, dtype=dtype), np.asarray(u_im, dtype=dtype)
    R = ur.shape[2]
    c_re = (np.einsum("ajrs,bjrs->sjab", ur, ur) + np.einsum("ajrs,bjrs->sjab", ui, ui)) / dtype(R)
    c_im = (np.einsum("ajrs,bjrs->sjab", ui, ur) - np.einsum("ajrs,bjrs->sjab", ur, ui)) / dtype(R)
    return c_re, c_im, np.sqrt(c_re * c_re + c_im * c_im)


def wrap(d):
    """Phase difference wrapped into [-pi, pi)."""
    return (np.asarray(d) + np.pi) % (2.0 * np.pi) - np.pi
