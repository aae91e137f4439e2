"""Grid helpers (host) and the Kronecker-eigen primitive (GPU).

Mirrors src/gpcsd/utility_functions.py: normalize :7-8, sort_grid :10-13, expand_grid :15-23, reduce_grid
:25-33, mykron :35-42 (API parity only -- never on the fast path), comp_eig_D :44-64 (two HIP symmetric
eigendecompositions + the D vector).  analytic_operator, band_phase, plv, plv_from_sums have no counterpart in the package: they are
the band-pass + Hilbert + phase-locking step the reference's analysis scripts end with, as one linear operator (host) and two HIP
launches (csrc/phase.hip); torus_graph, the conditional phase coupling those scripts fit next, likewise (csrc/torus.hip);
spectral_operator, power_spectrum, cross_spectrum, spectrum_from_sums: the periodogram those scripts take of every prediction, its
mean over the trials and the coherence of all site pairs (csrc/spectrum.hip); trial_shift_objective: the objective of the per-trial
shift fits those scripts run (auditory_lfp/fit_mean_function.py:306-321) with its analytic gradient (csrc/shift.hip);
roi_weights: box averages and contrasts over (z, t*) as the dense weights of predict_functionals (host only); region_features,
features_from_slots, simultaneous_band: extrema, their place and time, centres of mass (auditory_lfp/fit_mean_function.py:350-353
takes them of one segmented field on the host) and standardised suprema over labelled regions, per column of a field
(csrc/features.hip)."""
import numpy as np

from . import _hip


def normalize(x):
    """Scale each trial (last axis) by its max |value| over space and time."""
    x = np.asarray(x)
    return x / np.max(np.abs(x), axis=(0, 1))


def sort_grid(x):
    """Order (n, 2) points by first coordinate, ties by second (stable)."""
    x = np.asarray(x)
    by_second = x[np.argsort(x[:, 1])]
    return by_second[np.argsort(by_second[:, 0], kind="mergesort")]


def expand_grid(x1, x2):
    """All (a, b) pairs, x1-major: (len(x1)*len(x2), 2)."""
    a = np.asarray(x1, dtype=np.float64).reshape(-1)
    b = np.asarray(x2, dtype=np.float64).reshape(-1)
    return np.stack([np.repeat(a, b.size), np.tile(b, a.size)], axis=1)


def reduce_grid(x):
    """Inverse of expand_grid: sorted unique values of each column."""
    x = np.asarray(x)
    return np.unique(x[:, 0]), np.unique(x[:, 1])


def mykron(A, B):
    """Materialised Kronecker product (a1*b1, a2*b2); kept for API parity with the reference."""
    A = np.asarray(A)
    B = np.asarray(B)
    return (A[:, None, :, None] * B[None, :, None, :]).reshape(A.shape[0] * B.shape[0], A.shape[1] * B.shape[1])


def comp_eig_D(Ks, Kt, sig2n):
    """Eigenvectors of Ks and Kt and the diagonal D of kron(Ks,Kt) + sig2n*I in the Kronecker eigenbasis.

    D[x*nt + i] = evals_s[x]*evals_t[i] + sig2n   (scalar) or + sig2n[x] (per-electrode list, indexed by the
    ascending eigen-index x exactly as the reference does).  Returns (evec_s, evec_t, Dvec)."""
    return _hip.default_context().eig_D(Ks, Kt, sig2n)


def whitened_quadratic_forms(evec_s, evec_t, Dvec, resid):
    """Per-trial `sum((evec_s.T @ resid_b @ evec_t)**2 / Dvec)` for residuals `resid` of shape (nx, nt) or (nx, nt, nb),
    given the outputs of `comp_eig_D`.  Not a function of the reference package itself: it is the projection step of
    `loglik` (gpcsd1d.py:124-127) as reused by downstream per-trial objectives (auditory_lfp/fit_mean_function.py:311-321),
    batched over trials on the GPU."""
    from . import _hip
    return _hip.default_context().whitened_quad(evec_s, evec_t, Dvec, resid)


def analytic_operator(n, sos=None, ba=None, at=None, **filter_kwargs):
    """The complex matrix A (nsel, n), complex128, of "zero-phase band-pass, then analytic signal" along a time axis of length n:
    `A @ x == scipy.signal.hilbert(filt(x))` with filt = `scipy.signal.sosfiltfilt(sos, .)`, `scipy.signal.filtfilt(b, a, .)` for
    ba = (b, a), or nothing (pure Hilbert transform).  Both steps are linear in the signal for a fixed length (the filters'
    edge padding and initial conditions included), so the operator is their action on the n x n identity along axis 0;
    filter_kwargs (padtype, padlen, ...) go to the filter call.  at: time indices to keep, in any order (default: all) -- keeping a
    time is keeping a row.  Filter design stays with the caller (scipy.signal.butter ...), as in the reference's scripts
    (auditory_lfp/fit_gpcsd_baseline.py:303-334, neuropixels/fit_gpcsd2d.py:147-159).

    Prefer `sos` for narrow bands: the operator reproduces the direct call to 1e-14 of the largest entry with second-order
    sections, but only to about 1e-8 for an order-3 transfer-function (b, a) band-pass of 8-12 Hz at 1 kHz over 100 samples --
    that is the conditioning of the (b, a) form itself (the two calls, each as good as the other, differ by that much)."""
    import scipy.signal
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    if sos is not None and ba is not None:
        raise ValueError("give sos or ba, not both")
    F = np.eye(n)
    if sos is not None:
        F = scipy.signal.sosfiltfilt(sos, F, axis=0, **filter_kwargs)
    elif ba is not None:
        F = scipy.signal.filtfilt(ba[0], ba[1], F, axis=0, **filter_kwargs)
    elif filter_kwargs:
        raise ValueError("filter arguments without a filter: %s" % sorted(filter_kwargs))
    A = scipy.signal.hilbert(F, axis=0)
    if at is not None:
        A = A[np.asarray(at, dtype=np.intp).reshape(-1)]
    return np.ascontiguousarray(A, dtype=np.complex128)


def band_phase(x, A, want=("phase",), resident=False, ctx=None):
    """Band phase along the time axis of x (nz, n, M) or (nz, n, R, S) -- a NumPy array, or a `_hip.DeviceArray` such as a resident
    prediction (`m.csd_pred`, `m.csd_pred_list[c]`) or resident posterior draws -- under the operator A (nsel, n) of
    `analytic_operator`: dict with the wanted ones of "phase" (atan2), "amp" (hypot), "u_re", "u_im" (the unit phasor; (1, 0) and
    phase 0 where amp == 0), each shaped like x with n -> nsel.  One fp64 MFMA product with the nonlinear functions in its epilogue;
    outputs not asked for are not stored.  A device input is read where it lies (no copy over PCIe); with resident=True its results
    are zero-copy views of the library's buffers "phase_out", "phase_amp", "phasor_re", "phasor_im" (valid until the next call that
    writes them), otherwise host arrays.  ctx: the `_hip.Context` a host input is sent to (default: the process-wide one; a device
    input brings its own).  No reference counterpart."""
    A = np.asarray(A)
    shape = tuple(int(v) for v in x.shape)
    if len(shape) not in (3, 4):
        raise ValueError("x must be (nz, n, M) or (nz, n, R, S)")
    nz, n = shape[:2]
    M = int(np.prod(shape[2:]))
    out_shape = (nz, A.shape[0]) + shape[2:]
    if isinstance(x, _hip.DeviceArray):
        if x.base is None:
            raise ValueError("band_phase: the device array is not a view of a named buffer of the library")
        ctx = x._owner
        res = ctx.analytic_resident(x.base[0], x.base[1], (nz, n, M), A, want)
        if resident:
            return {k: _hip.DeviceArray(v.ptr, out_shape, ctx, v.name) for k, v in res.items()}
        return {k: ctx.fetch(v.name, out_shape) for k, v in res.items()}
    if resident:
        raise ValueError("resident=True needs a device input")
    res = (ctx or _hip.default_context()).analytic(np.asarray(x, dtype=np.float64).reshape(nz, n, M), A, want)
    return {k: v.reshape(out_shape) for k, v in res.items()}


def _region_labels(labels, nz, n):
    """The label map of region_features / sample_features as int32 (nz, n) and the number of regions J = max(labels.max(), 1);
    ValueError on another shape or a negative label, GPCSDCapacityError beyond _hip.MAX_REGIONS.  No device call."""
    labels = np.asarray(labels)
    if labels.shape != (nz, n):
        raise ValueError("labels must have shape (%d, %d), not %s" % (nz, n, labels.shape))
    if not np.issubdtype(labels.dtype, np.integer) and not np.array_equal(labels, np.floor(labels)):
        raise ValueError("labels must be integers: 0 for the background, 1..J for the regions")
    if labels.size and labels.min() < 0:
        raise ValueError("a label is out of range: labels are 0 for the background and 1..J for the regions, not %d" % labels.min())
    J = max(int(labels.max()) if labels.size else 0, 1)
    if J > _hip.MAX_REGIONS:
        raise _hip.GPCSDCapacityError("%d regions; at most %d (GPCSD_MAX_REGIONS)" % (J, _hip.MAX_REGIONS))
    return np.ascontiguousarray(labels, dtype=np.int32), J


def _region_coordinates(tstar, z, nz, n):
    tstar = np.arange(n, dtype=np.float64) if tstar is None else np.asarray(tstar, dtype=np.float64).reshape(-1)
    z = np.arange(nz, dtype=np.float64) if z is None else np.asarray(z, dtype=np.float64)
    z = z.reshape(-1, 1) if z.ndim == 1 else z
    if tstar.size != n or z.ndim != 2 or z.shape[0] != nz or z.shape[1] not in (1, 2):
        raise ValueError("tstar must hold %d times and z (%d,) or (%d, 1 or 2) sites" % (n, nz, nz))
    return tstar, z


def features_from_slots(feat, tail, tstar, z, band):
    """The dict region_features returns from the raw slots feat (J, NFEAT, M) of the library (include/gpcsd_hip.h lists them), the
    columns reshaped to `tail`; tstar (n,) and z (nz, dim) are the coordinates the call was given."""
    feat = np.asarray(feat)
    J, n = feat.shape[0], tstar.size
    f = feat.reshape((J, _hip.NFEAT) + tuple(tail))
    out = {"slots": f, "max": f[:, 0], "min": f[:, 2], "sum": f[:, 4], "abs_sum": f[:, 5]}
    for name, when, slot in (("argmax", "peak_time", 1), ("argmin", "trough_time", 3)):
        flat = f[:, slot].astype(np.int64)
        empty = flat < 0
        site, time = np.where(empty, -1, flat // n), np.where(empty, -1, flat % n)
        out[name] = np.stack([site, time], axis=-1)
        out[when] = np.where(empty, np.nan, tstar[np.where(empty, 0, time)])
    with np.errstate(invalid="ignore", divide="ignore"):
        none = f[:, 5] == 0
        out["com_time"] = np.where(none, np.nan, f[:, 6] / f[:, 5])
        out["com_site"] = np.stack([np.where(none, np.nan, f[:, 7 + k] / f[:, 5]) for k in range(z.shape[1])], axis=-1)
    if band:
        out["supdev"] = f[:, 9]
    return out


def region_features(x, labels, tstar=None, z=None, mean=None, isd=None, resident=False, ctx=None):
    """Nonlinear summaries of a field over labelled regions of the (z, t) plane, for every column: x is (nz, n, M) or (nz, n, R, S) --
    a NumPy array, or a `_hip.DeviceArray` such as a resident prediction or resident posterior draws, read where it lies --, labels
    an integer map (nz, n) with 0 for the background and 1..J for the regions (J = labels.max(); e.g. a watershed segmentation of
    the evoked prediction), tstar (n,) and z (nz,) or (nz, dim) the coordinates (default: the indices).  Returns a dict of arrays
    shaped (J,) + x.shape[2:]:

      max, min, sum, abs_sum     over the region's points
      argmax, argmin             integer (..., 2) = (site index, time index) of the FIRST occurrence in row-major (z, t) order;
                                 -1 for a region without a point
      peak_time, trough_time     tstar at those indices (NaN for a region without a point)
      com_time, com_site         centre of mass of |x|: sum |x| t / sum |x|, and (..., dim) likewise in z; NaN where abs_sum == 0
      supdev                     with mean (nz, n, R) and isd (nz, n): max over the region of |x - mean| isd, the trial of a column
                                 being its index over x.shape[2:] divided by S (-inf for a region without a point)
      slots                      the raw values of the library, (J, NFEAT) + x.shape[2:], of which the entries above are views or
                                 quotients (include/gpcsd_hip.h lists them): the sums |x| t and |x| z before the division

    One pass over the field on the device (csrc/features.hip); sums in a fixed order that depends on the labels alone, so the same
    call returns the same bits and a column's values do not depend on which other columns are passed with it.  NaN inputs are not
    supported.  resident=True (device input only) returns {"feat": zero-copy view (J, NFEAT) + x.shape[2:] of the library's
    "feat_out"} -- the raw slots, which `features_from_slots` turns into the dict above.  ctx as in band_phase.  The centre of mass
    is what the reference's analysis takes of each segmented region of one field on the host (scipy.ndimage.center_of_mass,
    auditory_lfp/fit_mean_function.py:350-353); as a routine over columns it has no reference counterpart."""
    shape = tuple(int(v) for v in x.shape)
    if len(shape) not in (3, 4):
        raise ValueError("x must be (nz, n, M) or (nz, n, R, S)")
    nz, n = shape[:2]
    M = int(np.prod(shape[2:]))
    S = shape[3] if len(shape) == 4 else 1
    labels, J = _region_labels(labels, nz, n)
    tstar, z = _region_coordinates(tstar, z, nz, n)
    if (mean is None) != (isd is None):
        raise ValueError("give both mean and isd, or neither")
    if mean is not None and len(shape) == 3:
        S = 1 if np.ndim(mean) != 3 or np.shape(mean)[2] == 0 or M % np.shape(mean)[2] else M // np.shape(mean)[2]
    if isinstance(x, _hip.DeviceArray):
        if x.base is None:
            raise ValueError("region_features: the device array is not a view of a named buffer of the library")
        ctx = x._owner
        view = ctx.region_features_resident(x.base[0], x.base[1], (nz, n, M), labels, J, tstar, z, mean, isd, S)
        if resident:
            return {"feat": _hip.DeviceArray(view.ptr, (J, _hip.NFEAT) + shape[2:], ctx, view.name)}
        feat = view.numpy()
    else:
        if resident:
            raise ValueError("resident=True needs a device input")
        feat = (ctx or _hip.default_context()).region_features(np.asarray(x, dtype=np.float64).reshape(nz, n, M), labels, J, tstar, z,
                                                                mean, isd, S)
    return features_from_slots(feat, shape[2:], tstar, z, mean is not None)


def simultaneous_band(supdev, level=0.95):
    """The half-width q, in posterior standard deviations, of a simultaneous band over each region: the `level` quantile over the
    draws (last axis) of supdev (J, ntrials, nsamples) as region_features / sample_features return it.  mean +- q sd then covers the
    whole region with posterior probability `level` (up to the Monte-Carlo error of the quantile).  Host NumPy."""
    if not 0.0 < float(level) < 1.0:
        raise ValueError("level must lie in (0, 1)")
    return np.quantile(np.asarray(supdev, dtype=np.float64), float(level), axis=-1)


def plv_from_sums(sums, ntrials):
    """(plv, c) from sum_r u_a conj(u_b) over `ntrials` trials, given as a complex array or as the stacked pair (2, ...) of its real
    and imaginary parts -- the host-side combine of a trial-sharded job: every rank forms R_local * c of its block, the sums add."""
    sums = np.asarray(sums)
    if not np.iscomplexobj(sums):
        sums = sums[0] + 1j * sums[1]
    c = sums / float(ntrials)
    return np.abs(c), c


def plv(phasors_or_phase, resident=False, ctx=None):
    """Phase-locking value of ALL site pairs over the trials.  Input: the dict `band_phase` returns (with "u_re" and "u_im"), a pair
    (u_re, u_im), or a host array of phases (cos / sin are then formed on the host), each array (nz, nsel, R) or (nz, nsel, R, S)
    with S draws per trial.  Returns (plv, c): plv[j, a, b] = |c[j, a, b]|, c[j, a, b] = mean over the trials of
    exp(i (phase_a - phase_b)) at kept time j -- the complex mean resultant, whose angle is the mean phase difference -- of shape
    (nsel, nz, nz), or (S, nsel, nz, nz) for a four-dimensional input.  One launch for all pairs, times and draws; plv and c.real
    are symmetric and c.imag antisymmetric bit for bit, and the same call gives the same bits.  Phasors that are resident views
    (band_phase(..., resident=True)) are read where they lie; resident=True then returns zero-copy views (plv, (c_re, c_im))
    instead of host arrays.  ctx as in band_phase.  No reference counterpart."""
    if isinstance(phasors_or_phase, dict):
        u_re, u_im = phasors_or_phase["u_re"], phasors_or_phase["u_im"]
    elif isinstance(phasors_or_phase, (tuple, list)):
        u_re, u_im = phasors_or_phase
    else:
        ph = np.asarray(phasors_or_phase, dtype=np.float64)
        u_re, u_im = np.cos(ph), np.sin(ph)
    shape = tuple(int(v) for v in u_re.shape)
    if len(shape) not in (3, 4) or tuple(u_im.shape) != shape:
        raise ValueError("the phasors must be two arrays of one shape, (nz, nsel, R) or (nz, nsel, R, S)")
    nz, nsel, R = shape[:3]
    S = shape[3] if len(shape) == 4 else 1
    out_shape = (S, nsel, nz, nz) if len(shape) == 4 else (nsel, nz, nz)
    if isinstance(u_re, _hip.DeviceArray) or isinstance(u_im, _hip.DeviceArray):
        if getattr(u_re, "name", None) != "phasor_re" or getattr(u_im, "name", None) != "phasor_im":
            raise ValueError("device phasors must be the views band_phase(..., resident=True) returned")
        ctx = u_re._owner
        views = ctx.plv_resident(nz, nsel, R, S)
        if resident:
            c_re, c_im, p = (_hip.DeviceArray(v.ptr, out_shape, ctx, v.name) for v in views)
            return p, (c_re, c_im)
        c_re, c_im, p = (ctx.fetch(v.name, out_shape) for v in views)
    else:
        if resident:
            raise ValueError("resident=True needs device phasors")
        c_re, c_im, p = (v.reshape(out_shape) for v in (ctx or _hip.default_context()).plv(
            np.asarray(u_re, dtype=np.float64).reshape(nz, nsel, R, S), np.asarray(u_im, dtype=np.float64).reshape(nz, nsel, R, S)))
    return p, c_re + 1j * c_im


def spectral_operator(n, fs=1.0, nfft=None, window="boxcar", scaling="density", detrend=False, return_onesided=True, rows=None):
    """(f, A): the complex matrix A (nrow, n), complex128, of a periodogram along a time axis of length n, and its frequencies f:
    `np.abs(A @ x)**2 == scipy.signal.periodogram(x, fs, window, nfft, detrend, return_onesided, scaling)[1]`.  Every step but the
    final modulus is linear in the signal for a fixed length, so the operator is their action on the identity along axis 0:
    rfft(window[:, None] * detrend(I), nfft), each row times the square root of its scale -- 1 / (fs sum w^2) for "density",
    1 / (sum w)^2 for "spectrum", doubled for the one-sided rows except DC and (nfft even) Nyquist.  window: a name or tuple for
    `scipy.signal.get_window`, or an array of length n; detrend: False, "constant" or "linear"; nfft < n reads the first nfft samples
    only, as SciPy does (the window then has that length).  rows: frequency indices to keep, in any order (default: all) -- keeping a
    frequency is keeping a row.  What the reference's scripts compute per call on the host (auditory_lfp/fit_gpcsd_baseline.py:189-195,
    neuropixels/fit_gpcsd2d.py:120-128); no counterpart in the package."""
    import scipy.signal
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    if not fs > 0:
        raise ValueError("fs must be positive")
    nseg = n
    if nfft is None:
        nfft = n
    else:
        nfft = int(nfft)
        if nfft < 1:
            raise ValueError("nfft must be at least 1")
        nseg = min(n, nfft)
    if isinstance(window, (str, tuple)):
        w = scipy.signal.get_window(window, nseg)
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.ndim != 1 or w.size != nseg:
            raise ValueError("a window array must have the length of the signal (%d), got %s" % (nseg, w.shape))
    if detrend is False or detrend is None:
        T = np.eye(nseg)
    elif detrend in ("constant", "linear"):
        T = scipy.signal.detrend(np.eye(nseg), axis=0, type=detrend)
    else:
        raise ValueError("detrend must be False, 'constant' or 'linear'")
    if scaling == "density":
        scale = 1.0 / (float(fs) * np.sum(w * w))
    elif scaling == "spectrum":
        scale = 1.0 / np.sum(w) ** 2
    else:
        raise ValueError("scaling must be 'density' or 'spectrum'")
    T = w[:, None] * T
    if return_onesided:
        A = np.fft.rfft(T, nfft, axis=0)
        f = np.fft.rfftfreq(nfft, 1.0 / float(fs))
        s = np.full(A.shape[0], scale)
        s[1:(None if nfft % 2 else -1)] *= 2.0
    else:
        A = np.fft.fft(T, nfft, axis=0)
        f = np.fft.fftfreq(nfft, 1.0 / float(fs))
        s = np.full(A.shape[0], scale)
    A = A * np.sqrt(s)[:, None]
    if nseg < n:
        A = np.concatenate([A, np.zeros((A.shape[0], n - nseg), dtype=A.dtype)], axis=1)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.intp).reshape(-1)
        A, f = A[rows], f[rows]
    return np.array(f, dtype=np.float64), np.ascontiguousarray(A, dtype=np.complex128)


def power_spectrum(x, A, per_trial=False, coefficients=False, resident=False, ctx=None):
    """Power spectrum along the time axis of x (nz, n, M) or (nz, n, R, S) -- a NumPy array, or a `_hip.DeviceArray` such as a resident
    prediction (`m.csd_pred`, `m.csd_pred_list[c]`) or resident posterior draws (R trials, S draws per trial) -- under the operator A
    (nrow, n) of `spectral_operator`, averaged over the trials: dict with "psd" (nz, nrow), or (nz, nrow, S) for a four-dimensional
    input (one trial-averaged spectrum per draw: a posterior band for the spectrum); per_trial=True adds "power", |A x|^2 per trial,
    coefficients=True "re" and "im", the parts of A x that `cross_spectrum` reads, each shaped like x with n -> nrow.  One fp64 MFMA
    product with the modulus in its epilogue and a sum over the trials in a fixed order (no atomics: the same call gives the same
    bits, "psd" the same bits whatever else is asked for); outputs not asked for are not stored.  Residency as in `band_phase`: a
    device input is read where it lies, with resident=True its results are zero-copy views of the library's buffers "spec_psd",
    "spec_power", "spec_re", "spec_im" (valid until the next call that writes them), otherwise host arrays.  No reference counterpart
    in the package (its scripts: scipy.signal.periodogram(..., axis=1), then a mean over the trials)."""
    A = np.asarray(A)
    shape = tuple(int(v) for v in x.shape)
    if len(shape) not in (3, 4):
        raise ValueError("x must be (nz, n, M) or (nz, n, R, S)")
    nz, n, R = shape[:3]
    S = shape[3] if len(shape) == 4 else 1
    want = (("power",) if per_trial else ()) + (("re", "im") if coefficients else ())
    if A.ndim != 2:
        raise ValueError("the operator must be (nrow, %d), got %s" % (n, A.shape))
    out_shape = {k: (nz, A.shape[0]) + shape[2:] for k in want}
    out_shape["psd"] = (nz, A.shape[0]) + shape[3:]
    if isinstance(x, _hip.DeviceArray):
        if x.base is None:
            raise ValueError("power_spectrum: the device array is not a view of a named buffer of the library")
        ctx = x._owner
        res = ctx.power_spectrum_resident(x.base[0], x.base[1], (nz, n, R, S), A, want)
        if resident:
            return {k: _hip.DeviceArray(v.ptr, out_shape[k], ctx, v.name) for k, v in res.items()}
        return {k: ctx.fetch(v.name, out_shape[k]) for k, v in res.items()}
    if resident:
        raise ValueError("resident=True needs a device input")
    res = (ctx or _hip.default_context()).power_spectrum(np.asarray(x, dtype=np.float64).reshape(nz, n, R, S), A, want)
    return {k: v.reshape(out_shape[k]) for k, v in res.items()}


def _coherence(Sx):
    d = np.real(np.diagonal(Sx, axis1=-2, axis2=-1))
    den = d[..., :, None] * d[..., None, :]
    num = Sx.real * Sx.real + Sx.imag * Sx.imag
    return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)


def spectrum_from_sums(sums, ntrials):
    """The host-side combine of a trial-sharded job: every rank forms R_local * psd and R_local * Sx of its block of trials, the sums
    add, and the coherence -- a quotient -- is formed after the sum.  sums: dict with "psd" (the summed R_local * psd) and / or
    "xspec" (the summed R_local * Sx, complex, or the stacked pair (2, ...) of its parts); returns a dict with "psd" and / or "xspec"
    (complex) and "coh", over all `ntrials` trials."""
    out = {}
    if "psd" in sums:
        out["psd"] = np.asarray(sums["psd"], dtype=np.float64) / float(ntrials)
    if "xspec" in sums:
        s = np.asarray(sums["xspec"])
        if not np.iscomplexobj(s):
            s = s[0] + 1j * s[1]
        out["xspec"] = s / float(ntrials)
        out["coh"] = _coherence(out["xspec"])
    return out


def cross_spectrum(coeffs, resident=False, ctx=None):
    """Cross-spectral matrix and magnitude-squared coherence of ALL site pairs over the trials.  Input: the dict `power_spectrum(...,
    coefficients=True)` returns, or a pair (re, im), each array (nz, nrow, R) or (nz, nrow, R, S).  Returns (Sx, coherence):
    Sx[j, a, b] = mean over the trials of X_a conj(X_b) at kept frequency j, complex, in the operator's scaling -- that is
    `scipy.signal.csd(x_b, x_a)` averaged over the trials (SciPy conjugates its FIRST argument), the orientation of `plv`'s
    phase_a - phase_b -- and coherence[j, a, b] = |Sx[j, a, b]|^2 / (Sx[j, a, a] Sx[j, b, b]), 0 where a site's power is 0; shapes
    (nrow, nz, nz), or (S, nrow, nz, nz) for a four-dimensional input.  Two launches for all pairs, frequencies and draws; Sx.real and
    the coherence are symmetric and Sx.imag antisymmetric bit for bit.  Coefficients that are resident views (`power_spectrum(...,
    coefficients=True, resident=True)`) are read where they lie; resident=True then returns zero-copy views ((s_re, s_im), coherence)
    of "xspec_re", "xspec_im", "xspec_coh" instead of host arrays.  ctx as in `band_phase`.  No reference counterpart."""
    re, im = (coeffs["re"], coeffs["im"]) if isinstance(coeffs, dict) else coeffs
    shape = tuple(int(v) for v in re.shape)
    if len(shape) not in (3, 4) or tuple(im.shape) != shape:
        raise ValueError("the coefficients must be two arrays of one shape, (nz, nrow, R) or (nz, nrow, R, S)")
    nz, nrow, R = shape[:3]
    S = shape[3] if len(shape) == 4 else 1
    out_shape = (S, nrow, nz, nz) if len(shape) == 4 else (nrow, nz, nz)
    if isinstance(re, _hip.DeviceArray) or isinstance(im, _hip.DeviceArray):
        if getattr(re, "name", None) != "spec_re" or getattr(im, "name", None) != "spec_im":
            raise ValueError("device coefficients must be the views power_spectrum(..., coefficients=True, resident=True) returned")
        ctx = re._owner
        views = ctx.cross_spectrum_resident(nz, nrow, R, S)
        if resident:
            s_re, s_im, coh = (_hip.DeviceArray(v.ptr, out_shape, ctx, v.name) for v in views)
            return (s_re, s_im), coh
        s_re, s_im, coh = (ctx.fetch(v.name, out_shape) for v in views)
    else:
        if resident:
            raise ValueError("resident=True needs device coefficients")
        s_re, s_im, coh = (v.reshape(out_shape) for v in (ctx or _hip.default_context()).cross_spectrum(
            np.asarray(re, dtype=np.float64).reshape(nz, nrow, R, S), np.asarray(im, dtype=np.float64).reshape(nz, nrow, R, S)))
    return s_re + 1j * s_im, coh


def _torus_graph_weights(N, weights, nboot, seed):
    """The replicate weights handed to the library: None (the unit-weight fit alone), or row 0 = ones followed by the bootstrap
    multiplicities / the caller's rows."""
    if weights is not None and nboot:
        raise ValueError("give weights or nboot, not both")
    if weights is not None:
        extra = np.atleast_2d(np.asarray(weights, dtype=np.float64))
        if extra.ndim != 2 or extra.shape[1] != N:
            raise ValueError("weights must be (B', %d), got %s" % (N, extra.shape))
    elif nboot:
        if nboot < 0:
            raise ValueError("nboot must not be negative")
        extra = np.random.default_rng(seed).multinomial(N, [1.0 / N] * N, size=int(nboot)).astype(np.float64)
    else:
        return None
    return np.concatenate([np.ones((1, N)), extra], axis=0)


def _torus_graph_result(res, d, inference):
    """The public dict from what `_hip.Context.torus_graph*` returns (replicate 0 = the unit-weight fit)."""
    import warnings
    import scipy.special
    status = np.asarray(res["status"])
    if status[0] != 0:
        raise np.linalg.LinAlgError("torus_graph: Gamma is singular (pivot %d of the factorisation failed): fewer trials than the "
                                    "%d parameters need?" % (status[0] - 1, d * (d - 1)))

    def coupling(phi):
        k = np.hypot(phi[..., 0], phi[..., 1])
        return scipy.special.i1e(k) / scipy.special.i0e(k)

    i, j = np.triu_indices(d, 1)
    phi = res["phi"]
    out = {"pairs": np.stack([i, j], axis=1), "phi": phi[0], "cond_coupling": coupling(phi[0]),
           "chi2": res["chi2"] if inference else None, "pvals": np.exp(-0.5 * res["chi2"]) if inference else None}
    if phi.shape[0] > 1:
        bad = np.flatnonzero(status[1:])
        if bad.size:
            warnings.warn("torus_graph: %d of %d replicates have a singular Gamma and stay NaN (first: %d)" % (bad.size, phi.shape[0] - 1, bad[0]))
        out.update(phi_boot=phi[1:], cond_coupling_boot=coupling(phi[1:]), status_boot=status[1:].copy())
    return out


def torus_graph(phases_or_phasors, weights=None, nboot=0, seed=None, inference=True, ctx=None, at=0, sites=None):
    """Phase-difference torus graph of d nodes over N trials by score matching: log p(x) = sum over the pairs p = (i, j), i < j, of
    phi[p, 0] cos(x_i - x_j) + phi[p, 1] sin(x_i - x_j) -- the CONDITIONAL phase coupling of every pair given all other nodes, where
    `plv` is the marginal one.  Input as for `plv`: a host array of phases (d, N), a pair (u_re, u_im) of unit phasors, or the dict
    `band_phase` returns; three-dimensional phasors (nz, nsel, R) are read at kept time `at` and rows `sites` (default: all) -- host
    arrays are sliced here, the resident views of band_phase(..., resident=True) are gathered on the device and never cross PCIe.
    Replicate 0 is always the unit-weight fit; nboot > 0 appends `np.random.default_rng(seed).multinomial(N, [1/N]*N, size=nboot)` as
    bootstrap weights, or explicit `weights` (B', N) may be given instead.  Returns a dict: `pairs` (P, 2) in the order of
    np.triu_indices(d, 1), `phi` (P, 2), `cond_coupling` (P,) = I1(k) / I0(k) with k = |phi[p]| (the partial phase-locking value),
    `chi2` and `pvals` (P,) (the edge test, chi-square with two degrees of freedom; None with inference=False), and with replicates
    `phi_boot` (B', P, 2), `cond_coupling_boot` (B', P), `status_boot` (B',).  One weighted Gram accumulation on fp64 MFMA and one dense
    Cholesky solve of order d (d - 1) per replicate; the same call gives the same bits.  np.linalg.LinAlgError if the unit-weight
    fit is singular; a singular replicate stays NaN (one warning).  No counterpart in the package: the reference's scripts call
    pyTG's torusGraphs(X, selMode=(False, True, False)) in a bootstrap loop (auditory_lfp/torus_graph_fit.py,
    neuropixels/fit_torus_graph.py)."""
    if isinstance(phases_or_phasors, dict):
        u_re, u_im = phases_or_phasors["u_re"], phases_or_phasors["u_im"]
    elif isinstance(phases_or_phasors, (tuple, list)):
        u_re, u_im = phases_or_phasors
    else:
        ph = np.asarray(phases_or_phasors, dtype=np.float64)
        u_re, u_im = np.cos(ph), np.sin(ph)
    shape = tuple(int(v) for v in u_re.shape)
    if len(shape) not in (2, 3) or tuple(u_im.shape) != shape:
        raise ValueError("the phases / phasors must be (d, N), or (nz, nsel, R) read at one kept time")
    N = shape[-1]
    if isinstance(u_re, _hip.DeviceArray) or isinstance(u_im, _hip.DeviceArray):
        if getattr(u_re, "name", None) != "phasor_re" or getattr(u_im, "name", None) != "phasor_im" or len(shape) != 3:
            raise ValueError("device phasors must be the views band_phase(..., resident=True) returned, (nz, nsel, R)")
        sites = np.arange(shape[0]) if sites is None else np.asarray(sites, dtype=np.intp).reshape(-1)
        w = _torus_graph_weights(N, weights, nboot, seed)
        res = u_re._owner.torus_graph_resident(sites, at, shape, weights=w, inference=inference)
        return _torus_graph_result(res, sites.size, inference)
    u_re, u_im = np.asarray(u_re, dtype=np.float64), np.asarray(u_im, dtype=np.float64)
    if len(shape) == 3:
        u_re, u_im = u_re[:, at, :], u_im[:, at, :]
    if sites is not None:
        sel = np.asarray(sites, dtype=np.intp).reshape(-1)
        u_re, u_im = u_re[sel], u_im[sel]
    w = _torus_graph_weights(N, weights, nboot, seed)
    res = (ctx or _hip.default_context()).torus_graph(u_re, u_im, weights=w, inference=inference)
    return _torus_graph_result(res, u_re.shape[0], inference)


def trial_shift_objective(evec_s, evec_t, Dvec, lfp_trials, mu_lfp, t, mutau=0.0, sigtau=10.0, ctx=None):
    """The trial-shift objective of auditory_lfp/fit_mean_function.py:306-321 and its analytic gradient, resident on the device.
    Arguments as `fit_trial_shifts`.  Everything is uploaded once (`Context.shift_plan`); returns a callable
    `obj(trials, taus, grad=True) -> (f (B,), g (B, nseg) or None)` for B points (trial index, tau (nseg,)) per call, any trial any
    number of times -- only the points and the results cross PCIe.

        mean(tau)[x, k] = mu[x, k, 0] + sum_i interp1d(t, mu[:, :, i], fill_value="extrapolate")(t_k + tau_i)
        f = 1/2 sum((evec_s.T @ r @ evec_t)**2 / Dvec) + 1/2 sum(((tau - mutau) / sigtau)**2),   r = lfp_trials[:, :, trial] - mean(tau)

    Between the knots of the interpolation f is exactly quadratic in tau; g is its derivative on the segments the interpolation itself
    uses, i.e. the LEFT derivative at a tau that puts samples on knots (tau = 0 is such a point: SciPy's segment search puts a sample
    on a knot into the segment to its left).  A context holds one plan: the callable refuses to run once another plan has replaced
    its own.  ctx: the `_hip.Context` to plan on (default: the process-wide one)."""
    ctx = ctx or _hip.default_context()
    gen = ctx.shift_plan(evec_s, evec_t, Dvec, lfp_trials, mu_lfp, t)
    mutau, sigtau = float(mutau), float(sigtau)

    def obj(trials, taus, grad=True):
        if ctx.shift_generation != gen:
            raise RuntimeError("trial_shift_objective: a later plan on the same context has replaced this one")
        return ctx.shift_eval(trials, taus, grad=grad, mutau=mutau, sigtau=sigtau)
    return obj


def fit_trial_shifts(evec_s, evec_t, Dvec, lfp_trials, mu_lfp, t, tau0=None, mutau=0.0, sigtau=10.0, width=None,
                     options=None, jac=False, return_evals=False):
    """Per-trial time shifts of the evoked components: the optimisation loop of auditory_lfp/fit_mean_function.py:299-335
    (one L-BFGS-B per trial over `tau`, objective = 0.5 * whitened quadratic form of `lfp_trial - mean(tau)` + Gaussian
    prior on the shifts), with every trial's optimiser running in lock-step so that ONE batched GPU call
    (`whitened_quadratic_forms`) evaluates the objectives all chains are waiting for -- the reference spreads the trials
    over CPU processes with joblib instead.

    evec_s, evec_t, Dvec: outputs of `comp_eig_D`;  lfp_trials (nx, nt, ntrials);  mu_lfp (nx, nt, nseg + 1): background in
    [..., 0], component means in [..., 1:];  t (nt,) or (nt, 1);  width: chains alive at a time (default min(ntrials, 128),
    memory-capped).  Returns (tau_hat (ntrials, nseg), success, messages).

    jac=True: the chains are `scipy.optimize.minimize(..., jac=True, method="l-bfgs-b")` on `trial_shift_objective` -- the shifted
    means, the residuals, the objective and its analytic gradient all stay on the device, one call per lock-step batch, and an
    iteration costs one evaluation instead of the nseg + 1 of SciPy's finite differences.  return_evals=True appends
    {"batches", "points"}: the batched evaluations issued and the points they covered."""
    import numpy as np
    import scipy.interpolate
    import scipy.optimize
    from .lockstep import run_chains
    lfp_trials = np.atleast_3d(np.asarray(lfp_trials, dtype=np.float64))
    nx, nt, ntrials = lfp_trials.shape
    nseg = mu_lfp.shape[2] - 1
    tt = np.asarray(t, dtype=np.float64).reshape(-1)
    tau0 = np.zeros(nseg) if tau0 is None else np.asarray(tau0, dtype=np.float64)
    if jac:
        obj = trial_shift_objective(evec_s, evec_t, Dvec, lfp_trials, mu_lfp, tt, mutau=mutau, sigtau=sigtau)

        def batch_fn(items):                 # items: [(trial, tau)] -> {trial: (objective, gradient)}
            f, g = obj([ti for ti, _ in items], np.array([tau for _, tau in items], dtype=np.float64).reshape(len(items), nseg))
            return {ti: (float(f[j]), g[j].copy()) for j, (ti, _) in enumerate(items)}
    else:
        mu_f = [scipy.interpolate.interp1d(tt, mu_lfp[:, :, i], axis=1, fill_value="extrapolate") for i in range(1, nseg + 1)]

        def batch_fn(items):                 # items: [(trial, tau)] -> {trial: objective}
            resid = np.empty((nx, nt, len(items)))
            for j, (ti, tau) in enumerate(items):
                mu = np.array(mu_lfp[:, :, 0], dtype=np.float64, copy=True)
                for i in range(nseg):
                    mu += mu_f[i](tt + tau[i])
                resid[:, :, j] = lfp_trials[:, :, ti] - mu
            quad = whitened_quadratic_forms(evec_s, evec_t, Dvec, resid)
            return {ti: float(0.5 * quad[j] + 0.5 * np.sum(np.square((np.asarray(tau) - mutau) / sigtau)))
                    for j, (ti, tau) in enumerate(items)}

    def chain(ti, evaluate):
        # keyed by the trial: the evaluator hands every chain the value of ITS point of the batch (with jac: value and gradient)
        return scipy.optimize.minimize(lambda tau: evaluate(np.array(tau, copy=True)), tau0, jac=True if jac else None,
                                       method="l-bfgs-b", options=options or {})
    if width is None:
        # one OS thread and one (nx, nt) residual per live chain: at most 128 chains, within a 1 GiB budget for the batch's
        # residuals (with jac no residual leaves the device, the same width keeps the two paths' batches alike); the remaining
        # trials wait in run_chains' queue and take the slot of a chain that converges
        width = int(max(1, min(ntrials, 128, (1 << 30) // max(8 * nx * nt, 1))))
    out, _ev = run_chains(list(range(ntrials)), chain, lambda items: batch_fn([(k, x) for k, x in items]), width)
    for r in out.values():
        if isinstance(r, Exception):
            raise r
    tau_hat = np.array([out[i].x for i in range(ntrials)])
    res = (tau_hat, np.array([bool(out[i].success) for i in range(ntrials)]), [out[i].message for i in range(ntrials)])
    return res + ({"batches": _ev.batches, "points": _ev.points},) if return_evals else res


def roi_weights(z, tstar, site_sets, time_windows, contrast=None):
    """Dense weights W (J, nz, ntstar) for `predict_functionals`: region-of-interest AVERAGES of a field over (z, tstar), and
    differences of two of them.  Plain NumPy, no device call.

    Box b is the sites `site_sets[b]` -- indices into the rows of z, or a boolean mask of length nz -- times the times of tstar inside
    the closed window `time_windows[b] = (t_lo, t_hi)`; its weight is 1 / (sites x times in the box) on the box and 0 elsewhere, so
    <W_b, f> is the mean of f over the box.  `site_sets` and `time_windows` have one entry per box.  contrast=None returns the boxes
    themselves (J = number of boxes); contrast = [(a, b), ...] returns W[a] - W[b] per pair instead (a sink-minus-source contrast).
    ValueError on an empty box, an index outside z or the boxes, or lists of different lengths."""
    nz = np.asarray(z).shape[0]
    ts = np.asarray(tstar, dtype=np.float64).reshape(-1)
    if len(site_sets) != len(time_windows) or len(site_sets) < 1:
        raise ValueError("roi_weights: site_sets and time_windows need one entry per box, at least one box")
    W = np.zeros((len(site_sets), nz, ts.size))
    for b, (sites, (lo, hi)) in enumerate(zip(site_sets, time_windows)):
        sites = np.asarray(sites)
        if sites.dtype == bool:
            if sites.shape != (nz,):
                raise ValueError("roi_weights: the mask of box %d has shape %s, not (%d,)" % (b, sites.shape, nz))
            sites = np.flatnonzero(sites)
        sites = np.unique(sites.astype(np.int64).reshape(-1))
        if sites.size and (sites[0] < 0 or sites[-1] >= nz):
            raise ValueError("roi_weights: box %d names a site outside [0, %d)" % (b, nz))
        times = np.flatnonzero((ts >= lo) & (ts <= hi))
        if sites.size == 0 or times.size == 0:
            raise ValueError("roi_weights: box %d is empty (%d sites, %d times)" % (b, sites.size, times.size))
        W[np.ix_([b], sites, times)] = 1.0 / (sites.size * times.size)
    if contrast is None:
        return W
    pairs = np.asarray(contrast, dtype=np.int64).reshape(-1, 2)
    if pairs.size == 0 or pairs.min() < 0 or pairs.max() >= W.shape[0]:
        raise ValueError("roi_weights: contrast needs pairs (a, b) of box indices below %d" % W.shape[0])
    return np.ascontiguousarray(W[pairs[:, 0]] - W[pairs[:, 1]])
