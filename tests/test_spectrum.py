"""Power spectrum, cross-spectrum and coherence on the device (gpcsd_power_spectrum, gpcsd_cross_spectrum; no reference counterpart in
the package).

The yardstick is tests/spectrum_ref.py: SciPy itself, called as the reference's analysis scripts call it (periodogram(..., axis=1) and a
mean over the trials, csd, coherence on the concatenated trials), and a longdouble einsum where a kernel is tested alone.  Bounds,
u = 2^-53, K = the length of the time axis, R = the number of trials:

  Re, Im of the coefficients: the GEMM core's rounding bound E = (K + 8) u sum_t |A||x| (E_re, E_im with A's real / imaginary part).
  power = fl(Re^2 + Im^2) of the COMPUTED parts: |d power| <= 2 |Re| E_re + 2 |Im| E_im + E_re^2 + E_im^2 (the parts' errors through
      the squares) + 3 u power (two products and a sum, each rounded once; 2 u with a fused multiply-add).
  psd = 1/R sum_r power: the mean of the per-trial bounds, plus the summation itself -- R non-negative terms added in at most two
      stages (within a column tile, then over a site's tiles; for the shapes here, S <= 64, at most R + 2 tiles), every partial sum
      at most the total: (2 R + 4) u psd for the additions and the division by R.
  All four outputs: 1e-6 of the largest entry (the project's gate).
  Sx from GIVEN coefficients: (2 R + 8) u max|X|^2 (2 R products of magnitude <= max|X|^2 per part, divided by R), as the PLV's.
  coherence, entrywise where the reference's S_aa S_bb >= (1e-3 max S_aa)^2: with e the bound on Sx and den = S_aa S_bb,
      |d |S_ab|^2| <= 2 sqrt(2) |S_ab| e + 2 e^2 and |d den| <= (S_aa + S_bb) e + e^2, |S_ab| <= sqrt(den), coh <= 1:
      tol = (2 sqrt(2) sqrt(den) + S_aa + S_bb + 3 e) e / den + 8 u (squares, product and quotient);  diag(coh) == 1 within 4 u.
  Through a model the comparison is with SciPy in double precision on the same field: the gate, 1e-6 of the largest entry.

The GPU tests print the maxima they observe."""
import ctypes
import os
import re

import numpy as np
import pytest

import spectrum_ref as SR

GATE = 1e-6                       # the project's contract (tests/test_hip_parity.py)
U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gpcsd_power_spectrum", "gpcsd_power_spectrum_resident", "gpcsd_cross_spectrum", "gpcsd_cross_spectrum_resident")


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("n,nfft,window,scaling,detrend", SR.OPERATOR_CASES + [(40, 64, ("tukey", 0.25), "spectrum", "linear"),
                                                                             (37, 20, "hann", "density", False)])
@pytest.mark.parametrize("onesided", [True, False])
def test_operator_equals_the_direct_scipy_call(n, nfft, window, scaling, detrend, onesided):
    """|A x|^2 against scipy.signal.periodogram, and the frequency vector.  Observed: at most 1.1e-15 of the largest entry."""
    from gpcsd_amd import utility_functions as UF
    fs = 2500.0
    f, A = UF.spectral_operator(n, fs, nfft, window, scaling, detrend, onesided)
    x = SR.signal(11, 3, n, 4)[..., 0]
    f_ref, ref = SR.periodogram(x, fs=fs, window=window, nfft=nfft, detrend=detrend, scaling=scaling, return_onesided=onesided)
    assert A.dtype == np.complex128 and A.shape == (f_ref.size, n) and f.shape == f_ref.shape
    assert np.allclose(f, f_ref, rtol=4 * U, atol=0)
    got = np.abs(np.einsum("jt,ztm->zjm", A, x)) ** 2
    err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print("operator %s: %.2e of the largest entry" % ((n, nfft, window, scaling, detrend, onesided), err))
    assert err <= 1e-12


def test_operator_window_array_rows_and_bad_arguments():
    import scipy.signal as ss
    from gpcsd_amd import utility_functions as UF
    n = 37
    w = ss.get_window(("kaiser", 5.0), n)
    f, A = UF.spectral_operator(n, 1000.0, 51, w, "density", "constant")
    x = SR.signal(12, 2, n, 3)[..., 0]
    f_ref, ref = SR.periodogram(x, fs=1000.0, window=w, nfft=51, detrend="constant")
    assert np.max(np.abs(np.abs(np.einsum("jt,ztm->zjm", A, x)) ** 2 - ref)) <= 1e-12 * np.max(ref)
    # rows: any order, repeats allowed; keeping a frequency is keeping a row
    rows = [20, 2, 11, 2, 0]
    f2, A2 = UF.spectral_operator(n, 1000.0, 51, w, "density", "constant", rows=rows)
    assert A2.shape == (5, n) and np.array_equal(A2, A[rows]) and np.array_equal(f2, f[rows])
    assert np.allclose(f2, f_ref[rows], rtol=4 * U, atol=0)
    for bad in (dict(n=0), dict(n=8, fs=0.0), dict(n=8, nfft=0), dict(n=8, window=np.ones(7)), dict(n=8, window=np.ones((8, 1))),
                dict(n=8, detrend="quadratic"), dict(n=8, detrend=lambda v: v), dict(n=8, scaling="power"), dict(n=8, window="no_such_window")):
        with pytest.raises(ValueError):
            UF.spectral_operator(**bad)
    with pytest.raises(IndexError):
        UF.spectral_operator(8, rows=[5])                                        # 8 samples have five one-sided frequencies, 0 .. 4


def test_reference_orientation_is_scipy_csd_and_coherence():
    """The yardsticks agree among themselves: the longdouble einsum of the header's definition is scipy.signal.csd(x_b, x_a) averaged over
    the trials, and its coherence is scipy.signal.coherence on the concatenated trials.  Also runs the CPU-side assertion of the
    coherence signal (fewer than 1 % of the entries under the floor)."""
    from gpcsd_amd import utility_functions as UF
    for S in (1, 2):
        x, A, cre, cim, s_re, s_im, coh, ok = SR.coherence_case(S)
        assert ok.shape == (S, 3, 70, 70) and np.count_nonzero(~ok) < 0.01 * ok.size
    x = np.array(SR.coherence_case(1)[0][:9, :, :, 0])
    rows = [7, 8, 9]
    f, A = UF.spectral_operator(40, fs=1.0, nfft=64, window="hann", rows=rows)
    cre, cim = SR.coefficients(A, x[..., None])[:2]
    s_re, s_im = SR.cross_spectrum(cre, cim)
    ref = SR.scipy_csd_mean(x, rows, fs=1.0, window="hann", nfft=64, detrend=False)
    assert np.max(np.abs((s_re[0] + 1j * s_im[0]).astype(np.complex128) - ref)) <= 1e-12 * np.max(np.abs(ref))
    assert np.max(np.abs(s_im)) > 1e-3 * np.max(np.abs(ref))                    # (the orientation is visible in the data)
    f_ref, coh_ref = SR.scipy_coherence(x, rows, fs=1.0, window="hann", nfft=64, detrend=False)
    assert np.allclose(f, f_ref, rtol=4 * U, atol=0)
    assert np.max(np.abs(SR.coherence(s_re, s_im)[0][0].astype(np.float64) - coh_ref)) <= 1e-12


def test_host_combine_of_rank_sums_equals_the_unsharded_spectrum():
    from gpcsd_amd import utility_functions as UF
    x = SR.signal(13, 6, 37, 5)
    _, A = UF.spectral_operator(37, nfft=51, window="hann", rows=[3, 9])
    f64 = lambda v: np.asarray(v, dtype=np.float64)

    def block(sl):
        cre, cim = (f64(v) for v in SR.coefficients(A, x[:, :, sl], dtype=np.float64)[:2])
        s_re, s_im = SR.cross_spectrum(cre, cim, dtype=np.float64)
        return (cre * cre + cim * cim).mean(axis=2)[..., 0], s_re[0] + 1j * s_im[0]

    psd, Sx = block(slice(0, 5))
    sums = {"psd": 0.0, "xspec": 0.0}
    for sl in (slice(0, 3), slice(3, 5)):
        p, s = block(sl)
        sums = {"psd": sums["psd"] + (sl.stop - sl.start) * p, "xspec": sums["xspec"] + (sl.stop - sl.start) * s}
    out = UF.spectrum_from_sums(sums, 5)
    assert np.max(np.abs(out["psd"] - psd)) <= 8 * U * np.max(psd) and np.max(np.abs(out["xspec"] - Sx)) <= 8 * U * np.max(np.abs(Sx))
    coh = f64(SR.coherence(Sx.real, Sx.imag)[0])
    assert np.max(np.abs(out["coh"] - coh)) <= 64 * U and np.all(np.abs(np.diagonal(out["coh"], axis1=1, axis2=2) - 1.0) <= 4 * U)
    pair = UF.spectrum_from_sums({"xspec": np.stack([sums["xspec"].real, sums["xspec"].imag])}, 5)      # the stacked form of the same sums
    assert sorted(pair) == ["coh", "xspec"] and np.array_equal(pair["xspec"], out["xspec"]) and np.array_equal(pair["coh"], out["coh"])
    zero = np.array(sums["xspec"])
    zero[:, 2, :] = zero[:, :, 2] = 0.0                                          # a site without power: coherence 0, not NaN
    c0 = UF.spectrum_from_sums({"xspec": zero}, 5)["coh"]
    assert np.all(c0[:, 2, :] == 0.0) and np.all(c0[:, :, 2] == 0.0) and np.all(np.isfinite(c0))


def test_surface_exists_and_fails_loudly_without_a_gpu():
    import torch
    from gpcsd_amd import build, _hip, utility_functions as UF
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    for cls in (GPCSD1D, GPCSD2D):
        assert callable(getattr(cls, "spectrum", None)) and callable(getattr(cls, "coherence", None))
    for fn in ("spectral_operator", "power_spectrum", "cross_spectrum", "spectrum_from_sums"):
        assert callable(getattr(UF, fn, None))
    assert "spectrum.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _hip.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read(), flags=re.S)
    for fn in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % fn, src), "%s is not declared" % fn
        assert fn in _hip.SIGNATURES
        assert hasattr(lib, fn), "libgpcsd_hip.so does not export %s" % fn
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipUnavailable):
            UF.power_spectrum(np.zeros((1, 4, 1)), np.eye(4))
        with pytest.raises(_hip.HipUnavailable):
            UF.cross_spectrum((np.zeros((2, 1, 3)), np.zeros((2, 1, 3))))


def test_header_notes_name_the_scripts():
    """Every new prototype carries its usage note: the script lines it replaces and that the package has no counterpart."""
    src = open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read()
    for fn in SYMBOLS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\s*\(" % fn, src, flags=re.S)
        assert m, fn
        note = " ".join(m.group(1).replace("*", " ").split())
        assert "NO REFERENCE COUNTERPART in the package" in note and "fit_gpcsd_baseline.py:189-195" in note and "fit_gpcsd2d.py:120-128" in note, fn


# ------------------------------------------------------------------------------------------------ GPU: the kernels alone
_CTX = []


def _ctx():
    if not _CTX:
        from gpcsd_amd import _hip
        _CTX.append(_hip.Context())
    return _CTX[0]


def _check_power(res, x, A, worst, label):
    """All four outputs of the power kernel for the field x (nz, n, R, S) under A against the longdouble reference and the bounds of
    the module docstring; the observed maxima (as fractions of the bounds, and of the largest entry) go to `worst`."""
    nz, K, R, S = x.shape
    re, im, mag_re, mag_im = SR.coefficients(A, x)
    E_re, E_im = (K + 8) * U * mag_re, (K + 8) * U * mag_im
    power = re * re + im * im
    psd = power.mean(axis=2)
    B_power = 2 * np.abs(re) * E_re + 2 * np.abs(im) * E_im + E_re ** 2 + E_im ** 2 + 3 * U * power
    B_psd = B_power.mean(axis=2) + (2 * R + 4) * U * psd
    assert res["psd"].shape == (nz, A.shape[0], S) and all(res[k].shape == (nz, A.shape[0], R, S) for k in ("power", "re", "im")), label
    f64 = lambda v: float(np.max(v))
    tiny = np.finfo(np.float64).tiny
    obs = {"re_im_bound": max(f64(np.abs(res["re"] - re) / (E_re + tiny)), f64(np.abs(res["im"] - im) / (E_im + tiny))),
           "power_bound": f64(np.abs(res["power"] - power) / (B_power + tiny)),
           "psd_bound": f64(np.abs(res["psd"] - psd) / (B_psd + tiny)),
           "re_im_gate": max(f64(np.abs(res["re"] - re)), f64(np.abs(res["im"] - im))) / f64(np.maximum(np.abs(re), np.abs(im))),
           "power_gate": f64(np.abs(res["power"] - power)) / f64(power), "psd_gate": f64(np.abs(res["psd"] - psd)) / f64(psd)}
    for k, v in obs.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert all(obs[k] <= 1.0 for k in ("re_im_bound", "power_bound", "psd_bound")), (label, obs)
    assert all(obs[k] <= GATE for k in ("re_im_gate", "power_gate", "psd_gate")), (label, obs)


POWER_SHAPES = [((3, 37, 5, 1), 51, 26),      # one partial row tile, K no multiple of 16, site boundaries inside a column tile
                ((2, 40, 70, 1), 128, 65),    # three row tiles, more than one column tile per site
                ((3, 37, 5, 3), 51, 26),      # the draw layout: trials S apart
                ((1, 16, 1, 1), None, 9)]     # one column, one full K tile, R = 1
# draws across column-tile borders: a tile that holds ONE column of a site (column 63 = site 3, draw 0 of 4 x 21 columns), so two of
# its three draws have no partial sum there; and sites of 69 columns, each draw in two or three tiles
DRAW_SHAPES = [((4, 16, 7, 3), None, 9), ((2, 16, 23, 3), None, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nfft,nrow", POWER_SHAPES + DRAW_SHAPES)
def test_power_kernel_against_extended_precision(shape, nfft, nrow):
    """Observed on an MI355X: see DESIGN.md 4.9 (the printed maxima)."""
    from gemm_ref import same_bits
    from gpcsd_amd import utility_functions as UF
    ctx = _ctx()
    nz, n, R, S = shape
    f, A = UF.spectral_operator(n, fs=1000.0, nfft=nfft, window="hann" if n > 16 else "boxcar")
    assert A.shape == (nrow, n)
    x = SR.signal(500 + n + R + S, nz, n, R, S)
    worst = {}
    full = ctx.power_spectrum(x, A, want=("power", "re", "im"))
    _check_power(full, x, A, worst, shape)
    # SciPy itself on the same field
    ref = SR.psd(x, fs=1000.0, window="hann" if n > 16 else "boxcar", nfft=nfft)[1]
    worst["psd_scipy"] = float(np.max(np.abs(full["psd"] - ref)) / np.max(ref))
    assert worst["psd_scipy"] <= GATE
    # psd has the same bits without the optional outputs, with each of them alone, and in a second call
    only = ctx.power_spectrum(x, A)
    assert sorted(only) == ["psd"] and same_bits(only["psd"], full["psd"])
    for k in ("power", "re", "im"):
        one = ctx.power_spectrum(x, A, want=(k,))
        assert sorted(one) == sorted(("psd", k)) and same_bits(one["psd"], full["psd"]) and same_bits(one[k], full[k]), k
    again = ctx.power_spectrum(x, A, want=("power", "re", "im"))
    assert all(same_bits(again[k], full[k]) for k in full)
    # the public function: three- and four-dimensional inputs
    pub = UF.power_spectrum(x if S > 1 else x[..., 0], A, per_trial=True, coefficients=True, ctx=ctx)
    assert pub["psd"].shape == ((nz, nrow, S) if S > 1 else (nz, nrow)) and pub["power"].shape == ((nz, nrow, R, S) if S > 1 else (nz, nrow, R))
    assert all(same_bits(pub[k].reshape(full[k].shape), full[k]) for k in full)
    # a NULL output is not touched
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None
    Are, Aim = np.ascontiguousarray(A.real), np.ascontiguousarray(A.imag)
    psd = np.full((nz, nrow, S), -777.0)
    assert ctx._lib.gpcsd_power_spectrum(ctx._h, dp(np.ascontiguousarray(x)), nz, n, R, S, dp(Are), dp(Aim), nrow, dp(psd), None, None, None) == 0
    assert same_bits(psd, full["psd"])
    print("power %s: " % (shape,) + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))


@pytest.mark.gpu
def test_resident_path_equals_the_host_path_bit_for_bit():
    from gemm_ref import same_bits
    from gpcsd_amd import _hip, utility_functions as UF
    ctx = _hip.Context()
    lib = ctx._lib
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for shape, nfft, nrow in POWER_SHAPES[:3]:
        nz, n, R, S = shape
        _, A = UF.spectral_operator(n, fs=1000.0, nfft=nfft, window="hann")
        x = SR.signal(600 + R + S, nz, n, R, S)
        host = ctx.power_spectrum(x, A, want=("power", "re", "im"))
        # the field as a named device buffer: the host call's own upload, "op_in0", is one
        src = ctx.device_array("op_in0", shape)
        res = UF.power_spectrum(src, A, per_trial=True, coefficients=True, resident=True)
        assert sorted(res) == ["im", "power", "psd", "re"] and all(hasattr(v, "__cuda_array_interface__") for v in res.values())
        assert [res[k].name for k in ("psd", "power", "re", "im")] == ["spec_psd", "spec_power", "spec_re", "spec_im"]
        assert tuple(res["psd"].shape) == (nz, nrow, S) and tuple(res["re"].shape) == (nz, nrow, R, S)
        assert all(same_bits(res[k].numpy(), host[k]) for k in host), shape
        fetched = UF.power_spectrum(src, A)                                     # resident source, host result
        assert sorted(fetched) == ["psd"] and isinstance(fetched["psd"], np.ndarray) and same_bits(fetched["psd"], host["psd"])
        # that last call stored no coefficients: the cross-spectrum has nothing to read
        assert lib.gpcsd_cross_spectrum_resident(ctx._h, nz, nrow, R, S) == -4
        coeffs = UF.power_spectrum(src, A, coefficients=True, resident=True)
        assert lib.gpcsd_cross_spectrum_resident(ctx._h, nz, nrow, R, S) == 0 and lib.gpcsd_cross_spectrum_resident(ctx._h, nz, nrow, S, R) == (-4 if R != S else 0)
        Sx, coh = UF.cross_spectrum(coeffs)
        Sx_h, coh_h = UF.cross_spectrum((host["re"], host["im"]), ctx=ctx)
        assert Sx.shape == (S, nrow, nz, nz) and same_bits(Sx.real, Sx_h.real) and same_bits(Sx.imag, Sx_h.imag) and same_bits(coh, coh_h)
        (v_re, v_im), v_coh = UF.cross_spectrum(coeffs, resident=True)
        assert [v.name for v in (v_re, v_im, v_coh)] == ["xspec_re", "xspec_im", "xspec_coh"] and same_bits(v_coh.numpy(), coh)
    # a source that is one of the outputs, an unknown one, a short one, a bad mask
    one = np.ones(1)
    res = lambda name, off, nz, nts, R, S, nrow, mask=0: lib.gpcsd_power_spectrum_resident(ctx._h, name, off, nz, nts, R, S, dp(one), dp(one), nrow, mask)
    for name in (b"spec_psd", b"spec_power", b"spec_re", b"spec_im"):
        assert res(name, 0, 1, 1, 1, 1, 1) == -3 and b"outputs" in lib.gpcsd_last_error(ctx._h)
    assert res(b"no_such_buffer", 0, 1, 1, 1, 1, 1) == -2 and res(None, 0, 1, 1, 1, 1, 1) == -3
    assert res(b"op_in0", 0, 1, 1, 1, 1, 1, mask=8) == -3 and res(b"op_in0", 0, 1, 1 << 21, 1, 1, 1) == -3 and res(b"op_in0", -1, 1, 1, 1, 1, 1) == -3
    assert res(b"op_in0", 0, 0, 1, 1, 1, 1) == -3 and res(b"op_in0", 0, 1, 1, 1 << 12, 1 << 11, 1) == _hip.ERR_CAPACITY
    assert res(b"op_in0", 0, 1, 1, 1, 1, 1) == 0                                 # x[0] under A = 1 + i: psd = 2 x[0]^2
    x0 = ctx.fetch("op_in0", (1,))[0]
    assert abs(ctx.fetch("spec_psd", (1,))[0] - 2 * x0 * x0) <= 4 * U * 2 * x0 * x0
    # host entry points: NULL and empty arguments, capacity before anything is read
    ps = lambda nz, nts, R, S, nrow, x=one, psd=one: lib.gpcsd_power_spectrum(ctx._h, dp(x) if x is not None else None, nz, nts, R, S, dp(one), dp(one), nrow,
                                                                               dp(psd) if psd is not None else None, None, None, None)
    assert ps(0, 1, 1, 1, 1) == -3 and ps(1, 0, 1, 1, 1) == -3 and ps(1, 1, 0, 1, 1) == -3 and ps(1, 1, 1, 0, 1) == -3 and ps(1, 1, 1, 1, 0) == -3
    assert ps(1, 1, 1, 1, 1, x=None) == -3 and ps(1, 1, 1, 1, 1, psd=None) == -3
    assert ps(1, 1, 1 << 12, 1 << 11, 1) == _hip.ERR_CAPACITY and ps(1, 1 << 22, 1, 1, 1) == _hip.ERR_CAPACITY and ps(1 << 20, 1, 1 << 11, 1, 1) == _hip.ERR_CAPACITY
    cs = lambda nz, nrow, R, S, a=one: lib.gpcsd_cross_spectrum(ctx._h, dp(a) if a is not None else None, dp(one), nz, nrow, R, S, dp(one), None, None)
    assert cs(0, 1, 1, 1) == -3 and cs(1, 0, 1, 1) == -3 and cs(1, 1, 0, 1) == -3 and cs(1, 1, 1, 0) == -3 and cs(1, 1, 1, 1, a=None) == -3
    assert cs(1, 1, 1 << 12, 1 << 11) == _hip.ERR_CAPACITY and cs(1 << 21, 1, 1, 1) == _hip.ERR_CAPACITY


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2])
def test_cross_spectrum_and_coherence_against_extended_precision(S):
    """nz = 70: a diagonal 64-wide tile, an off-diagonal one and its mirror image; three rows, five trials.  Observed on an MI355X: see
    DESIGN.md 4.9 (the printed maxima)."""
    from gemm_ref import same_bits
    ctx = _ctx()
    x, A, cre, cim, r_re, r_im, r_coh, ok = SR.coherence_case(S)
    nz, nrow, R = cre.shape[:3]
    s_re, s_im, coh = ctx.cross_spectrum(cre, cim)
    assert s_re.shape == s_im.shape == coh.shape == (S, nrow, nz, nz)
    e = (2 * R + 8) * U * float(np.max(cre * cre + cim * cim))
    e_s = float(max(np.max(np.abs(s_re - r_re)), np.max(np.abs(s_im - r_im)))) / e
    d = np.diagonal(r_re, axis1=2, axis2=3)
    den = d[..., :, None] * d[..., None, :]
    tol = (2 * np.sqrt(2.0) * np.sqrt(den) + d[..., :, None] + d[..., None, :] + 3 * e) * e / den + 8 * U
    e_c = float(np.max((np.abs(coh - r_coh) / tol)[ok]))
    e_d = float(np.max(np.abs(np.diagonal(coh, axis1=2, axis2=3) - 1.0))) / U
    print("cross-spectrum S=%d: Sx %.3f of (2 R + 8) u max|X|^2, coherence %.3f of its bound (largest error %.3g), |diag - 1| %.1f u, "
          "%d of %d entries under the floor" % (S, e_s, e_c, float(np.max(np.abs(coh - r_coh)[ok])), e_d, np.count_nonzero(~ok), ok.size))
    assert e_s <= 1.0 and e_c <= 1.0 and e_d <= 4.0
    assert np.count_nonzero(~ok) <= 0.01 * ok.size
    # Hermitian bit for bit
    T = lambda v: v.transpose(0, 1, 3, 2)
    assert same_bits(s_re, T(s_re)) and same_bits(coh, T(coh)) and np.array_equal(s_im, -T(s_im))
    assert np.all(np.diagonal(s_im, axis1=2, axis2=3) == 0.0)
    again = ctx.cross_spectrum(cre, cim)
    assert all(same_bits(a, b) for a, b in zip(again, (s_re, s_im, coh)))
    a_re, a_im, none = ctx.cross_spectrum(cre, cim, want_coh=False)
    assert none is None and same_bits(a_re, s_re) and same_bits(a_im, s_im)
    # one all-zero site: coherence 0 in its row and column, no NaN, every other entry as before
    zre, zim = np.array(cre), np.array(cim)
    zre[66] = zim[66] = 0.0
    z_re, z_im, z_coh = ctx.cross_spectrum(zre, zim)
    assert np.all(np.isfinite(z_coh)) and np.all(z_coh[:, :, 66, :] == 0.0) and np.all(z_coh[:, :, :, 66] == 0.0)
    assert np.all(z_re[:, :, 66, :] == 0.0) and np.all(z_im[:, :, :, 66] == 0.0)
    keep = np.ones(nz, dtype=bool)
    keep[66] = False
    assert same_bits(z_coh[:, :, keep][:, :, :, keep], coh[:, :, keep][:, :, :, keep])


# ------------------------------------------------------------------------------------------------ GPU: through a model
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1d_wide_24x60x3", "2d_grid_48x40x2"])
def test_model_spectrum_and_coherence_of_the_posterior_mean(name):
    from gemm_ref import same_bits
    from test_loo import _model, _case
    c = _case(name)[0]
    m = _model(name)
    ctx = m._context()
    nz, n, R = _case(name)[3].shape
    fs = 1000.0
    kw = dict(fs=fs, window="hann", nfft=64)
    rows = [2, 5]
    worst = {}

    def rel(got, ref):
        return float(np.max(np.abs(np.asarray(got) - ref)) / np.max(np.abs(ref)))

    results = {}
    for resident in (False, True):
        m.predict(c["x"], c["t"], type="both", resident=resident)
        m.predict_var(c["x"], c["t"], type="csd")
        A_phase = np.eye(n)[[3, 7]] + 1j * np.eye(n)[[4, 8]]
        m.phase(A_phase, type="csd")
        held = {k: getattr(m, k) for k in ("csd_pred", "lfp_pred", "csd_pred_list", "lfp_pred_list", "t_pred", "csd_phase", "csd_amp", "csd_var")}
        host = lambda v: np.array(v.numpy() if hasattr(v, "numpy") else v)
        before = {k: host(held[k]) for k in ("csd_pred", "lfp_pred", "csd_phase", "csd_amp", "csd_var")}
        ncomp = len(m.temporal_cov_list)
        comp_list = lambda: (list(np.array(ctx.fetch("pred_out_csd_list", (ncomp, nz, n, R)))) if resident else
                             [np.array(held["csd_pred_list"][i]) for i in range(ncomp)])
        before_list = comp_list()
        got = {}
        m.spectrum(fs, nfft=64, window="hann", per_trial=True, resident=resident)
        f_ref, ref = SR.psd(before["csd_pred"], **kw)
        assert np.allclose(m.f_spec, f_ref, rtol=4 * U, atol=0)
        assert hasattr(m.csd_psd, "__cuda_array_interface__") == resident and tuple(m.csd_psd.shape) == (nz, 33) and tuple(m.csd_power.shape) == (nz, 33, R)
        got["total"], got["power"] = host(m.csd_psd), host(m.csd_power)
        worst["psd"] = max(worst.get("psd", 0.0), rel(got["total"], ref))
        worst["power"] = max(worst.get("power", 0.0), rel(got["power"], SR.periodogram(before["csd_pred"], **kw)[1]))
        if len(before_list) > 1:
            m.spectrum(fs, nfft=64, window="hann", component=1, resident=resident)
            got["component"] = host(m.csd_psd)
            worst["component"] = max(worst.get("component", 0.0), rel(got["component"], SR.psd(before_list[1], **kw)[1]))
            assert not same_bits(got["component"], got["total"])
        with pytest.raises(ValueError):
            m.spectrum(fs, component=len(before_list))
        m.spectrum(fs, nfft=64, window="hann", type="lfp", resident=resident)
        got["lfp"] = host(m.lfp_psd)
        worst["lfp"] = max(worst.get("lfp", 0.0), rel(got["lfp"], SR.psd(before["lfp_pred"], **kw)[1]))
        m.spectrum(fs, rows=[5, 2])                                                       # defaults: boxcar, nfft = n; rows in the order asked for
        assert np.array_equal(m.f_spec, np.fft.rfftfreq(n, 1 / fs)[[5, 2]]) and isinstance(m.csd_psd, np.ndarray)
        assert rel(m.csd_psd, SR.psd(before["csd_pred"], fs=fs)[1][:, [5, 2]]) <= GATE
        m.coherence(fs, rows, nfft=64, window="hann")
        f_c, coh_ref = SR.scipy_coherence(before["csd_pred"], rows, detrend=False, **kw)      # (SciPy's default here is "constant")
        x_ref = SR.scipy_csd_mean(before["csd_pred"], rows, detrend=False, **kw)
        assert np.allclose(m.f_coh, f_c, rtol=4 * U, atol=0) and m.csd_coh.shape == (2, nz, nz) and np.iscomplexobj(m.csd_xspec)
        got["coh"], got["xspec"] = np.array(m.csd_coh), np.array(m.csd_xspec)
        worst["coh"] = max(worst.get("coh", 0.0), float(np.max(np.abs(got["coh"] - coh_ref))))        # (the largest coherence is 1)
        worst["xspec"] = max(worst.get("xspec", 0.0), rel(got["xspec"], x_ref))
        assert same_bits(got["coh"], got["coh"].transpose(0, 2, 1)) and same_bits(got["xspec"].real, got["xspec"].real.transpose(0, 2, 1))
        assert np.array_equal(got["xspec"].imag, -got["xspec"].imag.transpose(0, 2, 1))
        assert all(v <= GATE for v in worst.values()), worst
        # the prediction, phase and variance attributes are untouched
        assert all(getattr(m, k) is v for k, v in held.items())
        assert all(np.array_equal(host(held[k]), before[k]) for k in before)
        assert all(np.array_equal(v, b) for v, b in zip(comp_list(), before_list))
        if resident:
            with pytest.raises(ValueError):
                m.spectrum(fs, type="both", resident=True)
        else:
            with pytest.raises(ValueError):
                m.spectrum(fs, resident=True)
        results[resident] = got
    # the resident result, fetched, equals the host result
    assert sorted(results[True]) == sorted(results[False])
    for k in results[False]:
        assert np.array_equal(results[True][k], results[False][k]), k
    # a grid that is not uniformly spaced
    t = np.array(c["t"], dtype=np.float64)
    t[5] += 0.3 * (t[1] - t[0])
    m.predict_at(c["x"], t, type="csd")
    with pytest.raises(ValueError):
        m.spectrum(fs)
    with pytest.raises(ValueError):
        m.coherence(fs, rows)
    m.predict(c["x"], c["t"], type="csd")
    with pytest.raises(ValueError):
        m.coherence(fs, None)
    print("model %s: largest error relative to the largest entry: " % name + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))


@pytest.mark.gpu
def test_posterior_draws_give_a_spectrum_per_draw():
    from gpcsd_amd import utility_functions as UF
    from test_loo import _model, _case
    name = "1d_odd_17x37x5"
    c = _case(name)[0]
    m = _model(name)
    nz, n, R = _case(name)[3].shape
    f, A = UF.spectral_operator(n, fs=1000.0, nfft=64, window="hann")
    csd, lfp = m.sample_posterior(c["x"], c["t"], nsamples=2, type="csd", seed=3, resident=True)
    assert lfp is None and tuple(csd.shape) == (nz, n, R, 2)
    draws = np.array(csd.numpy())
    res = UF.power_spectrum(csd, A, per_trial=True)
    assert res["psd"].shape == (nz, 33, 2) and res["power"].shape == (nz, 33, R, 2)
    worst = 0.0
    for s in range(2):
        f_ref, ref = SR.psd(draws[..., s], fs=1000.0, window="hann", nfft=64)
        worst = max(worst, float(np.max(np.abs(res["psd"][..., s] - ref)) / np.max(ref)))
        assert np.max(np.abs(res["power"][..., s] - SR.periodogram(draws[..., s], fs=1000.0, window="hann", nfft=64)[1])) <= GATE * np.max(ref) * R
    assert np.allclose(f, f_ref, rtol=4 * U, atol=0) and worst <= GATE
    assert not np.array_equal(res["psd"][..., 0], res["psd"][..., 1])
    host = UF.power_spectrum(draws, A, ctx=m._context())                          # the host path on the fetched draws: the same bits
    assert np.array_equal(host["psd"], res["psd"])
    assert np.array_equal(np.array(csd.numpy()), draws)                           # the draws are left alone
    print("draws: psd %.3g of the largest entry" % worst)


@pytest.mark.gpu
def test_trial_shards_combine_to_the_unsharded_spectrum():
    """Two ranks one after the other in this process, as tests/test_phase_plv.py does it: a stand-in for gpcsd_amd.dist.TrialSharding
    whose all-reduce records what it was given and returns it, so the test forms the sum over the ranks itself."""
    from gpcsd_amd import utility_functions as UF
    from gpcsd_amd.dist import TrialSharding
    from test_loo import _model, _case

    class Rank(TrialSharding):
        def __init__(self, rank, world_size):
            self.rank, self.world_size, self.gather_predictions, self.sent = rank, world_size, False, []

        def allreduce_sum(self, values):
            self.sent.append(np.array(values, dtype=np.float64))
            return self.sent[-1]

    name = "1d_odd_17x37x5"                                                       # 5 trials: blocks of 3 and 2
    c = _case(name)[0]
    lfp = np.array(_case(name)[3])
    full = _model(name)
    full.predict(c["x"], c["t"], type="csd", resident=True)
    full.spectrum(1000.0, nfft=64, window="hann")
    full.coherence(1000.0, [2, 5], nfft=64, window="hann")
    sent = []
    for r in range(2):
        m = _model(name, lfp=lfp)
        sh = Rank(r, 2)
        m.shard_trials(sh)
        m.predict(c["x"], c["t"], type="csd", resident=bool(r))                 # one rank resident, one through host arrays
        m.spectrum(1000.0, nfft=64, window="hann", resident=bool(r))
        assert isinstance(m.csd_psd, np.ndarray)
        m.coherence(1000.0, [2, 5], nfft=64, window="hann")
        assert [s.shape for s in sh.sent] == [(17, 33), (2, 2, 17, 17)]
        sent.append(sh.sent)
    out = UF.spectrum_from_sums({"psd": sent[0][0] + sent[1][0], "xspec": sent[0][1] + sent[1][1]}, 5)
    assert np.max(np.abs(out["psd"] - full.csd_psd)) <= 1e-12 * np.max(full.csd_psd)
    assert np.max(np.abs(out["xspec"] - full.csd_xspec)) <= 1e-12 * np.max(np.abs(full.csd_xspec))
    assert np.max(np.abs(out["coh"] - full.csd_coh)) <= 1e-9
