"""Band phase and phase-locking value on the device (gpcsd_analytic, gpcsd_plv; no reference counterpart in the package).

The expected values come from tests/phase_ref.py: the analytic signal is `einsum('jt,ztm->zjm', A, x)` with A the operator of
`utility_functions.analytic_operator` (itself pinned to the direct SciPy call by the CPU tests), amplitude / phase / unit phasor
are NumPy's, the PLV is an einsum over the trials (in longdouble where the kernel alone is tested).  Bounds, u = 2^-53:

  Re, Im (recovered as amp * u_re, amp * u_im) and amp: 1e-6 of the largest entry (the project's gate), and the GEMM core's
      rounding bound (K + 8) u sum_t |A||x| plus 4 u amp for the division and the product that recover them (amp: both parts'
      bounds plus 2 u amp for the hypot);
  unit phasors and phases, entrywise where amp_ref >= 1e-3 max amp: GATE * max amp / amp_ref (what the gate on Re / Im leaves of
      a quotient by amp), phases as wrapped differences; at most 1 % of the entries may fall under that floor;
  |u|^2 - 1 <= 8 u;  c_re, c_im from given phasors: (2 R + 8) u (2 R products of magnitude <= 1, divided by R), plv sqrt(2) x that;
  a PLV formed from a FIELD inherits the phasors' bound: sqrt(2) (mean_r du_a + mean_r du_b) on top of the kernel's own.

The GPU tests print the maxima they observe."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import phase_ref as P

GATE = 1e-6                       # the project's contract (tests/test_hip_parity.py)
U = 2.0 ** -53
FLOOR = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL4 = ("phase", "amp", "u_re", "u_im")


@functools.lru_cache(maxsize=None)
def _operator(name, at=None):
    from gpcsd_amd import utility_functions as UF
    n, kind, design = P.filters()[name]
    A = UF.analytic_operator(n, at=None if at is None else list(at), **{kind: design})
    A.setflags(write=False)
    return A


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name,tol", [("sos37", 1e-12), ("sos95", 1e-12), ("ba40", GATE), ("ba100", GATE), ("none", 1e-12)])
def test_operator_equals_the_direct_scipy_call(name, tol):
    """Observed (relative to the largest |analytic|): sos 1.1e-15 (n = 37) / 2.6e-14 (n = 95); (b, a) 5e-13 (n = 40) / 1e-8
    (n = 100, 8-12 Hz at 1 kHz: the conditioning of the transfer-function form itself); pure Hilbert 4e-16."""
    from gpcsd_amd import utility_functions as UF
    if name == "none":
        n, kind, design = 37, None, None
        A = UF.analytic_operator(n)
    else:
        n, kind, design = P.filters()[name]
        A = _operator(name)
    assert A.shape == (n, n) and A.dtype == np.complex128
    x = P.signal(7, 5, n, 7)
    ref = P.direct_analytic(x, kind, design, axis=1)
    got = P.analytic(A, x)[0]
    err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print("operator %s: %.2e of max |analytic| (bound %.0e); min / max amplitude %.2e" % (name, err, tol, np.min(np.abs(ref)) / np.max(np.abs(ref))))
    assert err <= tol


def test_operator_keeps_rows_in_the_order_asked_for():
    from gpcsd_amd import utility_functions as UF
    n, kind, design = P.filters()["sos37"]
    at = [30, 2, 17, 2]
    A = UF.analytic_operator(n, sos=design, at=at)
    assert A.shape == (4, n) and np.array_equal(A, _operator("sos37")[at])
    x = P.signal(8, 5, n, 7)
    ref = P.direct_analytic(x, kind, design, axis=1)[:, at]
    assert np.max(np.abs(P.analytic(A, x)[0] - ref)) <= 1e-12 * np.max(np.abs(ref))
    padded = UF.analytic_operator(n, sos=design, padtype="even", padlen=5)          # filter arguments reach the filter
    import scipy.signal as ss
    ref = ss.hilbert(ss.sosfiltfilt(design, x, axis=1, padtype="even", padlen=5), axis=1)
    assert np.max(np.abs(P.analytic(padded, x)[0] - ref)) <= 1e-12 * np.max(np.abs(ref))
    with pytest.raises(ValueError):
        UF.analytic_operator(n, sos=design, ba=(np.ones(1), np.ones(1)))


def test_host_combine_of_rank_sums_equals_the_unsharded_plv():
    from gpcsd_amd import utility_functions as UF
    rs = np.random.RandomState(5)
    ph = rs.uniform(-np.pi, np.pi, (6, 2, 5, 1))
    c_re, c_im, plv = P.plv(np.cos(ph), np.sin(ph))
    sums = 0.0
    for sl in (slice(0, 3), slice(3, 5)):
        b_re, b_im, _ = P.plv(np.cos(ph[:, :, sl]), np.sin(ph[:, :, sl]))
        sums = sums + (sl.stop - sl.start) * np.stack([b_re, b_im])
    got, c = UF.plv_from_sums(sums, 5)
    assert np.max(np.abs(got - plv)) <= 8 * U and np.max(np.abs(c - (c_re + 1j * c_im))) <= 8 * U
    got2, c2 = UF.plv_from_sums(sums[0] + 1j * sums[1], 5)                           # the complex form of the same sums
    assert np.array_equal(got2, got) and np.array_equal(c2, c)


def test_surface_exists_and_fails_loudly_without_a_gpu():
    import torch
    from gpcsd_amd import build, _hip, utility_functions as UF
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    for cls in (GPCSD1D, GPCSD2D):
        assert callable(getattr(cls, "phase", None)) and callable(getattr(cls, "plv", None))
    assert "phase.hip" in build.SOURCES
    build.build(verbose=False)
    lib = _hip.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read(), flags=re.S)
    for fn in ("gpcsd_analytic", "gpcsd_analytic_resident", "gpcsd_plv", "gpcsd_plv_resident"):
        assert re.search(r"\b%s\s*\(" % fn, src), "%s is not declared" % fn
        assert fn in _hip.SIGNATURES
        assert hasattr(lib, fn), "libgpcsd_hip.so does not export %s" % fn
    if not torch.cuda.is_available():
        with pytest.raises(_hip.HipUnavailable):
            UF.band_phase(np.zeros((1, 4, 1)), np.eye(4))
        with pytest.raises(_hip.HipUnavailable):
            UF.plv(np.zeros((2, 1, 3)))


# ------------------------------------------------------------------------------------------------ GPU: the kernels alone
_CTX = []


def _ctx():
    if not _CTX:
        from gpcsd_amd import _hip
        _CTX.append(_hip.Context())
    return _CTX[0]


def _check_fields(res, x, A, worst, label):
    """Every output of the analytic kernel against the NumPy reference of the field x under A; the observed maxima go to `worst`."""
    w, (mag_re, mag_im) = P.analytic(A, x)
    amp_ref, phase_ref, u_ref = P.phasors(w)
    K = x.shape[1]
    top = float(np.max(amp_ref))
    amp, phase, u_re, u_im = (np.asarray(res[k]) for k in ("amp", "phase", "u_re", "u_im"))
    assert amp.shape == w.shape == phase.shape == u_re.shape == u_im.shape, label
    e_re, e_im, e_amp = np.abs(amp * u_re - w.real), np.abs(amp * u_im - w.imag), np.abs(amp - amp_ref)
    obs = {"re_im": float(max(e_re.max(), e_im.max())) / top, "amp": float(e_amp.max()) / top,
           "gemm_bound": float(max(np.max(e_re / ((K + 8) * U * mag_re + 4 * U * amp_ref + 1e-300)),
                                   np.max(e_im / ((K + 8) * U * mag_im + 4 * U * amp_ref + 1e-300)),
                                   np.max(e_amp / ((K + 8) * U * (mag_re + mag_im) + 2 * U * amp_ref + 1e-300))))}
    ok = amp_ref >= FLOOR * top
    assert np.count_nonzero(~ok) <= 0.01 * ok.size, (label, "entries under the amplitude floor", np.count_nonzero(~ok), ok.size)
    bound = GATE * top / amp_ref[ok]
    obs["phasor"] = float(np.max(np.maximum(np.abs(u_re - u_ref.real)[ok], np.abs(u_im - u_ref.imag)[ok]) / bound))
    obs["phase"] = float(np.max(np.abs(P.wrap(phase - phase_ref))[ok] / bound))
    obs["unit"] = float(np.max(np.abs(u_re * u_re + u_im * u_im - 1.0))) / U
    for k, v in obs.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert obs["re_im"] <= GATE and obs["amp"] <= GATE, (label, obs)
    assert obs["gemm_bound"] <= 1.0, (label, obs)
    assert obs["phasor"] <= 1.0 and obs["phase"] <= 1.0, (label, obs)
    assert obs["unit"] <= 8.0, (label, obs)
    return amp_ref, top


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sos37", "sos40"])
def test_analytic_kernel_against_numpy(name):
    """nts = 37 has a K tail of two k steps (the second partial), 40 one of two full ones; nsel = 1, 2 leave most of a 32-row tile
    clamped and nsel = nts needs a second, partial one; the columns (z, m) of 17 planes of 1, 5, 21 trials cross plane borders
    inside a fragment, fill more than one 64-column tile (17 x 5, 17 x 21) and end inside one.  Observed on an MI355X: Re, Im, amp
    8.1e-16 of the largest entry, 0.066 of the GEMM rounding bound; phasors / phases 5.3e-10 / 7.6e-10 of their bound; | |u|^2 - 1 |
    4 u."""
    ctx = _ctx()
    nts = P.filters()[name][0]
    worst = {}
    for nz in (1, 17):
        for M in (1, 5, 21):
            x = P.signal(1000 + 37 * nz + M, nz, nts, M)
            for nsel in (1, 2, nts):
                A = _operator(name) if nsel == nts else _operator(name, (nts - 4, 3)[:nsel])
                res = ctx.analytic(x, A, want=ALL4)
                _check_fields(res, x, A, worst, (name, nz, M, nsel))
    print("analytic %s: " % name + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))


@pytest.mark.gpu
def test_analytic_zero_columns_and_skipped_outputs():
    from gemm_ref import same_bits
    ctx = _ctx()
    lib = ctx._lib
    A = _operator("sos37", (20, 5, 36))
    x = P.signal(3, 3, 37, 5)
    x[:, :, 2] = 0.0                                            # a trial that is zero at every site, and a site that is zero in every trial
    x[1] = 0.0
    x[0, :, 4] = -0.0
    full = ctx.analytic(x, A, want=ALL4)
    zero = np.zeros((3, 3, 5), dtype=bool)
    zero[:, :, 2] = zero[1] = zero[0, :, 4] = True
    assert np.all(full["amp"][zero] == 0.0) and same_bits(full["phase"][zero], np.zeros(zero.sum()))
    assert np.all(full["u_re"][zero] == 1.0) and same_bits(full["u_im"][zero], np.zeros(zero.sum()))
    assert np.all(full["amp"][~zero] > 0.0)
    # every subset of the outputs: the arrays handed over get the bits of the full call, the others keep the sentinel
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None
    Are, Aim = np.ascontiguousarray(A.real), np.ascontiguousarray(A.imag)
    order = ("phase", "amp", "u_re", "u_im")
    for mask in range(1, 16):
        host = {k: np.full((3, 3, 5), -777.0) for k in order}
        args = [dp(host[k]) if mask & (1 << i) else None for i, k in enumerate(order)]
        assert lib.gpcsd_analytic(ctx._h, dp(x), 3, 37, 5, dp(Are), dp(Aim), 3, *args) == 0
        for i, k in enumerate(order):
            if mask & (1 << i):
                assert same_bits(host[k], full[k]), (mask, k)
            else:
                assert np.all(host[k] == -777.0), (mask, k)
        got = ctx.analytic(x, A, want=[k for i, k in enumerate(order) if mask & (1 << i)])
        assert sorted(got) == sorted(k for i, k in enumerate(order) if mask & (1 << i))


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [1, 5, 17, 70])
def test_plv_kernel_against_extended_precision(nz):
    """nz = 70 crosses the 64-wide tile: a diagonal tile, an off-diagonal one and its mirror image.  R = 1, 3 sit inside one k step,
    50 is six K tiles and a tail; S = 3 reads the trials with stride 3.  Observed on an MI355X: c_re / c_im at most 0.195 of
    (2 R + 8) u, plv 0.148 of sqrt(2) times that."""
    from gemm_ref import same_bits
    ctx = _ctx()
    rs = np.random.RandomState(77 + nz)
    worst = {"c": 0.0, "plv": 0.0}
    for nsel in (1, 4):
        for R in (1, 3, 50):
            for S in (1, 3):
                ph = rs.uniform(-np.pi, np.pi, (nz, nsel, R, S))
                u_re, u_im = np.cos(ph), np.sin(ph)
                c_re, c_im, plv = ctx.plv(u_re, u_im)
                assert c_re.shape == c_im.shape == plv.shape == (S, nsel, nz, nz)
                r_re, r_im, r_plv = P.plv(u_re, u_im, dtype=P.LD)
                bound = (2 * R + 8) * U
                e_c = float(max(np.max(np.abs(c_re - r_re)), np.max(np.abs(c_im - r_im)))) / bound
                e_p = float(np.max(np.abs(plv - r_plv))) / (np.sqrt(2.0) * bound)
                worst["c"], worst["plv"] = max(worst["c"], e_c), max(worst["plv"], e_p)
                assert e_c <= 1.0 and e_p <= 1.0, (nz, nsel, R, S, e_c, e_p)
                # Hermitian bit for bit; the diagonal is |u|^2 averaged and an exact zero
                assert same_bits(plv, plv.transpose(0, 1, 3, 2)) and same_bits(c_re, c_re.transpose(0, 1, 3, 2))
                assert np.array_equal(c_im, -c_im.transpose(0, 1, 3, 2))
                assert np.all(np.diagonal(c_im, axis1=2, axis2=3) == 0.0)
                again = ctx.plv(u_re, u_im)                                    # the same call: the same bits
                assert all(same_bits(a, b) for a, b in zip(again, (c_re, c_im, plv)))
                none_re, none_im, only = ctx.plv(u_re, u_im, want_c=False)
                assert none_re is None and none_im is None and same_bits(only, plv)
    print("plv nz=%d: largest error / bound: c %.3f, plv %.3f" % (nz, worst["c"], worst["plv"]))


@pytest.mark.gpu
def test_plv_of_a_common_offset_per_site_is_one():
    """Every trial carries the same phase offset per site: u_a conj(u_b) = exp(i (off_a - off_b)) in every trial, so plv = 1 and the
    angle is the offset difference.  Angle tolerance: the rounded sums base + off (u * 2 pi per site), the rounded cos / sin (u
    each) and the kernel's bound on c, seen from a resultant of length one."""
    from gpcsd_amd import utility_functions as UF
    ctx = _ctx()
    rs = np.random.RandomState(9)
    nz, nsel, R = 17, 2, 50
    base = rs.uniform(-np.pi / 2, np.pi / 2, (1, nsel, R))
    off = rs.uniform(-np.pi / 2, np.pi / 2, (nz, 1, 1))
    plv, c = UF.plv(base + off, ctx=ctx)                                        # a host phase array: cos / sin formed on the host
    assert plv.shape == (nsel, nz, nz) and c.shape == (nsel, nz, nz) and np.iscomplexobj(c)
    bound = np.sqrt(2.0) * (2 * R + 8) * U
    assert np.max(np.abs(plv - 1.0)) <= bound + 4 * U
    want = P.wrap(off[:, 0, 0][:, None] - off[:, 0, 0][None, :])
    assert np.max(np.abs(P.wrap(np.angle(c) - want[None]))) <= bound + (4 * np.pi + 6) * U


# ------------------------------------------------------------------------------------------------ GPU: through a model
def _field_plv(x, A):
    """Reference PLV of the field x (nz, n, R) under A and the tolerance it inherits from the phasors' bound."""
    w = P.analytic(A, x)[0]
    amp, _, u = P.phasors(w)
    top = float(np.max(amp))
    du = GATE * top / np.maximum(amp, FLOOR * top)
    c_re, c_im, plv = P.plv(u.real[..., None], u.imag[..., None])
    m = du.mean(axis=2).T                                                       # (nsel, nz)
    tol = np.sqrt(2.0) * (m[:, :, None] + m[:, None, :]) + np.sqrt(2.0) * (2 * x.shape[2] + 8) * U
    return c_re[0], c_im[0], plv[0], tol


def _check_model_plv(m, name, x, A, worst):
    c_re, c_im, plv, tol = _field_plv(x, A)
    got, ang = getattr(m, name + "_plv"), getattr(m, name + "_plv_angle")
    assert got.shape == plv.shape == ang.shape
    e = float(np.max(np.abs(got - plv) / tol))
    off = ~np.eye(plv.shape[1], dtype=bool)[None] & (plv > 0.1)                 # the angle of a resultant of some length
    e_ang = float(np.max(np.abs(P.wrap(ang - np.arctan2(c_im, c_re)))[off] * plv[off] / np.broadcast_to(tol, plv.shape)[off])) if off.any() else 0.0
    worst["plv"] = max(worst.get("plv", 0.0), float(np.max(np.abs(got - plv))))
    assert e <= 1.0 and e_ang <= 1.0, (name, e, e_ang)
    assert np.array_equal(got, got.transpose(0, 2, 1)) and np.array_equal(ang, -ang.transpose(0, 2, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("name,opname", [("1d_odd_17x37x5", "sos37"), ("2d_grid_48x40x2", "sos40")])
def test_model_phase_and_plv_of_the_posterior_mean(name, opname):
    from gemm_ref import same_bits
    from test_loo import _model, _case
    c = _case(name)[0]
    m = _model(name)
    ctx = m._context()
    at = (20, 5)
    A = _operator(opname, at)
    nz, n, R = _case(name)[3].shape
    worst = {}
    # resident predictions: read in HBM
    m.predict_at(c["x"], c["t"], type="both", resident=True)
    held = {k: getattr(m, k) for k in ("csd_pred", "lfp_pred", "csd_pred_list", "lfp_pred_list", "t_pred", "x_pred")}
    before = {k: np.array(held[k].numpy()) for k in ("csd_pred", "lfp_pred")}
    before_list = np.array(ctx.fetch("pred_out_csd_list", (len(m.temporal_cov_list), nz, n, R)))
    m.phase(A, type="both", at=at)
    assert np.array_equal(m.t_phase, np.asarray(c["t"])[list(at)])
    m.plv(type="both")
    dev = {}
    for k in ("csd", "lfp"):
        res = {"phase": getattr(m, k + "_phase"), "amp": getattr(m, k + "_amp")}
        assert isinstance(res["phase"], np.ndarray) and res["phase"].shape == (nz, 2, R)
        full = ctx.analytic(before[k + "_pred"], A, want=ALL4)                   # (the host-array entry point on the fetched field)
        assert same_bits(full["phase"], res["phase"]) and same_bits(full["amp"], res["amp"])
        _check_fields(full, before[k + "_pred"], A, worst, (name, k))
        _check_model_plv(m, k, before[k + "_pred"], A, worst)
        dev[k] = {a: np.array(getattr(m, k + a)) for a in ("_phase", "_amp", "_plv", "_plv_angle")}
    # the prediction attributes and buffers are untouched
    assert all(getattr(m, k) is v for k, v in held.items())
    assert all(same_bits(held[k].numpy(), before[k]) for k in before)
    assert same_bits(ctx.fetch("pred_out_csd_list", before_list.shape), before_list)
    # resident results, one type per call: views of the library's buffers with the same bits
    m.phase(A, type="lfp", resident=True)
    assert m.t_phase is None and hasattr(m.lfp_phase, "__cuda_array_interface__") and tuple(m.lfp_amp.shape) == (nz, 2, R)
    assert same_bits(m.lfp_phase.numpy(), dev["lfp"]["_phase"]) and same_bits(m.lfp_amp.numpy(), dev["lfp"]["_amp"])
    m.plv(type="lfp")
    assert same_bits(m.lfp_plv, dev["lfp"]["_plv"])
    with pytest.raises(ValueError):
        m.phase(A, type="both", resident=True)
    # one temporal component of the list, read at its offset in the list's buffer (the 2D case has two components)
    with pytest.raises(ValueError):
        m.phase(A, type="csd", component=len(m.temporal_cov_list))
    if len(m.temporal_cov_list) > 1:
        m.phase(A, type="csd", component=1)
        comp = before_list[1]
        _check_fields(ctx.analytic(comp, A, want=ALL4), comp, A, worst, (name, "component 1"))
        assert same_bits(m.csd_phase, ctx.analytic(comp, A, want=("phase",))["phase"])
        assert not same_bits(m.csd_phase, dev["csd"]["_phase"])
    # host predictions: the same bits
    m.predict_at(c["x"], c["t"], type="both")
    assert isinstance(m.csd_pred, np.ndarray) and same_bits(m.csd_pred, before["csd_pred"]) and same_bits(m.lfp_pred, before["lfp_pred"])
    pred = [np.array(m.csd_pred), np.array(m.lfp_pred)]
    m.phase(A, type="both", at=at)
    m.plv(type="both")
    for k in ("csd", "lfp"):
        for a in ("_phase", "_amp", "_plv", "_plv_angle"):
            assert same_bits(getattr(m, k + a), dev[k][a]), (k, a)
    assert same_bits(m.csd_pred, pred[0]) and same_bits(m.lfp_pred, pred[1])
    print("model %s: " % name + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))


@pytest.mark.gpu
def test_posterior_draws_give_a_plv_per_draw():
    from gpcsd_amd import utility_functions as UF
    from test_loo import _model, _case
    name = "1d_odd_17x37x5"
    c = _case(name)[0]
    m = _model(name)
    nz, n, R = _case(name)[3].shape
    A = _operator("sos37", (20, 5))
    csd, lfp = m.sample_posterior(c["x"], c["t"], nsamples=2, type="csd", seed=3, resident=True)
    assert lfp is None and tuple(csd.shape) == (nz, n, R, 2)
    draws = np.array(csd.numpy())
    ph = UF.band_phase(csd, A, want=("phase", "u_re", "u_im"), resident=True)
    assert tuple(ph["u_re"].shape) == (nz, 2, R, 2) and tuple(ph["phase"].shape) == (nz, 2, R, 2)
    plv, cc = UF.plv(ph)
    assert plv.shape == (2, 2, nz, nz) and cc.shape == plv.shape
    host = UF.band_phase(draws, A, want=("phase",), ctx=m._context())           # the host path on the fetched draws: the same bits
    assert np.array_equal(host["phase"], ph["phase"].numpy())
    worst = 0.0
    for s in range(2):
        c_re, c_im, ref, tol = _field_plv(draws[..., s], A)
        worst = max(worst, float(np.max(np.abs(plv[s] - ref))))
        assert np.max(np.abs(plv[s] - ref) / tol) <= 1.0 and np.max(np.abs(cc[s] - (c_re + 1j * c_im)) / tol) <= np.sqrt(2.0)
    assert not np.array_equal(plv[0], plv[1])
    assert np.array_equal(np.array(csd.numpy()), draws)                        # the draws are left alone
    print("draws: largest |plv - ref| %.3g" % worst)


@pytest.mark.gpu
def test_trial_shards_combine_to_the_unsharded_plv():
    """Two ranks one after the other in this process, as tests/test_loo.py does it: a stand-in for gpcsd_amd.dist.TrialSharding whose
    all-reduce records what it was given and returns it, so the test forms the sum over the ranks itself."""
    from gpcsd_amd import utility_functions as UF
    from gpcsd_amd.dist import TrialSharding
    from test_loo import _model, _case

    class Rank(TrialSharding):
        def __init__(self, rank, world_size):
            self.rank, self.world_size, self.gather_predictions, self.sent = rank, world_size, False, []

        def allreduce_sum(self, values):
            self.sent.append(np.array(values, dtype=np.float64))
            return self.sent[-1]

    name = "1d_odd_17x37x5"                                                      # 5 trials: blocks of 3 and 2
    c = _case(name)[0]
    lfp = np.array(_case(name)[3])
    A = _operator("sos37", (20, 5))
    full = _model(name)
    full.predict_at(c["x"], c["t"], type="both", resident=True)
    full.phase(A, type="both")
    full.plv(type="both")
    whole = {k: (np.array(getattr(full, k + "_plv")), np.array(getattr(full, k + "_plv_angle"))) for k in ("csd", "lfp")}
    sent = []
    for r in range(2):
        m = _model(name, lfp=lfp)
        sh = Rank(r, 2)
        m.shard_trials(sh)
        m.predict_at(c["x"], c["t"], type="both", resident=bool(r))             # one rank resident, one through host arrays
        m.phase(A, type="both")
        assert m.csd_phase.shape == (17, 2, (3, 2)[r])
        m.plv(type="both")
        assert len(sh.sent) == 2 and all(s.shape == (2, 2, 17, 17) for s in sh.sent)      # one all-reduce per requested type
        sent.append(sh.sent)
    for i, k in enumerate(("csd", "lfp")):
        plv, cc = UF.plv_from_sums(sent[0][i] + sent[1][i], 5)
        assert np.max(np.abs(plv - whole[k][0])) <= 1e-12, k
        big = whole[k][0] > 0.1
        assert np.max(np.abs(P.wrap(np.angle(cc) - whole[k][1]))[big]) <= 1e-11, k


@pytest.mark.gpu
def test_errors():
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    lib = ctx._lib
    one = np.ones(1)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    an = lambda nz, nts, M, nsel, x=one, out=one: lib.gpcsd_analytic(ctx._h, dp(x) if x is not None else None, nz, nts, M, dp(one), dp(one), nsel,
                                                                     dp(out), None, None, None)
    pl = lambda nz, nsel, R, S, u=one: lib.gpcsd_plv(ctx._h, dp(u) if u is not None else None, dp(one), nz, nsel, R, S, None, None, dp(one))
    # empty or NULL arguments
    assert an(0, 1, 1, 1) == -3 and an(1, 0, 1, 1) == -3 and an(1, 1, 0, 1) == -3 and an(1, 1, 1, 0) == -3 and an(1, 1, 1, 1, x=None) == -3
    assert pl(0, 1, 1, 1) == -3 and pl(1, 0, 1, 1) == -3 and pl(1, 1, 0, 1) == -3 and pl(1, 1, 1, 0) == -3 and pl(1, 1, 1, 1, u=None) == -3
    # capacity, before anything is read or launched: the arrays hold ONE double each
    assert an(1, 1, 1 << 23, 1) == _hip.ERR_CAPACITY and an(1, 1 << 22, 1, 1) == _hip.ERR_CAPACITY and an(1 << 20, 1, 1 << 11, 1) == _hip.ERR_CAPACITY
    assert pl(1, 1, 1 << 12, 1 << 11) == _hip.ERR_CAPACITY and pl(1 << 21, 1, 1, 1) == _hip.ERR_CAPACITY
    res = lambda name, off, nz, nts, M, nsel, mask=15: lib.gpcsd_analytic_resident(ctx._h, name, off, nz, nts, M, dp(one), dp(one), nsel, mask)
    assert res(b"pred_out_csd", 0, 1, 1, 1 << 23, 1) == _hip.ERR_CAPACITY
    # the phasors do not exist yet; unknown and short sources
    assert lib.gpcsd_plv_resident(ctx._h, 1, 1, 1, 1) == -4
    assert res(b"no_such_buffer", 0, 1, 1, 1, 1) == -2 and b"no_such_buffer" in lib.gpcsd_last_error(ctx._h)
    assert res(None, 0, 1, 1, 1, 1) == -3 and res(b"op_in0", 0, 1, 1, 1, 1, mask=0) == -3
    x = np.array([3.0, -4.0])
    assert an(1, 1, 2, 1, x=x, out=np.empty(2)) == 0                            # leaves "op_in0" with two doubles
    assert res(b"op_in0", 0, 1, 1, 2, 1) == 0
    assert res(b"op_in0", 1, 1, 1, 2, 1) == -3 and res(b"op_in0", 0, 1, 1, 1 << 20, 1) == -3 and res(b"phasor_re", 0, 1, 1, 1, 1) == -3
    # a failed call took the phasors' shape with it only if it got as far as writing them: (1, 1, 2) is still there
    assert lib.gpcsd_plv_resident(ctx._h, 1, 1, 2, 1) == 0 and lib.gpcsd_plv_resident(ctx._h, 1, 1, 1, 2) == 0
    assert lib.gpcsd_plv_resident(ctx._h, 2, 1, 1, 1) == -4 and lib.gpcsd_plv_resident(ctx._h, 1, 1, 3, 1) == -4
    assert res(b"op_in0", 0, 1, 1, 2, 1, mask=3) == 0 and lib.gpcsd_plv_resident(ctx._h, 1, 1, 2, 1) == -4      # phase and amp only: no phasors
    # the context is as usable as before: A = 1 + i on x = (3, -4)
    got = ctx.analytic(x.reshape(1, 1, 2), np.array([[1.0 + 1.0j]]), want=ALL4)
    assert np.allclose(got["amp"].ravel(), [3 * np.sqrt(2.0), 4 * np.sqrt(2.0)], rtol=4 * U, atol=0)
    assert np.allclose(got["phase"].ravel(), [np.pi / 4, -3 * np.pi / 4], rtol=4 * U, atol=0)
    c_re, c_im, plv = ctx.plv(got["u_re"].reshape(2, 1, 1, 1), got["u_im"].reshape(2, 1, 1, 1))      # two "sites", one trial
    assert abs(plv[0, 0, 0, 1] - 1.0) <= 12 * U and abs(c_re[0, 0, 0, 1] + 1.0) <= 12 * U and abs(c_im[0, 0, 0, 1]) <= 12 * U
