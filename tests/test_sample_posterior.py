"""sample_posterior: joint posterior draws of CSD and LFP (gpcsd_sample_posterior, gpcsd_normals; no reference counterpart).

The expected values come from tests/posterior_ref.py: a NumPy restatement of the generator, the affine map normals -> draw
(`matheron_map`) and the dense posterior covariance prior - k^T K^-1 k (`dense_posterior`).  The CPU tests pin the restatements;
the GPU tests drive the device's affine map with unit vectors of normals -- which decides correctness whatever the signs and
rotations of the device's eigenvectors -- and the device generator end to end through sample moments.  The GPU tests print the
maxima they observe (recorded in DESIGN.md 4.5)."""
import ctypes
import os
import re

import numpy as np
import pytest

import posterior_ref as PR
import test_predict_var as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = "1d_siglist_12x40x4"        # a noise list, two temporal components
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert " ".join("%08x" % int(w) for w in PR.philox4x32_10(ctr, key)) == want


def test_restated_normals_have_the_moments_of_a_standard_normal():
    n = 1 << 20
    x = PR.normals(2024, 0, 0, n)
    mean, var, m4 = float(x.mean()), float(np.mean((x - x.mean()) ** 2)), float(np.mean(x ** 4))
    print("normals(2^20): mean %.2e (5 sigma %.2e), var - 1 %.2e (%.2e), m4 - 3 %.2e (%.2e)"
          % (mean, 5 / np.sqrt(n), var - 1, 5 * np.sqrt(2 / n), m4 - 3, 5 * np.sqrt(96 / n)))
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(m4 - 3) < 5 * np.sqrt(96 / n)
    assert np.array_equal(PR.normals(7, 1, 5, 9), PR.normals(7, 1, 0, 20)[5:14])      # a range is a slice of the stream


@pytest.mark.parametrize("type", ["csd", "lfp"])
@pytest.mark.parametrize("tchoice", ["offgrid", "train"])
@pytest.mark.parametrize("name", ["1d_odd_17x37x5", SIG])
def test_matheron_map_has_the_dense_posterior_covariance(name, tchoice, type):
    z, tstar = PR.sites(name), PR.times(name, tchoice)
    _, M = PR.matheron_map(name, z, tstar, type)
    post, prior = PR.dense_posterior(name, z, tstar, type)
    err = float(np.max(np.abs(M @ M.T - post)) / np.max(np.abs(prior)))
    print("matheron vs dense %s %s %s: %.2e" % (name, tchoice, type, err))
    assert err <= 1e-11


def _prototype_args(src, fn):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % fn, src, flags=re.S)
    assert m, "%s is not declared" % fn
    return [a.strip() for a in m.group(1).split(",")]


def test_surface_exists_and_fails_loudly_without_a_gpu():
    import torch
    from gpcsd_amd import _hip
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.gpcsd2d import GPCSD2D
    for cls in (GPCSD1D, GPCSD2D):
        assert callable(getattr(cls, "sample_posterior", None)) and callable(getattr(cls, "_sample_posterior_from_normals", None))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read(), flags=re.S)
    for fn, nargs in (("gpcsd_normals", 6), ("gpcsd_sample_posterior", 13), ("gpcsd_sample_posterior_resident", 11)):
        args = _prototype_args(src, fn)
        assert len(args) == nargs, (fn, args)
        assert fn in _hip.SIGNATURES and len(_hip.SIGNATURES[fn][1]) == nargs
        for a, ct in zip(args, _hip.SIGNATURES[fn][1]):                        # pointers bound as pointers, integers by width
            assert ("*" in a) == (ct in (_hip._P, _hip._DP) or hasattr(ct, "contents")), (fn, a, ct)
            if "unsigned long long" in a:
                assert ct is ctypes.c_ulonglong, (fn, a, ct)
    if not torch.cuda.is_available():
        m = GPCSD1D(np.zeros((24, 50, 2)), np.linspace(0, 2300, 24)[:, None], np.arange(50.0)[:, None])
        with pytest.raises(_hip.HipUnavailable):
            m.sample_posterior(m.x, m.t, nsamples=2, type="both")


def test_validation_runs_before_any_device_call():
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from gpcsd_amd.covariances import GPCSDTemporalCovSE
    x, t = np.linspace(0, 2300, 24)[:, None], np.arange(50.0)[:, None]
    np.random.seed(0)
    m = GPCSD1D(np.zeros((24, 50, 2)), x, t, temporal_cov_list=[GPCSDTemporalCovSE(t), PV._UserCov(t)])
    with pytest.raises(NotImplementedError, match="user-defined temporal covariance"):
        m.sample_posterior(x, t)
    m = GPCSD1D(np.zeros((24, 50, 2)), x, t)
    for kw in ({"type": "draws"}, {"nsamples": 0}):
        with pytest.raises(ValueError):
            m.sample_posterior(x, t, **kw)
    with pytest.raises(ValueError):
        m.sample_posterior(x, np.zeros((0, 1)))

    class Gathering:
        gather_predictions = True
    m._sharding = Gathering()
    with pytest.raises(NotImplementedError, match="gather_predictions"):
        m.sample_posterior(x, t)
    assert getattr(m, "_ctx", None) is None                                    # no context was opened on the way


# ------------------------------------------------------------------------------------------------ GPU: the generator
GEN = [(1, 0, 0, 1), (1, 0, 7, 1001), (2024, 0, 0, (1 << 20) + 3), (5, 0, (1 << 33) + 12345, 4097), (5, 1, (1 << 33) + 12345, 4097),
       ((0xDEADBEEF << 32) | 17, 1, 3, 258)]


@pytest.mark.gpu
def test_device_normals_match_the_restatement():
    """Gate 1e-13 absolute, derived: |normal| <= sqrt(106 ln 2) = 8.6 and a few ulp per libm call give about 1e-14, with ten times
    margin; the argument 2 pi u2 rounds to 7e-16 absolute."""
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    worst = 0.0
    for seed, stream, first, count in GEN:
        got, ref = ctx.normals(seed, stream, first, count), PR.normals(seed, stream, first, count)
        assert got.shape == ref.shape == (count,)
        err = float(np.max(np.abs(got - ref)))
        worst = max(worst, err)
        assert err <= 1e-13, (seed, stream, first, count, err)
    a, b = ctx.normals(5, 0, (1 << 33) + 12345, 64), ctx.normals(5, 1, (1 << 33) + 12345, 64)
    assert not np.any(a == b)                                                  # two streams
    print("device normals vs restatement: largest |difference| %.2e" % worst)


@pytest.mark.gpu
def test_device_normals_do_not_depend_on_how_a_range_is_split():
    from gpcsd_amd import _hip
    ctx = _hip.Context()
    whole = ctx.normals(99, 1, 1001, 5000)
    for cuts in ((0, 1, 2, 1337, 5000), (0, 2500, 5000), (0, 4999, 5000)):
        parts = [ctx.normals(99, 1, 1001 + a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts), whole), cuts


# ------------------------------------------------------------------------------------------------ GPU: the affine map
_ONE = {}


def _one_trial_model(name):
    """The case's model on its first trial alone."""
    if name not in _ONE:
        c = PV._case(name)[0]
        _ONE[name] = PV._model(name, lfp=np.ascontiguousarray(np.atleast_3d(PV.C.case_lfp(c))[:, :, :1]))
    return _ONE[name]


def _stack(csd, lfp):
    """(csd, lfp) of shape (nz, ntstar, R, S) -> (R, [csd (z, j); lfp (z, j)], S), the ordering of posterior_ref."""
    parts = [np.moveaxis(np.asarray(a), 2, 0).reshape(a.shape[2], -1, a.shape[3]) for a in (csd, lfp) if a is not None]
    return np.concatenate(parts, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,zchoice,tchoice", [(SIG, "between", "offgrid"), (SIG, "between", "train"), (SIG, "electrodes", "offgrid"),
                                                  ("2d_grid_48x40x2", "between", "offgrid")])
def test_affine_map_has_the_mean_of_predict_at_and_the_dense_posterior_covariance(name, zchoice, tchoice):
    """Draw 0 has all-zero normals, draw k the k-th unit vector of (Xi, E): draw 0 is the mean, M = draws - draw 0 the linear part,
    and M M^T the covariance of a draw, whatever the signs and rotations of the device's eigenvectors.  Gates (the issue's): mean
    1e-12 of its largest entry; |M M^T - dense| <= 1e-9 of the largest prior entry -- a structural mistake (a missing noise term,
    jitter, a transposed block) shows at 1e-6 or more, the smallest posterior variance of these cases is 2e-6 of the prior."""
    m = _one_trial_model(name)
    c = PV._case(name)[0]
    z, tstar = PR.sites(name, zchoice), PR.times(name, tchoice)
    nx, nt = c["x"].shape[0], c["t"].shape[0]
    ns, ntt = 2 * z.shape[0] + nx, tstar.shape[0] + nt
    nxi, ne = ns * ntt, nx * nt
    K = nxi + ne
    xi, eps = np.zeros((1, K + 1, ns, ntt)), np.zeros((1, K + 1, nx, nt))
    xi.reshape(K + 1, nxi)[np.arange(1, nxi + 1), np.arange(nxi)] = 1.0
    eps.reshape(K + 1, ne)[np.arange(nxi + 1, K + 1), np.arange(ne)] = 1.0
    draws = _stack(*m._sample_posterior_from_normals(z, tstar, "both", xi, eps))[0]               # (nout, K + 1)
    m.predict_at(z, tstar, type="both")
    mean = np.concatenate([np.array(m.csd_pred)[:, :, 0].reshape(-1), np.array(m.lfp_pred)[:, :, 0].reshape(-1)])
    # CSD and LFP differ by ~5e5 in scale: each against its own largest entry
    half = mean.size // 2
    e_mean = max(float(np.max(np.abs(draws[s, 0] - mean[s])) / np.max(np.abs(mean[s]))) for s in (slice(0, half), slice(half, None)))
    M = draws[:, 1:] - draws[:, :1]
    post, prior = PR.dense_posterior(name, z, tstar, "both")
    e_cov = float(np.max(np.abs(M @ M.T - post)) / np.max(np.abs(prior)))
    ref_mean, ref_M = PR.matheron_map(name, z, tstar, "both")
    assert ref_M.shape == M.shape
    e_ref = float(np.max(np.abs(ref_mean - mean)) / np.max(np.abs(ref_mean)))
    # the sharper form of the same statement, block by block (the CSD block is 1e-6 of the largest prior entry): printed, not gated
    blocks = [(slice(0, half), slice(0, half)), (slice(half, None), slice(0, half)), (slice(half, None), slice(half, None))]
    e_blk = max(float(np.max(np.abs((M @ M.T - post)[b])) / np.max(np.abs(prior[b]))) for b in blocks)
    print("affine map %s z=%s t*=%s (%d draws): draw 0 vs predict_at %.2e, M M^T vs dense %.2e of the largest prior entry "
          "(block by block %.2e), predict_at vs restated mean %.2e" % (name, zchoice, tchoice, K + 1, e_mean, e_cov, e_blk, e_ref))
    assert e_mean <= 1e-12
    assert e_cov <= 1e-9


# ------------------------------------------------------------------------------------------------ GPU: the device generator end to end
@pytest.mark.gpu
def test_device_draws_have_the_posterior_mean_and_covariance():
    """20 000 draws of one trial: every entry of the sample mean within 6 sqrt(C_ii / S) and of the sample covariance within
    6 sqrt((C_ii C_jj + C_ij^2) / S) of the posterior's (posterior_ref); the restatement with this seed stays within 2.2 / 2.6 sigma."""
    S = 20000
    m = _one_trial_model(SIG)
    z, tstar = PR.sites(SIG), PR.times(SIG, "offgrid")
    x = _stack(*m.sample_posterior(z, tstar, nsamples=S, type="both", seed=2024))[0]              # (nout, S)
    mu, _ = PR.matheron_map(SIG, z, tstar, "both")
    Cov, _ = PR.dense_posterior(SIG, z, tstar, "both")
    d = np.diag(Cov)
    assert np.all(d > 0)
    mhat = x.mean(axis=1)
    xc = x - mu[:, None]
    Chat = xc @ xc.T / S                                                       # about the KNOWN mean: unbiased, variance as below
    z_mean = float(np.max(np.abs(mhat - mu) / np.sqrt(d / S)))
    z_cov = float(np.max(np.abs(Chat - Cov) / np.sqrt((np.outer(d, d) + Cov ** 2) / S)))
    print("device draws, %d samples: mean within %.2f sigma, covariance within %.2f sigma (gate 6)" % (S, z_mean, z_cov))
    assert z_mean <= 6.0
    assert z_cov <= 6.0


# ------------------------------------------------------------------------------------------------ GPU: chunking and determinism
@pytest.mark.gpu
def test_same_call_same_bits_and_chunking_changes_no_draw(monkeypatch):
    m = PV._model(SIG)                                                         # 4 trials
    z, tstar = PR.sites(SIG), PR.times(SIG, "train")
    S = 25                                                                     # 100 pseudo-trials of 33 KB of scratch each
    monkeypatch.delenv("GPCSD_SAMPLE_SCRATCH_MB", raising=False)
    a = _stack(*m.sample_posterior(z, tstar, nsamples=S, type="both", seed=11))
    b = _stack(*m.sample_posterior(z, tstar, nsamples=S, type="both", seed=11))
    assert np.array_equal(a, b)
    assert not np.array_equal(a, _stack(*m.sample_posterior(z, tstar, nsamples=S, type="both", seed=12)))
    monkeypatch.setenv("GPCSD_SAMPLE_SCRATCH_MB", "1")                         # 31 pseudo-trials per chunk: 4 chunks
    ch = _stack(*m.sample_posterior(z, tstar, nsamples=S, type="both", seed=11))
    monkeypatch.delenv("GPCSD_SAMPLE_SCRATCH_MB")
    half = a.shape[1] // 2
    err = max(float(np.max(np.abs(ch[:, s] - a[:, s])) / np.max(np.abs(a[:, s]))) for s in (slice(0, half), slice(half, None)))
    print("chunked (4 chunks) vs unchunked draws: %.2e relative" % err)
    assert err <= 1e-12
    # the trial index is the slowest axis of the normals: trial 0 of the 4-trial model has the one-trial model's draws
    one = _stack(*_one_trial_model(SIG).sample_posterior(z, tstar, nsamples=S, type="both", seed=11))
    err1 = max(float(np.max(np.abs(one[0, s] - a[0, s])) / np.max(np.abs(a[0, s]))) for s in (slice(0, half), slice(half, None)))
    print("trial 0 of 4 trials vs the one-trial model: %.2e relative" % err1)
    assert err1 <= 1e-12
    # one type alone returns None for the other; resident views hold what the host arrays hold
    csd, none = m.sample_posterior(z, tstar, nsamples=S, type="csd", seed=11)
    assert none is None and csd.shape == (3, 5, 4, S)
    rc, rl = m.sample_posterior(z, tstar, nsamples=S, type="both", seed=11, resident=True)
    assert tuple(rc.shape) == (3, 5, 4, S) and hasattr(rl, "__cuda_array_interface__")
    ctx = m._context()
    assert np.array_equal(_stack(ctx.fetch("post_sample_csd", (3, 5, 4, S)), ctx.fetch("post_sample_lfp", (3, 5, 4, S))), a)


class _Block:
    """A stand-in with TrialSharding's view of one rank: a contiguous block of the trials, nothing gathered."""
    gather_predictions = False

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.rank, self.world_size = a, 4                                      # (what the model keys its resident block by)

    def local_slice(self, ntrials):
        return slice(self.a, self.b)


@pytest.mark.gpu
def test_a_rank_draws_for_its_block_what_the_unsharded_job_draws():
    c = PV._case(SIG)[0]
    z, tstar = PR.sites(SIG), PR.times(SIG, "offgrid")
    whole = _stack(*PV._model(SIG).sample_posterior(z, tstar, nsamples=6, type="both", seed=5))            # 4 trials
    half = whole.shape[1] // 2
    for a, b in ((0, 2), (1, 3), (3, 4)):
        m = PV._model(SIG, lfp=PV.C.case_lfp(c))
        m._sharding = _Block(a, b)
        part = _stack(*m.sample_posterior(z, tstar, nsamples=6, type="both", seed=5))
        assert part.shape[0] == b - a
        err = max(float(np.max(np.abs(part[:, s] - whole[a:b, s])) / np.max(np.abs(whole[a:b, s]))) for s in (slice(0, half), slice(half, None)))
        print("block [%d, %d) of 4 trials vs the unsharded draws: %.2e relative" % (a, b, err))
        assert err <= 1e-12
    # the offset belongs to the resident data: new data start at trial 0 again
    from gpcsd_amd import _hip
    lfp = np.ascontiguousarray(PV.C.case_lfp(c))
    m = PV._model(SIG, lfp=lfp)
    ctx = m._sync_device()
    hp, _keep = m._hparams(0.0)

    def draw():
        res = ctx.sample_posterior(hp, z, tstar, _hip.PRED_BOTH, 6, 5, 4)
        return _stack(res["csd"], res["lfp"])
    ctx.set_trial_offset(1)
    assert not np.array_equal(draw(), whole)
    ctx.set_lfp(lfp)
    again = draw()
    err = max(float(np.max(np.abs(again[:, s] - whole[:, s])) / np.max(np.abs(whole[:, s]))) for s in (slice(0, half), slice(half, None)))
    print("after set_lfp the offset is 0 again: %.2e relative to the unsharded draws" % err)
    assert err <= 1e-12


# ------------------------------------------------------------------------------------------------ GPU: errors
@pytest.mark.gpu
def test_c_abi_argument_checks_and_the_means_are_left_alone():
    from gpcsd_amd import _hip
    m = PV._model(SIG)
    c = PV._case(SIG)[0]
    z, tstar = PR.sites(SIG), PR.times(SIG, "offgrid")
    m.predict_at(z, tstar, type="csd")
    mean = np.array(m.csd_pred)
    m.predict_at(z, tstar, type="csd", resident=True)
    ctx = m._context()
    before = np.array(ctx.fetch("pred_out_csd", (3, 4, 4)))
    hp, _keep = m._hparams(0.0)
    lib = ctx._lib
    zz, ts = np.ascontiguousarray(z.reshape(-1)), np.ascontiguousarray(tstar.reshape(-1))
    nx, nt = c["x"].shape[0], c["t"].shape[0]
    xi, eps = np.zeros((4, 2, 3 + nx, 4 + nt)), np.zeros((4, 2, nx, nt))
    out = np.empty((3, 4, 4, 2))
    dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    call = lambda S, a=None, b=None, p=hp, nts=4: lib.gpcsd_sample_posterior(ctx._h, ctypes.byref(p), dp(zz), 3, dp(ts), nts, _hip.PRED_CSD,
                                                                            S, 7, dp(a), dp(b), dp(out), None)
    assert call(2) == 0
    assert call(2, xi, eps) == 0
    assert np.max(np.abs(out - mean[..., None])) <= 1e-12 * np.max(np.abs(mean))       # zero normals: the mean of predict_at
    assert call(0) == -3
    assert call(2, xi, None) == -3 and call(2, None, eps) == -3
    assert b"both" in lib.gpcsd_last_error(ctx._h)
    assert lib.gpcsd_sample_posterior_resident(ctx._h, ctypes.byref(hp), dp(zz), 3, dp(ts), 4, 0, 2, 7, None, None) == -3
    assert call(2, nts=1 << 20) == _hip.ERR_CAPACITY                           # ntstar + nt beyond the eigensolver; tstar (4 doubles) is not read
    host = _hip.HParams.from_buffer_copy(hp)
    host.kind[0] = _hip.KIND_HOST
    assert call(2, p=host) == -3
    assert b"user-defined" in lib.gpcsd_last_error(ctx._h)
    assert call(2) == 0                                                        # the context is as usable as before
    assert np.array_equal(np.array(ctx.fetch("pred_out_csd", (3, 4, 4))), before)
