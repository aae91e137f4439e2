"""Matern-3/2 and Matern-5/2 temporal kernels: what needs no GPU -- the constants of the three places that name a kind, the host
derivative of the stationary classes against central differences of the long-double kernel, the refusal of an unknown kind, and
that a model of the new classes is a device-kind model.  (The device side: tests/test_matern_kinds.py.)"""
import os
import re

import numpy as np
import pytest

import matern_ref as MR

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _classes():
    from gpcsd_amd import covariances as CV
    return {MR.SE: CV.GPCSDTemporalCovSE, MR.MATERN: CV.GPCSDTemporalCovMatern, MR.MATERN32: CV.GPCSDTemporalCovMatern32,
            MR.MATERN52: CV.GPCSDTemporalCovMatern52}


def test_kinds_agree_between_header_python_and_classes():
    from gpcsd_amd import _hip, covariances as CV, gpcsd1d, gpcsd2d
    src = open(os.path.join(ROOT, "include", "gpcsd_hip.h")).read()
    header = {n: int(v) for n, v in re.findall(r"#define\s+GPCSD_KIND_(\w+)\s+(\d+)", src)}
    assert header == {"SE": 0, "MATERN": 1, "HOST": 2, "MATERN32": 3, "MATERN52": 4}
    assert (_hip.KIND_SE, _hip.KIND_MATERN, _hip.KIND_HOST, _hip.KIND_MATERN32, _hip.KIND_MATERN52) == (0, 1, 2, 3, 4)
    assert (MR.SE, MR.MATERN, MR.HOST, MR.MATERN32, MR.MATERN52) == (0, 1, 2, 3, 4)
    assert set(_hip.DEVICE_KINDS) == {0, 1, 3, 4}
    for kind, cls in _classes().items():
        assert cls.kind == kind and issubclass(cls, CV._StationaryTemporalCov)
    assert CV.GPCSDTemporalCovMatern32._sigma2_min == 1e-8 and CV.GPCSDTemporalCovMatern52._sigma2_min == 1e-8
    for mod in (gpcsd1d, gpcsd2d):                          # exported wherever the two reference classes are
        assert mod.GPCSDTemporalCovMatern32 is CV.GPCSDTemporalCovMatern32 and mod.GPCSDTemporalCovMatern52 is CV.GPCSDTemporalCovMatern52
    # sizeof(gpcsd_hparams) is pinned by tests/test_abi.py: no new parameter came with the kinds
    hdr = open(os.path.join(ROOT, "gpcsd_amd", "csrc", "temporal_kernel.hpp")).read()
    assert "default:" not in hdr                            # the dispatch has no default evaluation


def test_reference_float64_agrees_with_long_double():
    d = np.concatenate([[0.0], np.geomspace(1e-6, 300.0, 200)])
    for kind in (MR.MATERN32, MR.MATERN52):
        for ell in (0.5, 5.0, 80.0):
            (k, dk), (kl, dkl) = MR.unit_kernel(kind, d, ell), MR.unit_kernel(kind, d, ell, LD)
            a = MR.scaled_distance(kind, d, ell)
            on = a < 700.0        # (beyond, exp(-a) is subnormal in float64 and the plain product multiplies its rounding error)
            assert np.all(np.abs(k - kl)[on] <= ((16 + 4 * a) * 2.0 ** -53 * kl)[on])
            assert np.all(np.abs(dk - dkl)[on] <= ((16 + 4 * a) * 2.0 ** -53 * dkl)[on])
            assert k[0] == 1.0 and dk[0] == 0.0


@pytest.mark.parametrize("kind", [MR.MATERN32, MR.MATERN52])
def test_host_derivatives_vs_central_differences_of_the_long_double_kernel(kind):
    """compute_dKt("ell") and ("sigma2") on a non-uniform grid with repeated distances, against 4th-order central differences of
    the long-double kernel (step 1e-3 ell: truncation ~ h^4 / 30 of a derivative of order one, 3e-14; rounding 1e-19 / h)."""
    rs = np.random.RandomState(31 + kind)
    t = np.sort(np.concatenate([[0.0, 0.0, 2.5], np.cumsum(rs.uniform(0.2, 1.7, 34))]))[:, None]
    np.random.seed(0)
    tc = _classes()[kind](np.arange(37.0)[:, None])         # (the constructor's priors want distinct times)
    tc.t = t
    for ell, s2 in ((0.8, 0.7), (6.0, 1.3), (45.0, 2e-3)):
        tc.params["ell"]["value"], tc.params["sigma2"]["value"] = ell, s2
        h = LD(1e-3) * LD(ell)
        at = lambda k: MR.gram(kind, t, t, LD(ell) + k * h, s2, LD)
        fd = (8 * (at(1) - at(-1)) - (at(2) - at(-2))) / (12 * h)
        got = tc.compute_dKt("ell")
        err = float(np.max(np.abs(got.astype(LD) - fd)) / np.max(np.abs(fd)))
        hs = LD(0.25) * LD(s2)
        fds = (MR.gram(kind, t, t, ell, LD(s2) + hs, LD) - MR.gram(kind, t, t, ell, LD(s2) - hs, LD)) / (2 * hs)
        errs = float(np.max(np.abs(tc.compute_dKt("sigma2").astype(LD) - fds)))
        print("host dKt kind %d ell %g: d/d ell %.2e of the largest entry, d/d sigma2 %.2e absolute" % (kind, ell, err, errs))
        assert err < 1e-11 and errs < 1e-13
        assert np.array_equal(got, MR.dgram(kind, t, ell, s2, "ell")) or np.allclose(got, MR.dgram(kind, t, ell, s2, "ell"), rtol=1e-13, atol=0)
    with pytest.raises(KeyError):
        tc.compute_dKt("alpha")


def test_an_unknown_kind_raises():
    from gpcsd_amd import covariances as CV

    class Odd(CV._StationaryTemporalCov):
        kind = 7
    np.random.seed(0)
    with pytest.raises(ValueError):
        Odd(np.arange(12.0)[:, None]).compute_dKt("ell")
    for bad in (MR.HOST, 5):
        with pytest.raises(ValueError):
            MR.unit_kernel(bad, np.zeros(3), 1.0)
        with pytest.raises(ValueError):
            MR.temporal_gram(bad, np.zeros(3), np.zeros(3), 1.0, 1.0)


def test_a_model_of_the_new_classes_is_a_device_kind_model():
    from gpcsd_amd import _hip
    m = MR.model_for(MR.CASES[1])
    assert [k for k, _, _ in m._temporal_triplets()] == [_hip.KIND_MATERN52, _hip.KIND_MATERN32]
    assert m._uses_host_kt() is False and m._batch_can_evaluate() is True and m._vector_glue_applies() is True
    s = str(m)
    assert "GPCSDTemporalCovMatern52" in s and "Matern-5/2" in s and "Matern-3/2" in s
    # a subclass outside the device kinds is a host kernel, as before
    m.temporal_cov_list[0].kind = 7
    assert m._uses_host_kt() is True


def test_the_world_swaps_only_the_kinds_and_is_undone(monkeypatch):
    import helpers
    import test_predict_at as PA
    from oracle import gpcsd_oracle as O
    real = O.temporal_gram
    with monkeypatch.context() as mp:
        MR.world(mp)
        for name in MR.CASES:
            c, g, geom, hp, lfp = PA.load_model_case(name)
            c0, g0, geom0, hp0, lfp0 = helpers.load_model_case(name[len(MR.PREFIX):])
            assert [k for k, _, _ in hp["temporal"]] == list(MR.SWAPS[name[len(MR.PREFIX):]])
            assert [tc[1:] for tc in hp["temporal"]] == [tc[1:] for tc in hp0["temporal"]] and np.array_equal(lfp, lfp0)
            assert {k: v for k, v in hp.items() if k != "temporal"}.keys() == {k: v for k, v in hp0.items() if k != "temporal"}.keys()
        t = np.arange(5.0)
        assert np.array_equal(O.temporal_gram(O.SE, t, t, 2.0, 0.5), real(O.SE, t, t, 2.0, 0.5))
        assert O.temporal_gram(MR.MATERN32, t, t, 2.0, 0.5)[0, 0] == 0.5
    assert O.temporal_gram is real and PA.load_model_case is helpers.load_model_case
