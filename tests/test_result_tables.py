"""What a posterior call produces is written once, in its `*_outputs` table of gpcsd_amd/_hip.py, and read by its host form
(`host_outputs`) and its resident form (`device_views`).  On the CPU: the two readings of every table agree in keys and shapes, and
which host arrays are page-locked is pinned to a literal list, so that an edit of a table cannot silently change copy behaviour.
On the GPU: for each of the eight methods the resident form returns the keys, shapes and bits of the host form."""
import itertools

import numpy as np
import pytest

from gpcsd_amd import _hip

NZ, NTSTAR, R, C, J, NX, NT, NFOLDS, NSAMPLES, NG = 3, 4, 5, 2, 3, 17, 37, 4, 2, 7

# key -> page-locked on the host, per call: today's choices
PINNED = {
    "predict": {"csd": True, "csd_list": True, "lfp": True, "lfp_list": True},
    "predict_var": {"csd": True, "csd_list": True, "lfp": True, "lfp_list": True},
    "predict_functionals": {"%s_%s%s" % (q, kind, suf): False
                            for q in ("csd", "lfp") for kind in ("mean", "cov", "prior") for suf in ("", "_list")},
    "loo": {"var": False, "lpd": False, "sse": False, "mean": True},
    "cv_electrodes": {"var": False, "lpd": False, "sse": False, "mean": True},
    "trial_scores": {"scores": False},
    "sample_posterior": {"csd": True, "lfp": True},
    "sample_features": {"feat_csd": True, "feat_lfp": True, "csd": True, "lfp": True},
    "analytic": {"phase": True, "amp": True, "u_re": True, "u_im": True},
    "power_spectrum": {"psd": False, "power": True, "re": True, "im": True},
    "plv": {"c_re": False, "c_im": False, "plv": False},
    "cross_spectrum": {"s_re": False, "s_im": False, "coh": False},
}


def _tables():
    """(call, request, table) for every table and every setting of what a request may leave out."""
    draws = (NZ, NTSTAR, R, NSAMPLES)
    for code, flag in itertools.product((_hip.PRED_CSD, _hip.PRED_LFP, _hip.PRED_BOTH), (True, False)):
        yield "predict", (code, flag), _hip.predict_outputs(code, (NZ, NTSTAR, R), C, want_lists=flag)
        yield "sample_features", (code, flag), _hip.sample_features_outputs(code, draws, J, keep_draws=flag)
    for code in (_hip.PRED_CSD, _hip.PRED_LFP, _hip.PRED_BOTH):
        yield "predict_var", (code,), _hip.predict_var_outputs(code, (NZ, NTSTAR), C)
        yield "predict_functionals", (code,), _hip.predict_functionals_outputs(code, J, R, C)
        yield "sample_posterior", (code,), _hip.sample_posterior_outputs(code, draws)
    for flag in (True, False):
        yield "loo", (flag,), _hip.loo_outputs((NX, NT, R), want_mean=flag)
        yield "cv_electrodes", (flag,), _hip.cv_electrodes_outputs((NX, NT, R), NFOLDS, want_mean=flag)
    yield "trial_scores", (), _hip.trial_scores_outputs(R, NG)
    for mask in range(16):
        yield "analytic", (mask,), _hip._flag_table(_hip.Context.ANALYTIC_OUTPUTS, mask, (NZ, NTSTAR, R))
    for mask in range(8):
        yield "power_spectrum", (mask,), _hip.Context._spectrum_table(mask, NZ, NTSTAR, R, NSAMPLES)
        yield "plv", (mask,), _hip._flag_table(_hip.Context.PLV_OUTPUTS, mask, (NSAMPLES, NTSTAR, NZ, NZ), pinned=False)
        yield "cross_spectrum", (mask,), _hip._flag_table(_hip.Context.XSPEC_OUTPUTS, mask, (NSAMPLES, NTSTAR, NZ, NZ), pinned=False)


class _Recorder:
    """Stands in for the context (device_array) and for the page-locked pool (empty): records what it is asked for."""

    def __init__(self):
        self.asked = []

    def device_array(self, name, shape):
        self.asked.append(name)
        return (name, tuple(shape))

    def empty(self, shape):
        self.asked.append(tuple(shape))
        return np.empty(shape)


def test_host_arrays_and_views_of_every_table_agree(monkeypatch):
    for call, request, table in _tables():
        tag = (call, request)
        pool, ctx = _Recorder(), _Recorder()
        monkeypatch.setattr(_hip, "pinned_pool", pool)
        host, views = _hip.host_outputs(table), _hip.device_views(ctx, table)
        assert list(host) == list(views) == [o.key for o in table] and sorted(host) == sorted(PINNED[call]), tag
        assert len(set(o.buffer for o in table)) == len(table), tag                      # distinct buffers
        for o in table:
            if o.shape is None:
                assert host[o.key] is None and views[o.key] is None, (tag, o.key)
                continue
            assert isinstance(host[o.key], np.ndarray) and host[o.key].dtype == np.float64, (tag, o.key)
            assert host[o.key].shape == views[o.key][1] == o.shape and views[o.key][0] == o.buffer, (tag, o.key)
        assert ctx.asked == [o.buffer for o in table if o.shape is not None], tag
        # page-locked or not: as the literal list says, and the pool is asked for exactly the page-locked ones
        assert {o.key: o.pinned for o in table} == PINNED[call], tag
        assert pool.asked == [o.shape for o in table if o.shape is not None and o.pinned], tag


def test_what_a_request_leaves_out_is_absent():
    present = lambda table: sorted(o.key for o in table if o.shape is not None)
    for call, request, table in _tables():
        if call in ("predict", "predict_var", "predict_functionals", "sample_posterior", "sample_features"):
            code = request[0]
            quantities = [q for q, bit in (("csd", _hip.PRED_CSD), ("lfp", _hip.PRED_LFP)) if code & bit]
            keys = [o.key for o in table if o.shape is not None]
            assert keys and all(any(q in k.split("_") for q in quantities) for k in keys), (call, request, keys)
            assert sorted(set(q for k in keys for q in ("csd", "lfp") if q in k.split("_"))) == quantities, (call, request, keys)
    assert present(_hip.predict_outputs(_hip.PRED_CSD, (NZ, NTSTAR, R), C, want_lists=False)) == ["csd"]
    assert present(_hip.predict_outputs(_hip.PRED_BOTH, (NZ, NTSTAR, R), C)) == ["csd", "csd_list", "lfp", "lfp_list"]
    assert present(_hip.loo_outputs((NX, NT, R), want_mean=False)) == ["lpd", "sse", "var"]
    assert present(_hip.cv_electrodes_outputs((NX, NT, R), NFOLDS, want_mean=False)) == ["lpd", "sse", "var"]
    draws = (NZ, NTSTAR, R, NSAMPLES)
    assert present(_hip.sample_features_outputs(_hip.PRED_LFP, draws, J, keep_draws=False)) == ["feat_lfp"]
    assert present(_hip.sample_features_outputs(_hip.PRED_LFP, draws, J, keep_draws=True)) == ["feat_lfp", "lfp"]
    assert len(present(_hip.predict_functionals_outputs(_hip.PRED_CSD, J, R, C))) == 6


def test_shapes_and_buffer_names_of_the_tables():
    shapes = lambda table: {o.key: o.shape for o in table}
    names = lambda table: {o.key: o.buffer for o in table}
    for call, request, table in _tables():
        s = shapes(table)
        for key in s:                                                                    # a list is its sum with a leading C
            if key.endswith("_list") and s[key] is not None:
                assert s[key] == (C,) + s[key[:-5]], (call, request, key)
    both = _hip.PRED_BOTH
    assert shapes(_hip.predict_outputs(both, (NZ, NTSTAR, R), C))["lfp"] == (NZ, NTSTAR, R)
    assert names(_hip.predict_outputs(both, (NZ, NTSTAR, R), C)) == {"csd": "pred_out_csd", "csd_list": "pred_out_csd_list",
                                                                      "lfp": "pred_out_lfp", "lfp_list": "pred_out_lfp_list"}
    assert shapes(_hip.predict_var_outputs(both, (NZ, NTSTAR), C))["csd"] == (NZ, NTSTAR)
    assert names(_hip.predict_var_outputs(both, (NZ, NTSTAR), C))["lfp_list"] == "pred_var_lfp_list"
    fun = _hip.predict_functionals_outputs(both, J, R, C)
    assert [shapes(fun)[k] for k in ("csd_mean", "csd_cov", "lfp_prior", "lfp_cov_list")] == [(J, R), (J, J), (J, J), (C, J, J)]
    assert [names(fun)[k] for k in ("csd_mean", "csd_cov_list", "lfp_prior")] == ["fun_mean_csd", "fun_cov_csd_list", "fun_prior_lfp"]
    assert shapes(_hip.loo_outputs((NX, NT, R))) == {"var": (NX, NT), "lpd": (NX, R), "sse": (NX, R), "mean": (NX, NT, R)}
    assert names(_hip.loo_outputs((NX, NT, R))) == {"var": "loo_var", "lpd": "loo_lpd", "sse": "loo_sse", "mean": "loo_mean"}
    cv = _hip.cv_electrodes_outputs((NX, NT, R), NFOLDS)
    assert shapes(cv) == {"var": (NX, NT), "lpd": (NFOLDS, R), "sse": (NX, R), "mean": (NX, NT, R)}
    assert names(cv) == {"var": "cv_var", "lpd": "cv_lpd", "sse": "cv_sse", "mean": "cv_mean"}
    assert _hip.trial_scores_outputs(R, NG) == (_hip.Output("scores", "trial_scores", (R, NG), False),)
    draws = (NZ, NTSTAR, R, NSAMPLES)
    assert shapes(_hip.sample_posterior_outputs(both, draws)) == {"csd": draws, "lfp": draws}
    feats = _hip.sample_features_outputs(both, draws, J, keep_draws=True)
    assert shapes(feats) == {"feat_csd": (J, _hip.NFEAT, R, NSAMPLES), "feat_lfp": (J, _hip.NFEAT, R, NSAMPLES), "csd": draws, "lfp": draws}
    assert names(feats) == {"feat_csd": "feat_csd", "feat_lfp": "feat_lfp", "csd": "post_sample_csd", "lfp": "post_sample_lfp"}


# ------------------------------------------------------------------------------------------------ GPU: one method, two forms
@pytest.mark.gpu
def test_the_resident_form_returns_the_keys_shapes_and_bits_of_the_host_form():
    import test_posterior_family as PF
    import test_predict_at as PA
    m = PA._model(PF.NAME)
    ctx = m._sync_device()
    nx, nt, ntrials = np.shape(m.lfp)
    hp, _k0 = m._hparams(0.0)                                            # the model of the predictions: no jitter
    hpj, _k1 = m._hparams(m.JITTER)                                      # the model of loglik: loo, cv_electrodes, trial_scores
    z, ts = PF._request(3, 4)
    both, W = _hip.PRED_BOTH, PF._boxes(z, ts)
    labels = np.zeros((3, 4), dtype=np.int32)
    labels[:2, :2], labels[1:, 2:] = 1, 2                                # two regions and some background
    ptr, idx = np.arange(nx + 1, dtype=np.int32), np.arange(nx, dtype=np.int32)          # 17 folds of one electrode
    ng = 1 + m.dim + 2 * len(m.temporal_cov_list) + 1
    calls = {"predict_var": lambda **kw: ctx.predict_var(hp, z, ts, both, **kw),
             "predict_functionals": lambda **kw: ctx.predict_functionals(hp, z, ts, W, both, ntrials, **kw),
             "loo": lambda **kw: ctx.loo(hpj, (nx, nt, ntrials), **kw),
             "cv_electrodes": lambda **kw: ctx.cv_electrodes(hpj, (nx, nt, ntrials), ptr, idx, **kw),
             "trial_scores": lambda **kw: {"scores": ctx.trial_scores(hpj, ntrials, ng, **kw)},
             "predict_masked": lambda **kw: ctx.predict_masked(hp, np.ones((nx, nt), dtype=bool), z, ts, both, (3, 4, ntrials), **kw),
             "sample_posterior": lambda **kw: ctx.sample_posterior(hp, z, ts, both, 2, 1, ntrials, **kw),
             "sample_features": lambda **kw: ctx.sample_features(hp, z, ts, both, 2, 1, ntrials, labels, 2, keep_draws=True, **kw)}
    expected = {"predict_var": 4, "predict_functionals": 12, "loo": 4, "cv_electrodes": 5, "trial_scores": 1, "predict_masked": 4,
                "sample_posterior": 2, "sample_features": 4}
    for name, call in calls.items():
        host = call()
        res = call(resident=True)
        assert sorted(res) == sorted(host) and len(host) == expected[name], (name, sorted(res), sorted(host))
        for k, h in host.items():
            assert h is not None, (name, k)                              # type "both", lists, mean and draws: every output exists
            if k == "status":
                assert isinstance(res[k], np.ndarray) and res[k].dtype == h.dtype == np.int32, name
                assert res[k].shape == h.shape == (nx,) and not h.any() and np.array_equal(res[k], h), name
                continue
            assert isinstance(res[k], _hip.DeviceArray) and isinstance(h, np.ndarray), (name, k)
            assert res[k].shape == h.shape and res[k].numpy().tobytes() == h.tobytes(), (name, k)
