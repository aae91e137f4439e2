"""Shared machinery of GPCSD1D / GPCSD2D: hyper-parameter (un)packing, device residency, loglik / predict /
sample_prior on the GPU, and the multi-restart MAP fit.

Behavioural contract (reference: src/gpcsd/gpcsd1d.py, src/gpcsd/gpcsd2d.py):
  * hyper-parameters live in mutable dicts (`self.R`, `self.sig2n`, `spatial_cov.params`, `temporal_cov_list[i].params`)
    and are re-read at every call;
  * loglik adds JITTER*I to Ks, predict does not; neither adds the -N/2 log(2 pi) constant;
  * fit optimises -(loglik + log-prior) over log-parameters with L-BFGS-B from prior-sampled restarts and keeps the
    best finite optimum; the reference's autograd gradient is replaced by an analytic gradient computed on the GPU
    (scalar sig2n or a per-electrode list); restarts can run concurrently (`workers`) and be sharded over ranks;
  * predict(z, t, type) fills csd_pred / csd_pred_list / lfp_pred / lfp_pred_list / t_pred / x_pred.
"""
import numpy as np
import scipy.optimize
from tqdm import tqdm

from . import _hip
from .covariances import GPCSDTemporalCov

# kernels without a reference class of their own: __str__ prints their form beside the class name
_KIND_FORMS = {_hip.KIND_MATERN32: "Matern-3/2, sigma2 (1 + a) exp(-a), a = sqrt(3) |t-t'| / ell",
               _hip.KIND_MATERN52: "Matern-5/2, sigma2 (1 + a + a^2/3) exp(-a), a = sqrt(5) |t-t'| / ell"}


def _same_array(a, b):
    return a is b or (np.shape(a) == np.shape(b) and np.array_equal(a, b))


class GPCSDModel:
    """Base of GPCSD1D / GPCSD2D.  Subclasses set `dim`, `JITTER`, `_spatial_names` and build the covariances."""

    dim = None
    JITTER = None
    _spatial_names = ()          # names of the spatial length-scale params in spatial_cov.params

    # ------------------------------------------------------------------ device residency
    def _context(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is None:
            ctx = _hip.Context(getattr(self, "_device", None))
            self._ctx = ctx
            self._resident = {}
        return ctx

    def set_device(self, device):
        """Pin this model to a GPU ordinal (default: $LOCAL_RANK or 0).  Must be called before the first evaluation."""
        if getattr(self, "_ctx", None) is not None:
            raise RuntimeError("device already initialised for this model")
        self._device = int(device)

    def shard_trials(self, sharding):
        """Evaluate only this rank's contiguous block of trials and combine partial sums across ranks
        (gpcsd_amd.dist.TrialSharding).  `self.lfp` keeps the full array; predictions are returned for the local block
        unless `sharding.gather_predictions` is set."""
        self._sharding = sharding
        self._resident = {} if getattr(self, "_ctx", None) is not None else getattr(self, "_resident", {})

    def invalidate(self):
        """Force re-upload of lfp / coordinates at the next call (use after editing arrays in place)."""
        self._resident = {}

    def _local_lfp(self):
        lfp = np.atleast_3d(self.lfp)
        sh = getattr(self, "_sharding", None)
        if sh is None:
            return lfp
        return lfp[:, :, sh.local_slice(lfp.shape[2])]

    # "fp32 kernel build + fp64 factor" (BASELINE cfg5): set `model.gram_precision = 32` to evaluate the Gram builders of
    # this model's fused calls in single precision; everything after the Gram matrices stays fp64.  Default 64 = the reference.
    gram_precision = 64

    def _sync_device(self, need_lfp=True):
        ctx = self._context()
        res = self._resident
        sc = self.spatial_cov
        if res.get("gram_precision") != self.gram_precision:
            ctx.set_gram_precision(self.gram_precision)
            res["gram_precision"] = self.gram_precision
        # time grid: the reference evaluates each temporal covariance on its own `t`; they must agree
        t = self.temporal_cov_list[0].t
        for tc in self.temporal_cov_list[1:]:
            if not _same_array(tc.t, t):
                raise ValueError("temporal covariance components hold different time grids")
        if "t" not in res or not _same_array(res["t"], t):
            ctx.set_time(t)
            res["t"] = np.array(t, dtype=np.float64, copy=True)
        if self.dim == 1:
            key = (np.asarray(sc.x, dtype=np.float64).reshape(-1), np.asarray(sc.gl_x), np.asarray(sc.gl_w))
        else:
            key = (np.asarray(sc.x, dtype=np.float64), np.asarray(sc.gl_x1), np.asarray(sc.gl_w1), np.asarray(sc.gl_x2),
                   np.asarray(sc.gl_w2))
        old = res.get("geo")
        if old is None or len(old) != len(key) or not all(_same_array(a, b) for a, b in zip(old, key)):
            if self.dim == 1:
                ctx.set_geometry_1d(*key)
            else:
                ctx.set_geometry_2d(*key)
            res["geo"] = tuple(np.array(k, copy=True) for k in key)
        if need_lfp:
            lfp = self.lfp
            if np.ndim(lfp) != 3:
                raise ValueError("lfp must have shape (n_spatial, n_time, n_trials)")
            sh = getattr(self, "_sharding", None)
            ident = (id(lfp), lfp.__array_interface__["data"][0], lfp.shape, lfp.strides,
                     None if sh is None else (sh.rank, sh.world_size))
            if res.get("lfp") != ident:
                ctx.set_lfp(self._local_lfp())
                res["lfp"] = ident
        return ctx

    # ------------------------------------------------------------------ hyper-parameters
    def _temporal_triplets(self):
        """[(kind, ell, sigma2)] per temporal component.  The kinds of _hip.DEVICE_KINDS (SE, Matern-1/2, -3/2, -5/2) are
        evaluated by the library's own Gram builders; any other object with a `compute_Kt` method (the reference accepts
        those: covariances.py:235-238, gpcsd1d.py:118-120) is marked KIND_HOST and its Gram matrices are evaluated on the host by that method (see `_hparams`)."""
        out = []
        for tc in self.temporal_cov_list:
            kind = getattr(tc, "kind", None)
            if isinstance(tc, GPCSDTemporalCov) and kind in _hip.DEVICE_KINDS:
                out.append((kind, tc.params["ell"]["value"], tc.params["sigma2"]["value"]))
            elif callable(getattr(tc, "compute_Kt", None)):
                out.append((_hip.KIND_HOST, 0.0, 0.0))
            else:
                raise TypeError("temporal covariance %r has no compute_Kt method" % type(tc).__name__)
        return out

    def _uses_host_kt(self):
        return any(k == _hip.KIND_HOST for k, _, _ in self._temporal_triplets())

    def _host_kt_is_differentiable(self):
        """Every temporal component of a model with user-defined covariances offers compute_dKt(name)."""
        return all(callable(getattr(tc, "compute_dKt", None)) for tc in self.temporal_cov_list)

    def _hparams(self, jitter, tstar=None, want_dkt=False):
        ell_s = [self.spatial_cov.params[n]["value"] for n in self._spatial_names]
        eps = getattr(self, "eps", 0.0)
        ctx = self._context()
        trip = self._temporal_triplets()
        if any(k == _hip.KIND_HOST for k, _, _ in trip):
            # user-defined temporal covariance: its Gram matrices come from its own compute_Kt (host NumPy), everything after
            # them -- eigensolver, projections, predict chain -- still runs on the GPU
            Kt = sum(np.asarray(tc.compute_Kt(), dtype=np.float64) for tc in self.temporal_cov_list)
            cross = None
            if tstar is not None:
                cross = np.stack([np.asarray(tc.compute_Kt(tstar), dtype=np.float64) for tc in self.temporal_cov_list])
            ctx.set_host_temporal_gram(Kt, cross)
            if want_dkt:                             # d Kt / d (ell_c, sigma2_c) per component, from the objects themselves
                ctx.set_host_temporal_dgram(np.stack([np.asarray(tc.compute_dKt(nm), dtype=np.float64)
                                                      for tc in self.temporal_cov_list for nm in ("ell", "sigma2")]))
            self._resident["host_kt"] = True
        elif self._resident.get("host_kt"):
            ctx.set_host_temporal_gram(None)
            self._resident["host_kt"] = False
        hp, keep = ctx.make_hparams(self.R["value"], eps, ell_s, trip, self.sig2n["value"], jitter)
        return hp, keep

    def _sig2n_is_scalar(self):
        return np.isscalar(self.sig2n["value"]) or np.ndim(self.sig2n["value"]) == 0

    def extract_model_params(self):
        p = {"R": self.R["value"]}
        if self.dim == 2:
            p["eps"] = self.eps
        p["sig2n"] = self.sig2n["value"]
        if self.dim == 1:
            p["spatial_ell"] = self.spatial_cov.params["ell"]["value"]
        else:
            p["spatial_ell1"] = self.spatial_cov.params["ell1"]["value"]
            p["spatial_ell2"] = self.spatial_cov.params["ell2"]["value"]
        p["temporal_ell_list"] = [tc.params["ell"]["value"] for tc in self.temporal_cov_list]
        p["temporal_sigma2_list"] = [tc.params["sigma2"]["value"] for tc in self.temporal_cov_list]
        return p

    def restore_model_params(self, params):
        self.R["value"] = params["R"]
        if self.dim == 2:
            self.eps = params["eps"]
        self.sig2n["value"] = params["sig2n"]
        if self.dim == 1:
            self.spatial_cov.params["ell"]["value"] = params["spatial_ell"]
        else:
            self.spatial_cov.params["ell1"]["value"] = params["spatial_ell1"]
            self.spatial_cov.params["ell2"]["value"] = params["spatial_ell2"]
        if len(self.temporal_cov_list) != len(params["temporal_ell_list"]):
            print("different number of temporal covariance functions! stopping.")
            return
        for tc, ell, s2 in zip(self.temporal_cov_list, params["temporal_ell_list"], params["temporal_sigma2_list"]):
            tc.params["ell"]["value"] = ell
            tc.params["sigma2"]["value"] = s2

    def _describe(self, header_lines):
        s = "GPCSD1D object\n"          # (the reference prints this header for both classes)
        s += "LFP shape: (%d, %d, %d)\n" % tuple(np.shape(self.lfp)[:3])
        for line in header_lines:
            s += line
        s += "R parameter prior: %s\n" % str(self.R["prior"])
        s += "R parameter value %0.4g\n" % self.R["value"]
        return s

    def _describe_temporal(self):
        s = ""
        for i, tc in enumerate(self.temporal_cov_list):
            s += "Temporal covariance %d class name: %s\n" % (i + 1, type(tc).__name__)
            if getattr(tc, "kind", None) in _KIND_FORMS:
                s += "Temporal covariance %d kernel: %s\n" % (i + 1, _KIND_FORMS[tc.kind])
            s += "Temporal covariance %d ell prior: %s\n" % (i + 1, str(tc.params["ell"]["prior"]))
            s += "Temporal covariance %d ell value %0.4g\n" % (i + 1, tc.params["ell"]["value"])
            s += "Temporal covariance %d sigma2 prior: %s\n" % (i + 1, str(tc.params["sigma2"]["prior"]))
            s += "Temporal covariance %d sigma2 value %0.4g\n" % (i + 1, tc.params["sigma2"]["value"])
        return s

    # ------------------------------------------------------------------ likelihood
    def loglik(self):
        """Log marginal likelihood (up to the 2*pi constant) of all trials under the current hyper-parameters."""
        ctx = self._sync_device()
        hp, _keep = self._hparams(self.JITTER)
        sumlog, quad = ctx.loglik_parts(hp)
        sh = getattr(self, "_sharding", None)
        if sh is not None:
            quad = float(sh.allreduce_sum(np.array([quad]))[0])
        ntrials = np.shape(self.lfp)[2]
        return np.float64(-0.5 * ntrials * sumlog - 0.5 * quad)

    def _loglik_and_grad_natural(self):
        """(loglik, d loglik / d[R, ell_s.., (ell_t, sigma2_t).., sig2n or sig2n_0..sig2n_{nx-1}]) on the GPU."""
        host = self._uses_host_kt()
        if host and not self._host_kt_is_differentiable():
            raise NotImplementedError("no analytic gradient for user-defined temporal covariances without compute_dKt(name)")
        ctx = self._sync_device()
        hp, _keep = self._hparams(self.JITTER, want_dkt=host)
        nsig = 1 if self._sig2n_is_scalar() else len(self.sig2n["value"])
        ng = 1 + self.dim + 2 * len(self.temporal_cov_list) + nsig
        sumlog, quad, g = ctx.loglik_grad(hp, ng)
        r_local = self._local_lfp().shape[2]
        ll = -0.5 * r_local * sumlog - 0.5 * quad
        sh = getattr(self, "_sharding", None)
        if sh is not None:                       # both pieces are additive over shards
            red = sh.allreduce_sum(np.concatenate([[ll], g]))
            ll, g = float(red[0]), red[1:]
        return ll, g

    def _eval_batch_local(self, hps):
        """(loglik of the LOCAL trials [B], natural gradient [B, ng], status [B]) for a list of hyper-parameter structs: one
        shared chain of launches (gpcsd_loglik_grad_batch)."""
        ctx = self._sync_device()
        nsig = 1 if self._sig2n_is_scalar() else len(self.sig2n["value"])
        ng = 1 + self.dim + 2 * len(self.temporal_cov_list) + nsig
        sumlog, quad, g, st = ctx.loglik_grad_batch(hps, ng)
        r_local = self._local_lfp().shape[2]
        return -0.5 * r_local * sumlog - 0.5 * quad, g, st

    def _eval_batch_reduced(self, hps):
        """(loglik [B], natural gradient [B, ng], failed [B]) of a batch over ALL trials: the local evaluation, and under trial
        sharding ONE all-reduce for the whole batch.  Slot b must mean the same hyper-parameter set on every rank (the
        lock-step drivers hand their batches over sorted by restart index for exactly this reason)."""
        ll, g, st = self._eval_batch_local(hps)
        ll, g, st = np.asarray(ll, dtype=np.float64), np.asarray(g, dtype=np.float64), np.asarray(st)
        B, ng = g.shape
        sh = getattr(self, "_sharding", None)
        if sh is not None:                       # both pieces are additive over shards; a set that failed anywhere fails everywhere
            red = sh.allreduce_sum(np.concatenate([ll, g.ravel(), (st != 0).astype(np.float64)]))
            ll, g, st = red[:B], red[B:B + B * ng].reshape(B, ng), red[B + B * ng:]
        return ll, g, st != 0

    @staticmethod
    def _batch_failure(b):
        return np.linalg.LinAlgError("numerical failure in the eigensolver (hyper-parameter set %d of the batch)" % b)

    def _loglik_and_grad_natural_batch(self, hps):
        """[(loglik, gradient) or LinAlgError] for a batch of hyper-parameter structs."""
        ll, g, failed = self._eval_batch_reduced(hps)
        return [self._batch_failure(b) if failed[b] else (float(ll[b]), np.array(g[b])) for b in range(len(ll))]

    # ------------------------------------------------------------------ fit
    def _param_slots(self):
        """[(getter, setter, prior, (min, max), scale)] in the reference's log-parameter order."""
        slots = []

        def dict_slot(d, scale):
            return (lambda: d["value"], lambda v: d.__setitem__("value", v), d["prior"], (d["min"], d["max"]), scale)
        slots.append(dict_slot(self.R, 100.0))
        for n in self._spatial_names:
            slots.append(dict_slot(self.spatial_cov.params[n], 100.0))
        for tc in self.temporal_cov_list:
            slots.append(dict_slot(tc.params["ell"], 1.0))
            slots.append(dict_slot(tc.params["sigma2"], 1.0))
        return slots

    def _bounds(self):
        b = []
        with np.errstate(divide="ignore"):
            for _, _, _, (lo, hi), scale in self._param_slots():
                b.append((np.log(lo / scale), np.log(hi / scale)))
            if self._sig2n_is_scalar():
                b.append((np.log(self.sig2n["min"]), np.log(self.sig2n["max"])))
            else:
                for lo, hi in zip(self.sig2n["min"], self.sig2n["max"]):
                    b.append((np.log(lo), np.log(hi)))
        return b

    def _set_from_tparams(self, tparams, fix_R):
        slots = self._param_slots()
        for i, (_, setter, _, _, scale) in enumerate(slots):
            if i == 0 and fix_R:
                continue
            setter(np.exp(tparams[i]) * scale)
        p = len(slots)
        if self._sig2n_is_scalar():
            self.sig2n["value"] = np.exp(tparams[p])
        else:
            self.sig2n["value"] = np.exp(tparams[p:])

    def _log_prior(self):
        lp = 0.0
        for getter, _, prior, _, _ in self._param_slots():
            lp = lp + prior.lpdf(getter())
        if self._sig2n_is_scalar():
            lp = lp + self.sig2n["prior"].lpdf(self.sig2n["value"])
        else:
            for pr, v in zip(self.sig2n["prior"], self.sig2n["value"]):
                lp = lp + pr.lpdf(v)
        return lp

    def _safe_loglik(self):
        return self.loglik()

    def _objective(self, tparams, fix_R):
        """-(loglik + log prior) at log-parameters `tparams` (writes them into the param dicts, as the reference does)."""
        with np.errstate(all="ignore"):          # the reference runs under np.seterr(all='ignore') (gpcsd1d.py:7)
            self._set_from_tparams(tparams, fix_R)
            lp = self._log_prior()
            return -1.0 * (self._safe_loglik() + lp)

    def _objective_grad(self, tparams, fix_R, fd_step=1e-6):
        """Gradient of `_objective` w.r.t. the log-parameters (non-finite values are passed through to the optimiser
        silently, as under the reference's module-level `np.seterr(all='ignore')`, gpcsd1d.py:7)."""
        return self._objective_and_grad(tparams, fix_R, fd_step)[1]

    def _chain_rule(self, tparams, g_nat, fix_R):
        """d(-(loglik + log prior)) / d log-parameters from the natural-parameter gradient of loglik."""
        slots = self._param_slots()
        g = np.zeros_like(tparams)
        for i, (getter, _, prior, _, _) in enumerate(slots):
            v = getter()
            g[i] = -(g_nat[i] + prior.dlpdf(v)) * v          # d/dlog(v) = v d/dv
        p = len(slots)
        if self._sig2n_is_scalar():
            v = self.sig2n["value"]
            g[p] = -(g_nat[p] + self.sig2n["prior"].dlpdf(v)) * v
        else:                                                # per-electrode noise list (gpcsd1d.py:71-73)
            for k, (pr, v) in enumerate(zip(self.sig2n["prior"], self.sig2n["value"])):
                g[p + k] = -(g_nat[p + k] + pr.dlpdf(v)) * v
        if fix_R:
            g[0] = 0.0
        return g

    def _objective_and_grad(self, tparams, fix_R, fd_step=1e-6):
        """(objective, gradient) from ONE device evaluation: the front half (Gram builds + both eigendecompositions) is most
        of an evaluation, so the optimiser is driven with jac=True instead of separate fun / jac callbacks that would each
        run it.  A numerical failure raises LinAlgError, which ends the restart exactly as the reference's jac callback
        does (gpcsd1d.py:219, gpcsd2d.py:258)."""
        with np.errstate(all="ignore"):          # the reference runs under np.seterr(all='ignore') (gpcsd1d.py:7)
            tparams = np.asarray(tparams, dtype=np.float64)
            if getattr(self, "_use_analytic_grad", True) and (not self._uses_host_kt() or self._host_kt_is_differentiable()):
                if self._batch_can_evaluate() and self._vector_glue_applies():
                    # the batch of one: the same array expressions (and the same device code, gpcsd_loglik_grad is the B = 1 case
                    # of gpcsd_loglik_grad_batch), so a restart gets the same bits alone and in a lock-step batch
                    r = self._objective_and_grad_batch([(0, tparams)], fix_R)[0]
                    if isinstance(r, Exception):
                        raise r
                    return r
                self._set_from_tparams(tparams, fix_R)
                lp = self._log_prior()
                ll, g_nat = self._loglik_and_grad_natural()
                return -1.0 * (ll + lp), self._chain_rule(tparams, g_nat, fix_R)
            # finite differences of the objective (user-defined temporal covariances without compute_dKt; diagnostics)
            f = self._objective(tparams, fix_R)
            g = np.zeros_like(tparams)
            for i in range(tparams.size):
                if i == 0 and fix_R:
                    continue
                e = np.zeros_like(tparams)
                e[i] = fd_step
                g[i] = (self._objective(tparams + e, fix_R) - self._objective(tparams - e, fix_R)) / (2 * fd_step)
            self._set_from_tparams(tparams, fix_R)
            return f, g

    def _current_tparams(self):
        """The log-parameter vector of the current hyper-parameter state (inverse of `_set_from_tparams`)."""
        with np.errstate(divide="ignore"):
            tp = [np.log(getter() / scale) for getter, _, _, _, scale in self._param_slots()]
            tp.extend(np.log(np.atleast_1d(np.asarray(self.sig2n["value"], dtype=np.float64))))
        return np.array(tp, dtype=np.float64)

    def _sample_start(self, fix_R):
        slots = self._param_slots()
        tp = []
        for i, (getter, _, prior, _, scale) in enumerate(slots):
            if i == 0 and fix_R:
                tp.append(np.log(getter()) - np.log(scale))
            else:
                tp.append(np.log(prior.sample()) - np.log(scale))
        if self._sig2n_is_scalar():
            tp.append(np.log(self.sig2n["prior"].sample()))
        else:
            for pr in self.sig2n["prior"]:
                tp.append(np.log(pr.sample()))
        return np.array(tp)

    # ------------------------------------------------------------------ restarts: concurrency and sharding
    def shard_restarts(self, sharding):
        """Split the restarts of `fit` across ranks (restart k runs on rank k % world_size, every rank holds all trials);
        results are combined with two tiny all-reduces and every rank ends with the same best parameters
        (BASELINE cfg5).  `sharding`: gpcsd_amd.dist.TrialSharding (only rank / world_size / allreduce)."""
        self._restart_sharding = sharding

    def _clone_for_worker(self):
        """Independent hyper-parameter state on top of the SAME data arrays, with its own device context (= own HIP stream):
        restarts are latency-bound chains of small kernels, so several of them interleave well on one GPU."""
        import copy
        m = copy.copy(self)
        m.R = copy.deepcopy(self.R)
        m.sig2n = copy.deepcopy(self.sig2n)
        m.spatial_cov = copy.copy(self.spatial_cov)
        m.spatial_cov.params = copy.deepcopy(self.spatial_cov.params)
        m.temporal_cov_list = []
        for tc in self.temporal_cov_list:
            t2 = copy.copy(tc)
            t2.params = copy.deepcopy(tc.params)
            m.temporal_cov_list.append(t2)
        m._ctx = None
        m._resident = {}
        return m

    def _batch_can_evaluate(self):
        # (a subclass that brings its own objective is evaluated through it, one point at a time)
        cls = type(self)
        own = (cls._loglik_and_grad_natural_batch is not GPCSDModel._loglik_and_grad_natural_batch or
               cls._eval_batch_local is not GPCSDModel._eval_batch_local or
               (cls._objective_and_grad is GPCSDModel._objective_and_grad and
                cls._loglik_and_grad_natural is GPCSDModel._loglik_and_grad_natural))
        # (scalar noise or a per-electrode list: gpcsd_loglik_grad_batch takes either since round 5)
        return (own and getattr(self, "_use_analytic_grad", True) and not self._uses_host_kt())

    def _vector_glue_applies(self):
        """The hyper-parameters of a batch can be unpacked, their priors evaluated and the chain rule applied as array
        operations: the library's own temporal kernels, priors that offer lpdf_many / dlpdf_many (scalar noise or a
        per-electrode list of priors)."""
        if self._uses_host_kt():
            return False
        priors = [sl[2] for sl in self._param_slots()] + self._noise_priors()
        return all(callable(getattr(pr, "lpdf_many", None)) and callable(getattr(pr, "dlpdf_many", None)) for pr in priors)

    def _noise_priors(self):
        """the noise prior(s) as a list: one entry for scalar noise, nx for a per-electrode list (gpcsd1d.py:58-60)"""
        return [self.sig2n["prior"]] if self._sig2n_is_scalar() else list(self.sig2n["prior"])

    def _objective_and_grad_batch(self, items, fix_R):
        """{key: (objective, gradient) or exception} for [(key, tparams)]: the lock-step evaluation behind fit(batch=k).
        Runs single-threaded (every optimiser chain is waiting for its result), so walking the shared param dicts is safe.
        With the library's own priors and kernels the host side of a batch is array arithmetic (B x p): per tick of a 32-restart
        fit the Python loop below it cost about as much as a quarter of the device evaluation."""
        if not self._vector_glue_applies():
            return self._objective_and_grad_batch_loop(items, fix_R)
        with np.errstate(all="ignore"):
            slots = self._param_slots()
            p = len(slots)
            noise_priors = self._noise_priors()
            nsig = len(noise_priors)
            tps = np.stack([np.asarray(tp, dtype=np.float64) for _, tp in items])                 # (B, p + nsig)
            scales = np.array([sl[4] for sl in slots] + [1.0] * nsig)
            nat = np.exp(tps) * scales                                                            # natural values, slot order
            if fix_R:
                nat[:, 0] = slots[0][0]()
            priors = [sl[2] for sl in slots] + noise_priors
            lp = np.zeros(len(items))
            for i, pr in enumerate(priors):                                                       # same order as _log_prior
                lp = lp + pr.lpdf_many(nat[:, i])
            ns = len(self._spatial_names)
            C = len(self.temporal_cov_list)
            kinds = [k for k, _, _ in self._temporal_triplets()]
            tcols = nat[:, 1 + ns:1 + ns + 2 * C]
            hps = _hip.HParamsBatch(nat[:, 0], getattr(self, "eps", 0.0), nat[:, 1:1 + ns], kinds, tcols[:, 0::2], tcols[:, 1::2],
                                    nat[:, p] if self._sig2n_is_scalar() else nat[:, p:], self.JITTER)
            if getattr(self, "_resident", {}).get("host_kt"):
                self._context().set_host_temporal_gram(None)
                self._resident["host_kt"] = False
            ll, g_nat, failed = self._eval_batch_reduced(hps)
            dlp = np.stack([pr.dlpdf_many(nat[:, i]) for i, pr in enumerate(priors)], axis=1)
            G = -(g_nat + dlp) * nat                                                              # d/dlog(v) = v d/dv
            if fix_R:
                G[:, 0] = 0.0
            F = -1.0 * (ll + lp)
            out = {}
            for b, (key, _) in enumerate(items):
                out[key] = self._batch_failure(b) if failed[b] else (F[b], G[b])
            self._set_from_tparams(tps[-1], fix_R)       # the param dicts hold the last point evaluated, as after a scalar call
            return out

    def _objective_and_grad_batch_loop(self, items, fix_R):
        """The same, one hyper-parameter set at a time through the param dicts (user-defined priors without array methods)."""
        with np.errstate(all="ignore"):
            hps, keep, lps, tps = [], [], [], []
            for _, tp in items:
                tp = np.asarray(tp, dtype=np.float64)
                self._set_from_tparams(tp, fix_R)
                lps.append(self._log_prior())
                hp, k = self._hparams(self.JITTER)
                hps.append(hp)
                keep.append(k)
                tps.append(tp)
            res = self._loglik_and_grad_natural_batch(hps)
            out = {}
            for (key, _), tp, lp, r in zip(items, tps, lps, res):
                if isinstance(r, Exception):
                    out[key] = r
                    continue
                ll, g_nat = r
                self._set_from_tparams(tp, fix_R)            # the chain rule reads the values back from the dicts
                out[key] = (-1.0 * (ll + lp), self._chain_rule(tp, g_nat, fix_R))
            return out

    def _run_restart(self, tparams0, method, fix_R, options, bounds, evaluate=None):
        """One L-BFGS-B chain.  evaluate: callback x -> (objective, gradient) of a lock-step batch; default: this model."""
        fun = evaluate if evaluate is not None else (lambda tp: self._objective_and_grad(tp, fix_R))
        try:
            res = scipy.optimize.minimize(fun, tparams0, method=method, options=options, bounds=bounds, jac=True)
            return res.fun, res.x, res.message
        except (ValueError, np.linalg.LinAlgError) as e:
            print(e)
            if self.dim == 2:
                print("\nrestarting optimization...")
            return None

    # device memory a lock-step batch may take for its per-set arrays (five of nx * ntrials * nt doubles per set)
    FIT_BATCH_BYTES = 32 << 30
    # "auto" | "setulb" | "threads": who steps the restarts' optimisers between batched evaluations (see _fit)
    fit_driver = "auto"

    def _auto_batch(self, n):
        """Default lock-step width of fit(): all restarts of this rank, capped at 32 and by FIT_BATCH_BYTES."""
        lfp = self._local_lfp()
        per_set = 5 * 8 * lfp.shape[0] * lfp.shape[1] * lfp.shape[2]
        return int(max(1, min(n, 32, self.FIT_BATCH_BYTES // max(per_set, 1))))

    def _fit(self, n_restarts, method, fix_R, verbose, options, starts=None, workers=1, batch=None):
        bounds = self._bounds()
        # starting points are drawn up front, in the order the sequential loop of the reference consumes the RNG
        # (the optimiser itself draws nothing), so results do not depend on `workers` or on the number of ranks
        if starts is None:
            starts = [self._sample_start(fix_R) for _ in range(n_restarts)]
        starts = [np.asarray(s0, dtype=np.float64) for s0 in starts]
        rs = getattr(self, "_restart_sharding", None)
        # Ranks do not share a random stream: constructors and `_sample_start` draw from each process's own NumPy RNG.
        # Under trial sharding every rank must walk the SAME optimiser trajectory (the all-reduces inside the objective pair
        # up call by call), under restart sharding restart k must mean the same start everywhere: rank 0's current
        # hyper-parameters (fix_R reads R from them) and rank 0's starts are broadcast before anything is evaluated.
        sync = getattr(self, "_sharding", None) or rs
        if sync is not None and sync.world_size > 1:
            self._set_from_tparams(sync.broadcast(self._current_tparams(), src=0), False)
            if len(starts):
                flat = sync.broadcast(np.stack(starts).ravel(), src=0)
                starts = [row.copy() for row in flat.reshape(len(starts), -1)]
        self.fit_starts_ = [s0.copy() for s0 in starts]
        mine = [k for k in range(n_restarts) if rs is None or k % rs.world_size == rs.rank]
        results = {}
        workers = max(1, min(int(workers), len(mine)))
        # Replicas in one chain of launches are nearly free on the GPU and each restart gets the bits of a run of its own, so
        # by default all of this rank's restarts advance in lock-step
        if batch is None:
            batch = self._auto_batch(len(mine)) if (len(mine) > 1 and self._batch_can_evaluate()) else 1
        batch = max(1, min(int(batch), max(len(mine), 1)))
        if batch > 1 and self._batch_can_evaluate():
            # lock-step restarts: `batch` SciPy chains alive at a time, their evaluations served by ONE batched device call.
            # workers > 1: that many such groups side by side, each on its own context (= own streams and buffers).  A batched
            # evaluation is a latency-bound eigen phase (a few CUs) followed by a throughput-bound GEMM phase (all CUs); two
            # groups drift out of phase and one's eigen chains run under the other's GEMMs.  Not under trial sharding: the
            # groups' all-reduces would interleave differently on different ranks.
            from .lockstep import run_chains
            from . import lbfgsb_lockstep
            ngroups = 1 if getattr(self, "_sharding", None) is not None else max(1, min(workers, len(mine) // 2))
            parts = [mine[gi::ngroups] for gi in range(ngroups)]
            # Who steps the optimisers between the batched evaluations.  "setulb" (the default where this SciPy has it): ONE
            # driver steps every chain's L-BFGS-B state through SciPy's reverse-communication entry point -- the same compiled
            # optimiser scipy.optimize.minimize runs, the same trajectories bit for bit, without a thread, two condition-variable
            # hand-offs and a GIL switch per chain and evaluation.  "threads": unmodified minimize() calls on threads that
            # rendezvous in their objective callbacks (round 2; any `method`).
            driver = getattr(self, "fit_driver", "auto")
            use_setulb = (method == "L-BFGS-B" and driver in ("auto", "setulb") and lbfgsb_lockstep.available())
            if driver == "setulb" and not use_setulb:
                raise RuntimeError("fit_driver='setulb' needs method='L-BFGS-B' and scipy.optimize._lbfgsb.setulb")
            self.fit_driver_used_ = "setulb" if use_setulb else "threads"
            if driver == "auto" and not use_setulb:
                # never a silent fallback: the threaded rendezvous gives the same optima at about two thirds of the rate
                import warnings
                why = ("method=%r is not L-BFGS-B" % (method,) if method != "L-BFGS-B" else
                       "this SciPy (%s) does not reproduce minimize(method='L-BFGS-B') through scipy.optimize._lbfgsb.setulb "
                       "(lbfgsb_lockstep.available() is False)" % scipy.__version__)
                warnings.warn("gpcsd_amd.fit: lock-step restarts are stepped by the thread rendezvous around unmodified "
                              "scipy.optimize.minimize calls because %s; same optima, but 0.45-0.69 of the evaluation rate of "
                              "the single L-BFGS-B driver (measured: 5.2 k against 7.5 k evaluations/s on the 24 x 500 x 200 "
                              "fit).  Set model.fit_driver = 'threads' to choose this path without the warning." % why,
                              RuntimeWarning, stacklevel=3)

            class _Stats:
                batches = points = 0

            def run_group(model, ks):
                if not use_setulb:
                    return run_chains([starts[k] for k in ks],
                                      lambda s0, evaluate: model._run_restart(s0, method, fix_R, options, bounds, evaluate),
                                      lambda items: model._objective_and_grad_batch(items, fix_R), min(batch, len(ks)))
                res, st = lbfgsb_lockstep.minimize_many(lambda items: model._objective_and_grad_batch(items, fix_R),
                                                        [starts[k] for k in ks], bounds, options, min(batch, len(ks)))
                out = {}
                for i in range(len(ks)):
                    r = res[i]
                    if isinstance(r, Exception):          # what _run_restart does with a failed restart (gpcsd1d.py:219, gpcsd2d.py:258-260)
                        print(r)
                        if model.dim == 2:
                            print("\nrestarting optimization...")
                        r = None
                    out[i] = r
                ev = _Stats()
                ev.batches, ev.points = st["batches"], st["points"]
                return out, ev
            if ngroups == 1:
                outs = [run_group(self, parts[0])]
            else:
                from concurrent.futures import ThreadPoolExecutor
                models = [self] + [self._clone_for_worker() for _ in range(ngroups - 1)]
                with ThreadPoolExecutor(max_workers=ngroups) as ex:
                    outs = list(ex.map(lambda a: run_group(*a), zip(models, parts)))
            nb = npts = 0
            for ks, (out, ev) in zip(parts, outs):
                for i, k in enumerate(ks):
                    r = out[i]
                    if isinstance(r, Exception):
                        raise r
                    results[k] = r
                nb += ev.batches
                npts += ev.points
            self.fit_batches_ = (nb, npts)
        elif workers == 1:
            for k in tqdm(mine, desc="Restarts"):
                results[k] = self._run_restart(starts[k], method, fix_R, options, bounds)
        else:
            from concurrent.futures import ThreadPoolExecutor
            import queue
            pool = queue.Queue()
            for _ in range(workers):
                pool.put(self._clone_for_worker())

            def job(k):
                m = pool.get()
                try:
                    return k, m._run_restart(starts[k], method, fix_R, options, bounds)
                finally:
                    pool.put(m)
            with ThreadPoolExecutor(max_workers=workers) as ex:
                for k, r in ex.map(job, mine):
                    results[k] = r
        p = len(starts[0]) if starts else 0
        status = np.zeros(n_restarts)            # 0 failed, 1 finite optimum, 2 non-finite objective
        nll_all = np.zeros(n_restarts)
        par_all = np.zeros((n_restarts, p))
        msgs = {}
        for k, r in results.items():
            if r is None:
                continue
            fun, x, msg = r
            status[k] = 1 if np.isfinite(fun) else 2
            nll_all[k] = fun if np.isfinite(fun) else 0.0
            par_all[k] = x
            msgs[k] = msg
        if rs is not None:
            status = rs.allreduce_sum(status)
            nll_all = rs.allreduce_sum(nll_all)
            par_all = rs.allreduce_sum(par_all.ravel()).reshape(n_restarts, p)
        done = [k for k in range(n_restarts) if status[k] > 0]
        nll_values = np.array([nll_all[k] if status[k] == 1 else np.inf for k in done])
        if len(nll_values) < 1:
            print("problem with optimization!")
            return None
        finite = np.isfinite(nll_values)
        params = [par_all[k] for k, ok in zip(done, finite) if ok]
        best_ind = np.argmin(nll_values[finite])
        if verbose:
            print("\nNeg log lik values across different initializations:")
            print(nll_values)
            print("Best index termination message")
            print(msgs.get([k for k, ok in zip(done, finite) if ok][best_ind], "(other rank)"))
        self._set_from_tparams(params[best_ind], fix_R)
        self.fit_nll_values_ = nll_values
        self.fit_params_ = params
        return None

    # ------------------------------------------------------------------ prediction
    _TYPE_CODES = {"csd": _hip.PRED_CSD, "lfp": _hip.PRED_LFP, "both": _hip.PRED_BOTH}

    def _posterior_request(self, z, tstar, type, any_times=False):
        """What every posterior call at sites z and times tstar starts from: (z as float64, its (nz, dim) form, tstar as an array,
        the code of `type`).  ValueError on an unknown type and -- unless any_times (predict) -- on an empty tstar.  Opens no context."""
        if type not in self._TYPE_CODES:
            raise ValueError("type must be 'csd', 'lfp' or 'both'")
        z = np.asarray(z, dtype=np.float64)
        z2 = z.reshape(-1, 1) if self.dim == 1 else z
        tstar = np.asarray(tstar)
        if tstar.size < 1 and not any_times:
            raise ValueError("tstar must hold at least one time")
        return z, z2, tstar, self._TYPE_CODES[type]

    def _store_predictions(self, res, z, t):
        if res.get("csd") is not None:
            self.csd_pred_list = [res["csd_list"][i] for i in range(res["csd_list"].shape[0])]
            self.csd_pred = res["csd"]
        if res.get("lfp") is not None:
            self.lfp_pred_list = [res["lfp_list"][i] for i in range(res["lfp_list"].shape[0])]
            self.lfp_pred = res["lfp"]
        self.t_pred = t
        self.x_pred = z

    def predict(self, z, t, type="csd", resident=False):
        """Posterior mean of CSD and/or LFP at sites z and times t for every (local) trial (gpcsd1d.py:248-293 / gpcsd2d.py:289-334).

        resident=True (no reference counterpart) leaves the results in HBM: `csd_pred` / `lfp_pred` are then zero-copy device views
        (`__cuda_array_interface__`, float64, (nz, nt, ntrials); the `*_list` attributes (C, nz, nt, ntrials)) instead of NumPy
        arrays -- `torch.as_tensor(m.csd_pred, device="cuda")` -- valid until the model's next prediction.  Returning host arrays
        is bound by the PCIe link (231 MB per call at 384 x 500 x 50), the resident form by the GPU."""
        self._predict_mean(z, t, type, resident, at=False)

    def _predict_mean(self, z, t, type, resident, at):
        """predict (at=False: t is not checked, the reference's contraction) and predict_at (at=True)."""
        z, z2, t, code = self._posterior_request(z, t, type, any_times=not at)
        ctx = self._sync_device()
        hp, _keep = self._hparams(0.0, tstar=t)            # no jitter in predict
        shape = (z2.shape[0], t.size if at else t.shape[0], self._local_lfp().shape[2])
        sh = getattr(self, "_sharding", None)
        gather = sh is not None and getattr(sh, "gather_predictions", False)
        if resident or (gather and sh.on_device()):
            ctx.predict_resident(hp, z2, t, code, want_lists=True, at=at)
            res = ctx.predict_views(code, shape, len(self.temporal_cov_list))
            if gather:
                # trial blocks gathered ON THE DEVICE (RCCL all-gather over xGMI), one copy out on the gathering rank(s) only
                res = {k: sh.gather_trials_device(v, dst=getattr(sh, "gather_dst", None)) for k, v in res.items()}
        else:
            res = ctx.predict(hp, z2, t, code, shape, at=at)
            if gather:
                res = {k: sh.gather_trials(v) for k, v in res.items()}
        self._store_predictions(res, z, t)

    def predict_at(self, z, tstar, type="csd", resident=False):
        """Posterior mean of CSD and/or LFP at sites z and ARBITRARY times tstar (any length >= 1: up-sampling, a window, shifted
        times) for every (local) trial; arguments, attributes, `resident` and trial sharding as `predict`, with `t_pred = tstar`.

        Unlike `predict(z, t)`, which for t other than the training grid reproduces the reference's contraction of the test axis of
        compute_Kt(t) (gpcsd1d.py:277-279), this contracts the training axis and so is the GP prediction at tstar; the two agree
        when t is the training grid.  No reference counterpart."""
        self._predict_mean(z, tstar, type, resident, at=True)

    def _masked_args(self, mask, who):
        if getattr(self, "_sharding", None) is not None:
            raise NotImplementedError(who + ": trial-sharded models are not supported")
        if self._uses_host_kt():
            raise NotImplementedError(who + ": user-defined temporal covariances are not supported; only the library's own "
                                      "GPCSDTemporalCov* components are")
        mask = np.asarray(mask)
        shape = tuple(np.shape(self.lfp))
        if len(shape) != 3 or mask.shape not in (shape, shape[:2]):
            raise ValueError("%s: mask must have shape (nx, nt, ntrials) = %s or (nx, nt), not %s" % (who, shape, mask.shape))
        return mask

    def predict_masked(self, z, tstar, mask, type="csd", resident=False):
        """`predict_at(z, tstar)` when samples of the recording are MISSING: the posterior mean given the observed samples only.
        `mask` is a boolean array (nx, nt, ntrials), or (nx, nt) for one mask shared by all trials; True means observed.  Stores
        and returns what `predict_at` does (`csd_pred`, `lfp_pred`, the `*_list` attributes, `t_pred`, `x_pred`; `resident` as there).

        Exact and without iteration: with A the covariance of a full trial (no jitter, as in `predict`), M a trial's m missing
        samples and y~ the trial with zeros there, the weights are A^-1 (y~ + E_M u) with u = -G^-1 (A^-1 y~)_M and G = (A^-1)_MM, a
        dense m x m matrix per distinct mask that is assembled from the eigen-decomposition the full-grid calls use and factored by
        Cholesky.  The values of `lfp` at masked-out samples are never read as numbers: NaN or Inf there change no bit.  A trial
        without an observed sample predicts 0.  More than 8192 missing samples in one trial (GPCSD_MAX_MISSING) raise
        GPCSDCapacityError.  ValueError on a mask of another shape; NotImplementedError on trial-sharded models and on user-defined
        temporal covariances.  No reference counterpart."""
        z, z2, tstar, code = self._posterior_request(z, tstar, type)
        mask = self._masked_args(mask, "predict_masked")
        ctx = self._sync_device()
        hp, _keep = self._hparams(0.0)                     # no jitter, as predict
        shape = (z2.shape[0], tstar.size, np.shape(self.lfp)[2])
        res = ctx.predict_masked(hp, mask, z2, tstar, code, shape, resident=resident)
        self._store_predictions(res, z, tstar)
        return res

    def loglik_masked(self, mask):
        """Log marginal likelihood of the OBSERVED samples (`mask` as in `predict_masked`) under the model of the masked predictions
        (no jitter), in `loglik()`'s convention without the 2 pi term: -1/2 sum_r log det A_OO - 1/2 sum_r y_O^T A_OO^-1 y_O.  Sets
        `loglik_masked_trials` ((ntrials, 2): the two terms of every trial before the factor -1/2; a trial without an observed sample
        has (0, 0)) and `n_obs`, the number of observed samples, so that a caller comparing masks can add -1/2 n_obs log(2 pi).
        Exact (the Schur complement of the missing set); errors as `predict_masked`.  No reference counterpart."""
        mask = self._masked_args(mask, "loglik_masked")
        ctx = self._sync_device()
        hp, _keep = self._hparams(0.0)
        (ld, qd), rows, n_obs = ctx.loglik_masked(hp, mask, np.shape(self.lfp)[2])
        self.loglik_masked_trials = rows
        self.n_obs = n_obs
        return np.float64(-0.5 * ld - 0.5 * qd)

    def predict_var(self, z, tstar, type="csd", resident=False):
        """Posterior VARIANCE of CSD and/or LFP at sites z and arbitrary times tstar: the diagonal of the posterior covariance of the
        model whose mean `predict_at(z, tstar)` returns (no jitter; a per-electrode noise list on the eigen-index as in loglik).  It
        does not depend on the trials, so it is one (nz, ntstar) array per quantity.  Sets `csd_var` / `lfp_var` (the sum of the
        temporal components -- NOT the sum of the entries of the list: the components are correlated a posteriori) and
        `csd_var_list` / `lfp_var_list` (one array per temporal component), `t_var = tstar`, `x_var = z`; `csd_pred`, `lfp_pred`,
        `t_pred` and `x_pred` are left as they are.  resident=True: zero-copy device views as in `predict`.

        The LFP variance is that of the noise-free potential (no sig2n added).  Values are returned UNCLAMPED: where the data pin
        the estimate down (var << prior) the final subtraction prior - explained may leave a slightly negative entry; that is the
        caller's signal that the band is below the resolution of float64 there, not something to hide.  Under trial sharding every
        rank computes the same arrays locally (no communication; `gather_predictions` does not apply).  User-defined temporal
        covariances are not supported (no prior variance on the device): NotImplementedError.  No reference counterpart."""
        z, z2, tstar, code = self._posterior_request(z, tstar, type)
        if self._uses_host_kt():
            raise NotImplementedError("predict_var: a user-defined temporal covariance has no prior variance k(t*, t*) on the device; "
                                      "only the library's own GPCSDTemporalCov* components are supported")
        ctx = self._sync_device()
        hp, _keep = self._hparams(0.0)                     # no jitter, as predict
        C = len(self.temporal_cov_list)
        res = ctx.predict_var(hp, z2, tstar, code, resident=resident)
        for name in ("csd", "lfp"):
            if res.get(name) is not None:
                setattr(self, name + "_var_list", [res[name + "_list"][i] for i in range(C)])
                setattr(self, name + "_var", res[name])
        self.t_var = tstar
        self.x_var = z

    def predict_functionals(self, z, tstar, W, type="csd", resident=False):
        """Posterior mean and COVARIANCE of J linear summaries <W_j, f> = sum_{z,s} W[j, z, s] f(z, tstar_s) of the CSD and/or LFP
        field: a layer and time-window average, a sink-minus-source contrast, the amplitude of a segmented component
        (`utility_functions.roi_weights` builds box averages and their differences).  The model is that of `predict_at` /
        `predict_var`, which are the special case of point-mass weights: no jitter, a per-electrode noise list on the eigen-index,
        the LFP the noise-free potential.  Exact -- no Monte-Carlo error as with `sample_posterior` draws pushed through the summary --
        and with the posterior correlations that summing `predict_var` over a region ignores.

        z, tstar, type and resident as in `predict_at` / `predict_var`; W is float64 of shape (J, nz, ntstar), J >= 1 (ValueError on
        any other shape or on non-finite entries, before any device call).  Per requested quantity q in {csd, lfp} it sets, and
        returns in a dict under the same names,

          q_fun_mean        (J, ntrials)   posterior mean of every summary for every (local) trial, the sum of the components
          q_fun_mean_list   C of those     per temporal component
          q_fun_cov         (J, J)         posterior covariance of the summaries, the sum of the components -- NOT the sum of
                                           q_fun_cov_list: the components are correlated a posteriori
          q_fun_cov_list    C x (J, J)     per temporal component
          q_fun_prior, q_fun_prior_list    the prior covariance of the summaries, as the cov

        and `t_fun = tstar`, `x_fun = z`, `W_fun_shape`.  sqrt(diag(q_fun_cov)) is the standard error of a summary and
        (mean_j - mean_k) / sqrt(cov_jj + cov_kk - 2 cov_jk) the z-score of a contrast.  The covariances do not depend on the trials,
        are symmetric bit for bit and are returned UNCLAMPED (prior - explained may leave a slightly negative diagonal entry where
        the data pin a summary down below the resolution of float64).  Every sum is formed in a fixed order: the same call gives
        the same bits.  The attributes of the means, variances, leave-one-out scores and draws are left alone.

        Under trial sharding every rank computes the same covariances locally (no communication) and the means of its own trials,
        as in `predict_at`; `gather_predictions` does not apply.  User-defined temporal covariances are not supported (no k(t*, t*)
        on the device): NotImplementedError.  GPCSDCapacityError when the scratch (n_components * J * nx * nt doubles and about as
        much again) exceeds GPCSD_FUN_SCRATCH_MB megabytes (default 2048).  No reference counterpart."""
        z, z2, tstar, code = self._posterior_request(z, tstar, type)
        W = np.ascontiguousarray(W, dtype=np.float64)
        nz, nts = z2.shape[0], tstar.size
        if W.ndim != 3 or W.shape[0] < 1 or W.shape[1:] != (nz, nts):
            raise ValueError("predict_functionals: W must have shape (J, nz, ntstar) = (J >= 1, %d, %d), not %s" % (nz, nts, W.shape))
        if not np.all(np.isfinite(W)):
            raise ValueError("predict_functionals: W holds non-finite entries")
        if self._uses_host_kt():
            raise NotImplementedError("predict_functionals: a user-defined temporal covariance has no prior covariance k(t*, t*) on the "
                                      "device; only the library's own GPCSDTemporalCov* components are supported")
        ctx = self._sync_device()
        hp, _keep = self._hparams(0.0)                     # no jitter, as predict
        C = len(self.temporal_cov_list)
        raw = ctx.predict_functionals(hp, z2, tstar, W, code, self._local_lfp().shape[2], resident=resident)
        res = {}
        for name in ("csd", "lfp"):
            for kind in ("mean", "cov", "prior"):
                key = "%s_%s" % (name, kind)
                if raw.get(key) is not None:
                    res["%s_fun_%s" % (name, kind)] = raw[key]
                    res["%s_fun_%s_list" % (name, kind)] = [raw[key + "_list"][i] for i in range(C)]
        for k, v in res.items():
            setattr(self, k, v)
        self.t_fun = tstar
        self.x_fun = z
        self.W_fun_shape = tuple(W.shape)
        return res

    def loo(self, mean=True, resident=False):
        """Leave-one-out cross-validation of the model under its current hyper-parameters, in closed form and without a refit
        (Rasmussen & Williams, Gaussian Processes for Machine Learning, 5.4.2): how well the fitted model explains the recording
        it was fitted to -- to choose between restarts, noise models or numbers of temporal components, and to find the electrode
        or trial the model does not describe.  Returns the total log predictive density, the sum of `loo_lpd`, as a float.

        K is the covariance of the data exactly as `loglik()` sees it: (Ks + JITTER I) (x) Kt + noise, through its eigen-form
        (Qs (x) Qt) diag(D) (Qs (x) Qt)^T with D[x', i'] = es[x'] et[i'] + sig2n; the jitter sits on Ks, and a per-electrode noise
        list sits on the eigen-index x' as in the reference's comp_eig_D (utility_functions.py:54-63).  User-defined temporal
        covariances are allowed (only Kt on the training grid is used).  With c = diag(K^-1) and beta_r = K^-1 y_r it sets

          loo_var   (nx, nt)           1 / c: the predictive variance of the NOISY sample given all other samples of its trial
          loo_mean  (nx, nt, ntrials)  y - beta / c, or None with mean=False (which also spares the device its stores)
          loo_lpd   (nx, ntrials)      sum over t of 1/2 log c - 1/2 beta^2 / c - 1/2 log(2 pi)
          loo_sse   (nx, ntrials)      sum over t of the squared leave-one-out residual (y - loo_mean)^2

        Per-electrode and per-trial scores are `loo_lpd.sum(1)` and `loo_lpd.sum(0)`.  Unlike `loglik()` the log density KEEPS its
        2 pi constant: it is a density per sample, meant to be compared across models and data sizes.  The sums are formed in a
        fixed order: the same call gives the same bits.  resident=True: zero-copy device views as in `predict`.  `csd_pred`,
        `lfp_pred`, the `*_var` attributes and `t_pred` are left alone.  Under trial sharding the per-trial arrays are this rank's
        block of trials, `loo_var` is the same on every rank and the returned total is summed over the ranks.  No reference
        counterpart."""
        ctx = self._sync_device()
        hp, _keep = self._hparams(self.JITTER)             # the jitter of loglik
        res = ctx.loo(hp, self._local_lfp().shape, want_mean=mean, resident=resident)
        self.loo_var, self.loo_lpd, self.loo_sse, self.loo_mean = res["var"], res["lpd"], res["sse"], res["mean"]
        total = float(np.sum(res["lpd"].numpy() if resident else res["lpd"]))
        sh = getattr(self, "_sharding", None)
        if sh is not None:
            total = float(sh.allreduce_sum(np.array([total]))[0])
        return total

    CV_MAX_FOLD = 16                     # GPCSD_CV_MAX_FOLD

    @classmethod
    def _fold_arrays(cls, folds, nx):
        """folds of cv_electrodes -> (fold_ptr (nfolds + 1), fold_idx) int32 arrays, the CSR form of the C ABI, order kept.  None: one
        fold per electrode; an int k: electrode i in fold i % k; otherwise a sequence of index sequences.  ValueError on a malformed
        list (no fold, an empty fold, an index outside [0, nx), an electrode held out twice), GPCSDCapacityError on a fold above
        CV_MAX_FOLD electrodes.  Checked on whole arrays: a list of hundreds of folds costs no Python loop beyond its conversion."""
        nx = int(nx)
        if folds is None:
            sizes, idx = np.ones(nx, dtype=np.int64), np.arange(nx, dtype=np.int64)
        elif isinstance(folds, (int, np.integer)) and not isinstance(folds, bool):
            k = int(folds)
            if not 1 <= k <= nx:
                raise ValueError("cv_electrodes: folds=%d, need 1 <= k <= nx = %d" % (k, nx))
            idx = np.argsort(np.arange(nx) % k, kind="stable")                  # fold 0: 0, k, 2k, ...; fold 1: 1, k + 1, ...
            sizes = np.bincount(np.arange(nx) % k, minlength=k)
        else:
            try:
                parts = [np.atleast_1d(np.asarray(f)) for f in folds]
            except TypeError:
                raise ValueError("cv_electrodes: folds is None, an int or a sequence of index sequences")
            if len(parts) == 0:
                raise ValueError("cv_electrodes: no folds")
            if any(f.ndim != 1 or f.size == 0 for f in parts):
                raise ValueError("cv_electrodes: an empty fold (or one that is not a sequence of indices)")
            sizes = np.array([f.size for f in parts], dtype=np.int64)
            idx = np.concatenate(parts)
            if not np.issubdtype(idx.dtype, np.integer):
                if idx.dtype.kind not in "fiu" or not np.all(np.equal(np.mod(idx, 1), 0)):
                    raise ValueError("cv_electrodes: folds hold non-integer indices")
            idx = idx.astype(np.int64)
            if idx.min() < 0 or idx.max() >= nx:
                raise ValueError("cv_electrodes: a fold has an index outside [0, %d)" % nx)
            if np.bincount(idx, minlength=nx).max() > 1:
                raise ValueError("cv_electrodes: an electrode is held out twice")
        if sizes.max() > cls.CV_MAX_FOLD:
            raise _hip.GPCSDCapacityError("cv_electrodes: a fold of %d electrodes exceeds CV_MAX_FOLD = %d (predict_masked with a "
                                          "dead-electrode mask holds out larger sets)" % (sizes.max(), cls.CV_MAX_FOLD))
        ptr = np.zeros(sizes.size + 1, dtype=np.int32)
        ptr[1:] = np.cumsum(sizes)
        return ptr, np.ascontiguousarray(idx, dtype=np.int32)

    @staticmethod
    def _fold_tuple(ptr, idx):
        idx, p = idx.astype(np.int64), ptr.tolist()
        return tuple(idx[a:b] for a, b in zip(p[:-1], p[1:]))

    @classmethod
    def _normalise_folds(cls, folds, nx):
        """... as the tuple of 1-D int arrays that becomes `cv_folds`."""
        ptr, idx = cls._fold_arrays(folds, nx)
        return cls._fold_tuple(ptr, idx)

    def cv_electrodes(self, folds=None, mean=True, resident=False):
        """Leave-ELECTRODES-out cross-validation of the model under its current hyper-parameters, in closed form and without a
        refit: every sample of a fold's electrodes is held out at once and predicted from the other electrodes.  `loo()` keeps an
        electrode's neighbours in time, which explain almost all of a temporally smooth sample; this score asks whether the SPATIAL
        model -- the forward model, R and ell_s -- predicts a channel it has not seen, and is the score the CSD literature uses to
        compare estimators.  Returns the total log predictive density, the sum of `cv_lpd`, as a float.

        folds: None (one fold per electrode), an int k (electrode i in fold i % k) or a sequence of index sequences: disjoint, 1 to
        16 electrodes each, indices in [0, nx); electrodes in no fold are allowed.  A malformed list raises ValueError and a larger
        fold GPCSDCapacityError, both before the device is touched (predict_masked holds out larger sets).

        K is the covariance of `loglik()` and `loo()`: (Ks + JITTER I) (x) Kt + noise through (Qs (x) Qt) diag(D) (Qs (x) Qt)^T, a
        noise list on the eigen-index, user-defined temporal covariances allowed.  For a fold F of f electrodes (K^-1)_FF is
        Qt blockdiag_j(G_j) Qt^T with G_j[a][b] = sum_x' Qs[a][x'] Qs[b][x'] / D[x'][j], so with u_j,r = (K^-1 y_r)[F] in the temporal
        eigen-basis and e_j,r = G_j^-1 u_j,r (the held-out residual y - yhat in that basis) the call sets

          cv_folds   tuple of int arrays      the folds as given, order kept
          cv_lpd     (nfolds, ntrials)        1/2 sum_j log det G_j - 1/2 sum_j u^T e - 1/2 f nt log(2 pi): the JOINT log predictive
                                              density of the block, with its 2 pi constant as in `loo`
          cv_sse     (nx, ntrials)            sum_j e[a]^2 = sum over t of (y - yhat)^2 of electrode a (Qt is orthogonal)
          cv_var     (nx, nt)                 sum_j Qt[t][j]^2 (G_j^-1)[a][a]: predictive variance of the NOISY held-out sample
          cv_mean    (nx, nt, ntrials)        y - sum_j Qt[t][j] e[a], or None with mean=False (the other outputs keep their bits)
          cv_status  (nfolds,) int            1: some G_j of the fold lost positive definiteness; its outputs are NaN and it is
                                              left out of the returned total

        Rows of electrodes in no fold are NaN.  For a one-trial model and folds=None, `np.sqrt(cv_sse[:, 0]).sum()` is kCSD's
        cross-validation error sum_i ||V_i - Vhat_i||_2 (KCSD1D's leave-one-electrode-out scan), so GPCSD and kCSD can be ranked
        on the same held-out-channel score.  The sums are formed in a fixed order: the same call gives the same bits, and a fold's
        outputs depend neither on the other folds of the call nor on their order.  resident=True: zero-copy device views as in
        `loo` (`cv_status` stays a host array).  `csd_pred`, `lfp_pred`, `t_pred`, the `loo_*` and the `*_var` attributes are left
        alone.  Under trial sharding the per-trial arrays are this rank's block of trials, `cv_var` is the same on every rank and
        the returned total is summed over the ranks.  No reference counterpart."""
        ptr, idx = self._fold_arrays(folds, np.atleast_3d(self.lfp).shape[0])
        ctx = self._sync_device()
        hp, _keep = self._hparams(self.JITTER)             # the jitter of loglik
        res = ctx.cv_electrodes(hp, self._local_lfp().shape, ptr, idx, want_mean=mean, resident=resident)
        self.cv_var, self.cv_lpd, self.cv_sse, self.cv_mean = res["var"], res["lpd"], res["sse"], res["mean"]
        self.cv_status = res["status"]
        lpd = res["lpd"].numpy() if resident else res["lpd"]
        self.cv_folds = self._fold_tuple(ptr, idx)
        total = float(np.sum(lpd[self.cv_status == 0]))
        sh = getattr(self, "_sharding", None)
        if sh is not None:
            total = float(sh.allreduce_sum(np.array([total]))[0])
        return total

    # ------------------------------------------------------------------ hyper-parameter uncertainty
    def _fisher_args(self, who):
        """(ctx, hp, keep, ng) of the score / information calls: the model of loglik(), scalar noise only."""
        if not self._sig2n_is_scalar():
            raise NotImplementedError("%s: a per-electrode noise list ties the noise to the eigen-index of Ks, so the model is not a "
                                      "function of Ks alone; only a scalar sig2n is supported" % who)
        host = self._uses_host_kt()
        if host and not self._host_kt_is_differentiable():
            raise NotImplementedError("%s: user-defined temporal covariances need compute_dKt(name)" % who)
        ctx = self._sync_device()
        hp, keep = self._hparams(self.JITTER, want_dkt=host)
        return ctx, hp, keep, 1 + self.dim + 2 * len(self.temporal_cov_list) + 1

    def hyperparameter_names(self):
        """Names of the hyper-parameters in slot order: R, the spatial length scales, (ell, sigma2) per temporal component, sig2n."""
        names = ["R"] + ["spatial_%s" % n for n in self._spatial_names]
        for i in range(len(self.temporal_cov_list)):
            names += ["temporal%d_ell" % (i + 1), "temporal%d_sigma2" % (i + 1)]
        return names + ["sig2n"]

    def _natural_values(self):
        return np.array([getter() for getter, _, _, _, _ in self._param_slots()] + [self.sig2n["value"]], dtype=np.float64)

    def trial_scores(self, resident=False):
        """Per-trial scores s[r, i] = d log p(y_r | theta) / d theta_i at the current hyper-parameters, (ntrials, ng), in NATURAL
        parameters in slot order (`hyperparameter_names()`): [R, ell_s.., (ell_t, sigma2_t).., sig2n].  Their sum over the trials is
        the gradient that fit() follows; a trial whose row is large pulls the fit.  The sums are formed in a fixed order: the same
        call gives the same bits, and a trial's row does not depend on which other trials are resident.  Sets `trial_scores_`.
        resident=True: a zero-copy device view as in `predict` (this rank's block under trial sharding); otherwise a host array,
        under `shard_trials` the blocks of all ranks gathered in trial order.  A per-electrode noise list raises
        NotImplementedError.  No reference counterpart."""
        ctx, hp, _keep, ng = self._fisher_args("trial_scores")
        R_local = self._local_lfp().shape[2]
        if resident:                                       # this rank's block, where it lies: no gather
            self.trial_scores_ = ctx.trial_scores(hp, R_local, ng, resident=True)
            return self.trial_scores_
        S = ctx.trial_scores(hp, R_local, ng)
        sh = getattr(self, "_sharding", None)
        if sh is not None:
            # every rank's block at its own rows of a zero array: the sum over the ranks is the gather, in trial order
            full = np.zeros((np.shape(self.lfp)[2], ng))
            full[sh.local_slice(full.shape[0])] = S
            S = sh.allreduce_sum(full.ravel()).reshape(full.shape)
        self.trial_scores_ = S
        return S

    def fisher_information(self, kind="expected", log_params=True, fix_R=False):
        """Fisher information of the hyper-parameters from ALL trials, (ng, ng) in slot order (`hyperparameter_names()`).

          kind="expected"   R_total * I, I_ij = 1/2 tr(K^-1 d_i K K^-1 d_j K) of one trial: reads no data, no communication
          kind="empirical"  S^T S of the per-trial scores (`trial_scores()`)

        log_params=True: in the log-parameters of fit() (d/d tau = v d/d v, so I_tau = diag(v) I diag(v)); False: natural
        parameters.  fix_R drops row and column 0.  Symmetric bit for bit.  No reference counterpart."""
        if kind not in ("expected", "empirical"):
            raise ValueError("kind must be 'expected' or 'empirical'")
        if kind == "expected":
            ctx, hp, _keep, ng = self._fisher_args("fisher_information")
            info = ctx.fisher(hp, ng) * float(np.shape(self.lfp)[2])
        else:
            S = np.asarray(self.trial_scores())
            info = S.T @ S
            info = 0.5 * (info + info.T)
        if log_params:
            v = self._natural_values()
            info = info * np.outer(v, v)                  # (one product per entry: symmetric in, symmetric out)
        return info[1:, 1:] if fix_R else info

    def hyperparameter_cov(self, kind="expected", fix_R=False):
        """Large-sample covariance of the fitted hyper-parameters in the log-parameters of fit(), at the current values (meant for
        the point fit() returned).  With H = I_tau - d^2(log prior) / d tau^2 (I_tau the expected information of all trials,
        d^2/d tau^2 = v^2 lp''(v) + v lp'(v) per parameter):

          kind="expected"   H^-1
          kind="sandwich"   H^-1 (S_tau^T S_tau) H^-1, S_tau the per-trial scores in log-parameters (robust to misspecification)

        Returns a dict: "names" (slot order), "cov" (log units), "se" (standard errors, log units), "value" (natural units) and
        "interval" (n, 2) = exp(tau -+ 1.96 se) in natural units.  fix_R leaves R out.  Raises numpy.linalg.LinAlgError when H is
        not positive definite (the point is no maximum of the posterior, or a parameter is not identified)."""
        if kind not in ("expected", "sandwich"):
            raise ValueError("kind must be 'expected' or 'sandwich'")
        H = np.array(self.fisher_information("expected", log_params=True, fix_R=False))
        v = self._natural_values()
        priors = [prior for _, _, prior, _, _ in self._param_slots()] + [self.sig2n["prior"]]
        for i, (pr, x) in enumerate(zip(priors, v)):
            H[i, i] -= x * x * pr.d2lpdf(x) + x * pr.dlpdf(x)
        names = self.hyperparameter_names()
        if fix_R:
            H, v, names = H[1:, 1:], v[1:], names[1:]
        L = np.linalg.cholesky(H)                        # LinAlgError when H is not positive definite
        Linv = np.linalg.solve(L, np.eye(H.shape[0]))
        cov = Linv.T @ Linv
        if kind == "sandwich":
            S = np.asarray(self.trial_scores()) * self._natural_values()[None, :]
            S = S[:, 1:] if fix_R else S
            J = S.T @ S
            cov = cov @ (0.5 * (J + J.T)) @ cov
        cov = 0.5 * (cov + cov.T)
        se = np.sqrt(np.diag(cov))
        tau = np.log(v)
        return {"names": names, "cov": cov, "se": se, "value": v,
                "interval": np.stack([np.exp(tau - 1.96 * se), np.exp(tau + 1.96 * se)], axis=1)}

    @staticmethod
    def _types(type):
        if type not in ("csd", "lfp", "both"):
            raise ValueError("type must be 'csd', 'lfp' or 'both'")
        return ("csd", "lfp") if type == "both" else (type,)

    def phase(self, A, type="csd", component=None, at=None, resident=False):
        """Band phase and amplitude of the model's CURRENT prediction along time, at every site and (local) trial: the analytic
        signal of `csd_pred` / `lfp_pred` -- or of temporal component `component` of their `*_list` forms -- under the operator A
        (nsel, ntpred) of `utility_functions.analytic_operator` (zero-phase band-pass + Hilbert transform as one matrix; its rows are
        the kept times).  Works on what the last `predict` / `predict_at` / `loglik_predict_many` left, host arrays or resident
        views alike; a resident prediction is read in HBM and never crosses PCIe.  Sets `csd_phase`, `csd_amp` and / or
        `lfp_phase`, `lfp_amp`, each (nz, nsel, ntrials) -- host arrays, or with resident=True (resident predictions, one type per
        call: the library has one set of result buffers) zero-copy device views -- and `t_phase`: `t_pred` at the kept times when
        the caller passes the `at` the operator was built with, None otherwise.  The unit phasors are kept for `plv()`.  The
        prediction, variance, leave-one-out and sample attributes are left alone.  What the reference's scripts do on the host
        with filtfilt + hilbert + np.angle (auditory_lfp/fit_gpcsd_baseline.py:303-334, neuropixels/fit_gpcsd2d.py:147-159); no
        counterpart in the package."""
        from .utility_functions import band_phase
        types = self._types(type)
        A = np.asarray(A)
        if resident and len(types) > 1:
            raise ValueError("resident=True holds one field's results: call phase() per type")
        ctx = self._context()
        keep = dict(getattr(self, "_phasors", {}))
        for name in types:
            x = getattr(self, name + "_pred", None)
            if x is None:
                raise RuntimeError("phase: no %s prediction to work on (call predict / predict_at with type=%r first)" % (name, name))
            if component is not None:
                lst = getattr(self, name + "_pred_list")
                if not 0 <= int(component) < len(lst):
                    raise ValueError("component must be in [0, %d)" % len(lst))
                x = lst[int(component)]
            dev = isinstance(x, _hip.DeviceArray)
            if resident and not dev:
                raise ValueError("resident=True needs a resident prediction")
            res = band_phase(x, A, want=("phase", "amp", "u_re", "u_im"), resident=dev, ctx=ctx)
            if dev:
                # the phasors stay in the library's buffers; plv() forms them again from the source should a later call have
                # overwritten them (one product, no PCIe)
                keep[name] = {"source": x, "A": A, "generation": ctx.phasor_generation, "shape": tuple(res["u_re"].shape)}
                if not resident:
                    res = {k: v.numpy() for k, v in res.items() if k in ("phase", "amp")}
            else:
                keep[name] = {"u": (res["u_re"], res["u_im"]), "shape": tuple(res["u_re"].shape)}
            setattr(self, name + "_phase", res["phase"])
            setattr(self, name + "_amp", res["amp"])
        self._phasors = keep
        self.t_phase = None if at is None else np.asarray(self.t_pred)[np.asarray(at, dtype=np.intp).reshape(-1)]

    def plv(self, type="csd"):
        """Phase-locking value of all site pairs over the trials, from the phases of the last `phase()` call: sets `csd_plv` /
        `lfp_plv` (nsel, nz, nz), plv[j, a, b] = |mean over trials of exp(i (phase_a - phase_b))| at kept time j, and
        `csd_plv_angle` / `lfp_plv_angle`, the angle of that mean resultant (the mean phase difference a - b).  One launch for all
        pairs and times; plv is symmetric and the angle antisymmetric bit for bit.  Under trial sharding each rank forms the sums
        R_local * c of its block of trials, the sums are added over the ranks (one all-reduce per type) and every rank holds the
        PLV over all trials; `gather_predictions` does not apply.  The prediction, variance, leave-one-out and sample attributes
        are left alone.  No reference counterpart in the package (auditory_lfp/fit_gpcsd_baseline.py:303-334 loops over the pairs)."""
        from .utility_functions import band_phase, plv, plv_from_sums
        types = self._types(type)
        sh = getattr(self, "_sharding", None)
        if sh is not None and getattr(sh, "gather_predictions", False):
            raise NotImplementedError("plv: gather_predictions does not apply; each rank works on its block of trials")
        ctx = self._context()
        for name in types:
            rec = getattr(self, "_phasors", {}).get(name)
            if rec is None:
                raise RuntimeError("plv: call phase(A, type=%r) first" % name)
            if "u" in rec:
                u = rec["u"]
            else:
                if rec["generation"] == ctx.phasor_generation:
                    u = ctx.phasors(rec["shape"])
                else:
                    u = band_phase(rec["source"], rec["A"], want=("u_re", "u_im"), resident=True)
                    rec["generation"] = ctx.phasor_generation
            p, c = plv(u, ctx=ctx)
            if sh is not None:
                R_local = rec["shape"][2]
                sums = sh.allreduce_sum(np.stack([R_local * c.real, R_local * c.imag]))
                p, c = plv_from_sums(sums, np.atleast_3d(self.lfp).shape[2])
            setattr(self, name + "_plv", p)
            setattr(self, name + "_plv_angle", np.arctan2(c.imag, c.real))

    def _spectral_source(self, who, name, component):
        """The field `spectrum()` / `coherence()` work on: the current prediction of type `name`, or one temporal component of it."""
        x = getattr(self, name + "_pred", None)
        if x is None:
            raise RuntimeError("%s: no %s prediction to work on (call predict / predict_at with type=%r first)" % (who, name, name))
        if component is not None:
            lst = getattr(self, name + "_pred_list")
            if not 0 <= int(component) < len(lst):
                raise ValueError("component must be in [0, %d)" % len(lst))
            x = lst[int(component)]
        t = np.asarray(self.t_pred, dtype=np.float64).reshape(-1)
        if t.size > 2:
            dt = np.diff(t)
            if not np.max(np.abs(dt - dt.mean())) <= 1e-6 * abs(dt.mean()):
                raise ValueError("%s: t_pred is not uniformly spaced; a periodogram needs a uniform grid" % who)
        return x

    def _spectral_sharding(self, who):
        sh = getattr(self, "_sharding", None)
        if sh is not None and getattr(sh, "gather_predictions", False):
            raise NotImplementedError("%s: gather_predictions does not apply; each rank works on its block of trials" % who)
        return sh

    def spectrum(self, fs, nfft=None, window="boxcar", scaling="density", detrend=False, rows=None, type="csd", component=None,
                 per_trial=False, resident=False):
        """Power spectrum along time of the model's CURRENT prediction, averaged over the trials: what
        `scipy.signal.periodogram(pred, fs, window, nfft, detrend, scaling=scaling, axis=1)[1].mean(-1)` gives on the host
        (auditory_lfp/fit_gpcsd_baseline.py:189-195, neuropixels/fit_gpcsd2d.py:120-128), for `csd_pred` / `lfp_pred` or temporal
        component `component` of their `*_list` forms, host arrays or resident views alike; a resident prediction is read in HBM and
        only the (nz, nf) result crosses PCIe.  fs is the caller's sampling rate (the time unit of `t_pred` is theirs; `t_pred` must be
        uniformly spaced: ValueError otherwise); nfft, window, scaling, detrend, rows as in `utility_functions.spectral_operator`
        (one-sided).  Sets `f_spec` and `csd_psd` / `lfp_psd` (nz, nf); with per_trial=True also `csd_power` / `lfp_power`
        (nz, nf, ntrials), the periodogram of every trial -- host arrays, or with resident=True (resident predictions, one type per
        call: the library has one set of result buffers) zero-copy device views.  Under trial sharding the ranks' sums are added (one
        all-reduce per type) and every rank holds the spectrum over all trials as a host array; the per-trial power stays this rank's
        block; `gather_predictions` does not apply.  The prediction, phase, variance, leave-one-out and sample attributes are left
        alone.  No counterpart in the package."""
        from .utility_functions import power_spectrum, spectral_operator, spectrum_from_sums
        types = self._types(type)
        if resident and len(types) > 1:
            raise ValueError("resident=True holds one field's results: call spectrum() per type")
        sh = self._spectral_sharding("spectrum")
        ctx = self._context()
        for name in types:
            x = self._spectral_source("spectrum", name, component)
            if resident and not isinstance(x, _hip.DeviceArray):
                raise ValueError("resident=True needs a resident prediction")
            f, A = spectral_operator(x.shape[1], fs, nfft, window, scaling, detrend, True, rows)
            res = power_spectrum(x, A, per_trial=per_trial, resident=resident, ctx=ctx)
            psd = res["psd"]
            if sh is not None:
                local = psd.numpy() if resident else psd
                psd = spectrum_from_sums({"psd": sh.allreduce_sum(x.shape[2] * np.asarray(local))}, np.atleast_3d(self.lfp).shape[2])["psd"]
            setattr(self, name + "_psd", psd)
            if per_trial:
                setattr(self, name + "_power", res["power"])
            self.f_spec = f

    def coherence(self, fs, rows, nfft=None, window="boxcar", scaling="density", detrend=False, type="csd", component=None):
        """Cross-spectrum and magnitude-squared coherence of all site pairs of the model's CURRENT prediction over the trials, at the
        frequency indices `rows` of the periodogram `spectrum()` describes (required: the result has len(rows) nz^2 entries).  Sets
        `csd_xspec` / `lfp_xspec` (nf, nz, nz), complex: xspec[j, a, b] = mean over trials of X_a conj(X_b), which is
        `scipy.signal.csd(x_b, x_a)` averaged over the trials (SciPy conjugates its first argument; the orientation of `plv()`'s
        phase_a - phase_b), `csd_coh` / `lfp_coh` = |xspec[a, b]|^2 / (xspec[a, a] xspec[b, b]) -- what `scipy.signal.coherence` gives
        on the concatenated trials with nperseg = the trial length and no overlap; 0 where a site has no power -- and `f_coh`.  The
        coherence and xspec.real are symmetric, xspec.imag antisymmetric bit for bit.  `t_pred` must be uniformly spaced.  Under trial
        sharding each rank forms R_local * xspec of its block, the sums are added over the ranks (one all-reduce per type) and the
        coherence is formed after the sum; `gather_predictions` does not apply.  The prediction, phase, variance, leave-one-out and
        sample attributes are left alone.  No counterpart in the package."""
        from .utility_functions import cross_spectrum, power_spectrum, spectral_operator, spectrum_from_sums
        if rows is None:
            raise ValueError("coherence: rows (the frequency indices to keep) is required")
        types = self._types(type)
        sh = self._spectral_sharding("coherence")
        ctx = self._context()
        for name in types:
            x = self._spectral_source("coherence", name, component)
            f, A = spectral_operator(x.shape[1], fs, nfft, window, scaling, detrend, True, rows)
            res = power_spectrum(x, A, coefficients=True, resident=isinstance(x, _hip.DeviceArray), ctx=ctx)
            Sx, coh = cross_spectrum(res, ctx=ctx)
            if sh is not None:
                sums = sh.allreduce_sum(np.stack([x.shape[2] * Sx.real, x.shape[2] * Sx.imag]))
                out = spectrum_from_sums({"xspec": sums}, np.atleast_3d(self.lfp).shape[2])
                Sx, coh = out["xspec"], out["coh"]
            setattr(self, name + "_xspec", Sx)
            setattr(self, name + "_coh", coh)
            self.f_coh = f

    def torus_graph(self, type="csd", at=0, sites=None, nboot=0, seed=None):
        """Phase-difference torus graph (score matching) of the phases of the last `phase()` call at kept time `at`, over the trials:
        the CONDITIONAL coupling of every pair of `sites` (default: all prediction sites) given the others, where `plv()` is the
        marginal one.  Sets `csd_tg` / `lfp_tg` to the dict of `utility_functions.torus_graph` (pairs, phi, cond_coupling, chi2, pvals,
        and with nboot > 0 the bootstrap replicates under `seed`).  Phasors that are resident are gathered and fitted in HBM; only
        the small results come back.  Needs more trials than a model of d (d - 1) parameters can be fitted to: np.linalg.LinAlgError
        otherwise.  Trial-sharded models are not supported (fit on the gathered phases with utility_functions.torus_graph).  The
        prediction, phase, variance, leave-one-out and sample attributes are left alone.  No counterpart in the package
        (auditory_lfp/torus_graph_fit.py, neuropixels/fit_torus_graph.py)."""
        from .utility_functions import band_phase, torus_graph
        types = self._types(type)
        if getattr(self, "_sharding", None) is not None:
            raise NotImplementedError("torus_graph: trial-sharded models are out of scope; gather the phases and call utility_functions.torus_graph")
        ctx = self._context()
        for name in types:
            rec = getattr(self, "_phasors", {}).get(name)
            if rec is None:
                raise RuntimeError("torus_graph: call phase(A, type=%r) first" % name)
            if "u" in rec:
                u = rec["u"]
            elif rec["generation"] == ctx.phasor_generation:
                u = ctx.phasors(rec["shape"])
            else:
                u = band_phase(rec["source"], rec["A"], want=("u_re", "u_im"), resident=True)
                u = (u["u_re"], u["u_im"])
                rec["generation"] = ctx.phasor_generation
            setattr(self, name + "_tg", torus_graph(u, nboot=nboot, seed=seed, ctx=ctx, at=at, sites=sites))

    def loglik_predict_many(self, param_sets, z, t, type="csd", resident=False, share_spatial=False):
        """loglik() and predict(z, t, type) under each of a LIST of hyper-parameter sets -- dicts as extract_model_params() returns
        them: the optima of every restart of a fit, a grid, posterior draws -- in order.  Returns the log-likelihoods, one per set;
        the prediction attributes hold the LAST set's posterior means as after predict() (resident=True: left in HBM, see
        predict), and the model's hyper-parameters are left at the last set.

        No reference counterpart as ONE call: the reference's callers loop restore_model_params -> loglik -> predict
        (neuropixels/fit_gpcsd2d.py:93-107).  Because the sets are known up front, every set's evaluation is queued as one paired
        call (its four eigenproblems share launches two by two) that ANNOUNCES the next set (gpcsd_prefetch_pair): the next set's
        decomposition chains run under this set's products instead of behind the host's collection of its value.
        share_spatial=True additionally decomposes ONE spatial matrix per set where both calls have the same spatial
        hyper-parameters (Ks + jitter I and Ks share eigenvectors; results then differ from the fenced calls in the last bits)."""
        if type not in ("csd", "lfp", "both"):
            raise ValueError("type must be 'csd', 'lfp' or 'both'")
        param_sets = list(param_sets)
        if not param_sets:
            return np.zeros(0)
        ctx = self._sync_device()
        z = np.asarray(z, dtype=np.float64)
        z2 = np.ascontiguousarray(z.reshape(-1, 1) if self.dim == 1 else z)
        t = np.asarray(t)
        code = self._TYPE_CODES[type]
        sets = []
        for p in param_sets:                               # every set's two hyper-parameter structs, before anything is queued
            self.restore_model_params(p)
            sets.append((self._hparams(self.JITTER), self._hparams(0.0, tstar=t)))
        R_local = self._local_lfp().shape[2]
        ntrials = np.shape(self.lfp)[2]
        sh = getattr(self, "_sharding", None)
        was = ctx.pair_share_s_on()
        ctx.pair_share_s(bool(share_spatial))
        out = np.empty(len(sets))
        try:
            for k, ((hp, _k1), (hp0, _k0)) in enumerate(sets):
                ctx.loglik_predict_async(hp, hp0, z2, t, code, want_lists=True)
                if k + 1 < len(sets):
                    (hn, _a), (hn0, _b) = sets[k + 1]
                    ctx.prefetch_pair(hn, hn0, z2, t)
                sumlog, quad = ctx.loglik_parts_wait()
                if sh is not None:
                    quad = float(sh.allreduce_sum(np.array([quad]))[0])
                out[k] = -0.5 * ntrials * sumlog - 0.5 * quad
        finally:
            ctx.pair_share_s(was)
        res = ctx.predict_views(code, (z2.shape[0], t.shape[0], R_local), len(self.temporal_cov_list))
        gather = sh is not None and getattr(sh, "gather_predictions", False)
        if gather and sh.on_device():
            res = {k: sh.gather_trials_device(v, dst=getattr(sh, "gather_dst", None)) for k, v in res.items()}
        elif not resident or gather:
            res = {k: v.numpy() for k, v in res.items()}
            if gather:
                res = {k: sh.gather_trials(v) for k, v in res.items()}
        self._store_predictions(res, z, t)
        return out

    def _sample_posterior_args(self, z, tstar, type, nsamples):
        """Validation and shapes shared by sample_posterior and _sample_posterior_from_normals; opens no context."""
        _z, z2, tstar, code = self._posterior_request(z, tstar, type)
        if int(nsamples) < 1:
            raise ValueError("nsamples must be at least 1")
        if self._uses_host_kt():
            raise NotImplementedError("sample_posterior: a user-defined temporal covariance has no joint Gram over [t*; t] on the device; "
                                      "only the library's own GPCSDTemporalCov* components are supported")
        sh = getattr(self, "_sharding", None)
        if sh is not None and getattr(sh, "gather_predictions", False):
            raise NotImplementedError("sample_posterior: gather_predictions does not apply to draws; each rank returns its block of trials")
        return z2, tstar, code, sh

    def _sample_posterior_call(self, z2, tstar, code, sh, nsamples, seed, xi, eps, resident):
        ctx = self._sync_device()
        hp, _keep = self._hparams(0.0)                     # no jitter, as predict
        R_local = self._local_lfp().shape[2]
        # a rank's block of trials draws the normals the unsharded job draws for those trials
        ctx.set_trial_offset(0 if sh is None else sh.local_slice(np.atleast_3d(self.lfp).shape[2]).start or 0)
        res = ctx.sample_posterior(hp, z2, tstar, code, nsamples, seed, R_local, xi=xi, eps=eps, resident=resident)
        return res.get("csd"), res.get("lfp")

    def sample_posterior(self, z, tstar, nsamples=1, type="csd", seed=1, resident=False):
        """Joint draws from the posterior of the CSD and/or LFP at sites z and ARBITRARY times tstar: `nsamples` fields per (local)
        trial, each consistent with that trial's recording.  Returns (csd, lfp), arrays of shape (nz, ntstar, ntrials, nsamples)
        with None for the part not requested; resident=True returns zero-copy device views as in `predict`.  What `csd_var` cannot
        give -- the uncertainty of a peak latency, a sink's extent, a phase: any nonlinear functional of a whole (z, t) field --
        comes from pushing these draws through the same pipeline as the posterior mean.

        The model is the one whose mean `predict_at` and whose variance `predict_var` return: no jitter, a per-electrode noise
        list on the eigen-index as in loglik, and the LFP is the noise-free potential.  Draws are of the SUM of the temporal
        components (a joint draw does not identify them separately).  Each draw is f_prior + P (y - phi - eps) (Matheron's rule)
        with a joint prior draw (f_prior, phi), a noise draw eps and the linear map P of `predict_at`; the normals come from a
        counter-based generator on the GPU, so the same `seed` gives the same draws, however the work is chunked and -- under
        trial sharding, where each rank returns its block of trials -- however the trials are spread over ranks.
        `gather_predictions` does not apply (NotImplementedError), nor do user-defined temporal covariances.  The prediction,
        variance and leave-one-out attributes are left alone.  No reference counterpart (the reference has sample_prior only)."""
        z2, tstar, code, sh = self._sample_posterior_args(z, tstar, type, nsamples)
        return self._sample_posterior_call(z2, tstar, code, sh, int(nsamples), int(seed), None, None, resident)

    def sample_features(self, z, tstar, labels, nsamples=1, type="csd", seed=1, band=False, return_draws=False, resident=False,
                        floor=1e-10):
        """Posterior distributions of NONLINEAR features of the CSD and/or LFP field over labelled regions of the (z, t*) plane: the
        draws of `sample_posterior(z, tstar, nsamples, type, seed)` reduced on the device, chunk by chunk inside the sampler, so that
        nothing but the answer grows with `nsamples` -- a latency interval or a simultaneous band takes hundreds of draws per trial,
        whose fields would be gigabytes.  labels: integer map (nz, ntstar), 0 the background, 1..J the regions (J = labels.max()).
        Returns (csd_feat, lfp_feat), None for the part not requested: the dicts of `utility_functions.region_features` with arrays
        over (J, ntrials, nsamples) -- max, min, sum, abs_sum, argmax, argmin, peak_time, trough_time, com_time, com_site.

        band=True adds "supdev": sup over the region of |draw - mean| / sd with the mean of `predict_at` and the variance of
        `predict_var` at the same sites and times, formed inside the call (`csd_pred`, `csd_var`, ... and their device buffers are
        left alone); sd counts where var > floor * max(var), other points drop out.  `utility_functions.simultaneous_band(supdev)`
        is then the half-width of a simultaneous band mean +- q sd over each region.
        return_draws=True also keeps the draws and returns (csd_feat, lfp_feat, csd, lfp) with the draws as `sample_posterior`
        returns them; the features are the same bits either way.  resident=True returns the raw slots as zero-copy device views
        (J, NFEAT, ntrials, nsamples) instead of dicts (`utility_functions.features_from_slots`), and device views of the draws.
        Validation, seeds, trial sharding (each rank returns its block of trials) and what is not supported are those of
        `sample_posterior`.  No reference counterpart (the centre of mass as auditory_lfp/fit_mean_function.py:350-353 takes it of
        one field on the host)."""
        from .utility_functions import _region_labels, features_from_slots
        z2, tstar, code, sh = self._sample_posterior_args(z, tstar, type, nsamples)
        labels, J = _region_labels(labels, z2.shape[0], tstar.size)
        if band and not 0.0 <= float(floor) < 1.0:
            raise ValueError("floor must lie in [0, 1)")
        nsamples = int(nsamples)
        ctx = self._sync_device()
        hp, _keep = self._hparams(0.0)                     # no jitter, as predict
        R_local = self._local_lfp().shape[2]
        ctx.set_trial_offset(0 if sh is None else sh.local_slice(np.atleast_3d(self.lfp).shape[2]).start or 0)
        res = ctx.sample_features(hp, z2, tstar, code, nsamples, int(seed), R_local, labels, J, band=band, floor=floor,
                                  keep_draws=return_draws, resident=resident)
        feats = []
        for name in ("csd", "lfp"):
            f = res.get("feat_" + name)
            if f is not None and not resident:
                f = features_from_slots(f, (R_local, nsamples), tstar.reshape(-1).astype(np.float64), np.asarray(z2, dtype=np.float64), band)
            feats.append(f)
        if return_draws:
            return feats[0], feats[1], res.get("csd"), res.get("lfp")
        return feats[0], feats[1]

    def _sample_posterior_from_normals(self, z, tstar, type, xi, eps):
        """The affine map normals -> draws for host-supplied standard normals: xi (ntrials, nsamples, ns, ntt) with rows
        [CSD(z) if asked; LFP(z) if asked; LFP(x)] and columns [t*; t], eps (ntrials, nsamples, nx, nt).  For tests."""
        xi, eps = np.asarray(xi, dtype=np.float64), np.asarray(eps, dtype=np.float64)
        if xi.ndim != 4 or eps.ndim != 4 or xi.shape[:2] != eps.shape[:2]:
            raise ValueError("xi (ntrials, nsamples, ns, ntt) and eps (ntrials, nsamples, nx, nt) must share their first two axes")
        z2, tstar, code, sh = self._sample_posterior_args(z, tstar, type, xi.shape[1])
        nx, nt, R_local = self._local_lfp().shape
        ns = z2.shape[0] * (2 if type == "both" else 1) + nx
        if xi.shape != (R_local, xi.shape[1], ns, tstar.size + nt) or eps.shape[2:] != (nx, nt):
            raise ValueError("xi must be (%d, nsamples, %d, %d) and eps (%d, nsamples, %d, %d)"
                             % (R_local, ns, tstar.size + nt, R_local, nx, nt))
        return self._sample_posterior_call(z2, tstar, code, sh, xi.shape[1], 0, xi, eps, False)

    def _sample_prior_from_normals(self, normals, which):
        """Ls Z_r Lt^T on the GPU for host-supplied standard normals (nx, nt, ntrials)."""
        ctx = self._sync_device(need_lfp=False)
        hp, _keep = self._hparams(self.JITTER)
        return ctx.sample_prior(hp, which, normals)
