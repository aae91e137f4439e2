"""The trial-shift objective on the device (gpcsd_shift_plan / gpcsd_shift_eval, utility_functions.trial_shift_objective,
fit_trial_shifts(jac=True)) against the default path of fit_trial_shifts (host interpolation, residuals over PCIe,
whitened_quadratic_forms, SciPy's finite differences), at

  small   24 x 150 x 200 trials, nseg = 12    the shape of the reference's auditory_lfp/fit_mean_function.py
  large   384 x 500 x 50 trials, nseg = 12    the cfg3 geometry

Per shape, one batch of B = min(ntrials, 128) points (one per trial, random shifts):

  f               trial_shift_objective(..., grad=False)
  f_and_g         trial_shift_objective(..., grad=True)
  whitened_quad   whitened_quadratic_forms on the SAME residuals, formed on the host beforehand: the device part of one default-path batch
                  (its (nx, nt, B) upload included, the host interpolation NOT included)
  host_resid      the host interpolation that forms those residuals (no device work): the rest of one default-path batch
  fit_jac         fit_trial_shifts(jac=True, return_evals=True): wall time, batches, points
  fit_default     fit_trial_shifts(return_evals=True): wall time, batches, points

The batch variants are warmed up and then timed INTERLEAVED (each round runs every variant once, in order); the median over the rounds
of the fenced call time (host clock around a call that ends in a device synchronise) is reported, and a second pass with fenced profiling
scopes gives the time per launch.  Synthetic data from a seed: smooth component bumps at distinct latencies, trials = mean(true_tau) +
noise with true_tau uniform in [-4, 4] samples.  Figures from one box compare as ratios only.

Every run is a child process of its own under its own time limit; after a child that times out or dies the tool starts no further one.

    python tools/trial_shift_timing.py [--shapes small large] [--rounds 20] [--warmup 3] [--maxiter N] [--limit 600]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"small": (24, 150, 200, 12), "large": (384, 500, 50, 12)}
LAUNCHES = ("shift_locate", "shift_resid", "gemm_shift_spatial", "gemm_shift_temporal", "shift_quad", "gemm_shift_temporal_back",
            "gemm_shift_spatial_back", "shift_grad", "gemm_wq_spatial", "gemm_wq_temporal", "relayout")


def problem(nx, nt, ntrials, nseg, seed=7):
    """(Qs, Qt, Dvec, lfp, mu, t, true_tau): a decomposition with the spectrum of two squared-exponential Gram matrices plus noise, nseg
    Gaussian bumps of 12 samples' width at latencies spread over the window, each with a smooth spatial profile, and shifted noisy trials."""
    from scipy.interpolate import interp1d
    rs = np.random.RandomState(seed)
    t = np.arange(float(nt))
    x = np.linspace(0.0, 1.0, nx)
    Qs = np.linalg.qr(rs.standard_normal((nx, nx)))[0]
    Qt = np.linalg.qr(rs.standard_normal((nt, nt)))[0]
    es, et = np.exp(-0.5 * np.arange(nx)) + 1e-6, 4.0 * np.exp(-0.1 * np.arange(nt)) + 1e-6
    Dvec = (es[:, None] * et[None, :] + 0.05).reshape(-1)
    mu = np.zeros((nx, nt, nseg + 1))
    mu[:, :, 0] = 0.1 * np.sin(2 * np.pi * x)[:, None] * np.cos(2 * np.pi * t / nt)[None, :]
    for i in range(nseg):
        lat = nt * (i + 1.0) / (nseg + 1.0)
        prof = np.exp(-0.5 * np.square((x - rs.uniform(0.2, 0.8)) / 0.15)) * rs.choice([-1.0, 1.0])
        mu[:, :, i + 1] = prof[:, None] * np.exp(-0.5 * np.square((t - lat) / 12.0))[None, :]
    true_tau = rs.uniform(-4.0, 4.0, (ntrials, nseg))
    lfp = np.empty((nx, nt, ntrials))
    fi = [interp1d(t, mu[:, :, i + 1], axis=1, fill_value="extrapolate") for i in range(nseg)]
    for j in range(ntrials):
        lfp[:, :, j] = mu[:, :, 0] + sum(fi[i](t + true_tau[j, i]) for i in range(nseg)) + 0.05 * rs.standard_normal((nx, nt))
    return Qs, Qt, Dvec, lfp, mu, t, true_tau


def host_residuals(lfp, mu, t, trials, taus):
    """What the default path of fit_trial_shifts forms on the host for one batch."""
    from scipy.interpolate import interp1d
    nseg = mu.shape[2] - 1
    fi = [interp1d(t, mu[:, :, i + 1], axis=1, fill_value="extrapolate") for i in range(nseg)]
    resid = np.empty(lfp.shape[:2] + (len(trials),))
    for b, (j, tau) in enumerate(zip(trials, taus)):
        m = np.array(mu[:, :, 0], copy=True)
        for i in range(nseg):
            m += fi[i](t + tau[i])
        resid[:, :, b] = lfp[:, :, j] - m
    return resid


def child_batch(shape, rounds, warmup):
    from gpcsd_amd import _hip, utility_functions as UF
    nx, nt, ntrials, nseg = SHAPES[shape]
    Qs, Qt, Dvec, lfp, mu, t, _ = problem(nx, nt, ntrials, nseg)
    ctx = _hip.default_context()
    obj = UF.trial_shift_objective(Qs, Qt, Dvec, lfp, mu, t)
    B = min(ntrials, 128)
    trials = np.arange(B)
    taus = np.random.RandomState(11).uniform(-4.0, 4.0, (B, nseg))
    resid = host_residuals(lfp, mu, t, trials, taus)
    variants = [("f", lambda: obj(trials, taus, grad=False)), ("f_and_g", lambda: obj(trials, taus)),
                ("whitened_quad", lambda: UF.whitened_quadratic_forms(Qs, Qt, Dvec, resid)),
                ("host_resid", lambda: host_residuals(lfp, mu, t, trials, taus))]
    f_dev = obj(trials, taus, grad=False)[0]
    f_host = 0.5 * UF.whitened_quadratic_forms(Qs, Qt, Dvec, resid) + 0.5 * np.sum(np.square(taus / 10.0), axis=1)
    agree = float(np.max(np.abs(f_dev - f_host) / np.abs(f_host)))
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    ctx.synchronize()
    times = {label: [] for label, _ in variants}
    for _ in range(rounds):
        for label, fn in variants:
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            times[label].append(time.perf_counter() - t0)
    launches = {}
    for label, fn in variants[:3]:
        ctx.prof_enable(1)
        ctx.prof_reset()
        for _ in range(3):
            fn()
        ctx.synchronize()
        p = ctx.prof_all()
        launches[label] = {k: round(p[k]["ms"] / p[k]["count"], 4) for k in LAUNCHES if p.get(k) and p[k]["count"]}
        ctx.prof_enable(0)
    base = statistics.median(times["whitened_quad"]) + statistics.median(times["host_resid"])
    for label, _ in variants:
        v = sorted(times[label])
        print(json.dumps({"shape": shape, "nx": nx, "nt": nt, "ntrials": ntrials, "nseg": nseg, "B": B, "variant": label,
                          "median_ms": round(1e3 * statistics.median(v), 4), "min_ms": round(1e3 * v[0], 4), "max_ms": round(1e3 * v[-1], 4),
                          "ratio_to_default_batch": round(statistics.median(v) / base, 5), "rounds": rounds,
                          "ms_per_launch": launches.get(label, {}), "f_device_vs_default_path_rel": agree}), flush=True)


def child_fit(shape, jac, maxiter):
    from gpcsd_amd import utility_functions as UF
    nx, nt, ntrials, nseg = SHAPES[shape]
    Qs, Qt, Dvec, lfp, mu, t, true_tau = problem(nx, nt, ntrials, nseg)
    UF.whitened_quadratic_forms(Qs, Qt, Dvec, lfp[:, :, :1])         # (context, code objects: not part of the fit's time)
    options = {"maxiter": maxiter} if maxiter else None
    t0 = time.perf_counter()
    tau_hat, ok, _, ev = UF.fit_trial_shifts(Qs, Qt, Dvec, lfp, mu, t, jac=jac, return_evals=True, options=options)
    wall = time.perf_counter() - t0
    print(json.dumps({"shape": shape, "nx": nx, "nt": nt, "ntrials": ntrials, "nseg": nseg, "variant": "fit_jac" if jac else "fit_default",
                      "maxiter": maxiter, "wall_s": round(wall, 3), "batches": ev["batches"], "points": ev["points"],
                      "converged": int(np.sum(ok)), "max_abs_tau_error": round(float(np.max(np.abs(tau_hat - true_tau))), 4),
                      "median_abs_tau_error": round(float(np.median(np.abs(tau_hat - true_tau))), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["small", "large"], choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=0, help="L-BFGS-B iteration cap of BOTH fits (0: SciPy's default)")
    ap.add_argument("--limit", type=int, default=600, help="seconds each child run may take")
    ap.add_argument("--runs", nargs="+", default=["batch", "fit_jac", "fit_default"], choices=["batch", "fit_jac", "fit_default"])
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "RUN"))
    a = ap.parse_args()
    if a.child:
        shape, run = a.child
        if run == "batch":
            child_batch(shape, a.rounds, a.warmup)
        else:
            child_fit(shape, run == "fit_jac", a.maxiter)
        return 0
    for shape in a.shapes:
        for run in a.runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, run, "--rounds", str(a.rounds), "--warmup", str(a.warmup),
                   "--maxiter", str(a.maxiter)]
            try:
                r = subprocess.run(cmd, cwd=ROOT, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps({"shape": shape, "run": run, "error": "time limit of %d s" % a.limit}), flush=True)
                return 124
            if r.returncode != 0:            # nothing more is started on a device a run may have faulted
                print(json.dumps({"shape": shape, "run": run, "error": "exit status %d" % r.returncode}), flush=True)
                return r.returncode if r.returncode > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
