"""region_features and sample_features at the cfg3 (384 x 500 x 50) and cfg2 (24 x 500 x 200) geometries, results resident:

  (a) region_features on resident draws of 8 per trial, the launches alone (fenced profiling scope "region_features": the slice
      pass and the fold) against the bytes of the field they read, and the fenced call; at 384 x 500 also the launches alone for
      M = 1, 50 and 400 columns of a host field -- the case for or against a second mapping when few columns leave lanes idle;
  (b) sample_features(return_draws=False) against sample_posterior(resident=True) with the same arguments, for 8 and for 64
      draws per trial: what the reduction adds to the sampler, and what the draws it does not keep would occupy;
  (c) the same features by the route there is without it: sample_posterior to the host, then NumPy.

The label map is a 4 x 4 grid of boxes that covers the whole (z, t) plane, so every byte of the field is read.  One process; every
variant is warmed up, then the variants are timed in alternation and the median over the rounds of the fenced call time (host clock
around a call that ends in a device synchronise) is reported.

    python tools/sample_features_timing.py [--rounds 5] [--warmup 1] [--type csd] [--cfg cfg3 cfg2] [--skip-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import workloads as W  # noqa: E402
from gpcsd_amd import utility_functions as UF  # noqa: E402


def boxes(nz, n, gz=4, gt=4):
    lab = np.zeros((nz, n), dtype=np.int32)
    for a, rows in enumerate(np.array_split(np.arange(nz), gz)):
        for b, cols in enumerate(np.array_split(np.arange(n), gt)):
            lab[np.ix_(rows, cols)] = 1 + a * gt + b
    return lab


def numpy_features(x, labels, tau, zeta):
    """The slots of region_features by NumPy on a host field (nz, n, M): what a user computes today."""
    nz, n = labels.shape
    flat, lab = x.reshape(nz * n, -1), labels.reshape(-1)
    out = []
    for j in range(1, int(labels.max()) + 1):
        pts = np.flatnonzero(lab == j)
        v = flat[pts]
        av = np.abs(v)
        out.append((v.max(0), pts[v.argmax(0)], v.min(0), pts[v.argmin(0)], v.sum(0), av.sum(0), tau[pts % n] @ av, zeta[pts // n, 0] @ av))
    return out


def median_ms(fns, ctx, rounds, warmup):
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ctx.synchronize()
    for _ in range(rounds):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            times[k].append(time.perf_counter() - t0)
    return {k: 1e3 * statistics.median(v) for k, v in times.items()}


def launches_ms(ctx, fn, reps=3):
    ctx.prof_enable(1)
    ctx.prof_reset()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    p = ctx.prof_all()
    ctx.prof_enable(0)
    return p["region_features"]["ms"] / p["region_features"]["count"], p["region_features"]["count"] // reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--type", default="csd", choices=("csd", "lfp"))
    ap.add_argument("--cfg", nargs="+", default=["cfg3", "cfg2"])
    ap.add_argument("--skip-host", action="store_true", help="leave out (c), the host route")
    a = ap.parse_args()
    which = 0 if a.type == "csd" else 1
    for name in a.cfg:
        w = W.workload(name)
        m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
        R = w["trials_per_gpu"]
        m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
        ctx = m._sync_device()
        t = np.asarray(w["t"], dtype=np.float64).reshape(-1)
        z = np.asarray(w["x"], dtype=np.float64)
        z2 = z.reshape(z.shape[0], -1)
        nz, n = z2.shape[0], t.size
        labels = boxes(nz, n)
        base = {"cfg": name, "type": a.type, "nz": nz, "ntstar": n, "ntrials": R, "J": int(labels.max())}
        copy = [ctx.hbm_copy_peak() for _ in range(3)]
        print(json.dumps(dict(base, measure="the box's copy rate (gpcsd_hbm_copy_peak, read + write), three repeats",
                              GB_per_s=[round(v, 1) for v in copy])), flush=True)

        # (a) the reduction alone, on resident draws of 8 per trial
        draws = m.sample_posterior(z, t, nsamples=8, type=a.type, seed=1, resident=True)[which]
        nbytes = 8.0 * nz * n * R * 8
        call = median_ms({"rf": lambda: UF.region_features(draws, labels, tstar=t, z=z2, resident=True)}, ctx, a.rounds, a.warmup)["rf"]
        ms, _ = launches_ms(ctx, lambda: UF.region_features(draws, labels, tstar=t, z=z2, resident=True))
        print(json.dumps(dict(base, measure="a: region_features on resident draws, 8 per trial", columns=R * 8, field_MB=round(nbytes / 1e6, 1),
                              launches_ms=round(ms, 4), read_TB_per_s=round(nbytes / ms / 1e9, 3), fenced_call_ms=round(call, 4))), flush=True)
        if name == "cfg3":
            rs = np.random.RandomState(0)
            for M in (1, 50, 400):
                x = rs.standard_normal((nz, n, M))
                ms, _ = launches_ms(ctx, lambda: ctx.region_features(x, labels, int(labels.max()), t, z2))
                print(json.dumps(dict(base, measure="a: launches alone by column count", columns=M, field_MB=round(x.nbytes / 1e6, 2),
                                      launches_ms=round(ms, 4), read_TB_per_s=round(x.nbytes / ms / 1e9, 3))), flush=True)
            del x

        # (b) inside the sampler against the sampler alone
        for S in (8, 64):
            fns = {"sample_posterior": lambda S=S: m.sample_posterior(z, t, nsamples=S, type=a.type, seed=1, resident=True),
                   "sample_features": lambda S=S: m.sample_features(z, t, labels, nsamples=S, type=a.type, seed=1, resident=True),
                   "sample_features(band)": lambda S=S: m.sample_features(z, t, labels, nsamples=S, type=a.type, seed=1, band=True, resident=True)}
            med = median_ms(fns, ctx, a.rounds, a.warmup)
            ms, launches = launches_ms(ctx, fns["sample_features"], reps=1)
            print(json.dumps(dict(base, measure="b: sample_features (no draws kept) against sample_posterior (resident)", nsamples=S,
                                  sample_posterior_ms=round(med["sample_posterior"], 3), sample_features_ms=round(med["sample_features"], 3),
                                  sample_features_band_ms=round(med["sample_features(band)"], 3),
                                  added_ms=round(med["sample_features"] - med["sample_posterior"], 3),
                                  ratio=round(med["sample_features"] / med["sample_posterior"], 4), chunks=launches,
                                  reduction_launches_ms=round(ms * launches, 3), draws_not_kept_MB=round(8.0 * nz * n * R * S / 1e6, 1),
                                  features_kept_MB=round(8.0 * int(labels.max()) * 10 * R * S / 1e6, 3))), flush=True)

        # (c) the route without it: the draws to the host, then NumPy
        if not a.skip_host:
            def host_route():
                d = m.sample_posterior(z, t, nsamples=8, type=a.type, seed=1)[which]
                return numpy_features(np.asarray(d), labels, t, z2)
            t0 = time.perf_counter()
            d = m.sample_posterior(z, t, nsamples=8, type=a.type, seed=1)[which]
            t1 = time.perf_counter()
            numpy_features(np.asarray(d), labels, t, z2)
            t2 = time.perf_counter()
            del d
            med = median_ms({"host": host_route, "device": lambda: m.sample_features(z, t, labels, nsamples=8, type=a.type, seed=1)}, ctx,
                            max(a.rounds // 2, 2), 1)
            print(json.dumps(dict(base, measure="c: sample_posterior to the host + NumPy against sample_features (host dicts)", nsamples=8,
                                  host_route_ms=round(med["host"], 2), of_which_draws_to_host_ms=round(1e3 * (t1 - t0), 2),
                                  of_which_numpy_ms=round(1e3 * (t2 - t1), 2), sample_features_ms=round(med["device"], 3),
                                  ratio=round(med["host"] / med["device"], 2))), flush=True)


if __name__ == "__main__":
    main()
