"""sample_posterior(z = x, t* = t, nsamples = 1 and 8, resident=True) beside predict_at(..., resident=True) at the same sites and
times, at the cfg2 (24 x 500 x 200) and cfg3 (384 x 500 x 50) geometries, and the device generator alone against the streaming copy
peak.  The two joint eigen-decompositions are paid once per call, the rest per draw: the two sample counts separate them.

One process, decomposition cache on (its default); both calls are warmed up, then timed in alternation (rounds); the median over
the rounds of the fenced call time (host clock around a call that ends in a device synchronise) is reported.  A second, separate
pass with fenced profiling scopes gives the time per launch of the draw's own kernels.  The generator is timed on the device
(events around launches that write a device buffer; nothing is copied out) in GB/s of normals WRITTEN; gpcsd_hbm_copy_peak counts
reads and writes, so the store-bound ceiling of the generator is half of it.

    python tools/sample_posterior_timing.py [--rounds 30] [--warmup 3] [--type csd] [--cfg cfg2 cfg3] [--nsamples 1 8]
    python tools/sample_posterior_timing.py --generator-only [--count 134217728]     (a run a counter profile can wrap)
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
from gpcsd_amd import _hip  # noqa: E402

SCOPES = ("rng_normals", "gemm_sample_temporal", "gemm_sample_spatial", "gemm_sample_noise", "sample_residual", "gemm_proj_spatial",
          "gemm_pred_temporal_div", "gemm_pred_cross", "gemm_pred_at", "sample_combine", "eigh_sample_joint")


def generator(count, reps):
    ctx = _hip.Context()
    ctx.normals_bench(count, 2)                            # warm-up: code object, buffer
    gen = [ctx.normals_bench(count, reps) for _ in range(3)]
    peak = [ctx.hbm_copy_peak(1 << 30) for _ in range(3)]
    print(json.dumps({"generator": "philox4x32-10 + box-muller fp64", "normals": count, "reps": reps,
                      "normals_GBs_written": [round(g, 1) for g in gen], "hbm_copy_peak_GBs_read_plus_write": [round(p, 1) for p in peak],
                      "share_of_store_ceiling": round(statistics.median(gen) / (0.5 * statistics.median(peak)), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--type", default="csd", choices=("csd", "lfp", "both"))
    ap.add_argument("--cfg", nargs="+", default=["cfg2", "cfg3"])
    ap.add_argument("--nsamples", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--count", type=int, default=1 << 27)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--generator-only", action="store_true")
    a = ap.parse_args()
    generator(a.count, a.reps)
    if a.generator_only:
        return
    for name in a.cfg:
        w = W.workload(name)
        m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
        R = w["trials_per_gpu"]
        m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
        ctx = m._sync_device()
        t = np.asarray(w["t"], dtype=np.float64)
        z = w["x"]
        seed = [0]

        def draw(S):
            seed[0] += 1
            m.sample_posterior(z, t, nsamples=S, type=a.type, seed=seed[0], resident=True)

        variants = [("predict_at", lambda: m.predict_at(z, t, type=a.type, resident=True))]
        variants += [("sample_posterior(nsamples=%d)" % S, lambda S=S: draw(S)) for S in a.nsamples]
        times = {k: [] for k, _ in variants}
        for _, fn in variants:
            for _ in range(a.warmup):
                fn()
        ctx.synchronize()
        for _ in range(a.rounds):
            for label, fn in variants:
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                times[label].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in times.items()}
        launches = {}
        ctx.prof_enable(1)
        for label, fn in variants:                         # (fenced scopes serialise the call: not comparable with the times above)
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            launches[label] = {k: [round(p[k]["ms"] / 3, 4), p[k]["count"] // 3] for k in SCOPES if p.get(k) and p[k]["count"]}
        ctx.prof_enable(0)
        nq = 2 if a.type == "both" else 1
        for label, _ in variants:
            v = sorted(times[label])
            print(json.dumps({"cfg": name, "type": a.type, "variant": label, "nz": int(np.shape(z)[0]), "ntstar": int(t.shape[0]),
                              "ntrials": R, "joint_orders": [nq * int(np.shape(z)[0]) + w["nx"], 2 * int(t.shape[0])],
                              "median_ms": round(1e3 * med[label], 4), "min_ms": round(1e3 * v[0], 4), "max_ms": round(1e3 * v[-1], 4),
                              "rounds": a.rounds, "ratio_to_predict_at": round(med[label] / med["predict_at"], 4),
                              "ms_and_launches_per_call": launches[label]}), flush=True)


if __name__ == "__main__":
    main()
