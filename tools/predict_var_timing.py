"""predict_var(..., resident=True) beside predict_at(..., resident=True) at the same sites and times, at the cfg2 (24 x 500 x 200)
and cfg3 (384 x 500 x 50) geometries: tstar = t, a 125-sample window and a 2x up-sample.  The variance reads no trial data, the
mean has two trial-sized products: the expectation this tool confirms or refutes is that the variance is the cheaper call.

One process, decomposition cache on (its default); every variant is warmed up, then the variants are timed in alternation (rounds)
and the median over the rounds of the fenced call time (host clock around a call that ends in a device synchronise) is reported.
A second, separate pass with fenced profiling scopes gives the time per launch of the variance's own products (gemm_var_G: G =
(M1 o M1) / D; gemm_var: the last product with the prior subtracted in its epilogue) and of the mean's last product.

    python tools/predict_var_timing.py [--rounds 200] [--warmup 5] [--type both] [--cfg cfg2 cfg3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--type", default="both", choices=("csd", "lfp", "both"))
    ap.add_argument("--cfg", nargs="+", default=["cfg2", "cfg3"])
    a = ap.parse_args()
    for name in a.cfg:
        w = W.workload(name)
        m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
        R = w["trials_per_gpu"]
        m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
        ctx = m._sync_device()
        t = np.asarray(w["t"], dtype=np.float64)
        nt, dt = t.shape[0], float(t[1, 0] - t[0, 0])
        z = w["x"]
        grids = [("t", t), ("window 125", t[187:312]), ("2x up-sample", (t[0, 0] + 0.5 * dt * np.arange(2 * nt))[:, None])]
        variants = []
        for label, ts in grids:
            variants.append(("predict_at(%s)" % label, label, ts.shape[0], lambda ts=ts: m.predict_at(z, ts, type=a.type, resident=True)))
            variants.append(("predict_var(%s)" % label, label, ts.shape[0], lambda ts=ts: m.predict_var(z, ts, type=a.type, resident=True)))
        times = {v[0]: [] for v in variants}
        for _, _, _, fn in variants:
            for _ in range(a.warmup):
                fn()
        ctx.synchronize()
        for _ in range(a.rounds):
            for label, _, _, fn in variants:
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                times[label].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in times.items()}
        # the products alone (fenced scopes serialise the call: not comparable with the times above)
        launches = {}
        ctx.prof_enable(1)
        for label, _, _, fn in variants:
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            launches[label] = {k: round(p[k]["ms"] / p[k]["count"], 4) for k in ("gemm_var_G", "gemm_var", "gemm_pred_at", "gemm_pred_Pc")
                               if p.get(k) and p[k]["count"]}
        ctx.prof_enable(0)
        for label, grid, nts, _ in variants:
            v = sorted(times[label])
            print(json.dumps({"cfg": name, "type": a.type, "variant": label, "nz": int(np.shape(z)[0]), "ntstar": nts, "ntrials": R,
                              "median_ms": round(1e3 * med[label], 4), "min_ms": round(1e3 * v[0], 4), "max_ms": round(1e3 * v[-1], 4),
                              "rounds": a.rounds, "ratio_to_predict_at": round(med[label] / med["predict_at(%s)" % grid], 4),
                              "ms_per_launch": launches[label]}), flush=True)


if __name__ == "__main__":
    main()
