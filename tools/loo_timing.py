"""loo(resident=True) with and without the leave-one-out mean beside predict_at(x, t, resident=True) of one output kind, at the cfg2
(24 x 500 x 200) and cfg3 (384 x 500 x 50) geometries.  The last product of loo() has the flops of predict_at's on the electrodes
for one kind, so the expectation this tool confirms or refutes is that loo() lands near that call's time and loo(mean=False) below
it (its (nx, nt, ntrials) stores drop out).

One process, decomposition cache on (its default); every variant is warmed up, then the variants are timed in alternation (rounds)
and the median over the rounds of the fenced call time (host clock around a call that ends in a device synchronise) is reported.
Every timed call follows an untimed call of the same variant, so each is measured with both decompositions cached: loo() decomposes
Ks + JITTER I as loglik() does, predict_at() Ks itself, and a call that directly follows one of the other kind pays for a spatial
decomposition (at cfg3 about 0.5 ms) that the next call of its own kind does not.
A second, separate pass with fenced profiling scopes gives the time per launch: the two squared-operand products of diag(K^-1)
(gemm_var_H, gemm_var_c), the two projections (gemm_proj_spatial, gemm_pred_temporal_div), V = Qs Bm (gemm_loo_V), the fused last
product (gemm_loo) and its reduce (loo_reduce), beside predict_at's own last products.

    python tools/loo_timing.py [--rounds 100] [--warmup 5] [--type csd] [--cfg cfg2 cfg3]
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

LAUNCHES = ("gemm_var_H", "relayout", "gemm_var_c", "loo_var", "gemm_proj_spatial", "gemm_pred_temporal_div", "gemm_loo_V", "gemm_loo",
            "loo_reduce", "gemm_pred_cross", "gemm_pred_Pc", "gemm_pred_at")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--type", default="csd", choices=("csd", "lfp"))
    ap.add_argument("--cfg", nargs="+", default=["cfg2", "cfg3"])
    a = ap.parse_args()
    for name in a.cfg:
        w = W.workload(name)
        m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
        R = w["trials_per_gpu"]
        m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
        ctx = m._sync_device()
        t = np.asarray(w["t"], dtype=np.float64)
        z = w["x"]
        variants = [("predict_at(x, t)", lambda: m.predict_at(z, t, type=a.type, resident=True)),
                    ("loo(mean=True)", lambda: m.loo(mean=True, resident=True)),
                    ("loo(mean=False)", lambda: m.loo(mean=False, resident=True))]
        times = {v[0]: [] for v in variants}
        for _, fn in variants:
            for _ in range(a.warmup):
                fn()
        ctx.synchronize()
        for _ in range(a.rounds):
            for label, fn in variants:
                fn()                                   # untimed: this variant's decompositions are the cached ones
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                times[label].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in times.items()}
        # the launches alone (fenced scopes serialise the call: not comparable with the times above)
        launches = {}
        ctx.prof_enable(1)
        for label, fn in variants:
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            launches[label] = {k: round(p[k]["ms"] / p[k]["count"], 4) for k in LAUNCHES if p.get(k) and p[k]["count"]}
        ctx.prof_enable(0)
        for label, _ in variants:
            v = sorted(times[label])
            print(json.dumps({"cfg": name, "type": a.type, "variant": label, "nx": int(np.shape(z)[0]), "nt": int(t.shape[0]), "ntrials": R,
                              "median_ms": round(1e3 * med[label], 4), "min_ms": round(1e3 * v[0], 4), "max_ms": round(1e3 * v[-1], 4),
                              "rounds": a.rounds, "ratio_to_predict_at": round(med[label] / med["predict_at(x, t)"], 4),
                              "ms_per_launch": launches[label]}), flush=True)


if __name__ == "__main__":
    main()
