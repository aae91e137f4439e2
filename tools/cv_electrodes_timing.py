"""cv_electrodes(resident=True) beside loo(resident=True) and beside ONE predict_masked call with a single dead electrode, at the cfg2
(24 x 500 x 200) and cfg3 (384 x 500 x 50) geometries: folds=None (one fold per electrode), folds=24 at cfg3 (16 electrodes per
fold; at cfg2 folds=2, 12 per fold) and mean=False.  In the temporal eigen-basis every fold is block diagonal, so the expectation
this tool confirms or refutes is that ALL folds together cost about one loo(), where the dense route costs one predict_masked call
per fold.

One process, decomposition cache on (its default); every variant is warmed up, then the variants are timed in alternation (rounds)
and the median over the rounds of the fenced call time (host clock around a call that ends in a device synchronise) is reported.
Every timed call follows an untimed call of the same variant, so each is measured with both decompositions cached (loo and
cv_electrodes decompose Ks + JITTER I, predict_masked Ks itself).  A second, separate pass with fenced profiling scopes gives the
time per launch of the cv_electrodes variants.  One box: compare ratios only.

    python tools/cv_electrodes_timing.py [--rounds 30] [--warmup 3] [--cfg cfg2 cfg3]
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

LAUNCHES = ("gemm_proj_spatial", "gemm_pred_temporal_div", "gemm_loo_V", "gemm_var_Gp", "efold_solve", "relayout", "gemm_var_cv",
            "gemm_loo", "loo_reduce", "gemm_var_H", "gemm_var_c")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
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
        nx = int(np.shape(z)[0])
        k16 = -(-nx // 16)
        dead = np.ones((nx, t.shape[0]), dtype=bool)
        dead[nx // 2] = False                                  # one dead electrode: the dense route's cost PER FOLD
        variants = [("loo(mean=True)", lambda: m.loo(mean=True, resident=True)),
                    ("cv_electrodes(folds=None)", lambda: m.cv_electrodes(resident=True)),
                    ("cv_electrodes(folds=None, mean=False)", lambda: m.cv_electrodes(mean=False, resident=True)),
                    ("cv_electrodes(folds=%d)" % k16, lambda: m.cv_electrodes(folds=k16, resident=True)),
                    ("cv_electrodes(folds=%d, mean=False)" % k16, lambda: m.cv_electrodes(folds=k16, mean=False, resident=True)),
                    ("predict_masked(one dead electrode)", lambda: m.predict_masked(z, t, dead, type="lfp", resident=True))]
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
        for label, fn in variants[:-1]:
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            launches[label] = {k: round(p[k]["ms"] / p[k]["count"], 4) for k in LAUNCHES if p.get(k) and p[k]["count"]}
        ctx.prof_enable(0)
        for label, _ in variants:
            v = sorted(times[label])
            print(json.dumps({"cfg": name, "variant": label, "nx": nx, "nt": int(t.shape[0]), "ntrials": R,
                              "median_ms": round(1e3 * med[label], 4), "min_ms": round(1e3 * v[0], 4), "max_ms": round(1e3 * v[-1], 4),
                              "rounds": a.rounds, "ratio_to_loo": round(med[label] / med["loo(mean=True)"], 4),
                              "ratio_to_one_predict_masked": round(med[label] / med["predict_masked(one dead electrode)"], 4),
                              "ms_per_launch": launches.get(label, {})}), flush=True)


if __name__ == "__main__":
    main()
