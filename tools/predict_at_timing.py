"""predict_at(..., resident=True) at the cfg2 (24 x 500 x 200) and cfg3 (384 x 500 x 50) geometries: tstar = t, a 125-sample
window and a 2x up-sample, beside predict(..., resident=True) with the folded products off (the unfolded path: the same flops).

One process; every variant is warmed up, then the variants are timed in alternation (rounds) and the median over the rounds of
the fenced call time (host clock around a call that ends in a device synchronise) is reported.  A second, separate pass with
fenced profiling scopes gives the time of the last product alone: gemm_pred_at against gemm_pred_tstar + relayout.

    python tools/predict_at_timing.py [--rounds 200] [--warmup 5] [--type csd] [--cfg cfg2 cfg3]
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
    ap.add_argument("--type", default="csd", choices=("csd", "lfp", "both"))
    ap.add_argument("--cfg", nargs="+", default=["cfg2", "cfg3"])
    a = ap.parse_args()
    for name in a.cfg:
        w = W.workload(name)
        m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
        R = w["trials_per_gpu"]
        m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
        ctx = m._sync_device()
        ctx.fold_gemm(False)                    # predict's unfolded products: the baseline with the flops of predict_at(t)
        t = np.asarray(w["t"], dtype=np.float64)
        nt, dt = t.shape[0], float(t[1, 0] - t[0, 0])
        z = w["x"]
        variants = [
            ("predict(t) unfolded", nt, lambda: m.predict(z, t, type=a.type, resident=True)),
            ("predict_at(t)", nt, lambda: m.predict_at(z, t, type=a.type, resident=True)),
            ("predict_at(window 125)", 125, lambda tw=t[187:312]: m.predict_at(z, tw, type=a.type, resident=True)),
            ("predict_at(2x up-sample)", 2 * nt,
             lambda tu=(t[0, 0] + 0.5 * dt * np.arange(2 * nt))[:, None]: m.predict_at(z, tu, type=a.type, resident=True)),
        ]
        times = {v[0]: [] for v in variants}
        for label, _, fn in variants:
            for _ in range(a.warmup):
                fn()
        ctx.synchronize()
        for _ in range(a.rounds):
            for label, _, fn in variants:
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                times[label].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in times.items()}
        # the last product alone (fenced scopes serialise the call: not comparable with the times above)
        last = {}
        ctx.prof_enable(1)
        for label, _, fn in variants:
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            last[label] = {k: round(p[k]["ms"] / p[k]["count"], 4) for k in ("gemm_pred_at", "gemm_pred_tstar", "relayout")
                           if p.get(k) and p[k]["count"]}
        ctx.prof_enable(0)
        base = med["predict(t) unfolded"]
        for label, nts, _ in variants:
            v = sorted(times[label])
            print(json.dumps({"cfg": name, "type": a.type, "variant": label, "ntstar": nts, "median_ms": round(1e3 * med[label], 4),
                              "min_ms": round(1e3 * v[0], 4), "max_ms": round(1e3 * v[-1], 4), "rounds": a.rounds,
                              "ratio_to_unfolded_predict": round(med[label] / base, 4),
                              "last_product_ms_per_launch": last[label], "trials_per_s": round(R / med[label], 1)}))


if __name__ == "__main__":
    main()
