"""trial_scores(resident=True) and fisher_information() beside ONE fenced objective + gradient evaluation of the same build on the
same box, at the cfg2 (24 x 500 x 200) and cfg3 (384 x 500 x 50) geometries, with the decompositions cached and not cached.
Only RATIOS are reported: the absolute figure to hold them against is tools/grad_timing.py of the parent commit on the same box.

One process; every variant is warmed up, then the variants are timed in alternation (rounds) and the median over the rounds of
the fenced call time (host clock around a call that ends in a device synchronise) is taken.  "cached": every timed call follows an
untimed call of the same variant, so both decompositions come from the decomposition cache (the gradient has no cache: it always
decomposes).  "uncached": the cache is switched off, so the score and information calls decompose as well -- the like-for-like
comparison with the gradient.  A second pass with fenced profiling scopes gives the time per launch of the new kernels.

    python tools/fisher_timing.py [--rounds 50] [--warmup 5] [--cfg cfg2 cfg3]
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

LAUNCHES = ("fisher_score_spatial", "fisher_score_temporal", "fisher_pairs", "fisher_diag", "gemm_fisher_rotate", "gemm_fisher_M",
            "gemm_fisher_N", "gemm_proj_spatial", "gemm_pred_temporal_div")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cfg", nargs="+", default=["cfg2", "cfg3"])
    a = ap.parse_args()
    for name in a.cfg:
        w = W.workload(name)
        m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
        R = w["trials_per_gpu"]
        m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
        ctx = m._sync_device()
        variants = [("objective + gradient", lambda: m._loglik_and_grad_natural()),
                    ("trial_scores(resident=True)", lambda: m.trial_scores(resident=True)),
                    ("fisher_information()", lambda: m.fisher_information())]
        for cached in (True, False):
            ctx.decomposition_cache(cached)
            times = {v[0]: [] for v in variants}
            for _, fn in variants:
                for _ in range(a.warmup):
                    fn()
            ctx.synchronize()
            for _ in range(a.rounds):
                for label, fn in variants:
                    fn()                               # untimed: with the cache on, this variant's decompositions are the cached ones
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ctx.synchronize()
                    times[label].append(time.perf_counter() - t0)
            med = {k: statistics.median(v) for k, v in times.items()}
            base = med["objective + gradient"]
            for label, _ in variants[1:]:
                v = sorted(times[label])
                print(json.dumps({"cfg": name, "nx": w["nx"], "nt": w["nt"], "ntrials": R, "decompositions": "cached" if cached else "uncached",
                                  "variant": label, "ratio_to_gradient": round(med[label] / base, 4),
                                  "ratio_min": round(v[0] / base, 4), "ratio_max": round(v[-1] / base, 4), "rounds": a.rounds}), flush=True)
        ctx.decomposition_cache(True)
        # the launches alone, as shares of the call's fenced launches (fenced scopes serialise the call)
        ctx.prof_enable(1)
        for label, fn in variants[1:]:
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            tot = sum(e["ms"] for e in p.values() if e["count"])
            print(json.dumps({"cfg": name, "variant": label, "share_of_fenced_launch_time":
                              {k: round(p[k]["ms"] / tot, 4) for k in LAUNCHES if p.get(k) and p[k]["count"]}}), flush=True)
        ctx.prof_enable(0)


if __name__ == "__main__":
    main()
