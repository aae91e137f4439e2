"""predict_masked(z = x, t* = t, resident=True) beside predict_at(..., resident=True) at the same sites and times, at the cfg3
geometry (384 x 500 x 50), for three masks:

  scattered   1 % of the samples missing at random in every trial (m ~ 1920 per trial, 50 distinct masks)
  window      a 20-sample window over all electrodes in 10 of the 50 trials (m = 7680; one window per trial, 10 distinct masks)
  electrode   one dead electrode as a 2-D mask (m = 500, one mask for all trials)

One process, decomposition cache on (its default); every call is warmed up, then the calls are timed in alternation (rounds); the
median over the rounds of the fenced call time (host clock around a call that ends in a device synchronise) is reported with its
ratio to predict_at.  A second, separate pass with fenced profiling scopes gives the split of a masked call: front (zero-fill, the
two projections and the back-projection of all trials), G (the H_a products and the grouped product), solve (Cholesky factor, the
two triangular solves, gather and scatter), update (the projection of the imputed values) and tail (the cross products of
predict_at).  Fenced scopes serialise the call: the split is a split, not comparable with the times above.

    python tools/predict_masked_timing.py [--rounds 5] [--warmup 1] [--type csd] [--masks scattered window electrode]
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

SCOPES = ("masked_front", "masked_G", "masked_solve", "masked_update", "masked_tail", "gemm_masked_H", "masked_gram", "potrf", "trsm",
          "trsm_trans")


def masks(nx, nt, R, seed=7):
    rng = np.random.RandomState(seed)
    scattered = rng.random_sample((nx, nt, R)) >= 0.01
    window = np.ones((nx, nt, R), dtype=bool)
    for r in rng.permutation(R)[:10]:
        t0 = int(rng.randint(nt - 20))
        window[:, t0:t0 + 20, r] = False
    electrode = np.ones((nx, nt), dtype=bool)
    electrode[int(rng.randint(nx)), :] = False
    return {"scattered": scattered, "window": window, "electrode": electrode}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--type", default="csd", choices=("csd", "lfp", "both"))
    ap.add_argument("--masks", nargs="+", default=["scattered", "window", "electrode"])
    a = ap.parse_args()
    w = W.workload("cfg3")
    m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
    R = w["trials_per_gpu"]
    m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
    ctx = m._sync_device()
    t = np.asarray(w["t"], dtype=np.float64)
    z = w["x"]
    mk = masks(w["nx"], w["nt"], R)
    variants = [("predict_at", lambda: m.predict_at(z, t, type=a.type, resident=True))]
    variants += [(k, lambda k=k: m.predict_masked(z, t, mk[k], type=a.type, resident=True)) for k in a.masks]
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
    split = {}
    ctx.prof_enable(1)
    for label, fn in variants:
        ctx.prof_reset()
        fn()
        ctx.synchronize()
        p = ctx.prof_all()
        split[label] = {k: [round(p[k]["ms"], 3), p[k]["count"]] for k in SCOPES if p.get(k) and p[k]["count"]}
    ctx.prof_enable(0)
    for label, _ in variants:
        v = sorted(times[label])
        miss = None
        if label in mk:
            m3 = mk[label] if mk[label].ndim == 3 else mk[label][:, :, None]
            per = (~m3).reshape(-1, m3.shape[2]).sum(0)
            miss = {"missing_per_trial_max": int(per.max()), "trials_with_missing": int((per > 0).sum()) if m3.shape[2] > 1 else R}
        print(json.dumps({"cfg": "cfg3", "type": a.type, "variant": label, "nz": int(np.shape(z)[0]), "ntstar": int(t.shape[0]),
                          "ntrials": R, "mask": miss, "median_ms": round(1e3 * med[label], 3), "min_ms": round(1e3 * v[0], 3),
                          "max_ms": round(1e3 * v[-1], 3), "rounds": a.rounds, "ratio_to_predict_at": round(med[label] / med["predict_at"], 2),
                          "fenced_ms_and_launches": split[label]}), flush=True)


if __name__ == "__main__":
    main()
