"""Power spectrum and coherence of a resident prediction (gpcsd_power_spectrum_resident, gpcsd_cross_spectrum_resident) at the cfg3
geometry (384 x 500 x 50; cfg2 on request), everything left in HBM.

  power spectrum, all one-sided rows    psd only: the (nz, nf) result is all that is stored
  band_phase(want=("amp",)), same rows  the existing launch of the SAME operator and field: the same flops (2 x 2 nz nt nf R), but it
                                        stores every per-trial modulus (nz nf R doubles)
  coherence at 2 and at 26 rows         the coefficients of those rows (power kernel), then the cross-spectral matrix (plv kernel) and
                                        the coherence of all site pairs
  fetch the prediction (PCIe)           what a host-side periodogram would have to move first

One process; every variant is warmed up, then the variants are timed INTERLEAVED (each round runs every variant once, in order) and the
median over the rounds of the fenced call time (host clock around a call that ends in a device synchronise) is reported.  A second,
separate pass with fenced profiling scopes gives the time per launch ("power", "analytic", "plv", "coherence").  Figures from one box
compare as ratios only.

    python tools/spectrum_timing.py [--rounds 30] [--warmup 3] [--type csd] [--cfg cfg3]
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

LAUNCHES = ("power", "analytic", "plv", "coherence")
MFMA_F64_PEAK = 78.6e12          # the measured fp64 MFMA rate of the chip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--type", default="csd", choices=("csd", "lfp"))
    ap.add_argument("--cfg", nargs="+", default=["cfg3"])
    a = ap.parse_args()
    for name in a.cfg:
        w = W.workload(name)
        m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
        R = w["trials_per_gpu"]
        m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
        ctx = m._sync_device()
        t = np.asarray(w["t"], dtype=np.float64)
        z = w["x"]
        nz, nt = int(np.shape(z)[0]), int(t.shape[0])
        f, A_all = UF.spectral_operator(nt, fs=1.0)
        nf = A_all.shape[0]
        A_2 = UF.spectral_operator(nt, fs=1.0, rows=[nf // 10, nf // 5])[1]
        A_26 = UF.spectral_operator(nt, fs=1.0, rows=list(range(2, 28)))[1]
        src, shape3, shape4 = "pred_out_" + a.type, (nz, nt, R), (nz, nt, R, 1)
        m.predict_at(z, t, type=a.type, resident=True)

        def coherence_of(A):
            def run():
                ctx.power_spectrum_resident(src, 0, shape4, A, ("re", "im"))
                ctx.cross_spectrum_resident(nz, A.shape[0], R, 1)
            return run

        variants = [("power spectrum, all rows, psd only", lambda: ctx.power_spectrum_resident(src, 0, shape4, A_all)),
                    ("band_phase amp only, same operator", lambda: ctx.analytic_resident(src, 0, shape3, A_all, ("amp",))),
                    ("power spectrum, all rows, psd + per-trial power", lambda: ctx.power_spectrum_resident(src, 0, shape4, A_all, ("power",))),
                    ("coherence, 2 rows", coherence_of(A_2)),
                    ("coherence, 26 rows", coherence_of(A_26)),
                    ("fetch the prediction (PCIe)", lambda: ctx.fetch(src, shape3))]
        for _, fn in variants:
            for _ in range(a.warmup):
                fn()
        ctx.synchronize()
        times = {label: [] for label, _ in variants}
        for _ in range(a.rounds):
            for label, fn in variants:
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                times[label].append(time.perf_counter() - t0)
        launches = {}
        for label, fn in variants:
            ctx.prof_enable(1)
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            launches[label] = {k: round(p[k]["ms"] / p[k]["count"], 4) for k in LAUNCHES if p.get(k) and p[k]["count"]}
            ctx.prof_enable(0)
        flops = {"power spectrum, all rows, psd only": 4.0 * nz * R * nt * nf, "band_phase amp only, same operator": 4.0 * nz * R * nt * nf,
                 "power spectrum, all rows, psd + per-trial power": 4.0 * nz * R * nt * nf,
                 "coherence, 2 rows": 4.0 * nz * R * 2 * (nt + nz), "coherence, 26 rows": 4.0 * nz * R * 26 * (nt + nz)}
        base = statistics.median(times["band_phase amp only, same operator"])
        for label, _ in variants:
            v = sorted(times[label])
            rec = {"cfg": name, "type": a.type, "variant": label, "nz": nz, "nt": nt, "nf": nf, "ntrials": R,
                   "median_ms": round(1e3 * statistics.median(v), 4), "min_ms": round(1e3 * v[0], 4), "max_ms": round(1e3 * v[-1], 4),
                   "ratio_to_band_phase_amp": round(statistics.median(v) / base, 4), "rounds": a.rounds, "ms_per_launch": launches[label]}
            if label in flops:
                rec["gflop"] = round(flops[label] / 1e9, 3)
                rec["ms_at_mfma_peak"] = round(1e3 * flops[label] / MFMA_F64_PEAK, 4)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
