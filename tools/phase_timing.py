"""Band phase and PLV of a resident prediction (gpcsd_analytic_resident, gpcsd_plv_resident) beside predict_at(x, t, resident=True),
at the cfg2 (24 x 500 x 200) and cfg3 (384 x 500 x 50) geometries, everything left in HBM.

  analytic, all times kept   the flops of predict_at's last product for one output kind (2 x 2 nz nt^2 R: real and imaginary part),
                             with all four outputs stored and with the phase alone; compared per launch with gemm_pred_at
  analytic, two times kept   against the HBM time of reading the source once
  plv, all times / two       against its flop count (4 nz^2 R per kept time: four real products on the lower triangle) at the fp64 MFMA peak
  end to end                 predict_at + phase + plv (two times) on the device, against the PCIe time of fetching the prediction

One process; every variant is warmed up, then the variants are timed in alternation (rounds) and the median over the rounds of the
fenced call time (host clock around a call that ends in a device synchronise) is reported.  A second, separate pass with fenced
profiling scopes gives the time per launch ("analytic", "plv", "gemm_pred_at").

    python tools/phase_timing.py [--rounds 30] [--warmup 3] [--type csd] [--cfg cfg2 cfg3]
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

LAUNCHES = ("analytic", "plv", "gemm_pred_at")
MFMA_F64_PEAK = 78.6e12          # the measured fp64 MFMA rate of the chip


def main():
    import scipy.signal
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
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
        nz, nt = int(np.shape(z)[0]), int(t.shape[0])
        sos = scipy.signal.butter(1, (0.05, 0.15), btype="bandpass", output="sos")
        at = (nt // 3, (2 * nt) // 3)
        A_all, A_two = UF.analytic_operator(nt, sos=sos), UF.analytic_operator(nt, sos=sos, at=at)
        src, shape = "pred_out_" + a.type, (nz, nt, R)
        all4 = ("phase", "amp", "u_re", "u_im")
        m.predict_at(z, t, type=a.type, resident=True)
        hbm = ctx.hbm_copy_peak()                          # GB/s of a device copy, reads and writes counted

        def e2e():
            m.predict_at(z, t, type=a.type, resident=True)
            m.phase(A_two, type=a.type, at=at)
            m.plv(type=a.type)

        def plv_of(A):                                     # the phasors of A first (untimed by the per-launch pass: "plv" alone)
            ctx.analytic_resident(src, 0, shape, A, ("u_re", "u_im"))
            return lambda: ctx.plv_resident(nz, A.shape[0], R, 1)

        variants = [("predict_at(x, t)", lambda: m.predict_at(z, t, type=a.type, resident=True), None),
                    ("analytic all times, four outputs", lambda: ctx.analytic_resident(src, 0, shape, A_all, all4), None),
                    ("analytic all times, phase only", lambda: ctx.analytic_resident(src, 0, shape, A_all, ("phase",)), None),
                    ("analytic two times, four outputs", lambda: ctx.analytic_resident(src, 0, shape, A_two, all4), None),
                    ("plv all times", None, A_all), ("plv two times", None, A_two),
                    ("predict_at + phase + plv, two times", e2e, None),
                    ("fetch the prediction (PCIe)", lambda: ctx.fetch(src, shape), None)]
        times, launches = {}, {}
        for label, fn, A in variants:                      # (the PLV variants need their phasors in place: timed one after the other)
            if fn is None:
                fn = plv_of(A)
            for _ in range(a.warmup):
                fn()
            ctx.synchronize()
            ts = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                ts.append(time.perf_counter() - t0)
            times[label] = ts
            ctx.prof_enable(1)
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            launches[label] = {k: round(p[k]["ms"] / p[k]["count"], 4) for k in LAUNCHES if p.get(k) and p[k]["count"]}
            ctx.prof_enable(0)
        flops = {"analytic all times, four outputs": 4.0 * nz * R * nt * nt, "analytic all times, phase only": 4.0 * nz * R * nt * nt,
                 "analytic two times, four outputs": 4.0 * nz * R * nt * 2, "plv all times": 4.0 * nz * nz * R * nt,
                 "plv two times": 4.0 * nz * nz * R * 2, "predict_at(x, t)": 2.0 * nz * R * nt * nt * len(m.temporal_cov_list)}
        for label, _, _ in variants:
            v = sorted(times[label])
            rec = {"cfg": name, "type": a.type, "variant": label, "nz": nz, "nt": nt, "ntrials": R,
                   "median_ms": round(1e3 * statistics.median(v), 4), "min_ms": round(1e3 * v[0], 4), "max_ms": round(1e3 * v[-1], 4),
                   "rounds": a.rounds, "ms_per_launch": launches[label]}
            if label in flops:
                rec["gflop_of_last_product"] = round(flops[label] / 1e9, 3)
                rec["ms_at_mfma_peak"] = round(1e3 * flops[label] / MFMA_F64_PEAK, 4)
            if label.startswith("analytic two"):
                rec["ms_to_read_source_at_hbm_copy_rate"] = round(1e3 * 8.0 * nz * nt * R / (1e9 * hbm), 4)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
