"""Time the kernel-CSD cross-validation scan (KCSD1D.cross_validate: bases, kernels, eigen-decompositions, the leave-one-out table,
argmin and the selected estimate, host arrays in and out) beside the dense float64 NumPy statement of the same scan (tests/kcsd_ref.py
with dtype=float64: the same two-panel rule, one explicit refit per held-out electrode and pair) on the same box.

  sim    the scan of simulation_studies/sim_from_gp_1D.py:114-115: 24 electrodes, 5 trials x 60 samples = 300 columns, 15 R x 25 lambda
  probe  384 electrodes x 25 000 columns, 15 R x 25 lambda (about 2.7 TF of fp64 in the table's product)

Device: the median over --rounds fenced calls (host clock around a call that returns host arrays) after --warmup calls, and, from a
separate pass with fenced profiling scopes, the time per launch family.  NumPy: the whole scan once for `sim`; for `probe` the refits
of --ref-electrodes held-out electrodes at one pair and the bases of one R are timed and scaled to the whole scan -- the line says
"extrapolated".  Neither ratio is a gate.

    python tools/kcsd_timing.py [--rounds 5] [--warmup 1] [--problem sim probe] [--ref-electrodes 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kcsd_ref as KR  # noqa: E402
from gpcsd_amd import _hip  # noqa: E402
from gpcsd_amd.kcsd import KCSD1D, DEFAULT_LAMBDAS  # noqa: E402

# gdx: the script's deltax / 20 for `sim`; one estimation point per electrode for `probe` (its estimate is 384 x 25 000 either way)
PROBLEMS = {"sim": dict(n=24, T=300, span=2300.0, h=100.0, gdx_div=20), "probe": dict(n=384, T=25000, span=3830.0, h=100.0, gdx_div=1)}
LAUNCHES = ("kcsd_basis", "kcsd_gram", "kcsd_project", "kcsd_diag", "kcsd_cv", "kcsd_fold", "kcsd_estimate")


def potentials(x, T, seed=0):
    rs = np.random.default_rng(seed)
    z = np.linspace(x.min(), x.max(), 200)
    csd = np.exp(-0.5 * ((z[:, None] - rs.uniform(x.min(), x.max(), 6)[None, :]) / 150.0) ** 2) @ rs.standard_normal((6, T))
    r = x[:, None] - z[None, :]
    V = (np.sqrt(r * r + 100.0 ** 2) - np.abs(r)) @ csd
    return V / V.std() + 0.01 * rs.standard_normal(V.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--problem", nargs="+", default=["sim", "probe"], choices=sorted(PROBLEMS))
    ap.add_argument("--ref-electrodes", type=int, default=2)
    a = ap.parse_args()
    ctx = _hip.default_context()
    Rs = np.linspace(100, 1000, 15)
    for name in a.problem:
        p = PROBLEMS[name]
        x = np.linspace(0.0, p["span"], p["n"])
        V = potentials(x, p["T"])
        m = KCSD1D(x, V, gdx=(x[1] - x[0]) / p["gdx_div"], h=p["h"])
        for _ in range(a.warmup):
            m.cross_validate(Rs=Rs)
        times = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            m.cross_validate(Rs=Rs)
            times.append(time.perf_counter() - t0)
        ctx.prof_enable(1)
        ctx.prof_reset()
        m.cross_validate(Rs=Rs)
        prof = ctx.prof_all()
        ctx.prof_enable(0)
        launches = {k: round(prof[k]["ms"], 3) for k in LAUNCHES if prof.get(k) and prof[k]["count"]}
        dev = statistics.median(times)
        # the NumPy statement in float64
        gx, gw = KR.gauss_legendre(m.ngl)
        npairs = Rs.size * DEFAULT_LAMBDAS.size
        with np.errstate(all="ignore"):
            if name == "sim":
                t0 = time.perf_counter()
                for R in Rs:
                    K, _ = KR.kernels(m.src_x, x, m.estm_x, R, p["h"], 1.0, gx, gw, dtype=np.float64)
                    for lam in DEFAULT_LAMBDAS:
                        try:
                            KR.cv_refit(K, V, lam, dtype=np.float64)
                        except np.linalg.LinAlgError:              # (an exactly singular refit: its time is spent all the same)
                            pass
                ref, how = time.perf_counter() - t0, "measured"
            else:
                t0 = time.perf_counter()
                K, _ = KR.kernels(m.src_x, x, m.estm_x, Rs[7], p["h"], 1.0, gx, gw, dtype=np.float64)
                t_basis = time.perf_counter() - t0
                ne = max(1, a.ref_electrodes)
                t0 = time.perf_counter()
                for i in range(ne):
                    keep = np.arange(p["n"]) != i
                    A = K[np.ix_(keep, keep)] + 1e-3 * np.eye(p["n"] - 1)
                    V[i] - K[i, keep] @ np.linalg.solve(A, V[keep])
                t_refit = (time.perf_counter() - t0) / ne
                ref, how = Rs.size * t_basis + npairs * p["n"] * t_refit, "extrapolated from %d refits and one R" % ne
        print(json.dumps({"problem": name, "n": p["n"], "T": p["T"], "nR": int(Rs.size), "nlam": int(DEFAULT_LAMBDAS.size),
                          "device_scan_s": round(dev, 5), "device_min_s": round(min(times), 5), "device_max_s": round(max(times), 5),
                          "rounds": a.rounds, "numpy_float64_refits_s": round(ref, 3), "numpy": how, "ratio": round(ref / dev, 1),
                          "selected": [m.R, m.lambd], "singular_pairs": int(m.cv_status.sum()), "ms_per_launch_family": launches}),
              flush=True)


if __name__ == "__main__":
    main()
