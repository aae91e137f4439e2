"""Torus graph fit with bootstrap (gpcsd_torus_graph) at the two shapes the reference's analyses fit:

  auditory     d = 48 nodes (two probes of 24 sites), B = 100 replicates, N = 2000 trials -- N is a STAND-IN: the data set is not part
               of this repository (auditory_lfp/torus_graph_fit.py reads it from disk)
  neuropixels  d = 8, N = 129, B = 1000 (neuropixels/fit_torus_graph.py)

on synthetic phases (von Mises noise per node around a common per-trial phase).  Reported per shape, one JSON line each:

  per launch (fenced profiling scopes): the node-Gram kernel against its flops (d B nv (nv + 1) N, nv = 2 d - 1: the lower triangles)
      at the 78.6 TF/s fp64 MFMA peak, and per (node, replicate) product against one gpcsd_gemm launch of the same M = N = nv, K = N;
  the factorisation share: potrf + pivot check ("tg_factor") of the whole call's device time per replicate;
  the whole call per replicate (host clock around the fenced call, median over the rounds, inference off), and one call with the
      inference for replicate 0;
  the float64 NumPy statement of the estimator (dense D per trial, accumulated in chunks of trials, numpy.linalg.solve), one replicate.

    python tools/torus_graph_timing.py [--rounds 5] [--shape auditory neuropixels]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpcsd_amd import _hip  # noqa: E402

MFMA_F64_PEAK = 78.6e12          # the measured fp64 MFMA rate of the chip
SHAPES = {"auditory": (48, 2000, 100), "neuropixels": (8, 129, 1000)}
LAUNCHES = ("tg_node_gram", "tg_assemble", "tg_factor", "potrf", "trsm", "trsm_trans", "tg_inference")


def numpy_fit(u_re, u_im, w, chunk=50):
    """Gamma, H, phi of one replicate in float64 from the dense per-trial Jacobian (the statement of tests/torus_ref.py)."""
    d, N = u_re.shape
    i, j = np.triu_indices(d, 1)
    P = i.size
    p = np.arange(P)
    Gamma, H = np.zeros((2 * P, 2 * P)), np.zeros(2 * P)
    for n0 in range(0, N, chunk):
        sl = slice(n0, min(N, n0 + chunk))
        re, im, ww = u_re[:, sl], u_im[:, sl], w[sl]
        c = (re[i] * re[j] + im[i] * im[j]).T
        s = (im[i] * re[j] - re[i] * im[j]).T
        D = np.zeros((c.shape[0], 2 * P, d))
        D[:, 2 * p, i], D[:, 2 * p, j], D[:, 2 * p + 1, i], D[:, 2 * p + 1, j] = -s, s, c, -c
        A = D.transpose(0, 2, 1).reshape(-1, 2 * P)
        Gamma += (A * np.repeat(ww, d)[:, None]).T @ A
        H[0::2] += ww @ c
        H[1::2] += ww @ s
    W = w.sum()
    return np.linalg.solve(Gamma / W, 2 * H / W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", nargs="+", default=list(SHAPES))
    a = ap.parse_args()
    ctx = _hip.Context()
    for name in a.shape:
        d, N, B = SHAPES[name]
        rng = np.random.default_rng(0)
        x = rng.vonmises(0, 1, (d, N)) + rng.vonmises(0, 2, N)
        u_re, u_im = np.cos(x), np.sin(x)
        w = np.concatenate([np.ones((1, N)), rng.multinomial(N, [1.0 / N] * N, size=B - 1).astype(np.float64)])
        nv, m = 2 * d - 1, d * (d - 1)
        boot = lambda: ctx.torus_graph(u_re, u_im, weights=w, inference=False)
        res = boot()
        ctx.synchronize()
        ts = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            boot()
            ctx.synchronize()
            ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ctx.torus_graph(u_re, u_im, inference=True)
        ctx.synchronize()
        t_inf = time.perf_counter() - t0
        ctx.prof_enable(1)
        ctx.prof_reset()
        boot()
        ctx.synchronize()
        p = ctx.prof_all()
        ctx.prof_reset()
        ctx.gemm(np.ones((nv, N)), np.ones((nv, N)), transB=True)
        ctx.synchronize()
        pg = ctx.prof_all()
        ctx.prof_enable(0)
        per = {k: {"ms_total": round(p[k]["ms"], 3), "launches": p[k]["count"]} for k in LAUNCHES if p.get(k) and p[k]["count"]}
        gram_ms, gram_n = p["tg_node_gram"]["ms"], p["tg_node_gram"]["count"]
        gram_flops = float(d) * B * nv * (nv + 1.0) * N
        gemm_ms = pg["gemm_f64"]["ms"] / pg["gemm_f64"]["count"]
        t0 = time.perf_counter()
        phi_np = numpy_fit(u_re, u_im, w[1])
        t_np = time.perf_counter() - t0
        rec = {"shape": name, "d": d, "N": N, "B": B, "m": m, "failed_replicates": int(np.count_nonzero(res["status"])),
               "node_gram_launches": gram_n, "node_gram_ms_total": round(gram_ms, 3), "node_gram_gflop": round(gram_flops / 1e9, 2),
               "node_gram_fraction_of_mfma_peak": round(gram_flops / (gram_ms * 1e-3) / MFMA_F64_PEAK, 4),
               "node_gram_us_per_node_replicate": round(1e3 * gram_ms / (d * B), 3),
               "gemm_us_same_M_N_K": round(1e3 * gemm_ms, 3),
               "factor_share_of_device_time": round(p["tg_factor"]["ms"] / sum(p[k]["ms"] for k in ("tg_node_gram", "tg_assemble", "tg_factor", "trsm", "trsm_trans") if p.get(k)), 3),
               "call_ms_median": round(1e3 * statistics.median(ts), 2), "call_ms_min": round(1e3 * min(ts), 2), "call_ms_max": round(1e3 * max(ts), 2),
               "ms_per_replicate": round(1e3 * statistics.median(ts) / B, 4), "rounds": a.rounds,
               "one_fit_with_inference_ms": round(1e3 * t_inf, 2),
               "numpy_float64_one_replicate_ms": round(1e3 * t_np, 1),
               "numpy_vs_device_phi_relerr": float(np.linalg.norm(phi_np - res["phi"][1].ravel()) / np.linalg.norm(phi_np)),
               "per_scope": per}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
