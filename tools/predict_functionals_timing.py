"""predict_functionals(..., resident=True) for J = 4 and J = 64 box averages over (z, t*) = (x, t), beside predict_at at the same
sites and times and beside the route available without it -- sample_posterior draws pushed through the same summaries -- at the cfg2
(24 x 500 x 200) and cfg3 (384 x 500 x 50) geometries.  The expectation this tool confirms or refutes: the call costs a small multiple
of predict_at and a small fraction of the sampling route.

The sampling route is timed in its cheapest form: the draws stay resident and the summaries W . draws are one torch product on the
device (a host reduction would first copy nz ntstar ntrials nsamples doubles out); what it returns still carries Monte-Carlo error.

One process, decomposition cache on (its default); every variant is warmed up, then the variants are timed in alternation (rounds)
and the median over the rounds of the fenced call time (host clock around a call that ends in a device synchronise) is reported.
A second, separate pass with fenced profiling scopes splits predict_functionals into forming alpha and the prior's operands (the
gemm_fun_* products of the GEMM core) and the Gram launches (fun_gram_*: the new kernel and its chunk sum).

    python tools/predict_functionals_timing.py [--rounds 50] [--warmup 3] [--type csd] [--nsamples 8] [--cfg cfg2 cfg3]
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
from gpcsd_amd.utility_functions import roi_weights  # noqa: E402


def boxes(z, t, J):
    """J box averages: the sites in consecutive groups times consecutive time windows."""
    nz, ts = np.shape(z)[0], np.asarray(t, dtype=np.float64).reshape(-1)
    gs = 1
    while (gs * 2) ** 2 <= J and gs * 2 <= nz:
        gs *= 2
    gt = J // gs
    sites = np.array_split(np.arange(nz), gs)
    edges = np.array_split(np.arange(ts.size), gt)
    sets = [sites[j // gt] for j in range(gs * gt)]
    wins = [(ts[edges[j % gt][0]], ts[edges[j % gt][-1]]) for j in range(gs * gt)]
    return roi_weights(z, t, sets, wins)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--type", default="csd", choices=("csd", "lfp"))
    ap.add_argument("--nsamples", type=int, default=8)
    ap.add_argument("--cfg", nargs="+", default=["cfg2", "cfg3"])
    a = ap.parse_args()
    import torch
    for name in a.cfg:
        w = W.workload(name)
        m = W.build_model(w, np.zeros((w["nx"], w["nt"], 1)))
        R = w["trials_per_gpu"]
        m.update_lfp(W.synth_data(w, m, R, seed=1000), w["t"])
        ctx = m._sync_device()
        t = np.asarray(w["t"], dtype=np.float64)
        z = w["x"]
        Ws = {J: boxes(z, t, J) for J in (4, 64)}
        Wdev = torch.as_tensor(Ws[64].reshape(64, -1), device="cuda")

        def sampling_route():
            draws = m.sample_posterior(z, t, nsamples=a.nsamples, type=a.type, seed=1, resident=True)[0 if a.type == "csd" else 1]
            d = torch.as_tensor(draws, device="cuda").reshape(Wdev.shape[1], -1)
            s = (Wdev @ d).reshape(64, R, a.nsamples)
            mean = s.mean(2)
            dev = s - mean[:, :, None]
            cov = torch.einsum("jrs,krs->jk", dev, dev) / (R * (a.nsamples - 1))
            return mean.cpu(), cov.cpu()

        variants = [("predict_at", lambda: m.predict_at(z, t, type=a.type, resident=True))]
        for J in (4, 64):
            variants.append(("predict_functionals(J=%d)" % J, lambda J=J: m.predict_functionals(z, t, Ws[J], type=a.type, resident=True)))
        variants.append(("sample_posterior(%d draws) + summaries(J=64)" % a.nsamples, sampling_route))
        times = {v[0]: [] for v in variants}
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
        # the launches alone (fenced scopes serialise the call: not comparable with the times above)
        launches = {}
        ctx.prof_enable(1)
        for label, fn in variants[1:3]:
            ctx.prof_reset()
            for _ in range(3):
                fn()
            ctx.synchronize()
            p = ctx.prof_all()
            per = {k: p[k]["ms"] / 3.0 for k in p if k.startswith(("gemm_fun_", "fun_")) and p[k]["count"]}
            launches[label] = {"alpha_and_prior_operands_ms": round(sum(v for k, v in per.items() if k.startswith("gemm_fun_")), 4),
                               "gram_launches_ms": round(sum(v for k, v in per.items() if k.startswith("fun_gram")), 4),
                               "ms_per_call": {k: round(v, 4) for k, v in sorted(per.items())}}
        ctx.prof_enable(0)
        for label, _ in variants:
            v = sorted(times[label])
            print(json.dumps({"cfg": name, "type": a.type, "variant": label, "nz": int(np.shape(z)[0]), "ntstar": int(t.shape[0]),
                              "ntrials": R, "median_ms": round(1e3 * med[label], 4), "min_ms": round(1e3 * v[0], 4),
                              "max_ms": round(1e3 * v[-1], 4), "rounds": a.rounds,
                              "ratio_to_predict_at": round(med[label] / med["predict_at"], 4),
                              "split": launches.get(label)}), flush=True)


if __name__ == "__main__":
    main()
