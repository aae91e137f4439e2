"""bench.py's step benchmark: loglik() + predict() over the resident trials, as one queued pair per step (BASELINE cfg2 / cfg3 / cfg4)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from .cpu import cpu_baseline
from .profiles import pmc_step_traffic, rocprof_kernel
from .workloads import (FP64_MFMA_SPEC_TFLOPS, HBM_PEAK_GBS, N_CUS, SETTLE_S, algorithmic_flops, build_model, oracle_setup,
                        synth_data)


def run_step_bench(args, w, rank, world, local_rank, backend, compact=False, cpu_legs=None, outputs=None):
    import torch
    from gpcsd_amd import _hip
    from gpcsd_amd.dist import TrialSharding
    n_gpus = world
    R_local = args.trials_per_gpu or w["trials_per_gpu"]
    sharding = TrialSharding() if (world > 1 or os.environ.get("GPCSD_BENCH_FORCE_DIST") == "1") else None

    # ---- synthetic resident data (each rank draws its own block of trials) ----
    m = build_model(w, np.zeros((w["nx"], w["nt"], 1)))
    m.set_device(local_rank)
    lfp = synth_data(w, m, R_local, seed=1000 + rank)
    m.update_lfp(lfp, w["t"])
    ctx = m._sync_device()
    # `value` is measured with every call doing its own decompositions: the library's decomposition cache (predict right
    # after loglik reuses the unchanged temporal side) is switched off here and reported as a separate line below
    ctx.decomposition_cache(False)
    z = w.get("z", w["x"])
    C = len(m.temporal_cov_list)
    R_total = R_local * n_gpus

    # Hyper-parameters originate on rank 0: ONE broadcast before the loop (what fit() does -- every rank then walks the same
    # deterministic optimiser trajectory, no per-evaluation broadcast is needed); every rank re-assembles Ks / Kt and their
    # decompositions itself (deterministic kernels: bit-identical replicas).  Per step the only collective is the sum
    # all-reduce of the partial quadratic term (one double over RCCL).
    if sharding is not None:
        m._set_from_tparams(sharding.broadcast(m._current_tparams(), src=0), False)

    paired = os.environ.get("GPCSD_BENCH_UNPAIRED") != "1"
    # Successive steps of a throughput loop are independent and their hyper-parameters known: each step ANNOUNCES the next
    # (gpcsd_prefetch_pair) right after queueing itself, so that the next step's two decomposition chains start under this step's
    # products instead of behind the host's collection of its log-likelihood -- every chain is still queued, run and consumed
    # inside the timed region (the last announcement is work nobody takes).  An optimiser cannot do this (its next point depends on
    # the value it waits for): `unannounced_ms_per_step` in the line is the same loop without announcements.
    # GPCSD_BENCH_ANNOUNCE=0 / GPCSD_BENCH_SHARE_S=0: A/B.  Sharing the spatial side (one decomposition for Ks + jitter I and Ks:
    # same eigenvectors, shifted spectrum -- gpcsd_pair_share_s) is off in the library by default and switched on here, where the
    # main stream is the bound.
    announce = {"on": paired and os.environ.get("GPCSD_BENCH_ANNOUNCE", "1") == "1"}
    share_s = paired and os.environ.get("GPCSD_BENCH_SHARE_S", "1") == "1"
    ctx.pair_share_s(share_s)

    def one_step():
        hp, keep = m._hparams(m.JITTER)
        hp0, keep0 = m._hparams(0.0)
        # queue both calls, then come back for the log-likelihood.  As one paired call (gpcsd_loglik_predict_async) the two
        # temporal and the two spatial eigenproblems of the step share one chain of launches as replicas -- every one of them
        # is solved, the results are the bits of the two calls made separately -- and the next step's chain runs beside this
        # step's predict GEMMs.  GPCSD_BENCH_UNPAIRED=1: the same as two queued calls (four chains per step).
        if paired:
            ctx.loglik_predict_async(hp, hp0, z, w["t"], _hip.PRED_CSD, want_lists=True)
            if announce["on"]:
                ctx.prefetch_pair(hp, hp0, z, w["t"])
        else:
            ctx.loglik_parts_async(hp)
            ctx.predict_resident(hp0, z, w["t"], _hip.PRED_CSD, want_lists=True)
        if sharding is None:
            sumlog, quad = ctx.loglik_parts_wait()
            return -0.5 * R_total * sumlog - 0.5 * quad, 0.0, 0.0
        # Multi-rank: the only collective of a step is one double summed over the ranks (RCCL).  A rank has its partial sum
        # when its log-likelihood comes back; the host then queues the next step FIRST and runs the all-reduce of the step
        # before behind that queueing -- while the GPU works on the next step's eigen-chain and the host would be idle
        # anyway (issuing it in front of the queueing costs 0.25 ms of host time per step on the critical path).  The global
        # log-likelihood of step k is therefore complete during step k+1 (the last one before the final fence).
        ll_prev = flush()
        sumlog, quad = ctx.loglik_parts_wait()
        state["partial"] = (sumlog, quad)
        return ll_prev, 0.0, 0.0

    def solo_step():
        hp, keep = m._hparams(m.JITTER)
        hp0, keep0 = m._hparams(0.0)
        ctx.loglik_predict_async(hp, hp0, z, w["t"], _hip.PRED_CSD, want_lists=True)
        return ctx.loglik_parts_wait()

    state = {}

    def flush():
        prev = state.pop("partial", None)
        if prev is None or sharding is None:
            return None
        return -0.5 * R_total * prev[0] - 0.5 * float(sharding.allreduce_sum_async(np.array([prev[1]]))()[0])

    def fence():
        last = flush()
        if last is not None:
            state["ll"] = last
        ctx.synchronize()
        torch.cuda.synchronize()
        if sharding is not None:
            import torch.distributed as td
            td.barrier()

    # Setup, not warm-up: a fresh process on a cold box needs a few evaluations before it is in steady state (first call
    # eager + allocations, second captured into hipGraphs, third replayed; GPU clocks and host caches ramp over the first
    # tenths of a second -- a 10-step timed region measured 4.6 ms/step as the first command on a fresh box against 2.63
    # afterwards).  A fixed number of untimed evaluations (reported as "setup_steps"; the same count on every rank, each
    # step carries collectives), then the W warm-up steps the contract asks for, then K timed.
    t_first_eval = time.perf_counter()
    for _ in range(args.setup_steps):
        one_step()
    # A model's first ~0.1 s: on this pool every second model sees ONE interval of 9 / 19 / 29 ms, 35-110 ms after its first
    # evaluation, in which none of the process's queues make progress (not the host's wait, not allocations, frees or
    # new contexts injected into a model in steady state; tools/stall_probe.py, tools/stall_inject.py).  With the driver's K = 20
    # the timed region is 16 ms: it starts no earlier than SETTLE_S after the model's first evaluation, the setup steps continuing
    # until then (the same count on every rank: rank 0 decides).
    n_settle = 0
    if sharding is None:
        while time.perf_counter() - t_first_eval < SETTLE_S:
            one_step()
            n_settle += 1
    else:                                                  # every step carries a collective: the same count on every rank
        n_settle = 400
        for _ in range(n_settle):
            one_step()
    for _ in range(args.warmup):
        one_step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ll, _a, _b = one_step()
    fence()
    elapsed = time.perf_counter() - t0
    if sharding is not None:
        ll = state["ll"]                          # the last step's global log-likelihood, collected inside the timed region
    if outputs is not None:
        # what the timed loop's last step hands its caller (this rank's trials), fetched before anything else is queued: the
        # log-likelihood and the prediction it left in HBM, as predict() would return it (csd_pred, csd_pred_list)
        shape = (z.shape[0], w["nt"], R_local)
        outputs["loglik"] = np.array([float(ll)])
        outputs["csd_pred"] = ctx.fetch("pred_out_csd", shape).copy()
        outputs["csd_pred_list"] = ctx.fetch("pred_out_csd_list", (C,) + shape).copy()
    dist_info = None
    if sharding is not None:
        import torch.distributed as td
        solo = 0.0
        if not args.only_value:
            # the same steps on every rank WITHOUT the collective (each rank alone with its card, as an N = 1 run): what the
            # sharded job's rate is quoted against when no N = 1 figure is handed in (--n1-value)
            for _ in range(min(args.warmup, 3)):
                solo_step()
            ctx.synchronize()
            tsolo = time.perf_counter()
            for _ in range(args.steps):
                solo_step()
            ctx.synchronize()
            solo = time.perf_counter() - tsolo
        dev = "cuda" if backend == "nccl" else "cpu"
        per_rank = torch.zeros(2 * world, dtype=torch.float64, device=dev)
        per_rank[rank], per_rank[world + rank] = elapsed, solo
        td.all_reduce(per_rank, op=td.ReduceOp.SUM)
        per_rank = per_rank.cpu().numpy()
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        td.all_reduce(tt, op=td.ReduceOp.MAX)
        elapsed = float(tt.cpu()[0])
        value_now = R_total * args.steps / elapsed
        dist_info = {
            "collective_backend": td.get_backend(), "rccl_ranks": td.get_world_size() if td.get_backend() == "nccl" else 0,
            "ranks": td.get_world_size(),
            "per_rank_ms_per_step": [1e3 * float(v) / args.steps for v in per_rank[:world]],
        }
        if not args.only_value:
            unsharded_rate = float(np.sum(R_local * args.steps / per_rank[world:]))
            dist_info["per_rank_ms_per_step_without_collectives"] = [1e3 * float(v) / args.steps for v in per_rank[world:]]
            dist_info["efficiency_vs_ranks_without_collectives"] = value_now / unsharded_rate
            dist_info["scaling_efficiency"] = value_now / unsharded_rate
            dist_info["scaling_efficiency_against"] = ("sum of the ranks' own rates over the same steps without the all-reduce "
                                                       "(same processes)")
        if args.n1_value:
            dist_info["scaling_efficiency"] = value_now / (world * args.n1_value)
            dist_info["scaling_efficiency_against"] = "--n1-value %.6g trials/s" % args.n1_value
    ms_per_step = 1e3 * elapsed / args.steps
    pf_queued, pf_taken = ctx.prefetch_stats()
    # the prediction the TIMED loop's last step left in HBM, in the mode `value` is timed in (announced, one spatial decomposition
    # per pair: not the bits of a fenced call), fetched before anything else is queued: the line's parity gate reads this one
    timed_pred = None
    if not args.only_value and world == 1:
        timed_pred = {"csd": ctx.fetch("pred_out_csd", (z.shape[0], w["nt"], R_local)).copy()}
    if args.only_value:                      # the plain run (and the command the rocprofv3 passes under profiles/ are taken over)
        if rank != 0:
            return None
        return {"metric": "gpcsd_loglik_plus_predict_trials_per_sec", "value": R_total * args.steps / elapsed, "unit": "trials/s",
                "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup, "setup_steps": args.setup_steps + n_settle,
                "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
                "data": "synthetic", "loglik": float(ll),
                "config": {"workload": w["label"], "n_elec": w["nx"], "n_t": w["nt"], "trials_per_gpu": R_local,
                           "total_trials": R_total, "parallelism": "trial-sharded x%d" % n_gpus,
                           "next_step_announced": bool(announce["on"]), "pair_shares_spatial_side": bool(share_s)},
                "distributed": dist_info}

    # ---- the two halves on their own (rank-local, every call fenced: nothing of one call overlaps the next) ----
    # In the step loop above predict_resident returns with its GEMM tail in flight (its results stay on the device) and
    # the next loglik's temporal chain runs beside that tail, so the per-call host times of the loop do not separate the
    # halves; these two loops do.  Their sum is the unpipelined step.
    n_sub = max(10, min(args.steps, 50))
    hp_s, keep_s = m._hparams(m.JITTER)
    hp0_s, keep0_s = m._hparams(0.0)
    ctx.synchronize()
    ts0 = time.perf_counter()
    for _ in range(n_sub):
        ctx.loglik_parts(hp_s)
    t_ll = (time.perf_counter() - ts0) / n_sub
    ts0 = time.perf_counter()
    for _ in range(n_sub):
        ctx.predict_resident(hp0_s, z, w["t"], _hip.PRED_CSD, want_lists=True)
        ctx.synchronize()
    t_pr = (time.perf_counter() - ts0) / n_sub

    # ---- the same loop WITHOUT announcements (every step queues its own chains when it starts: what a caller whose next
    # hyper-parameters depend on this step's value gets), and with the library's defaults on top (spatial side not shared:
    # the pair then has the bits of its fenced calls) -- never part of `value`; the same counts on every rank (collectives) ----
    unannounced_ms = default_ms = None
    if paired and (announce["on"] or share_s):
        n_un = max(10, min(args.steps, 100))

        def timed_loop(n):
            for _ in range(5):
                one_step()
            flush()
            ctx.synchronize()
            tu = time.perf_counter()
            for _ in range(n):
                one_step()
            flush()
            ctx.synchronize()
            return 1e3 * (time.perf_counter() - tu) / n
        was = announce["on"]
        announce["on"] = False
        unannounced_ms = timed_loop(n_un)
        ctx.pair_share_s(False)
        default_ms = timed_loop(n_un)
        ctx.pair_share_s(share_s)
        announce["on"] = was

    # ---- the same steps with the host loop two steps deep: step k+1 is queued before step k's log-likelihood is collected, so
    # the chains of consecutive steps run back to back (rank-local, no collective; never part of `value`, whose steps each
    # return their result before the next one is queued) ----
    deep_ms = None
    if paired:
        hp_d, keep_d = m._hparams(m.JITTER)
        hp0_d, keep0_d = m._hparams(0.0)

        def run_deep(n):
            ctx.loglik_predict_async(hp_d, hp0_d, z, w["t"], _hip.PRED_CSD, want_lists=True)
            for _ in range(n - 1):
                ctx.loglik_predict_async(hp_d, hp0_d, z, w["t"], _hip.PRED_CSD, want_lists=True)
                ctx.loglik_parts_wait()
            return ctx.loglik_parts_wait()
        run_deep(10)
        ctx.synchronize()
        td0 = time.perf_counter()
        n_deep = max(10, min(args.steps, 100))
        run_deep(n_deep)
        ctx.synchronize()
        deep_ms = 1e3 * (time.perf_counter() - td0) / n_deep
        # ... and the same with the eigenvector form of the log-likelihood forced (gpcsd_ll_tridiag mode 0): the tridiagonal form
        # (the default at this size) makes the next temporal chain wait for the previous log-likelihood's tail, which is what a
        # two-deep loop would overlap -- DESIGN 4.9
        ctx.ll_tridiag(0)
        run_deep(10)
        ctx.synchronize()
        td1 = time.perf_counter()
        run_deep(n_deep)
        ctx.synchronize()
        deep_ms_eig = 1e3 * (time.perf_counter() - td1) / n_deep
        ctx.ll_tridiag(int(os.environ.get("GPCSD_LL_TRIDIAG", "2")[:1] or 2))      # back to the mode this context was created with

    # ---- same step with the decomposition cache on (a user's loglik -> predict sequence; never part of `value`) ----
    ctx.decomposition_cache(True)
    for _ in range(5):
        one_step()
    ctx.synchronize()
    tc0 = time.perf_counter()
    n_cached = max(10, min(args.steps, 50))
    for _ in range(n_cached):
        one_step()
    flush()
    ctx.synchronize()
    cached_ms = 1e3 * (time.perf_counter() - tc0) / n_cached
    ctx.decomposition_cache(False)

    # ---- the class API as a drop-in user calls it: predict() returns host arrays (PCIe inclusive), rank-local ----
    for _ in range(3):                                         # the result arrays ping-pong between two pinned blocks of the
        m.predict(z, w["t"], type="csd")                       # pool: both exist after the second call (steady state of a loop)
    t1 = time.perf_counter()
    n_pcie = 3
    for _ in range(n_pcie):
        m.predict(z, w["t"], type="csd")
    pcie_predict = R_local * n_pcie / (time.perf_counter() - t1)
    out_bytes = (1 + C) * z.shape[0] * w["nt"] * R_local * 8
    # ... and with the decomposition cache on, the library's default: what predict() costs right after fit() / loglik() at the
    # fitted hyper-parameters (neuropixels/fit_gpcsd2d.py:101-107) -- both decompositions are reused, the call is its GEMM tail
    # and the copy
    ctx.decomposition_cache(True)
    for _ in range(3):
        m.predict(z, w["t"], type="csd")
    t1 = time.perf_counter()
    for _ in range(n_pcie):
        m.predict(z, w["t"], type="csd")
    pcie_predict_cached = R_local * n_pcie / (time.perf_counter() - t1)
    ctx.decomposition_cache(False)

    # ---- roofline: HIP events around the kernels of the SAME paired, queued step the timed loop runs ----
    # mode 2: asynchronous scopes, chains launched eagerly so the scopes inside them record (per-kernel launch times);
    # mode 3: asynchronous scopes with the chains replayed as hipGraphs exactly as in the timed loop (chain-level scopes)
    def profiled_pass(mode, n):
        # (without announcements: the tail's own clock stamps of a step are read when its log-likelihood is back, i.e. when ITS
        # chains have finished -- an announced next chain would be in flight on the same stamps.  The kernels are the same.)
        was_announcing = announce["on"]
        announce["on"] = False
        try:
            return _profiled_pass(mode, n)
        finally:
            announce["on"] = was_announcing

    def _profiled_pass(mode, n):
        flush()
        ctx.synchronize()
        ctx.prof_reset()
        ctx.prof_enable(mode)
        for _ in range(3):
            one_step()
        flush()
        ctx.synchronize()
        ctx.prof_reset()
        clk = {0: [], 1: []}
        tp0 = time.perf_counter()
        for _ in range(n):
            one_step()
            # the step's log-likelihood is back, so both of its chains have finished: the tridiagonalisation tail's own
            # wall-clock stamps of this step (the one timing that also exists inside a replayed hipGraph, mode 3)
            for region in (0, 1):
                ms, nwg, fl = ctx.prof_tail_clock(region)
                if ms > 0.0:
                    clk[region].append((ms, nwg, fl))
        flush()
        ctx.synchronize()
        dt = (time.perf_counter() - tp0) / n
        ctx.prof_enable(0)
        return ctx.prof_all(), 1e3 * dt, clk
    n_prof = max(10, min(args.steps, 40))
    prof, eager_ms, _clk_eager = profiled_pass(2, n_prof)
    prof_graph, graph_ms, clk_graph = profiled_pass(3, n_prof)
    if rank != 0:
        return None

    f_ll, f_pred, f_pred_trial = algorithmic_flops(w, R_local, z.shape[0], C)
    ref_flops = f_ll + f_pred
    gemms = {k: v for k, v in prof_graph.items() if k.startswith("gemm_") and v["count"] > 0}
    # flops actually launched per step: every GEMM launch as recorded by the library (2 M N K per launch, batch included:
    # folded-basis projections, Gram assembly, D&C merge products), the tridiagonalisations ((4/3) n^3 per half problem) and
    # the compact-WY back-transformations (4 n^3 per half problem: V Z, T W, V^T W per panel of 64 reflectors)
    gemm_flops = sum(v["flops"] for k, v in prof.items() if k.startswith("gemm_")) / n_prof       # (incl. the D&C merge products)
    tail = prof.get("sytrd_rtail")
    tail_flops = tail["flops"] / n_prof if tail else 0.0
    wy_flops = 3.0 * tail_flops                                  # 4 n^3 = 3 x (4/3) n^3 for the same half problems
    exec_flops = gemm_flops + tail_flops + wy_flops
    step_s = ms_per_step * 1e-3
    wl = args.workload if (args.trials_per_gpu is None and n_gpus == 1) else "none"
    roof = {
        "bound": "mfma", "unit": "TFLOP/s", "peak": FP64_MFMA_SPEC_TFLOPS,
        "achieved": exec_flops / step_s / 1e12, "frac": exec_flops / step_s / 1e12 / FP64_MFMA_SPEC_TFLOPS,
        "scope": "one step = loglik + predict(csd) of %d trials; flops actually launched (folded-basis GEMMs, "
                 "symmetry-folded eigensolver) / ms_per_step" % R_local,
        "executed_gflop_per_step": exec_flops / 1e9,
        "executed_breakdown_gflop": {"gemm": gemm_flops / 1e9, "tridiagonalisation": tail_flops / 1e9,
                                     "back_transformation": wy_flops / 1e9},
        "reference_algorithm": {"gflop_per_step": ref_flops / 1e9, "achieved": ref_flops / step_s / 1e12,
                                "frac": ref_flops / step_s / 1e12 / FP64_MFMA_SPEC_TFLOPS,
                                "note": "SURVEY 8(d) unit: F_spatial + F_eig + R F_proj (+ predict); the library executes "
                                        "about half of its GEMM part and a quarter of its eigensolver part"},
        "measured_mfma_f64_peak_tflops": ctx.mfma_f64_peak(),
        "profiled_passes": {"steps": n_prof, "eager_chains_ms_per_step": eager_ms, "graph_chains_ms_per_step": graph_ms,
                            "note": "the timed step re-run with event scopes on the library's streams: chains eager (per-kernel "
                                    "scopes below) and chains as hipGraphs (chain-level scopes); both leave the step queued and paired"},
    }
    if tail and tail["count"]:
        avg = tail["ms"] / tail["count"]
        per_launch = tail["flops"] / tail["count"]
        share, rp_avg, rp_calls, src = rocprof_kernel(wl, "sytrd_rtail_kernel")
        lps = tail["count"] / n_prof
        # the same kernel inside the replayed hipGraphs of the timed loop (mode 3): its workgroups' own wall-clock stamps
        in_graph = None
        stamps = clk_graph[0] + clk_graph[1]
        if stamps:
            g_avg = sum(ms for ms, _, _ in stamps) / len(stamps)
            g_fl = sum(fl for _, _, fl in stamps) / len(stamps)
            in_graph = {"avg_launch_ms": g_avg, "launches_timed": len(stamps),
                        "temporal_chain_ms": (sum(ms for ms, _, _ in clk_graph[0]) / len(clk_graph[0])) if clk_graph[0] else None,
                        "spatial_chain_ms": (sum(ms for ms, _, _ in clk_graph[1]) / len(clk_graph[1])) if clk_graph[1] else None,
                        "achieved": g_fl / (g_avg * 1e-3) / 1e12, "frac": g_fl / (g_avg * 1e-3) / 1e12 / FP64_MFMA_SPEC_TFLOPS,
                        "how": "last end - first start over the launch's workgroups, device wall clock stamped by the kernel "
                               "itself (graph replay, where event scopes cannot record)"}
        roof["dominant_kernel"] = {
            "kernel": "sytrd_rtail_kernel", "why": "largest share of GPU time in the rocprofv3 kernel stats of `bench.py --only-value`",
            "in_graph_replay": in_graph,
            "share_of_gpu_time_rocprof": share, "rocprof_avg_launch_ms": rp_avg, "rocprof_launches": rp_calls, "rocprof_source": src,
            # the headline figures are those of the kernel as it runs in the timed loop (graph replay: its own clock stamps,
            # which the committed rocprofv3 average reproduces); HIP events exist for the eagerly launched chains of the
            # other profiled pass only, where the host issues ~100 launches per chain and the tails overlap other work differently
            "avg_launch_ms": in_graph["avg_launch_ms"] if in_graph else avg,
            "avg_launch_ms_hip_events_eager_chains": avg,
            "launches_per_step": lps, "ms_per_step": (in_graph["avg_launch_ms"] if in_graph else avg) * lps, "flops_per_launch": per_launch,
            "achieved": in_graph["achieved"] if in_graph else per_launch / (avg * 1e-3) / 1e12,
            "frac": in_graph["frac"] if in_graph else per_launch / (avg * 1e-3) / 1e12 / FP64_MFMA_SPEC_TFLOPS,
            "workgroups_per_launch": 4 if paired else 2,
            "cus_busy": "%d of %d (one 768-thread workgroup per half problem)" % (4 if paired else 2, N_CUS),
            "bound": "latency: ~250 dependent Householder columns per launch, two workgroup barriers each",
            "note": "one launch per chain "
                    "per step, each with the two replicas' half problems as workgroups -- the temporal chain's (4 x 250 rows, "
                    "on the critical path) and the spatial chain's (4 x 192 rows, beside it); the two overlap in time, so "
                    "their sum is not a share of the step's wall time",
        }
    if gemms:
        name = max(gemms, key=lambda k: gemms[k]["ms"])
        g = gemms[name]
        avg_ms = g["ms"] / g["count"]
        ach = (g["flops"] / g["count"]) / (avg_ms * 1e-3) / 1e12
        roof["largest_gemm"] = {
            "kernel": "gemm_f64_kernel [" + name + "]", "avg_launch_ms": avg_ms, "flops_per_launch": g["flops"] / g["count"],
            "achieved": ach, "frac": ach / FP64_MFMA_SPEC_TFLOPS, "share_of_step_wall": (g["count"] / n_prof) * avg_ms / ms_per_step,
            "all_gemm_tflops": sum(v["flops"] for v in gemms.values()) / (sum(v["ms"] for v in gemms.values()) * 1e-3) / 1e12}
    traffic, tdetail = pmc_step_traffic(wl)
    alg_bytes = 2 * w["nx"] * w["nt"] * R_local * 8 + out_bytes          # lfp read once per call + predict outputs written once
    roof["traffic"] = traffic
    roof["traffic_unit"] = "HBM bytes per step (rocprofv3 --pmc over `bench.py --only-value`, corrected as the gfx950 guide prescribes)"
    roof["traffic_detail"] = tdetail
    roof["algorithmic_bytes_per_step"] = alg_bytes
    roof["per_kernel_ms_per_step"] = {k: v["ms"] / n_prof for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}
    roof["per_kernel_launches_per_step"] = {k: v["count"] / n_prof for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])}
    roof["chains_ms_per_step_graph_replay"] = {k: v["ms"] / n_prof for k, v in sorted(prof_graph.items(), key=lambda kv: -kv[1]["ms"])
                                               if v["count"] > 0}

    # scalars of the nested reports once more at the first level of `roofline` (a record that keeps scalars only keeps these)
    dk, lg = roof.get("dominant_kernel"), roof.get("largest_gemm")
    if dk:
        roof["dominant_kernel_name"] = dk["kernel"]
        roof["dominant_kernel_frac"] = dk["frac"]
        roof["dominant_kernel_avg_ms"] = dk["avg_launch_ms"]
        roof["dominant_kernel_share"] = dk["share_of_gpu_time_rocprof"]
    if lg:
        roof["largest_gemm_frac"] = lg["frac"]
        roof["largest_gemm_avg_ms"] = lg["avg_launch_ms"]
        roof["all_gemm_frac"] = lg["all_gemm_tflops"] / FP64_MFMA_SPEC_TFLOPS
    roof["traffic_over_algorithmic"] = (traffic / alg_bytes) if traffic else None
    roof["reference_algorithm_frac"] = roof["reference_algorithm"]["frac"]

    out = {
        "metric": "gpcsd_loglik_plus_predict_trials_per_sec",
        "value": R_total * args.steps / elapsed,
        "unit": "trials/s",
        "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup, "setup_steps": args.setup_steps + n_settle,
        "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": w["label"], "n_elec": w["nx"], "n_t": w["nt"], "trials_per_gpu": R_local,
                   "total_trials": R_total, "predict": "z=%s, t*=t, type=csd, %d temporal components" % ("electrodes" if "z" not in w else "%d sites" % len(z), C),
                   "parallelism": "trial-sharded x%d" % n_gpus,
                   "class_api_predict_trials_per_sec": pcie_predict, "class_api_predict_host_gb_per_sec": pcie_predict / R_local * out_bytes / 1e9,
                   "class_api_predict_cached_trials_per_sec": pcie_predict_cached,
                   "class_api_predict_cached_host_gb_per_sec": pcie_predict_cached / R_local * out_bytes / 1e9},
        "pipelining": "a step queues loglik + predict as one paired call (gpcsd_loglik_predict_async: the eigenproblems of the step -- "
                      "Kt (once: both sets have the same temporal hyper-parameters), Ks with jitter for loglik and without for predict -- "
                      "run as one temporal and one spatial chain; nothing is reused from another step; results stay in HBM), then "
                      "waits for the log-likelihood; the next step's chains run beside this step's predict GEMMs "
                      "(double-buffered chain outputs).  Every "
                      "step's log-likelihood is returned to the host inside the step; the timed region ends with a full "
                      "device fence.  Each step announces the next one (gpcsd_prefetch_pair: the next step's two chains are queued "
                      "behind this step's launches and start under its products -- config.next_step_announced; "
                      "config.unannounced_ms_per_step is the same loop without) and its pair decomposes ONE spatial matrix "
                      "(Ks + jitter I and Ks share eigenvectors: config.pair_shares_spatial_side; the prediction then agrees with "
                      "the separately decomposed one to 1e-13, config.library_default_ms_per_step is the loop with neither)."
                      + ("  N > 1: a rank's partial sum is back inside the step; the 8-byte RCCL all-reduce that completes the "
                         "global log-likelihood of step k runs behind the queueing of step k+1 (the last one before the final "
                         "fence)." if n_gpus > 1 or sharding is not None else ""),
        "fenced_calls": {"loglik_ms": 1e3 * t_ll, "predict_resident_ms": 1e3 * t_pr, "sum_ms": 1e3 * (t_ll + t_pr),
                         "loglik_evals_per_sec_per_gpu": 1.0 / t_ll, "loglik_trial_evals_per_sec_per_gpu": R_local / t_ll,
                         "predict_trials_per_sec_per_gpu": R_local / t_pr,
                         "note": "each call alone, device fenced after every call (rank-local, no collective)"},
        "two_steps_in_flight": None if deep_ms is None else {
            "ms_per_step": deep_ms, "trials_per_sec_per_gpu": R_local / (deep_ms * 1e-3),
            "ms_per_step_eigenvector_form": deep_ms_eig,
            "note": "host loop two steps deep (step k+1 queued before step k's log-likelihood is collected; up to four "
                    "evaluations may be outstanding per context): the chains of consecutive steps run back to back.  NOT "
                    "part of value, whose steps each hand their result back before the next step is queued.  With the "
                    "log-likelihood's tridiagonal form (the default at this size, built for the one-deep loop) the next "
                    "temporal chain waits for the previous log-likelihood's tail; ms_per_step_eigenvector_form is the same "
                    "loop with gpcsd_ll_tridiag mode 0"},
        "with_decomposition_cache": {"ms_per_step": cached_ms, "trials_per_sec_per_gpu": R_local / (cached_ms * 1e-3),
                                     "note": "library default for users (predict after loglik reuses the unchanged temporal "
                                             "eigendecomposition, bit-identical); NOT part of value"},
        "class_api_predict_trials_per_sec_per_gpu_pcie_inclusive": pcie_predict,
        "class_api_predict_host_gb_per_sec": pcie_predict / R_local * out_bytes / 1e9,
        "class_api_predict_cached_trials_per_sec_per_gpu_pcie_inclusive": pcie_predict_cached,
        "class_api_predict_cached_host_gb_per_sec": pcie_predict_cached / R_local * out_bytes / 1e9,
        "class_api_predict_note": "predict() returns host arrays: device time + one PCIe copy of (1 + C) nz nt R doubles into pinned "
                                  "blocks.  First pair: every call decomposes both sides (cache off, as `value`); `cached`: the "
                                  "library default, unchanged hyper-parameters reuse both decompositions",
        "loglik": float(ll),
        "distributed": dist_info,
        "roofline": roof,
    }
    out["config"]["fenced_loglik_ms"], out["config"]["fenced_predict_ms"] = 1e3 * t_ll, 1e3 * t_pr
    out["config"]["two_steps_in_flight_ms"] = deep_ms
    out["config"]["next_step_announced"] = bool(announce["on"])
    out["config"]["pair_shares_spatial_side"] = bool(share_s)
    out["config"]["unannounced_ms_per_step"] = unannounced_ms
    out["config"]["library_default_ms_per_step"] = default_ms
    out["config"]["announcements_taken"] = pf_taken
    want_baseline = not args.no_cpu_baseline and world == 1       # the CPU baseline is reported at N=1 only
    if want_baseline or compact:
        # the GPU half of the parity spot check now (the step's own prediction, fetched); the oracle half is a CPU leg
        hp0, _k = m._hparams(0.0)
        ctx.predict_resident(hp0, z, w["t"], _hip.PRED_CSD, want_lists=True)
        got_fenced = ctx.fetch("pred_out_csd", (z.shape[0], w["nt"], R_local))
        got = timed_pred["csd"] if timed_pred is not None else got_fenced
        ll_gpu = float(ll)

        def cpu_leg():
            if want_baseline:
                cb, ll_cpu, pred_cpu = cpu_baseline(w, m, lfp, args.cpu_budget_s)
                out["cpu_baseline"] = cb
                cb["reference_layout_loglik_evals_per_sec"] = cb["faithful_layout"]["loglik_evals_per_sec"]
                cb["single_thread_trials_per_sec"] = cb["single_thread"]["value"]
            else:                                    # sub-result of the default line: parity spot check without the timing legs
                O, geom, hpo, hpo0 = oracle_setup(w, m)
                ll_cpu = O.loglik(geom, hpo, lfp)
                pred_cpu = O.predict(geom, hpo0, lfp, z, w["t"], type="csd")["csd"]
            # parity spot check beside the numbers: the outputs of the TIMED loop's last step (its log-likelihood and the prediction
            # it left in HBM, in the mode `value` is timed in) vs the oracle on the same trials; the fenced call's beside it
            out["parity_rel_err_loglik_vs_oracle"] = abs(ll_gpu - ll_cpu) / abs(ll_cpu)
            out["parity_rel_err_predict_vs_oracle"] = float(np.max(np.abs(got - pred_cpu)) / np.max(np.abs(pred_cpu)))
            out["parity_predict_source"] = ("last step of the timed loop (announced=%s, one spatial decomposition per pair=%s)"
                                            % (bool(announce["on"]), bool(share_s))) if timed_pred is not None else "fenced call"
            out["parity_rel_err_fenced_predict_vs_oracle"] = float(np.max(np.abs(got_fenced - pred_cpu)) / np.max(np.abs(pred_cpu)))
        if cpu_legs is None:
            cpu_leg()
        else:
            cpu_legs.append(cpu_leg)
    return out
