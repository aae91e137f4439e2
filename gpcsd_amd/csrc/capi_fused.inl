// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip are in scope) --
// fused hot calls on resident data: loglik (synchronous, queued), predict (folded / full-size, resident), the paired call, sample_prior.
// (The posterior quantities at arbitrary times, which start from predict's full-size front, are capi_posterior.inl.)

// ------------------------------------------------------------------------------------------------
// fused hot calls
// ------------------------------------------------------------------------------------------------
// End of an asynchronous loglik: the scalars and status words go to the pinned block behind an event; nothing is waited for
// and the status words are left alone (the chains of later calls may already be reporting into them).
// the pinned slot the next asynchronous log-likelihood lands in (the tail's last launch may write it itself: k_ll_tridiag)
static double *next_ll_slot(gpcsd_ctx *c) { return c->h_ll + gpcsd_ctx::RESULT_DOUBLES * ((c->ll_head + c->ll_count) % gpcsd_ctx::LL_SLOTS); }

static int finish_loglik_async(gpcsd_ctx *c, const EigState &e, bool two, bool slot_written = false) {
    const int k = (c->ll_head + c->ll_count) % gpcsd_ctx::LL_SLOTS;       // callers have checked that a slot is free
    gpcsd_ctx::LlSlot &sl = c->ll_slot[k];
    if (!slot_written)
        GP_HIP(hipMemcpyAsync(c->h_ll + gpcsd_ctx::RESULT_DOUBLES * k, e.scal, gpcsd_ctx::RESULT_DOUBLES * sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
    GP_HIP(hipEventRecord(sl.ev, c->stream));
    c->tl("loglik result copied (main)", c->stream);
    ++c->ll_count;
    sl.done = false;
    sl.two = two;
    c->async_pending = true;
    c->status_zeroed = false;
    return 0;
}

// Folded-basis tail of the log-likelihood: the two projections as 2 + 2 half-size GEMMs, the quadratic form as two partial
// sums (one when the parity blocks went out as one batched launch: returns true), sum(log D) folded into the reduce launch.
// Shifted-tridiagonal form (EigState::tri): X = Y~ Q needs stage 1 of the temporal chain only and is queued BEFORE the main
// stream waits for the spatial chain; after that wait W = diag(U)^T X, and one forward recurrence per row gives the quadratic
// form, the pivots the log-determinant (k_ll_tridiag).  The temporal eigenvectors are never read.
// out[(x, r)][t~ block p] = in[(x, r)][t~ block p] Q_p, both parity blocks in one launch (Q of replica e.tri_rep; waits for stage 3)
static void tri_times_Q(gpcsd_ctx *c, EigState &e, const FoldMode &fm, const double *in, double *out, const char *prof) {
    const int nx = c->nx, nt = c->nt, R = c->ntrials;
    hipStream_t s = c->stream;
    if (e.wait_q) GP_HIP(hipStreamWaitEvent(s, c->ev_q[c->tgen], 0));
    e.wait_q = false;
    const char *const *tg = eigh_fold_tags(c, 1);
    GemmDesc g[2];
    for (int p = 0; p < 2; ++p) {
        const int np = p ? fm.ft.na : fm.ft.ns, c0 = p ? fm.ft.ns : 0;
        g[p].M = nx * R; g[p].N = np; g[p].K = np;
        g[p].A = in + c0; g[p].lda = nt;
        g[p].B = eigh_Q_view(c, tg[p], np, e.tri_count) + (size_t)e.tri_rep * np * np; g[p].ldb = np;
        g[p].C = out + c0; g[p].ldc = nt;
        g[p].prof_name = prof;
    }
    gemm_pair(c, g[0], g[1], s);
}

// X = Y~ Q of a tridiagonal-form consumer: the log-likelihood's (pred == null) or that prediction's own
static void loglik_tri_pre(gpcsd_ctx *c, EigState &e, const FoldMode &fm, const double *Yf, const PredCall *pred) {
    const char *xname = pred ? "pred_X" : "ll_X";
    if (e.pipe_pending) {                              // stage 1 ran with progress words: T, Q and X panel by panel (queue_q_pipeline)
        queue_q_pipeline(c, e, Yf, xname);
        return;
    }
    tri_times_Q(c, e, fm, Yf, c->buf<double>(xname, (size_t)c->nx * c->ntrials * c->nt), pred ? "gemm_pred_YQ" : "gemm_ll_YQ");
}

// The shifted tridiagonal systems of replica e.tri_rep.  Behind a pipelined stage 5 nothing on the stream is ordered behind the END
// of stage 1 yet (d, e, the scale): their first reader's wait is queued here.
struct TriOperands {
    const double *d[2], *e[2], *amax[2];
    int np[2], c0[2];
};
static TriOperands tri_operands(gpcsd_ctx *c, const EigState &e, const FoldMode &fm, hipStream_t s) {
    TriOperands o;
    const char *const *tg = eigh_fold_tags(c, 1);
    for (int p = 0; p < 2; ++p) {
        o.np[p] = p ? fm.ft.na : fm.ft.ns;
        o.c0[p] = p ? fm.ft.ns : 0;
        const EigArenaView av = eigh_arena_view(c, tg[p], o.np[p], e.tri_count);
        const long off = (long)e.tri_rep * av.blk;
        o.d[p] = av.d + off; o.e[p] = av.e + off; o.amax[p] = av.amax + off;
    }
    if (c->t1_wait_pending) {
        GP_HIP(hipStreamWaitEvent(s, c->ev_t1, 0));
        c->t1_wait_pending = false;
    }
    return o;
}

// host_slot: the caller's pinned result slot when the evaluation is asynchronous (else null); returns true when the tail wrote it
static bool loglik_tri_tail(gpcsd_ctx *c, EigState &e, const FoldMode &fm, double *W, double *host_slot = nullptr) {
    const int nx = c->nx, nt = c->nt, R = c->ntrials;
    hipStream_t s = c->stream;
    ++c->fold_gemm_calls;
    ++c->ll_tridiag_calls;
    join_spatial(c, e);
    fold_proj_spatial(c, fm.fs, c->buf<double>("ll_X", (size_t)nx * R * nt), W, (long)R * nt, s);
    const TriOperands o = tri_operands(c, e, fm, s);
    const bool wrote = k_ll_tridiag(c, W, fm.fs.w, o.d, o.e, o.amax, e.d_sig, nx, R, nt, o.np, o.c0, e.scal, e.scal + 1, s, host_slot,
                                    e.scal + gpcsd_ctx::SCAL_N, gpcsd_ctx::SCAL_N, gpcsd_ctx::RESULT_DOUBLES - gpcsd_ctx::SCAL_N);
    GP_HIP(hipEventRecord(c->ev_tri_done[c->tgen], s));
    c->tri_reader_queued[c->tgen] = true;
    return wrote;
}

static bool loglik_fold_tail(gpcsd_ctx *c, EigState &e, const FoldMode &fm, const double *Yf, double *W, double *host_slot = nullptr,
                             bool *slot_written = nullptr) {
    const int nx = c->nx, nt = c->nt, R = c->ntrials;
    hipStream_t s = c->stream;
    if (e.tri) {
        loglik_tri_pre(c, e, fm, Yf, nullptr);
        const bool wrote = loglik_tri_tail(c, e, fm, W, host_slot);
        if (slot_written) *slot_written = wrote;
        return true;
    }
    ++c->fold_gemm_calls;
    join_spatial(c, e);
    fold_proj_spatial(c, fm.fs, Yf, W, (long)R * nt, s);
    const int nparts = join_temporal(c, e, &fm, false);         // sum(log D): summed by the reduce launch of the GEMM below
    GemmDesc g2[2];
    g2[0].extra_sum_in = c->buf<double>("buildD_partials", 256);
    g2[0].extra_sum_n = nparts;
    g2[0].extra_sum_out = e.scal;
    for (int p = 0; p < 2; ++p) {
        const int np = p ? fm.ft.na : fm.ft.ns, c0 = p ? fm.ft.ns : 0;
        g2[p].M = nx * R; g2[p].N = np; g2[p].K = np;
        g2[p].A = W + c0; g2[p].lda = nt;
        g2[p].B = fm.ft.U + (p ? (size_t)fm.ft.ns * fm.ft.ns : 0); g2[p].ldb = np;
        g2[p].epi = EPI_QUAD; g2[p].D = e.Dinv + c0; g2[p].rdiv = R; g2[p].ldd = nt; g2[p].quad_out = e.scal + 1 + p;
        g2[p].prof_name = "gemm_proj_temporal_quad";
    }
    return gemm_pair(c, g2[0], g2[1], s);
}

static int loglik_parts_impl(gpcsd_ctx *c, const gpcsd_hparams *hp, double *out2, bool async) {
    GP_REQUIRE(c->d_lfp != nullptr, -4, "lfp not set (call gpcsd_set_lfp)");
    if (async && c->prof_mode == 1) {     // fenced profiling (mode 1): evaluate now, hand the result over at the wait
        gpcsd_ctx::LlSlot &sl = c->ll_slot[(c->ll_head + c->ll_count) % gpcsd_ctx::LL_SLOTS];
        sl.rc = loglik_parts_impl(c, hp, sl.out, false);
        sl.done = true;
        ++c->ll_count;
        return 0;
    }
    const FoldMode fm0 = fold_mode(c, hp);                          // the decision; its views are of the previous generation
    const double *Yf = fm0.on ? folded_lfp(c, fm0) : nullptr;
    // (the spatial chain is joined by the tail: the tridiagonal form queues its first product in front of that wait)
    // (X = Y~ Q goes through loglik_tri_pre below: stage 5 may apply)
    EigState e = front_half(c, hp, hp->jitter, !fm0.on, /*join_s=*/!fm0.on, /*want_tri=*/fm0.on, -1, /*x_via_tri_pre=*/fm0.on && fm0.ft.on);
    const FoldMode fm = fold_mode(c, hp);                           // views of the generation the front half just launched
    const int nx = c->nx, nt = c->nt, R = c->ntrials;
    hipStream_t s = c->stream;
    double *W = c->buf<double>("proj_W", (size_t)nx * R * nt);
    if (fm.on) {
        bool wrote = false;
        const bool batched = loglik_fold_tail(c, e, fm, Yf, W, async ? next_ll_slot(c) : nullptr, &wrote);
        if (async) return finish_loglik_async(c, e, !batched, wrote);
        double h3[3] = {0.0, 0.0, 0.0};
        const int rc = finish_call(c, e, h3, 3);
        out2[0] = h3[0];
        out2[1] = batched ? h3[1] : h3[1] + h3[2];
        return rc;
    }
    GemmDesc g1;                          // W[x'][(r,t)] = sum_x Qs[x][x'] Y[x][(r,t)]        (gpcsd1d.py:125 inner dot)
    g1.M = nx; g1.N = R * nt; g1.K = nx;
    g1.A = e.Qs; g1.lda = nx; g1.transA = true;
    g1.B = c->d_lfp; g1.ldb = (long)R * nt;
    g1.C = W; g1.ldc = (long)R * nt;
    g1.prof_name = "gemm_proj_spatial";
    gemm_f64(c, g1, s);
    join_temporal(c, e);
    GemmDesc g2;                          // alpha[(x',r)][i'] = sum_t W[(x',r)][t] Qt[t][i'];  quad = sum alpha^2 / D
    g2.M = nx * R; g2.N = nt; g2.K = nt;
    g2.A = W; g2.lda = nt;
    g2.B = e.Qt; g2.ldb = nt;
    g2.epi = EPI_QUAD; g2.D = e.Dinv; g2.rdiv = R; g2.ldd = nt; g2.quad_out = e.scal + 1;
    g2.prof_name = "gemm_proj_temporal_quad";
    gemm_f64(c, g2, s);
    if (async) return finish_loglik_async(c, e, false);
    return finish_call(c, e, out2, 2);
}

// clean status words for whatever is queued from here on (everything has been drained: nobody reports into them now)
static void clear_status_words(gpcsd_ctx *c) {
    if (int *dst = reinterpret_cast<int *>(c->buf<double>("scal_status", gpcsd_ctx::RESULT_DOUBLES) + gpcsd_ctx::SCAL_N)) {
        GP_HIP(hipMemsetAsync(dst, 0, gpcsd_ctx::STATUS_N * sizeof(int), c->stream));
        GP_HIP(hipStreamSynchronize(c->stream));
        c->status_zeroed = true;
    }
}

// Status 7 is not a numerical failure: a gate of the pipelined stage 5 (wy.hip: wy_qstage_kernel) gave up waiting for the
// tridiagonalisation that should have been running beside it -- kernels serialised by a profiler or a debugger, an oversubscribed
// card, a tail that could not get a CU.  The launch did nothing with the unfinished reflectors, so the evaluation is void, not
// wrong.  The call that collects it switches the pipeline off for this context (latched: the conditions that made one gate miss
// make the next one miss), counts it (gpcsd_q_pipeline_stats) and evaluates again: behind the END of the tail the unpipelined
// stage 5 (tchain_finish) forms the same T, Q and X.  `piped`: the call was queued while the pipeline was on.
static bool q_pipe_missed(gpcsd_ctx *c, int rc, bool piped) {
    if (rc != 7 || !piped) return false;
    c->q_pipe = false;
    ++c->q_pipe_timeouts;
    drain_after_failure(c);                // (also drops an announced front half: it was queued with the pipeline on)
    clear_status_words(c);
    c->last_error.clear();
    return true;
}

static int predict_impl(gpcsd_ctx *c, const PredCall &q);
static void sink_release(gpcsd_ctx *c, PredSink *sk);

// The one routine every collecting call goes through (q_pipe_missed's only caller): `rc` is what the call found for an evaluation
// queued with the pipeline on or off (`piped`).  A scheduling miss is answered by evaluating again, unpipelined now, what the
// collecting call owns -- the log-likelihood at `ll_hp` into out2 (null: none), the prediction `pred` (null: none, or no longer the
// owner of the resident outputs), both for a pair: rc becomes that evaluation's status and the return value is true.
static bool replay_if_missed(gpcsd_ctx *c, int &rc, bool piped, const gpcsd_hparams *ll_hp, double *out2, const PredCall *pred) {
    if (!q_pipe_missed(c, rc, piped)) return false;
    rc = 0;
    if (ll_hp) rc = loglik_parts_impl(c, ll_hp, out2, false);
    if (rc == 0 && pred) {
        PredCall again = *pred;
        again.async = false;
        sink_release(c, again.sink);  // (gpcsd_predict: the copies of the void evaluation have landed before the next ones start)
        rc = predict_impl(c, again);
    }
    return true;
}

// The request of a queued prediction, kept with copies of what it points to until another prediction owns the resident outputs
static void keep_prediction(gpcsd_ctx *c, bool piped, const PredCall &q) {
    gpcsd_ctx::PredKeep &k = c->last_pred;
    ++c->pred_seq;
    k.have = true;
    k.piped = piped;
    k.hp.set(q.hp);
    k.z.assign(q.z, q.z + (size_t)q.nz * c->dim);
    k.ts.assign(q.tstar, q.tstar + q.ntstar);
    k.call = q;
    k.call.hp = &k.hp.hp; k.call.z = k.z.data(); k.call.tstar = k.ts.data();
    k.call.sink = nullptr; k.call.ll = nullptr; k.call.prelude_side = false; k.call.solve_pass = 0;     // (of the queued call alone)
}
// ... for the call that collects slot sl: null unless the slot's paired prediction still owns the resident outputs
static const PredCall *kept_prediction(const gpcsd_ctx *c, const gpcsd_ctx::LlSlot &sl) {
    return (sl.pred_seq >= 0 && sl.pred_seq == c->pred_seq && c->last_pred.have) ? &c->last_pred.call : nullptr;
}

extern "C" int gpcsd_loglik_parts(gpcsd_ctx *c, const gpcsd_hparams *hp, double *out2) {
    GP_API_BEGIN(c)
    GP_REQUIRE(out2 != nullptr, -3, "null output");
    const bool piped = c->q_pipe;
    int rc = loglik_parts_impl(c, hp, out2, false);
    replay_if_missed(c, rc, piped, hp, out2, nullptr);
    return rc;
    GP_API_END(c)
}

extern "C" int gpcsd_loglik_parts_async(gpcsd_ctx *c, const gpcsd_hparams *hp) {
    if (c && c->ll_count >= gpcsd_ctx::LL_SLOTS)   // refused before anything is touched: the outstanding ones stay collectable
        return fail(c, HipError{-3, "loglik_parts_async: too many asynchronous evaluations outstanding (collect with "
                                    "gpcsd_loglik_parts_wait)"});
    GP_API_BEGIN(c)
    GP_REQUIRE(c->d_lfp != nullptr, -4, "lfp not set (call gpcsd_set_lfp)");
    check_hp(c, hp, c->nx);              // before anything of hp is copied into the slot (HpKeep::set reads n_sig2n doubles)
    gpcsd_ctx::LlSlot &sl = c->ll_slot[(c->ll_head + c->ll_count) % gpcsd_ctx::LL_SLOTS];
    sl.piped = c->q_pipe;
    sl.pred_seq = -1;
    sl.hp.set(hp);
    return loglik_parts_impl(c, hp, nullptr, true);
    GP_API_END(c)
}

extern "C" int gpcsd_loglik_parts_wait(gpcsd_ctx *c, double *out2) {
    if (c && (!out2 || c->ll_count == 0))
        return fail(c, HipError{-3, out2 ? "loglik_parts_wait: no asynchronous evaluation pending" : "null output"});
    GP_API_BEGIN(c)
    const int k = c->ll_head;
    gpcsd_ctx::LlSlot &sl = c->ll_slot[k];
    c->ll_head = (k + 1) % gpcsd_ctx::LL_SLOTS;
    --c->ll_count;
    if (sl.done) {                        // fenced profiling: evaluated when it was queued
        out2[0] = sl.out[0];
        out2[1] = sl.out[1];
        replay_if_missed(c, sl.rc, sl.piped, &sl.hp.hp, out2, kept_prediction(c, sl));
        return sl.rc;
    }
    GP_HIP(hipEventSynchronize(sl.ev));
    const double *host = c->h_ll + gpcsd_ctx::RESULT_DOUBLES * k;
    out2[0] = host[0];
    out2[1] = sl.two ? host[1] + host[2] : host[1];
    int st[gpcsd_ctx::STATUS_N];
    memcpy(st, host + gpcsd_ctx::SCAL_N, sizeof(st));
    // (asynchronous calls: every word as it stood when this evaluation's copy ran, the late stages' of EARLIER chains included)
    const int bad = fold_status(st, true);
    if (bad == 0) return 0;
    // this evaluation's, or an earlier asynchronous call's that nobody collected yet
    char b[160];
    snprintf(b, sizeof(b), "numerical failure (status %d): eigensolver did not converge or matrix not positive definite", bad);
    c->last_error = b;
    int rc = bad;
    if (replay_if_missed(c, rc, sl.piped, &sl.hp.hp, out2, kept_prediction(c, sl))) return rc;     // not a failure: evaluated again
    // The status words are sticky while asynchronous work is outstanding (nobody may clear them under a running chain).
    // Now that a failure has been reported: drain everything and clear them, so that evaluations queued from here on
    // start clean.  Evaluations that were ALREADY outstanding copied the words as they stood and report the failure too
    // (a failed wait poisons the ones queued before it returned; documented in gpcsd_hip.h).
    drain_after_failure(c);
    clear_status_words(c);
    return bad > 0 ? bad : 1;
    GP_API_END(c)
}

extern "C" int gpcsd_loglik(gpcsd_ctx *c, const gpcsd_hparams *hp, double *out) {
    if (!out) return fail(c, HipError{-3, "null output"});
    double p[2] = {0.0, 0.0};
    int rc = gpcsd_loglik_parts(c, hp, p);
    if (rc < 0) return rc;
    *out = -0.5 * (double)c->ntrials * p[0] - 0.5 * p[1];      // gpcsd1d.py:122,127-128
    return rc;
}

// Reflection symmetry of the prediction sites under the SAME reflection as the electrodes (then the cross-covariances
// commute with the pair of involutions and fold as well).  Cached on the site coordinates; ns == 0: none.
static const SymDev &site_symmetry(gpcsd_ctx *c, const double *z, int nz, int dim) {
    const size_t cnt = (size_t)nz * dim;
    if (c->sym_z_pts.size() == cnt && memcmp(c->sym_z_pts.data(), z, cnt * sizeof(double)) == 0) return c->sym_z;
    c->sym_z_pts.assign(z, z + cnt);
    if (c->geo_host.size() == cnt && memcmp(c->geo_host.data(), z, cnt * sizeof(double)) == 0) c->sym_z = c->sym_s;
    else c->sym_z = find_symmetry(c, "sym_z_tbl", z, nz, dim, c->sym_s_ctr, c->sym_s_refl);
    return c->sym_z;
}

// The host outputs of gpcsd_predict (the class API's predict(), gpcsd1d.py:286-293: the arrays ARE the result), a local of that call:
// the caller's arrays, which of them the chunked copy-out has filled (done), and the events it took from the pool.
static void sink_release(gpcsd_ctx *c, PredSink *sk);
struct PredSink {
    bool active = false;                  // every array is page-locked: a folded prediction may copy out under its last product
    double *sum[2] = {nullptr, nullptr}, *list[2] = {nullptr, nullptr};       // [0] csd, [1] lfp
    bool done[2] = {false, false};
    std::vector<hipEvent_t> events;
    gpcsd_ctx *owner = nullptr;           // gpcsd_predict: the end of the call releases (normal end, negative code, exception)
    ~PredSink() { sink_release(owner, this); }
};
// The one place that waits for the copies on stream4 and gives the events back; a replay comes here too (the outputs are then to
// be filled again).
static void sink_release(gpcsd_ctx *c, PredSink *sk) {
    if (!c || !sk) return;
    (void)hipStreamSynchronize(c->stream4);
    c->event_pool.insert(c->event_pool.end(), sk->events.begin(), sk->events.end());
    sk->events.clear();
    sk->done[0] = sk->done[1] = false;
}

// The paired call's log-likelihood (gpcsd_loglik_predict_async), whose products predict_fold queues among its own
struct PairLl {
    EigState *e;
    const FoldMode *fm;
    bool share_x, share_w;                // the prediction reads the log-likelihood's X = Y~ Q / its W~ = diag(U)^T X instead of forming its own
};

static PredCall pred_call(const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar, int type, bool lists, bool async) {
    PredCall q;
    q.hp = hp; q.z = z; q.nz = nz; q.tstar = tstar; q.ntstar = ntstar; q.type = type; q.want_lists = lists; q.async = async;
    return q;
}
static void check_predict_args(const gpcsd_ctx *c, const PredCall &q) {
    GP_REQUIRE(q.z && q.tstar && q.nz > 0 && q.ntstar > 0, -3, "predict: bad arguments");
    GP_REQUIRE(q.type >= 1 && q.type <= 3, -3, "predict: type must be CSD(1), LFP(2) or BOTH(3)");
    GP_REQUIRE(c->nt > 0 && q.ntstar == c->nt, -22,
               "predict: len(t)=%d must equal the training nt=%d (the reference's reshape raises ValueError, gpcsd1d.py:279)",
               q.ntstar, c->nt);
    GP_REQUIRE(c->d_lfp != nullptr, -4, "lfp not set (call gpcsd_set_lfp)");
}

// Which form a prediction takes, decided before anything is queued.  A folded side needs its outputs on a grid with the same
// symmetry (t* = t; mirror-symmetric sites); an unfolded side takes any sites / times.
struct PredPlan {
    enum Form { FULL, FOLD_T, FOLD } form = FULL;      // full size; temporal side folded, spatial side unfolded; folded on both sides
    bool fold_s() const { return form == FOLD; }
    bool tri = false;           // in the basis U (x) Q (predict_tridiag_applies)
    FoldMode fm;                // the decision; the caller takes the views again once its front half has started their generation
    SymDev sz;                  // the sites' orbit tables (identity for an unfolded spatial side)
    const double *Yf = nullptr, *dz = nullptr, *dts = nullptr;      // pred_operands
};
static PredPlan pred_plan(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar) {
    PredPlan P;
    P.fm = fold_mode(c, hp);
    const bool t_ok = P.fm.on && ntstar == c->nt &&
                      (!P.fm.ft.on || ((int)c->time_host.size() == c->nt &&
                                       memcmp(c->time_host.data(), tstar, (size_t)ntstar * sizeof(double)) == 0));
    if (!t_ok) return P;
    P.sz = P.fm.fs.on ? site_symmetry(c, z, nz, c->dim) : identity_sym(c, nz);
    P.form = PredPlan::FOLD;
    // sites without the electrodes' symmetry (the reference's own use: four off-grid depths): the spatial side unfolded, the
    // temporal side folded as ever -- not the full-size path
    if (!(P.sz.ns > 0 && P.sz.ns + P.sz.na == nz) && P.fm.fs.on && P.fm.ft.on) {
        P.form = PredPlan::FOLD_T;
        P.sz = identity_sym(c, nz);
    }
    if (!(P.sz.ns > 0 && P.sz.ns + P.sz.na == nz)) P.form = PredPlan::FULL;
    else P.tri = P.fm.ft.on && predict_tridiag_applies(P.fm.ft.ns, P.fm.ft.na, c->ntrials);
    return P;
}
// Behind the front half of a folded prediction: the views of the generation it started (fm), the folded data, and this call's sites
// and times on the device.  Returns true when sites or times had to be uploaded just now (on the main stream).
static bool pred_operands(gpcsd_ctx *c, const PredCall &q, PredPlan &P, const FoldMode &fm) {
    P.fm = fm;
    P.Yf = folded_lfp(c, fm);
    const long up0 = c->upload_count;
    P.dz = c->upload_cached<double>("pred_z", q.z, (size_t)q.nz * c->dim);
    P.dts = c->upload_cached<double>("pred_tstar", q.tstar, q.ntstar);
    return c->upload_count != up0;
}

// The resident outputs of output `which` (1 csd, 2 lfp): the sum, and the per-component list when wanted
struct PredOut {
    double *sum, *list;
};
static PredOut pred_out_bufs(gpcsd_ctx *c, int which, size_t out_elems, int C, bool want_lists) {
    return {c->buf<double>(which == 1 ? "pred_out_csd" : "pred_out_lfp", out_elems),
            want_lists ? c->buf<double>(which == 1 ? "pred_out_csd_list" : "pred_out_lfp_list", out_elems * C) : nullptr};
}
// ... into the caller's arrays (those of `sk` that are not null and that the chunked copy-out has not filled already)
static void pred_download(gpcsd_ctx *c, const PredCall &q, const PredSink &sk) {
    const size_t out_elems = (size_t)q.nz * q.ntstar * c->ntrials;
    for (int w = 0; w < 2; ++w) {
        if (!(q.type & (w + 1)) || sk.done[w]) continue;
        if (sk.sum[w]) c->download(sk.sum[w], c->bufs[w ? "pred_out_lfp" : "pred_out_csd"].p, out_elems * sizeof(double));
        if (sk.list[w])
            c->download(sk.list[w], c->bufs[w ? "pred_out_lfp_list" : "pred_out_csd_list"].p, out_elems * q.hp->n_temporal * sizeof(double));
    }
}

static bool pred_unfold_chunked(gpcsd_ctx *c, const PredCall &q, PredUnfoldDesc pu, int which0, size_t out_elems, hipStream_t s);

// The paired call's log-likelihood behind the wait for the spatial chain: its whole tail, in front of everything of the prediction that
// needs a decomposition -- it is what the caller waits for -- and the copy of its result into the next slot.
static void pair_ll_tail(gpcsd_ctx *c, const PairLl &ll, const double *Yf) {
    double *Wll = c->buf<double>("proj_W_ll", (size_t)c->nx * c->ntrials * c->nt);
    bool batched = true, wrote = false;
    if (ll.e->tri) wrote = loglik_tri_tail(c, *ll.e, *ll.fm, Wll, next_ll_slot(c));
    else batched = loglik_fold_tail(c, *ll.e, *ll.fm, Yf, Wll);
    (void)finish_loglik_async(c, *ll.e, !batched, wrote);
}

// predict_impl in the folded basis (see FoldMode).  Prediction sites and times must share the symmetry of the grids:
//   out_c = Fz^T [ diag_p( (Kc_pp^T U_p) ) Bm~ diag_q( V_q^T Kt*_c,qq ) ] Ft   with Bm~ = (diag(U)^T Y~ diag(V)) / D~ ,
// every flat GEMM split in its two parity blocks; the last pass unfolds sites and times while it transposes.
static int predict_fold(gpcsd_ctx *c, const PredCall &q, const PredPlan &P, EigState &e) {
    const gpcsd_hparams *hp = q.hp;
    const FoldMode &fm = P.fm;
    const SymDev &sz = P.sz;
    const double *Yf = P.Yf, *dz = P.dz, *dts = P.dts;
    const int nz = q.nz, type = q.type;
    const bool want_lists = q.want_lists, prelude_side = q.prelude_side;
    const Geo g = resident_geo(c);
    const int nx = c->nx, nt = c->nt, R = c->ntrials, C = hp->n_temporal;
    const long RT = (long)R * nt;
    const int ns = fm.fs.ns, na = fm.fs.na, nts = fm.ft.ns, nta = fm.ft.na, nzs = sz.ns, nza = sz.na;
    hipStream_t s = c->stream;
    // The paired call (q.ll) with equal temporal hyper-parameters (share_x): X = Y~ Q is the log-likelihood's own product -- the two
    // replicas of the temporal problem are the same matrix, decomposed by the same deterministic launches into the same bits, so a
    // second product would only recompute it (0.1 ms of MFMA time and 154 MB of traffic per cfg3 step).  With the spatial
    // eigenvectors shared as well (share_w): W~ = diag(U)^T X is the log-likelihood's too.  The buffers those flags select:
    const bool shared_x = q.ll && q.ll->share_x, shared_w = q.ll && q.ll->share_w;
    const char *xname = shared_x ? "ll_X" : "pred_X", *wname = shared_w ? "proj_W_ll" : "proj_W";
    double *W = c->buf<double>(wname, (size_t)nx * RT);
    double *Bm = c->buf<double>("pred_B", (size_t)nx * RT);
    const double *t = (const double *)c->bufs["time_t"].p;
    double *Kc = c->buf<double>("pred_Kcross", (size_t)nx * nz);
    const size_t kcf_sz = (size_t)ns * nzs + (size_t)na * nza;
    double *Kcf = c->buf<double>("pred_Kcross_fold", 2 * kcf_sz);
    double *S = c->buf<double>("pred_S", (size_t)nz * RT);
    // comp~ and Pcat keep every (parity, component) block of columns on a 128-byte boundary (block widths padded to a multiple
    // of 16 doubles): the final relayout pass reads comp~ in 16-column pieces per trial row, and unaligned blocks (250 columns)
    // made every piece straddle two cache lines -- 291 MB fetched for 154 MB of comp~ per cfg3 step
    const int ntsP = (nts + 15) & ~15, ntaP = (nta + 15) & ~15;
    // (+16: a row stride that is a power of two -- 1024 doubles at nt = 500 -- walks the same HBM channels row after row)
    const long ldcomp = (long)C * (ntsP + ntaP) + 16;
    double *comp = c->buf<double>("pred_comp", std::max((size_t)C * nz * RT, (size_t)nz * R * ldcomp));
    double *Kts = c->buf<double>("pred_Ktstar", (size_t)C * nt * nt);
    const size_t ktf_sz = (size_t)nts * nts + (size_t)nta * nta;
    double *Ktf = c->buf<double>("pred_Ktstar_fold", (size_t)C * ktf_sz);
    const size_t m1_sz = (size_t)nzs * ns + (size_t)nza * na;
    double *M1 = c->buf<double>("pred_M1", 2 * std::max(m1_sz, (size_t)nz * nx));
    const size_t pc_s = (size_t)nts * C * ntsP;                     // Pcat_sym: nts rows of C * ntsP columns; Pcat_anti follows
    double *Pc = c->buf<double>("pred_Pc", std::max(pc_s + (size_t)nta * C * ntaP, (size_t)C * nt * nt));
    const size_t out_elems = (size_t)nz * RT;
    ++c->fold_gemm_calls;
    // what needs neither decomposition runs first, beside both chains: the cross-covariances and the prediction-time Grams,
    // folded
    // (prelude_side -- the paired call: on stream5, behind the previous call's side products there; the main stream is still busy
    // with the previous prediction and has the log-likelihood's products to queue first)
    hipStream_t sp = prelude_side ? c->stream5 : s;
    if (prelude_side && c->m1_read_queued) GP_HIP(hipStreamWaitEvent(sp, c->ev_m1, 0));     // the last reader of Kc~ on the main stream
    for (int which = 1; which <= 2; ++which) {
        if (!(type & which)) continue;
        double *kf = Kcf + (size_t)(which - 1) * kcf_sz;
        if (which == 1) build_kphig(c, g, hp->R, hp->eps, hp->ell_s, dz, nz, Kc, sp);       // gpcsd1d.py:273
        else build_kphi(c, g, hp->R, hp->eps, hp->ell_s, dz, nz, 0.0, Kc, sp);              // gpcsd1d.py:275
        k_sym_fold_rect(c, Kc, nz, fm.sym_s, sz, kf, kf + (size_t)ns * nzs, sp);
    }
    for (int cc = 0; cc < C; ++cc) {
        temporal_cross_gram(c, hp, cc, dts, nt, t, nt, Kts + (size_t)cc * nt * nt, sp);
        k_sym_fold_rect(c, Kts + (size_t)cc * nt * nt, nt, fm.sym_t, fm.sym_t, Ktf + cc * ktf_sz,
                        Ktf + cc * ktf_sz + (size_t)nts * nts, sp);
    }
    if (prelude_side) GP_HIP(hipEventRecord(c->ev_prelude, sp));
    // then everything that needs only the spatial eigenvectors, beside the temporal eigensolver.  In the tridiagonal form (EigState::tri)
    // X = Y~ Q needs the temporal tridiagonalisation + Q only and is queued in front of the wait for the spatial chain -- the
    // log-likelihood's in the paired call, this call's own otherwise
    if (q.ll && q.ll->e->tri) loglik_tri_pre(c, *q.ll->e, *q.ll->fm, Yf, nullptr);
    if (e.tri && !q.ll) loglik_tri_pre(c, e, fm, Yf, &q);
    join_spatial(c, e);
    if (q.ll) pair_ll_tail(c, *q.ll, Yf);
    // (the paired call's own X: behind the log-likelihood's tail -- in front of it the product delays the result the caller is waiting
    // for by its 0.09 ms)
    if (e.tri && q.ll && !shared_x) loglik_tri_pre(c, e, fm, Yf, &q);
    if (e.tri && shared_x) {              // (the wait for Q the skipped product would have queued; the log-likelihood's tail has passed it)
        if (e.wait_q) GP_HIP(hipStreamWaitEvent(s, c->ev_q[c->tgen], 0));
        e.wait_q = false;
    }
    if (!shared_w) fold_proj_spatial(c, fm.fs, e.tri ? c->buf<double>(xname, (size_t)nx * RT) : Yf, W, RT, s);   // W~ = diag(U)^T Y~ (or of Y~ Q)
    if (prelude_side) GP_HIP(hipStreamWaitEvent(s, c->ev_prelude, 0));
    for (int which = 1; which <= 2; ++which) {
        if (!(type & which)) continue;
        const double *kf = Kcf + (size_t)(which - 1) * kcf_sz;
        for (int p = 0; p < 2; ++p) {
            const int np = p ? na : ns, nzp = p ? nza : nzs;
            if (np == 0 || nzp == 0) continue;
            GemmDesc gm;                  // M1_p[zq][x'] = sum_xq Kc~_pp[xq][zq] U_p[xq][x']
            gm.M = nzp; gm.N = np; gm.K = np;
            gm.A = kf + (p ? (size_t)ns * nzs : 0); gm.lda = nzp; gm.transA = true;
            gm.B = fm.fs.U + (p ? (size_t)ns * ns : 0); gm.ldb = np;
            gm.C = M1 + (size_t)(which - 1) * m1_sz + (p ? (size_t)nzs * ns : 0); gm.ldc = np;
            gm.prof_name = "gemm_pred_M1";
            gemm_f64(c, gm, s);
        }
    }
    GP_HIP(hipEventRecord(c->ev_m1, s));
    c->m1_read_queued = true;
    // the temporal basis of everything below: the eigenvectors V_p (blocks of fm.ft.U), or in the tridiagonal form the orthogonal
    // factors Q_p of the tridiagonalisation (replica e.tri_rep of the temporal classes)
    const double *Tb[2] = {fm.ft.U, fm.ft.U + (size_t)nts * nts};
    if (e.tri) {
        const char *const *tg = eigh_fold_tags(c, 1);
        for (int p = 0; p < 2; ++p) {
            const int np = p ? nta : nts;
            Tb[p] = np > 0 ? eigh_Q_view(c, tg[p], np, e.tri_count) + (size_t)e.tri_rep * np * np : nullptr;
        }
    } else {
        join_temporal(c, e, &fm, false);  // predict never reads sum(log D)
    }
    GemmDesc g2[2];                       // Bm~[:, p block] = (W~[:, p block] V_p) / D~
    for (int p = 0; p < 2; ++p) {
        const int np = p ? nta : nts, c0 = p ? nts : 0;
        g2[p].M = nx * R; g2[p].N = np; g2[p].K = np;
        g2[p].A = W + c0; g2[p].lda = nt;
        g2[p].B = Tb[p]; g2[p].ldb = np;
        g2[p].C = Bm + c0; g2[p].ldc = nt;
        g2[p].epi = EPI_DIV_D; g2[p].D = e.Dinv + c0; g2[p].rdiv = R; g2[p].ldd = nt;
        g2[p].prof_name = "gemm_pred_temporal_div";
    }
    // Pcat = V^T Kt*~ needs the temporal eigenvectors and the folded prediction-time Grams only: it runs on a stream of its
    // own beside the large Bm~ / S~ products of the main stream instead of in front of them (two small launches off the
    // serial tail) -- not on stream2, where it would sit between this call's temporal chain and the next call's
    GP_HIP(hipEventRecord(c->ev_aux, s));                            // Kt*~ and the temporal eigenvectors are complete here
    GP_HIP(hipStreamWaitEvent(c->stream5, c->ev_aux, 0));
    for (int p = 0; p < 2; ++p) {
        const int np = p ? nta : nts, npP = p ? ntaP : ntsP;
        if (np == 0) continue;
        GemmDesc gp;                      // Pcat_p[i'][cc*npP + b] = sum_j V_p[j][i'] Kt*~_cc,pp[j][b], all components batched
        gp.M = np; gp.N = np; gp.K = np;
        gp.A = Tb[p]; gp.lda = np; gp.transA = true;
        gp.B = Ktf + (p ? (size_t)nts * nts : 0); gp.ldb = np;
        gp.C = Pc + (p ? pc_s : 0); gp.ldc = (long)C * npP;
        gp.batch = C; gp.sA = 0; gp.sB = (long)ktf_sz; gp.sC = npP;
        gp.prof_name = "gemm_pred_Pc";
        gemm_f64(c, gp, c->stream5);
    }
    GP_HIP(hipEventRecord(c->ev_pc, c->stream5));
    c->tl("Pc end (s5)", c->stream5);
    if (e.tri) {
        // Bm~ = the solutions of the shifted tridiagonal systems (es[x'] m T_p + sig2 I) b = w, row by row of W~ = diag(U)^T Y~ Q
        const TriOperands o = tri_operands(c, e, fm, s);
        k_tridiag_solve(c, W, Bm, fm.fs.w, o.d, o.e, o.amax, e.d_sig, nx, R, nt, o.np, o.c0, s, /*pass=*/0, /*hint=*/q.solve_pass);
        GP_HIP(hipEventRecord(c->ev_tri_done[c->tgen], s));     // the last reader of Q / the tridiagonal on this stream
        c->tri_reader_queued[c->tgen] = true;
    } else {
        gemm_pair(c, g2[0], g2[1], s);
    }
    for (int which = 1; which <= 2; ++which) {
        if (!(type & which)) continue;
        const PredOut out = pred_out_bufs(c, which, out_elems, C, want_lists);
        GemmDesc g5[2], g6[2];
        for (int p = 0; p < 2; ++p) {     // S~[p rows] = M1_p Bm~[p rows]
            const int np = p ? na : ns, nzp = p ? nza : nzs;
            g5[p].M = nzp; g5[p].N = (int)RT; g5[p].K = np;
            g5[p].A = M1 + (size_t)(which - 1) * m1_sz + (p ? (size_t)nzs * ns : 0); g5[p].lda = np;
            g5[p].B = Bm + (p ? (size_t)ns * RT : 0); g5[p].ldb = RT;
            g5[p].C = S + (p ? (size_t)nzs * RT : 0); g5[p].ldc = RT;
            g5[p].prof_name = "gemm_pred_cross";
        }
        gemm_pair(c, g5[0], g5[1], s);
        if (which == 1 || !(type & 1)) GP_HIP(hipStreamWaitEvent(s, c->ev_pc, 0));     // Pcat (stream5) before its first use
        for (int p = 0; p < 2; ++p) {     // comp~[(zq, r)][p][cc][b] = sum_i' S~[(zq, r)][p block i'] Pcat_p[i'][cc*npP + b]
            const int np = p ? nta : nts, npP = p ? ntaP : ntsP, c0 = p ? nts : 0;
            // (the padding columns between two components are computed along -- whatever Pcat holds there only reaches comp~'s
            // own padding columns, which nobody reads; the last component's padding is left out)
            g6[p].M = nz * R; g6[p].N = (C - 1) * npP + np; g6[p].K = np;
            g6[p].A = S + c0; g6[p].lda = nt;
            g6[p].B = Pc + (p ? pc_s : 0); g6[p].ldb = (long)C * npP;
            g6[p].C = comp + (p ? (size_t)C * ntsP : 0); g6[p].ldc = ldcomp;
            g6[p].prof_name = "gemm_pred_tstar";
        }
        if (gemm_pred_unfold_supported(C, (long)nz * R, nt)) {
            // ... as ONE launch whose epilogue unfolds in site and time, turns (r, t) into (t, r) and sums the components:
            // comp~ is never written (gemm_f64.hip: gemm_pred_unfold_kernel)
            PredUnfoldDesc pu{};
            pu.S = S; pu.lds = nt;
            pu.Pc[0] = Pc; pu.Pc[1] = Pc + pc_s;
            pu.ldp[0] = (long)C * ntsP; pu.ldp[1] = (long)C * ntaP;
            pu.npP[0] = ntsP; pu.npP[1] = ntaP;
            pu.K[0] = nts; pu.K[1] = nta;
            pu.kcol0[0] = 0; pu.kcol0[1] = nts;
            pu.nb = nts; pu.nba = nta;
            pu.ncolS = (long)nzs * R; pu.ncolA = (long)nza * R; pu.anti_row0 = (long)nzs * R;
            pu.R = R; pu.nt = nt; pu.C = C;
            pu.sz = sz; pu.st = fm.sym_t;
            pu.list = out.list; pu.list_stride = (long)out_elems; pu.sum = out.sum;
            if (!pred_unfold_chunked(c, q, pu, which - 1, out_elems, s)) gemm_pred_unfold(c, pu, s);
        } else {
            gemm_pair(c, g6[0], g6[1], s);
            k_unfold_swap_sum(c, comp, C, out.list, (long)out_elems, out.sum, R, nt, sz, fm.sym_t, s, ntsP, ntaP, ldcomp);
        }
    }
    c->tl("predict end (main)", s);
    if (q.async && c->prof_mode != 1) {   // results stay on the device: return with the tail still in flight
        c->async_pending = true;
        c->status_zeroed = false;
        return 0;
    }
    return finish_call(c, e, nullptr, 0);
}

// ------------------------------------------------------------------------------------------------------------------
// gpcsd_predict with host outputs (the class API's predict(), gpcsd1d.py:286-293: the arrays ARE the result): the copy of 231 MB
// at cfg3 is 4 ms on the host link against ~1 ms of device work, and it used to start when the last launch had finished.  The
// fused last product writes whole output rows [z][t][r] per site orbit, so it is launched in chunks of column tiles and a chunk's
// finished rows leave through the DMA engine (stream4) while the next chunk computes: the copy starts one chunk (~40 us) after
// the product instead of ~220 us.  Rows: orbit a writes z = rep_i[a] and rep_j[a] -- runs of consecutive rows are one copy each
// (a mirror-symmetric probe gives two runs per chunk).  Returns false when it does not apply (the caller launches the product whole).
// gpcsd_predict_chunked_copy(ctx, 0) / GPCSD_PRED_CHUNKED=0: A/B.
static bool pred_unfold_chunked(gpcsd_ctx *c, const PredCall &q, PredUnfoldDesc pu, int which0, size_t out_elems, hipStream_t s) {
    if (!q.sink) return false;
    PredSink &sk = *q.sink;
    const int nz = q.nz;
    const bool want_lists = q.want_lists;
    if (!sk.active || !c->pred_chunked || !sk.sum[which0] || (want_lists && !sk.list[which0]) || c->prof_mode == 1) return false;
    const auto it = c->sym_host.find(pu.sz.rep_i);
    if (it == c->sym_host.end()) return false;
    const int nso = pu.sz.ns;                                         // site orbits
    if ((int)it->second.size() < 2 * nso || pu.ncolS != (long)nso * pu.R) return false;
    const int *rep_i = it->second.data(), *rep_j = rep_i + nso;
    const long tiles_all = (pu.ncolS + PRED_UNFOLD_BN - 1) / PRED_UNFOLD_BN;
    const size_t row_bytes = (size_t)pu.nt * pu.R * sizeof(double);
    const size_t total = (size_t)nz * row_bytes * (1 + (want_lists ? pu.C : 0));
    if (total < ((size_t)32 << 20) || tiles_all < 16) return false;   // small outputs: one launch, one copy
    // chunk boundaries in eighths of the tiles (GPCSD_PRED_CHUNKS="1,8": a first eighth, then the rest).  Every copy costs the DMA
    // engine ~10 us of set-up and a chunk is two runs of rows x (1 + C) arrays: six equal chunks (36 copies) were SLOWER than one
    // copy behind the whole product (5.60 against 5.41 ms per call at cfg3) -- what pays is starting the first copy early.
    static const std::vector<int> cuts = [] {
        std::vector<int> v;
        const char *e = getenv("GPCSD_PRED_CHUNKS");
        for (const char *p = e ? e : "1,8"; *p;) {
            v.push_back(atoi(p));
            while (*p && *p != ',') ++p;
            if (*p == ',') ++p;
        }
        if (v.empty() || v.back() != 8) v.push_back(8);
        return v;
    }();
    const int nchunk = (int)cuts.size();
    hipStream_t sc = c->stream4;
    std::vector<char> have((size_t)nz, 0);
    int done_orbits = 0;
    for (int k = 0; k < nchunk; ++k) {
        pu.tile_c0 = k == 0 ? 0 : tiles_all * cuts[k - 1] / 8;
        pu.tile_c1 = tiles_all * cuts[k] / 8;
        gemm_pred_unfold(c, pu, s);
        // orbits all of whose R columns lie in front of the end of this chunk are complete
        const int upto = (k + 1 == nchunk) ? nso : (int)std::min<long>(nso, pu.tile_c1 * PRED_UNFOLD_BN / pu.R);
        if (upto <= done_orbits) continue;
        std::vector<int> rows;
        for (int a = done_orbits; a < upto; ++a) {
            for (int z : {rep_i[a], rep_j[a]})
                if (z >= 0 && z < nz && !have[z]) { have[z] = 1; rows.push_back(z); }
        }
        done_orbits = upto;
        std::sort(rows.begin(), rows.end());
        hipEvent_t ev = c->get_event();
        GP_HIP(hipEventRecord(ev, s));
        GP_HIP(hipStreamWaitEvent(sc, ev, 0));
        sk.events.push_back(ev);                                  // (back to the pool once gpcsd_predict has synchronised)
        for (size_t i = 0; i < rows.size();) {
            size_t j = i + 1;
            while (j < rows.size() && rows[j] == rows[j - 1] + 1) ++j;
            const size_t off = (size_t)rows[i] * (size_t)pu.nt * pu.R, cnt = (j - i) * row_bytes;
            GP_HIP(hipMemcpyAsync(sk.sum[which0] + off, pu.sum + off, cnt, hipMemcpyDeviceToHost, sc));
            if (want_lists)
                for (int cc = 0; cc < pu.C; ++cc)
                    GP_HIP(hipMemcpyAsync(sk.list[which0] + (size_t)cc * out_elems + off, pu.list + (size_t)cc * pu.list_stride + off, cnt,
                                          hipMemcpyDeviceToHost, sc));
            i = j;
        }
    }
    for (int z = 0; z < nz; ++z)
        if (!have[z]) return true;                                    // (cannot happen: every site belongs to an orbit) -- not marked done
    sk.done[which0] = true;
    ++c->pred_chunked_calls;
    return true;
}

// What the full-size (unfolded) predictions share up to the last two products: W = Qs^T Y, the cross-covariances with
// M1 = Kc^T Qs per requested output and the (ntstar, nt) temporal cross Grams queued beside the temporal eigensolver, then
// Bm = (W Qt) / D.
//   invy = (Qs (x) Qt) vec(Bm) (gpcsd1d.py:262-265) is never formed: the cross-covariance contraction
//   out_c = Kc^T Qs Bm Qt^T Kt*_c  is re-associated as  (Kc^T Qs) Bm (Qt^T Kt*_c),
// i.e. two small (n^3) products M1, Pc and two flat GEMMs, instead of back-projecting to the original bases first
// (saves 2 nx^2 nt + 2 nx nt^2 flops per trial; identical up to rounding).
struct PredFullFront {
    double *Bm = nullptr, *M1 = nullptr, *Kts = nullptr;     // (nx, R, nt); (2, nz, nx): CSD, LFP; (C, ntstar, nt) = cov_c.compute_Kt(tstar)
    const double *dz = nullptr, *dts = nullptr;              // the call's sites and times on the device ("pred_z", "pred_tstar")
};
// The part of it that reads no trial data (all a posterior variance needs): sites and times to the device, the cross-covariances
// with M1 = Kc^T Qs per requested output and the cross Grams -- everything that needs only Qs, queued before the join, i.e. it runs
// beside the temporal eigensolver -- then the join.
static void pred_cross_front(gpcsd_ctx *c, const gpcsd_hparams *hp, EigState &e, const double *z, int nz, const double *tstar, int ntstar,
                             int type, PredFullFront &f) {
    const Geo g = resident_geo(c);
    const int nx = c->nx, nt = c->nt, C = hp->n_temporal;
    hipStream_t s = c->stream;
    const double *dz = f.dz = c->upload_cached<double>("pred_z", z, (size_t)nz * g.dim);
    const double *dts = f.dts = c->upload_cached<double>("pred_tstar", tstar, ntstar);
    const double *t = (const double *)c->bufs["time_t"].p;
    double *Kc = c->buf<double>("pred_Kcross", (size_t)nx * nz);
    f.Kts = c->buf<double>("pred_Ktstar", (size_t)C * ntstar * nt);
    f.M1 = c->buf<double>("pred_M1", (size_t)2 * nz * nx);
    for (int which = 1; which <= 2; ++which) {
        if (!(type & which)) continue;
        if (which == 1) build_kphig(c, g, hp->R, hp->eps, hp->ell_s, dz, nz, Kc, s);        // gpcsd1d.py:273
        else build_kphi(c, g, hp->R, hp->eps, hp->ell_s, dz, nz, 0.0, Kc, s);               // gpcsd1d.py:275
        GemmDesc gm;                      // M1[z][x'] = sum_x Kc[x][z] Qs[x][x']
        gm.M = nz; gm.N = nx; gm.K = nx;
        gm.A = Kc; gm.lda = nz; gm.transA = true; gm.B = e.Qs; gm.ldb = nx; gm.C = f.M1 + (size_t)(which - 1) * nz * nx; gm.ldc = nx;
        gm.prof_name = "gemm_pred_M1";
        gemm_f64(c, gm, s);
    }
    GP_HIP(hipEventRecord(c->ev_m1, s));          // (a later paired call rewrites the cross-covariances on stream5)
    c->m1_read_queued = true;
    for (int cc = 0; cc < C; ++cc)
        temporal_cross_gram(c, hp, cc, dts, ntstar, t, nt, f.Kts + (size_t)cc * ntstar * nt, s);
    join_temporal(c, e, nullptr, false);      // predict never reads sum(log D)
}
// The part of it that reads the trials and neither sites nor times (all the leave-one-out scores need), in two steps because the
// second one needs the joined temporal side: W = Qs^T Y (spatial side only), then Bm = (W Qt) / D.
// Y: R trials -- the resident data, or the residuals of a chunk of posterior draws -- as [x][r][t].
static void pred_data_spatial(gpcsd_ctx *c, EigState &e, double *W, const double *Y, int R) {
    const int nx = c->nx;
    const long RT = (long)R * c->nt;
    GemmDesc g1;                          // W = Qs^T Y
    g1.M = nx; g1.N = (int)RT; g1.K = nx;
    g1.A = e.Qs; g1.lda = nx; g1.transA = true;
    g1.B = Y; g1.ldb = RT; g1.C = W; g1.ldc = RT;
    g1.prof_name = "gemm_proj_spatial";
    gemm_f64(c, g1, c->stream);
}
static void pred_data_temporal(gpcsd_ctx *c, EigState &e, const double *W, double *Bm, int R) {
    const int nx = c->nx, nt = c->nt;
    GemmDesc g2;                          // Bm = (W Qt) / D
    g2.M = nx * R; g2.N = nt; g2.K = nt;
    g2.A = W; g2.lda = nt; g2.B = e.Qt; g2.ldb = nt; g2.C = Bm; g2.ldc = nt;
    g2.epi = EPI_DIV_D; g2.D = e.Dinv; g2.rdiv = R; g2.ldd = nt;
    g2.prof_name = "gemm_pred_temporal_div";
    gemm_f64(c, g2, c->stream);
}
static PredFullFront predict_full_front(gpcsd_ctx *c, const gpcsd_hparams *hp, EigState &e, const double *z, int nz, const double *tstar,
                                        int ntstar, int type) {
    const long RT = (long)c->ntrials * c->nt;
    double *W = c->buf<double>("proj_W", (size_t)c->nx * RT);
    PredFullFront f;
    f.Bm = c->buf<double>("pred_B", (size_t)c->nx * RT);
    pred_data_spatial(c, e, W, c->d_lfp, c->ntrials);
    pred_cross_front(c, hp, e, z, nz, tstar, ntstar, type, f);
    pred_data_temporal(c, e, W, f.Bm, c->ntrials);
    return f;
}
// S[z][(r,i')] = sum_x' M1[z][x'] Bm[x'][(r,i')] with the M1 of output `which` (1 csd, 2 lfp); RT = columns of Bm: trials x nt
static void pred_cross_S(gpcsd_ctx *c, const double *M1, int which, int nz, const double *Bm, double *S, long RT) {
    const int nx = c->nx;
    GemmDesc g5;
    g5.M = nz; g5.N = (int)RT; g5.K = nx;
    g5.A = M1 + (size_t)(which - 1) * nz * nx; g5.lda = nx; g5.B = Bm; g5.ldb = RT; g5.C = S; g5.ldc = RT;
    g5.prof_name = "gemm_pred_cross";
    gemm_f64(c, g5, c->stream);
}

// Posterior mean into ctx-owned device buffers, already in the reference's output layout (z, t, trial):
//   pred_out_csd / pred_out_lfp            (nz, ntstar, R)
//   pred_out_csd_list / pred_out_lfp_list  (C, nz, ntstar, R)     when want_lists
static int predict_impl(gpcsd_ctx *c, const PredCall &q) {
    check_predict_args(c, q);
    const gpcsd_hparams *hp = q.hp;
    const double *z = q.z, *tstar = q.tstar;
    const int nz = q.nz, ntstar = q.ntstar, type = q.type;
    const bool want_lists = q.want_lists;
    PredPlan P = pred_plan(c, hp, z, nz, tstar, ntstar);
    if (P.form != PredPlan::FULL) {
        // the chains go first (they need no upload of this call), then the host-side uploads
        // no jitter in predict (gpcsd1d.py:258); X = Y~ Q goes through loglik_tri_pre: stage 5 may apply
        EigState ef = front_half(c, hp, 0.0, false, /*join_s=*/false, /*want_tri=*/P.tri, P.fold_s() ? -1 : 1, /*x_via_tri_pre=*/P.tri);
        pred_operands(c, q, P, fold_mode(c, hp, P.fold_s()));
        return predict_fold(c, q, P, ef);
    }
    EigState e = front_half(c, hp, 0.0);           // no jitter in predict (gpcsd1d.py:258)
    const int nt = c->nt, R = c->ntrials, C = hp->n_temporal;
    const long RT = (long)R * nt;
    hipStream_t s = c->stream;
    // Ktstar_c = cov_c.compute_Kt(tstar): (ntstar, nt); its FIRST axis is contracted with the training
    // time index (reference quirk when tstar != t)      gpcsd1d.py:277-279
    const PredFullFront f = predict_full_front(c, hp, e, z, nz, tstar, ntstar, type);
    double *const Bm = f.Bm, *const M1 = f.M1, *const Kts = f.Kts;
    double *S = c->buf<double>("pred_S", (size_t)nz * RT);
    double *comp = c->buf<double>("pred_comp", (size_t)C * nz * RT);
    double *Pc = c->buf<double>("pred_Pc", (size_t)C * nt * nt);
    const size_t out_elems = (size_t)nz * RT;
    for (int which = 1; which <= 2; ++which) {
        if (!(type & which)) continue;
        const PredOut out = pred_out_bufs(c, which, out_elems, C, want_lists);
        pred_cross_S(c, M1, which, nz, Bm, S, RT);
        for (int cc = 0; cc < C; ++cc) {
            GemmDesc gp;                  // Pcat[i'][cc*nt + t'] = sum_j Qt[j][i'] Ktstar_cc[j][t']
            gp.M = nt; gp.N = nt; gp.K = ntstar;
            gp.A = e.Qt; gp.lda = nt; gp.transA = true; gp.B = Kts + (size_t)cc * ntstar * nt; gp.ldb = nt;
            gp.C = Pc + (size_t)cc * nt; gp.ldc = (long)C * nt;
            gp.prof_name = "gemm_pred_Pc";
            gemm_f64(c, gp, s);
        }
        // All temporal components in ONE flat GEMM: out[(z,r)][cc*nt + t'] = sum_i' S[(z,r)][i'] Pcat[i'][cc*nt + t'],
        // then one pass writes every component in the reference's (z, t, r) layout plus their sum (no read-modify-write
        // epilogue, one launch instead of C, a single relayout pass instead of C + 1).
        GemmDesc g6;
        g6.M = nz * R; g6.N = C * nt; g6.K = nt;
        g6.A = S; g6.lda = nt; g6.B = Pc; g6.ldb = (long)C * nt; g6.C = comp; g6.ldc = (long)C * nt;
        g6.prof_name = "gemm_pred_tstar";
        gemm_f64(c, g6, s);
        k_swap_last2_sum(c, comp, C, out.list, (long)out_elems, out.sum, nz, R, nt, s);     // (z,r,c,t) -> (c,z,t,r), sum over c
    }
    return finish_call(c, e, nullptr, 0);
}

// ------------------------------------------------------------------------------------------------------------------
// loglik + predict as ONE queued call with the four decompositions batched two by two.
//
// Chains of small dependent launches do not overlap on this part (1.4x at best, however many queues), but
// replicas inside one chain are nearly free (gpcsd_eigh_batch: 8 problems in 1.09 ms against 0.93 ms for one).  So when a
// caller wants the log-likelihood at one hyper-parameter set and the prediction at another (the same set without jitter, in
// practice), the two temporal problems go through ONE chain as two replicas and the two spatial problems through another:
// two chains per pair of calls instead of four.  Every problem is still solved (nothing is reused between the two unless the
// decomposition cache is on and the temporal hyper-parameters coincide: then that side is solved once, as the cache would).
// Results: the bits of the two calls made separately.
struct PairFront {
    EigState e[2];
    FoldMode fm[2];
    bool share_s = false;       // one spatial decomposition served both sets (gpcsd_ctx::pair_share_s)
};

static bool same_temporal(const gpcsd_hparams *a, const gpcsd_hparams *b) {
    if (a->n_temporal != b->n_temporal) return false;
    for (int i = 0; i < a->n_temporal; ++i)
        if (a->kind[i] != b->kind[i] || a->ell_t[i] != b->ell_t[i] || a->sigma2_t[i] != b->sigma2_t[i]) return false;
    return true;
}

// Both sets decomposed, set b's results at replica b of the generation just started (folded-basis callers only).
// pred_tri: the prediction (set 1) takes the tridiagonal form too, so that nobody reads the temporal spectrum or eigenvectors: the
// staged temporal chain then stops behind stages 1 and 3.
// x_via_tri_pre: the log-likelihood forms X = Y~ Q through loglik_tri_pre (a pipelined stage 5 may apply: TChain).
// fold_s = false: the tails take the spatial side unfolded (merged eigenvectors; the eigensolver still folds it internally).
static void front_half_pair(gpcsd_ctx *c, const gpcsd_hparams *const hp[2], const double jitter[2], PairFront &out, bool pred_tri,
                            bool x_via_tri_pre, bool fold_s = true) {
    const Geo g = resident_geo(c);
    const int nx = c->nx, nt = c->nt;
    const long nxx = (long)nx * nx, ntt = (long)nt * nt;
    hipStream_t s = c->stream, s2 = c->stream2, s3 = c->stream3;
    const SymDev *sym_s = c->sym_s.ns > 0 ? &c->sym_s : nullptr, *sym_t = c->sym_t.ns > 0 ? &c->sym_t : nullptr;
    const double *t = (const double *)c->bufs["time_t"].p;
    // replicas of the temporal problem: ONE when the two sets have the same temporal hyper-parameters (every loglik -> predict
    // pair: the jitter is spatial) and either the decomposition cache or the pair's sharing of X says that equal sides are formed
    // once -- the second replica would be the same launches on the same matrix, the same bits
    const int nT = (same_temporal(hp[0], hp[1]) && (c->decomp_cache_on || c->pair_share_x)) ? 1 : 2;
    double *scal = c->buf<double>("scal_status", gpcsd_ctx::RESULT_DOUBLES);
    int *status = reinterpret_cast<int *>(scal + gpcsd_ctx::SCAL_N);
    const bool clear_now = !c->status_zeroed && !c->async_pending;
    if (clear_now) GP_HIP(hipMemsetAsync(status, 0, gpcsd_ctx::STATUS_N * sizeof(int), s));
    c->status_zeroed = false;
    begin_generation(c, 1, s2, clear_now);
    begin_generation(c, 0, s3, clear_now);
    // inputs and outputs (of the generations just started), two replicas each.  The inputs have names of their own: the
    // one-chain form below reads them on stream2, the separate calls' spatial chain writes "Ks" on stream3.
    double *Ks = c->buf<double>("Ks_pair", (size_t)nxx * 2), *Kt = c->buf<double>("Kt_pair", (size_t)ntt * 2);
    double *Qs = c->buf<double>(gen_name(c, 0, "Qs"), (size_t)nxx * 2), *es = c->buf<double>(gen_name(c, 0, "es"), (size_t)nx * 2);
    double *Qt = c->buf<double>(gen_name(c, 1, "Qt"), (size_t)ntt * 2), *et = c->buf<double>(gen_name(c, 1, "et"), (size_t)nt * 2);
    const FoldView vs = sym_s ? eigh_fold_view(c, 0, sym_s, nx, 2) : FoldView(), vt = sym_t ? eigh_fold_view(c, 1, sym_t, nt, 2) : FoldView();
    c->tl("call start (main)", s);
    // Gram matrices.  Temporal (stream2): replica b = Kt(hp[b]).  Spatial (stream3): replica b = Ks(hp[b]) + jitter[b] I; with
    // equal spatial hyper-parameters -- the usual pair -- the two differ by the diagonal shift only, so the matrix is
    // assembled once and copied (the same GEMM output plus the same diagonal add: the same bits).
    // The temporal chain is the critical path of the call: its first part is queued before the host spends its time on the launches
    // of the spatial Gram assembly (status words [1], [3]; one replica when the problem is shared -- decomposition cache on, equal
    // temporal hyper-parameters).  (All four problems in ONE chain was measured slower, 1.38 against 1.18 ms per cfg3 step: with
    // two chains the log-likelihood's spatial projection runs under the end of the temporal one.)
    TChain tc(c, sym_t, nt, /*host_kt=*/false);           // (the paired call is refused for host temporal Grams)
    tc.Kt = Kt; tc.et = et; tc.Qt = Qt; tc.hp = hp; tc.t = t; tc.nT = nT;
    tc.need_merged = false; tc.status = status; tc.stride = 2;
    tc.tri = tc.staged && pred_tri; tc.x_via_tri_pre = x_via_tri_pre; tc.scope2 = "eigh_temporal_stage2";
    auto build_kts = [&](hipStream_t st) {
        for (int b = 0; b < nT; ++b) build_kt(c, hp[b], t, nt, t, nt, Kt + b * ntt, st);
    };
    const bool same_ks = hp[0]->R == hp[1]->R && hp[0]->ell_s[0] == hp[1]->ell_s[0] &&
                         (g.dim == 1 || (hp[0]->eps == hp[1]->eps && hp[0]->ell_s[1] == hp[1]->ell_s[1]));
    // Equal spatial hyper-parameters: the two matrices are Ks + jitter[b] I -- the same eigenvectors, spectra that differ by the
    // shift.  ONE replica is decomposed (set 0's, with its jitter); set 1 reads its eigenvectors and a shifted copy of its spectrum.
    const bool share_s = c->pair_share_s && same_ks;
    const int nS = share_s ? 1 : 2;
    out.share_s = share_s;
    if (share_s) ++c->pair_shared_s_calls;
    // The temporal chain's long first kernels go first; staged, the host queues the spatial chain (~0.1 ms of launches) before
    // it comes back for the temporal chain's second stage -- stage 1 runs half a millisecond, the queue is never empty
    tchain_begin(c, tc, build_kts);
    c->tl("S chain start (s3)", s3);
    const bool sfill = spatial_fill_applies(c, sym_s, nx);
    if (sfill) {
        // the fill folds Ks and adds each replica's jitter to the folded diagonals: one assembly, no copy, no diagonal pass
        if (same_ks) build_kphi(c, g, hp[0]->R, hp[0]->eps, hp[0]->ell_s, nullptr, 0, 0.0, Ks, s3, "ks_");
        else for (int b = 0; b < 2; ++b) build_kphi(c, g, hp[b]->R, hp[b]->eps, hp[b]->ell_s, nullptr, 0, 0.0, Ks + b * nxx, s3, "ks_");
        spatial_fill(c, Ks, nx, same_ks ? 0 : nxx, nS, jitter, *sym_s, status, 2, s3);
    } else if (share_s) {
        build_kphi(c, g, hp[0]->R, hp[0]->eps, hp[0]->ell_s, nullptr, 0, jitter[0], Ks, s3, "ks_");
    } else if (same_ks) {
        const int lo = jitter[0] == 0.0 ? 0 : 1, hi = 1 - lo;           // assemble the one without a shift (if any) first
        build_kphi(c, g, hp[lo]->R, hp[lo]->eps, hp[lo]->ell_s, nullptr, 0, 0.0, Ks + lo * nxx, s3, "ks_");
        GP_HIP(hipMemcpyAsync(Ks + hi * nxx, Ks + lo * nxx, (size_t)nxx * sizeof(double), hipMemcpyDeviceToDevice, s3));
        if (jitter[lo] != 0.0) k_add_diag(c, Ks + lo * nxx, nx, jitter[lo], s3);
        if (jitter[hi] != 0.0) k_add_diag(c, Ks + hi * nxx, nx, jitter[hi], s3);
    } else {
        for (int b = 0; b < 2; ++b) build_kphi(c, g, hp[b]->R, hp[b]->eps, hp[b]->ell_s, nullptr, 0, jitter[b], Ks + b * nxx, s3, "ks_");
    }
    // two replicas of the spatial problem on stream3 (status words [0], [2]) -- or the one both sets share
    {
        ProfScope ps(c, "eigh_spatial", 9.0 * (double)nx * nx * nx * nS, s3);
        EighCall r;
        r.side[0] = {Ks, nx, es, Qs, sym_s, nS, /*prefolded=*/sfill};
        r.status = status; r.status_stride = 2;
        r.need_merged = !fold_s;
        eigh_pair_device(c, r, s3);
    }
    if (share_s) {                   // set 1's spectrum: set 0's shifted by the difference of the jitters, in replica 1's slots
        const double dj = jitter[1] - jitter[0];
        if (vs.on) k_shift_copy(c, vs.w, vs.w + vs.sw, nx, dj, s3);
        if (!vs.on || !fold_s) k_shift_copy(c, es, es + nx, nx, dj, s3);
    }
    GP_HIP(hipEventRecord(c->ev_sjoin, s3));
    c->tl("S chain end (s3)", s3);
    tchain_finish(c, tc);
    c->decomp_gen[0] = c->decomp_gen[1] = -1;          // replicas are not what the separate calls' cache looks for
    const double *d_sig[2] = {c->upload_cached<double>("sig2n", hp[0]->sig2n, 1), c->upload_cached<double>("sig2n_pair", hp[1]->sig2n, 1)};
    for (int b = 0; b < 2; ++b) {
        const int bt = nT == 2 ? b : 0;
        EigState &e = out.e[b];
        const int bs = share_s ? 0 : b;      // the replica whose EIGENVECTORS set b reads (the spectra: always slot b)
        e.Qs = Qs + bs * nxx; e.es = es + (long)b * nx; e.Qt = Qt + bt * ntt; e.et = et + (long)bt * nt;
        e.D = c->buf<double>("D", (size_t)nx * nt);
        e.Dinv = c->buf<double>("Dinv", (size_t)nx * nt);
        e.scal = scal;
        e.status = status;
        e.pending = true;
        e.wait_temporal = e.wait_spatial = true;
        e.d_sig = d_sig[b];
        e.nsig = 1;
        // set 0 is the log-likelihood's: replica 0 of the temporal classes, and X with replica 0's Q
        if (tc.staged && (b == 0 || pred_tri)) tchain_consumer(c, tc, e, bt, /*forms_x=*/b == 0);
        FoldMode &fm = out.fm[b];
        fm = fold_mode(c, hp[b], fold_s);               // replica 0 of the generations just started ...
        if (fm.fs.on) { fm.fs.w += (long)b * vs.sw; fm.fs.U += (long)bs * vs.sU; }      // ... moved to replica b
        else { fm.fs.w += (long)b * nx; fm.fs.U += bs * nxx; }
        if (fm.ft.on) { fm.ft.w += (long)bt * vt.sw; fm.ft.U += (long)bt * vt.sU; }
        else { fm.ft.w += (long)bt * nt; fm.ft.U += bt * ntt; }
    }
}

// Collect the status words of an asynchronous predict (see gpcsd_ctx::async_pending): drains the streams.
static int drain_async(gpcsd_ctx *c) {
    if (!c->async_pending) return 0;
    c->async_pending = false;
    int *st = reinterpret_cast<int *>(c->buf<double>("scal_status", gpcsd_ctx::RESULT_DOUBLES) + gpcsd_ctx::SCAL_N);
    GP_HIP(hipStreamSynchronize(c->stream2));
    GP_HIP(hipStreamSynchronize(c->stream3));
    int rc = finish_status(c, st, gpcsd_ctx::STATUS_N);        // downloads + synchronises; the words are cleared by the next call's front half
    if (c->last_pred.have) replay_if_missed(c, rc, c->last_pred.piped, nullptr, nullptr, &c->last_pred.call);     // the queued prediction
    return rc;
}

extern "C" int gpcsd_predict_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar,
                                      int ntstar, int type, int want_lists) {
    GP_API_BEGIN(c)
    const bool piped = c->q_pipe;
    const PredCall q = pred_call(hp, z, nz, tstar, ntstar, type, want_lists != 0, /*async=*/true);
    const int rc = predict_impl(c, q);
    if (rc == 0) keep_prediction(c, piped, q);
    return rc;
    GP_API_END(c)
}

// What a paired call decides before it queues anything: the prediction's plan, which both sets take -- or FULL where the paired front
// half does not apply (it serves the folded-basis tails only): the call is then the two calls one after the other.
static PredPlan pair_plan(gpcsd_ctx *c, const gpcsd_hparams *hp_ll, const gpcsd_hparams *hp_pr, const double *z, int nz, const double *tstar,
                          int ntstar) {
    const bool may = two_stream_front() && c->prof_mode != 1 && !uses_host_kt(hp_ll) && !uses_host_kt(hp_pr) && hp_ll->n_sig2n == 1 &&
                     hp_pr->n_sig2n == 1 && fold_mode(c, hp_ll).on;
    return may ? pred_plan(c, hp_pr, z, nz, tstar, ntstar) : PredPlan();
}

// Everything the paired front half's launches depend on (a prefetched front half is only taken by a call with the same key)
static std::vector<unsigned char> pair_key(const gpcsd_ctx *c, const gpcsd_hparams *const hp[2], const double jit[2], const PredPlan &P) {
    std::vector<double> k;
    for (int b = 0; b < 2; ++b) {
        const gpcsd_hparams *h = hp[b];
        k.push_back(h->R); k.push_back(h->eps); k.push_back(h->ell_s[0]); k.push_back(h->ell_s[1]); k.push_back(jit[b]);
        k.push_back((double)h->n_temporal); k.push_back((double)h->n_sig2n); k.push_back(h->sig2n[0]);
        for (int i = 0; i < h->n_temporal; ++i) { k.push_back((double)h->kind[i]); k.push_back(h->ell_t[i]); k.push_back(h->sigma2_t[i]); }
    }
    const double cfg[] = {(double)P.tri, (double)P.fold_s(), (double)c->grid_epoch, (double)c->alloc_epoch, (double)c->ntrials, (double)c->nx,
                          (double)c->nt, (double)c->q_pipe, (double)c->pair_share_s, (double)c->tail_early_exit,
                          (double)c->ll_tridiag_mode, (double)c->gram_fp32, (double)c->decomp_cache_on, (double)c->fold_gemm_on};
    k.insert(k.end(), cfg, cfg + sizeof(cfg) / sizeof(cfg[0]));
    const unsigned char *p = reinterpret_cast<const unsigned char *>(k.data());
    return std::vector<unsigned char>(p, p + k.size() * sizeof(double));
}

struct PairPrefetch {
    std::vector<unsigned char> key;
    PairFront pf;
};
static void pair_prefetch_drop(gpcsd_ctx *c) {
    delete static_cast<PairPrefetch *>(c->pair_prefetch);
    c->pair_prefetch = nullptr;
}

// gpcsd_prefetch_pair: the caller knows the hyper-parameters of its NEXT paired call (a grid or a chain of proposals fixed in
// advance, the replicas of a lock-step batch, a benchmark loop): the two decomposition chains of that call are queued NOW, on their own
// streams, and start as soon as those streams are free -- typically while the current call's log-likelihood is still being
// formed, instead of after the host has collected it.  The next gpcsd_loglik_predict_async with the same arguments takes them
// over; any other call on the context drops them (they have then run for nothing).  Returns 1 when queued, 0 when the paired
// form does not apply to these arguments.
extern "C" int gpcsd_prefetch_pair(gpcsd_ctx *c, const gpcsd_hparams *hp_ll, const gpcsd_hparams *hp_pr, const double *z, int nz,
                                   const double *tstar, int ntstar) {
    GP_API_BEGIN(c)
    GP_REQUIRE(hp_ll && hp_pr && z && tstar && nz > 0 && ntstar > 0, -3, "prefetch_pair: bad arguments");
    GP_REQUIRE(c->d_lfp != nullptr && c->nt > 0 && ntstar == c->nt, -4, "prefetch_pair: resident data / time grid do not match");
    pair_prefetch_drop(c);
    const PredPlan P = pair_plan(c, hp_ll, hp_pr, z, nz, tstar, ntstar);
    if (P.form == PredPlan::FULL || c->time_nt != c->nt || resident_geo(c).nx != c->nx) return 0;
    check_hp(c, hp_ll, c->nx);
    check_hp(c, hp_pr, c->nx);
    const gpcsd_hparams *hps[2] = {hp_ll, hp_pr};
    const double jit[2] = {hp_ll->jitter, 0.0};
    PairPrefetch *pp = new PairPrefetch();
    try {
        // (not pipelined: the chain has a whole step's head start, T and Q follow it at once -- the same kernels, the same bits)
        front_half_pair(c, hps, jit, pp->pf, P.tri, /*x_via_tri_pre=*/false, P.fold_s());
    } catch (...) {
        delete pp;
        throw;
    }
    pp->key = pair_key(c, hps, jit, P);
    c->pair_prefetch = pp;                 // (begin_generation dropped whatever was there; set after the front half for the same reason)
    ++c->pair_prefetch_queued;
    return 1;
    GP_API_END(c)
}

extern "C" int gpcsd_prefetch_stats(gpcsd_ctx *c, long *queued, long *taken) {
    GP_API_BEGIN(c)
    if (queued) *queued = c->pair_prefetch_queued;
    if (taken) *taken = c->pair_prefetch_taken;
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_loglik_predict_async(gpcsd_ctx *c, const gpcsd_hparams *hp_ll, const gpcsd_hparams *hp_pr, const double *z, int nz,
                                          const double *tstar, int ntstar, int type, int want_lists) {
    if (c && c->ll_count >= gpcsd_ctx::LL_SLOTS)
        return fail(c, HipError{-3, "loglik_predict_async: too many asynchronous evaluations outstanding (collect with "
                                    "gpcsd_loglik_parts_wait)"});
    GP_API_BEGIN(c)
    GP_REQUIRE(hp_ll && hp_pr, -3, "loglik_predict_async: null hparams");
    PredCall q = pred_call(hp_pr, z, nz, tstar, ntstar, type, want_lists != 0, /*async=*/true);
    check_predict_args(c, q);
    check_hp(c, hp_ll, c->nx);            // both sets, before anything of them is copied into the slot or into last_pred
    check_hp(c, hp_pr, c->nx);
    PredPlan P = pair_plan(c, hp_ll, hp_pr, z, nz, tstar, ntstar);
    const bool pair = P.form != PredPlan::FULL;
    if (pair) {
        GP_REQUIRE(c->time_nt == c->nt, -4, "time grid has %d points but lfp has nt=%d", c->time_nt, c->nt);
        GP_REQUIRE(resident_geo(c).nx == c->nx, -4, "geometry has %d electrodes but lfp has nx=%d", resident_geo(c).nx, c->nx);
    }
    {   // what gpcsd_loglik_parts_wait needs to evaluate the pair again (replay_if_missed)
        gpcsd_ctx::LlSlot &sl = c->ll_slot[(c->ll_head + c->ll_count) % gpcsd_ctx::LL_SLOTS];
        sl.piped = c->q_pipe;
        sl.hp.set(hp_ll);
        keep_prediction(c, sl.piped, q);
        sl.pred_seq = c->pred_seq;
    }
    if (!pair) {
        const int rc = loglik_parts_impl(c, hp_ll, nullptr, true);
        if (rc != 0) return rc;
        return predict_impl(c, q);
    }
    const gpcsd_hparams *hps[2] = {hp_ll, hp_pr};
    const double jit[2] = {hp_ll->jitter, 0.0};          // no jitter in predict (gpcsd1d.py:258)
    PairFront pf;
    // the front half: prefetched by the previous call's gpcsd_prefetch_pair (same arguments, nothing in between), or queued now
    bool taken = false;
    if (PairPrefetch *pp = static_cast<PairPrefetch *>(c->pair_prefetch)) {
        if (pp->key == pair_key(c, hps, jit, P)) {
            pf = pp->pf;
            // (device copies of the noise variances: the prefetch's uploads are the same values, the pointers the same buffers)
            taken = true;
            ++c->pair_prefetch_taken;
        }
        pair_prefetch_drop(c);
    }
    if (!taken) front_half_pair(c, hps, jit, pf, P.tri, /*x_via_tri_pre=*/P.fm.ft.on, P.fold_s());
    const bool uploaded = pred_operands(c, q, P, pf.fm[1]);
    // what needs no decomposition goes to stream5 exactly when stage 5 is pending (the main stream has the log-likelihood's products
    // to queue first) and nothing was uploaded just now on the main stream (the builders that read sites or times then stay there)
    q.prelude_side = !uploaded && pf.e[0].pipe_pending;
    PairLl ll{&pf.e[0], &pf.fm[0], false, false};
    // equal temporal hyper-parameters (every loglik -> predict pair of a fit or a bench step: the jitter is spatial): the prediction
    // reads the log-likelihood's X = Y~ Q instead of forming its own from the bit-identical second replica
    // (gpcsd_pair_share_x(ctx, 0, ..) / GPCSD_PAIR_SHARE_X=0: A/B)
    ll.share_x = c->pair_share_x && pf.e[0].tri && pf.e[1].tri && same_temporal(hp_ll, hp_pr);
    if (ll.share_x) ++c->pair_shared_x_calls;
    // one spatial decomposition (PairFront::share_s): the two projected data sets W~ = diag(U)^T (Y~ Q or Y~) are then the same
    // product whenever both sets take the same form -- tridiagonal with X shared, or both with the temporal eigenvectors
    ll.share_w = pf.share_s && (ll.share_x || (!pf.e[0].tri && !pf.e[1].tri));
    q.ll = &ll;
    // a pair that queued its own front half is (in a loop) followed by one that does the same while this one's solve runs: the
    // narrow form of the solve leaves room beside it (gram.hip: k_tridiag_solve)
    q.solve_pass = taken ? 64 : 32;
    return predict_fold(c, q, P, pf.e[1]);
    GP_API_END(c)
}

extern "C" int gpcsd_fetch(gpcsd_ctx *c, const char *name, double *host, long count) {
    GP_API_BEGIN(c)
    GP_REQUIRE(name && host && count > 0, -3, "fetch: bad arguments");
    auto it = c->bufs.find(name);
    GP_REQUIRE(it != c->bufs.end() && it->second.p, -2, "fetch: no device buffer named '%s'", name);
    GP_REQUIRE((size_t)count * sizeof(double) <= it->second.bytes, -3, "fetch: '%s' holds %zu bytes, asked for %ld doubles", name,
               it->second.bytes, count);
    // a numerical failure of a preceding asynchronous predict surfaces here -- collected BEFORE the copy: a prediction whose
    // pipelined stage missed its tail is evaluated again by drain_async (q_pipe_missed), and the caller gets that result
    const int rc = drain_async(c);
    c->download(host, it->second.p, (size_t)count * sizeof(double));
    c->sync();
    return rc;
    GP_API_END(c)
}

// The device address of a named result buffer (what gpcsd_fetch copies from), for callers that keep working on the GPU: a
// prediction left in HBM by gpcsd_predict_resident gathered over ranks with RCCL, handed to another library through
// __cuda_array_interface__ / DLPack.  Collects a queued prediction's deferred status first (as gpcsd_fetch does) and drains the
// context's streams: the buffer is complete when the call returns, and stays valid until the next call that writes it.
extern "C" int gpcsd_device_buffer(gpcsd_ctx *c, const char *name, unsigned long long *dev_ptr, unsigned long long *bytes) {
    GP_API_BEGIN(c)
    GP_REQUIRE(name && dev_ptr && bytes, -3, "device_buffer: bad arguments");
    auto it = c->bufs.find(name);
    GP_REQUIRE(it != c->bufs.end() && it->second.p, -2, "device_buffer: no device buffer named '%s'", name);
    const int rc = drain_async(c);
    c->sync();
    *dev_ptr = (unsigned long long)(uintptr_t)it->second.p;
    *bytes = (unsigned long long)it->second.bytes;
    return rc;
    GP_API_END(c)
}

extern "C" int gpcsd_predict(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar,
                             int type, double *csd_list, double *csd, double *lfp_list, double *lfp) {
    GP_API_BEGIN(c)
    // the caller's arrays are known to the tail: a folded prediction copies its outputs out chunk by chunk under its last product
    // (... into page-locked arrays only -- the class API's come from its pinned pool.  Pageable arrays of another caller are
    // filled through the context's bounce blocks after the product: the runtime never gets to register the caller's pages,
    // ctx.hpp copy_in / copy_out)
    PredSink sk;
    sk.owner = c;
    sk.active = true;
    for (const double *p : {csd, csd_list, lfp, lfp_list})
        if (p && !gpcsd_ctx::host_is_pinned(p)) sk.active = false;
    sk.sum[0] = csd; sk.list[0] = csd_list; sk.sum[1] = lfp; sk.list[1] = lfp_list;
    PredCall q = pred_call(hp, z, nz, tstar, ntstar, type, csd_list != nullptr || lfp_list != nullptr, /*async=*/false);
    q.sink = &sk;
    const bool piped = c->q_pipe;
    int rc = predict_impl(c, q);
    replay_if_missed(c, rc, piped, nullptr, nullptr, &q);
    if (rc < 0) return rc;
    pred_download(c, q, sk);
    c->sync();
    return rc;
    GP_API_END(c)
}

extern "C" int gpcsd_sample_prior(gpcsd_ctx *c, const gpcsd_hparams *hp, int which, const double *normals, int ntrials,
                                  double *out) {
    GP_API_BEGIN(c)
    const Geo g = resident_geo(c);
    GP_REQUIRE(normals && out && ntrials > 0, -3, "sample_prior: bad arguments");
    GP_REQUIRE(which == GPCSD_PRED_CSD || which == GPCSD_PRED_LFP, -3, "sample_prior: which must be CSD(1) or LFP(2)");
    GP_REQUIRE(c->time_nt > 0, -4, "time grid not set");
    check_hp(c, hp, g.nx);
    const int nx = g.nx, nt = c->time_nt, R = ntrials;
    const long RT = (long)R * nt;
    hipStream_t s = c->stream;
    double *Ks = c->buf<double>("Ks", (size_t)nx * nx);
    double *Kt = c->buf<double>("Kt", (size_t)nt * nt);
    int *st = c->buf<int>("status", 4);
    GP_HIP(hipMemsetAsync(st, 0, 4 * sizeof(int), s));
    const double *t = (const double *)c->bufs["time_t"].p;
    if (which == GPCSD_PRED_CSD) {
        build_ks_csd(c, g, hp->ell_s, Ks, s);                                      // gpcsd1d.py:298
        k_add_diag(c, Ks, nx, hp->jitter, s);
    } else {
        build_kphi(c, g, hp->R, hp->eps, hp->ell_s, nullptr, 0, hp->jitter, Ks, s);   // gpcsd2d.py:346-347
    }
    if (uses_host_kt(hp)) {
        GP_REQUIRE(c->host_kt_nt == nt && (int)c->host_kt.size() == nt * nt, -3, "host temporal Gram does not match nt=%d", nt);
        c->copy_in(Kt, c->host_kt.data(), (size_t)nt * nt * sizeof(double), s);
    } else {
        build_kt(c, hp, t, nt, t, nt, Kt, s);
    }
    potrf_device(c, Kt, nt, st, s);                                                 // Lt
    potrf_device(c, Ks, nx, st, s);                                                 // Ls
    double *stage = c->upload<double>("sp_stage", normals, (size_t)nx * RT);
    double *Z = c->buf<double>("sp_Z", (size_t)nx * RT);
    double *T1 = c->buf<double>("sp_T1", (size_t)nx * RT);
    k_swap_last2(c, stage, Z, nx, nt, R, s);                                        // (x,t,r) -> (x,r,t)
    GemmDesc g1;                          // T1[x'][(r,t)] = sum_x Ls[x'][x] Z[x][(r,t)]
    g1.M = nx; g1.N = (int)RT; g1.K = nx;
    g1.A = Ks; g1.lda = nx; g1.B = Z; g1.ldb = RT; g1.C = T1; g1.ldc = RT;
    g1.prof_name = "gemm_sample_spatial";
    gemm_f64(c, g1, s);
    GemmDesc g2;                          // out[(x',r)][t'] = sum_t T1[(x',r)][t] Lt[t'][t]
    g2.M = nx * R; g2.N = nt; g2.K = nt;
    g2.A = T1; g2.lda = nt; g2.B = Kt; g2.ldb = nt; g2.transB = true; g2.C = Z; g2.ldc = nt;
    g2.prof_name = "gemm_sample_temporal";
    gemm_f64(c, g2, s);
    k_swap_last2(c, Z, stage, nx, R, nt, s);                                        // (x,r,t) -> (x,t,r)
    c->download(out, stage, (size_t)nx * RT * sizeof(double));
    return finish_status(c, st);
    GP_API_END(c)
}
