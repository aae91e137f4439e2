// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip and capi_fused.inl are in scope) --
// posterior quantities at sites z and ARBITRARY times t*: what the family shares (one request check, one front, one mean tail, one
// download helper) and the calls that consist of little else (gpcsd_predict_at, gpcsd_predict_var); the leave-one-out scores
// (gpcsd_loo), which read the same data operand.  capi_masked.inl, capi_sample.inl and capi_functionals.inl build on this part.

// ------------------------------------------------------------------------------------------------------------------
// the request check: which of the family's checks a call wants.  They run in the order of the bits, so a call with checks of its own
// in between asks in several steps (the precedence of the return codes is part of the ABI); every capacity check precedes the
// first read of z or tstar.
// ------------------------------------------------------------------------------------------------------------------
enum : unsigned {
    REQ_SITES = 1u,           // z, tstar, nz > 0, ntstar > 0 (-3); type in 1..3 (-3)
    REQ_HP = 2u,              // null hparams (-3)
    REQ_LFP = 4u,             // no resident trials (-4)
    REQ_NO_HOST_KT = 8u,      // a GPCSD_KIND_HOST component (-3): the device has its Gram on the training grid only
    REQ_CAP_OUT_ROW = 16u,    // ntrials * ntstar doubles are one output row, nz * ntrials columns one index (GPCSD_ERR_CAPACITY)
    REQ_CAP_PC_ROW = 32u,     // n_temporal * ntstar doubles are one row of the concatenated P_c (GPCSD_ERR_CAPACITY)
};
static void posterior_request(const gpcsd_ctx *c, const char *who, const PredCall &q, unsigned checks) {
    const gpcsd_hparams *hp = q.hp;
    if (checks & REQ_SITES) {
        GP_REQUIRE(q.z && q.tstar && q.nz > 0 && q.ntstar > 0, -3, "%s: bad arguments", who);
        GP_REQUIRE(q.type >= 1 && q.type <= 3, -3, "%s: type must be CSD(1), LFP(2) or BOTH(3)", who);
    }
    if (checks & REQ_HP) GP_REQUIRE(hp != nullptr, -3, "null hparams");
    if (checks & REQ_LFP) GP_REQUIRE(c->d_lfp != nullptr, -4, "lfp not set (call gpcsd_set_lfp)");
    if (checks & REQ_NO_HOST_KT)
        GP_REQUIRE(!uses_host_kt(hp), -3, "%s: a user-defined temporal covariance (GPCSD_KIND_HOST) has no Gram beyond the training grid "
                   "(k_c(t*, t*), the joint one over [t*; t]) on the device; only the built-in kinds are supported", who);
    const long pc_row = (checks & (REQ_CAP_OUT_ROW | REQ_CAP_PC_ROW)) ? (long)std::max(hp->n_temporal, 1) * q.ntstar : 0;
    if (checks & REQ_CAP_OUT_ROW)
        GP_REQUIRE((long)c->ntrials * q.ntstar < GPCSD_MAX_GEMM_LD_KMAJOR && pc_row < GPCSD_MAX_GEMM_LD_KMAJOR &&
                       (long)q.nz * c->ntrials < (1L << 31),
                   GPCSD_ERR_CAPACITY, "%s: ntrials * ntstar = %ld (or n_temporal * ntstar, or nz * ntrials) exceeds the capacity of "
                   "one output row (%ld doubles; GPCSD_MAX_GEMM_LD_KMAJOR)", who, (long)c->ntrials * q.ntstar, (long)GPCSD_MAX_GEMM_LD_KMAJOR);
    else if (checks & REQ_CAP_PC_ROW)
        GP_REQUIRE(pc_row < GPCSD_MAX_GEMM_LD_KMAJOR, GPCSD_ERR_CAPACITY,
                   "%s: n_temporal * ntstar = %ld exceeds the capacity of one operand row (%ld doubles; GPCSD_MAX_GEMM_LD_KMAJOR)", who, pc_row,
                   (long)GPCSD_MAX_GEMM_LD_KMAJOR);
}

// ------------------------------------------------------------------------------------------------------------------
// the front: everything up to the operands the family contracts
// ------------------------------------------------------------------------------------------------------------------
// The temporal operand, on the main stream behind the joined temporal side: Pcat[i'][cc * ntstar + j] = sum_i Qt[i][i'] k_cc(t*_j, t_i),
// the TRAINING axis of the cross Grams Kts (C, ntstar, nt) contracted, the components side by side in "pred_Pc" (nt, C * ntstar).
static double *pred_at_Pc(gpcsd_ctx *c, const EigState &e, const double *Kts, int C, int ntstar) {
    const int nt = c->nt;
    double *Pc = c->buf<double>("pred_Pc", (size_t)C * nt * ntstar);
    for (int cc = 0; cc < C; ++cc) {
        GemmDesc gp;
        gp.M = nt; gp.N = ntstar; gp.K = nt;
        gp.A = e.Qt; gp.lda = nt; gp.transA = true; gp.B = Kts + (size_t)cc * ntstar * nt; gp.ldb = nt; gp.transB = true;
        gp.C = Pc + (size_t)cc * ntstar; gp.ldc = (long)C * ntstar;
        gp.prof_name = "gemm_pred_Pc";
        gemm_f64(c, gp, c->stream);
    }
    return Pc;
}

// The decomposition of the model without jitter (as predict, gpcsd1d.py:258) and, of PredFullFront, M1 (2, nz, nx), Kts, the sites
// and times on the device and Bm (nx, R, nt) -- null unless the front formed it or the caller supplied it -- plus Pcat.
struct PostFront : PredFullFront {
    EigState e;
    double *Pc = nullptr;
};
enum : unsigned {
    FRONT_DRAIN = 1u,         // the prediction scratch is rewritten: what an earlier queued prediction still owes is collected first
    FRONT_TRIALS = 2u,        // Bm from the resident trials (predict_full_front); otherwise the trials are not read here
};
// own_data: a caller's own data operand (gpcsd_predict_masked), formed where the resident trials' would be complete -- behind the
// joined decomposition, in front of Pcat; its value becomes f.Bm.  Returns what drain_async found (not 0: nothing was queued).
static int posterior_front(gpcsd_ctx *c, const PredCall &q, unsigned how, PostFront &f,
                           const std::function<double *(EigState &)> &own_data = nullptr) {
    if (how & FRONT_DRAIN)
        if (int rc = drain_async(c)) return rc;
    f.e = front_half(c, q.hp, 0.0);
    if (how & FRONT_TRIALS) static_cast<PredFullFront &>(f) = predict_full_front(c, q.hp, f.e, q.z, q.nz, q.tstar, q.ntstar, q.type);
    else pred_cross_front(c, q.hp, f.e, q.z, q.nz, q.tstar, q.ntstar, q.type, f);
    if (own_data) f.Bm = own_data(f.e);
    f.Pc = pred_at_Pc(c, f.e, f.Kts, q.hp->n_temporal, q.ntstar);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// the mean tail: out_c[z][j][r] = sum_i' S[(z, r)][i'] P_c[i'][j] with S = M1[which] Bm, the last product writing the output layout
// (z, t*, r) itself (gemm_pred_at), for R columns of trials or pseudo-trials in f.Bm.  S: scratch of nz * R * nt doubles;
// list (C planes list_stride apart) may be null.
// ------------------------------------------------------------------------------------------------------------------
static void pred_mean_tail(gpcsd_ctx *c, const PostFront &f, const PredCall &q, int which, int R, double *S, double *sum, double *list,
                           long list_stride) {
    const int nt = c->nt, C = q.hp->n_temporal;
    pred_cross_S(c, f.M1, which, q.nz, f.Bm, S, (long)R * nt);
    PredAtDesc pa;                        // out[cc][z][j][r] = sum_i' Pcat[i'][cc*ntstar + j] S[(z,r)][i'], and the sum over cc
    pa.S = S; pa.lds = nt; pa.Pc = f.Pc; pa.ldp = (long)C * q.ntstar;
    pa.K = nt; pa.nts = q.ntstar; pa.C = C; pa.R = R; pa.ncol = (long)q.nz * R;
    pa.list = list; pa.list_stride = list_stride; pa.sum = sum;
    gemm_pred_at(c, pa, c->stream);
}
// ... of the resident trials into the buffers of predict_impl, (nz, ntstar, R) / (C, nz, ntstar, R)
static void pred_mean_outputs(gpcsd_ctx *c, const PostFront &f, const PredCall &q) {
    const int R = c->ntrials;
    const size_t out_elems = (size_t)q.nz * q.ntstar * R;
    double *S = c->buf<double>("pred_S", (size_t)q.nz * R * c->nt);
    for (int which = 1; which <= 2; ++which) {
        if (!(q.type & which)) continue;
        const PredOut out = pred_out_bufs(c, which, out_elems, q.hp->n_temporal, q.want_lists);
        pred_mean_tail(c, f, q, which, R, S, out.sum, out.list, (long)out_elems);
    }
}

// The resident outputs are this call's now: nothing queued earlier may be evaluated again over them (drain_async, the paired wait)
static void own_resident_outputs(gpcsd_ctx *c) {
    ++c->pred_seq;
    c->last_pred.have = false;
}

// ------------------------------------------------------------------------------------------------------------------
// host outputs: the named result buffers into the caller's arrays (a null array is skipped), one wait for all of them
// ------------------------------------------------------------------------------------------------------------------
struct HostOut {
    double *host;
    std::string name;
    size_t count;
};
static void download_outputs(gpcsd_ctx *c, const std::vector<HostOut> &outs) {
    for (const HostOut &o : outs)
        if (o.host) c->download(o.host, c->bufs[o.name].p, o.count * sizeof(double));
    c->sync();
}
// ... of the shape "csd / lfp x sum / list": PREFIXcsd, PREFIXcsd_list (C planes), PREFIXlfp, PREFIXlfp_list, the requested quantities only
static void download_sum_list(gpcsd_ctx *c, const std::string &prefix, int type, size_t out_elems, int C, double *csd_list, double *csd,
                              double *lfp_list, double *lfp) {
    double *const sum[2] = {csd, lfp}, *const list[2] = {csd_list, lfp_list};
    std::vector<HostOut> outs;
    for (int w = 0; w < 2; ++w) {
        if (!(type & (w + 1))) continue;
        const std::string name = prefix + (w ? "lfp" : "csd");
        outs.push_back({sum[w], name, out_elems});
        outs.push_back({list[w], name + "_list", out_elems * C});
    }
    download_outputs(c, outs);
}

// ------------------------------------------------------------------------------------------------------------------
// Posterior mean at ARBITRARY prediction times (gpcsd_predict_at; no reference counterpart): as the full-size path of predict_impl
// up to S = (Kc^T Qs) Bm, then the TRAINING axis of the cross Grams is contracted,
//   P_c[i'][j] = sum_i Qt[i][i'] k_c(t*_j, t_i),      out_c[z][j][r] = sum_i' S[(z, r)][i'] P_c[i'][j].
// Both sides unfolded: a window of t has no mirror symmetry.  Outputs: the buffers of predict_impl, (nz, ntstar, R) / (C, nz, ntstar, R).
// (No FRONT_DRAIN, alone in the family.  Everything here is queued on the main stream behind an earlier queued prediction's tail, so
// the shared scratch is safe either way; what differs is whose status it is: front_half leaves the sticky status words alone while
// async_pending is set, and this call's finish_call reports and clears them -- an earlier prediction's failure, a missed pipelined
// stage (status 7) included, comes back as this call's code instead of being collected, and replayed, first.)
// ------------------------------------------------------------------------------------------------------------------
static int predict_at_impl(gpcsd_ctx *c, const PredCall &q) {
    posterior_request(c, "predict_at", q, REQ_SITES | REQ_HP | REQ_LFP | REQ_CAP_OUT_ROW | REQ_CAP_PC_ROW);
    PostFront f;
    posterior_front(c, q, FRONT_TRIALS, f);
    pred_mean_outputs(c, f, q);
    own_resident_outputs(c);
    return finish_call(c, f.e, nullptr, 0);
}

extern "C" int gpcsd_predict_at_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar,
                                         int ntstar, int type, int want_lists) {
    GP_API_BEGIN(c)
    return predict_at_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, want_lists != 0, false));
    GP_API_END(c)
}

extern "C" int gpcsd_predict_at(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar,
                                int type, double *csd_list, double *csd, double *lfp_list, double *lfp) {
    GP_API_BEGIN(c)
    const PredCall q = pred_call(hp, z, nz, tstar, ntstar, type, csd_list != nullptr || lfp_list != nullptr, false);
    const int rc = predict_at_impl(c, q);
    if (rc < 0) return rc;
    download_sum_list(c, "pred_out_", type, (size_t)nz * ntstar * c->ntrials, hp->n_temporal, csd_list, csd, lfp_list, lfp);
    return rc;
    GP_API_END(c)
}

// ------------------------------------------------------------------------------------------------------------------
// Posterior VARIANCE at the sites and times of gpcsd_predict_at (gpcsd_predict_var; no reference counterpart), of the model whose
// mean that call returns: D = es (x) et + sig2n exactly as front_half(c, hp, 0.0) builds it.  With M1 = Kcross^T Qs and
// P_c[i'][j] = sum_i Qt[i][i'] k_c(t*_j, t_i) the explained part of component c at (z, t*_j) is
//   sum_{x',i'} M1[z][x']^2 P_c[i'][j]^2 / D[x'][i']  =  sum_i' G[z][i'] P_c[i'][j]^2,     G[z][i'] = sum_x' M1[z][x']^2 / D[x'][i'],
// G formed first and once (it depends on neither t* nor the component), every sum over non-negative terms; the component SUM has
// (sum_c P_c)^2 in place of P_c^2 -- the components are correlated a posteriori, so it is a plane of its own.  Reads no trial data.
// Outputs: pred_var_csd / pred_var_lfp (nz, ntstar), pred_var_csd_list / pred_var_lfp_list (C, nz, ntstar) -- or under another
// prefix, for a call that needs the variance and must leave the caller's alone (gpcsd_sample_features).
// ------------------------------------------------------------------------------------------------------------------
static int predict_var_impl(gpcsd_ctx *c, const PredCall &q, const std::string &prefix = "pred_var_") {
    posterior_request(c, "predict_var", q, REQ_SITES | REQ_HP | REQ_LFP | REQ_NO_HOST_KT | REQ_CAP_PC_ROW);
    PostFront f;
    if (int rc = posterior_front(c, q, FRONT_DRAIN, f)) return rc;
    const gpcsd_hparams *hp = q.hp;
    const Geo g = resident_geo(c);
    const int nx = c->nx, nt = c->nt, C = hp->n_temporal, nz = q.nz, ntstar = q.ntstar;
    hipStream_t s = c->stream;
    double *G = c->buf<double>("pred_var_G", (size_t)nz * nt);
    double *prior = c->buf<double>("pred_var_prior", (size_t)nz);
    const size_t out_elems = (size_t)nz * ntstar;
    for (int which = 1; which <= 2; ++which) {
        if (!(q.type & which)) continue;
        // prior variance of the spatial factor at the sites: compute_Ks has a unit diagonal (covariances.py:50-56, 177-186); the
        // potential's is the diagonal of compKphi at the sites themselves (covariances.py:74-96, 204-232)
        if (which == 1) k_fill(c, prior, nz, 1.0, s);
        else build_kphi_diag(c, g, hp->R, hp->eps, hp->ell_s, f.dz, nz, prior, s);
        VarDesc v1;                       // G[z][i'] = sum_x' M1[z][x']^2 Dinv[x'][i']
        v1.A = f.M1 + (size_t)(which - 1) * nz * nx; v1.lda = nx; v1.B = f.e.Dinv; v1.ldb = nt;
        v1.nrow = nz; v1.ncol = nt; v1.K = nx; v1.sq_a = true; v1.list = G;
        v1.prof_name = "gemm_var_G";
        gemm_var(c, v1, s);
        VarDesc v2;                       // var_c[z][j] = prior[z] k_c(0) - sum_i' G[z][i'] P_c[i'][j]^2, and the component sum's plane
        v2.A = G; v2.lda = nt; v2.B = f.Pc; v2.ldb = (long)C * ntstar;
        v2.nrow = nz; v2.ncol = ntstar; v2.K = nt; v2.C = C;
        v2.prior = prior;
        // k_c(t*, t*) = sigma2_c for both built-in kinds (covariances.py:270, 304), rounded as the Gram builders round it
        for (int cc = 0; cc < C; ++cc) v2.kd[cc] = c->gram_fp32 ? (double)(float)hp->sigma2_t[cc] : hp->sigma2_t[cc];
        const std::string name = prefix + (which == 1 ? "csd" : "lfp");
        v2.list = c->buf<double>(name + "_list", out_elems * C);
        v2.sum = c->buf<double>(name, out_elems);
        gemm_var(c, v2, s);
    }
    return finish_call(c, f.e, nullptr, 0);
}

extern "C" int gpcsd_predict_var_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar,
                                          int ntstar, int type) {
    GP_API_BEGIN(c)
    return predict_var_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, true, false));
    GP_API_END(c)
}

extern "C" int gpcsd_predict_var(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar,
                                 int type, double *csd_var_list, double *csd_var, double *lfp_var_list, double *lfp_var) {
    GP_API_BEGIN(c)
    const int rc = predict_var_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, true, false));
    if (rc < 0) return rc;
    download_sum_list(c, "pred_var_", type, (size_t)nz * ntstar, hp->n_temporal, csd_var_list, csd_var, lfp_var_list, lfp_var);
    return rc;
    GP_API_END(c)
}

// ------------------------------------------------------------------------------------------------------------------
// Leave-one-out predictive mean, variance and log score of every training sample (gpcsd_loo; no reference counterpart), of the
// model whose log-likelihood gpcsd_loglik returns: K = (Qs (x) Qt) diag(D) (Qs (x) Qt)^T exactly as front_half(c, hp, hp->jitter)
// builds it (the jitter on Ks, a noise list on the eigen-index).  With c = diag(K^-1) and beta_r = K^-1 y_r (Rasmussen & Williams
// 5.4.2) the score of sample (x, t) of trial r needs no refit:
//   c[x][t] = sum_{x',i'} Qs[x][x']^2 Qt[t][i']^2 / D[x'][i']          two squared-operand products, every term >= 0
//   beta_r  = Qs ((Qs^T Y_r Qt) / D) Qt^T                               the prediction front's Bm, V = Qs Bm, then gemm_loo
// in the merged (unfolded, eigenvector) basis, which is correct for every model the library accepts.  Outputs: loo_var (nx, nt),
// loo_lpd / loo_sse (nx, R), loo_mean (nx, nt, R) when asked.  (A front of its own, shared with gpcsd_cv_electrodes: the jitter of loglik, no sites, no times.)
// ------------------------------------------------------------------------------------------------------------------
// The request check and the front that gpcsd_loo and gpcsd_cv_electrodes (capi_cv.inl) share: the decomposition with loglik's jitter
// and V = Qs ((Qs^T Y_r Qt) / D) = K^-1 y_r in the temporal eigen-basis, (nx, R, nt) in "loo_V".  The launches behind the joined
// decomposition are all on the main stream, so their order among themselves is free (loo's bits do not depend on it).
static void loo_request(const gpcsd_ctx *c, const gpcsd_hparams *hp, const char *who) {
    GP_REQUIRE(hp != nullptr, -3, "null hparams");
    GP_REQUIRE(c->d_lfp != nullptr, -4, "lfp not set (call gpcsd_set_lfp)");
    const long RT = (long)c->ntrials * c->nt, nrow = (long)c->nx * c->ntrials;
    // (checked before anything is read: one row of the projected data is a flat GEMM operand row)
    GP_REQUIRE(RT < GPCSD_MAX_GEMM_LD_KMAJOR && nrow < (1L << 31), GPCSD_ERR_CAPACITY,
               "%s: ntrials * nt = %ld (or nx * ntrials = %ld) exceeds the capacity of one operand row (%ld doubles; "
               "GPCSD_MAX_GEMM_LD_KMAJOR)", who, RT, nrow, (long)GPCSD_MAX_GEMM_LD_KMAJOR);
}
struct LooFront {
    EigState e;
    double *V = nullptr;
};
static int loo_front(gpcsd_ctx *c, const gpcsd_hparams *hp, LooFront &f) {
    const int nx = c->nx, nt = c->nt, R = c->ntrials;
    const long RT = (long)R * nt;
    // the scratch of the prediction calls is rewritten below: whatever an earlier queued prediction still owes is collected first
    if (int rc = drain_async(c)) return rc;
    f.e = front_half(c, hp, hp->jitter);           // the jitter of loglik (gpcsd1d.py:117)
    double *W = c->buf<double>("proj_W", (size_t)nx * RT);
    double *Bm = c->buf<double>("pred_B", (size_t)nx * RT);
    f.V = c->buf<double>("loo_V", (size_t)nx * RT);
    pred_data_spatial(c, f.e, W, c->d_lfp, R);
    join_temporal(c, f.e, nullptr, false);         // nobody reads sum(log D) here
    pred_data_temporal(c, f.e, W, Bm, R);
    GemmDesc g3;                          // V[x][(r,i')] = sum_x' Qs[x][x'] Bm[x'][(r,i')]
    g3.M = nx; g3.N = (int)RT; g3.K = nx;
    g3.A = f.e.Qs; g3.lda = nx; g3.B = Bm; g3.ldb = RT; g3.C = f.V; g3.ldc = RT;
    g3.prof_name = "gemm_loo_V";
    gemm_f64(c, g3, c->stream);
    return 0;
}

static int loo_impl(gpcsd_ctx *c, const gpcsd_hparams *hp, bool want_mean) {
    loo_request(c, hp, "loo");
    const int nx = c->nx, nt = c->nt, R = c->ntrials;
    const long RT = (long)R * nt, nrow = (long)nx * R;
    LooFront f;
    if (int rc = loo_front(c, hp, f)) return rc;
    EigState &e = f.e;
    hipStream_t s = c->stream;
    double *H = c->buf<double>("loo_H", (size_t)nx * nt);
    double *QtT = c->buf<double>("loo_QtT", (size_t)nt * nt);
    double *cdiag = c->buf<double>("loo_c", (size_t)nx * nt);
    double *var = c->buf<double>("loo_var", (size_t)nx * nt);
    double *lpd = c->buf<double>("loo_lpd", (size_t)nrow), *sse = c->buf<double>("loo_sse", (size_t)nrow);
    double *mean = want_mean ? c->buf<double>("loo_mean", (size_t)nx * RT) : nullptr;
    VarDesc v1;                           // H[x][i'] = sum_x' Qs[x][x']^2 Dinv[x'][i']
    v1.A = e.Qs; v1.lda = nx; v1.B = e.Dinv; v1.ldb = nt;
    v1.nrow = nx; v1.ncol = nt; v1.K = nx; v1.sq_a = true; v1.list = H;
    v1.prof_name = "gemm_var_H";
    gemm_var(c, v1, s);
    k_swap_last2(c, e.Qt, QtT, 1, nt, nt, s);      // the eigen-index leading: the squared operand's layout
    VarDesc v2;                           // c[x][t] = sum_i' H[x][i'] Qt[t][i']^2
    v2.A = H; v2.lda = nt; v2.B = QtT; v2.ldb = nt;
    v2.nrow = nx; v2.ncol = nt; v2.K = nt; v2.list = cdiag;
    v2.prof_name = "gemm_var_c";
    gemm_var(c, v2, s);
    k_loo_var(c, cdiag, var, (long)nx * nt, s);
    LooDesc l;                            // beta[(x,r)][t] = sum_i' V[(x,r)][i'] Qt[t][i'], and everything behind it
    l.V = f.V; l.ldv = nt; l.Qt = e.Qt; l.ldq = nt; l.c = cdiag; l.y = c->d_lfp;
    l.K = nt; l.nt = nt; l.R = R; l.nrow = nrow;
    l.mean = mean; l.lpd = lpd; l.sse = sse;
    gemm_loo(c, l, s);
    return finish_call(c, e, nullptr, 0);
}

extern "C" int gpcsd_loo_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, int want_mean) {
    GP_API_BEGIN(c)
    return loo_impl(c, hp, want_mean != 0);
    GP_API_END(c)
}

extern "C" int gpcsd_loo(gpcsd_ctx *c, const gpcsd_hparams *hp, double *var, double *mean, double *lpd, double *sse) {
    GP_API_BEGIN(c)
    const int rc = loo_impl(c, hp, mean != nullptr);
    if (rc < 0) return rc;
    const size_t nxt = (size_t)c->nx * c->nt, nrow = (size_t)c->nx * c->ntrials;
    download_outputs(c, {{var, "loo_var", nxt}, {mean, "loo_mean", nxt * c->ntrials}, {lpd, "loo_lpd", nrow}, {sse, "loo_sse", nrow}});
    return rc;
    GP_API_END(c)
}
