// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip, capi_fused.inl and capi_posterior.inl are in scope) --
// the device generator's entry point and joint posterior draws of CSD and LFP (gpcsd_sample_posterior).

extern "C" int gpcsd_normals(gpcsd_ctx *c, unsigned long long seed, unsigned stream, unsigned long long first, long count, double *out) {
    GP_API_BEGIN(c)
    GP_REQUIRE(out && count > 0, -3, "normals: bad arguments");
    double *d = c->buf<double>("rng_out", (size_t)count);
    k_normals(c, seed, stream, first, count, d, c->stream);
    c->download(out, d, (size_t)count * sizeof(double));
    c->sync();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_set_trial_offset(gpcsd_ctx *c, long first) {
    GP_API_BEGIN(c)
    GP_REQUIRE(first >= 0, -3, "set_trial_offset: first=%ld must not be negative", first);
    c->trial_offset = first;
    return 0;
    GP_API_END(c)
}

// Scratch of one chunk of pseudo-trials, in bytes: GPCSD_SAMPLE_SCRATCH_MB (read per call: tests force several chunks with it),
// 2048 MB otherwise -- about 80 pseudo-trials of 384 x 500 with z = x, t* = t (25 MB each): one draw per trial of a 50-trial block
// is one chunk, and its flat GEMMs are as large as a prediction's.
static size_t sample_scratch_budget() {
    const char *e = getenv("GPCSD_SAMPLE_SCRATCH_MB");
    const long mb = e ? atol(e) : 0;
    return (size_t)(mb > 0 ? mb : 2048) << 20;
}

// Joint posterior draws by Matheron's rule (pathwise conditioning; no reference counterpart, which has sample_prior only):
//   sample = f_prior + P (y_r - phi - eps),
// (f_prior, phi) a joint PRIOR draw of the requested quantity at (z, t*) and of the potential at the electrodes and training times,
// eps a draw of the noise exactly as K contains it, P the linear map of gpcsd_predict_at.  Model and decomposition are those of
// predict_at / predict_var: front_half(c, hp, 0.0), no jitter anywhere.
//   joint prior   G = Fs Xi Ft^T with Fs Fs^T = Js, the spatial covariance of the stacked rows [CSD(z) | LFP(z) | LFP(x)] (the first
//                 two as requested; order ns), and Ft Ft^T = Jt = sum_c k_c on the stacked times [t*; t] (order ntt).  Both factors
//                 are Q diag(sqrt(max(w, 0))) from the symmetric eigensolver: Jt is exactly singular when t* holds training times,
//                 Js when z holds electrodes.  Js is assembled block by block from one triangle and equilibrated to a unit diagonal
//                 before it is decomposed (its LFP blocks are ~5e5 times the CSD block), the factor's rows scaled back.
//   noise         eps = Qs diag(sqrt(sig2n)) E: white for a scalar sig2n, the eigen-index list otherwise.
// Only two blocks of G are formed: (requested rows) x t* and LFP(x) x t.  The draws are processed in chunks of pseudo-trials
// p = r nsamples + s whose scratch fits sample_scratch_budget(); the decompositions, factors and the operands of P are formed once.
// The normals of pseudo-trial p are entries [p ns ntt, (p + 1) ns ntt) of stream 0 (Xi) and [p nx nt, (p + 1) nx nt) of stream 1 (E)
// with p counted from the GLOBAL trial index (gpcsd_ctx::trial_offset): no chunk size, grid or rank changes a normal.
// Outputs: post_sample_csd / post_sample_lfp (nz, ntstar, R, nsamples).
// sink (gpcsd_sample_features): a consumer of every chunk's draws where the combine pass left them.  Its scratch counts in the chunk
// length whether or not the draws are kept, so that both settings form the same draws; without a sink nothing here changes.
struct SampleSink {
    bool keep_draws = true;                // false: the combine writes a chunk-sized scratch, post_sample_* is not allocated
    size_t per_extra = 0;                  // doubles of the consumer's scratch per pseudo-trial, the chunk's draws included
    std::function<int()> prelude;          // runs after every check, before anything of the sampler is queued
    // the draws of quantity `which` (1 csd, 2 lfp) of pseudo-trials [p0, p0 + np): F[point][q], rows of ld doubles
    std::function<void(int which, const double *F, long ld, long p0, int np)> consume;
};
static int sample_posterior_impl(gpcsd_ctx *c, const PredCall &q, int nsamples, unsigned long long seed, const double *normals_xi,
                                 const double *normals_eps, const SampleSink *sink = nullptr) {
    const gpcsd_hparams *hp = q.hp;
    const int nz = q.nz, ntstar = q.ntstar, type = q.type;
    posterior_request(c, "sample_posterior", q, REQ_SITES);
    GP_REQUIRE(nsamples >= 1, -3, "sample_posterior: nsamples=%d must be at least 1", nsamples);
    GP_REQUIRE((normals_xi == nullptr) == (normals_eps == nullptr), -3,
               "sample_posterior: give both normals_xi and normals_eps, or neither (the device generator)");
    posterior_request(c, "sample_posterior", q, REQ_HP | REQ_LFP | REQ_NO_HOST_KT);
    const int nx = c->nx, nt = c->nt, R = c->ntrials, S = nsamples;
    const int nq = (type & 1) + ((type >> 1) & 1);               // requested quantities
    const long ns_l = (long)nq * nz + nx, ntt_l = (long)ntstar + nt;
    const long P = (long)R * S;
    // (checked before z or tstar is read)
    GP_REQUIRE(ns_l <= GPCSD_MAX_EIG_N && ntt_l <= GPCSD_MAX_EIG_N, GPCSD_ERR_CAPACITY,
               "sample_posterior: the joint spatial order %ld (sites per requested quantity + electrodes) or temporal order %ld "
               "(ntstar + nt) exceeds the eigensolver's capacity of %d rows (GPCSD_MAX_EIG_N)", ns_l, ntt_l, GPCSD_MAX_EIG_N);
    const int ns = (int)ns_l, ntt = (int)ntt_l;
    // doubles of scratch per pseudo-trial: Xi and Xi Ft^T; E, eps, the residual, W and Bm; S; the prior block and the update
    const size_t per = 2 * (size_t)ns * ntt + 5 * (size_t)nx * nt + (size_t)nz * nt + 2 * (size_t)nz * ntstar + (sink ? sink->per_extra : 0);
    long chunk = (long)std::max<size_t>(1, sample_scratch_budget() / (per * sizeof(double)));
    chunk = std::min(chunk, (GPCSD_MAX_GEMM_LD_KMAJOR - 1) / ntt);       // rows of chunk * nt (or ntstar) doubles are flat GEMM operands
    chunk = std::min(chunk, ((1L << 31) - 1) / std::max(ns, nz));        // chunk * ns rows of Xi, (z, pseudo-trial) columns
    chunk = std::min(chunk, 65535L);                                      // one batch entry per pseudo-trial
    chunk = std::min(chunk, P);
    GP_REQUIRE(chunk >= 1, GPCSD_ERR_CAPACITY, "sample_posterior: one pseudo-trial alone exceeds the capacity of one operand row");
    if (sink && sink->prelude)
        if (int rc = sink->prelude()) return rc;
    PostFront f;                                   // (the trials are read chunk by chunk below, as residuals)
    if (int rc = posterior_front(c, q, FRONT_DRAIN, f)) return rc;
    EigState &e = f.e;
    const Geo g = resident_geo(c);
    hipStream_t s = c->stream;
    const double *dz = f.dz, *dts = f.dts;
    const double *t = (const double *)c->bufs["time_t"].p;
    int *st = c->buf<int>("sp_status", 4);
    GP_HIP(hipMemsetAsync(st, 0, 4 * sizeof(int), s));

    // ---- Js, one triangle block by block: every block is a Gram builder with the sites in the electrodes' place where needed ----
    Geo gz = g;
    gz.x = dz;
    gz.nx = nz;
    double *Js = c->buf<double>("sp_Js", (size_t)ns * ns);
    double *blk = c->buf<double>("sp_blk", std::max((size_t)std::max(nx, nz) * std::max(nx, nz), (size_t)ntt * ntt));      // one block; then Jt
    const int r_csd = 0, r_lfp = (type & 1) ? nz : 0, r_x = nq * nz;      // first rows of CSD(z), LFP(z), LFP(x)
    if (type & 1) {
        build_ks_csd(c, gz, hp->ell_s, blk, s);                                         // CSD(z) - CSD(z)
        k_sym_place(c, Js, ns, r_csd, r_csd, blk, nz, nz, s);
        build_kphig(c, g, hp->R, hp->eps, hp->ell_s, dz, nz, blk, s);                   // LFP(x) - CSD(z)
        k_sym_place(c, Js, ns, r_x, r_csd, blk, nx, nz, s);
    }
    if (type & 2) {
        build_kphi(c, gz, hp->R, hp->eps, hp->ell_s, nullptr, 0, 0.0, blk, s, "kv_");   // LFP(z) - LFP(z)
        k_sym_place(c, Js, ns, r_lfp, r_lfp, blk, nz, nz, s);
        build_kphi(c, g, hp->R, hp->eps, hp->ell_s, dz, nz, 0.0, blk, s);               // LFP(x) - LFP(z)
        k_sym_place(c, Js, ns, r_x, r_lfp, blk, nx, nz, s);
    }
    if (type == 3) {
        build_kphig(c, gz, hp->R, hp->eps, hp->ell_s, dz, nz, blk, s);                  // LFP(z) - CSD(z)
        k_sym_place(c, Js, ns, r_lfp, r_csd, blk, nz, nz, s);
    }
    build_kphi(c, g, hp->R, hp->eps, hp->ell_s, nullptr, 0, 0.0, blk, s);               // LFP(x) - LFP(x)
    k_sym_place(c, Js, ns, r_x, r_x, blk, nx, nx, s);
    double *dsq = c->buf<double>("sp_dsq", (size_t)2 * ns), *ws = c->buf<double>("sp_ws", (size_t)ns);
    double *Fs = c->buf<double>("sp_Fs", (size_t)ns * ns);
    k_sym_equilibrate(c, Js, ns, dsq, dsq + ns, s);
    {
        ProfScope ps(c, "eigh_sample_joint", 9.0 * (double)ns * ns * ns, s);
        eigh_device(c, Js, ns, ws, Fs, st, s);
    }
    k_eig_factor(c, Fs, ws, ns, dsq, Fs, ns, s);

    // ---- Jt on [t*; t] ----
    double *tt = c->buf<double>("sp_tt", (size_t)ntt), *Jt = c->buf<double>("sp_Jt", (size_t)ntt * ntt);
    double *wt = c->buf<double>("sp_wt", (size_t)ntt), *Ft = c->buf<double>("sp_Ft", (size_t)ntt * ntt);
    GP_HIP(hipMemcpyAsync(tt, dts, (size_t)ntstar * sizeof(double), hipMemcpyDeviceToDevice, s));
    GP_HIP(hipMemcpyAsync(tt + ntstar, t, (size_t)nt * sizeof(double), hipMemcpyDeviceToDevice, s));
    build_kt(c, hp, tt, ntt, tt, ntt, blk, s);
    k_sym_place(c, Jt, ntt, 0, 0, blk, ntt, ntt, s);                                   // (both triangles from one, as Js)
    {
        ProfScope ps(c, "eigh_sample_joint", 9.0 * (double)ntt * ntt * ntt, s);
        eigh_device(c, Jt, ntt, wt, Ft, st + 1, s);
    }
    k_eig_factor(c, Ft, wt, ntt, nullptr, Ft, ntt, s);

    // ---- the noise factor Qs diag(sqrt(sig2n)) ----
    double *Fn = c->buf<double>("sp_Fn", (size_t)nx * nx);
    k_eig_factor(c, e.Qs, e.d_sig, e.nsig, nullptr, Fn, nx, s);

    // ---- chunks of pseudo-trials ----
    const size_t cn = (size_t)chunk;
    double *Xi = c->buf<double>("sp_Xi", cn * ns * ntt), *T1 = c->buf<double>("sp_T1", cn * ns * ntt);
    double *E = c->buf<double>("sp_E", cn * nx * nt), *eps = c->buf<double>("sp_eps", cn * nx * nt);
    double *res = c->buf<double>("sp_res", cn * nx * nt);
    double *W = c->buf<double>("proj_W", cn * nx * nt), *Bm = f.Bm = c->buf<double>("pred_B", cn * nx * nt);
    double *Sm = c->buf<double>("pred_S", cn * nz * nt);
    double *fp = c->buf<double>("sp_prior", cn * nz * ntstar), *upd = c->buf<double>("sp_upd", cn * nz * ntstar);
    double *out[2] = {nullptr, nullptr};
    const bool keep = !sink || sink->keep_draws;
    for (int w = 0; w < 2; ++w)
        if (keep && (type & (w + 1))) out[w] = c->buf<double>(w ? "post_sample_lfp" : "post_sample_csd", (size_t)nz * ntstar * P);
    double *draw = keep ? nullptr : c->buf<double>("feat_draw", cn * nz * ntstar);       // one chunk of one quantity
    const unsigned long long pg0 = (unsigned long long)c->trial_offset * (unsigned long long)S;     // first global pseudo-trial
    for (long p0 = 0; p0 < P; p0 += chunk) {
        const int np = (int)std::min(chunk, P - p0);
        const size_t nxi = (size_t)np * ns * ntt, ne = (size_t)np * nx * nt;
        if (normals_xi) {
            c->copy_in(Xi, normals_xi + (size_t)p0 * ns * ntt, nxi * sizeof(double), s);
            c->copy_in(E, normals_eps + (size_t)p0 * nx * nt, ne * sizeof(double), s);
        } else {
            k_normals(c, seed, 0u, (pg0 + (unsigned long long)p0) * ((unsigned long long)ns * ntt), (long)nxi, Xi, s);
            k_normals(c, seed, 1u, (pg0 + (unsigned long long)p0) * ((unsigned long long)nx * nt), (long)ne, E, s);
        }
        const long RT = (long)np * nt;
        GemmDesc g1;                      // T1[(q, k)][j] = sum_m Xi[(q, k)][m] Ft[j][m]
        g1.M = np * ns; g1.N = ntt; g1.K = ntt;
        g1.A = Xi; g1.lda = ntt; g1.B = Ft; g1.ldb = ntt; g1.transB = true; g1.C = T1; g1.ldc = ntt;
        g1.prof_name = "gemm_sample_temporal";
        gemm_f64(c, g1, s);
        GemmDesc g2;                      // phi[x][q][i] = sum_k Fs[LFP(x) row x][k] T1[(q, k)][ntstar + i]
        g2.M = nx; g2.N = nt; g2.K = ns;
        g2.A = Fs + (size_t)r_x * ns; g2.lda = ns; g2.B = T1 + ntstar; g2.ldb = ntt; g2.C = res; g2.ldc = RT;
        g2.batch = np; g2.sB = (long)ns * ntt; g2.sC = nt;
        g2.prof_name = "gemm_sample_spatial";
        gemm_f64(c, g2, s);
        GemmDesc g3;                      // eps[x][q][i] = sum_x' Fn[x][x'] E[(q, x')][i]
        g3.M = nx; g3.N = nt; g3.K = nx;
        g3.A = Fn; g3.lda = nx; g3.B = E; g3.ldb = nt; g3.C = eps; g3.ldc = RT;
        g3.batch = np; g3.sB = (long)nx * nt; g3.sC = nt;
        g3.prof_name = "gemm_sample_noise";
        gemm_f64(c, g3, s);
        k_sample_residual(c, c->d_lfp, res, eps, res, nx, nt, R, p0, np, S, s);
        pred_data_spatial(c, e, W, res, np);
        pred_data_temporal(c, e, W, Bm, np);
        for (int which = 1; which <= 2; ++which) {
            if (!(type & which)) continue;
            GemmDesc g4;                  // fp[z][q][j] = sum_k Fs[row z of the quantity][k] T1[(q, k)][j], j < ntstar
            g4.M = nz; g4.N = ntstar; g4.K = ns;
            g4.A = Fs + (size_t)(which == 1 ? r_csd : r_lfp) * ns; g4.lda = ns; g4.B = T1; g4.ldb = ntt; g4.C = fp;
            g4.ldc = (long)np * ntstar;
            g4.batch = np; g4.sB = (long)ns * ntt; g4.sC = ntstar;
            g4.prof_name = "gemm_sample_spatial";
            gemm_f64(c, g4, s);
            pred_mean_tail(c, f, q, which, np, Sm, upd, nullptr, 0);     // upd[z][j][q] = P (the residuals), the components summed
            // the one add pass: + f_prior, into (z, t*, p)
            if (keep) k_sample_combine(c, upd, fp, out[which - 1], nz, ntstar, np, P, p0, s);
            else k_sample_combine(c, upd, fp, draw, nz, ntstar, np, np, 0, s);
            if (sink) sink->consume(which, keep ? out[which - 1] + p0 : draw, keep ? P : (long)np, p0, np);
        }
    }
    const int rc = finish_call(c, e, nullptr, 0);      // (waits for everything queued above)
    const int rc2 = finish_status(c, st);
    return rc != 0 ? rc : rc2;
}

extern "C" int gpcsd_sample_posterior_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar,
                                               int ntstar, int type, int nsamples, unsigned long long seed, const double *normals_xi,
                                               const double *normals_eps) {
    GP_API_BEGIN(c)
    return sample_posterior_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, false, false), nsamples, seed, normals_xi, normals_eps);
    GP_API_END(c)
}

extern "C" int gpcsd_sample_posterior(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar,
                                      int type, int nsamples, unsigned long long seed, const double *normals_xi,
                                      const double *normals_eps, double *csd, double *lfp) {
    GP_API_BEGIN(c)
    const int rc = sample_posterior_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, false, false), nsamples, seed, normals_xi, normals_eps);
    if (rc < 0) return rc;
    const size_t count = (size_t)nz * ntstar * c->ntrials * nsamples;
    download_outputs(c, {{(type & 1) ? csd : nullptr, "post_sample_csd", count}, {(type & 2) ? lfp : nullptr, "post_sample_lfp", count}});
    return rc;
    GP_API_END(c)
}
