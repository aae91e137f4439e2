// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip, capi_fused.inl and capi_posterior.inl are in scope) --
// posterior mean and covariance of linear functionals of the CSD / LFP field (gpcsd_predict_functionals) and its Gram kernel alone
// (gpcsd_fun_gram).

// Scratch of one call, in bytes: GPCSD_FUN_SCRATCH_MB (read per call: tests force the capacity error with it), 2048 MB otherwise --
// J = 64 functionals over 384 x 500 with two temporal components need 197 MB for alpha and about as much again for the rest.
static size_t fun_scratch_budget() {
    const char *e = getenv("GPCSD_FUN_SCRATCH_MB");
    const long mb = e ? atol(e) : 0;
    return (size_t)(mb > 0 ? mb : 2048) << 20;
}

extern "C" int gpcsd_fun_gram_chunk(int K) { return K > 0 ? fun_gram_chunk(K) : -3; }

// The Gram kernel alone on host arrays (no reference counterpart; fungram.hip): upload, two launches, download.
extern "C" int gpcsd_fun_gram(gpcsd_ctx *c, const double *A, int C, int nb, int J, int K, const double *s, const double *B, int N,
                              double *out) {
    GP_API_BEGIN(c)
    GP_REQUIRE(A && out && nb > 0 && J > 0 && K > 0 && (B == nullptr || N > 0), -3, "fun_gram: bad arguments");
    GP_REQUIRE(C >= 1 && C <= GPCSD_MAX_TEMPORAL, -3, "fun_gram: C=%d outside [1,%d]", C, GPCSD_MAX_TEMPORAL);
    const int Nn = B ? N : J;
    const size_t plane = (size_t)J * Nn;
    double *dA = c->upload<double>("op_in0", A, (size_t)C * nb * J * K);
    double *ds = s ? c->upload<double>("op_in1", s, (size_t)nb * K) : nullptr;
    double *dB = B ? c->upload<double>("op_in2", B, (size_t)nb * N * K) : nullptr;
    double *dO = c->buf<double>("op_out", plane * (C + 1));
    FunGramDesc d;
    d.A = dA; d.C = C; d.nb = nb; d.J = J; d.K = K; d.s = ds; d.B = dB; d.N = Nn;
    d.part = c->buf<double>("fun_part", fun_gram_part_elems(C, nb, J, K, Nn));
    d.list = dO; d.sum = dO + plane * C;
    k_fun_gram(c, d, c->stream);
    c->download(out, dO, plane * (C + 1) * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

// Posterior mean and covariance of J linear functionals <W_j, f> of the field f at the sites z and times t* of gpcsd_predict_at
// (gpcsd_predict_functionals; no reference counterpart), of the model whose mean that call returns: front_half(c, hp, 0.0), no jitter,
// a noise list on the eigen-index, the LFP the noise-free potential.  With M1 = Kcross^T Qs, P_c[i'][s] = sum_i Qt[i][i'] k_c(t*_s, t_i),
// Dinv and Bm = (Qs^T y Qt) / D of the prediction front, Kzz the prior spatial covariance at the sites and Ktt_c = k_c(t*, t*):
//   alpha_j^c[x'][i'] = sum_z sum_s M1[z][x'] W_j[z][s] P_c[i'][s]           c < C; plane C reads sum_c alpha^c (never stored)
//   expl_p[j][k]  = sum_{x',i'} alpha_j^p alpha_k^p Dinv[x'][i']
//   mean_p[j][r]  = sum_{x',i'} alpha_j^p Bm[x'][r][i']
//   prior_p[j][k] = sum_{z,s} (Kzz W_j Ktt_p)[z][s] W_k[z][s]               Ktt_C = sum_c Ktt_c, added as alpha is
//   cov_p = prior_p - expl_p                                                  (unclamped)
// alpha for all J functionals is two products of the GEMM core per component, J in the place of the trials of the [x'][j][i']
// layout; so are Kzz W_k and (.) Ktt_c.  The three sums over (x', i') resp. (z, s) are k_fun_gram launches (fungram.hip): the
// explained term is its symmetric form, the prior is made symmetric bit for bit from its lower triangle (as k_sym_place treats the
// builders' blocks, whose diagonal blocks are symmetric only to ~1e-11).  The covariances read no trial data.
// Outputs per quantity q: fun_mean_q (J, R), fun_cov_q / fun_prior_q (J, J) and their _list forms (C times that).
static int predict_functionals_impl(gpcsd_ctx *c, const PredCall &q, const double *W, int J) {
    const gpcsd_hparams *hp = q.hp;
    const int nz = q.nz, ntstar = q.ntstar, type = q.type;
    GP_REQUIRE(W && J > 0, -3, "predict_functionals: bad arguments");
    posterior_request(c, "predict_functionals", q, REQ_SITES | REQ_HP);
    GP_REQUIRE(hp->n_temporal >= 1 && hp->n_temporal <= GPCSD_MAX_TEMPORAL, -3, "n_temporal=%d outside [1,%d]", hp->n_temporal,
               GPCSD_MAX_TEMPORAL);
    posterior_request(c, "predict_functionals", q, REQ_LFP | REQ_NO_HOST_KT);
    const int nx = c->nx, nt = c->nt, R = c->ntrials, C = hp->n_temporal;
    // (checked before z, tstar or W is read) rows of the flat products, one batch entry per functional, and the scratch
    const long ldmax = std::max({(long)C * ntstar, (long)J * nt, (long)J * ntstar, (long)R * nt, (long)R * ntstar});
    GP_REQUIRE(ldmax < (1L << 22) && J <= 65535 && (long)J * nz < (1L << 31) && (long)nz * R < (1L << 31), GPCSD_ERR_CAPACITY,
               "predict_functionals: a row of %ld doubles (J * nt, J * ntstar, ntrials * nt or n_temporal * ntstar) or J = %d "
               "functionals (at most 65535) exceed the capacity of one operand", ldmax, J);
    const size_t n_alpha = (size_t)C * J * nx * nt, n_T = (size_t)J * nz * nt, n_W = (size_t)J * nz * ntstar;
    const size_t n_part = std::max({fun_gram_part_elems(C, nx, J, nt, J), fun_gram_part_elems(C, nx, J, nt, R),
                                    fun_gram_part_elems(C, nz, J, ntstar, J)});
    const size_t need = (n_alpha + n_T + (size_t)(3 + C) * n_W + n_part) * sizeof(double);
    GP_REQUIRE(need <= fun_scratch_budget(), GPCSD_ERR_CAPACITY,
               "predict_functionals: J = %d functionals need %zu MB of scratch (alpha alone n_temporal * J * nx * nt = %zu doubles), "
               "more than the budget of %zu MB (GPCSD_FUN_SCRATCH_MB)", J, need >> 20, n_alpha, fun_scratch_budget() >> 20);
    PostFront f;
    if (int rc = posterior_front(c, q, FRONT_DRAIN | FRONT_TRIALS, f)) return rc;
    const EigState &e = f.e;
    const Geo g = resident_geo(c);
    hipStream_t s = c->stream;
    const double *Pc = f.Pc, *dz = f.dz, *dts = f.dts;
    double *dW = c->upload<double>("fun_W", W, n_W);
    double *Wt = c->buf<double>("fun_Wt", n_W), *X = c->buf<double>("fun_X", n_W), *V = c->buf<double>("fun_V", (size_t)C * n_W);
    double *T = c->buf<double>("fun_T", n_T), *alpha = c->buf<double>("fun_alpha", n_alpha);
    double *part = c->buf<double>("fun_part", n_part);
    double *Ktt = c->buf<double>("fun_Ktt", (size_t)C * ntstar * ntstar);
    double *blk = c->buf<double>("fun_blk", (size_t)nz * nz), *Kzz = c->buf<double>("fun_Kzz", (size_t)nz * nz);
    const size_t JJ = (size_t)J * J;
    double *expl = c->buf<double>("fun_expl", (C + 1) * JJ), *raw = c->buf<double>("fun_prior_raw", (C + 1) * JJ);
    k_fun_relayout(c, dW, J, nz, ntstar, Wt, s);                                        // Wt[z][j][s]
    for (int cc = 0; cc < C; ++cc)
        temporal_cross_gram(c, hp, cc, dts, ntstar, dts, ntstar, Ktt + (size_t)cc * ntstar * ntstar, s);
    Geo gz = g;
    gz.x = dz;
    gz.nx = nz;
    for (int which = 1; which <= 2; ++which) {
        if (!(type & which)) continue;
        const std::string q = which == 1 ? "csd" : "lfp";
        // ---- the prior: Kzz from the builders gpcsd_sample_posterior runs at the sites, both triangles from one ----
        if (which == 1) build_ks_csd(c, gz, hp->ell_s, blk, s);
        else build_kphi(c, gz, hp->R, hp->eps, hp->ell_s, nullptr, 0, 0.0, blk, s, "kv_");
        k_sym_place(c, Kzz, nz, 0, 0, blk, nz, nz, s);
        for (int cc = 0; cc < C; ++cc) {
            GemmDesc g1;                  // X[(j, z')][s] = sum_s' W[(j, z')][s'] Ktt_c[s'][s]
            g1.M = J * nz; g1.N = ntstar; g1.K = ntstar;
            g1.A = dW; g1.lda = ntstar; g1.B = Ktt + (size_t)cc * ntstar * ntstar; g1.ldb = ntstar; g1.C = X; g1.ldc = ntstar;
            g1.prof_name = "gemm_fun_WKtt";
            gemm_f64(c, g1, s);
            GemmDesc g2;                  // V_c[z][j][s] = sum_z' Kzz[z][z'] X[j][z'][s]
            g2.M = nz; g2.N = ntstar; g2.K = nz;
            g2.A = Kzz; g2.lda = nz; g2.B = X; g2.ldb = ntstar; g2.C = V + (size_t)cc * n_W; g2.ldc = (long)J * ntstar;
            g2.batch = J; g2.sB = (long)nz * ntstar; g2.sC = ntstar;
            g2.prof_name = "gemm_fun_KzzX";
            gemm_f64(c, g2, s);
        }
        FunGramDesc pr;                   // raw[p][j][k] = sum_{z,s} V_p[z][j][s] Wt[z][k][s]
        pr.A = V; pr.C = C; pr.nb = nz; pr.J = J; pr.K = ntstar; pr.B = Wt; pr.N = J;
        pr.part = part; pr.list = raw; pr.sum = raw + C * JJ;
        pr.prof_name = "fun_gram_prior";
        k_fun_gram(c, pr, s);
        // ---- alpha ----
        for (int cc = 0; cc < C; ++cc) {
            GemmDesc g3;                  // T[(j, z)][i'] = sum_s W[(j, z)][s] Pcat[i'][cc * ntstar + s]
            g3.M = J * nz; g3.N = nt; g3.K = ntstar;
            g3.A = dW; g3.lda = ntstar; g3.B = Pc + (size_t)cc * ntstar; g3.ldb = (long)C * ntstar; g3.transB = true; g3.C = T; g3.ldc = nt;
            g3.prof_name = "gemm_fun_WP";
            gemm_f64(c, g3, s);
            GemmDesc g4;                  // alpha_c[x'][j][i'] = sum_z M1[z][x'] T[j][z][i']
            g4.M = nx; g4.N = nt; g4.K = nz;
            g4.A = f.M1 + (size_t)(which - 1) * nz * nx; g4.lda = nx; g4.transA = true; g4.B = T; g4.ldb = nt;
            g4.C = alpha + (size_t)cc * nx * J * nt; g4.ldc = (long)J * nt;
            g4.batch = J; g4.sB = (long)nz * nt; g4.sC = nt;
            g4.prof_name = "gemm_fun_alpha";
            gemm_f64(c, g4, s);
        }
        FunGramDesc ex;                   // expl[p][j][k] = sum_{x',i'} alpha_j^p alpha_k^p Dinv[x'][i']
        ex.A = alpha; ex.C = C; ex.nb = nx; ex.J = J; ex.K = nt; ex.s = e.Dinv;
        ex.part = part; ex.list = expl; ex.sum = expl + C * JJ;
        ex.prof_name = "fun_gram_expl";
        k_fun_gram(c, ex, s);
        FunGramDesc mn;                   // mean[p][j][r] = sum_{x',i'} alpha_j^p Bm[x'][r][i']   (Bm carries 1 / D already)
        mn.A = alpha; mn.C = C; mn.nb = nx; mn.J = J; mn.K = nt; mn.B = f.Bm; mn.N = R;
        mn.part = part;
        mn.list = c->buf<double>("fun_mean_" + q + "_list", (size_t)C * J * R);
        mn.sum = c->buf<double>("fun_mean_" + q, (size_t)J * R);
        mn.prof_name = "fun_gram_mean";
        k_fun_gram(c, mn, s);
        double *prior_l = c->buf<double>("fun_prior_" + q + "_list", C * JJ), *prior_s = c->buf<double>("fun_prior_" + q, JJ);
        double *cov_l = c->buf<double>("fun_cov_" + q + "_list", C * JJ), *cov_s = c->buf<double>("fun_cov_" + q, JJ);
        k_fun_finish(c, raw, expl, J, C, prior_l, cov_l, s);
        k_fun_finish(c, raw + C * JJ, expl + C * JJ, J, 1, prior_s, cov_s, s);
    }
    return finish_call(c, e, nullptr, 0);
}

extern "C" int gpcsd_predict_functionals_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar,
                                                  int ntstar, const double *W, int J, int type) {
    GP_API_BEGIN(c)
    return predict_functionals_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, true, false), W, J);
    GP_API_END(c)
}

extern "C" int gpcsd_predict_functionals(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar,
                                         const double *W, int J, int type, double *csd_mean_list, double *csd_mean,
                                         double *csd_cov_list, double *csd_cov, double *csd_prior_list, double *csd_prior,
                                         double *lfp_mean_list, double *lfp_mean, double *lfp_cov_list, double *lfp_cov,
                                         double *lfp_prior_list, double *lfp_prior) {
    GP_API_BEGIN(c)
    const int rc = predict_functionals_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, true, false), W, J);
    if (rc < 0) return rc;
    const size_t C = (size_t)hp->n_temporal, JJ = (size_t)J * J, JR = (size_t)J * c->ntrials;
    double *const host[2][6] = {{csd_mean_list, csd_mean, csd_cov_list, csd_cov, csd_prior_list, csd_prior},
                                {lfp_mean_list, lfp_mean, lfp_cov_list, lfp_cov, lfp_prior_list, lfp_prior}};
    static const char *const kind[3] = {"fun_mean_", "fun_cov_", "fun_prior_"};
    std::vector<HostOut> outs;
    for (int w = 0; w < 2; ++w) {
        if (!(type & (w + 1))) continue;
        for (int k = 0; k < 3; ++k) {
            const std::string name = std::string(kind[k]) + (w ? "lfp" : "csd");
            outs.push_back({host[w][2 * k], name + "_list", C * (k == 0 ? JR : JJ)});
            outs.push_back({host[w][2 * k + 1], name, k == 0 ? JR : JJ});
        }
    }
    download_outputs(c, outs);
    return rc;
    GP_API_END(c)
}
