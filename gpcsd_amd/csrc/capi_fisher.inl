// Part of capi.hip (included there, behind capi_grad.inl: its Kronecker helpers and hp_image are in scope) --
// hyper-parameter uncertainty: per-trial scores and the expected Fisher information of one trial (fisher.hip).
//
// Natural parameters in the order of gpcsd_loglik_grad: [R, ell_s (dim), (ell_t, sigma2_t) per component, sig2n], scalar noise.
// The front half is front_half(c, hp, hp->jitter) -- the model of gpcsd_loglik, through the decomposition cache -- in the merged
// (full-size, eigenvector) basis, which holds for every geometry; B is the prediction front's Bm = (Qs^T Y Qt) / D as [x][r][t].
//   spatial p:   dKs/dR = dA T^T + T dA^T (T = A Kgl), dKs/dell_k = (A dKgl_k) A^T;   Ahat_p = Qs^T dKs_p Qs
//   temporal q:  dKt/d(ell_c, sigma2_c) elementwise (or the caller's matrices);        Bhat_q = Qt^T dKt_q Qt
//   scores:      s[r][i] = 1/2 quad_i[r] - 1/2 trace_i   quad: k_fisher_score (spatial: one launch, temporal: one launch),
//                                                         the noise direction's is sum B_r^2; trace: k_fisher_diag
//   information: spatial-spatial 1/2 <Ahat_p o Ahat_p', M>, M = (U diag(et^2)) U^T; temporal-temporal 1/2 <Bhat_q o Bhat_q', N>,
//                N = U^T diag(es^2) U (two K-scaled products of the GEMM core, k_fisher_pairs); every other block from the
//                diagonals alone (k_fisher_diag).  It reads no trial data.
// Only pairs i <= j are formed and the host mirrors them: the information is symmetric bit for bit.

namespace {
struct FisherOut {
    int ng = 0, nsp = 0, ntp = 0;
    double *diag = nullptr;         // device: [ng traces][pairs i <= j of the diagonal forms]
    double *pss = nullptr, *ptt = nullptr;      // device: pairs of the spatial / temporal directions
};

// shapes of a context without resident data, for the duration of a call that reads none: the geometry's and the time grid's
struct ShapeGuard {
    gpcsd_ctx *c;
    int nx, nt, R;
    bool on;
    explicit ShapeGuard(gpcsd_ctx *ctx) : c(ctx), nx(ctx->nx), nt(ctx->nt), R(ctx->ntrials), on(ctx->d_lfp == nullptr) {
        if (on) {
            c->nx = c->geo_nx; c->nt = c->time_nt; c->ntrials = 0;
        }
    }
    ~ShapeGuard() {
        if (on) {
            c->nx = nx; c->nt = nt; c->ntrials = R;
        }
    }
};
}  // namespace

static int fisher_impl(gpcsd_ctx *c, const gpcsd_hparams *hp, int ng, bool want_scores, bool want_info, FisherOut &out) {
    GP_REQUIRE(hp != nullptr, -3, "fisher: null hparams");
    GP_REQUIRE(hp->n_sig2n == 1, -3,
               "fisher: a per-electrode noise list ties the noise to the eigen-index of Ks -- the model is not a function of Ks alone -- "
               "and is not supported (scalar sig2n only)");
    const Geo g = resident_geo(c);
    GP_REQUIRE(c->time_nt > 0, -4, "time grid not set (call gpcsd_set_time)");
    GP_REQUIRE(!want_scores || c->d_lfp != nullptr, -4, "trial_scores: lfp not set (call gpcsd_set_lfp)");
    const int C = hp->n_temporal, nsp = 1 + g.dim, ntp = 2 * C;
    GP_REQUIRE(ng == nsp + ntp + 1, -3, "fisher: ng=%d, expected %d", ng, nsp + ntp + 1);
    ShapeGuard shapes(c);
    const int nx = c->nx, nt = c->nt, R = c->ntrials, G = g.G();
    const bool host_kt = uses_host_kt(hp);
    GP_REQUIRE(!host_kt || (c->host_kt_on && c->host_kt_nt == nt && c->host_dkt_n == ntp && c->host_dkt.size() == (size_t)ntp * nt * nt),
               -3, "fisher: user-defined temporal covariances need their Gram matrix and the %d derivative matrices "
               "d Kt / d (ell_c, sigma2_c) (gpcsd_set_host_temporal_gram + gpcsd_set_host_temporal_dgram)", ntp);
    const long RT = (long)R * nt, nxx = (long)nx * nx, ntt = (long)nt * nt, nxG = (long)nx * G;
    GP_REQUIRE(RT < GPCSD_MAX_GEMM_LD_KMAJOR && (long)nx * R < (1L << 31), GPCSD_ERR_CAPACITY,
               "trial_scores: ntrials * nt = %ld exceeds the capacity of one operand row (%ld doubles; GPCSD_MAX_GEMM_LD_KMAJOR)", RT,
               (long)GPCSD_MAX_GEMM_LD_KMAJOR);
    if (int rc = drain_async(c)) return rc;
    EigState e = front_half(c, hp, hp->jitter, true, true, false, -1, false, /*need_lfp=*/want_scores);
    hipStream_t s = c->stream;
    out.ng = ng; out.nsp = nsp; out.ntp = ntp;

    // ---- spatial directions: the Gram builders' own launches (capi_grad.inl), then dKs_p and its rotation
    const HpDev himg = hp_image(hp);
    GradPlan P;
    P.g = g; P.nx = nx; P.B = 1; P.G = G; P.nxG = nxG; P.GG = (long)G * G; P.nxx = nxx;
    P.n1 = g.ngl1; P.n2 = g.dim == 2 ? g.ngl2 : 0; P.kron = g.dim == 2; P.s = s;
    P.tab = c->upload_cached<HpDev>("fi_hp_tab", &himg, 1);
    P.A = c->buf<double>("fi_A", nxG); P.Tm = c->buf<double>("fi_T", nxG);
    double *Tl[2] = {c->buf<double>("fi_Tl1", nxG), nullptr};
    if (P.kron) {
        P.K1 = c->buf<double>("fi_K1", (size_t)P.n1 * P.n1); P.dK1 = c->buf<double>("fi_dK1", (size_t)P.n1 * P.n1);
        P.K2 = c->buf<double>("fi_K2", (size_t)P.n2 * P.n2); P.dK2 = c->buf<double>("fi_dK2", (size_t)P.n2 * P.n2);
        P.Uk = c->buf<double>("fi_U", nxG); P.U2 = c->buf<double>("fi_U2", nxG);
        P.Tl1 = Tl[0]; P.Tl2 = Tl[1] = c->buf<double>("fi_Tl2", nxG);
    } else {
        P.Kgl = c->buf<double>("fi_Kgl", P.GG);
    }
    double *dKs = c->buf<double>("fi_dKs", (size_t)nsp * nxx), *rot = c->buf<double>("fi_rot", (size_t)std::max(nsp * nxx, ntp * ntt));
    double *Ah = c->buf<double>("fi_Ahat", (size_t)nsp * nxx), *Bh = c->buf<double>("fi_Bhat", (size_t)ntp * ntt);
    grad_spatial_gram(c, P, rot);                        // A, T = A Kgl (and the axis factors); the Gram itself is not used
    if (P.kron) {                                        // Tl1 = A (dK1 (x) K2), Tl2 = A (K1 (x) dK2): never the flat G x G matrix
        kron_axis1(c, P, P.dK1, P.Uk, P.Tl1, "gemm_fisher_dK1U");
        kron_axis2(c, P, P.dK2, P.U2, "gemm_fisher_AdK2");
        kron_axis1(c, P, P.K1, P.U2, P.Tl2, "gemm_fisher_K1U2");
    } else {                                             // 1D: dKgl from the axis builder, Tl1 = A dKgl
        double *dKgl = c->buf<double>("fi_dKgl", P.GG);
        k_se_axis_tab(c, g.gx1, G, 0, P.tab, 1, P.Kgl, dKgl, s);
        GemmDesc d;
        d.M = nx; d.N = G; d.K = G; d.A = P.A; d.lda = G; d.B = dKgl; d.ldb = G; d.C = Tl[0]; d.ldc = G;
        d.prof_name = "gemm_fisher_AdKgl";
        gemm_f64(c, d, s);
    }
    double *dA = c->buf<double>("fi_dA", nxG);
    k_fisher_dA_dR(c, g.x, nx, g.gx1, g.gw1, g.gx2, g.gw2, G, P.n2, hp->R, hp->eps, dA, s);
    auto xyT = [&](const double *X, const double *Y, double *Cm, int epi, const char *name) {      // C (+)= X Y^T, nx x G x nx
        GemmDesc d;
        d.M = nx; d.N = nx; d.K = G; d.A = X; d.lda = G; d.B = Y; d.ldb = G; d.transB = true; d.C = Cm; d.ldc = nx; d.epi = epi;
        d.prof_name = name;
        gemm_f64(c, d, s);
    };
    xyT(dA, P.Tm, dKs, EPI_STORE, "gemm_fisher_dKsR");
    xyT(P.Tm, dA, dKs, EPI_ACCUM, "gemm_fisher_dKsR");
    for (int k = 0; k < g.dim; ++k) xyT(Tl[k], P.A, dKs + (1 + k) * nxx, EPI_STORE, "gemm_fisher_dKsell");
    // Xhat_p = Q^T X_p Q for a stack of np matrices of order n
    auto rotate = [&](const double *X, const double *Q, int n, int np, double *Xh) {
        const long nn = (long)n * n;
        GemmDesc a;                                      // rot_p = X_p Q
        a.M = n; a.N = n; a.K = n; a.A = X; a.lda = n; a.B = Q; a.ldb = n; a.C = rot; a.ldc = n;
        a.batch = np; a.sA = nn; a.sB = 0; a.sC = nn;
        GemmDesc b;                                      // Xhat_p = Q^T rot_p
        b.M = n; b.N = n; b.K = n; b.A = Q; b.lda = n; b.transA = true; b.B = rot; b.ldb = n; b.C = Xh; b.ldc = n;
        b.batch = np; b.sA = 0; b.sB = nn; b.sC = nn;
        a.prof_name = b.prof_name = "gemm_fisher_rotate";
        gemm_f64(c, a, s);
        gemm_f64(c, b, s);
    };
    rotate(dKs, e.Qs, nx, nsp, Ah);

    // ---- temporal directions
    double *dKt = c->buf<double>("fi_dKt", (size_t)ntp * ntt);
    if (host_kt) {
        c->copy_in(dKt, c->host_dkt.data(), (size_t)ntp * ntt * sizeof(double), s);
    } else {
        TemporalSet ts{};
        ts.ncomp = C;
        for (int i = 0; i < C; ++i) {
            ts.kind[i] = hp->kind[i]; ts.ell[i] = hp->ell_t[i]; ts.sigma2[i] = hp->sigma2_t[i];
        }
        k_fisher_temporal_dgram(c, ts, (const double *)c->bufs["time_t"].p, nt, dKt, s);
    }
    double *W = nullptr, *Bm = nullptr;
    if (want_scores) {
        W = c->buf<double>("proj_W", (size_t)nx * RT);
        Bm = c->buf<double>("pred_B", (size_t)nx * RT);
        pred_data_spatial(c, e, W, c->d_lfp, R);
    }
    join_temporal(c, e, nullptr, false);                 // Qt, et, D and U = Dinv from here on
    rotate(dKt, e.Qt, nt, ntp, Bh);

    // ---- the diagonals' sums: traces of the scores; cross and noise blocks of the information
    double *sv = c->buf<double>("fi_sv", (size_t)ng * nx), *tv = c->buf<double>("fi_tv", (size_t)ng * nt);
    double *es2 = c->buf<double>("fi_es2", nx), *et2 = c->buf<double>("fi_et2", nt);
    k_fisher_weights(c, Ah, Bh, e.es, e.et, nx, nt, nsp, ntp, sv, tv, es2, et2, s);
    out.diag = c->buf<double>("fi_diag", (size_t)ng + (size_t)ng * (ng + 1) / 2);
    k_fisher_diag(c, sv, tv, e.Dinv, nx, nt, ng, out.diag, s);

    if (want_info) {
        double *Mm = c->buf<double>("fi_M", nxx), *Nm = c->buf<double>("fi_N", ntt);
        GemmDesc m;                                      // M = (U diag(et^2)) U^T
        m.M = nx; m.N = nx; m.K = nt; m.A = e.Dinv; m.lda = nt; m.kscale = et2; m.B = e.Dinv; m.ldb = nt; m.transB = true;
        m.C = Mm; m.ldc = nx; m.prof_name = "gemm_fisher_M";
        gemm_f64(c, m, s);
        GemmDesc n;                                      // N = (U^T diag(es^2)) U
        n.M = nt; n.N = nt; n.K = nx; n.A = e.Dinv; n.lda = nt; n.transA = true; n.kscale = es2; n.B = e.Dinv; n.ldb = nt;
        n.C = Nm; n.ldc = nt; n.prof_name = "gemm_fisher_N";
        gemm_f64(c, n, s);
        out.pss = c->buf<double>("fi_pairs_s", (size_t)nsp * (nsp + 1) / 2);
        out.ptt = c->buf<double>("fi_pairs_t", (size_t)ntp * (ntp + 1) / 2);
        k_fisher_pairs(c, Ah, Mm, nxx, nsp, out.pss, s);
        k_fisher_pairs(c, Bh, Nm, ntt, ntp, out.ptt, s);
    }

    if (want_scores) {
        pred_data_temporal(c, e, W, Bm, R);
        double *quad = c->buf<double>("fi_quad", (size_t)ng * R);
        FisherScoreDesc ds;                              // (Ahat_p B)[x][(r,i)] B[x][(r,i)] et[i]: all spatial directions, one launch
        ds.A = Ah; ds.lda = nx; ds.sA = nxx; ds.B = Bm; ds.ldb = RT; ds.sB = 0; ds.E = Bm; ds.lde = RT; ds.w = e.et;
        ds.M = nx; ds.N = (int)RT; ds.K = nx; ds.batch = nsp; ds.trial_in_col = true; ds.nt = nt; ds.R = R;
        ds.quad = quad; ds.prof_name = "fisher_score_spatial";
        k_fisher_score(c, ds, s);
        FisherScoreDesc dt;                              // (B Bhat_q)[(x,r)][i] B[(x,r)][i] es[x]: all temporal directions, one launch
        dt.A = Bm; dt.lda = nt; dt.sA = 0; dt.B = Bh; dt.ldb = nt; dt.sB = ntt; dt.E = Bm; dt.lde = nt; dt.w = e.es;
        dt.M = nx * R; dt.N = nt; dt.K = nt; dt.batch = ntp; dt.trial_in_col = false; dt.nt = nt; dt.R = R;
        dt.quad = quad + (size_t)nsp * R; dt.prof_name = "fisher_score_temporal";
        k_fisher_score(c, dt, s);
        k_fisher_trial_sumsq(c, Bm, nx, R, nt, quad + (size_t)(nsp + ntp) * R, s);
        k_fisher_scores(c, quad, out.diag, R, ng, c->buf<double>("trial_scores", (size_t)R * ng), s);
    }
    return finish_call(c, e, nullptr, 0);
}

extern "C" int gpcsd_fisher(gpcsd_ctx *c, const gpcsd_hparams *hp, double *info, int ng) {
    GP_API_BEGIN(c)
    GP_REQUIRE(info != nullptr, -3, "fisher: null output");
    FisherOut o;
    const int rc = fisher_impl(c, hp, ng, false, true, o);
    if (rc != 0) return rc;
    const int npd = ng * (ng + 1) / 2, nps = o.nsp * (o.nsp + 1) / 2, npt = o.ntp * (o.ntp + 1) / 2;
    std::vector<double> hd((size_t)ng + npd), hs(nps), ht(npt);
    c->download(hd.data(), o.diag, hd.size() * sizeof(double));
    c->download(hs.data(), o.pss, hs.size() * sizeof(double));
    c->download(ht.data(), o.ptt, ht.size() * sizeof(double));
    c->sync();
    // I_ij = 1/2 (pair sum), pairs i <= j in row order; both triangles from the one value
    auto put = [&](int i, int j, double v) { info[(size_t)i * ng + j] = info[(size_t)j * ng + i] = 0.5 * v; };
    int k = 0;
    for (int i = 0; i < ng; ++i)
        for (int j = i; j < ng; ++j) put(i, j, hd[(size_t)ng + k++]);
    k = 0;
    for (int i = 0; i < o.nsp; ++i)
        for (int j = i; j < o.nsp; ++j) put(i, j, hs[k++]);
    k = 0;
    for (int i = 0; i < o.ntp; ++i)
        for (int j = i; j < o.ntp; ++j) put(o.nsp + i, o.nsp + j, ht[k++]);
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_trial_scores_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, int ng) {
    GP_API_BEGIN(c)
    FisherOut o;
    return fisher_impl(c, hp, ng, true, false, o);
    GP_API_END(c)
}

extern "C" int gpcsd_trial_scores(gpcsd_ctx *c, const gpcsd_hparams *hp, double *scores, int ng) {
    GP_API_BEGIN(c)
    GP_REQUIRE(scores != nullptr, -3, "trial_scores: null output");
    FisherOut o;
    const int rc = fisher_impl(c, hp, ng, true, false, o);
    if (rc != 0) return rc;
    download_outputs(c, {{scores, "trial_scores", (size_t)c->ntrials * ng}});
    return 0;
    GP_API_END(c)
}
