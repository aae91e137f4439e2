// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip are in scope) -- kernel CSD in one
// dimension with Gaussian sources (kcsd.hip): the two kernels on host arrays, and the resident chains bases -> K, K~ -> batched
// eigen-decomposition -> W = U^T V -> cross-validation table -> argmin -> estimate.

namespace {

bool kc_finite(const double *p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

struct KcsdProblem {
    const char *who;
    const double *ele; int n;            // electrodes
    const double *V; int T;              // potentials (n, T)
    const double *src; int M;            // source centres
    const double *est; int n_est;        // estimation points
    double h, varsigma;
    const double *gl_x, *gl_w; int ngl;
};

// sizes first (capacity before anything is read), then the values
void kcsd_check(const KcsdProblem &p, const double *Rs, int nR, const double *lambdas, int nlam) {
    GP_REQUIRE(p.ele && p.V && p.src && p.est && p.gl_x && p.gl_w && Rs && lambdas, -3, "%s: NULL operand", p.who);
    GP_REQUIRE(p.n >= 1 && p.T >= 1 && p.n_est >= 1 && nR >= 1 && nlam >= 1, -3, "%s: empty operand", p.who);
    GP_REQUIRE(p.M >= 1 && p.ngl >= 2, -3, "%s: M = %d sources (at least 1), ngl = %d nodes per panel (at least 2)", p.who, p.M, p.ngl);
    GP_REQUIRE(p.n <= GPCSD_MAX_EIG_N && (long)nR * nlam <= 65535 && p.T < GPCSD_MAX_GEMM_LD_KMAJOR, GPCSD_ERR_CAPACITY,
               "%s: n = %d electrodes (at most %d), nR nlam = %ld pairs (at most 65535) or T = %d columns (below %ld)", p.who, p.n,
               GPCSD_MAX_EIG_N, (long)nR * nlam, p.T, GPCSD_MAX_GEMM_LD_KMAJOR);
    GP_REQUIRE(p.M < (1 << 22) && p.n_est < (1 << 22) && (long)p.M * std::max(p.n, p.n_est) < (1L << 31), GPCSD_ERR_CAPACITY,
               "%s: M = %d sources or n_est = %d estimation points exceed one operand", p.who, p.M, p.n_est);
    GP_REQUIRE(std::isfinite(p.h) && p.h > 0.0 && std::isfinite(p.varsigma) && p.varsigma > 0.0, -3, "%s: h = %g and sigma = %g must be positive",
               p.who, p.h, p.varsigma);
    for (int r = 0; r < nR; ++r) GP_REQUIRE(std::isfinite(Rs[r]) && Rs[r] > 0.0, -3, "%s: R[%d] = %g must be positive", p.who, r, Rs[r]);
    for (int l = 0; l < nlam; ++l)
        GP_REQUIRE(std::isfinite(lambdas[l]) && lambdas[l] >= 0.0, -3, "%s: lambda[%d] = %g must not be negative", p.who, l, lambdas[l]);
    GP_REQUIRE(kc_finite(p.ele, p.n) && kc_finite(p.src, p.M) && kc_finite(p.est, p.n_est) && kc_finite(p.gl_x, p.ngl) &&
                   kc_finite(p.gl_w, p.ngl) && kc_finite(p.V, (size_t)p.n * p.T),
               -3, "%s: non-finite input", p.who);
}

struct KcsdDev {
    double *K, *Kc, *U, *s, *W;          // per R: (n, n), (n_est, n), (n, n), (n), (n, T)
};

// everything up to W = U^T V for every R, on the device
KcsdDev kcsd_front(gpcsd_ctx *c, const KcsdProblem &p, const double *Rs, int nR) {
    hipStream_t s = c->stream;
    const int n = p.n, M = p.M, ne = p.n_est, T = p.T;
    const double *dele = c->upload<double>("kcsd_ele", p.ele, n);
    const double *dsrc = c->upload<double>("kcsd_src", p.src, M);
    const double *dest = c->upload<double>("kcsd_est", p.est, ne);
    const double *dgx = c->upload<double>("kcsd_gx", p.gl_x, p.ngl);
    const double *dgw = c->upload<double>("kcsd_gw", p.gl_w, p.ngl);
    const double *dV = c->upload<double>("kcsd_V", p.V, (size_t)n * T);
    double *Bp = c->buf<double>("kcsd_bpot", (size_t)nR * M * n);
    double *Bs = c->buf<double>("kcsd_bsrc", (size_t)nR * M * ne);
    KcsdDev d;
    d.K = c->buf<double>("kcsd_K", (size_t)nR * n * n);
    d.Kc = c->buf<double>("kcsd_Kcross", (size_t)nR * ne * n);
    d.U = c->buf<double>("kcsd_U", (size_t)nR * n * n);
    d.s = c->buf<double>("kcsd_s", (size_t)nR * n);
    d.W = c->buf<double>("kcsd_W", (size_t)nR * n * T);
    double *Kwork = c->buf<double>("kcsd_Kwork", (size_t)nR * n * n);
    int *st = c->buf<int>("kcsd_eig_status", (size_t)nR);
    for (int r = 0; r < nR; ++r) {
        k_kcsd_basis(c, dsrc, M, dele, n, Rs[r], p.h, p.varsigma, dgx, dgw, p.ngl, 0, Bp + (size_t)r * M * n, s);
        k_kcsd_basis(c, dsrc, M, dest, ne, Rs[r], p.h, p.varsigma, dgx, dgw, p.ngl, 1, Bs + (size_t)r * M * ne, s);
    }
    {
        GemmDesc g;                         // K = B_pot^T B_pot / M
        g.M = n; g.N = n; g.K = M;
        g.A = Bp; g.transA = true; g.lda = n; g.sA = (long)M * n;
        g.B = Bp; g.ldb = n; g.sB = (long)M * n;
        g.C = d.K; g.ldc = n; g.sC = (long)n * n;
        g.batch = nR; g.alpha = 1.0 / M;
        g.prof_name = "kcsd_gram";
        gemm_f64(c, g, s);
        g.M = ne;                           // K~ = B_src^T B_pot / M
        g.A = Bs; g.lda = ne; g.sA = (long)M * ne;
        g.C = d.Kc; g.sC = (long)ne * n;
        gemm_f64(c, g, s);
    }
    GP_HIP(hipMemcpyAsync(Kwork, d.K, (size_t)nR * n * n * sizeof(double), hipMemcpyDeviceToDevice, s));
    GP_HIP(hipMemsetAsync(st, 0, (size_t)nR * sizeof(int), s));
    {
        EighCall e;
        e.side[0] = {Kwork, n, d.s, d.U, nullptr, nR};
        e.status = st; e.status_stride = 1;
        eigh_pair_device(c, e, s);
    }
    {
        GemmDesc g;                         // W = U^T V
        g.M = n; g.N = T; g.K = n;
        g.A = d.U; g.transA = true; g.lda = n; g.sA = (long)n * n;
        g.B = dV; g.ldb = T; g.sB = 0;
        g.C = d.W; g.ldc = T; g.sC = (long)n * T;
        g.batch = nR;
        g.prof_name = "kcsd_project";
        gemm_f64(c, g, s);
    }
    std::vector<int> hst((size_t)nR);
    c->download(hst.data(), st, (size_t)nR * sizeof(int));
    c->sync();
    for (int r = 0; r < nR; ++r)
        GP_REQUIRE(hst[r] == 0, hst[r] > 0 ? hst[r] : 1, "%s: the eigen-decomposition of K for R[%d] = %g failed (status %d)", p.who, r, Rs[r],
                   hst[r]);
    return d;
}

// C^ = K~ U diag(1 / (s + lambda)) W and the potentials K (K + lambda)^-1 V = U diag(s / (s + lambda)) W for the R at index r
void kcsd_back(gpcsd_ctx *c, const KcsdProblem &p, const KcsdDev &d, int r, double R, double lambda, double *csd, double *pot, double *k_pot,
               double *k_cross) {
    hipStream_t s = c->stream;
    const int n = p.n, ne = p.n_est, T = p.T;
    double *dd = c->buf<double>("kcsd_d", (size_t)2 * n), *sd = dd + n;
    int *st = c->buf<int>("kcsd_est_status", 1);
    k_kcsd_scale(c, d.s + (size_t)r * n, n, lambda, dd, sd, st, s);
    int hst = 0;
    c->download(&hst, st, sizeof(int));
    c->sync();
    GP_REQUIRE(hst == 0, 1, "%s: K + lambda I is numerically singular for R = %g, lambda = %g (s_min + lambda < n 2^-52 s_max)", p.who, R, lambda);
    double *beta = c->buf<double>("kcsd_beta", (size_t)n * T);
    double *Wd = c->buf<double>("kcsd_Wd", (size_t)n * T);
    GemmDesc g;
    g.M = n; g.N = T; g.K = n;
    g.A = d.U + (size_t)r * n * n; g.lda = n;
    g.B = Wd; g.ldb = T;
    g.C = beta; g.ldc = T;
    g.prof_name = "kcsd_estimate";
    if (csd) {
        k_kcsd_rowscale(c, d.W + (size_t)r * n * T, dd, n, T, Wd, s);
        gemm_f64(c, g, s);
        double *out = c->buf<double>("kcsd_csd", (size_t)ne * T);
        GemmDesc h;
        h.M = ne; h.N = T; h.K = n;
        h.A = d.Kc + (size_t)r * ne * n; h.lda = n;
        h.B = beta; h.ldb = T;
        h.C = out; h.ldc = T;
        h.prof_name = "kcsd_estimate";
        gemm_f64(c, h, s);
        c->download(csd, out, (size_t)ne * T * sizeof(double));
    }
    if (pot) {
        k_kcsd_rowscale(c, d.W + (size_t)r * n * T, sd, n, T, Wd, s);
        gemm_f64(c, g, s);
        c->download(pot, beta, (size_t)n * T * sizeof(double));
    }
    if (k_pot) c->download(k_pot, d.K + (size_t)r * n * n, (size_t)n * n * sizeof(double));
    if (k_cross) c->download(k_cross, d.Kc + (size_t)r * ne * n, (size_t)ne * n * sizeof(double));
    c->sync();
}

}  // namespace

extern "C" int gpcsd_kcsd_basis_1d(gpcsd_ctx *c, const double *src, int M, const double *pts, int npts, double R, double h, double varsigma,
                                   const double *gl_x, const double *gl_w, int ngl, int which, double *out) {
    GP_API_BEGIN(c)
    GP_REQUIRE(src && pts && gl_x && gl_w && out && npts >= 1 && (which == 0 || which == 1), -3, "kcsd_basis_1d: bad arguments");
    GP_REQUIRE(M >= 1 && ngl >= 2, -3, "kcsd_basis_1d: M = %d sources (at least 1), ngl = %d nodes per panel (at least 2)", M, ngl);
    GP_REQUIRE((long)M * npts < (1L << 31), GPCSD_ERR_CAPACITY, "kcsd_basis_1d: M npts = %ld entries (below 2^31)", (long)M * npts);
    GP_REQUIRE(std::isfinite(R) && R > 0.0 && std::isfinite(h) && h > 0.0 && std::isfinite(varsigma) && varsigma > 0.0, -3,
               "kcsd_basis_1d: R = %g, h = %g and sigma = %g must be positive", R, h, varsigma);
    GP_REQUIRE(kc_finite(src, M) && kc_finite(pts, npts) && kc_finite(gl_x, ngl) && kc_finite(gl_w, ngl), -3, "kcsd_basis_1d: non-finite input");
    const double *dsrc = c->upload<double>("kcsd_src", src, M);
    const double *dpts = c->upload<double>("kcsd_est", pts, npts);
    const double *dgx = c->upload<double>("kcsd_gx", gl_x, ngl);
    const double *dgw = c->upload<double>("kcsd_gw", gl_w, ngl);
    double *o = c->buf<double>("op_out", (size_t)M * npts);
    k_kcsd_basis(c, dsrc, M, dpts, npts, R, h, varsigma, dgx, dgw, ngl, which, o, c->stream);
    c->download(out, o, (size_t)M * npts * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_kcsd_cv(gpcsd_ctx *c, const double *U, const double *s, const double *W, int n, int T, int nR, const double *lambdas,
                             int nlam, double *err, int *status) {
    GP_API_BEGIN(c)
    GP_REQUIRE(U && s && W && lambdas && err && status && n >= 1 && T >= 1 && nR >= 1 && nlam >= 1, -3, "kcsd_cv: bad arguments");
    GP_REQUIRE(n <= GPCSD_MAX_EIG_N && (long)nR * nlam <= 65535 && T < GPCSD_MAX_GEMM_LD_KMAJOR, GPCSD_ERR_CAPACITY,
               "kcsd_cv: n = %d electrodes (at most %d), nR nlam = %ld pairs (at most 65535) or T = %d columns (below %ld)", n, GPCSD_MAX_EIG_N,
               (long)nR * nlam, T, GPCSD_MAX_GEMM_LD_KMAJOR);
    for (int l = 0; l < nlam; ++l)
        GP_REQUIRE(std::isfinite(lambdas[l]) && lambdas[l] >= 0.0, -3, "kcsd_cv: lambda[%d] = %g must not be negative", l, lambdas[l]);
    GP_REQUIRE(kc_finite(U, (size_t)nR * n * n) && kc_finite(s, (size_t)nR * n) && kc_finite(W, (size_t)nR * n * T), -3, "kcsd_cv: non-finite input");
    const double *dU = c->upload<double>("kcsd_U", U, (size_t)nR * n * n);
    const double *ds = c->upload<double>("kcsd_s", s, (size_t)nR * n);
    const double *dW = c->upload<double>("kcsd_W", W, (size_t)nR * n * T);
    const double *dl = c->upload<double>("kcsd_lam", lambdas, nlam);
    double *derr = c->buf<double>("kcsd_err", (size_t)nR * nlam);
    int *dst = c->buf<int>("kcsd_cv_status", (size_t)nR * nlam);
    k_kcsd_cv(c, dU, ds, dW, n, T, nR, dl, nlam, derr, dst, c->stream);
    c->download(err, derr, (size_t)nR * nlam * sizeof(double));
    c->download(status, dst, (size_t)nR * nlam * sizeof(int));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_kcsd_cross_validate(gpcsd_ctx *c, const double *ele, int n, const double *V, int T, const double *src, int M,
                                         const double *est, int n_est, double h, double varsigma, const double *gl_x, const double *gl_w,
                                         int ngl, const double *Rs, int nR, const double *lambdas, int nlam, double *err, int *status,
                                         int *best, double *csd, double *pot, double *k_pot, double *k_cross) {
    GP_API_BEGIN(c)
    GP_REQUIRE(err && status && best, -3, "kcsd_cross_validate: NULL output");
    const KcsdProblem p{"kcsd_cross_validate", ele, n, V, T, src, M, est, n_est, h, varsigma, gl_x, gl_w, ngl};
    kcsd_check(p, Rs, nR, lambdas, nlam);
    const KcsdDev d = kcsd_front(c, p, Rs, nR);
    const double *dl = c->upload<double>("kcsd_lam", lambdas, nlam);
    double *derr = c->buf<double>("kcsd_err", (size_t)nR * nlam);
    int *dst = c->buf<int>("kcsd_cv_status", (size_t)nR * nlam);
    k_kcsd_cv(c, d.U, d.s, d.W, n, T, nR, dl, nlam, derr, dst, c->stream);
    c->download(err, derr, (size_t)nR * nlam * sizeof(double));
    c->download(status, dst, (size_t)nR * nlam * sizeof(int));
    c->sync();
    // argmin: the smallest R index wins a tie, then the smallest lambda index; a singular pair is never selected
    int bi = -1;
    for (int i = 0; i < nR * nlam; ++i)
        if (status[i] == 0 && std::isfinite(err[i]) && (bi < 0 || err[i] < err[bi])) bi = i;
    best[0] = bi < 0 ? -1 : bi / nlam;
    best[1] = bi < 0 ? -1 : bi % nlam;
    GP_REQUIRE(bi >= 0, 1, "kcsd_cross_validate: K + lambda I is numerically singular for every pair (R, lambda)");
    if (csd || pot || k_pot || k_cross) kcsd_back(c, p, d, best[0], Rs[best[0]], lambdas[best[1]], csd, pot, k_pot, k_cross);
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_kcsd_estimate(gpcsd_ctx *c, const double *ele, int n, const double *V, int T, const double *src, int M, const double *est,
                                   int n_est, double h, double varsigma, const double *gl_x, const double *gl_w, int ngl, double R,
                                   double lambda, double *csd, double *pot, double *k_pot, double *k_cross) {
    GP_API_BEGIN(c)
    const KcsdProblem p{"kcsd_estimate", ele, n, V, T, src, M, est, n_est, h, varsigma, gl_x, gl_w, ngl};
    kcsd_check(p, &R, 1, &lambda, 1);
    const KcsdDev d = kcsd_front(c, p, &R, 1);
    kcsd_back(c, p, d, 0, R, lambda, csd, pot, k_pot, k_cross);
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}
