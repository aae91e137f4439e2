// Part of capi.hip (included there, behind capi_posterior.inl: loo_request, loo_front and download_outputs are in scope) --
// leave-electrodes-out cross-validation in closed form (gpcsd_cv_electrodes, gpcsd_efold_contract; no reference counterpart).
//
// The model is gpcsd_loo's: K = (Qs (x) Qt) diag(D) (Qs (x) Qt)^T from front_half(c, hp, hp->jitter).  For a held-out electrode set F
// (K^-1)_FF = Qt blockdiag_j(G_j) Qt^T, one f x f block per temporal eigen-index j, so all folds together are
//   1. the front of gpcsd_loo up to V = K^-1 y in the temporal eigen-basis                                        (loo_front)
//   2. every G_j of every fold as ONE product, Gp[(F, a >= b)][j] = sum_x' (Qs[a][x'] Qs[b][x']) Dinv[x'][j]       (gemm_var, pair form)
//   3. factor and solve per (fold, j), the sums over j in a fixed order                                           (efold.hip)
//   4. cv_var[a][t] = sum_j pdiag[a][j] Qt[t][j]^2                                                                (gemm_var, as loo's c)
//   5. cv_mean = y - E Qt^T: gemm_loo with V := E and a unit cdiag, whose epilogue writes y - e in the data's layout (x, t, r);
//      division by 1.0 is exact; its two row sums go to scratch (cv_sse comes from step 3 whether the mean is wanted or not)
// Rows of electrodes in no fold: pdiag, E and sse are filled with NaN first, which the products of steps 4 and 5 carry into cv_var
// and cv_mean (a row of the output reads its own row of the operand only).

// The folds of a call, checked and expanded on the host: what the device needs beside the CSR arrays themselves
struct CvFolds {
    std::vector<int> row0, mem_fold, pa, pb;
    int nmem = 0, nrows = 0;
};
// rc -3 / GPCSD_ERR_CAPACITY before anything is read from the data or launched (the fold arrays themselves are read here)
static void cv_check_folds(const char *who, const int *fold_ptr, const int *fold_idx, int nfolds, int nx, CvFolds &F) {
    GP_REQUIRE(fold_ptr && fold_idx && nfolds > 0 && nx > 0, -3, "%s: bad fold arguments", who);
    GP_REQUIRE(nfolds <= nx && nfolds < 65536 && fold_ptr[0] == 0, -3, "%s: %d folds over %d electrodes (or fold_ptr[0] != 0)", who, nfolds, nx);
    std::vector<char> seen((size_t)nx, 0);
    bool oversize = false;
    for (int i = 0; i < nfolds; ++i) {
        const int f = fold_ptr[i + 1] - fold_ptr[i];
        GP_REQUIRE(f >= 1 && f <= nx, -3, "%s: fold %d holds %d electrodes (1 .. nx)", who, i, f);
        if (f > GPCSD_CV_MAX_FOLD) oversize = true;
        for (int m = fold_ptr[i]; m < fold_ptr[i + 1]; ++m) {
            const int a = fold_idx[m];
            GP_REQUIRE(a >= 0 && a < nx, -3, "%s: electrode %d of fold %d is out of range [0, %d)", who, a, i, nx);
            GP_REQUIRE(!seen[a], -3, "%s: electrode %d is held out twice (fold %d)", who, a, i);
            seen[a] = 1;
        }
    }
    GP_REQUIRE(!oversize, GPCSD_ERR_CAPACITY, "%s: a fold holds more than %d electrodes (GPCSD_CV_MAX_FOLD; gpcsd_predict_masked "
               "holds out larger sets)", who, GPCSD_CV_MAX_FOLD);
    F.nmem = fold_ptr[nfolds];
    F.row0.resize(nfolds);
    F.mem_fold.resize(F.nmem);
    for (int i = 0; i < nfolds; ++i) {
        const int m0 = fold_ptr[i], f = fold_ptr[i + 1] - m0;
        F.row0[i] = (int)F.pa.size();
        for (int a = 0; a < f; ++a) {
            F.mem_fold[m0 + a] = i;
            for (int b = 0; b <= a; ++b) {            // packed lower triangle: row a (a + 1) / 2 + b
                F.pa.push_back(fold_idx[m0 + a]);
                F.pb.push_back(fold_idx[m0 + b]);
            }
        }
    }
    F.nrows = (int)F.pa.size();
}

// Steps 2 and 3 on device operands: A (nx, K), W (K, nt), V (nx, R, nt) -> E (nx, R, nt) or null, pdiag (nx, nt), lpd (nfolds, R),
// sse (nx, R), status (nfolds); rows of electrodes in no fold NaN
static void cv_blocks(gpcsd_ctx *c, const double *A, const double *W, const double *V, int nx, int K, int nt, int R, const int *fold_ptr,
                      const int *fold_idx, int nfolds, const CvFolds &F, double *E, double *pdiag, double *lpd, double *sse, int *status) {
    hipStream_t s = c->stream;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    EfoldDesc d;
    d.fold_ptr = c->upload<int>("cv_fold_ptr", fold_ptr, (size_t)nfolds + 1);
    d.fold_idx = c->upload<int>("cv_fold_idx", fold_idx, (size_t)F.nmem);
    d.row0 = c->upload<int>("cv_row0", F.row0.data(), (size_t)nfolds);
    d.mem_fold = c->upload<int>("cv_mem_fold", F.mem_fold.data(), (size_t)F.nmem);
    const int *pa = c->upload<int>("cv_pair_a", F.pa.data(), (size_t)F.nrows);
    const int *pb = c->upload<int>("cv_pair_b", F.pb.data(), (size_t)F.nrows);
    double *Gp = c->buf<double>("cv_Gp", (size_t)F.nrows * nt);
    k_fill(c, pdiag, (long)nx * nt, nan, s);
    k_fill(c, sse, (long)nx * R, nan, s);
    if (E) k_fill(c, E, (long)nx * R * nt, nan, s);
    VarDesc v1;                           // Gp[(F, a >= b)][j] = sum_x' (A[a][x'] A[b][x']) W[x'][j]
    v1.A = A; v1.lda = K; v1.B = W; v1.ldb = nt;
    v1.nrow = F.nrows; v1.ncol = nt; v1.K = K; v1.list = Gp;
    v1.pair_a = pa; v1.pair_b = pb; v1.a_rows = nx;
    v1.prof_name = "gemm_var_Gp";
    gemm_var(c, v1, s);
    d.Gp = Gp; d.V = V;
    d.nfolds = nfolds; d.nt = nt; d.R = R;
    d.E = E; d.pdiag = pdiag; d.lpd = lpd; d.sse = sse; d.status = status;
    d.partials = c->buf<double>("cv_partials", (size_t)efold_partials(d, F.nmem));
    efold_solve(c, d, fold_ptr, s);
}

static int cv_impl(gpcsd_ctx *c, const gpcsd_hparams *hp, const int *fold_ptr, const int *fold_idx, int nfolds, bool want_mean) {
    GP_REQUIRE(hp != nullptr, -3, "null hparams");
    GP_REQUIRE(fold_ptr && fold_idx && nfolds > 0, -3, "cv_electrodes: bad fold arguments");
    GP_REQUIRE(c->d_lfp != nullptr, -4, "lfp not set (call gpcsd_set_lfp)");
    const int nx = c->nx, nt = c->nt, R = c->ntrials;
    CvFolds F;
    cv_check_folds("cv_electrodes", fold_ptr, fold_idx, nfolds, nx, F);
    loo_request(c, hp, "cv_electrodes");
    const long RT = (long)R * nt, nrow = (long)nx * R;
    LooFront f;
    if (int rc = loo_front(c, hp, f)) return rc;
    hipStream_t s = c->stream;
    double *pdiag = c->buf<double>("cv_pdiag", (size_t)nx * nt);
    double *var = c->buf<double>("cv_var", (size_t)nx * nt);
    double *lpd = c->buf<double>("cv_lpd", (size_t)nfolds * R), *sse = c->buf<double>("cv_sse", (size_t)nrow);
    int *status = c->buf<int>("cv_status", (size_t)nfolds + 1);        // (an even count: read back as doubles)
    double *E = want_mean ? c->buf<double>("cv_E", (size_t)nx * RT) : nullptr;
    cv_blocks(c, f.e.Qs, f.e.Dinv, f.V, nx, nx, nt, R, fold_ptr, fold_idx, nfolds, F, E, pdiag, lpd, sse, status);
    double *QtT = c->buf<double>("loo_QtT", (size_t)nt * nt);
    k_swap_last2(c, f.e.Qt, QtT, 1, nt, nt, s);    // the eigen-index leading: the squared operand's layout
    VarDesc v2;                           // cv_var[a][t] = sum_j pdiag[a][j] Qt[t][j]^2
    v2.A = pdiag; v2.lda = nt; v2.B = QtT; v2.ldb = nt;
    v2.nrow = nx; v2.ncol = nt; v2.K = nt; v2.list = var;
    v2.prof_name = "gemm_var_cv";
    gemm_var(c, v2, s);
    if (want_mean) {
        double *ones = c->buf<double>("cv_ones", (size_t)nx * nt);
        double *junk = c->buf<double>("cv_junk", (size_t)2 * nrow);
        k_fill(c, ones, (long)nx * nt, 1.0, s);
        LooDesc l;                        // mean[x][t][r] = y - sum_j E[(x,r)][j] Qt[t][j]
        l.V = E; l.ldv = nt; l.Qt = f.e.Qt; l.ldq = nt; l.c = ones; l.y = c->d_lfp;
        l.K = nt; l.nt = nt; l.R = R; l.nrow = nrow;
        l.mean = c->buf<double>("cv_mean", (size_t)nx * RT); l.lpd = junk; l.sse = junk + nrow;
        gemm_loo(c, l, s);
    }
    return finish_call(c, f.e, nullptr, 0);
}

extern "C" int gpcsd_cv_electrodes_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, const int *fold_ptr, const int *fold_idx, int nfolds,
                                            int want_mean) {
    GP_API_BEGIN(c)
    return cv_impl(c, hp, fold_ptr, fold_idx, nfolds, want_mean != 0);
    GP_API_END(c)
}

extern "C" int gpcsd_cv_electrodes(gpcsd_ctx *c, const gpcsd_hparams *hp, const int *fold_ptr, const int *fold_idx, int nfolds,
                                   double *var, double *mean, double *lpd, double *sse, int *status) {
    GP_API_BEGIN(c)
    const int rc = cv_impl(c, hp, fold_ptr, fold_idx, nfolds, mean != nullptr);
    if (rc < 0) return rc;
    const size_t nxt = (size_t)c->nx * c->nt, nrow = (size_t)c->nx * c->ntrials;
    if (status) c->download(status, c->bufs["cv_status"].p, (size_t)nfolds * sizeof(int));
    download_outputs(c, {{var, "cv_var", nxt}, {mean, "cv_mean", nxt * c->ntrials}, {lpd, "cv_lpd", (size_t)nfolds * c->ntrials},
                         {sse, "cv_sse", nrow}});
    return rc;
    GP_API_END(c)
}

extern "C" int gpcsd_efold_contract(gpcsd_ctx *c, const double *A, const double *W, const double *V, int nx, int K, int nt, int R,
                                    const int *fold_ptr, const int *fold_idx, int nfolds, double *E, double *pdiag, double *lpd,
                                    double *sse, int *status) {
    GP_API_BEGIN(c)
    GP_REQUIRE(A && W && V && pdiag && lpd && sse && status && nx > 0 && K > 0 && nt > 0 && R > 0, -3, "efold_contract: bad arguments");
    CvFolds F;
    cv_check_folds("efold_contract", fold_ptr, fold_idx, nfolds, nx, F);
    // (checked before anything is read)
    GP_REQUIRE((long)R * nt < GPCSD_MAX_GEMM_LD_KMAJOR && (long)nx * R < (1L << 31) && K < (1 << 22) && (long)nx * K < (1L << 28),
               GPCSD_ERR_CAPACITY, "efold_contract: R * nt = %ld (or nx * R = %ld, or nx * K = %ld) exceeds the capacity of one operand",
               (long)R * nt, (long)nx * R, (long)nx * K);
    const size_t nrow = (size_t)nx * R, nxt = (size_t)nx * nt;
    const double *dA = c->upload<double>("op_in0", A, (size_t)nx * K);
    const double *dW = c->upload<double>("op_in1", W, (size_t)K * nt);
    const double *dV = c->upload<double>("op_in2", V, nrow * nt);
    double *dO = c->buf<double>("op_out", nxt + (size_t)nfolds * R + nrow + (E ? nrow * nt : 0));
    double *dpd = dO, *dlpd = dO + nxt, *dsse = dlpd + (size_t)nfolds * R, *dE = E ? dsse + nrow : nullptr;
    int *dst = c->buf<int>("cv_status", (size_t)nfolds + 1);        // (an even count: read back as doubles)
    cv_blocks(c, dA, dW, dV, nx, K, nt, R, fold_ptr, fold_idx, nfolds, F, dE, dpd, dlpd, dsse, dst);
    c->download(pdiag, dpd, nxt * sizeof(double));
    c->download(lpd, dlpd, (size_t)nfolds * R * sizeof(double));
    c->download(sse, dsse, nrow * sizeof(double));
    c->download(status, dst, (size_t)nfolds * sizeof(int));
    if (E) c->download(E, dE, nrow * nt * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}
