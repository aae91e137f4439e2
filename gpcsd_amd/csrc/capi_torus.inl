// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip are in scope) -- the
// phase-difference torus graph (torus.hip): score-matching fit of all bootstrap replicates, inference for replicate 0, and the
// transposed triangular solve it needs (chol.hip).

extern "C" int gpcsd_trsm_lower_trans(gpcsd_ctx *c, const double *L, int n, const double *B, int nrhs, double *X) {
    GP_API_BEGIN(c)
    GP_REQUIRE(L && B && X && n > 0 && nrhs > 0, -3, "trsm_lower_trans: bad arguments");
    GP_REQUIRE(nrhs < GPCSD_MAX_GEMM_LD_KMAJOR && n < (1 << 22), GPCSD_ERR_CAPACITY, "trsm_lower_trans: n = %d or nrhs = %d exceeds one operand row", n, nrhs);
    double *dL = c->upload<double>("op_in0", L, (size_t)n * n);
    double *dB = c->upload<double>("op_in1", B, (size_t)n * nrhs);
    trsm_lower_trans_device(c, dL, n, dB, nrhs, c->stream);
    c->download(X, dB, (size_t)n * nrhs * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

// bytes of Gamma and node blocks a chunk of replicates may hold (GPCSD_TORUS_CHUNK_MB, default 256; read per call)
static size_t tg_chunk_budget() {
    const char *e = getenv("GPCSD_TORUS_CHUNK_MB");
    const long mb = e ? atol(e) : 256;
    return (size_t)std::max(mb, 0L) << 20;
}

// (checked before anything is read)
static void tg_check(const char *who, int d, int N, const double *weights, int B) {
    GP_REQUIRE(B >= 1 && (weights || B == 1), -3, "%s: B = %d replicates need B rows of weights", who, B);
    GP_REQUIRE(d >= 2 && N >= 1, -22, "%s: d = %d nodes (at least 2) and N = %d trials (at least 1)", who, d, N);
    GP_REQUIRE(d <= TG_MAX_NODES && N < GPCSD_MAX_GEMM_LD_KMAJOR && N < (1 << 22), GPCSD_ERR_CAPACITY,
               "%s: d = %d exceeds %d nodes (a dense system of d (d - 1) parameters per replicate), or N = %d one operand row", who, d,
               TG_MAX_NODES, N);
}

// The whole fit on phasors that are on the device: node a's N trials at ure / uim + off[a].
static void tg_run(gpcsd_ctx *c, const char *who, const double *ure, const double *uim, const std::vector<long> &off, int d, int N,
                   const double *weights, int B, double *phi, int *status, double *chi2, double *gamma0, double *h0) {
    const int P = d * (d - 1) / 2, m = 2 * P, nv = 2 * d - 1;
    hipStream_t s = c->stream;
    std::vector<double> W((size_t)B, (double)N);
    if (weights) {
        for (int b = 0; b < B; ++b) {
            double sum = 0.0;
            for (int n = 0; n < N; ++n) {
                const double w = weights[(size_t)b * N + n];
                GP_REQUIRE(std::isfinite(w) && w >= 0.0, -22, "%s: weight [%d][%d] = %g is negative or not finite", who, b, n, w);
                sum += w;
            }
            GP_REQUIRE(sum > 0.0 && std::isfinite(sum), -22, "%s: the weights of replicate %d sum to %g", who, b, sum);
            W[b] = sum;
        }
    }
    std::vector<int> pij((size_t)2 * P);
    for (int i = 0, p = 0; i < d; ++i)
        for (int j = i + 1; j < d; ++j, ++p) { pij[p] = i; pij[P + p] = j; }
    TgDesc t;
    t.ure = ure; t.uim = uim; t.d = d; t.N = N;
    t.off = c->upload<long>("tg_off", off.data(), (size_t)d);
    t.pi = c->upload<int>("tg_pairs", pij.data(), (size_t)2 * P);
    t.pj = t.pi + P;
    const double *dw = weights ? c->upload<double>("tg_w", weights, (size_t)B * N) : nullptr;
    const double *dW = c->upload<double>("tg_W", W.data(), (size_t)B);
    double *dphi = c->buf<double>("tg_phi", (size_t)B * m);
    int *dst = c->buf<int>("tg_status", (size_t)B);
    GP_HIP(hipMemsetAsync(dst, 0, (size_t)B * sizeof(int), s));
    // replicates in chunks whose Gammas and node blocks fit the budget: nothing but weights, phi and status grows with B
    const size_t per_rep = ((size_t)m * m + (size_t)d * nv * nv + (size_t)m) * sizeof(double);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, std::min<size_t>(tg_chunk_budget() / per_rep, 16384)));
    double *G = c->buf<double>("tg_G", (size_t)chunk * d * nv * nv);
    double *Gamma = c->buf<double>("tg_gamma", (size_t)chunk * m * m);
    double *dg = c->buf<double>("tg_diag", (size_t)chunk * m);
    double *dchi = chi2 ? c->buf<double>("tg_chi2", (size_t)P) : nullptr;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nrep = std::min(chunk, B - b0);
        k_tg_node_gram(c, t, dw ? dw + (size_t)b0 * N : nullptr, dW + b0, nrep, G, s);
        k_tg_assemble(c, t, G, nrep, Gamma, dphi + (size_t)b0 * m, s);          // H lands where phi is solved in place
        k_tg_diag_save(c, Gamma, m, nrep, dg, s);
        if (b0 == 0) {
            if (gamma0) c->download(gamma0, Gamma, (size_t)m * m * sizeof(double));
            if (h0) c->download(h0, dphi, (size_t)m * sizeof(double));
        }
        for (int r = 0; r < nrep; ++r) {
            double *L = Gamma + (size_t)r * m * m, *ph = dphi + (size_t)(b0 + r) * m;
            {
                ProfScope ps(c, "tg_factor", (double)m * m * m / 3.0, s);
                potrf_device(c, L, m, dst + b0 + r, s);
                k_tg_pivot_check(c, L, dg + (size_t)r * m, m, dst + b0 + r, s);
            }
            trsm_lower_device(c, L, m, ph, 1, s);
            trsm_lower_trans_device(c, L, m, ph, 1, s);
            if (b0 + r == 0 && chi2) {
                // inference for replicate 0: Z = Gamma^-1 R by the factor that is still in place, then the row-pair products
                ProfScope ps(c, "tg_inference", 4.0 * (double)m * m * N, s);
                double *R = c->buf<double>("tg_R", (size_t)m * N);
                double *g = c->buf<double>("tg_g", (size_t)d * N);
                k_tg_residuals(c, t, ph, g, R, s);
                trsm_lower_device(c, L, m, R, N, s);
                trsm_lower_trans_device(c, L, m, R, N, s);
                k_tg_chi2(c, R, dw, ph, P, N, W[0], dchi, s);
            }
        }
    }
    c->download(phi, dphi, (size_t)B * m * sizeof(double));
    c->download(status, dst, (size_t)B * sizeof(int));
    if (chi2) c->download(chi2, dchi, (size_t)P * sizeof(double));
    c->sync();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int b = 0; b < B; ++b)
        if (status[b] != 0) std::fill(phi + (size_t)b * m, phi + (size_t)(b + 1) * m, nan);
    if (chi2 && status[0] != 0) std::fill(chi2, chi2 + P, nan);
    if (c->prof_mode == 1) c->prof_collect();
}

extern "C" int gpcsd_torus_graph(gpcsd_ctx *c, const double *u_re, const double *u_im, int d, int N, const double *weights, int B,
                                 double *phi, int *status, double *chi2, double *gamma0, double *h0) {
    GP_API_BEGIN(c)
    GP_REQUIRE(u_re && u_im && phi && status, -3, "torus_graph: bad arguments");
    tg_check("torus_graph", d, N, weights, B);
    std::vector<long> off((size_t)d);
    for (int a = 0; a < d; ++a) off[a] = (long)a * N;
    const double *dre = c->upload<double>("tg_u_re", u_re, (size_t)d * N);
    const double *dim_ = c->upload<double>("tg_u_im", u_im, (size_t)d * N);
    tg_run(c, "torus_graph", dre, dim_, off, d, N, weights, B, phi, status, chi2, gamma0, h0);
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_torus_graph_resident(gpcsd_ctx *c, const int *sites, int d, int j, int nz, int nsel, int R, const double *weights,
                                          int B, double *phi, int *status, double *chi2) {
    GP_API_BEGIN(c)
    GP_REQUIRE(sites && phi && status && nz > 0 && nsel > 0 && j >= 0 && j < nsel, -3, "torus_graph_resident: bad arguments");
    tg_check("torus_graph_resident", d, R, weights, B);
    GP_REQUIRE(c->phasor_shape[0] == nz && c->phasor_shape[1] == nsel && c->phasor_shape[2] == (long)R, -4,
               "torus_graph_resident: no gpcsd_analytic_resident call has left unit phasors of shape (%d, %d, %d) (found (%ld, %ld, %ld))",
               nz, nsel, R, c->phasor_shape[0], c->phasor_shape[1], c->phasor_shape[2]);
    std::vector<long> off((size_t)d);
    for (int a = 0; a < d; ++a) {
        GP_REQUIRE(sites[a] >= 0 && sites[a] < nz, -3, "torus_graph_resident: site %d = %d is not in [0, %d)", a, sites[a], nz);
        off[a] = ((long)sites[a] * nsel + j) * R;
    }
    tg_run(c, "torus_graph_resident", static_cast<const double *>(c->bufs["phasor_re"].p), static_cast<const double *>(c->bufs["phasor_im"].p),
           off, d, R, weights, B, phi, status, chi2, nullptr, nullptr);
    return 0;
    GP_API_END(c)
}
