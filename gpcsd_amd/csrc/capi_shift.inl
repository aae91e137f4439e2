// Part of capi.hip (included there: one translation unit) -- the trial-shift objective and its analytic gradient (shift.hip): a plan
// uploads the decomposition, the trials, the component means and the time grid once; an evaluation sends B (trial, tau) points and
// brings back B objective values and, if asked for, B x nseg gradient entries.

static_assert(gpcsd::SHIFT_MAX_NSEG == GPCSD_MAX_SHIFT_NSEG, "the gradient kernel's register array and the public limit");

// (checked before anything is read or launched)
static void shift_check(const char *who, int nx, int nt, int ntrials, int nseg, long B) {
    const long BT = B * nt;
    GP_REQUIRE(nseg <= GPCSD_MAX_SHIFT_NSEG && BT < GPCSD_MAX_GEMM_LD_KMAJOR && nx <= 65535 && nt < (1 << 22) && (long)nx * B < (1L << 31) &&
                   B * nseg * nt < (1L << 31) && (long)nseg * nx * nt < (1L << 31) && (long)ntrials * nt < (1L << 31),
               GPCSD_ERR_CAPACITY, "%s: nseg = %d exceeds GPCSD_MAX_SHIFT_NSEG = %d, or B * nt = %ld the capacity of one operand row (%ld doubles; "
               "GPCSD_MAX_GEMM_LD_KMAJOR), or nx = %d, nt = %d, nx * B, B * nseg * nt, nseg * nx * nt or ntrials * nt an index range", who, nseg,
               GPCSD_MAX_SHIFT_NSEG, BT, (long)GPCSD_MAX_GEMM_LD_KMAJOR, nx, nt);
}

extern "C" int gpcsd_shift_plan(gpcsd_ctx *c, const double *Qs, int nx, const double *Qt, int nt, const double *Dvec, const double *lfp,
                                int ntrials, const double *mu, int nseg, const double *t) {
    GP_API_BEGIN(c)
    GP_REQUIRE(Qs && Qt && Dvec && lfp && mu && t && nx > 0 && nt > 1 && ntrials > 0 && nseg > 0, -3, "shift_plan: bad arguments");
    for (int k = 0; k < nt; ++k)
        GP_REQUIRE(std::isfinite(t[k]) && (k == 0 || t[k] > t[k - 1]), -3, "shift_plan: t must be finite and strictly increasing (t[%d])", k);
    shift_check("shift_plan", nx, nt, ntrials, nseg, 1);
    hipStream_t s = c->stream;
    c->shift_shape[0] = 0;                                  // (until every table is in place)
    c->upload<double>("shift_Qs", Qs, (size_t)nx * nx);
    c->upload<double>("shift_Qt", Qt, (size_t)nt * nt);
    c->upload<double>("shift_D", Dvec, (size_t)nx * nt);
    const double *dt = c->upload<double>("shift_t", t, (size_t)nt);
    // the two work buffers of an evaluation stage the host layouts: (x, t, trial) -> (x, trial, t), (x, t, c) -> (x, c, t)
    const double *raw = c->upload<double>("shift_w0", lfp, (size_t)nx * nt * ntrials);
    k_swap_last2(c, raw, c->buf<double>("shift_lfp", (size_t)nx * nt * ntrials), nx, nt, ntrials, s);
    const double *mraw = c->upload<double>("shift_w1", mu, (size_t)nx * nt * (nseg + 1));
    double *dmu = c->buf<double>("shift_mu", (size_t)nx * nt * (nseg + 1));
    k_swap_last2(c, mraw, dmu, nx, nt, nseg + 1, s);
    k_shift_slopes(c, dmu, dt, nx, nt, nseg, c->buf<double>("shift_slope", (size_t)nseg * nx * (nt - 1)), s);
    c->sync();
    c->shift_shape[0] = nx; c->shift_shape[1] = nt; c->shift_shape[2] = ntrials; c->shift_shape[3] = nseg;
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_shift_eval(gpcsd_ctx *c, const int *trial_idx, const double *tau, int B, double mutau, double sigtau, double *f_out,
                                double *g_out) {
    GP_API_BEGIN(c)
    GP_REQUIRE(trial_idx && tau && f_out && B > 0, -3, "shift_eval: bad arguments");
    GP_REQUIRE(c->shift_shape[0] > 0, -2, "shift_eval: no plan (gpcsd_shift_plan)");
    const int nx = c->shift_shape[0], nt = c->shift_shape[1], ntrials = c->shift_shape[2], nseg = c->shift_shape[3];
    GP_REQUIRE(sigtau > 0.0 && std::isfinite(sigtau) && std::isfinite(mutau), -3, "shift_eval: sigtau must be positive and finite, mutau finite");
    for (int b = 0; b < B; ++b) {
        GP_REQUIRE(trial_idx[b] >= 0 && trial_idx[b] < ntrials, -3, "shift_eval: trial index %d of point %d is outside [0, %d)", trial_idx[b], b, ntrials);
        for (int i = 0; i < nseg; ++i)
            GP_REQUIRE(std::isfinite(tau[(size_t)b * nseg + i]), -3, "shift_eval: tau[%d][%d] is not finite", b, i);
    }
    shift_check("shift_eval", nx, nt, ntrials, nseg, B);
    hipStream_t s = c->stream;
    const long BT = (long)B * nt;
    const size_t nfield = (size_t)nx * BT;
    ShiftDesc d;
    d.nx = nx; d.nt = nt; d.ntrials = ntrials; d.nseg = nseg; d.B = B;
    d.mutau = mutau; d.sigtau = sigtau;
    d.t = c->buf<double>("shift_t", nt);
    d.mu = c->buf<double>("shift_mu", (size_t)nx * nt * (nseg + 1));
    d.slope = c->buf<double>("shift_slope", (size_t)nseg * nx * (nt - 1));
    d.lfp = c->buf<double>("shift_lfp", (size_t)nx * nt * ntrials);
    d.D = c->buf<double>("shift_D", (size_t)nx * nt);
    const double *dQs = c->buf<double>("shift_Qs", (size_t)nx * nx), *dQt = c->buf<double>("shift_Qt", (size_t)nt * nt);
    d.trial = c->upload<int>("shift_trial", trial_idx, (size_t)B);
    d.tau = c->upload<double>("shift_tau", tau, (size_t)B * nseg);
    d.lo = c->buf<int>("shift_lo", (size_t)B * nseg * nt);
    d.dt = c->buf<double>("shift_dt", (size_t)B * nseg * nt);
    double *w0 = c->buf<double>("shift_w0", nfield), *w1 = c->buf<double>("shift_w1", nfield);     // each field overwrites a dead one
    double *df = c->buf<double>("shift_f", B);
    double *part = c->buf<double>("shift_part", (size_t)B * shift_slabs(nx) * nseg);       // per-slab partial sums of f, then of g
    k_shift_locate(c, d, s);
    k_shift_resid(c, d, w0, s);                             // w0 = R
    GemmDesc g1;                                            // w1 = W = Qs^T R
    g1.M = nx; g1.N = (int)BT; g1.K = nx;
    g1.A = dQs; g1.lda = nx; g1.transA = true; g1.B = w0; g1.ldb = BT; g1.C = w1; g1.ldc = BT;
    g1.prof_name = "gemm_shift_spatial";
    gemm_f64(c, g1, s);
    GemmDesc g2;                                            // w0 = alpha[(x,b)][i] = sum_t W[(x,b)][t] Qt[t][i]
    g2.M = nx * B; g2.N = nt; g2.K = nt;
    g2.A = w1; g2.lda = nt; g2.B = dQt; g2.ldb = nt; g2.C = w0; g2.ldc = nt;
    g2.prof_name = "gemm_shift_temporal";
    gemm_f64(c, g2, s);
    k_shift_quad(c, d, w0, g_out ? w1 : nullptr, part, df, s);    // w1 = beta
    c->download(f_out, df, (size_t)B * sizeof(double));
    if (g_out) {
        GemmDesc g3;                                        // w0 = G[(x,b)][k] = sum_i beta[(x,b)][i] Qt[k][i]
        g3.M = nx * B; g3.N = nt; g3.K = nt;
        g3.A = w1; g3.lda = nt; g3.B = dQt; g3.ldb = nt; g3.transB = true; g3.C = w0; g3.ldc = nt;
        g3.prof_name = "gemm_shift_temporal_back";
        gemm_f64(c, g3, s);
        GemmDesc g4;                                        // w1 = Z = Qs G
        g4.M = nx; g4.N = (int)BT; g4.K = nx;
        g4.A = dQs; g4.lda = nx; g4.B = w0; g4.ldb = BT; g4.C = w1; g4.ldc = BT;
        g4.prof_name = "gemm_shift_spatial_back";
        gemm_f64(c, g4, s);
        double *dg = c->buf<double>("shift_g", (size_t)B * nseg);
        k_shift_grad(c, d, w1, part, dg, s);
        c->download(g_out, dg, (size_t)B * nseg * sizeof(double));
    }
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}
