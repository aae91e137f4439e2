// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip, capi_fused.inl and capi_posterior.inl are in scope) --
// missing samples: posterior means and the log-likelihood under a mask of observed samples (gpcsd_predict_masked,
// gpcsd_loglik_masked) and the assembly of the Schur complement alone (gpcsd_masked_gram).  No reference counterpart.
//
// A = K of a full trial = (Qs (x) Qt) diag(D) (Qs (x) Qt)^T, M the m missing samples of a trial, O the observed ones, y~ the trial
// with zeros on M, c = (A^-1 y~)_M, G = (A^-1)_MM (SPD).  Exactly:
//   A_OO^-1 y_O        = [A^-1 (y~ + E_M u)]_O,  u = -G^-1 c        (the imputed values make the weights vanish on M)
//   y_O^T A_OO^-1 y_O  = y~^T A^-1 y~ - c^T G^-1 c
//   log det A_OO       = log det A + log det G
// so the masked problem is the full-grid solve, one dense SPD matrix per distinct mask and its Cholesky factor.

// Scratch of the H_a blocks of one launch of the grouped product, in bytes: GPCSD_MASKED_SCRATCH_MB (read per call: tests force
// several chunks with it, and may give a fraction), 256 MB otherwise.
static size_t masked_scratch_budget() {
    const char *e = getenv("GPCSD_MASKED_SCRATCH_MB");
    const double mb = e ? atof(e) : 0.0;
    return (size_t)((mb > 0.0 ? mb : 256.0) * 1048576.0);
}

// G (m, m) of the samples (xs[p], ts[p]), which must be sorted by time, then electrode:
//   G[p][q] = sum_{a,b} Qs[x_p][a] Qs[x_q][a] Qt[i_p][b] Qt[i_q][b] Dinv[a][b] = sum_a Qs[x_p][a] Qs[x_q][a] H_a[j(p)][j(q)],
//   H_a = Qt_u diag(Dinv[a, :]) Qt_u^T over the nu distinct times (2 nx nt nu^2 flops: one batched launch of the GEMM core with its
//   kscale operand per chunk), then the grouped product (2 nx m^2 flops on the padded strips; masked.hip).
// The tile rows of G are processed in chunks whose H blocks fit masked_scratch_budget(); neither the chunking nor anything else
// changes the order of a sum.  Qs (nx, nx), Qt (nt, nt), Dinv (nx, nt) on the device.
static void masked_assemble(gpcsd_ctx *c, const double *Qs, const double *Qt, const double *Dinv, int nx, int nt, const std::vector<int> &xs,
                            const std::vector<int> &ts, double *G, hipStream_t s) {
    const int m = (int)xs.size();
    constexpr int SW = MASKED_STRIP, ST = MASKED_TILE_STRIPS;
    std::vector<int> tu, s_off, s_cnt, s_grp;
    for (int p = 0; p < m;) {
        int q = p;
        while (q < m && ts[q] == ts[p]) ++q;
        const int g = (int)tu.size();
        tu.push_back(ts[p]);
        for (int o = p; o < q; o += SW) {
            s_off.push_back(o);
            s_cnt.push_back(std::min(SW, q - o));
            s_grp.push_back(g);
        }
        p = q;
    }
    const int nu = (int)tu.size(), ns = (int)s_off.size();
    const int nsp = (ns + ST - 1) / ST * ST, ntile = nsp / ST;
    // one upload: xi | s_off | s_cnt | s_grp (padded with empty strips) | tu
    std::vector<int> desc((size_t)m + 3 * (size_t)nsp + nu, 0);
    std::copy(xs.begin(), xs.end(), desc.begin());
    std::copy(s_off.begin(), s_off.end(), desc.begin() + m);
    std::copy(s_cnt.begin(), s_cnt.end(), desc.begin() + m + nsp);
    std::copy(s_grp.begin(), s_grp.end(), desc.begin() + m + 2 * (size_t)nsp);
    std::copy(tu.begin(), tu.end(), desc.begin() + m + 3 * (size_t)nsp);
    const int *dd = c->upload<int>("mk_desc", desc.data(), desc.size());
    double *Qtu = c->buf<double>("mk_Qtu", (size_t)nu * nt);
    k_gather_rows(c, Qt, nt, dd + m + 3 * (size_t)nsp, nu, Qtu, s);
    const size_t budget = masked_scratch_budget();
    for (int t0 = 0; t0 < ntile;) {
        const int gA = s_grp[(size_t)t0 * ST];
        auto last_grp = [&](int t1) { return s_grp[std::min(ns, t1 * ST) - 1]; };      // of the tile rows [.., t1)
        int t1 = t0 + 1;
        while (t1 < ntile) {
            const size_t gB = (size_t)last_grp(t1 + 1) + 1;
            if ((size_t)nx * (gB - gA) * gB * sizeof(double) > budget) break;
            ++t1;
        }
        const int gB = last_grp(t1) + 1, nuc = gB - gA;
        double *H = c->buf<double>("mk_H", (size_t)nx * nuc * gB);
        GemmDesc gh;                      // H[a][g - gA][g'] = sum_b Qtu[g][b] Dinv[a][b] Qtu[g'][b]
        gh.M = nuc; gh.N = gB; gh.K = nt;
        gh.A = Qtu + (size_t)gA * nt; gh.lda = nt; gh.B = Qtu; gh.ldb = nt; gh.transB = true; gh.C = H; gh.ldc = gB;
        gh.kscale = Dinv; gh.sKscale = nt;
        gh.batch = nx; gh.sC = (long)nuc * gB;
        gh.lower = true; gh.lower_shift = gA;          // only H_a[g][g'] with g' <= g is ever read (tiles above the diagonal exit)
        gh.prof_name = "gemm_masked_H";
        gemm_f64(c, gh, s);
        MaskedGramDesc d;
        d.Qs = Qs; d.nx = nx; d.xi = dd; d.s_off = dd + m; d.s_cnt = dd + m + nsp; d.s_grp = dd + m + 2 * (size_t)nsp;
        d.H = H; d.sH = (long)nuc * gB; d.ldh = gB; d.gA = gA; d.t0 = t0; d.t1 = t1; d.m = m; d.G = G;
        k_masked_gram(c, d, s);
        t0 = t1;
    }
}

// The assembly alone, on host operands (no reference counterpart; masked.hip: masked_gram_kernel): Qs (nx, nx) and Qt (nt, nt) row-major
// with the eigen-index in columns, D (nx, nt) > 0, samples (xi[p], ti[p]), p < m, in any order -> G (m, m) row-major in that order,
//   G[p][q] = sum_{a,b} Qs[xi[p]][a] Qs[xi[q]][a] Qt[ti[p]][b] Qt[ti[q]][b] / D[a][b],
// symmetric bit for bit; the same call returns the same bits.
extern "C" int gpcsd_masked_gram(gpcsd_ctx *c, const double *Qs, int nx, const double *Qt, int nt, const double *D, const int *xi,
                                 const int *ti, int m, double *G) {
    GP_API_BEGIN(c)
    GP_REQUIRE(Qs && Qt && D && xi && ti && G && nx > 0 && nt > 0 && m > 0, -3, "masked_gram: bad arguments");
    // (checked before anything is read)
    GP_REQUIRE(m <= GPCSD_MAX_MISSING && nx < (1 << 22) && nt < (1 << 22) && nx <= 65535, GPCSD_ERR_CAPACITY,
               "masked_gram: m=%d exceeds GPCSD_MAX_MISSING=%d (or nx=%d, nt=%d beyond one operand row)", m, GPCSD_MAX_MISSING, nx, nt);
    for (int p = 0; p < m; ++p)
        GP_REQUIRE(xi[p] >= 0 && xi[p] < nx && ti[p] >= 0 && ti[p] < nt, -3, "masked_gram: sample %d = (%d, %d) outside the %d x %d grid", p,
                   xi[p], ti[p], nx, nt);
    std::vector<int> perm(m), xs(m), ts(m);
    for (int p = 0; p < m; ++p) perm[p] = p;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return ti[a] != ti[b] ? ti[a] < ti[b] : xi[a] < xi[b]; });
    for (int p = 0; p < m; ++p) {
        xs[p] = xi[perm[p]];
        ts[p] = ti[perm[p]];
    }
    hipStream_t s = c->stream;
    double *dQs = c->upload<double>("op_in0", Qs, (size_t)nx * nx);
    double *dQt = c->upload<double>("op_in1", Qt, (size_t)nt * nt);
    double *dD = c->upload<double>("op_in2", D, (size_t)nx * nt);
    double *dDinv = c->buf<double>("op_in3", (size_t)nx * nt);
    k_loo_var(c, dD, dDinv, (long)nx * nt, s);                      // 1 / D elementwise
    double *dG = c->buf<double>("mk_G", (size_t)m * m);
    masked_assemble(c, dQs, dQt, dDinv, nx, nt, xs, ts, dG, s);
    std::vector<double> Gs((size_t)m * m);
    c->download(Gs.data(), dG, (size_t)m * m * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    for (int p = 0; p < m; ++p)
        for (int q = 0; q < m; ++q) G[(size_t)perm[p] * m + perm[q]] = Gs[(size_t)p * m + q];
    return 0;
    GP_API_END(c)
}

// What a mask asks for, from the host copy of the mask alone: per distinct missing set (keys i * nx + x, ascending = by time, then
// electrode) the trials that share it; trials without a missing sample and trials without an observed one belong to no set.
struct MaskPlan {
    std::vector<std::vector<int>> keys, trials;
    std::vector<int> group_of;          // per trial: its set, -1 none missing, -2 none observed
    std::vector<int> slot_of, affected; // per trial: its slot among the trials that belong to a set (-1 otherwise); those trials
    long n_obs = 0;
};
static MaskPlan mask_plan(const gpcsd_ctx *c, const unsigned char *mask, int mask_trials) {
    const int nx = c->nx, nt = c->nt, R = c->ntrials, MT = mask_trials;
    const long N = (long)nx * nt;
    MaskPlan P;
    P.group_of.assign(R, -1);
    P.slot_of.assign(R, -1);
    std::map<std::vector<int>, int> seen;
    std::vector<int> k;
    for (int r = 0; r < MT; ++r) {
        k.clear();
        for (int i = 0; i < nt; ++i)
            for (int x = 0; x < nx; ++x)
                if (!mask[((size_t)x * nt + i) * MT + r]) k.push_back(i * nx + x);
        const long m = (long)k.size();
        const int nrep = MT == 1 ? R : 1;
        P.n_obs += (N - m) * nrep;
        int g = -1;
        if (m == N) g = -2;
        else if (m > 0) {
            // (before any data is read)
            GP_REQUIRE(m <= GPCSD_MAX_MISSING, GPCSD_ERR_CAPACITY, "masked: trial %d has %ld missing samples, more than GPCSD_MAX_MISSING=%d "
                       "(the Schur complement is dense, m x m)", r, m, GPCSD_MAX_MISSING);
            auto it = seen.find(k);
            if (it == seen.end()) {
                g = (int)P.keys.size();
                seen.emplace(k, g);
                P.keys.push_back(k);
                P.trials.emplace_back();
            } else g = it->second;
        }
        for (int rr = (MT == 1 ? 0 : r); rr < (MT == 1 ? R : r + 1); ++rr) {
            P.group_of[rr] = g;
            if (g >= 0) {
                P.trials[g].push_back(rr);
                P.slot_of[rr] = (int)P.affected.size();
                P.affected.push_back(rr);
            }
        }
    }
    return P;
}

static void masked_check(const gpcsd_ctx *c, const gpcsd_hparams *hp, const unsigned char *mask, int mask_trials, const char *who) {
    GP_REQUIRE(hp != nullptr, -3, "null hparams");
    GP_REQUIRE(mask != nullptr, -3, "%s: null mask", who);
    GP_REQUIRE(c->d_lfp != nullptr, -4, "lfp not set (call gpcsd_set_lfp)");
    GP_REQUIRE(mask_trials == 1 || mask_trials == c->ntrials, -3, "%s: mask_trials=%d must be 1 or ntrials=%d", who, mask_trials, c->ntrials);
    GP_REQUIRE(!uses_host_kt(hp), -3, "%s: user-defined temporal covariances (GPCSD_KIND_HOST) are not supported", who);
    GP_REQUIRE((long)c->ntrials * c->nt < GPCSD_MAX_GEMM_LD_KMAJOR && c->nx <= 65535, GPCSD_ERR_CAPACITY,
               "%s: ntrials * nt = %ld exceeds the capacity of one operand row (%ld doubles; GPCSD_MAX_GEMM_LD_KMAJOR)", who,
               (long)c->ntrials * c->nt, (long)GPCSD_MAX_GEMM_LD_KMAJOR);
}

// Bm = (Qs^T (y~ + E_M u) Qt) / D of all trials in "pred_B" ((nx, R, nt), the operand of the predictions' cross products), behind the
// joined decomposition e.  res (3 R doubles on the device, "mk_res") when want_ll: [r] = y~_r^T A^-1 y~_r, [R + r] = |L^-1 c_r|^2 and
// [2 R + r] = log det G of trial r's set (0 where the trial belongs to none).  st: a status word for the factorisations.
static double *masked_core(gpcsd_ctx *c, EigState &e, const MaskPlan &P, const unsigned char *mask, int MT, bool want_ll, int *st) {
    const int nx = c->nx, nt = c->nt, R = c->ntrials;
    const long RT = (long)R * nt;
    hipStream_t s = c->stream;
    const unsigned char *dmask = c->upload<unsigned char>("mk_mask", mask, (size_t)nx * nt * MT);
    double *Y = c->buf<double>("mk_Y", (size_t)nx * RT);
    double *W = c->buf<double>("proj_W", (size_t)nx * RT), *Bm = c->buf<double>("pred_B", (size_t)nx * RT);
    double *res = c->buf<double>("mk_res", (size_t)3 * R);
    GP_HIP(hipMemsetAsync(res, 0, (size_t)3 * R * sizeof(double), s));
    k_mask_fill(c, c->d_lfp, dmask, MT, nx, R, nt, Y, s);
    {
        ProfScope ps(c, "masked_front", 0.0, s);
        pred_data_spatial(c, e, W, Y, R);
        pred_data_temporal(c, e, W, Bm, R);
    }
    const int na = (int)P.affected.size();
    if (na == 0 && !want_ll) return Bm;
    double *T1 = c->buf<double>("mk_T1", (size_t)nx * RT), *V = c->buf<double>("mk_V", (size_t)nx * RT);
    {
        ProfScope ps(c, "masked_front", 0.0, s);
        GemmDesc g1;                      // T1[(x', r)][t] = sum_i Bm[(x', r)][i] Qt[t][i]
        g1.M = nx * R; g1.N = nt; g1.K = nt;
        g1.A = Bm; g1.lda = nt; g1.B = e.Qt; g1.ldb = nt; g1.transB = true; g1.C = T1; g1.ldc = nt;
        g1.prof_name = "gemm_masked_back_temporal";
        gemm_f64(c, g1, s);
        GemmDesc g2;                      // V[x][(r, t)] = sum_x' Qs[x][x'] T1[x'][(r, t)] = (A^-1 y~_r)[x, t]
        g2.M = nx; g2.N = (int)RT; g2.K = nx;
        g2.A = e.Qs; g2.lda = nx; g2.B = T1; g2.ldb = RT; g2.C = V; g2.ldc = RT;
        g2.prof_name = "gemm_masked_back_spatial";
        gemm_f64(c, g2, s);
        if (want_ll) k_mask_dot(c, Y, V, dmask, MT, nx, R, nt, res, s);
    }
    if (na == 0) return Bm;
    double *U = c->buf<double>("mk_U", (size_t)nx * na * nt);
    GP_HIP(hipMemsetAsync(U, 0, (size_t)nx * na * nt * sizeof(double), s));
    std::vector<int> xs, ts, idx;
    for (size_t g = 0; g < P.keys.size(); ++g) {
        const std::vector<int> &k = P.keys[g], &tr = P.trials[g];
        const int m = (int)k.size(), nr = (int)tr.size();
        xs.resize(m);
        ts.resize(m);
        for (int p = 0; p < m; ++p) {
            xs[p] = k[p] % nx;
            ts[p] = k[p] / nx;
        }
        double *G = c->buf<double>("mk_G", (size_t)m * m);
        {
            ProfScope ps(c, "masked_G", 0.0, s);
            masked_assemble(c, e.Qs, e.Qt, e.Dinv, nx, nt, xs, ts, G, s);
        }
        // one upload: xi | ti | trials | slots
        idx.assign((size_t)2 * m + 2 * nr, 0);
        std::copy(xs.begin(), xs.end(), idx.begin());
        std::copy(ts.begin(), ts.end(), idx.begin() + m);
        for (int q = 0; q < nr; ++q) {
            idx[(size_t)2 * m + q] = tr[q];
            idx[(size_t)2 * m + nr + q] = P.slot_of[tr[q]];
        }
        const int *di = c->upload<int>("mk_idx", idx.data(), idx.size());
        double *Cb = c->buf<double>("mk_rhs", (size_t)m * nr);
        ProfScope ps(c, "masked_solve", 0.0, s);
        k_mask_gather(c, V, di, di + m, m, di + 2 * m, nr, R, nt, Cb, s);
        potrf_device(c, G, m, st, s);
        trsm_lower_device(c, G, m, Cb, nr, s);                       // L^-1 c
        if (want_ll) {
            k_mask_colsumsq(c, Cb, m, nr, di + 2 * m, res + R, s);
            double *ld = c->buf<double>("mk_logdet", 1);
            logdet_chol_device(c, G, m, ld, s);
            for (int q = 0; q < nr; ++q)
                GP_HIP(hipMemcpyAsync(res + 2 * (size_t)R + tr[q], ld, sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        trsm_lower_trans_device(c, G, m, Cb, nr, s);                 // G^-1 c
        k_mask_scatter(c, Cb, di, di + m, m, di + 2 * m + nr, nr, na, nt, U, s);      // u = -G^-1 c
    }
    {
        ProfScope ps(c, "masked_update", 0.0, s);
        double *B2 = c->buf<double>("mk_B2", (size_t)nx * na * nt);
        const int *da = c->upload<int>("mk_affected", P.affected.data(), (size_t)na);
        pred_data_spatial(c, e, W, U, na);
        pred_data_temporal(c, e, W, B2, na);
        k_mask_add(c, Bm, B2, da, nx, R, na, nt, s);                 // linearity: Bm += the projection of E_M u
    }
    return Bm;
}

// Posterior means with missing samples: gpcsd_predict_at of the model conditioned on the observed samples only.  As predict_at_impl
// except that the data operand Bm comes from masked_core (and that it collects an earlier queued prediction first).  Outputs: the buffers of predict_impl.
static int predict_masked_impl(gpcsd_ctx *c, const PredCall &q, const unsigned char *mask, int mask_trials) {
    posterior_request(c, "predict_masked", q, REQ_SITES);
    masked_check(c, q.hp, mask, mask_trials, "predict_masked");
    posterior_request(c, "predict_masked", q, REQ_CAP_OUT_ROW | REQ_CAP_PC_ROW);
    const MaskPlan P = mask_plan(c, mask, mask_trials);              // (capacity: before any data is read)
    int *st = nullptr;                                               // a status word for the factorisations
    PostFront f;
    const int rc0 = posterior_front(c, q, FRONT_DRAIN, f, [&](EigState &e) {
        st = c->buf<int>("mk_status", 4);
        GP_HIP(hipMemsetAsync(st, 0, 4 * sizeof(int), c->stream));
        return masked_core(c, e, P, mask, mask_trials, false, st);
    });
    if (rc0) return rc0;
    {
        ProfScope ps(c, "masked_tail", 0.0, c->stream);
        pred_mean_outputs(c, f, q);
    }
    own_resident_outputs(c);
    const int rc = finish_call(c, f.e, nullptr, 0);
    const int rc2 = finish_status(c, st);
    return rc != 0 ? rc : rc2;
}

extern "C" int gpcsd_predict_masked_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, const unsigned char *mask, int mask_trials,
                                             const double *z, int nz, const double *tstar, int ntstar, int type, int want_lists) {
    GP_API_BEGIN(c)
    return predict_masked_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, want_lists != 0, false), mask, mask_trials);
    GP_API_END(c)
}

extern "C" int gpcsd_predict_masked(gpcsd_ctx *c, const gpcsd_hparams *hp, const unsigned char *mask, int mask_trials, const double *z,
                                    int nz, const double *tstar, int ntstar, int type, double *csd_list, double *csd, double *lfp_list,
                                    double *lfp) {
    GP_API_BEGIN(c)
    const PredCall q = pred_call(hp, z, nz, tstar, ntstar, type, csd_list != nullptr || lfp_list != nullptr, false);
    const int rc = predict_masked_impl(c, q, mask, mask_trials);
    if (rc < 0) return rc;
    download_sum_list(c, "pred_out_", type, (size_t)nz * ntstar * c->ntrials, hp->n_temporal, csd_list, csd, lfp_list, lfp);
    return rc;
    GP_API_END(c)
}

// The log-likelihood of the observed samples in loglik()'s convention without the 2 pi term and WITHOUT the jitter of loglik (the
// model of the masked predictions): out2 = {sum_r (log det A + log det G_r), sum_r (y~_r^T A^-1 y~_r - c_r^T G_r^-1 c_r)}, the value
// is -1/2 out2[0] - 1/2 out2[1]; per_trial (ntrials, 2) holds the two terms of every trial (a trial without an observed sample: 0, 0).
extern "C" int gpcsd_loglik_masked(gpcsd_ctx *c, const gpcsd_hparams *hp, const unsigned char *mask, int mask_trials, double *out2,
                                   double *per_trial, long *n_obs) {
    GP_API_BEGIN(c)
    GP_REQUIRE(out2 != nullptr, -3, "loglik_masked: null output");
    masked_check(c, hp, mask, mask_trials, "loglik_masked");
    const MaskPlan P = mask_plan(c, mask, mask_trials);              // (capacity: before any data is read)
    if (int rc = drain_async(c)) return rc;
    EigState e = front_half(c, hp, 0.0);
    const int R = c->ntrials;
    hipStream_t s = c->stream;
    int *st = c->buf<int>("mk_status", 4);
    GP_HIP(hipMemsetAsync(st, 0, 4 * sizeof(int), s));
    join_temporal(c, e, nullptr, true);            // D and sum(log D) = log det A in scal[0]
    masked_core(c, e, P, mask, mask_trials, true, st);
    std::vector<double> res((size_t)3 * R);
    c->download(res.data(), c->bufs["mk_res"].p, res.size() * sizeof(double));
    double sumlog = 0.0;
    const int rc = finish_call(c, e, &sumlog, 1);
    const int rc2 = finish_status(c, st);
    if (rc != 0 || rc2 != 0) return rc != 0 ? rc : rc2;
    out2[0] = out2[1] = 0.0;
    for (int r = 0; r < R; ++r) {
        const bool none = P.group_of[r] == -2;
        const double ld = none ? 0.0 : sumlog + res[2 * (size_t)R + r], qd = none ? 0.0 : res[r] - res[(size_t)R + r];
        if (per_trial) {
            per_trial[2 * (size_t)r] = ld;
            per_trial[2 * (size_t)r + 1] = qd;
        }
        out2[0] += ld;
        out2[1] += qd;
    }
    if (n_obs) *n_obs = P.n_obs;
    return 0;
    GP_API_END(c)
}
