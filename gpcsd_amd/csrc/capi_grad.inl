// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip are in scope) --
// log-likelihood + analytic gradient, one or B hyper-parameter sets per chain of launches.

// ---- log-likelihood + analytic gradient for B hyper-parameter sets in ONE chain of launches ---------------------------------
// fit() restarts are independent optimiser chains (gpcsd1d.py:193-220) whose evaluations are latency-bound: ~100 dependent
// launches in which the longest kernel occupies one workgroup per eigenproblem.  B sets evaluated together share every launch:
// the Gram builders and derivative kernels take the set index as a grid dimension (scalars from a device table of
// hyper-parameters), the eigensolver runs B replicas of each problem class, every GEMM gets an outer batch level.  Each set
// executes exactly the arithmetic of an evaluation on its own (same kernels, same tile configurations, same reduction
// order), so its results do not depend on B.
// An evaluation is decided once (grad_plan) and queued phase by phase (grad_front ... grad_collect: DESIGN 2 top to bottom).
// Folded basis (see FoldMode): with a scalar noise variance it runs on the half-size eigenvector blocks of the symmetry-folded
// eigensolver -- projections, the Ghat_s / Ghat_t sums and the back-rotations are each two half-size products, half the GEMM flops.
// The cross-parity blocks of Ghat are never needed: dKs and dKt commute with the reflections, so <G, dK> only sees the
// parity-diagonal blocks.  The full-size path is the same code with two sides of one block each.
static HpDev hp_image(const gpcsd_hparams *hp) {
    HpDev h{};
    h.R = hp->R; h.eps = hp->eps; h.ell_s[0] = hp->ell_s[0]; h.ell_s[1] = hp->ell_s[1];
    h.ncomp = hp->n_temporal;
    for (int i = 0; i < hp->n_temporal; ++i) {
        h.kind[i] = hp->kind[i];
        h.ell_t[i] = hp->ell_t[i];
        h.sigma2_t[i] = hp->sigma2_t[i];
    }
    h.sig2n = hp->sig2n[0];
    h.jitter = hp->jitter;
    return h;
}

// Everything the host reads back lives in ONE block -- [scalars NS B][gradient slots NG B][status words 2 B] -- so that it comes
// back in one copy into a page-locked block (three copies into pageable vectors were three staged round trips, ~70 us).  The same
// layout on the device and in the host's copy.
struct GradRes {
    static constexpr int NS = 8, NG = 64;           // scalars and gradient slots per set
    // scalars of a set: sum log D; quad and sum B^2 (first temporal parity block, or both); sum 1/D; quad and sum B^2 (second block)
    enum { SUMLOG = 0, QUAD = 1, SUMB2 = 2, SUMINVD = 3, QUAD_A = 4, SUMB2_A = 5 };
    double *scal = nullptr, *grad = nullptr;        // [set][NS]; [set][NG] in natural-parameter order: R, ell_s (dim), (ell_t, sigma2_t)
                                                    // per component (the noise entries are put together on the host)
    int *st = nullptr;                              // [0, B): spatial chains, [B, 2B): temporal chains
    static size_t doubles(int B) { return (size_t)(NS + NG + 1) * B; }
    static GradRes at(double *blk, int B) { return {blk, blk + (size_t)NS * B, reinterpret_cast<int *>(blk + (size_t)(NS + NG) * B)}; }
};

// One side (spatial / temporal) as the tail sees it: the parity blocks of its eigenvectors in fold order.  A side that is not folded
// takes part as one "symmetric" block of full size: {n, n, 0, Q, eigenvalues, n^2, identity fold}.
struct Side {
    int n = 0, ns = 0, na = 0;
    const double *U = nullptr, *w = nullptr;        // per set: U = (Us ns x ns | Ua na x na), w = (ws | wa); sets sU / n apart
    long sU = 0;
    SymDev sym;                                     // fold tables (identity beside a folded side; unused when neither side folds)
    int rows(int p) const { return p ? na : ns; }                   // block p = 0 symmetric, 1 antisymmetric
    int row0(int p) const { return p ? ns : 0; }                    // its first row / column in fold order
    long off(int p) const { return p ? (long)ns * ns : 0; }         // ... and its place in U and in any matrix kept block by block
    long blocks() const { return (long)ns * ns + (long)na * na; }
};

static Side grad_side(gpcsd_ctx *c, int slot, bool folded, const SymDev &sym, int n, const double *Q, const double *ev, int B) {
    Side sd;
    sd.n = n;
    sd.sym = sym;
    if (folded) {
        const FoldView fv = eigh_fold_view(c, slot, slot ? &c->sym_t : &c->sym_s, n, B);
        sd.ns = fv.ns; sd.na = fv.na; sd.U = fv.U; sd.w = fv.w; sd.sU = fv.sU;
    } else {
        sd.ns = n; sd.na = 0; sd.U = Q; sd.w = ev; sd.sU = (long)n * n;
    }
    return sd;
}

// One evaluation, decided before anything is queued
struct GradPlan {
    const gpcsd_hparams *hps = nullptr;                      // the request: B sets in, (B, 2) values, (B, ngrad) gradients, (B) status out
    int B = 0, ngrad = 0, *status = nullptr;
    double *out2 = nullptr, *grad = nullptr;
    Geo g;
    int nx = 0, nt = 0, R = 0, C = 0, G = 0, nsig = 0, nhead = 0, n1 = 0, n2 = 0;
    long RT = 0, nxx = 0, ntt = 0, nD = 0, nxRT = 0, nxG = 0, GG = 0, nmx = 0;
    bool host_kt = false, variances_nonneg = true, jitters_nonneg = true;    // (what the fills may announce as psd: EigArenaView::psd)
    const SymDev *sym_s = nullptr, *sym_t = nullptr;         // the solver's (a caller's Gram need not commute with the time grid's reflection)
    // ---- switches (environment, read once per process)
    bool kron = false;          // 2D: forward AND backward on the per-axis factors of Kgl = K1 (x) K2 (GPCSD_GRAD_KRON=0: flat, A/B)
    int ch = 512;               // row chunk of the Ghat_t sums (GPCSD_GRAD_CH)
    int mid_cfg = 3;            // tile configuration of Gs A and Gs T from 128 rows (GPCSD_GRAD_MID_CFG; both paths)
    // ---- the fold decision and what differs between the folded and the full-size evaluation (these decide bits and launches)
    FoldMode fm;                // the decision and the sides' fold tables; its views are not used (grad_front takes the sides)
    bool fold = false;
    int gs_cfg = 0, gt_cfg = 0; // tiles of the Ghat_s / Ghat_t products from 64 rows: GPCSD_GRAD_GS_CFG / _GT_CFG folded, 0 = automatic full-size
    int rot_cfg = 0;            // ... and of the rotations U Ghat U^T from 128 rows: GPCSD_GRAD_MID_CFG folded, automatic full-size
    hipStream_t sT = nullptr;   // the temporal half's stream: stream2 beside the spatial half only folded, not profiling (prof_mode 1), not
                                // with GPCSD_GRAD_BRANCHES=0; else the main stream
    bool temporal_first = false;// queuing order of the two halves: folded Ghat_t, Ghat_s, rotate t, rotate s; full-size s before t
    bool need_merged = true;    // the solver merges the parity blocks into full eigenvectors: the full-size path reads Qs / Qt
    bool unfold = false;        // rotations leave fold-order blocks for k_sym_unfold_mat (an identity side too); full-size they write Gs / Gt
    bool quad_in_two = false;   // the quadratic form arrives as two partial sums (temporal parity blocks of unequal shape)
    // (the noise-list terms -- nsig > 1 -- exist on the full-size path only: fold_mode wants a scalar noise)
    // ---- bound by grad_front: uploads, and what belongs to the generation it starts
    const HpDev *tab = nullptr;
    const double *d_siglist = nullptr;      // per-electrode noise lists (fit_gpcsd_baseline.py:85-89): set b's nx variances at + b * nx
    const double *Y = nullptr;              // the data: Fs Y Ft^T when a side is folded
    Side S, T;
    // ---- streams (main, temporal chain) and the buffers more than one phase touches
    hipStream_t s = nullptr, s2 = nullptr;
    GradRes res;                         // device block
    double *Qs, *Qt, *es, *et, *D, *Dinv, *A, *Tm, *Kgl = nullptr, *W, *Bm, *av, *bv, *Ghs, *Ght, *Gs, *Gt;
    double *K1 = nullptr, *K2 = nullptr, *dK1 = nullptr, *dK2 = nullptr, *Uk = nullptr, *U2 = nullptr, *Tl1 = nullptr, *Tl2 = nullptr;   // kron
    const double *t;
};

// every argument check comes before any work is queued (the front half launches on two streams)
static GradPlan grad_plan(gpcsd_ctx *c, const gpcsd_hparams *hps, int B, double *out2, double *grad, int ngrad, int *status) {
    GP_REQUIRE(out2 && grad && hps && B >= 1, -3, "loglik_grad: null argument");
    GradPlan P;
    P.hps = hps; P.B = B; P.out2 = out2; P.grad = grad; P.ngrad = ngrad; P.status = status;
    const Geo g = P.g = resident_geo(c);
    GP_REQUIRE(c->d_lfp != nullptr, -4, "lfp not set (call gpcsd_set_lfp)");
    GP_REQUIRE(c->time_nt == c->nt, -4, "time grid has %d points but lfp has nt=%d", c->time_nt, c->nt);
    GP_REQUIRE(g.nx == c->nx, -4, "geometry has %d electrodes but lfp has nx=%d", g.nx, c->nx);
    const int nx = P.nx = c->nx, nt = P.nt = c->nt, C = P.C = hps[0].n_temporal, nsig = P.nsig = hps[0].n_sig2n;
    P.R = c->ntrials; P.G = g.G();
    for (int b = 0; b < B; ++b) {
        check_hp(c, &hps[b], nx);
        // user-defined temporal covariances: the caller supplies d Kt / d theta_k (gpcsd_set_host_temporal_dgram), one set at a time
        GP_REQUIRE(!uses_host_kt(&hps[b]) || (B == 1 && c->host_kt_on && c->host_kt_nt == nt && c->host_dkt_n == 2 * C &&
                                              c->host_dkt.size() == (size_t)2 * C * nt * nt), -3,
                   "loglik_grad: user-defined temporal covariances need their Gram matrix and the %d derivative matrices "
                   "d Kt / d (ell_c, sigma2_c) (gpcsd_set_host_temporal_gram + gpcsd_set_host_temporal_dgram), one set per call", 2 * C);
        GP_REQUIRE(hps[b].n_temporal == C && hps[b].n_sig2n == nsig, -3,
                   "loglik_grad_batch: every hyper-parameter set must have the same number of temporal components and noise entries");
        for (int i = 0; i < C; ++i)
            GP_REQUIRE(hps[b].kind[i] == hps[0].kind[i], -3, "loglik_grad_batch: temporal kernel kinds differ between sets");
        P.jitters_nonneg = P.jitters_nonneg && hps[b].jitter >= 0.0;                 // (the signs are the host's to check)
        for (int cc = 0; cc < C; ++cc) P.variances_nonneg = P.variances_nonneg && hps[b].sigma2_t[cc] >= 0.0;
    }
    // scalar sig2n: one trailing entry; per-electrode list (indexed by eigen-row like the reference's D): nx entries
    GP_REQUIRE(nsig == 1 || nsig == nx, -3, "loglik_grad: sig2n must be a scalar or a list of nx=%d values (got %d)", nx, nsig);
    P.nhead = 1 + g.dim + 2 * C;
    GP_REQUIRE(ngrad == P.nhead + nsig, -3, "loglik_grad: ngrad=%d, expected %d", ngrad, P.nhead + nsig);
    P.RT = (long)P.R * nt; P.nxx = (long)nx * nx; P.ntt = (long)nt * nt; P.nD = (long)nx * nt; P.nxRT = (long)nx * P.RT;
    P.nxG = (long)nx * P.G; P.GG = (long)P.G * P.G; P.nmx = (long)std::max(nx, nt) * std::max(nx, nt);
    P.n1 = g.ngl1; P.n2 = g.dim == 2 ? g.ngl2 : 0; P.host_kt = uses_host_kt(&hps[0]);
    P.sym_s = c->sym_s.ns > 0 ? &c->sym_s : nullptr;
    P.sym_t = (c->sym_t.ns > 0 && !P.host_kt) ? &c->sym_t : nullptr;
    // 2D: the GL grid is a tensor grid and Kgl = K1 (x) K2 (covariances.py:216); 1D keeps the flat Kgl
    static const bool kron_off = getenv("GPCSD_GRAD_KRON") && getenv("GPCSD_GRAD_KRON")[0] == '0';
    // A chunk of the Ghat_t sums is one K range of a 64 x 64 tile.  Measured: 256-row chunks make the product itself faster for ONE
    // set at 384 x 500 x 50 (592 tiles of 32 dependent K steps are too few to hide the load latency: 94 -> 61 us per parity) but the
    // evaluation no faster (the product runs beside the spatial branch), and every batch slower (twice the partial matrices written
    // and read back: 8 sets 4.41 against 4.17 ms; cfg5 at 32 sets 7.8 k against 8.5 k evaluations/s).  512 it stays; the choice
    // never depends on the batch: a set is summed the same way alone and in a batch.
    static const int CH = getenv("GPCSD_GRAD_CH") ? std::max(64, atoi(getenv("GPCSD_GRAD_CH"))) : 512;
    static const int GS_CFG = getenv("GPCSD_GRAD_GS_CFG") ? atoi(getenv("GPCSD_GRAD_GS_CFG")) : 3;
    static const int GT_CFG = getenv("GPCSD_GRAD_GT_CFG") ? atoi(getenv("GPCSD_GRAD_GT_CFG")) : 3;
    // the mid-size products of the tail (Gs A, Gs T: nx x G x nx; the rotations): the automatic choice looks at ONE set's tile count (it
    // must not depend on the batch) and takes the 32 x 32 latency tile, which at a batch of 8 sets is 13 % of the GPU time at a sixth
    // of the MFMA rate.  Default 3 (64 x 64, BK 16): 8 sets 4.30 -> 4.05 ms, one set unchanged.  GPCSD_GRAD_MID_CFG=0: automatic (A/B).
    static const int MID_CFG = getenv("GPCSD_GRAD_MID_CFG") ? atoi(getenv("GPCSD_GRAD_MID_CFG")) : 3;
    // GPCSD_GRAD_BRANCHES=0: the two halves of the gradient one after the other on the main stream (A/B; same kernels, same bits)
    static const bool branches_off = getenv("GPCSD_GRAD_BRANCHES") && getenv("GPCSD_GRAD_BRANCHES")[0] == '0';
    P.kron = g.dim == 2 && !kron_off; P.ch = CH; P.mid_cfg = MID_CFG;
    P.s = P.sT = c->stream; P.s2 = c->stream2;
    P.fm = fold_mode(c, &hps[0]);
    P.fold = P.fm.on;
    if (P.fold) {               // (else: the full-size defaults of the fields)
        P.gs_cfg = GS_CFG; P.gt_cfg = GT_CFG; P.rot_cfg = MID_CFG;
        if (!branches_off && c->prof_mode != 1) P.sT = P.s2;
        P.temporal_first = P.unfold = true;
        P.need_merged = false;
    }
    const int tns = P.fm.ft.on ? P.fm.ft.ns : nt, tna = P.fm.ft.on ? P.fm.ft.na : 0;
    P.quad_in_two = tna > 0 && tna != tns;
    const long sUs = P.fm.fs.on ? P.fm.fs.sU : P.nxx, sUt = P.fm.ft.on ? P.fm.ft.sU : P.ntt;

    auto buf = [&](const char *name, size_t per_set) { return c->buf<double>(name, per_set * B); };
    P.res = GradRes::at(buf("b_result", GradRes::doubles(1)), B);
    P.Qs = buf("b_Qs", P.nxx); P.Qt = buf("b_Qt", P.ntt); P.es = buf("b_es", nx); P.et = buf("b_et", nt);
    P.D = buf("b_D", P.nD); P.Dinv = buf("b_Dinv", P.nD); P.W = buf("b_W", P.nxRT); P.Bm = buf("b_Bm", P.nxRT);
    P.A = buf("b_ks_A", P.nxG); P.Tm = buf("b_ks_T", P.nxG);
    if (P.kron) {
        P.K1 = buf("b_ks_K1", (size_t)P.n1 * P.n1); P.dK1 = buf("b_ks_dK1", (size_t)P.n1 * P.n1);
        P.K2 = buf("b_ks_K2", (size_t)P.n2 * P.n2); P.dK2 = buf("b_ks_dK2", (size_t)P.n2 * P.n2);
        P.Uk = buf("b_ks_U", P.nxG); P.U2 = buf("b_ks_U2", P.nxG); P.Tl1 = buf("b_ks_Tl1", P.nxG); P.Tl2 = buf("b_ks_Tl2", P.nxG);
    } else {
        P.Kgl = buf("b_ks_Kgl", P.GG);
    }
    P.av = buf("b_grad_a", nx); P.bv = buf("b_grad_b", nt); P.Ghs = buf("b_grad_Ghs", sUs); P.Ght = buf("b_grad_Ght", sUt);
    P.Gs = buf("b_grad_Gs", P.nxx); P.Gt = buf("b_grad_Gt", P.ntt);
    P.t = (const double *)c->bufs["time_t"].p;
    return P;
}

// `to` goes on once everything queued on `from` so far has run (one stream: nothing to do)
static void stream_after(gpcsd_ctx *c, hipStream_t from, hipStream_t to) {
    if (from == to) return;
    hipEvent_t ev = c->get_event();
    GP_HIP(hipEventRecord(ev, from));
    GP_HIP(hipStreamWaitEvent(to, ev, 0));
    c->event_pool.push_back(ev);
}

// out[x][(h1,h2)] = sum_g1 F1[g1][h1] V[x][(g1,h2)], one small product per electrode and set (F1 = K1 or dK1)
static void kron_axis1(gpcsd_ctx *c, const GradPlan &P, const double *F1, const double *V, double *out, const char *name) {
    GemmDesc v;
    v.M = P.n1; v.N = P.n2; v.K = P.n1;
    v.A = F1; v.lda = P.n1; v.transA = true; v.B = V; v.ldb = P.n2; v.C = out; v.ldc = P.n2;
    v.batch = P.nx; v.sA = 0; v.sB = P.G; v.sC = P.G;
    v.batch2 = P.B; v.sA2 = (long)P.n1 * P.n1; v.sB2 = P.nxG; v.sC2 = P.nxG;
    v.prof_name = name;
    gemm_f64(c, v, P.s);
}

// out[(x,g1)][h2] = sum_g2 A[(x,g1)][g2] F2[g2][h2] (F2 = K2 or dK2)
static void kron_axis2(gpcsd_ctx *c, const GradPlan &P, const double *F2, double *out, const char *name) {
    GemmDesc u;
    u.M = P.nx * P.n1; u.N = P.n2; u.K = P.n2;
    u.A = P.A; u.lda = P.n2; u.B = F2; u.ldb = P.n2; u.C = out; u.ldc = P.n2;
    u.batch2 = P.B; u.sA2 = P.nxG; u.sB2 = (long)P.n2 * P.n2; u.sC2 = P.nxG;
    u.prof_name = name;
    gemm_f64(c, u, P.s);
}

// One side's eigen-chain (slot 0 spatial, 1 temporal) on `sq`: B replicas, reporting into that side's status words
static void grad_chain(gpcsd_ctx *c, const GradPlan &P, int slot, double *K, bool prefolded, hipStream_t sq) {
    const int n = slot ? P.nt : P.nx;
    ProfScope ps(c, slot ? "eigh_temporal" : "eigh_spatial", 9.0 * (double)n * n * n * P.B, sq);
    EighCall r;
    r.side[slot] = {K, n, slot ? P.et : P.es, slot ? P.Qt : P.Qs, slot ? P.sym_t : P.sym_s, P.B, prefolded};
    r.status = P.res.st + slot * P.B; r.status_stride = 1;
    r.need_merged = P.need_merged;
    eigh_pair_device(c, r, sq);
}

// Ks_b = A_b Kgl_b A_b^T (the jitter comes with the fill)                     covariances.py:74-96 / :204-232
static void grad_spatial_gram(gpcsd_ctx *c, const GradPlan &P, double *Ks) {
    const Geo &g = P.g;
    const int nx = P.nx, B = P.B, G = P.G;
    const long nxG = P.nxG, GG = P.GG;
    hipStream_t s = P.s;
    if (g.dim == 1) {
        k_fwd_weights_1d(c, g.x, nx, g.gx1, g.gw1, g.ngl1, 0.0, P.A, s, P.tab, B, nxG);
        k_se_1d(c, g.gx1, G, g.gx1, G, 0.0, P.Kgl, s, P.tab, B, GG);
    } else {
        k_fwd_weights_2d(c, g.x, nx, g.gx1, g.gw1, g.ngl1, g.gx2, g.gw2, g.ngl2, 0.0, 0.0, P.A, s, P.tab, B, nxG);
        if (!P.kron) k_se_2d(c, g.gx1, g.gx2, G, g.ngl2, g.gx1, g.gx2, G, g.ngl2, 0.0, 0.0, P.Kgl, s, P.tab, B, GG);
    }
    if (P.kron) {
        // T = A (K1 (x) K2) as two small products (build_kphi does the same for the fused calls: 74 MF instead of 1.1 GF at
        // 384 x 20 x 60, and Kgl's 1200^2 exponentials are never formed)
        k_se_axis_tab(c, g.gx1, P.n1, 0, P.tab, B, P.K1, P.dK1, s);
        k_se_axis_tab(c, g.gx2, P.n2, 1, P.tab, B, P.K2, P.dK2, s);
        kron_axis2(c, P, P.K2, P.Uk, "gemm_Ks_AK2");
        kron_axis1(c, P, P.K1, P.Uk, P.Tm, "gemm_Ks_K1U");
    } else {
        GemmDesc d1;                                   // T = A Kgl
        d1.M = nx; d1.N = G; d1.K = G;
        d1.A = P.A; d1.lda = G; d1.B = P.Kgl; d1.ldb = G; d1.C = P.Tm; d1.ldc = G;
        d1.batch2 = B; d1.sA2 = nxG; d1.sB2 = GG; d1.sC2 = nxG;
        d1.prof_name = "gemm_Ks_AKgl";
        gemm_f64(c, d1, s);
    }
    GemmDesc d2;                                       // Ks = T A^T
    d2.M = nx; d2.N = nx; d2.K = G;
    d2.A = P.Tm; d2.lda = G; d2.B = P.A; d2.ldb = G; d2.transB = true; d2.C = Ks; d2.ldc = nx;
    d2.batch2 = B; d2.sA2 = nxG; d2.sB2 = nxG; d2.sC2 = P.nxx;
    d2.prof_name = "gemm_Ks_TAt";
    gemm_f64(c, d2, s);
}

// Front half: temporal chain on stream2 (queued first: the critical path), spatial chain on the main stream.  Both read the
// hyper-parameter table and report into the status words cleared here: they start behind the main stream's current position (this
// call returns values, so nothing of it outlives it anyway).
static void grad_front(gpcsd_ctx *c, GradPlan &P) {
    const int nx = P.nx, nt = P.nt, B = P.B;
    hipStream_t s = P.s, s2 = P.s2;
    int *st = P.res.st;
    // ---- device table of the hyper-parameter sets
    std::vector<HpDev> himg(B);
    for (int b = 0; b < B; ++b) himg[b] = hp_image(&P.hps[b]);
    const HpDev *tab = P.tab = c->upload_cached<HpDev>("b_hp_tab", himg.data(), B);
    if (P.nsig > 1) {
        std::vector<double> lists((size_t)P.nsig * B);
        for (int b = 0; b < B; ++b) memcpy(lists.data() + (size_t)b * P.nsig, P.hps[b].sig2n, (size_t)P.nsig * sizeof(double));
        P.d_siglist = c->upload_cached<double>("b_sig2n_lists", lists.data(), lists.size());
    }
    double *Ks = c->buf<double>("b_Ks", P.nxx * B), *Kt = c->buf<double>("b_Kt", P.ntt * B);
    GP_HIP(hipMemsetAsync(st, 0, (size_t)2 * B * sizeof(int), s));
    begin_generation(c, 1, s2, true);
    begin_generation(c, 0, s, true);
    P.S = grad_side(c, 0, P.fm.fs.on, P.fm.sym_s, nx, P.Qs, P.es, B);       // (fold views belong to the generation just started)
    P.T = grad_side(c, 1, P.fm.ft.on, P.fm.sym_t, nt, P.Qt, P.et, B);
    P.Y = P.unfold ? folded_lfp(c, P.fm) : c->d_lfp;
    // the temporal chain's input as one launch straight from t and the hyper-parameter table (folded, scaled blocks in the class
    // arenas: capi.hip temporal_fill) instead of Gram -> fold -> absmax -> scale, as in the fused calls
    const bool tfill = temporal_fill_applies(c, P.sym_t, nt, P.host_kt);
    staged_chain_guard(c, s2);            // (a queued staged chain's side-stream readers of the class arenas)
    if (tfill) {
        const char *const *tg = eigh_fold_tags(c, 1);
        const EigArenaView as = eigh_arena_view(c, tg[0], P.sym_t->ns, B), aa = eigh_arena_view(c, tg[1], P.sym_t->na, B);
        k_temporal_fold_fill_tab(c, tab, B, P.t, nt, *P.sym_t, as, aa, st + B, 1, s2, P.variances_nonneg);
    } else if (P.host_kt) {
        c->copy_in(Kt, c->host_kt.data(), (size_t)P.ntt * sizeof(double), s2);
    } else {
        k_temporal_gram(c, P.C, nullptr, nullptr, nullptr, P.t, nt, P.t, nt, Kt, s2, tab, B, P.ntt);
    }
    grad_chain(c, P, 1, Kt, /*prefolded=*/tfill, s2);
    GP_HIP(hipEventRecord(c->ev_join, s2));
    grad_spatial_gram(c, P, Ks);
    // the spatial chain's input the same way (psd fold fill: fold + jitter on the folded diagonals + scale in one launch)
    const bool sfill = spatial_fill_applies(c, P.sym_s, nx);
    if (sfill) {
        const char *const *tg = eigh_fold_tags(c, 0);
        const EigArenaView as = eigh_arena_view(c, tg[0], P.sym_s->ns, B), aa = eigh_arena_view(c, tg[1], P.sym_s->na, B);
        k_psd_fold_fill(c, Ks, nx, P.nxx, B, nullptr, *P.sym_s, as, aa, st, 1, s, tab, P.jitters_nonneg);
    } else {
        k_add_diag(c, Ks, nx, 0.0, s, tab, B, P.nxx);
    }
    grad_chain(c, P, 0, Ks, /*prefolded=*/sfill, s);
    if (P.kron) {
        // the backward pass's hyper-parameter-only factors, queued here where the main stream would otherwise wait for the chains:
        // Tl1 = A (dK1 (x) K2) = dK1^T (A K2),  Tl2 = A (K1 (x) dK2) = K1^T (A dK2)
        kron_axis1(c, P, P.dK1, P.Uk, P.Tl1, "gemm_grad_dK1U");
        kron_axis2(c, P, P.dK2, P.U2, "gemm_grad_AdK2");
        kron_axis1(c, P, P.K1, P.U2, P.Tl2, "gemm_grad_K1U2");
    }
}

// W = Us^T Y, D and sum log D, B~ = (W Ut) / D with the sums of alpha B~ and B~^2, a and b -- all in fold order
static void grad_project(gpcsd_ctx *c, const GradPlan &P) {
    const Side &S = P.S, &T = P.T;
    const int nx = P.nx, nt = P.nt, B = P.B;
    hipStream_t s = P.s;
    // W_b = diag(U_b)^T Y per spatial parity block (gpcsd1d.py:125 inner dot); the data is shared by all sets
    for (int p = 0; p < 2; ++p) {
        const int np = S.rows(p), r0 = S.row0(p);
        if (np == 0) continue;
        GemmDesc gw;
        gw.M = np; gw.N = (int)P.RT; gw.K = np;
        gw.A = S.U + S.off(p); gw.lda = np; gw.transA = true;
        gw.B = P.Y + r0 * P.RT; gw.ldb = P.RT; gw.C = P.W + r0 * P.RT; gw.ldc = P.RT;
        gw.batch2 = B; gw.sA2 = S.sU; gw.sB2 = 0; gw.sC2 = P.nxRT;
        gw.prof_name = "gemm_proj_spatial";
        gemm_f64(c, gw, s);
    }
    GP_HIP(hipStreamWaitEvent(s, c->ev_join, 0));
    // D_b = ws_b (x) wt_b + sig2n_b, sum log D_b -> SUMLOG
    k_build_D(c, S.w, nx, T.w, nt, P.d_siglist, P.nsig, P.D, P.Dinv, P.res.scal + GradRes::SUMLOG, s, P.tab, B, GradRes::NS);
    // alpha = W V per temporal parity block;  B~ = alpha / D;  sums of alpha B~ and B~^2 -> QUAD, SUMB2 (second block: QUAD_A, SUMB2_A)
    GemmDesc gq[2];
    for (int q = 0; q < 2; ++q) {
        const int nq = T.rows(q), c0 = T.row0(q);
        gq[q].M = nx * P.R; gq[q].N = nq; gq[q].K = nq;
        gq[q].A = P.W + c0; gq[q].lda = nt; gq[q].B = T.U + T.off(q); gq[q].ldb = nq;
        // (no B~ wt / B~ ws copies: the Ghat products scale B~ along their contracted index as they load it -- GemmDesc::kscale --
        // the same rounded products, without 2 x 0.6 GB written and read back per 32-set batch)
        gq[q].C = P.Bm + c0; gq[q].ldc = nt; gq[q].C2 = nullptr; gq[q].C3 = nullptr;
        gq[q].epi = EPI_GRAD; gq[q].D = P.Dinv + c0; gq[q].rdiv = P.R; gq[q].ldd = nt;
        gq[q].colscale = T.w + c0; gq[q].rowscale = S.w;
        gq[q].quad_out = P.res.scal + (q ? GradRes::QUAD_A : GradRes::QUAD);
        gq[q].batch2 = B; gq[q].sA2 = P.nxRT; gq[q].sB2 = T.sU; gq[q].sC2 = P.nxRT; gq[q].sD2 = P.nD;
        gq[q].sColscale2 = nt; gq[q].sRowscale2 = nx; gq[q].sQuad2 = GradRes::NS;
        gq[q].prof_name = "gemm_grad_temporal";
    }
    if (T.na > 0 && T.na == T.ns) {
        // equal parity blocks: one launch, one sum over both (not gemm_pair: the pair's colscale is a batch apart as well)
        gq[0].batch = 2;
        gq[0].sA = gq[1].A - gq[0].A; gq[0].sB = gq[1].B - gq[0].B; gq[0].sC = gq[1].C - gq[0].C;
        gq[0].sD = gq[1].D - gq[0].D; gq[0].sColscale = gq[1].colscale - gq[0].colscale;
        gemm_f64(c, gq[0], s);
    } else {
        gemm_f64(c, gq[0], s);
        if (T.na > 0) gemm_f64(c, gq[1], s);          // (P.quad_in_two)
    }
    k_D_sums(c, P.D, S.w, T.w, nx, nt, P.av, P.bv, P.res.scal + GradRes::SUMINVD, s, B, GradRes::NS);      // a, b in fold order; sum 1/D
}

// Ghat_t parity blocks: 1/2 sum_{(x,r)} (B~ ws)[:, q]^T B~[:, q] - R/2 diag(b[q block])   (row chunks, then a fixed-order sum)
static void grad_ghat_t(gpcsd_ctx *c, const GradPlan &P) {
    const Side &S = P.S, &T = P.T;
    const int nx = P.nx, nt = P.nt, R = P.R, B = P.B, CH = P.ch;
    hipStream_t sT = P.sT;
    const long rows = (long)nx * R, sUt = T.blocks();
    double *wsr = c->buf<double>("b_grad_ws_rows", (size_t)rows * B);        // ws spread over the (x', r) rows
    k_repeat_rows(c, S.w, nx, nx, R, B, wsr, sT);
    const int nfull = (int)(rows / CH), rem = (int)(rows % CH), nchunk = nfull + (rem > 0 ? 1 : 0);
    const long sCt = nchunk * sUt;
    double *Ct = c->buf<double>("b_grad_Ct", (size_t)sCt * B);
    for (int q = 0; q < 2; ++q) {
        const int nq = T.rows(q), c0 = T.row0(q);
        const long o_in = nchunk * T.off(q), nqq = (long)nq * nq;
        if (nq == 0) continue;
        // `count` chunks of K rows each, from chunk `first` on: their partial matrices
        auto chunks = [&](int first, int K, int count) {
            const long row0 = (long)first * CH;
            GemmDesc gt;
            gt.M = nq; gt.N = nq; gt.K = K;
            gt.A = P.Bm + row0 * nt + c0; gt.lda = nt; gt.transA = true; gt.B = gt.A; gt.ldb = nt;
            gt.C = Ct + o_in + first * nqq; gt.ldc = nq;
            gt.kscale = wsr + row0; gt.sKscale = K; gt.sKscale2 = rows;       // (B~ ws)^T B~: the factor runs along the contracted row
            gt.batch = count; gt.sA = (long)K * nt; gt.sB = (long)K * nt; gt.sC = nqq;
            gt.batch2 = B; gt.sA2 = P.nxRT; gt.sB2 = P.nxRT; gt.sC2 = sCt;
            if (nq >= 64) gt.cfg = P.gt_cfg;
            gt.lower = true;
            gt.prof_name = "gemm_grad_Gt";
            gemm_f64(c, gt, sT);
        };
        if (nfull > 0) chunks(0, CH, nfull);
        if (rem > 0) chunks(nfull, rem, 1);
        k_batch_reduce(c, Ct + o_in, nchunk, nqq, nq, 0.5, P.bv + c0, -0.5 * R, P.Ght + T.off(q), sT, B, sCt, nt, sUt);
    }
}

// Ghat_s parity blocks: 1/2 sum_r (B~ wt)[p rows] B~[p rows]^T - R/2 diag(a[p rows])   (one product per trial, then a fixed-order sum)
static void grad_ghat_s(gpcsd_ctx *c, const GradPlan &P) {
    const Side &S = P.S, &T = P.T;
    const int nx = P.nx, nt = P.nt, R = P.R, B = P.B;
    hipStream_t s = P.s;
    const long sUs = S.blocks(), sCs = (long)R * sUs;
    double *Cs = c->buf<double>("b_grad_Cs", (size_t)sCs * B);
    auto product = [&](int p) {
        const int np = S.rows(p), r0 = S.row0(p);
        GemmDesc gs;
        gs.M = np; gs.N = np; gs.K = nt;
        gs.A = P.Bm + r0 * P.RT; gs.lda = P.RT; gs.B = gs.A; gs.ldb = P.RT; gs.transB = true; gs.C = Cs + R * S.off(p); gs.ldc = np;
        gs.kscale = T.w; gs.sKscale = 0; gs.sKscale2 = nt;            // (B~ wt) B~^T: the factor runs along the contracted t'
        gs.batch = R; gs.sA = nt; gs.sB = nt; gs.sC = (long)np * np;
        gs.batch2 = B; gs.sA2 = P.nxRT; gs.sB2 = P.nxRT; gs.sC2 = sCs;
        // the tile configuration must not depend on B (a set has to run the same tiles alone or in a batch)
        if (np >= 64) gs.cfg = P.gs_cfg;
        gs.lower = true;                                              // symmetric: k_batch_reduce mirrors the lower triangle
        gs.prof_name = "gemm_grad_Gs";
        return gs;
    };
    for (int p = 0; p < 2; ++p) {
        const int np = S.rows(p);
        if (np == 0) continue;
        gemm_f64(c, product(p), s);
        k_batch_reduce(c, Cs + R * S.off(p), R, (long)np * np, np, 0.5, P.av + S.row0(p), -0.5 * R, P.Ghs + S.off(p), s, B, sCs, nx, sUs);
    }
    if (P.nsig > 1) {
        // noise tied to the eigen-index (full-size: one block): eigenvector-rotation term, S = sum_r B_r B_r^T (see grad.hip)
        GemmDesc g3 = product(0);
        g3.kscale = nullptr;
        g3.prof_name = "gemm_grad_BBt";
        gemm_f64(c, g3, s);
        double *Ssum = c->buf<double>("grad_Ssum", (size_t)P.nxx * B), *zero = c->buf<double>("grad_zero", nx);
        k_fill(c, zero, nx, 0.0, s);
        k_batch_reduce(c, Cs, R, P.nxx, nx, 1.0, zero, 0.0, Ssum, s, B, sCs, /*s_dvec=*/0, P.nxx);
        k_siglist_eigvec_term(c, P.Ghs, Ssum, P.es, P.d_siglist, nx, 0.0, s, B);
    }
}

// Back to the original bases, block by block: G~_pp = U_p Ghat_pp U_p^T, then G = F^T diag(G~_ss, G~_aa) F (P.unfold)
static void grad_rotate_back(gpcsd_ctx *c, const GradPlan &P) {
    const int B = P.B;
    auto rotate = [&](const Side &sd, const double *H, double *G, const char *fold_buf, const char *tmp_buf, hipStream_t sq) {
        const long sH = sd.blocks();
        double *out = P.unfold ? c->buf<double>(fold_buf, (size_t)sH * B) : G;
        double *tmp = c->buf<double>(tmp_buf, (size_t)P.nmx * B);
        for (int p = 0; p < 2; ++p) {
            const int np = sd.rows(p);
            const long o = sd.off(p);
            if (np == 0) continue;
            GemmDesc a;                                // tmp = U_p Ghat_pp
            a.M = np; a.N = np; a.K = np; a.A = sd.U + o; a.lda = np; a.B = H + o; a.ldb = np; a.C = tmp; a.ldc = np;
            a.batch2 = B; a.sA2 = sd.sU; a.sB2 = sH; a.sC2 = P.nmx;
            GemmDesc bq;                               // out_pp = tmp U_p^T
            bq.M = np; bq.N = np; bq.K = np; bq.A = tmp; bq.lda = np; bq.B = sd.U + o; bq.ldb = np; bq.transB = true; bq.C = out + o; bq.ldc = np;
            bq.batch2 = B; bq.sA2 = P.nmx; bq.sB2 = sd.sU; bq.sC2 = sH;
            if (np >= 128) a.cfg = bq.cfg = P.rot_cfg;
            a.prof_name = bq.prof_name = "gemm_grad_sandwich";
            gemm_f64(c, a, sq);
            gemm_f64(c, bq, sq);
        }
        if (P.unfold) k_sym_unfold_mat(c, out, sH, sd.sym, sd.n, G, sq, B);
    };
    if (P.temporal_first) rotate(P.T, P.Ght, P.Gt, "b_grad_Gtf", "b_grad_T1t", P.sT);      // (the temporal half has its own scratch)
    rotate(P.S, P.Ghs, P.Gs, "b_grad_Gsf", "b_grad_T1", P.s);
    if (!P.temporal_first) rotate(P.T, P.Ght, P.Gt, "b_grad_Gtf", "b_grad_T1t", P.sT);
}

// <Gt, dKt> on the temporal half's stream; <Gs, dKs / d ell> and <Gs, dKs / d R> through P = Gs A and Gs T on the main stream
static void grad_contract(gpcsd_ctx *c, const GradPlan &P) {
    constexpr int NG = GradRes::NG;
    const Geo &g = P.g;
    const int nx = P.nx, nt = P.nt, B = P.B, G = P.G;
    const long nxG = P.nxG, GG = P.GG;
    hipStream_t s = P.s, sT = P.sT;
    double *gdev = P.res.grad;
    if (P.host_kt) {                      // <Gt, d Kt / d theta_k> with the caller's derivative matrices
        double *dK = c->upload<double>("b_host_dkt", c->host_dkt.data(), (size_t)2 * P.C * P.ntt);
        stream_after(c, s, sT);           // (the upload is on the main stream)
        k_frob_inner(c, P.Gt, dK, P.ntt, 2 * P.C, gdev + 1 + g.dim, sT);
    } else {
        k_temporal_grad(c, &P.hps[0], P.Gt, P.t, nt, gdev + 1 + g.dim, sT, P.tab, B, NG);
    }
    double *Pm = c->buf<double>("b_grad_P", nxG * B);
    auto gs_times = [&](const double *X, const char *name) {          // Pm = Gs X  (nx x G x nx)
        GemmDesc gp;
        gp.M = nx; gp.N = G; gp.K = nx; gp.A = P.Gs; gp.lda = nx; gp.B = X; gp.ldb = G; gp.C = Pm; gp.ldc = G;
        gp.batch2 = B; gp.sA2 = P.nxx; gp.sB2 = nxG; gp.sC2 = nxG;
        if (nx >= 128) gp.cfg = P.mid_cfg;
        gp.prof_name = name;
        gemm_f64(c, gp, s);
    };
    gs_times(P.A, "gemm_grad_GsA");
    if (P.kron) {                         // <A^T Gs A, dKgl/dell_k> = <Gs A, Tl_k>   (grad.hip: k_frob_pair)
        k_frob_pair(c, Pm, P.Tl1, P.Tl2, nxG, gdev + 1, s, B, NG);
    } else {
        double *Mg = c->buf<double>("b_grad_M", GG * B);
        GemmDesc gm;                      // M = A^T P
        gm.M = G; gm.N = G; gm.K = nx; gm.A = P.A; gm.lda = G; gm.transA = true; gm.B = Pm; gm.ldb = G; gm.C = Mg; gm.ldc = G;
        gm.batch2 = B; gm.sA2 = nxG; gm.sB2 = nxG; gm.sC2 = GG;
        gm.prof_name = "gemm_grad_AtP";
        gemm_f64(c, gm, s);
        k_kgl_grad(c, Mg, P.Kgl, g.gx1, g.gx2, G, P.n2, 0.0, 0.0, gdev + 1, s, P.tab, B, NG);
    }
    gs_times(P.Tm, "gemm_grad_GsT");      // Gs T  (T = A Kgl from the forward pass)
    k_fwdR_grad(c, Pm, g.x, nx, g.gx1, g.gw1, g.gx2, g.gw2, G, P.n2, 0.0, 0.0, gdev, s, P.tab, B, NG);
}

// Results to the host in one copy; out2: (B, 2) = (sum log D, quad) per set; grad: (B, ngrad); status: (B) -- 0 ok, > 0 numerical
// failure of that set alone.  Returns the worst status.
static int grad_collect(gpcsd_ctx *c, const GradPlan &P) {
    const int nx = P.nx, R = P.R, B = P.B;
    std::vector<double> hb2, hinv;
    if (P.nsig > 1) {                     // d/d sig2n_x = -R/2 sum_i 1/D_xi + 1/2 sum_{r,i} B_{(x,r),i}^2
        double *b2row = c->buf<double>("grad_b2row", (size_t)nx * B);               // (Bm is [set][x][r][t]: nx * B rows of R nt)
        k_rowgroup_sumsq(c, P.Bm, nx * B, P.RT, b2row, P.s);
        hb2.resize((size_t)nx * B); hinv.resize((size_t)nx * B);
        c->download(hb2.data(), b2row, hb2.size() * sizeof(double));
        c->download(hinv.data(), c->bufs["grad_s1row"].p, hinv.size() * sizeof(double));   // written by k_D_sums, [set][x]
    }
    stream_after(c, P.sT, P.s);           // the temporal half ended with its contraction: the main stream takes it in before the copy
    double *hres = c->pinned<double>("b_result_host", GradRes::doubles(B));
    c->download(hres, P.res.scal, GradRes::doubles(B) * sizeof(double));
    GP_HIP(hipStreamSynchronize(P.s2));
    c->sync();
    const GradRes h = GradRes::at(hres, B);
    if (c->prof_mode == 1) c->prof_collect();
    int worst = 0;
    for (int b = 0; b < B; ++b) {
        const double *hs = h.scal + (size_t)GradRes::NS * b, *hg = h.grad + (size_t)GradRes::NG * b;
        P.out2[2 * b] = hs[GradRes::SUMLOG];
        P.out2[2 * b + 1] = hs[GradRes::QUAD] + (P.quad_in_two ? hs[GradRes::QUAD_A] : 0.0);
        double *gb = P.grad + (size_t)b * P.ngrad;
        for (int k = 0; k < P.nhead; ++k) gb[k] = hg[k];
        if (P.nsig == 1)
            gb[P.nhead] = -0.5 * R * hs[GradRes::SUMINVD] + 0.5 * (hs[GradRes::SUMB2] + (P.quad_in_two ? hs[GradRes::SUMB2_A] : 0.0));
        else
            for (int x = 0; x < nx; ++x) gb[P.nhead + x] = -0.5 * R * hinv[(size_t)b * nx + x] + 0.5 * hb2[(size_t)b * nx + x];
        int stb = h.st[b] != 0 ? h.st[b] : h.st[B + b];
        if (stb < 0) stb = 1;
        if (P.status) P.status[b] = stb;
        worst = std::max(worst, stb);
    }
    if (worst != 0) {
        char msg[160];
        snprintf(msg, sizeof(msg), "numerical failure (status %d): eigensolver did not converge or matrix not positive definite", worst);
        c->last_error = msg;
    }
    return worst;
}

static int loglik_grad_impl(gpcsd_ctx *c, const gpcsd_hparams *hps, int B, double *out2, double *grad, int ngrad, int *status) {
    GradPlan P = grad_plan(c, hps, B, out2, grad, ngrad, status);
    grad_front(c, P);
    c->fold_gemm_calls += P.fold ? 1 : 0;             // (folded evaluations only)
    grad_project(c, P);
    // From here the spatial and the temporal half of the gradient are independent (both read B~, a, b): folded, the temporal one --
    // Ghat_t, its rotation back, <Gt, dKt> -- runs on stream2, idle since its chain ended, beside the spatial one on the main
    // stream; each half's small launches (reductions, the rotations' 8 us products) hide under the other's large products.
    stream_after(c, P.s, P.sT);
    if (P.temporal_first) grad_ghat_t(c, P);
    grad_ghat_s(c, P);
    if (!P.temporal_first) grad_ghat_t(c, P);
    grad_rotate_back(c, P);
    grad_contract(c, P);
    return grad_collect(c, P);
}

extern "C" int gpcsd_loglik_grad(gpcsd_ctx *c, const gpcsd_hparams *hp, double *out2, double *grad, int ngrad) {
    GP_API_BEGIN(c)
    GP_REQUIRE(hp != nullptr, -3, "loglik_grad: null hparams");
    if (int rc = drain_async(c)) return rc;      // (this path keeps its own status words)
    return loglik_grad_impl(c, hp, 1, out2, grad, ngrad, nullptr);
    GP_API_END(c)
}

extern "C" int gpcsd_loglik_grad_batch(gpcsd_ctx *c, const gpcsd_hparams *hps, int nsets, double *out2, double *grad, int ngrad,
                                       int *status) {
    GP_API_BEGIN(c)
    GP_REQUIRE(hps && nsets >= 1 && status, -3, "loglik_grad_batch: bad arguments");
    if (int rc = drain_async(c)) return rc;
    (void)loglik_grad_impl(c, hps, nsets, out2, grad, ngrad, status);   // per-set failures are reported in status[], not as rc
    return 0;
    GP_API_END(c)
}
